"""The row tail of the k_decode row loops -- noise, rematrix, staging, the row's counters -- held to what the compiler
makes of it (CPU only: hipcc cross-compiles; compiled the way tests/test_isa_budget.py does).

tools/isa_mix.py walks the path a wave executes from behind the last slot to the hand-written wait for the chunk, cold
branches left out.  profiles/isa_mix_row_tail_before.txt is that path in the tree before the fast pass placed a matrix's
result by an LDS store and derived the row's counters (HIP 7.2.26015-fc0010cf6a, clang 22.0.0git): for the headline
instance 124 VALU instructions, 96 of them slow or unclassified, 12 selects on an SGPR pair, and six compiler-placed
waits for vector memory among the rematrix's multiply-adds.  profiles/isa_mix_row_tail_after.txt is what it is now."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "k_decode<6,false,false,true,false,false,false>"
# fast pass: frame-major with packed WAV payload, frame-major (the headline), planar, two substreams frame-major / planar
FAST_PASS = [
    "k_decode<6,false,false,true,false,false,true>",
    HEADLINE,
    "k_decode<6,false,false,false,false,false,false>",
    "k_decode<6,false,false,true,false,true,false>",
    "k_decode<6,false,false,false,false,true,false>",
]
# the one-substream lane instances: those three and the chain parse pass
ONE_SUBSTREAM_LANE = FAST_PASS[:3] + ["k_decode<6,false,false,false,true,false,false>"]
MIN_GAIN = 20           # item 1 alone removes 26 compares and selects per PCM frame and adds at most 6 instructions


def _isa_mix():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recorded(name, instance):
    """-> (VALU, slow + unclassified) of `instance` in the row-tail table of profiles/<name>"""
    text = open(os.path.join(ROOT, "profiles", name)).read()
    table = text[text.index("== row tail"):]
    for line in table.split("\n"):
        m = re.match(r"\s+(k_decode<\S+>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", line)
        if m and m.group(1) == instance:
            return int(m.group(3)), int(m.group(5)) + int(m.group(6))
    raise AssertionError("%s: no row-tail line for %s" % (name, instance))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    m = _isa_mix()
    asm = m.compile_asm(str(tmp_path_factory.mktemp("isa_tail") / "mlp_hip.s"))
    loops = {}
    for name, info, blocks, parents in m.kernels(asm):
        head, lb = m.row_loop(blocks, parents)
        if head is not None:
            loops[name] = lb
    return m, m.analyse_row_tail(asm), loops


def test_headline_row_tail_is_shorter_than_before(built):
    _, tails, _ = built
    t = tails[HEADLINE]
    valu, slow = t["valu"], t["slow"] + t["unclassified"]
    v0, s0 = _recorded("isa_mix_row_tail_before.txt", HEADLINE)
    v1, s1 = _recorded("isa_mix_row_tail_after.txt", HEADLINE)
    print("row tail, headline: VALU %d (before %d, recorded %d), slow + unclassified %d (before %d, recorded %d)" %
          (valu, v0, v1, slow, s0, s1))
    assert t["total"] > 0 and any(o == "v_mad_i64_i32" for b in t["path"] for o, _, _ in b.ins), "row tail not found"
    assert valu <= v0 - MIN_GAIN and slow <= s0 - MIN_GAIN
    assert valu <= v1 and slow <= s1


@pytest.mark.parametrize("name", ONE_SUBSTREAM_LANE)
def test_no_vector_memory_wait_among_multiply_adds(built, name):
    m, _, loops = built
    assert name in loops, "row loop not found"
    waits = m.vmcnt_waits_beside_mads(loops[name])
    assert not waits, waits


@pytest.mark.parametrize("name", FAST_PASS)
def test_no_select_on_an_sgpr_pair_in_the_row_tail(built, name):
    _, tails, _ = built
    t = tails[name]
    assert t["total"] > 0 and any(o == "v_mad_i64_i32" for b in t["path"] for o, _, _ in b.ins), "row tail not found"
    assert not t["sgpr_selects"], t["sgpr_selects"]
