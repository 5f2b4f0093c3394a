"""What the compiler made of the k_decode row loops, held to a budget (CPU only: hipcc cross-compiles).

The fast pass sits on the edge of the register file (256 VGPRs, two waves per SIMD) and its time is the row loop's
instruction stream.  A source-shape change once cost 18 % through two spill reloads inside the loop and only a
human reading the ISA saw it.  These cases read the ISA on every build instead: tools/isa_mix.py compiles
csrc/mlp_hip.hip to assembly once (shared by all cases), finds each instance's row loop and prices its VALU
instructions by the two issue classes of profiles/r05_valu_issue_rates.txt.

The slot budget is what profiles/isa_mix_after.txt records for the headline instance
(HIP 7.2.26015-fc0010cf6a, clang 22.0.0git): a slot is at most 53 VALU instructions, at most 24 of them in the slow
class (unclassified opcodes count as slow).  Before the hot parameter word it was 63 and 38.

The two-substream instances used to keep the granules of the row phase's synchronous ring top-up in scratch (21 / 12 / 6
scratch_ instructions inside their row loops): that top-up now fetches one granule at a time, and every instance's
row loop is free of scratch_.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INSTANCES = [
    "k_decode<6,false,false,true,false,false,true>",       # frame-major, packed WAV payload
    "k_decode<6,false,false,true,false,false,false>",      # frame-major: the headline
    "k_decode<6,false,false,false,false,false,false>",     # planar
    "k_decode<6,false,false,true,false,true,false>",       # two substreams, frame-major
    "k_decode<6,false,false,false,false,true,false>",      # two substreams, planar
    "k_decode<6,false,false,false,true,false,false>",      # chain parse pass
    "k_decode<6,false,false,false,true,true,false>",       # chain parse pass, two substreams
    "k_decode<6,true,true,false,false,false,false>",       # sequential pass
]
SLOT_VALU_MAX = 53
SLOT_SLOW_MAX = 24


def _isa_mix():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    m = _isa_mix()
    asm = m.compile_asm(str(tmp_path_factory.mktemp("isa") / "mlp_hip.s"))
    return m, {name: (info, regions, whole) for name, info, _, regions, whole in m.analyse(asm)}


def test_every_instance_is_found(mix):
    _, res = mix
    assert sorted(res) == sorted(INSTANCES)


def test_class_table_comes_from_the_measurement():
    r = _isa_mix().Rates()
    assert 1.2 < r.threshold < 1.6 and r.fast_cycles < 2.6 and r.slow_cycles > 4.0
    assert r.classify("v_lshrrev_b32_e32", "v1, 5, v2") == "fast" and r.classify("v_lshlrev_b32_e32", "v1, 5, v2") == "slow"
    assert r.classify("v_bfe_u32", "v1, v2, 2, 5") == "slow" and r.classify("v_bitop3_b32", "v1, v2, v3, v4") == "fast"
    assert r.classify("v_cndmask_b32_e32", "v1, v2, v3, vcc") == "fast"
    assert r.classify("v_cndmask_b32_e64", "v1, v2, v3, s[0:1]") == "slow"
    assert r.classify("v_frobnicate_b32", "v1, v2") == "unclassified"


@pytest.mark.parametrize("name", INSTANCES)
def test_row_loop_has_no_scratch_and_no_lane_moves(mix, name):
    _, res = mix
    info, regions, whole = res[name]
    assert any(r.startswith("slot") for r in regions), "row loop not found"
    assert whole["scratch"] == 0, "%d scratch_ instructions between the row loop's labels" % whole["scratch"]
    assert whole["lane_moves"] == 0, "%d v_readlane / v_writelane between the row loop's labels" % whole["lane_moves"]


@pytest.mark.parametrize("name", INSTANCES)
def test_registers_and_occupancy(mix, name):
    _, res = mix
    info = res[name][0]
    assert info["NumVgprs"] <= 256 and info["Occupancy"] == 2, info


def test_headline_slot_budget(mix):
    m, res = mix
    _, regions, _ = res[m.HEADLINE]
    slots = {r: x for r, x in regions.items() if r.startswith("slot ") and r != "slot masks"}
    assert len(slots) == 6, list(regions)
    for r, x in slots.items():
        print(r, "VALU", x["valu"], "slow", x["slow"], "unclassified", x["unclassified"])
        assert x["valu"] <= SLOT_VALU_MAX, (r, x["valu"])
        assert x["slow"] + x["unclassified"] <= SLOT_SLOW_MAX, (r, x["slow"], x["unclassified"])
