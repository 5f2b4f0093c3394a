"""The row loop of k_decode outside the slots and the row tail -- loop control, the row gate, the refill test and request,
the ring commit, the flush's decision, offsets and addresses -- held to what the compiler makes of it (CPU only: hipcc
cross-compiles; compiled the way tests/test_isa_budget.py does).

tools/isa_mix.py walks what a lockstep wave executes in one turn of the loop, cold branches left out, for three kinds
of turn: a plain row, a row that requests and commits a refill, a row that flushes; "rest" is the part of that path
outside the slots, the slot masks and the row tail.  profiles/isa_mix_row_rest_before.txt is the tree before this
region was priced (HIP 7.2.26015-fc0010cf6a, clang 22.0.0git): for the headline instance 47 / 109 / 97 VALU
instructions, 27 / 66 / 59 of them slow or unclassified.  profiles/isa_mix_row_rest_after.txt is what it is now, and the
figures a build is held to; docs/history.md A.15 has what was changed.

The other cases hold every k_decode instance to where the kernel stands on the ISA: registers and occupancy, nothing in
scratch and no lane moves inside a row loop, LDS per workgroup, the slots as they were instruction for instruction, the
headline's row tail, the hazard checker clean, every placed store with its wait states.  The plane arithmetic of a
refill turn (ring_turn_off) is checked against BitReaderT's slot() and the first-plane rule by a static_assert in
csrc/mlp_decode.h, which every compile of the library evaluates -- this one too; a case here makes sure it is there."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "k_decode<6,false,false,true,false,false,false>"
INSTANCES = [
    "k_decode<6,false,false,true,false,false,true>",       # frame-major, packed WAV payload
    HEADLINE,                                               # frame-major
    "k_decode<6,false,false,false,false,false,false>",     # planar
    "k_decode<6,false,false,true,false,true,false>",       # two substreams, frame-major
    "k_decode<6,false,false,false,false,true,false>",      # two substreams, planar
    "k_decode<6,false,false,false,true,false,false>",      # chain parse pass
    "k_decode<6,false,false,false,true,true,false>",       # chain parse pass, two substreams
    "k_decode<6,true,true,false,false,false,false>",       # sequential pass
]
TURNS = ("plain", "refill", "flush")
LDS_MAX = 31232             # four workgroups share a CU up to here
ROW_TAIL = (59, 40)         # the headline's row tail: VALU, slow + unclassified (profiles/isa_mix_row_tail_after.txt)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recorded_turns(name, instance):
    """-> {turn: (rest VALU, rest slow + unclassified)} of `instance` in the turns table of profiles/<name>"""
    text = open(os.path.join(ROOT, "profiles", name)).read()
    table = text[text.index("== turns"):]
    out = {}
    for line in table.split("\n"):
        m = re.match(r"\s+(k_decode<\S+>)\s+(\w+)\s+(\d+)\s+(\d+)\s+\|\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", line)
        if m and m.group(1) == instance:
            out[m.group(2)] = (int(m.group(6)), int(m.group(8)) + int(m.group(9)))
    assert sorted(out) == sorted(TURNS), "%s: turns of %s not found" % (name, instance)
    return out


def _recorded_slots(name, instance):
    """-> {slot region: histogram line or (instr, VALU)} of `instance` in profiles/<name>"""
    text = open(os.path.join(ROOT, "profiles", name)).read()
    part = text[text.index("== " + instance):]
    part = part[:part.index("\n== ", 3)]
    return {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"^\s+(slot \d|slot masks)\s+(\d+)\s+(\d+)\s", part, re.M)}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    m = _tool("isa_mix")
    asm = m.compile_asm(str(tmp_path_factory.mktemp("isa_rest") / "mlp_hip.s"))
    res = {name: (info, regions, whole) for name, info, _, regions, whole in m.analyse(asm)}
    return m, asm, res, m.analyse_turns(asm), m.analyse_row_tail(asm)


def test_every_instance_is_found(built):
    _, _, res, _, _ = built
    assert sorted(res) == sorted(INSTANCES)


@pytest.mark.parametrize("turn", TURNS)
def test_headline_turn_outside_the_slots_and_the_tail(built, turn):
    _, _, _, turns, _ = built
    t = turns[HEADLINE][turn]
    assert t["tail_agrees"], "the walk does not pass through the row tail as tools/isa_mix.py row_tail_path has it"
    assert t["slots"]["hist"]["v_ffbh_u32"] == 6, "the walk does not pass through six slots"
    valu, slow = t["rest"]["valu"], t["rest"]["slow"] + t["rest"]["unclassified"]
    v0, s0 = _recorded_turns("isa_mix_row_rest_before.txt", HEADLINE)[turn]
    v1, s1 = _recorded_turns("isa_mix_row_rest_after.txt", HEADLINE)[turn]
    print("%s turn, headline, rest: VALU %d (before %d, recorded %d), slow + unclassified %d (before %d, recorded %d)" %
          (turn, valu, v0, v1, slow, s0, s1))
    assert v1 < v0 and s1 <= s0, "the record does not show the turn below what it was"
    assert valu <= v1 and slow <= s1


def test_a_refill_and_a_flush_are_walked(built):
    """the three walks differ by what they are about: loads and byte swaps in the refill turn only, stores in the flush
    turn only"""
    _, _, _, turns, _ = built
    h = {turn: turns[HEADLINE][turn]["whole"]["hist"] for turn in TURNS}
    assert h["refill"]["global_load_dwordx4"] == 4 and h["refill"]["v_perm_b32"] == 16
    assert h["flush"]["global_store_dwordx4"] == 7 and h["flush"]["ds_bpermute_b32"] == 7
    for turn, ops in (("plain", ("global_load_dwordx4", "v_perm_b32", "global_store_dwordx4")),
                      ("refill", ("global_store_dwordx4",)), ("flush", ("global_load_dwordx4", "v_perm_b32"))):
        assert not any(h[turn][o] for o in ops), (turn, {o: h[turn][o] for o in ops})


@pytest.mark.parametrize("name", INSTANCES)
def test_lds_per_workgroup(built, name):
    """At most 31 232 B, for every instance.  The three instances of the two-substream lane were at 31 240 B (two rings of
    17 planes per wave 17 408, the PCM tile 12 288, s_cold 1 536, s_nchained 8: docs/history.md A.14); they count the lanes
    that stopped on ST_CHAINED from the lanes' status words now, not in LDS, and stand at 31 232 B."""
    _, _, res, _, _ = built
    info = res[name][0]
    print(name, "LDS", info["LDSByteSize"])
    assert info["LDSByteSize"] <= LDS_MAX, info


@pytest.mark.parametrize("name", INSTANCES)
def test_registers_occupancy_scratch_and_lane_moves(built, name):
    _, _, res, _, _ = built
    info, regions, whole = res[name]
    assert any(r.startswith("slot") for r in regions), "row loop not found"
    assert info["NumVgprs"] <= 256 and info["Occupancy"] == 2, info
    assert whole["scratch"] == 0, "%d scratch_ instructions between the row loop's labels" % whole["scratch"]
    assert whole["lane_moves"] == 0, "%d v_readlane / v_writelane between the row loop's labels" % whole["lane_moves"]


@pytest.mark.parametrize("name", INSTANCES)
def test_slots_are_what_they_were(built, name):
    """instruction for instruction: a slot's count and its VALU count against the tree before (a slot region of the
    record is a block of the loop; the headline's histogram line is compared opcode by opcode below)"""
    _, _, res, _, _ = built
    regions = res[name][1]
    before = _recorded_slots("isa_mix_row_rest_before.txt", name)
    now = {r: (x["total"], x["valu"]) for r, x in regions.items() if r.startswith("slot")}
    assert now == before, (now, before)


def test_headline_slot_histogram_is_what_it_was(built):
    m, _, res, _, _ = built
    regions = res[HEADLINE][1]
    text = open(os.path.join(ROOT, "profiles", "isa_mix_row_rest_before.txt")).read()
    part = text[text.index("== " + HEADLINE):]
    line = re.search(r"^\s+slot 1: (.*)$", part, re.M).group(1)
    assert ", ".join("%s %d" % (o, n) for o, n in regions["slot 1"]["hist"].most_common()) == line


def test_headline_row_tail_is_what_it_was(built):
    _, _, _, _, tails = built
    t = tails[HEADLINE]
    assert (t["valu"], t["slow"] + t["unclassified"]) == ROW_TAIL, (t["valu"], t["slow"], t["unclassified"])
    assert not t["vmcnt_beside_mads"] and not t["sgpr_selects"]


def test_hazard_checker_is_clean_and_every_placed_store_keeps_its_wait_states(built):
    _, asm, _, _, _ = built
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hazard_check.py"), asm], capture_output=True,
                         text=True)
    print(out.stdout[-400:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert re.search(r"hazard violations: 0\b", out.stdout), out.stdout[-400:]
    # a placed store (the cooperative flush's, "sc1") is followed by its two wait states
    lines = [l.strip() for l in open(asm)]
    placed = [i for i, l in enumerate(lines) if l.startswith("global_store_dwordx4") and l.endswith("sc1")]
    assert placed
    assert all(lines[i + 1] == "s_nop 1" for i in placed)


def test_the_plane_arithmetic_is_checked_where_it_is_compiled():
    src = open(os.path.join(ROOT, "libdvd-audio_amd", "csrc", "mlp_decode.h")).read()
    assert "static_assert(ring_turn_off_ok<RING_DWORDS>()" in src
    assert "ring_turn_off<RD>(f8, g)" in src and "ring_slot_index<RD>(d)" in src
