"""Conceal mode's case table, CPU side: the premises of tests/test_gpu_conceal_cases.py, held on the oracle and on the
bytes, so that the GPU file cannot pass for a reason other than the one it is written for -- every recipe of
tests/conceal_cases.py decodes clean, every damage is one the oracle reports, the model makes of each case what the case's
name claims, the model with the library's limits is the rule itself up to the turns and carries DVDA_CONCEAL_ROUNDS beyond
them, and the limits are the ones the headers state."""
import os
import re

import numpy as np
import pytest

from tests import conceal_cases as cc
from tests import conceal_model as cm
from tests.stream_tools import is_major_sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(cc.CASES)
DAMAGED = [n for n in NAMES if not cc.CASES[n].claim.get("clean")]
EDGES = [n for n in DAMAGED if cc.CASES[n].group == "edge"]


def test_limits_are_the_headers():
    """a changed limit fails here instead of silently moving the turns away from the table"""
    kern = open(os.path.join(ROOT, "libdvd-audio_amd", "csrc", "mlp_conceal.h")).read()
    pub = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()

    def num(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    assert cm.LIMITS == (num(kern, r"constexpr uint32_t CONCEAL_MAX_RANGES = (\d+);"),
                         num(kern, r"constexpr uint32_t CONCEAL_ROUNDS = (\d+);"))
    assert (cm.LEADING, cm.TRAILING, cm.ROUNDS) == (num(pub, r"#define DVDA_CONCEAL_LEADING\s+(\d+)u"),
                                                    num(pub, r"#define DVDA_CONCEAL_TRAILING\s+(\d+)u"),
                                                    num(pub, r"#define DVDA_CONCEAL_ROUNDS\s+(\d+)u"))
    # the rule's sentence and the constant say the same number of decode rounds
    assert "at most %d decode rounds" % cm.LIMITS[1] in pub
    # the turns of the edge cases, from the limits (conceal_model.limited_ranges derives them)
    per_plan, reach = cm.LIMITS[0] - 1, (cm.LIMITS[0] - 1) * (cm.LIMITS[1] - 1)
    have = {int(n[4:]) for n in EDGES if n[4:].isdigit()}
    assert {per_plan - 1, per_plan, per_plan + 1, per_plan + 2, 2 * per_plan, 2 * per_plan + 1, reach, reach + 1} <= have


def test_table_covers_the_shapes_and_features():
    shapes = {(r.asg, r.rate, r.S) for r in cc.RECIPES.values()}
    assert {(0, 0, 1), (1, 0, 1), (12, 1, 1), (12, 1, 2), (12, 2, 2)} <= shapes
    feats = {frozenset(r.feats) for r in cc.RECIPES.values()}
    assert {frozenset(("CHAINED", "FIRRAND")), frozenset(("VARROWS",)), frozenset(("NOCHECK",))} <= feats
    assert any({"DISC", "CHAINED"} <= f for f in feats)
    used = {c.recipe for n, c in cc.CASES.items() if n in DAMAGED}
    assert used == set(cc.RECIPES), "a recipe without a damaged case"
    assert all(c.group in cc.GROUPS for c in cc.CASES.values())
    assert all(24 <= r.n_aus <= 104 for r in cc.RECIPES.values())


@pytest.mark.parametrize("recipe", list(cc.RECIPES))
def test_recipe_decodes_clean(pkg, oracle, recipe):
    s = cc.stream(pkg.synth, recipe)
    r = cc.RECIPES[recipe]
    pcm, frames, st = oracle.decode(s.b, s.nch, s.frames)
    assert st == 0 and frames == s.frames and pcm.shape == (s.nch, frames) and pcm.any()
    assert len(s.offs) == r.n_aus and len(s.b) < 128 << 10
    assert [s.offs.index(p) for p in s.syncs] == list(range(0, r.n_aus, r.interval))
    assert (int(s.b[20]) >> 4) == r.S == s.S
    got, spans = cm.conceal(s.b, s.nch, s.rpa, oracle, limits=cm.LIMITS)
    assert spans == [] and np.array_equal(got, pcm)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_claims(pkg, oracle, name):
    c = cc.CASES[name]
    s = cc.stream(pkg.synth, c.recipe)
    d = cc.damaged(pkg.synth, oracle, name)
    claim = c.claim
    cap = (len(d) + 4096) * 2
    st = oracle.decode(d, s.nch, cap)[2]
    pcm, spans = cc.expect(pkg.synth, oracle, name)
    R, tail_flags = cm.limited_ranges(d, s.nch, oracle, cap, cm.LIMITS)
    assert cm.kept_ranges(d, s.nch, s.rpa, oracle, limits=cm.LIMITS) == [r[:5] for r in R]
    U = cm.kept_ranges(d, s.nch, s.rpa, oracle)
    if claim.get("clean"):
        assert st == 0 and spans == [] and np.array_equal(d, s.b)
        return
    assert st & cm.ORA_DAMAGE, "the damage must be one the oracle reports"
    assert spans, "the damage must show in the model"
    assert len(R) == claim["ranges"]
    assert len(U) == claim.get("unlimited", claim["ranges"])
    rounds = any(sp[4] & cm.ROUNDS for sp in spans)
    assert rounds == bool(claim.get("rounds"))
    upcm, uspans = cm.conceal(d, s.nch, s.rpa, oracle)
    if not rounds:
        # within the library's reach: the limited model is the rule
        assert [r[:5] for r in R] == U and spans == uspans and np.array_equal(pcm, upcm)
    else:
        # beyond it: the rule's first ranges, and everything behind the last one a single TRAILING | ROUNDS span
        assert [r[:5] for r in R] == U[:len(R)] and len(U) > len(R)
        assert spans[-1] == (pcm.shape[1], 0, R[-1][1], len(d), cm.TRAILING | cm.ROUNDS)
        assert not any(sp[4] for sp in spans[:-1])
        assert pcm.shape[1] < upcm.shape[1]
        # the silence is measured with the mean of the ranges kept, not of all the rule would keep
        K, F = sum(r[1] - r[0] for r in R), sum(r[2] for r in R)
        for k, sp in enumerate(spans[:-1]):
            g = (R[k + 1][3] - R[k][4]) & 0xFFFF
            assert sp[1] == cm.gap_frames(sp[3] - sp[2], g, K / F)
    assert pcm.shape == (s.nch, sum(r[2] for r in R) + sum(sp[1] for sp in spans))
    if "frames" in claim:
        assert pcm.shape[1] == claim["frames"]
    if "flags" in claim:
        assert [sp[4] for sp in spans] == claim["flags"]
    if "first" in claim:
        units, frames = claim["first"]
        assert (cm.kept_units(d, R[:1]), R[0][2]) == (units, frames)
        assert frames != units * s.rpa, "non-standard timing: the standard size must not hold the range"
    if "skipped" in claim:
        p = s.syncs[claim["skipped"]]
        assert is_major_sync(d, p) and all(r[0] != p for r in R)
        assert R[0][1] < p and R[1][0] == s.syncs[claim["skipped"] + 1], "the next major sync is taken"
    if "replanned" in claim:
        first_plan = cm.plan(d, s.nch, oracle, cap, cm.LIMITS[0])
        assert (first_plan != [r[:2] for r in R]) == claim["replanned"]
        if claim["replanned"]:
            # a range of round 0's plan holds damage its own decode reports, and more than one range of the result
            assert any(oracle.decode(d[a:b], s.nch, cap)[2] & cm.ORA_DAMAGE and sum(a <= r[0] < b for r in R) > 1
                       for a, b in first_plan)
    if claim.get("merged"):
        assert len(spans) == 1 and len(R) == 2


@pytest.mark.parametrize("name", EDGES)
def test_edge_damages_are_isolated(pkg, oracle, name):
    """D flips, each in the non-sync unit of a segment of its own, the first D segments"""
    s = cc.stream(pkg.synth, cc.CASES[name].recipe)
    d = cc.damaged(pkg.synth, oracle, name)
    at = np.nonzero(d != s.b)[0].tolist()
    D = int(re.match(r"edge(\d+)", name).group(1))
    assert len(at) == D
    units = [max(j for j, o in enumerate(s.offs) if o <= p) for p in at]
    assert units == [2 * k + 1 for k in range(D)]
    assert not any(is_major_sync(s.b, s.offs[j]) for j in units)
    assert all(cm.unit_check(d, s.offs[j], s.S) for j in units), "every flip is one its unit's check data locates"
    R = cm.kept_ranges(d, s.nch, s.rpa, oracle)
    assert [r[:2] for r in R] == [(s.offs[2 * k], s.offs[2 * k + 1]) for k in range(D)] + [(s.offs[2 * D], len(d))]


def test_resume_cases_leave_only_the_resume_rule(pkg, oracle):
    """the refused major sync's unit verifies (header cases) -- the restart header alone refuses it -- or fails its CRC"""
    for name, want in (("resume_header", 0), ("resume_header_ss1", 0), ("resume_crc", 1 << 3)):
        s = cc.stream(pkg.synth, cc.CASES[name].recipe)
        d = cc.damaged(pkg.synth, oracle, name)
        p = s.syncs[2]
        sync = cm.packed_sync(s.b, 0)
        assert cm.can_resume(s.b, p, sync) and not cm.can_resume(d, p, sync)
        assert cm.unit_check(d, p, s.S) == want, name
        assert cm.can_resume(d, s.syncs[3], sync)


def test_adjacent_damage_has_nothing_between(pkg, oracle):
    s = cc.stream(pkg.synth, "six96")
    d = cc.damaged(pkg.synth, oracle, "adjacent")
    j = s.offs.index(s.syncs[2])
    assert cm.unit_check(d, s.offs[j - 1], s.S) and cm.unit_check(d, s.offs[j], s.S)
    _, spans = cc.expect(pkg.synth, oracle, "adjacent")
    assert spans[0][2] == s.offs[j - 1] and spans[0][3] == s.syncs[3]


def test_leading_bytes_and_the_even_scan(pkg, oracle):
    """the index looks for major syncs at even offsets of the stream: 3 bytes in front put every one at an odd offset"""
    s = cc.stream(pkg.synth, "stereo48")
    for n, found in ((2, True), (64, True), (3, False)):
        d = cc.damaged(pkg.synth, oracle, "lead%d" % n)
        assert bool(cm.sync_offsets(d)) == found
        assert bytes(d[n:]) == bytes(s.b) and set(d[:n].tolist()) == {0x55}
    d = cc.damaged(pkg.synth, oracle, "no_sync")
    assert len(d) == 4096 and b"\xF8\x72\x6F\xBB" not in bytes(d)


def test_ends(pkg, oracle):
    s = cc.stream(pkg.synth, "six96x2")
    d = cc.damaged(pkg.synth, oracle, "cut_odd")
    assert len(d) % 2 == 1 and s.offs[-1] < len(d) < len(s.b)
    R = cm.kept_ranges(d, s.nch, s.rpa, oracle, limits=cm.LIMITS)
    assert R[-1][1] == len(d), "the last range runs to the odd end: the gather's single last byte"
    s = cc.stream(pkg.synth, "mono48")
    d = cc.damaged(pkg.synth, oracle, "last_unit")
    _, spans = cc.expect(pkg.synth, oracle, "last_unit")
    assert spans == [(31 * 40, 0, s.offs[-1], len(d), cm.TRAILING)]
