"""Conceal mode's cases (csrc/mlp_conceal.h: k_conceal_plan, k_conceal_gather, k_conceal_move, k_conceal_fill;
csrc/mlp_conceal_run.h: conceal_run and its decode rounds), one table for the CPU file (tests/test_conceal_cases_model.py:
the premises, on the oracle and on the bytes) and the GPU file (tests/test_gpu_conceal_cases.py: the library against
tests/conceal_model.py with the library's limits, bit for bit).

TEST INFRASTRUCTURE.  Plain Python, no GPU.  A case is a stream recipe and a damage function; every position of a damage
comes from the undamaged stream's framing.  A case's `claim` says what the model must make of it -- the CPU file holds the
model to it, so that an edit to the generator fails there instead of emptying a GPU test:

    ranges      kept ranges of the limited model
    unlimited   kept ranges of the rule without the limits (default: the same)
    rounds      True: a span carries DVDA_CONCEAL_ROUNDS (default: none does)
    frames      PCM frames of the composed stream
    flags       the spans' flags, in order
    first       (access units, PCM frames) of the first kept range
    skipped     index of a major sync (among the undamaged stream's) at which no range may begin
    merged      True: one span stands for two damages (nothing kept between them)
    replanned   True: the plan of round 0 is not the result -- a range it holds is found damaged by its own decode and
                planned again; False: round 0's plan stands
    clean       True: the damage is none (the recipe's clean stream, decoded in the same batches)
"""
import collections

import numpy as np

from tests import conceal_model as cm
from tests.stream_tools import frame_offsets, is_major_sync

L, T = cm.LEADING, cm.TRAILING

Recipe = collections.namedtuple("Recipe", "asg rate S n_aus interval feats seed")

RECIPES = collections.OrderedDict(
    # ---- the shapes: (assignment, rate code, substreams); frames per access unit 40 / 80 / 160
    mono48=Recipe(0, 0, 1, 32, 8, (), 21),
    stereo48=Recipe(1, 0, 1, 48, 8, (), 22),
    six96=Recipe(12, 1, 1, 48, 8, (), 11),
    six96x2=Recipe(12, 1, 2, 48, 8, (), 23),
    six192x2=Recipe(12, 2, 2, 24, 8, (), 24),
    # ---- a major sync on every second unit: 52 segments, room for 50 damages one segment apart
    six96_r2=Recipe(12, 1, 1, 104, 2, (), 25),
    stereo48_r2=Recipe(1, 0, 1, 104, 2, (), 26),
    # ---- the generator's features (CHAINED with random FIR taps at the restart points, as encoders write them)
    chained=Recipe(12, 1, 1, 48, 8, ("CHAINED", "FIRRAND"), 11),
    chained_nocheck=Recipe(12, 1, 1, 48, 8, ("CHAINED", "FIRRAND", "NOCHECK"), 11),
    disc_chained=Recipe(12, 1, 2, 48, 8, ("DISC", "CHAINED", "FIRRAND"), 11),
    varrows=Recipe(12, 1, 1, 48, 8, ("VARROWS",), 11),
    nocheck=Recipe(12, 1, 1, 48, 8, ("NOCHECK",), 11),
)

Stream = collections.namedtuple("Stream", "b frames nch rpa S offs syncs")
_STREAMS = {}


def stream(syn, recipe):
    """the recipe's undamaged stream with its framing (cached: read-only)"""
    if recipe not in _STREAMS:
        r = RECIPES[recipe]
        f = 0
        for name in r.feats:
            f |= syn.SF[name]
        cfg = syn.make_cfg(assignment=r.asg, rate_code=r.rate, n_substreams=r.S, n_aus=r.n_aus, profile=1 if f else 0,
                           features=f, restart_interval=r.interval)
        b, frames = syn.stream(cfg, r.seed)
        b.setflags(write=False)
        offs = frame_offsets(b)
        _STREAMS[recipe] = Stream(b, frames, syn.channels(r.asg), syn.rows_per_au(r.rate), r.S, offs,
                                  [o for o in offs if is_major_sync(b, o)])
    return _STREAMS[recipe]


# ------------------------------------------------------------------------------------------------ damage functions
# each: (Stream, oracle) -> damaged copy of the stream's bytes

def mid(s, j):
    """the middle byte of access unit j"""
    end = s.offs[j + 1] if j + 1 < len(s.offs) else len(s.b)
    return s.offs[j] + (end - s.offs[j]) // 2


def flips(*units):
    """one bit flipped in the middle of each of the units"""
    def f(s, oracle):
        d = s.b.copy()
        for j in units:
            d[mid(s, j)] ^= 0x10
        return d
    return f


def isolated(n):
    """one bit flipped in the middle of the non-sync unit of the first n segments (restart interval 2)"""
    return flips(*[2 * k + 1 for k in range(n)])


def nocheck_damage(s, oracle, first):
    """a flip the oracle rejects in a unit j >= first without check data -> (damaged copy, j); None when there is none
    (test_conceal_model.nocheck_flip's search, for a Stream of any channel count)"""
    for j in range(first, len(s.offs) - 9):
        p = s.offs[j]
        if is_major_sync(s.b, p) or (int(s.b[p + 4]) >> 5) & 1:
            continue
        for k in range(p + 6, s.offs[j + 1] - 2):
            d = s.b.copy()
            d[k:k + 2] ^= 0xFF
            if oracle.decode(d[:s.offs[j + 1]], s.nch, s.frames)[2] & cm.ORA_DAMAGE:
                return d, j
    return None


def checked_unit(s, first):
    """the first unit j >= first that is no major sync and carries check data"""
    return next(j for j in range(first, len(s.offs)) if not is_major_sync(s.b, s.offs[j]) and (int(s.b[s.offs[j] + 4]) >> 5) & 1)


def checked_then_nocheck(s, oracle):
    """a flip that the unit's check data catches in the second segment, and in a later segment a flip in a unit without
    check data: the plan of round 0 passes over the second, the decode of round 1 finds it"""
    d, j = nocheck_damage(s, oracle, 25)
    k = checked_unit(s, 9)
    assert k < 16
    d[mid(s, k)] ^= 0x10
    return d


def nocheck_then_checked(s, oracle):
    """the mirror: the flip without check data in the second segment, the checked one behind it"""
    d, j = nocheck_damage(s, oracle, 9)
    assert j < 24
    d[mid(s, checked_unit(s, 33))] ^= 0x10
    return d


def nocheck_twice(s, oracle):
    """flips without check data in the second and in the fourth segment: each conceals its segment whole, and the second
    one is found only by the decode of the range that the first one's resume opens -- two plans behind the first.  A
    resume that took the concealed segment's own major sync again would need a round more for each and lose the tail"""
    d1, j1 = nocheck_damage(s, oracle, 9)
    d2, j2 = nocheck_damage(s, oracle, 25)
    assert 8 < j1 < 16 and 24 < j2 < 32
    d = d1.copy()
    at = np.nonzero(d2 != s.b)[0]
    d[at] = d2[at]
    return d


def nocheck_alone(s, oracle):
    return nocheck_damage(s, oracle, 17)[0]


def substream_starts(b, p, S):
    """-> (first byte of the substreams of the unit at p, [end of substream s relative to it], check flag)"""
    q = p + 32 if is_major_sync(b, p) else p + 4
    ends, check = [], 0
    for k in range(S):
        w = (int(b[q]) << 8) | int(b[q + 1])
        if k == 0:
            check = (w >> 13) & 1
        ends.append((w & 0xFFF) * 2)
        q += 4 if w & 0x8000 else 2
    return q, ends, check


def fix_checks(d, p, S):
    """writes the parity and CRC-8 bytes of the substreams of the unit at p again, so that the unit verifies (the
    arithmetic of conceal_model.unit_check)"""
    q, ends, check = substream_starts(d, p, S)
    assert check
    prev = 0
    for e in ends:
        parity, crc, fin = 0, 0x3C, 0
        for k in range(q + prev, q + e - 2):
            v = int(d[k])
            parity ^= v
            fin = crc ^ v
            crc = fin
            for _ in range(8):
                crc = ((crc << 1) ^ 0x63) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
        d[q + e - 2] = parity ^ 0xA9
        d[q + e - 1] = fin
        prev = e


def no_restart_header(substream):
    """a flip in the second segment, and the major sync behind it (the stream's third) loses the restart header of
    `substream` -- the unit's check data written again, so that nothing but the resume rule refuses that sync"""
    def f(s, oracle):
        d = s.b.copy()
        d[mid(s, 11)] ^= 0x10
        p = s.syncs[2]
        q, ends, _ = substream_starts(d, p, s.S)
        at = q + (ends[substream - 1] if substream else 0)
        assert int(d[at]) & 0xC0 == 0xC0
        d[at] &= 0x3F
        fix_checks(d, p, s.S)
        return d
    return f


def resume_crc(s, oracle):
    """a flip in the second segment, and the CRC byte of the major-sync unit behind it inverted"""
    d = s.b.copy()
    d[mid(s, 11)] ^= 0x10
    q, ends, check = substream_starts(d, s.syncs[2], s.S)
    assert check
    d[q + ends[0] - 1] ^= 0xFF
    return d


def adjacent(s, oracle):
    """damage in the last unit of the second segment and in the major-sync unit of the third: nothing kept between"""
    d = s.b.copy()
    j = s.offs.index(s.syncs[2])
    d[mid(s, j - 1)] ^= 0x10
    d[mid(s, j)] ^= 0x10
    return d


def leading(n):
    def f(s, oracle):
        return np.concatenate([np.full(n, 0x55, np.uint8), s.b])
    return f


def no_sync(s, oracle):
    """4 096 bytes of access units, none of them a major sync"""
    parts, n = [], 0
    for j, o in enumerate(s.offs[:-1]):
        if not is_major_sync(s.b, o):
            parts.append(s.b[o:s.offs[j + 1]])
            n += len(parts[-1])
            if n >= 4096:
                break
    return np.concatenate(parts)[:4096].copy()


def last_unit(s, oracle):
    return flips(len(s.offs) - 1)(s, oracle)


def first_and_last(s, oracle):
    return flips(0, len(s.offs) - 1)(s, oracle)


def cut_odd(s, oracle):
    """a flip in the second segment; the stream ends in the middle of its last unit, at an odd length"""
    d = flips(11)(s, oracle)
    cut = mid(s, len(s.offs) - 1) | 1
    return d[:cut].copy()


def zero2048(s, oracle):
    d = s.b.copy()
    d[mid(s, 13):mid(s, 13) + 2048] = 0
    return d


def delete_and_flip(s, oracle):
    d = s.b.copy()
    d[mid(s, 19)] ^= 0x10
    return np.concatenate([d[:mid(s, 5)], d[mid(s, 5) + 1024:]])


def clean(s, oracle):
    return s.b.copy()


# ---------------------------------------------------------------------------------------------------- the table
Case = collections.namedtuple("Case", "recipe damage group claim")
CASES = collections.OrderedDict()


def _case(name, recipe, damage, group, **claim):
    CASES[name] = Case(recipe, damage, group, claim)


# ---- plan and round edges: D isolated damages; the turns are derived in conceal_model.limited_ranges
#      (a plan holds 15 closed ranges and an open one; three decode rounds behind the first plan: 45, and a clean 46th)
for _D in (14, 15, 16, 17, 30, 31, 45):
    _case("edge%d" % _D, "six96_r2", isolated(_D), "edge", ranges=_D + 1)
for _D in (46, 50):
    _case("edge%d" % _D, "six96_r2", isolated(_D), "edge", ranges=45, unlimited=_D + 1, rounds=True)
_case("edge16_stereo", "stereo48_r2", isolated(16), "edge", ranges=17)
_case("edge45_stereo", "stereo48_r2", isolated(45), "edge", ranges=46)
_case("edge50_stereo", "stereo48_r2", isolated(50), "edge", ranges=45, unlimited=51, rounds=True)
# ---- round-2 discovery: damage that only the decode of a range behind damage can find
_case("round2_chained", "chained_nocheck", checked_then_nocheck, "round2", ranges=3, replanned=True)
_case("round2_plain", "nocheck", checked_then_nocheck, "round2", ranges=3, replanned=True)
_case("round2_mirror_chained", "chained_nocheck", nocheck_then_checked, "round2", ranges=3, replanned=False)
_case("round2_mirror_plain", "nocheck", nocheck_then_checked, "round2", ranges=3, replanned=False)
_case("nocheck_alone", "nocheck", nocheck_alone, "round2", ranges=2, replanned=False)
_case("nocheck_twice", "nocheck", nocheck_twice, "round2", ranges=3, replanned=True)
# ---- the resume rule: the major sync behind the damage is refused, the next one taken
_case("resume_header", "six96", no_restart_header(0), "shapes", ranges=2, skipped=2)
_case("resume_header_ss1", "six96x2", no_restart_header(1), "shapes", ranges=2, skipped=2)
_case("resume_crc", "six96", resume_crc, "shapes", ranges=2, skipped=2)
# ---- adjacent damage: one span
_case("adjacent", "six96", adjacent, "shapes", ranges=2, merged=True, skipped=2)
# ---- leading bytes (the index scans even offsets)
_case("lead2", "stereo48", leading(2), "shapes", ranges=1, flags=[L], frames=1920)
_case("lead64", "stereo48", leading(64), "shapes", ranges=1, flags=[L], frames=1920)
_case("lead3", "stereo48", leading(3), "shapes", ranges=0, flags=[L | T], frames=0)
_case("no_sync", "six96", no_sync, "shapes", ranges=0, flags=[L | T], frames=0)
# ---- ends
_case("last_unit", "mono48", last_unit, "shapes", ranges=1, flags=[T], frames=31 * 40)
_case("cut_odd", "six96x2", cut_odd, "shapes", ranges=2)
_case("first_and_last", "six192x2", first_and_last, "shapes", ranges=1, flags=[L, T])
# ---- non-standard timing: the range's scratch at the standard size is too small
_case("varrows_flip", "varrows", flips(19), "shapes", ranges=2, first=(19, 1785))
# ---- the other shapes and features, plain damage
_case("mono_flip", "mono48", flips(11), "shapes", ranges=2)
_case("stereo_two", "stereo48", flips(11, 35), "shapes", ranges=3)
_case("six96x2_zero2048", "six96x2", zero2048, "shapes", ranges=2)
_case("six192x2_delete_flip", "six192x2", delete_and_flip, "shapes", ranges=2, flags=[0, T])
_case("chained_flip", "chained", flips(19), "shapes", ranges=2)
_case("disc_chained_two", "disc_chained", flips(11, 35), "shapes", ranges=3)
# ---- the recipes' clean streams: in the same batches, as without conceal mode
for _r in RECIPES:
    _case("clean_" + _r, _r, clean, "edge" if _r.endswith("_r2") else "round2" if "nocheck" in _r else "shapes",
          clean=True, ranges=1)

GROUPS = ("edge", "round2", "shapes")
_DAMAGED = {}


def damaged(syn, oracle, name):
    """the case's damaged stream (cached: read-only)"""
    if name not in _DAMAGED:
        c = CASES[name]
        d = np.ascontiguousarray(c.damage(stream(syn, c.recipe), oracle), np.uint8)
        d.setflags(write=False)
        _DAMAGED[name] = d
    return _DAMAGED[name]


_EXPECT = {}


def expect(syn, oracle, name, limits=cm.LIMITS):
    """-> (pcm, spans) of the model with the library's limits for the case (cached: read-only)"""
    key = (name, limits)
    if key not in _EXPECT:
        s = stream(syn, CASES[name].recipe)
        pcm, spans = cm.conceal(damaged(syn, oracle, name), s.nch, s.rpa, oracle, limits=limits)
        pcm.setflags(write=False)
        _EXPECT[key] = (pcm, spans)
    return _EXPECT[key]


_UNITS = {}


def kept_units(syn, oracle, name, limits=cm.LIMITS):
    """access units in the case's kept ranges under the limited model: what mlp_frames reports (cached)"""
    key = (name, limits)
    if key not in _UNITS:
        s = stream(syn, CASES[name].recipe)
        d = damaged(syn, oracle, name)
        _UNITS[key] = cm.kept_units(d, cm.kept_ranges(d, s.nch, s.rpa, oracle, limits=limits))
    return _UNITS[key]
