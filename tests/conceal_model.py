"""The conceal-mode rule (include/dvda_mlp_hip.h, dvda_mlp_hip_set_conceal) restated on the host with the CPU oracle:
what a damaged stream must come out as, composed from oracle calls on byte ranges of it --

    oracle.decode(D[a0:b0]) ++ zeros(G1) ++ oracle.decode(D[a1:b1]) ++ ...

Kept ranges: a fresh decoder starts at the first major sync (of the stream's parameters) whose every substream opens
with a restart header and whose access unit verifies; the range ends in front of the first damaged access unit the
oracle stops at -- that unit itself when its framing / parity / CRC-8 fails, else the major sync that starts its
segment (the whole segment is damaged).  Silence between two ranges: the input-timing gap, wrapped by 65536 frames
to the stream's mean bytes per frame.
"""
import math

import numpy as np

ORA_DAMAGE = 0x1FD          # oracle status bits that mark damage (all but SYNC_CHANGE and ENVELOPE: a fresh decoder at a
                            # major sync that continues the FIR history is outside the reference's envelope, not damaged)
LEADING, TRAILING = 1, 2    # DVDA_CONCEAL_* span flags
ROUNDS = 4                  # DVDA_CONCEAL_ROUNDS: the span holds a range still damaged after the last decode round
LIMITS = (16, 4)            # (CONCEAL_MAX_RANGES, CONCEAL_ROUNDS) of csrc/mlp_conceal.h: tests/test_conceal_cases_model.py
                            # holds them to the headers
SYNC_PARAMS = 0x00FFFFFF


def u8(D, p):
    return int(D[p])


def au_size(D, p):
    return 2 * (((u8(D, p) & 0xF) << 8) | u8(D, p + 1))


def au_timing(D, p):
    return (u8(D, p + 2) << 8) | u8(D, p + 3)


def is_sync(D, p, lim=None):
    lim = len(D) if lim is None else lim
    if p + 32 > lim or au_size(D, p) < 32:
        return False
    return bytes(D[p + 4:p + 8]) == b"\xF8\x72\x6F\xBB" and (u8(D, p + 20) >> 4) in (1, 2)


def packed_sync(D, p):
    """SegRec.sync layout of csrc/mlp_index.h"""
    return ((u8(D, p + 8) >> 4) | ((u8(D, p + 8) & 0xF) << 4) | ((u8(D, p + 9) >> 4) << 8) |
            ((u8(D, p + 9) & 0xF) << 12) | ((u8(D, p + 11) & 0x1F) << 16) | ((u8(D, p + 20) >> 4) << 24))


def unit_check(D, p, S, lim=None):
    """0 when the access unit at p is framed and its substreams verify (reference src/mlp.c:656-712), else a bit"""
    lim = len(D) if lim is None else lim
    if p + 4 > lim:
        return 1 << 4
    size = au_size(D, p)
    if size < 4 or p + size > lim:
        return 1 << 4
    fe = p + size
    q = p + 32 if is_sync(D, p, fe) else p + 4
    ends, check = [], 0
    for s in range(S):
        if q + 2 > fe:
            return 1 << 4
        w = (u8(D, q) << 8) | u8(D, q + 1)
        if s == 0:
            check = (w >> 13) & 1
        ends.append((w & 0xFFF) * 2)
        q += 4 if w & 0x8000 else 2
    if q > fe:
        return 1 << 4
    prev = 0
    for e in ends:
        if e < prev or q + e > fe or (check and e - prev < 2):
            return 1 << 4
        if check:
            parity, crc, fin = 0, 0x3C, 0
            for k in range(q + prev, q + e - 2):
                v = u8(D, k)
                parity ^= v
                fin = crc ^ v
                crc = fin
                for _ in range(8):
                    crc = ((crc << 1) ^ 0x63) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
            if (u8(D, q + e - 2) ^ parity) != 0xA9:
                return 1 << 2
            if fin != u8(D, q + e - 1):
                return 1 << 3
        prev = e
    return 0


def can_resume(D, p, want):
    """a fresh decoder may start at p: major sync of the stream's parameters, every substream opens with a restart
    header (decode_block src/mlp.c:748-753), the unit verifies"""
    if not is_sync(D, p) or (packed_sync(D, p) ^ want) & SYNC_PARAMS:
        return False
    S = u8(D, p + 20) >> 4
    fe = p + au_size(D, p)
    if fe > len(D):
        return False
    q, end0 = p + 32, 0
    for s in range(S):
        if q + 2 > fe:
            return False
        w = (u8(D, q) << 8) | u8(D, q + 1)
        if s == 0:
            end0 = (w & 0xFFF) * 2
        q += 4 if w & 0x8000 else 2
    if q >= fe or (u8(D, q) & 0xC0) != 0xC0:
        return False
    if S == 2 and (q + end0 >= fe or (u8(D, q + end0) & 0xC0) != 0xC0):
        return False
    return unit_check(D, p, S) == 0


def sync_offsets(D):
    """every even offset that holds a major-sync access unit (what the index's pattern scan finds)"""
    b = np.asarray(D, np.uint8)
    hits = np.nonzero((b[4:-3] == 0xF8) & (b[5:-2] == 0x72) & (b[6:-1] == 0x6F) & (b[7:] == 0xBB))[0] if len(b) > 8 else []
    return [int(p) for p in hits if p % 2 == 0 and is_sync(D, int(p))]


def chain(D, a):
    """offsets of the access units the size chain from a frames (the walk stops where a unit cannot be framed)"""
    out, p = [], a
    while p + 4 <= len(D):
        size = au_size(D, p)
        if size < 4 or p + size > len(D):
            break
        out.append(p)
        p += size
    return out, p


def range_end(D, r, nch, oracle, cap, fresh=False):
    """-> where the range that a decoder opens at the usable major sync r of D ends (len(D): it runs to the end).
    fresh=False: the rule -- in front of the first unit whose own checks fail, or, when the oracle stops at a unit in front
    of that one, at the major sync of that unit's segment.  fresh=True: what k_conceal_plan can say of a range behind
    damage before the range has been decoded by itself -- the units' own checks only."""
    offs, chain_end = chain(D, r)
    S = u8(D, r + 20) >> 4

    def bad(e):
        return oracle.decode(D[r:e], nch, cap)[2] & ORA_DAMAGE

    unframed = chain_end + 4 <= len(D) and au_size(D, chain_end) < 4     # not a cut tail: a broken header
    if not fresh and not unframed and not bad(chain_end):
        # (the oracle verifies every unit's check data: nothing to look for unit by unit)
        u_c = None
    else:
        # the first unit whose own framing / check data fails
        u_c = next((k for k, o in enumerate(offs) if unit_check(D, o, S)), None)
    if u_c is None and unframed:
        u_c = len(offs)
        offs = offs + [chain_end]
    ends = offs[1:u_c + 1] if u_c is not None else offs[1:] + [chain_end]
    # the first unit the oracle's decode fails on in front of it (the oracle drops a failing unit and goes on:
    # the shortest failing prefix says which one)
    u_d = None
    if not fresh and ends and bad(ends[-1]):
        lo, hi = 0, len(ends) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if bad(ends[mid]):
                hi = mid
            else:
                lo = mid + 1
        u_d = lo
    if u_d is not None and (u_c is None or u_d < u_c):
        # nothing the unit says: its segment (from the major sync in front of it) is damaged whole
        return max(o for o in offs[:u_d + 1] if is_sync(D, o))
    if u_c is not None:
        return offs[u_c]                        # the unit itself is damaged
    return len(D)


def kept_ranges(D, nch, rows_per_au, oracle, cap=None, limits=None):
    """-> list of (a, b, frames, t_first, t_end): the kept byte ranges of D under the rule
    limits=(max_ranges, rounds): only those the library's plan and rounds reach (limited_ranges), without their flags"""
    D = np.asarray(D, np.uint8)
    cap = cap or (len(D) + 4096) * 2
    if limits is not None:
        return [r[:5] for r in limited_ranges(D, nch, oracle, cap, limits)[0]]
    syncs = sync_offsets(D)
    if not syncs:
        return []
    want = packed_sync(D, syncs[0])
    out, bound = [], 0
    while True:
        r = next((p for p in syncs if p >= bound and can_resume(D, p, want)), None)
        if r is None:
            return out
        kept_end = range_end(D, r, nch, oracle, cap)
        if kept_end > r:
            # behind the range's last unit: its first unit's input timing + the PCM frames the range decodes to
            _, frames, _ = oracle.decode(D[r:kept_end], nch, cap)
            out.append((r, kept_end, frames, au_timing(D, r), (au_timing(D, r) + frames) & 0xFFFF))
        if kept_end >= len(D):
            return out
        bound = kept_end + 2


def plan(P, nch, oracle, cap, max_ranges):
    """k_conceal_plan on a piece P (a caller's stream, or a range decoded again as a stream of its own) whose decode
    reported damage -> [(a, b)] relative to P.  A range that opens at the piece's first byte was decoded with the state a
    fresh decoder has there: the whole rule ends it.  A range behind damage was not (`fresh` in the kernel): only its
    units' own checks end it, and its decode is judged in the next round.  The plan's last slot is an open range to the
    piece's end.
    (The kernel checks the units of a segment only when the segment's decode status gives a reason: a damage bit, or that
    the fast pass left it to the sequential pass, which never got there.  The model checks every unit; the two agree as
    long as a unit that fails its checks makes its segment report one or the other, and the GPU file's 50 isolated flips
    hold the library to that: a flip can make a unit's timing look non-standard, DVDA_ST_TIMING alone.)"""
    syncs = sync_offsets(P)
    if not syncs:
        return []
    want = packed_sync(P, syncs[0])
    out, bound = [], 0
    while True:
        r = next((p for p in syncs if p >= bound and can_resume(P, p, want)), None)
        if r is None:
            return out
        if len(out) + 1 == max_ranges:
            return out + [(r, len(P))]
        kept_end = range_end(P, r, nch, oracle, cap, fresh=r != 0)
        if kept_end > r:
            out.append((r, kept_end))
        if kept_end >= len(P):
            return out
        bound = kept_end + 2


def limited_ranges(D, nch, oracle, cap, limits):
    """The rule as conceal_run reaches it -> ([(a, b, frames, t_first, t_end, flags)], tail_flags); flags: the
    DVDA_CONCEAL_* flags of the span in front of the range beyond LEADING / TRAILING, tail_flags: of the span behind the
    last one.

    Round 0 plans the stream (plan: at most max_ranges - 1 closed ranges and one open one).  Each of the rounds 1 ..
    rounds - 1 decodes every range not yet known to be clean as a stream of its own; a clean one is kept; a damaged one
    is planned again (the same plan, on the range) and its ranges go into the next round -- except in the last round,
    where nothing is planned any more: the damaged range is concealed whole, and the span it falls into carries ROUNDS.

    How far that reaches, for D isolated damages that the units' own checks locate (every plan is final then): the
    unlimited rule keeps D + 1 ranges.  Round 0 plans ranges 0 .. 14 closed and range 15 open; round 1 decodes those 16,
    the open one is damaged when D > 15 and is planned again: 15 .. 29 closed, 30 open; round 2 decodes those 16 and
    plans 30 .. 44 closed, 45 open; round 3, the last, decodes those 16 and plans nothing.  So rounds 1 .. 3 keep
    (max_ranges - 1) * (rounds - 1) = 45 closed ranges, and the open range of round 3 is kept only when it is clean,
    which is when it is the stream's last range: D + 1 <= 46.  D <= 14 needs no open range at all, D = 15 has a clean
    open range in round 1, D = 16 .. 30 need round 2 (30: clean open range), D = 31 .. 45 round 3 (45: clean open
    range), D >= 46 leaves everything from range 45's first byte on as one TRAILING | ROUNDS span.

    A range behind damage that holds damage its units' checks do not locate costs a round of its own: the plan passes
    over it, the range's own decode finds it, and the range is planned again."""
    max_ranges, rounds = limits
    items = [[a, b, 0, 0] for a, b in plan(D, nch, oracle, cap, max_ranges)]      # a, b, state (1: clean), flags
    tail_flags = 0
    for rnd in range(1, rounds):
        if all(it[2] for it in items):
            break
        nv, carry = [], 0
        for a, b, state, flags in items:
            flags |= carry
            carry = 0
            if state:
                nv.append([a, b, 1, flags])
            elif not oracle.decode(D[a:b], nch, cap)[2] & ORA_DAMAGE:
                nv.append([a, b, 1, flags])
            elif rnd + 1 == rounds:
                carry = flags | ROUNDS
            else:
                sub = plan(D[a:b], nch, oracle, cap, max_ranges)
                nv += [[a + x, a + y, 0, flags if k == 0 else 0] for k, (x, y) in enumerate(sub)]
        tail_flags |= carry
        items = nv
    out = []
    for a, b, state, flags in items:
        assert state, "a range no round decoded"
        frames = oracle.decode(D[a:b], nch, cap)[1]
        out.append((a, b, frames, au_timing(D, a), (au_timing(D, a) + frames) & 0xFFFF, flags))
    return out, tail_flags


def kept_units(D, R):
    """access units in the kept ranges R of D: what mlp_frames counts in conceal mode"""
    D = np.asarray(D, np.uint8)
    return sum(len(chain(D[r[0]:r[1]], 0)[0]) for r in R)


def gap_frames(B, g, m):
    """g + 65536 w, w >= 0 bringing B bytes per frame closest to m (no mean: g)"""
    if not m > 0:
        return g
    w0 = max(math.floor((B / m - g) / 65536.0), 0)
    best = None
    for k in (0, 1):
        G = g + 65536 * (w0 + k)
        d = abs(B / G - m) if G else math.inf
        if best is None or d < best[1]:
            best = (G, d)
    return best[0]


def conceal(D, nch, rows_per_au, oracle, cap=None, limits=None):
    """-> (pcm int32 [nch, frames], spans [(first_frame, frames, byte_off, byte_end, flags)]) under the rule
    limits=(max_ranges, rounds), the library's LIMITS: under the rule as far as its plans and rounds reach it
    (limited_ranges) -- what no round decoded clean is concealed, its span carries ROUNDS, and the mean bytes per frame
    is that of the ranges kept"""
    D = np.asarray(D, np.uint8)
    cap = cap or (len(D) + 4096) * 2
    if limits is None:
        R, tail_flags = [r + (0,) for r in kept_ranges(D, nch, rows_per_au, oracle, cap)], 0
    else:
        R, tail_flags = limited_ranges(D, nch, oracle, cap, limits)
    if not R:
        return np.zeros((nch, 0), np.int32), [(0, 0, 0, len(D), LEADING | TRAILING | tail_flags)]
    K = sum(r[1] - r[0] for r in R)
    F = sum(r[2] for r in R)
    m = K / F if K and F else 0.0
    parts, spans, pos = [], [], 0
    for k, (a, b, f, t_first, _, flags) in enumerate(R):
        if k == 0:
            if a > 0:
                spans.append((0, 0, 0, a, LEADING | flags))
        else:
            pb, pt_end = R[k - 1][1], R[k - 1][4]
            G = gap_frames(a - pb, (t_first - pt_end) & 0xFFFF, m)
            spans.append((pos, G, pb, a, flags))
            parts.append(np.zeros((nch, G), np.int32))
            pos += G
        pcm, _, _ = oracle.decode(D[a:b], nch, cap)
        parts.append(pcm)
        pos += f
    if R[-1][1] < len(D):
        spans.append((pos, 0, R[-1][1], len(D), TRAILING | tail_flags))
    return np.concatenate(parts, axis=1), spans
