"""The channel mix of include/dvda_mlp_hip.h (csrc/pcm_mix.h) restated: once with Python integers, one value at a time,
once in numpy int64 over a whole [channels, frames] array -- exact, because a valid row has sum |coef| <= 2^31, so
|acc| <= 2^62 and acc + 2^29 < 2^63 -- and the integer recipe of the default matrices."""
import numpy as np

TILE = 4096                     # DVDA_LVL_TILE_FRAMES: the pass's tiles, aligned to a stream's first frame
DEPTHS = (16, 20, 24)
Q = 30
ONE, A, HALF = 1 << 30, 759250125, 1 << 29      # A = rint(2^30 / sqrt 2)
NORMALIZED, UNITY, LFE = 0, 1, 2                # DVDA_MIX_*
FL, FR, FC, LF, BL, BR, BC = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x100
MASKS = [FC, FL | FR, FL | FR | BC, FL | FR | BL | BR, FL | FR | LF, FL | FR | LF | BC, FL | FR | LF | BL | BR,
         FL | FR | FC, FL | FR | FC | BC, FL | FR | FC | BL | BR, FL | FR | FC | LF, FL | FR | FC | LF | BC,
         FL | FR | FC | LF | BL | BR, FL | FR | FC | BC, FL | FR | FC | BL | BR, FL | FR | FC | LF,
         FL | FR | FC | LF | BC, FL | FR | FC | LF | BL | BR, FL | FR | BL | BR | LF, FL | FR | BL | BR | FC,
         FL | FR | BL | BR | FC | LF]           # per DVD-Audio channel assignment 0..20
MAX_ROW = 1 << 31               # the largest sum of |coef| a valid row has


def speaker_mask(assignment):
    return MASKS[assignment] if 0 <= assignment < 21 else 0


# ---- a matrix: dict(in_channels, out_channels, coef [8][8] of int), as hipdec.PcmMix.as_dict() gives it
def matrix(in_channels, out_channels, rows):
    """rows[o][c] for o < out, c < in; the rest of the 8 x 8 is zero"""
    coef = [[0] * 8 for _ in range(8)]
    for o, row in enumerate(rows):
        for c, g in enumerate(row):
            coef[o][c] = int(g)
    return dict(in_channels=int(in_channels), out_channels=int(out_channels), coef=coef)


def identity(ch):
    return matrix(ch, ch, [[ONE if c == o else 0 for c in range(ch)] for o in range(ch)])


def valid(m):
    if not (1 <= m["in_channels"] <= 8 and 1 <= m["out_channels"] <= 8):
        return False
    return all(sum(abs(g) for g in m["coef"][o][:m["in_channels"]]) <= MAX_ROW for o in range(m["out_channels"]))


def weights(bit, flags):
    """(wL, wR) of the speaker `bit`"""
    lfe = A if flags & LFE else 0
    return {FL: (ONE, 0), FR: (0, ONE), FC: (A, A), LF: (lfe, lfe), BL: (A, 0), BR: (0, A), BC: (HALF, HALF)}[bit]


def default_matrix(mask, out_channels, flags=0):
    """the integer recipe of dvda_pcm_hip_mix_matrix; None where that answers EINVAL"""
    if mask == 0 or mask & ~0x13F or out_channels not in (1, 2) or flags & ~3:
        return None
    bits = [1 << b for b in range(9) if mask >> b & 1]
    w = [[weights(b, flags)[o] for b in bits] for o in range(2)]
    if out_channels == 1:
        w = [[l + r for l, r in zip(*w)]]
    if flags & UNITY:
        rows = [[g >> 1 for g in w[0]]] if out_channels == 1 else w
    else:
        s = max(sum(row) for row in w)
        rows = [[(g << 30) // s if s else 0 for g in row] for row in w]
    return matrix(len(bits), out_channels, rows)


# ---- Python integers
def finish(acc, bits):
    """-> (output value, 1 when the clamp changed it else 0)"""
    q = (acc + (1 << (Q - 1))) >> Q
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return min(max(q, lo), hi), int(q < lo or q > hi)


def value(x, m, o, bits):
    """output channel o of the frame whose values are x -> (value, clipped)"""
    assert valid(m) and o < m["out_channels"] and len(x) == m["in_channels"] and bits in DEPTHS
    return finish(sum(int(g) * int(v) for g, v in zip(m["coef"][o], x)), bits)


def mix(pcm, m, bits):
    """the integer form over [in_channels, frames] -> (int32 [out_channels, frames], clipped per OUTPUT channel, 8 entries)"""
    ch, n = pcm.shape
    assert ch == m["in_channels"]
    out = np.zeros((m["out_channels"], n), np.int32)
    clipped = [0] * 8
    for o in range(m["out_channels"]):
        for f in range(n):
            out[o, f], cl = value([int(v) for v in pcm[:, f]], m, o, bits)
            clipped[o] += cl
    return out, clipped


# ---- numpy
def mix_np(pcm, m, bits):
    """the numpy form -> (int32 array, clipped per OUTPUT channel, 8 entries)"""
    ch, n = pcm.shape
    assert valid(m) and ch == m["in_channels"] and bits in DEPTHS
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    x = pcm.astype(np.int64)
    out = np.zeros((m["out_channels"], n), np.int32)
    clipped = [0] * 8
    for o in range(m["out_channels"]):
        acc = np.zeros(n, np.int64)
        for c in range(ch):
            acc += np.int64(m["coef"][o][c]) * x[c]     # (partial sums stay inside sum |coef| * 2^31 <= 2^62)
        v = (acc + (1 << (Q - 1))) >> Q
        clipped[o] = int(((v < lo) | (v > hi)).sum())
        out[o] = np.clip(v, lo, hi)
    return out, clipped


def report(frames, clipped):
    """as hipdec.PcmMixReport.as_dict() gives it"""
    return dict(frames=int(frames), clipped=[int(c) for c in clipped])


NOT_TAKEN = report(0, [0] * 8)


def add_reports(a, b):
    return report(a["frames"] + b["frames"], [x + y for x, y in zip(a["clipped"], b["clipped"])])


def random_matrix(rng, ich, och, full_rows=()):
    """a valid matrix with coefficients of both signs; the rows in full_rows have sum |coef| == 2^31 exactly"""
    rows = []
    for o in range(och):
        mag = rng.integers(0, MAX_ROW // ich + 1, ich, dtype=np.int64)
        if o in full_rows:
            mag[int(rng.integers(ich))] += MAX_ROW - int(mag.sum())
        sign = rng.integers(0, 2, ich) * 2 - 1
        g = mag * sign
        g[g > (1 << 31) - 1] = -(1 << 31)           # (+2^31 is no int32: the one entry that large goes negative)
        rows.append([int(v) for v in g])
    m = matrix(ich, och, rows)
    assert valid(m) and all(sum(abs(g) for g in rows[o]) == MAX_ROW for o in full_rows if o < och)
    return m
