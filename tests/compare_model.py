"""The compare of two PCM buffers (include/dvda_mlp_hip.h, dvda_pcm_diff; csrc/pcm_compare.h) restated in numpy.

The contract, for one pair of streams A (`frames_a` frames) and B (`frames_b` frames) with the same `channels` (1..8,
RIFF-WAVE order), over the first compared = min(frames_a, frames_b) frames:

    bits == 0           the int32 values as they are; |a - b| in 64 bits, at most 2^32 - 1
    bits == 16, 20, 24  every value first as it would be written, written(): (v & (2^(bits-1) - 1)) - (v < 0 ? 2^(bits-1) : 0)
    diff_frames         frames in which at least one channel differs
    first_diff          the smallest such frame (none: compared);  diff_end  the largest + 1 (none: 0)
    runs                maximal runs of consecutive differing frames
    diff_values[c]      values of channel c that differ;  max_abs[c]  the largest |a - b| of the channel
    entries at index `channels` and above are 0
    channel counts that differ, or outside 1..8: flags = CMP_SHAPE, nothing compared, channels = 0

The decomposition the kernels use (tile_partial / join):

    tiles   DVDA_CMP_TILE_FRAMES frames each, aligned to the START of the pair: the last tile is the ragged one
    bitmap  one bit per frame of the tile, "this frame differs", in 64 words of 64 bits; frames behind `compared` are zero
            bits.  Word i with the top bit of word i - 1 as carry gives count (popcount), first / last (lowest / highest
            set bit) and runs = popcount(m & ~((m << 1) | carry)); the tile's first and last frame give two edge bits.
    record  per tile: first (NONE: there is none), end, count, runs, the edge bits, per channel (values, max)
    join    sums, minima and maxima; runs = the sum of the tiles' runs - the neighbouring tiles of which the earlier one's
            last frame and the later one's first frame both differ

combine() is the host arithmetic that joins the diffs of two pieces: diff(A1 || A2, B1 || B2).

Test infrastructure only."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u" % name, text).group(1))


TILE = _header_constant("DVDA_CMP_TILE_FRAMES")
CMP_SHAPE = _header_constant("DVDA_CMP_SHAPE")
NONE = 0xFFFFFFFF
MAX_CHANNELS = 8
M64 = (1 << 64) - 1


def zero():
    return dict(frames_a=0, frames_b=0, compared=0, diff_frames=0, first_diff=0, diff_end=0, runs=0,
                diff_values=[0] * 8, max_abs=[0] * 8, channels=0, flags=0)


def written(v, bits):
    """int32 values (as int64) as they would be written at `bits`; bits == 0: as they are"""
    v = np.asarray(v).astype(np.int64)
    if bits == 0:
        return v
    h = 1 << (bits - 1)
    return (v & (h - 1)) - np.where(v < 0, h, 0)


def _taken(ch):
    return 1 <= ch <= MAX_CHANNELS


def diff(a, b, bits):
    """straight from the definition; a, b: int32 [channels, frames], planar"""
    a, b = np.asarray(a), np.asarray(b)
    out = zero()
    out["frames_a"] = a.shape[1] if _taken(a.shape[0]) else 0
    out["frames_b"] = b.shape[1] if _taken(b.shape[0]) else 0
    if a.shape[0] != b.shape[0] or not _taken(a.shape[0]):
        out["flags"] = CMP_SHAPE
        return out
    ch = a.shape[0]
    n = min(a.shape[1], b.shape[1])
    out["channels"], out["compared"], out["first_diff"] = ch, n, n
    d = np.abs(written(a[:, :n], bits) - written(b[:, :n], bits))
    frames = np.flatnonzero((d != 0).any(axis=0))
    if len(frames):
        out["diff_frames"] = len(frames)
        out["first_diff"], out["diff_end"] = int(frames[0]), int(frames[-1]) + 1
        out["runs"] = 1 + int((np.diff(frames) > 1).sum())
    for c in range(ch):
        out["diff_values"][c] = int((d[c] != 0).sum())
        out["max_abs"][c] = int(d[c].max()) if n else 0
    return out


def tile_partial(ta, tb, bits):
    """the record of one tile (int32 [channels, 1..TILE] each, the same shape) -> (first, end, count, runs, head, tail,
    [(values, max) per channel]), the per-frame part from the bitmap as the kernel derives it"""
    d = np.abs(written(ta, bits) - written(tb, bits))
    ch, nf = d.shape
    assert 1 <= nf <= TILE
    bit = np.zeros(TILE, bool)
    bit[:nf] = (d != 0).any(axis=0)
    words = [sum(1 << int(k) for k in np.flatnonzero(bit[64 * i:64 * i + 64])) for i in range(TILE // 64)]
    first, end, count, runs = NONE, 0, 0, 0
    for i, m in enumerate(words):
        carry = words[i - 1] >> 63 if i else 0
        count += bin(m).count("1")
        runs += bin(m & ~((m << 1 | carry) & M64) & M64).count("1")
        if m:
            first = min(first, 64 * i + (m & -m).bit_length() - 1)
            end = max(end, 64 * i + m.bit_length())
    head = words[0] & 1
    tail = words[(nf - 1) >> 6] >> ((nf - 1) & 63) & 1
    per = [(int((d[c] != 0).sum()), int(d[c].max())) for c in range(ch)]
    return first, end, count, runs, head, tail, per


def join(records, out, ch):
    """a pair's tile records, in order, into the figures of `out` (frames_a, frames_b, compared, channels are set)"""
    assert len(records) == -(-out["compared"] // TILE)
    first, end = out["compared"], 0
    for i, (f, e, count, runs, head, tail, per) in enumerate(records):
        if f != NONE:
            first = min(first, i * TILE + f)
        if e:
            end = max(end, i * TILE + e)
        out["diff_frames"] += count
        out["runs"] += runs - (1 if i and head and records[i - 1][5] else 0)
        for c in range(ch):
            out["diff_values"][c] += per[c][0]
            out["max_abs"][c] = max(out["max_abs"][c], per[c][1])
    out["first_diff"], out["diff_end"] = first, end
    return out


def diff_by_tiles(a, b, bits):
    a, b = np.asarray(a), np.asarray(b)
    out = zero()
    out["frames_a"] = a.shape[1] if _taken(a.shape[0]) else 0
    out["frames_b"] = b.shape[1] if _taken(b.shape[0]) else 0
    if a.shape[0] != b.shape[0] or not _taken(a.shape[0]):
        out["flags"] = CMP_SHAPE
        return out
    n = min(a.shape[1], b.shape[1])
    out["channels"], out["compared"] = a.shape[0], n
    return join([tile_partial(a[:, f:min(f + TILE, n)], b[:, f:min(f + TILE, n)], bits) for f in range(0, n, TILE)], out,
                a.shape[0])


def _copy(d):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in d.items()}


def combine(a, b):
    """diff(A1 || A2, B1 || B2) from a = diff(A1, B1) and b = diff(A2, B2); None where the library says EINVAL: either
    carries CMP_SHAPE; or, neither being neutral (no frames on either side, no flag), the first piece's sides have
    different lengths or the channel counts differ"""
    if (a["flags"] | b["flags"]) & CMP_SHAPE:
        return None
    for x, other in ((a, b), (b, a)):
        if x["frames_a"] == 0 and x["frames_b"] == 0 and not x["flags"]:
            return _copy(other)
    if a["frames_a"] != a["frames_b"] or a["channels"] != b["channels"]:
        return None
    out = zero()
    for k in ("frames_a", "frames_b", "compared", "diff_frames"):
        out[k] = a[k] + b[k]
    out["first_diff"] = a["first_diff"] if a["first_diff"] < a["compared"] else a["compared"] + b["first_diff"]
    out["diff_end"] = a["compared"] + b["diff_end"] if b["diff_end"] else a["diff_end"]
    seam = a["diff_end"] == a["compared"] and a["compared"] and b["compared"] and b["first_diff"] == 0
    out["runs"] = a["runs"] + b["runs"] - (1 if seam else 0)
    for c in range(8):
        out["diff_values"][c] = a["diff_values"][c] + b["diff_values"][c]
        out["max_abs"][c] = max(a["max_abs"][c], b["max_abs"][c])
    out["channels"] = a["channels"]
    return out
