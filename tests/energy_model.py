"""The energy report of decoded PCM (include/dvda_mlp_hip.h, dvda_pcm_energy_block; csrc/pcm_energy.h) restated with
Python integers.

The contract, for one stream of `frames` PCM frames with `channels` channels, a block length B and a first-block length
`lead` in 1 .. B:

    frame f lies in block 0 when f < lead, else in block 1 + (f - lead) // B
    nblocks = 0 for no frames, else 1 + ceil(max(frames - lead, 0) / B)
    per block and channel: sq = sum of v * v (exact; stored as sq_hi * 2^64 + sq_lo), peak = largest |v|
    frames = the frames the block holds; entries at index `channels` and above are 0

A record is a dict as hipdec.EnergyBlock.as_dict() gives it: sq_lo, sq_hi, peak (eight ints each) and frames.

append() joins a piece's blocks to a track's, total() folds blocks into one record, next_lead() is the lead of the piece
that follows `frames` frames of a track.

Test infrastructure only."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u" % name, text).group(1))


MIN_BLOCK = _header_constant("DVDA_NRG_MIN_BLOCK")
MAX_BLOCK = _header_constant("DVDA_NRG_MAX_BLOCK")
PIECE = _header_constant("DVDA_NRG_PIECE_FRAMES")
MAX_CHANNELS = 8
M64 = (1 << 64) - 1


def nblocks(frames, B, lead=None):
    lead = B if lead is None else lead
    if frames <= 0 or not 1 <= lead <= B:
        return 0
    return 1 + -(-max(frames - lead, 0) // B)


def block_of(f, B, lead):
    return 0 if f < lead else 1 + (f - lead) // B


def record(sq, peak, frames):
    sq = list(sq) + [0] * (8 - len(sq))
    peak = list(peak) + [0] * (8 - len(peak))
    return dict(sq_lo=[s & M64 for s in sq], sq_hi=[s >> 64 for s in sq], peak=peak, frames=frames)


def sums(rec):
    return [(h << 64) | l for l, h in zip(rec["sq_lo"], rec["sq_hi"])]


def energy(planar, B, lead=None):
    """straight from the definition; planar: int32 [channels, frames] -> the stream's records"""
    planar = np.asarray(planar)
    ch, frames = planar.shape
    lead = B if lead is None else lead
    if not 1 <= ch <= MAX_CHANNELS or not 1 <= lead <= B:
        return []
    out = []
    start = 0
    while start < frames:
        end = min(frames, lead if start == 0 else start + B)
        assert block_of(start, B, lead) == block_of(end - 1, B, lead) == len(out)
        sq, peak = [], []
        for c in range(ch):
            vals = [int(v) for v in planar[c, start:end]]
            sq.append(sum(v * v for v in vals))
            peak.append(max(abs(v) for v in vals))
        out.append(record(sq, peak, end - start))
        start = end
    assert len(out) == nblocks(frames, B, lead)
    return out


def energy_fast(planar, B, lead=None):
    """energy() for long streams: the squares in numpy as two exact halves (|v| = h * 2^16 + l), summed per block"""
    planar = np.asarray(planar)
    ch, frames = planar.shape
    lead = B if lead is None else lead
    if not 1 <= ch <= MAX_CHANNELS or not 1 <= lead <= B:
        return []
    a = np.abs(planar.astype(np.int64)).astype(np.uint64)
    h, l = a >> np.uint64(16), a & np.uint64(0xFFFF)
    hh, hl, ll = h * h, h * l, l * l            # each below 2^32: a block of 2^24 frames sums below 2^56
    edges = [0] + list(range(min(lead, frames), frames, B)) + [frames] if frames else [0]
    edges = sorted(set(edges))
    out = []
    for s, e in zip(edges[:-1], edges[1:]):
        sq = [(int(hh[c, s:e].sum()) << 32) + (int(hl[c, s:e].sum()) << 17) + int(ll[c, s:e].sum()) for c in range(ch)]
        out.append(record(sq, [int(a[c, s:e].max()) for c in range(ch)], e - s))
    assert len(out) == nblocks(frames, B, lead)
    return out


def next_lead(frames_so_far, B):
    return B - frames_so_far % B


def add_into(t, p):
    """block p added into block t (a new record)"""
    sq = [x + y for x, y in zip(sums(t), sums(p))]
    return record(sq, [max(x, y) for x, y in zip(t["peak"], p["peak"])], t["frames"] + p["frames"])


def append(track, piece, B):
    """the track's blocks with the piece joined to them (a new list); ValueError when the piece is not on the grid"""
    if not piece:
        return list(track)
    merge = bool(track) and track[-1]["frames"] < B
    head = (track[-1]["frames"] if merge else 0) + piece[0]["frames"]
    if head > B or (len(piece) > 1 and head != B):
        raise ValueError("the piece is not on the track's grid")
    for j in range(1, len(piece)):
        if piece[j]["frames"] > B or (j + 1 < len(piece) and piece[j]["frames"] != B):
            raise ValueError("a short block inside the piece")
    if merge:
        return list(track[:-1]) + [add_into(track[-1], piece[0])] + list(piece[1:])
    return list(track) + list(piece)


def total(blocks):
    out = record([0] * 8, [0] * 8, 0)
    for b in blocks:
        out = add_into(out, b)
    out["frames"] = min(out["frames"], 0xFFFFFFFF)
    return out


def pieces_of_stream(frames, B, lead=None):
    """pieces of the kernels' flat list a stream has: ceil(L / PIECE) per block of L frames"""
    lead = B if lead is None else lead
    if frames <= 0 or not 1 <= lead <= B:
        return 0
    l0 = min(frames, lead)
    rest = frames - l0
    return -(-l0 // PIECE) + (rest // B) * -(-B // PIECE) + -(-(rest % B) // PIECE)
