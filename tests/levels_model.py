"""The level report of decoded PCM (include/dvda_mlp_hip.h, dvda_pcm_levels; csrc/pcm_levels.h) restated in numpy.

The contract, for one stream of `frames` PCM frames with `channels` channels (RIFF-WAVE order) at nominal depth `bits`
(16, 20 or 24):

    frames        PCM frames covered
    lead_silent   frames from the start in which every channel is 0
    trail_silent  frames up to the end in which every channel is 0      (an all-zero stream: both == frames)
    sum[c]        exact sum of the channel's values
    over[c]       values outside [-2^(bits-1), 2^(bits-1) - 1]
    min[c], max[c]
    entries at index `channels` and above are 0; frames == 0 gives all zeros

The decomposition the kernels use (tile_partial / join):

    tiles   DVDA_LVL_TILE_FRAMES frames each, aligned to the START of the stream: the last tile is the ragged one
    record  per tile: the first frame of the tile that holds a non-zero value (NONE: there is none), the last such frame
            + 1 (0: none), and per channel min, max, over, sum
    join    min of the mins, max of the maxes, sums of over and sum; lead_silent = the smallest (tile start + first)
            (none: frames), trail_silent = frames - the largest (tile start + last + 1) (none: frames - 0)

combine() is the host arithmetic that joins the reports of two pieces, A || B.

Test infrastructure only."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u" % name, text).group(1))


TILE = _header_constant("DVDA_LVL_TILE_FRAMES")
NONE = 0xFFFFFFFF
MAX_CHANNELS = 8


def zero():
    return dict(frames=0, lead_silent=0, trail_silent=0, sum=[0] * 8, over=[0] * 8, min=[0] * 8, max=[0] * 8)


def levels(planar, bits):
    """straight from the definition; planar: int32 [channels, frames]"""
    planar = np.asarray(planar)
    ch, frames = planar.shape
    out = zero()
    if frames == 0 or not 1 <= ch <= MAX_CHANNELS:
        return out
    v = planar.astype(np.int64)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    out["frames"] = frames
    loud = np.flatnonzero((v != 0).any(axis=0))
    out["lead_silent"] = int(loud[0]) if len(loud) else frames
    out["trail_silent"] = frames - 1 - int(loud[-1]) if len(loud) else frames
    for c in range(ch):
        out["sum"][c] = int(v[c].sum())
        out["over"][c] = int(((v[c] < lo) | (v[c] > hi)).sum())
        out["min"][c] = int(v[c].min())
        out["max"][c] = int(v[c].max())
    return out


def tile_partial(tile, bits):
    """the record of one tile (int32 [channels, 1..TILE]) -> (first, last1, [(min, max, over, sum) per channel])"""
    tile = np.asarray(tile).astype(np.int64)
    ch, nf = tile.shape
    assert 1 <= nf <= TILE
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    loud = np.flatnonzero((tile != 0).any(axis=0))
    first = int(loud[0]) if len(loud) else NONE
    last1 = int(loud[-1]) + 1 if len(loud) else 0
    per = [(int(tile[c].min()), int(tile[c].max()), int(((tile[c] < lo) | (tile[c] > hi)).sum()), int(tile[c].sum()))
           for c in range(ch)]
    return first, last1, per


def join(records, frames, ch):
    """a stream's tile records, in order -> the report"""
    out = zero()
    if frames == 0:
        return out
    assert len(records) == -(-frames // TILE)
    out["frames"] = frames
    lead, end = frames, 0
    for i, (first, last1, per) in enumerate(records):
        if first != NONE:
            lead = min(lead, i * TILE + first)
        if last1:
            end = max(end, i * TILE + last1)
        for c in range(ch):
            mn, mx, over, sm = per[c]
            out["min"][c] = mn if i == 0 else min(out["min"][c], mn)
            out["max"][c] = mx if i == 0 else max(out["max"][c], mx)
            out["over"][c] += over
            out["sum"][c] += sm
    out["lead_silent"] = lead
    out["trail_silent"] = frames - end
    return out


def levels_by_tiles(planar, bits):
    planar = np.asarray(planar)
    ch, frames = planar.shape
    return join([tile_partial(planar[:, f:f + TILE], bits) for f in range(0, frames, TILE)], frames, ch)


def combine(a, b):
    """the report of A || B"""
    if a["frames"] == 0 or b["frames"] == 0:
        src = a if a["frames"] else b
        return {k: (list(v) if isinstance(v, list) else v) for k, v in src.items()}
    out = zero()
    out["frames"] = a["frames"] + b["frames"]
    out["lead_silent"] = a["frames"] + b["lead_silent"] if a["lead_silent"] == a["frames"] else a["lead_silent"]
    out["trail_silent"] = b["frames"] + a["trail_silent"] if b["trail_silent"] == b["frames"] else b["trail_silent"]
    for c in range(8):
        out["sum"][c] = a["sum"][c] + b["sum"][c]
        out["over"][c] = a["over"][c] + b["over"][c]
        out["min"][c] = min(a["min"][c], b["min"][c])
        out["max"][c] = max(a["max"][c], b["max"][c])
    return out
