"""The decimation of include/dvda_mlp_hip.h (csrc/pcm_decim.h) restated: once with Python integers, one value at a time,
once in numpy int64 over a whole [channels, frames] array -- exact, because sum |h| * 2^31 + 2^29 < 2^63 -- and the piece
arithmetic.  The taps are the library's committed table (hipdec.decim_taps); callers hand them in."""
import numpy as np

TILE = 1024                     # DVDA_DCM_TILE_FRAMES: OUTPUT frames of a tile, aligned to a stream's first output frame
RATIOS = (2, 4)
DEPTHS = (16, 20, 24)
Q = 30


def n_taps(ratio):
    return 96 * ratio - 1


def half(ratio):
    return 48 * ratio - 1


def ceil_div(a, d):
    return -(-a // d)


def out_frames(frame0, own, ratio):
    """the M with frame0 <= ratio * M < frame0 + own"""
    return ceil_div(frame0 + own, ratio) - ceil_div(frame0, ratio)


# ---- Python integers
def finish(acc, bits):
    """-> (output value, 1 when the clamp changed it else 0)"""
    q = (acc + (1 << (Q - 1))) >> Q
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return min(max(q, lo), hi), int(q < lo or q > hi)


def value(window, taps, bits):
    """one output value from its window of 2 H + 1 input values -> (value, clipped)"""
    assert len(window) == len(taps) and bits in DEPTHS
    return finish(sum(int(h) * int(x) for h, x in zip(taps, window)), bits)


def decimate(region, taps, ratio, bits, frame0=0, before=0, after=0):
    """the integer form over a region [channels, before + own + after] -> (int32 array [channels, out_frames], clipped
    per channel, 8 entries).  What the region does not hold is 0."""
    ch, n = region.shape
    own = n - before - after
    assert own >= 0 and len(taps) == n_taps(ratio)
    H = half(ratio)
    m0 = ceil_div(frame0, ratio)
    nm = out_frames(frame0, own, ratio)
    out = np.zeros((ch, nm), np.int32)
    clipped = [0] * 8
    for c in range(ch):
        row = [int(v) for v in region[c]]
        for m in range(nm):
            j = before + ratio * (m0 + m) - frame0          # the region's index of the centre
            win = [row[i] if 0 <= i < n else 0 for i in range(j - H, j + H + 1)]
            out[c, m], cl = value(win, taps, bits)
            clipped[c] += cl
    return out, clipped


# ---- numpy
def decimate_np(region, taps, ratio, bits, frame0=0, before=0, after=0):
    """the numpy form -> (int32 array, clipped per channel, 8 entries)"""
    ch, n = region.shape
    own = n - before - after
    assert own >= 0 and len(taps) == n_taps(ratio) and bits in DEPTHS
    H = half(ratio)
    nm = out_frames(frame0, own, ratio)
    first = before + ratio * ceil_div(frame0, ratio) - frame0       # the region's index of output 0's centre
    out = np.zeros((ch, nm), np.int32)
    clipped = [0] * 8
    if nm == 0:
        return out, clipped
    # the region with zeros around it, so that every window lies inside: index i of the region at i + lead
    lead = max(H - first, 0)
    tail = max(first + ratio * (nm - 1) + H + 1 - n, 0)
    h = np.asarray(taps, np.int64)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for c in range(ch):
        x = np.concatenate([np.zeros(lead, np.int64), region[c].astype(np.int64), np.zeros(tail, np.int64)])
        start = first + lead - H
        acc = np.zeros(nm, np.int64)
        for k in range(len(h)):
            if h[k]:
                acc += h[k] * x[start + k:start + k + ratio * (nm - 1) + 1:ratio]
        q = (acc + (1 << (Q - 1))) >> Q
        clipped[c] = int(((q < lo) | (q > hi)).sum())
        out[c] = np.clip(q, lo, hi)
    return out, clipped


def cut(track, a, b, context_before, context_after):
    """the piece [a, b) of a track [channels, frames] with up to that much context on either side, as far as the track
    reaches -> (region, frame0, before, after)"""
    before = min(context_before, a)
    after = min(context_after, track.shape[1] - b)
    return track[:, a - before:b + after], a, before, after


def report(frames_in, frames_out, clipped):
    """as hipdec.DecimReport.as_dict() gives it"""
    return dict(frames_in=int(frames_in), frames_out=int(frames_out), clipped=[int(c) for c in clipped])


def add_reports(a, b):
    return report(a["frames_in"] + b["frames_in"], a["frames_out"] + b["frames_out"],
                  [x + y for x, y in zip(a["clipped"], b["clipped"])])


def payload(pcm, bits):
    """the WAV data chunk of int32 PCM [channels, frames] at 16 or 24 bits: frame-major, little-endian -> bytes"""
    assert bits in (16, 24)
    v = np.ascontiguousarray(pcm.T).reshape(-1).astype(np.int64)
    w = (v & ((1 << (bits - 1)) - 1)) | np.where(v < 0, 1 << (bits - 1), 0)
    b = np.empty((w.size, bits // 8), np.uint8)
    for k in range(bits // 8):
        b[:, k] = (w >> (8 * k)) & 0xFF
    return b.tobytes()
