"""The 48 kHz -> 44.1 kHz resampler of include/dvda_mlp_hip.h (csrc/pcm_resample.h) restated: once with Python integers,
one value at a time, once in numpy int64 over a whole [channels, frames] array -- exact, because sum |g| * 2^31 + 2^29 <
2^63 -- and the piece arithmetic.  The table is the library's committed one (hipdec.resample_taps); callers hand it in."""
import numpy as np

UP, DOWN = 147, 160             # 48 000 Hz * 147 / 160 = 44 100 Hz
TAPS = 96
FRONT = 47                      # input frames of a window in front of frame q = (160 m) div 147; 48 behind it
TILE = 9408                     # DVDA_RSM_TILE_FRAMES: OUTPUT frames of a tile, aligned to a stream's first output frame
DEPTHS = (16, 20, 24)
Q = 30


def ceil_div(a, d):
    return -(-a // d)


def first_out(frame):
    """the first output frame m whose q = (160 m) div 147 is at or behind the absolute input frame `frame`"""
    return ceil_div(UP * frame, DOWN)


def out_frames(frame0, own):
    """the m with frame0 <= (160 m) div 147 < frame0 + own"""
    return first_out(frame0 + own) - first_out(frame0)


def out_frames_brute(frame0, own):
    """... counted"""
    m = max(UP * frame0 // DOWN - 2, 0)
    n = 0
    while DOWN * m // UP < frame0 + own:
        n += DOWN * m // UP >= frame0
        m += 1
    return n


# ---- Python integers
def finish(acc, bits):
    """-> (output value, 1 when the clamp changed it else 0)"""
    q = (acc + (1 << (Q - 1))) >> Q
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return min(max(q, lo), hi), int(q < lo or q > hi)


def value(window, row, bits):
    """one output value from its window of 96 input values and its phase's row of the table -> (value, clipped)"""
    assert len(window) == TAPS and len(row) == TAPS and bits in DEPTHS
    return finish(sum(int(g) * int(x) for g, x in zip(row, window)), bits)


def resample(region, table, bits, frame0=0, before=0, after=0):
    """the integer form over a region [channels, before + own + after] -> (int32 array [channels, out_frames], clipped
    per channel, 8 entries).  What the region does not hold is 0."""
    ch, n = region.shape
    own = n - before - after
    assert own >= 0 and tuple(np.shape(table)) == (UP, TAPS)
    m0 = first_out(frame0)
    nm = out_frames(frame0, own)
    out = np.zeros((ch, nm), np.int32)
    clipped = [0] * 8
    rows = [[int(v) for v in r] for r in table]
    for c in range(ch):
        x = [int(v) for v in region[c]]
        for k in range(nm):
            q, p = divmod(DOWN * (m0 + k), UP)
            j = before + q - frame0 - FRONT             # the region's index of the window's first frame
            win = [x[i] if 0 <= i < n else 0 for i in range(j, j + TAPS)]
            out[c, k], cl = value(win, rows[p], bits)
            clipped[c] += cl
    return out, clipped


# ---- numpy
def resample_np(region, table, bits, frame0=0, before=0, after=0):
    """the numpy form -> (int32 array, clipped per channel, 8 entries)"""
    ch, n = region.shape
    own = n - before - after
    assert own >= 0 and tuple(np.shape(table)) == (UP, TAPS) and bits in DEPTHS
    m0 = first_out(frame0)
    nm = out_frames(frame0, own)
    out = np.zeros((ch, nm), np.int32)
    clipped = [0] * 8
    if nm == 0:
        return out, clipped
    m = np.arange(m0, m0 + nm, dtype=np.int64)
    q, p = (DOWN * m) // UP, (DOWN * m) % UP
    start = q - frame0 + before - FRONT                 # the region's index of every window's first frame
    lead = max(-int(start.min()), 0)
    tail = max(int(start.max()) + TAPS - n, 0)
    g = np.asarray(table, np.int64)[p]                  # [nm, TAPS]
    idx = (start + lead)[:, None] + np.arange(TAPS)[None, :]
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for c in range(ch):
        x = np.concatenate([np.zeros(lead, np.int64), region[c].astype(np.int64), np.zeros(tail, np.int64)])
        acc = (g * x[idx]).sum(axis=1)
        v = (acc + (1 << (Q - 1))) >> Q
        clipped[c] = int(((v < lo) | (v > hi)).sum())
        out[c] = np.clip(v, lo, hi)
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
