"""The word-length reduction of include/dvda_mlp_hip.h (csrc/pcm_requant.h) restated: once with Python integers, one value
at a time, once in numpy over a whole [channels, frames] array, and the WAV payload of the result."""
import numpy as np

TILE = 4096                     # DVDA_LVL_TILE_FRAMES: the pass's tiles, aligned to the start of a stream
TRUNCATE, ROUND, TPDF = 0, 1, 2
DEPTHS = (16, 20, 24)
M64 = (1 << 64) - 1
G, C1, C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def params_ok(bits_in, bits_out, mode):
    return bits_in in DEPTHS and bits_out in DEPTHS and bits_out <= bits_in and mode in (TRUNCATE, ROUND, TPDF)


# ---- Python integers
def word(seed, quad, ch):
    """output number 8 * quad + ch + 1 of splitmix64 seeded with `seed`"""
    z = (seed + G * (8 * quad + ch + 1)) & M64
    z = ((z ^ (z >> 30)) * C1) & M64
    z = ((z ^ (z >> 27)) * C2) & M64
    return z ^ (z >> 31)


def noise(seed, frame, ch, s):
    """u1 - u2 of absolute frame `frame` of channel ch"""
    f = (word(seed, frame >> 2, ch) >> (16 * (frame & 3))) & 0xFFFF
    m = (1 << s) - 1
    return (f & m) - ((f >> 8) & m)


def value(v, bits_in, bits_out, mode, seed, frame, ch):
    """-> (output value, 1 when the clamp changed it else 0)"""
    assert params_ok(bits_in, bits_out, mode)
    s = bits_in - bits_out
    v = int(v)
    if s:
        if mode != TRUNCATE:
            v += 1 << (s - 1)
        if mode == TPDF:
            v += noise(seed, frame, ch, s)
        v >>= s
    lo, hi = -(1 << (bits_out - 1)), (1 << (bits_out - 1)) - 1
    return min(max(v, lo), hi), int(v < lo or v > hi)


def requant(pcm, bits_in, bits_out, mode, seed=0, frame0=0):
    """the integer form over an array [channels, frames] -> (int32 array, clipped per channel, 8 entries)"""
    ch, n = pcm.shape
    out = np.zeros((ch, n), np.int32)
    clipped = [0] * 8
    for c in range(ch):
        for f in range(n):
            out[c, f], cl = value(pcm[c, f], bits_in, bits_out, mode, seed, frame0 + f, c)
            clipped[c] += cl
    return out, clipped


# ---- numpy
def word_np(seed, quad, ch):
    u = np.uint64
    with np.errstate(over="ignore"):
        z = u(seed) + u(G) * (u(8) * quad.astype(np.uint64) + u(ch + 1))
        z = (z ^ (z >> u(30))) * u(C1)
        z = (z ^ (z >> u(27))) * u(C2)
        return z ^ (z >> u(31))


def noise_np(seed, frames, ch, s):
    """u1 - u2 (int64) of the absolute frames `frames` (a uint64 array) of channel ch"""
    u = np.uint64
    f = (word_np(seed, frames >> u(2), ch) >> (u(16) * (frames & u(3)))) & u(0xFFFF)
    m = u((1 << s) - 1)
    return (f & m).astype(np.int64) - ((f >> u(8)) & m).astype(np.int64)


def requant_np(pcm, bits_in, bits_out, mode, seed=0, frame0=0):
    """the numpy form -> (int32 array, clipped per channel, 8 entries)"""
    assert params_ok(bits_in, bits_out, mode)
    s = bits_in - bits_out
    ch, n = pcm.shape
    with np.errstate(over="ignore"):
        fr = np.arange(n, dtype=np.uint64) + np.uint64(frame0)
    out = np.zeros((ch, n), np.int32)
    clipped = [0] * 8
    lo, hi = -(1 << (bits_out - 1)), (1 << (bits_out - 1)) - 1
    for c in range(ch):
        v = pcm[c].astype(np.int64)
        if s:
            if mode != TRUNCATE:
                v = v + (1 << (s - 1))
            if mode == TPDF:
                v = v + noise_np(seed, fr, c, s)
            v = v >> s
        clipped[c] = int(((v < lo) | (v > hi)).sum())
        out[c] = np.clip(v, lo, hi)
    return out, clipped


# ---- the payload
def payload(pcm, bits):
    """the WAV data chunk of int32 PCM [channels, frames] at 16 or 24 bits: frame-major, every value as write_signed(bits),
    little-endian -> bytes"""
    assert bits in (16, 24)
    v = np.ascontiguousarray(pcm.T).reshape(-1).astype(np.int64)
    w = (v & ((1 << (bits - 1)) - 1)) | np.where(v < 0, 1 << (bits - 1), 0)
    b = np.empty((w.size, bits // 8), np.uint8)
    for k in range(bits // 8):
        b[:, k] = (w >> (8 * k)) & 0xFF
    return b.tobytes()


def report(frames, clipped):
    """as hipdec.RequantReport.as_dict() gives it"""
    return dict(frames=int(frames), clipped=[int(c) for c in clipped])
