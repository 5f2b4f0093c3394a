"""Helpers for tests that edit synthetic MLP byte streams (framing per reference src/mlp.c:384-405, 614-654)."""
import numpy as np


def frame_offsets(stream):
    """byte offset of every complete access unit (12-bit size chain)"""
    out, pos, n = [], 0, len(stream)
    while pos + 4 <= n:
        size = 2 * (((int(stream[pos]) & 0xF) << 8) | int(stream[pos + 1]))
        if size < 4 or pos + size > n:
            break
        out.append(pos)
        pos += size
    return out


def is_major_sync(stream, pos):
    return (len(stream) >= pos + 32 and bytes(stream[pos + 4:pos + 8]) == b"\xF8\x72\x6F\xBB" and
            (int(stream[pos + 20]) >> 4) in (1, 2))


def padded_unit(b, which, new_size):
    """stream `b` with access unit `which` grown to `new_size` bytes by zero bytes behind its last substream (the
    reference ignores what follows the last substream of a frame, src/mlp.c:463-468: the size field says where the
    next frame starts)"""
    pos = 0
    for _ in range(which):
        pos += 2 * (((int(b[pos]) & 0x0F) << 8) | int(b[pos + 1]))
    size = 2 * (((int(b[pos]) & 0x0F) << 8) | int(b[pos + 1]))
    assert new_size % 2 == 0 and size < new_size <= 8190
    out = np.concatenate([b[:pos + size], np.zeros(new_size - size, np.uint8), b[pos + size:]])
    w = new_size // 2
    out[pos] = (int(b[pos]) & 0xF0) | (w >> 8)
    out[pos + 1] = w & 0xFF
    return out


def major_syncs(stream):
    """byte offset of every major-sync access unit"""
    return [p for p in frame_offsets(stream) if is_major_sync(stream, p)]


def splice(a, b, sync_index):
    """the access units of `a` in front of its `sync_index`-th major sync (0 = the stream's first), then `b` from its
    `sync_index`-th major sync on"""
    return np.concatenate([a[:major_syncs(a)[sync_index]], b[major_syncs(b)[sync_index]:]])


def cuts_at_units(stream):
    """where every complete access unit ends: fed as packets [0, c0), [c0, c1), ... each call holds one unit (the last
    one also what follows the last complete unit)"""
    return frame_offsets(stream)[1:] + [len(stream)]


def change_sync_params(stream, which, g1_bps=None, assignment=None):
    """Returns a copy of `stream` whose `which`-th major syncs (indices into the list of major-sync access
    units, 0 = the stream's first) announce other stream parameters: group-1 bits-per-sample code and / or
    channel assignment -- two of the five fields reference dvda_params_equal compares (src/mlp.c:449-460).
    Nothing else changes; the major sync is covered by no parity / CRC byte the reference checks."""
    out = np.array(stream, np.uint8, copy=True)
    syncs = [p for p in frame_offsets(out) if is_major_sync(out, p)]
    for w in which:
        p = syncs[w]
        if g1_bps is not None:
            out[p + 8] = (int(out[p + 8]) & 0xF0) | (g1_bps & 0xF)
        if assignment is not None:
            out[p + 11] = (int(out[p + 11]) & 0xE0) | (assignment & 0x1F)
    return out, [syncs[w] for w in which]
