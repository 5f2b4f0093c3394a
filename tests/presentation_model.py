"""The presentation rule (include/dvda_mlp_hip.h, dvda_mlp_hip_set_presentation) restated on the host: the
*presentation stream* of a two-substream MLP stream is the one-substream stream that is left when substream 1 is
taken out of every access unit -- substream 0's own restart headers, filters, matrices and output shifts then give
the 2-channel (k-channel) mix a 2-channel decoder plays.  A one-substream stream is its own presentation stream.

Per complete access unit of the size chain, in order:
    frame header   the 4 check bits and the 16-bit input timing kept, the 12-bit length = the new unit's 16-bit words
    major sync     its 28 bytes with substream count 1 and the identity assignment of k channels
    directory      substream 0's word (and its extra word) kept, substream 1's dropped
    body           bytes [0, 2 * substream_end_0) of the substream area; a range that leaves the unit is clamped to it
k = substream 0's max_matrix_channel + 1 from the restart header of the stream's first unit.
"""
import numpy as np

from tests.stream_tools import frame_offsets, is_major_sync

IDENTITY_ASSIGNMENT = {1: 0x00, 2: 0x01, 3: 0x02, 4: 0x03, 5: 0x06}
ST_ENVELOPE = 1 << 9


def _unit_parts(D, p, fe, S):
    """-> (sync bytes or 0, [d, d_end) of substream 0's directory words, [q, q_end) of substream 0's body) of the unit
    [p, fe) of a stream of S substreams; every range clamped to the unit"""
    sync = 28 if (is_major_sync(D, p) and p + 32 <= fe) else 0
    d = p + 4 + sync
    q, ranges = d, []
    for s in range(S):
        if q + 2 > fe:
            ranges.append((q, q, 0))
            continue
        w = (int(D[q]) << 8) | int(D[q + 1])
        n = min(4 if w & 0x8000 else 2, fe - q)
        ranges.append((q, q + n, (w & 0xFFF) * 2))
        q += n
    d0, d0_end, end0 = ranges[0]
    return sync, (d0, d0_end), (q, min(q + end0, fe))


def channels_of(stream):
    """k of a two-substream stream (None: its first unit's substream 0 does not begin with a restart header, or k has
    no identity assignment); the channel count of the assignment is the caller's business for one substream"""
    D = np.asarray(stream, np.uint8)
    offs = frame_offsets(D)
    if not offs or not is_major_sync(D, 0):
        return None
    fe = offs[1] if len(offs) > 1 else offs[0] + 2 * (((int(D[0]) & 0xF) << 8) | int(D[1]))
    _, _, (q, q_end) = _unit_parts(D, 0, fe, 2)
    if q_end - q < 6 or (int(D[q]) & 0xC0) != 0xC0:
        return None
    k = (int(D[q + 5]) >> 4) + 1
    return k if k in IDENTITY_ASSIGNMENT else None


def substreams_of(stream):
    D = np.asarray(stream, np.uint8)
    return int(D[20]) >> 4 if is_major_sync(D, 0) else 0


def strip(stream):
    """-> (presentation stream as uint8 array, k or None for a one-substream stream, status: 0 or ST_ENVELOPE)"""
    D = np.asarray(stream, np.uint8)
    if substreams_of(D) != 2:
        return D.copy(), None, 0
    k = channels_of(D)
    if k is None:
        return np.zeros(0, np.uint8), None, ST_ENVELOPE
    offs = frame_offsets(D)
    out = []
    for j, p in enumerate(offs):
        fe = p + 2 * (((int(D[p]) & 0xF) << 8) | int(D[p + 1]))
        sync, (d, d_end), (q, q_end) = _unit_parts(D, p, fe, 2)
        words = (4 + sync + (d_end - d) + (q_end - q)) // 2
        hdr = np.array([(int(D[p]) & 0xF0) | (words >> 8), words & 0xFF, D[p + 2], D[p + 3]], np.uint8)
        out.append(hdr)
        if sync:
            ms = D[p + 4:p + 32].copy()
            ms[7] = (int(ms[7]) & 0xE0) | IDENTITY_ASSIGNMENT[k]         # unit byte 11: the 5-bit assignment
            ms[16] = (int(ms[16]) & 0x0F) | 0x10                         # unit byte 20: substream count
            out.append(ms)
        out.append(D[d:d_end])
        out.append(D[q:q_end])
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), k, 0


def consumed(stream):
    """source bytes covered by complete access units"""
    D = np.asarray(stream, np.uint8)
    offs = frame_offsets(D)
    if not offs:
        return 0
    p = offs[-1]
    return p + 2 * (((int(D[p]) & 0xF) << 8) | int(D[p + 1]))


_EXPECT = {}


def expect(stream, oracle, nch=None):
    """-> (pcm int32 [k, frames], frames, oracle status, k): the presentation stream decoded by the oracle as the
    one-substream stream it now is (nch: the channel count of a one-substream source's assignment).  Cached."""
    D = np.asarray(stream, np.uint8)
    key = (D.tobytes(), nch)
    if key not in _EXPECT:
        s, k, st = strip(D)
        if st:
            _EXPECT[key] = (np.zeros((0, 0), np.int32), 0, st, None)
        else:
            k = k if k is not None else nch
            pcm, frames, ost = oracle.decode(s, k, len(s) + 4096)
            _EXPECT[key] = (pcm, frames, ost, k)
    return _EXPECT[key]
