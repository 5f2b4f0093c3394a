"""Sector builder, case table and plain model for the sector tier.

TEST INFRASTRUCTURE.  disc._sector writes one sector shape: one audio packet, no stuffing, pad_1 = 0 and an even
payload offset.  build_sector() composes a 2048-byte sector from an explicit list of packets instead, SECTOR_SHAPES
names the cases tests/test_sector_model.py (no GPU) and tests/test_gpu_sectors.py share, and the model says what every
sector holds:

    raw PCM      pcm_oracle_decode_sectors (oracle/pcm_oracle.c, pinned to the compiled src/pcm.c) one sector at a time;
                 -1 = "bad: contributes nothing, counted", the contract of include/dvda_mlp_hip.h
    demux        walk() below: a few lines by the rules of src/packet.c and src/dvd-audio.c
    WAV payload  wav_oracle_pack

Nothing here calls the code under test."""
import ctypes
import struct

import numpy as np

import libdvd_audio_amd.disc as disc
from tests import oracle_lib

SECTOR = 2048
LAYOUTS = [(16, 1, 0), (16, 2, 1), (16, 3, 2), (16, 4, 3), (16, 5, 6), (16, 6, 12),
           (24, 1, 0), (24, 2, 1), (24, 3, 2), (24, 4, 3), (24, 5, 6), (24, 6, 12)]
MLP_CHUNK = 5          # MLP payloads read a shape's "chunks" as runs of 5 bytes: odd, so that dst & 3 moves
MAX_AUDIO = 8          # audio packets per sector the kernels keep; a ninth makes the sector malformed


# ------------------------------------------------------------------------------------------------ shapes
def A(pay, pad1=0, pad2x=0, codec=None):
    """An audio packet (0xBD).  pay: ("c", chunks, extra_bytes) | ("rest",) = every byte up to the end of the sector
    (less what the packets behind it need).  pad2x: pad_2 bytes beyond the parameter block (PCM: 9 + pad2x; MLP:
    pad2x), or "fit": the fewest that leave the rest of the sector whole chunks.  codec: override (malformed cases)."""
    return {"kind": "A", "pay": pay, "pad1": pad1, "pad2x": pad2x, "codec": codec}


def O(sid, length):
    """Any other PES packet: 0xBE padding, 0xBF, 0xBB ... with `length` body bytes."""
    return {"kind": "O", "sid": sid, "len": length}


def shape(pkts, stuffing=0, stray=0):
    return {"pkts": pkts, "stuffing": stuffing, "stray": stray}


def _c(n, extra=0):
    return ("c", n, extra)


REST = ("rest",)

SECTOR_SHAPES = {
    # ---- one packet, payload offset & 3 = 0, 1, 2, 3 (stuffing moves it byte by byte)
    "off0": shape([A(_c(20, 3))], stuffing=0),
    "off1": shape([A(_c(21, 1))], stuffing=1),
    "off2": shape([A(_c(22, 2))], stuffing=2),
    "off3": shape([A(_c(23))], stuffing=3),
    "off1_pad1": shape([A(_c(9), pad1=5, pad2x=0)], stuffing=0),
    "off3_pad2": shape([A(_c(9), pad1=0, pad2x=3)], stuffing=4),
    "stuffing7_pad1_255": shape([A(_c(7, 1), pad1=255, pad2x=246)], stuffing=7),
    # ---- packet counts; the packets of one sector start at different off & 3; non-audio in front, between, behind
    "two": shape([A(_c(5, 1), pad1=1), A(_c(6, 2), pad1=0, pad2x=2)], stuffing=1),
    "three_others": shape([O(0xBB, 12), A(_c(4, 1)), O(0xBF, 9), A(_c(3, 2), pad1=2), O(0xBE, 0), A(_c(5), pad2x=1),
                           O(0xBF, 3)], stuffing=2),
    "eight": shape([A(_c(2, k % 3), pad1=k % 4, pad2x=(3 * k) % 5) for k in range(8)], stuffing=3),
    "eight_and_others": shape([O(0xBE, 1)] + [A(_c(1 + k % 2, 1), pad1=(k * 3) % 4) for k in range(8)] + [O(0xBB, 2)]),
    # ---- chunks per packet: 0 (shorter than a chunk), 1, 63, 64, 65, the most that fit; remainders dropped per packet
    "zero_chunks": shape([A(_c(0, 1)), A(_c(2)), A(_c(0, 3), pad1=1)], stuffing=1),
    "empty_payload": shape([A(_c(0, 0)), A(_c(1, 1), pad1=2)]),
    "one_chunk": shape([A(_c(1)), A(_c(1, 1), pad1=1), A(_c(1, 2), pad1=2)], stuffing=3),
    "c63": shape([A(_c(63), pad1=1)]),
    "c64": shape([A(_c(64), pad1=2)]),
    "c65": shape([A(_c(65), pad1=3)]),
    "c63_c1": shape([A(_c(63, 1), pad1=1), A(_c(1, 1))], stuffing=2),
    "most": shape([A(REST)], stuffing=0),
    "most_off1": shape([A(REST, pad1=1)], stuffing=0),
    "most_off2": shape([A(REST, pad1=0, pad2x=1)], stuffing=1),
    "small_then_most": shape([O(0xBE, 2), A(_c(1, 1), pad1=1), A(REST, pad1=2, pad2x=1)], stuffing=1),
    # ---- sector boundaries: whole chunks up to byte 2047 -- the last chunk's dword window reads the extra LDS vector
    "to_the_end": shape([A(REST, pad2x="fit")], stuffing=1),
    "to_the_end_two": shape([A(_c(3, 1), pad1=1), A(REST, pad1=3, pad2x="fit")], stuffing=2),
    # ---- 1-5 stray bytes behind the last packet (the reference stops reading the track there, the kernels go on)
    "stray1": shape([A(REST, pad1=1)], stuffing=1, stray=1),
    "stray5": shape([A(_c(4, 1)), A(REST, pad1=2)], stuffing=0, stray=5),
}

# MLP payloads in bytes: shorter than the head run (0-3), 4-7, and runs that leave dst & 3 at every value
MLP_SHAPES = dict(SECTOR_SHAPES)
MLP_SHAPES.update({
    "mlp_tiny": shape([A(("b", k), pad1=k % 3, pad2x=k % 2) for k in (1, 2, 3, 0, 1, 3, 2, 1)], stuffing=1),
    "mlp_4_to_7": shape([A(("b", k), pad1=(k + 1) % 4) for k in (4, 5, 6, 7, 7, 6, 5, 4)], stuffing=2),
    "mlp_dst_walk": shape([A(("b", k), pad2x=k % 3) for k in (9, 1, 10, 2, 11, 3, 64 * 4 + 3, 13)], stuffing=3),
    "mlp_no_pad2": shape([A(REST, pad1=1, pad2x=0)], stuffing=0),
    # packets long enough to complete an access unit each (the reference ends a track at a packet that does not)
    "mlp_big3": shape([O(0xBB, 5), A(("b", 601)), O(0xBF, 2), A(("b", 602), pad1=2, pad2x=1), A(REST, pad1=1)],
                      stuffing=3),
    "mlp_big2": shape([A(("b", 803), pad1=3), A(("b", 801), pad1=1, pad2x=2), O(0xBE, 40)], stuffing=2),
})

RULES = ("start_code", "marker0", "marker1", "marker2", "marker3", "marker4", "marker5", "pes_start", "overrun",
         "plen_lt_7", "plen_lt_pad1", "codec", "pad2_lt_9", "hdr_gt_plen", "ninth")


# ------------------------------------------------------------------------------------------------ builder
def params_block(bps, asg, rate_code=0):
    code = {16: 0, 24: 2}[bps]
    return struct.pack(">HBBBBBBB", 0, 0, (code << 4) | code, (rate_code << 4) | rate_code, 0, asg, 0, 0)


def pack_header(stuffing):
    h = bytearray(disc._pack_header())
    assert 0 <= stuffing <= 7
    h[13] = (h[13] & 0xF8) | stuffing
    return bytes(h) + b"\xFF" * stuffing


def build_sector(sh, chunk, params, codec, source):
    """One sector of shape `sh`.  chunk: bytes per PCM chunk (MLP: MLP_CHUNK); params: the PCM parameter block or b"";
    source(n) -> the next n payload bytes.  Returns (sector bytes, [payload offset per audio packet])."""
    # 63, 64 and 65 chunks of 36 bytes (24-bit, 6 channels) do not fit a sector: that layout gets the 52 that do
    pkts = [dict(p, pay=("c", p["pay"][1] if p["pay"][1] * chunk <= 1950 else 1900 // chunk, p["pay"][2]))
            if p["kind"] == "A" and p["pay"][0] == "c" else p for p in sh["pkts"]]
    head = pack_header(sh["stuffing"])
    fixed = len(head) + sh["stray"]
    for p in pkts:                                   # what every packet needs apart from a "rest" payload
        if p["kind"] == "O":
            fixed += 6 + p["len"]
        else:
            fixed += 6 + 7 + p["pad1"] + len(params) + (0 if p["pad2x"] == "fit" else p["pad2x"])
            if p["pay"][0] == "c":
                fixed += p["pay"][1] * chunk + p["pay"][2]
            elif p["pay"][0] == "b":
                fixed += p["pay"][1]
    out, offs = bytearray(head), []
    for p in pkts:
        if p["kind"] == "O":
            out += b"\x00\x00\x01" + bytes([p["sid"]]) + struct.pack(">H", p["len"]) + b"\xFF" * p["len"]
            continue
        pad2x = p["pad2x"]
        if p["pay"][0] == "rest":
            n = SECTOR - fixed
            if pad2x == "fit":
                pad2x = n % chunk
                n -= pad2x
        else:
            n = p["pay"][1] * chunk + p["pay"][2] if p["pay"][0] == "c" else p["pay"][1]
        assert n >= 0 and pad2x != "fit"
        pad2 = len(params) + pad2x
        assert pad2 <= 255
        body = (b"\x81\x00" + bytes([p["pad1"]]) + b"\xC3" * p["pad1"] +
                bytes([codec if p["codec"] is None else p["codec"], 0, 0, pad2]) + params + b"\x5A" * pad2x)
        offs.append(len(out) + 6 + len(body))
        body += source(n)
        out += b"\x00\x00\x01\xBD" + struct.pack(">H", len(body)) + body
    room = SECTOR - sh["stray"] - len(out)
    assert room == 0 or room >= 6, "cannot tile the sector: %d bytes left" % room
    if room:
        out += b"\x00\x00\x01\xBE" + struct.pack(">H", room - 6) + b"\xFF" * (room - 6)
    out += b"\xA5" * sh["stray"]
    assert len(out) == SECTOR
    return bytes(out), offs


def pattern_samples(bps, ch, n_chunks, salt):
    """[2 * n_chunks, ch] samples.  Every byte of a chunk's sample block differs from the others of the chunk (its
    index in the chunk plus a salt per chunk), so a wrong permute selector cannot go unnoticed; the second chunk of a
    run holds both rails of the width in every channel."""
    nb = bps // 8
    cs = 2 * ch * nb
    k = np.arange(n_chunks * cs, dtype=np.int64).reshape(n_chunks, cs)
    by = ((k % cs) + 1 + (salt + 41 * (k // cs)) * 37) & 0xFF
    by = by.reshape(n_chunks * 2 * ch, nb)
    v = sum(by[:, b] << (8 * b) for b in range(nb))
    v = np.where(v & (1 << (bps - 1)), v - (1 << bps), v).reshape(n_chunks * 2, ch)
    if n_chunks >= 2:
        v[2, :] = -(1 << (bps - 1))
        v[3, :] = (1 << (bps - 1)) - 1
    return v


def swizzle(samples, bps):
    """[frames, ch] samples -> AOB payload bytes, by disc.AOB_BYTE_SWAP (the muxer's tables, src/pcm.c:103-139)"""
    samples = np.asarray(samples, np.int64)
    frames, ch = samples.shape
    nb = bps // 8
    cs = 2 * ch * nb
    flat = samples.reshape(-1) & ((1 << bps) - 1)
    le = np.zeros((frames * ch, nb), np.uint8)
    for b in range(nb):
        le[:, b] = (flat >> (8 * b)) & 0xFF
    le = le.reshape(frames // 2, cs)
    aob = np.zeros_like(le)
    for i, s in enumerate(disc.AOB_BYTE_SWAP[bps][ch - 1]):
        aob[:, i] = le[:, s]
    return aob.tobytes()


def pcm_sector(sh, bps, ch, asg, salt=0):
    """-> (sector, samples [frames, ch] it carries, payload offsets).  A remainder behind a packet's last whole chunk
    is junk: src/pcm.c:147 drops it per packet, it is not carried over."""
    cs = 2 * ch * (bps // 8)
    got = []

    def source(n):
        s = pattern_samples(bps, ch, n // cs, salt + 7 * len(got))
        got.append(s)
        return swizzle(s, bps) + bytes((0xE0 + i) & 0xFF for i in range(n % cs))

    sec, offs = build_sector(sh, cs, params_block(bps, asg), disc.PCM_CODEC, source)
    return sec, np.concatenate(got) if got else np.zeros((0, ch), np.int64), offs


def mlp_sector(sh, data, pos):
    """-> (sector, bytes of `data` consumed, payload offsets): consecutive slices of one byte string, zeros behind
    its end"""
    used = [0]

    def source(n):
        b = bytes(data[pos + used[0]:pos + used[0] + n])
        used[0] += n
        return b + b"\x00" * (n - len(b))

    sec, offs = build_sector(sh, MLP_CHUNK, b"", disc.MLP_CODEC, source)
    return sec, used[0], offs


def mlp_sectors(names, data):
    """`data` carried by the MLP shapes `names`, repeated until it is all muxed -> list of sectors"""
    out, pos, i = [], 0, 0
    while pos < len(data):
        sec, n, _ = mlp_sector(MLP_SHAPES[names[i % len(names)]], data, pos)
        out.append(sec)
        pos += n
        i += 1
    return out


def good_base(codec_params, codec, n_audio=1):
    """a plain well-formed sector to mutate: small audio packets (plen < 262), a padding packet behind them"""
    sh = shape([A(("b", 24), pad1=1, pad2x=2) for _ in range(n_audio)], stuffing=1)
    return bytearray(build_sector(sh, 1, codec_params, codec, lambda n: bytes(range(1, n + 1)))[0])


def malformed(rule, bps=16, asg=1, mlp=False):
    """One field of a good sector changed so that exactly `rule` of the walk rejects it."""
    params = b"" if mlp else params_block(bps, asg)
    codec = disc.MLP_CODEC if mlp else disc.PCM_CODEC
    s = good_base(params, codec, 9 if rule == "ninth" else 1)
    pos = 14 + 1                               # the audio packet behind one stuffing byte
    q = pos + 6
    if rule == "start_code":
        s[3] = 0xBB
    elif rule.startswith("marker"):
        i, bit = [(4, 0x40), (4, 4), (6, 4), (8, 4), (9, 1), (12, 1)][int(rule[6])]
        s[i] ^= bit
    elif rule == "pes_start":
        s[pos + 2] = 2
    elif rule == "overrun":                    # the last packet (the filler) claims one byte more than the sector has
        p = pos + 6 + ((s[pos + 4] << 8) | s[pos + 5])
        plen = ((s[p + 4] << 8) | s[p + 5]) + 1
        s[p + 4], s[p + 5] = plen >> 8, plen & 0xFF
    elif rule == "plen_lt_7":
        s[pos + 4], s[pos + 5] = 0, 6
    elif rule == "plen_lt_pad1":
        s[q + 2] = 255
    elif rule == "codec":
        s[q + 3 + 1] ^= 1                      # 0xA0 <-> 0xA1
    elif rule == "pad2_lt_9":
        assert not mlp
        s[q + 6 + 1] = 8
    elif rule == "hdr_gt_plen":
        s[q + 6 + 1] = 255
    else:
        assert rule == "ninth"
    return bytes(s)


def rules_for(mlp):
    return tuple(r for r in RULES if not (mlp and r == "pad2_lt_9"))


# ------------------------------------------------------------------------------------------------ model
def walk(p, want_codec):
    """The audio payloads of one sector -> (None, [(offset, length)]) or (rule that rejects it, [])."""
    p = p.tobytes() if isinstance(p, np.ndarray) else bytes(p)
    if p[0:4] != b"\x00\x00\x01\xBA":                   # src/packet.c:173 sync_bytes
        return "start_code", []
    for i, ok in enumerate([(p[4] >> 6) == 1, p[4] & 4, p[6] & 4, p[8] & 4, p[9] & 1, (p[12] & 3) == 3]):
        if not ok:                                                 # src/packet.c:177-178 pad[0..5]
            return "marker%d" % i, []
    pos = 14 + (p[13] & 7)                                        # src/packet.c:169 stuffing_count skipped
    out = []
    while pos + 6 <= SECTOR:                                      # src/packet.c:97 "24u 8u 16u"
        sid, plen = p[pos + 3], (p[pos + 4] << 8) | p[pos + 5]
        if bytes(p[pos:pos + 3]) != b"\x00\x00\x01":              # src/packet.c:101
            return "pes_start", []
        if pos + 6 + plen > SECTOR:                               # src/packet.c:107 substream past the sector
            return "overrun", []
        if sid == 0xBD:                                           # src/packet.c:129 AUDIO_STREAM_ID
            q = pos + 6
            if plen < 7:                                          # src/dvd-audio.c:1245-1247: 3 + pad_1 + 4 bytes
                return "plen_lt_7", []
            pad1 = p[q + 2]                                       # src/dvd-audio.c:1245 "16p 8u"
            if plen < 7 + pad1:
                return "plen_lt_pad1", []
            codec, pad2 = p[q + 3 + pad1], p[q + 6 + pad1]        # src/dvd-audio.c:1247 "8u 8p 8p 8u"
            if codec != want_codec:                               # src/dvd-audio.c:1042, :1203
                return "codec", []
            if want_codec == 0xA0 and pad2 < 9:                   # src/dvd-audio.c:1058 skips pad_2 - 9
                return "pad2_lt_9", []
            if 7 + pad1 + pad2 > plen:                            # src/dvd-audio.c:1058, :1210 skip past the packet
                return "hdr_gt_plen", []
            if len(out) == MAX_AUDIO:                             # this project's limit (pcm_unswizzle.h MAX_PACKETS)
                return "ninth", []
            out.append((q + 7 + pad1 + pad2, plen - 7 - pad1 - pad2))
        pos += 6 + plen
    return None, out


_lib = None


def oracle():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(oracle_lib.build_oracle())
        L.pcm_oracle_decode_sectors.restype = ctypes.c_long
        L.pcm_oracle_decode_sectors.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint,
                                                ctypes.c_void_p, ctypes.c_size_t]
        L.wav_oracle_pack.restype = ctypes.c_long
        L.wav_oracle_pack.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_size_t,
                                      ctypes.c_uint, ctypes.c_void_p]
        _lib = L
    return _lib


class Model:
    """What a run of sectors holds: counts[s], base[s] (exclusive prefix sums, base[n] = the total), bad, reasons
    {sector: rule}, and pcm [ch, total] (raw PCM) or mlp bytes with packets [(first output byte, length, offset in
    its sector)] (demux)."""

    def __init__(self, counts, bad, reasons, pcm=None, mlp=None, packets=None):
        self.counts, self.bad, self.reasons = counts, bad, reasons
        self.base = np.concatenate([[0], np.cumsum(counts)])
        self.pcm, self.mlp, self.packets = pcm, mlp, packets


def model_pcm(data, bps, ch):
    data = np.ascontiguousarray(data, np.uint8).reshape(-1, SECTOR)
    n = len(data)
    cs = 2 * ch * (bps // 8)
    L = oracle()
    counts, reasons = np.zeros(n, np.int64), {}
    cap = 2 * (SECTOR // cs)
    one = np.zeros((ch, cap), np.int32)
    parts = []
    for s in range(n):
        why, pk = walk(data[s], 0xA0)
        r = L.pcm_oracle_decode_sectors(data[s].ctypes.data, 1, bps, ch, one.ctypes.data, cap)
        if why is not None:
            assert r == -1 or why == "ninth", (s, why, r)          # the oracle has no packet limit of its own
            reasons[s] = why
            continue
        assert r == sum(2 * (ln // cs) for _, ln in pk), (s, r, pk)
        counts[s] = r
        parts.append(one[:, :r].copy())
    pcm = np.concatenate(parts, axis=1) if parts else np.zeros((ch, 0), np.int32)
    return Model(counts, len(reasons), reasons, pcm=pcm)


def model_mlp(data):
    data = np.ascontiguousarray(data, np.uint8).reshape(-1, SECTOR)
    n = len(data)
    counts, reasons, packets = np.zeros(n, np.int64), {}, []
    parts, total = [], 0
    for s in range(n):
        why, pk = walk(data[s], 0xA1)
        if why is not None:
            reasons[s] = why
            continue
        for off, ln in pk:                                         # src/dvd-audio.c:1210-1215: payloads in order
            packets.append((total, ln, off))
            parts.append(data[s, off:off + ln])
            counts[s] += ln
            total += ln
    mlp = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return Model(counts, len(reasons), reasons, mlp=mlp, packets=packets)


def wav_payload(pcm, bits):
    """planar int32 [ch, frames] -> the bytes dvda2wav writes (wav_oracle_pack)"""
    pcm = np.ascontiguousarray(pcm, np.int32)
    ch, frames = pcm.shape
    out = np.zeros(ch * frames * 3 + 8, np.uint8)
    n = oracle().wav_oracle_pack(pcm.ctypes.data, frames, ch, max(frames, 1), bits, out.ctypes.data)
    return out[:n].copy()


# ------------------------------------------------------------------------------------------------ long runs
EDGES = (255, 256, 1023, 1024, 4095, 4096)
COUNTS = (1, 3, 4, 5, 4096, 4097, 5120, 5121)


def run_shift(index, n):
    """the rotation of the rules in the run of `n` sectors of parametrised case `index` (a layout, or a shift of the
    MLP test): chosen so that over the cases every rule comes to lie at every named position
    (tests/test_sector_model.py asserts it)"""
    return index + 4 * COUNTS.index(n)


def bad_plan(n, shift, rules):
    """[(sector, rule)] of a run of n sectors: a malformed sector first, in the middle, last, on both sides of the
    256-, 1024- and 4096-sector edges (255 | 256 ... lie side by side) and one every 317 sectors; the rules in turn,
    starting at rules[shift]"""
    named = [0 if n >= 3 else None, n // 2 if n >= 5 else None, n - 1 if n >= 4 else None]
    named += [p if p < n else None for p in EDGES]
    plan = {}
    for j, pos in enumerate(named):
        if pos is not None:
            plan.setdefault(pos, rules[(shift + j) % len(rules)])
    for k, pos in enumerate(range(150, n, 317)):
        plan.setdefault(pos, rules[(shift + len(named) + k) % len(rules)])
    return sorted(plan.items())


def roles(pos, n):
    """the named positions sector `pos` of a run of n holds"""
    r = {p for p in EDGES if p == pos}
    if pos == 0:
        r.add("first")
    if pos == n // 2 and n >= 5:
        r.add("middle")
    if pos == n - 1:
        r.add("last")
    return r


def salted_run(period, masks, n, plan, bad_sectors):
    """n sectors: `period` (list of sectors) repeated, every payload byte (masks[j]: the payload bytes of period
    member j) moved by a value per sector, so a sector written at a wrong base is seen; then sector pos becomes
    bad_sectors[rule] for every (pos, rule) of `plan`"""
    P = len(period)
    base = np.frombuffer(b"".join(period), np.uint8).reshape(P, SECTOR)
    data = base[np.arange(n) % P].copy()
    salt = ((np.arange(n) * 89 + 17) & 0xFF).astype(np.uint8)
    for j in range(P):
        rows = np.arange(j, n, P)
        cols = np.flatnonzero(masks[j])
        data[np.ix_(rows, cols)] += salt[rows, None]
    for pos, rule in plan:
        data[pos] = np.frombuffer(bad_sectors[rule], np.uint8)
    return data


def payload_mask(sector, want_codec):
    m = np.zeros(SECTOR, bool)
    why, pk = walk(sector, want_codec)
    assert why is None
    for off, ln in pk:
        m[off:off + ln] = True
    return m
