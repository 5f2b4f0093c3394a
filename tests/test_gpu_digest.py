"""The PCM digest on the GPU (dvda_pcm_hip_crc32, dvda_mlp_hip_pcm_crc32; csrc/pcm_digest.h): the CRC-32 the device
computes from PCM in any of the four layouts is zlib.crc32 of the WAV payload the oracle packs from the same values.
Every comparison is exact."""
import zlib

import numpy as np
import pytest

from tests import presentation_model as pm
from tests.stream_tools import frame_offsets
from tests.test_conceal_model import make_stream as conceal_stream
from tests.test_presentation_model import make_stream

pytestmark = pytest.mark.gpu

COMBOS = [("planar", 24), ("planar", 16), ("interleaved", 24), ("interleaved", 16), ("wav24", 24), ("wav16", 16)]
FILL = np.array(0xA5A5A5A5, np.uint32).view(np.int32)[()]


def _layout(hd, name):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24, "wav16": hd.PCM_WAV16}[name]


def random_pcm(rng, ch, frames):
    """full int32 range: write_signed's truncation is part of what is tested"""
    return rng.integers(-2 ** 31, 2 ** 31, (ch, frames), dtype=np.int64).astype(np.int32)


def place(oracle, pcms, layout, bits, slack, off_mod=None):
    """lays the streams (planar int32 [ch, frames]) out in `layout` in one buffer filled with 0xA5, stream i with
    capacity frames + slack[i] and at an offset = off_mod[i] (mod 4) int32 units
    -> (flat int32 array, desc list, expected [(crc, bytes)])"""
    nb = bits // 8
    parts, desc, want, pos = [], [], [], 0
    for i, p in enumerate(pcms):
        ch, frames = p.shape
        stride = frames + slack[i % len(slack)]
        if off_mod is not None:
            pad = (off_mod[i % len(off_mod)] - pos) % 4
            parts.append(np.full(pad, FILL, np.int32))
            pos += pad
        payload = oracle.wav_pack(p, bits)
        assert len(payload) == frames * ch * nb
        if layout.startswith("wav"):
            region = np.full((stride * ch * nb + 3) // 4, FILL, np.int32)
            region.view(np.uint8)[:len(payload)] = np.frombuffer(payload, np.uint8)
        elif layout == "planar":
            region = np.full((ch, stride), FILL, np.int32)
            region[:, :frames] = p
            region = region.reshape(-1)
        else:
            region = np.full((stride, ch), FILL, np.int32)
            region[:frames] = p.T
            region = region.reshape(-1)
        desc.append((pos, stride, frames, ch))
        want.append((zlib.crc32(payload) if payload else 0, len(payload)))
        parts.append(region)
        pos += len(region)
    parts.append(np.full(4, FILL, np.int32))
    return np.concatenate(parts), desc, want


def run(hd, flat, layout, bits, desc, **kw):
    import torch
    d_pcm = torch.from_numpy(flat).to(torch.device("cuda", 0))
    return hd.crc_list(*hd.pcm_crc32(d_pcm, _layout(hd, layout), bits, desc, **kw))


def edge_frames(hd, ch, nb):
    """0, 1, 2, 3, 5; the counts around one tile of payload; 3 tiles + 7 frames"""
    spf, tile = ch * nb, hd.CRC_TILE_BYTES
    lo, hi = tile // spf, -(-tile // spf)
    return sorted({0, 1, 2, 3, 5, lo - 1, lo, hi, hi + 1, 3 * tile // spf + 7})


@pytest.mark.parametrize("ch", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("layout,bits", COMBOS)
def test_sweep(pkg, oracle, layout, bits, ch):
    hd = pkg.hipdec
    rng = np.random.default_rng(1000 * ch + bits + len(layout))
    frames = edge_frames(hd, ch, bits // 8)
    if ch == 1 and bits == 16:      # (a tile of payload less one sample, exactly, plus one sample)
        assert {hd.CRC_TILE_BYTES // 2 - 1, hd.CRC_TILE_BYTES // 2, hd.CRC_TILE_BYTES // 2 + 1} <= set(frames)
    pcms = [random_pcm(rng, ch, f) for f in frames]
    flat, desc, want = place(oracle, pcms, layout, bits, slack=[0, 1, 2])
    got = run(hd, flat, layout, bits, desc)
    for f, g, w in zip(frames, got, want):
        print(layout, bits, ch, f, "%08x %d" % g, "%08x %d" % w)
    assert got == want


@pytest.mark.parametrize("layout,bits", COMBOS)
def test_alignment_and_order(pkg, oracle, layout, bits):
    """streams at off = 0, 1, 2, 3 (mod 4) int32 units in one call, lengths in no order, capacity beyond `frames`
    filled with 0xA5"""
    hd = pkg.hipdec
    rng = np.random.default_rng(77 + bits)
    tile = hd.CRC_TILE_BYTES
    chans = [2, 3, 6, 1, 5, 2, 3, 1]
    nbytes = [3 * tile + 7, 5, 0, tile + 1, 2, tile - 1, 40000, 2 * tile]
    pcms = [random_pcm(rng, c, b // (c * (bits // 8))) for c, b in zip(chans, nbytes)]
    flat, desc, want = place(oracle, pcms, layout, bits, slack=[37], off_mod=[0, 1, 2, 3, 3, 2, 1, 0])
    assert sorted(d[0] % 4 for d in desc) == [0, 0, 1, 1, 2, 2, 3, 3] and all(d[1] > d[2] for d in desc)
    assert run(hd, flat, layout, bits, desc) == want


@pytest.mark.parametrize("layout,bits", [("planar", 24), ("interleaved", 16), ("wav24", 24), ("wav16", 16)])
def test_many_streams(pkg, oracle, layout, bits):
    hd = pkg.hipdec
    rng = np.random.default_rng(300 + bits)
    pcms = []
    for _ in range(300):
        ch = int(rng.integers(1, 7))
        pcms.append(random_pcm(rng, ch, int(rng.integers(0, 3 * hd.CRC_TILE_BYTES + 1)) // (ch * (bits // 8))))
    flat, desc, want = place(oracle, pcms, layout, bits, slack=[0, 3])
    assert run(hd, flat, layout, bits, desc) == want


@pytest.mark.parametrize("layout,bits", [("planar", 24), ("interleaved", 16), ("wav24", 24), ("wav16", 16)])
def test_long_stream(pkg, oracle, layout, bits):
    """one more tile than a join workgroup folds in one turn of its loop"""
    hd = pkg.hipdec
    ch = 2
    spf = ch * (bits // 8)
    frames = hd.CRC_JOIN_TILES * hd.CRC_TILE_BYTES // spf + 1
    assert -(-frames * spf // hd.CRC_TILE_BYTES) == hd.CRC_JOIN_TILES + 1 and frames * spf <= 128 << 20
    pcms = [random_pcm(np.random.default_rng(5), ch, frames), random_pcm(np.random.default_rng(6), 1, 9)]
    flat, desc, want = place(oracle, pcms, layout, bits, slack=[5])
    assert run(hd, flat, layout, bits, desc) == want


def test_poisoned_workspace(pkg, oracle):
    import torch
    hd = pkg.hipdec
    rng = np.random.default_rng(9)
    pcms = [random_pcm(rng, c, f) for c, f in ((2, 9000), (6, 0), (3, 17), (1, 30000))]
    flat, desc, want = place(oracle, pcms, "interleaved", 24, slack=[1])
    total = sum(w[1] for w in want)
    work = torch.full((hd.pcm_crc32_workspace_words(len(desc), total),), -1, dtype=torch.int32, device="cuda:0")
    first = run(hd, flat, "interleaved", 24, desc, work=work)
    work.fill_(-1)
    second = run(hd, flat, "interleaved", 24, desc, work=work)
    assert first == second == want


def test_bound_too_small_reads_nothing_wrong(pkg, oracle):
    """a stream whose tiles fall outside max_total_bytes is reported as (0, 0); the streams inside it are right"""
    hd = pkg.hipdec
    rng = np.random.default_rng(10)
    tile = hd.CRC_TILE_BYTES
    pcms = [random_pcm(rng, 1, tile // 2), random_pcm(rng, 1, 4 * tile // 2)]       # 1 tile, 4 tiles at 16 bits
    flat, desc, want = place(oracle, pcms, "planar", 16, slack=[0])
    got = run(hd, flat, "planar", 16, desc, max_total_bytes=tile)                   # room for 1 + 2 tiles
    assert got == [want[0], (0, 0)]


_ORACLE = {}


def oracle_pcm(pkg, oracle, feat, seed):
    if (feat, seed) not in _ORACLE:
        b, frames = make_stream(pkg, feat, seed)
        want, r, st = oracle.decode(b, 6, frames)
        assert st == 0 and r == frames
        _ORACLE[(feat, seed)] = (b, want)
    return _ORACLE[(feat, seed)]


@pytest.mark.parametrize("layout,bits", COMBOS)
@pytest.mark.parametrize("feat", [0, "CHAINED", "DISC|CHAINED"])
def test_after_a_decode(pkg, oracle, feat, layout, bits):
    hd = pkg.hipdec
    cases = [oracle_pcm(pkg, oracle, feat, seed) for seed in (0, 1, 2)]
    streams = [b for b, _ in cases]
    if layout.startswith("wav"):
        _, infos, digests = hd.decode_streams_wav(streams, bits, crc32=True)
    else:
        _, infos, digests = hd.decode_streams(streams, layout=_layout(hd, layout), crc32=True, crc_bits=bits)
    for (b, want), inf, dg in zip(cases, infos, digests):
        assert inf.status & ~hd.ST_BENIGN == 0
        payload = oracle.wav_pack(want, bits)
        assert dg == (zlib.crc32(payload), len(payload))


def test_default_return_shape_is_unchanged(pkg, oracle):
    hd = pkg.hipdec
    b, _ = oracle_pcm(pkg, oracle, 0, 0)
    assert len(hd.decode_streams([b])) == 2 and len(hd.decode_streams_wav([b], 24)) == 2
    assert len(hd.decode_streams_concealed([b])) == 3


def test_presentation(pkg, oracle):
    hd = pkg.hipdec
    streams = [make_stream(pkg, "CHAINED", seed)[0] for seed in (0, 1, 2)]
    pcm, infos, digests = hd.decode_streams(streams, presentation=hd.PRESENT_SUBSTREAM0, crc32=True, crc_bits=24)
    for b, inf, dg in zip(streams, infos, digests):
        want, frames, ost, k = pm.expect(b, oracle)
        assert ost == 0 and int(inf.channels) == k == 2 and int(inf.pcm_frames) == frames
        payload = oracle.wav_pack(want, 24)
        assert dg == (zlib.crc32(payload), len(payload))


@pytest.mark.parametrize("layout,bits", [("planar", 24), ("wav24", 24)])
def test_conceal_mode(pkg, oracle, layout, bits):
    """the digest of what conceal mode handed out (this tests the digest, not the concealment)"""
    hd = pkg.hipdec
    b, _, _ = conceal_stream(pkg, 2, "CHAINED")
    d = b.copy()
    offs = frame_offsets(b)
    d[offs[19] + (offs[20] - offs[19]) // 2] ^= 0x10
    pcm, infos, spans, digests = hd.decode_streams_concealed([d, b], layout=_layout(hd, layout), crc32=True, crc_bits=bits)
    assert infos[0].status & hd.ST_CONCEALED and spans[0] and not spans[1]
    for p, inf, dg in zip(pcm, infos, digests):
        payload = p.tobytes() if layout.startswith("wav") else oracle.wav_pack(p, bits)
        assert len(payload) == int(inf.pcm_frames) * int(inf.channels) * (bits // 8) > 0
        assert dg == (zlib.crc32(payload), len(payload))


def test_overflow_reports_nothing(pkg, oracle):
    """a stream given too small a capacity carries DVDA_ST_OVERFLOW: (0, 0); the stream beside it is digested"""
    hd = pkg.hipdec
    cases = [oracle_pcm(pkg, oracle, 0, seed) for seed in (0, 1)]
    batch = hd.Batch([b for b, _ in cases])
    st = batch.current_stream
    ctx = hd.Context(0, batch.n, max(64, batch.total // 64))
    try:
        ctx.index_batch(batch, st)
        rows = [hd.standard_rows(i) for i in ctx.stream_info(stream=st)]
        rows[0] //= 2                                       # too small for stream 0
        out = hd.PcmRegions(rows, [6, 6], slack=4)
        ctx.decode(*out.ptrs, st)
        infos = ctx.stream_info(stream=st)
        assert infos[0].status & hd.ST["OVERFLOW"] and not infos[1].status & ~hd.ST_BENIGN
        got = ctx.pcm_crc32(*out.ptrs, 24, stream=st)
        payload = oracle.wav_pack(cases[1][1], 24)
        assert got == [(0, 0), (zlib.crc32(payload), len(payload))]
    finally:
        ctx.close()
