"""The level report on the GPU (dvda_pcm_hip_levels, dvda_mlp_hip_pcm_levels; csrc/pcm_levels.h): what the device reports
of int32 PCM in either layout is tests/levels_model.levels of the same values.  Every comparison is exact."""
import numpy as np
import pytest

from tests import levels_model as lm
from tests import presentation_model as pm
from tests.stream_tools import frame_offsets, is_major_sync
from tests.test_conceal_model import make_stream as conceal_stream
from tests.test_presentation_model import make_stream

pytestmark = pytest.mark.gpu

T = lm.TILE
LAYOUTS = ["planar", "interleaved"]
FILL = np.array(0xA5A5A5A5, np.uint32).view(np.int32)[()]       # poison around every region: never part of a report


def _layout(hd, name):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24, "wav16": hd.PCM_WAV16}[name]


def mixed_pcm(rng, ch, frames, bits):
    """full int32 range with a block inside the nominal range: `over` is neither 0 nor everything"""
    pcm = rng.integers(-2 ** 31, 2 ** 31, (ch, frames), dtype=np.int64)
    a, b = frames // 4, frames - frames // 4
    pcm[:, a:b] = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (ch, b - a), dtype=np.int64)
    return pcm.astype(np.int32)


def place(pcms, layout, slack, off_mod=None, order=None):
    """lays the streams (planar int32 [ch, frames]) out in `layout` in one buffer filled with poison, stream i with
    capacity frames + slack[i] and at an offset = off_mod[i] (mod 4) int32 units; `order`: the sequence in which the
    streams lie in memory (the descriptors stay in the streams' order) -> (flat int32 array, desc list)"""
    parts, desc, pos = [np.full(5, FILL, np.int32)], [None] * len(pcms), 5
    for i in (order if order is not None else range(len(pcms))):
        p = pcms[i]
        ch, frames = p.shape
        stride = frames + slack[i % len(slack)]
        if off_mod is not None:
            pad = (off_mod[i % len(off_mod)] - pos) % 4
            parts.append(np.full(pad, FILL, np.int32))
            pos += pad
        if layout == "planar":
            region = np.full((ch, stride), FILL, np.int32)
            region[:, :frames] = p
        else:
            region = np.full((stride, ch), FILL, np.int32)
            region[:frames] = p.T
        desc[i] = (pos, stride, frames, ch)
        parts.append(region.reshape(-1))
        pos += region.size
    parts.append(np.full(7, FILL, np.int32))
    return np.concatenate(parts), desc


def run(hd, flat, layout, bits, desc, **kw):
    import torch
    d_pcm = torch.from_numpy(flat).to(torch.device("cuda", 0))
    return hd.levels_list(hd.pcm_levels(d_pcm, _layout(hd, layout), bits, desc, **kw))


def check(hd, pcms, layout, bits, slack, **kw):
    flat, desc = place(pcms, layout, slack, **kw)
    got = run(hd, flat, layout, bits, desc)
    want = [lm.levels(p, bits) for p in pcms]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, pcms[i].shape, desc[i])
    return desc


@pytest.mark.parametrize("ch", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("bits", [16, 20, 24])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sweep(pkg, layout, bits, ch):
    rng = np.random.default_rng(1000 * ch + bits + len(layout))
    frames = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]
    pcms = [mixed_pcm(rng, ch, f, bits) for f in frames]
    check(pkg.hipdec, pcms, layout, bits, slack=[0, 1, 2])
    big = lm.levels(pcms[-1], bits)
    assert all(0 < big["over"][c] < frames[-1] for c in range(ch))


@pytest.mark.parametrize("bits", [16, 20, 24])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rails(pkg, layout, bits):
    """exactly the values at and next to the rails of the nominal range and of int32, in chosen channels"""
    h = 1 << (bits - 1)
    rails = [-h - 1, -h, h - 1, h, -2 ** 31, 2 ** 31 - 1]
    pcms = []
    for frames in (6, T + 6):
        p = np.zeros((6, frames), np.int64)
        for c, v in enumerate(rails):
            p[c, :] = v                         # a channel that holds nothing but one rail
        pcms.append(p.astype(np.int32))
        q = np.zeros((3, frames), np.int64)
        q[1, -6:] = rails                       # every rail once, in the middle channel, at the stream's end
        q[2, 0] = -2 ** 31
        q[2, 1:] = 2 ** 31 - 1                  # a sum far beyond 32 bits
        pcms.append(q.astype(np.int32))
    check(pkg.hipdec, pcms, layout, bits, slack=[3])
    want = lm.levels(pcms[2], bits)
    assert want["over"][:6] == [T + 6, 0, 0, T + 6, T + 6, T + 6]
    assert want["sum"][5] == (T + 6) * (2 ** 31 - 1) and want["sum"][4] == -(T + 6) * 2 ** 31
    assert lm.levels(pcms[3], bits)["over"][:3] == [0, 4, T + 6]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_silence(pkg, layout):
    ch, frames = 3, 3 * T + 7
    pcms = [np.zeros((ch, frames), np.int32)]
    for at in (0, frames - 1, T - 1, T, frames // 2):
        p = np.zeros((ch, frames), np.int32)
        p[ch - 1, at] = -1                      # one non-zero value, in the last channel only
        pcms.append(p)
    p = mixed_pcm(np.random.default_rng(4), ch, frames, 24)
    p[:, :T + 5] = 0                            # silent for more than one whole tile at each end
    p[:, frames - T - 9:] = 0
    p[0, T + 5] = 1
    p[1, frames - T - 10] = 1
    pcms.append(p)
    pcms.append(np.zeros((1, 1), np.int32))
    check(pkg.hipdec, pcms, layout, 24, slack=[2])
    want = lm.levels(pcms[-2], 24)
    assert (want["lead_silent"], want["trail_silent"]) == (T + 5, T + 9)
    assert [lm.levels(q, 24)["lead_silent"] for q in pcms[:6]] == [frames, 0, frames - 1, T - 1, T, frames // 2]


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_alignment_and_order(pkg, layout, bits):
    """off at every residue mod 4 int32 units, an odd planar stride, descriptors in no order of off, poison in the slack"""
    rng = np.random.default_rng(77 + bits)
    chans = [2, 3, 6, 1, 5, 2, 3, 1, 6, 4, 8, 7]
    frames = [3 * T + 7, 5, 0, T + 1, 2, T - 1, 10000, 2 * T, 3, T + 2, 700, 2 * T + 3]
    pcms = [mixed_pcm(rng, c, f, bits) for c, f in zip(chans, frames)]
    slack = [37 + (f & 1) for f in frames] if layout == "planar" else [37]         # planar: every stride is odd
    order = [7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4]
    desc = check(pkg.hipdec, pcms, layout, bits, slack=slack, off_mod=[0, 1, 2, 3, 3, 2, 1, 0, 1, 3, 2, 0], order=order)
    assert {d[0] % 4 for d in desc} == {0, 1, 2, 3} and all(d[1] > d[2] for d in desc)
    assert [d[0] for d in desc] != sorted(d[0] for d in desc)
    if layout == "planar":
        assert all(d[1] & 1 for d in desc)


@pytest.mark.parametrize("layout,bits", [("planar", 24), ("interleaved", 16)])
def test_many_streams(pkg, layout, bits):
    """more streams than one block of the plan kernel, more tiles than the tile kernel has workgroups"""
    rng = np.random.default_rng(300 + bits)
    pcms = []
    for i in range(300):
        ch = int(rng.choice([1, 1, 1, 1, 2, 2, 3, 4, 5, 6]))
        # (the long ones have few channels: many tiles in few bytes)
        frames = 0 if i % 37 == 5 else int(rng.integers(0, (22 if ch <= 2 else 3) * T + 1))
        p = mixed_pcm(rng, ch, frames, bits)
        if i % 5 == 0:
            p[:, :frames // 3] = 0
        pcms.append(p)
    assert sum(-(-p.shape[1] // T) for p in pcms) > 2048
    check(pkg.hipdec, pcms, layout, bits, slack=[0, 3])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_long_stream(pkg, layout):
    """one more tile than a join workgroup has threads"""
    frames = 256 * T + 1
    pcms = [mixed_pcm(np.random.default_rng(5), 1, frames, 20), mixed_pcm(np.random.default_rng(6), 2, 9, 20)]
    pcms[0][:, :T + 1] = 0
    pcms[0][:, -3:] = 0
    assert -(-frames // T) == 257 and frames * 4 < 8 << 20
    check(pkg.hipdec, pcms, layout, 20, slack=[5])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_poisoned_workspace(pkg, layout):
    import torch
    hd = pkg.hipdec
    rng = np.random.default_rng(9)
    pcms = [mixed_pcm(rng, c, f, 24) for c, f in ((2, 9000), (6, 0), (3, 17), (1, 30000))]
    flat, desc = place(pcms, layout, slack=[1])
    total = sum(p.shape[1] for p in pcms)
    work = torch.empty(hd.pcm_levels_workspace_words(len(desc), total), dtype=torch.int32, device="cuda:0")
    work.fill_(-1)                      # 0xFF bytes
    first = run(hd, flat, layout, 24, desc, work=work)
    work.fill_(0)
    second = run(hd, flat, layout, 24, desc, work=work)
    assert first == second == [lm.levels(p, 24) for p in pcms]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bound_too_small_reads_nothing_wrong(pkg, layout):
    """a stream whose tiles fall outside max_total_frames is reported as zeros; the streams inside it are right"""
    hd = pkg.hipdec
    rng = np.random.default_rng(10)
    pcms = [mixed_pcm(rng, 2, T, 16), mixed_pcm(rng, 2, 4 * T, 16), mixed_pcm(rng, 1, 5, 16)]    # 1, 4 and 1 tiles
    flat, desc = place(pcms, layout, slack=[0])
    got = run(hd, flat, layout, 16, desc, max_total_frames=T)                   # room for 1 + 3 tiles
    assert got == [lm.levels(pcms[0], 16), lm.zero(), lm.zero()]


@pytest.mark.parametrize("layout", ["wav24", "wav16"])
def test_wav_layouts_are_refused(pkg, oracle, layout):
    import torch
    hd = pkg.hipdec
    d_pcm = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.pcm_levels(d_pcm, _layout(hd, layout), 24 if layout == "wav24" else 16, [(0, 8, 8, 1)])
    b, _ = oracle_pcm(pkg, oracle, 0, 0)
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.decode_streams([b], layout=_layout(hd, layout), levels=24)


_ORACLE = {}


def oracle_pcm(pkg, oracle, feat, seed):
    if (feat, seed) not in _ORACLE:
        b, frames = make_stream(pkg, feat, seed)
        want, r, st = oracle.decode(b, 6, frames)
        assert st == 0 and r == frames
        _ORACLE[(feat, seed)] = (b, want)
    return _ORACLE[(feat, seed)]


@pytest.mark.parametrize("bits", [16, 20, 24])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("feat", [0, "CHAINED", "DISC|CHAINED"])
def test_after_a_decode(pkg, oracle, feat, layout, bits):
    hd = pkg.hipdec
    cases = [oracle_pcm(pkg, oracle, feat, seed) for seed in (0, 1, 2)]
    pcm, infos, reports = hd.decode_streams([b for b, _ in cases], layout=_layout(hd, layout), levels=bits)
    for (b, want), got, inf, rep in zip(cases, pcm, infos, reports):
        assert inf.status & ~hd.ST_BENIGN == 0 and np.array_equal(got, want)
        assert rep == lm.levels(want, bits)
    # ... beside the digest: both appended, the digest first
    res = hd.decode_streams([cases[0][0]], layout=_layout(hd, layout), crc32=True, crc_bits=24, levels=bits)
    assert len(res) == 4 and res[3] == [lm.levels(cases[0][1], bits)] and len(res[2][0]) == 2


def test_default_return_shape_is_unchanged(pkg, oracle):
    hd = pkg.hipdec
    b, _ = oracle_pcm(pkg, oracle, 0, 0)
    assert len(hd.decode_streams([b], levels=None)) == 2 and len(hd.decode_streams([b], crc32=True, levels=None)) == 3
    assert len(hd.decode_streams_concealed([b], levels=None)) == 3
    assert len(hd.decode_streams([b], levels=24)) == 3 and len(hd.decode_streams_concealed([b], levels=24)) == 4


def test_presentation(pkg, oracle):
    hd = pkg.hipdec
    streams = [make_stream(pkg, "CHAINED", seed)[0] for seed in (0, 1, 2)]
    pcm, infos, reports = hd.decode_streams(streams, presentation=hd.PRESENT_SUBSTREAM0, levels=24)
    for b, inf, rep in zip(streams, infos, reports):
        want, frames, ost, k = pm.expect(b, oracle)
        assert ost == 0 and int(inf.channels) == k == 2 and int(inf.pcm_frames) == frames
        assert rep == lm.levels(want, 24)
        assert rep["min"][2:] == [0] * 6 and rep["sum"][2:] == [0] * 6


@pytest.mark.parametrize("layout", LAYOUTS)
def test_conceal_mode(pkg, oracle, layout):
    """the report of what conceal mode handed out: the concealed gap is in it as exact zeros.  A stream damaged in its
    first unit has a leading span; the rule gives a leading span no frames of silence (tests/conceal_model.py: the
    stream starts with the first range that is kept), so lead_silent is at least that span's frames and otherwise what
    the kept PCM opens with."""
    hd = pkg.hipdec
    b, _, _ = conceal_stream(pkg, 2, "CHAINED")
    offs = frame_offsets(b)
    syncs = [o for o in offs if is_major_sync(b, o)]
    mid = b.copy()
    mid[offs[19] + (offs[20] - offs[19]) // 2] ^= 0x10
    head = b.copy()
    head[syncs[0] + 40:syncs[0] + 200] ^= 0x5A
    pcm, infos, spans, reports = hd.decode_streams_concealed([mid, head, b], layout=_layout(hd, layout), levels=24)
    assert infos[0].status & hd.ST_CONCEALED and infos[1].status & hd.ST_CONCEALED and not spans[2]
    for p, inf, rep in zip(pcm, infos, reports):
        assert p.shape == (int(inf.channels), int(inf.pcm_frames)) and p.shape[1] > 0
        assert rep == lm.levels(p, 24)
    # the gap inside stream 0: zeros in every channel, and they are in the figures
    first, frames = spans[0][0][0], spans[0][0][1]
    assert frames > 0 and not pcm[0][:, first:first + frames].any()
    assert reports[0]["sum"][:6] == [int(pcm[0][c].astype(np.int64).sum()) for c in range(6)]
    assert all(reports[0]["min"][c] <= 0 <= reports[0]["max"][c] for c in range(6))
    assert spans[1][0][0] == 0 and spans[1][0][5] & hd.CONCEAL_LEADING
    assert reports[1]["lead_silent"] >= spans[1][0][1]


def test_overflow_reports_zeros(pkg, oracle):
    """a stream given too small a capacity carries DVDA_ST_OVERFLOW: zeros; the stream beside it is reported"""
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
        assert ctx.pcm_levels(*out.ptrs, 24, stream=st) == [lm.zero(), lm.levels(cases[1][1], 24)]
        ctx.set_pcm_layout(hd.PCM_WAV24)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_levels(*out.ptrs, 24, stream=st)
    finally:
        ctx.close()
