"""Conceal mode on the GPU (dvda_mlp_hip_set_conceal): every damaged stream must equal the composed oracle expectation
of tests/conceal_model.py bit for bit, with its spans where the damage is; clean streams as without conceal mode."""
import ctypes

import numpy as np
import pytest

from tests import conceal_model as cm
from tests.stream_tools import frame_offsets, is_major_sync
from tests.test_conceal_model import make_stream, nocheck_flip

pytestmark = pytest.mark.gpu

KINDS = [(1, 0), (2, 0), (1, "CHAINED"), (2, "CHAINED"), (1, "DISC|CHAINED"), (2, "DISC|CHAINED")]
LAYOUTS = ["planar", "interleaved", "wav24"]


def _layout(hd, name):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24}[name]


def damaged_cases(b):
    """name -> damaged copy of b; positions from the undamaged stream's framing"""
    offs = frame_offsets(b)
    syncs = [o for o in offs if is_major_sync(b, o)]
    mid = lambda j: offs[j] + (offs[j + 1] - offs[j]) // 2           # noqa: E731
    out = {}
    d = b.copy()
    d[mid(19)] ^= 0x10
    out["flip"] = d
    d = b.copy()
    d[mid(13):mid(13) + 2048] = 0
    out["zero2048"] = d
    out["delete2048"] = np.concatenate([b[:mid(13)], b[mid(13) + 2048:]])
    d = b.copy()
    n = ((int(d[offs[21]]) & 0xF) << 8 | int(d[offs[21] + 1])) + 2   # unit 21 two words longer: 22 is damaged
    d[offs[21]] = (int(d[offs[21]]) & 0xF0) | (n >> 8)
    d[offs[21] + 1] = n & 0xFF
    out["length"] = d
    d = b.copy()
    d[syncs[0] + 40:syncs[0] + 200] ^= 0x5A         # the first major sync's unit: its payload, not its parameters
    out["lead"] = d
    d = b.copy()
    d[mid(37):] = 0
    out["tail"] = d
    d = b.copy()
    d[mid(11)] ^= 0x10
    d[mid(35)] ^= 0x04
    out["two"] = d
    return out


_EXPECT = {}


def expect(oracle, d):
    """the composed oracle expectation of damaged stream d (cached: the same streams go through three layouts)"""
    key = d.tobytes()
    if key not in _EXPECT:
        _EXPECT[key] = cm.conceal(d, 6, 80, oracle)
    return _EXPECT[key]


def check(hd, oracle, streams, layout, want_damage=True):
    pcm, infos, spans = hd.decode_streams_concealed(streams, device=0, layout=_layout(hd, layout))
    for i, (d, got, inf, sp) in enumerate(zip(streams, pcm, infos, spans)):
        want, want_sp = expect(oracle, d)
        if want_damage:
            assert want_sp, "case %d: the damage must show in the model" % i
        if layout == "wav24":
            want = np.frombuffer(oracle.wav_pack(want, 24), np.uint8)
        assert int(inf.pcm_frames) == (want.shape[-1] if layout != "wav24" else want.size // 18), i
        assert np.array_equal(got, want), "case %d differs from the composed oracle expectation" % i
        assert [s[:4] + (s[5] & 3,) for s in sp] == want_sp, i
        assert all(s[4] for s in sp), "every span names its cause"
        if want_sp:
            assert inf.status & hd.ST_CONCEALED and not inf.status & ~(hd.ST_BENIGN | hd.ST_CONCEALED), hex(inf.status)
        else:
            assert inf.status & ~hd.ST_BENIGN == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S,feat", KINDS)
def test_damaged_streams(pkg, oracle, S, feat, layout):
    b, frames, _ = make_stream(pkg, S, feat)
    cases = damaged_cases(b)
    check(pkg.hipdec, oracle, list(cases.values()), layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S,feat", KINDS)
def test_clean_batch_same_as_conceal_off(pkg, S, feat, layout):
    hd = pkg.hipdec
    streams = [make_stream(pkg, S, feat, seed=s)[0] for s in (3, 4, 5)]
    if layout == "wav24":
        off, ioff = hd.decode_streams_wav(streams, 24)
    else:
        off, ioff = hd.decode_streams(streams, layout=_layout(hd, layout))
    on, ion, spans = hd.decode_streams_concealed(streams, layout=_layout(hd, layout))
    assert spans == [[], [], []]
    for a, b_, x, y in zip(off, on, ioff, ion):
        assert np.array_equal(a, b_)
        assert (x.status, x.pcm_frames, x.mlp_frames) == (y.status, y.pcm_frames, y.mlp_frames)


@pytest.mark.parametrize("S", [1])
def test_nocheck_flip_conceals_segment(pkg, oracle, S):
    b, frames, _ = make_stream(pkg, S, "NOCHECK")
    d, j = nocheck_flip(b, frame_offsets(b), oracle, frames)
    check(pkg.hipdec, oracle, [d], "planar")


def test_gap_longer_than_65536_frames(pkg, oracle):
    b, frames, rpa = make_stream(pkg, 1, 0, n_aus=1200)
    offs = frame_offsets(b)
    lo, hi = offs[100] + 40, offs[1000] + 40           # 900 units' worth of unreadable bytes: 72 000 frames and more
    d = b.copy()
    d[lo:hi] = 0
    want, sp = cm.conceal(d, 6, rpa, oracle)
    assert sp[0][1] > 65536
    check(pkg.hipdec, oracle, [d], "planar")


def test_batch_of_256_few_damaged(pkg, oracle):
    hd = pkg.hipdec
    streams = [make_stream(pkg, 1 + (s & 1), 0, seed=100 + s, n_aus=24)[0] for s in range(256)]
    for k in (7, 100, 201):
        offs = frame_offsets(streams[k])
        streams[k] = streams[k].copy()
        streams[k][offs[12] + 40] ^= 0x08
    pcm, infos, spans = hd.decode_streams_concealed(streams)
    for i, (d, got, inf, sp) in enumerate(zip(streams, pcm, infos, spans)):
        want, want_sp = cm.conceal(d, 6, 80, oracle)
        assert bool(want_sp) == (i in (7, 100, 201))
        assert np.array_equal(got, want), i
        assert [s[:4] + (s[5] & 3,) for s in sp] == want_sp


def test_decode_async_refused_in_conceal_mode(pkg):
    import torch
    hd = pkg.hipdec
    b, _, _ = make_stream(pkg, 1, 0, n_aus=16)
    flat, offs, lens = hd.pack_streams([b])
    dev = torch.device("cuda", 0)
    ctx = hd.Context(0, 1, 64)
    try:
        assert hd.lib().dvda_mlp_hip_set_conceal(ctx._h, 1) == 0
        d_bytes = torch.from_numpy(flat).to(dev)
        d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.astype(np.int64)).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        ctx.index(d_bytes.data_ptr(), len(flat) - 64, d_off.data_ptr(), d_len.data_ptr(), 1, st)
        d_pcm = torch.zeros(6 * 16 * 80, dtype=torch.int32, device=dev)
        d_oo = torch.zeros(1, dtype=torch.int64, device=dev)
        d_os = torch.full((1,), 16 * 80, dtype=torch.int64, device=dev)
        rc = hd.lib().dvda_mlp_hip_decode_async(ctx._h, d_pcm.data_ptr(), d_oo.data_ptr(), d_os.data_ptr(), st)
        assert rc == -3                                 # DVDA_HIP_EINVAL
        n = ctypes.c_uint32(7)
        assert hd.lib().dvda_mlp_hip_conceal_spans(ctx._h, 0, None, 0, ctypes.byref(n), st) == 0 and n.value == 0
    finally:
        ctx.close()


def _segment_fir(hd, b, segment):
    """FIR history [2][48] at the end of `segment` of stream b, from a decode of the whole stream"""
    import torch
    ctx = hd.Context(0, 1, 1024)
    try:
        hd.decode_streams([b], ctx=ctx)
        fir = np.zeros((2, 48), np.int32)
        st = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
        hd._check(hd.lib().dvda_mlp_hip_segment_fir(ctx._h, segment, fir.ctypes.data, st), "segment_fir")
        return fir
    finally:
        ctx.close()


@pytest.mark.parametrize("S", [1, 2])
def test_initial_fir_carried_into_the_kept_range(pkg, oracle, S):
    # a stream cut at a major sync whose first block continues the FIR history, decoded with that history
    # (dvda_mlp_hip_set_initial_fir, as a window of a long track is): its kept range is the output without conceal mode
    hd = pkg.hipdec
    b, frames, rpa = make_stream(pkg, S, "DISC|CHAINED")
    offs = frame_offsets(b)
    syncs = [o for o in offs if is_major_sync(b, o)]
    cut = syncs[2]
    cut_frames = offs.index(cut) * rpa
    fir = _segment_fir(hd, b, 1)
    assert fir.any()
    tail = b[cut:].copy()
    t_offs = frame_offsets(tail)
    tail[t_offs[11] + (t_offs[12] - t_offs[11]) // 2] ^= 0x10
    pcm, infos, spans = hd.decode_streams_concealed([tail], init_fir=fir[None])
    want, want_sp = cm.conceal(tail, 6, rpa, oracle)
    a0, b0, f0 = cm.kept_ranges(tail, 6, rpa, oracle)[0][:3]
    assert a0 == 0
    carried = oracle.decode(np.concatenate([b[:cut], tail[:b0]]), 6, frames)[0][:, cut_frames:]
    assert carried.shape[1] == f0
    assert not np.array_equal(carried, want[:, :f0]), "the history must matter for this test"
    want[:, :f0] = carried
    assert np.array_equal(pcm[0], want)
    assert [s[:4] + (s[5] & 3,) for s in spans[0]] == want_sp


def test_second_decode_after_overflow_starts_from_the_index(pkg, oracle):
    # conceal mode reports a capacity that is too small (pcm_frames = what it needs); the same index decoded again --
    # conceal mode off -- reports what the plain decode reports, nothing of the concealed record
    import torch
    hd = pkg.hipdec
    b, frames, rpa = make_stream(pkg, 1, 0)
    d = damaged_cases(b)["delete2048"]
    want, _ = cm.conceal(d, 6, rpa, oracle)
    _, plain = hd.decode_streams([d])
    flat, offs, lens = hd.pack_streams([d])
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ctx = hd.Context(0, 1, 1024)
    try:
        d_bytes = torch.from_numpy(flat).to(dev)
        d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.astype(np.int64)).to(dev)
        ctx.index(d_bytes.data_ptr(), len(flat) - 64, d_off.data_ptr(), d_len.data_ptr(), 1, st)
        cap = want.shape[1] - 1
        d_pcm = torch.zeros(6 * cap, dtype=torch.int32, device=dev)
        d_oo = torch.zeros(1, dtype=torch.int64, device=dev)
        d_os = torch.full((1,), cap, dtype=torch.int64, device=dev)
        hd._check(hd.lib().dvda_mlp_hip_set_conceal(ctx._h, 1), "set_conceal")
        ctx.decode(d_pcm.data_ptr(), d_oo.data_ptr(), d_os.data_ptr(), st)
        inf = ctx.stream_info(stream=st)[0]
        assert inf.status & hd.ST_CONCEALED and inf.status & hd.ST["OVERFLOW"]
        assert int(inf.pcm_frames) == want.shape[1]
        hd._check(hd.lib().dvda_mlp_hip_set_conceal(ctx._h, 0), "set_conceal")
        ctx.decode(d_pcm.data_ptr(), d_oo.data_ptr(), d_os.data_ptr(), st)
        again = ctx.stream_info(stream=st)[0]
        ovf = hd.ST["OVERFLOW"]
        assert (again.status & ~ovf) == (plain[0].status & ~ovf) and not again.status & hd.ST_CONCEALED
        assert again.mlp_frames == plain[0].mlp_frames
    finally:
        ctx.close()
