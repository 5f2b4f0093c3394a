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
    hd = pkg.hipdec
    b, _, _ = make_stream(pkg, 1, 0, n_aus=16)
    batch = hd.Batch([b])
    st = batch.current_stream
    ctx = hd.Context(0, 1, 64)
    try:
        ctx.set_conceal(True)
        ctx.index_batch(batch, st)
        out = hd.PcmRegions([16 * 80], [6])
        rc = hd.lib().dvda_mlp_hip_decode_async(ctx._h, *out.ptrs, st)      # (the raw return code is what is asserted)
        assert rc == -3                                 # DVDA_HIP_EINVAL
        n = ctypes.c_uint32(7)
        assert hd.lib().dvda_mlp_hip_conceal_spans(ctx._h, 0, None, 0, ctypes.byref(n), st) == 0 and n.value == 0
    finally:
        ctx.close()


def _segment_fir(hd, b, segment):
    """FIR history [2][48] at the end of `segment` of stream b, from a decode of the whole stream"""
    ctx = hd.Context(0, 1, 1024)
    try:
        hd.decode_streams([b], ctx=ctx)
        return ctx.segment_fir(segment)
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
    hd = pkg.hipdec
    b, frames, rpa = make_stream(pkg, 1, 0)
    d = damaged_cases(b)["delete2048"]
    want, _ = cm.conceal(d, 6, rpa, oracle)
    _, plain = hd.decode_streams([d])
    batch = hd.Batch([d])
    st = batch.current_stream
    ctx = hd.Context(0, 1, 1024)
    try:
        ctx.index_batch(batch, st)
        out = hd.PcmRegions([want.shape[1] - 1], [6])
        ctx.set_conceal(True)
        ctx.decode(*out.ptrs, st)
        inf = ctx.stream_info(stream=st)[0]
        assert inf.status & hd.ST_CONCEALED and inf.status & hd.ST["OVERFLOW"]
        assert int(inf.pcm_frames) == want.shape[1]
        ctx.set_conceal(False)
        ctx.decode(*out.ptrs, st)
        again = ctx.stream_info(stream=st)[0]
        ovf = hd.ST["OVERFLOW"]
        assert (again.status & ~ovf) == (plain[0].status & ~ovf) and not again.status & hd.ST_CONCEALED
        assert again.mlp_frames == plain[0].mlp_frames
    finally:
        ctx.close()


def _three_streams(pkg):
    """three 6-channel 96 kHz one-substream streams of 16 access units, one byte flipped in the middle of a unit of the second"""
    streams = [make_stream(pkg, 1, 0, seed=40 + s, n_aus=16)[0] for s in range(3)]
    offs = frame_offsets(streams[1])
    streams[1] = streams[1].copy()
    streams[1][offs[11] + (offs[12] - offs[11]) // 2] ^= 0x10
    return streams


def test_conceal_on_a_context_that_was_used_for_something_else(pkg, oracle):
    """after a presentation decode on the same context: the result of a context of its own, and conceal mode off again"""
    hd = pkg.hipdec
    streams = _three_streams(pkg)
    want_pcm, want_infos, want_spans = hd.decode_streams_concealed(streams)
    ctx = hd.Context(0, 3, 64)
    try:
        hd.decode_streams(streams, ctx=ctx, presentation=hd.PRESENT_SUBSTREAM0)
        pcm, infos, spans = hd.decode_streams_concealed(streams, ctx=ctx)
        for got, want in zip(pcm, want_pcm):
            assert got.shape == want.shape and np.array_equal(got, want)
        assert [(int(i.pcm_frames), int(i.status)) for i in infos] == [(int(i.pcm_frames), int(i.status)) for i in want_infos]
        assert spans == want_spans and spans[1] and not spans[0] and not spans[2]
        assert infos[1].status & hd.ST_CONCEALED
        plain, pinf = hd.decode_streams(streams, ctx=ctx)
        assert pinf[1].status & ~(hd.ST_BENIGN | hd.ST_CONCEALED) and not pinf[1].status & hd.ST_CONCEALED, hex(pinf[1].status)
        for k in (0, 2):
            ref, r, st = oracle.decode(streams[k], 6, 16 * 80)
            assert st == 0 and pinf[k].status & ~hd.ST_BENIGN == 0 and infos[k].status & ~hd.ST_BENIGN == 0
            assert np.array_equal(plain[k], ref) and np.array_equal(pcm[k], ref)
    finally:
        ctx.close()


def test_conceal_on_too_small_a_context_raises_and_leaves_conceal_off(pkg):
    hd = pkg.hipdec
    streams = _three_streams(pkg)
    syncs = sum(1 for b in streams for o in frame_offsets(b) if is_major_sync(b, o))
    ctx = hd.Context(0, 3, syncs - 2)               # holds the first two streams' major syncs, not the third's
    try:
        with pytest.raises(hd.HipError):
            hd.decode_streams_concealed(streams, ctx=ctx)
        # off again: the presentation, which a context in conceal mode refuses, can be chosen ...
        ctx.set_presentation(hd.PRESENT_SUBSTREAM0)
        ctx.set_presentation(hd.PRESENT_FULL)
        # ... and the damaged stream alone, which the context holds, is reported and not concealed
        _, infos = hd.decode_streams(streams[1:2], ctx=ctx)
        assert infos[0].status & ~(hd.ST_BENIGN | hd.ST_CONCEALED) and not infos[0].status & hd.ST_CONCEALED, hex(infos[0].status)
    finally:
        ctx.close()
