"""DVDA_PRESENT_SUBSTREAM0 on the GPU (dvda_mlp_hip_set_presentation): a two-substream stream decodes to the k-channel
presentation substream 0 carries, bit for bit what tests/presentation_model.py makes of it with the CPU oracle; a
one-substream stream, and every stream under DVDA_PRESENT_FULL, decodes as it always did."""
import numpy as np
import pytest

from tests import presentation_model as pm
from tests.stream_tools import frame_offsets, is_major_sync
from tests.test_presentation_model import make_stream, ss1_flip

pytestmark = pytest.mark.gpu

KINDS = [0, "CHAINED", "DISC|CHAINED", "SYNCONLY|CHAINED", "IIR|QSS", "CHECKQUIRK|EXTRAWORD"]
LAYOUTS = ["planar", "interleaved", "wav24"]
EINVAL = -3


def _layout(hd, name):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24}[name]


def check(pkg, oracle, streams, layout="planar", lanes=0, nch=None, clean=True):
    """decodes `streams` as one batch under DVDA_PRESENT_SUBSTREAM0 and holds every one against the model"""
    hd = pkg.hipdec
    if layout == "wav24":
        got, infos = hd.decode_streams_wav(streams, 24, lanes_per_segment=lanes, presentation=hd.PRESENT_SUBSTREAM0)
    else:
        got, infos = hd.decode_streams(streams, layout=_layout(hd, layout), lanes_per_segment=lanes,
                                       presentation=hd.PRESENT_SUBSTREAM0)
    for i, (b, g, inf) in enumerate(zip(streams, got, infos)):
        want, frames, ost, k = pm.expect(b, oracle, nch[i] if nch else None)
        if clean:
            assert ost == 0, "case %d: the model must decode clean" % i
        assert int(inf.channels) == k, i
        assert inf.status & ~hd.ST_BENIGN == 0, "case %d: status %#x" % (i, inf.status)
        assert int(inf.pcm_frames) == frames and int(inf.mlp_frames) == len(frame_offsets(b)), i
        assert int(inf.bytes_consumed) == pm.consumed(b), i
        assert int(inf.substreams) == pm.substreams_of(b) and int(inf.assignment) == int(b[11]) & 0x1F, i
        if layout == "wav24":
            want = np.frombuffer(oracle.wav_pack(want, 24), np.uint8)
        assert g.shape == want.shape and np.array_equal(g, want), "case %d differs from the model" % i
    return got, infos


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("feat", KINDS)
def test_kinds_and_layouts(pkg, oracle, feat, layout):
    streams = [make_stream(pkg, feat, seed)[0] for seed in (0, 1, 2)]
    check(pkg, oracle, streams, layout)


@pytest.mark.parametrize("feat", ["CHAINED", "DISC|CHAINED", 0])
def test_forced_lane_kernels(pkg, oracle, feat):
    streams = [make_stream(pkg, feat, seed)[0] for seed in (0, 1, 2)]
    check(pkg, oracle, streams, lanes=3)


@pytest.mark.parametrize("form", [1, 2])
def test_chain_forms(pkg, oracle, form):
    hd = pkg.hipdec
    hd.CHAIN_FORM = form
    try:
        streams = [make_stream(pkg, "CHAINED", seed)[0] for seed in (0, 1, 2)]
        check(pkg, oracle, streams)
        check(pkg, oracle, streams, lanes=3)
    finally:
        hd.CHAIN_FORM = 0


def _manual(pkg, streams, presentation=1, use_async=False, reserve=None, init_fir=None, after=None, lanes=0):
    """index + decode on a context of the test's own; after(ctx, stream) runs before the context closes"""
    import torch
    hd = pkg.hipdec
    batch = hd.Batch(streams)
    ctx = hd.Context(0, batch.n, max(64, batch.total // 64), lanes)
    try:
        ctx.set_presentation(presentation)
        if reserve is not None:
            ctx.reserve(*reserve)
        d_fir = None
        if init_fir is not None:
            d_fir = torch.from_numpy(np.ascontiguousarray(init_fir, np.int32).reshape(batch.n, 2, 48)).to(batch.dev)
            ctx.set_initial_fir(d_fir.data_ptr())
        pcm, infos, _ = hd.decode_batch(ctx, batch, hd.PCM_PLANAR, decode=hd.Context.decode_async if use_async else hd.Context.decode)
        extra = after(ctx, batch.current_stream) if after else None
        return pcm, infos, extra
    finally:
        ctx.close()


def test_decode_async_after_reserve(pkg, oracle):
    hd = pkg.hipdec
    streams = [make_stream(pkg, "CHAINED", seed) for seed in (0, 1, 2)]
    rows = sum(f for _, f in streams) + 4000
    for lanes in (3, 0):
        pcm, infos, _ = _manual(pkg, [b for b, _ in streams], use_async=True, reserve=(rows, 64, 8), lanes=lanes)
        for (b, f), got, inf in zip(streams, pcm, infos):
            want, frames, ost, k = pm.expect(b, oracle)
            assert ost == 0 and inf.status & ~hd.ST_BENIGN == 0 and int(inf.pcm_frames) == frames
            assert np.array_equal(got, want)


def test_fuzz_profile(pkg, oracle):
    streams = [make_stream(pkg, "SF_ALL", seed)[0] for seed in (0, 1, 2)]
    check(pkg, oracle, streams)
    check(pkg, oracle, streams, lanes=3)


def test_mixed_batch(pkg, oracle):
    hd, syn = pkg.hipdec, pkg.synth
    streams = [make_stream(pkg, "CHAINED", 5, 12, S=1)[0], make_stream(pkg, 0, 6, 1, S=1)[0]]
    nch = [6, 2]
    for j, (asg, ss0) in enumerate([(12, 1), (12, 2), (20, 3), (12, 5), (6, 2), (20, 5), (6, 1), (6, 3)]):
        streams.append(make_stream(pkg, ["CHAINED", 0, "DISC|CHAINED"][j % 3], 10 + j, asg, ss0)[0])
        nch.append(None)
        assert pm.expect(streams[-1], oracle)[3] == ss0
    for layout in ("planar", "interleaved"):
        got, _ = check(pkg, oracle, streams, layout, nch=nch)
        plain, _ = hd.decode_streams(streams[:2], layout=_layout(hd, layout))
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    check(pkg, oracle, streams, lanes=3, nch=nch)


def test_damage_in_substream_1_does_not_reach_the_presentation(pkg, oracle):
    hd = pkg.hipdec
    b, _ = make_stream(pkg, "CHAINED", 0)
    d = ss1_flip(b, 19, 1)
    _, full = hd.decode_streams([d])
    assert full[0].status & ~hd.ST_BENIGN, "the full decode must see the damage"
    got, _ = check(pkg, oracle, [d])
    assert np.array_equal(got[0], pm.expect(b, oracle)[0])


def test_damage_in_substream_0_is_reported(pkg, oracle):
    hd = pkg.hipdec
    b, _ = make_stream(pkg, "CHAINED", 0)
    d = ss1_flip(b, 19, 0)
    assert pm.expect(d, oracle)[2] != 0
    _, infos = hd.decode_streams([d], presentation=hd.PRESENT_SUBSTREAM0)
    assert infos[0].status & ~hd.ST_BENIGN, hex(infos[0].status)


def test_default_mode_is_untouched(pkg):
    hd = pkg.hipdec
    streams = [make_stream(pkg, "CHAINED", 0)[0], make_stream(pkg, 0, 1, S=1)[0]]
    want, winf = hd.decode_streams(streams)
    ctx = hd.Context(0, len(streams), 4096)
    try:
        ctx.set_presentation(hd.PRESENT_SUBSTREAM0)
        ctx.set_presentation(hd.PRESENT_FULL)
        got, ginf = hd.decode_streams(streams, ctx=ctx)
    finally:
        ctx.close()
    fields = [f for f, _ in hd.StreamInfo._fields_]
    for a, b, x, y in zip(want, got, winf, ginf):
        assert np.array_equal(a, b)
        assert [getattr(x, f) for f in fields] == [getattr(y, f) for f in fields]
    L = hd.lib()
    ctx = hd.Context(0, 1, 64)
    try:
        assert L.dvda_mlp_hip_set_presentation(ctx._h, 7) == EINVAL
        assert L.dvda_mlp_hip_set_conceal(ctx._h, 1) == 0
        assert L.dvda_mlp_hip_set_presentation(ctx._h, hd.PRESENT_SUBSTREAM0) == EINVAL
        assert L.dvda_mlp_hip_set_presentation(ctx._h, hd.PRESENT_FULL) == 0
    finally:
        ctx.close()
    ctx = hd.Context(0, 1, 64)
    try:
        assert L.dvda_mlp_hip_set_presentation(ctx._h, hd.PRESENT_SUBSTREAM0) == 0
        assert L.dvda_mlp_hip_set_conceal(ctx._h, 1) == EINVAL
        assert L.dvda_mlp_hip_set_conceal(ctx._h, 0) == 0
    finally:
        ctx.close()


def _segments(ctx, st):
    return [ctx.segment_info(j, st) for j in range(ctx.segment_count(st))]


def test_segment_info_speaks_of_the_source_buffer(pkg, oracle):
    hd = pkg.hipdec
    b, _ = make_stream(pkg, "DISC|CHAINED", 1)
    syncs = [o for o in frame_offsets(b) if is_major_sync(b, o)]
    _, infos, segs = _manual(pkg, [b], after=_segments)
    live = [s for s in segs if not s.status & hd.ST["FALSE_SYNC"]]
    assert len(live) == len(syncs) and int(infos[0].segments) >= len(live)
    offs = [int(s.offset) for s in live]
    assert offs[0] == 0 and offs == sorted(set(offs)) and set(offs) <= set(syncs)
    assert int(live[-1].end) <= len(b) and all(int(s.end) > int(s.offset) for s in live)
    assert [int(s.end) for s in live[:-1]] == offs[1:]


def test_history_carried_across_a_cut(pkg, oracle):
    hd = pkg.hipdec
    b, _ = make_stream(pkg, "CHAINED", 2)
    want, frames, ost, k = pm.expect(b, oracle)
    assert ost == 0

    def fourth_and_fir(ctx, st):
        segs = [(j, s) for j, s in enumerate(_segments(ctx, st)) if not s.status & hd.ST["FALSE_SYNC"]]
        return int(segs[3][1].offset), segs

    _, _, (cut, _) = _manual(pkg, [b], after=fourth_and_fir)
    assert cut in frame_offsets(b) and is_major_sync(b, cut)

    def last_fir(ctx, st):
        segs = [j for j, s in enumerate(_segments(ctx, st)) if not s.status & hd.ST["FALSE_SYNC"]]
        return ctx.segment_fir(segs[-1], st)

    head, hinf, fir = _manual(pkg, [b[:cut]], after=last_fir)
    assert fir[0].any(), "the history must matter for this test"
    tail, tinf, _ = _manual(pkg, [b[cut:]], init_fir=fir[None])
    fresh, _, _ = _manual(pkg, [b[cut:]])
    assert not np.array_equal(fresh[0], tail[0])
    for inf in (hinf[0], tinf[0]):
        assert inf.status & ~hd.ST_BENIGN == 0 and int(inf.channels) == k
    assert np.array_equal(np.concatenate([head[0], tail[0]], axis=1), want)
