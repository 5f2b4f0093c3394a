"""The channel mix behind a decode (dvda_mlp_hip_pcm_mix, hipdec.decode_streams_downmixed; csrc/pcm_report_run.h): what
comes out is the oracle's decode through tests/mix_model, a stream that already has the channels asked for comes back
untouched, an overflowed stream reports zeros, and the mix between the other seven passes on one context leaves their
results as they are.  Every comparison is exact."""
import numpy as np
import pytest

from tests import mix_model as mm
from tests.test_gpu_reports_together import AU, _decode, _seven_passes

pytestmark = pytest.mark.gpu

TITLES = [(12, 6, 60), (9, 5, 7), (7, 3, 52), (1, 2, 9)]      # (channel assignment, its channels, access units)
_CASES = {}


def cases(pkg, oracle):
    """the synthetic one-substream titles and the oracle's decode of each, made once"""
    if not _CASES:
        syn = pkg.synth
        for k, (a, ch, n) in enumerate(TITLES):
            b, frames = syn.stream(syn.make_cfg(assignment=a, rate_code=1, n_substreams=1, n_aus=n), 60 + k)
            want, r, st = oracle.decode(b, ch, frames)
            assert st == 0 and r == frames == n * AU and want.shape == (ch, frames)
            _CASES[a] = (b, want)
    return [_CASES[a] for a, _, _ in TITLES]


@pytest.mark.parametrize("och,flags", [(2, mm.NORMALIZED), (1, mm.NORMALIZED), (2, mm.NORMALIZED | mm.LFE), (1, mm.UNITY | mm.LFE)])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_downmixed_is_the_oracle_through_the_model(pkg, oracle, layout, och, flags):
    hd = pkg.hipdec
    lay = {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED}[layout]
    got = cases(pkg, oracle)
    if flags & mm.UNITY:
        # the weights as they are: 5.1 and 5.0 to mono sum above 2^31 in a row; judged before anything is mixed
        with pytest.raises(ValueError, match="2\\^31"):
            hd.decode_streams_downmixed([b for b, _ in got], och, flags, layout=lay)
        got = got[2:]
    pcm, infos, reports = hd.decode_streams_downmixed([b for b, _ in got], och, flags, layout=lay)
    for (b, want), p, inf, rep in zip(got, pcm, infos, reports):
        assert inf.status & ~hd.ST_BENIGN == 0 and int(inf.channels) == want.shape[0]
        if want.shape[0] == och:
            assert rep is None and np.array_equal(p, want)          # handed out as it is
            continue
        m = mm.default_matrix(mm.speaker_mask(int(inf.assignment)), och, flags)
        out, cl = mm.mix_np(want, m, 24)
        assert p.shape == (och, want.shape[1]) and np.array_equal(p, out)
        assert rep == mm.report(want.shape[1], cl)
        assert flags & mm.UNITY or cl == [0] * 8


def test_the_callers_matrices(pkg, oracle):
    """a matrix per stream where the caller has one -- a 2-channel stream too -- and the default elsewhere"""
    hd = pkg.hipdec
    got = cases(pkg, oracle)
    mats = [mm.random_matrix(np.random.default_rng(4), 6, 2), None, None, mm.matrix(2, 2, [[0, mm.ONE], [mm.ONE, 0]])]
    pcm, infos, reports = hd.decode_streams_downmixed([b for b, _ in got], 2, matrices=mats)
    for (b, want), p, inf, rep, m in zip(got, pcm, infos, reports, mats):
        m = m or mm.default_matrix(mm.speaker_mask(int(inf.assignment)), 2)
        out, cl = mm.mix_np(want, m, 24)
        assert np.array_equal(p, out) and rep == mm.report(want.shape[1], cl)
    assert np.array_equal(pcm[3], got[3][1][::-1])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_overflow_and_mismatch_report_zeros(pkg, oracle, layout):
    """a stream that carries DVDA_ST_OVERFLOW, and one whose matrix says other input channels, write nothing"""
    import torch
    hd = pkg.hipdec
    lay = {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED}[layout]
    got = cases(pkg, oracle)[:3]
    batch = hd.Batch([b for b, _ in got])
    st = batch.current_stream
    ctx = hd.Context(0, batch.n, 4096, 0, lay)
    try:
        ctx.index_batch(batch, st)
        infos = ctx.stream_info(stream=st)
        rows = [hd.standard_rows(i) for i in infos]
        rows[0] //= 2                                       # too small for stream 0
        out = hd.PcmRegions(rows, [6, 5, 3], lay, slack=4)
        ctx.decode(*out.ptrs, st)
        infos = ctx.stream_info(stream=st)
        assert infos[0].status & hd.ST["OVERFLOW"] and not infos[2].status & ~hd.ST_BENIGN
        mats = [mm.default_matrix(mm.speaker_mask(a), 2) for a in (12, 12, 7)]     # (stream 1 has 5 channels, not 6)
        frames = [int(i.pcm_frames) for i in infos]
        off = [0, 2 * frames[0], 2 * frames[0] + 2 * frames[1]]
        d_out = torch.full((off[2] + 2 * frames[2] + 8,), 0x5A5A5A5A, dtype=torch.int32, device=out.dev)
        d_off = torch.tensor(off, dtype=torch.int64, device=out.dev)
        d_stride = torch.tensor(frames, dtype=torch.int64, device=out.dev)
        rep = ctx.pcm_mix(*out.ptrs, d_out.data_ptr(), d_off.data_ptr(), d_stride.data_ptr(), mats, 24, stream=st)
        want, cl = mm.mix_np(got[2][1], mats[2], 24)
        assert rep == [mm.NOT_TAKEN, mm.NOT_TAKEN, mm.report(frames[2], cl)]
        host = d_out.cpu().numpy()
        assert (host[:off[2]] == 0x5A5A5A5A).all() and (host[off[2] + 2 * frames[2]:] == 0x5A5A5A5A).all()
        part = host[off[2]:off[2] + 2 * frames[2]]
        assert np.array_equal(part.reshape(2, -1) if layout == "planar" else part.reshape(-1, 2).T, want)
        ctx.set_pcm_layout(hd.PCM_WAV24)
        with pytest.raises(hd.HipError, match="EINVAL"):
            ctx.pcm_mix(*out.ptrs, d_out.data_ptr(), d_off.data_ptr(), d_stride.data_ptr(), mats, 24, stream=st)
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_the_mix_between_the_other_seven_passes(pkg, layout):
    """the eight passes share one staging path and one result block: the mix comes out the same before and after another
    pass has used them, and the other seven behind it come out as they do alone"""
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    lay = {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED}[layout]
    streams = [syn.stream(syn.make_cfg(assignment=a, rate_code=1, n_substreams=1, n_aus=n), 40 + i)[0]
               for i, (a, n) in enumerate([(1, 1), (1, 60), (12, 60)])]
    mats = [mm.matrix(2, 1, [[mm.HALF, mm.HALF]]), mm.matrix(2, 2, [[0, mm.ONE], [mm.ONE, 0]]),
            mm.matrix(6, 2, [[mm.ONE, 0, mm.HALF, 0, mm.HALF, 0], [0, mm.ONE, mm.HALF, 0, 0, -mm.HALF]])]
    ctx = hd.Context(0, 3, 4096, 0, lay)
    try:
        out, st, pcm = _decode(hd, ctx, streams, lay)
        infos = ctx.stream_info(stream=st)
        want = [mm.mix_np(p, m, 24) for p, m in zip(pcm, mats)]
        frames = [p.shape[1] for p in pcm]
        off = [3, 3 + frames[0] + 2, 3 + frames[0] + 2 + 2 * frames[1] + 3]
        words = off[2] + 2 * frames[2] + 5
        d_off = torch.tensor(off, dtype=torch.int64, device=out.dev)
        d_stride = torch.tensor(frames, dtype=torch.int64, device=out.dev)

        def mixed():
            d_out = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=out.dev)
            rep = ctx.pcm_mix(*out.ptrs, d_out.data_ptr(), d_off.data_ptr(), d_stride.data_ptr(), mats, 24, stream=st)
            assert rep == [mm.report(f, cl) for f, (_, cl) in zip(frames, want)]
            got = hd.cut_regions(d_out.cpu().numpy(), off, frames, [1, 2, 2], frames, lay)
            assert all(np.array_equal(g, w) for g, (w, _) in zip(got, want))
            return d_out.cpu().numpy()

        first = mixed()
        assert ctx.pcm_levels(*out.ptrs, 24, stream=st)[2]["frames"] == frames[2]
        assert np.array_equal(mixed(), first)
        _seven_passes(hd, ctx, out, st, pcm, infos)     # (ends with the PCM requantized to 16 bits in place)
    finally:
        ctx.close()
