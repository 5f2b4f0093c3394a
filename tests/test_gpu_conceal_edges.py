"""dvda_mlp_hip_conceal_edges (Context.conceal_edges): the edges of a stream after a decode in conceal mode -- where its
kept bytes begin and end, the input timing at both ends, the sums for a caller's running mean and the FIR history behind
the last kept unit -- against tests/conceal_model.kept_ranges and a plain decode of the last kept range."""
import numpy as np
import pytest

from tests import conceal_model as cm
from tests.stream_tools import frame_offsets
from tests.test_conceal_model import make_stream

pytestmark = pytest.mark.gpu

FALSE_SYNC = 1 << 24


def defined(fir, S):
    """the entries of a FIR history [2][48] that a decode of these streams writes: row = substream, 8 taps per channel
    slot, slots numbered within the substream -- 6 channels in one substream, or channels 0-1 | 2-5 in two.  The rest of
    the workspace column is whatever the allocation held (dvda_mlp_hip_segment_fir hands that out as it is, and
    dvda_mlp_hip_set_initial_fir never reads it): not compared"""
    return fir[0, :48].copy() if S == 1 else np.concatenate([fir[0, :16], fir[1, :32]])


def last_segment_fir(hd, piece, zero_history):
    """FIR history [2][48] behind the last live segment of a plain decode of `piece` (with explicit zero history, as a
    fresh decoder behind damage starts, or with none at all)"""
    ctx = hd.Context(0, 1, 1024)
    try:
        if zero_history:
            hd.decode_streams_concealed([piece], init_fir=np.zeros((1, 2, 48), np.int32), ctx=ctx)
        else:
            hd.decode_streams([piece], ctx=ctx)
        live = [s for s in range(ctx.segment_count()) if not ctx.segment_info(s).status & FALSE_SYNC]
        return ctx.segment_fir(live[-1])
    finally:
        ctx.close()


def damaged(b, name):
    offs = frame_offsets(b)
    mid = lambda j: offs[j] + (offs[j + 1] - offs[j]) // 2           # noqa: E731
    d = b.copy()
    if name == "flip":              # ends kept: the last range runs to the stream's end
        d[mid(19)] ^= 0x10
    elif name == "tail":            # ends in damage: a TRAILING span
        d[mid(37):] = 0
    elif name == "lead_and_two":    # damage in the first unit and twice more
        d[offs[0] + 40:offs[0] + 200] ^= 0x5A
        d[mid(11)] ^= 0x10
        d[mid(35)] ^= 0x04
    return d


@pytest.mark.parametrize("feat", [0, "DISC|CHAINED"])
@pytest.mark.parametrize("S", [1, 2])
def test_edges_of_damaged_and_clean_streams_in_one_batch(pkg, oracle, S, feat):
    hd = pkg.hipdec
    b, frames, rpa = make_stream(pkg, S, feat, n_aus=48)
    clean = make_stream(pkg, S, feat, seed=12, n_aus=48)[0]
    names = ["flip", "tail", "lead_and_two"]
    streams = [damaged(b, n) for n in names] + [clean]
    batch = hd.Batch(streams)
    st = batch.current_stream
    ctx = hd.Context(0, len(streams), 1024)
    try:
        ctx.set_conceal(True)
        hd.decode_batch(ctx, batch, hd.PCM_PLANAR, attempts=3, capacity="report")
        infos = ctx.stream_info(stream=st)
        for i, (name, d) in enumerate(zip(names, streams)):
            R = cm.kept_ranges(d, 6, rpa, oracle)
            assert R, name
            e = ctx.conceal_edges(i, st)
            assert infos[i].status & hd.ST_CONCEALED, name
            assert (e["kept_begin"], e["kept_end"]) == (R[0][0], R[-1][1]), name
            assert (e["t_first"], e["t_end"]) == (R[0][3], R[-1][4]), name
            assert e["kept_bytes"] == sum(r[1] - r[0] for r in R) and e["kept_frames"] == sum(r[2] for r in R), name
            assert e["ends_kept"] == int(R[-1][1] == len(d)), name
            a_last = R[-1][0]
            want = last_segment_fir(hd, d[a_last:R[-1][1]], zero_history=True)
            assert np.array_equal(defined(e["fir"], S), defined(want, S)), name
        assert names[0] == "flip" and ctx.conceal_edges(0, st)["ends_kept"] == 1
        assert ctx.conceal_edges(1, st)["ends_kept"] == 0
        assert ctx.conceal_edges(2, st)["kept_begin"] > 0
        # the clean stream: all of it kept, the history of its last segment
        e = ctx.conceal_edges(3, st)
        assert infos[3].status & ~hd.ST_BENIGN == 0
        assert (e["kept_begin"], e["kept_end"], e["ends_kept"]) == (0, int(infos[3].bytes_consumed), 1)
        assert e["kept_bytes"] == len(clean) and e["kept_frames"] == int(infos[3].pcm_frames) == frames
        assert e["t_first"] == cm.au_timing(clean, 0) and e["t_end"] == (e["t_first"] + frames) & 0xFFFF
        assert np.array_equal(defined(e["fir"], S), defined(last_segment_fir(hd, clean, zero_history=False), S))
        if feat:
            assert defined(e["fir"], S).any(), "the history must matter for this test"
        # not after a decode with conceal mode off
        ctx.set_conceal(False)
        with pytest.raises(hd.HipError):
            ctx.conceal_edges(0, st)
        hd.decode_batch(ctx, batch, hd.PCM_PLANAR, attempts=3, capacity="report")
        with pytest.raises(hd.HipError):
            ctx.conceal_edges(3, st)
    finally:
        ctx.close()


def test_edges_of_a_clean_batch(pkg):
    """no damage anywhere: the decode launches nothing more, the edges are still there"""
    hd = pkg.hipdec
    kinds = [1 + (s & 1) for s in range(3)]
    streams = [make_stream(pkg, S, "CHAINED", seed=30 + s, n_aus=48)[0] for s, S in enumerate(kinds)]
    batch = hd.Batch(streams)
    st = batch.current_stream
    ctx = hd.Context(0, 3, 1024)
    try:
        ctx.set_conceal(True)
        hd.decode_batch(ctx, batch, hd.PCM_PLANAR, attempts=3, capacity="report")
        for i, s in enumerate(streams):
            e = ctx.conceal_edges(i, st)
            assert (e["kept_begin"], e["kept_end"], e["ends_kept"]) == (0, len(s), 1)
            got, want = defined(e["fir"], kinds[i]), defined(last_segment_fir(hd, s, zero_history=False), kinds[i])
            assert np.array_equal(got, want) and got.any()
    finally:
        ctx.close()
