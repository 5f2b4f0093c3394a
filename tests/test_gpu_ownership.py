"""What a context owns, on the GPU: every workspace, event and child context is a member that frees itself
(csrc/hip_ws.h, csrc/mlp_ctx.h).  The two mistakes such ownership can make:

  * something is not freed with the context -- contexts that have used every mode (the presentation's inner context,
    conceal mode's second context and the buffers it grows) are made and destroyed in a row, and the device's free
    memory must not go down by as much as ONE context in seven rounds;
  * something is freed, or kept, when a buffer grows under a context that goes on being used -- a small batch, a large
    one with a chained title (the byte-proportional workspaces, the presentation buffer and the chain workspaces all
    reallocate), the small one again, on one context and stream.

Every decode is held bit for bit against what the other GPU tests hold it against: the oracle, tests/conceal_model.py,
tests/presentation_model.py."""
import numpy as np
import pytest

from tests import conceal_model as cm
from tests import presentation_model as pm
from tests.test_conceal_model import make_stream as conceal_stream
from tests.test_gpu_conceal import damaged_cases
from tests.test_presentation_model import make_stream as present_stream

pytestmark = pytest.mark.gpu


def _full(oracle, b, frames):
    want, r, st = oracle.decode(b, 6, frames)
    assert st == 0 and r == frames
    return want


def _check_full(hd, oracle, ctx, streams, frames, cache):
    pcm, infos = hd.decode_streams(streams, ctx=ctx, presentation=hd.PRESENT_FULL)
    for i, (b, f, got, inf) in enumerate(zip(streams, frames, pcm, infos)):
        key = ("full", b.tobytes())
        if key not in cache:
            cache[key] = _full(oracle, b, f)
        assert inf.status & ~hd.ST_BENIGN == 0 and int(inf.pcm_frames) == f, "stream %d: status %#x" % (i, inf.status)
        assert np.array_equal(got, cache[key]), "stream %d differs from the oracle" % i


def _check_presentation(hd, oracle, ctx, streams):
    pcm, infos = hd.decode_streams(streams, ctx=ctx, presentation=hd.PRESENT_SUBSTREAM0)
    for i, (b, got, inf) in enumerate(zip(streams, pcm, infos)):
        want, frames, ost, k = pm.expect(b, oracle, 6)      # (cached there; 6: what assignment 12 means for one substream)
        assert ost == 0 and int(inf.channels) == k and inf.status & ~hd.ST_BENIGN == 0, "stream %d: status %#x" % (i, inf.status)
        assert int(inf.pcm_frames) == frames
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d differs from the presentation model" % i


def _check_concealed(hd, oracle, ctx, streams, cache):
    pcm, infos, spans = hd.decode_streams_concealed(streams, ctx=ctx)
    damaged = 0
    for i, (b, got, inf, sp) in enumerate(zip(streams, pcm, infos, spans)):
        key = ("conceal", b.tobytes())
        if key not in cache:
            cache[key] = cm.conceal(b, 6, 80, oracle)
        want, want_sp = cache[key]
        assert int(inf.pcm_frames) == want.shape[1] and np.array_equal(got, want), \
            "stream %d differs from the composed oracle expectation" % i
        assert [s[:4] + (s[5] & 3,) for s in sp] == want_sp, i
        if want_sp:
            damaged += 1
            assert inf.status & hd.ST_CONCEALED and not inf.status & ~(hd.ST_BENIGN | hd.ST_CONCEALED), hex(inf.status)
        else:
            assert inf.status & ~hd.ST_BENIGN == 0
    return damaged


def test_contexts_that_used_every_mode_leave_nothing_behind(pkg, oracle):
    import torch
    hd, syn = pkg.hipdec, pkg.synth
    # two one-substream titles and two two-substream ones, as smoke() decodes
    streams, frames = [], []
    for seed in range(1, 5):
        b, f = syn.stream(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1 + (seed & 1), n_aus=32), seed)
        streams.append(b)
        frames.append(f)
    hurt = streams[:3] + [damaged_cases(conceal_stream(pkg, 1, 0)[0])["flip"]]
    cache = {}
    # One context's footprint: free memory before create minus free memory after it.  A context of this size is made of
    # buffers far smaller than the blocks the runtime takes device memory in, and it hands freed pieces of such blocks
    # out again: one create alone can read as nothing, or as a whole block.  So FOOTPRINT_OVER contexts are created
    # and held together and the drop is divided by their number -- the same measure, with that many times less of the
    # block size in it, and never more than the true footprint plus 1/FOOTPRINT_OVER of a block.
    FOOTPRINT_OVER = 32
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    held, drops = [], []
    try:
        for _ in range(FOOTPRINT_OVER):
            held.append(hd.Context(0, 64, 256))
            drops.append(before - torch.cuda.mem_get_info(0)[0])
    finally:
        for ctx in held:
            ctx.close()
    print("free memory taken after each of %d creates: %s" % (FOOTPRINT_OVER, drops))
    footprint = drops[-1] // FOOTPRINT_OVER
    free_at = {}
    for cycle in range(1, 9):
        torch.cuda.synchronize()
        ctx = hd.Context(0, 64, 256)
        try:
            _check_full(hd, oracle, ctx, streams, frames, cache)
            _check_presentation(hd, oracle, ctx, streams)        # (makes the inner context)
            assert _check_concealed(hd, oracle, ctx, hurt, cache) == 1  # (makes conceal mode's context and buffers)
        finally:
            ctx.close()
        torch.cuda.synchronize()
        free_at[cycle] = torch.cuda.mem_get_info(0)[0]
    print("context footprint %d bytes; free memory after cycle 1: %d, after cycle 8: %d (difference %d)"
          % (footprint, free_at[1], free_at[8], free_at[1] - free_at[8]))
    assert footprint > 0, "the measure needs a context that takes device memory"
    # (a buffer or child context leaked per cycle costs seven times its size between the two readings)
    assert abs(free_at[1] - free_at[8]) < footprint


@pytest.mark.parametrize("mode", ["full", "substream0"])
def test_small_large_small_on_one_context(pkg, oracle, mode):
    hd = pkg.hipdec

    def batch(n, n_aus, seed0):
        made = [present_stream(pkg, 0, seed0 + s, S=1 + (s & 1), n_aus=n_aus) for s in range(n)]
        return [b for b, _ in made], [f for _, f in made]

    a_streams, a_frames = batch(2, 8, 0)
    b_streams, b_frames = batch(8, 64, 10)
    # ... and a chained title in the large batch: the chain workspaces grow from nothing under a used context
    for S in (1, 2):
        b, f = present_stream(pkg, "CHAINED", 20 + S, S=S, n_aus=64)
        b_streams.append(b)
        b_frames.append(f)
    total_b = sum((len(b) + 15) & ~15 for b in b_streams)
    assert total_b > 8 * sum((len(b) + 15) & ~15 for b in a_streams), "the large batch must outgrow the small one's workspaces"
    cache = {}
    ctx = hd.Context(0, 16, max(64, total_b // 64))
    try:
        for streams, frames in ((a_streams, a_frames), (b_streams, b_frames), (a_streams, a_frames)):
            if mode == "full":
                _check_full(hd, oracle, ctx, streams, frames, cache)
            else:
                _check_presentation(hd, oracle, ctx, streams)
        chained = hd.decode_streams(b_streams[-2:], ctx=ctx, presentation=hd.PRESENT_FULL)[1]
        # (the generator chains at a restart point or not, by its random taps: one title that does is enough)
        assert any(inf.status & hd.ST["CHAINED"] for inf in chained), "the large batch must go through the chain passes"
    finally:
        ctx.close()
