"""dvda_mlp_hip_decode_async + dvda_mlp_hip_reserve: the non-blocking decode call (no host wait, no allocation) gives
what the blocking call gives when the reservation covers the batch, and says DVDA_ST_CAPACITY -- never short or wrong
PCM under a clean status -- when it does not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _decode(pkg, streams, reserve, lanes=0, layout=None):
    """index + decode_async on a fresh context with `reserve` = (pcm_frames, segments, seq_streams) or None"""
    hip = pkg.hipdec
    batch = hip.Batch(streams)
    layout = hip.PCM_PLANAR if layout is None else layout
    ctx = hip.Context(0, batch.n, max(64, batch.total // 64), lanes, layout)
    try:
        if reserve is not None:
            ctx.reserve(*reserve)
        pcm, infos, _ = hip.decode_batch(ctx, batch, layout, decode=hip.Context.decode_async)
        return pcm, infos
    finally:
        ctx.close()


@pytest.mark.parametrize("lanes", [0, 1, 64])
def test_regular_titles_need_no_reservation(pkg, oracle, lanes):
    syn, hip = pkg.synth, pkg.hipdec
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=40)
    streams = [syn.stream(cfg, 6100 + i) for i in range(6)]
    pcm, infos = _decode(pkg, [b for b, _ in streams], None, lanes=lanes, layout=hip.PCM_INTERLEAVED)
    for (b, f), got, inf in zip(streams, pcm, infos):
        want, r, st = oracle.decode(b, 6, f)
        assert st == 0 and inf.status == 0 and inf.pcm_frames == f and np.array_equal(got, want)


@pytest.mark.parametrize("S", [1, 2])
def test_chained_and_deferred_titles_on_reserved_workspaces(pkg, oracle, S):
    syn, hip = pkg.synth, pkg.hipdec
    SF = syn.SF
    cfgs = [syn.make_cfg(assignment=12, rate_code=1, n_substreams=S, n_aus=32, profile=1,
                         features=SF["CHAINED"] | SF["FIRRAND"], restart_interval=4),
            syn.make_cfg(assignment=12 if S == 2 else 1, rate_code=0, n_substreams=S, n_aus=24, profile=1,
                         features=SF["MIDMATRIX"] | SF["PARAMBLOCKS"] | SF["MATRIXRAND"] | SF["VARBLOCK"], restart_interval=3),
            syn.make_cfg(assignment=12, rate_code=2, n_substreams=S, n_aus=20, profile=1,
                         features=SF["VARROWS"] | SF["VARBLOCK"], restart_interval=5),
            syn.make_cfg(assignment=12, rate_code=1, n_substreams=S, n_aus=24)]
    streams = [syn.stream(c, 6200 + 10 * S + i) for i, c in enumerate(cfgs)]
    total_rows = sum(f for _, f in streams) + 4000
    for lanes in (S, 0):
        pcm, infos = _decode(pkg, [b for b, _ in streams], (total_rows, 64, 8), lanes=lanes)
        for (b, f), got, inf in zip(streams, pcm, infos):
            want, r, st = oracle.decode(b, 6 if got.shape[0] == 6 else got.shape[0], f)
            assert st == 0 and r == f
            if inf.status & hip.ST["OVERFLOW"]:
                continue            # (non-standard timing: the rows do not fit the standard-length buffer; reported)
            assert (inf.status & ~hip.ST_BENIGN) == 0 and inf.pcm_frames == f, hex(inf.status)
            assert np.array_equal(got, want)


def test_too_small_a_reservation_is_reported_not_decoded_short(pkg, oracle):
    syn, hip = pkg.synth, pkg.hipdec
    SF = syn.SF
    chained = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=32, profile=1,
                           features=SF["CHAINED"] | SF["FIRRAND"], restart_interval=4)
    plain = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=32)
    streams = [syn.stream(chained, 6301), syn.stream(plain, 6302), syn.stream(chained, 6303)]
    for reserve in (None, (80, 1, 0)):
        pcm, infos = _decode(pkg, [b for b, _ in streams], reserve, lanes=1)
        for k, ((b, f), got, inf) in enumerate(zip(streams, pcm, infos)):
            want, r, st = oracle.decode(b, 6, f)
            if k == 1:
                assert inf.status == 0 and np.array_equal(got, want)
            else:
                assert inf.status & hip.ST["CAPACITY"], hex(inf.status)
    # and the blocking call (which sizes its workspaces itself) decodes the same batch
    pcm, infos = hip.decode_streams([b for b, _ in streams], lanes_per_segment=1)
    for (b, f), got, inf in zip(streams, pcm, infos):
        want, r, st = oracle.decode(b, 6, f)
        assert (inf.status & ~hip.ST_BENIGN) == 0 and np.array_equal(got, want)
