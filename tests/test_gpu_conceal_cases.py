"""Conceal mode on the GPU at its edges (csrc/mlp_conceal.h, csrc/mlp_conceal_run.h): every case of
tests/conceal_cases.py through hipdec.decode_streams_concealed against tests/conceal_model.py with the library's limits
(a plan's 16 ranges, the 4 decode rounds), bit for bit -- PCM or WAV payload, pcm_frames, mlp_frames, the spans with their
flags, the status -- in the four layouts and with the lane settings that send the ranges through the other fast passes;
then batches that mix every shape, a caller's context used for few, many and few ranges again, and what the move and fill
kernels must leave alone.  tests/test_conceal_cases_model.py holds the premises of every case on the CPU.

PCM_WAV16: the generator's bps_code only labels a stream (its values stay 24 bits wide), so the 16-bit payload is taken of
the 24-bit streams, against the same packer (oracle.wav_pack(.., 16)) that states what the library's 16-bit payload is."""
import numpy as np
import pytest

from tests import conceal_cases as cc
from tests import conceal_model as cm

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
LAYOUTS = ("planar", "interleaved", "wav24", "wav16")
# group -> the (layout, lanes_per_segment) it runs with: every case planar x {0, 3} and a WAV layout; the plan / round
# edges and the round-2 cases with all three lane settings (3: the lane kernels only, 64: the cooperative kernel only)
CONFIGS = {
    "edge": [("planar", 0), ("planar", 3), ("planar", 64), ("wav16", 0), ("interleaved", 3)],
    "round2": [("planar", 0), ("planar", 3), ("planar", 64), ("wav24", 3), ("interleaved", 64)],
    "shapes": [("planar", 0), ("planar", 3), ("interleaved", 0), ("wav24", 0), ("wav16", 3), ("wav24", 64)],
}


def _layout(hd, name):
    return {"planar": hd.PCM_PLANAR, "interleaved": hd.PCM_INTERLEAVED, "wav24": hd.PCM_WAV24, "wav16": hd.PCM_WAV16}[name]


def names_of(group):
    return [n for n, c in cc.CASES.items() if c.group == group]


def compare(pkg, oracle, names, result, layout):
    """the library's result for the cases `names` (in that order) against the limited model"""
    hd, syn = pkg.hipdec, pkg.synth
    pcm, infos, spans = result
    assert len(pcm) == len(names)
    for name, got, inf, sp in zip(names, pcm, infos, spans):
        c = cc.CASES[name]
        s = cc.stream(syn, c.recipe)
        want, want_sp = cc.expect(syn, oracle, name)
        frames = want.shape[1]
        if layout in ("wav24", "wav16"):
            want = np.frombuffer(oracle.wav_pack(want, int(layout[3:])), np.uint8)
            assert want.size == frames * s.nch * int(layout[3:]) // 8
        assert int(inf.pcm_frames) == frames, name
        if frames:
            assert got.shape == want.shape, name
            assert np.array_equal(got, want), "%s differs from the model" % name
        else:
            assert got.size == 0, name                  # (no major sync: the stream has no channel count either)
        assert int(inf.mlp_frames) == cc.kept_units(syn, oracle, name), name
        assert [x[:4] + (x[5] & 7,) for x in sp] == want_sp, name
        assert all(x[5] & ~7 == 0 for x in sp), name
        if c.claim.get("clean"):
            assert sp == [] and inf.status & ~hd.ST_BENIGN == 0, name
        else:
            assert want_sp and all(x[4] for x in sp), "%s: every span names its cause" % name
            assert inf.status & hd.ST_CONCEALED and not inf.status & ~(hd.ST_BENIGN | hd.ST_CONCEALED), (name, hex(inf.status))


def run(pkg, oracle, names, layout, lanes, ctx=None):
    hd = pkg.hipdec
    streams = [cc.damaged(pkg.synth, oracle, n) for n in names]
    return hd.decode_streams_concealed(streams, device=0, layout=_layout(hd, layout), lanes_per_segment=lanes, ctx=ctx)


@pytest.mark.parametrize("group,layout,lanes", [(g, lay, ln) for g in cc.GROUPS for lay, ln in CONFIGS[g]])
def test_cases_equal_the_limited_model(pkg, oracle, group, layout, lanes):
    names = names_of(group)
    compare(pkg, oracle, names, run(pkg, oracle, names, layout, lanes), layout)


def test_every_case_runs_with_the_settings_it_must():
    """the table and CONFIGS together: no case is left out of a setting the file is there for"""
    assert sorted(n for g in cc.GROUPS for n in names_of(g)) == sorted(cc.CASES)
    for g in cc.GROUPS:
        have = set(CONFIGS[g])
        assert {("planar", 0), ("planar", 3)} <= have and any(lay.startswith("wav") for lay, _ in have), g
    for g in ("edge", "round2"):
        assert {ln for _, ln in CONFIGS[g]} == {0, 3, 64}
    assert {lay for g in cc.GROUPS for lay, _ in CONFIGS[g]} == set(LAYOUTS)


@pytest.mark.parametrize("layout", ["planar", "wav24"])
def test_clean_streams_as_without_conceal_mode(pkg, oracle, layout):
    hd = pkg.hipdec
    names = [n for n, c in cc.CASES.items() if c.claim.get("clean")]
    streams = [cc.damaged(pkg.synth, oracle, n) for n in names]
    off, ioff = hd.decode_streams_wav(streams, 24) if layout == "wav24" else hd.decode_streams(streams)
    on, ion, spans = hd.decode_streams_concealed(streams, layout=_layout(hd, layout))
    assert spans == [[] for _ in names]
    for a, b, x, y in zip(off, on, ioff, ion):
        assert np.array_equal(a, b)
        assert (x.status, x.pcm_frames, x.mlp_frames) == (y.status, y.pcm_frames, y.mlp_frames)


MANY = ("edge14", "edge15", "edge16", "edge17", "edge30")      # round 1: 15 + 4 * 16 pieces, more than the child's floor of 64


def test_mixed_shapes_in_one_batch_on_the_lane_kernels(pkg, oracle):
    names = names_of("shapes") + names_of("round2")
    assert {cc.stream(pkg.synth, cc.CASES[n].recipe).rpa for n in names} == {40, 80, 160}
    compare(pkg, oracle, names, run(pkg, oracle, names, "planar", 3), "planar")


def test_mixed_shapes_with_more_pieces_than_the_child_floor(pkg, oracle):
    """every case of the table in one batch: the child context is created for more than 64 ranges at once"""
    names = list(cc.CASES)
    pieces = sum(min(cc.CASES[n].claim["ranges"], cm.LIMITS[0]) for n in MANY)
    assert pieces > 64 and set(MANY) <= set(names)
    compare(pkg, oracle, names, run(pkg, oracle, names, "interleaved", 0), "interleaved")


def test_one_context_few_many_few(pkg, oracle):
    """a caller's context: a call with few ranges, one with more than the child context holds, one with few again --
    each as on a context of its own (the child is created again, the rounds' scratch grows and is used smaller)"""
    hd = pkg.hipdec
    few, few2 = ["mono_flip", "clean_six96", "varrows_flip"], ["stereo_two", "lead2", "six96x2_zero2048"]
    ctx = hd.Context(0, len(MANY), 2048)
    try:
        for names in (few, list(MANY), few2):
            got = run(pkg, oracle, names, "planar", 0, ctx=ctx)
            own = run(pkg, oracle, names, "planar", 0)
            for a, b in zip(got[0], own[0]):
                assert a.shape == b.shape and np.array_equal(a, b)
            key = lambda infos: [(int(i.status), int(i.pcm_frames), int(i.mlp_frames)) for i in infos]     # noqa: E731
            assert key(got[1]) == key(own[1]) and got[2] == own[2]
            compare(pkg, oracle, names, got, "planar")
    finally:
        ctx.close()


def _guarded_decode(hd, streams, rows, channels, layout, conceal, slack=64):
    """index and one decode into regions of `rows` frames in a buffer that starts out as SENTINEL everywhere
    -> (host copy of the whole buffer, infos, regions)"""
    batch = hd.Batch(streams)
    st = batch.current_stream
    ctx = hd.Context(0, len(streams), 1024, 0, layout)
    try:
        ctx.set_conceal(conceal)
        ctx.index_batch(batch, st)
        out = hd.PcmRegions(rows, channels, layout, slack=slack, fill=SENTINEL)
        ctx.decode(*out.ptrs, st)
        infos = list(ctx.stream_info(stream=st))
        return out.d_pcm.cpu().numpy(), infos, out
    finally:
        ctx.close()


def _three(pkg, oracle):
    """a damaged six-channel stream between two clean ones; the damaged one composes to the frames its bytes decode to
    without conceal mode, so what lies behind pcm_frames is nobody's"""
    syn = pkg.synth
    names = ["clean_six96", "resume_header", "clean_chained"]
    streams = [cc.damaged(syn, oracle, n) for n in names]
    wants = [cc.expect(syn, oracle, n)[0] for n in names]
    assert wants[1].shape[1] == cc.stream(syn, "six96").frames
    return names, streams, wants


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_nothing_written_outside_the_streams_frames(pkg, oracle, layout):
    hd = pkg.hipdec
    names, streams, wants = _three(pkg, oracle)
    rows = [w.shape[1] + 5 for w in wants]
    host, infos, out = _guarded_decode(hd, streams, rows, [6, 6, 6], _layout(hd, layout), True)
    sent = np.int32(SENTINEL)
    for name, w, inf, o, r in zip(names, wants, infos, out.out_off, rows):
        f = int(inf.pcm_frames)
        assert f == w.shape[1], name
        if layout == "planar":
            region = host[o:o + 6 * r].reshape(6, r)
            assert np.array_equal(region[:, :f], w), name
            assert (region[:, f:] == sent).all(), "%s: written at or behind pcm_frames of a channel row" % name
        else:
            region = host[o:o + 6 * r]
            assert np.array_equal(region[:6 * f].reshape(f, 6).T, w), name
            assert (region[6 * f:] == sent).all(), "%s: written behind pcm_frames * channels" % name
    end = out.out_off[-1] + 6 * rows[-1]
    assert len(host) == end + 64 and (host[end:] == sent).all(), "the slack behind the last region"
    assert infos[1].status & hd.ST_CONCEALED and not infos[0].status & ~hd.ST_BENIGN and not infos[2].status & ~hd.ST_BENIGN


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_region_one_frame_too_small_holds_no_concealed_output(pkg, oracle, layout):
    """DVDA_ST_OVERFLOW, pcm_frames = the need; the region is what the decode without conceal mode leaves there; the
    neighbours and the slack are untouched by it"""
    hd = pkg.hipdec
    names, streams, wants = _three(pkg, oracle)
    rows = [w.shape[1] for w in wants]
    rows[1] -= 1
    host, infos, out = _guarded_decode(hd, streams, rows, [6, 6, 6], _layout(hd, layout), True)
    plain, pinfos, _ = _guarded_decode(hd, streams, rows, [6, 6, 6], _layout(hd, layout), False)
    assert infos[1].status & hd.ST_CONCEALED and infos[1].status & hd.ST["OVERFLOW"]
    assert not infos[1].status & ~(hd.ST_BENIGN | hd.ST_CONCEALED | hd.ST["OVERFLOW"])
    assert int(infos[1].pcm_frames) == wants[1].shape[1] == rows[1] + 1
    assert np.array_equal(host, plain), "conceal mode wrote into a buffer whose region could not hold the stream"
    for k in (0, 2):
        o, r = out.out_off[k], rows[k]
        got = host[o:o + 6 * r].reshape(6, r) if layout == "planar" else host[o:o + 6 * r].reshape(r, 6).T
        assert np.array_equal(got, wants[k]) and not infos[k].status & ~hd.ST_BENIGN
    end = out.out_off[-1] + 6 * rows[-1]
    assert (host[end:] == np.int32(SENTINEL)).all()
