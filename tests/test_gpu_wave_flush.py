"""The wave's cooperative PCM flush (csrc/mlp_decode.h: coop_out) hands the lanes' output offsets round first, reads the
staging tile's pieces in groups and stores them by the register quad, from a tile whose planes are 65 dwords apart in
the headline instance.  What that can get wrong is a matter of WHICH lane stores which piece of whose run (all seven store
instructions, the last one lanes 0..23's for the runs of lanes 60..63), of WHERE the runs lie (regions out of lane
order, not on multiples of 96 bytes, guards either side), of waves that stop flushing together (lanes leaving one by one,
a lane out of output capacity), of waves whose tile is not in output order, of the instances that share the code (the
two-substream lane) or the tile (planar, packed WAV), and of the chain parse pass's line flush (built the same way, measured
slower and left as it was: its cases stay) -- so these cases vary
exactly those, each bit-exact against the oracle for PCM, frame counts and status.  Every batch is forced onto the lane
kernels: lanes_per_segment = 1, and 3 for the two-substream titles (under 1 the one-substream kernel takes the whole batch and
reports a two-substream stream as DVDA_ST_ENVELOPE; 3 picks the lane kernel by the substream count and never the
wave-cooperative kernel).  The frame-major batches run with the cooperative flush forced (DVDA_COOP_MIN_SEG=1, read when a
context is made)."""
import numpy as np
import pytest

from tests import test_gpu_ring_refill as R

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
GUARD_WORDS = 64
LANES_BY_SUBSTREAMS = {1: R.LANES, 2: 3}


def _check_int32(pkg, titles, layout, lanes):
    """tests.test_gpu_ring_refill._check_int32 with the lane kernels chosen by `lanes`"""
    hip = pkg.hipdec
    pcm, infos = hip.decode_streams([t[0] for t in titles], lanes_per_segment=lanes, layout=layout)
    for i, ((b, f, nch, want), got, inf) in enumerate(zip(titles, pcm, infos)):
        assert inf.status & ~hip.ST_BENIGN == 0, "stream %d status %#x" % (i, inf.status)
        assert inf.pcm_frames == f and inf.channels == nch, (i, inf.pcm_frames, f)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "stream %d differs at %s" % (i, np.argwhere(got != want)[:4].tolist())
    return infos


def _coop(monkeypatch):
    monkeypatch.setenv("DVDA_COOP_MIN_SEG", "1")


# ---------------------------------------------------------------- whole waves and a part-filled one; the layouts that share the tile
@pytest.fixture(scope="module")
def recipe_titles(pkg, oracle):
    """65 six-channel recipe titles of 16 access units, two segments each: the first 32 / 64 / 65 of them are 64 / 128 / 130
    segments -- one wave, two waves, two waves and a wave of two lanes (which flushes per lane)"""
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=16)
    return R._titles(pkg, oracle, [(cfg, 71000 + i) for i in range(65)])


@pytest.mark.parametrize("layout", ["interleaved", "planar", "wav24"])
@pytest.mark.parametrize("n_titles", [32, 64, 65], ids=["64_segments", "128_segments", "130_segments"])
def test_whole_waves_and_a_part_filled_one(pkg, oracle, recipe_titles, n_titles, layout, monkeypatch):
    _coop(monkeypatch)
    titles = recipe_titles[:n_titles]
    if layout == "wav24":
        R._check_wav24(pkg, oracle, titles)
        return
    hip = pkg.hipdec
    infos = R._check_int32(pkg, titles, hip.PCM_INTERLEAVED if layout == "interleaved" else hip.PCM_PLANAR)
    assert all(inf.status == 0 and inf.segments == 2 for inf in infos)


# ---------------------------------------------------------------- regions placed by the caller, guards either side
def _placed(titles, rows, seed):
    """-> (out_off[i], words of the buffer): the regions (rows[i] frames of the title's channels, frame-major) in a seeded
    shuffled order, each on 16 bytes but on no multiple of 96, GUARD_WORDS words between neighbours and at both ends"""
    order = np.random.default_rng(seed).permutation(len(titles))
    out_off, pos = [0] * len(titles), GUARD_WORDS
    for t in order:
        pos = (pos + 3) & ~3
        if pos % 24 == 0:
            pos += 4
        out_off[t] = pos
        pos += rows[t] * titles[t][2] + GUARD_WORDS
    assert any(out_off[i] > out_off[i + 1] for i in range(len(titles) - 1))
    assert all(o % 4 == 0 and o % 24 != 0 for o in out_off)
    return out_off, pos


def _decode_placed(pkg, titles, rows, out_off, words):
    """frame-major decode into caller-placed regions of a guard-filled buffer -> (host copy of the buffer, infos)"""
    hip = pkg.hipdec
    n = len(titles)
    batch = hip.Batch([t[0] for t in titles])
    ctx = hip.Context(0, n, 1024, R.LANES, hip.PCM_INTERLEAVED)
    try:
        ctx.index_batch(batch)
        out = hip.PcmRegions(rows, [t[2] for t in titles], hip.PCM_INTERLEAVED, out_off=out_off,
                             slack=words - max(o + r * t[2] for o, r, t in zip(out_off, rows, titles)), fill=GUARD)
        assert out.d_pcm.numel() == words
        ctx.decode(*out.ptrs, 0)
        infos = list(ctx.stream_info(n))
        return out.d_pcm.cpu().numpy(), infos
    finally:
        ctx.close()


def _guards_untouched(host, titles, rows, out_off):
    """every word outside the titles' regions still holds the fill"""
    outside = np.ones(len(host), bool)
    for o, r, t in zip(out_off, rows, titles):
        outside[o:o + r * t[2]] = False
    assert outside.sum() >= GUARD_WORDS * (len(titles) + 1)
    bad = np.flatnonzero(outside & (host != GUARD))
    assert bad.size == 0, "stray stores at words %s" % bad[:8].tolist()


def test_regions_out_of_lane_order_between_guards(pkg, oracle, recipe_titles, monkeypatch):
    """130 segments into regions in a shuffled order, none on a multiple of 96 bytes, 64 guard words around each: a wrong
    lane-to-run mapping puts a piece into another title's region, a stray store into a guard"""
    _coop(monkeypatch)
    hip = pkg.hipdec
    titles = recipe_titles
    rows = [t[1] for t in titles]
    out_off, words = _placed(titles, rows, 7)
    host, infos = _decode_placed(pkg, titles, rows, out_off, words)
    for i, ((b, f, nch, want), inf, o) in enumerate(zip(titles, infos, out_off)):
        assert inf.status == 0 and inf.pcm_frames == f, (i, hex(inf.status))
        got = host[o:o + f * nch].reshape(f, nch).T
        assert np.array_equal(got, want), "title %d differs at %s" % (i, np.argwhere(got != want)[:4].tolist())
    _guards_untouched(host, titles, rows, out_off)


# ---------------------------------------------------------------- lanes leaving the wave one by one
@pytest.fixture(scope="module")
def ragged_titles(pkg, oracle):
    """48 six-channel titles of 9..31 access units with a restart every 4: three to eight segments each, over three waves
    whose lanes run out of rows at different turns -- the wave's vote fails from there on and the rest flush per lane"""
    syn = pkg.synth
    titles = R._titles(pkg, oracle, [(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=9 + (i * 7) % 23,
                                                   restart_interval=4), 72000 + i) for i in range(48)])
    assert len({t[1] for t in titles}) >= 16
    return titles


def test_lanes_leave_the_wave_one_by_one(pkg, oracle, ragged_titles, monkeypatch):
    _coop(monkeypatch)
    infos = R._check_int32(pkg, ragged_titles, pkg.hipdec.PCM_INTERLEAVED)
    assert all(inf.status == 0 for inf in infos)


# ---------------------------------------------------------------- output capacity ending inside a group of four frames
def test_capacity_ends_inside_a_group_of_four_frames(pkg, oracle, recipe_titles, monkeypatch):
    """One title of a full wave is given 6 frames less than it has (its last whole group of four frames ends 2 frames in
    front of the capacity): it reports ST_OVERFLOW, its lane stops flushing with the wave, and what the wave's other
    lanes store -- per lane from there on -- is theirs alone"""
    _coop(monkeypatch)
    hip = pkg.hipdec
    titles = recipe_titles[:32]
    short = 13                                              # segments 26 and 27: inside the wave
    rows = [t[1] for t in titles]
    assert rows[short] % 4 == 0
    rows[short] -= 6
    out_off, words = _placed(titles, rows, 11)
    host, infos = _decode_placed(pkg, titles, rows, out_off, words)
    for i, ((b, f, nch, want), inf, o) in enumerate(zip(titles, infos, out_off)):
        if i == short:
            assert inf.status & hip.ST["OVERFLOW"] and inf.status & ~(hip.ST_BENIGN | hip.ST["OVERFLOW"]) == 0, hex(inf.status)
            f = rows[i] & ~3                                # the whole groups of four in front of the capacity
        else:
            assert inf.status == 0 and inf.pcm_frames == f, (i, hex(inf.status))
        got = host[o:o + f * nch].reshape(f, nch).T
        assert np.array_equal(got, want[:, :f]), "title %d differs at %s" % (i, np.argwhere(got != want[:, :f])[:4].tolist())
    _guards_untouched(host, titles, rows, out_off)


# ---------------------------------------------------------------- waves that are not in identity channel order
@pytest.fixture(scope="module")
def mixed_shape_titles(pkg, oracle):
    """64 two-channel titles (whole waves of them: the tile is [channel][frame][lane], the flush per lane), then 6-, 2-,
    6-channel (another rate) and 5-channel titles title by title (waves of mixed shapes), then 32 six-channel recipe titles
    (a wave that flushes together): 12 access units, restart every 4, three segments each"""
    syn = pkg.synth
    feats = syn.SF_FAST & ~(syn.SF["IIR"] | syn.SF["MATRIXRAND"])
    cases = []
    for i in range(64):
        cases.append((syn.make_cfg(assignment=1, rate_code=1, n_substreams=1, n_aus=12, restart_interval=4), 73000 + i))
    for i in range(32):
        asg, rc = [(12, 1), (1, 1), (12, 2), (6, 0)][i % 4]
        cases.append((syn.make_cfg(assignment=asg, rate_code=rc, n_substreams=1, n_aus=12, profile=1, features=feats,
                                   restart_interval=4), 73100 + i))
    for i in range(32):
        cases.append((syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=12, restart_interval=4), 73200 + i))
    return R._titles(pkg, oracle, cases)


def test_waves_not_in_identity_channel_order(pkg, oracle, mixed_shape_titles, monkeypatch):
    _coop(monkeypatch)
    R._check_int32(pkg, mixed_shape_titles, pkg.hipdec.PCM_INTERLEAVED)


# ---------------------------------------------------------------- the two-substream lane
@pytest.fixture(scope="module")
def two_substream_titles(pkg, oracle):
    """35 six-channel titles in two substreams, 16 access units, two segments each"""
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=2, n_aus=16)
    return R._titles(pkg, oracle, [(cfg, 74000 + i) for i in range(35)])


@pytest.mark.parametrize("n_titles", [32, 35], ids=["64_segments", "70_segments"])
def test_two_substream_lane(pkg, oracle, two_substream_titles, n_titles, monkeypatch):
    _coop(monkeypatch)
    infos = _check_int32(pkg, two_substream_titles[:n_titles], pkg.hipdec.PCM_INTERLEAVED, LANES_BY_SUBSTREAMS[2])
    assert all(inf.status == 0 and inf.substreams == 2 for inf in infos)


# ---------------------------------------------------------------- the chain parse pass's line flush
@pytest.fixture(scope="module")
def chained_titles(pkg, oracle):
    """per substream count, 35 chained six-channel titles of 8 access units with a restart every 4: two segments each,
    64 segments (whole waves of the parse pass write their lines together) or 70 (one wave does not)"""
    syn = pkg.synth
    SF = syn.SF
    return {ns: R._titles(pkg, oracle, [(syn.make_cfg(assignment=12, rate_code=1, n_substreams=ns, n_aus=8, profile=1,
                                                      features=SF["CHAINED"], restart_interval=4), 75000 + 100 * ns + i)
                                        for i in range(35)]) for ns in (1, 2)}


@pytest.mark.parametrize("n_titles", [32, 35], ids=["64_segments", "70_segments"])
@pytest.mark.parametrize("n_substreams", [1, 2])
def test_chain_parse_pass_writes_its_lines_together(pkg, oracle, chained_titles, n_substreams, n_titles, monkeypatch):
    _coop(monkeypatch)
    hip = pkg.hipdec
    titles = chained_titles[n_substreams][:n_titles]
    for layout in (hip.PCM_INTERLEAVED, hip.PCM_PLANAR):
        infos = _check_int32(pkg, titles, layout, LANES_BY_SUBSTREAMS[n_substreams])       # (ST_BENIGN allowed)
        assert sum(1 for inf in infos if inf.status & hip.ST["CHAINED"]) >= n_titles // 2     # (the parse pass ran)
