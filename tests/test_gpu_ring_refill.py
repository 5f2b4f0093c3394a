"""The one-substream lane kernels refill their input rings by 16-byte granules, the whole wave in the same row
(csrc/mlp_decode.h: WAVE_FILL, BitReaderT<32, 4>): when any lane of a wave is down to half a ring, every lane takes the
granules its ring has room for -- none, or up to four.  What that can get wrong is a matter of WHERE a lane's bytes
start (the phase of a stream inside a 64-byte chunk), of HOW MUCH each lane of a wave eats per row, and of the END of
the buffer, so these cases vary exactly those, each bit-exact against the oracle for PCM, frame counts and status.
Every batch is forced onto the lane kernels (lanes_per_segment = 1): batches of this size are otherwise the
wave-cooperative kernel's."""
import numpy as np
import pytest

from tests import test_gpu_parity as T

pytestmark = pytest.mark.gpu

LANES = 1       # the one-substream lane kernel for every stream (and the lane instance of the chain parse pass)


def _titles(pkg, oracle, cfgs_seeds):
    """-> [(bytes, frames, channels, oracle PCM)] -- generated and decoded by the oracle once per case list"""
    syn = pkg.synth
    out = []
    for cfg, seed in cfgs_seeds:
        b, f = syn.stream(cfg, seed)
        nch = syn.channels(cfg.assignment)
        want, r, st = oracle.decode(b, nch, f)
        assert st == 0 and r == f
        out.append((b, f, nch, want))
    return out


def _check_int32(pkg, titles, layout):
    hip = pkg.hipdec
    pcm, infos = hip.decode_streams([t[0] for t in titles], lanes_per_segment=LANES, layout=layout)
    for i, ((b, f, nch, want), got, inf) in enumerate(zip(titles, pcm, infos)):
        assert inf.status & ~hip.ST_BENIGN == 0, "stream %d status %#x" % (i, inf.status)
        assert inf.pcm_frames == f and inf.channels == nch, (i, inf.pcm_frames, f)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "stream %d differs at %s" % (i, np.argwhere(got != want)[:4].tolist())
    return infos


def _check_wav24(pkg, oracle, titles):
    hip = pkg.hipdec
    got, infos = hip.decode_streams_wav([t[0] for t in titles], 24, lanes_per_segment=LANES)
    for i, ((b, f, nch, want), payload, inf) in enumerate(zip(titles, got, infos)):
        assert inf.status & ~hip.ST_BENIGN == 0, "stream %d status %#x" % (i, inf.status)
        assert inf.pcm_frames == f and inf.channels == nch
        ref = np.frombuffer(oracle.wav_pack(want, 24), np.uint8)
        assert len(payload) == len(ref) and np.array_equal(payload, ref), "stream %d: first difference at byte %d" % (
            i, int(np.argmax(payload != ref)) if len(payload) == len(ref) else -1)


def _check(pkg, oracle, titles, layout):
    if layout == "wav24":
        _check_wav24(pkg, oracle, titles)
    else:
        _check_int32(pkg, titles, pkg.hipdec.PCM_INTERLEAVED if layout == "interleaved" else pkg.hipdec.PCM_PLANAR)


LAYOUTS = ["planar", "interleaved", "wav24"]


# ---------------------------------------------------------------- phases
@pytest.fixture(scope="module")
def phase_titles(pkg, oracle):
    """130 recipe titles of 16 access units (two segments each: over four waves of segments), in an order in which
    their starts fall on all four 16-byte phases of a 64-byte chunk"""
    syn, hip = pkg.synth, pkg.hipdec
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=16)
    titles = _titles(pkg, oracle, [(cfg, 52000 + i) for i in range(130)])
    _, offs, _ = hip.pack_streams([t[0] for t in titles])
    phases = (offs % 64 // 16).astype(np.int64)
    counts = np.bincount(phases, minlength=4)
    assert (offs % 16 == 0).all() and (counts >= 8).all(), counts.tolist()     # every phase, each many times
    return titles


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stream_starts_on_every_phase_of_a_chunk(pkg, oracle, phase_titles, layout):
    _check(pkg, oracle, phase_titles, layout)


# ---------------------------------------------------------------- unequal appetites in one wave
@pytest.fixture(scope="module")
def appetite_titles(pkg, oracle):
    """Lanes side by side that eat a dword a row and lanes that eat five: 1- / 2-channel titles with two LSBs per value
    interleaved title by title with 6-channel titles at the generator's largest huffman_lsbs (24), of unequal
    lengths -- on most turns the light lanes take no granule while the heavy ones take four, and lanes leave the
    wave at different rows."""
    syn = pkg.synth
    cases = []
    for i in range(48):
        if i % 2:
            cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=8 + (i * 5) % 17, huffman_lsbs=24,
                               restart_interval=8)
        else:
            cfg = syn.make_cfg(assignment=(i // 2) % 2, rate_code=1, n_substreams=1, n_aus=8 + (i * 7) % 19,
                               huffman_lsbs=2, restart_interval=8)
        cases.append((cfg, 53000 + i))
    titles = _titles(pkg, oracle, cases)
    per_frame = [len(b) / f for b, f, _, _ in titles]
    assert max(per_frame[0::2]) < 3.0 and min(per_frame[1::2]) >= 20.0, (max(per_frame[0::2]), min(per_frame[1::2]))
    assert len({f for _, f, _, _ in titles}) >= 12          # lengths unequal
    return titles


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unequal_appetites_in_one_wave(pkg, oracle, appetite_titles, layout):
    _check(pkg, oracle, appetite_titles, layout)


# ---------------------------------------------------------------- hungry rows
@pytest.fixture(scope="module")
def hungry_titles(pkg, oracle):
    """6-channel titles of at least 20 bytes per PCM frame: four granules a turn (64 bytes in three rows and more) cannot
    keep up with every lane of the wave, and the row loop's synchronous top-up (ensure(12)) runs"""
    syn = pkg.synth
    cases = []
    for i in range(40):
        cfg = syn.make_cfg(assignment=12, rate_code=[1, 2, 0][i % 3], n_substreams=1, n_aus=12, huffman_lsbs=24,
                           codebook=1 + i % 3, restart_interval=4)
        cases.append((cfg, 54000 + i))
    titles = _titles(pkg, oracle, cases)
    for b, f, _, _ in titles:
        assert len(b) >= 20 * f, (len(b), f)
    return titles


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hungry_rows_take_the_synchronous_top_up(pkg, oracle, hungry_titles, layout):
    _check(pkg, oracle, hungry_titles, layout)


# ---------------------------------------------------------------- end of buffer
@pytest.mark.parametrize("layout", LAYOUTS)
def test_last_stream_ends_inside_the_last_granule(pkg, oracle, layout):
    """The batch's last stream ends inside the buffer's last 16-byte granule; behind it only the 64 spare bytes: the
    fills past it are clamped to the buffer's last granules"""
    syn, hip = pkg.synth, pkg.hipdec
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=16)
    titles = _titles(pkg, oracle, [(cfg, 55000 + i) for i in range(70)])
    # the last title: one whose length is no multiple of 16 (so it ends INSIDE its last granule)
    k = next(i for i in range(len(titles) - 1, -1, -1) if len(titles[i][0]) % 16 != 0)
    titles = titles[:k] + titles[k + 1:] + [titles[k]]
    flat, offs, lens = hip.pack_streams([t[0] for t in titles])
    end = int(offs[-1] + lens[-1])
    assert len(flat) - 64 - end in range(1, 16) and not flat[end:].any()
    _check(pkg, oracle, titles, layout)


@pytest.mark.parametrize("n_aus", [1, 2, 3])
def test_one_stream_of_a_few_access_units(pkg, oracle, n_aus):
    syn = pkg.synth
    for asg, rate in ((12, 1), (1, 0), (12, 2)):
        cfg = syn.make_cfg(assignment=asg, rate_code=rate, n_substreams=1, n_aus=n_aus)
        titles = _titles(pkg, oracle, [(cfg, 56000 + n_aus)])
        for layout in LAYOUTS:
            _check(pkg, oracle, titles, layout)


def test_stream_truncated_inside_an_access_unit(pkg, oracle):
    """The last stream of the batch cut in the middle of an access unit (what
    tests/test_gpu_parity.py::test_edge_cases_truncated_ragged_and_single_unit expects of it): the whole units are
    decoded, the tail is left unconsumed and reported as truncated -- here on the lane kernels, alone and behind
    other titles, so that the cut is the end of the buffer"""
    syn, hip = pkg.synth, pkg.hipdec
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_aus=40)
    others = [syn.stream(cfg, 57000 + i)[0] for i in range(3)]
    whole, frames = syn.stream(cfg, 57010)
    cut = whole[:len(whole) - 123]                      # ends inside the last access unit
    want, r, st = oracle.decode(cut, 6, frames)
    assert st == 0 and r == frames - 80
    for batch in ([cut], others + [cut]):
        pcm, infos = T._both(hip, batch, lanes_per_segment=LANES)
        inf = infos[-1]
        assert inf.status & hip.ST["TRUNCATED"] and inf.status & ~hip.ST_BENIGN == 0, hex(inf.status)
        assert inf.pcm_frames == r and np.array_equal(pcm[-1], want)
        assert inf.bytes_consumed < len(cut)
        for b, got, i2 in zip(batch[:-1], pcm, infos):
            w2, r2, s2 = oracle.decode(b, 6, frames)
            assert s2 == 0 and i2.status & ~hip.ST_BENIGN == 0 and i2.pcm_frames == r2 and np.array_equal(got, w2)


# ---------------------------------------------------------------- the chain parse pass's lane instance
@pytest.fixture(scope="module")
def chained_titles(pkg, oracle):
    syn = pkg.synth
    SF = syn.SF
    cases = []
    for i in range(64):
        cfg = syn.make_cfg(assignment=12 if i % 4 else 1, rate_code=1, n_substreams=1, n_aus=24, profile=1,
                           features=SF["CHAINED"] | (SF["FIRRAND"] if i % 2 else 0), restart_interval=[4, 8, 3, 6][i % 4])
        cases.append((cfg, 58000 + i))
    return _titles(pkg, oracle, cases)


@pytest.mark.parametrize("form", [1, 2], ids=["fused", "two_pass"])
def test_chained_titles_through_the_parse_lanes(pkg, oracle, chained_titles, form):
    """64 chained titles of 24 access units: their segments are deferred to the chain passes, whose parse pass -- lanes
    forced -- is the k_decode instance that reads the whole segment without decoding its rows; both forms of the passes
    behind it (dvda_mlp_hip_set_chain_form)"""
    hip = pkg.hipdec
    hip.CHAIN_FORM = form
    try:
        for layout in (hip.PCM_PLANAR, hip.PCM_INTERLEAVED):
            infos = _check_int32(pkg, chained_titles, layout)
            assert sum(1 for inf in infos if inf.status & hip.ST["CHAINED"]) >= 60
    finally:
        hip.CHAIN_FORM = 0
