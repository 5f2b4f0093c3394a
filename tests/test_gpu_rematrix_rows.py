"""The fast pass puts a matrix's result into the staging tile by an LDS store on top of its output channel's value
(csrc/mlp_decode.h: PLACE), under the lanes that have the matrix, and matrix 1 reads matrix 0's result through a
coefficient taken out of its own at the block header.  What that can get wrong is a matter of WHICH lanes of a wave have
which matrices, of two matrices that write one channel, of every per-channel parameter the stored values are made from
(output channel, quantisation step, output shift, noise), of headers that change them inside a title, and of waves whose
lanes do not flush together -- so these cases vary exactly those, each bit-exact against the oracle for PCM, frame counts
and status, in the three layouts, the interleaved one also with the wave's cooperative flush forced.  Every batch is
forced onto the lane kernels (lanes_per_segment = 1).  Titles are 8 access units with a restart every 8: one segment."""
import numpy as np
import pytest

from tests import test_gpu_ring_refill as R

pytestmark = pytest.mark.gpu

# planar, interleaved (per-lane flush: the batch is below the cooperative flush's threshold), interleaved with the
# cooperative flush forced for every batch, packed 24-bit WAV payload
LAYOUTS = ["planar", "interleaved", "interleaved_coop", "wav24"]


def _run(pkg, oracle, titles, layout, monkeypatch):
    """every title bit-exact, status benign -> infos"""
    hip = pkg.hipdec
    if layout == "interleaved_coop":
        monkeypatch.setenv("DVDA_COOP_MIN_SEG", "1")        # read when the context is made
        layout = "interleaved"
    if layout == "wav24":
        R._check_wav24(pkg, oracle, titles)
        return None
    return R._check_int32(pkg, titles, hip.PCM_INTERLEAVED if layout == "interleaved" else hip.PCM_PLANAR)


# ---------------------------------------------------------------- matrix counts mixed in one wave
@pytest.fixture(scope="module")
def mixed_count_titles(pkg, oracle):
    """96 six-channel recipe titles with 0, 1 and 2 matrices, title by title: in every wave some lanes have no matrix and
    some no matrix 1"""
    syn = pkg.synth
    return R._titles(pkg, oracle, [(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=8, restart_interval=8,
                                                 n_matrices=i % 3), 61000 + i) for i in range(96)])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_matrix_counts_mixed_in_one_wave(pkg, oracle, mixed_count_titles, layout, monkeypatch):
    infos = _run(pkg, oracle, mixed_count_titles, layout, monkeypatch)
    if infos is not None:
        assert all(inf.status == 0 for inf in infos)        # the fast pass alone


# ---------------------------------------------------------------- both matrices write one channel
@pytest.fixture(scope="module")
def one_channel_titles(pkg, oracle):
    """Mono titles with two matrices (the generator gives both output channel 0: the later store wins, and matrix 1
    reads matrix 0's result) beside stereo titles with two (matrix 1 writes channel 1 and reads matrix 0's channel 0
    through a coefficient the generator never makes zero), title by title in the same waves"""
    syn = pkg.synth
    return R._titles(pkg, oracle, [(syn.make_cfg(assignment=i % 2, rate_code=1, n_substreams=1, n_aus=8, restart_interval=8,
                                                 n_matrices=2), 62000 + i) for i in range(80)])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_both_matrices_write_one_channel(pkg, oracle, one_channel_titles, layout, monkeypatch):
    infos = _run(pkg, oracle, one_channel_titles, layout, monkeypatch)
    if infos is not None:
        assert all(inf.status == 0 for inf in infos)


# ---------------------------------------------------------------- every output channel, noise, quant steps, output shifts
def _fuzz_titles(pkg, oracle, feats, n, n_aus, seed0):
    syn = pkg.synth
    f = 0
    for name in feats:
        f |= syn.SF[name]
    return R._titles(pkg, oracle, [(syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=n_aus, profile=1, features=f,
                                                 restart_interval=8), seed0 + i) for i in range(n)])


@pytest.fixture(scope="module")
def random_matrix_titles(pkg, oracle):
    """256 six-channel titles with 0..6 random matrices (any output channel, fractional bits, bypassed LSBs, coefficients
    present or not), noise shifts and coefficients, quantisation steps and output shifts"""
    return _fuzz_titles(pkg, oracle, ("MATRIXRAND", "NOISE", "QSS", "OUTSHIFT"), 256, 8, 63000)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_output_channel_noise_steps_and_shifts(pkg, oracle, random_matrix_titles, layout, monkeypatch):
    infos = _run(pkg, oracle, random_matrix_titles, layout, monkeypatch)
    if infos is not None:
        fast = sum(1 for inf in infos if inf.status == 0)
        print("decoded by the fast pass alone: %d of %d" % (fast, len(infos)))
        assert fast >= 64, fast                             # (the generator draws 0..6 matrices: about 3 in 7 have <= 2)


# ---------------------------------------------------------------- parameters that change inside a title
@pytest.fixture(scope="module")
def changing_titles(pkg, oracle):
    """The same with blocks that carry new matrices, quantisation steps and output shifts inside a title: 32 access
    units, four segments, the folded coefficient and the stored values redone at the headers.  Titles that leave the
    fast pass (more than two matrices, a change inside a frame) are compared like the rest."""
    return _fuzz_titles(pkg, oracle, ("MATRIXRAND", "NOISE", "QSS", "OUTSHIFT", "PARAMBLOCKS"), 64, 32, 64000)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_parameters_change_inside_a_title(pkg, oracle, changing_titles, layout, monkeypatch):
    _run(pkg, oracle, changing_titles, layout, monkeypatch)


# ---------------------------------------------------------------- a wave with one lane
@pytest.fixture(scope="module")
def one_lane_wave_titles(pkg, oracle):
    """65 segments of the recipe: the second wave has one lane, and its vote for the cooperative flush fails"""
    syn = pkg.synth
    cfg = syn.make_cfg(assignment=12, rate_code=1, n_substreams=1, n_aus=8, restart_interval=8)
    return R._titles(pkg, oracle, [(cfg, 65000 + i) for i in range(65)])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_wave_with_one_lane(pkg, oracle, one_lane_wave_titles, layout, monkeypatch):
    infos = _run(pkg, oracle, one_lane_wave_titles, layout, monkeypatch)
    if infos is not None:
        assert all(inf.status == 0 for inf in infos)
