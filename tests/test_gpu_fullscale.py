"""The HIP path at full 24-bit scale and at the rails of every parameter: the batches of tests/test_fullscale_model.py
(generator modes FULLSCALE and WIDEPARAMS; the CPU tests there show that each batch stays inside the envelope, reaches
accumulators of 2^36 and more and carries every extreme of every field) through each piece of arithmetic the library
has -- lane kernels, cooperative kernel, both forms of the chain passes, sequential and general pass, the two-substream
lane, the streaming tier's stepper, the presentation kernels, conceal mode -- bit for bit against the restatement.
The four reference-made goldens of these modes run in tests/test_gpu_parity.py::test_golden_vectors_on_gpu (and with
each chain form in tests/test_gpu_chain_forms.py), which take every tests/golden/*.npz."""
import ctypes

import numpy as np
import pytest

from tests import test_fullscale_model as M
from tests import test_gpu_parity as T
from tests.test_gpu_chain_forms import form  # noqa: F401  (the fixture that forces a form of the chain passes)
from tests.test_gpu_presentation import check as check_presentation

pytestmark = pytest.mark.gpu


def _want(pkg, oracle, name):
    """-> [(cfg, bytes, frames, pcm of the restatement)]"""
    out = []
    for (cfg, b, f), (pcm, r, st, _) in zip(M.streams(pkg, name), M.decoded(pkg, oracle, name)):
        assert st == 0 and r == f
        out.append((cfg, b, f, pcm))
    return out


# (one lane per segment takes one-substream streams only: include/dvda_mlp_hip.h)
LANES = [(1, 0), (1, 1), (1, 2), (1, 64), (2, 0), (2, 2), (2, 64)]


@pytest.mark.parametrize("S,lanes", LANES)
@pytest.mark.parametrize("kind", ["full", "wide", "both_fast"])
def test_lane_kernels_and_cooperative_kernel(pkg, oracle, kind, S, lanes):
    """planar and interleaved int32 PCM (T._check decodes into both)"""
    T._check(pkg, oracle, M.cases(pkg, "%s_S%d" % (kind, S)), lanes=lanes)


# the lane kernels' own payload writers (forced lanes: a batch this small goes to the cooperative kernel otherwise) for the
# batches of the fast pass; the chain passes' and the sequential pass's writers for the two that are deferred
WAV_CASES = [(k, S, lanes) for k in ("full", "wide", "both_fast") for S, lanes in LANES] + \
            [(k, S, 0) for k in ("chained_firrand", "varrows") for S in (1, 2)]


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("kind,S,lanes", WAV_CASES)
def test_wav_payload(pkg, oracle, kind, S, lanes, bits):
    """the WAV payload cuts what the shift pushed past 24 (16) bits and keeps -2^23: oracle.wav_pack is the
    reference's write_signed.  Every writer of it: cooperative kernel (lanes 0 and 64), one-lane kernel, two-substream
    lane and lane pairs (1, 2), chain and sequential pass"""
    hip = pkg.hipdec
    want = _want(pkg, oracle, "%s_S%d" % (kind, S))
    got, infos = hip.decode_streams_wav([b for _, b, _, _ in want], bits, lanes_per_segment=lanes)
    for (cfg, b, f, pcm), payload, inf in zip(want, got, infos):
        assert inf.status & ~hip.ST_BENIGN == 0 and inf.pcm_frames == f, hex(inf.status)
        ref = np.frombuffer(oracle.wav_pack(pcm, bits), np.uint8)
        assert len(payload) == len(ref) == f * pcm.shape[0] * bits // 8
        assert np.array_equal(payload, ref), "first difference at byte %d" % int(np.argmax(payload != ref))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("kind", ["chained_firrand", "disc_chained_mixbooks", "iir"])
def test_chain_passes_in_each_form(pkg, oracle, form, kind, S):  # noqa: F811
    T._check(pkg, oracle, M.cases(pkg, "%s_S%d" % (kind, S)), lanes=2)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("kind", ["midrestart_varblock", "midmatrix", "varrows"])
def test_sequential_and_general_pass(pkg, oracle, kind, S):
    T._check(pkg, oracle, M.cases(pkg, "%s_S%d" % (kind, S)), lanes=2)


@pytest.mark.parametrize("lanes", [0, 2])
@pytest.mark.parametrize("S", [1, 2])
def test_iir_up_to_order_8_with_step_sizes_up_to_15(pkg, oracle, S, lanes):
    """the fast pass's cold path and, where the library defers, the chain passes in the form it picks itself"""
    T._check(pkg, oracle, M.cases(pkg, "iir_S%d" % S), lanes=lanes)


@pytest.mark.parametrize("ss0", [1, 2, 3, 4, 5])
def test_two_substreams_of_any_split(pkg, oracle, ss0):
    T._check(pkg, oracle, M.cases(pkg, "duo_ss0_%d" % ss0), lanes=2)


@pytest.mark.parametrize("lanes", [0, 2])
def test_lanes_of_one_wave_that_disagree(pkg, oracle, lanes):
    """128 titles of 8 access units, every other one at full scale with wide parameters, the rest the plain recipe.
    lanes=2 is the case that puts both kinds into one wave (forced lane kernels: neighbouring lanes hold neighbouring
    titles); lanes=0 is the library's own choice, which for a batch this small is the cooperative kernel, one workgroup
    per segment -- the same titles, nothing diverging inside a wave"""
    hip = pkg.hipdec
    want = _want(pkg, oracle, "disagree_128")
    pcm, infos = T._both(hip, [b for _, b, _, _ in want], lanes_per_segment=lanes)
    for i, ((cfg, b, f, ref), got, inf) in enumerate(zip(want, pcm, infos)):
        assert inf.status & ~hip.ST_BENIGN == 0 and inf.pcm_frames == f, "title %d status %#x" % (i, inf.status)
        assert got.shape == ref.shape and np.array_equal(got, ref), "title %d differs at %s" % (
            i, np.argwhere(got != ref)[:4].tolist())


@pytest.mark.parametrize("chunk", [2048, 777, 2013])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_streaming_tier(pkg, oracle, which, chunk):
    """MLPDecoder.decode_packet with packets of 2 KB and of odd sizes: the PCM and every call's return value are the
    restatement's (modelled on tests/test_gpu_parity.py::test_streaming_tier_mirrors_mlp_h)"""
    syn, hip = pkg.synth, pkg.hipdec
    cfg, data, frames, want = _want(pkg, oracle, "streaming")[which]
    nch = syn.channels(cfg.assignment)
    ol = oracle.lib
    ol.mlp_oracle_open.restype = ctypes.c_void_p
    ol.mlp_oracle_decode_packet.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    ol.mlp_oracle_decode_packet.restype = ctypes.c_uint
    ol.mlp_oracle_close.argtypes = [ctypes.c_void_p]
    od = ol.mlp_oracle_open(nch)
    dec = hip.MLPDecoder(cfg.bps_code, cfg.bps_code, cfg.rate_code, cfg.rate_code, cfg.assignment)
    samples = [[] for _ in range(nch)]
    try:
        for off in range(0, len(data), chunk):
            piece = np.ascontiguousarray(data[off:off + chunk])
            want_n = ol.mlp_oracle_decode_packet(od, piece.ctypes.data, len(piece))
            got_n = dec.decode_packet(piece, samples)
            assert dec.status & ~hip.ST_BENIGN == 0, hex(dec.status)
            assert got_n == want_n, "packet at %d: %d vs %d" % (off, got_n, want_n)
    finally:
        ol.mlp_oracle_close(od)
        dec.close()
    got = np.asarray(samples, np.int32)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("layout", ["planar", "interleaved", "wav24"])
def test_presentation_of_substream_0(pkg, oracle, layout):
    """presentation=1: substream 0's own matrices and output shifts, against tests/presentation_model.py"""
    streams = [b for _, b, _ in M.streams(pkg, "presentation")]
    check_presentation(pkg, oracle, streams, layout)
    check_presentation(pkg, oracle, streams, layout, lanes=3)


@pytest.mark.parametrize("S", [1, 2])
def test_conceal_mode_leaves_undamaged_titles_alone(pkg, oracle, S):
    hip = pkg.hipdec
    want = _want(pkg, oracle, "full_S%d" % S)
    streams = [b for _, b, _, _ in want]
    off, ioff = hip.decode_streams(streams)
    on, ion, spans = hip.decode_streams_concealed(streams)
    assert spans == [[] for _ in streams]
    for (cfg, b, f, ref), a, c, x, y in zip(want, off, on, ioff, ion):
        assert x.status & ~hip.ST_BENIGN == 0
        assert (x.status, x.pcm_frames, x.mlp_frames) == (y.status, y.pcm_frames, y.mlp_frames)
        assert np.array_equal(a, ref) and np.array_equal(c, ref)
