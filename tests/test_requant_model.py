"""CPU tests of the word-length reduction (csrc/pcm_requant.h): the contract's known answers, the two forms of
tests/requant_model.py against each other, the library's host arithmetic against the model, the dither's statistics, the
entry points without a GPU, the structs and the symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import requant_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY, ENODEV = -3, -4, -1
SYMBOLS = ("dvda_pcm_hip_requantize", "dvda_pcm_hip_requantize_workspace_words", "dvda_mlp_hip_pcm_requantize",
           "dvda_pcm_hip_requant_value")
# (bits_in, bits_out): s = 8, 4, 4, 0, 0 at the three output depths
DEPTHS = [(24, 16), (24, 20), (20, 16), (24, 24), (16, 16)]
MODES = [rm.TRUNCATE, rm.ROUND, rm.TPDF]


def test_known_answers():
    assert rm.word(0, 0, 0) == 0xe220a8397b1dcdaf            # splitmix64's first output for seed 0
    assert rm.word(0x0123456789ABCDEF, 5, 3) == 0x374ca94be4ab03ac
    want = {0: (101, -133, 9), 1: (-135, 41, -201), 2: (191, 20, 76), 3: (-135, 45, -101), 4: (107, 47, 18),
            2 ** 40 - 1: (-103, 25, -29)}
    for frame, row in want.items():
        assert tuple(rm.noise(1, frame, c, 8) for c in range(3)) == row, frame
    assert tuple(rm.noise(1, 0, c, 4) for c in range(3)) == (-11, -5, 9)
    # the numpy form of the same
    frames = np.array(sorted(want), np.uint64)
    for c in range(3):
        assert rm.noise_np(1, frames, c, 8).tolist() == [want[int(f)][c] for f in frames]
    assert int(rm.word_np(0, np.zeros(1, np.uint64), 0)[0]) == 0xe220a8397b1dcdaf


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits_in,bits_out", DEPTHS)
def test_numpy_form_is_the_integer_form(bits_in, bits_out, mode):
    rng = np.random.default_rng(bits_in * 100 + bits_out + mode)
    pcm = rng.integers(-2 ** 31, 2 ** 31, (3, 300), dtype=np.int64).astype(np.int32)
    pcm[0, :4] = [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]
    pcm[1, 100:200] >>= 32 - bits_in            # inside the nominal range: most do not clip
    for seed, frame0 in ((0, 0), (0xDEADBEEFCAFEF00D, 2 ** 40 - 5), (7, 12345)):
        a, ca = rm.requant(pcm, bits_in, bits_out, mode, seed, frame0)
        b, cb = rm.requant_np(pcm, bits_in, bits_out, mode, seed, frame0)
        assert np.array_equal(a, b) and ca == cb
        assert 0 < ca[1] < 300
    lo, hi = -(1 << (bits_out - 1)), (1 << (bits_out - 1)) - 1
    assert a.min() == lo and a.max() == hi


def test_library_value_is_the_model(pkg):
    hd = pkg.hipdec
    rails = [-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 23, -2 ** 23, 2 ** 23 - 1, -2 ** 23 + 1, 2 ** 23 + 1,
             -2 ** 23 - 1, 0, -1, 1, 127, 128, -128, -129, 2 ** 15 - 1, 2 ** 15, -2 ** 15, -2 ** 15 - 1, 2 ** 19, -2 ** 19 - 1]
    rng = np.random.default_rng(5)
    rand = rng.integers(-2 ** 31, 2 ** 31, 10000, dtype=np.int64)
    rand[::3] >>= 8                              # a third inside 24 bits
    frames = rng.integers(0, 2 ** 41, 10000, dtype=np.int64)
    assert hd.requant_value(2 ** 23 - 1, 0, 0, 24, 16, hd.RQ_ROUND) == (32767, 1)
    assert hd.requant_value(2 ** 23 - 129, 0, 0, 24, 16, hd.RQ_ROUND) == (32767, 0)
    assert hd.requant_value(-2 ** 31, 3, 1, 24, 16, hd.RQ_TRUNCATE) == (-32768, 1)
    for bits_in, bits_out in DEPTHS:
        for mode in MODES:
            for seed in (0, 1, 0xFFFFFFFFFFFFFFFF):
                for i, v in enumerate(rails):
                    for frame in (0, 1, 2, 3, 2 ** 40 - 1, 2 ** 64 - 1):
                        assert hd.requant_value(v, frame, i % 8, bits_in, bits_out, mode, seed) == \
                            rm.value(v, bits_in, bits_out, mode, seed, frame, i % 8), (v, frame, bits_in, bits_out, mode)
    L = hd.lib()
    for k, (bits_in, bits_out) in enumerate(DEPTHS):
        for mode in MODES:
            par = hd.Requant(bits_in, bits_out, mode, 0, 99 + k)
            cl = ctypes.c_int()
            for i in range(10000):
                got = L.dvda_pcm_hip_requant_value(int(rand[i]), int(frames[i]), i % 8, ctypes.byref(par), ctypes.byref(cl))
                assert (got, cl.value) == rm.value(int(rand[i]), bits_in, bits_out, mode, 99 + k, int(frames[i]), i % 8)
    # clipped may be NULL; invalid params: 0 and -1
    par = hd.Requant(24, 16, 1, 0, 0)
    assert L.dvda_pcm_hip_requant_value(2 ** 23 - 1, 0, 0, ctypes.byref(par), None) == 32767
    for bad in ((16, 24, 0, 0), (24, 18, 0, 0), (12, 12, 0, 0), (24, 16, 3, 0), (24, 16, 0, 1)):
        cl = ctypes.c_int(5)
        assert L.dvda_pcm_hip_requant_value(1000, 0, 0, ctypes.byref(hd.Requant(*bad, 0)), ctypes.byref(cl)) == 0
        assert cl.value == -1
        assert L.dvda_pcm_hip_requant_value(1000, 0, 0, ctypes.byref(hd.Requant(*bad, 0)), None) == 0
    with pytest.raises(hd.HipError):
        hd.requant_value(0, 0, 0, 16, 24)


def test_piece_invariance_of_the_model():
    rng = np.random.default_rng(11)
    pcm = (rng.integers(-2 ** 31, 2 ** 31, (4, 6000), dtype=np.int64) >> 7).astype(np.int32)
    for bits_in, bits_out in ((24, 16), (24, 20)):
        whole, cw = rm.requant_np(pcm, bits_in, bits_out, rm.TPDF, 9, 1001)
        total = [0] * 8
        for a, b in ((0, 777), (777, 5000), (5000, 6000)):
            part, cp = rm.requant_np(pcm[:, a:b], bits_in, bits_out, rm.TPDF, 9, 1001 + a)
            assert np.array_equal(whole[:, a:b], part)
            total = [x + y for x, y in zip(total, cp)]
        assert total == cw and sum(cw) > 0


def test_distribution_of_the_dither():
    """TPDF: the error's variance is 1/4 output LSB^2 whatever the input's low bits are (that is what the triangular
    density buys), its mean is zero, and it stays inside +-1.5 LSB; plain rounding has the uniform's 1/12 on a signal
    that sweeps the low bits"""
    n = 1 << 18
    for val in (0, 37, 128, 200):
        x = np.full((1, n), val, np.int32)
        y, cl = rm.requant_np(x, 24, 16, rm.TPDF, 7, 0)
        e = y.astype(np.int64) * 256 - x
        assert cl == [0] * 8
        assert abs(e.var() / 65536 - 0.25) <= 0.005, (val, e.var() / 65536)
        assert abs(e.mean()) <= 2, (val, e.mean())
        assert -384 < e.min() and e.max() < 384
    rng = np.random.default_rng(3)
    x = rng.integers(-2 ** 22, 2 ** 22, (1, n), dtype=np.int64).astype(np.int32)
    y, _ = rm.requant_np(x, 24, 16, rm.ROUND)
    e = y.astype(np.int64) * 256 - x
    assert abs(e.var() / 65536 - 1 / 12) <= 0.002 and -128 <= e.min() and e.max() <= 128


def test_payload_is_write_signed():
    pcm = np.array([[0, -1, 32767, -32768, 65536 + 5], [1, 2, 3, 4, -65536 - 5]], np.int32)
    p16 = rm.payload(pcm, 16)
    assert len(p16) == 20 and p16[:8] == bytes([0, 0, 1, 0, 0xFF, 0xFF, 2, 0]) and p16[16:] == bytes([5, 0, 0xFB, 0xFF])
    p24 = rm.payload(pcm, 24)
    assert len(p24) == 30 and p24[6:12] == bytes([0xFF, 0xFF, 0xFF, 2, 0, 0])


def test_structs_and_constants(pkg):
    hd = pkg.hipdec
    assert ctypes.sizeof(hd.Requant) == 24 and ctypes.sizeof(hd.RequantReport) == 72
    assert (hd.RQ_TRUNCATE, hd.RQ_ROUND, hd.RQ_TPDF) == (rm.TRUNCATE, rm.ROUND, rm.TPDF) == (0, 1, 2)
    assert rm.TILE == hd.LVL_TILE_FRAMES
    r = hd.RequantReport.from_dict(rm.report(7, range(8)))
    assert r.as_dict() == dict(frames=7, clipped=list(range(8)))
    p = hd.Requant.from_dict(dict(bits_in=24, bits_out=16, mode=2, seed=2 ** 64 - 1))
    assert p.as_dict() == dict(bits_in=24, bits_out=16, mode=2, seed=2 ** 64 - 1) and p.reserved == 0


def test_arguments_are_judged_before_the_device(pkg):
    """every DVDA_HIP_EINVAL of the contract, with or without a device; then DVDA_HIP_ECAPACITY; then -- on a machine
    without one -- DVDA_HIP_ENODEV"""
    hd = pkg.hipdec
    L = hd.lib()
    n, bound = 3, 1 << 20
    words = L.dvda_pcm_hip_requantize_workspace_words(n, bound)
    assert words >= 2 * (n + 1) + (bound // rm.TILE + n) * 8
    last = 0
    for k in (0, 1, 2, 100):
        for total in (0, 1, rm.TILE, 10 * rm.TILE + 1, 1 << 30):
            w = L.dvda_pcm_hip_requantize_workspace_words(k, total)
            assert w >= last and w <= L.dvda_pcm_hip_requantize_workspace_words(k + 1, total)
            last = w
        last = L.dvda_pcm_hip_requantize_workspace_words(k, 0)
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data

    def call(par=(24, 16, 2, 0, 0), layout_in=0, layout_out=0, work_words=words, null=None, total=bound):
        q = hd.Requant(*par)
        args = [p, layout_in, p, p, layout_out, p, p, n, ctypes.byref(q), total, p, p, work_words, None]
        if null is not None:
            args[null] = None
        return L.dvda_pcm_hip_requantize(*args)

    for par in ((12, 12, 0, 0, 0), (24, 8, 0, 0, 0), (32, 16, 0, 0, 0), (24, 18, 0, 0, 0), (16, 20, 0, 0, 0),
                (16, 24, 0, 0, 0), (20, 24, 2, 0, 0), (24, 16, 3, 0, 0), (24, 16, 0xFFFFFFFF, 0, 0), (24, 16, 2, 1, 0)):
        assert call(par=par) == EINVAL, par
    for layout_in in (2, 3, 4):
        assert call(layout_in=layout_in) == EINVAL
    assert call(par=(24, 24, 2, 0, 0), layout_in=2, layout_out=2) == EINVAL
    # a WAV output layout of the other depth, any for 20 bits, an unknown one
    for par, layout_out in (((24, 16, 2, 0, 0), 2), ((24, 24, 2, 0, 0), 3), ((16, 16, 0, 0, 0), 2), ((24, 20, 2, 0, 0), 2),
                            ((24, 20, 2, 0, 0), 3), ((24, 16, 2, 0, 0), 4)):
        assert call(par=par, layout_out=layout_out) == EINVAL, (par, layout_out)
    for null in (0, 2, 3, 5, 8, 10, 11):
        assert call(null=null) == EINVAL, null
    assert call(work_words=words - 1) == EINVAL
    huge = 1 << 43
    assert call(total=huge, work_words=L.dvda_pcm_hip_requantize_workspace_words(n, huge)) == ECAPACITY
    rep = (hd.RequantReport * 1)()
    q = hd.Requant(24, 16, 2, 0, 0)
    assert L.dvda_mlp_hip_pcm_requantize(None, p, p, p, ctypes.byref(q), None, rep, 1, None) == EINVAL
    import torch
    if not torch.cuda.is_available():
        # what is legal reaches the device question: d_frame0 may be NULL, the WAV outputs of the right depth
        assert call() == ENODEV and call(null=6) == ENODEV
        assert call(par=(24, 16, 2, 0, 0), layout_out=3) == ENODEV and call(par=(24, 24, 0, 0, 5), layout_out=2) == ENODEV
        assert call(par=(20, 20, 1, 0, 0), layout_in=1, layout_out=0) == ENODEV
        with pytest.raises(hd.HipError):
            hd.pcm_requantize(torch.zeros(4, dtype=torch.int32), 0, [(0, 4, 4, 1)], 24, 16)


def test_symbols_are_declared_and_exported(pkg):
    hd = pkg.hipdec
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    L = hd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hd.EXPORTS and getattr(L, name) is not None
    for const in ("DVDA_RQ_TRUNCATE", "DVDA_RQ_ROUND", "DVDA_RQ_TPDF", "dvda_pcm_requant_report", "noise shaping"):
        assert const in text
