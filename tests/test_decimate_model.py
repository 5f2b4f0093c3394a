"""CPU tests of the decimation (csrc/pcm_decim.h): the committed tap tables' properties and their frequency response,
the recipe against the committed integers, the two forms of tests/decimate_model.py against each other, the library's
host arithmetic against the model, the entry points without a GPU, the structs and the symbols."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import decimate_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY, ENODEV = -3, -4, -1
SYMBOLS = ("dvda_pcm_hip_decimate", "dvda_pcm_hip_decimate_workspace_words", "dvda_mlp_hip_pcm_decimate",
           "dvda_pcm_hip_decim_taps", "dvda_pcm_hip_decim_out_frames", "dvda_pcm_hip_decim_value")
SUM_ABS = {2: 2122621608, 4: 2352308816}        # what the header states


def taps_of(pkg, ratio):
    return [int(v) for v in pkg.hipdec.decim_taps(ratio)]


def tap_tool():
    spec = importlib.util.spec_from_file_location("make_decim_taps", os.path.join(ROOT, "tools", "make_decim_taps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("ratio", dm.RATIOS)
def test_tap_table(pkg, ratio):
    t = taps_of(pkg, ratio)
    N, H = dm.n_taps(ratio), dm.half(ratio)
    assert len(t) == N == {2: 191, 4: 383}[ratio] and H == (N - 1) // 2 == {2: 95, 4: 191}[ratio]
    assert t == t[::-1]
    assert sum(t) == 1 << 30
    assert all(t[H + k] == 0 for k in range(-H, H + 1) if k and k % ratio == 0)
    assert all(t[H + k] != 0 for k in range(-H, H + 1) if k % ratio)     # (the kernel's multiply count: every other tap works)
    assert all(-2 ** 31 <= v < 2 ** 31 for v in t)
    assert sum(abs(v) for v in t) == SUM_ABS[ratio]
    assert sum(abs(v) for v in t) * 2 ** 31 + 2 ** 29 < 2 ** 63
    hd = pkg.hipdec
    n = ctypes.c_uint32(7)
    assert not hd.lib().dvda_pcm_hip_decim_taps(3, ctypes.byref(n)) and n.value == 0
    assert hd.lib().dvda_pcm_hip_decim_taps(ratio, None)
    with pytest.raises(hd.HipError):
        hd.decim_taps(8)


@pytest.mark.parametrize("ratio", dm.RATIOS)
def test_frequency_response_of_the_committed_integers(pkg, ratio):
    h = np.array(taps_of(pkg, ratio), np.float64) / 2.0 ** 30
    points = 1 << 16
    mag = np.abs(np.fft.rfft(h, 2 * points))
    f = np.arange(points + 1) / (2.0 * points) * ratio          # in units of fs_out; the input Nyquist is ratio / 2
    db = 20.0 * np.log10(np.maximum(mag, 1e-300))
    ripple = np.abs(db[f <= 0.4535]).max()
    stop = db[f >= 0.5465].max()
    print("ratio %d: passband within +-%.3g dB, stopband %.2f dB" % (ratio, ripple, stop))
    assert f[-1] == ratio / 2
    assert ripple <= 1e-4
    assert stop <= -110.0
    assert mag[0] == 1.0                                        # the gain at DC is exactly 1


@pytest.mark.parametrize("ratio", dm.RATIOS)
def test_recipe_reproduces_the_table(pkg, ratio):
    tool = tap_tool()
    made = tool.make(ratio)
    t = taps_of(pkg, ratio)
    assert len(made) == len(t) and sum(made) == 1 << 30
    assert max(abs(a - b) for a, b in zip(made, t)) <= 1
    # the header is that tool's text with the committed integers in it
    text = open(os.path.join(ROOT, "libdvd-audio_amd", "csrc", "pcm_decim_taps.h")).read()
    body = text[text.index("Taps<%du>" % ratio):]
    body = body[body.index("{", body.index("h[%d]" % len(t))) + 1:body.index("};")]
    assert [int(v) for v in body.replace(",", " ").split()] == t


def test_out_frames(pkg):
    hd = pkg.hipdec
    for ratio in dm.RATIOS:
        for frame0 in range(10):
            for own in range(10):
                want = len([m for m in range(64) if frame0 <= ratio * m < frame0 + own])
                assert dm.out_frames(frame0, own, ratio) == want
                assert hd.decim_out_frames(frame0, own, ratio) == want, (frame0, own, ratio)
        for frame0, own in ((2 ** 40 - 3, 2 ** 40), (2 ** 62, 2 ** 40), (2 ** 61 + 1, 2 ** 62)):
            assert hd.decim_out_frames(frame0, own, ratio) == dm.out_frames(frame0, own, ratio)
        # a track of F frames gives ceil(F / D)
        for F in (0, 1, 2, 3, 4, 5, 1000, 1001, 1002, 1003):
            assert hd.decim_out_frames(0, F, ratio) == -(-F // ratio)
    assert hd.decim_out_frames(0, 100, 3) == 0 and hd.decim_out_frames(0, 100, 0) == 0 and hd.decim_out_frames(0, 100, 8) == 0
    assert hd.decim_out_frames(2 ** 62 + 1, 100, 2) == 0 and hd.decim_out_frames(0, 2 ** 62 + 1, 2) == 0


@pytest.mark.parametrize("ratio", dm.RATIOS)
def test_library_value_is_the_model(pkg, ratio):
    hd = pkg.hipdec
    t = taps_of(pkg, ratio)
    N, H = len(t), dm.half(ratio)
    rng = np.random.default_rng(ratio)
    for bits in dm.DEPTHS:
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        for _ in range(40):
            w = rng.integers(-2 ** 31, 2 ** 31, N, dtype=np.int64)
            assert hd.decim_value(w, ratio, bits) == dm.value(w, t, bits)
            w >>= 32 - bits + 1                                  # inside the range: does not clip
            got = hd.decim_value(w, ratio, bits)
            assert got == dm.value(w, t, bits) and got[1] == 0
        # the rails of int32: no overflow, and the clamp
        for fill, want in ((-2 ** 31, lo), (2 ** 31 - 1, hi)):
            w = np.full(N, fill, np.int64)
            assert hd.decim_value(w, ratio, bits) == dm.value(w, t, bits) == (want, 1)
        # ... with the signs of the taps, the largest accumulator there is
        for sign in (1, -1):
            w = np.where(np.array(t) * sign >= 0, 2 ** 31 - 1, -2 ** 31)
            assert hd.decim_value(w, ratio, bits) == dm.value(w, t, bits) == ((hi, 1) if sign > 0 else (lo, 1))
        # a constant inside the range comes back exactly
        for v in (0, 1, -1, hi, lo, 12345 % hi, -(54321 % hi)):
            assert hd.decim_value(np.full(N, v, np.int64), ratio, bits) == (v, 0)
    # an impulse at every window position reads the table back (2^30 x / 2^30, no rounding)
    for j in range(N):
        w = np.zeros(N, np.int64)
        w[j] = 1 << 20
        want = (t[j] * (1 << 20) + (1 << 29)) >> 30
        assert hd.decim_value(w, ratio, 24) == (want, 0) == dm.value(w, t, 24), j
        w[j] = -(1 << 30)
        assert hd.decim_value(w, ratio, 24) == dm.value(w, t, 24), j
    L = hd.lib()
    w = np.ascontiguousarray(np.full(N, 77), np.int32)
    assert L.dvda_pcm_hip_decim_value(w.ctypes.data, ratio, 16, None) == 77
    for bad_ratio, bad_bits in ((3, 16), (0, 16), (ratio, 12), (ratio, 32), (ratio, 0)):
        cl = ctypes.c_int(5)
        assert L.dvda_pcm_hip_decim_value(w.ctypes.data, bad_ratio, bad_bits, ctypes.byref(cl)) == 0 and cl.value == -1
    cl = ctypes.c_int(5)
    assert L.dvda_pcm_hip_decim_value(None, ratio, 16, ctypes.byref(cl)) == 0 and cl.value == -1
    with pytest.raises(hd.HipError):
        hd.decim_value(np.zeros(N + 1, np.int32), ratio, 16)
    with pytest.raises(hd.HipError):
        hd.decim_value(np.zeros(N, np.int32), ratio, 18)


@pytest.mark.parametrize("ratio", dm.RATIOS)
def test_numpy_form_is_the_integer_form(pkg, ratio):
    t = taps_of(pkg, ratio)
    H = dm.half(ratio)
    rng = np.random.default_rng(10 + ratio)
    for frames in (0, 1, ratio - 1, ratio, H, H + 1, 2 * H + 1, 2 * H + 40):
        pcm = rng.integers(-2 ** 31, 2 ** 31, (2, frames), dtype=np.int64).astype(np.int32)
        pcm[1] >>= 9
        for bits in (16, 24):
            a, ca = dm.decimate(pcm, t, ratio, bits)
            b, cb = dm.decimate_np(pcm, t, ratio, bits)
            assert a.shape == (2, -(-frames // ratio)) and np.array_equal(a, b) and ca == cb
    # pieces: any frame0 and context
    track = (rng.integers(-2 ** 31, 2 ** 31, (2, 700), dtype=np.int64) >> 8).astype(np.int32)
    for a, b, cb_, ca_ in ((0, 333, 0, 10), (333, 335, 50, 1000), (335, 700, 400, 0), (5, 5, 3, 3), (7, 9, 1000, 1000)):
        region, frame0, before, after = dm.cut(track, a, b, cb_, ca_)
        x, cx = dm.decimate(region, t, ratio, 24, frame0, before, after)
        y, cy = dm.decimate_np(region, t, ratio, 24, frame0, before, after)
        assert x.shape[1] == dm.out_frames(a, b - a, ratio) and np.array_equal(x, y) and cx == cy


@pytest.mark.parametrize("ratio", dm.RATIOS)
def test_piece_invariance_of_the_model(pkg, ratio):
    t = taps_of(pkg, ratio)
    H = dm.half(ratio)
    rng = np.random.default_rng(20 + ratio)
    track = rng.integers(-2 ** 23, 2 ** 23, (3, 3001), dtype=np.int64).astype(np.int32)
    track[0] = np.where((np.arange(3001) // 7) % 2, 2 ** 23 - 1, -2 ** 23)       # rails in runs: overshoot
    whole, cw = dm.decimate_np(track, t, ratio, 24)
    assert cw[0] > 0
    cuts = (0, 1001, 2003, 3001)                  # no multiples of 2 or 4
    for context in (H, H + 77, 10 ** 6):
        parts, total = [], dm.report(0, 0, [0] * 8)
        for a, b in zip(cuts, cuts[1:]):
            region, frame0, before, after = dm.cut(track, a, b, context, context)
            y, cl = dm.decimate_np(region, t, ratio, 24, frame0, before, after)
            parts.append(y)
            total = dm.add_reports(total, dm.report(b - a, y.shape[1], cl))
        assert np.array_equal(np.concatenate(parts, 1), whole)
        assert total == dm.report(3001, whole.shape[1], cw)
    # less than H of context away from the track's ends is another signal: zeros where the context was cut
    # (half of H: the outermost taps are a few units of 2^-30, and the first centre may lie D - 1 frames inside the piece)
    region, frame0, before, after = dm.cut(track, 1001, 2003, H // 2, H // 2)
    y, _ = dm.decimate_np(region, t, ratio, 24, frame0, before, after)
    m0 = -(-1001 // ratio)
    assert not np.array_equal(y, whole[:, m0:m0 + y.shape[1]])
    holed = track.copy()
    holed[:, :1001 - H // 2] = 0
    holed[:, 2003 + H // 2:] = 0
    assert np.array_equal(y, dm.decimate_np(holed, t, ratio, 24)[0][:, m0:m0 + y.shape[1]])


def test_structs_and_constants(pkg):
    hd = pkg.hipdec
    assert ctypes.sizeof(hd.DecimPiece) == 16 and ctypes.sizeof(hd.DecimReport) == 80
    assert dm.TILE == hd.DCM_TILE_FRAMES
    r = hd.DecimReport.from_dict(dm.report(9, 5, range(8)))
    assert r.as_dict() == dict(frames_in=9, frames_out=5, clipped=list(range(8)))
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    assert re.search(r"#define DVDA_DCM_TILE_FRAMES %du" % dm.TILE, text)


def test_arguments_are_judged_before_the_device(pkg):
    """every DVDA_HIP_EINVAL of the contract, with or without a device; then DVDA_HIP_ECAPACITY; then -- on a machine
    without one -- DVDA_HIP_ENODEV"""
    hd = pkg.hipdec
    L = hd.lib()
    n, bound = 3, 1 << 20
    words = L.dvda_pcm_hip_decimate_workspace_words(n, bound)
    assert words >= 2 * (n + 1) + (bound // dm.TILE + n) * 8
    last = 0
    for k in (0, 1, 2, 100):
        for total in (0, 1, dm.TILE, 10 * dm.TILE + 1, 1 << 30):
            w = L.dvda_pcm_hip_decimate_workspace_words(k, total)
            assert w >= last and w <= L.dvda_pcm_hip_decimate_workspace_words(k + 1, total)
            last = w
        last = L.dvda_pcm_hip_decimate_workspace_words(k, 0)
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data

    def call(ratio=2, bits=24, layout_in=0, layout_out=0, work_words=words, null=None, total=bound):
        args = [p, layout_in, p, p, layout_out, p, p, n, ratio, bits, total, p, p, work_words, None]
        if null is not None:
            args[null] = None
        return L.dvda_pcm_hip_decimate(*args)

    for ratio in (0, 1, 3, 5, 8, 0xFFFFFFFF):
        assert call(ratio=ratio) == EINVAL, ratio
    for bits in (0, 8, 12, 18, 32):
        assert call(bits=bits) == EINVAL, bits
    for layout in (2, 3, 4):
        assert call(layout_in=layout) == EINVAL and call(layout_out=layout) == EINVAL
    for null in (0, 2, 3, 5, 11, 12):
        assert call(null=null) == EINVAL, null
    assert call(work_words=words - 1) == EINVAL
    huge = 1 << 42
    assert call(total=huge, work_words=L.dvda_pcm_hip_decimate_workspace_words(n, huge)) == ECAPACITY
    rep = (hd.DecimReport * 1)()
    arr = (ctypes.c_uint64 * 1)(0)
    assert L.dvda_mlp_hip_pcm_decimate(None, p, p, p, 2, 24, p, 0, arr, arr, rep, 1, None) == EINVAL
    import torch
    if not torch.cuda.is_available():
        # what is legal reaches the device question: d_piece may be NULL, every pair of int32 layouts, both ratios
        assert call() == ENODEV and call(null=6) == ENODEV
        for ratio in (2, 4):
            for bits in (16, 20, 24):
                for li in (0, 1):
                    for lo in (0, 1):
                        assert call(ratio=ratio, bits=bits, layout_in=li, layout_out=lo) == ENODEV
        with pytest.raises(hd.HipError):
            hd.pcm_decimate(torch.zeros(4, dtype=torch.int32), 0, [(0, 4, 4, 1)], 2, 24)


def test_symbols_are_declared_and_exported(pkg):
    hd = pkg.hipdec
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    L = hd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hd.EXPORTS and getattr(L, name) is not None
    for const in ("dvda_pcm_decim_piece", "dvda_pcm_decim_report", "DVDA_DCM_TILE_FRAMES", "2 122 621 608", "2 352 308 816",
                  "5.2e18 < 2^63"):
        assert const in text
