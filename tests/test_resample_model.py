"""CPU tests of the 48 kHz -> 44.1 kHz resampler (csrc/pcm_resample.h): the committed table's properties and its
frequency response, the recipe against the committed integers, the two forms of tests/resample_model.py against each
other, the library's host arithmetic against the model, the entry points without a GPU, the constants and the symbols."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import resample_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY, ENODEV = -3, -4, -1
SYMBOLS = ("dvda_pcm_hip_resample", "dvda_pcm_hip_resample_workspace_words", "dvda_mlp_hip_pcm_resample",
           "dvda_pcm_hip_resample_taps", "dvda_pcm_hip_resample_out_frames", "dvda_pcm_hip_resample_value")
MAX_SUM_ABS = 2561819644        # what the header states


@pytest.fixture(scope="module")
def table(pkg):
    return pkg.hipdec.resample_taps()


def tap_tool():
    spec = importlib.util.spec_from_file_location("make_resample_taps", os.path.join(ROOT, "tools", "make_resample_taps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tap_table(pkg, table):
    assert table.shape == (147, 96) == (rm.UP, rm.TAPS) and table.dtype == np.int32
    g = [[int(v) for v in row] for row in table]
    assert all(sum(row) == 1 << 30 for row in g)                # DC gain exactly 1 at every output frame
    assert all(g[147 - p][i] == g[p][95 - i] for p in range(1, 147) for i in range(96))
    sum_abs = max(sum(abs(v) for v in row) for row in g)
    assert sum_abs == MAX_SUM_ABS and sum_abs < 2 ** 32
    assert sum_abs * 2 ** 31 + 2 ** 29 < 2 ** 63
    # phase 0 is a frame of the input: its largest tap is the one at q
    assert max(range(96), key=lambda i: g[0][i]) == rm.FRONT
    L = pkg.hipdec.lib()
    ph, tp = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert L.dvda_pcm_hip_resample_taps(ctypes.byref(ph), ctypes.byref(tp)) and (ph.value, tp.value) == (147, 96)
    assert L.dvda_pcm_hip_resample_taps(None, None)


def test_frequency_response_of_the_committed_integers(table):
    """the whole 147-times oversampled prototype the phases are cut from, images included"""
    g = table.astype(np.float64) / 2.0 ** 30
    proto = np.zeros(147 * 97)
    for p in range(147):
        proto[147 * (np.arange(96) + 1) - p] = g[p]             # time (i - 47 - p / 147) input samples, shifted
    points = 1 << 20
    mag = np.abs(np.fft.rfft(proto, 2 * points)) / 147.0
    f = np.arange(points + 1) / (2.0 * points) * 160.0          # in units of fs_out: the prototype runs at 160 fs_out
    db = 20.0 * np.log10(np.maximum(mag, 1e-300))
    ripple = np.abs(db[f <= 0.4535]).max()
    stop = db[f >= 0.5465].max()
    print("passband within +-%.3g dB, stopband %.2f dB" % (ripple, stop))
    assert f[-1] == 80.0
    assert ripple <= 2e-5
    assert stop <= -117.0
    assert abs(mag[0] - 1.0) < 1e-12


def test_recipe_reproduces_the_table(table):
    tool = tap_tool()
    made = tool.make()
    assert len(made) == 147 and all(len(r) == 96 and sum(r) == 1 << 30 for r in made)
    assert max(abs(a - int(b)) for ra, rb in zip(made, table) for a, b in zip(ra, rb)) <= 1
    # the header is that tool's text with the committed integers in it
    text = open(os.path.join(ROOT, "libdvd-audio_amd", "csrc", "pcm_resample_taps.h")).read()
    body = text[text.index("g[PHASES][TAPS]"):]
    body = re.sub(r"//[^\n]*", "", body[body.index("{") + 1:body.index("};")])
    assert [int(v) for v in re.findall(r"-?\d+", body)] == [int(v) for v in table.reshape(-1)]


def test_out_frames(pkg):
    hd = pkg.hipdec
    for frame0 in list(range(0, 330, 7)) + [159, 160, 161, 320]:
        for own in list(range(0, 12)) + [47, 48, 95, 96, 159, 160, 161, 320, 321]:
            want = rm.out_frames_brute(frame0, own)
            assert rm.out_frames(frame0, own) == want, (frame0, own)
            assert hd.resample_out_frames(frame0, own) == want, (frame0, own)
    for frame0, own in ((2 ** 40 - 3, 2 ** 40), (2 ** 62, 2 ** 40), (2 ** 61 + 1, 2 ** 62), (2 ** 62 - 1, 2 ** 62)):
        assert hd.resample_out_frames(frame0, own) == rm.out_frames(frame0, own)
    # a track of F frames gives ceil(147 F / 160)
    for F in (0, 1, 2, 3, 159, 160, 161, 1000, 48000, 48001, 10 ** 9 + 7):
        assert hd.resample_out_frames(0, F) == -(-147 * F // 160)
    assert hd.resample_out_frames(0, 48000) == 44100
    assert hd.resample_out_frames(2 ** 62 + 1, 100) == 0 and hd.resample_out_frames(0, 2 ** 62 + 1) == 0
    # the pieces of random cuts add up to the whole
    rng = np.random.default_rng(5)
    for _ in range(200):
        F = int(rng.integers(0, 5000))
        cuts = [0] + sorted(int(v) for v in rng.integers(0, F + 1, int(rng.integers(0, 6)))) + [F]
        parts = [hd.resample_out_frames(a, b - a) for a, b in zip(cuts, cuts[1:])]
        assert parts == [rm.out_frames_brute(a, b - a) for a, b in zip(cuts, cuts[1:])]
        assert sum(parts) == -(-147 * F // 160)


def test_library_value_is_the_model(pkg, table):
    hd = pkg.hipdec
    rng = np.random.default_rng(3)
    N = rm.TAPS
    for bits in rm.DEPTHS:
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        for phase in range(147):
            row = table[phase]
            w = rng.integers(-2 ** 31, 2 ** 31, N, dtype=np.int64)
            assert hd.resample_value(w, phase, bits) == rm.value(w, row, bits)
            w >>= 32 - bits + 3                                  # inside the range: does not clip (sum |g| < 2.4 * 2^30)
            got = hd.resample_value(w, phase, bits)
            assert got == rm.value(w, row, bits) and got[1] == 0
            # the rails of int32: no overflow, and the clamp
            for fill, want in ((-2 ** 31, lo), (2 ** 31 - 1, hi)):
                w = np.full(N, fill, np.int64)
                assert hd.resample_value(w, phase, bits) == rm.value(w, row, bits) == (want, 1)
            # ... with the signs of the taps, the largest accumulator there is
            for sign in (1, -1):
                w = np.where(row.astype(np.int64) * sign >= 0, 2 ** 31 - 1, -2 ** 31)
                assert hd.resample_value(w, phase, bits) == rm.value(w, row, bits) == ((hi, 1) if sign > 0 else (lo, 1))
            # a constant inside the range comes back exactly: every phase sums to 2^30
            for v in (0, 1, -1, hi, lo, 12345 % hi):
                assert hd.resample_value(np.full(N, v, np.int64), phase, bits) == (v, 0)
    # an impulse at every window position of every phase reads the table back
    for phase in range(147):
        for j in range(N):
            w = np.zeros(N, np.int64)
            w[j] = 1 << 20
            want = (int(table[phase][j]) * (1 << 20) + (1 << 29)) >> 30
            assert hd.resample_value(w, phase, 24) == (want, 0), (phase, j)
    L = hd.lib()
    w = np.ascontiguousarray(np.full(N, 77), np.int32)
    assert L.dvda_pcm_hip_resample_value(w.ctypes.data, 5, 16, None) == 77
    for bad_phase, bad_bits in ((147, 16), (0xFFFFFFFF, 16), (0, 12), (0, 32), (0, 0)):
        cl = ctypes.c_int(5)
        assert L.dvda_pcm_hip_resample_value(w.ctypes.data, bad_phase, bad_bits, ctypes.byref(cl)) == 0 and cl.value == -1
    cl = ctypes.c_int(5)
    assert L.dvda_pcm_hip_resample_value(None, 0, 16, ctypes.byref(cl)) == 0 and cl.value == -1
    with pytest.raises(hd.HipError):
        hd.resample_value(np.zeros(N + 1, np.int32), 0, 16)
    with pytest.raises(hd.HipError):
        hd.resample_value(np.zeros(N, np.int32), 0, 18)
    with pytest.raises(hd.HipError):
        hd.resample_value(np.zeros(N, np.int32), 147, 16)


def test_numpy_form_is_the_integer_form(table):
    rng = np.random.default_rng(11)
    for frames in (0, 1, 47, 48, 49, 95, 96, 97, 159, 160, 161, 320, 500):
        pcm = rng.integers(-2 ** 31, 2 ** 31, (2, frames), dtype=np.int64).astype(np.int32)
        pcm[1] >>= 9
        for bits in (16, 24):
            a, ca = rm.resample(pcm, table, bits)
            b, cb = rm.resample_np(pcm, table, bits)
            assert a.shape == (2, -(-147 * frames // 160)) and np.array_equal(a, b) and ca == cb
    # pieces: any frame0 and context
    track = (rng.integers(-2 ** 31, 2 ** 31, (2, 700), dtype=np.int64) >> 8).astype(np.int32)
    for a, b, cb_, ca_ in ((0, 333, 0, 10), (333, 335, 50, 1000), (335, 700, 400, 0), (5, 5, 3, 3), (7, 9, 1000, 1000)):
        region, frame0, before, after = rm.cut(track, a, b, cb_, ca_)
        x, cx = rm.resample(region, table, 24, frame0, before, after)
        y, cy = rm.resample_np(region, table, 24, frame0, before, after)
        assert x.shape[1] == rm.out_frames(a, b - a) and np.array_equal(x, y) and cx == cy


def test_piece_invariance_of_the_model(table):
    rng = np.random.default_rng(21)
    track = rng.integers(-2 ** 23, 2 ** 23, (3, 3001), dtype=np.int64).astype(np.int32)
    track[0] = np.where((np.arange(3001) // 7) % 2, 2 ** 23 - 1, -2 ** 23)       # rails in runs: overshoot
    whole, cw = rm.resample_np(track, table, 24)
    assert cw[0] > 0 and whole.shape[1] == -(-147 * 3001 // 160)
    cuts = (0, 1001, 2003, 3001)
    for context in (48, 48 + 77, 10 ** 6):
        parts, total = [], rm.report(0, 0, [0] * 8)
        for a, b in zip(cuts, cuts[1:]):
            region, frame0, before, after = rm.cut(track, a, b, context, context)
            y, cl = rm.resample_np(region, table, 24, frame0, before, after)
            parts.append(y)
            total = rm.add_reports(total, rm.report(b - a, y.shape[1], cl))
        assert np.array_equal(np.concatenate(parts, 1), whole)
        assert total == rm.report(3001, whole.shape[1], cw)
    # less context is another signal: zeros where the context was cut
    region, frame0, before, after = rm.cut(track, 1001, 2003, 24, 24)
    y, _ = rm.resample_np(region, table, 24, frame0, before, after)
    m0 = rm.first_out(1001)
    assert not np.array_equal(y, whole[:, m0:m0 + y.shape[1]])
    holed = track.copy()
    holed[:, :1001 - 24] = 0
    holed[:, 2003 + 24:] = 0
    assert np.array_equal(y, rm.resample_np(holed, table, 24)[0][:, m0:m0 + y.shape[1]])


def test_constants(pkg):
    hd = pkg.hipdec
    assert rm.TILE == hd.RSM_TILE_FRAMES == 64 * 147 and (hd.RSM_PHASES, hd.RSM_TAPS) == (rm.UP, rm.TAPS)
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    assert re.search(r"#define DVDA_RSM_TILE_FRAMES %du" % rm.TILE, text)


def test_arguments_are_judged_before_the_device(pkg):
    """every DVDA_HIP_EINVAL of the contract, with or without a device; then DVDA_HIP_ECAPACITY; then -- on a machine
    without one -- DVDA_HIP_ENODEV"""
    hd = pkg.hipdec
    L = hd.lib()
    n, bound = 3, 1 << 20
    words = L.dvda_pcm_hip_resample_workspace_words(n, bound)
    assert words >= 2 * (n + 1) + (bound // rm.TILE + n) * 8
    last = 0
    for k in (0, 1, 2, 100):
        for total in (0, 1, rm.TILE, 10 * rm.TILE + 1, 1 << 30):
            w = L.dvda_pcm_hip_resample_workspace_words(k, total)
            assert w >= last and w <= L.dvda_pcm_hip_resample_workspace_words(k + 1, total)
            last = w
        last = L.dvda_pcm_hip_resample_workspace_words(k, 0)
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data

    def call(bits=24, layout_in=0, layout_out=0, work_words=words, null=None, total=bound):
        args = [p, layout_in, p, p, layout_out, p, p, n, bits, total, p, p, work_words, None]
        if null is not None:
            args[null] = None
        return L.dvda_pcm_hip_resample(*args)

    for bits in (0, 8, 12, 18, 32):
        assert call(bits=bits) == EINVAL, bits
    for layout in (2, 3, 4):
        assert call(layout_in=layout) == EINVAL and call(layout_out=layout) == EINVAL
    for null in (0, 2, 3, 5, 10, 11):
        assert call(null=null) == EINVAL, null
    assert call(work_words=words - 1) == EINVAL
    huge = 1 << 46
    assert call(total=huge, work_words=L.dvda_pcm_hip_resample_workspace_words(n, huge)) == ECAPACITY
    rep = (hd.DecimReport * 1)()
    arr = (ctypes.c_uint64 * 1)(0)
    assert L.dvda_mlp_hip_pcm_resample(None, p, p, p, 24, p, 0, arr, arr, rep, 1, None) == EINVAL
    import torch
    if not torch.cuda.is_available():
        # what is legal reaches the device question: d_piece may be NULL, every pair of int32 layouts
        assert call() == ENODEV and call(null=6) == ENODEV
        for bits in (16, 20, 24):
            for li in (0, 1):
                for lo in (0, 1):
                    assert call(bits=bits, layout_in=li, layout_out=lo) == ENODEV
        with pytest.raises(hd.HipError):
            hd.pcm_resample(torch.zeros(4, dtype=torch.int32), 0, [(0, 4, 4, 1)], 24)
    with pytest.raises(ValueError):
        hd.decode_streams_resampled([], rate=48000)


def test_symbols_are_declared_and_exported(pkg):
    hd = pkg.hipdec
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    L = hd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hd.EXPORTS and getattr(L, name) is not None
    for const in ("DVDA_RSM_TILE_FRAMES", "2 561 819 644", "g[147 - p][i] == g[p][95 - i]", "-118.2 dB"):
        assert const in text
