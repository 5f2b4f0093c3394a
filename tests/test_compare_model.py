"""CPU tests of the compare of two PCM buffers (csrc/pcm_compare.h): its decomposition restated in numpy
(tests/compare_model.py) against the definition, the library's host arithmetic, the entry points without a GPU, and the
kernels' ISA."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import compare_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = cm.TILE
EINVAL, ENODEV = -3, -1


def pair(rng, ch, fa, fb, share=0.02):
    """random int32 [ch, fa] and [ch, fb]: B is A (as far as both go) except for a `share` of the values"""
    a = rng.integers(-2 ** 31, 2 ** 31, (ch, fa), dtype=np.int64).astype(np.int32)
    b = rng.integers(-2 ** 31, 2 ** 31, (ch, fb), dtype=np.int64).astype(np.int32)
    n = min(fa, fb)
    keep = rng.random((ch, n)) >= share
    b[:, :n][keep] = a[:, :n][keep]
    return a, b


def test_constants_agree(pkg):
    hd = pkg.hipdec
    assert T == hd.CMP_TILE_FRAMES == 4096 and cm.CMP_SHAPE == hd.CMP_SHAPE == 1
    assert ctypes.sizeof(hd.Diff) == 160
    d = cm.diff(*pair(np.random.default_rng(0), 3, 50, 40, 0.5), 0)
    assert hd.Diff.from_dict(d).as_dict() == d


@pytest.mark.parametrize("bits", [0, 16, 24])
@pytest.mark.parametrize("frames", [0, 1, T - 1, T, T + 1, 3 * T + 7])
def test_decomposition_is_the_definition(frames, bits):
    rng = np.random.default_rng(frames + bits)
    for ch in (1, 2, 6):
        a, b = pair(rng, ch, frames, frames)
        want = cm.diff(a, b, bits)
        assert cm.diff_by_tiles(a, b, bits) == want
        if frames > 3 * T:
            assert 0 < want["diff_frames"] < frames and want["runs"] > 1
        # no difference at all
        same = cm.diff_by_tiles(a, a, bits)
        assert same == cm.diff(a, a, bits)
        assert (same["diff_frames"], same["runs"], same["first_diff"], same["diff_end"]) == (0, 0, frames, 0)
        # unequal lengths, both ways
        for fa, fb in ((frames, frames // 2), (frames // 3, frames)):
            assert cm.diff_by_tiles(a[:, :fa], b[:, :fb], bits) == cm.diff(a[:, :fa], b[:, :fb], bits)
        # differing frames placed: at 0, at the end, across a tile seam (one run), either side of a clean frame (two)
        for places, runs in (([0], 1), ([frames - 1], 1), ([T - 1, T], 1), ([T - 1, T + 1], 2), ([0, frames - 1], 2)):
            if not all(0 <= f < frames for f in places) or len(set(places)) != len(places):
                continue
            q = a.copy()
            q[ch - 1, places] ^= 1
            got = cm.diff_by_tiles(a, q, bits)
            assert got == cm.diff(a, q, bits)
            assert (got["runs"], got["diff_frames"]) == (runs, len(places))
            assert (got["first_diff"], got["diff_end"]) == (min(places), max(places) + 1)


def test_definition_on_known_values():
    lo, hi = np.array([[-2 ** 31]], np.int32), np.array([[2 ** 31 - 1]], np.int32)
    assert cm.diff(lo, hi, 0)["max_abs"][0] == 2 ** 32 - 1 == cm.diff(hi, lo, 0)["max_abs"][0]
    for x, y in ((40000, 7232), (-40000, -7232), (5, 5 + 65536)):
        a, b = np.array([[x]], np.int32), np.array([[y]], np.int32)
        assert cm.diff(a, b, 16)["diff_frames"] == 0, (x, y)        # the same WAV sample
        assert cm.diff(a, b, 0)["diff_frames"] == 1
    # plain truncation would call 40000 (0x9C40 -> -25536 as int16) and 7232 different
    assert np.array(40000, np.int32).astype(np.int16) != 7232
    got = cm.diff(np.array([[0, 5, 5, 0, 9], [1, 1, 1, 1, 1]], np.int32), np.array([[0, 6, 1, 0, 9], [1, 1, 1, 1, 8]], np.int32), 0)
    assert (got["compared"], got["diff_frames"], got["first_diff"], got["diff_end"], got["runs"]) == (5, 3, 1, 5, 2)
    assert got["diff_values"][:3] == [2, 1, 0] and got["max_abs"][:3] == [4, 7, 0] and got["channels"] == 2
    shape = cm.diff(np.zeros((2, 4), np.int32), np.zeros((3, 4), np.int32), 0)
    assert shape["flags"] == cm.CMP_SHAPE and shape["compared"] == 0 and (shape["frames_a"], shape["frames_b"]) == (4, 4)
    assert cm.diff(np.zeros((9, 4), np.int32), np.zeros((9, 4), np.int32), 0)["frames_a"] == 0


def _lib_combine(hd, a, b, alias=None):
    """-> (rc, out as dict) through the C entry point; alias: 'a' / 'b' -- that operand is `out`"""
    sa, sb = hd.Diff.from_dict(a), hd.Diff.from_dict(b)
    out = sa if alias == "a" else sb if alias == "b" else hd.Diff.from_dict(cm.zero())
    rc = hd.lib().dvda_pcm_hip_diff_combine(ctypes.byref(sa), ctypes.byref(sb), ctypes.byref(out))
    return rc, out.as_dict()


def test_combine_from_the_library(pkg):
    """random splits, a differing frame on both sides of the seam / on one side only, empty operands, unequal second
    pieces -- against the model and against the diff of the concatenation; each operand also as `out`"""
    hd = pkg.hipdec
    rng = np.random.default_rng(2026)
    seams = 0
    for k in range(160):
        ch, bits = int(rng.integers(1, 7)), (0, 16, 20, 24)[k % 4]
        na = 0 if k % 10 == 0 else int(rng.integers(1, 300))
        nb = 0 if k % 15 == 0 else int(rng.integers(1, 300))
        extra_a, extra_b = (int(rng.integers(0, 9)), 0) if k % 3 == 0 else (0, int(rng.integers(0, 9)) if k % 3 == 1 else 0)
        a1, b1 = pair(rng, ch, na, na, 0.05)
        a2, b2 = pair(rng, ch, nb + extra_a, nb + extra_b, 0.05)
        if na and nb:
            left, right = k % 4 in (0, 1), k % 4 in (0, 2)          # the frames at the seam: differ / are equal
            b1[:, -1] = a1[:, -1]
            b2[:, 0] = a2[:, 0]
            b1[0, -1] ^= 1 if left else 0
            b2[ch - 1, 0] ^= 1 if right else 0
            seams += left and right
        da, db = cm.diff(a1, b1, bits), cm.diff(a2, b2, bits)
        want = cm.diff(np.concatenate([a1, a2], axis=1), np.concatenate([b1, b2], axis=1), bits)
        if na == 0 or (nb + extra_a == 0 and nb + extra_b == 0):    # a neutral operand: the other one, as it is
            want = db if na == 0 else da
        assert cm.combine(da, db) == want, k
        assert hd.diff_combine(da, db) == want, k
        for alias in ("a", "b"):
            assert _lib_combine(hd, da, db, alias) == (0, want), (k, alias)
    assert seams > 20


def test_combine_refuses_what_does_not_line_up(pkg):
    hd = pkg.hipdec
    rng = np.random.default_rng(3)
    a, b = pair(rng, 2, 40, 40, 0.3)
    good = cm.diff(a, b, 0)
    uneven = cm.diff(a, b[:, :30], 0)
    other_ch = cm.diff(a[:1], b[:1], 0)
    shape = cm.diff(a, b[:1], 0)
    assert shape["flags"] == cm.CMP_SHAPE and uneven["frames_a"] != uneven["frames_b"]
    marker = dict(cm.zero(), frames_a=7, frames_b=7, compared=7, first_diff=7, runs=12345, channels=2)
    for x, y in ((uneven, good), (good, other_ch), (shape, good), (good, shape), (cm.zero(), shape)):
        assert cm.combine(x, y) is None
        sa, sb, out = hd.Diff.from_dict(x), hd.Diff.from_dict(y), hd.Diff.from_dict(marker)
        assert hd.lib().dvda_pcm_hip_diff_combine(ctypes.byref(sa), ctypes.byref(sb), ctypes.byref(out)) == EINVAL
        assert out.as_dict() == marker
        with pytest.raises(hd.HipError, match="EINVAL"):
            hd.diff_combine(x, y)
    # the second piece may be uneven: it is where the longer side's tail lies
    assert hd.diff_combine(good, uneven) == cm.combine(good, uneven) == cm.diff(np.concatenate([a, a], axis=1),
                                                                                np.concatenate([b, b[:, :30]], axis=1), 0)


def _args(p, words, n=3, bound=1 << 20):
    # d_a, layout_a, d_desc_a, d_b, layout_b, d_desc_b, n, bits, max_total_frames, d_diff, d_work, work_words, stream
    return [p, 0, p, p, 1, p, n, 0, bound, p, p, words, None]


def test_arguments_are_judged_before_the_device(pkg):
    """DVDA_HIP_EINVAL for bad bits, a WAV layout on either side, a null pointer, a workspace too small -- with or without
    a device"""
    L = pkg.hipdec.lib()
    n, bound = 3, 1 << 20
    words = L.dvda_pcm_hip_compare_workspace_words(n, bound)
    assert words >= 2 * (n + 1) + (bound // T + n) * 20
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data
    for bits in (8, 17, 32):
        args = _args(p, words)
        args[7] = bits
        assert L.dvda_pcm_hip_compare(*args) == EINVAL
    for side in (1, 4):
        for layout in (2, 3, 4):
            args = _args(p, words)
            args[side] = layout
            assert L.dvda_pcm_hip_compare(*args) == EINVAL
    for null in (0, 2, 3, 5, 9, 10):
        args = _args(p, words)
        args[null] = None
        assert L.dvda_pcm_hip_compare(*args) == EINVAL
    assert L.dvda_pcm_hip_compare(*_args(p, words - 1)) == EINVAL
    assert L.dvda_pcm_hip_compare(*_args(p, 1 << 40, n=1, bound=(1 << 31) * T)) == -4        # DVDA_HIP_ECAPACITY
    assert L.dvda_mlp_hip_pcm_compare(None, p, p, p, p, 0, p, 0, None, 1, None) == EINVAL
    assert L.dvda_pcm_hip_diff_combine(None, None, None) == EINVAL


def test_no_device_is_an_error(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pkg.hipdec.lib()
    words = L.dvda_pcm_hip_compare_workspace_words(3, 1 << 20)
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    for la, lb, bits in ((0, 0, 0), (0, 1, 16), (1, 0, 20), (1, 1, 24)):
        args = _args(p, words)
        args[1], args[4], args[7] = la, lb, bits
        assert L.dvda_pcm_hip_compare(*args) == ENODEV
    with pytest.raises(pkg.hipdec.HipError):
        z = torch.zeros(4, dtype=torch.int32)
        pkg.hipdec.pcm_compare(z, 0, [(0, 4, 4, 1)], z, 1, [(0, 4, 4, 1)])


def test_compare_kernels_use_no_scratch(tmp_path):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    lines = open(isa.compile_asm(str(tmp_path / "mlp_hip.s"))).read().split("\n")
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"(_ZN3cmp\d+k_cmp\w+):", lines[i])
        i += 1
        if not m:
            continue
        count = 0
        while not lines[i].startswith(".Lfunc_end"):
            count += bool(re.match(r"\s+scratch_", lines[i]))
            i += 1
        found[m.group(1)] = count
    names = " ".join(found)
    for k in ("k_cmp_plan", "k_cmp_tilesILb0ELb0E", "k_cmp_tilesILb0ELb1E", "k_cmp_tilesILb1ELb0E", "k_cmp_tilesILb1ELb1E",
              "k_cmp_join"):
        assert k in names, (k, names)
    assert len(found) == 6 and all(v == 0 for v in found.values()), found
