"""CPU tests of the level report (csrc/pcm_levels.h): its decomposition restated in numpy (tests/levels_model.py)
against the definition, the library's host arithmetic, the entry point without a GPU, and the kernels' ISA."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import levels_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lm.TILE


def mixed_pcm(rng, ch, frames, bits):
    """full int32 range with a block inside the nominal range: `over` is neither 0 nor everything"""
    pcm = rng.integers(-2 ** 31, 2 ** 31, (ch, frames), dtype=np.int64)
    a, b = frames // 4, frames - frames // 4
    pcm[:, a:b] = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (ch, b - a), dtype=np.int64)
    return pcm.astype(np.int32)


def test_constants_agree(pkg):
    assert T == pkg.hipdec.LVL_TILE_FRAMES and T % 4 == 0
    assert ctypes.sizeof(pkg.hipdec.Levels) == 24 + 8 * (8 + 8 + 4 + 4)


@pytest.mark.parametrize("bits", [16, 20, 24])
@pytest.mark.parametrize("frames", [0, 1, T - 1, T, T + 1, 3 * T + 7])
def test_decomposition_is_the_definition(frames, bits):
    rng = np.random.default_rng(frames + bits)
    for ch in (1, 2, 6):
        pcm = mixed_pcm(rng, ch, frames, bits)
        want = lm.levels(pcm, bits)
        assert lm.levels_by_tiles(pcm, bits) == want
        if frames > 8:
            assert 0 < want["over"][0] < frames and want["lead_silent"] == 0
        # silence at both ends, across tile edges
        for lead, trail in ((frames, frames), (min(frames, T), 0), (0, min(frames, T + 3)), (frames // 3, frames // 2)):
            q = pcm.copy()
            q[:, :lead] = 0
            q[:, frames - trail:] = 0
            assert lm.levels_by_tiles(q, bits) == lm.levels(q, bits)


def test_definition_on_known_values():
    pcm = np.array([[0, 0, 5, -7, 0], [0, 0, 0, 1 << 23, 0]], np.int32)
    got = lm.levels(pcm, 24)
    assert (got["frames"], got["lead_silent"], got["trail_silent"]) == (5, 2, 1)
    assert got["sum"][:2] == [-2, 1 << 23] and got["over"][:2] == [0, 1]
    assert got["min"][:2] == [-7, 0] and got["max"][:2] == [5, 1 << 23]
    assert got["sum"][2:] == [0] * 6 and got["min"][2:] == [0] * 6
    zeros = lm.levels(np.zeros((3, 9), np.int32), 16)
    assert zeros["lead_silent"] == zeros["trail_silent"] == zeros["frames"] == 9
    assert lm.levels(np.zeros((3, 0), np.int32), 16) == lm.zero()


def test_combine_from_the_library(pkg):
    """random splits, empty operands, all-silent operands on either side -- and the report of the whole"""
    rng = np.random.default_rng(2025)
    comb = pkg.hipdec.levels_combine
    for k in range(120):
        ch, bits = int(rng.integers(1, 7)), (16, 20, 24)[k % 3]
        na = 0 if k % 10 == 0 else int(rng.integers(1, 300))
        nb = 0 if k % 15 == 0 else int(rng.integers(1, 300))
        a, b = mixed_pcm(rng, ch, na, bits), mixed_pcm(rng, ch, nb, bits)
        if k % 4 == 1:
            a[:] = 0
        if k % 4 == 2:
            b[:] = 0
        if k % 7 == 3:
            a[:, :na // 2] = 0
            b[:, nb // 2:] = 0
        if k % 9 == 4:          # all values positive / negative on one side: a neutral operand's zeros would show
            a, b = np.abs(a // 2) + 1, -np.abs(b // 2) - 1
        la, lb = lm.levels(a, bits), lm.levels(b, bits)
        want = lm.levels(np.concatenate([a, b], axis=1), bits)
        assert lm.combine(la, lb) == want, k
        assert comb(la, lb) == want, k


def test_combine_may_alias_its_output(pkg):
    hd = pkg.hipdec
    L = hd.lib()
    rng = np.random.default_rng(5)
    a, b = mixed_pcm(rng, 3, 40, 16), mixed_pcm(rng, 3, 25, 16)
    la, lb = lm.levels(a, 16), lm.levels(b, 16)
    want = lm.levels(np.concatenate([a, b], axis=1), 16)
    for alias in ("a", "b"):
        sa, sb = hd.Levels.from_dict(la), hd.Levels.from_dict(lb)
        out = sa if alias == "a" else sb
        L.dvda_pcm_hip_levels_combine(ctypes.byref(sa), ctypes.byref(sb), ctypes.byref(out))
        assert out.as_dict() == want
    # ... and with an empty operand
    sa, sb = hd.Levels.from_dict(lm.zero()), hd.Levels.from_dict(lb)
    L.dvda_pcm_hip_levels_combine(ctypes.byref(sa), ctypes.byref(sb), ctypes.byref(sa))
    assert sa.as_dict() == lb


def test_arguments_are_judged_before_the_device(pkg):
    """DVDA_HIP_EINVAL for bad bits, a WAV layout, a null pointer, a workspace too small -- with or without a device"""
    L = pkg.hipdec.lib()
    n, bound = 3, 1 << 20
    words = L.dvda_pcm_hip_levels_workspace_words(n, bound)
    assert words >= 2 * (n + 1) + (bound // T + n) * 42
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data
    EINVAL = -3
    for bits in (0, 8, 17, 32):
        assert L.dvda_pcm_hip_levels(p, 0, bits, p, n, bound, p, p, words, None) == EINVAL
    for layout in (2, 3, 4):
        assert L.dvda_pcm_hip_levels(p, layout, 24, p, n, bound, p, p, words, None) == EINVAL
    for null in range(4):
        args = [p, 0, 24, p, n, bound, p, p, words, None]
        args[(0, 3, 6, 7)[null]] = None
        assert L.dvda_pcm_hip_levels(*args) == EINVAL
    assert L.dvda_pcm_hip_levels(p, 1, 16, p, n, bound, p, p, words - 1, None) == EINVAL
    assert L.dvda_mlp_hip_pcm_levels(None, p, p, p, 24, None, 1, None) == EINVAL


def test_no_device_is_an_error(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pkg.hipdec.lib()
    n, bound = 1, 1 << 20
    words = L.dvda_pcm_hip_levels_workspace_words(n, bound)
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    for layout, bits in ((0, 24), (1, 16), (0, 20)):
        assert L.dvda_pcm_hip_levels(p, layout, bits, p, n, bound, p, p, words, None) == -1      # DVDA_HIP_ENODEV
    with pytest.raises(pkg.hipdec.HipError):
        pkg.hipdec.pcm_levels(torch.zeros(4, dtype=torch.int32), 0, 24, [(0, 4, 4, 1)])


def test_levels_kernels_use_no_scratch(tmp_path):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    lines = open(isa.compile_asm(str(tmp_path / "mlp_hip.s"))).read().split("\n")
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"(_ZN3lvl\d+k_lvl\w+):", lines[i])
        i += 1
        if not m:
            continue
        count = 0
        while not lines[i].startswith(".Lfunc_end"):
            count += bool(re.match(r"\s+scratch_", lines[i]))
            i += 1
        found[m.group(1)] = count
    names = " ".join(found)
    for k in ("k_lvl_plan", "k_lvl_tilesILb0E", "k_lvl_tilesILb1E", "k_lvl_join"):
        assert k in names, (k, names)
    assert all(v == 0 for v in found.values()), found
