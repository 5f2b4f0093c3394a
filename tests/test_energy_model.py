"""CPU tests of the energy report (csrc/pcm_energy.h): the rule restated with Python integers (tests/energy_model.py),
the library's host arithmetic against it, the entry points without a GPU, the symbols, and the kernels' ISA."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import energy_model as em
from tests import levels_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY, ENODEV = -3, -4, -1
SYMBOLS = ("dvda_pcm_hip_energy", "dvda_pcm_hip_energy_workspace_words", "dvda_mlp_hip_pcm_energy",
           "dvda_pcm_hip_energy_append", "dvda_pcm_hip_energy_total")


def rail_pcm(rng, ch, frames):
    """full-range int32 with runs of -2^31 and of 2^31 - 1"""
    pcm = rng.integers(-2 ** 31, 2 ** 31, (ch, frames), dtype=np.int64)
    for c in range(ch):
        a = int(rng.integers(0, max(frames, 1)))
        pcm[c, a:a + 7] = -2 ** 31
        b = int(rng.integers(0, max(frames, 1)))
        pcm[c, b:b + 5] = 2 ** 31 - 1
    return pcm.astype(np.int32)


def test_constants_agree(pkg):
    hd = pkg.hipdec
    assert (em.MIN_BLOCK, em.MAX_BLOCK, em.PIECE) == (hd.NRG_MIN_BLOCK, hd.NRG_MAX_BLOCK, hd.NRG_PIECE_FRAMES) == (64, 1 << 24, 4096)
    assert ctypes.sizeof(hd.EnergyBlock) == 168
    for frames, B, lead in ((0, 64, None), (1, 64, None), (64, 64, None), (65, 64, 1), (1000, 100, 99), (5, 64, 65), (5, 64, 0)):
        assert hd.energy_nblocks(frames, B, lead) == em.nblocks(frames, B, lead)


def test_known_values():
    pcm = np.array([[3, -4, 0, -2 ** 31], [1, 1, 1, 1]], np.int32)
    (b0,) = em.energy(np.tile(pcm, (1, 16)), 64)
    b1 = em.energy(pcm, 64, lead=2)[1]
    assert em.sums(b0)[:3] == [16 * (25 + 2 ** 62), 64, 0] and b0["peak"][:3] == [2 ** 31, 1, 0] and b0["frames"] == 64
    assert b0["sq_hi"][0] == 4 and b0["sq_lo"][0] == 16 * 25        # four values of -2^31 already carry into sq_hi
    assert em.sums(b1)[:2] == [2 ** 62, 2] and b1["frames"] == 2
    assert em.energy(np.zeros((2, 0), np.int32), 64) == [] and em.energy(np.zeros((9, 5), np.int32), 64) == []
    four = em.energy(np.full((1, 4), -2 ** 31, np.int32), 64)[0]
    assert (four["sq_lo"][0], four["sq_hi"][0], four["peak"][0]) == (0, 1, 2 ** 31)


@pytest.mark.parametrize("B", [64, 100, 4410])
def test_grid_and_fast_model(B):
    rng = np.random.default_rng(B)
    for frames in (1, B - 1, B, B + 1, 3 * B + 5):
        for lead in (None, 1, B - 1):
            pcm = rail_pcm(rng, 3, frames)
            got = em.energy(pcm, B, lead)
            assert got == em.energy_fast(pcm, B, lead)
            ld = B if lead is None else lead
            assert [b["frames"] for b in got] == [min(ld, frames)] + [B] * ((frames - min(ld, frames)) // B) + \
                ([(frames - ld) % B] if frames > ld and (frames - ld) % B else [])
            assert sum(b["frames"] for b in got) == frames
            assert em.pieces_of_stream(frames, B, lead) <= frames // em.PIECE + frames // B + 2


def test_peak_is_the_level_reports(pkg):
    rng = np.random.default_rng(3)
    for ch, frames in ((1, 10), (2, 700), (6, 129)):
        pcm = rail_pcm(rng, ch, frames)
        lv = lm.levels(pcm, 24)
        tot = em.total(em.energy(pcm, 64, 17))
        assert tot["peak"] == [max(abs(lv["min"][c]), abs(lv["max"][c])) for c in range(8)]
        assert tot["frames"] == frames
        assert em.sums(tot)[:ch] == [sum(int(v) ** 2 for v in pcm[c]) for c in range(ch)]


def test_append_is_the_model_of_the_whole(pkg):
    """model(A || B) == append(model(A), model(B, lead = next lead)), in the model and in the library: random cuts, B, lead"""
    hd = pkg.hipdec
    rng = np.random.default_rng(2026)
    for k in range(60):
        B = int(rng.choice([64, 65, 100, 333]))
        ch = int(rng.integers(1, 9))
        frames = int(rng.integers(1, 6 * B))
        pcm = rail_pcm(rng, ch, frames)
        if k % 5 == 0:
            pcm[:] = -2 ** 31                   # every sum carries into sq_hi
        whole = em.energy(pcm, B)
        cuts = sorted(set(int(c) for c in rng.integers(0, frames + 1, int(rng.integers(1, 5)))))
        track_m, track_l, done = [], [], 0
        for end in cuts + [frames]:
            piece = em.energy(pcm[:, done:end], B, em.next_lead(done, B))
            track_m = em.append(track_m, piece, B)
            track_l = hd.energy_append(track_l, piece, B)
            done = end
        assert track_m == whole, k
        assert track_l == whole, k
        assert hd.energy_total(whole) == em.total(whole)
        assert hd.energy_sums(whole) == [em.sums(b) for b in whole]


def test_append_refuses_what_is_off_the_grid(pkg):
    hd = pkg.hipdec
    B = 64
    rng = np.random.default_rng(8)
    pcm = rail_pcm(rng, 2, 200)
    track = em.energy(pcm[:, :70], B)                       # 64 + 6
    good = em.energy(pcm[:, 70:], B, em.next_lead(70, B))   # 58 + 64 + 8
    assert hd.energy_append(track, good, B) == em.energy(pcm, B)
    for lead in (59, 64, 57):                               # one frame too many; a whole block; too few with blocks behind
        off = em.energy(pcm[:, 70:], B, lead)
        with pytest.raises(ValueError):
            em.append(track, off, B)
        with pytest.raises(hd.HipError, match="EINVAL"):
            hd.energy_append(track, off, B)
    # too few frames and nothing behind them: still on the grid
    short = em.energy(pcm[:, 70:80], B, 58)
    assert hd.energy_append(track, short, B) == em.append(track, short, B) == em.energy(pcm[:, :80], B)
    # the room: exactly enough, and one block short -- nothing is written then
    need = len(em.energy(pcm, B))
    assert hd.energy_append(track, good, B, cap=need) == em.energy(pcm, B)
    L = hd.lib()
    arr = (hd.EnergyBlock * need)()
    for j, b in enumerate(track):
        arr[j] = hd.EnergyBlock.from_dict(b)
    piece = (hd.EnergyBlock * len(good))(*[hd.EnergyBlock.from_dict(b) for b in good])
    n = ctypes.c_uint64(len(track))
    before = bytes(arr)
    assert L.dvda_pcm_hip_energy_append(arr, ctypes.byref(n), need - 1, piece, len(good), B) == ECAPACITY
    assert n.value == len(track) and bytes(arr) == before
    for bad_b in (63, (1 << 24) + 1):
        assert L.dvda_pcm_hip_energy_append(arr, ctypes.byref(n), need, piece, len(good), bad_b) == EINVAL
    assert L.dvda_pcm_hip_energy_append(arr, None, need, piece, len(good), B) == EINVAL
    assert L.dvda_pcm_hip_energy_append(arr, ctypes.byref(n), need, None, 1, B) == EINVAL
    assert L.dvda_pcm_hip_energy_append(arr, ctypes.byref(n), need, None, 0, B) == 0 and n.value == len(track)


def test_total_saturates_its_frames(pkg):
    hd = pkg.hipdec
    blk = em.record([2 ** 64 - 1, 5], [7, 9], 1 << 24)
    many = [blk] * 300                          # 300 * 2^24 frames > 2^32
    want = em.total(many)
    assert want["frames"] == 0xFFFFFFFF and em.sums(want)[0] == 300 * (2 ** 64 - 1)
    assert hd.energy_total(many) == want
    assert hd.energy_total([]) == em.record([0] * 8, [0] * 8, 0)


def test_arguments_are_judged_before_the_device(pkg):
    """DVDA_HIP_EINVAL for a block length outside its range, a WAV layout, a null pointer, a workspace one word short --
    with or without a device"""
    L = pkg.hipdec.lib()
    n, bound, B = 3, 1 << 20, 9600
    words = L.dvda_pcm_hip_energy_workspace_words(n, bound, B)
    assert words >= 2 * (n + 1) + (bound // em.PIECE + bound // B + 2 * n) * 32
    assert L.dvda_pcm_hip_energy_workspace_words(n, bound, 63) == 0
    assert L.dvda_pcm_hip_energy_workspace_words(n, bound, (1 << 24) + 1) == 0
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data

    def call(layout=0, block=B, work_words=words, null=None, lead=p):
        args = [p, layout, p, n, block, lead, bound, p, p, p, p, p, work_words, None]
        if null is not None:
            args[null] = None
        return L.dvda_pcm_hip_energy(*args)

    for block in (0, 63, (1 << 24) + 1, 0xFFFFFFFF):
        assert call(block=block) == EINVAL
    for layout in (2, 3, 4):
        assert call(layout=layout) == EINVAL
    for null in (0, 2, 7, 8, 9, 10, 11):
        assert call(null=null) == EINVAL
    assert call(work_words=words - 1) == EINVAL
    # 2^31 pieces or more
    huge = 1 << 38
    assert L.dvda_pcm_hip_energy(p, 0, p, n, 64, None, huge, p, p, p, p, p,
                                 L.dvda_pcm_hip_energy_workspace_words(n, huge, 64), None) == ECAPACITY
    first = (ctypes.c_uint64 * 2)()
    assert L.dvda_mlp_hip_pcm_energy(None, p, p, p, B, None, 0, first, 1, None) == EINVAL


def test_no_device_is_an_error(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pkg.hipdec.lib()
    n, bound = 1, 1 << 20
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    for layout, B, lead in ((0, 64, None), (1, 9600, p), (0, 1 << 24, None)):
        words = L.dvda_pcm_hip_energy_workspace_words(n, bound, B)
        assert L.dvda_pcm_hip_energy(p, layout, p, n, B, lead, bound, p, p, p, p, p, words, None) == ENODEV
    with pytest.raises(pkg.hipdec.HipError):
        pkg.hipdec.pcm_energy(torch.zeros(4, dtype=torch.int32), 0, [(0, 4, 4, 1)], 64)


def test_symbols_are_declared_and_exported(pkg):
    hd = pkg.hipdec
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    L = hd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hd.EXPORTS and getattr(L, name) is not None
    for const in ("DVDA_NRG_MIN_BLOCK", "DVDA_NRG_MAX_BLOCK", "DVDA_NRG_PIECE_FRAMES", "dvda_pcm_energy_block"):
        assert const in text
    assert "does not fit 64 bits" not in text


def test_energy_kernels_use_no_scratch(tmp_path):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    lines = open(isa.compile_asm(str(tmp_path / "mlp_hip.s"))).read().split("\n")
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"(_ZN3nrg\d+k_nrg\w+):", lines[i])
        i += 1
        if not m:
            continue
        count = 0
        while not lines[i].startswith(".Lfunc_end"):
            count += bool(re.match(r"\s+scratch_", lines[i]))
            i += 1
        found[m.group(1)] = count
    names = " ".join(found)
    for k in ("k_nrg_plan", "k_nrg_tilesILb0E", "k_nrg_tilesILb1E", "k_nrg_join"):
        assert k in names, (k, names)
    assert all(v == 0 for v in found.values()), found
