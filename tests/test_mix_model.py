"""The channel mix's host arithmetic (include/dvda_mlp_hip.h, csrc/pcm_mix.h) against tests/mix_model.py: the value the
kernel compiles, the validity rule at its edge, the speaker masks, the default matrices by their integer recipe, and every
argument the entry points judge before they ask for a device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mix_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY, ENODEV = -3, -4, -1
SYMBOLS = ("dvda_pcm_hip_mix", "dvda_pcm_hip_mix_workspace_words", "dvda_mlp_hip_pcm_mix", "dvda_pcm_hip_speaker_mask",
           "dvda_pcm_hip_mix_matrix", "dvda_pcm_hip_mix_valid", "dvda_pcm_hip_mix_value")
FLAGS = [mm.NORMALIZED, mm.UNITY, mm.NORMALIZED | mm.LFE, mm.UNITY | mm.LFE]
LO, HI = -2 ** 31, 2 ** 31 - 1


def test_library_value_is_the_model(pkg):
    hd = pkg.hipdec
    rng = np.random.default_rng(5)
    for ich in range(1, 9):
        for och in (1, 2, ich, 8):
            m = mm.random_matrix(rng, ich, och, full_rows=(0,) if och > 1 else ())
            assert hd.mix_valid(m)
            x = rng.integers(LO, HI + 1, (40, ich), dtype=np.int64)
            x[0], x[1] = LO, HI
            for bits in mm.DEPTHS:
                for row in x:
                    for o in range(och):
                        assert hd.mix_value(row, m, o, bits) == mm.value(list(row), m, o, bits), (ich, och, bits, o)
    # the numpy form is the integer form
    for ich, och in ((6, 2), (3, 3), (8, 1), (1, 8)):
        m = mm.random_matrix(rng, ich, och, full_rows=(0,))
        pcm = rng.integers(LO, HI + 1, (ich, 97), dtype=np.int64).astype(np.int32)
        pcm[:, :3] = [[LO, HI, 0]] * ich
        a, ca = mm.mix(pcm, m, 20)
        b, cb = mm.mix_np(pcm, m, 20)
        assert np.array_equal(a, b) and ca == cb


def test_rails_with_rows_of_exactly_two_to_the_31(pkg):
    """acc = +2^62 and -2^62, exact: the sum of |coef| at its limit and every input at a rail of int32"""
    hd = pkg.hipdec
    half = 1 << 30
    cases = [
        (mm.matrix(2, 1, [[half, half]]), [LO, LO]),
        (mm.matrix(2, 1, [[-half, -half]]), [LO, LO]),
        (mm.matrix(1, 1, [[LO]]), [LO]),
        (mm.matrix(1, 1, [[LO]]), [HI]),
        (mm.matrix(2, 1, [[half, -half]]), [LO, HI]),
        (mm.matrix(8, 1, [[1 << 28] * 8]), [LO] * 8),
        (mm.matrix(8, 1, [[-(1 << 28)] * 8]), [LO] * 8),
        (mm.matrix(8, 1, [[1 << 28] * 8]), [HI] * 8),
    ]
    accs = []
    for m, x in cases:
        assert sum(abs(g) for g in m["coef"][0]) == mm.MAX_ROW and hd.mix_valid(m) and mm.valid(m)
        acc = sum(g * v for g, v in zip(m["coef"][0], x))
        accs.append(acc)
        for bits in mm.DEPTHS:
            got = hd.mix_value(x, m, 0, bits)
            assert got == mm.value(x, m, 0, bits) == mm.finish(acc, bits)
            assert got == ((1 << (bits - 1)) - 1 if acc > 0 else -(1 << (bits - 1)), 1)
    assert accs[:3] == [-(1 << 62), 1 << 62, 1 << 62] and accs[5:7] == [-(1 << 62), 1 << 62]
    assert max(abs(a) for a in accs) == 1 << 62


def test_validity_at_its_edge(pkg):
    hd = pkg.hipdec
    half = 1 << 30
    assert hd.mix_valid(mm.matrix(2, 2, [[half, half], [-half, half]]))
    for rows in ([[half, half + 1]], [[half, half], [half + 1, -half]], [[LO, 1]], [[LO, -1]]):
        m = mm.matrix(2, len(rows), rows)
        assert not hd.mix_valid(m) and not mm.valid(m)
        with pytest.raises(hd.HipError):
            hd.mix_value([0, 0], m, 0, 24)
    # entries outside [out)[in) are ignored
    m = mm.matrix(2, 1, [[half, half]])
    m["coef"][0][2] = 5
    m["coef"][1][0] = HI
    m["coef"][7][7] = LO
    assert hd.mix_valid(m) and hd.mix_value([3, 5], m, 0, 16) == (8, 0)
    for ich, och in ((0, 1), (1, 0), (9, 1), (1, 9), (0, 0)):
        assert not hd.mix_valid(dict(in_channels=ich, out_channels=och, coef=mm.identity(1)["coef"]))
    ok = mm.identity(2)
    for o, bits in ((2, 24), (0, 8), (0, 18), (0, 32)):
        with pytest.raises(hd.HipError):
            hd.mix_value([0, 0], ok, o, bits)
    with pytest.raises(hd.HipError):
        hd.mix_value([0, 0, 0], ok, 0, 24)
    cl = ctypes.c_int(7)
    assert hd.lib().dvda_pcm_hip_mix_value(None, None, 0, 24, ctypes.byref(cl)) == 0 and cl.value == -1
    assert hd.lib().dvda_pcm_hip_mix_valid(None) == 0


def test_identity_permutation_and_extraction(pkg):
    """2^30 on the diagonal copies values inside `bits`; rows of one 2^30 permute or extract: the library's value, and
    the model's"""
    hd = pkg.hipdec
    rng = np.random.default_rng(9)
    pcm = rng.integers(-2 ** 15, 2 ** 15, (5, 33), dtype=np.int64).astype(np.int32)
    pcm[:, 0], pcm[:, 1] = -2 ** 15, 2 ** 15 - 1
    perm = [3, 0, 4, 1, 2]
    for m, want in ((mm.identity(5), pcm),
                    (mm.matrix(5, 5, [[mm.ONE if c == perm[o] else 0 for c in range(5)] for o in range(5)]), pcm[perm]),
                    (mm.matrix(5, 1, [[0, 0, mm.ONE, 0, 0]]), pcm[2:3])):
        out, cl = mm.mix_np(pcm, m, 16)
        assert np.array_equal(out, want) and cl == [0] * 8
        for f in range(pcm.shape[1]):
            for o in range(m["out_channels"]):
                assert hd.mix_value(pcm[:, f], m, o, 16) == (int(want[o, f]), 0)


def test_speaker_masks(pkg):
    hd = pkg.hipdec
    assert mm.A == int(np.rint(2.0 ** 30 / np.sqrt(2.0))) == 759250125
    for a in range(21):
        assert hd.speaker_mask(a) == mm.MASKS[a] == mm.speaker_mask(a) and mm.MASKS[a] & ~0x13F == 0
    for a in list(range(21, 32)) + [255, 2 ** 31]:
        assert hd.speaker_mask(a) == 0
    # (that a reader of the disc tier answers the same: tests/test_gpu_mix_disc.py and tests/test_disc_api.py, on readers)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("och", [1, 2])
def test_default_matrices(pkg, och, flags):
    hd = pkg.hipdec
    for a in range(21):
        mask = mm.MASKS[a]
        got = hd.mix_matrix(mask, och, flags)
        want = mm.default_matrix(mask, och, flags)
        assert got == want, (a, och, flags)
        ich = bin(mask).count("1")
        assert got["in_channels"] == ich and got["out_channels"] == och
        bits = [1 << b for b in range(9) if mask >> b & 1]
        rows = [got["coef"][o][:ich] for o in range(och)]
        assert all(g >= 0 for row in rows for g in row)
        assert all(g == 0 for o in range(8) for c in range(8) if o >= och or c >= ich for g in [got["coef"][o][c]])
        if not flags & mm.UNITY:
            assert all(sum(row) <= 1 << 30 for row in rows) and hd.mix_valid(got)
            assert max(sum(row) for row in rows) > (1 << 30) - 8        # (the largest row loses at most one per entry)
        else:
            # the weights as they are: the fronts at gain 1 (mono: a half each)
            for c, b in enumerate(bits):
                if b in (mm.FL, mm.FR):
                    assert rows[0 if och == 1 or b == mm.FL else 1][c] == (mm.ONE >> 1 if och == 1 else mm.ONE)
            # a matrix the kernels take exactly when no row's weights sum above 2^31
            assert hd.mix_valid(got) == all(sum(row) <= mm.MAX_ROW for row in rows) == mm.valid(got)
        if LFE_IN(mask) and not flags & mm.LFE:
            assert all(row[bits.index(mm.LF)] == 0 for row in rows)
        if LFE_IN(mask) and flags & mm.LFE:
            assert all(row[bits.index(mm.LF)] > 0 for row in rows)
        if och == 2:
            # every DVD-Audio mask is symmetric: L / R mirror each other over FL <-> FR, BL <-> BR
            mirror = {mm.FL: mm.FR, mm.FR: mm.FL, mm.BL: mm.BR, mm.BR: mm.BL}
            assert all((mirror.get(b, b) in bits) for b in bits)
            for c, b in enumerate(bits):
                assert rows[0][c] == rows[1][bits.index(mirror.get(b, b))]


def LFE_IN(mask):
    return bool(mask & mm.LF)


def test_default_matrices_that_are_refused(pkg):
    hd = pkg.hipdec
    L = hd.lib()
    rec = hd.PcmMix()
    for mask, och, flags in ((0, 2, 0), (0x40, 2, 0), (0x80, 2, 0), (0x200, 1, 0), (0x3F | 0x400, 2, 0), (0x3F, 0, 0),
                             (0x3F, 3, 0), (0x3F, 8, 0), (0x3F, 2, 4), (0x3F, 2, 8)):
        assert L.dvda_pcm_hip_mix_matrix(mask, och, flags, ctypes.byref(rec)) == EINVAL, (mask, och, flags)
        assert mm.default_matrix(mask, och, flags) is None
        with pytest.raises(hd.HipError, match="EINVAL"):
            hd.mix_matrix(mask, och, flags)
    assert L.dvda_pcm_hip_mix_matrix(0x3F, 2, 0, None) == EINVAL
    # every mask inside 0x13F is taken, whatever its channels: 1 .. 7 of them
    for mask in (0x1, 0x8, 0x100, 0x13F, 0x120, 0x5):
        for och in (1, 2):
            for flags in FLAGS:
                assert hd.mix_matrix(mask, och, flags) == mm.default_matrix(mask, och, flags)


@pytest.mark.parametrize("bits", mm.DEPTHS)
def test_normalized_matrices_never_clip_input_inside_the_depth(pkg, bits):
    """held at the rails: every channel at the depth's lowest and highest value, and every mix of the two"""
    hd = pkg.hipdec
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for a in range(21):
        for och in (1, 2):
            for flags in (mm.NORMALIZED, mm.NORMALIZED | mm.LFE):
                m = hd.mix_matrix(mm.MASKS[a], och, flags)
                ich = m["in_channels"]
                frames = np.array([[hi if k >> c & 1 else lo for k in range(1 << ich)] for c in range(ich)], np.int32)
                out, clipped = mm.mix_np(frames, m, bits)
                assert clipped == [0] * 8 and out.min() >= lo and out.max() <= hi, (a, och, flags)
                for x in ([lo] * ich, [hi] * ich):
                    for o in range(och):
                        assert hd.mix_value(x, m, o, bits)[1] == 0
    # ... which UNITY does not promise: the 5.1 fronts at gain 1 clip at the rails
    m = hd.mix_matrix(mm.MASKS[1], 1, mm.UNITY)
    assert hd.mix_value([hi, hi], m, 0, bits) == (hi, 0)
    m = hd.mix_matrix(mm.FL | mm.FR | mm.FC, 2, mm.UNITY)
    assert hd.mix_value([hi, hi, hi], m, 0, bits) == (hi, 1) and hd.mix_value([lo, lo, lo], m, 1, bits) == (lo, 1)


def test_arguments_are_judged_before_the_device(pkg):
    """every DVDA_HIP_EINVAL of the contract, with or without a device; then DVDA_HIP_ECAPACITY; then -- on a machine
    without one -- DVDA_HIP_ENODEV"""
    hd = pkg.hipdec
    L = hd.lib()
    n, bound = 3, 1 << 20
    words = L.dvda_pcm_hip_mix_workspace_words(n, bound)
    assert words == hd.pcm_mix_workspace_words(n, bound) >= 2 * (n + 1) + (bound // mm.TILE + n) * 8
    last = 0
    for k in (0, 1, 2, 100):
        for total in (0, 1, mm.TILE, 10 * mm.TILE + 1, 1 << 30):
            w = L.dvda_pcm_hip_mix_workspace_words(k, total)
            assert w >= last and w <= L.dvda_pcm_hip_mix_workspace_words(k + 1, total)
            last = w
        last = L.dvda_pcm_hip_mix_workspace_words(k, 0)
    buf = np.zeros(256, np.uint64)       # (stands in for every device pointer: nothing is read when the arguments are bad)
    p = buf.ctypes.data

    def call(bits=24, layout_in=0, layout_out=0, work_words=words, null=None, total=bound):
        args = [p, layout_in, p, p, layout_out, p, p, n, bits, total, p, p, work_words, None]
        if null is not None:
            args[null] = None
        return L.dvda_pcm_hip_mix(*args)

    for bits in (0, 8, 12, 18, 32):
        assert call(bits=bits) == EINVAL, bits
    for layout in (2, 3, 4):
        assert call(layout_in=layout) == EINVAL and call(layout_out=layout) == EINVAL
    for null in (0, 2, 3, 5, 6, 10, 11):
        assert call(null=null) == EINVAL, null
    assert call(work_words=words - 1) == EINVAL
    huge = 1 << 46
    assert call(total=huge, work_words=L.dvda_pcm_hip_mix_workspace_words(n, huge)) == ECAPACITY
    rep = (hd.PcmMixReport * 1)()
    mat = (hd.PcmMix * 1)()
    assert L.dvda_mlp_hip_pcm_mix(None, p, p, p, p, p, p, mat, 24, rep, 1, None) == EINVAL
    import torch
    if not torch.cuda.is_available():
        assert call() == ENODEV
        for bits in (16, 20, 24):
            for li in (0, 1):
                for lo in (0, 1):
                    assert call(bits=bits, layout_in=li, layout_out=lo) == ENODEV
        with pytest.raises(hd.HipError):
            hd.pcm_mix(torch.zeros(4, dtype=torch.int32), 0, [(0, 4, 4, 1)], [mm.identity(1)], 24)
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.decode_streams_downmixed([], out_channels=3)
    with pytest.raises(hd.HipError, match="EINVAL"):
        hd.decode_streams_downmixed([], layout=hd.PCM_WAV24)


def test_records_and_constants(pkg):
    hd = pkg.hipdec
    assert ctypes.sizeof(hd.PcmMix) == 264 and ctypes.sizeof(hd.PcmMixReport) == 72
    assert (hd.MIX_NORMALIZED, hd.MIX_UNITY, hd.MIX_LFE) == (mm.NORMALIZED, mm.UNITY, mm.LFE) == (0, 1, 2)
    assert mm.TILE == hd.LVL_TILE_FRAMES
    m = mm.random_matrix(np.random.default_rng(1), 5, 3)
    assert hd.PcmMix.from_dict(m).as_dict() == m
    assert hd.PcmMixReport.from_dict(mm.report(7, range(8))).as_dict() == mm.report(7, range(8))
    assert mm.add_reports(mm.report(3, [1] * 8), mm.report(4, [2] * 8)) == mm.report(7, [3] * 8)


def test_symbols_are_declared_and_exported(pkg):
    hd = pkg.hipdec
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    L = hd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in hd.EXPORTS and getattr(L, name) is not None
    for const in ("759250125", "sum_c |coef[o][c]| <= 2^31", "2^62 + 2^29 < 2^63", "#define DVDA_MIX_UNITY      1u",
                  "#define DVDA_MIX_LFE        2u", "can then never clip"):
        assert const in text, const
