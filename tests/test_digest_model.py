"""CPU tests of the PCM digest (csrc/pcm_digest.h): its decomposition restated in numpy (tests/digest_model.py)
against zlib, the library's host arithmetic, the entry point without a GPU, and the kernels' ISA."""
import importlib.util
import os
import re
import zlib

import numpy as np
import pytest

from tests import digest_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u" % name, text).group(1))


def test_constants_agree(pkg):
    assert dm.TILE == _header_constant("DVDA_CRC_TILE_BYTES") == pkg.hipdec.CRC_TILE_BYTES
    assert dm.JOIN == _header_constant("DVDA_CRC_JOIN_TILES") == pkg.hipdec.CRC_JOIN_TILES
    assert dm.TILE % 256 == 0


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, dm.TILE - 1, dm.TILE, dm.TILE + 1, 3 * dm.TILE + 7])
def test_decomposition_is_zlib(n):
    """end-aligned tiles with a zero prefix, strided Horner through the tables, lane weights, join, x^(8n) term"""
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert dm.crc32(data) == zlib.crc32(data)


def test_join_folds_more_than_one_turn():
    """more tiles than the join takes per turn: the strided Horner over tile values against the plain one"""
    rng = np.random.default_rng(11)
    for n_t in (dm.JOIN, dm.JOIN + 1, 2 * dm.JOIN + 5):
        vals = [int(v) for v in rng.integers(0, 1 << 32, n_t)]
        raw, step = 0, dm.xpow(8 * dm.TILE)
        for v in vals:
            raw = dm.gfmul(raw, step) ^ v
        n = n_t * dm.TILE - 5
        assert dm.join(vals, n) == raw ^ dm.gfmul(0xFFFFFFFF, dm.xpow(8 * n)) ^ 0xFFFFFFFF


def test_payload_is_the_oracles(oracle):
    """the model's write_signed / interleave is oracle.wav_pack over the full int32 range"""
    rng = np.random.default_rng(3)
    for bits in (16, 24):
        for ch in (1, 2, 3, 5, 6):
            pcm = rng.integers(-2 ** 31, 2 ** 31, (ch, 37), dtype=np.int64).astype(np.int32)
            assert dm.wav_payload(pcm, bits) == oracle.wav_pack(pcm, bits)


def test_combine_from_the_library(pkg):
    rng = np.random.default_rng(2024)
    comb = pkg.hipdec.crc32_combine
    for k in range(200):
        a = rng.integers(0, 256, int(rng.integers(0, 4000)), dtype=np.uint8).tobytes()
        b = rng.integers(0, 256, 0 if k % 20 == 0 else int(rng.integers(0, 4000)), dtype=np.uint8).tobytes()
        assert comb(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b), (k, len(a), len(b))
    # len_b >= 2^32: B = zeros, whose CRC the model computes without the buffer; A followed by L zero bytes is A's
    # state advanced by x^(8 L)
    for L in (1 << 32, (1 << 32) + 12345, 5 * (1 << 32) - 1, (1 << 40) + 7):
        a = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
        ca = zlib.crc32(a)
        want = dm.gfmul(ca ^ 0xFFFFFFFF, dm.xpow(8 * L)) ^ 0xFFFFFFFF
        assert comb(ca, dm.crc32_zeros(L), L) == want == dm.combine(ca, dm.crc32_zeros(L), L)
    assert dm.crc32_zeros(1000) == zlib.crc32(bytes(1000))


def test_no_device_is_an_error(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pkg.hipdec.lib()
    n, bound = 1, 1 << 20
    words = L.dvda_pcm_hip_crc32_workspace_words(n, bound)
    assert words >= 2 * (n + 1) + bound // dm.TILE + n
    buf = np.zeros(64, np.uint64)        # (stands in for every device pointer: nothing is read without a device)
    p = buf.ctypes.data
    for layout, bits in ((0, 24), (1, 16), (2, 24), (3, 16)):
        assert L.dvda_pcm_hip_crc32(p, layout, bits, p, n, bound, p, p, p, words, None) == -1      # DVDA_HIP_ENODEV
    for layout, bits in ((0, 20), (0, 32), (2, 16), (3, 24), (4, 24)):
        assert L.dvda_pcm_hip_crc32(p, layout, bits, p, n, bound, p, p, p, words, None) == -3      # DVDA_HIP_EINVAL
    with pytest.raises(pkg.hipdec.HipError):
        pkg.hipdec.pcm_crc32(torch.zeros(4, dtype=torch.int32), 0, 24, [(0, 4, 4, 1)])


def test_digest_kernels_use_no_scratch(tmp_path):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    lines = open(isa.compile_asm(str(tmp_path / "mlp_hip.s"))).read().split("\n")
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"(_ZN3crc\d+k_crc\w+):", lines[i])
        i += 1
        if not m:
            continue
        count = 0
        while not lines[i].startswith(".Lfunc_end"):
            count += bool(re.match(r"\s+scratch_", lines[i]))
            i += 1
        found[m.group(1)] = count
    names = " ".join(found)
    for k in ("k_crc_plan", "k_crc_tilesILi0E", "k_crc_tilesILi1E", "k_crc_tilesILi2E", "k_crc_join"):
        assert k in names, (k, names)
    assert all(v == 0 for v in found.values()), found
