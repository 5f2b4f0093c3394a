"""What the compiler made of the channel mix's kernels (csrc/pcm_mix.h, k_mix_tiles), held to what DESIGN.md section 20
records (CPU only: hipcc cross-compiles).

The multiply-add is an asm statement with the coefficient in an SGPR: 8 rows x 8 coefficients x a lane's 4 frames = 256
of them per instance, each row's 32 under a wave-uniform branch on the row and each coefficient's 4 under one on the
coefficient.  The rows come over the scalar side, 32 bytes at a time.  The pass is bound by its bytes, so what it costs
depends on the compiler keeping the wide accesses and the occupancy: these cases read the assembly of every build -- the
four instances, no scratch and no scratch_ instruction, the LDS size and register count that keep four workgroups per
CU, the exact number of v_mad_i64_i32 and that no multiply between the first and the last of them has been split into
v_mad_u64_u32 / v_mul_lo_u32 pieces, 16-byte global loads and stores on either side.  Only ordinary instructions are
counted."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MADS = 8 * 8 * 4                # rows x coefficients x frames of a lane
PITCH = 4 * 256 + 4             # mix::PITCH: words between the planes of a chunk
INSTANCES = [(i, o) for i in (1, 0) for o in (1, 0)]     # input planar, output planar


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = open(mod.compile_asm(str(tmp_path_factory.mktemp("isa") / "mlp_hip.s"))).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"_ZN3mix11k_mix_tilesILb(\d)ELb(\d)EE\w+:", lines[i])
        i += 1
        if not m:
            continue
        ops, info, seq = {}, {}, []
        while not lines[i].startswith(".Lfunc_end"):
            t = lines[i].strip()
            i += 1
            op = re.match(r"([a-z_0-9]+)", t) if t and t[0] not in ".;" else None
            if op:
                ops[op.group(1)] = ops.get(op.group(1), 0) + 1
                seq.append(op.group(1))
        for t in lines[i:i + 120]:                  # the "; Kernel info:" comment block behind the function
            mm = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", t.strip())
            if mm:
                info.setdefault(mm.group(1), int(mm.group(2)))
        # the frame loop: from the first multiply-add to the last
        first = seq.index("v_mad_i64_i32")
        last = len(seq) - 1 - seq[::-1].index("v_mad_i64_i32")
        out[tuple(int(g) for g in m.groups())] = (ops, info, seq[first:last + 1])
    return out


def test_every_instance_is_found(kernels):
    assert sorted(kernels) == sorted(INSTANCES)


@pytest.mark.parametrize("inst", INSTANCES)
def test_registers_scratch_and_lds(kernels, inst):
    ops, info, loop = kernels[inst]
    print(inst, info)
    assert info["ScratchSize"] == 0 and not any(op.startswith("scratch_") for op in ops)
    # 8 planes of PITCH words and the fold's 4 x 8 bytes: four workgroups per CU in 160 KB, 4 waves per SIMD, which 128
    # registers allow
    assert info["LDSByteSize"] == 4 * 8 * PITCH + 32 == 32928 and 4 * info["LDSByteSize"] <= 160 * 1024
    assert info["Occupancy"] == 4
    assert info["NumVgprs"] <= 128              # (96 - 112 today)


@pytest.mark.parametrize("inst", INSTANCES)
def test_the_frame_loop(kernels, inst):
    ops, _, loop = kernels[inst]
    count = lambda name: sum(1 for op in loop if op == name)
    print(inst, "v_mad_i64_i32", ops.get("v_mad_i64_i32"), "v_mad_u64_u32 / v_mul_lo_u32 in the loop", count("v_mad_u64_u32"),
          count("v_mul_lo_u32"), "s_load_dwordx8 in the loop", count("s_load_dwordx8"), "loop length", len(loop))
    assert ops.get("v_mad_i64_i32") == MADS and count("v_mad_i64_i32") == MADS
    assert count("v_mad_u64_u32") == 0 and count("v_mul_lo_u32") == 0 and count("v_mul_hi_u32") == 0
    # the rows over the scalar side, one load of 32 bytes each (the first lies in front of the first multiply-add), and
    # nothing from global memory among the multiplies
    assert 7 <= count("s_load_dwordx8") <= 8 and count("s_load_dword") == 0
    assert not any(op.startswith(("global_load", "buffer_load", "flat_load")) for op in loop)


@pytest.mark.parametrize("inst", INSTANCES)
def test_wide_accesses_on_either_side(kernels, inst):
    ops, _, _ = kernels[inst]
    print(inst, {k: v for k, v in ops.items() if k.startswith(("global_", "ds_"))})
    assert ops.get("global_load_dwordx4", 0) >= 1 and ops.get("global_store_dwordx4", 0) >= 1
    assert not any(op.startswith(("buffer_", "flat_")) for op in ops)
