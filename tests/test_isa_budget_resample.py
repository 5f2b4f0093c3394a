"""What the compiler made of the resampler's kernels (csrc/pcm_resample.h, k_rs_tiles), held to what DESIGN.md section 19
records (CPU only: hipcc cross-compiles).

The tap loop's multiply-add is an asm statement with the tap in an SGPR, 291 of them per instance, fully unrolled, the
taps read with scalar loads of the table and the window with LDS reads, one block of 8 positions ahead of the
multiplies.  What the kernel costs depends on the compiler keeping that shape: these cases read the assembly of every
build -- the four instances, no scratch and no scratch_ instruction, the LDS size that sets two workgroups per CU, the
register count, the exact number of v_mad_i64_i32 and that the multiply has not been split into v_mad_u64_u32 pieces,
the taps on the scalar side (s_load, not per-lane loads), and at most one s_nop per multiply-add (HIP 7.2, clang
22.0.0git gives 270 - 271 between the first and the last of them).  Only ordinary instructions are counted."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MADS = 291                      # 96 + 97 + 98: three outputs per work item, their rows padded by 0, 1 and 2 zeros
TAP_DWORDS = 96 + 97 + 98
INSTANCES = [(i, o) for i in (1, 0) for o in (1, 0)]     # input planar, output planar


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = open(mod.compile_asm(str(tmp_path_factory.mktemp("isa") / "mlp_hip.s"))).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"_ZN3rsm10k_rs_tilesILb(\d)ELb(\d)EE\w+:", lines[i])
        i += 1
        if not m:
            continue
        ops, info, loop = {}, {}, []
        while not lines[i].startswith(".Lfunc_end"):
            t = lines[i].strip()
            i += 1
            op = re.match(r"([a-z_0-9]+)", t) if t and t[0] not in ".;" else None
            if op:
                ops[op.group(1)] = ops.get(op.group(1), 0) + 1
                loop.append(op.group(1))
        for t in lines[i:i + 120]:                  # the "; Kernel info:" comment block behind the function
            mm = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", t.strip())
            if mm:
                info.setdefault(mm.group(1), int(mm.group(2)))
        # the tap loop: from the first multiply-add to the last
        first = loop.index("v_mad_i64_i32")
        last = len(loop) - 1 - loop[::-1].index("v_mad_i64_i32")
        out[tuple(int(g) for g in m.groups())] = (ops, info, loop[first:last + 1])
    return out


def test_every_instance_is_found(kernels):
    assert sorted(kernels) == sorted(INSTANCES)


@pytest.mark.parametrize("inst", INSTANCES)
def test_registers_scratch_and_lds(kernels, inst):
    ops, info, loop = kernels[inst]
    print(inst, info)
    assert info["ScratchSize"] == 0 and not any(op.startswith("scratch_") for op in ops)
    assert not any(op.startswith("scratch_") for op in loop)
    # 64 pairs x 255 words + 2, and the fold's 4 x 8 bytes, rounded up to 16: two workgroups per CU, 2 waves per SIMD
    assert info["LDSByteSize"] == (4 * (64 * 255 + 2) + 32 + 15) // 16 * 16 == 65328 and info["Occupancy"] == 2
    assert info["NumVgprs"] <= 64               # (47 - 49 today)


@pytest.mark.parametrize("inst", INSTANCES)
def test_the_tap_loop(kernels, inst):
    ops, _, loop = kernels[inst]
    count = lambda name: sum(1 for op in loop if op == name)
    loads = {n: count("s_load_dwordx%d" % n) for n in (2, 4, 8, 16)}
    loads[1] = count("s_load_dword")
    tap_dwords = sum(n * k for n, k in loads.items())
    lds = 2 * count("ds_read2_b32") + count("ds_read_b32") + 2 * count("ds_read_b64") + 4 * count("ds_read_b128")
    print(inst, "v_mad_i64_i32", ops.get("v_mad_i64_i32"), "v_mad_u64_u32 in the loop", count("v_mad_u64_u32"),
          "s_nop in the loop", count("s_nop"), "scalar loads", loads, "LDS dwords", lds, "loop length", len(loop))
    assert ops.get("v_mad_i64_i32") == MADS and count("v_mad_i64_i32") == MADS
    assert count("v_mad_u64_u32") == 0 and count("v_mul_lo_u32") == 0 and count("v_mul_hi_u32") == 0
    assert count("s_nop") <= MADS
    # the taps come over the scalar side, each once or nearly so; the window's 100 values over LDS, each once (the loop
    # is read from its first multiply-add on: the first two blocks' loads, 2 x 8 positions of 3 rows, lie in front of it)
    assert TAP_DWORDS - 64 <= tap_dwords <= TAP_DWORDS + 16
    assert not any(op.startswith("global_load") or op.startswith("buffer_load") or op.startswith("flat_load") for op in loop)
    assert 100 - 16 <= lds <= 104
    # nothing else of weight: the loop is its multiply-adds, their s_nop, the loads and their waits
    assert len(loop) <= 2 * MADS + 160
