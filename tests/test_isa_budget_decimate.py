"""What the compiler made of the decimation kernels (csrc/pcm_decim.h, k_dc_tiles), held to what DESIGN.md section 17
records (CPU only: hipcc cross-compiles).

The tap loop's multiply-add is an asm statement with the tap pinned to an SGPR, 776 (by 2) / 1 156 (by 4) of them per
instance, fully unrolled: what the kernel costs depends on the compiler's hazard recognizer (an s_nop behind an asm
statement) and on its scalar register allocation (taps that do not fit the scalar file are rematerialised with s_mov /
s_movk inside the loop), and a build that spills the window's loads runs out of scratch.  These cases read the assembly
of every build: no scratch, the LDS size that sets two workgroups per CU, the register count, the exact number of
v_mad_i64_i32 -- and that the compiler has not gone back to factoring the symmetric taps into v_mad_u64_u32 -- and
bounds on the s_nop and s_mov counts with some room over what HIP 7.2 (clang 22.0.0git) gives: 725 - 742 / 839 - 866
s_nop and 66 - 76 / 274 - 304 s_mov_b32 + s_movk_i32 per instance."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MADS = {2: 776, 4: 1156}
SMOV_MAX = {2: 100, 4: 330}
INSTANCES = [(d, i, o) for d in (2, 4) for i in (1, 0) for o in (1, 0)]     # ratio, input planar, output planar


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = open(mod.compile_asm(str(tmp_path_factory.mktemp("isa") / "mlp_hip.s"))).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"_ZN3dcm10k_dc_tilesILj(\d)ELb(\d)ELb(\d)EE\w+:", lines[i])
        i += 1
        if not m:
            continue
        ops, info = {}, {}
        while not lines[i].startswith(".Lfunc_end"):
            t = lines[i].strip()
            i += 1
            op = re.match(r"([a-z_0-9]+)", t) if t and t[0] not in ".;" else None
            if op:
                ops[op.group(1)] = ops.get(op.group(1), 0) + 1
        for t in lines[i:i + 120]:                  # the "; Kernel info:" comment block behind the function
            mm = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", t.strip())
            if mm:
                info.setdefault(mm.group(1), int(mm.group(2)))
        out[tuple(int(g) for g in m.groups())] = (ops, info)
    return out


def test_every_instance_is_found(kernels):
    assert sorted(kernels) == sorted(INSTANCES)


@pytest.mark.parametrize("inst", INSTANCES)
def test_registers_scratch_and_lds(kernels, inst):
    ops, info = kernels[inst]
    print(inst, info)
    assert info["ScratchSize"] == 0 and not any(op.startswith("scratch_") for op in ops)
    assert info["LDSByteSize"] == 62496 and info["Occupancy"] == 2 and info["NumVgprs"] <= 80


@pytest.mark.parametrize("inst", INSTANCES)
def test_multiply_adds_and_what_the_asm_statements_cost(kernels, inst):
    ops, _ = kernels[inst]
    smov = ops.get("s_mov_b32", 0) + ops.get("s_movk_i32", 0)
    print(inst, "v_mad_i64_i32", ops.get("v_mad_i64_i32"), "v_mad_u64_u32", ops.get("v_mad_u64_u32", 0),
          "s_nop", ops.get("s_nop", 0), "s_mov_b32 + s_movk_i32", smov)
    assert ops.get("v_mad_i64_i32") == MADS[inst[0]]
    assert ops.get("v_mad_u64_u32", 0) <= 2         # (the address arithmetic outside the tap loop)
    assert ops.get("s_nop", 0) <= MADS[inst[0]]
    assert smov <= SMOV_MAX[inst[0]]
