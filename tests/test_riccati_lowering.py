"""CPU: ``solve_discrete_are`` lowers under ``mode="hip"`` (single, batched, with its gradient) with no host
fallback, and csrc/riccati.hip compiles for gfx950 with scalar memory instructions that only load."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import make_ref

pytestmark = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pt():
    make_ref.activate()
    import pytensor
    import pytensor.tensor as ptt

    import pytensor_amd

    pytensor_amd.register()
    return pytensor, ptt


def _ops(f):
    return [n.op for n in f.maker.linker.last_ir.nodes]


def _inputs(ptt, dtype="float64", batched=False):
    A = (ptt.tensor3 if batched else ptt.matrix)("A", dtype=dtype)
    return A, ptt.matrix("B", dtype=dtype), ptt.matrix("Q", dtype=dtype), ptt.matrix("R", dtype=dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dare_lowers_to_one_node(pt, dtype):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_discrete_are

    ins = _inputs(ptt, dtype)
    X = solve_discrete_are(*ins)
    f = pytensor.function(list(ins), X, mode="hip")
    ops = _ops(f)
    assert ops.count("SolveDiscreteARE") == 1, ops
    assert "HostPerform" not in ops
    out = f.maker.linker.last_ir
    # (the reference's graph returns float64 for float32 operands too; the device keeps its dtype)
    assert str(out.vars[out.outputs[0]].dtype) == X.dtype == "float64"


def test_batched_dare_is_one_blockwise_node(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_discrete_are

    ins = _inputs(ptt, batched=True)
    f = pytensor.function(list(ins), solve_discrete_are(*ins), mode="hip")
    nodes = f.maker.linker.last_ir.nodes
    bw = [n for n in nodes if n.op == "Blockwise"]
    assert len(bw) == 1 and bw[0].params["core_op"] == "SolveDiscreteARE"
    assert not any(n.op == "HostPerform" for n in nodes)


def test_dare_gradient_lowers(pt):
    """the reference's pullback (solve(assume_a="sym"), matrix_dot, a second DARE and the bilinear discrete
    Lyapunov solve) lowers with no new code and no host fallback"""
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_discrete_are

    ins = _inputs(ptt)
    X = solve_discrete_are(*ins)
    cost = (X ** 2).sum() + ptt.linalg.det(X)
    grads = pytensor.grad(cost, list(ins))
    f = pytensor.function(list(ins), [cost, *grads], mode="hip")
    ops = _ops(f)
    assert "HostPerform" not in ops
    assert "SolveDiscreteARE" in ops and "SolveSylvester" in ops
    # (the pullback builds its own SolveDiscreteARE instance, which the merge rewrite does not unify with the
    #  forward one: two launches per call, DESIGN §4 "Riccati")
    assert ops.count("SolveDiscreteARE") == 2


def test_batched_dare_gradient_lowers(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_discrete_are

    ins = _inputs(ptt, batched=True)
    X = solve_discrete_are(*ins)
    grads = pytensor.grad(X.sum(), list(ins))
    f = pytensor.function(list(ins), grads, mode="hip")
    assert "HostPerform" not in _ops(f)


def test_qz_family_stays_unlowered(pt):
    """the DARE is lowered on its own class; the decompositions its inner graph uses are not"""
    from pytensor.tensor.linalg import QZ, Schur

    from pytensor_amd.lower import hip_funcify

    for cls in (QZ, Schur):
        assert hip_funcify.dispatch(cls) is hip_funcify.dispatch(object), cls


def test_shape_validation(pt):
    import pytensor_amd.dispatch.riccati as r

    class _A:
        def __init__(self, *shape):
            self.shape = shape

    with pytest.raises(ValueError, match="incompatible shapes"):
        r._check_shapes(_A(3, 3), _A(3, 2), _A(3, 3), _A(3, 3))
    assert r._check_shapes(_A(4, 4), _A(4, 2), _A(4, 4), _A(2, 2)) == (4, 2)


def test_abi_declares_the_dare_entry_points():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    for name in ("pthip_dare", "pthip_dare_workspace", "pthip_dare_finish"):
        assert name in ffi.SIGNATURES and re.search(rf"\b{name}\s*\(", header)


def _smem_is_loads_only(asm: str):
    """every SMEM-encoded instruction (GFX9 encoding: the first dword's bits 31:26 are 110000) is a load"""
    bad, n = [], 0
    for line in asm.splitlines():
        m = re.match(r"\s+(s_\w+)\b.*//\s*[0-9A-Fa-f]+:\s*([0-9A-Fa-f]{8})", line)
        if not m:
            continue
        if (int(m.group(2), 16) >> 26) == 0b110000:
            n += 1
            if not m.group(1).startswith(("s_load_", "s_buffer_load_")):
                bad.append(m.group(1))
    return n, bad


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not found")
def test_riccati_hip_compiles_for_gfx950_without_scalar_memory_writes(tmp_path):
    src = os.path.join(ROOT, "pytensor_amd", "csrc", "riccati.hip")
    obj = str(tmp_path / "riccati_gfx950.o")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src,
                    "-o", obj], check=True, cwd=os.path.dirname(src))
    objdump = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
    if not os.path.exists(objdump):
        objdump = shutil.which("llvm-objdump")
    if objdump is None:
        pytest.skip("llvm-objdump not found")
    asm = subprocess.run([objdump, "-d", obj], check=True, capture_output=True, text=True).stdout
    assert "dare_sda_kernel" in asm and "dare_finish_kernel" in asm
    n, bad = _smem_is_loads_only(asm)
    assert n > 0, "no scalar memory instruction recognised: the disassembly format changed"
    assert not bad, sorted(set(bad))
    # every kernel's register use stays in registers
    notes = subprocess.run([objdump.replace("objdump", "readelf"), "--notes", obj], capture_output=True, text=True).stdout
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", notes)]
    assert spills and not any(spills), spills


def test_smem_classifier_recognises_a_write():
    # (a synthetic line whose SMEM opcode is not a load must be reported)
    assert _smem_is_loads_only("\ts_foo_dword s4, s[0:1], 0x0 // 000000000000: C0420100 00000000\n") == (1, ["s_foo_dword"])
    assert _smem_is_loads_only("\ts_load_dword s4, s[0:1], 0x0 // 000000000000: C0020100 00000000\n") == (1, [])
