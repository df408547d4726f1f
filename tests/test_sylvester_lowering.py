"""CPU: the Bartels-Stewart tier of ``SolveSylvester``: its ABI, its kernels' gfx950 code, the ``b_is_a_t`` flag of the
lowering (one Schur form for Lyapunov equations) and the tier choice."""
import os
import re
import shutil
import subprocess

import pytest

import make_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not make_ref.importable(), reason="no importable reference copy (oracle/_ref not built: the reference was not found)")


@pytest.fixture(scope="module")
def pt():
    make_ref.activate()
    import pytensor
    import pytensor.tensor as ptt

    import pytensor_amd

    pytensor_amd.register()
    return pytensor, ptt


def _sylvester_nodes(ir):
    """every SolveSylvester (or its Blockwise) node of a lowered graph, inner graphs included"""
    out = []
    for n in ir.nodes:
        if n.op == "SolveSylvester" or (n.op == "Blockwise" and n.params.get("core_op") == "SolveSylvester"):
            out.append(n)
        for v in n.params.values():
            for w in (v.values() if isinstance(v, dict) else [v]):
                if hasattr(w, "nodes"):
                    out.extend(_sylvester_nodes(w))
    return out


def _flags(f):
    nodes = _sylvester_nodes(f.maker.linker.last_ir)
    assert nodes
    return [n.params["b_is_a_t"] if n.op == "SolveSylvester" else n.params["core_params"]["b_is_a_t"] for n in nodes]


def test_abi_declares_the_sylvester_entry_points():
    from pytensor_amd import ffi

    header = open(os.path.join(ROOT, "include", "pthip.h")).read()
    for name in ("pthip_sylvester_workspace", "pthip_real_schur", "pthip_trsyl"):
        assert name in ffi.SIGNATURES and re.search(rf"\b{name}\s*\(", header), name


def test_tier_choice():
    from pytensor_amd.dispatch.decomp import sylvester_tier

    assert sylvester_tier(64, 64) == "kronecker"
    assert sylvester_tier(4096, 1) == "kronecker"
    assert sylvester_tier(65, 64) == "schur"
    assert sylvester_tier(300, 20) == sylvester_tier(20, 300) == "schur"
    assert sylvester_tier(1024, 1024) == "schur"
    assert sylvester_tier(1025, 8) is None and sylvester_tier(8, 1025) is None


def test_refusal_names_the_bound():
    from pytensor_amd.dispatch.decomp import _sylvester_refused

    assert "1024" in str(_sylvester_refused(2000, 3))


@needs_ref
def test_b_is_a_t_continuous_lyapunov(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_continuous_lyapunov

    A, Q = ptt.dmatrix("A"), ptt.dmatrix("Q")
    f = pytensor.function([A, Q], solve_continuous_lyapunov(A, Q), mode="hip")
    assert _flags(f) == [True]


@needs_ref
def test_b_is_a_t_bilinear_discrete_lyapunov(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_discrete_lyapunov

    A, Q = ptt.dmatrix("A"), ptt.dmatrix("Q")
    f = pytensor.function([A, Q], solve_discrete_lyapunov(A, Q, method="bilinear"), mode="hip")
    assert "HostPerform" not in [n.op for n in f.maker.linker.last_ir.nodes]
    assert _flags(f) == [True]


@needs_ref
def test_b_is_a_t_in_dare_gradient(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_discrete_are

    ins = [ptt.dmatrix(nm) for nm in "ABQR"]
    X = solve_discrete_are(*ins)
    f = pytensor.function(ins, pytensor.grad((X ** 2).sum(), ins), mode="hip")
    assert all(_flags(f))


@needs_ref
def test_b_is_a_t_false_for_independent_operands(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_sylvester

    A, B, C = ptt.dmatrix("A"), ptt.dmatrix("B"), ptt.dmatrix("C")
    f = pytensor.function([A, B, C], solve_sylvester(A, B, C), mode="hip")
    assert _flags(f) == [False]
    # (B = A, not A^T, and A^T with a different matrix: both false)
    f = pytensor.function([A, C], solve_sylvester(A, A, C), mode="hip")
    assert _flags(f) == [False]
    f = pytensor.function([A, B, C], solve_sylvester(A, B.T, C), mode="hip")
    assert _flags(f) == [False]


@needs_ref
def test_b_is_a_t_batched(pt):
    pytensor, ptt = pt
    from pytensor.tensor.linalg import solve_continuous_lyapunov, solve_sylvester

    A, B, C = ptt.dtensor3("A"), ptt.dtensor3("B"), ptt.dtensor3("C")
    f = pytensor.function([A, C], solve_continuous_lyapunov(A, C), mode="hip")
    assert _flags(f) == [True]
    f = pytensor.function([A, B, C], solve_sylvester(A, B, C), mode="hip")
    assert _flags(f) == [False]


@needs_ref
def test_schur_family_stays_unlowered(pt):
    from pytensor.tensor.linalg import QZ, Schur
    from pytensor.tensor.linalg.solvers.linear_control import TRSYL

    from pytensor_amd.lower import hip_funcify

    for cls in (QZ, Schur, TRSYL):
        assert hip_funcify.dispatch(cls) is hip_funcify.dispatch(object), cls


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
def test_sylvester_hip_compiles_for_gfx950_without_spills_or_scalar_memory_writes(tmp_path):
    src = os.path.join(ROOT, "pytensor_amd", "csrc", "sylvester.hip")
    obj = str(tmp_path / "sylvester_gfx950.o")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src,
                    "-o", obj], check=True, cwd=os.path.dirname(src))
    objdump = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
    if not os.path.exists(objdump):
        objdump = shutil.which("llvm-objdump")
    if objdump is None:
        pytest.skip("llvm-objdump not found")
    asm = subprocess.run([objdump, "-d", obj], check=True, capture_output=True, text=True).stdout
    assert "real_schur_kernel" in asm and "trsyl_kernel" in asm
    n, bad = _smem_is_loads_only(asm)
    assert n > 0, "no scalar memory instruction recognised: the disassembly format changed"
    assert not bad, sorted(set(bad))
    notes = subprocess.run([objdump.replace("objdump", "readelf"), "--notes", obj], capture_output=True, text=True).stdout
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", notes)]
    assert spills and not any(spills), spills
