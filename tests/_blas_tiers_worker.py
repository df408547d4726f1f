"""Device-side runners of the dense-BLAS sweep (tests/test_gpu_tiers_blas.py), and its child process.

As a module: ``run_gemm`` / ``run_partials`` / ``run_gemv`` / ``run_finish`` / ``run_ger`` upload the NaN-padded parents
of tests/blas_cases.py, call the C ABI with offset pointers, count the launches the call made and verify the sentinels
around every output.  ``job`` runs one named row of the table the same way in the parent and in the child.

As a program: ``_blas_tiers_worker.py OUT.npz JOB...`` — the ``PTHIP_*`` A/B switches are read once into ``static
const``s, so the parent sets them in the environment of a fresh child; the child runs the named jobs of the same table
and returns the raw outputs, which the parent checks with the same checker.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import blas_cases as bc  # noqa: E402

GUARD = 256  # bytes of sentinel on each side of an output


class Out:
    """An output of ``n`` elements inside a longer device buffer: sentinel bytes on both sides, NaN bits in between (an
    element the kernel does not write fails the checker)."""

    def __init__(self, n, dt, tail_guard_only=False):
        from pytensor_amd.device import DeviceArray

        self.dt, self.n = np.dtype(dt), int(n)
        nbytes = self.n * self.dt.itemsize
        self.lead = 0 if tail_guard_only else GUARD
        host = np.full(self.lead + nbytes + GUARD, 0xFF, dtype=np.uint8)
        pat = (np.arange(GUARD) * 37 + 11).astype(np.uint8)
        host[:self.lead] = pat[:self.lead]
        host[self.lead + nbytes:] = pat[::-1]
        self.host = host
        self.dev = DeviceArray.from_host(host)
        assert self.dev.ptr % 256 == 0
        self.ptr = self.dev.ptr + self.lead

    def fetch(self, shape=None):
        """the output; raises if a sentinel byte changed"""
        back = self.dev.to_host()
        nbytes = self.n * self.dt.itemsize
        assert np.array_equal(back[:self.lead], self.host[:self.lead]), "bytes in FRONT of the output were overwritten"
        assert np.array_equal(back[self.lead + nbytes:], self.host[self.lead + nbytes:]), "bytes BEHIND the output were overwritten"
        out = back[self.lead:self.lead + nbytes].view(self.dt).copy()
        return out.reshape(shape) if shape is not None else out


def upload(parent, off):
    """(owner, device pointer of element ``off``) of a host parent array"""
    from pytensor_amd.device import DeviceArray

    d = DeviceArray.from_host(np.ascontiguousarray(parent))
    assert d.ptr % 256 == 0
    return d, d.ptr + off * parent.itemsize


def _counted(ffi, fn, *args):
    lib = ffi.lib()
    before = lib.pthip_launch_count()
    rc = fn(*args)
    return rc, int(lib.pthip_launch_count() - before)


def run_gemm(ffi, dt, shape, alpha, opA, opB, beta=0.0, opC=None):
    """``pthip_gemm`` on Operand views; returns (out (batch, M, N), launches)"""
    nb, M, N, K = shape
    keep = []
    ptrs = []
    for op in (opA, opB, opC):
        if op is None:
            ptrs.append(None)
            continue
        d, p = upload(op.parent, op.off)
        keep.append(d)
        ptrs.append(p)
    out = Out(nb * M * N, dt)
    sC = (opC.sb, opC.s0, opC.s1) if opC is not None else (0, 0, 0)
    rc, launches = _counted(ffi, ffi.lib().pthip_gemm, ffi.np_dtype_code(dt), nb, M, N, K, float(alpha), ptrs[0], opA.sb, opA.s0, opA.s1,
                            ptrs[1], opB.sb, opB.s0, opB.s1, float(beta), ptrs[2], sC[0], sC[1], sC[2], out.ptr)
    ffi.check(rc)
    return out.fetch((nb, M, N)), launches


def run_partials(ffi, dt, shape, opA, opB, nslabs):
    """``pthip_gemm_partials``; returns (rc, part (nslabs, batch, M, N) or None, launches)"""
    nb, M, N, K = shape
    dA, pA = upload(opA.parent, opA.off)
    dB, pB = upload(opB.parent, opB.off)
    out = Out(max(nslabs, 1) * nb * M * N, dt)
    rc, launches = _counted(ffi, ffi.lib().pthip_gemm_partials, ffi.np_dtype_code(dt), nb, M, N, K, pA, opA.sb, opA.s0, opA.s1,
                            pB, opB.sb, opB.s0, opB.s1, out.ptr, nslabs)
    part = out.fetch((max(nslabs, 1), nb, M, N))
    return rc, (part if rc == 0 else None), launches


def sum_slabs(part):
    """the slabs added in ascending order, in the operand dtype (what splitk_finish_kernel and the consumers do)"""
    acc = part[0].copy()
    for s in range(1, part.shape[0]):
        acc = acc + part[s]
    return acc


def run_gemv(ffi, d, alpha, beta, ymode="null", sy=1):
    """``pthip_gemv`` on a blas_cases.GemvData; ymode "null" (no y), "nan" (a y full of NaN) or "vals".  The workspace is
    exactly ``pthip_gemv_workspace`` bytes with sentinels behind it.  Returns (out, launches)."""
    lib = ffi.lib()
    case, dt = d.case, d.dt
    code = ffi.np_dtype_code(dt)
    dA, pA = upload(d.a_parent, d.a_off)
    dx, px = upload(d.x_parent, d.x_off)
    py, dy = None, None
    if ymode != "null":
        yv = d.y if ymode == "vals" else np.full(case.M, np.nan, dt)
        yp, yo = bc.embed_vec(yv, sy)
        dy, py = upload(yp, yo)
    wsb = int(lib.pthip_gemv_workspace(code, case.M, case.N, d.sA0, d.sA1))
    ws = Out(wsb, np.uint8, tail_guard_only=True)
    out = Out(case.M, dt)
    rc, launches = _counted(ffi, lib.pthip_gemv, code, case.M, case.N, float(alpha), pA, d.sA0, d.sA1, px, case.sx, float(beta), py, sy,
                            out.ptr, ws.ptr, wsb)
    ffi.check(rc)
    ws.fetch()
    return out.fetch(), launches


def run_finish(ffi, dt, part, alpha, beta, y, sy):
    lib = ffi.lib()
    nparts, M = part.shape
    dp, pp = upload(part.reshape(-1), 0)
    py, dy = None, None
    if y is not None:
        yp, yo = bc.embed_vec(y, sy)
        dy, py = upload(yp, yo)
    out = Out(M, dt)
    rc, launches = _counted(ffi, lib.pthip_gemv_finish, ffi.np_dtype_code(dt), M, nparts, pp, float(alpha), float(beta), py, sy, out.ptr)
    ffi.check(rc)
    return out.fetch(), launches


def run_ger(ffi, dt, opA, x, sx, y, sy, alpha):
    lib = ffi.lib()
    _, M, N = opA.shape
    dA, pA = upload(opA.parent, opA.off)
    xp, xo = bc.embed_vec(x, sx)
    yp, yo = bc.embed_vec(y, sy)
    dx, px = upload(xp, xo)
    dy, py = upload(yp, yo)
    out = Out(M * N, dt)
    rc, launches = _counted(ffi, lib.pthip_ger, ffi.np_dtype_code(dt), M, N, float(alpha), pA, opA.s0, opA.s1, px, sx, py, sy, out.ptr)
    ffi.check(rc)
    return out.fetch((M, N)), launches


# ---------------------------------------------------------------------------------------------------------------
# jobs: one named row, run identically by the parent (default settings) and by the child (a switch set)
# ---------------------------------------------------------------------------------------------------------------
def long_row(name):
    _, M, N, K, trans = next(r for r in bc.LONG_ROWS if r[0] == name)
    return bc.GemmRow(name, 1, M, N, K, "long", "long"), trans


def job(ffi, spec):
    """``gemm:ROW:DT`` / ``long:ROW:DT`` / ``gemv:CASE:DT`` -> {key: array}: the output of the aligned call with
    alpha = -0.75, beta = 1.25, and for gemm rows ``route`` = [nslabs, launches, partials accepts nslabs and refuses
    nslabs + 1]"""
    kind, name, dt = spec.split(":")
    res = {}
    if kind in ("gemm", "long"):
        row, trans = (bc.GEMM_BY_NAME[name], False) if kind == "gemm" else long_row(name)
        d = bc.GemmData(row, dt)
        opA, opB, opC = bc.embed(d.A, trans=trans, **bc.ALIGNED), bc.embed(d.B, **bc.ALIGNED), bc.embed(d.C, **bc.ALIGNED)
        out, launches = run_gemm(ffi, dt, row.shape, bc.ALPHA, opA, opB, bc.BETA, opC)
        ns = int(ffi.lib().pthip_gemm_nslabs(*row.shape))
        ok = 0
        if kind == "gemm" and row.K > 0:
            rc, part, _ = run_partials(ffi, dt, row.shape, opA, opB, ns)
            rc2, _, n2 = run_partials(ffi, dt, row.shape, opA, opB, ns + 1)
            ok = int(rc == 0 and rc2 != 0 and n2 == 0)
            if rc == 0:
                res[spec + ":psum"] = sum_slabs(part)
        res[spec] = out
        res[spec + ":route"] = np.array([ns, launches, ok], dtype=np.int64)
    elif kind == "gemv":
        d = bc.gemv_data(bc.GEMV_BY_NAME[name], dt)
        out, launches = run_gemv(ffi, d, bc.ALPHA, bc.BETA, "vals", 1)
        res[spec] = out
        res[spec + ":route"] = np.array([0, launches, 0], dtype=np.int64)
    else:
        raise ValueError(spec)
    return res


def main(argv):
    from pytensor_amd import ffi

    ffi.init(0)
    res = {}
    for spec in argv[2:]:
        res.update(job(ffi, spec))
    np.savez(argv[1], **res)


if __name__ == "__main__":
    main(sys.argv)
