"""CPU: csrc/schur_device.h (the core of csrc/sylvester.hip) compiled for the host with a team of one thread.

The real Schur form (Hessenberg reduction + Francis double-shift QR) is checked for backward error, orthogonality,
quasi-triangular standard form, eigenvalues and bounded iteration counts on random, companion, rotation-heavy,
defective and nearly-repeated-eigenvalue matrices; the quasi-triangular Sylvester solve against SciPy.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pytensor_amd", "csrc")

DRIVER = r"""
#include <cmath>
using namespace std;
#define SCHUR_DEV static inline
#define SCHUR_SYNC() ((void)0)
#define SCHUR_TEAM_MAX(v) (v)
#include "schur_device.h"
extern "C" int pt_real_schur(int n, double* H, double* Zt, int* counts) {
  return pt_schur::real_schur(H, Zt, n, n, 0, 1, counts, counts + 1);
}
extern "C" void pt_trsyl(int m, int n, const double* R, const double* S, double* F, int trans) {
  pt_schur::trsyl(R, m, S, n, F, n, m, n, trans != 0, 0, 1);
}
"""
P = ctypes.POINTER(ctypes.c_double)


def _compiler():
    for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("schur_host")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def schur(L, A):
    """(T, Z, info, max iterations per deflation, sweeps) with A = Z T Z^T"""
    n = A.shape[0]
    H = np.array(A, dtype=np.float64, order="C")
    Zt = np.zeros((n, n))
    counts = np.zeros(2, np.int32)
    info = L.pt_real_schur(n, H.ctypes.data_as(P), Zt.ctypes.data_as(P), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return H, Zt.T.copy(), info, int(counts[0]), int(counts[1])


def trsyl(L, R, S, F, trans):
    m, n = F.shape
    Y = np.array(F, dtype=np.float64, order="C")
    R, S = np.ascontiguousarray(R, dtype=np.float64), np.ascontiguousarray(S, dtype=np.float64)
    L.pt_trsyl(m, n, R.ctypes.data_as(P), S.ctypes.data_as(P), Y.ctypes.data_as(P), int(trans))
    return Y


def _orth(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def make(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.normal(size=(n, n))
    if kind == "companion":  # AR(p) / seasonal state transition: coefficients in the first row, shifted identity below
        A = np.zeros((n, n))
        A[0] = 0.3 * rng.normal(size=n) / np.sqrt(n)
        A[0, -1] += 0.9 if n > 1 else 0.0
        A[1:, :-1] += np.eye(n - 1)
        return A
    if kind == "rotation":  # many 2x2 blocks: rotations by assorted angles, conjugated by an orthogonal matrix
        D = np.zeros((n, n))
        for k in range(0, n - 1, 2):
            th = rng.uniform(0.1, 3.0)
            r = rng.uniform(0.5, 2.0)
            D[k:k + 2, k:k + 2] = r * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        if n % 2:
            D[-1, -1] = rng.normal()
        Q = _orth(rng, n)
        return Q @ D @ Q.T
    if kind == "defective":  # Jordan blocks of size <= 3
        J = np.diag(rng.normal(size=n))
        k = 0
        while k < n:
            s = min(int(rng.integers(1, 4)), n - k)
            J[k:k + s, k:k + s] = np.diag(np.full(s, J[k, k])) + np.diag(np.ones(s - 1), 1)
            k += s
        Q = _orth(rng, n)
        return Q @ J @ Q.T
    if kind == "near_repeated":  # eigenvalues in tight clusters
        ev = np.repeat(rng.normal(size=(n + 2) // 3), 3)[:n] + 1e-9 * rng.normal(size=n)
        Q = _orth(rng, n)
        return Q @ np.diag(ev) @ Q.T
    raise ValueError(kind)


KINDS = ["random", "companion", "rotation", "defective", "near_repeated"]
SIZES = [1, 2, 3, 17, 64, 150]


def _blocks(T):
    """diagonal block starts and sizes of a quasi-triangular T"""
    n, k, out = T.shape[0], 0, []
    while k < n:
        s = 2 if k + 1 < n and T[k + 1, k] != 0 else 1
        out.append((k, s))
        k += s
    return out


def _eigs_of_quasi(T):
    ev = []
    for k, s in _blocks(T):
        ev.extend(np.linalg.eigvals(T[k:k + s, k:k + s]) if s == 2 else [T[k, k]])
    return np.array(ev, dtype=complex)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_real_schur_form(lib, kind, n):
    from scipy.optimize import linear_sum_assignment

    A = make(kind, n, 100 * n + KINDS.index(kind))
    T, Z, info, max_its, sweeps = schur(lib, A)
    assert info == 0
    assert max_its < 30 * max(10, n)  # (the cap per deflation)
    nA = np.linalg.norm(A)
    assert np.linalg.norm(Z @ T @ Z.T - A) <= 1e-13 * max(n, 1) * nA
    assert np.linalg.norm(Z.T @ Z - np.eye(n)) <= 1e-13 * max(n, 1)
    assert not np.any(np.tril(T, -2)), "nonzero below the subdiagonal"
    sub = np.diag(T, -1) != 0
    assert not np.any(sub[1:] & sub[:-1]), "two consecutive nonzero subdiagonal entries"
    for k, s in _blocks(T):
        if s == 2:  # standard form: equal diagonal, off-diagonals of opposite sign
            assert T[k, k] == T[k + 1, k + 1]
            assert T[k, k + 1] * T[k + 1, k] < 0
    got, want = _eigs_of_quasi(T), np.linalg.eigvals(A)
    cost = np.abs(got[:, None] - want[None, :])
    r, c = linear_sum_assignment(cost)
    # (a Jordan block of size 3 moves its eigenvalue by eps^(1/3) under a perturbation of size eps)
    tol = (3e-5 if kind == "defective" else 1e-7 if kind == "near_repeated" else 1e-10) * max(nA, 1.0)
    assert cost[r, c].max() <= tol


def test_iteration_counts_stay_small(lib):
    """a sweep count of about two per eigenvalue, far from the cap"""
    for kind in KINDS:
        T, Z, info, max_its, sweeps = schur(lib, make(kind, 150, 7))
        assert info == 0 and max_its <= 40 and sweeps <= 4 * 150, (kind, max_its, sweeps)


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("mn", [(1, 1), (2, 3), (17, 5), (64, 64), (40, 150)])
def test_trsyl_against_scipy(lib, trans, mn):
    import scipy.linalg as sl

    m, n = mn
    rng = np.random.default_rng(m * 1000 + n)
    R, _, info_r, _, _ = schur(lib, make("rotation", m, m) + 3.0 * np.eye(m))
    S, _, info_s, _, _ = schur(lib, make("random", n, n) + 3.0 * np.sqrt(n) * np.eye(n))
    assert info_r == info_s == 0
    F = rng.normal(size=(m, n))
    Y = trsyl(lib, R, S, F, trans)
    opS = S.T if trans else S
    want = sl.solve_sylvester(R, opS, F)
    assert np.max(np.abs(Y - want)) <= 1e-11 * np.max(np.abs(want))
    assert np.max(np.abs(R @ Y + Y @ opS - F)) <= 1e-12 * max(m, n) * np.max(np.abs(F))


def test_nearly_resonant_pair_stays_finite(lib):
    """A and -B share an eigenvalue (exactly and within 1e-17): the pivot is raised to smin, as dtrsyl does"""
    R = np.array([[1.0, 2.0], [0.0, 3.0]])
    for S in (np.array([[-1.0]]), np.array([[-3.0 + 1e-17]]), np.array([[-1.0, 5.0], [0.0, -7.0]])):
        Y = trsyl(lib, R, S, np.ones((2, S.shape[0])), False)
        assert np.all(np.isfinite(Y)), Y


def test_lyapunov_transposed_solve(lib):
    """R Y + Y R^T = F with one Schur form (the Lyapunov case)"""
    import scipy.linalg as sl

    A = make("random", 30, 5) - 6.0 * np.eye(30)
    R, U, info, _, _ = schur(lib, A)
    Q = np.random.default_rng(1).normal(size=(30, 30))
    Y = trsyl(lib, R, R, U.T @ Q @ U, True)
    X = U @ Y @ U.T
    assert np.max(np.abs(X - sl.solve_continuous_lyapunov(A, Q))) <= 1e-12 * np.max(np.abs(X))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_operand_is_flagged(lib, bad):
    """a non-finite operand gives info = -1, which the device turns into an all-NaN X (as Schur.perform NaN-fills)"""
    A = make("random", 5, 3)
    A[2, 4] = bad
    _, _, info, _, _ = schur(lib, A)
    assert info == -1


def test_empty_and_scalar(lib):
    T, Z, info, _, _ = schur(lib, np.array([[2.5]]))
    assert info == 0 and T[0, 0] == 2.5 and Z[0, 0] == 1.0
    Y = trsyl(lib, np.array([[2.0]]), np.array([[3.0]]), np.array([[10.0]]), False)
    assert Y[0, 0] == 2.0
