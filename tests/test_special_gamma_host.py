"""CPU: the device helpers of csrc/special_gammainc.h, special_betainc.h, special_polygamma.h and special_betaincinv.h
compiled for the host.

The same text the generated kernels carry (``codegen_scalar.prelude_for``: the generated log-factorial tables, then the
headers) is built with a host C++ compiler (``PT_DEV`` / ``__device__`` defined away, standard ``<cmath>`` only) and
checked against what the reference evaluates: its C backend's incomplete gamma / beta (restated by
oracle/special_c.py, which tests/test_oracle.py pins to the reference's C results) and SciPy's polygamma / betaincinv.
special_ndtri_exp.h and special_gammaincinv.h (the device library's ``erfcinv``) and scalar_device.h (``__builtin_amdgcn_*``)
have no host build.
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
#define PT_DEV static inline
#define __device__
%s
#include "special_gammainc.h"
#include "special_betainc.h"
#include "special_polygamma.h"
#include "special_betaincinv.h"
extern "C" void pt_eval(int op, long n, const double* a, const double* b, const double* c, double* out) {
  for (long i = 0; i < n; i++)
    out[i] = op == 0 ? pt_gammainc(a[i], b[i]) : op == 1 ? pt_gammaincc(a[i], b[i]) : op == 2 ? pt_betainc(a[i], b[i], c[i])
           : op == 3 ? pt_polygamma(a[i], b[i]) : pt_betaincinv(a[i], b[i], c[i]);
}
"""
OPS = {"gammainc": 0, "gammaincc": 1, "betainc": 2, "polygamma": 3, "betaincinv": 4}

# the project's fp64 parity tolerance.  Measured with g++ 11 on these inputs: gammainc / gammaincc 5000 of 5000 bit-equal to
# the oracle; betainc max relative difference 1.6e-15; polygamma 1.3e-14 and betaincinv 7.6e-14 against SciPy
RTOL = 1e-12


def _compiler():
    for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    from pytensor_amd import codegen_scalar

    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("special_gamma_host")
    src, so = d / "drv.cpp", d / "drv.so"
    src.write_text(DRIVER % codegen_scalar.gamma_tables_src())
    # -ffp-contract=off: the host compiler must not fuse what the device code rounds separately
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", str(src), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def ev(L, op, a, b, c=None):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    c = np.ascontiguousarray(a if c is None else c, np.float64)
    assert a.shape == b.shape == c.shape
    out = np.empty_like(a)
    P = ctypes.POINTER(ctypes.c_double)
    L.pt_eval(OPS[op], ctypes.c_long(a.size), a.ctypes.data_as(P), b.ctypes.data_as(P), c.ctypes.data_as(P), out.ctypes.data_as(P))
    return out


@pytest.fixture(scope="module")
def gamma_points():
    rng = np.random.default_rng(0)
    k = np.concatenate([rng.uniform(0.05, 30.0, 4000), rng.integers(1, 200, 500).astype(np.float64), rng.integers(0, 100, 500) + 0.5])
    x = rng.uniform(0.0, 60.0, k.size) * rng.choice([0.01, 1.0, 3.0], k.size)
    return k, x


@pytest.mark.parametrize("name", ["gammainc", "gammaincc"])
def test_incomplete_gamma_against_the_c_oracle(lib, gamma_points, name):
    import special_c

    k, x = gamma_points
    ref = {"gammainc": special_c.GammaInc, "gammaincc": special_c.GammaIncC}[name](k, x)
    got = ev(lib, name, k, x)
    assert (np.isnan(got) == np.isnan(ref)).all()
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)


def test_incomplete_beta_against_the_c_oracle(lib):
    import special_c

    rng = np.random.default_rng(0)
    a, b, x = rng.uniform(0.1, 40.0, 5000), rng.uniform(0.1, 40.0, 5000), rng.uniform(0.0, 1.0, 5000)
    np.testing.assert_allclose(ev(lib, "betainc", a, b, x), special_c.BetaInc(a, b, x), rtol=RTOL, atol=0)


def test_polygamma_against_scipy(lib):
    sp = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(0)
    n, x = rng.integers(0, 6, 3000).astype(np.float64), rng.uniform(0.1, 30.0, 3000)
    got = ev(lib, "polygamma", n, x)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, sp.polygamma(n, x), rtol=RTOL, atol=0)


def test_betaincinv_against_scipy(lib):
    sp = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(0)
    # (a, b over the range of the incomplete-beta test above)
    a, b, p = rng.uniform(0.1, 40.0, 3000), rng.uniform(0.1, 40.0, 3000), rng.uniform(0.001, 0.999, 3000)
    got = ev(lib, "betaincinv", a, b, p)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, sp.betaincinv(a, b, p), rtol=RTOL, atol=0)
