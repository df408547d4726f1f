"""Device time of pthip_gemm for a few shapes (HIP events around back-to-back launches).

usage: python tools/bench_gemm.py [shape indices]
       python tools/bench_gemm.py half     (pthip_hgemm against cast + fp32 product + cast, four orientations)
       python tools/bench_gemm.py attention  (pthip_hattention against the unfused float16 and float32 chains)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytensor_amd import ffi  # noqa: E402
from pytensor_amd.device import DeviceArray  # noqa: E402

PEAK = {"float64": 78.6, "float32": 157.3}


def timed(lib, fn, reps):
    e0, e1 = C.c_void_p(), C.c_void_p()
    ffi.check(lib.pthip_event_create(C.byref(e0)))
    ffi.check(lib.pthip_event_create(C.byref(e1)))
    for _ in range(3):
        fn()
    ffi.check(lib.pthip_event_record(e0))
    for _ in range(reps):
        fn()
    ffi.check(lib.pthip_event_record(e1))
    ffi.check(lib.pthip_event_synchronize(e1))
    ms = C.c_float()
    ffi.check(lib.pthip_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / reps


# the last three are deep-K shapes with few tiles (split-K): 512 x 512 x 65536 in orientation TN is the weight gradient
# x.T @ gy of a 512 -> 512 dense layer at batch 65536
HALF_SHAPES = [(1, 4096, 4096, 4096), (512, 256, 256, 256), (1, 64, 4096, 4096), (1, 512, 512, 65536), (1, 16, 4096, 4096),
               (1, 64, 1024, 32768)]
HALF_GEMV = [(4, 10 ** 6), (1, 10 ** 7)]  # (M, K), row layout: four long rows, the inner product
ORIENT = (("NN", False, False), ("NT", False, True), ("TN", True, False), ("TT", True, True))


def half_rows(lib):
    """float16 products (pthip_hgemm) in the four operand orientations, next to what a user had to write before it
    existed: cast both operands to float32, the fp32 product, cast back — same buffers, same run, alternating.  The
    fp16 MFMA peak is 256 CUs x 4 SIMDs x 1024 flop/cycle (a 32x32x16 MFMA is 32768 flop in 32 cycles) at the clock the
    device reports."""
    from pytensor_amd.dispatch.elemwise import _StreamEnv, _cast

    khz = C.c_int()
    assert C.CDLL("libamdhip64.so").hipDeviceGetAttribute(C.byref(khz), 5, 0) == 0  # hipDeviceAttributeClockRate
    mhz = khz.value / 1e3
    peak = 256 * 4 * 1024 * mhz * 1e6 / 1e12
    env = _StreamEnv()
    rng = np.random.default_rng(0)
    f32 = ffi.np_dtype_code("float32")
    for batch, M, N, K in HALF_SHAPES:
        A = DeviceArray.from_host(rng.standard_normal((batch, M, K)).astype(np.float16))
        B = DeviceArray.from_host(rng.standard_normal((batch, K, N)).astype(np.float16))
        out = DeviceArray.empty((batch, M, N), "float16")
        for tag, tA, tB in ORIENT:
            # the same buffers read as the stored transposes: other operand values, the same work
            (a0, a1), (b0, b1) = ((1, M) if tA else (K, 1)), ((1, K) if tB else (N, 1))

            def half():
                ffi.check(lib.pthip_hgemm(batch, M, N, K, A.ptr, M * K, a0, a1, B.ptr, K * N, b0, b1, out.ptr))

            def cast_sgemm():
                A32, B32 = _cast(env, A, "float32"), _cast(env, B, "float32")
                o32 = DeviceArray.empty((batch, M, N), "float32")
                ffi.check(lib.pthip_gemm(f32, batch, M, N, K, 1.0, A32.ptr, M * K, a0, a1, B32.ptr, K * N, b0, b1, 0.0, None, 0, 0, 0, o32.ptr))
                return _cast(env, o32, "float16")

            runs = [(timed(lib, half, 20), timed(lib, cast_sgemm, 20)) for _ in range(2)]
            ms_h, ms_c = min(r[0] for r in runs), min(r[1] for r in runs)
            tf = 2.0 * batch * M * N * K / ms_h / 1e9
            print(json.dumps({"dtype": "float16", "batch": batch, "M": M, "N": N, "K": K, "orient": tag, "hgemm_ms": round(ms_h, 4),
                              "S": lib.pthip_hgemm_splits(batch, M, N, K),
                              "cast_sgemm_ms": round(ms_c, 4), "speedup": round(ms_c / ms_h, 2), "TFLOPs": round(tf, 1),
                              "clock_MHz": round(mhz), "peak_TFLOPs": round(peak, 1), "frac": round(tf / peak, 3),
                              "runs_ms": [[round(v, 4) for v in r] for r in runs]}), flush=True)
    for M, K in HALF_GEMV:  # bandwidth-bound: GB/s of A and x read once
        A = DeviceArray.from_host(rng.standard_normal((M, K)).astype(np.float16))
        x = DeviceArray.from_host(rng.standard_normal(K).astype(np.float16))
        out = DeviceArray.empty((M,), "float16")

        def gemv():
            ffi.check(lib.pthip_hgemv(M, K, A.ptr, K, 1, x.ptr, 1, out.ptr))

        runs = [timed(lib, gemv, 20) for _ in range(2)]
        print(json.dumps({"dtype": "float16", "op": "hgemv", "M": M, "K": K, "S": lib.pthip_hgemv_splits(M, K, K, 1), "hgemv_ms": round(min(runs), 4),
                          "GBs": round(2.0 * (M + 1) * K / min(runs) / 1e6, 1), "runs_ms": [round(v, 4) for v in runs]}), flush=True)


ATTENTION_SHAPES = [(16, 1024, 1024, 64), (16, 4096, 4096, 128), (64, 128, 128, 64)]  # (batch, S, T, D = Dv)


def attention_rows(lib):
    """float16 attention softmax(q k^T / sqrt(D)) v: the fused kernel (pthip_hattention), this build's unfused float16
    chain (what PTHIP_ATTENTION=0 runs: hgemm, scale, float16 softmax, hgemm) and the float32 form of the same chain
    (what a user had to write before float16 softmax existed: fp32 products with the scale as alpha, fp32 softmax) —
    same process, alternating, three rounds; every round's time is reported."""
    from pytensor_amd.dispatch import blas
    from pytensor_amd.dispatch.elemwise import _StreamEnv

    env = _StreamEnv()
    env.to_device = lambda x: x  # (every operand here is on the device already)
    rng = np.random.default_rng(0)
    f32 = ffi.np_dtype_code("float32")
    for nb, S, T, D in ATTENTION_SHAPES:
        host = [rng.standard_normal(s).astype(np.float16) for s in ((nb, S, D), (nb, T, D), (nb, T, D))]
        q, k, v = (DeviceArray.from_host(x) for x in host)
        q32, k32, v32 = (DeviceArray.from_host(x.astype(np.float32)) for x in host)
        kT, kT32 = (x.view((nb, D, T), (T * D, 1, D)) for x in (k, k32))
        scale = float(np.float16(D ** -0.5))
        sc = DeviceArray.from_host(np.array([scale], np.float16))
        out = DeviceArray.empty((nb, S, D), "float16")

        def fused():
            ffi.check(lib.pthip_hattention(nb, S, T, D, D, q.ptr, S * D, D, k.ptr, T * D, D, v.ptr, T * D, D, sc.ptr, 0, out.ptr))

        def unfused():
            return blas._attention_unfused(env, q, kT, v, sc, "mul")

        def float32():
            s = blas.gemm_device(env, scale, q32, kT32, batch=True)
            p = DeviceArray.empty(s.shape, "float32")
            ffi.check(lib.pthip_softmax(f32, 0, nb * S, T, s.ptr, p.ptr))
            return blas.gemm_device(env, 1.0, p, v32, batch=True)

        reps = 5 if S * T >= 1 << 24 else 20
        runs = [[timed(lib, f, reps) for f in (fused, unfused, float32)] for _ in range(3)]
        best = [min(r[i] for r in runs) for i in range(3)]
        print(json.dumps({"op": "attention", "batch": nb, "S": S, "T": T, "D": D, "fused_ms": round(best[0], 4), "unfused_ms": round(best[1], 4),
                          "float32_ms": round(best[2], 4), "vs_unfused": round(best[1] / best[0], 2), "vs_float32": round(best[2] / best[0], 2),
                          "TFLOPs": round(4.0 * nb * S * T * D / best[0] / 1e9, 1), "runs_ms": [[round(x, 4) for x in r] for r in runs]}), flush=True)


def main():
    ffi.init(0)
    lib = ffi.lib()
    if sys.argv[1:] == ["half"]:  # the float16 rows only
        return half_rows(lib)
    if sys.argv[1:] == ["attention"]:
        return attention_rows(lib)
    shapes = [
        ("float32", 1, 4096, 4096, 4096), ("float32", 1, 8192, 8192, 1024), ("float32", 512, 256, 256, 256),
        ("float32", 64, 1024, 1024, 256), ("float64", 1, 4096, 4096, 4096), ("float32", 1, 64, 2048, 1024),
        ("float32", 1, 64000, 1024, 1024),  # the hoisted x_t @ W of config #5 (T*B rows)
        # mid-size fp64 products (the solve steps of the blocked triangular solve, GP graphs): 64 x 64 tiles since round 5
        ("float64", 1, 512, 2048, 512), ("float64", 1, 1024, 1024, 1024), ("float64", 1, 512, 512, 512), ("float64", 1, 256, 2048, 256),
        ("float64", 1, 1024, 2048, 1024), ("float64", 1, 2048, 2048, 2048),
    ]
    if len(sys.argv) > 1:  # indices of the shapes to run (profiling one kernel at a time)
        shapes = [shapes[int(a)] for a in sys.argv[1:]]
    for dtype, batch, M, N, K in shapes:
        A = DeviceArray.empty((batch, M, K), dtype)
        B = DeviceArray.empty((batch, K, N), dtype)
        out = DeviceArray.empty((batch, M, N), dtype)
        # N(0,1) operands (all-zero ones run ~8 % faster: data-dependent power, tools/clock_probe.py)
        rng = np.random.default_rng(0)
        keep = []
        for x in (A, B):
            chunk = rng.normal(size=min(x.size, 1 << 24)).astype(dtype)
            keep.append(chunk)
            for off in range(0, x.size, chunk.size):
                n = min(chunk.size, x.size - off)
                ffi.check(lib.pthip_h2d(x.ptr + off * chunk.itemsize, chunk.ctypes.data, n * chunk.itemsize))
        ffi.check(lib.pthip_synchronize())
        dt = ffi.np_dtype_code(dtype)

        def run():
            ffi.check(lib.pthip_gemm(dt, batch, M, N, K, 1.0, A.ptr, M * K, K, 1, B.ptr, K * N, N, 1, 0.0, None, 0, 0, 0, out.ptr))

        # the very first launch of this shape on fresh buffers, timed on its own: rocprofv3 summaries of the bench show one
        # 25-27 ms launch per GEMM kernel (profiles/r3z_c3_kernel_stats.md max column) — is it this one?
        e0, e1 = C.c_void_p(), C.c_void_p()
        ffi.check(lib.pthip_event_create(C.byref(e0)))
        ffi.check(lib.pthip_event_create(C.byref(e1)))
        firsts = []
        for _ in range(3):
            ffi.check(lib.pthip_event_record(e0))
            run()
            ffi.check(lib.pthip_event_record(e1))
            ffi.check(lib.pthip_event_synchronize(e1))
            m1 = C.c_float()
            ffi.check(lib.pthip_event_elapsed_ms(e0, e1, C.byref(m1)))
            firsts.append(round(m1.value, 4))
        ms = timed(lib, run, 10)
        tf = 2.0 * batch * M * N * K / ms / 1e9
        rec = {"dtype": dtype, "batch": batch, "M": M, "N": N, "K": K, "ms": round(ms, 4), "TFLOPs": round(tf, 1), "frac": round(tf / PEAK[dtype], 3),
               "first_three_launches_ms": firsts}
        if dtype == "float32" and M % 256 == 0 and N % 256 == 0 and os.environ.get("PTHIP_BENCH_ORIENT", "1") != "0":
            # the same product with A and / or B stored transposed (strides swapped: same buffers, other operand values)
            for tag, (a0, a1), (b0, b1) in (("NT", (K, 1), (1, K)), ("TN", (1, M), (N, 1)), ("TT", (1, M), (1, K))):
                def run_o(a0=a0, a1=a1, b0=b0, b1=b1):
                    ffi.check(lib.pthip_gemm(dt, batch, M, N, K, 1.0, A.ptr, M * K, a0, a1, B.ptr, K * N, b0, b1, 0.0, None, 0, 0, 0, out.ptr))
                mo = timed(lib, run_o, 10)
                rec[f"frac_{tag}"] = round(2.0 * batch * M * N * K / mo / 1e9 / PEAK[dtype], 3)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
