"""Skinny product + epilogue (gemmfuse.fuse_dot_epilogue): out = body(.., A@B, ..)"""

from __future__ import annotations

from pytensor_amd.codegen import BLOCK
from pytensor_amd.codegen_scalar import CTYPE, emit_body, prelude_for

DOTEW_CHUNK = 8  # k-groups (16 k each) per register buffer; two buffers in flight
DOTEW_MAX_K = 16384
_MFMA16 = {"float32": "__builtin_amdgcn_mfma_f32_16x16x4f32", "float64": "__builtin_amdgcn_mfma_f64_16x16x4f64"}


def dot_epilogue_source(name: str, body: dict, dot_pos, K: int, byvalue=(), chunk: int = DOTEW_CHUNK, share=None, lds_a: bool = False, var: str = "",
                        packed_a=(), pack_outs=()) -> str:
    """One 16x16 output tile per workgroup of ``out = body(.., A_d @ B_d, ..)``, full K.

    The recurrent products of a Scan step (``h @ U``: M = batch <= a few hundred rows, K = N =
    hidden) followed by their gate ``Composite``: reference ``Dot22``/``Gemm`` (blas/gemm.py:
    76, 248) + ``Elemwise`` (elemwise.py:755) of one step in ONE launch, no split-K slabs through
    HBM, no finish pass.  MI355X mapping: 256 tiles for (64, 1024) = one per CU; the four waves
    split K, each lane streams its operands with 16-byte loads straight into the MFMA operand
    registers (``v_mfma_*_16x16x4``: lane (i = l%16, q = l/16) supplies A[i][k] and B[k][i] for
    k = 16g + 4q + j, j = 0..3 — one 4-vector load per operand feeds four MFMAs).  ``B`` arrives
    packed by ``pthip_pack_b16`` as ``[N/16][K/4][16][4]`` so that a wave's load is 1 KiB
    contiguous; A is row-major (16 rows x 64 B per instruction).  The wave partials are added in
    wave order through LDS (deterministic), then thread t owns element (t/16, t%16) of the tile
    and runs the scalar graph; operands of the epilogue are requested before the K loop.

    ``share``: ``{follower dot position: leader dot position}`` — products with the SAME left
    operand (``h @ U_r`` and ``h @ U_z``): the leader's A registers feed both MFMA chains, the
    follower loads only its packed B (64 KB less per tile, and two independent accumulator chains).

    ``lds_a`` (float32, K % 128 == 0): the left operand is fetched in full 128-byte lines by
    LDS-DMA (``global_load_lds`` x4: per wave and pair of k-groups two 1 KiB copies, lane = (row l/8,
    16-byte piece l%8 XOR row&7 on the source side so that the linear LDS image is bank-swizzled) and
    the MFMA fragments are read back with ``ds_read_b128`` — instead of fragment-shaped loads (16 rows x
    64 B per instruction), which the texture addresser serves at half rate.  Wave-local: no barrier.

    ``var``: ``"acc4"`` (the default of dispatch/dotew.py) / ``"acc2"`` split every product's
    accumulator into 4 / 2 chains (k-groups round-robin; two chains each when two products share
    their left operand), added in a fixed order at the end.  Measured: no time (the kernels wait on
    memory, profiles/r3a_dotew_variants.txt) but accuracy — an MFMA chain is a k-ordered fma chain,
    and 1000 GRU steps of 256-term chains drifted 1.3x further from the fp64 trajectory than
    OpenBLAS's blocked sums; shorter chains close most of that (tests/test_gpu_fullsize.py).
    The other values are TIMING-ONLY decompositions (wrong results; tools/dotew_variants.py):
    ``nomfma`` (VALU stand-ins for the MFMAs), ``noload`` (operands from a kernel argument),
    ``apacked`` (the left operand fetched with the packed operand's 1-KiB-contiguous pattern).

    ``packed_a``: dot positions whose LEFT operand arrives in the MFMA operand order as well
    (``Ap[M/16][K/4][16][4]``, ``Ap[rt][k4][i][j] = A[16 rt + i][4 k4 + j]``): a wave's load is then
    1 KiB contiguous like the packed right operand, instead of 16 row segments of 64 B (measured
    with the timing-only ``apacked`` variant: -1.1 us per GRU step, profiles/r3a_dotew_variants.txt).
    ``pack_outs``: outputs this kernel ALSO stores in that order (one extra pointer each, after the
    regular outputs) because a later step kernel multiplies them from the left: the 16x16 tile a
    workgroup owns is one contiguous 1 KiB piece of the packed image.  Needs N % 16 == 0.

    Arguments: M, N, then per body input — dot: (A, lda, Bp) | by value: bits | other:
    (ptr, stride0, stride1) — then per output (ptr, row stride), then per packed output its pointer."""
    dot_pos = list(dot_pos)
    packed_a = set(packed_a)
    pack_outs = list(pack_outs)
    nacc = 4 if "acc4" in var else 2 if "acc2" in var else 1
    byvalue = set(byvalue)
    T = body["in_dtypes"][dot_pos[0]]
    assert T in _MFMA16 and all(body["in_dtypes"][p] == T for p in dot_pos)
    assert K % 16 == 0 and 0 < K <= DOTEW_MAX_K
    ct = CTYPE[T]
    G = K // 16
    GW = (G + 3) // 4
    guard = G % 4 != 0
    nd = len(dot_pos)
    P = ["long long M", "long long N"]
    for k, dt in enumerate(body["in_dtypes"]):
        if k in dot_pos:
            P += [f"const {ct}* __restrict__ A{k}", f"long long lda{k}", f"const {ct}* __restrict__ Bp{k}"]
        elif k in byvalue:
            P.append(f"const long long in{k}")
        else:
            P += [f"const {CTYPE[dt]}* __restrict__ in{k}", f"long long s{k}_0", f"long long s{k}_1"]
    for k, dt in enumerate(body["out_dtypes"]):
        P += [f"{CTYPE[dt]}* __restrict__ out{k}", f"long long ldo{k}"]
    for k in pack_outs:
        P.append(f"{CTYPE[body['out_dtypes'][k]]}* __restrict__ pk{k}")
    L = [prelude_for(body)]
    L.append(f"typedef {ct} __attribute__((ext_vector_type(4))) dvec4;")
    L.append(f'extern "C" __global__ __launch_bounds__({BLOCK}) void {name}({", ".join(P)}) {{')
    lds_a = bool(lds_a) and T == "float32" and K % 128 == 0 and chunk % 2 == 0
    L.append(f"  __shared__ {ct} red_[{nd}][4][256];")
    if lds_a:
        # per wave: two buffers of `chunk` k-groups = chunk/2 line pairs of 16 rows x 128 B
        L.append(f"  __shared__ __attribute__((aligned(16))) float lda_[4][2][{chunk // 2}][16 * 32];")
    L.append("  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;")
    L.append("  const long long ctile = blockIdx.x, r0 = (long long)blockIdx.y * 16;")
    L.append("  const long long er = r0 + (tid >> 4), ec = ctile * 16 + (tid & 15);")
    L.append("  const bool live = er < M && ec < N;")
    L.append("  const long long err = live ? er : 0, ecc = live ? ec : 0;")
    in_names, early, ew_loads = [], [], []
    for k, dt in enumerate(body["in_dtypes"]):
        if k in dot_pos:
            in_names.append(f"dot{k}")
        elif k in byvalue:
            c = CTYPE[dt]
            L.append(f"  {c} bv{k}; {{ const long long b = in{k}; __builtin_memcpy(&bv{k}, &b, sizeof({c})); }}")
            in_names.append(f"bv{k}")
        else:
            ew_loads.append(f"  {CTYPE[dt]} e{k} = in{k}[err * s{k}_0 + ecc * s{k}_1];")
            in_names.append(f"e{k}")
            if dt in ("float32", "float64", "int32", "int64", "uint32", "uint64"):
                early.append(f"e{k}")
    # (the machine scheduler otherwise sinks every load next to its use: 48 VGPRs, one load in
    #  flight per MFMA group, and the epilogue operands requested after the barrier)
    SB = "  __builtin_amdgcn_sched_barrier(0);"
    L.append("  long long arow = r0 + li; if (arow >= M) arow = M - 1;")
    if "noload" in var:
        L.append(f"  const {ct} fake_ = ({ct})M;")
    for p in dot_pos:
        L.append(f"  dvec4 acc{p} = {{0, 0, 0, 0}};")
        for a in range(1, nacc):
            L.append(f"  dvec4 acc{p}_{a} = {{0, 0, 0, 0}};")
        if "apacked" in var or p in packed_a:
            L.append(f"  const dvec4* ap{p} = (const dvec4*)A{p} + (((long long)blockIdx.y * {K // 4} + (long long)wave * {GW * 4} + kq) * 16 + li);")
        else:
            L.append(f"  const dvec4* ap{p} = (const dvec4*)(A{p} + arow * lda{p}) + ((long long)wave * {GW * 4} + kq);")
        L.append(f"  const dvec4* bp{p} = (const dvec4*)Bp{p} + ((ctile * {K // 4} + (long long)wave * {GW * 4} + kq) * 16 + li);")
    # the stream of (dot group, chunk) register buffers, double-buffered; a group = a leader and
    # the dots that share its left operand (at most one follower: register budget)
    share = dict(share or {})
    groups = []
    for p in dot_pos:
        if p in share:
            continue
        fol = [f for f in dot_pos if share.get(f) == p][:1]
        for f in [f for f in dot_pos if share.get(f) == p][1:]:
            share.pop(f)  # further followers stream their own copy of A
        groups.append([p] + fol)
    groups += [[p] for p in dot_pos if p not in {q for g in groups for q in g}]
    chunks = []
    for gr in groups:
        for c0 in range(0, GW, chunk):
            chunks.append((gr, c0, min(chunk, GW - c0)))
    L.append(f"  dvec4 ra_[2][{chunk}], rb_[2][{chunk}];")
    if any(len(gr) > 1 for gr in groups):
        L.append(f"  dvec4 rc_[2][{chunk}];")
    bufs = ["rb_", "rc_"]

    def loads(s):
        gr, c0, n = chunks[s]
        out = []
        for u in range(n):
            g = c0 + u
            if "ntb" in var:  # (timing experiment: non-temporal weight loads)
                bl = " ".join(f"{bufs[q]}[{s & 1}][{u}] = __builtin_nontemporal_load(bp{p} + {g * 64});" for q, p in enumerate(gr))
            else:
                bl = " ".join(f"{bufs[q]}[{s & 1}][{u}] = bp{p}[{g * 64}];" for q, p in enumerate(gr))
            if lds_a:
                la = bl
                if u % 2 == 0:
                    # the 128-byte lines of k-groups g, g+1 of this wave's slice: rows 0-7, then 8-15
                    for hr in (0, 1):
                        la += (f" __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ag{gr[0]}_{hr} + {g * 16}), "
                               f"(__attribute__((address_space(3))) void*)&lda_[wave][{s & 1}][{u // 2}][{hr * 256}], 16, 0, 0);")
            else:
                la = f"ra_[{s & 1}][{u}] = ap{gr[0]}[{g * (64 if ('apacked' in var or gr[0] in packed_a) else 4)}]; " + bl
                if "noload" in var:
                    la = (f"ra_[{s & 1}][{u}] = dvec4{{fake_, fake_, fake_, fake_}}; "
                          + " ".join(f"{bufs[q]}[{s & 1}][{u}] = dvec4{{fake_, fake_, fake_, fake_}};" for q in range(len(gr))))
            if guard:
                zero = f"ra_[{s & 1}][{u}] = dvec4{{0, 0, 0, 0}}; " + " ".join(f"{bufs[q]}[{s & 1}][{u}] = dvec4{{0, 0, 0, 0}};" for q in range(len(gr)))
                la = f"if (wave * {GW} + {g} < {G}) {{ {la} }} else {{ {zero} }}"
            out.append("  " + la)
        return out

    def frags(s):
        """LDS path: the DMAs of chunk s have landed (vmcnt(0)); read its MFMA fragments"""
        gr, c0, n = chunks[s]
        out = ['  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");']
        for u in range(n):
            out.append(f"  ra_[{s & 1}][{u}] = *(const dvec4*)&lda_[wave][{s & 1}][{u // 2}][li * 32 + ((({4 * (u % 2)} + kq) ^ (li & 7)) << 2)];")
        return out

    def mfmas(s):
        gr, c0, n = chunks[s]
        out = []
        for u in range(n):
            for j in range(4):
                for q, p in enumerate(gr):
                    a = u % (nacc if len(gr) == 1 else max(nacc // 2, 1))
                    acc = f"acc{p}_{a}" if a else f"acc{p}"
                    if "nomfma" in var:
                        out.append(f"  acc{p}[{j}] += ra_[{s & 1}][{u}][{j}] * {bufs[q]}[{s & 1}][{u}][{j}];")
                    else:
                        out.append(f"  {acc} = {_MFMA16[T]}(ra_[{s & 1}][{u}][{j}], {bufs[q]}[{s & 1}][{u}][{j}], {acc}, 0, 0, 0);")
        return out

    # issue order: operand chunks 0 and 1, then the epilogue operands (vmcnt retires in order:
    # requested first, a load from HBM would hold up the first MFMA group), then the MFMA stream
    if lds_a:
        # source addresses of the two DMAs per line pair: lane l -> row l/8 (+8), piece (l%8) ^ (row&7)
        L.append("  const int lr_ = lane >> 3, lc_ = lane & 7;")
        for p in sorted({gr[0] for gr, _, _ in chunks}):
            for hr in (0, 1):
                L.append(f"  long long arow{p}_{hr} = r0 + lr_ + {8 * hr}; if (arow{p}_{hr} >= M) arow{p}_{hr} = M - 1;")
                L.append(f"  const {ct}* ag{p}_{hr} = A{p} + arow{p}_{hr} * lda{p} + (long long)wave * {GW * 16} + ((lc_ ^ (lr_ & 7)) << 2);")
        assert not guard
        # (the DMA wait is a plain vmcnt(0): the epilogue operands are requested first so that it
        #  never waits for anything younger than the chunk it needs)
        L += ew_loads + [SB] + loads(0) + [SB]
        for s in range(len(chunks)):
            L += frags(s) + [SB]
            if s + 1 < len(chunks):
                L += loads(s + 1) + [SB]
            L += mfmas(s) + [SB]
    else:
        L += loads(0) + [SB]
        for s in range(len(chunks)):
            if s + 1 < len(chunks):
                L += loads(s + 1) + [SB]
            if s == 0:
                L += ew_loads + [SB]
            L += mfmas(s) + [SB]
    # pin the epilogue operands here: without a use in this block the whole scalar graph, loads
    # included, is sunk into `if (live)` behind the barrier
    for e in early:
        L.append(f'  asm volatile("" : "+v"({e}));')
    if nacc > 1:
        for p in dot_pos:
            # fixed order: ((a0 + a1) + (a2 + a3)); chains a product never used stay zero
            if nacc == 4:
                L.append(f"  acc{p} = (acc{p} + acc{p}_1) + (acc{p}_2 + acc{p}_3);")
            else:
                L.append(f"  acc{p} += acc{p}_1;")
    for d, p in enumerate(dot_pos):
        # accumulator register v of lane (li, kq): f32 16x16x4 -> row 4*kq + v; f64 -> row kq + 4*v
        row = "4 * kq + v" if T == "float32" else "kq + 4 * v"
        L.append(f"#pragma unroll\n  for (int v = 0; v < 4; v++) red_[{d}][wave][({row}) * 16 + li] = acc{p}[v];")
    L.append("  __syncthreads();")
    for d, p in enumerate(dot_pos):
        L.append(f"  const {ct} dot{p} = ((red_[{d}][0][tid] + red_[{d}][1][tid]) + red_[{d}][2][tid]) + red_[{d}][3][tid];")
    out_names = []
    for k, dt in enumerate(body["out_dtypes"]):
        L.append(f"  {CTYPE[dt]} o{k};")
        out_names.append(f"o{k}")
    L.append(emit_body(body, in_names, out_names, indent="  "))
    L.append("  if (live) {")
    for k in range(len(body["out_dtypes"])):
        L.append(f"    out{k}[er * ldo{k} + ec] = o{k};")
    L.append("  }")
    for k in pack_outs:
        # element (i = tid/16, column ec) of row tile blockIdx.y: k4 = ec/4, j = ec%4 (all 256 threads: rows
        # past M hold zeros, so that a consumer's MFMA never multiplies uninitialised memory)
        L.append(f"  pk{k}[((blockIdx.y * (N >> 2) + (ctile * 4 + ((tid & 15) >> 2))) * 16 + (tid >> 4)) * 4 + (tid & 3)] = live ? o{k} : ({CTYPE[body['out_dtypes'][k]]})0;")
    L.append("}")
    return "\n".join(L)
