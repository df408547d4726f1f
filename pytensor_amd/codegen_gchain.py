"""``gchain``: ``Gemv → Elemwise → Gemv`` over one matrix in one pass (dispatch/fused.py)."""

from __future__ import annotations

from pytensor_amd.codegen import BLOCK, REDUCE_OPS, _reduce_epilogue, _stream_load, nt_loads
from pytensor_amd.codegen_scalar import CTYPE, device_header, emit_body, prelude_for


def gemv_chain_source(name, body, e_modes, reduce_spec, w_out, C, RG, store_r, has_y1,
                      out_store=None, scatter_out=None, scatter_groups=2, pack=2, atype="float64", pipe=False, full=False) -> str:
    """One-pass ``r = b1*y1 + a1*A@x ; outs = body(.., r, ..) ; partial += A.T@w`` (fp64).

    Work decomposition (wave64): a wave owns groups of ``RG`` consecutive rows.  Lane l
    holds columns {2l, 2l+1} + 128c (c < C) of every row of the group in registers
    (16-byte coalesced loads: one wave instruction = one 1 KiB row chunk), so the
    matrix is read from HBM exactly once and used twice:

    1. per-row partial dot products (2C FMAs per row per lane);
    2. a *transposing* butterfly: log2(RG) exchange steps in which every lane gives away
       half of its rows (RG-1 exchanges instead of 6 per row), then 6-log2(RG) plain
       steps — lanes (row << s .. ) end up owning one finished row each;
    3. the scalar graph runs once per row on the owning lanes (other row inputs are
       coalesced loads or table gathers), reductions accumulate per lane, vector outputs
       are stored only if something outside the fused node reads them;
    4. w[row] is broadcast back with ``v_readlane`` (compile-time lane) and multiplied
       into the still-resident row registers: acc[c] += row * w;
    5. optionally the scatter-add ``out[sidx[row]] += o[row]`` (gradient of a gather) is
       accumulated in the same pass: lane b owns bins b, b+64, ... (``scatter_groups`` x 64 <= 256 bins), rows are
       visited in order, per-workgroup partials are combined in a fixed order afterwards
       (deterministic, like every other reduction here).

    ``pack`` = 2: lane l holds columns {2l, 2l+1} of every 128-column chunk (one 16-byte load; rows must start on
    16-byte boundaries: even ``lda``, even K).  ``pack`` = 1: columns {l, l+64} (two 8-byte loads, each a coalesced
    512-byte row piece): any K, any ``lda`` — the odd-K instance.  ``C`` > 8 chunks (K > 1024): the multiplier vector
    ``x`` lives in LDS instead of registers, and fewer rows ride per group (``RG`` = 2: K <= 2048, 1: K <= 4096) so that
    the row registers (``RG*C`` <= 32 packs) and the ``A.T@w`` accumulators (``C`` packs) still fit.

    ``atype`` = "float32": the matrix, ``x``, ``y1`` and the stored Gemv result are float arrays — converted on load
    (an 8-byte ``float2`` per lane and chunk with ``pack`` = 2), everything between the loads and the stores stays the
    double-precision kernel (dot products, butterfly, ``A.T@w`` accumulators, partial slabs); the scalar graph gets the
    Gemv result rounded to float, as the reference's float32 ``Gemv`` output would be.

    ``pipe``: the software-pipelined row loop (csrc/gchain_device.h; ``RG`` >= 4, at most one gather input; the
    dispatcher selects it only where it measured faster, dispatch/fused._pipelined).  A group
    is worked on in two halves of ``RG/2`` rows with a register buffer each: the loads of the next half — which may be
    the first half of the wave's next group — and that half's per-row operands (``y1``, vector inputs, the gather and
    scatter indices) are issued before the current half is reduced, so the wait in front of a half's first dot product
    is a partial ``vmcnt``.  Each half runs its own butterfly (the transposing steps at distance 32 and 16 are the
    gfx950 half-swaps, no LDS crossbar) and its own pass of the scalar graph; a row's add tree, the order of the rows
    in ``accT`` and the bins, and — after ``to_group_lanes`` — the lanes that hold the reduction accumulators are
    those of the plain loop, so both forms give the same bits.  ``full`` (K = 128 ``C``): every lane is inside every
    row, and the loads carry no column predicate.  The gather table is copied into dynamic LDS
    (``glen`` entries) in the block prologue and read from there: a table read from memory would queue behind the
    prefetch.  The wave index is made uniform, which moves row numbers, clamps and row addresses to scalar registers.

    ``e_modes[k]`` ∈ {'R' the Gemv result, 'V' N-vector, 'S' scalar, 'G' gather
    ``table[gidx[row]]``} per elementwise input.
    Kernel params (all 8 bytes): N, K, A, lda, x, y1, alpha1, beta1, <per elementwise input
    except R: ptr (and for 'G': index ptr, table length)>, [r_out], <per output: stored ptr
    (if stored) | partial ptr (if reduced)>, partT, [sidx, sbins, partS], status.
    """
    import math

    nout = len(body["out_dtypes"])
    out_store = list(out_store) if out_store is not None else [True] * nout
    lg = int(math.log2(RG))
    assert 1 << lg == RG and 1 <= RG <= 32 and RG * C <= 32 and pack in (1, 2, 4)
    assert pack != 4 or (atype == "float32" and C % 2 == 0)
    b_lds = C > 8
    if pack == 4:
        # float32 only: a lane's 16-byte load is FOUR columns {4l .. 4l+3} of a 256-column chunk PAIR; the two halves are
        # chunks c (even) and c + 1 of the double-precision register image.  (8-byte loads — float2 per lane — fetch the
        # same bytes per instruction and run 2.6x slower: the waves sit at s_waitcnt 6x as long, profiles/r6a_gchain_f32_pmc.md)
        col0 = "(c >> 1) * 256 + 4 * lane + 2 * (c & 1)"
        col1 = col0 + " + 1"
    else:
        col0 = "c * 128 + 2 * lane" if pack == 2 else "c * 128 + lane"  # first column of lane's pack in chunk c
        col1 = "c * 128 + 2 * lane + 1" if pack == 2 else "c * 128 + 64 + lane"

    at = CTYPE[atype]

    def ld_pack(base, stream=True):  # the lane's two columns of chunk c from `base` (a pointer to `atype`)
        if pack == 2 and atype == "float64":
            ld = _stream_load(f"(const pt_d2*)({base} + {col0})") if stream else f"*(const pt_d2*)({base} + {col0})"
            return f"(({col0}) < K) ? {ld} : (pt_d2){{0.0, 0.0}}"
        if pack == 2:
            ld = _stream_load(f"(const pt_f2*)({base} + {col0})") if stream else f"*(const pt_f2*)({base} + {col0})"
            return f"(({col0}) < K) ? pt_widen({ld}) : (pt_d2){{0.0, 0.0}}"
        if pack == 4 and not stream:  # (the short multiplier vector: element loads)
            return f"(pt_d2){{(({col0}) < K) ? (double){base}[{col0}] : 0.0, (({col1}) < K) ? (double){base}[{col1}] : 0.0}}"
        assert pack != 4, "the matrix rows of the four-column form are loaded pairwise (below)"
        return f"(pt_d2){{(({col0}) < K) ? (double){base}[{col0}] : 0.0, (({col1}) < K) ? (double){base}[{col1}] : 0.0}}"

    rest = 6 - lg  # plain butterfly steps after the transposing ones
    params = [
        "long long N", "long long K", f"const {CTYPE[atype]}* __restrict__ A", "long long lda",
        f"const {CTYPE[atype]}* __restrict__ x", f"const {CTYPE[atype]}* __restrict__ y1", "double alpha1", "double beta1",
    ]
    for k, m in enumerate(e_modes):
        if m == "R":
            continue
        params.append(f"const {CTYPE[body['in_dtypes'][k]]}* __restrict__ in{k}")
        if m == "G":
            params += [f"const long long* __restrict__ gidx{k}", f"long long glen{k}"]
    if store_r:
        params.append(f"{CTYPE[atype]}* __restrict__ r_out")
    for k, dt in enumerate(body["out_dtypes"]):
        if reduce_spec[k] is not None:
            params.append(f"{CTYPE[reduce_spec[k][1]]}* __restrict__ part{k}")
        elif out_store[k]:
            params.append(f"{CTYPE[dt]}* __restrict__ out{k}")
    params.append("double* __restrict__ partT")
    if scatter_out is not None:
        params += ["const long long* __restrict__ sidx", "long long sbins", "double* __restrict__ partS"]
    params.append("int* __restrict__ status")
    if pipe:
        # what the generator can emit (two halves of >= 2 rows, multipliers in registers, one table in LDS); which
        # instances RUN pipelined is the dispatcher's choice, by measurement (dispatch/fused._pipelined)
        assert RG >= 4 and not b_lds and sum(m == "G" for m in e_modes) <= 1
    L = [device_header("reduce_device.h"), prelude_for(body)]
    if pipe:
        if not nt_loads():
            L.append("#define GCHAIN_PLAIN_LOADS 1")
        L.append(device_header("gchain_device.h"))
    L.append("typedef double pt_d2 __attribute__((ext_vector_type(2)));")
    L.append("typedef float pt_f2 __attribute__((ext_vector_type(2)));")
    L.append("typedef float pt_f4 __attribute__((ext_vector_type(4)));")
    L.append("static __device__ __forceinline__ pt_d2 pt_widen(pt_f2 v) { return (pt_d2){(double)v.x, (double)v.y}; }")
    L.append("static __device__ __forceinline__ double pt_shfl_xor(double v, int m) { return pthip_dev::shfl_xor_any(v, m); }")
    L.append("static __device__ __forceinline__ double pt_readlane(double v, int l) {")
    L.append("  union { double d; int i[2]; } u; u.d = v;")
    L.append("  u.i[0] = __builtin_amdgcn_readlane(u.i[0], l); u.i[1] = __builtin_amdgcn_readlane(u.i[1], l); return u.d; }")
    L.append(f'extern "C" __global__ __launch_bounds__({BLOCK}) void {name}({", ".join(params)}) {{')
    L.append(f"  constexpr int C = {C}, RG = {RG};")
    if pipe:
        L.append("  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);")
    else:
        L.append("  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;")
    L.append("  pt_d2 accT[C];")
    red_w = f"(128 * C > {64 * int(scatter_groups)} ? 128 * C : {64 * int(scatter_groups)})" if scatter_out is not None else "128 * C"
    L.append(f"  __shared__ double redT[{BLOCK // 64}][{red_w}];")
    if b_lds:
        # the multiplier vector: read per use (registers hold the rows and the accumulators); it lives in the memory the
        # block combine uses after the row loop
        L.append("  pt_d2 (*b)[64] = reinterpret_cast<pt_d2 (*)[64]>(&redT[0][0]);")
        L.append(f"  for (int j = threadIdx.x; j < C * 64; j += {BLOCK}) {{ const int c = j >> 6, lane = j & 63; b[c][lane] = " + ld_pack("x", stream=False) + "; }")
        L.append("  __syncthreads();")
        L.append("#pragma unroll\n  for (int c = 0; c < C; c++) accT[c] = (pt_d2){0.0, 0.0};")
        bref = "b[c][lane]"
    else:
        L.append("  pt_d2 b[C];")
        L.append("#pragma unroll\n  for (int c = 0; c < C; c++) {")
        L.append("    b[c] = " + ld_pack("x", stream=False) + ";")
        L.append("    accT[c] = (pt_d2){0.0, 0.0};\n  }")
        bref = "b[c]"
    if scatter_out is not None:
        SG = int(scatter_groups)
        assert 1 <= SG <= 4
        L.append("  double " + ", ".join(f"accS{q} = 0.0" for q in range(SG)) + ";  // bins lane, lane + 64, ...")
    for k, m in enumerate(e_modes):
        if m == "S":
            L.append(f"  const {CTYPE[body['in_dtypes'][k]]} s{k} = in{k}[0];")
    for k, rs in enumerate(reduce_spec):
        if rs is not None:
            act = CTYPE[rs[1]]
            L.append(f"  {act} acc{k}_0 = pthip_dev::{REDUCE_OPS[rs[0]]}::identity<{act}>();")
    def finish_rows(ind, first, dot, sfx, y1_of, vec_of, gidx_of, table_of, sidx_of, rowc):
        """What follows the butterfly, for the rows starting at ``first`` whose dot products sit in ``dot`` on the owning
        lanes: the Gemv result, the scalar graph, the reductions (accumulators ``acc<k><sfx>``) and stores, ``w`` and the
        scatter bin ``si``.  The per-row operands are named by the caller: read in place (plain loop, ``rowc``: the
        clamped row is declared) or carried from the request one stage ahead (pipelined loop).  ONE emitter for both
        loops: their bit equality rests on this text being the same."""
        o = [f"{ind}const long long row = {first} + myrow;", f"{ind}const bool valid = row < N;"]
        if rowc:
            o.append(f"{ind}const long long rowc = valid ? row : N - 1;")
        o.append(f"{ind}double res = alpha1 * {dot};")
        if has_y1:
            o.append(f"{ind}if (beta1 != 0.0) res += beta1 * {y1_of};")
        if store_r:
            o.append(f"{ind}if (valid && owner) r_out[row] = res;")
        in_names = []
        for k, m in enumerate(e_modes):
            if m == "R":
                in_names.append("res" if body["in_dtypes"][k] == "float64" else f"(({CTYPE[body['in_dtypes'][k]]})res)")
            elif m == "S":
                in_names.append(f"s{k}")
            elif m == "G":
                o.append(f"{ind}long long gi{k} = {gidx_of(k)};")
                o.append(f"{ind}if (gi{k} < 0) gi{k} += glen{k};")
                o.append(f"{ind}if (gi{k} < 0 || gi{k} >= glen{k}) {{ atomicOr(status, 1); gi{k} = 0; }}  // IndexError, reported by the host")
                in_names.append(table_of(k))
            else:
                in_names.append(vec_of(k))
        out_names = []
        for k, dt in enumerate(body["out_dtypes"]):
            o.append(f"{ind}{CTYPE[dt]} o{k};")
            out_names.append(f"o{k}")
        o.append(emit_body(body, in_names, out_names, indent=ind))
        for k, rs in enumerate(reduce_spec):
            if rs is not None:
                o.append(f"{ind}if (valid && owner) acc{k}{sfx} = pthip_dev::{REDUCE_OPS[rs[0]]}::apply(acc{k}{sfx}, ({CTYPE[rs[1]]})o{k});")
            elif out_store[k]:
                o.append(f"{ind}if (valid && owner) out{k}[row] = o{k};")
        o.append(f"{ind}const double w = valid ? (double)o{w_out} : 0.0;")
        if scatter_out is not None:
            if scatter_out != w_out:
                o.append(f"{ind}const double sv = valid ? (double)o{scatter_out} : 0.0;")
            o.append(f"{ind}long long si_ = {sidx_of};")
            o.append(f"{ind}if (si_ < 0) si_ += sbins;")
            o.append(f"{ind}if (valid && (si_ < 0 || si_ >= sbins)) {{ atomicOr(status, 1); }}")
            o.append(f"{ind}const int si = (valid && si_ >= 0 && si_ < sbins) ? (int)si_ : -1;")
        return o

    def accumulate_rows(ind, nrows, shift, readlane, axpy):
        """``accT += row * w[row]`` and the bins, rows in order: ``w`` and ``si`` of row r come from lane ``r << shift``."""
        o = [f"#pragma unroll\n{ind}for (int r = 0; r < {nrows}; r++) {{",
             f"{ind}  const double wr = {readlane}(w, r << {shift});",
             axpy]
        if scatter_out is not None:
            sval = "wr" if scatter_out == w_out else f"{readlane}(sv, r << {shift})"
            o.append(f"{ind}  const int ir = __builtin_amdgcn_readlane(si, r << {shift});")
            o.append(f"{ind}  const double svr = {sval};")
            for q in range(SG):
                o.append(f"{ind}  accS{q} += (ir == lane + {64 * q}) ? svr : 0.0;")
        o.append(f"{ind}}}")
        return o

    if pipe:
        L += _pipelined_loop(body, e_modes, reduce_spec, has_y1, scatter_out, RG, at, pack, full, finish_rows, accumulate_rows)
    else:
        L.append(f"  const int myrow = (lane >> {rest}) & (RG - 1);   // row of the group this lane finishes")
        L.append(f"  const bool owner = (lane & {(1 << rest) - 1}) == 0;")
        L.append("  const long long ngroups = (N + RG - 1) / RG;")
        L.append(f"  for (long long g = (long long)blockIdx.x * {BLOCK // 64} + wid; g < ngroups; g += (long long)gridDim.x * {BLOCK // 64}) {{")
        L.append("    const long long row0 = g * RG;")
        L.append("    pt_d2 xr[RG][C];")
        L.append("#pragma unroll\n    for (int r = 0; r < RG; r++) {")
        L.append("      const long long row = (row0 + r < N) ? row0 + r : N - 1;")
        L.append(f"      const {at}* __restrict__ Ar = A + row * lda;")
        if pack == 4:
            L.append("#pragma unroll\n      for (int c = 0; c < C; c += 2) {")
            L.append("        const long long cq = (c >> 1) * 256 + 4 * lane;")
            L.append("        pt_f4 t4 = {0.f, 0.f, 0.f, 0.f};")
            L.append("        if (cq < K) t4 = " + _stream_load("(const pt_f4*)(Ar + cq)") + ";  // (K % 4 == 0: a pack is inside the row or outside)")
            L.append("        xr[r][c] = (pt_d2){(double)t4.x, (double)t4.y};")
            L.append("        xr[r][c + 1] = (pt_d2){(double)t4.z, (double)t4.w};\n      }\n    }")
        else:
            L.append("#pragma unroll\n      for (int c = 0; c < C; c++) {")
            L.append("        xr[r][c] = " + ld_pack("Ar") + ";\n      }\n    }")
        L.append("    double p[RG];")
        L.append("#pragma unroll\n    for (int r = 0; r < RG; r++) {")
        L.append("      double s = 0.0;")
        L.append(f"#pragma unroll\n      for (int c = 0; c < C; c++) {{ const pt_d2 bc = {bref}; s += xr[r][c].x * bc.x + xr[r][c].y * bc.y; }}")
        L.append("      p[r] = s;\n    }")
        half = RG // 2
        mask = 32
        while half >= 1:
            L.append(f"    {{ const bool up = (lane & {mask}) != 0;")
            L.append(f"#pragma unroll\n      for (int i = 0; i < {half}; i++) {{")
            L.append(f"        const double send = up ? p[i] : p[i + {half}];")
            L.append(f"        const double keep = up ? p[i + {half}] : p[i];")
            L.append(f"        p[i] = keep + pt_shfl_xor(send, {mask});\n      }} }}")
            half //= 2
            mask //= 2
        while mask >= 1:
            L.append(f"    p[0] += pt_shfl_xor(p[0], {mask});")
            mask //= 2
        L += finish_rows("    ", "row0", "p[0]", "_0", "y1[rowc]", lambda k: f"in{k}[rowc]", lambda k: f"gidx{k}[rowc]",
                         lambda k: f"in{k}[gi{k}]", "sidx[rowc]", rowc=True)
        L += accumulate_rows("    ", "RG", rest, "pt_readlane",
                             "#pragma unroll\n      for (int c = 0; c < C; c++) { accT[c].x += xr[r][c].x * wr; accT[c].y += xr[r][c].y * wr; }")
        L.append("  }")
    # block combine of accT (fixed wave order), of the scatter bins and of the reductions
    if b_lds:
        L.append("  __syncthreads();  // every wave is done reading the multiplier vector out of this memory")
    L.append(f"#pragma unroll\n  for (int c = 0; c < C; c++) {{ redT[wid][{col0}] = accT[c].x; redT[wid][{col1}] = accT[c].y; }}")
    L.append("  __syncthreads();")
    L.append(f"  for (int j = threadIdx.x; j < 128 * C; j += {BLOCK}) {{")
    L.append("    double v = redT[0][j];")
    L.append(f"#pragma unroll\n    for (int q = 1; q < {BLOCK // 64}; q++) v += redT[q][j];")
    L.append("    if (j < K) partT[(long long)blockIdx.x * K + j] = v;\n  }")
    if scatter_out is not None:
        L.append("  __syncthreads();")
        L.append("  " + " ".join(f"redT[wid][lane + {64 * q}] = accS{q};" for q in range(SG)))
        L.append("  __syncthreads();")
        L.append(f"  if (threadIdx.x < {64 * SG}) {{")
        L.append("    double v = redT[0][threadIdx.x];")
        L.append(f"#pragma unroll\n    for (int q = 1; q < {BLOCK // 64}; q++) v += redT[q][threadIdx.x];")
        L.append("    if (threadIdx.x < sbins) partS[(long long)blockIdx.x * sbins + threadIdx.x] = v;\n  }")
    L.append(_reduce_epilogue(reduce_spec, 1))
    L.append("}")
    return "\n".join(L)


def _pipelined_loop(body, e_modes, reduce_spec, has_y1, scatter_out, RG, at, pack, full, finish_rows, accumulate_rows):
    """The row loop over two half-group buffers (csrc/gchain_device.h), see ``pipe`` above.  The text of one stage —
    request a half's loads, reduce a half — is emitted once per buffer, so the buffers are static registers; what is
    done with a finished row is the plain loop's own text (``finish_rows`` / ``accumulate_rows`` of the caller)."""
    RH = RG // 2
    resth = 6 - (RH.bit_length() - 1)  # plain butterfly steps of a half
    L = []
    gk = [k for k, m in enumerate(e_modes) if m == "G"]
    if gk:
        k = gk[0]
        tt = CTYPE[body["in_dtypes"][k]]
        L.append("  extern __shared__ __attribute__((aligned(16))) unsigned char pt_dyn_lds[];")
        L.append(f"  {tt}* gtab = reinterpret_cast<{tt}*>(pt_dyn_lds);  // the gather table, glen{k} entries (the launch sizes it)")
        L.append(f"  for (long long j = threadIdx.x; j < glen{k}; j += {BLOCK}) gtab[j] = in{k}[j];")
        L.append("  __syncthreads();")
    for k, rs in enumerate(reduce_spec):
        if rs is not None:
            L.append(f"  {CTYPE[rs[1]]} acc{k}_h0 = acc{k}_0, acc{k}_h1 = acc{k}_0;  // per half: other lanes finish the rows (to_group_lanes)")
    L.append(f"  typedef gchain::Rows<{RH}, C, {pack}, {at}, {'true' if full else 'false'}> rows_t;")
    L.append(f"  const int myrow = (lane >> {resth}) & {RH - 1};   // row of a half this lane finishes")
    L.append(f"  const bool owner = (lane & {(1 << resth) - 1}) == 0;")
    L.append("  const long long ngroups = (N + RG - 1) / RG;")
    L.append(f"  const long long gstep = (long long)gridDim.x * {BLOCK // 64};")
    L.append(f"  long long g = (long long)blockIdx.x * {BLOCK // 64} + wid;")
    # what a half carries from its request to its use: the rows and the owning lane's per-row operands
    for s in "01":
        L.append(f"  rows_t X{s};")
        if has_y1:
            L.append(f"  {at} y1_{s} = 0;")
        for k, m in enumerate(e_modes):
            if m == "V":
                L.append(f"  {CTYPE[body['in_dtypes'][k]]} v{k}_{s} = 0;")
            elif m == "G":
                L.append(f"  long long gi{k}_{s} = 0;")
        if scatter_out is not None:
            L.append(f"  long long si_{s} = 0;")

    def request(s, first, ind):
        o = [f"{ind}X{s}.load(A, lda, {first}, N, K, lane);",
             f"{ind}{{ const long long rq = {first} + myrow; const long long rc = rq < N ? rq : N - 1;"]
        if has_y1:
            o.append(f"{ind}  if (beta1 != 0.0) y1_{s} = y1[rc];")
        for k, m in enumerate(e_modes):
            if m == "V":
                o.append(f"{ind}  v{k}_{s} = in{k}[rc];")
            elif m == "G":
                o.append(f"{ind}  gi{k}_{s} = gidx{k}[rc];")
        if scatter_out is not None:
            o.append(f"{ind}  si_{s} = sidx[rc];")
        o.append(f"{ind}}}")
        # (the scheduler would otherwise sink these loads below the arithmetic of the other half, to save registers)
        o.append(f"{ind}__builtin_amdgcn_sched_barrier(0);")
        return o

    def reduce_half(s, first, ind):
        o = [f"{ind}{{",
             f"{ind}  double p[{RH}];",
             f"{ind}  X{s}.dots(b, p);",
             f"{ind}  const double dot = gchain::butterfly<{RH}>(p, lane);"]
        o += finish_rows(ind + "  ", first, "dot", f"_h{s}", f"y1_{s}", lambda k: f"v{k}_{s}", lambda k: f"gi{k}_{s}",
                         lambda k: f"gtab[gi{k}]", f"si_{s}", rowc=False)
        o += accumulate_rows(ind + "  ", RH, resth, "gchain::readlane", f"{ind}    X{s}.axpy(r, wr, accT);")
        o.append(f"{ind}}}")
        return o

    L.append("  if (g < ngroups) {  // (a wave with no group issues nothing)")
    L += request("0", "g * RG", "    ")
    L.append("    for (;;) {")
    L.append("      const long long row0 = g * RG, gn = g + gstep;")
    L += request("1", f"row0 + {RH}", "      ")
    L += reduce_half("0", "row0", "      ")
    L.append("      if (gn >= ngroups) break;")
    L += request("0", "gn * RG", "      ")
    L += reduce_half("1", f"row0 + {RH}", "      ")
    L.append("      g = gn;")
    L.append("    }")
    L += reduce_half("1", f"g * RG + {RH}", "    ")  # (the last group's second half: nothing left to ask for)
    L.append("  }")
    for k, rs in enumerate(reduce_spec):
        if rs is not None:
            act = CTYPE[rs[1]]
            L.append(f"  acc{k}_0 = gchain::to_group_lanes<RG, {act}>(acc{k}_h0, acc{k}_h1, pthip_dev::{REDUCE_OPS[rs[0]]}::identity<{act}>(), lane);")
    return L
