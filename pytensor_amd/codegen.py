"""Fused ``Elemwise``/``Composite`` → HIP kernel source for gfx950.

The reference emits the fused body with ``Composite.c_code_template``
(pytensor/scalar/basic.py:4111-4170) by concatenating each scalar op's ``c_code``
statement, and wraps it in the loop nest of ``Elemwise._c_all``
(pytensor/tensor/elemwise.py:848-1167; contiguous fast path 1083-1166).  Here the
same SSA walk emits a device expression per scalar op (``codegen_scalar.emit_body``)
and this module wraps it in one of three loop shapes designed for CDNA4 rather than
for a CPU:

``flat``    every operand is either fully contiguous (same shape) or a scalar
            broadcast → grid-stride loop, 16-byte vector loads/stores per lane
            (coalesced 1 KiB per wave instruction), ``UNROLL`` independent packs
            in flight per thread;
``nd``      general broadcasting / arbitrary strides → collapsed N-d index with
            per-operand element strides (0 for broadcast dims);
``reduce``  ``flat`` or ``nd`` loads fused with a full reduction of selected
            outputs: per-thread accumulators (acc dtype) → wave64 butterfly →
            LDS → one partial per workgroup; reduced outputs never touch HBM.

Kernel parameters are all 8 bytes wide (pointers, ``long long``) so the host
packs the argument buffer with plain ``struct.pack("<q...")``.

The other generated families live beside this module and import from it:
``codegen_tile`` (tiled N-d), ``codegen_gchain``, ``codegen_dotew``, ``codegen_tail``.
"""

from __future__ import annotations

import hashlib
import os

import numpy as np

from pytensor_amd.codegen_scalar import _EMIT_CTX, CTYPE, device_header, emit_body, prelude_for

BLOCK = 256
REDUCE_OPS = {"Add": "OpAdd", "Mul": "OpMul", "Maximum": "OpMax", "Minimum": "OpMin"}


def _vec_width(dtypes) -> int:
    """elements per 16-byte pack, limited by the widest participating dtype"""
    w = max(np.dtype(d).itemsize for d in dtypes)
    return max(1, 16 // w)


def _vec_type(ctype: str, n: int) -> str:
    return f"pt_vec<{ctype}, {n}>"


VEC_HELPERS = r"""
template <class T, int N> struct __attribute__((aligned(sizeof(T) * N))) pt_vec { T v[N]; };
template <class P> static __device__ __forceinline__ P pthip_nt_pack(const P* p) {
  typedef unsigned int pt_u4 __attribute__((ext_vector_type(4)));
  P o;
  if constexpr (sizeof(P) == 16) { const pt_u4 r = __builtin_nontemporal_load((const pt_u4*)p); __builtin_memcpy(&o, &r, 16); }
  else if constexpr (sizeof(P) == 8) { const unsigned long long r = __builtin_nontemporal_load((const unsigned long long*)p); __builtin_memcpy(&o, &r, 8); }
  else if constexpr (sizeof(P) == 4) { const unsigned int r = __builtin_nontemporal_load((const unsigned int*)p); __builtin_memcpy(&o, &r, 4); }
  else o = *p;
  return o;
}
"""


def nt_loads() -> bool:
    """Whether streamed-once operands are read with non-temporal loads (``PTHIP_NT_LOADS=0``: plain loads)."""
    return os.environ.get("PTHIP_NT_LOADS", "1") != "0"


def _stream_load(ptr_expr: str, struct=False) -> str:
    """Load of an operand that is streamed once (the vector inputs of a flat fused kernel, the
    matrix of ``gchain``): non-temporal (``nt``) — the line is not retained in L2/MALL, which is
    what a pass over 0.16-1 GB wants (MI355X_MICROARCH.md price list, nt-weights row).  Measured
    (profiles/r2f_nt_loads.txt): ``gchain`` 184.5 -> 171.2 us (5.64 -> 6.08 TB/s), config #4
    4072 -> 4366 evals/s; 52-op Composite+Sum at N=1e7 39.9 -> 38.1 us.  ``PTHIP_NT_LOADS=0``
    restores plain loads."""
    if nt_loads():
        if struct:  # the pack types are structs: reinterpret as one 16/8/4-byte word
            return f"pthip_nt_pack({ptr_expr})"
        return f"__builtin_nontemporal_load({ptr_expr})"
    return f"*({ptr_expr})"


def _flat_params(body: dict, modes: str, reduce_spec, vec: int, finish=None):
    params = ["long long n"]
    for k, dt in enumerate(body["in_dtypes"]):
        if modes[k] == "C":  # host-known scalar: travels by value in the argument block
            params.append(f"const long long in{k}")
        elif modes[k] == "G":  # in{k}[gx{k}[i]]: a gather (AdvancedSubtensor on axis 0) read in the loop
            params += [f"const {CTYPE[dt]}* __restrict__ in{k}", f"const long long* __restrict__ gx{k}", f"long long gn{k}"]
        else:
            params.append(f"const {CTYPE[dt]}* __restrict__ in{k}")
    for k, dt in enumerate(body["out_dtypes"]):
        if reduce_spec[k] is None:
            params.append(f"{CTYPE[dt]}* __restrict__ out{k}")
        else:
            params.append(f"{CTYPE[reduce_spec[k][1]]}* __restrict__ part{k}")
    if "G" in modes:
        assert vec == 1, "gather inputs use the scalar loop"
        params.append("int* __restrict__ status")
    if finish:
        for k, dt in enumerate(finish):
            if dt is not None:
                params.append(f"{CTYPE[dt]}* __restrict__ fin{k}")
        params += ["int* __restrict__ ticket", "int* __restrict__ pt_status"]
    return params


def flat_kernel_source(name: str, body: dict, modes: str, vec: int, reduce_spec=None, unroll=2, device_fn=False, prefetch=False, finish=None, finish_per_thread=None) -> str:
    """:func:`_flat_kernel_source` with the emit context set: when EVERY output of the body is summed (a logp term and its
    gradients in a many-term launch, a fused Elemwise + Sum) no element is ever seen — only sums over ~1e6 of them, held to
    rtol 1e-12 — so divisions that share a float64 denominator may share ONE reciprocal (x * (1/d) is within 1.5 ulp of
    x / d; an fp64 division is ~28 VALU instructions).  Never when an element-wise output is stored: 6 * (1/3) != 2."""
    all_summed = bool(reduce_spec) and all(rs is not None and rs[0] == "Add" and rs[1] == "float64" for rs in reduce_spec)
    old = _EMIT_CTX["share_recip"]
    _EMIT_CTX["share_recip"] = bool(all_summed and os.environ.get("PTHIP_SHARE_RECIP", "1") != "0")
    try:
        return _flat_kernel_source(name, body, modes, vec, reduce_spec, unroll, device_fn, prefetch, finish, finish_per_thread)
    finally:
        _EMIT_CTX["share_recip"] = old


def _flat_kernel_source(name: str, body: dict, modes: str, vec: int, reduce_spec=None, unroll=2, device_fn=False, prefetch=False, finish=None, finish_per_thread=None) -> str:
    """``flat`` loop.  ``modes[k]`` ∈ {'V' contiguous vector, 'S' scalar broadcast} per input.

    reduce_spec: None or list (per output) of None | (op_name, acc_dtype): reduced
    outputs are accumulated instead of stored; the kernel then takes one partial
    pointer per reduced output (laid out [gridDim.x]).

    ``device_fn``: emit the loop as a ``__device__`` function taking the workgroup index and count as
    two trailing arguments, without the headers (``multi_flat_source`` dispatches several of them
    from one launch).

    ``prefetch``: software-pipelined main loop — the packs of iteration i+1 are requested before the
    scalar graph of iteration i runs, so a wave keeps ``unroll`` x 16 B per operand in flight WHILE
    it computes.  For a long fp64 body (BASELINE config #2: ~270 VALU instructions per 4 elements,
    17 us of issue next to 25 us of HBM time) the plain loop alternates between the two — every
    wave either waits or computes, and the bytes in flight per CU drop with the share of waves
    that are computing; pipelined, the two overlap.
    """
    nin = len(body["in_dtypes"])
    nout = len(body["out_dtypes"])
    reduce_spec = reduce_spec or [None] * nout
    params = _flat_params(body, modes, reduce_spec, vec, finish)
    if device_fn:
        # (inlined into every case of the dispatching switch: as ONE shared copy per family (__noinline__) the kernel of
        #  north_star's 48-term graph shrank from 40,000 to 5,500 instructions but needed 99 VGPRs instead of 50 for the
        #  call and ran 218 us instead of 196 — measured, profiles/r5m notes in DESIGN.md)
        src = [f"static __device__ __forceinline__ void {name}({', '.join(params)}, const unsigned pt_bidx, const unsigned pt_gdim) {{"]
    else:
        src = [device_header("reduce_device.h") if any(reduce_spec) else "", prelude_for(body), VEC_HELPERS, PT_PAIR_HELPERS if finish else ""]
        src.append(f'extern "C" __global__ __launch_bounds__({BLOCK}) void {name}({", ".join(params)}) {{')
    # scalars
    for k, m in enumerate(modes):
        if m == "S":
            src.append(f"  const {CTYPE[body['in_dtypes'][k]]} s{k} = in{k}[0];")
        elif m == "C":
            ct = CTYPE[body["in_dtypes"][k]]
            src.append(f"  {ct} s{k}; {{ const long long b = in{k}; __builtin_memcpy(&s{k}, &b, sizeof({ct})); }}")
    for k, rs in enumerate(reduce_spec):
        if rs is not None:
            act = CTYPE[rs[1]]
            for u in range(unroll):
                src.append(f"  {act} acc{k}_{u} = pthip_dev::{REDUCE_OPS[rs[0]]}::identity<{act}>();")
    src.append(f"  const long long tid = (long long)blockIdx.x * {BLOCK} + threadIdx.x;")
    src.append(f"  const long long nthreads = (long long)gridDim.x * {BLOCK};")
    V = vec
    if V > 1:
        src.append(f"  const long long npack = n / {V};")
        # main vector loop, `unroll` packs per iteration
        src.append(f"  long long p = tid;")
        vins = [(k, CTYPE[body["in_dtypes"][k]]) for k, m in enumerate(modes) if m == "V"]

        def _ld(k, ct, u, pv):
            return _stream_load(f'reinterpret_cast<const {_vec_type(ct, V)}*>(in{k}) + ({pv} + {u} * nthreads)', struct=True)

        if prefetch and vins:
            for u in range(unroll):
                for k, ct in vins:
                    src.append(f"  {_vec_type(ct, V)} n{k}_{u};")
            src.append(f"  bool pt_more = p + {unroll - 1} * nthreads < npack;")
            src.append("  if (pt_more) {")
            for u in range(unroll):
                for k, ct in vins:
                    src.append(f"    n{k}_{u} = {_ld(k, ct, u, 'p')};")
            src.append("  }")
            src.append("  while (pt_more) {")
            for u in range(unroll):
                for k, ct in vins:
                    src.append(f"    const {_vec_type(ct, V)} a{k}_{u} = n{k}_{u};")
            src.append(f"    const long long pn = p + {unroll} * nthreads;")
            src.append(f"    pt_more = pn + {unroll - 1} * nthreads < npack;")
            src.append("    if (pt_more) {")
            for u in range(unroll):
                for k, ct in vins:
                    src.append(f"      n{k}_{u} = {_ld(k, ct, u, 'pn')};")
            src.append("    }")
            # (the machine scheduler would otherwise sink the requests next to their first use)
            src.append("    __builtin_amdgcn_sched_barrier(0);")
        else:
            src.append(f"  for (; p + {unroll - 1} * nthreads < npack; p += {unroll} * nthreads) {{")
            for u in range(unroll):
                for k, ct in vins:
                    src.append(f"    const {_vec_type(ct, V)} a{k}_{u} = {_ld(k, ct, u, 'p')};")
        for u in range(unroll):
            for k, dt in enumerate(body["out_dtypes"]):
                if reduce_spec[k] is None:
                    src.append(f"    {_vec_type(CTYPE[dt], V)} r{k}_{u};")
            src.append(f"#pragma unroll\n    for (int e = 0; e < {V}; e++) {{")
            in_names = [(f"a{k}_{u}.v[e]" if m == "V" else f"s{k}") for k, m in enumerate(modes)]
            out_names = []
            for k, dt in enumerate(body["out_dtypes"]):
                if reduce_spec[k] is None:
                    out_names.append(f"r{k}_{u}.v[e]")
                else:
                    src.append(f"      {CTYPE[dt]} o{k};")
                    out_names.append(f"o{k}")
            src.append(emit_body(body, in_names, out_names))
            for k, rs in enumerate(reduce_spec):
                if rs is not None:
                    src.append(f"      acc{k}_{u} = pthip_dev::{REDUCE_OPS[rs[0]]}::apply(acc{k}_{u}, ({CTYPE[rs[1]]})o{k});")
            src.append("    }")
            for k, dt in enumerate(body["out_dtypes"]):
                if reduce_spec[k] is None:
                    src.append(f"    reinterpret_cast<{_vec_type(CTYPE[dt], V)}*>(out{k})[p + {u} * nthreads] = r{k}_{u};")
        if prefetch and vins:
            src.append("    p = pn;")
        src.append("  }")
        # remaining packs one at a time, then the scalar tail
        src.append(f"  for (; p < npack; p += nthreads) {{")
        src.append(_flat_scalar_block(body, modes, reduce_spec, V, "p"))
        src.append("  }")
        src.append(f"  for (long long i = npack * {V} + tid; i < n; i += nthreads) {{")
        src.append(_flat_elem(body, modes, reduce_spec, "i"))
        src.append("  }")
    else:
        src.append(f"  for (long long i = tid; i < n; i += nthreads) {{")
        src.append(_flat_elem(body, modes, reduce_spec, "i"))
        src.append("  }")
    src.append(_reduce_epilogue(reduce_spec, unroll, finish, finish_per_thread))
    src.append("}")
    text = "\n".join(src)
    if device_fn:
        text = text.replace("blockIdx.x", "pt_bidx").replace("gridDim.x", "pt_gdim")
    return text


def multi_finish_layout(nred: int, groups: int):
    """One term's block of a self-finishing many-term launch, in 8-byte words: ``nred`` pair arrays of ``2 * groups`` words,
    then the finished values; returns ``(offset of the finals, words in all — even, so the next term's pairs stay 16-byte
    aligned)``."""
    fin = 2 * groups * nred
    return fin, (fin + nred + 1) // 2 * 2


def multi_flat_source(name: str, terms, finish: bool = False) -> str:
    """Several independent flat kernels in ONE launch (widefuse.fuse_independent_reductions):
    ``(blockIdx.x + blockIdx.y) % gridDim.x`` selects the term, ``blockIdx.y`` / the term's ``groups`` are the
    workgroup index / count within it.  ``terms``: ``[{body, modes, vec, rs, unroll}]``; terms with the same (body, modes,
    vec, reductions) share one device function.  Arguments: the terms' flat-kernel arguments, one
    term after the other.

    ``finish``: every term finishes its own reductions (``_reduce_epilogue``'s one-pass form: the term's last workgroup
    folds its <= BLOCK pairs).  A term's pair arrays and finished values then live in ONE block (``multi_finish_layout``)
    passed as a single pointer, its ticket is ``tickets[term]`` and the status word is shared: the argument block shrinks
    instead of growing (4 KB limit: north_star's 48 terms)."""
    bodies = [t["body"] for t in terms]
    head = [device_header("reduce_device.h"), prelude_for(*bodies), VEC_HELPERS, PT_PAIR_HELPERS if finish else ""]
    fns, fn_of = {}, []
    for t in terms:
        key = source_key(repr((t["body"], t["modes"], t["vec"], t["rs"], t["unroll"], bool(t.get("prefetch")), finish)))
        if key not in fns:
            fname = f"mt_{key[:12]}"
            fin = [rs[1] for rs in t["rs"]] if finish else None  # (finished in the accumulator dtype: 8-byte words)
            fns[key] = (fname, flat_kernel_source(fname, t["body"], t["modes"], t["vec"], t["rs"], t["unroll"], device_fn=True, prefetch=bool(t.get("prefetch")),
                                                  finish=fin, finish_per_thread=1 if finish else None))
        fn_of.append(fns[key][0])
    P, calls = [], []
    for ti, t in enumerate(terms):
        ps = _flat_params(t["body"], t["modes"], t["rs"], t["vec"])
        names = []
        nred = len(t["rs"])
        for q, prm in enumerate(ps):
            decl, nm = prm.rsplit(" ", 1)
            if finish and nm.startswith("part"):
                if nm == "part0":
                    P.append(f"double* __restrict__ t{ti}_blk")
                k = int(nm[4:])
                names.append(f"({decl})(t{ti}_blk + {2 * int(t['groups']) * k})")
                continue
            P.append(f"{decl} t{ti}_{nm}")
            names.append(f"t{ti}_{nm}")
        gt = t.get("groups")  # this term's workgroup count (cost-proportional, dispatch/wide.py); default: the whole grid column
        if finish:
            fin0, _ = multi_finish_layout(nred, int(gt))
            names += [f"({CTYPE[rs[1]]}*)(t{ti}_blk + {fin0 + k})" for k, rs in enumerate(t["rs"])] + [f"pt_tickets + {ti}", "pt_status"]
        if gt:
            calls.append(f"    case {ti}: if (blockIdx.y < {int(gt)}) {fn_of[ti]}({', '.join(names)}, blockIdx.y, {int(gt)}u); break;")
        else:
            calls.append(f"    case {ti}: {fn_of[ti]}({', '.join(names)}, blockIdx.y, gridDim.y); break;")
    if finish:
        P += ["int* __restrict__ pt_tickets", "int* __restrict__ pt_status"]
    L = head + [f for _, f in fns.values()]
    L.append(f'extern "C" __global__ __launch_bounds__({BLOCK}) void {name}({", ".join(P)}) {{')
    # grid (terms, workgroups per term), the term rotated by the round: consecutive workgroup ids — which the
    # dispatcher deals out round-robin over XCDs and CUs — belong to different terms AND the ids a CU's slots receive
    # (c, c + 256, ...) to different families.  With the term on blockIdx.y and four families cycling through the terms
    # every CU's eight slots held the SAME family: the CUs of the expensive one ran 3x longer than the rest idled
    # (north_star's 48-term graph: mean occupancy 7 of 32 waves per CU, profiles/r5h_wide_multi_pmc.md).
    L.append("  switch ((blockIdx.x + blockIdx.y) % gridDim.x) {")
    L += calls
    L.append("    default: break;")
    L.append("  }")
    L.append("}")
    return "\n".join(L)


def _flat_scalar_block(body, modes, reduce_spec, V, pvar):
    lines = []
    for k, m in enumerate(modes):
        if m == "V":
            ct = CTYPE[body["in_dtypes"][k]]
            lines.append(f"    const {_vec_type(ct, V)} a{k} = reinterpret_cast<const {_vec_type(ct, V)}*>(in{k})[{pvar}];")
    for k, dt in enumerate(body["out_dtypes"]):
        if reduce_spec[k] is None:
            lines.append(f"    {_vec_type(CTYPE[dt], V)} r{k};")
    lines.append(f"#pragma unroll\n    for (int e = 0; e < {V}; e++) {{")
    in_names = [(f"a{k}.v[e]" if m == "V" else f"s{k}") for k, m in enumerate(modes)]
    out_names = []
    for k, dt in enumerate(body["out_dtypes"]):
        if reduce_spec[k] is None:
            out_names.append(f"r{k}.v[e]")
        else:
            lines.append(f"      {CTYPE[dt]} o{k};")
            out_names.append(f"o{k}")
    lines.append(emit_body(body, in_names, out_names))
    for k, rs in enumerate(reduce_spec):
        if rs is not None:
            lines.append(f"      acc{k}_0 = pthip_dev::{REDUCE_OPS[rs[0]]}::apply(acc{k}_0, ({CTYPE[rs[1]]})o{k});")
    lines.append("    }")
    for k, dt in enumerate(body["out_dtypes"]):
        if reduce_spec[k] is None:
            lines.append(f"    reinterpret_cast<{_vec_type(CTYPE[dt], V)}*>(out{k})[{pvar}] = r{k};")
    return "\n".join(lines)


def _flat_elem(body, modes, reduce_spec, ivar):
    lines = []
    in_names = []
    for k, m in enumerate(modes):
        if m == "V":
            in_names.append(f"in{k}[{ivar}]")
        elif m == "G":
            # NumPy index semantics: negative wraps once, out of range is an IndexError (raised
            # by the host from the device flag; the lane reads entry 0 meanwhile)
            lines.append(f"      long long gi{k} = gx{k}[{ivar}];")
            lines.append(f"      if (gi{k} < 0) gi{k} += gn{k};")
            lines.append(f"      if (gi{k} < 0 || gi{k} >= gn{k}) {{ atomicOr(status, 1); gi{k} = 0; }}")
            in_names.append(f"in{k}[gi{k}]")
        else:
            in_names.append(f"s{k}")
    out_names = []
    for k, dt in enumerate(body["out_dtypes"]):
        lines.append(f"      {CTYPE[dt]} o{k};")
        out_names.append(f"o{k}")
    lines.append(emit_body(body, in_names, out_names))
    for k, rs in enumerate(reduce_spec):
        if rs is None:
            lines.append(f"      out{k}[{ivar}] = o{k};")
        else:
            lines.append(f"      acc{k}_0 = pthip_dev::{REDUCE_OPS[rs[0]]}::apply(acc{k}_0, ({CTYPE[rs[1]]})o{k});")
    return "\n".join(lines)


FINISH_MAX_PER_THREAD = 8  # pairs a thread of the last workgroup folds: one-pass reductions need gridDim.x <= 8 * BLOCK

PT_PAIR_HELPERS = r"""
// one-pass reductions: a workgroup's partial travels as a self-validating 16-byte pair {bits, bits ^ MAGIC} in one
// write-through store; the last workgroup polls the pairs (agent-scope loads) — no fence anywhere.  (A fence per
// workgroup — __threadfence() before a ticket — made BASELINE config #2 ten times slower: every agent-scope
// release / acquire writes back and invalidates the XCD's L2 under 2000 streaming workgroups,
// profiles/r4i_c2_ab.txt.)
typedef unsigned long long pt_u64;
typedef pt_u64 pt_u2 __attribute__((ext_vector_type(2)));
static constexpr pt_u64 PT_PAIR_MAGIC = 0x7ff4c0de5ea1ed03ull;
static __device__ __forceinline__ void pt_pair_store(pt_u64* slot, pt_u64 lo, pt_u64 hi) {
  pt_u2 pr = {lo, hi};
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 2" : : "v"((pt_u2*)slot), "v"(pr) : "memory");
}
static __device__ __forceinline__ bool pt_pair_poll(const pt_u64* slot, pt_u64& bits) {
  bits = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const pt_u64 b = __hip_atomic_load(slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (bits ^ b) == PT_PAIR_MAGIC;
}
"""


def _reduce_epilogue(reduce_spec, unroll, finish=None, per_thread=None):
    """``finish`` (per output: final dtype | None): ONE pass — every workgroup publishes its partial as a
    self-validating pair and takes a ticket (a relaxed device atomic); the last one to arrive polls all pairs, folds
    them in a fixed order (thread t takes partials t, t+BLOCK, ... in order, then the block combine: deterministic
    for a given grid), stores the final value and zeroes the pairs for the next launch of this kernel.  The
    second-stage launch (~3 us + a launch gap behind a 30 us streaming kernel) goes away, and no fence is needed.
    ``part{k}`` is then the pair array (2 x 8 bytes per workgroup)."""
    if not any(reduce_spec):
        return ""
    FM = per_thread or FINISH_MAX_PER_THREAD
    lines = []
    for k, rs in enumerate(reduce_spec):
        if rs is None:
            continue
        act = CTYPE[rs[1]]
        op = f"pthip_dev::{REDUCE_OPS[rs[0]]}"
        lines.append(f"  __shared__ {act} smem{k}[{BLOCK // 64}];")
        e = f"acc{k}_0"
        for u in range(1, unroll):
            e = f"{op}::apply({e}, acc{k}_{u})"
        lines.append(f"  {act} tot{k} = pthip_dev::block_reduce<{op}, {act}, {BLOCK}>({e}, smem{k});")
        if finish:
            lines.append(f"  if (threadIdx.x == 0) {{ pt_u64 b = 0; __builtin_memcpy(&b, &tot{k}, sizeof(tot{k})); pt_pair_store((pt_u64*)part{k} + 2 * blockIdx.x, b, b ^ PT_PAIR_MAGIC); }}")
        else:
            lines.append(f"  if (threadIdx.x == 0) part{k}[blockIdx.x] = tot{k};")
    if finish:
        lines.append("  __shared__ int pt_last;")
        lines.append("  if (threadIdx.x == 0) pt_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;")
        lines.append("  __syncthreads();")
        lines.append("  if (pt_last) {")
        lines.append("    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);")
        for k, rs in enumerate(reduce_spec):
            if rs is None:
                continue
            act = CTYPE[rs[1]]
            op = f"pthip_dev::{REDUCE_OPS[rs[0]]}"
            lines.append(f"    {act} fa{k} = {op}::identity<{act}>();")
            lines.append("    {")
            # all of a thread's pairs are requested before the first is examined: one memory round trip for the
            # whole fold (polled one after the other the 8 pairs of a thread cost ~1 us each)
            lines.append(f"      pt_u64 b[{FM}];")
            lines.append(f"      bool got[{FM}];")
            lines.append(f"#pragma unroll\n      for (int u = 0; u < {FM}; u++) {{ b[u] = 0; got[u] = threadIdx.x + u * {BLOCK} >= gridDim.x; }}")
            lines.append("      for (long long spins = 0;; spins++) {")
            lines.append("        bool all = true;")
            lines.append(f"#pragma unroll\n        for (int u = 0; u < {FM}; u++)")
            lines.append(f"          if (!got[u]) {{ got[u] = pt_pair_poll((const pt_u64*)part{k} + 2 * (threadIdx.x + u * {BLOCK}), b[u]); all = all && got[u]; }}")
            lines.append("        if (all) break;")
            lines.append("        if (spins > (1ll << 22)) { atomicOr(pt_status, 16); break; }")
            lines.append("      }")
            lines.append(f"#pragma unroll\n      for (int u = 0; u < {FM}; u++)")
            lines.append(f"        if (threadIdx.x + u * {BLOCK} < gridDim.x) {{")
            lines.append(f"          {act} v; __builtin_memcpy(&v, &b[u], sizeof(v));")
            lines.append(f"          fa{k} = {op}::apply(fa{k}, v);")
            lines.append(f"          pt_pair_store((pt_u64*)part{k} + 2 * (threadIdx.x + u * {BLOCK}), 0, 0);  // clean for the next launch")
            lines.append("        }")
            lines.append("    }")
            lines.append("    __syncthreads();")
            lines.append(f"    fa{k} = pthip_dev::block_reduce<{op}, {act}, {BLOCK}>(fa{k}, smem{k});")
            lines.append(f"    if (threadIdx.x == 0) fin{k}[0] = ({CTYPE[finish[k]]})fa{k};")
        lines.append("  }")
    return "\n".join(lines)


MAX_ND = 5


def nd_kernel_source(name: str, body: dict, ndim: int, reduce_spec=None, partial=(), byvalue=()) -> str:
    """General broadcasting loop: collapsed ``ndim``-d index (row-major over the output
    shape), per-operand element strides (0 on broadcast dims); outputs contiguous.

    ``partial``: input positions that arrive as unfinished split-K slabs ``[np][n]`` (contiguous,
    same iteration space as the output): the value is their sum in ascending slab order — the
    order ``splitk_finish_kernel`` uses — folded into this kernel instead of a launch of its own."""
    nin = len(body["in_dtypes"])
    nout = len(body["out_dtypes"])
    reduce_spec = reduce_spec or [None] * nout
    partial = set(partial)
    byvalue = set(byvalue)
    params = ["long long n"]
    params += [f"long long d{j}" for j in range(ndim)]
    for k, dt in enumerate(body["in_dtypes"]):
        if k in byvalue:  # host-known scalar: travels in the argument block
            params.append(f"const long long in{k}")
            continue
        params.append(f"const {CTYPE[dt]}* __restrict__ in{k}")
        if k in partial:
            # np slabs, slab stride ps; rows of pn elements, pld apart (a column block of wider slabs)
            params += [f"long long np{k}", f"long long ps{k}", f"long long pn{k}", f"long long pld{k}"]
        else:
            params += [f"long long s{k}_{j}" for j in range(ndim)]
    for k, dt in enumerate(body["out_dtypes"]):
        if reduce_spec[k] is None:
            params.append(f"{CTYPE[dt]}* __restrict__ out{k}")
        else:
            params.append(f"{CTYPE[reduce_spec[k][1]]}* __restrict__ part{k}")
    src = [device_header("reduce_device.h") if any(reduce_spec) else "", prelude_for(body)]
    src.append(f'extern "C" __global__ __launch_bounds__({BLOCK}) void {name}({", ".join(params)}) {{')
    for k, rs in enumerate(reduce_spec):
        if rs is not None:
            act = CTYPE[rs[1]]
            src.append(f"  {act} acc{k}_0 = pthip_dev::{REDUCE_OPS[rs[0]]}::identity<{act}>();")
    for k in sorted(byvalue):
        ct = CTYPE[body["in_dtypes"][k]]
        src.append(f"  {ct} bv{k}; {{ const long long b = in{k}; __builtin_memcpy(&bv{k}, &b, sizeof({ct})); }}")
    src.append(f"  for (long long i = (long long)blockIdx.x * {BLOCK} + threadIdx.x; i < n; i += (long long)gridDim.x * {BLOCK}) {{")
    src.append("      long long rem = i;")
    for j in range(ndim - 1, 0, -1):
        src.append(f"      const long long c{j} = rem % d{j}; rem /= d{j};")
    src.append("      const long long c0 = rem;")
    in_names = []
    for k in range(nin):
        if k in byvalue:
            in_names.append(f"bv{k}")
            continue
        if k in partial:
            ct = CTYPE[body["in_dtypes"][k]]
            # eight independent loads in flight, added in ascending slab order (deterministic)
            src.append(f"      const long long pi{k} = (pld{k} == pn{k}) ? i : (i / pn{k}) * pld{k} + (i % pn{k});")
            src.append(f"      {ct} p{k} = in{k}[pi{k}];")
            src.append(f"      long long sl{k} = 1;")
            src.append(f"      for (; sl{k} + 7 < np{k}; sl{k} += 8) {{")
            src.append(f"        {ct} q{k}[8];")
            src.append(f"#pragma unroll\n        for (int u = 0; u < 8; u++) q{k}[u] = in{k}[(sl{k} + u) * ps{k} + pi{k}];")
            src.append(f"#pragma unroll\n        for (int u = 0; u < 8; u++) p{k} += q{k}[u];")
            src.append("      }")
            src.append(f"      for (; sl{k} < np{k}; sl{k}++) p{k} += in{k}[sl{k} * ps{k} + pi{k}];")
            in_names.append(f"p{k}")
            continue
        off = " + ".join(f"c{j} * s{k}_{j}" for j in range(ndim)) or "0"
        in_names.append(f"in{k}[{off}]")
    out_names = []
    for k, dt in enumerate(body["out_dtypes"]):
        src.append(f"      {CTYPE[dt]} o{k};")
        out_names.append(f"o{k}")
    src.append(emit_body(body, in_names, out_names))
    for k, rs in enumerate(reduce_spec):
        if rs is None:
            src.append(f"      out{k}[i] = o{k};")
        else:
            src.append(f"      acc{k}_0 = pthip_dev::{REDUCE_OPS[rs[0]]}::apply(acc{k}_0, ({CTYPE[rs[1]]})o{k});")
    src.append("  }")
    src.append(_reduce_epilogue(reduce_spec, 1))
    src.append("}")
    return "\n".join(src)


def source_key(src: str) -> str:
    return hashlib.sha256(src.encode()).hexdigest()[:24]
