"""Tail kernel: a chain of small nodes in ONE single-workgroup launch (tailfuse.py)"""

from __future__ import annotations

import os

from pytensor_amd.codegen import REDUCE_OPS
from pytensor_amd.codegen_scalar import CTYPE, device_header, emit_body, prelude_for

TAIL_BLOCK = 256

TAIL_SHRINK_MAX_TASKS = 4  # the by-value task table of the fused form (csrc/tail_device.h TailTasksT<4>, 192 bytes)


def tail_shrink_pack(tasks):
    """``TailTasksT<4>`` as kernel-argument bytes: ``tasks`` = [(op code, part ptr, nparts, M, S, out ptr)];
    returns (bytes, number of blocks)."""
    import struct

    n = len(tasks)
    assert 1 <= n <= TAIL_SHRINK_MAX_TASKS
    pad = TAIL_SHRINK_MAX_TASKS - n
    blk0, nb = [], 0
    for _, _, _, M, S, _ in tasks:
        blk0.append(nb)
        nb += (int(M) + 15) // 16 * int(S)
    blk0 += [nb] * (pad + 1)
    col = lambda k, fill=0: [int(t[k]) for t in tasks] + [fill] * pad
    buf = struct.pack("<i4i4x4Q4q4q4i4Q5i4x", n, *col(0), *col(1), *col(2), *col(3, 1), *col(4, 1), *col(5), *blk0)
    assert len(buf) == 192
    return buf, nb


def _tail_prologue(L, shrink):
    """``shrink`` = {"dtype": accumulator dtype}: the launch has one workgroup per slab piece; each shrinks its
    piece (csrc/tail_device.h, the code of pthip_multi_finish), takes a ticket, and only the LAST one to finish
    goes on to the chain (release: fence before the ticket; acquire: fence after it) and puts the ticket back."""
    # device-side join of a segmented plan's two streams (csrc/tail_device.h; include/pthip.h pthip_join_signal): wait
    # for the other stream's signal word and put it back.  Null outside such a plan.  Where kernels of different streams
    # cannot overlap (a counter-collecting profiler serialises them) the signal launch cannot run while this one spins:
    # the wait gives up after 1 ms and says so through the done word.
    L.append("  __shared__ int join_fail_;")
    L.append("  if (join_src != nullptr) {")
    L.append("    if (tid == 0) {")
    L.append("      const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime();")
    L.append("      // 1 ms when the host can run this segment again (it polls done_dst), else 3 s and the status bit")
    L.append("      const unsigned long long lim_ = done_dst != nullptr ? 100000ull : 300000000ull;")
    L.append("      int ok_ = 1;")
    L.append("      while (__hip_atomic_load(join_src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {")
    L.append("        __builtin_amdgcn_s_sleep(2);")
    L.append("        if (__builtin_amdgcn_s_memrealtime() - t0_ > lim_) { ok_ = 0; break; }")
    L.append("      }")
    L.append("      if (ok_) __hip_atomic_store(join_src, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);")
    L.append("      else if (done_dst != nullptr) __hip_atomic_store(done_dst, 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);")
    L.append("      else if (status_src != nullptr) atomicOr((int*)status_src, 16);")
    L.append("      join_fail_ = !ok_ && done_dst != nullptr;")
    L.append("    }")
    if os.environ.get("PTHIP_JOIN_FENCE", "0") == "1":
        # opt-in: the formally ordered form — an agent-scope acquire behind the wait.  It invalidates this XCD's L2, so
        # the slab this launch shrinks next comes back from HBM (4.8 -> 11 us, profiles/r4_c4_device_join.txt): the
        # default leans on the invalidate every kernel start performs instead, checked by pthip_join_probe per process.
        L.append("    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, \"agent\");")
    L.append("    __syncthreads();  // (default: no acquire fence — see csrc/tail_device.h plan_join_wait; PTHIP_JOIN_FENCE=1 adds one)")
    L.append("    if (join_fail_) return;  // done word 2: pthip_plan_replay4 waits for the other stream and runs this segment again")
    L.append("  }")
    if not shrink:
        return
    ct = CTYPE[shrink["dtype"]]
    L.append("  {  // prologue: the partial slabs shrink in THIS launch; the last workgroup to finish runs the chain")
    L.append(f"    __shared__ {ct} shr_[{TAIL_BLOCK}];")
    L.append("    __shared__ int last_;")
    L.append(f"    pthip_dev::tail_shrink_block<{ct}, {TAIL_SHRINK_MAX_TASKS}>(tasks_, (int)blockIdx.x, shr_);")
    L.append("    __threadfence();")
    L.append("    __syncthreads();")
    L.append("    if (tid == 0) last_ = atomicAdd(ticket_, 1) == (int)gridDim.x - 1;")
    L.append("    __syncthreads();")
    L.append("    if (!last_) return;")
    L.append("    if (tid == 0) __hip_atomic_store(ticket_, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);")
    L.append("    __threadfence();")
    L.append("  }")


def _tail_epilogue(L, spec):
    for k, o in enumerate(spec["outs"]):
        L.append(f"  for (long long i = tid; i < len{k}; i += {TAIL_BLOCK}) dst{k}[i] = l{o}[i];")
    L.append("  if (tid == 0 && status_dst != nullptr) *status_dst = __hip_atomic_load(status_src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);")
    # the plan's completion word (pinned host memory, polled by pthip_plan_replay4): behind every result store
    L.append("  if (done_dst != nullptr) {")
    L.append("    __threadfence_system();")
    L.append("    __syncthreads();")
    L.append("    if (tid == 0) __hip_atomic_store(done_dst, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);")
    L.append("  }")
    L.append("}")


def tail_chain_source(name: str, spec: dict, sizes: dict | None = None, shrink: dict | None = None) -> str:
    """One workgroup runs ``spec["steps"]`` in order, intermediates in LDS.

    ``spec`` is purely structural (extents are kernel arguments, so one code object serves every
    size):

    * ``ext``   — external operands: ``{"kind": "V" (vector: pointer + element stride) | "S"
      (device scalar) | "C" (host scalar by value) | "P" (row-major partial slab / partials),
      "dtype"}``;
    * ``slots`` — LDS values ``{"dtype"}`` (byte offset and length arrive as arguments);
    * ``steps`` — ``finish``: ``out[i] = beta*y[i] + alpha*sum_s src[s*M+i]`` (the second stage +
      epilogue of a split Gemv / scatter-add, blas/gemv.py:64-108; ``y`` optional),
      ``rsum``: a deferred full reduction over ``rows`` partials (elemwise.py:1233 second stage),
      ``ew``: an ``Elemwise`` / ``ElemwiseReduce`` over ``n`` elements with per-operand modes;
    * ``outs``  — LDS slots copied to their destinations at the end; optional status-word copy.

    Operand references are ``("e", k)`` (external) or ("l", k) (LDS slot).  Argument order =
    the order of ``tail_chain_args``.
    """
    ext, slots, steps = spec["ext"], spec["slots"], spec["steps"]
    P = []
    for k, e in enumerate(ext):
        ct = CTYPE[e["dtype"]]
        if e["kind"] == "C":
            P.append(f"const long long ec{k}")
        elif e["kind"] == "V":
            P += [f"const {ct}* __restrict__ e{k}", f"const long long es{k}"]
        else:
            P.append(f"const {ct}* __restrict__ e{k}")
    # one-element slots sit at static offsets (16 B apart, first in the LDS block): a wide graph has
    # hundreds of them and the kernel-argument block is 4 KB; vector slots get run-time offsets
    for k in range(len(slots)):
        if not slots[k].get("scalar"):
            P += [f"const long long off{k}"]
    for j, st in enumerate(steps):
        if st["op"] == "finish":
            P += [f"const long long rows{j}", f"const long long M{j}", f"const double alpha{j}", f"const double beta{j}"]
        elif st["op"] == "rsum":
            P += [f"const long long rows{j}"]
        else:
            P += [f"const long long n{j}"]
    for k, o in enumerate(spec["outs"]):
        P += [f"{CTYPE[slots[o]['dtype']]}* __restrict__ dst{k}", f"const long long len{k}"]
    P += ["const int* status_src", "int* status_dst", "int* done_dst", "int* join_src"]
    if shrink:
        P += [f"const pthip_dev::TailTasksT<{TAIL_SHRINK_MAX_TASKS}> tasks_", "int* ticket_"]
    bodies = [st["body"] for st in steps if st["op"] == "ew"]
    if sizes is not None:
        return _tail_preload_source(name, spec, sizes, P, bodies, shrink)
    L = [device_header("reduce_device.h"), device_header("tail_device.h") if shrink else "", prelude_for(*bodies)]
    L.append(f'extern "C" __global__ __launch_bounds__({TAIL_BLOCK}) void {name}({", ".join(P)}) {{')
    L.append("  extern __shared__ __attribute__((aligned(16))) unsigned char lds_[];")
    L.append("  __shared__ double red_[8];")
    L.append("  const int tid = threadIdx.x;")
    _tail_prologue(L, shrink)
    for k, e in enumerate(ext):
        if e["kind"] == "C":
            ct = CTYPE[e["dtype"]]
            L.append(f"  {ct} c{k}; {{ const long long b = ec{k}; __builtin_memcpy(&c{k}, &b, sizeof({ct})); }}")
    n_sc = 0
    for k, s in enumerate(slots):
        ct = CTYPE[s["dtype"]]
        if s.get("scalar"):
            L.append(f"  {ct}* const l{k} = ({ct}*)(lds_ + {16 * n_sc});")
            n_sc += 1
        else:
            L.append(f"  {ct}* const l{k} = ({ct}*)(lds_ + off{k});")

    def operand(ref, mode, i="i"):
        kind, k = ref
        if kind == "e":
            e = ext[k]
            if e["kind"] == "C":
                return f"c{k}"
            if e["kind"] == "V":
                return f"e{k}[{i} * es{k}]" if mode == "V" else f"e{k}[0]"
            return f"e{k}[0]"
        return f"l{k}[{i}]" if mode == "V" else f"l{k}[0]"

    for j, st in enumerate(steps):
        if st["op"] == "finish":
            ct = CTYPE[st["dtype"]]
            src = f"e{st['src'][1]}"
            L.append(f"  // step {j}: second stage + epilogue of a split Gemv / scatter-add")
            L.append(f"  for (long long i = tid; i < M{j}; i += {TAIL_BLOCK}) {{")
            L.append(f"    {ct} a0 = 0, a1 = 0;")
            L.append(f"    long long s = 0;")
            L.append(f"    for (; s + 1 < rows{j}; s += 2) {{ a0 += {src}[s * M{j} + i]; a1 += {src}[(s + 1) * M{j} + i]; }}")
            L.append(f"    if (s < rows{j}) a0 += {src}[s * M{j} + i];")
            L.append(f"    {ct} r = ({ct})alpha{j} * (a0 + a1);")
            if st.get("y") is not None:
                L.append(f"    if (beta{j} != 0.0) r += ({ct})beta{j} * ({ct}){operand(st['y'], st['ymode'])};")
            L.append(f"    l{st['out']}[i] = r;")
            L.append("  }")
            L.append("  __syncthreads();")
        elif st["op"] == "rsum":
            act, oct_ = CTYPE[st["acc_dtype"]], CTYPE[st["dtype"]]
            op = REDUCE_OPS[st["red"]]
            src = f"e{st['src'][1]}"
            L.append(f"  // step {j}: deferred second stage of a fused Elemwise+reduce kernel")
            L.append("  {")
            L.append(f"    {act} a = pthip_dev::{op}::identity<{act}>();")
            L.append(f"    for (long long p = tid; p < rows{j}; p += {TAIL_BLOCK}) a = pthip_dev::{op}::apply(a, ({act}){src}[p]);")
            L.append(f"    a = pthip_dev::block_reduce<pthip_dev::{op}, {act}, {TAIL_BLOCK}, true>(a, ({act}*)red_);")
            L.append(f"    if (tid == 0) l{st['out']}[0] = ({oct_})a;")
            L.append("  }")
            L.append("  __syncthreads();")
        elif st["op"] == "scatter":
            ct = CTYPE[st["dtype"]]
            L.append(f"  // step {j}: a chain of one-element IncSubtensor updates (widefuse.collect_scalar_updates)")
            L.append(f"  for (long long i = tid; i < n{j}; i += {TAIL_BLOCK}) l{st['out']}[i] = ({ct}){operand(st['base'], st['bmode'])};")
            L.append("  __syncthreads();")
            L.append("  if (tid == 0) {")
            for k, is_set, y in zip(st["indices"], st["set"], st["ys"]):
                L.append(f"    l{st['out']}[{k}] {'=' if is_set else '+='} ({ct}){operand(y, 'S')};")
            L.append("  }")
            L.append("  __syncthreads();")
        else:
            body, modes, red = st["body"], st["modes"], st["reduce"]
            L.append(f"  // step {j}: Elemwise over n{j} elements, operand modes {modes}")
            L.append("  {")
            for q, r in enumerate(red):
                if r is not None:
                    act = CTYPE[r[1]]
                    L.append(f"    {act} acc{q} = pthip_dev::{REDUCE_OPS[r[0]]}::identity<{act}>();")
            L.append(f"    for (long long i = tid; i < n{j}; i += {TAIL_BLOCK}) {{")
            in_names = [operand(ref, m) for ref, m in zip(st["ins"], modes)]
            out_names = []
            for q, dt in enumerate(body["out_dtypes"]):
                L.append(f"      {CTYPE[dt]} o{q};")
                out_names.append(f"o{q}")
            L.append(emit_body(body, in_names, out_names, indent="      "))
            for q, r in enumerate(red):
                if r is None:
                    L.append(f"      l{st['outs'][q]}[i] = o{q};")
                else:
                    L.append(f"      acc{q} = pthip_dev::{REDUCE_OPS[r[0]]}::apply(acc{q}, ({CTYPE[r[1]]})o{q});")
            L.append("    }")
            for q, r in enumerate(red):
                if r is not None:
                    act = CTYPE[r[1]]
                    L.append(f"    acc{q} = pthip_dev::block_reduce<pthip_dev::{REDUCE_OPS[r[0]]}, {act}, {TAIL_BLOCK}, true>(acc{q}, ({act}*)red_);")
                    L.append(f"    if (tid == 0) l{st['outs'][q]}[0] = ({CTYPE[r[2]]})acc{q};")
            L.append("  }")
            L.append("  __syncthreads();")
    _tail_epilogue(L, spec)
    return "\n".join(L)


TAIL_PRELOAD_MAX_REGS = 160  # 8-byte values a thread may hold in flight in the preloading form
TAIL_WAVE_FOLD_INTERLEAVED = os.environ.get("PTHIP_TAIL_FOLD_INTERLEAVED", "1") != "0"
TAIL_WAVE_Q = int(os.environ.get("PTHIP_TAIL_WAVE_Q", 4))  # a wave folds deferred reductions of up to 64 * this many partials
TAIL_SCALAR_STEPS_BY_WAVE = os.environ.get("PTHIP_TAIL_SCALAR_BY_WAVE", "1") != "0"


def tail_preload_sizes(spec: dict, ext_len, step_n):
    """Static size classes for ``tail_chain_source(..., sizes=)`` or ``None`` when the operands
    are too long to sit in registers.  ``ext_len[k]``: elements of external ``k`` ("V"), rows of
    a partial array; ``step_n[j]``: ``(rows, M)`` of a finish step, ``rows`` of an rsum step,
    ``n`` of an elementwise step."""
    ext, steps = spec["ext"], spec["steps"]
    cl = lambda n: max(1, (int(n) + TAIL_BLOCK - 1) // TAIL_BLOCK)
    eu = [cl(ext_len[k]) if e["kind"] == "V" else 0 for k, e in enumerate(ext)]
    su, regs = [], sum(eu) + sum(1 for e in ext if e["kind"] in ("S", "V"))
    for st, n in zip(steps, step_n):
        if st["op"] == "finish":
            rows, M = n
            R = (int(rows) + 3) // 4 * 4
            su.append((R, cl(M)))
            regs += R * cl(M)
        elif st["op"] == "rsum":
            su.append(cl(n))
            regs += cl(n) if n > 64 * TAIL_WAVE_Q else 0  # (few partials: values in ONE wave's lanes, see "wave")
        else:
            su.append(cl(n))
    if regs > TAIL_PRELOAD_MAX_REGS or any((u[0] > 64 or u[1] > 4) if isinstance(u, tuple) else u > 16 for u in su) or any(u > 16 for u in eu):
        return None
    # deferred reductions over <= 64 * TAIL_WAVE_Q partials are folded by single waves, four at a time (a lane adds its
    # up to TAIL_WAVE_Q values in index order first)
    wave = [st["op"] == "rsum" and int(n) <= 64 * TAIL_WAVE_Q for st, n in zip(steps, step_n)]
    wave_q = [max(1, (int(n) + 63) // 64) if w else 0 for w, n in zip(wave, step_n)]
    return {"ext_u": eu, "step_u": su, "wave": wave, "wave_q": wave_q}


def _tail_preload_source(name: str, spec: dict, sizes: dict, P, bodies, shrink=None) -> str:
    """The chain with every *global* operand requested up front (one memory latency for the whole
    kernel instead of one per step — a single workgroup cannot hide it with occupancy): partial
    slabs and partial arrays are summed in registers as they arrive, vectors stay in registers;
    the steps then run out of registers and LDS.  Loop trip counts are static (``sizes``)."""
    ext, slots, steps = spec["ext"], spec["slots"], spec["steps"]
    eu, su = sizes["ext_u"], sizes["step_u"]
    L = [device_header("reduce_device.h"), device_header("tail_device.h") if shrink else "", prelude_for(*bodies)]
    L.append(f'extern "C" __global__ __launch_bounds__({TAIL_BLOCK}) void {name}({", ".join(P)}) {{')
    L.append("  extern __shared__ __attribute__((aligned(16))) unsigned char lds_[];")
    L.append("  __shared__ double red_[8];")
    L.append("  const int tid = threadIdx.x;")
    _tail_prologue(L, shrink)  # (before the operand requests below: the shrunk slabs are among them)
    for k, e in enumerate(ext):
        ct = CTYPE[e["dtype"]]
        if e["kind"] == "C":
            L.append(f"  {ct} c{k}; {{ const long long b = ec{k}; __builtin_memcpy(&c{k}, &b, sizeof({ct})); }}")
    n_sc = 0
    for k, s in enumerate(slots):
        ct = CTYPE[s["dtype"]]
        if s.get("scalar"):
            L.append(f"  {ct}* const l{k} = ({ct}*)(lds_ + {16 * n_sc});")
            n_sc += 1
        else:
            L.append(f"  {ct}* const l{k} = ({ct}*)(lds_ + off{k});")
    # ---- phase 0: every global operand in flight ------------------------------------------
    used_len = {}  # V external -> name of its length (first elementwise step reading it as a vector)
    for j, st in enumerate(steps):
        if st["op"] == "ew":
            for ref, m in zip(st["ins"], st["modes"]):
                if ref[0] == "e" and ext[ref[1]]["kind"] == "V" and m == "V":
                    used_len.setdefault(ref[1], f"n{j}")
        elif st["op"] == "finish" and st.get("y") is not None and st["y"][0] == "e" and st["ymode"] == "V":
            used_len.setdefault(st["y"][1], f"M{j}")
        elif st["op"] == "scatter" and st["base"][0] == "e" and st["bmode"] == "V" and ext[st["base"][1]]["kind"] == "V":
            used_len.setdefault(st["base"][1], f"n{j}")
    for k, e in enumerate(ext):
        ct = CTYPE[e["dtype"]]
        if e["kind"] == "S":
            L.append(f"  const {ct} s{k} = e{k}[0];")
        elif e["kind"] == "V":
            L.append(f"  const {ct} s{k} = e{k}[0];")
            if k in used_len:
                for u in range(eu[k]):
                    # clamped, unconditional (a predicated load becomes an exec-masked branch with its own wait)
                    L.append(f"  const {ct} v{k}_{u} = e{k}[(tid + {u * TAIL_BLOCK} < {used_len[k]} ? (long long)(tid + {u * TAIL_BLOCK}) : {used_len[k]} - 1) * es{k}];")
    wave = sizes.get("wave") or [False] * len(steps)
    for j, st in enumerate(steps):
        if st["op"] == "finish":
            ct = CTYPE[st["dtype"]]
            src = f"e{st['src'][1]}"
            R, U = su[j]
            for u in range(U):
                for r in range(R):
                    L.append(f"  {ct} f{j}_{u}_{r} = {src}[({r} < rows{j} ? {r} : rows{j} - 1) * M{j} + (tid + {u * TAIL_BLOCK} < M{j} ? tid + {u * TAIL_BLOCK} : M{j} - 1)];")
        elif st["op"] == "rsum" and not wave[j]:
            act = CTYPE[st["acc_dtype"]]
            op = REDUCE_OPS[st["red"]]
            src = f"e{st['src'][1]}"
            for u in range(su[j]):
                L.append(f"  {act} p{j}_{u} = ({act}){src}[tid + {u * TAIL_BLOCK} < rows{j} ? tid + {u * TAIL_BLOCK} : rows{j} - 1];")
    # deferred second stages over <= 64 partials: wave w folds every fourth of them with shuffles —
    # no LDS scratch, no barrier per reduction (a wide graph hands over ~3 per likelihood term)
    wsteps = [j for j, st in enumerate(steps) if st["op"] == "rsum" and wave[j]]
    if wsteps:
        L.append("  {")
        L.append("    const int wv_ = tid >> 6, ln_ = tid & 63;")
        for w in range(TAIL_BLOCK // 64):
            mine = wsteps[w :: TAIL_BLOCK // 64]
            if not mine:
                continue
            L.append(f"    if (wv_ == {w}) {{")
            wq = sizes.get("wave_q") or [1] * len(steps)
            for j in mine:
                st = steps[j]
                act = CTYPE[st["acc_dtype"]]
                for q in range(wq[j]):
                    L.append(f"      {act} w{j}_{q} = ({act})e{st['src'][1]}[ln_ + {64 * q} < rows{j} ? ln_ + {64 * q} : rows{j} - 1];")
            L.append("      __builtin_amdgcn_sched_barrier(0);")
            for j in mine:
                st = steps[j]
                act = CTYPE[st["acc_dtype"]]
                op = REDUCE_OPS[st["red"]]
                for q in range(wq[j]):
                    L.append(f"      if (ln_ + {64 * q} >= rows{j}) w{j}_{q} = pthip_dev::{op}::identity<{act}>();")
                L.append(f"      {act} w{j} = w{j}_0;")
                for q in range(1, wq[j]):
                    L.append(f"      w{j} = pthip_dev::{op}::apply(w{j}, w{j}_{q});")
            if TAIL_WAVE_FOLD_INTERLEAVED:
                # step-major: every butterfly level runs over ALL of this wave's reductions before the next level —
                # their cross-lane exchanges (two ds_bpermute per double, ~100 cycles each) are in flight together.
                # Value by value (round 5) a wide graph's ~36 reductions per wave were 36 x 6 dependent exchanges:
                # most of the 25 + 39 us of north_star's two tail launches (profiles/r7_wide200_*).  Same butterfly
                # per value: the same bits.
                L.append("#pragma unroll")
                L.append("      for (int off_ = 32; off_ > 0; off_ >>= 1) {")
                for j in mine:
                    L.append(f"        const auto x{j}_ = pthip_dev::shfl_xor_any(w{j}, off_);")
                for j in mine:
                    L.append(f"        w{j} = pthip_dev::{REDUCE_OPS[steps[j]['red']]}::apply(w{j}, x{j}_);")
                L.append("      }")
            else:
                for j in mine:
                    L.append(f"      w{j} = pthip_dev::wave_reduce<pthip_dev::{REDUCE_OPS[steps[j]['red']]}>(w{j});")
            for j in mine:
                st = steps[j]
                L.append(f"      if (ln_ == 0) l{st['out']}[0] = ({CTYPE[st['dtype']]})w{j};")
            L.append("    }")
        L.append("  }")
    L.append("  __builtin_amdgcn_sched_barrier(0);")
    for j, st in enumerate(steps):
        if st["op"] == "finish":
            R, U = su[j]
            for u in range(U):
                for r in range(R):
                    L.append(f"  if ({r} >= rows{j}) f{j}_{u}_{r} = 0;")
        elif st["op"] == "rsum" and not wave[j]:
            act = CTYPE[st["acc_dtype"]]
            for u in range(su[j]):
                L.append(f"  if (tid + {u * TAIL_BLOCK} >= rows{j}) p{j}_{u} = pthip_dev::{REDUCE_OPS[st['red']]}::identity<{act}>();")

    def operand(ref, mode, u):
        kind, k = ref
        if kind == "e":
            e = ext[k]
            if e["kind"] == "C":
                return f"c{k}"
            if e["kind"] == "V" and mode == "V":
                return f"v{k}_{u}"
            return f"s{k}"
        return f"l{k}[tid + {u * TAIL_BLOCK}]" if mode == "V" else f"l{k}[0]"

    # phases: a step reads LDS slots written in earlier phases only, so the steps of one phase need
    # no barrier between them (slots are written once); one __syncthreads() per phase instead of one
    # per step — the scalar bookkeeping of a wide graph is dozens of independent one-element steps
    def lds_reads(st):
        refs = []
        if st["op"] == "finish" and st.get("y") is not None:
            refs.append(st["y"])
        elif st["op"] == "ew":
            refs += list(st["ins"])
        elif st["op"] == "scatter":
            refs += [st["base"], *st["ys"]]
        return [r[1] for r in refs if r[0] == "l"]

    def lds_writes(st):
        return list(st["outs"]) if st["op"] == "ew" else [st["out"]]

    writer, phase = {}, []
    for j, st in enumerate(steps):
        ph = 0
        for k in lds_reads(st):
            if k in writer:
                ph = max(ph, phase[writer[k]] + 1)
        if st["op"] == "rsum" and wave[j]:
            ph = 0
        phase.append(ph)
        for k in lds_writes(st):
            writer[k] = j
    # the wave-folded reductions were emitted above: everything that reads them is in phase >= 1
    if wsteps:
        L.append("  __syncthreads();")
    def scalar_only(st):
        """an Elemwise step whose operands are all one-element values and that reduces nothing: n == 1 by construction"""
        return st["op"] == "ew" and all(m in "SC" for m in st["modes"]) and all(r is None for r in st["reduce"])

    for ph in range(max(phase, default=-1) + 1):
        emitted = False
        n_scalar = 0
        for j, st in enumerate(steps):
            if phase[j] != ph or (st["op"] == "rsum" and wave[j]):
                continue
            emitted = True
            if TAIL_SCALAR_STEPS_BY_WAVE and scalar_only(st):
                # The steps of a phase are independent of each other, and a one-element step is one lane's work: the
                # first lane of wave (k mod 4) takes the k-th of them, so four run side by side instead of thread 0
                # running all of them in a row (a wide graph: ~30 scalar Composites with an exp each per phase).
                body = st["body"]
                w_ = n_scalar % (TAIL_BLOCK // 64)
                n_scalar += 1
                L.append(f"  // step {j}: one-element Elemwise (operand modes {st['modes']}), on wave {w_}")
                L.append(f"  if (tid == {64 * w_}) {{")
                in_names = [operand(ref, m, 0) for ref, m in zip(st["ins"], st["modes"])]
                out_names = []
                for q, dt in enumerate(body["out_dtypes"]):
                    L.append(f"    {CTYPE[dt]} o{q};")
                    out_names.append(f"o{q}")
                L.append(emit_body(body, in_names, out_names, indent="    "))
                for q in range(len(body["out_dtypes"])):
                    L.append(f"    l{st['outs'][q]}[0] = o{q};")
                L.append("  }")
                continue
            if st["op"] == "finish":
                ct = CTYPE[st["dtype"]]
                R, U = su[j]
                L.append(f"  // step {j}: second stage + epilogue of a split Gemv / scatter-add (rows even/odd, then the pair: the order of the looping form)")
                for u in range(U):
                    L.append(f"  if (tid + {u * TAIL_BLOCK} < M{j}) {{")
                    L.append(f"    {ct} a0 = 0, a1 = 0;")
                    for r in range(0, R, 2):
                        L.append(f"    a0 += f{j}_{u}_{r}; a1 += f{j}_{u}_{r + 1};")
                    L.append(f"    {ct} r = ({ct})alpha{j} * (a0 + a1);")
                    if st.get("y") is not None:
                        L.append(f"    if (beta{j} != 0.0) r += ({ct})beta{j} * ({ct}){operand(st['y'], st['ymode'], u)};")
                    L.append(f"    l{st['out']}[tid + {u * TAIL_BLOCK}] = r;")
                    L.append("  }")
            elif st["op"] == "rsum":
                act, oct_ = CTYPE[st["acc_dtype"]], CTYPE[st["dtype"]]
                op = REDUCE_OPS[st["red"]]
                L.append(f"  // step {j}: deferred second stage of a fused Elemwise+reduce kernel")
                L.append("  {")
                L.append(f"    {act} a = pthip_dev::{op}::identity<{act}>();")
                for u in range(su[j]):
                    L.append(f"    a = pthip_dev::{op}::apply(a, p{j}_{u});")
                L.append(f"    a = pthip_dev::block_reduce<pthip_dev::{op}, {act}, {TAIL_BLOCK}, true>(a, ({act}*)red_);")
                L.append(f"    if (tid == 0) l{st['out']}[0] = ({oct_})a;")
                L.append("  }")
            elif st["op"] == "scatter":
                ct = CTYPE[st["dtype"]]
                L.append(f"  // step {j}: a chain of one-element IncSubtensor updates (widefuse.collect_scalar_updates)")
                for u in range(su[j]):
                    L.append(f"  if (tid + {u * TAIL_BLOCK} < n{j}) l{st['out']}[tid + {u * TAIL_BLOCK}] = ({ct}){operand(st['base'], st['bmode'], u)};")
                L.append("  __syncthreads();")
                L.append("  if (tid == 0) {")
                for k, is_set, y in zip(st["indices"], st["set"], st["ys"]):
                    L.append(f"    l{st['out']}[{k}] {'=' if is_set else '+='} ({ct}){operand(y, 'S', 0)};")
                L.append("  }")
            else:
                body, modes, red = st["body"], st["modes"], st["reduce"]
                L.append(f"  // step {j}: Elemwise over n{j} elements, operand modes {modes}")
                L.append("  {")
                for q, r in enumerate(red):
                    if r is not None:
                        act = CTYPE[r[1]]
                        L.append(f"    {act} acc{q} = pthip_dev::{REDUCE_OPS[r[0]]}::identity<{act}>();")
                for u in range(su[j]):
                    L.append(f"    if (tid + {u * TAIL_BLOCK} < n{j}) {{")
                    in_names = [operand(ref, m, u) for ref, m in zip(st["ins"], modes)]
                    out_names = []
                    for q, dt in enumerate(body["out_dtypes"]):
                        L.append(f"      {CTYPE[dt]} o{q};")
                        out_names.append(f"o{q}")
                    L.append(emit_body(body, in_names, out_names, indent="      "))
                    for q, r in enumerate(red):
                        if r is None:
                            L.append(f"      l{st['outs'][q]}[tid + {u * TAIL_BLOCK}] = o{q};")
                        else:
                            L.append(f"      acc{q} = pthip_dev::{REDUCE_OPS[r[0]]}::apply(acc{q}, ({CTYPE[r[1]]})o{q});")
                    L.append("    }")
                for q, r in enumerate(red):
                    if r is not None:
                        act = CTYPE[r[1]]
                        L.append(f"    acc{q} = pthip_dev::block_reduce<pthip_dev::{REDUCE_OPS[r[0]]}, {act}, {TAIL_BLOCK}, true>(acc{q}, ({act}*)red_);")
                        L.append(f"    if (tid == 0) l{st['outs'][q]}[0] = ({CTYPE[r[2]]})acc{q};")
                L.append("  }")
        if emitted:
            L.append("  __syncthreads();")
    _tail_epilogue(L, spec)
    return "\n".join(L)
