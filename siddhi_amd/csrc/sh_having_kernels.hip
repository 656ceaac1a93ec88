// sh_having_kernels.hip — `having` on the batch group-by selector (sh_having.h), gfx950.
//
// QuerySelector.processInBatchGroupBy (QuerySelector.java:315-374) tests the condition after every event
// of a chunk on the key's running aggregates and keeps the event only when it passes. The pending
// entries are sorted by (window, key slot) as for stream.current.event (sh_kernels.hip k_sc_*); one
// thread folds each (window, key) run in event order and evaluates the program after every entry of
// the current call. Per (chunk, key) group it leaves k_sc_emit's contract: ghead at the group's FIRST
// passing entry (the row's position), slast / sval the LAST passing entry and the values there.
#include "sh_device.h"
#include "sh_having.h"

namespace shd {

// the running state a program reads: the key's values (scalars: a run-time choice between two array
// elements would index the array) and the key's count after the current event; the folded fields go
// beside it as the array they are
struct HvRow {
    i64 k0, k1;
    u32 c;
};

// operand `o` (SH_OP_KEY / SH_OP_AGG) in java_cmp's raw 8-byte form; only the aggregate a program names
// is finished (agg_out: avg divides). nul: the operand is Java null — never for a batch window, whose
// count is at least 1; the rule (a null operand makes a comparison false,
// CompareConditionExpressionExecutor.java:38-42) stays in the evaluator for windows whose rows can be null
__device__ __forceinline__ void hv_operand(const FilterOpD& o, const u64 (&f)[SH_MAX_AGGS], const HvRow& r, u32 null_mask,
                                           int& t, i64& v, bool& nul) {
    t = o.type;
    if (o.op == SH_OP_KEY) {
        v = o.col ? r.k1 : r.k0;
        nul = false;
        return;
    }
    // (the aggregate's field and kind stand in the op itself — sh_query_set_having — so the plan's arrays
    // are never indexed by a run-time number)
    // (a mask per field, not a chain of selects: the compiler turns that chain into one load at a
    // selected address, which puts the fields into scratch)
    u64 fv = 0;
#pragma unroll
    for (int j = 0; j < SH_MAX_AGGS; j++) fv |= f[j] & (u64)(-(i64)(o.pad == j));
    v = (i64)agg_out_kind((int)o.ival, r.c, fv);
    nul = (null_mask >> o.col) & 1u;
}

// `agg|key <cmp> const` (ops i .. i+2) in registers
__device__ __forceinline__ bool hv_leaf(const HavingProg& h, int i, const u64 (&f)[SH_MAX_AGGS], const HvRow& r, u32 null_mask) {
    int tc, ta;
    i64 vc, va;
    bool nul;
    filter_const(h.ops[i + 1], tc, vc);
    hv_operand(h.ops[i], f, r, null_mask, ta, va, nul);
    return !nul && java_cmp(h.ops[i + 2].op, ta, va, tc, vc);
}

// HK narrows the forms an instance handles (having_kind on the host): 1 the register-only forms, 2 any
// program. The program is a kernel argument, so every branch on it is uniform.
template <int HK>
__device__ __forceinline__ bool hv_eval(const HavingProg& h, const u64 (&f)[SH_MAX_AGGS], const HvRow& r, u32 null_mask) {
    if (HK == 1) {
        if (h.n == 3) return hv_leaf(h, 0, f, r, null_mask);
        const bool a = hv_leaf(h, 0, f, r, null_mask), b = hv_leaf(h, 3, f, r, null_mask);
        return h.ops[6].op == SH_OP_AND ? (a && b) : (a || b);
    }
    // the general stack machine (the fallback only: a runtime-indexed operand stack costs registers or scratch)
    i64 sv[16];
    int st[16];
    u32 sn = 0;  // bit i: stack entry i is null
    int sp = 0;
    for (int i = 0; i < h.n; i++) {
        const FilterOpD& o = h.ops[i];
        switch (o.op) {
            case SH_OP_KEY:
            case SH_OP_AGG: {
                int t;
                i64 v;
                bool nul;
                hv_operand(o, f, r, null_mask, t, v, nul);
                sv[sp] = v; st[sp] = t;
                sn = nul ? sn | (1u << sp) : sn & ~(1u << sp);
                sp++;
                break;
            }
            case SH_OP_CONST: {
                int t;
                i64 v;
                filter_const(o, t, v);
                sv[sp] = v; st[sp] = t;
                sn &= ~(1u << sp);
                sp++;
                break;
            }
            case SH_OP_AND: sp--; sv[sp - 1] = (sv[sp - 1] && sv[sp]) ? 1 : 0; st[sp - 1] = SH_T_BOOL; break;
            case SH_OP_OR: sp--; sv[sp - 1] = (sv[sp - 1] || sv[sp]) ? 1 : 0; st[sp - 1] = SH_T_BOOL; break;
            case SH_OP_NOT: sv[sp - 1] = sv[sp - 1] ? 0 : 1; st[sp - 1] = SH_T_BOOL; break;
            default: {
                sp--;
                const bool nul = (sn >> (sp - 1)) & 3u;
                const bool res = !nul && java_cmp(o.op, st[sp - 1], sv[sp - 1], st[sp], sv[sp]);
                sv[sp - 1] = res ? 1 : 0;
                st[sp - 1] = SH_T_BOOL;
                sn &= ~(3u << (sp - 1));
            }
        }
    }
    return sp > 0 && sv[sp - 1] != 0;
}

__global__ __launch_bounds__(kBlock) void k_hv_keys(i64 M, i64 n_old, i64 seq0, const Segment* __restrict__ segs,
                                                   int nseg, const u32* __restrict__ pend_pos,
                                                   const u64* __restrict__ pend_gidx, u64* skey, u32* idx, i64* chunk,
                                                   i64* send) {
    const i64 m = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (m >= M) return;
    // combined index: the queued entries first, then the push's events by their index in the push
    const i64 ci = m < n_old ? m : n_old + ((i64)pend_gidx[m] - seq0);
    int lo = 0, hi = nseg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].hi <= ci) lo = mid + 1; else hi = mid;
    }
    const bool closed = lo < nseg;  // (nseg: an event of the window that stays open)
    chunk[m] = closed ? (i64)lo : -1;
    send[m] = -(i64)(closed ? lo : 0) - 1;
    skey[m] = ((u64)(u32)lo << 32) | (u64)pend_pos[m];
    idx[m] = (u32)m;
}

template <int HK>
__global__ __launch_bounds__(kBlock) void k_hv_walk(i64 M, const u32* __restrict__ pos, const u32* __restrict__ starts,
                                                   const u32* __restrict__ idx, const i64* __restrict__ chunk,
                                                   const u64* __restrict__ pend_vals, i64 pend_cap,
                                                   const u32* __restrict__ pend_pos, AggPlan ap, KeyTable kt, KeyPlan kp,
                                                   HavingProg hp, u32* ghead, u64* sval, u32* slast) {
    const i64 sg = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (sg >= (i64)pos[M]) return;
    const i64 i = starts[sg], hi = starts[sg + 1];
    u64 f[SH_MAX_AGGS];
#pragma unroll
    for (int j = 0; j < SH_MAX_AGGS; j++) f[j] = 0;
    u32 c = 0;
    u32 m_nx = idx[i];
    i64 ch_nx = chunk[m_nx];
    i64 kv[kKeyParts] = {0, 0};
    unpack_key(kp, slot_key(kt, pend_pos[m_nx]), kv, 1);
    // the group's first passing entry, and the state at its last passing entry (the row)
    i64 head = -1;
    u32 last_m = 0, last_c = 0;
    u64 last_f[SH_MAX_AGGS];
#pragma unroll
    for (int j = 0; j < SH_MAX_AGGS; j++) last_f[j] = 0;
    for (i64 t = i; t < hi; t++) {
        const u32 m = m_nx;
        const i64 ch = ch_nx;
        if (t + 1 < hi) {
            m_nx = idx[t + 1];
            ch_nx = chunk[m_nx];
        }
        i64 v[SH_MAX_AGGS];
#pragma unroll
        for (int j = 0; j < SH_MAX_AGGS; j++) v[j] = j < ap.n_vcols ? (i64)pend_vals[(size_t)j * pend_cap + m] : 0;
        fold_fields<SH_MAX_AGGS>(ap, f, c == 0, v);
        c++;
        if (ch < 0) continue;  // an earlier call's entry, or one of the window that stays open: folds only
        if (hv_eval<HK>(hp, f, HvRow{kv[0], kv[1], c}, 0u)) {
            if (head < 0) {
                head = m;
                ghead[m] = 1;
            }
            last_m = m;
            last_c = c;
#pragma unroll
            for (int j = 0; j < SH_MAX_AGGS; j++) last_f[j] = f[j];
        }
        if ((t + 1 == hi || ch_nx != ch) && head >= 0) {  // the group's last event: its row, if any entry passed
#pragma unroll
            for (int a = 0; a < SH_MAX_AGGS; a++) {
                if (a >= ap.n) break;
                u64 fv = last_f[0];
#pragma unroll
                for (int j = 1; j < SH_MAX_AGGS; j++) if (ap.field[a] == j) fv = last_f[j];
                sval[(size_t)head * ap.n + a] = agg_out(ap, a, last_c, fv);
            }
            slast[head] = last_m;
            head = -1;
        }
    }
}

void launch_hv_keys(hipStream_t s, i64 M, i64 n_old, i64 seq0, const Segment* segs, int nseg, const u32* pend_pos,
                    const u64* pend_gidx, u64* skey, u32* idx, i64* chunk, i64* send) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k_hv_keys, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, M, n_old, seq0, segs,
                       nseg, pend_pos, pend_gidx, skey, idx, chunk, send);
}

void launch_hv_walk(hipStream_t s, int kind, i64 M, const u32* pos, const u32* starts, const u32* idx, const i64* chunk,
                    const u64* pend_vals, i64 pend_cap, const u32* pend_pos, AggPlan ap, KeyTable kt, KeyPlan kp,
                    HavingProg hp, u32* ghead, u64* sval, u32* slast) {
    if (M <= 0) return;
    const dim3 grid((unsigned)((M + kBlock - 1) / kBlock));
    if (kind == 1)
        hipLaunchKernelGGL(k_hv_walk<1>, grid, dim3(kBlock), 0, s, M, pos, starts, idx, chunk, pend_vals, pend_cap,
                           pend_pos, ap, kt, kp, hp, ghead, sval, slast);
    else
        hipLaunchKernelGGL(k_hv_walk<2>, grid, dim3(kBlock), 0, s, M, pos, starts, idx, chunk, pend_vals, pend_cap,
                           pend_pos, ap, kt, kp, hp, ghead, sval, slast);
}

}  // namespace shd
