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
// is finished (agg_out: avg divides). nul: the operand is Java null — never for a CURRENT row of a batch
// window, whose count is at least 1, but an EXPIRED row's aggregates can be (k_hvx_walk's null mask); a
// null operand makes a comparison false (CompareConditionExpressionExecutor.java:38-42)
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

// ---- expired / all-events output of the stream.current.event batch windows --------------------------------
// A window that closes hands the selector EXPIRED copies of all its events in arrival order, then RESET
// (LengthBatchWindowProcessor.java:245-274, TimeBatchWindowProcessor.java:262-340). The selector removes
// each from its key's aggregators and tests the condition on the row after every removal
// (QuerySelector.java:280-291, :325-339): the key's expired row is that of its last PASSING removal, at the
// position of its first passing removal. k_hv_walk's fold, then for a run whose window closes in this call
// (w < nb) a second walk in the same order with the remove forms (sh_device.h) and the real null mask.
// Per run it leaves xhead at the first passing removal's entry, xlast / xval / xnul the last passing
// removal's entry and the row there, and xrun (at the run's first sorted entry) the head's entry or kNoHead.
// The CURRENT role is k_hv_walk's and only kept with current output on (cur_on): with `insert expired
// events` a current event folds but its row is never kept, so it need not be tested.
// dq: the min / max deques, field j of the run [i, hi) in dq[j * M + i, j * M + hi) (null: no such field).
constexpr u32 kNoHead = 0xFFFFFFFFu;

// value column j of an entry (a mask per column, as hv_operand: beside the deque loops the compiler turns
// pick<>'s chain of selects into one load at a selected address, which puts the columns into scratch)
__device__ __forceinline__ i64 hvx_pick(const i64 (&v)[SH_MAX_AGGS], int j) {
    i64 x = 0;
#pragma unroll
    for (int i = 0; i < SH_MAX_AGGS; i++) x |= v[i] & -(i64)(j == i);
    return x;
}

template <int HK>
__global__ __launch_bounds__(kBlock) void k_hvx_walk(i64 M, const u32* __restrict__ pos, const u32* __restrict__ starts,
                                                    const u32* __restrict__ idx, const i64* __restrict__ chunk,
                                                    const u64* __restrict__ skey, int nb, int cur_on,
                                                    const u64* __restrict__ pend_vals, i64 pend_cap,
                                                    const u32* __restrict__ pend_pos, AggPlan ap, KeyTable kt, KeyPlan kp,
                                                    HavingProg hp, u32* ghead, u64* sval, u32* slast, u32* xhead,
                                                    u64* xval, unsigned char* xnul, u32* xlast, u32* xrun, u32* dq) {
    const i64 sg = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (sg >= (i64)pos[M]) return;
    const i64 i = starts[sg], hi = starts[sg + 1];
    u64 f[SH_MAX_AGGS];
    u32 dl[SH_MAX_AGGS];  // deque lengths (min / max fields)
#pragma unroll
    for (int j = 0; j < SH_MAX_AGGS; j++) { f[j] = 0; dl[j] = 0; }
    u32 c = 0;
    u32 m_nx = idx[i];
    i64 ch_nx = chunk[m_nx];
    const bool closing = (i64)(skey[m_nx] >> 32) < (i64)nb;
    i64 kv[kKeyParts] = {0, 0};
    unpack_key(kp, slot_key(kt, pend_pos[m_nx]), kv, 1);
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
        if (closing && dq) {
#pragma unroll
            for (int j = 0; j < SH_MAX_AGGS; j++) {
                if (j >= ap.n_fields) break;
                if (fop_is_minmax(ap.fop[j]))
                    fop_dq_add(ap.fop[j], dq + (size_t)j * M + i, dl[j], pend_vals + (size_t)ap.fvcol[j] * pend_cap, m,
                              (u64)hvx_pick(v, ap.fvcol[j]));
            }
        }
        if (ch < 0 || !cur_on) continue;
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
        if ((t + 1 == hi || ch_nx != ch) && head >= 0) {
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
    if (!closing) return;
    // ---- the remove pass: every entry of the run, the earlier calls' included, in arrival order ----
    u32 dh[SH_MAX_AGGS];
#pragma unroll
    for (int j = 0; j < SH_MAX_AGGS; j++) dh[j] = 0;
    u32 fnull = 0;  // bit j: min / max field j has an empty deque
    u32 last_n = 0;
    head = -1;
    for (i64 t = i; t < hi; t++) {
        const u32 m = idx[t];
        i64 v[SH_MAX_AGGS];
#pragma unroll
        for (int j = 0; j < SH_MAX_AGGS; j++) v[j] = j < ap.n_vcols ? (i64)pend_vals[(size_t)j * pend_cap + m] : 0;
        c--;
#pragma unroll
        for (int j = 0; j < SH_MAX_AGGS; j++) {
            if (j >= ap.n_fields) break;
            const int op = ap.fop[j];
            const i64 x = hvx_pick(v, ap.fvcol[j]);
            if (!fop_is_minmax(op)) {
                f[j] = unfold_sum(op, f[j], x);
            } else {
                u64 front = 0;
                const bool has = fop_dq_remove(op, dq + (size_t)j * M + i, dh[j], dl[j],
                                              pend_vals + (size_t)ap.fvcol[j] * pend_cap, (u64)x, &front);
                f[j] = has ? front : 0;
                fnull = has ? fnull & ~(1u << j) : fnull | (1u << j);
            }
        }
        // the row's nulls: count never; min / max when the deque is empty; sum / avg at count 0
        u32 nm = 0;
#pragma unroll
        for (int a = 0; a < SH_MAX_AGGS; a++) {
            if (a >= ap.n) break;
            const int k = ap.kind[a];
            u32 fb = 0;
#pragma unroll
            for (int j = 0; j < SH_MAX_AGGS; j++) fb |= ap.field[a] == j ? (fnull >> j) & 1u : 0u;
            const bool nul = k == AK_COUNT ? false : k >= AK_MIN_L ? fb != 0 : c == 0;
            nm |= nul ? 1u << a : 0u;
        }
        if (hv_eval<HK>(hp, f, HvRow{kv[0], kv[1], c}, nm)) {
            if (head < 0) {
                head = m;
                xhead[m] = 1;
            }
            last_m = m;
            last_c = c;
            last_n = nm;
#pragma unroll
            for (int j = 0; j < SH_MAX_AGGS; j++) last_f[j] = f[j];
        }
    }
    xrun[idx[i]] = head >= 0 ? (u32)head : kNoHead;
    if (head < 0) return;
#pragma unroll
    for (int a = 0; a < SH_MAX_AGGS; a++) {
        if (a >= ap.n) break;
        u64 fv = last_f[0];
#pragma unroll
        for (int j = 1; j < SH_MAX_AGGS; j++) if (ap.field[a] == j) fv = last_f[j];
        const bool nul = (last_n >> a) & 1u;
        xval[(size_t)head * ap.n + a] = nul ? 0 : agg_out(ap, a, last_c, fv);
        xnul[(size_t)head * ap.n + a] = nul ? 1 : 0;
    }
    xlast[head] = last_m;
}

// lengthBatch(L, true): rows of every new entry's chunk. The event that starts batch w carries batch
// w - 1's passing expired heads; its own row, if it passes (ghead), takes its key's expired row's place
// (rank_e: that row's rank) or follows them (k_scx_count's join over passing heads instead of all keys).
__global__ __launch_bounds__(kBlock) void k_hvx_count(i64 M, i64 n_old, const i64* __restrict__ pcb,
                                                     const u64* __restrict__ skey, const u64* __restrict__ skey2,
                                                     const u32* __restrict__ idx2, const u32* __restrict__ xpre,
                                                     const u32* __restrict__ xrun, const u32* __restrict__ ghead,
                                                     u32* rows, i64* rank_e) {
    const i64 j = (i64)blockIdx.x * kBlock + threadIdx.x;
    const i64 m = n_old + j;
    if (m > M) return;
    if (m == M) { rows[j] = 0; return; }
    const u64 key = skey[m];
    const i64 w = (i64)(key >> 32);
    const bool cur = ghead[m] != 0;
    i64 re = -1;
    u32 r = cur ? 1u : 0u;
    if (w >= 1 && m == sc_wstart(w, n_old, pcb)) {
        const i64 ws0 = sc_wstart(w - 1, n_old, pcb);
        const i64 nprev = (i64)xpre[m] - (i64)xpre[ws0];
        if (cur) {
            const u64 want = ((u64)(w - 1) << 32) | (key & 0xFFFFFFFFull);
            i64 lo = 0, hi = M;
            while (lo < hi) {
                const i64 mid = (lo + hi) >> 1;
                if (skey2[mid] < want) lo = mid + 1; else hi = mid;
            }
            if (lo < M && skey2[lo] == want) {
                const u32 h = xrun[idx2[lo]];
                if (h != kNoHead) re = (i64)xpre[h] - (i64)xpre[ws0];
            }
        }
        r = (u32)nprev + ((cur && re < 0) ? 1u : 0u);
    }
    rows[j] = r;
    rank_e[j] = re;
}

// the expired rows, one per passing head. mode 0 lengthBatch: in the chunk of the event that starts the
// next batch, at that send's clock; 1 timeBatch: the TIMER chunk -(w + 1) at the window start's clock;
// 2 the open window closed by a TIMER alone: one flush at `now`
__global__ __launch_bounds__(kBlock) void k_hvx_expired(i64 M, i64 n_old, const i64* __restrict__ pcb,
                                                       const u64* __restrict__ skey, const u32* __restrict__ xhead,
                                                       const u32* __restrict__ xpre, const u32* __restrict__ xlast,
                                                       const u64* __restrict__ xval,
                                                       const unsigned char* __restrict__ xnul,
                                                       const u32* __restrict__ base, const i64* __restrict__ rank_e,
                                                       const i64* __restrict__ send, const i64* __restrict__ clk,
                                                       i64 now, const u32* __restrict__ pend_pos,
                                                       const u64* __restrict__ pend_gidx, KeyTable kt, KeyPlan kp, int na,
                                                       int mode, i64 T, i64* out_ts, i64* out_keys, u64* out_vals,
                                                       unsigned char* out_nulls, unsigned char* out_exp, i64* out_rep,
                                                       i64* out_chunk, i64* out_send) {
    const i64 m = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (m >= M || !xhead[m]) return;
    i64 o, ts;
    if (mode == 2) {
        o = xpre[m];
        ts = now;
    } else {
        const i64 w = (i64)(skey[m] >> 32);
        const i64 jb = pcb[w];  // the new entry that starts window w + 1 (timeBatch: may be past the last)
        const i64 rank = (i64)xpre[m] - (i64)xpre[sc_wstart(w, n_old, pcb)];
        if (mode == 0 && n_old + jb >= M) return;     // (a batch closes at the event that starts the next one)
        if (mode == 0 && rank == rank_e[jb]) return;  // the new event's current row takes this position
        o = base[jb] + rank;
        if (o < 0 || o >= T) return;
        ts = mode == 0 ? clk[send[n_old + jb]] : clk[w];
        out_chunk[o] = mode == 0 ? jb : -(w + 1);
        out_send[o] = mode == 0 ? send[n_old + jb] : -(w + 1);
    }
    if (o < 0 || o >= T) return;
    out_ts[o] = ts;
    out_rep[o] = (i64)pend_gidx[xlast[m]];
    i64 kv[kKeyParts] = {0, 0};
    unpack_key(kp, slot_key(kt, pend_pos[m]), kv, 1);
    for (int k = 0; k < kp.n; k++) out_keys[(size_t)k * T + o] = kv[k];
    for (int a = 0; a < na; a++) {
        out_vals[(size_t)a * T + o] = xval[(size_t)m * na + a];
        out_nulls[(size_t)a * T + o] = xnul[(size_t)m * na + a];
    }
    out_exp[o] = 1;
}

// lengthBatch(L, true): the current rows that pass (every new entry is its own chunk, so its own head)
__global__ __launch_bounds__(kBlock) void k_hvx_current(i64 M, i64 n_old, const i64* __restrict__ pcb,
                                                       const u64* __restrict__ skey, const u32* __restrict__ xpre,
                                                       const u32* __restrict__ ghead, const u32* __restrict__ base,
                                                       const i64* __restrict__ rank_e, const u64* __restrict__ sval,
                                                       const i64* __restrict__ send, const i64* __restrict__ pend_ts,
                                                       const u64* __restrict__ pend_gidx, KeyTable kt, KeyPlan kp, int na,
                                                       i64 T, i64* out_ts, i64* out_keys, u64* out_vals,
                                                       unsigned char* out_nulls, unsigned char* out_exp, i64* out_rep,
                                                       i64* out_chunk, i64* out_send) {
    const i64 j = (i64)blockIdx.x * kBlock + threadIdx.x;
    const i64 m = n_old + j;
    if (m >= M || !ghead[m]) return;
    const u64 key = skey[m];
    const i64 w = (i64)(key >> 32);
    i64 o = base[j];
    if (w >= 1 && m == sc_wstart(w, n_old, pcb)) {
        const i64 nprev = (i64)xpre[m] - (i64)xpre[sc_wstart(w - 1, n_old, pcb)];
        o += rank_e[j] >= 0 ? rank_e[j] : nprev;
    }
    if (o < 0 || o >= T) return;
    out_ts[o] = pend_ts[m];
    out_rep[o] = (i64)pend_gidx[m];
    i64 kv[kKeyParts] = {0, 0};
    unpack_key(kp, slot_key(kt, (u32)key), kv, 1);
    for (int k = 0; k < kp.n; k++) out_keys[(size_t)k * T + o] = kv[k];
    for (int a = 0; a < na; a++) {
        out_vals[(size_t)a * T + o] = sval[(size_t)m * na + a];
        out_nulls[(size_t)a * T + o] = 0;
    }
    out_exp[o] = 0;
    out_chunk[o] = j;
    out_send[o] = send[m];
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

void launch_hvx_walk(hipStream_t s, int kind, i64 M, const u32* pos, const u32* starts, const u32* idx, const i64* chunk,
                     const u64* skey, int nb, int cur_on, const u64* pend_vals, i64 pend_cap, const u32* pend_pos,
                     AggPlan ap, KeyTable kt, KeyPlan kp, HavingProg hp, u32* ghead, u64* sval, u32* slast, u32* xhead,
                     u64* xval, unsigned char* xnul, u32* xlast, u32* xrun, u32* dq) {
    if (M <= 0) return;
    const dim3 grid((unsigned)((M + kBlock - 1) / kBlock));
    if (kind == 1)
        hipLaunchKernelGGL(k_hvx_walk<1>, grid, dim3(kBlock), 0, s, M, pos, starts, idx, chunk, skey, nb, cur_on, pend_vals,
                           pend_cap, pend_pos, ap, kt, kp, hp, ghead, sval, slast, xhead, xval, xnul, xlast, xrun, dq);
    else
        hipLaunchKernelGGL(k_hvx_walk<2>, grid, dim3(kBlock), 0, s, M, pos, starts, idx, chunk, skey, nb, cur_on, pend_vals,
                           pend_cap, pend_pos, ap, kt, kp, hp, ghead, sval, slast, xhead, xval, xnul, xlast, xrun, dq);
}

void launch_hvx_count(hipStream_t s, i64 M, i64 n_old, const i64* pcb, const u64* skey, const u64* skey2, const u32* idx2,
                      const u32* xpre, const u32* xrun, const u32* ghead, u32* rows, i64* rank_e) {
    hipLaunchKernelGGL(k_hvx_count, dim3((unsigned)((M - n_old + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, M, n_old,
                       pcb, skey, skey2, idx2, xpre, xrun, ghead, rows, rank_e);
}

void launch_hvx_expired(hipStream_t s, i64 M, i64 n_old, const i64* pcb, const u64* skey, const u32* xhead,
                        const u32* xpre, const u32* xlast, const u64* xval, const unsigned char* xnul, const u32* base,
                        const i64* rank_e, const i64* send, const i64* clk, i64 now, const u32* pend_pos,
                        const u64* pend_gidx, KeyTable kt, KeyPlan kp, int na, int mode, i64 T, i64* out_ts, i64* out_keys,
                        u64* out_vals, unsigned char* out_nulls, unsigned char* out_exp, i64* out_rep, i64* out_chunk,
                        i64* out_send) {
    if (T <= 0 || M <= 0) return;
    hipLaunchKernelGGL(k_hvx_expired, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, M, n_old, pcb, skey,
                       xhead, xpre, xlast, xval, xnul, base, rank_e, send, clk, now, pend_pos, pend_gidx, kt, kp, na, mode,
                       T, out_ts, out_keys, out_vals, out_nulls, out_exp, out_rep, out_chunk, out_send);
}

void launch_hvx_current(hipStream_t s, i64 M, i64 n_old, const i64* pcb, const u64* skey, const u32* xpre,
                        const u32* ghead, const u32* base, const i64* rank_e, const u64* sval, const i64* send,
                        const i64* pend_ts, const u64* pend_gidx, KeyTable kt, KeyPlan kp, int na, i64 T, i64* out_ts,
                        i64* out_keys, u64* out_vals, unsigned char* out_nulls, unsigned char* out_exp, i64* out_rep,
                        i64* out_chunk, i64* out_send) {
    if (T <= 0 || M <= n_old) return;
    hipLaunchKernelGGL(k_hvx_current, dim3((unsigned)((M - n_old + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, M, n_old,
                       pcb, skey, xpre, ghead, base, rank_e, sval, send, pend_ts, pend_gidx, kt, kp, na, T, out_ts,
                       out_keys, out_vals, out_nulls, out_exp, out_rep, out_chunk, out_send);
}

}  // namespace shd
