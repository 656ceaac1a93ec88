// sh_having.h — the `having` condition of the batch group-by selector (sh_query_set_having).
//
// QuerySelector.processInBatchGroupBy (core/query/selector/QuerySelector.java:315-374, the test at
// :333-339) evaluates the condition after every event of a chunk, on the key's running aggregates, and
// keeps the event (groupedEvents.put) only when it holds: a key's row carries the values of its last
// passing event, sits at the position of its first passing event, and a key that never passes emits
// nothing (processInBatchNoGroupBy :271-313 likewise, with one implicit key). The program is therefore
// evaluated per event inside the (window, key) walk (sh_having_kernels.hip), never once per final row.
#pragma once

#include "sh_internal.h"

namespace shd {

// Having program (postfix), a kernel argument like FilterProg. An operand op's `type` is resolved by the
// compiler: SH_OP_KEY carries its group-by column's stream type, SH_OP_AGG the aggregate's output type
// and, on a live query, its fold field in `pad` and its AggKind in `ival` (-1: count has no field).
struct HavingProg {
    int n;
    int pad;
    FilterOpD ops[kMaxFilterOps];
};

inline bool having_operand(int op) { return op == SH_OP_KEY || op == SH_OP_AGG; }

// Which k_hv_walk instance evaluates a program (as filter_kind): 1 `agg|key <cmp> const` or two of those
// joined by AND / OR (registers only), 2 anything else (the stack machine).
inline int having_kind(const HavingProg& h) {
    auto leaf = [&](int i) {
        return having_operand(h.ops[i].op) && h.ops[i + 1].op == SH_OP_CONST && h.ops[i + 2].op >= SH_OP_GT &&
               h.ops[i + 2].op <= SH_OP_NE;
    };
    if (h.n == 3 && leaf(0)) return 1;
    if (h.n == 7 && leaf(0) && leaf(3) && (h.ops[6].op == SH_OP_AND || h.ops[6].op == SH_OP_OR)) return 1;
    return 2;
}

// (window, key slot) sort keys of the plain batch windows' closed segments: entry m of the pending
// buffer ([0, n_old) the open window's earlier events, then the push's passing events) lies in the
// segment holding its combined index; its chunk is that segment, its flush clock the segment's
// (send = -(segment + 1), k_sc_flushes' TIMER form). Entries past the last closed segment get chunk -1.
void launch_hv_keys(hipStream_t s, i64 M, i64 n_old, i64 seq0, const Segment* segs, int nseg, const u32* pend_pos,
                    const u64* pend_gidx, u64* skey, u32* idx, i64* chunk, i64* send);
// One thread per (window, key) run (k_sc_walk's layout): folds in event order, evaluates the program
// after every entry whose chunk is >= 0 and leaves k_sc_emit's contract — ghead at the first passing
// entry of each (chunk, key) group, slast / sval the last passing entry and its values.
void launch_hv_walk(hipStream_t s, int kind, i64 M, const u32* pos, const u32* starts, const u32* idx, const i64* chunk,
                    const u64* pend_vals, i64 pend_cap, const u32* pend_pos, AggPlan ap, KeyTable kt, KeyPlan kp,
                    HavingProg hp, u32* ghead, u64* sval, u32* slast);

// Expired / all-events output of lengthBatch(L, true) / timeBatch(T, true) (sh_stream_current.cpp sc_rows,
// sc_expire_pending). launch_hvx_walk is launch_hv_walk plus, for a run whose window closes in the call
// (its window index in skey's high word below nb), the ordered remove pass: xhead flags the entry of the
// run's first passing removal, xlast / xval / xnul (at that entry) give the last passing removal's entry,
// values and null flags, xrun (at the run's first sorted entry) the head's entry or 0xFFFFFFFF. The
// current role's flags are kept only with cur_on. dq: n_fields * M entry numbers, the min / max deques
// (NULL when the plan has no min or max). xhead must be zero on entry.
void launch_hvx_walk(hipStream_t s, int kind, i64 M, const u32* pos, const u32* starts, const u32* idx, const i64* chunk,
                     const u64* skey, int nb, int cur_on, const u64* pend_vals, i64 pend_cap, const u32* pend_pos,
                     AggPlan ap, KeyTable kt, KeyPlan kp, HavingProg hp, u32* ghead, u64* sval, u32* slast, u32* xhead,
                     u64* xval, unsigned char* xnul, u32* xlast, u32* xrun, u32* dq);
// lengthBatch: launch_scx_count's rows per chunk and key rank of a batch's first event, over passing heads
// (xpre: xhead scanned)
void launch_hvx_count(hipStream_t s, i64 M, i64 n_old, const i64* pcb, const u64* skey, const u64* skey2, const u32* idx2,
                      const u32* xpre, const u32* xrun, const u32* ghead, u32* rows, i64* rank_e);
// the expired rows of the passing heads. mode 0 lengthBatch (clk: the sends' clocks), 1 timeBatch (clk: the
// window starts' clocks), 2 one flush at `now` (row = xpre, no chunk columns)
void launch_hvx_expired(hipStream_t s, i64 M, i64 n_old, const i64* pcb, const u64* skey, const u32* xhead,
                        const u32* xpre, const u32* xlast, const u64* xval, const unsigned char* xnul, const u32* base,
                        const i64* rank_e, const i64* send, const i64* clk, i64 now, const u32* pend_pos,
                        const u64* pend_gidx, KeyTable kt, KeyPlan kp, int na, int mode, i64 T, i64* out_ts, i64* out_keys,
                        u64* out_vals, unsigned char* out_nulls, unsigned char* out_exp, i64* out_rep, i64* out_chunk,
                        i64* out_send);
// lengthBatch: the passing current rows (launch_scx_rows' current half over ghead)
void launch_hvx_current(hipStream_t s, i64 M, i64 n_old, const i64* pcb, const u64* skey, const u32* xpre,
                        const u32* ghead, const u32* base, const i64* rank_e, const u64* sval, const i64* send,
                        const i64* pend_ts, const u64* pend_gidx, KeyTable kt, KeyPlan kp, int na, i64 T, i64* out_ts,
                        i64* out_keys, u64* out_vals, unsigned char* out_nulls, unsigned char* out_exp, i64* out_rep,
                        i64* out_chunk, i64* out_send);

}  // namespace shd

// Per-query state: the compiled program (configuration, not state: snapshots neither store nor
// fingerprint it) and the instance picked for it.
struct HavingState {
    bool on = false;
    int kind = 0;
    shd::HavingProg prog{};
};

// The validation and type check behind sh_having_check and sh_query_set_having.
int having_compile(const sh_query_desc* d, const sh_filter_op* ops, int32_t n_ops, shd::HavingProg* out);
