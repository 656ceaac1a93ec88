// sh_stream_current.cpp — batch-window rows per event instead of per closed window: stream.current.event
// (sc_rows), the open window's keys as EXPIRED rows at a TIMER (sc_expire_pending), `having` (hv_closed).
// One pipeline over sh_window.cpp's pending entries (kernels: sh_kernels.hip k_sc_* / k_scx_*,
// sh_having_kernels.hip): key every entry by (window, key slot), sort, find the runs, walk them, count the
// rows, emit them, build the flushes. Each stage is written once; a caller keeps what only it does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sh_agg.h"
#include "sh_internal.h"
#include "sh_runtime.h"

using namespace shd;

#define HIPCHK(x)                                                                                          \
    do {                                                                                                   \
        hipError_t _e = (x);                                                                               \
        if (_e != hipSuccess) return sh_fail(SH_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define RCHK(x)            \
    do {                   \
        int _r = (x);      \
        if (_r) return _r; \
    } while (0)

// ---- the stages ----------------------------------------------------------------------------------------
// scratch of launch_scan_sum_large_u32 over n values
static size_t scan_tmp_bytes(int64_t n) { return (size_t)((n + kTile - 1) / kTile + 16) * 8; }

// Scratch per entry, M entries: the (window, slot) sort keys and entry indices before and after the sort,
// every entry's chunk and send, and the sorted runs (launch_rate_segments).
static int reserve_entries(sh_query* q, int64_t M) {
    for (DevBuf* d : {&q->sc_skey, &q->sc_skey2, &q->sc_chunk, &q->sc_send}) RCHK(d->reserve((size_t)M * 8, false));
    for (DevBuf* d : {&q->sc_idx, &q->sc_idx2}) RCHK(d->reserve((size_t)M * 4, false));
    for (DevBuf* d : {&q->sc_hd, &q->sc_pos, &q->sc_starts}) RCHK(d->reserve((size_t)(M + 1) * 4, false));
    return q->sc_tmp.reserve(scan_tmp_bytes(M + 1), false);
}

// ... and what a walk that folds the aggregates leaves per entry: the head flag of each (chunk, key)
// group and its scan, the group's last entry and the running values there.
static int reserve_walk(sh_query* q, int64_t M) {
    for (DevBuf* d : {&q->sc_ghead, &q->sc_pre}) RCHK(d->reserve((size_t)(M + 1) * 4, false));
    RCHK(q->sc_slast.reserve((size_t)M * 4, false));
    return q->sc_sval.reserve((size_t)std::max(q->ap.n, 1) * M * 8, false);
}

// The sorted keys are compared for equality alone, so the window index can sit right above the slot bits
// and the radix sort read those bits only: the sort's end bit for `n_slots` distinct slot values and
// window indices 0..n_windows, with the slot bits in *kb; 64 (the keys stay as they are) when the slot
// needs more than 32 bits or the two more than 48.
// This one loop gives what the two earlier ones gave for every table size up to 2^32 (pend_pos is a u32,
// so larger tables cannot occur). kb is the smallest k >= 1 with 2^k >= n_slots. stream.current passes
// the table size: its loop `kb < 32 && 2^kb < size` stopped at that same k, which is at most 32 for a
// size up to 2^32, so its cap never bound and the kb <= 32 test below never fails for it (once a key equal to
// EMPTY holds the reserved slot it passes the table size + 1, as `having` does). `having`
// passes the table size + 1: its loop `kb < 33 && 2^kb <= size` is this loop literally, and it kept the
// keys unpacked when kb reached 33 (a table of 2^32 slots), as the test below does.
static unsigned sort_end_bit(uint64_t n_slots, int64_t n_windows, unsigned* kb_out) {
    unsigned kb = 1, wb = 1;
    while (kb < 33 && ((uint64_t)1 << kb) < n_slots) kb++;
    while (wb < 31 && ((int64_t)1 << wb) <= n_windows) wb++;
    *kb_out = kb;
    return kb <= 32 && kb + wb <= 48 ? kb + wb : 64;
}

// the entry keys packed for that sort, where they fit; returns the sort's end bit
static unsigned pack_keys(sh_query* q, int64_t M, uint64_t n_slots, int64_t n_windows) {
    unsigned kb;
    const unsigned end_bit = sort_end_bit(n_slots, n_windows, &kb);
    if (end_bit < 64) launch_sc_pack_keys(q->ctx->stream, M, kb, q->sc_skey.as<u64>());
    return end_bit;
}

// The entries sorted by key bits [0, end_bit) (stable: a run keeps stream order) and the runs of equal
// keys: sc_skey2 / sc_idx2 sorted, sc_hd / sc_pos / sc_starts the runs.
static int sort_runs(sh_query* q, int64_t M, unsigned end_bit, const char* who) {
    hipStream_t s = q->ctx->stream;
    size_t tb = 0;
    if (sort_u64_pairs_bits(nullptr, &tb, nullptr, nullptr, nullptr, nullptr, M, end_bit, s))
        return sh_fail(SH_ERR_DEVICE, std::string(who) + ": sort sizing");
    RCHK(q->sc_sort.reserve(std::max<size_t>(tb, 16), false));
    if (sort_u64_pairs_bits(q->sc_sort.p, &tb, q->sc_skey.as<u64>(), q->sc_skey2.as<u64>(), q->sc_idx.as<u32>(),
                            q->sc_idx2.as<u32>(), M, end_bit, s))
        return sh_fail(SH_ERR_DEVICE, std::string(who) + ": sort failed");
    launch_rate_segments(s, M, q->sc_skey2.as<u64>(), q->sc_idx2.as<u32>(), 1, 0, q->sc_hd.as<u32>(),
                         q->sc_pos.as<u32>(), q->sc_starts.as<u32>(), q->sc_tmp.as<int64_t>());
    return SH_OK;
}

// v[0, n) scanned in place (inclusive sums; sc_tmp holds scan_tmp_bytes(n)) and its total read back:
// synchronises the stream.
static int scan_total(sh_query* q, u32* v, int64_t n, int64_t* total) {
    hipStream_t s = q->ctx->stream;
    launch_scan_sum_large_u32(s, v, n, q->sc_tmp.as<int64_t>());
    HIPCHK(hipGetLastError());
    RCHK(q->h_small_sc.reserve(64));
    HIPCHK(hipMemcpyAsync(q->h_small_sc.p, v + n - 1, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *total = *q->h_small_sc.as<uint32_t>();
    return SH_OK;
}

// rows in output order: the walk's head flags of entries [first, first + n) scanned into sc_pre
static int head_rows(sh_query* q, int64_t first, int64_t n, int64_t* T) {
    HIPCHK(hipMemcpyAsync(q->sc_pre.p, q->sc_ghead.as<uint32_t>() + first, (size_t)(n + 1) * 4, hipMemcpyDeviceToDevice,
                          q->ctx->stream));
    return scan_total(q, q->sc_pre.as<u32>(), n + 1, T);
}

// expired rows: every run's first entry flagged (scx_fe; scx_last its last entry), the flags copied to
// scx_fpre for the caller's scan
static int first_entries(sh_query* q, int64_t M) {
    hipStream_t s = q->ctx->stream;
    for (DevBuf* d : {&q->scx_fe, &q->scx_fpre}) RCHK(d->reserve((size_t)(M + 1) * 4, false));
    RCHK(q->scx_last.reserve((size_t)M * 4, false));
    HIPCHK(hipMemsetAsync(q->scx_fe.p, 0, (size_t)(M + 1) * 4, s));
    launch_scx_first(s, M, q->sc_hd.as<u32>(), q->sc_pos.as<u32>(), q->sc_starts.as<u32>(), q->sc_idx2.as<u32>(),
                     q->scx_fe.as<u32>(), q->scx_fpre.as<u32>(), q->scx_last.as<u32>());
    HIPCHK(hipMemcpyAsync(q->scx_fpre.p, q->scx_fe.p, (size_t)(M + 1) * 4, hipMemcpyDeviceToDevice, s));
    return SH_OK;
}

// n values — value(0) .. value(n - 1) — through pinned memory `h` into `d`. The caller knows that no copy
// out of or into `h` is in flight.
template <typename F>
static int upload_i64(sh_query* q, PinnedBuf& h, DevBuf& d, int n, F value) {
    RCHK(h.reserve((size_t)std::max(n, 1) * 8 + 64));
    RCHK(d.reserve((size_t)std::max(n, 1) * 8, false));
    for (int i = 0; i < n; i++) h.as<int64_t>()[i] = value(i);
    if (n) HIPCHK(hipMemcpyAsync(d.p, h.p, (size_t)n * 8, hipMemcpyHostToDevice, q->ctx->stream));
    return SH_OK;
}

static bool plan_has_minmax(const AggPlan& ap) {
    for (int j = 0; j < ap.n_fields; j++)
        if (ap.fop[j] >= FOP_MIN_I) return true;
    return false;
}

// Scratch of a having program's remove pass over M entries (k_hvx_walk): the passing heads (scx_fe,
// zeroed; scx_fpre for their scan; scx_last the last passing removal), each run's head, the rows' values
// and null flags, and — only for a plan with a min or max — the deques: a run of n entries needs at most
// n slots per field, at its own offset in the sorted order.
static int reserve_remove_pass(sh_query* q, int64_t M) {
    const size_t na = std::max(q->ap.n, 1);
    for (DevBuf* d : {&q->scx_fe, &q->scx_fpre}) RCHK(d->reserve((size_t)(M + 1) * 4, false));
    for (DevBuf* d : {&q->scx_last, &q->hvx_run}) RCHK(d->reserve((size_t)std::max<int64_t>(M, 1) * 4, false));
    RCHK(q->hvx_val.reserve(na * std::max<int64_t>(M, 1) * 8, false));
    RCHK(q->hvx_nul.reserve(na * std::max<int64_t>(M, 1), false));
    if (plan_has_minmax(q->ap)) RCHK(q->hvx_dq.reserve((size_t)q->ap.n_fields * std::max<int64_t>(M, 1) * 4, false));
    HIPCHK(hipMemsetAsync(q->scx_fe.p, 0, (size_t)(M + 1) * 4, q->ctx->stream));
    return SH_OK;
}

// One thread per run folds its entries in event order, timed between ev_agg0 and ev_agg1: the head flag of
// each (chunk, key) group among the entries from n_old on, its last entry and the running values there.
// A having program (sh_having.h) is evaluated after every entry: first / last passing entry per group.
// heads == false: every new entry is a chunk of its own, so a head, and no flags are kept.
// closing >= 0 (a program with expired output; reserve_remove_pass came first): the runs of the windows
// below `closing` close in this call and are walked a second time with the remove forms (k_hvx_walk).
static int walk_runs(sh_query* q, int64_t M, int64_t n_old, bool heads, int closing = -1) {
    hipStream_t s = q->ctx->stream;
    if (heads) HIPCHK(hipMemsetAsync(q->sc_ghead.p, 0, (size_t)(M + 1) * 4, s));
    HIPCHK(hipEventRecord(q->ev_agg0, s));
    if (q->hv.on && closing >= 0)
        launch_hvx_walk(s, q->hv.kind, M, q->sc_pos.as<u32>(), q->sc_starts.as<u32>(), q->sc_idx2.as<u32>(),
                        q->sc_chunk.as<int64_t>(), q->sc_skey.as<u64>(), closing, q->d.current_on ? 1 : 0,
                        q->pend_vals.as<u64>(), q->pend_cap, q->pend_pos.as<u32>(), q->ap, q->kt.dev(), q->kp, q->hv.prog,
                        q->sc_ghead.as<u32>(), q->sc_sval.as<u64>(), q->sc_slast.as<u32>(), q->scx_fe.as<u32>(),
                        q->hvx_val.as<u64>(), q->hvx_nul.as<unsigned char>(), q->scx_last.as<u32>(), q->hvx_run.as<u32>(),
                        plan_has_minmax(q->ap) ? q->hvx_dq.as<u32>() : nullptr);
    else if (q->hv.on)
        launch_hv_walk(s, q->hv.kind, M, q->sc_pos.as<u32>(), q->sc_starts.as<u32>(), q->sc_idx2.as<u32>(),
                       q->sc_chunk.as<int64_t>(), q->pend_vals.as<u64>(), q->pend_cap, q->pend_pos.as<u32>(), q->ap,
                       q->kt.dev(), q->kp, q->hv.prog, q->sc_ghead.as<u32>(), q->sc_sval.as<u64>(), q->sc_slast.as<u32>());
    else
        launch_sc_walk(s, M, q->sc_hd.as<u32>(), q->sc_pos.as<u32>(), q->sc_starts.as<u32>(), q->sc_idx2.as<u32>(),
                       q->sc_chunk.as<int64_t>(), q->pend_vals.as<u64>(), q->pend_cap, q->ap, n_old,
                       heads ? q->sc_ghead.as<u32>() : nullptr, q->sc_sval.as<u64>(), q->sc_slast.as<u32>());
    HIPCHK(hipEventRecord(q->ev_agg1, s));
    return SH_OK;
}

// the walk's device time into the call's statistics; after a synchronisation
static void add_walk_ms(sh_query* q) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, q->ev_agg0, q->ev_agg1);
    q->stats.main_kernel_ms += ms;
}

// Output columns for T rows (for one at least: sh_out's pointers are never NULL). The row kernel writes
// every byte of the flag columns, so they are not known to be zero afterwards.
static int reserve_out_rows(sh_query* q, int64_t T) {
    const int64_t TC = std::max<int64_t>(T, 1);
    const size_t nk = std::max(1, q->kp.n), na = std::max(1, q->ap.n);
    RCHK(q->out_ts.reserve(TC * 8, false));
    RCHK(q->out_keys.reserve(nk * TC * 8, false));
    RCHK(q->out_vals.reserve(na * TC * 8, false));
    RCHK(q->out_nulls.reserve(na * TC, false));
    RCHK(q->out_expired.reserve(TC, false));
    RCHK(q->out_rep.reserve(TC * 8, false));
    q->zeroed_nulls = nullptr;
    q->zeroed_expired = nullptr;
    return SH_OK;
}

// ... for rows that also carry their chunk and send (what their flushes are built from), and whose
// kernels only ever set flags: the null and expired columns are zeroed here
static int reserve_chunk_rows(sh_query* q, int64_t T) {
    hipStream_t s = q->ctx->stream;
    RCHK(reserve_out_rows(q, T));
    for (DevBuf* d : {&q->sc_ochunk, &q->sc_osend}) RCHK(d->reserve((size_t)std::max<int64_t>(T, 1) * 8, false));
    HIPCHK(hipMemsetAsync(q->out_nulls.p, 0, q->out_nulls.cap, s));
    HIPCHK(hipMemsetAsync(q->out_expired.p, 0, q->out_expired.cap, s));
    q->zeroed_nulls = q->out_nulls.p;
    q->zeroed_expired = q->out_expired.p;
    return SH_OK;
}

// CURRENT rows of the walk: one per flagged head among the entries from n_old on (heads == false: every one
// of them is a row, and no row carries a chunk), with the values at its group's last entry
static void emit_rows(sh_query* q, int64_t M, int64_t n_old, bool heads, int64_t T) {
    launch_sc_emit(q->ctx->stream, M, n_old, heads ? q->sc_ghead.as<u32>() : nullptr, q->sc_pre.as<u32>(),
                   q->sc_slast.as<u32>(), q->sc_sval.as<u64>(), q->pend_pos.as<u32>(), q->pend_ts.as<int64_t>(),
                   q->pend_gidx.as<u64>(), q->sc_chunk.as<int64_t>(), q->sc_send.as<int64_t>(), q->kt.dev(), q->kp,
                   q->ap.n, T, q->out_ts.as<int64_t>(), q->out_keys.as<int64_t>(), q->out_vals.as<u64>(),
                   q->out_rep.as<int64_t>(), heads ? q->sc_ochunk.as<int64_t>() : nullptr, q->sc_osend.as<int64_t>(),
                   q->given ? q->out_order.as<int64_t>() : nullptr);
}

// a flush ends where the row's chunk changes: the flags (sc_fflag, scanned) and the number of flushes
static int flush_count(sh_query* q, int64_t T, int64_t* nf) {
    RCHK(q->sc_fflag.reserve((size_t)(T + 1) * 4, false));
    RCHK(q->sc_tmp.reserve(scan_tmp_bytes(T + 1), false));
    launch_sc_flush_flags(q->ctx->stream, T, q->sc_ochunk.as<int64_t>(), q->sc_fflag.as<u32>());
    return scan_total(q, q->sc_fflag.as<u32>(), T + 1, nf);
}

// The nf flushes' offsets and clocks on the device (sc_fo / sc_fc). flags: the scanned flush flags, NULL
// for a flush per row. A row of send j >= 0 takes that send's clock (send_clk: the running maximum over
// the sends, continued from clock0 if cv0), a row of a window's TIMER chunk that window's (sc_bclk).
static int build_flushes(sh_query* q, int64_t T, int64_t nf, const u32* flags, const int64_t* send_clk, bool cv0,
                         int64_t clock0) {
    RCHK(q->sc_fo.reserve((size_t)std::max<int64_t>(nf, 1) * 8, false));
    RCHK(q->sc_fc.reserve((size_t)std::max<int64_t>(nf, 1) * 8, false));
    launch_sc_flushes(q->ctx->stream, T, q->sc_osend.as<int64_t>(), flags, send_clk, cv0 ? 1 : 0, clock0,
                      q->sc_bclk.as<int64_t>(), q->sc_fo.as<int64_t>(), q->sc_fc.as<int64_t>());
    HIPCHK(hipGetLastError());
    return SH_OK;
}

// ... and into the call's flush vectors (queued: complete after the caller's next synchronisation)
static int flushes_to_host(sh_query* q, int64_t nf, const FlushVecs& fl) {
    hipStream_t s = q->ctx->stream;
    fl.offsets.resize((size_t)nf + 1);
    fl.clocks.resize((size_t)nf);
    if (nf) {
        HIPCHK(hipMemcpyAsync(fl.offsets.data() + 1, q->sc_fo.p, (size_t)nf * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(fl.clocks.data(), q->sc_fc.p, (size_t)nf * 8, hipMemcpyDeviceToHost, s));
    }
    return SH_OK;
}

// The call's T rows as its output: device output names the out_* columns as they are; host output copies
// them and synchronises. flags_zero: the rows are CURRENT events that always have a value (`having`
// rows), so the host's flag arrays are filled here instead of copied.
static int rows_out(sh_query* q, int64_t T, bool host_out, bool flags_zero) {
    if (!host_out) {
        q->dev_out.n_rows = T;
        return SH_OK;
    }
    hipStream_t s = q->ctx->stream;
    const size_t nk = q->kp.n, na = q->ap.n;
    OutHost& o = q->out;
    o.ts.resize(T);
    o.rep.resize(T);
    o.keys.resize(nk * T);
    o.vals.resize(na * T);
    if (flags_zero) {
        o.expired.assign(T, 0);
        o.nulls.assign(na * T, 0);
    } else {
        o.expired.resize(T);
        o.nulls.resize(na * T);
    }
    if (T == 0) return SH_OK;
    if (!flags_zero) {
        HIPCHK(hipMemcpyAsync(o.expired.data(), q->out_expired.p, T, hipMemcpyDeviceToHost, s));
        if (na) HIPCHK(hipMemcpyAsync(o.nulls.data(), q->out_nulls.p, na * T, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(o.ts.data(), q->out_ts.p, T * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(o.rep.data(), q->out_rep.p, T * 8, hipMemcpyDeviceToHost, s));
    if (nk) HIPCHK(hipMemcpyAsync(o.keys.data(), q->out_keys.p, nk * T * 8, hipMemcpyDeviceToHost, s));
    if (na) HIPCHK(hipMemcpyAsync(o.vals.data(), q->out_vals.p, na * T * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SH_OK;
}

// ---- the three pipelines -------------------------------------------------------------------------------
// `having` on the plain batch windows (sh_having.h; QuerySelector.processInBatchGroupBy :315-374 keeps an
// event only when the condition holds on the key's running aggregates): the stream.current.event
// machinery with the chunk redefined — a row's chunk is its closed window, its flush clock that window's.
// The push's passing events join the pending entries, the entries are sorted by (window, key slot), one
// thread walks each run evaluating the program per event (k_hv_walk), and k_sc_emit / k_sc_flush_flags /
// k_sc_flushes build rows and flushes: a window that keeps no row gives no flush. Synchronous: the rows
// (device, or host for host_out) and the flush arrays (host) are complete on return.
int hv_closed(sh_query* q, const std::vector<Segment>& segs, const std::vector<int64_t>& clocks, const sh_batch* b,
              bool host_out) {
    hipStream_t s = q->ctx->stream;
    const int na = q->ap.n, nseg = (int)segs.size();
    const int64_t n_old = q->n_pend;
    const int64_t M = n_old + (b ? q->h_info->total_pass : 0);
    const FlushVecs fl = flush_vecs(q, host_out);
    if (fl.offsets.size() != 1) return sh_fail(SH_ERR_INVALID, "having: output appended twice in one call");
    if (M <= 0) return SH_OK;
    if (b && M > n_old) RCHK(append_pending(q, b, n_old, M));
    RCHK(upload_segments(q, segs));
    RCHK(upload_i64(q, q->sc_h, q->sc_bclk, nseg, [&](int i) { return clocks[i]; }));
    RCHK(reserve_entries(q, M));
    RCHK(reserve_walk(q, M));
    launch_hv_keys(s, M, n_old, q->seq, q->segs.as<Segment>(), nseg, q->pend_pos.as<u32>(), q->pend_gidx.as<u64>(),
                   q->sc_skey.as<u64>(), q->sc_idx.as<u32>(), q->sc_chunk.as<int64_t>(), q->sc_send.as<int64_t>());
    // slot values: the table's and the sentinel key's (mask + 1); window indices: nseg is the window staying open
    const unsigned end_bit = pack_keys(q, M, (uint64_t)q->kt.size_ + 1, nseg);
    RCHK(sort_runs(q, M, end_bit, "having"));
    RCHK(walk_runs(q, M, 0, true));
    // the heads scanned over every entry (a closed window's queued entries emit too)
    int64_t T = 0;
    RCHK(head_rows(q, 0, M, &T));
    add_walk_ms(q);
    q->agg_bytes += M * (int64_t)(4 + 8 + 8 * q->ap.n_vcols) + T * (int64_t)(4 + 8 * na);
    RCHK(reserve_chunk_rows(q, T));
    if (T > 0) {
        emit_rows(q, M, 0, true, T);
        // a flush ends where the row's window changes; its clock is the window's
        int64_t nf = 0;
        RCHK(flush_count(q, T, &nf));
        RCHK(build_flushes(q, T, nf, q->sc_fflag.as<u32>(), nullptr, false, 0));
        RCHK(flushes_to_host(q, nf, fl));
    }
    RCHK(rows_out(q, T, host_out, true));
    HIPCHK(hipStreamSynchronize(s));
    return SH_OK;
}

// stream.current.event batch windows (LengthBatchWindowProcessor.processStreamCurrentEvents :245-274,
// TimeBatchWindowProcessor RESET mode :262-340): the pending entries [0, n_old) are the open window's
// earlier events, [n_old, M) this push's passing events (sh_kernels.hip k_sc_*). One flush per chunk:
// every passing event for lengthBatch (:160-182 sends each event's chunk on its own), every send with
// passing events for timeBatch; the flush clock is the send's playback clock.
int sc_rows(sh_query* q, const sh_batch* b, const std::vector<Bound>& bounds, int64_t n_old, int64_t M, bool cv0,
            int64_t clock0, int64_t seq0, bool host_out) {
    hipStream_t s = q->ctx->stream;
    const int nb = (int)bounds.size();
    const bool per_event = q->d.window == SH_WIN_LENGTH_BATCH;
    const int64_t N = b->n, ss = b->send_size;
    const int64_t n_sends = ss > 0 ? (N + ss - 1) / ss : 1;
    RCHK(upload_i64(q, q->sc_hp, q->sc_pcb, nb, [&](int i) { return bounds[i].pcb; }));
    auto bound_clock = [&](int i) { return bounds[i].clock; };  // the clock of each window start
    RCHK(reserve_entries(q, M));
    RCHK(reserve_walk(q, M));
    RCHK(q->sc_sl.reserve((size_t)n_sends * 8, false));
    // (a sharded owner: records are one send each for their clocks, chunks are the global sends)
    const bool gv = q->given_clk != nullptr;
    const bool xs = q->d.expired_on && per_event;   // lengthBatch(L, true) with expired / all events
    const bool xt = q->d.expired_on && !per_event;  // timeBatch(T, true) with expired / all events
    // every new entry its own chunk (per-event sends, lengthBatch(L, true)): each is its own row, no head
    // flags, no scan of them, no chunk column and no read-back of the row count (current rows only)
    // (a having program: a chunk's rows are the entries that pass, so the heads are always flagged and scanned)
    const bool hv = q->hv.on;
    const bool all_heads = !hv && !(xs || xt) && (per_event || (gv ? q->given_ss : ss) == 1);
    launch_sc_keys(s, M, n_old, q->sc_pcb.as<int64_t>(), nb, q->pend_pos.as<u32>(), q->pend_gidx.as<u64>(),
                   per_event ? 1 : 0, gv ? q->given_ss : ss, gv ? q->given_seq0 : seq0, q->sc_skey.as<u64>(),
                   q->sc_idx.as<u32>(), all_heads ? nullptr : q->sc_chunk.as<int64_t>(), q->sc_send.as<int64_t>(),
                   gv ? 1 : 0);
    // current rows only: the radix sort reads the slot and window bits alone (C2: 24 of 64); the expired
    // rows' kernels read the keys whole
    // (the reserved slot mask + 1 takes one more slot bit, which may be one more sort pass: counted only once
    // a key equal to EMPTY has been looked up: the table's control words say so, read back at the end of
    // every push and, for this push's own lookups, beside the push info — sh_window.cpp)
    const bool rsv = q->kt.reserved_used;
    const unsigned end_bit = xs || xt ? 64 : pack_keys(q, M, (uint64_t)q->kt.size_ + (rsv ? 1 : 0), nb);
    RCHK(sort_runs(q, M, end_bit, "stream.current"));
    // (a program with expired output: the closing windows' runs are walked again with the remove forms, and
    // the expired rows are those of the passing heads — scx_fe — instead of every key of a closing window)
    const bool hvx = hv && (xs || xt);
    if (hvx) RCHK(reserve_remove_pass(q, M));
    RCHK(walk_runs(q, M, n_old, !all_heads, hvx ? nb : -1));
    const int64_t nn = M - n_old;
    // the sends' playback clocks: TimestampGeneratorImpl only moves forward (prefix max of send-last ts);
    // a sharded owner's records (one send each) carry their global send's clock instead
    if (q->given_clk) {
        if (ss != 1) return sh_fail(SH_ERR_INVALID, "sharded stream.current: records are one send each");
        cv0 = false;  // (the records' clocks are whole; the owner's clock is already the push's end clock)
        HIPCHK(hipMemcpyAsync(q->sc_sl.p, q->given_clk, (size_t)N * 8, hipMemcpyDeviceToDevice, s));
    } else {
        launch_sc_send_last(s, b->ts, N, ss, n_sends, q->sc_sl.as<int64_t>());
    }
    HIPCHK(hipGetLastError());
    // (host scratch kept by the query: a fresh 8-byte-per-send vector per push faulted in its pages —
    // hundreds of MB per C2-sized push)
    std::vector<int64_t>& sl = q->sc_sl_host;
    if (xs || xt) {
        RCHK(q->sc_h.reserve((size_t)n_sends * 8 + 64));
        HIPCHK(hipMemcpyAsync(q->sc_h.p, q->sc_sl.p, (size_t)n_sends * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        sl.resize((size_t)n_sends);
        const int64_t* hs = q->sc_h.as<int64_t>();
        bool cv = cv0;
        int64_t c = clock0;
        for (int64_t i = 0; i < n_sends; i++) {
            c = cv ? std::max(c, hs[i]) : hs[i];
            cv = true;
            sl[i] = c;
        }
    } else {
        // current rows only: the sends' clocks stay on the device (the flushes are built there too)
        size_t stb = 0;
        RCHK(q->sc_slp.reserve((size_t)n_sends * 8, false));
        if (scan_max_i64(nullptr, &stb, q->sc_sl.as<int64_t>(), q->sc_slp.as<int64_t>(), n_sends, s))
            return sh_fail(SH_ERR_DEVICE, "stream.current: scan sizing");
        RCHK(q->sc_sort.reserve(std::max<size_t>(stb, 16), false));
        if (scan_max_i64(q->sc_sort.p, &stb, q->sc_sl.as<int64_t>(), q->sc_slp.as<int64_t>(), n_sends, s))
            return sh_fail(SH_ERR_DEVICE, "stream.current: scan failed");
    }
    const int cur_on = q->d.current_on ? 1 : 0;
    int64_t T = 0;
    if (xs || xt) {
        RCHK(q->scx_rows.reserve((size_t)(nn + 2) * 4, false));
        RCHK(q->scx_rank.reserve((size_t)std::max<int64_t>(nn, 1) * 8, false));
        RCHK(q->scx_clk.reserve((size_t)n_sends * 8, false));
        if (hvx)
            HIPCHK(hipMemcpyAsync(q->scx_fpre.p, q->scx_fe.p, (size_t)(M + 1) * 4, hipMemcpyDeviceToDevice, s));
        else
            RCHK(first_entries(q, M));
        launch_scan_sum_large_u32(s, q->scx_fpre.as<u32>(), M + 1, q->sc_tmp.as<int64_t>());
        if (xs && hvx)
            launch_hvx_count(s, M, n_old, q->sc_pcb.as<int64_t>(), q->sc_skey.as<u64>(), q->sc_skey2.as<u64>(),
                             q->sc_idx2.as<u32>(), q->scx_fpre.as<u32>(), q->hvx_run.as<u32>(), q->sc_ghead.as<u32>(),
                             q->scx_rows.as<u32>(), q->scx_rank.as<int64_t>());
        else if (xs)
            launch_scx_count(s, M, n_old, q->sc_pcb.as<int64_t>(), q->sc_skey.as<u64>(), q->sc_skey2.as<u64>(),
                             q->sc_idx2.as<u32>(), q->scx_fpre.as<u32>(), cur_on, 1, q->scx_rows.as<u32>(),
                             q->scx_rank.as<int64_t>());
        else
            launch_scxt_count(s, M, n_old, q->sc_pcb.as<int64_t>(), nb, q->sc_skey.as<u64>(), q->scx_fpre.as<u32>(),
                              q->sc_ghead.as<u32>(), cur_on, q->scx_rows.as<u32>());
        // the rows' clocks go up ahead of the row count's read-back: sc_h was last the landing area of the
        // sends' clocks, synchronised above, and is not written again before scan_total's synchronisation
        if (xs) {
            std::memcpy(q->sc_h.p, sl.data(), (size_t)n_sends * 8);
            HIPCHK(hipMemcpyAsync(q->scx_clk.p, q->sc_h.p, (size_t)n_sends * 8, hipMemcpyHostToDevice, s));
        } else {  // timeBatch: the clock of each window start (the TIMER chunk's clock)
            RCHK(upload_i64(q, q->sc_h, q->scx_clk, nb, bound_clock));
        }
        const int64_t nr = xs ? nn + 1 : nn + 2;  // (timeBatch: rows[nn] = windows closing after the last entry)
        RCHK(scan_total(q, q->scx_rows.as<u32>(), nr, &T));
    } else if (all_heads) {
        T = nn;
    } else {
        RCHK(head_rows(q, n_old, nn, &T));
    }
    RCHK(reserve_chunk_rows(q, T));
    if (q->given) RCHK(q->out_order.reserve((size_t)std::max<int64_t>(T, 1) * 8, false));
    if (hvx) {
        // the expired rows of the passing heads, with their values and nulls; the current rows that pass
        launch_hvx_expired(s, M, n_old, q->sc_pcb.as<int64_t>(), q->sc_skey.as<u64>(), q->scx_fe.as<u32>(),
                           q->scx_fpre.as<u32>(), q->scx_last.as<u32>(), q->hvx_val.as<u64>(),
                           q->hvx_nul.as<unsigned char>(), q->scx_rows.as<u32>(), q->scx_rank.as<int64_t>(),
                           q->sc_send.as<int64_t>(), q->scx_clk.as<int64_t>(), 0, q->pend_pos.as<u32>(),
                           q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap.n, xs ? 0 : 1, T, q->out_ts.as<int64_t>(),
                           q->out_keys.as<int64_t>(), q->out_vals.as<u64>(), q->out_nulls.as<unsigned char>(),
                           q->out_expired.as<unsigned char>(), q->out_rep.as<int64_t>(), q->sc_ochunk.as<int64_t>(),
                           q->sc_osend.as<int64_t>());
        if (cur_on && xs)
            launch_hvx_current(s, M, n_old, q->sc_pcb.as<int64_t>(), q->sc_skey.as<u64>(), q->scx_fpre.as<u32>(),
                               q->sc_ghead.as<u32>(), q->scx_rows.as<u32>(), q->scx_rank.as<int64_t>(),
                               q->sc_sval.as<u64>(), q->sc_send.as<int64_t>(), q->pend_ts.as<int64_t>(),
                               q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap.n, T, q->out_ts.as<int64_t>(),
                               q->out_keys.as<int64_t>(), q->out_vals.as<u64>(), q->out_nulls.as<unsigned char>(),
                               q->out_expired.as<unsigned char>(), q->out_rep.as<int64_t>(),
                               q->sc_ochunk.as<int64_t>(), q->sc_osend.as<int64_t>());
        else if (cur_on)
            launch_scxt_current(s, M, n_old, q->sc_pcb.as<int64_t>(), nb, q->sc_skey.as<u64>(), q->scx_fpre.as<u32>(),
                                q->sc_ghead.as<u32>(), q->scx_rows.as<u32>(), q->sc_slast.as<u32>(), q->sc_sval.as<u64>(),
                                q->sc_chunk.as<int64_t>(), q->sc_send.as<int64_t>(), q->pend_ts.as<int64_t>(),
                                q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap.n, T, q->out_ts.as<int64_t>(),
                                q->out_keys.as<int64_t>(), q->out_vals.as<u64>(), q->out_nulls.as<unsigned char>(),
                                q->out_expired.as<unsigned char>(), q->out_rep.as<int64_t>(),
                                q->sc_ochunk.as<int64_t>(), q->sc_osend.as<int64_t>());
    } else if (xs) {
        launch_scx_rows(s, M, n_old, q->sc_pcb.as<int64_t>(), nb, q->sc_skey.as<u64>(), q->scx_fe.as<u32>(),
                        q->scx_fpre.as<u32>(), q->scx_last.as<u32>(), q->scx_rows.as<u32>(), q->scx_rank.as<int64_t>(),
                        q->sc_sval.as<u64>(), q->sc_send.as<int64_t>(), q->scx_clk.as<int64_t>(),
                        q->pend_ts.as<int64_t>(), q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap, cur_on, 1, T,
                        q->out_ts.as<int64_t>(), q->out_keys.as<int64_t>(), q->out_vals.as<u64>(),
                        q->out_nulls.as<unsigned char>(), q->out_expired.as<unsigned char>(), q->out_rep.as<int64_t>(),
                        q->sc_ochunk.as<int64_t>(), q->sc_osend.as<int64_t>());
    } else if (xt) {
        launch_scxt_rows(s, M, n_old, q->sc_pcb.as<int64_t>(), nb, q->sc_skey.as<u64>(), q->scx_fe.as<u32>(),
                         q->scx_fpre.as<u32>(), q->scx_last.as<u32>(), q->sc_ghead.as<u32>(), q->scx_rows.as<u32>(),
                         q->sc_slast.as<u32>(), q->sc_sval.as<u64>(), q->sc_chunk.as<int64_t>(),
                         q->sc_send.as<int64_t>(), q->scx_clk.as<int64_t>(), q->pend_ts.as<int64_t>(),
                         q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap, cur_on, T, q->out_ts.as<int64_t>(),
                         q->out_keys.as<int64_t>(), q->out_vals.as<u64>(), q->out_nulls.as<unsigned char>(),
                         q->out_expired.as<unsigned char>(), q->out_rep.as<int64_t>(), q->sc_ochunk.as<int64_t>(),
                         q->sc_osend.as<int64_t>());
    } else {
        emit_rows(q, M, n_old, !all_heads, T);
    }
    HIPCHK(hipGetLastError());
    const FlushVecs fl = flush_vecs(q, host_out);
    fl.offsets.assign(1, 0);
    fl.clocks.clear();
    if (!(xs || xt)) {
        // current rows: the flushes are built on the device — a flush ends where the row's chunk changes
        RCHK(upload_i64(q, q->sc_h, q->sc_bclk, nb, bound_clock));
        RCHK(q->h_small_sc.reserve(64));
        int64_t nf = T;  // (every row its own chunk: a flush per row, no flags to scan)
        if (!all_heads) RCHK(flush_count(q, T, &nf));
        const u32* flags = all_heads ? nullptr : q->sc_fflag.as<u32>();
        q->compact_now = false;
        const bool want_compact = q->compact_flushes && q->rate.kind == SH_RATE_NONE && !q->xmode && !hv && nf > 0 && nf == T;
        if (all_heads && want_compact) {
            // (a flush per row: check the rows' clocks against their timestamps before writing any flush)
            launch_sc_clock_is_ts(s, T, q->sc_osend.as<int64_t>(), q->sc_slp.as<int64_t>(), cv0 ? 1 : 0, clock0,
                                  q->out_ts.as<int64_t>(), q->h_small_sc.as<uint32_t>() + 1);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));
            q->compact_now = q->h_small_sc.as<uint32_t>()[1] == 1u;
        }
        if (!q->compact_now) RCHK(build_flushes(q, T, nf, flags, q->sc_slp.as<int64_t>(), cv0, clock0));
        if (!all_heads && want_compact) {
            // one row per flush: offsets implicit; clocks implicit too when each equals its row's ts
            launch_flush_clock_is_ts(s, nf, q->sc_fc.as<int64_t>(), q->out_ts.as<int64_t>(), q->h_small_sc.as<uint32_t>() + 1);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));
            q->compact_now = q->h_small_sc.as<uint32_t>()[1] == 1u;
        }
        if (!q->compact_now) RCHK(flushes_to_host(q, nf, fl));
        HIPCHK(hipStreamSynchronize(s));
    } else if (T > 0) {
        // expired / all events: the flushes are built here from every row's chunk and send — a row of send
        // j >= 0 goes out at that send's clock, a row of a TIMER chunk at its window start's
        RCHK(q->sc_ho.reserve((size_t)2 * T * 8 + 64));
        int64_t* och = q->sc_ho.as<int64_t>();  // read in place from the pinned landing area
        int64_t* osd = och + T;
        HIPCHK(hipMemcpyAsync(och, q->sc_ochunk.p, (size_t)T * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(osd, q->sc_osend.p, (size_t)T * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        fl.offsets.reserve((size_t)T + 1);  // (one pinned allocation, not a doubling series)
        fl.clocks.reserve((size_t)T);
        for (int64_t i = 0; i < T; i++) {
            if (i + 1 == T || och[i + 1] != och[i]) {
                fl.offsets.push_back(i + 1);
                fl.clocks.push_back(osd[i] >= 0 ? sl[osd[i]] : bounds[-osd[i] - 1].clock);
            }
        }
    }
    add_walk_ms(q);
    RCHK(rows_out(q, T, host_out, false));
    // sharded owner: a row's merge order is the global stream index of its group's first event in the chunk
    if (host_out && q->given) {
        q->order_host.resize(T);
        if (T) HIPCHK(hipMemcpyAsync(q->order_host.data(), q->out_order.p, T * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return SH_OK;
}

// timeBatch(T, true) with expired output: the open window closed by a TIMER without events
// (sh_advance_time): one flush of its keys' EXPIRED rows (empty state) at clock `now`
int sc_expire_pending(sh_query* q, int64_t now, bool host_out) {
    hipStream_t s = q->ctx->stream;
    const int64_t M = q->n_pend;
    RCHK(reserve_entries(q, M));
    RCHK(q->sc_pcb.reserve(8, false));
    launch_sc_keys(s, M, M, q->sc_pcb.as<int64_t>(), 0, q->pend_pos.as<u32>(), q->pend_gidx.as<u64>(), 0, 0, 0,
                   q->sc_skey.as<u64>(), q->sc_idx.as<u32>(), q->sc_chunk.as<int64_t>(), q->sc_send.as<int64_t>());
    RCHK(sort_runs(q, M, 64, "stream.current"));
    int64_t T = 0;
    if (q->hv.on) {
        // a program: every run folds (no entry is of this call, so none is tested as CURRENT), then the
        // remove pass; the rows are the passing heads', in arrival order
        RCHK(reserve_walk(q, M));
        RCHK(reserve_remove_pass(q, M));
        RCHK(walk_runs(q, M, M, true, 1));
        HIPCHK(hipMemcpyAsync(q->scx_fpre.p, q->scx_fe.p, (size_t)(M + 1) * 4, hipMemcpyDeviceToDevice, s));
        RCHK(scan_total(q, q->scx_fpre.as<u32>(), M + 1, &T));
        add_walk_ms(q);
        RCHK(reserve_out_rows(q, T));
        launch_hvx_expired(s, M, M, nullptr, nullptr, q->scx_fe.as<u32>(), q->scx_fpre.as<u32>(), q->scx_last.as<u32>(),
                           q->hvx_val.as<u64>(), q->hvx_nul.as<unsigned char>(), nullptr, nullptr, nullptr, nullptr, now,
                           q->pend_pos.as<u32>(), q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap.n, 2, T,
                           q->out_ts.as<int64_t>(), q->out_keys.as<int64_t>(), q->out_vals.as<u64>(),
                           q->out_nulls.as<unsigned char>(), q->out_expired.as<unsigned char>(), q->out_rep.as<int64_t>(),
                           nullptr, nullptr);
        HIPCHK(hipGetLastError());
        const FlushVecs fl = flush_vecs(q, host_out);
        fl.offsets.assign(1, 0);
        fl.clocks.clear();
        if (T) {
            fl.offsets.push_back(T);
            fl.clocks.push_back(now);
        }
        return rows_out(q, T, host_out, false);
    }
    RCHK(first_entries(q, M));
    RCHK(scan_total(q, q->scx_fpre.as<u32>(), M + 1, &T));
    RCHK(reserve_out_rows(q, T));
    launch_scx_pending_rows(s, M, q->scx_fe.as<u32>(), q->scx_fpre.as<u32>(), q->scx_last.as<u32>(),
                            q->pend_pos.as<u32>(), q->pend_gidx.as<u64>(), q->kt.dev(), q->kp, q->ap, now, T,
                            q->out_ts.as<int64_t>(), q->out_keys.as<int64_t>(), q->out_vals.as<u64>(),
                            q->out_nulls.as<unsigned char>(), q->out_expired.as<unsigned char>(),
                            q->out_rep.as<int64_t>());
    HIPCHK(hipGetLastError());
    const FlushVecs fl = flush_vecs(q, host_out);
    fl.offsets.assign(1, 0);
    fl.clocks.clear();
    if (T) {
        fl.offsets.push_back(T);
        fl.clocks.push_back(now);
    }
    return rows_out(q, T, host_out, false);
}
