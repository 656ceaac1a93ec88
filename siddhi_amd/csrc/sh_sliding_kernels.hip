// sh_sliding_kernels.hip — gfx950 kernels of the sliding `#window.time(T)` group-by path: the prefix,
// records and multisplit passes, the key-partition replays (k_sl_own, k_sl_own_d), emit, flush and rekey.
// The keyed replay (one wave per key) is in sh_sliding_wkey.hip.
//
// TimeWindowProcessor.process (core/query/processor/stream/window/TimeWindowProcessor.java:132-169)
// expires, before each event, the longest queue prefix whose events satisfy ts + T <= now. For the
// j-th passing event that prefix condition is PM(j) + T <= clock, PM(j) = max ts of passing events
// 0..j. Per key, an expiry only has to be applied before the key's next add (its state is only
// observed at its own events), so each key's window is a ring of (value, PM) and expiry is applied
// lazily when the key is next touched. Aggregators run in SLIDE mode: sums with Java's sequential
// add/remove (residue included), min/max with the reference's monotone deque and its
// removeFirstOccurrence(value) quirk (MinAttributeAggregatorExecutor.java:170-205).
#include "sh_device.h"
#include "sh_sliding.h"
#include "sh_sliding_wave.h"

namespace shd {

// ------------------------------------------------------------------------------------------------
// s_blockagg: per workgroup pass count, max send-last ts, max ts over passing events.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sl_blockagg(const i64* __restrict__ ts, ColSet cols, FilterProg f,
                                                       WinParams wp, i64* blk_pass, i64* blk_tl, i64* blk_pm) {
    i64 base = (i64)blockIdx.x * kTile + (i64)threadIdx.x * kItems;
    i64 cnt = 0, tl = INT64_MIN, pm = INT64_MIN;
    bool pass[kItems];
    filter_items(f, cols, base, wp.N, pass);
    // externalTime: PM runs over the timestamp attribute instead of the event timestamps
    // (length(N): PM is the ordinal of the passing event, base + rank — no maximum to carry)
    const bool ext = wp.kind == SH_WIN_EXT_TIME, len = wp.kind == SH_WIN_LENGTH;
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        i64 e = base + i;
        if (e < wp.N) {
            i64 t = ts[e];
            if (pass[i]) { cnt++; if (!len) pm = max(pm, ext ? load_raw(cols, wp.ts_col, e) : t); }
            if (is_send_last(wp, e)) tl = max(tl, t);
        }
    }
    i64 c = block_reduce(cnt, SumOp(), 0);
    i64 t = block_reduce(tl, MaxOp(), INT64_MIN);
    i64 p = block_reduce(pm, MaxOp(), INT64_MIN);
    if (threadIdx.x == 0) { blk_pass[blockIdx.x] = c; blk_tl[blockIdx.x] = t; blk_pm[blockIdx.x] = p; }
}

__global__ __launch_bounds__(1024) void k_sl_scan(i64* blk_pass, i64* blk_tl, i64* blk_pm, int nblk, SlInfo* info) {
    __shared__ i64 a[1024], b[1024], c[1024];
    int t = threadIdx.x;
    int per = (nblk + 1023) / 1024;
    int lo = t * per, hi = min(nblk, lo + per);
    i64 s = 0, m = INT64_MIN, p = INT64_MIN;
    for (int i = lo; i < hi; i++) { s += blk_pass[i]; m = max(m, blk_tl[i]); p = max(p, blk_pm[i]); }
    a[t] = s; b[t] = m; c[t] = p;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        i64 x = t >= d ? a[t - d] : 0, y = t >= d ? b[t - d] : INT64_MIN, z = t >= d ? c[t - d] : INT64_MIN;
        __syncthreads();
        a[t] += x; b[t] = max(b[t], y); c[t] = max(c[t], z);
        __syncthreads();
    }
    i64 rs = t ? a[t - 1] : 0, rm = t ? b[t - 1] : INT64_MIN, rp = t ? c[t - 1] : INT64_MIN;
    for (int i = lo; i < hi; i++) {
        i64 x = blk_pass[i], y = blk_tl[i], z = blk_pm[i];
        blk_pass[i] = rs; blk_tl[i] = rm; blk_pm[i] = rp;
        rs += x; rm = max(rm, y); rp = max(rp, z);
    }
    if (t == 1023) { info->total_pass = a[1023]; info->max_tl = b[1023]; info->max_pm = c[1023]; }
}

void launch_sl_prefix(hipStream_t s, const i64* ts, ColSet cols, FilterProg f, WinParams wp, i64* blk_pass,
                      i64* blk_tl, i64* blk_pm, int nblk, SlInfo* info) {
    hipLaunchKernelGGL(k_sl_blockagg, dim3(nblk), dim3(kBlock), 0, s, ts, cols, f, wp, blk_pass, blk_tl, blk_pm);
    hipLaunchKernelGGL(k_sl_scan, dim3(1), dim3(1024), 0, s, blk_pass, blk_tl, blk_pm, nblk, info);
}

// ------------------------------------------------------------------------------------------------
// s_records: passing events -> rank-indexed records {raw idx, slot, clock, PM, ts, values} and the
// per-slot count of new events (for ring sizing).
// ------------------------------------------------------------------------------------------------
// The per-slot count through a workgroup table in LDS: the tile's events add to their slot's LDS
// counter and each distinct slot of the tile makes one global atomic at the end. A Zipf-hot key
// (partition lanes over 10M Zipf keys: the hottest holds ~10% of the events) otherwise sends millions
// of same-address atomics into one L2 channel, which serialises them (43 ms per 33.5M-event push).
constexpr int kSlotTab = 2 * kTile;  // at most kTile distinct slots per tile: never full
__device__ __forceinline__ void slot_tab_add(u32* tk, u32* tc, u32 pos) {
    u32 h = (pos * 2654435761u) & (kSlotTab - 1);
    for (;;) {
        const u32 old = atomicCAS(&tk[h], 0xFFFFFFFFu, pos);
        if (old == 0xFFFFFFFFu || old == pos) { atomicAdd(&tc[h], 1u); return; }
        h = (h + 1) & (kSlotTab - 1);
    }
}

__global__ __launch_bounds__(kBlock) void k_sl_records(const i64* __restrict__ ts, ColSet cols, FilterProg f,
                                                      WinParams wp, KeyPlan kp, KeyTable kt, AggPlan ap,
                                                      const i64* blk_pass_pre, const i64* blk_tl_pre,
                                                      const i64* blk_pm_pre, i64 pm0, SlRecords rec, u32* slot_cnt,
                                                      i64* send_clock) {
    __shared__ u32 tk[kSlotTab], tc[kSlotTab];
    for (int i = threadIdx.x; i < kSlotTab; i += kBlock) { tk[i] = 0xFFFFFFFFu; tc[i] = 0; }
    i64 base = (i64)blockIdx.x * kTile + (i64)threadIdx.x * kItems;
    bool pass[kItems];
    i64 cnt = 0, tl = INT64_MIN, pm = INT64_MIN;
    filter_items(f, cols, base, wp.N, pass);
    const bool ext = wp.kind == SH_WIN_EXT_TIME, len = wp.kind == SH_WIN_LENGTH;
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        i64 e = base + i;
        if (e < wp.N) {
            i64 t = ts[e];
            cnt += pass[i];
            if (pass[i] && !len) pm = max(pm, ext ? load_raw(cols, wp.ts_col, e) : t);
            if (is_send_last(wp, e)) tl = max(tl, t);
        }
    }
    i64 r = block_excl_scan(cnt, SumOp(), 0, nullptr) + blk_pass_pre[blockIdx.x];
    i64 cm = max(block_excl_scan(tl, MaxOp(), INT64_MIN, nullptr), blk_tl_pre[blockIdx.x]);
    // length(N) (LengthWindowProcessor :106-142): the clock is the count of passing events, so the PM and
    // the clock of a record are its ordinal pm0 + rank (pm0 = the passing events of earlier pushes) and
    // "PM(j) + N <= clock(i)" is j <= i - N; no max-scan of the timestamps
    i64 pmx = len ? 0 : max(max(block_excl_scan(pm, MaxOp(), INT64_MIN, nullptr), blk_pm_pre[blockIdx.x]), pm0);
    const i64 c0 = wp.clock_valid ? wp.clock0 : INT64_MIN;
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        i64 e = base + i;
        const bool in = e < wp.N;
        const bool valid = in && pass[i];
        u32 pos = 0;
        i64 t = in ? ts[e] : 0;
        if (valid) {
            // externalTime (ExternalTimeWindowProcessor :126-161): an event expires the queue head
            // while headTime + T <= its own attribute, so event j has left the window at event i iff
            // PMa(j) + T <= PMa(i) (PMa = running max of the attribute): clock = PMa(i)
            pmx = len ? pm0 + r : max(pmx, ext ? load_raw(cols, wp.ts_col, e) : t);
            const i64 sclk = max(c0, max(cm, ts[send_last_of(wp, e)]));
            i64 clk = ext || len ? pmx : sclk;
            if (send_clock) send_clock[r] = sclk;  // the flush clock of an externalTime row
            pos = key_slot(kt, make_key(kp, cols, e));
            rec.raw[r] = (u32)e;
            rec.slot[r] = pos;
            if (rec.aos) {
                ulonglong2* o = (ulonglong2*)(rec.aos + (size_t)r * kSlAosWords);
                o[0] = make_ulonglong2((u64)clk, (u64)pmx);
                o[1] = make_ulonglong2((u64)t, (u64)load_raw(cols, ap.vcol_src[0], e));
                o[2] = make_ulonglong2((u64)e, 0ull);
            } else {
                rec.clock[r] = clk;
                rec.pm[r] = pmx;
                rec.ts[r] = t;
                for (int j = 0; j < ap.n_vcols; j++) rec.vals[(size_t)j * rec.cap + r] = (u64)load_raw(cols, ap.vcol_src[j], e);
            }
            slot_tab_add(tk, tc, pos);
            r++;
        }
        if (in && is_send_last(wp, e)) cm = max(cm, t);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSlotTab; i += kBlock)
        if (tc[i]) atomicAdd(&slot_cnt[tk[i]], tc[i]);
}

// The common case of k_sl_records — no filter, one event per send, time(T) — with the tile's events
// taken lane-strided (round i: events tile + i * kBlock + lane), so consecutive lanes write consecutive
// records (whole lines; the thread-contiguous form stored 48-byte records 8 apart per lane, and PMC saw
// 2.3x the record bytes written). Every event passes and ends its own send, so its clock and PM are the
// running maximum of the timestamps (a block max-scan per round, carried across rounds).
template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_sl_records_seq(const i64* __restrict__ ts, ColSet cols, WinParams wp,
                                                          KeyPlan kp, KeyTable kt, AggPlan ap,
                                                          const i64* blk_pass_pre, const i64* blk_tl_pre,
                                                          const i64* blk_pm_pre, i64 pm0, SlRecords rec,
                                                          u32* slot_cnt, i64* send_clock) {
    // (without the slot table the block needs 12 KB of LDS instead of 45: 8 resident waves, not 3)
    __shared__ u32 tk[COUNT ? kSlotTab : 1], tc[COUNT ? kSlotTab : 1];
    // the wave's 64 records staged in LDS, then stored as contiguous 16-byte pieces (each store
    // instruction covers 1 KB of whole lines instead of one piece of 64 records 48 bytes apart)
    __shared__ ulonglong2 stg[kBlock * 3];
    // slot_cnt null: the caller takes the per-slot counts from the sorted slots instead (k_counts_sorted:
    // r05, the tile's LDS table and its global atomics were 1.2 of the kernel's 1.9 ms at C3)
    constexpr bool count = COUNT;
    if (count)
        for (int i = threadIdx.x; i < kSlotTab; i += kBlock) { tk[i] = 0xFFFFFFFFu; tc[i] = 0; }
    const i64 tile0 = (i64)blockIdx.x * kTile;
    const i64 r0 = blk_pass_pre[blockIdx.x];
    i64 carry_cm = blk_tl_pre[blockIdx.x];
    i64 carry_pm = max(blk_pm_pre[blockIdx.x], pm0);
    const i64 c0 = wp.clock_valid ? wp.clock0 : INT64_MIN;
    // length(N): every event passes, so a record's clock and PM are its ordinal pm0 + r and the block
    // max-scan below only serves the send's playback clock (column records only: the keyed replay's
    // 48-byte records hold one clock, and a length row's flush clock is not its expiry clock)
    const bool len = wp.kind == SH_WIN_LENGTH;
    const int lane = threadIdx.x & 63, wb = threadIdx.x & ~63;
    for (int it = 0; it < kItems; it++) {
        const i64 e = tile0 + (i64)it * kBlock + threadIdx.x;
        const bool in = e < wp.N;
        const i64 t = in ? ts[e] : INT64_MIN;
        const u32 pos = in ? key_slot(kt, make_key(kp, cols, e)) : 0u;
        const u64 v = in ? (u64)load_raw(cols, ap.vcol_src[0], e) : 0ull;
        i64 tot;
        const i64 incl = max(block_excl_scan(t, MaxOp(), INT64_MIN, &tot), t);
        if (rec.aos) {
            // (every event of the tile passes: record r0 + it * kBlock + thread; the wave's run is whole
            // records r_w .. r_w + 63, fewer at the push's end)
            const i64 pmx = max(carry_pm, incl);
            const i64 sclk = max(c0, max(carry_cm, incl));
            const i64 r = r0 + (i64)it * kBlock + threadIdx.x;
            if (in) {
                if (send_clock) send_clock[r] = sclk;
                rec.raw[r] = (u32)e;
                rec.slot[r] = pos;
                if (count) slot_tab_add(tk, tc, pos);
            }
            stg[threadIdx.x * 3 + 0] = make_ulonglong2((u64)sclk, (u64)pmx);
            stg[threadIdx.x * 3 + 1] = make_ulonglong2((u64)t, v);
            stg[threadIdx.x * 3 + 2] = make_ulonglong2((u64)e, 0ull);
            __syncthreads();
            const i64 rw = r0 + (i64)it * kBlock + wb;  // the wave's first record
            const i64 ew = tile0 + (i64)it * kBlock + wb;
            const int nw = (int)max((i64)0, min((i64)64, wp.N - ew));
            ulonglong2* dst = (ulonglong2*)(rec.aos + (size_t)rw * kSlAosWords);
            for (int q = lane; q < nw * 3; q += 64) dst[q] = stg[wb * 3 + q];
            __syncthreads();
        } else if (in) {
            const i64 r = r0 + (i64)it * kBlock + threadIdx.x;
            const i64 pmx = len ? pm0 + r : max(carry_pm, incl);
            const i64 sclk = max(c0, max(carry_cm, incl));
            if (send_clock) send_clock[r] = sclk;
            rec.raw[r] = (u32)e;
            rec.slot[r] = pos;
            {
                rec.clock[r] = len ? pmx : sclk;
                rec.pm[r] = pmx;
                rec.ts[r] = t;
                for (int j = 0; j < ap.n_vcols; j++) rec.vals[(size_t)j * rec.cap + r] = (u64)load_raw(cols, ap.vcol_src[j], e);
            }
            if (count) slot_tab_add(tk, tc, pos);
        }
        carry_pm = max(carry_pm, tot);
        carry_cm = max(carry_cm, tot);
    }
    __syncthreads();
    if (count)
        for (int i = threadIdx.x; i < kSlotTab; i += kBlock)
            if (tc[i]) atomicAdd(&slot_cnt[tk[i]], tc[i]);
}

bool sl_records_seq_applies(FilterProg f, WinParams wp, AggPlan ap) {
    return filter_kind(f) == 0 && wp.send_size == 1 && (wp.kind == SH_WIN_TIME || wp.kind == SH_WIN_LENGTH) &&
           ap.n_vcols >= 1 && wp.rec_seq;
}

void launch_sl_records(hipStream_t s, const i64* ts, ColSet cols, FilterProg f, WinParams wp, KeyPlan kp,
                       KeyTable kt, AggPlan ap, const i64* blk_pass_pre, const i64* blk_tl_pre, const i64* blk_pm_pre,
                       i64 pm0, SlRecords rec, u32* slot_cnt, int nblk, i64* send_clock) {
    if (sl_records_seq_applies(f, wp, ap)) {
        if (slot_cnt)
            hipLaunchKernelGGL(k_sl_records_seq<true>, dim3(nblk), dim3(kBlock), 0, s, ts, cols, wp, kp, kt, ap,
                               blk_pass_pre, blk_tl_pre, blk_pm_pre, pm0, rec, slot_cnt, send_clock);
        else
            hipLaunchKernelGGL(k_sl_records_seq<false>, dim3(nblk), dim3(kBlock), 0, s, ts, cols, wp, kp, kt, ap,
                               blk_pass_pre, blk_tl_pre, blk_pm_pre, pm0, rec, nullptr, send_clock);
        return;
    }
    hipLaunchKernelGGL(k_sl_records, dim3(nblk), dim3(kBlock), 0, s, ts, cols, f, wp, kp, kt, ap, blk_pass_pre,
                       blk_tl_pre, blk_pm_pre, pm0, rec, slot_cnt, send_clock);
}

// Sharded owner (sh_shard.cpp): the records arrive filtered and re-keyed, with the global clock of
// their send and the global PM computed by the source slice (sh_shard_kernels.hip k_shard_sl_assign);
// raw = position in the global push, so send = send_base + raw / send_size as in the single stream.
__device__ __forceinline__ void sl_record_given(i64 r, const i64* __restrict__ ts, ColSet cols, KeyPlan kp, KeyTable kt,
                                                AggPlan ap, const i64* __restrict__ gclk, const i64* __restrict__ gpm,
                                                const u64* __restrict__ gidx, i64 raw_base, SlRecords rec, u32* tk,
                                                u32* tc) {
    const u32 pos = key_slot(kt, make_key(kp, cols, r));
    const u32 raw = (u32)((i64)gidx[r] - raw_base);
    rec.raw[r] = raw;
    rec.slot[r] = pos;
    if (rec.aos) {
        ulonglong2* o = (ulonglong2*)(rec.aos + (size_t)r * kSlAosWords);
        o[0] = make_ulonglong2((u64)gclk[r], (u64)gpm[r]);
        o[1] = make_ulonglong2((u64)ts[r], (u64)load_raw(cols, ap.vcol_src[0], r));
        o[2] = make_ulonglong2((u64)raw, 0ull);
    } else {
        rec.clock[r] = gclk[r];
        rec.pm[r] = gpm[r];
        rec.ts[r] = ts[r];
        for (int j = 0; j < ap.n_vcols; j++) rec.vals[(size_t)j * rec.cap + r] = (u64)load_raw(cols, ap.vcol_src[j], r);
    }
    slot_tab_add(tk, tc, pos);
}

__global__ __launch_bounds__(kBlock) void k_sl_records_given(i64 M, const i64* __restrict__ ts, ColSet cols,
                                                            KeyPlan kp, KeyTable kt, AggPlan ap,
                                                            const i64* __restrict__ gclk, const i64* __restrict__ gpm,
                                                            const u64* __restrict__ gidx, i64 raw_base,
                                                            SlRecords rec, u32* slot_cnt) {
    __shared__ u32 tk[kSlotTab], tc[kSlotTab];
    for (int i = threadIdx.x; i < kSlotTab; i += kBlock) { tk[i] = 0xFFFFFFFFu; tc[i] = 0; }
    __syncthreads();
    const i64 r = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (r < M) sl_record_given(r, ts, cols, kp, kt, ap, gclk, gpm, gidx, raw_base, rec, tk, tc);
    __syncthreads();
    for (int i = threadIdx.x; i < kSlotTab; i += kBlock)
        if (tc[i]) atomicAdd(&slot_cnt[tk[i]], tc[i]);
}


void launch_sl_records_given(hipStream_t s, i64 M, const i64* ts, ColSet cols, KeyPlan kp, KeyTable kt, AggPlan ap,
                             const i64* gclk, const i64* gpm, const u64* gidx, i64 raw_base, SlRecords rec,
                             u32* slot_cnt) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k_sl_records_given, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, M, ts,
                       cols, kp, kt, ap, gclk, gpm, gidx, raw_base, rec, slot_cnt);
}

// max over slots of (ring length + new events): the ring capacity this push needs
__global__ __launch_bounds__(kBlock) void k_sl_need(const u32* slot_cnt, const i64* rlen, i64 n, i64* out) {
    i64 m = 0;
    for (i64 i = (i64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (i64)gridDim.x * kBlock)
        if (slot_cnt[i]) m = max(m, rlen[i] + (i64)slot_cnt[i]);
    i64 t = block_reduce(m, MaxOp(), 0);
    if (threadIdx.x == 0) atomicMax((unsigned long long*)out, (unsigned long long)t);
}

void launch_sl_need(hipStream_t s, const u32* slot_cnt, const i64* rlen, i64 n, i64* out) {
    hipLaunchKernelGGL(k_sl_need, dim3(256), dim3(kBlock), 0, s, slot_cnt, rlen, n, out);
}

// Per-slot counts from the slot-sorted records: the first position of a slot's run subtracts its index,
// the last adds its index + 1 (two atomics per run, each on its own slot: no contention), so
// slot_cnt[k] = the run's length; zeroed by the caller. (Writing the key offsets directly from the run
// starts loops over every absent slot in between: with sparse slots — 231k Zipf partitions in a 10M-slot
// dictionary — single lanes filled gaps of thousands, plb 20 -> 103 ms per push.)
__global__ __launch_bounds__(kBlock) void k_counts_sorted(const u32* __restrict__ ps, i64 M, u32* slot_cnt) {
    const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const u32 cur = ps[i];
    if (i == 0 || ps[i - 1] != cur) atomicAdd(&slot_cnt[cur], (u32)(-(i64)i));
    if (i == M - 1 || ps[i + 1] != cur) atomicAdd(&slot_cnt[cur], (u32)(i + 1));
}

void launch_counts_sorted(hipStream_t s, const u32* ps, i64 M, u32* slot_cnt) {
    if (M > 0)
        hipLaunchKernelGGL(k_counts_sorted, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ps, M,
                           slot_cnt);
}

// ------------------------------------------------------------------------------------------------
// stable multisplit of the records by key partition p = slot & (P-1): rank lists per partition.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sl_ms_count(const u32* __restrict__ slot, i64 n, int P, i64* counts,
                                                       int nblk) {
    extern __shared__ __attribute__((aligned(16))) u32 hist[];
    for (int i = threadIdx.x; i < P; i += kBlock) hist[i] = 0;
    __syncthreads();
    i64 t0 = (i64)blockIdx.x * kTile;
    for (int r = 0; r < kItems; r++) {
        i64 e = t0 + (i64)r * kBlock + threadIdx.x;
        if (e < n) atomicAdd(&hist[slot[e] & (P - 1)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += kBlock) counts[(i64)i * nblk + blockIdx.x] = hist[i];
}

__global__ __launch_bounds__(kBlock) void k_sl_ms_scatter(const u32* __restrict__ slot, i64 n, int P,
                                                         const i64* __restrict__ offsets, int nblk, u32* out_rank) {
    __shared__ u32 stage[kTile];
    extern __shared__ __attribute__((aligned(16))) u32 dyn[];
    u32* hist = dyn;
    u32* local_start = hist + P;
    u32* running = local_start + P;
    u32* wave_cnt = running + P;  // [4][P]
    u32* stage_p = wave_cnt + 4 * P;  // [kTile]
    for (int i = threadIdx.x; i < P; i += kBlock) {
        hist[i] = 0; running[i] = 0;
        for (int w = 0; w < 4; w++) wave_cnt[w * P + i] = 0;
    }
    __syncthreads();
    const i64 t0 = (i64)blockIdx.x * kTile;
    u32 my_p[kItems];
    bool ok_[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        i64 e = t0 + (i64)r * kBlock + threadIdx.x;
        ok_[r] = e < n;
        my_p[r] = ok_[r] ? (slot[e] & (P - 1)) : 0;
        if (ok_[r]) atomicAdd(&hist[my_p[r]], 1u);
    }
    __syncthreads();
    {
        int per = (P + kBlock - 1) / kBlock;
        int a = threadIdx.x * per, b = min(P, a + per);
        i64 sum = 0;
        for (int i = a; i < b; i++) sum += hist[i];
        i64 pre = block_excl_scan(sum, SumOp(), 0, nullptr);
        for (int i = a; i < b; i++) { local_start[i] = (u32)pre; pre += hist[i]; }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int bits = 0;
    while ((1 << bits) < P) bits++;
    for (int r = 0; r < kItems; r++) {
        bool ok = ok_[r];
        u32 p = my_p[r];
        u64 peers = __ballot(ok);
        for (int bt = 0; bt < bits; bt++) {
            u64 m = __ballot((p >> bt) & 1);
            peers &= ((p >> bt) & 1) ? m : ~m;
        }
        u32 lrank = __popcll(peers & lt_mask);
        bool leader = ok && lrank == 0;
        if (leader) wave_cnt[wave * P + p] = __popcll(peers);
        __syncthreads();
        if (ok) {
            u32 before = running[p];
            for (int w = 0; w < wave; w++) before += wave_cnt[w * P + p];
            u32 sl = local_start[p] + before + lrank;
            stage[sl] = (u32)(t0 + (i64)r * kBlock + threadIdx.x);
            stage_p[sl] = p;
        }
        __syncthreads();
        if (leader) { atomicAdd(&running[p], wave_cnt[wave * P + p]); wave_cnt[wave * P + p] = 0; }
        __syncthreads();
    }
    u32 n_tile = local_start[P - 1] + hist[P - 1];
    for (u32 j = threadIdx.x; j < n_tile; j += kBlock) {
        u32 p = stage_p[j];
        out_rank[offsets[(i64)p * nblk + blockIdx.x] + (j - local_start[p])] = stage[j];
    }
}

void launch_sl_multisplit(hipStream_t s, const u32* slot, i64 n, int P, i64* counts, i64* tmp, u32* out_rank,
                          i64* part_off) {
    int nblk = (int)((n + kTile - 1) / kTile);
    if (nblk == 0) return;
    hipLaunchKernelGGL(k_sl_ms_count, dim3(nblk), dim3(kBlock), P * 4, s, slot, n, P, counts, nblk);
    i64 ncnt = (i64)P * nblk;
    (void)hipMemsetAsync(counts + ncnt, 0, 8, s);
    launch_scan_sum_large(s, counts, ncnt + 1, tmp);
    size_t lds = (size_t)P * 4 * 7 + (size_t)kTile * 4 + 16;
    hipLaunchKernelGGL(k_sl_ms_scatter, dim3(nblk), dim3(kBlock), lds, s, slot, n, P, counts, nblk, out_rank);
    launch_part_off(s, counts, nblk, P, part_off);
}

// ------------------------------------------------------------------------------------------------
// k_sliding: one wave per key partition walks its records in event order. Lanes sharing a key are
// resolved in rounds (lowest lane first), so each key's adds / removes run in the reference's order.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mm_worse(int kind, u64 cur, u64 v) {
    // `next > value` (min) / `next < value` (max) on unboxed values of the input type
    switch (kind) {
        case AK_MIN_L: return (i64)cur > (i64)v;
        case AK_MAX_L: return (i64)cur < (i64)v;
        case AK_MIN_D: return __longlong_as_double((i64)cur) > __longlong_as_double((i64)v);
        case AK_MAX_D: return __longlong_as_double((i64)cur) < __longlong_as_double((i64)v);
        case AK_MIN_F: return (float)__longlong_as_double((i64)cur) > (float)__longlong_as_double((i64)v);
        default: return (float)__longlong_as_double((i64)cur) < (float)__longlong_as_double((i64)v);
    }
}

// Double.equals / Float.equals (bit equality, NaN == NaN) and Integer/Long.equals
__device__ __forceinline__ bool boxed_eq(int kind, u64 a, u64 b) {
    if (kind == AK_MIN_L || kind == AK_MAX_L) return a == b;
    double x = __longlong_as_double((i64)a), y = __longlong_as_double((i64)b);
    if (kind == AK_MIN_F || kind == AK_MAX_F) {
        float fx = (float)x, fy = (float)y;
        if (fx != fx && fy != fy) return true;
        return __float_as_uint(fx) == __float_as_uint(fy);
    }
    if (x != x && y != y) return true;
    return a == b;
}

// ------------------------------------------------------------------------------------------------
// k_sl_own: one wave per key partition, lane ownership. Local key li = slot >> logP belongs to lane
// li & 63 (with NL <= 64 local keys every lane owns at most one key, whose state — counts, sums,
// min/max values, ring and deque heads — stays in registers for the whole push). The partition's
// records (event order) are taken in chunks; each chunk is split stably in LDS into 64 per-lane
// lists, and every lane replays its key's events in order: lazy expiry from the ring head, add, row.
// No conflict rounds. Latency is what bounds it (one dependent chain per key), so:
//  - the next record's fields and the next ring-head entry are loaded one step ahead;
//  - the min/max deques (MinAttributeAggregatorExecutor's LinkedList with removeFirstOccurrence)
//    live in LDS, kDqL entries per (key, aggregator); a deque that outgrows that spills to its ring
//    in global memory for the rest of the push (sorted input makes deques as long as the window).
// ------------------------------------------------------------------------------------------------
constexpr int kSlCh = 2048;
#ifndef SH_SL_KL
#define SH_SL_KL 8
#endif
// records staged per chunk of k_sl_own_d. Measured on MI355X, C3 (10k keys, 16.7M events per
// push): CH 512 -> 23.9 ms at KL 8 with CH 256, 20.2 ms at CH 128, 20.1 ms at CH 64; KL 4/8/16
// within 10% at CH 256, KL 2 31 ms (the ~11 KB LDS footprint at CH 128 keeps ~14 waves per CU)
#ifndef SH_SL_CH
#define SH_SL_CH 128
#endif
constexpr int kSlKeyLanes = SH_SL_KL;  // key-owning lanes per wave of k_sl_own_d
constexpr int kDqL = 32;

template <int NA, int NV>
struct LaneKey {
    u32 k;  // cached slot (kNoPos: none)
    i64 cnt, rh, rlen, cur_send, cur_first;
    u64 f[NA], mm[NA], dqf[NA], dqb[NA];
    i64 dqh[NA], dql[NA];
    unsigned char mmh[NA];
    bool spill[NA];
    bool hvalid;
    i64 hpm;
    u64 hval[NV];
    i64 hb_base;  // ring index of the first entry in the lane's LDS head cache
    int hb_n;     // valid entries there
};
constexpr int kHb = 8;  // ring-head entries fetched per refill (one latency per kHb expiries)

__device__ __forceinline__ bool is_mm(int kind) { return kind >= AK_MIN_L; }

// v[i] with a run-time i, as a select chain over the unrolled slots (keeps v in registers)
template <int NV>
__device__ __forceinline__ u64 pick(const u64 (&v)[NV], int i) {
    u64 x = v[0];
#pragma unroll
    for (int q = 1; q < NV; q++) x = (i == q) ? v[q] : x;
    return x;
}

// deque storage of aggregator a for the lane's key: LDS ring (kDqL) or, spilled, the global ring
struct DqView {
    u64* g;
    u64* l;
    i64 gm;
    bool spill;
    __device__ __forceinline__ u64 get(i64 i) const { return spill ? g[i & gm] : l[i & (kDqL - 1)]; }
    __device__ __forceinline__ void set(i64 i, u64 v) const {
        if (spill) g[i & gm] = v;
        else l[i & (kDqL - 1)] = v;
    }
};

template <int NA, int NV>
__device__ __forceinline__ DqView dq_view(const LaneKey<NA, NV>& L, const SlState& S, const AggPlan& ap, u64* lds_dq,
                                          const int (&mmi)[NA], int a) {
    DqView d;
    d.g = S.dq + ((size_t)ap.field[a] * S.nslots + L.k) * S.rc;
    d.l = lds_dq + ((size_t)mmi[a] * 64 + threadIdx.x) * kDqL;
    d.gm = S.rc - 1;
    d.spill = L.spill[a];
    return d;
}

template <int NA, int NV>
__device__ __forceinline__ void lk_load(LaneKey<NA, NV>& L, const SlState& S, const AggPlan& ap, u64* lds_dq,
                                        const int (&mmi)[NA], u32 k) {
    L.k = k;
    L.cnt = S.cnt[k];
    L.rh = S.rhead[k];
    L.rlen = S.rlen[k];
    L.cur_send = S.cur_send[k];
    L.cur_first = S.cur_first[k];
    L.hvalid = false;
    L.hb_n = 0;
#pragma unroll
    for (int a = 0; a < NA; a++) {
        if (a >= ap.n) break;
        const int kind = ap.kind[a];
        if (kind == AK_COUNT) continue;
        const size_t fi = (size_t)ap.field[a] * S.nslots + k;
        L.f[a] = S.f[fi];
        if (is_mm(kind)) {
            L.mm[a] = S.mm[fi];
            L.mmh[a] = S.mm_has[fi];
            L.dqh[a] = S.dq_head[fi];
            L.dql[a] = S.dq_len[fi];
            L.spill[a] = L.dql[a] >= kDqL;
            const DqView d = dq_view(L, S, ap, lds_dq, mmi, a);
            const i64 h = L.dqh[a], len = L.dql[a];
            if (!d.spill)
                for (i64 i = 0; i < len; i++) d.l[(h + i) & (kDqL - 1)] = d.g[(h + i) & d.gm];
            if (len > 0) {
                L.dqf[a] = d.get(h);
                L.dqb[a] = d.get(h + len - 1);
            }
        }
    }
}

template <int NA, int NV>
__device__ __forceinline__ void lk_store(const LaneKey<NA, NV>& L, const SlState& S, const AggPlan& ap, u64* lds_dq,
                                         const int (&mmi)[NA]) {
    const u32 k = L.k;
    S.cnt[k] = L.cnt;
    S.rhead[k] = L.rh;
    S.rlen[k] = L.rlen;
    S.cur_send[k] = L.cur_send;
    S.cur_first[k] = L.cur_first;
#pragma unroll
    for (int a = 0; a < NA; a++) {
        if (a >= ap.n) break;
        const int kind = ap.kind[a];
        if (kind == AK_COUNT) continue;
        const size_t fi = (size_t)ap.field[a] * S.nslots + k;
        S.f[fi] = L.f[a];
        if (is_mm(kind)) {
            S.mm[fi] = L.mm[a];
            S.mm_has[fi] = L.mmh[a];
            S.dq_head[fi] = L.dqh[a];
            S.dq_len[fi] = L.dql[a];
            const DqView d = dq_view(L, S, ap, lds_dq, mmi, a);
            if (!d.spill)
                for (i64 i = 0; i < L.dql[a]; i++) d.g[(L.dqh[a] + i) & d.gm] = d.l[(L.dqh[a] + i) & (kDqL - 1)];
        }
    }
}

// the ring head entry (index rh) into registers, from the lane's LDS cache of the next kHb
// entries; a refill loads up to kHb entries (never past the current tail) in one round trip
template <int NA, int NV>
__device__ __forceinline__ void lk_head(LaneKey<NA, NV>& L, const SlState& S, const AggPlan& ap, i64* hb_pm,
                                        u64* hb_v) {
    const int lane = threadIdx.x;
    if (!(L.rh >= L.hb_base && L.rh < L.hb_base + L.hb_n)) {
        const int n = (int)min<i64>(kHb, L.rlen);
        i64 pm[kHb];
        u64 vv[NV][kHb];
#pragma unroll
        for (int e = 0; e < kHb; e++) {
            if (e < n) {
                const i64 sl = (L.rh + e) & (S.rc - 1);
                pm[e] = S.rpm[(size_t)L.k * S.rc + sl];
#pragma unroll
                for (int j = 0; j < NV; j++)
                    if (j < ap.n_vcols) vv[j][e] = S.rval[((size_t)j * S.nslots + L.k) * S.rc + sl];
            }
        }
#pragma unroll
        for (int e = 0; e < kHb; e++) {
            if (e < n) {
                hb_pm[lane * kHb + e] = pm[e];
#pragma unroll
                for (int j = 0; j < NV; j++)
                    if (j < ap.n_vcols) hb_v[(j * 64 + lane) * kHb + e] = vv[j][e];
            }
        }
        L.hb_base = L.rh;
        L.hb_n = n;
    }
    const int e = (int)(L.rh - L.hb_base);
    L.hpm = hb_pm[lane * kHb + e];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        if (j >= ap.n_vcols) break;
        L.hval[j] = hb_v[(j * 64 + lane) * kHb + e];
    }
    L.hvalid = true;
}

// AttributeAggregatorExecutor.processRemove for every aggregator (same arithmetic as sl_remove)
template <int NA, int NV>
__device__ __forceinline__ void lk_remove(LaneKey<NA, NV>& L, const SlState& S, const AggPlan& ap, u64* lds_dq,
                                          const int (&mmi)[NA], const u64 (&v)[NV]) {
    const i64 c = L.cnt - 1;
    L.cnt = c;
#pragma unroll
    for (int a = 0; a < NA; a++) {
        if (a >= ap.n) break;
        const int kind = ap.kind[a];
        if (kind == AK_COUNT) continue;
        const u64 x = pick(v, ap.vcol[a]);
        if (kind == AK_SUM_L) {
            L.f[a] = (u64)java_d2l((double)(i64)L.f[a] - (double)(i64)x);
        } else if (kind == AK_SUM_D || kind == AK_AVG) {
            const double xv = (kind == AK_AVG && !(ap.vcol_type[ap.vcol[a]] == SH_T_FLOAT ||
                                                   ap.vcol_type[ap.vcol[a]] == SH_T_DOUBLE))
                                  ? (double)(i64)x : __longlong_as_double((i64)x);
            double r = __longlong_as_double((i64)L.f[a]) - xv;
            if (c == 0 && r == 0.0) r = 0.0;  // destroyed state restarts from +0.0 (canDestroy)
            L.f[a] = (u64)__double_as_longlong(r);
        } else {
            // removeFirstOccurrence(value): the front in the common case, else a scan
            const DqView d = dq_view(L, S, ap, lds_dq, mmi, a);
            i64 h = L.dqh[a], len = L.dql[a];
            if (len > 0 && boxed_eq(kind, L.dqf[a], x)) {
                h++;
                len--;
                if (len > 0) L.dqf[a] = d.get(h);
            } else if (len > 1) {
                i64 found = -1;
                for (i64 i = 1; i < len; i++)
                    if (boxed_eq(kind, d.get(h + i), x)) { found = i; break; }
                if (found >= 0) {
                    for (i64 i = found; i + 1 < len; i++) d.set(h + i, d.get(h + i + 1));
                    len--;
                    L.dqb[a] = d.get(h + len - 1);
                }
            }
            L.dqh[a] = h;
            L.dql[a] = len;
            if (len > 0) { L.mm[a] = L.dqf[a]; L.mmh[a] = 1; }
            else L.mmh[a] = 0;
        }
    }
}

// processAdd (same arithmetic as sl_add)
template <int NA, int NV>
__device__ __forceinline__ void lk_add(LaneKey<NA, NV>& L, const SlState& S, const AggPlan& ap, u64* lds_dq,
                                       const int (&mmi)[NA], const u64 (&v)[NV]) {
    L.cnt = L.cnt + 1;
#pragma unroll
    for (int a = 0; a < NA; a++) {
        if (a >= ap.n) break;
        const int kind = ap.kind[a];
        if (kind == AK_COUNT) continue;
        const u64 x = pick(v, ap.vcol[a]);
        if (kind == AK_SUM_L) {
            L.f[a] = (u64)((i64)L.f[a] + (i64)x);
        } else if (kind == AK_SUM_D || kind == AK_AVG) {
            const double xv = (kind == AK_AVG && !(ap.vcol_type[ap.vcol[a]] == SH_T_FLOAT ||
                                                   ap.vcol_type[ap.vcol[a]] == SH_T_DOUBLE))
                                  ? (double)(i64)x : __longlong_as_double((i64)x);
            L.f[a] = (u64)__double_as_longlong(__longlong_as_double((i64)L.f[a]) + xv);
        } else {
            DqView d = dq_view(L, S, ap, lds_dq, mmi, a);
            const i64 h = L.dqh[a];
            i64 len = L.dql[a];
            while (len > 0 && mm_worse(kind, L.dqb[a], x)) {
                len--;
                if (len > 0) L.dqb[a] = d.get(h + len - 1);
            }
            if (!d.spill && len == kDqL) {  // the LDS ring is full: move to the global ring
                for (i64 i = 0; i < len; i++) d.g[(h + i) & d.gm] = d.l[(h + i) & (kDqL - 1)];
                L.spill[a] = true;
                d.spill = true;
            }
            d.set(h + len, x);
            len++;
            L.dqb[a] = x;
            if (len == 1) L.dqf[a] = x;
            L.dql[a] = len;
            if (!L.mmh[a] || mm_worse(kind, L.mm[a], x)) { L.mm[a] = x; L.mmh[a] = 1; }
        }
    }
}

template <int NV>
struct SlRec {
    i64 clk, pm, ts;
    u32 raw;
    u64 v[NV];
};

template <int NV>
__device__ __forceinline__ void sl_rec_load(SlRec<NV>& o, const SlRecords& rec, const AggPlan& ap, i64 r) {
    o.clk = rec.clock[r];
    o.pm = rec.pm[r];
    o.ts = rec.ts[r];
    o.raw = rec.raw[r];
#pragma unroll
    for (int q = 0; q < NV; q++) {
        if (q >= ap.n_vcols) break;
        o.v[q] = rec.vals[(size_t)q * rec.cap + r];
    }
}

// Chunk split shared by the k_sl_own kernels: records [c0, c0+n) of the partition (event order)
// into 64 stable per-lane lists (lane = (slot >> logP) & 63). Returns this lane's count and start.
// BYRANK: slot is indexed by record rank (records not gathered into partition order).
template <int KL = 64, bool BYRANK = false>
__device__ __forceinline__ void sl_chunk_split(const u32* __restrict__ rank_list, const u32* __restrict__ slot, i64 c0,
                                               int n, int logP, u32* ch_rank, u32* ch_slot, unsigned short* list,
                                               u32* run, u32& mine_out, u32& start_out) {
    constexpr int B = KL == 64 ? 6 : KL == 32 ? 5 : KL == 16 ? 4 : KL == 8 ? 3 : KL == 4 ? 2 : 1;
    const int lane = threadIdx.x;
    const u64 lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    u32 mine = 0;
    for (int g = 0; g < n; g += 64) {
        const int j = g + lane;
        u32 o = 0;
        if (j < n) {
            const u32 rk = rank_list[c0 + j];
            const u32 k = BYRANK ? slot[rk] : slot[c0 + j];
            o = (k >> logP) & (KL - 1);
            ch_rank[j] = rk;
            ch_slot[j] = k;
        }
        u64 mask = __ballot(j < n);
#pragma unroll
        for (int bt = 0; bt < B; bt++) {
            const u64 b = __ballot((o >> bt) & 1);
            mask &= ((lane >> bt) & 1) ? b : ~b;
        }
        if (lane < KL) mine += (u32)__popcll(mask);
    }
    u32 incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    const u32 start = incl - mine;
    run[lane] = start;
    __syncthreads();
    for (int g = 0; g < n; g += 64) {
        const int j = g + lane;
        const bool ok = j < n;
        const u32 o = ok ? ((ch_slot[j] >> logP) & (KL - 1)) : 0;
        u64 peers = __ballot(ok);
#pragma unroll
        for (int bt = 0; bt < B; bt++) {
            const bool bit = (o >> bt) & 1;
            const u64 b = __ballot(bit);
            peers &= bit ? b : ~b;
        }
        const u32 lr = (u32)__popcll(peers & lt_mask);
        u32 base = 0;
        if (ok) base = run[o];
        __syncthreads();
        if (ok) list[base + lr] = (unsigned short)j;
        if (ok && lr == 0) run[o] = base + (u32)__popcll(peers);
        __syncthreads();
    }
    mine_out = mine;
    start_out = start;
}

// ---- k_sl_own_d: the same replay specialised for the common shape — every aggregator is count or
// reads one DOUBLE column with sum / avg / min / max (each at most once). Sum and avg perform the
// identical += / -= sequence (with the same canDestroy reset), so they share one running sum; the
// min and max deques use plain double comparisons and Double.equals. Far fewer instructions per
// event than the generic kernel, whose run-time aggregator dispatch dominated its chain latency.
// (The shape's fields, DFields, and the double comparisons d_eq / d_worse / d_isnan: sh_sliding_wave.h.)
struct DDeque {
    i64 h, len;
    u64 f, b, mm;
    bool mmh, spill;
    bool nan;  // a NaN may be in the deque (Java comparisons with NaN are false: order no longer holds)
};

// The deque of the lane's key lives in its LDS ring `l` (kDqL entries) unless it outgrew that
// (`spill`): then in its global ring `g`. The two paths are separate so each uses plain LDS or
// global instructions (a pointer select would compile to FLAT accesses that wait on both counters).
__device__ __forceinline__ void dd_load(DDeque& q, const SlState& S, int field, u32 k, u64* l) {
    const size_t fi = (size_t)field * S.nslots + k;
    q.mm = S.mm[fi];
    q.mmh = S.mm_has[fi];
    q.h = S.dq_head[fi];
    q.len = S.dq_len[fi];
    q.spill = q.len >= kDqL;
    q.nan = q.spill;
    const u64* g = S.dq + fi * S.rc;
    const i64 gm = S.rc - 1;
    if (!q.spill) {
        for (i64 i = 0; i < q.len; i++) {
            const u64 v = g[(q.h + i) & gm];
            l[((q.h + i) & (kDqL - 1))] = v;
            q.nan |= d_isnan(v);
        }
    }
    if (q.len > 0) {
        q.f = g[q.h & gm];
        q.b = g[(q.h + q.len - 1) & gm];
    }
}

__device__ __forceinline__ void dd_store(const DDeque& q, const SlState& S, int field, u32 k, const u64* l) {
    const size_t fi = (size_t)field * S.nslots + k;
    S.mm[fi] = q.mm;
    S.mm_has[fi] = q.mmh;
    S.dq_head[fi] = q.h;
    S.dq_len[fi] = q.len;
    u64* g = S.dq + fi * S.rc;
    const i64 gm = S.rc - 1;
    if (!q.spill)
        for (i64 i = 0; i < q.len; i++) g[(q.h + i) & gm] = l[((q.h + i) & (kDqL - 1))];
}

// removeFirstOccurrence(x) then minValue = peekFirst() (Min/MaxAttributeAggregatorExecutor).
// The front is the common case. Otherwise, while no NaN is in the deque it is monotone (min:
// non-decreasing, max: non-increasing), so an x beyond the back cannot be in it and needs no scan.
template <bool MIN, bool GLOBAL>
__device__ __forceinline__ void dd_remove_t(DDeque& q, u64* g, i64 gm, u64* l, u64 x) {
    auto at = [&](i64 i) -> u64 { return GLOBAL ? g[i & gm] : l[(i & (kDqL - 1))]; };
    if (q.len > 0 && d_eq(q.f, x)) {
        q.h++;
        q.len--;
        if (q.len > 0) q.f = at(q.h);
    } else if (q.len > 1 && (q.nan || !d_worse<MIN>(x, q.b))) {
        i64 found = -1;
        for (i64 i = 1; i < q.len; i++)
            if (d_eq(at(q.h + i), x)) { found = i; break; }
        if (found >= 0) {
            for (i64 i = found; i + 1 < q.len; i++) {
                const u64 v = at(q.h + i + 1);
                if (GLOBAL) g[(q.h + i) & gm] = v;
                else l[((q.h + i) & (kDqL - 1))] = v;
            }
            q.len--;
            q.b = at(q.h + q.len - 1);
        }
    }
    if (q.len > 0) { q.mm = q.f; q.mmh = true; }
    else { q.mmh = false; q.nan = q.spill; }
}

template <bool MIN>
__device__ __forceinline__ void dd_remove(DDeque& q, u64* g, i64 gm, u64* l, u64 x) {
    if (q.spill) dd_remove_t<MIN, true>(q, g, gm, l, x);
    else dd_remove_t<MIN, false>(q, g, gm, l, x);
}

template <bool MIN, bool GLOBAL>
__device__ __forceinline__ void dd_add_t(DDeque& q, u64* g, i64 gm, u64* l, u64 x) {
    while (q.len > 0 && d_worse<MIN>(q.b, x)) {
        q.len--;
        if (q.len > 0) q.b = GLOBAL ? g[(q.h + q.len - 1) & gm] : l[((q.h + q.len - 1) & (kDqL - 1))];
    }
}

template <bool MIN>
__device__ __forceinline__ void dd_add(DDeque& q, u64* g, i64 gm, u64* l, u64 x) {
    if (q.spill) dd_add_t<MIN, true>(q, g, gm, l, x);
    else dd_add_t<MIN, false>(q, g, gm, l, x);
    if (!q.spill && q.len == kDqL) {  // the LDS ring is full: move to the global ring
        for (i64 i = 0; i < q.len; i++) g[(q.h + i) & gm] = l[((q.h + i) & (kDqL - 1))];
        q.spill = true;
        q.nan = true;  // the global path always scans
    }
    if (q.spill) g[(q.h + q.len) & gm] = x;
    else l[((q.h + q.len) & (kDqL - 1))] = x;
    q.len++;
    q.b = x;
    q.nan |= d_isnan(x);
    if (q.len == 1) q.f = x;
    if (!q.mmh || d_worse<MIN>(q.mm, x)) { q.mm = x; q.mmh = true; }
}

// `rec` is the push's records in rank order (no k_sl_gather pass): the chunk's fields are read through
// the partition's rank list, and their latency overlaps the other waves' replay
template <bool HSUM, bool HMIN, bool HMAX>
__global__ __launch_bounds__(64) void k_sl_own_d(const u32* __restrict__ rank_list, const i64* __restrict__ part_off,
                                                int logP, SlRecords rec, SlState S, AggPlan ap, DFields fd, i64 T,
                                                i64 send_size, i64 send_base, SlRows rows, unsigned char* flags) {
    // KL key lanes per wave (one key each when the partition has <= KL local keys): few lanes keep
    // the divergence of the per-key chains low, and the small LDS footprint (≈ 11 KB) lets many
    // waves share a CU, which is what hides each chain's instruction latency
    constexpr int KL = kSlKeyLanes;
    constexpr int CH = SH_SL_CH;
    __shared__ u32 ch_rank[CH];
    __shared__ u32 ch_slot[CH];
    __shared__ unsigned short list[CH];
    __shared__ i64 ch_clk[CH];
    __shared__ i64 ch_pm[CH];
    __shared__ i64 ch_ts[CH];
    __shared__ u32 ch_raw[CH];
    __shared__ u64 ch_v[CH];
    __shared__ u32 run[64];
    __shared__ i64 hb_pm[KL * kHb];
    __shared__ u64 hb_v[KL * kHb];
    __shared__ u64 dq_min[KL * kDqL];
    __shared__ u64 dq_max[KL * kDqL];
    const int lane = threadIdx.x;
    const int kl = lane & (KL - 1);
    u64* lmin = dq_min + kl * kDqL;
    u64* lmax = dq_max + kl * kDqL;
    const i64 lo = part_off[blockIdx.x], hi = part_off[blockIdx.x + 1];
    const i64 gm = S.rc - 1;
    // lane state
    u32 K = kNoPos;
    i64 cnt = 0, rh = 0, rlen = 0, cur_send = 0, cur_first = 0, hb_base = 0;
    int hb_n = 0;
    u64 sum = 0;
    DDeque qn{}, qx{};
    u64* gmin = nullptr;
    u64* gmax = nullptr;
    auto store_key = [&]() {
        S.cnt[K] = cnt;
        S.rhead[K] = rh;
        S.rlen[K] = rlen;
        S.cur_send[K] = cur_send;
        S.cur_first[K] = cur_first;
        if (HSUM) {
            if (fd.sum >= 0) S.f[(size_t)fd.sum * S.nslots + K] = sum;
            if (fd.avg >= 0) S.f[(size_t)fd.avg * S.nslots + K] = sum;
        }
        if (HMIN) dd_store(qn, S, fd.mn, K, lmin);
        if (HMAX) dd_store(qx, S, fd.mx, K, lmax);
    };
    for (i64 c0 = lo; c0 < hi; c0 += CH) {
        const int n = (int)min<i64>(CH, hi - c0);
        u32 mine, start;
        sl_chunk_split<KL, true>(rank_list, rec.slot, c0, n, logP, ch_rank, ch_slot, list, run, mine, start);
        // each thread fetches the fields of the records whose rank it staged in the split
#pragma unroll 4
        for (int g = 0; g < CH; g += 64) {
            const int j = g + lane;
            if (j < n) {
                const u32 rk = ch_rank[j];
                ch_clk[j] = rec.clock[rk];
                ch_pm[j] = rec.pm[rk];
                ch_ts[j] = rec.ts[rk];
                ch_raw[j] = rec.raw[rk];
                ch_v[j] = rec.vals[rk];
            }
        }
        __syncthreads();
        for (u32 i = 0; i < mine; i++) {
            const int j = list[start + i];
            const u32 r = ch_rank[j], k = ch_slot[j];
            const i64 clk = ch_clk[j], pmr = ch_pm[j], tsr = ch_ts[j];
            const u32 raw = ch_raw[j];
            const u64 x = ch_v[j];
            if (k != K) {
                if (K != kNoPos) store_key();
                K = k;
                cnt = S.cnt[k];
                rh = S.rhead[k];
                rlen = S.rlen[k];
                cur_send = S.cur_send[k];
                cur_first = S.cur_first[k];
                hb_n = 0;
                if (HSUM) sum = S.f[(size_t)(fd.sum >= 0 ? fd.sum : fd.avg) * S.nslots + k];
                if (HMIN) { dd_load(qn, S, fd.mn, k, lmin); gmin = S.dq + ((size_t)fd.mn * S.nslots + k) * S.rc; }
                if (HMAX) { dd_load(qx, S, fd.mx, k, lmax); gmax = S.dq + ((size_t)fd.mx * S.nslots + k) * S.rc; }
            }
            // lazy expiry: ring head events with PM + T <= clock (TimeWindowProcessor.java:132-169)
            while (rlen > 0) {
                if (!(rh >= hb_base && rh < hb_base + hb_n)) {  // refill the head cache
                    const int m = (int)min<i64>(kHb, rlen);
                    i64 pm8[kHb];
                    u64 v8[kHb];
#pragma unroll
                    for (int e = 0; e < kHb; e++) {
                        if (e < m) {
                            const i64 sl = (rh + e) & gm;
                            pm8[e] = S.rpm[(size_t)k * S.rc + sl];
                            v8[e] = S.rval[(size_t)k * S.rc + sl];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < kHb; e++)
                        if (e < m) { hb_pm[kl * kHb + e] = pm8[e]; hb_v[kl * kHb + e] = v8[e]; }
                    hb_base = rh;
                    hb_n = m;
                }
                const int e = (int)(rh - hb_base);
                if (hb_pm[kl * kHb + e] + T > clk) break;
                const u64 y = hb_v[kl * kHb + e];
                cnt--;
                if (HSUM) {
                    double rr = __longlong_as_double((i64)sum) - __longlong_as_double((i64)y);
                    if (cnt == 0 && rr == 0.0) rr = 0.0;  // destroyed state restarts from +0.0
                    sum = (u64)__double_as_longlong(rr);
                }
                if (HMIN) dd_remove<true>(qn, gmin, gm, lmin, y);
                if (HMAX) dd_remove<false>(qx, gmax, gm, lmax, y);
                rh++;
                rlen--;
            }
            // the event joins the ring and the aggregators
            const i64 sl = (rh + rlen) & gm;
            S.rpm[(size_t)k * S.rc + sl] = pmr;
            S.rval[(size_t)k * S.rc + sl] = x;
            rlen++;
            cnt++;
            if (HSUM) sum = (u64)__double_as_longlong(__longlong_as_double((i64)sum) + __longlong_as_double((i64)x));
            if (HMIN) dd_add<true>(qn, gmin, gm, lmin, x);
            if (HMAX) dd_add<false>(qx, gmax, gm, lmax, x);
            // output row of (send, key): first occurrence position, last event's values
            const i64 send = send_base + (send_size > 0 ? (i64)raw / send_size : 0);
            i64 first;
            if (cur_send != send) { cur_send = send; cur_first = r; first = r; flags[r] = 1; }
            else first = cur_first;
            rows.ts[first] = tsr;
            rows.rep[first] = raw;
            rows.slot[first] = k;
            rows.send[first] = send;
            rows.clock[first] = clk;
            for (int a = 0; a < ap.n; a++) {
                const int kind = ap.kind[a];
                u64 o = 0;
                unsigned char nl = 0;
                if (kind == AK_COUNT) o = (u64)cnt;
                else if (kind == AK_SUM_D) o = sum;
                else if (kind == AK_AVG) o = (u64)__double_as_longlong(__longlong_as_double((i64)sum) / (double)cnt);
                else if (kind == AK_MIN_D) { o = qn.mm; nl = qn.mmh ? 0 : 1; }
                else { o = qx.mm; nl = qx.mmh ? 0 : 1; }
                rows.vals[(size_t)a * rows.cap + first] = o;
                rows.nulls[(size_t)a * rows.cap + first] = nl;
            }
        }
        __syncthreads();
    }
    if (K != kNoPos) store_key();
}

template <int NA, int NV>
__global__ __launch_bounds__(64) void k_sl_own(const u32* __restrict__ rank_list, const i64* __restrict__ part_off,
                                              int logP, SlRecords rec, SlState S, AggPlan ap, i64 T, i64 send_size,
                                              i64 send_base, SlRows rows, unsigned char* flags) {
    __shared__ u32 ch_rank[kSlCh];
    __shared__ u32 ch_slot[kSlCh];
    __shared__ unsigned short list[kSlCh];
    __shared__ u32 run[64];
    __shared__ i64 hb_pm[64 * kHb];
    __shared__ u64 hb_v[NV * 64 * kHb];
    extern __shared__ __attribute__((aligned(16))) u64 lds_dq[];  // [min/max aggregator][lane][kDqL]
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    const u64 lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const i64 lo = part_off[p], hi = part_off[p + 1];
    int mmi[NA];
    {
        int c = 0;
#pragma unroll
        for (int a = 0; a < NA; a++) {
            mmi[a] = c;
            if (a < ap.n && is_mm(ap.kind[a])) c++;
        }
    }
    LaneKey<NA, NV> L;
    L.k = kNoPos;
    L.hvalid = false;
    L.hb_n = 0;
    L.hb_base = 0;
    for (i64 c0 = lo; c0 < hi; c0 += kSlCh) {
        const int n = (int)min<i64>(kSlCh, hi - c0);
        // per-lane counts of the chunk
        u32 mine = 0;
        for (int g = 0; g < n; g += 64) {
            const int j = g + lane;
            u32 o = 64;
            if (j < n) {
                const u32 r = rank_list[c0 + j];
                const u32 k = rec.slot[c0 + j];
                o = (k >> logP) & 63;
                ch_rank[j] = r;
                ch_slot[j] = k;
            }
            // how many of this group's records go to my lane
            u64 mask = __ballot(j < n);
#pragma unroll
            for (int bt = 0; bt < 6; bt++) {
                const u64 b = __ballot((o >> bt) & 1);
                mask &= ((lane >> bt) & 1) ? b : ~b;
            }
            mine += (u32)__popcll(mask);
        }
        // exclusive scan of the lane counts -> list starts
        u32 incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        const u32 start = incl - mine;
        run[lane] = start;
        __syncthreads();
        // stable placement: rank among the group's same-owner records + that owner's running count
        for (int g = 0; g < n; g += 64) {
            const int j = g + lane;
            const bool ok = j < n;
            const u32 o = ok ? ((ch_slot[j] >> logP) & 63) : 0;
            u64 peers = __ballot(ok);
#pragma unroll
            for (int bt = 0; bt < 6; bt++) {
                const bool bit = (o >> bt) & 1;
                const u64 b = __ballot(bit);
                peers &= bit ? b : ~b;
            }
            const u32 lr = (u32)__popcll(peers & lt_mask);
            u32 base = 0;
            if (ok) base = run[o];
            __syncthreads();
            if (ok) list[base + lr] = (unsigned short)j;
            if (ok && lr == 0) run[o] = base + (u32)__popcll(peers);
            __syncthreads();
        }
        // replay: my key's events in order, the next record's fields loaded one step ahead
        SlRec<NV> nx;
        if (mine > 0) sl_rec_load(nx, rec, ap, c0 + list[start]);
        for (u32 i = 0; i < mine; i++) {
            const int j = list[start + i];
            const u32 r = ch_rank[j], k = ch_slot[j];
            const SlRec<NV> cur = nx;
            if (i + 1 < mine) sl_rec_load(nx, rec, ap, c0 + list[start + i + 1]);
            if (k != L.k) {
                if (L.k != kNoPos) lk_store(L, S, ap, lds_dq, mmi);
                lk_load(L, S, ap, lds_dq, mmi, k);
            }
            const i64 clk = cur.clk;
            // lazy expiry: ring head events with PM + T <= clock (TimeWindowProcessor.java:132-169)
            while (L.rlen > 0) {
                if (!L.hvalid) lk_head(L, S, ap, hb_pm, hb_v);
                if (L.hpm + T > clk) break;
                lk_remove(L, S, ap, lds_dq, mmi, L.hval);
                L.rh++;
                L.rlen--;
                L.hvalid = false;
                if (L.rlen > 0) lk_head(L, S, ap, hb_pm, hb_v);
            }
            // the event joins the ring and the aggregators
            const i64 sl = (L.rh + L.rlen) & (S.rc - 1);
            S.rpm[(size_t)k * S.rc + sl] = cur.pm;
#pragma unroll
            for (int q = 0; q < NV; q++) {
                if (q >= ap.n_vcols) break;
                S.rval[((size_t)q * S.nslots + k) * S.rc + sl] = cur.v[q];
            }
            if (L.rlen == 0) {
                L.hpm = cur.pm;
#pragma unroll
                for (int q = 0; q < NV; q++) {
                    if (q >= ap.n_vcols) break;
                    L.hval[q] = cur.v[q];
                }
                L.hvalid = true;
            }
            L.rlen++;
            lk_add(L, S, ap, lds_dq, mmi, cur.v);
            // output row of (send, key): first occurrence position, last event's values
            const i64 send = send_base + (send_size > 0 ? (i64)cur.raw / send_size : 0);
            i64 first;
            if (L.cur_send != send) { L.cur_send = send; L.cur_first = r; first = r; flags[r] = 1; }
            else first = L.cur_first;
            rows.ts[first] = cur.ts;
            rows.rep[first] = cur.raw;
            rows.slot[first] = k;
            rows.send[first] = send;
            rows.clock[first] = clk;
            const i64 c = L.cnt;
#pragma unroll
            for (int a = 0; a < NA; a++) {
                if (a >= ap.n) break;
                const int kind = ap.kind[a];
                u64 o;
                unsigned char nl = 0;
                if (kind == AK_COUNT) o = (u64)c;
                else if (kind == AK_SUM_L || kind == AK_SUM_D) o = L.f[a];
                else if (kind == AK_AVG) o = (u64)__double_as_longlong(__longlong_as_double((i64)L.f[a]) / (double)c);
                else { o = L.mm[a]; nl = L.mmh[a] ? 0 : 1; }
                rows.vals[(size_t)a * rows.cap + first] = o;
                rows.nulls[(size_t)a * rows.cap + first] = nl;
            }
        }
        __syncthreads();
    }
    if (L.k != kNoPos) lk_store(L, S, ap, lds_dq, mmi);
}

// rank-indexed records -> partition order (position q of the multisplit's rank list), so the
// per-key replay reads each partition's records from one contiguous range
__global__ __launch_bounds__(kBlock) void k_sl_gather(const u32* __restrict__ ranks, i64 M, SlRecords rec, SlRecords out,
                                                     int nv) {
    const i64 q = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (q >= M) return;
    const u32 r = ranks[q];
    out.raw[q] = rec.raw[r];
    out.slot[q] = rec.slot[r];
    out.clock[q] = rec.clock[r];
    out.pm[q] = rec.pm[r];
    out.ts[q] = rec.ts[r];
    for (int j = 0; j < nv; j++) out.vals[(size_t)j * out.cap + q] = rec.vals[(size_t)j * rec.cap + r];
}

void launch_sl_gather(hipStream_t s, const u32* ranks, i64 M, SlRecords rec, SlRecords out, int nv) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k_sl_gather, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ranks, M, rec, out,
                       nv);
}

// keys a key partition should hold so that every key gets a lane of its own in the replay kernel
// (k_sl_own_d: kSlKeyLanes per wave; k_sl_own: 64). A lane owning several keys switches per-key
// state (global loads and stores) whenever consecutive records of its list change key.
int sliding_keys_per_partition(AggPlan ap) {
    DFields fd;
    return own_d_fields(ap, fd) ? kSlKeyLanes : 64;
}

void launch_sliding_own(hipStream_t s, const u32* rank_list, const i64* part_off, int P, int logP, SlRecords rec,
                        SlState S, AggPlan ap, i64 T, i64 send_size, i64 send_base, SlRows rows,
                        unsigned char* flags, SlRecords rec_by_rank) {
    {
        DFields fd;
        const bool ok = own_d_fields(ap, fd);
        if (ok) {
            for_agg_shape(fd, [&](auto HS, auto HN, auto HX) {
                hipLaunchKernelGGL((k_sl_own_d<HS.value, HN.value, HX.value>), dim3(P), dim3(64), 0, s, rank_list,
                                   part_off, logP, rec_by_rank, S, ap, fd, T, send_size, send_base, rows, flags);
            });
            return;
        }
    }
    int n_mm = 0;
    for (int a = 0; a < ap.n; a++) n_mm += ap.kind[a] >= AK_MIN_L;
    const size_t lds = (size_t)std::max(1, n_mm) * 64 * kDqL * 8;
#define SH_SL_OWN(A, V)                                                                                        \
    hipLaunchKernelGGL((k_sl_own<A, V>), dim3(P), dim3(64), lds, s, rank_list, part_off, logP, rec, S, ap, T, \
                       send_size, send_base, rows, flags)
    const int nv = std::max(1, ap.n_vcols);
    if (ap.n <= 2 && nv <= 1) SH_SL_OWN(2, 1);
    else if (ap.n <= 4 && nv <= 1) SH_SL_OWN(4, 1);
    else if (ap.n <= 4 && nv <= 2) SH_SL_OWN(4, 2);
    else if (nv <= 2) SH_SL_OWN(8, 2);
    else SH_SL_OWN(8, 8);
#undef SH_SL_OWN
}

// ------------------------------------------------------------------------------------------------
// emit: flagged ranks -> output rows in rank order; flush starts where the send changes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sl_emit(const unsigned char* __restrict__ flags, i64 n,
                                                   const i64* __restrict__ blk_pre, SlRows rows, int n_aggs,
                                                   KeyTable kt, KeyPlan kp, i64 out_cap, i64* out_ts, i64* out_keys,
                                                   u64* out_vals, unsigned char* out_nulls, i64* out_send,
                                                   i64* out_clock, const u32* __restrict__ rank_raw, i64 raw_base,
                                                   i64* out_order, const i64* __restrict__ clock_by_rank,
                                                   i64* out_rep) {
    // striped over the tile (round it: elements tile + it * kBlock + lane), so every row read and
    // every output column store of a wave is one contiguous run; the tile's first output row is
    // blk_pre (k_count_flags counts whole tiles, whatever the order inside)
    const i64 tile = (i64)blockIdx.x * kTile;
    i64 run = blk_pre[blockIdx.x];
    for (int it = 0; it < kItems; it++) {
        const i64 j = tile + (i64)it * kBlock + threadIdx.x;
        const i64 fl = j < n ? flags[j] : 0;
        i64 tot;
        const i64 r = run + block_excl_scan(fl, SumOp(), 0, &tot);
        run += tot;
        if (!fl) continue;
        out_ts[r] = rows.ts[j];
        unpack_key(kp, slot_key(kt, rows.slot[j]), out_keys + r, out_cap);
        for (int a = 0; a < n_aggs; a++) {
            out_vals[(size_t)a * out_cap + r] = rows.vals[(size_t)a * rows.cap + j];
            out_nulls[(size_t)a * out_cap + r] = rows.nulls[(size_t)a * rows.cap + j];
        }
        out_send[r] = rows.send[j];
        out_clock[r] = clock_by_rank ? clock_by_rank[j] : rows.clock[j];
        if (out_order) out_order[r] = raw_base + (i64)rank_raw[j];
        out_rep[r] = raw_base + (i64)rows.rep[j];
    }
}

__global__ __launch_bounds__(kBlock) void k_flush_starts(const i64* __restrict__ out_send, i64 n, i64* blk_cnt) {
    i64 base = (i64)blockIdx.x * kTile + (i64)threadIdx.x * kItems;
    i64 c = 0;
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        i64 r = base + i;
        if (r < n && (r == 0 || out_send[r] != out_send[r - 1])) c++;
    }
    i64 t = block_reduce(c, SumOp(), 0);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = t;
}

__global__ __launch_bounds__(kBlock) void k_flush_write(const i64* __restrict__ out_send, const i64* __restrict__ out_clock,
                                                       i64 n, const i64* blk_pre, i64* flush_off, i64* flush_clock) {
    i64 base = (i64)blockIdx.x * kTile + (i64)threadIdx.x * kItems;
    i64 c = 0;
    bool st[kItems];
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        i64 r = base + i;
        st[i] = r < n && (r == 0 || out_send[r] != out_send[r - 1]);
        c += st[i];
    }
    i64 f = block_excl_scan(c, SumOp(), 0, nullptr) + blk_pre[blockIdx.x];
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        if (!st[i]) continue;
        flush_off[f] = base + i;
        flush_clock[f] = out_clock[base + i];
        f++;
    }
}

void launch_sl_emit(hipStream_t s, const unsigned char* flags, i64 n, const i64* blk_pre, int nblk, SlRows rows,
                    int n_aggs, KeyTable kt, KeyPlan kp, i64 out_cap, i64* out_ts, i64* out_keys, u64* out_vals,
                    unsigned char* out_nulls, i64* out_send, i64* out_clock, const u32* rank_raw, i64 raw_base,
                    i64* out_order, const i64* clock_by_rank, i64* out_rep) {
    hipLaunchKernelGGL(k_sl_emit, dim3(nblk), dim3(kBlock), 0, s, flags, n, blk_pre, rows, n_aggs, kt, kp, out_cap,
                       out_ts, out_keys, out_vals, out_nulls, out_send, out_clock, rank_raw, raw_base, out_order,
                       clock_by_rank, out_rep);
}

void launch_flush_starts(hipStream_t s, const i64* out_send, i64 n_rows, i64* blk_cnt, int nb) {
    hipLaunchKernelGGL(k_flush_starts, dim3(nb), dim3(kBlock), 0, s, out_send, n_rows, blk_cnt);
}

__global__ __launch_bounds__(kBlock) void k_iota_i64(i64* a, i64 n) {
    const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) a[i] = i;
}

void launch_iota_i64(hipStream_t s, i64* a, i64 n) {
    if (n > 0) hipLaunchKernelGGL(k_iota_i64, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, n);
}

void launch_flush_write(hipStream_t s, const i64* out_send, const i64* out_clock, i64 n_rows, const i64* blk_pre,
                        int nb, i64* flush_off, i64* flush_clock) {
    hipLaunchKernelGGL(k_flush_write, dim3(nb), dim3(kBlock), 0, s, out_send, out_clock, n_rows, blk_pre, flush_off,
                       flush_clock);
}

// grow the per-key rings / deques to a new capacity (power of two), preserving contents
__global__ void k_sl_regrow(const u64* old_buf, u64* new_buf, const i64* head, const i64* len, i64 nslots, int nsub,
                            i64 old_rc, i64 new_rc, const i64* hsel) {
    // one thread per (sub-array, slot): copies len elements starting at head into [0, len)
    i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nslots * nsub) return;
    i64 k = t % nslots;
    i64 h = head[hsel ? (t) : k], l = len[hsel ? (t) : k];
    const u64* src = old_buf + (size_t)t * old_rc;
    u64* dst = new_buf + (size_t)t * new_rc;
    for (i64 i = 0; i < l; i++) dst[i] = src[(h + i) & (old_rc - 1)];
}

void launch_sl_regrow(hipStream_t s, const u64* old_buf, u64* new_buf, const i64* head, const i64* len, i64 nslots,
                      int nsub, i64 old_rc, i64 new_rc, bool per_sub) {
    i64 n = nslots * nsub;
    if (n == 0) return;
    hipLaunchKernelGGL(k_sl_regrow, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, old_buf, new_buf, head, len,
                       nslots, nsub, old_rc, new_rc, per_sub ? head : nullptr);
}


// ---- key-table rebuild of a sliding window (sh_sliding.cpp sliding_rekey): a key whose window holds
// no event that can still be in it for any later event (last ring entry's PM + T <= the clock every
// later record carries at least) is in the state the reference destroys (canDestroy): it is dropped;
// the live keys move to a fresh table and their state follows them to the new slots --------------------
__global__ __launch_bounds__(kBlock) void k_sl_rekey_map(i64 size, KeyTable old_kt, KeyTable new_kt,
                                                        const i64* __restrict__ rhead, const i64* __restrict__ rlen,
                                                        const i64* __restrict__ rpm, i64 rc, i64 T, i64 bound,
                                                        u32* map) {
    const i64 s = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (s > size) return;
    if (s == size) { map[s] = (u32)size; return; }  // the spare slot keeps its place
    map[s] = 0xFFFFFFFFu;
    const u64 key = old_kt.keys[s];
    if (key == kEmptyKey) return;
    const i64 n = rlen[s];
    if (n <= 0) return;
    const i64 last_pm = rpm[(size_t)s * rc + ((rhead[s] + n - 1) & (rc - 1))];
    if (last_pm + T <= bound) return;
    map[s] = key_slot(new_kt, key);
}

// dst[o][map[s]][.] = src[o][s][.] for live slots (unit-sized words; rings keep their head offsets)
__global__ __launch_bounds__(kBlock) void k_sl_rekey_copy(const unsigned char* __restrict__ src, unsigned char* dst,
                                                         i64 outer, i64 n, i64 inner, int unit,
                                                         const u32* __restrict__ map) {
    const i64 per = inner / unit;
    const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= outer * n * per) return;
    const i64 w = i % per, sl = (i / per) % n, o = i / (per * n);
    const u32 to = map[sl];
    if (to == 0xFFFFFFFFu) return;
    const size_t from_off = ((size_t)o * n + sl) * inner + (size_t)w * unit;
    const size_t to_off = ((size_t)o * n + to) * inner + (size_t)w * unit;
    if (unit == 8) *(u64*)(dst + to_off) = *(const u64*)(src + from_off);
    else dst[to_off] = src[from_off];
}

void launch_sl_rekey_map(hipStream_t s, i64 size, KeyTable old_kt, KeyTable new_kt, const i64* rhead, const i64* rlen,
                         const i64* rpm, i64 rc, i64 T, i64 bound, u32* map) {
    hipLaunchKernelGGL(k_sl_rekey_map, dim3((unsigned)((size + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, size,
                       old_kt, new_kt, rhead, rlen, rpm, rc, T, bound, map);
}

void launch_sl_rekey_copy(hipStream_t s, const void* src, void* dst, i64 outer, i64 n, i64 inner, const u32* map) {
    const int unit = inner % 8 == 0 ? 8 : 1;
    const i64 total = outer * n * (inner / unit);
    if (total <= 0) return;
    hipLaunchKernelGGL(k_sl_rekey_copy, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       (const unsigned char*)src, (unsigned char*)dst, outer, n, inner, unit, map);
}
}  // namespace shd
