// sh_sliding_wkey.hip — the keyed replay of the sliding `#window.time(T)` group-by path on gfx950: current
// rows of the count / sum / avg / min / max-of-one-double shape, one wave per key (k_sl_wkey), and their
// emission. What it shares with the expired / all-events replay (k_slx_wkey) is in sh_sliding_wave.h.
#include "sh_sliding_wave.h"

namespace shd {

// ---- key-sorted replay: the records of a push sorted stably by key slot (sh_sort.hip), so each key's
// events form one contiguous run in event order, walked by one wave per key (k_sl_wkey). The key's
// window is its carried ring (events of earlier pushes) followed by the run itself; only the entries
// still in the window at the end of the push go to the ring. Rows are written in key order as one record
// each (full-line stores) and put in stream order by the emit kernel. ------------------------------------
// resident waves per SIMD k_sl_wkey is compiled for: 4 (the full instantiation takes all 128 VGPRs, without
// spill: profiles/sliding_wave_core_resources_after.txt; left alone the compiler took 131 and 3 waves: C3
// 8.29 -> 7.53 ms per push, r05_wpe; 5 spills 412 bytes and runs 3x slower); timing experiments override it
#ifndef SH_WK_WPE
#define SH_WK_WPE 4
#endif
#define SH_WK_ATTR __attribute__((amdgpu_waves_per_eu(SH_WK_WPE)))
constexpr u32 kFirstBit = 0x80000000u;

__global__ void k_sl_keyoff(const u32* __restrict__ slot_cnt, i64 nslots, u32* key_off) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= nslots) key_off[k] = k < nslots ? slot_cnt[k] : 0u;
}

// ---- one wave per key (round 3): the 64 lanes of a wave share one key's run, 64 records at a time.
// Everything per record that does not depend on the running aggregates is computed lane-parallel:
// the expiry prefix (the heads with PM + T <= the record's clock form a prefix, PM and the clock both
// being non-decreasing along a key's events — one binary search per lane over the staged heads), the
// count, the row position and the row stores. The Java-order double sum runs sequentially, by the whole
// wave in lockstep on wave-uniform state, reading the records' values and expiry points from the lanes'
// registers (readlane). With a wave per key a SIMD holds several keys' waves, whose sequential parts
// interleave. TimeWindowProcessor.java:132-169; QuerySelector.processInBatchGroupBy :315-374.
//
// Min / max off the sequential chain (round 4). MinAttributeAggregatorExecutor (:187-236) keeps a
// LinkedList deque: processAdd pops the back while it is strictly worse, processRemove calls
// removeFirstOccurrence(value) and reads the front. The expiring event is the window's oldest, so when it
// is in the deque it is the front and leaves; the result differs from the window's true minimum only if
// it was popped earlier and a bit-equal value sits in the deque (the reference's quirk), or once a NaN
// breaks the order. While neither can happen the deque after every event is the monotone deque of the
// window and minValue is the window's range minimum (the older entry on ties, which the front and the
// strict `minValue > value` both keep). So per chunk the lanes check that no expiring head meets a
// bit-equal value among the deque (entries carry their window index) or the chunk's records and that no
// NaN is in sight, then compute each record's result in parallel: the first deque entry at or after the
// record's first unexpired head, against the leftmost best of the chunk's records in its window. The
// deque after the chunk is the old entries still unexpired and not worse than the chunk's best, then the
// chunk's suffix bests. A chunk that fails the check or would outgrow the LDS ring runs the sequential
// deque (kdq_*), and its key stays sequential for the rest of the push (the indices are not kept there).
constexpr int kWS = 128;  // window-head entries staged per chunk (two per lane)

// The records are read in key order through the sort's rank list from the 48-byte records
// (SlRecords.aos); the lanes write the key-order (PM, value) columns the window-head reads use, and
// the first-record flags / key-order positions the emit needs.
template <bool HSUM, bool HMIN, bool HMAX>
__global__ __launch_bounds__(64) SH_WK_ATTR void k_sl_wkey(const u32* __restrict__ key_off, u32 nslots, i64* __restrict__ g_pm,
                                               u64* __restrict__ g_v, SlState S, DFields fd, KOut ko, i64 T,
                                               u32 send_size, i64 send_base, u64* __restrict__ rowsK, int RW,
                                               const u32* __restrict__ sorted_rank, const u64* __restrict__ aos,
                                               unsigned char* __restrict__ flags) {
    __shared__ u64 dq_min[HMIN ? kDqK : 1];
    __shared__ u64 dq_max[HMAX ? kDqK : 1];
    __shared__ int di_min[HMIN ? kDqK : 1];
    __shared__ int di_max[HMAX ? kDqK : 1];
    __shared__ i64 s_pm[kWS];
    __shared__ u64 s_x[64];
    // the order-dependent sum chain of a chunk as one operation list (kWS removes + 64 adds at most)
    __shared__ u64 s_op[kWS + 64];
    __shared__ int s_lo[64];
    __shared__ unsigned char s_fl[kWS + 64];
    __shared__ u32 s_bf[kBfWords];
    const u32 k = blockIdx.x;
    const int lane = threadIdx.x;
    if (k >= nslots) return;
    const u32 a = key_off[k], b = key_off[k + 1];
    if (a == b) return;
    const int gm = (int)(S.rc - 1);
    const i64* rpm = S.rpm + (size_t)k * S.rc;
    const u64* rval = S.rval + (size_t)k * S.rc;
    const int rh0 = (int)(S.rhead[k] & gm), H0 = (int)S.rlen[k];
    const int n = (int)(b - a), HN = H0 + n;
    // the records are read through the sort's rank list and the key-order PM / value columns written here
    // (a key-ordered copy of the records, tried in round 5, cost what it saved: r05_c3_kgather_*)
    auto run_pm = [&](u32 j) -> i64 { return g_pm[j]; };
    auto run_v = [&](u32 j) -> u64 { return g_v[j]; };
    auto head_pm = [&](int h) -> i64 { return h < H0 ? rpm[(rh0 + h) & gm] : run_pm(a + (u32)(h - H0)); };
    auto head_v = [&](int h) -> u64 { return h < H0 ? rval[(rh0 + h) & gm] : run_v(a + (u32)(h - H0)); };
    WkState w{};
    // (the parallel min / max needs the deque entries' window indices)
    bool par = wk_load<HSUM, HMIN, HMAX>(w, S, fd, k, rh0, H0, dq_min, dq_max, di_min, di_max, s_bf, lane);
    // (the running state under the names the replay uses)
    i64& cnt = w.cnt;
    double& sum = w.sum;
    KDq &qn = w.qn, &qx = w.qx;
    int hj = 0;         // heads expired so far
    int open_row = 0;   // key-order index of the (send, key) row open at the chunk start
    i64 last_send = 0;
    u32 prev_raw = 0;   // the previous chunk's last record
    for (int o0 = 0; o0 < n; o0 += 64) {
        const int m = min(64, n - o0);
        const bool in = lane < m;
        const u32 i = a + (u32)(o0 + min(lane, m - 1));
        i64 clk, ts;
        u64 x;
        u32 raw, rk;
        {
            const u32 r = sorted_rank[i];  // the record's stream rank
            const ulonglong2* rp = (const ulonglong2*)(aos + (size_t)r * kSlAosWords);
            const ulonglong2 w0 = rp[0], w1 = rp[1], w2 = rp[2];
            clk = (i64)w0.x;
            ts = (i64)w1.x;
            x = w1.y;
            raw = (u32)w2.x;
            // a record opens a row when it is its key's first of its send (every record per-event)
            u32 pr = __shfl_up(raw, 1, 64);
            if (lane == 0) pr = prev_raw;
            const bool fst = send_size == 1 || (o0 + lane == 0) || (send_size == 0 ? false : pr / send_size != raw / send_size);
            rk = r | (fst ? kFirstBit : 0u);
            if (in) {
                g_pm[i] = (i64)w0.y;  // the window-head columns, in key order
                g_v[i] = x;
                if (flags) flags[r] = fst ? 1 : 0;  // (per-event sends: every record opens its row, no flags)
            }
            s_x[lane] = x;
            prev_raw = __shfl(raw, m - 1, 64);
            __threadfence_block();  // this chunk's own records may expire within it
            __syncthreads();
        }
        const int hb = hj;
        // the next kWS window heads: PM in LDS (the lanes' binary searches), values in two registers
        // per lane (entry d in lane d & 63 of hv0 / hv1, read back with readlane by the sequential part)
        u64 hv0 = 0, hv1 = 0;
        if (hb + lane < HN) { s_pm[lane] = head_pm(hb + lane); hv0 = head_v(hb + lane); }
        if (hb + 64 + lane < HN) { s_pm[64 + lane] = head_pm(hb + 64 + lane); hv1 = head_v(hb + 64 + lane); }
        __syncthreads();
        // heads expired before this record: the first h in [hb, added) whose PM + T exceeds its clock
        int lo = hb, hi = in ? H0 + o0 + lane : hb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const i64 pm = mid - hb < kWS ? s_pm[mid - hb] : head_pm(mid);
            if (pm + T <= clk) lo = mid + 1;
            else hi = mid;
        }
        // the effective expiry point of each record: the running max over the earlier lanes
        int lo_eff = in ? lo : hb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(lo_eff, d, 64);
            if (lane >= d) lo_eff = max(lo_eff, up);
        }
        const int Sx = H0 + o0;  // window index of the chunk's first record
        u64 r_mn = 0, r_mx = 0;
        u32 r_fl = 0;
        bool pc = par;  // this chunk's min / max in parallel
        DqPlan pn{}, px{};
        bool sn = false, sx_ = false;
        if (pc) {
            const int lo_end = __builtin_amdgcn_readlane(lo_eff, m - 1);
            const int ne = lo_end - hb;
            pc = ne <= kWS && !__any(in && d_isnan(x));
            if (pc) {
                // the quirk check: an expiring head meeting a bit-equal value of another event among the
                // deque entries or the chunk's records
                bool dirty = false;
                // (the filter holds the chunk's records and the deques' entries)
                const u32 hx = bf_hash(x);
                const u32 hn = HMIN && lane < qn.len ? bf_hash(dq_min[(qn.h + lane) & (kDqK - 1)]) : 0u;
                const u32 hm = HMAX && lane < qx.len ? bf_hash(dq_max[(qx.h + lane) & (kDqK - 1)]) : 0u;
                if (in) atomicOr(&s_bf[hx >> 5], 1u << (hx & 31));
                if (HMIN && lane < qn.len) atomicOr(&s_bf[hn >> 5], 1u << (hn & 31));
                if (HMAX && lane < qx.len) atomicOr(&s_bf[hm >> 5], 1u << (hm & 31));
                __syncthreads();
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const int d = lane + 64 * t;
                    if (d >= ne) continue;
                    const u64 v = t ? hv1 : hv0;
                    const int idx = hb + d;
                    if (!bf_hit(s_bf, v)) continue;
                    if (HMIN) dirty |= dq_quirk(qn, dq_min, di_min, v, idx);
                    if (HMAX) dirty |= dq_quirk(qx, dq_max, di_max, v, idx);
                    for (int j = 0; j < m; j++) dirty |= s_x[j] == v && Sx + j != idx;
                }
                __syncthreads();
                // (after every lane's test)
                if (in) s_bf[hx >> 5] = 0;
                if (HMIN && lane < qn.len) s_bf[hn >> 5] = 0;
                if (HMAX && lane < qx.len) s_bf[hm >> 5] = 0;
                pc = !__any(dirty);
            }
            if (pc) {
                const bool from0 = !__any(in && lo_eff > Sx);
                if (HMIN) r_mn = par_best<true>(qn, dq_min, di_min, s_x, x, lo_eff, Sx, from0, lane);
                if (HMAX) r_mx = par_best<false>(qx, dq_max, di_max, s_x, x, lo_eff, Sx, from0, lane);
                if (HMIN) pn = dq_plan<true>(qn, dq_min, di_min, x, in, Sx, lo_end, lane, sn);
                if (HMAX) px = dq_plan<false>(qx, dq_max, di_max, x, in, Sx, lo_end, lane, sx_);
                pc = (!HMIN || pn.i1 - pn.i0 + pn.n_new <= kDqK) && (!HMAX || px.i1 - px.i0 + px.n_new <= kDqK);
            }
            if (pc) {
                if (HMIN) dq_commit<true>(qn, dq_min, di_min, pn, x, sn, Sx, lane, rl64(r_mn, m - 1));
                if (HMAX) dq_commit<false>(qx, dq_max, di_max, px, x, sx_, Sx, lane, rl64(r_mx, m - 1));
                r_fl = 3;
            } else {
                par = false;  // the sequential deque takes over for the rest of the push
            }
        }
        // The order-dependent part, run by the whole wave in lockstep on wave-uniform values (so the
        // compiler keeps the running state scalar): each record's expiry point and value, and the
        // expiring heads' values, come from other lanes' registers by readlane instead of LDS, and
        // record q's results land in lane q's registers (a select, no LDS store).
        i64 r_cnt = 0;
        u64 r_sum = 0;
        // Fast chain: with the min / max handled in parallel (or none), what stays sequential is the
        // Java-order double sum. Record q's removes are the heads [lo_eff(q-1), lo_eff(q)) and its add
        // follows them, so every operation's place in the chunk's list is known in parallel: add q at
        // (lo_eff(q) - hb) + q, head d at d + #{q : lo_eff(q) <= hb + d}. The lanes write the values
        // (a remove as the negated value: a - b is a + (-b) exactly in IEEE 754), the counts are
        // closed-form, and the wave then only adds the list up in order, reading it from LDS with a
        // uniform address (no readlane per value), capturing the running sum after each add.
        const int R = __builtin_amdgcn_readlane(lo_eff, m - 1) - hb;  // heads expiring in the chunk
        const bool fast = (pc || (!HMIN && !HMAX)) && R <= kWS;
        if (fast) {
            const int nops = R + m;
            if (in) s_lo[lane] = lo_eff;
            for (int j = lane; j < nops; j += 64) s_fl[j] = 0;
            __syncthreads();
            const int ap_q = (lo_eff - hb) + lane;  // this lane's add (lanes < m)
            if (in) {
                s_op[ap_q] = x;
                s_fl[ap_q] = 1;
            }
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int d = lane + 64 * t;
                if (d >= R) continue;
                // adds before head d: the records whose expiry point is at or below it
                int lo2 = 0, hi2 = m;
                while (lo2 < hi2) {
                    const int mid = (lo2 + hi2) >> 1;
                    if (s_lo[mid] <= hb + d) lo2 = mid + 1;
                    else hi2 = mid;
                }
                s_op[d + lo2] = (t ? hv1 : hv0) ^ 0x8000000000000000ull;  // -v
                // the count after this remove: zero -> the sum restarts from +0.0 (canDestroy)
                if (cnt + lo2 - (d + 1) == 0) s_fl[d + lo2] = 2;
            }
            __syncthreads();
            u64 czm[3];
#pragma unroll
            for (int wd = 0; wd < 3; wd++) {
                const int j = wd * 64 + lane;
                const unsigned char fv = j < nops ? s_fl[j] : 0;
                czm[wd] = __ballot(fv == 2);
            }
            // each lane keeps the running sum at its own add (position ap_q)
            if (HSUM) r_sum = wk_sum_chain(sum, s_op, nops, czm, in ? ap_q : -1);
            r_cnt = cnt + (lane + 1) - (lo_eff - hb);
            cnt = cnt + m - R;
            hj = hb + R;
            __syncthreads();  // (s_op / s_lo / s_fl are refilled by the next chunk)
        }
        if (!fast) {
            int h = hb;
            for (int q = 0; q < m; q++) {
                const int e = max(__builtin_amdgcn_readlane(lo, q), h);
                for (; h < e; h++) {  // expired heads leave, oldest first
                    const int d = h - hb;
                    const u64 v = d < 64 ? rl64(hv0, d) : d < kWS ? rl64(hv1, d - 64) : head_v(h);
                    wk_remove<HSUM, HMIN, HMAX>(w, dq_min, dq_max, v, !pc);
                }
                wk_add<HSUM, HMIN, HMAX>(w, dq_min, dq_max, rl64(x, q), !pc);  // the event joins the window
                if (lane == q) {
                    r_cnt = cnt;
                    r_sum = (u64)__double_as_longlong(sum);
                    if (!pc) {
                        r_mn = qn.mm;
                        r_mx = qx.mm;
                        r_fl = (qn.mmh ? 1u : 0u) | (qx.mmh ? 2u : 0u);
                    }
                }
            }
            hj = h;
        }
        // the row of (send, key): opened by the group's first record (its key-order position), written
        // with the values after the group's last record of this chunk (a later chunk overwrites it)
        const bool first = in && (rk & kFirstBit);
        int grp = first ? o0 + lane : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(grp, d, 64);
            if (lane >= d) grp = max(grp, up);
        }
        grp = max(grp, open_row);
        // (the shuffle runs on every lane: a lane may only read a lane that executes it)
        const u32 rk_next = __shfl_down(rk, 1, 64);
        const bool next_first = lane + 1 < m ? (rk_next & kFirstBit) != 0 : true;
        const i64 send = send_base + (send_size == 1 ? (i64)raw : send_size ? (i64)(raw / send_size) : 0);
        if (in && next_first) {
            u64 row[4 + SH_MAX_AGGS];
            row[0] = (u64)ts;
            row[1] = (u64)raw | ((u64)k << 32);
            row[2] = (u64)clk;
            // (the same packing as slx_row_values, sh_slx_kernels.hip, without its null-at-count-0 rule: a
            // row here follows a record's add, so the count is >= 1; a change to one belongs in both)
            u32 nulls = 0;
            const i64 c = r_cnt;
            const u64 sb = r_sum;
            const u32 fl = r_fl;
#pragma unroll
            for (int o = 0; o < SH_MAX_AGGS; o++) {
                if (o >= ko.n) break;
                const int src = ko.src[o];
                u64 v = 0;
                if (src == 0) v = (u64)c;
                else if (src == 1) v = sb;
                else if (src == 2) v = (u64)__double_as_longlong(__longlong_as_double((i64)sb) / (double)c);
                else if (src == 3) { v = r_mn; nulls |= ((fl & 1) ? 0u : 1u) << o; }
                else { v = r_mx; nulls |= ((fl & 2) ? 0u : 1u) << o; }
                row[4 + o] = v;
            }
            row[3] = (u64)send | ((u64)nulls << 56);
            // the row lands at the stream rank of its first record, so the emission reads the rows in
            // stream order (whole lines) instead of gathering them from key order
            const u32 row_rank = grp == o0 + lane ? (rk & ~kFirstBit)
                                 : sorted_rank[a + (u32)grp];
            ulonglong2* dst = (ulonglong2*)(rowsK + (size_t)row_rank * RW);
            if (!flags) {
                // per-event sends: every record's row follows its own add (count >= 1, no nulls) and the
                // emission takes ts / clock / event / slot from the stream-order records, so the row is
                // its values alone — half the bytes of the random stores (r05: 2.4 ms of the replay)
#pragma unroll
                for (int o = 0; o < SH_MAX_AGGS / 2; o++)
                    if (2 * o < RW) dst[o] = make_ulonglong2(row[4 + 2 * o], row[4 + 2 * o + 1]);
            } else {
#pragma unroll
                for (int o = 0; o < (4 + SH_MAX_AGGS) / 2; o++)
                    if (2 * o < RW) dst[o] = make_ulonglong2(row[2 * o], row[2 * o + 1]);
            }
        }
        open_row = __shfl(grp, m - 1, 64);
        last_send = __shfl(send, m - 1, 64);
        __syncthreads();  // the staging arrays are refilled by the next chunk
    }
    // the window after the push: heads [hj, HN) (the run's records from their key-order columns)
    wk_write_back<HSUM, HMIN, HMAX>(w, S, fd, k, rh0, H0, HN, hj, dq_min, dq_max, lane, [&](size_t sl, int j) {
        S.rpm[sl] = run_pm(a + (u32)j);
        S.rval[sl] = run_v(a + (u32)j);
    });
    if (lane == 0) {
        S.cur_send[k] = last_send;
        S.cur_first[k] = 0;
    }
}

// emit of the keyed replay: flagged ranks in stream order, each row read from its record at that rank
__global__ __launch_bounds__(kBlock) void k_slk_emit(const unsigned char* __restrict__ flags, i64 n,
                                                    const i64* __restrict__ blk_pre,
                                                    const u64* __restrict__ rowsK, int RW, int n_aggs, KeyTable kt,
                                                    KeyPlan kp, i64 out_cap, i64* out_ts, i64* out_keys, u64* out_vals,
                                                    unsigned char* out_nulls, i64* out_send, i64* out_clock,
                                                    const u32* __restrict__ rank_raw, i64 raw_base, i64* out_order,
                                                    i64* out_rep, const u64* __restrict__ aos,
                                                    const u32* __restrict__ rank_slot) {
    const i64 tile = (i64)blockIdx.x * kTile;
    if (!flags) {
        // per-event sends: row j is record j's (compact: values only); the rest from the record itself
        for (int it = 0; it < kItems; it++) {
            const i64 j = tile + (i64)it * kBlock + threadIdx.x;
            if (j >= n) continue;
            const ulonglong2* rp = (const ulonglong2*)(aos + (size_t)j * kSlAosWords);
            const ulonglong2 w0 = rp[0], w1 = rp[1], w2 = rp[2];
            const u64* src = rowsK + (size_t)j * RW;
            out_ts[j] = (i64)w1.x;
            unpack_key(kp, slot_key(kt, rank_slot[j]), out_keys + j, out_cap);
            for (int a = 0; a < n_aggs; a++) {
                out_vals[(size_t)a * out_cap + j] = src[a];
                out_nulls[(size_t)a * out_cap + j] = 0;
            }
            out_clock[j] = (i64)w0.x;
            if (out_order) out_order[j] = raw_base + (i64)rank_raw[j];
            out_rep[j] = raw_base + (i64)(u32)w2.x;
        }
        return;
    }
    i64 run = flags ? blk_pre[blockIdx.x] : tile;
    for (int it = 0; it < kItems; it++) {
        const i64 j = tile + (i64)it * kBlock + threadIdx.x;
        i64 r = j;
        if (flags) {
            const i64 fl = j < n ? flags[j] : 0;
            i64 tot;
            r = run + block_excl_scan(fl, SumOp(), 0, &tot);
            run += tot;
            if (!fl) continue;
        } else if (j >= n) {
            continue;  // (per-event sends: every record's rank holds a row)
        }
        const u64* src = rowsK + (size_t)j * RW;
        u64 w[4 + SH_MAX_AGGS];
#pragma unroll
        for (int o = 0; o < (4 + SH_MAX_AGGS) / 2; o++) {
            if (2 * o >= RW) break;
            const ulonglong2 v = ((const ulonglong2*)src)[o];
            w[2 * o] = v.x;
            w[2 * o + 1] = v.y;
        }
        out_ts[r] = (i64)w[0];
        unpack_key(kp, slot_key(kt, (u32)(w[1] >> 32)), out_keys + r, out_cap);
        const u32 nulls = (u32)(w[3] >> 56);
        for (int a = 0; a < n_aggs; a++) {
            out_vals[(size_t)a * out_cap + r] = w[4 + a];
            out_nulls[(size_t)a * out_cap + r] = (nulls >> a) & 1u;
        }
        if (out_send) out_send[r] = (i64)(w[3] & ((1ull << 56) - 1));  // (per-event sends: the flushes are the rows)
        out_clock[r] = (i64)w[2];
        if (out_order) out_order[r] = raw_base + (i64)rank_raw[j];
        out_rep[r] = raw_base + (i64)(u32)w[1];
    }
}

void launch_slk_emit(hipStream_t s, const unsigned char* flags, i64 n, const i64* blk_pre, int nblk,
                     const u64* rowsK, int RW, int n_aggs, KeyTable kt, KeyPlan kp, i64 out_cap, i64* out_ts,
                     i64* out_keys, u64* out_vals, unsigned char* out_nulls, i64* out_send, i64* out_clock,
                     const u32* rank_raw, i64 raw_base, i64* out_order, i64* out_rep, const u64* aos,
                     const u32* rank_slot) {
    hipLaunchKernelGGL(k_slk_emit, dim3(nblk), dim3(kBlock), 0, s, flags, n, blk_pre, rowsK, RW, n_aggs, kt, kp,
                       out_cap, out_ts, out_keys, out_vals, out_nulls, out_send, out_clock, rank_raw, raw_base,
                       out_order, out_rep, aos, rank_slot);
}

// The keyed replay is used where it measured faster than the key-partition replay (k_sl_own_d): with
// a min or max deque (C3's count/min/max/avg: 18.5 vs 20.7 ms per 16.7M-event push on MI355X);
// count/sum/avg alone stay on k_sl_own_d (5.5 vs 6.1 ms).
bool sliding_keyed_ok(AggPlan ap) {
    DFields fd;
    return own_d_fields(ap, fd) && ap.n <= SH_MAX_AGGS && (fd.mn >= 0 || fd.mx >= 0);
}

int sliding_keyed_row_words(int n_aggs, bool compact) { return compact ? (n_aggs + 1) & ~1 : (4 + n_aggs + 1) & ~1; }

void launch_sliding_keyed(hipStream_t s, const u32* slot_cnt, u32* key_off, i64* tmp, const u32* sorted_rank,
                          SlRecords rec, i64* g_pm, u64* g_v, SlState S, AggPlan ap, i64 T,
                          i64 send_size, i64 send_base, u64* rowsK, unsigned char* flags) {
    DFields fd;
    own_d_fields(ap, fd);
    const KOut ko = agg_outputs(ap);
    const i64 n = S.nslots;
    const u32 ss = send_size > 0 ? (u32)send_size : 0u;
    {
        hipLaunchKernelGGL(k_sl_keyoff, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, slot_cnt, n, key_off);
        launch_scan_sum_large_u32(s, key_off, n + 1, tmp);
    }
    const int RW = sliding_keyed_row_words(ap.n, flags == nullptr);
    // (callers come here with a min or a max, sliding_keyed_ok: the two instantiations without one are
    // compiled but never launched)
    for_agg_shape(fd, [&](auto HS, auto HN, auto HX) {
        hipLaunchKernelGGL((k_sl_wkey<HS.value, HN.value, HX.value>), dim3((unsigned)n), dim3(64), 0, s, key_off,
                           (u32)n, g_pm, g_v, S, fd, ko, T, ss, send_base, rowsK, RW, sorted_rank, rec.aos, flags);
    });
}

}  // namespace shd
