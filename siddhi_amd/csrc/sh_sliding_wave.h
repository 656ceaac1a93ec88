// sh_sliding_wave.h — device code shared by the wave-per-key sliding replays: k_sl_wkey (current rows,
// sh_sliding_wkey.hip) and k_slx_wkey (`insert expired / all events`, sh_slx_kernels.hip). Only .hip files
// include it. Its last section is the host side of their launches (and of k_sl_own_d's): the shape test,
// the output plan and the <sum, min, max> dispatch.
#pragma once
#include "sh_device.h"
#include "sh_sliding.h"
#include <type_traits>

namespace shd {

// The shape these replays (and k_sl_own_d) are specialised for: every aggregator is count or reads one
// DOUBLE column with sum / avg / min / max, each at most once (own_d_fields below).
struct DFields {
    int sum, avg, mn, mx;  // field index of each (-1: absent)
};

__device__ __forceinline__ bool d_eq(u64 a, u64 b) {
    const double x = __longlong_as_double((i64)a), y = __longlong_as_double((i64)b);
    return a == b || (x != x && y != y);
}

template <bool MIN>
__device__ __forceinline__ bool d_worse(u64 cur, u64 x) {
    const double c = __longlong_as_double((i64)cur), v = __longlong_as_double((i64)x);
    return MIN ? (c > v) : (c < v);
}

__device__ __forceinline__ bool d_isnan(u64 a) {
    const double x = __longlong_as_double((i64)a);
    return x != x;
}

constexpr int kDqK = 64;  // LDS min/max deque entries per lane (longer deques continue in global memory)

// Wait for this wave's vector-memory loads right where a rare path issued them. The replay step keeps
// the next step's loads and this step's row stores in flight; a load result that flows out of a
// rare branch would otherwise make the compiler wait for every outstanding vector-memory operation
// at the merge point, on every record, taken or not (the counter retires in order).
__device__ __forceinline__ void wait_vm_here() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // vmcnt(0)

// a lane's min or max deque (MinAttributeAggregatorExecutor's LinkedList with removeFirstOccurrence):
// ring `l` in LDS (kDqK entries, one ring per wave) or, once longer, ring `g` in global memory
struct KDq {
    int h, len;
    u64 f, b, mm;
    bool mmh, spill, nan;
};

// GLOBAL: the deque lives in its global ring; otherwise in LDS. Separate instances, so each uses plain
// LDS or global instructions (no pointer select)
template <bool MIN, bool GLOBAL>
__device__ __forceinline__ void kdq_remove_t(KDq& q, u64* g, int gm, u64* l, u64 x) {
    auto at = [&](int i) -> u64 {
        if (!GLOBAL) return l[i & (kDqK - 1)];
        const u64 v = g[i & gm];
        wait_vm_here();
        return v;
    };
    if (q.len > 0 && d_eq(q.f, x)) {
        q.h++;
        q.len--;
        if (q.len > 0) q.f = at(q.h);
    } else if (q.len > 1 && (q.nan || !d_worse<MIN>(x, q.b))) {
        int found = -1;
        if (!q.nan) {
            // NaN-free: the deque is monotone (min: non-decreasing), so the first entry not better
            // than x is found by bisection; x is present iff that entry equals it
            int lo = 1, hi = q.len;  // answer in [lo, hi]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (d_worse<MIN>(x, at(q.h + mid))) lo = mid + 1;
                else hi = mid;
            }
            // among numerically equal entries (0.0 / -0.0) Double.equals wants the same bits
            for (int i = lo; i < q.len; i++) {
                const u64 e = at(q.h + i);
                if (d_eq(e, x)) { found = i; break; }
                if (d_worse<MIN>(e, x)) break;  // past every entry equal to x
            }
        } else {
            for (int i = 1; i < q.len; i++)
                if (d_eq(at(q.h + i), x)) { found = i; break; }
        }
        if (found >= 0) {
            for (int i = found; i + 1 < q.len; i++) {
                const u64 v = at(q.h + i + 1);
                if (GLOBAL) g[(q.h + i) & gm] = v;
                else l[((q.h + i) & (kDqK - 1))] = v;
            }
            q.len--;
            q.b = at(q.h + q.len - 1);
        }
    }
    if (q.len > 0) { q.mm = q.f; q.mmh = true; }
    else { q.mmh = false; q.nan = q.spill; }
}

template <bool MIN>
__device__ __forceinline__ void kdq_remove(KDq& q, u64* g, int gm, u64* l, u64 x) {
    if (q.spill) kdq_remove_t<MIN, true>(q, g, gm, l, x);
    else kdq_remove_t<MIN, false>(q, g, gm, l, x);
}

template <bool MIN, bool GLOBAL>
__device__ __forceinline__ void kdq_pop_t(KDq& q, const u64* g, int gm, const u64* l, u64 x) {
    while (q.len > 0 && d_worse<MIN>(q.b, x)) {
        q.len--;
        if (q.len > 0) {
            if (GLOBAL) { q.b = g[(q.h + q.len - 1) & gm]; wait_vm_here(); }
            else q.b = l[((q.h + q.len - 1) & (kDqK - 1))];
        }
    }
}

template <bool MIN>
__device__ __forceinline__ void kdq_add(KDq& q, u64* g, int gm, u64* l, u64 x) {
    if (q.spill) kdq_pop_t<MIN, true>(q, g, gm, l, x);
    else kdq_pop_t<MIN, false>(q, g, gm, l, x);
    if (!q.spill && q.len == kDqK) {  // the LDS ring is full: the deque moves to its global ring
        for (int i = 0; i < q.len; i++) g[(q.h + i) & gm] = l[((q.h + i) & (kDqK - 1))];
        q.spill = true;
        q.nan = true;  // the global path always scans
    }
    if (q.spill) g[(q.h + q.len) & gm] = x;
    else l[((q.h + q.len) & (kDqK - 1))] = x;
    q.len++;
    q.b = x;
    q.nan |= d_isnan(x);
    if (q.len == 1) q.f = x;
    if (!q.mmh || d_worse<MIN>(q.mm, x)) { q.mm = x; q.mmh = true; }
}

__device__ __forceinline__ void kdq_load(KDq& q, const SlState& S, int field, u32 k, u64* l) {
    const size_t fi = (size_t)field * S.nslots + k;
    q.mm = S.mm[fi];
    q.mmh = S.mm_has[fi];
    q.len = (int)S.dq_len[fi];
    q.h = (int)(S.dq_head[fi] & (S.rc - 1));
    q.spill = q.len > kDqK;
    q.nan = q.spill;
    const u64* g = S.dq + fi * S.rc;
    const int gm = (int)(S.rc - 1);
    if (!q.spill) {
        for (int i = 0; i < q.len; i++) {
            const u64 v = g[(q.h + i) & gm];
            l[((q.h + i) & (kDqK - 1))] = v;
            q.nan |= d_isnan(v);
        }
    }
    if (q.len > 0) {
        q.f = g[q.h & gm];
        q.b = g[(q.h + q.len - 1) & gm];
    }
}

__device__ __forceinline__ void kdq_store(const KDq& q, const SlState& S, int field, u32 k, const u64* l) {
    const size_t fi = (size_t)field * S.nslots + k;
    S.mm[fi] = q.mm;
    S.mm_has[fi] = q.mmh;
    const int gm = (int)(S.rc - 1);
    S.dq_head[fi] = q.h & gm;
    S.dq_len[fi] = q.len;
    u64* g = S.dq + fi * S.rc;
    if (!q.spill)
        for (int i = 0; i < q.len; i++) g[(q.h + i) & gm] = l[((q.h + i) & (kDqK - 1))];
}

// output aggregator sources of the keyed replay: 0 count, 1 sum, 2 avg, 3 min, 4 max
struct KOut {
    int n;
    int src[SH_MAX_AGGS];
};

// The quirk check compares every expiring head with each of the chunk's records; bit-equal pairs are
// rare, so the records first go into a 32K-bit filter in LDS and a head runs the exact comparison only
// on a hit (about 0.2% of heads on distinct values). One wave per block: its LDS accesses are in order.
constexpr int kBfWords = 1024;
__device__ __forceinline__ u32 bf_hash(u64 v) { return (u32)((v * 0x9E3779B97F4A7C15ull) >> 49); }
__device__ __forceinline__ void bf_init(u32* bf, int lane) {
    for (int i = lane; i < kBfWords; i += 64) bf[i] = 0;
}
__device__ __forceinline__ bool bf_hit(const u32* bf, u64 v) {
    const u32 h = bf_hash(v);
    return (bf[h >> 5] >> (h & 31)) & 1u;
}

// lane l's value of a 64-bit register (l wave-uniform)
__device__ __forceinline__ u64 rl64(u64 v, int l) {
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l);
    const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const u32 lo = (u32)__shfl((int)(u32)v, src, 64), hi = (u32)__shfl((int)(u32)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

// a (value, present) pair's leftmost-best combination: the right one only when strictly better
template <bool MIN>
__device__ __forceinline__ void best_comb(u64& bv, bool& bh, u64 v, bool h) {
    if (h && (!bh || d_worse<MIN>(bv, v))) { bv = v; bh = true; }
}

// The window indices of the deque loaded from the carried state: it must be the suffix-best chain of
// the carried ring (no quirk in its history), entry by entry, with minValue at its front; false leaves
// the key sequential.
template <bool MIN>
__device__ bool dq_index_init(const KDq& q, const u64* dv, int* di, const u64* rval, int rh0, int gm, int H0,
                              int lane) {
    if (q.spill || q.nan) return false;
    if (q.len == 0) return H0 == 0;
    if (!q.mmh || q.mm != dv[q.h & (kDqK - 1)]) return false;
    int seen = 0;      // chain entries found in the blocks after the current one
    u64 after = 0;     // best value after the current block
    bool after_h = false, ok = true;
    for (int b1 = H0; b1 > 0 && ok; b1 -= 64) {
        const int b0 = b1 - 64 > 0 ? b1 - 64 : 0, h = b0 + lane;
        const bool in = h < b1;
        const u64 v = in ? rval[(rh0 + h) & gm] : 0;
        if (__any(in && d_isnan(v))) return false;
        // inclusive suffix best over the block's lanes (a numeric best: all the membership test needs)
        u64 t = v;
        bool th = in;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            // (every lane runs every shuffle: a lane that skipped one would leave its source register stale)
            const int src = lane + d < 64 ? lane + d : lane;
            const u64 ov = shfl64(t, src);
            const int oth = __shfl(th ? 1 : 0, src, 64);
            const bool oh = lane + d < 64 && oth != 0;
            if (oh && (!th || d_worse<MIN>(t, ov))) { t = ov; th = true; }
        }
        // best strictly after h: the next lane's suffix, then the later blocks
        const int nx = lane + 1 < 64 ? lane + 1 : lane;
        u64 nb = shfl64(t, nx);
        const int nth = __shfl(th ? 1 : 0, nx, 64);
        bool nh = lane + 1 < 64 && nth != 0;
        if (after_h && (!nh || d_worse<MIN>(nb, after))) { nb = after; nh = true; }
        const bool member = in && !(nh && d_worse<MIN>(v, nb));
        const unsigned long long bal = __ballot(member);
        const int above = lane == 63 ? 0 : __popcll(bal >> (lane + 1));
        const int pos = q.len - 1 - seen - above;
        bool bad = false;
        if (member) {
            if (pos < 0) bad = true;
            else {
                const int sl = (q.h + pos) & (kDqK - 1);
                if (dv[sl] != v) bad = true;
                else di[sl] = h;
            }
        }
        ok = !__any(bad);
        seen += __popcll(bal);
        const u64 bv = shfl64(t, 0);
        const bool bh = __shfl(th ? 1 : 0, 0, 64) != 0;
        if (bh && (!after_h || d_worse<MIN>(after, bv))) { after = bv; after_h = true; }
    }
    return ok && seen == q.len;
}

// per lane: the result after its record — the first deque entry at or after lo_eff against the chunk's
// records [max(lo_eff, S), S + lane] (leftmost best)
template <bool MIN>
__device__ __forceinline__ u64 par_best(const KDq& q, const u64* dv, const int* di, const u64* sx, u64 x, int lo_eff,
                                         int S, bool in_from0, int lane) {
    int a = 0, b = q.len;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (di[(q.h + mid) & (kDqK - 1)] < lo_eff) a = mid + 1;
        else b = mid;
    }
    u64 pv = a < q.len ? dv[(q.h + a) & (kDqK - 1)] : 0;
    bool ph = a < q.len;
    u64 cv;
    bool ch;
    if (in_from0) {
        // every lane's range starts at the chunk's first record: an inclusive prefix scan
        cv = x;
        ch = true;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 ov = shfl64(cv, lane >= d ? lane - d : lane);
            const bool oh = lane >= d;
            // left operand (earlier lanes) wins ties
            if (oh && !d_worse<MIN>(ov, cv)) cv = ov;
        }
    } else {
        ch = false;
        cv = 0;
        for (int j = lo_eff - S > 0 ? lo_eff - S : 0; j <= lane; j++) best_comb<MIN>(cv, ch, sx[j], true);
    }
    best_comb<MIN>(pv, ph, cv, ch);
    return pv;
}

// The deque after a chunk handled in parallel: the old entries still unexpired (from i0) and not worse
// than the chunk's best (up to i1), then the chunk's n_new suffix bests (`surv`: this lane's record is
// one). Nothing is written here; the caller commits only if i1 - i0 + n_new fits the LDS ring.
struct DqPlan {
    int i0, i1, n_new;
};
template <bool MIN>
__device__ __forceinline__ DqPlan dq_plan(const KDq& q, const u64* dv, const int* di, u64 x, bool in, int S,
                                          int lo_end, int lane, bool& surv) {
    // chunk's best over all its records
    u64 cb = x;
    bool chh = in;
    u64 sb = x;  // suffix best strictly after the lane
    bool sbh = false;
    {
        u64 t = x;
        bool th = in;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {  // inclusive suffix scan
            // (every lane runs every shuffle: a lane that skipped one would leave its source register stale)
            const int src = lane + d < 64 ? lane + d : lane;
            const u64 ov = shfl64(t, src);
            const int oth = __shfl(th ? 1 : 0, src, 64);
            const bool oh = lane + d < 64 && oth != 0;
            if (oh && (!th || d_worse<MIN>(t, ov))) { t = ov; th = true; }
        }
        cb = shfl64(t, 0);
        chh = __shfl(th ? 1 : 0, 0, 64) != 0;
        const int src = lane + 1 < 64 ? lane + 1 : lane;
        sb = shfl64(t, src);
        const int sth = __shfl(th ? 1 : 0, src, 64);
        sbh = lane + 1 < 64 && sth != 0;
    }
    surv = in && S + lane >= lo_end && !(sbh && d_worse<MIN>(x, sb));
    DqPlan p;
    int a = 0, b = q.len;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (di[(q.h + mid) & (kDqK - 1)] < lo_end) a = mid + 1;
        else b = mid;
    }
    p.i0 = a;
    int c = a;
    if (chh)
        while (c < q.len && !d_worse<MIN>(dv[(q.h + c) & (kDqK - 1)], cb)) c++;
    else
        c = q.len;
    p.i1 = c;
    p.n_new = __popcll(__ballot(surv));
    return p;
}

template <bool MIN>
__device__ __forceinline__ void dq_commit(KDq& q, u64* dv, int* di, const DqPlan& p, u64 x, bool surv, int S,
                                          int lane, u64 last_best) {
    const unsigned long long bal = __ballot(surv);
    const int rank = __popcll(bal & ((1ull << lane) - 1ull));
    if (surv) {
        const int sl = (q.h + p.i1 + rank) & (kDqK - 1);
        dv[sl] = x;
        di[sl] = S + lane;
    }
    __syncthreads();
    q.h += p.i0;
    q.len = p.i1 - p.i0 + p.n_new;
    if (q.len > 0) {
        q.f = dv[q.h & (kDqK - 1)];
        q.b = dv[(q.h + q.len - 1) & (kDqK - 1)];
    }
    q.mm = last_best;
    q.mmh = true;
}

// ---- one key's replay state and the steps both kernels take on it ------------------------------------
// The running aggregates of the wave's key, the same in every lane (the order-dependent parts run
// wave-uniform): count, the sum shared by sum and avg, the min / max deques and their global rings.
struct WkState {
    i64 cnt;
    double sum;
    KDq qn, qx;
    u64 *gmin, *gmax;
    int gm;  // ring mask
};

// The key's carried state into `w` and the deques' LDS rings. Returns whether min / max can run in
// parallel: the deque entries' window indices were found (dq_index_init) from the ring [rh0, rh0 + H0).
template <bool HSUM, bool HMIN, bool HMAX>
__device__ __forceinline__ bool wk_load(WkState& w, const SlState& S, const DFields& fd, u32 k, int rh0, int H0,
                                        u64* dq_min, u64* dq_max, int* di_min, int* di_max, u32* bf, int lane) {
    w.gm = (int)(S.rc - 1);
    w.cnt = S.cnt[k];
    w.sum = 0.0;
    if (HSUM) w.sum = __longlong_as_double((i64)S.f[(size_t)(fd.sum >= 0 ? fd.sum : fd.avg) * S.nslots + k]);
    w.gmin = HMIN ? S.dq + ((size_t)fd.mn * S.nslots + k) * S.rc : nullptr;
    w.gmax = HMAX ? S.dq + ((size_t)fd.mx * S.nslots + k) * S.rc : nullptr;
    if (HMIN) kdq_load(w.qn, S, fd.mn, k, dq_min);
    if (HMAX) kdq_load(w.qx, S, fd.mx, k, dq_max);
    if (HMIN || HMAX) bf_init(bf, lane);
    __syncthreads();
    const u64* rval = S.rval + (size_t)k * S.rc;
    bool par = HMIN || HMAX;
    if (HMIN && par) par = dq_index_init<true>(w.qn, dq_min, di_min, rval, rh0, w.gm, H0, lane);
    if (HMAX && par) par = dq_index_init<false>(w.qx, dq_max, di_max, rval, rh0, w.gm, H0, lane);
    __syncthreads();
    return par;
}

// The window after the push, by the whole wave: of its entries [0, HN) — the carried ring's H0, then the
// push's — the first `done` have left. Ring entries keep their place; put(slot, j) writes the push's j-th
// record to the key's ring slot. Lane 0 then stores the ring bounds and the aggregates.
template <bool HSUM, bool HMIN, bool HMAX, class Put>
__device__ __forceinline__ void wk_write_back(const WkState& w, const SlState& S, const DFields& fd, u32 k, int rh0,
                                              int H0, int HN, int done, const u64* dq_min, const u64* dq_max,
                                              int lane, Put put) {
    const int keep = done < H0 ? H0 - done : 0;
    const int rh = (rh0 + (done < H0 ? done : H0)) & w.gm;
    const int j0 = done > H0 ? done : H0;
    for (int j = j0 + lane; j < HN; j += 64) put((size_t)k * S.rc + (size_t)((rh + keep + (j - j0)) & w.gm), j - H0);
    if (lane == 0) {
        S.cnt[k] = w.cnt;
        S.rhead[k] = rh;
        S.rlen[k] = keep + (HN - j0);
        if (HSUM) {
            const u64 sb = (u64)__double_as_longlong(w.sum);
            if (fd.sum >= 0) S.f[(size_t)fd.sum * S.nslots + k] = sb;
            if (fd.avg >= 0) S.f[(size_t)fd.avg * S.nslots + k] = sb;
        }
        if (HMIN) kdq_store(w.qn, S, fd.mn, k, dq_min);
        if (HMAX) kdq_store(w.qx, S, fd.mx, k, dq_max);
    }
}

// the quirk: the expiring value v of window index idx meets a bit-equal deque entry of another event
__device__ __forceinline__ bool dq_quirk(const KDq& q, const u64* dv, const int* di, u64 v, int idx) {
    bool hit = false;
    for (int e = 0; e < q.len; e++) {
        const int sl = (q.h + e) & (kDqK - 1);
        hit |= dv[sl] == v && di[sl] != idx;
    }
    return hit;
}

// The sequential steps, on wave-uniform values: an event joins the window (processAdd) / the oldest
// leaves (processRemove). dq false: this chunk's min / max were computed in parallel, the deques stay.
template <bool HSUM, bool HMIN, bool HMAX>
__device__ __forceinline__ void wk_add(WkState& w, u64* dq_min, u64* dq_max, u64 v, bool dq) {
    w.cnt++;
    if (HSUM) w.sum = w.sum + __longlong_as_double((i64)v);
    if (dq) {
        if (HMIN) kdq_add<true>(w.qn, w.gmin, w.gm, dq_min, v);
        if (HMAX) kdq_add<false>(w.qx, w.gmax, w.gm, dq_max, v);
    }
}

template <bool HSUM, bool HMIN, bool HMAX>
__device__ __forceinline__ void wk_remove(WkState& w, u64* dq_min, u64* dq_max, u64 v, bool dq) {
    w.cnt--;
    if (HSUM) {
        w.sum = w.sum - __longlong_as_double((i64)v);
        if (w.cnt == 0 && w.sum == 0.0) w.sum = 0.0;  // destroyed state restarts from +0.0 (canDestroy)
    }
    if (dq) {
        if (HMIN) kdq_remove<true>(w.qn, w.gmin, w.gm, dq_min, v);
        if (HMAX) kdq_remove<false>(w.qx, w.gmax, w.gm, dq_max, v);
    }
}

// The Java-order double sum of a chunk as one operation list in LDS (a remove as the negated value:
// a - b is a + (-b) exactly in IEEE 754), added up in order by the whole wave with a uniform address.
// Bit j of the NW-word mask cz: the count is 0 after operation j, where the sum restarts from +0.0 (the
// restarts are rare, so a chunk without one runs the loop without their check). Returns the running sum
// after operation `mine` (none: -1).
template <int NW>
__device__ __forceinline__ u64 wk_sum_chain(double& sum, const u64* ops, int nops, const u64 (&cz)[NW], int mine) {
    double sm = sum;
    u64 r = 0, any = 0;
#pragma unroll
    for (int wd = 0; wd < NW; wd++) any |= cz[wd];
    if (any == 0) {
        for (int j = 0; j < nops; j++) {
            sm = sm + __longlong_as_double((i64)ops[j]);
            r = j == mine ? (u64)__double_as_longlong(sm) : r;
        }
    } else {
        for (int j = 0; j < nops; j++) {
            sm = sm + __longlong_as_double((i64)ops[j]);
            u64 m = cz[0];
#pragma unroll
            for (int wd = 1; wd < NW; wd++) m = (j >> 6) == wd ? cz[wd] : m;
            if ((m >> (j & 63)) & 1ull) sm = sm == 0.0 ? 0.0 : sm;
            r = j == mine ? (u64)__double_as_longlong(sm) : r;
        }
    }
    sum = sm;
    return r;
}

// ---- host side of the launches -------------------------------------------------------------------------
// the double-column shape (C3): count + at most one each of sum / avg / min / max of one DOUBLE
inline bool own_d_fields(const AggPlan& ap, DFields& fd) {
    fd = DFields{-1, -1, -1, -1};
    bool ok = ap.n_vcols == 1 && ap.vcol_type[0] == SH_T_DOUBLE;
    for (int a = 0; ok && a < ap.n; a++) {
        int* slotp = nullptr;
        switch (ap.kind[a]) {
            case AK_COUNT: continue;
            case AK_SUM_D: slotp = &fd.sum; break;
            case AK_AVG: slotp = &fd.avg; break;
            case AK_MIN_D: slotp = &fd.mn; break;
            case AK_MAX_D: slotp = &fd.mx; break;
            default: ok = false; continue;
        }
        if (*slotp >= 0) ok = false;
        else *slotp = ap.field[a];
    }
    return ok;
}

inline KOut agg_outputs(const AggPlan& ap) {
    KOut ko{};
    ko.n = ap.n;
    for (int q = 0; q < ap.n; q++) {
        const int kind = ap.kind[q];
        ko.src[q] = kind == AK_COUNT ? 0 : kind == AK_SUM_D ? 1 : kind == AK_AVG ? 2 : kind == AK_MIN_D ? 3 : 4;
    }
    return ko;
}

// f(HSUM, HMIN, HMAX) with the shape's aggregators as compile-time booleans (std::true_type / false_type):
// the launch of a kernel template's matching instantiation
template <class F>
void for_agg_shape(const DFields& fd, F f) {
    auto with = [](bool b, auto g) {
        if (b) g(std::true_type{});
        else g(std::false_type{});
    };
    with(fd.sum >= 0 || fd.avg >= 0, [&](auto hs) {
        with(fd.mn >= 0, [&](auto hn) { with(fd.mx >= 0, [&](auto hx) { f(hs, hn, hx); }); });
    });
}

}  // namespace shd
