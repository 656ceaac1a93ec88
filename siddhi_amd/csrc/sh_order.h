// sh_order.h — `order by` / `limit` / `offset` of the selector (sh_query_set_order).
//
// The last step of QuerySelector.processInBatchGroupBy (core/query/selector/QuerySelector.java:355-370;
// processNoGroupBy :191-199 and processInBatchNoGroupBy :304-310 end the same way), after `having` and
// before the OutputRateLimiter, once per selector output chunk — one flush of a call's sh_out:
//   1. orderEventChunk (:452-483): the chunk is cut into maximal runs of consecutive rows of one type
//      (CURRENT / EXPIRED); each run is sorted on its own, stably, and keeps its place;
//   2. OrderByEventComparator.compare (:63-117), term by term: two non-null values by their type's
//      compareTo (Double: -0.0 < 0.0, every NaN equal and above +Infinity; Boolean: false < true), negated
//      for `desc`; exactly one null: the non-null row first, for asc and desc alike; both null or equal: the
//      next term; all terms equal: the earlier row first;
//   3. offsetEventChunk (:502-519): the chunk's first `offset` rows go;
//   4. limitEventChunk (:485-500): `(limit > count) && CURRENT && currentOn || EXPIRED && expiredOn` with
//      `&&` binding first — an EXPIRED row is always kept and counted, a CURRENT row only while fewer than
//      `limit` rows were kept: a row at position p after the offset is kept iff EXPIRED or p < limit;
//   5. a chunk that keeps no row gives no flush (OutputRateLimiter.sendToCallBacks :89-105);
//   6. processInBatchNoGroupBy (aggregators without group-by; the selector batches for every window family,
//      execute :140-159): the chunk's one row is kept iff offset is unset or 0 and limit is unset or > 0.
// The step is a pass over a call's finished device rows (order_apply), placed where rate_apply is and in
// front of it. It has no state: nothing is carried from call to call and a snapshot has no section for it.
// The spec is configuration, like the having program: the caller sets it again on a restored query.
#pragma once

#include "sh_internal.h"

namespace shd {

constexpr int kOrdMaxTerms = 4;
// the largest flush one workgroup sorts in LDS (k_ord_block: 36 B of LDS per row with four terms)
constexpr int kOrdBlockRows = 1024;

// How a term's 8-byte slot orders: as a signed integer, or as an IEEE double (Double.compareTo)
enum OrdImage { kOrdInt = 0, kOrdDouble = 1 };

// The compiled spec, a kernel argument. A term reads the key column `index` (kind SH_ORD_KEY) or the
// aggregate `index` (SH_ORD_AGG: its value slot and null flag).
struct OrdSpec {
    int n_terms;
    int single;  // rule 6: every flush holds one row, kept or dropped by limit / offset alone
    int kind[kOrdMaxTerms], index[kOrdMaxTerms], image[kOrdMaxTerms], desc[kOrdMaxTerms];
    int nullable[kOrdMaxTerms];  // the term can be null: an aggregate other than count
    i64 limit, offset;  // -1: not given
};

// A call's rows as the kernels read and write them (column-major, `stride` rows per column)
struct OrdRows {
    i64* ts;
    unsigned char* expired;
    i64* rep;
    i64* keys;
    u64* vals;
    unsigned char* nulls;
    i64 stride;
};

// Global route, step 1: per row its run's head flag (head[i] = 1 where a flush or a type run starts,
// head[n] = 0) and, per term, the order-preserving 64-bit image (inverted for desc; 0 where the value is
// null) and the null flag as a sort key (img / nul: [n_terms][n])
void launch_ord_keys(hipStream_t s, OrdSpec sp, OrdRows in, i64 n, const i64* foff, int nf, u32* head, u64* img, u64* nul);
// key[j] = col[perm[j]], or col32[perm[j]], or col32[perm[j]] << 1 | col[perm[j]] & 1 when both are given
// (perm NULL: the identity); iota[j] = j when it is given
void launch_ord_pick(hipStream_t s, i64 n, const u64* col, const u32* col32, const u32* perm, u64* key, u32* iota);
// Block route: one workgroup per flush of at most kOrdBlockRows rows ranks the flush's rows in LDS by
// (run, term 0 .. term n-1, position); perm[sorted position] = source row
void launch_ord_block(hipStream_t s, OrdSpec sp, OrdRows in, const i64* foff, int nf, u32* perm);
// Step 3: flag[j] = the row at sorted position j survives offset and limit (flag[n] = 0)
void launch_ord_cut(hipStream_t s, OrdSpec sp, const unsigned char* expired, const u32* perm, i64 n, const i64* foff,
                    int nf, u32* flag);
// ... after the scan of the flags (pre): the kept rows in front of every flush (cnt[f] = pre[foff[f]],
// f = 0 .. nf; cnt[nf] = all kept rows), and the kept rows gathered into `out`
void launch_ord_counts(hipStream_t s, const u32* pre, const i64* foff, int nf, u32* cnt);
void launch_ord_gather(hipStream_t s, const u32* flag, const u32* pre, const u32* perm, OrdRows in, OrdRows out, i64 n,
                       int nk, int na);

}  // namespace shd
