// sh_order.cpp — `order by` / `limit` / `offset` of the selector: the validation behind sh_order_check and
// sh_query_set_order, and order_apply, the pass over a call's finished device rows (sh_order.h has the rules,
// sh_order_kernels.hip the kernels). Modelled on the output rate limiter's pass (sh_rate.cpp), which it
// precedes: it reads an sh_out whose rows are on the device and whose flush layout is on the host, owns its
// result buffers and gives back a host or a device view.
#include "sh_order.h"

#include <atomic>
#include <cstring>
#include <string>

#include "sh_agg.h"
#include "sh_runtime.h"
#include "sh_wide.h"

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

namespace {
// calls that entered order_apply, and those among them that sorted on the block / the global route
std::atomic<int64_t> g_passes{0}, g_block{0}, g_global{0};

bool fp_type(int t) { return t == SH_T_FLOAT || t == SH_T_DOUBLE; }

unsigned bits_of(int64_t n) {  // bits needed for values < n
    unsigned b = 1;
    while (b < 63 && ((int64_t)1 << b) < n) b++;
    return b;
}
}  // namespace

// Debug hook (not part of the ABI, found by symbol lookup): process-wide counts of the calls that entered the
// pass and of those that sorted on either route. A test reads it around a query without a spec to see that
// such a query never pays for the step, and around forced routes to see which one ran.
extern "C" void sh_order_debug_counts(int64_t* passes, int64_t* block_route, int64_t* global_route) {
    if (passes) *passes = g_passes.load();
    if (block_route) *block_route = g_block.load();
    if (global_route) *global_route = g_global.load();
}

// The validation behind sh_order_check and sh_query_set_order.
static int order_compile(const sh_query_desc* d, const sh_order_term* terms, int32_t n_terms, int64_t limit,
                         int64_t offset, OrdSpec* out) {
    if (!d) return sh_fail(SH_ERR_INVALID, "order: NULL descriptor");
    if (n_terms < 0 || n_terms > kOrdMaxTerms) return sh_fail(SH_ERR_INVALID, "order by: more than 4 terms");
    if (n_terms > 0 && !terms) return sh_fail(SH_ERR_INVALID, "order by: NULL terms");
    if (limit < -1) return sh_fail(SH_ERR_INVALID, "'limit' cannot have negative value");
    if (offset < -1) return sh_fail(SH_ERR_INVALID, "'offset' cannot have negative value");
    if (n_terms == 0 && limit == -1 && offset == -1)
        return sh_fail(SH_ERR_INVALID, "order: nothing to do (no term, no limit, no offset)");
    if (d->n_cols <= 0 || d->n_cols > SH_MAX_COLS || d->n_group_by < 0 || d->n_group_by > SH_MAX_GROUP ||
        d->n_aggs < 0 || d->n_aggs > SH_MAX_AGGS)
        return sh_fail(SH_ERR_INVALID, "order: bad descriptor");
    for (int g = 0; g < d->n_group_by; g++)
        if (d->group_by[g] < 0 || d->group_by[g] >= d->n_cols) return sh_fail(SH_ERR_INVALID, "group-by column out of range");
    for (int a = 0; a < d->n_aggs; a++)
        if (d->aggs[a].fn != SH_AGG_COUNT && (d->aggs[a].col < 0 || d->aggs[a].col >= d->n_cols))
            return sh_fail(SH_ERR_INVALID, "aggregator column out of range");
    for (int t = 0; t < n_terms; t++) {
        const sh_order_term& o = terms[t];
        if (o.kind != SH_ORD_KEY && o.kind != SH_ORD_AGG) return sh_fail(SH_ERR_INVALID, "order by: unknown term kind");
        // (a pass-through query has neither: its terms are refused below, by name)
        if (d->n_aggs > 0 && (o.index < 0 || o.index >= (o.kind == SH_ORD_KEY ? d->n_group_by : d->n_aggs)))
            return sh_fail(SH_ERR_INVALID, o.kind == SH_ORD_KEY ? "order by: group-by number out of range"
                                                                : "order by: aggregate number out of range");
    }
    // ---- the shapes that stay on the CPU ----
    if (d->window == SH_WIN_NONE) return sh_fail(SH_ERR_UNSUPPORTED, "order by / limit without a window: not a GPU path");
    if (d->partition_col >= 0)
        return sh_fail(SH_ERR_UNSUPPORTED,
                       "order by / limit in a partitioned query (the partition lanes keep one selector per partition)");
    if (d->n_group_by > 0 && WideKeys::needed(d->n_group_by, d->group_by, d->col_types))
        return sh_fail(SH_ERR_UNSUPPORTED, "order by / limit with a group-by the library interns (wide keys)");
    if (n_terms > 0 && d->n_aggs == 0)
        return sh_fail(SH_ERR_UNSUPPORTED,
                       "order by on a pass-through query (select *): the term is a stream attribute of the event, which "
                       "the rows do not carry; limit and offset alone run there");
    OrdSpec sp{};
    sp.n_terms = n_terms;
    sp.limit = limit;
    sp.offset = offset;
    sp.single = d->n_group_by == 0 && d->n_aggs > 0;  // (processInBatchNoGroupBy, for every window family)
    for (int t = 0; t < n_terms; t++) {
        const sh_order_term& o = terms[t];
        int type;
        if (o.kind == SH_ORD_KEY) {
            type = d->col_types[d->group_by[o.index]];
            if (type == SH_T_STRID)
                return sh_fail(SH_ERR_UNSUPPORTED,
                               "order by a string group key: String.compareTo needs the text (dictionary ids do not order)");
        } else {
            const int fn = d->aggs[o.index].fn;
            if (fn < SH_AGG_SUM || fn > SH_AGG_MAX) return sh_fail(SH_ERR_INVALID, "unknown aggregator");
            const int ct = fn == SH_AGG_COUNT ? SH_T_LONG : d->col_types[d->aggs[o.index].col];
            type = fn == SH_AGG_COUNT ? SH_T_LONG : fn == SH_AGG_AVG ? SH_T_DOUBLE
                   : fn == SH_AGG_SUM ? (fp_type(ct) ? SH_T_DOUBLE : SH_T_LONG) : ct;
            // (today only an EXPIRED row's aggregates are null; the flag is sorted on for every aggregate that
            // can carry one, as k_ord_block honours it, so the two routes agree whatever the rows hold)
            sp.nullable[t] = fn != SH_AGG_COUNT;
        }
        sp.kind[t] = o.kind;
        sp.index[t] = o.index;
        sp.image[t] = fp_type(type) ? kOrdDouble : kOrdInt;  // (a float is reported widened to double)
        sp.desc[t] = o.desc != 0;
    }
    if (out) *out = sp;
    return SH_OK;
}

extern "C" int sh_order_check(const sh_query_desc* desc, const sh_order_term* terms, int32_t n_terms, int64_t limit,
                              int64_t offset) {
    return order_compile(desc, terms, n_terms, limit, offset, nullptr);
}

extern "C" int sh_query_set_order(sh_query* q, const sh_order_term* terms, int32_t n_terms, int64_t limit, int64_t offset) {
    if (!q) return sh_fail(SH_ERR_INVALID, "sh_query_set_order: NULL query");
    if (q->ord.on) return sh_fail(SH_ERR_STATE, "sh_query_set_order: the spec is set once");
    if (q->seq != 0 || q->n_pend != 0 || q->clock_valid)
        return sh_fail(SH_ERR_STATE, "sh_query_set_order: set it before the first push");
    if (q->wide) return sh_fail(SH_ERR_UNSUPPORTED, "order by / limit with a group-by the library interns (wide keys)");
    if (q->given || q->internal_keys)
        return sh_fail(SH_ERR_UNSUPPORTED, "order by / limit on a sharded query's owner or an aggregation root");
    OrdSpec sp{};
    RCHK(order_compile(&q->d, terms, n_terms, limit, offset, &sp));
    if (q->xt_replace) return sh_fail(SH_ERR_UNSUPPORTED, "order by / limit with replaceTimestampWithBatchEndTime");
    q->ord.spec = sp;
    q->ord.on = true;
    return SH_OK;
}

namespace {
int reserve_rows(DevBuf& b, int64_t rows, int cols, size_t elem) {
    return b.reserve((size_t)std::max<int64_t>(rows, 1) * std::max(cols, 1) * elem, false);
}

// the kept rows (T of them in `o`, flushes in q->ord.flush_*) as the caller's host or device view
int order_finish(sh_query* q, const OrdRows& o, int64_t T, int nk, int na, bool host_out, const sh_out** out) {
    auto& r = q->ord;
    hipStream_t s = q->ctx->stream;
    if (host_out) {
        OutHost& ho = q->out;
        ho.reset();
        ho.flush_offsets.assign(r.flush_offsets.begin(), r.flush_offsets.end());
        ho.flush_clock.assign(r.flush_clock.begin(), r.flush_clock.end());
        ho.ts.resize(T);
        ho.expired.resize(T);
        ho.rep.resize(T);
        ho.keys.resize((size_t)nk * T);
        ho.vals.resize((size_t)na * T);
        ho.nulls.resize((size_t)na * T);
        if (T > 0) {
            HIPCHK(hipMemcpyAsync(ho.ts.data(), o.ts, T * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(ho.expired.data(), o.expired, T, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(ho.rep.data(), o.rep, T * 8, hipMemcpyDeviceToHost, s));
            if (nk) HIPCHK(hipMemcpyAsync(ho.keys.data(), o.keys, (size_t)nk * T * 8, hipMemcpyDeviceToHost, s));
            if (na) {
                HIPCHK(hipMemcpyAsync(ho.vals.data(), o.vals, (size_t)na * T * 8, hipMemcpyDeviceToHost, s));
                HIPCHK(hipMemcpyAsync(ho.nulls.data(), o.nulls, (size_t)na * T, hipMemcpyDeviceToHost, s));
            }
            HIPCHK(hipStreamSynchronize(s));
        }
        *out = ho.view(nk, na, q->vtypes);
    } else {
        sh_out& d = r.dev_out;
        d = sh_out{};
        d.n_flushes = (int64_t)r.flush_clock.size();
        d.n_rows = T;
        d.n_keys = nk;
        d.n_vals = na;
        for (int i = 0; i < na; i++) d.val_types[i] = q->vtypes[i];
        d.flush_offsets = r.flush_offsets.data();
        d.flush_clock = r.flush_clock.data();
        d.ts = o.ts;
        d.expired = o.expired;
        d.keys = o.keys;
        d.vals = (const uint64_t*)o.vals;
        d.nulls = o.nulls;
        d.rep = o.rep;
        *out = &d;
    }
    return SH_OK;
}

// Global route: stable radix passes over the whole call, last term first and the rows' runs last — the
// runs are numbered through the call, so the last pass also puts the flushes back in order. A term that
// can be null takes a second, one-bit pass for its null flag (above the image: nulls last).
int sort_global(sh_query* q, const OrdRows& in, int64_t n, const i64* foff, int nf, u32** perm_out) {
    auto& r = q->ord;
    hipStream_t s = q->ctx->stream;
    const OrdSpec& sp = r.spec;
    RCHK(r.head.reserve((size_t)(n + 1) * 4, false));
    RCHK(r.img.reserve((size_t)sp.n_terms * n * 8, false));
    RCHK(r.nul.reserve((size_t)sp.n_terms * n * 8, false));
    RCHK(r.key.reserve((size_t)n * 8, false));
    RCHK(r.key2.reserve((size_t)n * 8, false));
    RCHK(r.perm.reserve((size_t)n * 4, false));
    RCHK(r.perm2.reserve((size_t)n * 4, false));
    RCHK(r.tmp.reserve((size_t)((n + 1 + kTile - 1) / kTile + 16) * 8, false));
    launch_ord_keys(s, sp, in, n, foff, nf, r.head.as<u32>(), r.img.as<u64>(), r.nul.as<u64>());
    // head -> the runs before each row: row i lies in run head[i + 1] (counted through the call, from 1)
    launch_scan_sum_large_u32(s, r.head.as<u32>(), n + 1, r.tmp.as<i64>());
    HIPCHK(hipGetLastError());
    const unsigned run_bits = bits_of(n + 1);
    size_t tb = 0, tb1 = 0, tbr = 0;  // (the sort's temporary storage may depend on the bit range)
    if (sort_u64_pairs(nullptr, &tb, nullptr, nullptr, nullptr, nullptr, n, s) ||
        sort_u64_pairs_bits(nullptr, &tb1, nullptr, nullptr, nullptr, nullptr, n, 1, s) ||
        sort_u64_pairs_bits(nullptr, &tbr, nullptr, nullptr, nullptr, nullptr, n, run_bits + 1, s))
        return sh_fail(SH_ERR_DEVICE, "order by: sort sizing");
    RCHK(r.sort_tmp.reserve(std::max<size_t>(std::max(tb, std::max(tb1, tbr)), 16), false));
    u32* cur = nullptr;  // the order so far (NULL: the rows' own)
    u32* a = r.perm.as<u32>();
    u32* b = r.perm2.as<u32>();
    auto pass = [&](const u64* col, const u32* col32, unsigned bits) -> int {
        // the column in the order so far, then one stable sort of (key, row)
        launch_ord_pick(s, n, col, col32, cur, r.key.as<u64>(), cur ? nullptr : a);
        const u32* vin = cur ? cur : a;
        u32* vout = vin == a ? b : a;
        size_t bytes = r.sort_tmp.cap;
        const int rc = bits == 64 ? sort_u64_pairs(r.sort_tmp.p, &bytes, r.key.as<u64>(), r.key2.as<u64>(), vin, vout, n, s)
                                  : sort_u64_pairs_bits(r.sort_tmp.p, &bytes, r.key.as<u64>(), r.key2.as<u64>(), vin, vout,
                                                        n, bits, s);
        if (rc) return sh_fail(SH_ERR_DEVICE, "order by: sort failed");
        cur = vout;
        return SH_OK;
    };
    for (int t = sp.n_terms - 1; t >= 0; t--) {
        RCHK(pass(r.img.as<u64>() + (size_t)t * n, nullptr, 64));
        if (sp.nullable[t] && t > 0) RCHK(pass(r.nul.as<u64>() + (size_t)t * n, nullptr, 1));
    }
    // (the first term's null flag rides below the run number: one pass for both)
    if (sp.nullable[0]) RCHK(pass(r.nul.as<u64>(), r.head.as<u32>() + 1, run_bits + 1));
    else RCHK(pass(nullptr, r.head.as<u32>() + 1, run_bits));
    HIPCHK(hipGetLastError());
    *perm_out = cur;
    return SH_OK;
}
}  // namespace

int order_apply(sh_query* q, const sh_out* in, bool host_out, const sh_out** out) {
    auto& r = q->ord;
    hipStream_t s = q->ctx->stream;
    const OrdSpec& sp = r.spec;
    const int nk = (int)in->n_keys, na = (int)in->n_vals;
    const int64_t n = in->n_rows;
    const int64_t nf64 = in->n_flushes;
    g_passes++;
    r.flush_offsets.assign(1, 0);
    r.flush_clock.clear();
    if (n == 0) return order_finish(q, OrdRows{}, 0, nk, na, host_out, out);  // no chunk reaches the step
    if (n >= ((int64_t)1 << 32) - 1 || nf64 >= ((int64_t)1 << 31) - 1)
        return sh_fail(SH_ERR_UNSUPPORTED, "order by / limit over 2^32 rows in one call");
    const int nf = (int)nf64;
    // the flush layout: every row in exactly one flush, in order (the kernels search it)
    const int64_t* off = in->flush_offsets;
    if (!off || !in->flush_clock || nf < 1 || off[0] != 0 || off[nf] != n)
        return sh_fail(SH_ERR_STATE, "order by / limit: the call's output has no full flush layout");
    int64_t m_max = 0;
    for (int f = 0; f < nf; f++) {
        if (off[f + 1] < off[f]) return sh_fail(SH_ERR_STATE, "order by / limit: flush offsets decrease");
        m_max = std::max(m_max, off[f + 1] - off[f]);
    }
    RCHK(r.foff.reserve((size_t)(nf + 1) * 8, false));
    HIPCHK(hipMemcpyAsync(r.foff.p, off, (size_t)(nf + 1) * 8, hipMemcpyHostToDevice, s));
    const i64* foff = r.foff.as<i64>();
    const OrdRows rows{(i64*)in->ts, (unsigned char*)in->expired, (i64*)in->rep, (i64*)in->keys, (u64*)in->vals,
                       (unsigned char*)in->nulls, n};
    // ---- sort (skipped where no flush has two rows, without terms and for the one-row chunks of rule 6) ----
    u32* perm = nullptr;
    if (sp.n_terms > 0 && !sp.single && m_max > 1) {
        if (m_max <= q->tune.ord_block_max) {
            RCHK(r.perm.reserve((size_t)n * 4, false));
            perm = r.perm.as<u32>();
            launch_ord_block(s, sp, rows, foff, nf, perm);
            HIPCHK(hipGetLastError());
            g_block++;
        } else {
            RCHK(sort_global(q, rows, n, foff, nf, &perm));
            g_global++;
        }
    }
    // ---- cut: offset and limit by the sorted position in the flush; scan; the flushes' kept rows ----
    RCHK(r.flag.reserve((size_t)(n + 1) * 4, false));
    RCHK(r.pre.reserve((size_t)(n + 1) * 4, false));
    RCHK(r.tmp.reserve((size_t)((n + 1 + kTile - 1) / kTile + 16) * 8, false));
    RCHK(r.cnt.reserve((size_t)(nf + 1) * 4, false));
    launch_ord_cut(s, sp, rows.expired, perm, n, foff, nf, r.flag.as<u32>());
    HIPCHK(hipMemcpyAsync(r.pre.p, r.flag.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToDevice, s));
    launch_scan_sum_large_u32(s, r.pre.as<u32>(), n + 1, r.tmp.as<i64>());
    launch_ord_counts(s, r.pre.as<u32>(), foff, nf, r.cnt.as<u32>());
    HIPCHK(hipGetLastError());
    r.h_cnt.resize((size_t)nf + 1);
    HIPCHK(hipMemcpyAsync(r.h_cnt.data(), r.cnt.p, (size_t)(nf + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (also: `off` may be the caller's pageable memory)
    const int64_t T = r.h_cnt[nf];
    // the flushes that keep a row, with their clocks
    for (int f = 0; f < nf; f++)
        if (r.h_cnt[f + 1] > r.h_cnt[f]) {
            r.flush_offsets.push_back((int64_t)r.h_cnt[f + 1]);
            r.flush_clock.push_back(in->flush_clock[f]);
        }
    // ---- compact ----
    RCHK(reserve_rows(r.o_ts, T, 1, 8));
    RCHK(reserve_rows(r.o_exp, T, 1, 1));
    RCHK(reserve_rows(r.o_rep, T, 1, 8));
    RCHK(reserve_rows(r.o_keys, T, nk, 8));
    RCHK(reserve_rows(r.o_vals, T, na, 8));
    RCHK(reserve_rows(r.o_nulls, T, na, 1));
    const OrdRows o{r.o_ts.as<i64>(), r.o_exp.as<unsigned char>(), r.o_rep.as<i64>(), r.o_keys.as<i64>(),
                    r.o_vals.as<u64>(), r.o_nulls.as<unsigned char>(), T};
    if (T > 0) {
        launch_ord_gather(s, r.flag.as<u32>(), r.pre.as<u32>(), perm, rows, o, n, nk, na);
        HIPCHK(hipGetLastError());
    }
    return order_finish(q, o, T, nk, na, host_out, out);
}
