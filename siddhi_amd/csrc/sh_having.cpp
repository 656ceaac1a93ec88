// sh_having.cpp — the `having` program of a batch-window query: the type-checking compiler behind
// sh_having_check and sh_query_set_having, and the per-query state (sh_having.h). The evaluation is in
// sh_having_kernels.hip, routed from run_closed (sh_window.cpp) and sc_rows / sc_expire_pending
// (sh_stream_current.cpp).
#include "sh_having.h"

#include <string>

#include "sh_runtime.h"
#include "sh_wide.h"

using namespace shd;

#define RCHK(x)            \
    do {                   \
        int _r = (x);      \
        if (_r) return _r; \
    } while (0)

namespace {
// operand types on the compiler's stack: SH_T_* or the result of a condition
constexpr int kCond = 0;
bool numeric_t(int t) { return t == SH_T_INT || t == SH_T_LONG || t == SH_T_FLOAT || t == SH_T_DOUBLE; }
bool boolean_t(int t) { return t == kCond || t == SH_T_BOOL; }

const char* window_name(int w) {
    switch (w) {
        case SH_WIN_NONE: return "no window";
        case SH_WIN_TIME: return "a sliding time window";
        case SH_WIN_EXT_TIME: return "a sliding externalTime window";
        case SH_WIN_LENGTH: return "a sliding length window";
        default: return "this window";
    }
}

// the output type of aggregate a (compile_aggs' out_types, without building a plan)
int agg_type(const sh_query_desc* d, int a, int* t) {
    const int fn = d->aggs[a].fn, col = d->aggs[a].col;
    if (fn == SH_AGG_COUNT) { *t = SH_T_LONG; return SH_OK; }
    if (col < 0 || col >= d->n_cols) return sh_fail(SH_ERR_INVALID, "aggregator column out of range");
    const int ct = d->col_types[col];
    if (!numeric_t(ct)) return sh_fail(SH_ERR_INVALID, "aggregator over a non-numeric attribute");
    const bool fp = ct == SH_T_FLOAT || ct == SH_T_DOUBLE;
    switch (fn) {
        case SH_AGG_SUM: *t = fp ? SH_T_DOUBLE : SH_T_LONG; return SH_OK;
        case SH_AGG_AVG: *t = SH_T_DOUBLE; return SH_OK;
        case SH_AGG_MIN:
        case SH_AGG_MAX: *t = ct; return SH_OK;
        default: return sh_fail(SH_ERR_INVALID, "unknown aggregator");
    }
}
}  // namespace

int having_compile(const sh_query_desc* d, const sh_filter_op* ops, int32_t n_ops, HavingProg* out) {
    if (!d) return sh_fail(SH_ERR_INVALID, "having: NULL descriptor");
    if (n_ops <= 0 || !ops) return sh_fail(SH_ERR_INVALID, "having: empty program");
    if (n_ops > kMaxFilterOps) return sh_fail(SH_ERR_INVALID, "having program longer than 32 ops");
    if (d->n_cols <= 0 || d->n_cols > SH_MAX_COLS || d->n_group_by < 0 || d->n_group_by > SH_MAX_GROUP ||
        d->n_aggs < 0 || d->n_aggs > SH_MAX_AGGS)
        return sh_fail(SH_ERR_INVALID, "having: bad descriptor");
    for (int g = 0; g < d->n_group_by; g++)
        if (d->group_by[g] < 0 || d->group_by[g] >= d->n_cols) return sh_fail(SH_ERR_INVALID, "group-by column out of range");
    // ---- the shapes that stay on the CPU ----
    if (d->window != SH_WIN_LENGTH_BATCH && d->window != SH_WIN_TIME_BATCH && d->window != SH_WIN_EXT_TIME_BATCH)
        return sh_fail(SH_ERR_UNSUPPORTED, std::string("having on ") + window_name(d->window) +
                                               ": the GPU runs having on lengthBatch, timeBatch and externalTimeBatch");
    // expired rows show the aggregates after every removal: the stream.current.event forms keep the whole
    // window in the pending buffer and walk it again (k_hvx_walk); the plain windows would have to carry
    // the previous batch's events across calls
    if (d->expired_on != 0 && !(d->stream_current && (d->window == SH_WIN_LENGTH_BATCH || d->window == SH_WIN_TIME_BATCH)))
        return sh_fail(SH_ERR_UNSUPPORTED,
                       "having with expired / all-events output on this window: it runs on lengthBatch(L, true) and "
                       "timeBatch(T, true) (stream.current.event); the other batch windows run it with current-events "
                       "output only");
    if (d->partition_col >= 0) return sh_fail(SH_ERR_UNSUPPORTED, "having in a partitioned query (partition lanes)");
    if (d->n_group_by > 0 && WideKeys::needed(d->n_group_by, d->group_by, d->col_types))
        return sh_fail(SH_ERR_UNSUPPORTED, "having with a group-by the library interns (wide keys)");
    if (d->n_aggs == 0) return sh_fail(SH_ERR_UNSUPPORTED, "having on a query without aggregators (pass-through)");
    for (int i = 0; i < n_ops; i++)
        if (ops[i].op == SH_OP_COL)
            return sh_fail(SH_ERR_UNSUPPORTED,
                           "having on a stream attribute of the representative event (SH_OP_COL operand)");
    // ---- the program ----
    HavingProg hp{};
    hp.n = n_ops;
    int st[kMaxFilterOps];
    int sp = 0;
    for (int i = 0; i < n_ops; i++) {
        const sh_filter_op& o = ops[i];
        FilterOpD od{o.op, o.type, o.col, 0, o.ival, o.dval};
        switch (o.op) {
            case SH_OP_KEY:
                if (o.col < 0 || o.col >= d->n_group_by) return sh_fail(SH_ERR_INVALID, "having: group-by number out of range");
                od.type = d->col_types[d->group_by[o.col]];
                st[sp++] = od.type;
                break;
            case SH_OP_AGG: {
                if (o.col < 0 || o.col >= d->n_aggs) return sh_fail(SH_ERR_INVALID, "having: aggregate number out of range");
                int t = 0;
                RCHK(agg_type(d, o.col, &t));
                od.type = t;
                st[sp++] = t;
                break;
            }
            case SH_OP_CONST:
                if (o.type < SH_T_INT || o.type > SH_T_BOOL) return sh_fail(SH_ERR_INVALID, "having: bad constant type");
                st[sp++] = o.type;
                break;
            case SH_OP_NOT:
                if (sp < 1) return sh_fail(SH_ERR_INVALID, "having: stack underflow");
                if (!boolean_t(st[sp - 1])) return sh_fail(SH_ERR_INVALID, "having: NOT of a value that is not boolean");
                st[sp - 1] = kCond;
                break;
            case SH_OP_AND:
            case SH_OP_OR:
                if (sp < 2) return sh_fail(SH_ERR_INVALID, "having: stack underflow");
                if (!boolean_t(st[sp - 1]) || !boolean_t(st[sp - 2]))
                    return sh_fail(SH_ERR_INVALID, "having: AND / OR of a value that is not boolean");
                sp--;
                st[sp - 1] = kCond;
                break;
            case SH_OP_GT: case SH_OP_GE: case SH_OP_LT: case SH_OP_LE: case SH_OP_EQ: case SH_OP_NE: {
                if (sp < 2) return sh_fail(SH_ERR_INVALID, "having: stack underflow");
                const int a = st[sp - 2], b = st[sp - 1];
                const bool rel = o.op != SH_OP_EQ && o.op != SH_OP_NE;
                if (a == kCond || b == kCond) return sh_fail(SH_ERR_INVALID, "having: a boolean fed to a comparison");
                if (rel && !(numeric_t(a) && numeric_t(b)))
                    return sh_fail(SH_ERR_INVALID, "having: relational comparison on a string or bool operand");
                if (!rel && !((numeric_t(a) && numeric_t(b)) || (a == b)))
                    return sh_fail(SH_ERR_INVALID, "having: == / != between operands of different kinds");
                sp--;
                st[sp - 1] = kCond;
                break;
            }
            default: return sh_fail(SH_ERR_INVALID, "having: unknown opcode");
        }
        if (sp > 16) return sh_fail(SH_ERR_INVALID, "having: stack deeper than 16");
        hp.ops[i] = od;
    }
    if (sp != 1) return sh_fail(SH_ERR_INVALID, "having: program leaves stack depth != 1");
    if (!boolean_t(st[0])) return sh_fail(SH_ERR_INVALID, "having: the result is not boolean");
    if (out) *out = hp;
    return SH_OK;
}

extern "C" int sh_having_check(const sh_query_desc* desc, const sh_filter_op* ops, int32_t n_ops) {
    return having_compile(desc, ops, n_ops, nullptr);
}

extern "C" int sh_query_set_having(sh_query* q, const sh_filter_op* ops, int32_t n_ops) {
    if (!q) return sh_fail(SH_ERR_INVALID, "sh_query_set_having: NULL query");
    if (q->hv.on) return sh_fail(SH_ERR_STATE, "sh_query_set_having: the program is set once");
    if (q->seq != 0 || q->n_pend != 0 || q->clock_valid)
        return sh_fail(SH_ERR_STATE, "sh_query_set_having: set it before the first push");
    if (q->wide) return sh_fail(SH_ERR_UNSUPPORTED, "having with a group-by the library interns (wide keys)");
    if (q->given || q->internal_keys)
        return sh_fail(SH_ERR_UNSUPPORTED, "having on a sharded query's owner or an aggregation root");
    HavingProg hp{};
    RCHK(having_compile(&q->d, ops, n_ops, &hp));
    if (q->kind != 0) return sh_fail(SH_ERR_UNSUPPORTED, "having on a sliding window or partition lanes");
    if (q->xt_timeout > 0) return sh_fail(SH_ERR_UNSUPPORTED, "having with an externalTimeBatch timeout");
    if (q->xt_replace) return sh_fail(SH_ERR_UNSUPPORTED, "having with replaceTimestampWithBatchEndTime");
    // an aggregate operand carries its fold field and kind (k_hv_walk reads them from the op)
    for (int i = 0; i < hp.n; i++)
        if (hp.ops[i].op == SH_OP_AGG) {
            hp.ops[i].pad = q->ap.field[hp.ops[i].col];
            hp.ops[i].ival = q->ap.kind[hp.ops[i].col];
        }
    q->hv.prog = hp;
    q->hv.kind = having_kind(hp);
    q->hv.on = true;
    return SH_OK;
}
