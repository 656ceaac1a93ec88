// sh_length_kernels.hip — the front end of `insert expired events` / `insert all events` and pass-through
// output of the sliding `#window.length(N)` on gfx950.
//
// LengthWindowProcessor.process (core/query/processor/stream/window/LengthWindowProcessor.java:106-142)
// keeps a count and one FIFO of the last N passing events. Numbering the passing events of the query's
// lifetime g = 0, 1, 2, ..., arrivals 0 .. N-1 only enter; from arrival N on, arrival g first polls the
// head — arrival g - N — re-stamps it with currentTime (read once per process call: the send's playback
// clock) and inserts it before the current event (insertBeforeCurrent). No scheduler, no TIMER chunk, no
// RESET. So where the time window searches two monotone sequences (sh_slx_kernels.hip), everything here
// is arithmetic on ordinals:
//   - arrival g leaves at the point of arrival g + N, the push's record g + N - G0 (G0 = the passing
//     events before the push), if the push reaches it;
//   - before and at the point of record i, max(0, G0 + i - N + 1) arrivals have left in all, X0 of them
//     in earlier pushes: the add of record i is operation i + max(0, G0 + i - N + 1 - X0) of the push and
//     the remove of its own point sits one before;
//   - an operation's chunk is the send of the record at whose point it happens.
// The kernel writes what k_slx_walk / k_slx_wkey / k_slx_pass read (per record the add's operation index,
// per window position the remove's operation index, chunk, stamp and flush clock), and appends the
// push's records to the carried FIFO of unexpired arrivals (ordinal, stream index; at most N entries).
#include "sh_device.h"
#include "sh_sliding.h"

namespace shd {

namespace {
constexpr u64 kNoOp = ~0ull;
}

// one thread per window position u of U = [carried unexpired arrivals (W0) | the push's records (M)];
// arrival of position u = X0 + u, and X0 + W0 = G0
__global__ __launch_bounds__(kBlock) void k_len_ops(i64 n_u, i64 W0, i64 M, i64 X0, i64 G0, i64 L, i64 seq_base,
                                                   i64 send_size, SlRecords rec, const i64* __restrict__ rsclk,
                                                   i64* upm, i64* useq, u64* xop, i64* xch, i64* xts, i64* xclk,
                                                   u64* aop, u64* xx, u64* xa) {
    const i64 u = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (u >= n_u) return;
    i64 ev;  // the position's event (global stream index)
    if (u >= W0) {
        // a record of this push: it joins the FIFO, and its add follows every remove up to its own point
        const i64 i = u - W0;
        const u32 raw = rec.raw[i];
        ev = seq_base + (i64)raw;
        upm[u] = G0 + i;
        useq[u] = ev;
        const u64 op = (u64)(i + min(max((i64)0, G0 + i - L + 1 - X0), u));
        if (xa) {
            ulonglong2* o = (ulonglong2*)(xa + (size_t)i * kXaWords);
            o[0] = make_ulonglong2(op, rec.vals[i]);
            o[1] = make_ulonglong2((u64)rec.ts[i], (u64)rsclk[i]);
            o[2] = make_ulonglong2((u64)raw, (u64)(G0 + i));
        } else {
            aop[i] = op;
        }
    } else {
        ev = useq[u];
    }
    // the remove: at the point of record ie = arrival + N - G0, when the push has that record
    const i64 ie = X0 + u + L - G0;
    u64 op = kNoOp;
    i64 c_ch = 0, c_clk = 0;
    if (ie >= 0 && ie < M) {
        op = (u64)(u + ie);
        c_ch = 2 * (send_size > 0 ? (i64)rec.raw[ie] / send_size : 0) + 1;
        c_clk = rsclk[ie];  // currentTime of the send: the expired copy's timestamp and the flush clock
    }
    if (xx) {
        ulonglong2* o = (ulonglong2*)(xx + (size_t)u * kXaWords);
        o[0] = make_ulonglong2(op, u >= W0 ? rec.vals[u - W0] : 0ull);
        o[1] = make_ulonglong2((u64)c_clk, (u64)c_clk);
        o[2] = make_ulonglong2((u64)ev, (u64)c_ch);
    } else {
        if (op != kNoOp) {
            xch[u] = c_ch;
            xts[u] = c_clk;
            xclk[u] = c_clk;
        }
        xop[u] = op;
    }
}

void launch_len_ops(hipStream_t s, i64 n_u, i64 W0, i64 M, i64 X0, i64 G0, i64 L, i64 seq_base, i64 send_size,
                    SlRecords rec, const i64* rsclk, i64* upm, i64* useq, u64* xop, i64* xch, i64* xts, i64* xclk,
                    u64* aop, u64* xx, u64* xa) {
    if (n_u <= 0) return;
    hipLaunchKernelGGL(k_len_ops, dim3((unsigned)((n_u + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n_u, W0, M, X0, G0,
                       L, seq_base, send_size, rec, rsclk, upm, useq, xop, xch, xts, xclk, aop, xx, xa);
}

}  // namespace shd
