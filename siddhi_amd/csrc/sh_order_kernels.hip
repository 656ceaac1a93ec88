// sh_order_kernels.hip — the kernels of `order by` / `limit` / `offset` (sh_order.h, sh_order.cpp), gfx950.
//
// A call's rows lie flush after flush; a sort never moves a row out of its type run, so every kernel
// addresses rows by their position in the call. Bytes per row (nk key columns, na aggregates, t terms):
//   k_ord_keys    reads 1 + t * (8 + 1), writes 4 + t * 16           (global route)
//   k_ord_pick    reads 8 + 4, writes 8 (+ 4)                          (global route, once per radix pass)
//   k_ord_block   reads 1 + t * (8 + 1), writes 4; the keys stay in LDS (block route)
//   k_ord_cut     reads 4 + 1, writes 4
//   k_ord_gather  reads 8 + 4 and, per kept row, 17 + 8 * nk + 9 * na, which it writes
#include <hip/hip_runtime.h>

#include "sh_order.h"
#include "../../include/siddhi_hip.h"

namespace shd {

namespace {

// the flush holding position i: the last f with foff[f] <= i (empty flushes never hold a position)
__device__ inline int ord_flush_of(const i64* foff, int nf, i64 i) {
    int lo = 0, hi = nf;  // foff[lo] <= i < foff[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (foff[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Term t of row `row`: the null flag and the image whose unsigned order is the comparator's order.
// Integers: the sign bit flipped. Doubles (Double.compareTo): NaN canonicalised, then negative values
// inverted and the others given the top bit, so -0.0 < 0.0 and NaN lies above +Infinity. `desc` inverts
// the image, never the null flag; a null's image is 0 (two nulls compare equal: the next term decides).
__device__ inline u64 ord_image(const OrdSpec& sp, const OrdRows& in, i64 row, int t, u32* null_out) {
    const int c = sp.index[t];
    u64 v;
    u32 nl = 0;
    if (sp.kind[t] == SH_ORD_KEY) {
        v = (u64)in.keys[(i64)c * in.stride + row];
    } else {
        v = in.vals[(i64)c * in.stride + row];
        nl = in.nulls[(i64)c * in.stride + row] ? 1u : 0u;
    }
    *null_out = nl;
    if (nl) return 0;
    const u64 top = 0x8000000000000000ull;
    if (sp.image[t] == kOrdDouble) {
        if ((v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) v = 0x7FF8000000000000ull;
        v = (v & top) ? ~v : (v | top);
    } else {
        v ^= top;
    }
    return sp.desc[t] ? ~v : v;
}

__global__ __launch_bounds__(256) void k_ord_keys(OrdSpec sp, OrdRows in, i64 n, const i64* foff, int nf, u32* head,
                                                  u64* img, u64* nul) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { head[n] = 0; return; }
    const int f = ord_flush_of(foff, nf, i);
    head[i] = (i == foff[f] || in.expired[i] != in.expired[i - 1]) ? 1u : 0u;
#pragma unroll
    for (int t = 0; t < kOrdMaxTerms; t++) {
        if (t < sp.n_terms) {
            u32 nl;
            img[(i64)t * n + i] = ord_image(sp, in, i, t, &nl);
            if (sp.nullable[t]) nul[(i64)t * n + i] = nl;
        }
    }
}

__global__ __launch_bounds__(256) void k_ord_pick(i64 n, const u64* col, const u32* col32, const u32* perm, u64* key,
                                                  u32* iota) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const i64 src = perm ? (i64)perm[j] : j;
    // a 64-bit column, a 32-bit one, or the 32-bit one above the other's low bit (run number | null flag)
    key[j] = !col32 ? col[src] : !col ? (u64)col32[src] : ((u64)col32[src] << 1) | (col[src] & 1);
    if (iota) iota[j] = (u32)j;
}

constexpr int kOrdPerThread = kOrdBlockRows / 256;

// One workgroup per flush. The rows' images and null bits go to LDS once; every row then counts the rows
// of its run that come before it under (term 0 .. term n-1, position) — a rank sort: stable by
// construction, no padding to a power of two, and a wave's lanes read the same LDS words (broadcast)
// while their runs coincide. m^2 comparisons for a flush of m rows: the route is for small flushes.
__global__ __launch_bounds__(256) void k_ord_block(OrdSpec sp, OrdRows in, const i64* foff, int nf, u32* perm) {
    __shared__ u64 s_img[kOrdMaxTerms][kOrdBlockRows];
    __shared__ u32 s_meta[kOrdBlockRows];  // the terms' null bits | head of a run << 8 | the run's first row << 16
    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    const i64 lo = foff[f];
    const i64 m64 = foff[f + 1] - lo;
    if (m64 <= 1 || m64 > kOrdBlockRows) {
        // one row, or a flush the caller should not have sent here: its rows keep their places
        for (i64 i = tid; i < m64; i += 256) perm[lo + i] = (u32)(lo + i);
        return;
    }
    const int m = (int)m64;
    for (int i = tid; i < m; i += 256) {
        const i64 row = lo + i;
        u32 meta = (i == 0 || in.expired[row] != in.expired[row - 1]) ? 0x100u : 0u;
#pragma unroll
        for (int t = 0; t < kOrdMaxTerms; t++) {
            if (t < sp.n_terms) {
                u32 nl;
                s_img[t][i] = ord_image(sp, in, row, t, &nl);
                meta |= nl << t;
            }
        }
        s_meta[i] = meta;
    }
    __syncthreads();
    int rs[kOrdPerThread];
#pragma unroll
    for (int r = 0; r < kOrdPerThread; r++) {
        const int i = tid + r * 256;
        int b = i < m ? i : 0;
        while (!(s_meta[b] & 0x100u)) b--;  // (row 0 heads a run)
        rs[r] = b;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kOrdPerThread; r++) {
        const int i = tid + r * 256;
        if (i < m) s_meta[i] |= (u32)rs[r] << 16;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kOrdPerThread; r++) {
        const int i = tid + r * 256;
        if (i >= m) continue;
        const u32 mi = s_meta[i];
        u64 a[kOrdMaxTerms];
#pragma unroll
        for (int t = 0; t < kOrdMaxTerms; t++) a[t] = t < sp.n_terms ? s_img[t][i] : 0;
        int rank = 0;
        for (int j = rs[r]; j < m; j++) {
            const u32 mj = s_meta[j];
            if ((int)(mj >> 16) != rs[r]) break;
            // c < 0: row j comes first by the terms; 0: they tie
            int c = 0;
#pragma unroll
            for (int t = 0; t < kOrdMaxTerms; t++) {
                if (t < sp.n_terms && c == 0) {
                    const u32 nj = (mj >> t) & 1u, ni = (mi >> t) & 1u;
                    const u64 b = s_img[t][j];
                    if (nj != ni) c = nj ? 1 : -1;  // the null row is last
                    else if (b != a[t]) c = b < a[t] ? -1 : 1;
                }
            }
            rank += (c < 0 || (c == 0 && j < i)) ? 1 : 0;
        }
        perm[lo + rs[r] + rank] = (u32)(lo + i);
    }
}

__global__ __launch_bounds__(256) void k_ord_cut(OrdSpec sp, const unsigned char* expired, const u32* perm, i64 n,
                                                 const i64* foff, int nf, u32* flag) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { flag[n] = 0; return; }
    bool keep;
    if (sp.single) {
        keep = sp.offset <= 0 && sp.limit != 0;
    } else {
        const i64 p = j - foff[ord_flush_of(foff, nf, j)];
        const i64 off = sp.offset > 0 ? sp.offset : 0;
        const i64 src = perm ? (i64)perm[j] : j;
        keep = p >= off && (expired[src] != 0 || sp.limit < 0 || p - off < sp.limit);
    }
    flag[j] = keep ? 1u : 0u;
}

__global__ void k_ord_counts(const u32* pre, const i64* foff, int nf, u32* cnt) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f <= nf) cnt[f] = pre[foff[f]];
}

__global__ __launch_bounds__(256) void k_ord_gather(const u32* flag, const u32* pre, const u32* perm, OrdRows in,
                                                    OrdRows out, i64 n, int nk, int na) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !flag[j]) return;
    const i64 src = perm ? (i64)perm[j] : j;
    const i64 o = pre[j];
    out.ts[o] = in.ts[src];
    out.expired[o] = in.expired[src];
    out.rep[o] = in.rep[src];
    for (int k = 0; k < nk; k++) out.keys[(i64)k * out.stride + o] = in.keys[(i64)k * in.stride + src];
    for (int a = 0; a < na; a++) {
        out.vals[(i64)a * out.stride + o] = in.vals[(i64)a * in.stride + src];
        out.nulls[(i64)a * out.stride + o] = in.nulls[(i64)a * in.stride + src];
    }
}

inline dim3 ord_grid(i64 n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

void launch_ord_keys(hipStream_t s, OrdSpec sp, OrdRows in, i64 n, const i64* foff, int nf, u32* head, u64* img, u64* nul) {
    hipLaunchKernelGGL(k_ord_keys, ord_grid(n + 1), dim3(256), 0, s, sp, in, n, foff, nf, head, img, nul);
}

void launch_ord_pick(hipStream_t s, i64 n, const u64* col, const u32* col32, const u32* perm, u64* key, u32* iota) {
    if (n > 0) hipLaunchKernelGGL(k_ord_pick, ord_grid(n), dim3(256), 0, s, n, col, col32, perm, key, iota);
}

void launch_ord_block(hipStream_t s, OrdSpec sp, OrdRows in, const i64* foff, int nf, u32* perm) {
    if (nf > 0) hipLaunchKernelGGL(k_ord_block, dim3((unsigned)nf), dim3(256), 0, s, sp, in, foff, nf, perm);
}

void launch_ord_cut(hipStream_t s, OrdSpec sp, const unsigned char* expired, const u32* perm, i64 n, const i64* foff,
                    int nf, u32* flag) {
    hipLaunchKernelGGL(k_ord_cut, ord_grid(n + 1), dim3(256), 0, s, sp, expired, perm, n, foff, nf, flag);
}

void launch_ord_counts(hipStream_t s, const u32* pre, const i64* foff, int nf, u32* cnt) {
    hipLaunchKernelGGL(k_ord_counts, ord_grid(nf + 1), dim3(256), 0, s, pre, foff, nf, cnt);
}

void launch_ord_gather(hipStream_t s, const u32* flag, const u32* pre, const u32* perm, OrdRows in, OrdRows out, i64 n,
                       int nk, int na) {
    if (n > 0) hipLaunchKernelGGL(k_ord_gather, ord_grid(n), dim3(256), 0, s, flag, pre, perm, in, out, n, nk, na);
}

}  // namespace shd
