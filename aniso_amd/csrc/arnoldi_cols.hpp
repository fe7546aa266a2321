// arnoldi_cols.hpp -- the fp64 DCGS2 sweeps of arnoldi.hpp for several independent
// columns in one launch (the multi-source forward solve).  Every
// column has a basis, a state block and partials of its own; blockIdx.y is the slot of
// a by-value table of at most kMaxCols descriptors, so one launch serves all the
// columns still active at a step.  Per column the launch shape (kSweepThreads x kParts),
// the element ranges and the order of every sum are those of the one-column kernels:
// no atomics, and a column's bits do not depend on which other columns run beside it.
#pragma once

#include "arnoldi.hpp"

namespace aniso {
namespace arn {

constexpr int kMaxCols = 16;    // slots per launch: the widest group of a solve (the wide forward solve)
constexpr int kNarrowCols = 8;  // a group of every other solve

struct ColSlot {
    double* V;        // the column's basis (rows at the table's ldv)
    const double* w;  // the operator's output row of this step
    const double* b;  // the right-hand side (k_arn_resid_cols)
    double* part;     // sweep partials, row k at part + k * kParts
    double* st;       // state block (Layout)
    double* x;        // the solution row (k_arn_axpy_cols)
    int used;         // basis rows the solution update takes
    int pad;
};

struct ColTable {
    ColSlot c[kMaxCols];
};

// dst[slot * n + e] = V[row][e]: the active columns' vectors as compact rows for the operator
__global__ void __launch_bounds__(kThreads) k_arn_gather_cols(int64_t n, int row, int64_t ldv, ColTable t,
                                                              double* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const double* __restrict__ v = t.c[blockIdx.y].V + (size_t)row * ldv;
    dst[(size_t)blockIdx.y * n + e] = v[e];
}

// V[0] = b - w: the residual that starts a cycle (w = A x)
__global__ void __launch_bounds__(kThreads) k_arn_resid_cols(int64_t n, ColTable t) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const ColSlot& c = t.c[blockIdx.y];
    c.V[e] = c.b[e] - c.w[e];
}

// sweep A (k_arn_project) per slot: part[k][blk] = sum over the block's range of V[k][e] w[e]
template <int NV, int TB = kSweepThreads>
__global__ void __launch_bounds__(TB) k_arn_project_cols(int64_t n, int nv, int row0, int64_t ldv, ColTable t) {
    __shared__ double red[(TB / 64) * NV];
    const double* __restrict__ V = t.c[blockIdx.y].V + (size_t)row0 * ldv;
    const double* __restrict__ w = t.c[blockIdx.y].w;
    double* __restrict__ part = t.c[blockIdx.y].part + (size_t)row0 * kParts;
    int64_t j0, j1;
    block_range(n, blockIdx.x, j0, j1);
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int64_t e = j0 + threadIdx.x; e < j1; e += TB) {
        double v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (k < nv) v[k] = V[(size_t)k * ldv + e];
        const double we = w[e];
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (k < nv) acc[k] = __builtin_fma(v[k], we, acc[k]);
    }
    block_store<NV, TB>(acc, nv, -1, red, part, blockIdx.x);
}

// sweep B (k_arn_update, variant 0) per slot for nv <= NV stored rows: p = w inv_r - sum_k
// e_k V_k -> V[nv]; the partials of V_k . p (rows k < nv) and p . p (row nv)
template <int NV, int TB = kSweepThreads>
__global__ void __launch_bounds__(TB) k_arn_update_cols(int64_t n, int nv, int64_t ldv, int m, ColTable t) {
    constexpr int NA = NV + 1;
    __shared__ double red[(TB / 64) * NA];
    __shared__ double cf[NV + 1];  // -e[0 .. nv), inv_r
    double* __restrict__ V = t.c[blockIdx.y].V;
    const double* __restrict__ w = t.c[blockIdx.y].w;
    const double* __restrict__ st = t.c[blockIdx.y].st;
    double* __restrict__ part = t.c[blockIdx.y].part;
    const Layout L(m);
    for (int k = threadIdx.x; k < NV; k += TB) cf[k] = k < nv ? -st[L.e + k] : 0.0;
    if (threadIdx.x == 0) cf[NV] = st[L.sc + kInvR];
    __syncthreads();
    const double ir = cf[NV];
    const int b = blockIdx.x;
    int64_t j0, j1;
    block_range(n, b, j0, j1);
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    double* __restrict__ Vn = V + (size_t)nv * ldv;
    // the store of the previous element's p goes after this element's loads (k_arn_update)
    double pPrev = 0.0;
    int64_t ePrev = j0 + threadIdx.x;
    for (int64_t e = j0 + threadIdx.x; e < j1; e += TB) {
        double v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = V[(size_t)(k < nv ? k : nv - 1) * ldv + e];
        const double we = w[e];
        asm volatile("" ::: "memory");
        Vn[ePrev] = pPrev;
        double p = we * ir;
#pragma unroll
        for (int k = 0; k < NV; ++k) p = __builtin_fma(cf[k], v[k], p);
        pPrev = p;
        ePrev = e;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] = __builtin_fma(v[k], p, acc[k]);  // rows >= nv: not stored
        acc[NA - 1] = __builtin_fma(p, p, acc[NA - 1]);
    }
    if (ePrev < j1) Vn[ePrev] = pPrev;
    block_store<NA, TB>(acc, nv, nv, red, part, b);
}

// sweep B beyond kMaxRegs rows, first half (k_arn_update_wide) per slot: p -> V[nv]; the
// partials then come from k_arn_project_cols over V[0 .. nv] with w = p
__global__ void __launch_bounds__(kThreads) k_arn_update_wide_cols(int64_t n, int nv, int64_t ldv, int m, ColTable t) {
    extern __shared__ double cw[];  // -e[0 .. nv)
    double* __restrict__ V = t.c[blockIdx.y].V;
    const double* __restrict__ w = t.c[blockIdx.y].w;
    const double* __restrict__ st = t.c[blockIdx.y].st;
    const Layout L(m);
    for (int k = threadIdx.x; k < nv; k += kThreads) cw[k] = -st[L.e + k];
    __syncthreads();
    const double ir = st[L.sc + kInvR];
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    double p = w[e] * ir;
    for (int k = 0; k < nv; ++k) p = __builtin_fma(cw[k], V[(size_t)k * ldv + e], p);
    V[(size_t)nv * ldv + e] = p;
}

// the cycle's update (k_arn_axpy) per slot, every column with its own row count:
// x[e] += sum_{k < used} y[k] V[k][e] (y: the state block's update coefficients)
__global__ void __launch_bounds__(kThreads) k_arn_axpy_cols(int64_t n, int64_t ldv, int m, ColTable t) {
    extern __shared__ double ys[];
    const ColSlot& c = t.c[blockIdx.y];
    const int nv = c.used;
    const double* __restrict__ y = c.st + Layout(m).y;
    for (int k = threadIdx.x; k < nv; k += kThreads) ys[k] = y[k];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const double* __restrict__ V = c.V;
    double* __restrict__ x = c.x;
    double a = x[e];
    for (int k = 0; k < nv; ++k) a = __builtin_fma(ys[k], V[(size_t)k * ldv + e], a);
    x[e] = a;
}

// out[slot] = the sum of row 0 of the slot's partials (|v|^2 after a one-row sweep A), in
// reduce_rows' fixed order
__global__ void __launch_bounds__(kThreads) k_arn_sums_cols(ColTable t, double* __restrict__ out) {
    __shared__ double scratch[kRedRows * 64];
    __shared__ double a[1];
    reduce_rows(t.c[blockIdx.x].part, kParts, kParts, 1, a, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = a[0];
}

// ---- host launchers (nslots <= kMaxCols slots of t)

// sweep A over rows 0 .. nv - 1 of every slot, in groups of kMaxRegs rows
inline void launch_project_cols(int64_t n, int nv, int64_t ldv, const ColTable& t, int nslots, hipStream_t s) {
    for (int k0 = 0; k0 < nv; k0 += kMaxRegs) {
        const int g = nv - k0 < kMaxRegs ? nv - k0 : kMaxRegs;
        nv_dispatch(g, [&](auto c) {
            k_arn_project_cols<decltype(c)::value><<<dim3(kParts, nslots), kSweepThreads, 0, s>>>(n, g, k0, ldv, t);
        });
    }
}

// sweep B of step j (nv = j + 1 stored rows) of every slot: V[nv] written, part rows 0 .. nv
inline void launch_update_cols(int64_t n, int nv, int64_t ldv, int m, const ColTable& t, int nslots, hipStream_t s) {
    if (nv <= kMaxRegs) {
        nv_dispatch(nv, [&](auto c) {
            k_arn_update_cols<decltype(c)::value><<<dim3(kParts, nslots), kSweepThreads, 0, s>>>(n, nv, ldv, m, t);
        });
        return;
    }
    k_arn_update_wide_cols<<<dim3((unsigned)((n + kThreads - 1) / kThreads), nslots), kThreads,
                             (size_t)nv * sizeof(double), s>>>(n, nv, ldv, m, t);
    ColTable tp = t;  // the second half reads p where the first wrote it
    for (int a = 0; a < nslots; ++a) tp.c[a].w = t.c[a].V + (size_t)nv * ldv;
    launch_project_cols(n, nv + 1, ldv, tp, nslots, s);
}

}  // namespace arn
}  // namespace aniso
