// block_multi.hip -- the block operator's M2L for several sources on a high-order handle
// (np = 6, 8): k_ho_m2l of high_order.hip with S source vectors per
// read of a stored E block.
//
// The M2L of a high-order block matvec is bound by instructions per cache entry, and what
// an entry costs -- r^2, 1/r with two Newton steps, the Chebyshev recurrence, the loads of
// the source node's coordinates -- does not depend on the source vector.  hm_rows_src forms
// it once and spends 2K FMAs per source on it.  P2M / M2M before and L2L / L2P after the
// launch run per source on the kernels of high_order.hip: the S multipole and S local
// buffers are [node][R][K] each, addressed by a base pointer and a per-source stride.
// Every sum runs in a fixed order, there are no atomics and no workgroup waits for
// another; a source's arithmetic does not depend on S or on its slot.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"

namespace aniso {

// One workgroup per target node; thread (row t, column phase ph) of the NPH = 256 / R
// phases owns target row t and walks the columns s = ph, ph + NPH, ..., G of them in
// flight; a V pair stored once by its smaller id is read transposed through the LDS tile
// (row stride R + 1).  Per pair the weighted multipoles hw_b mult_j[B] of all S sources
// are staged as XW[column][source][KS] (KS = K rounded up to even: a source's row is whole
// 16-byte vectors; a wave's lanes read one or two columns, so the reads broadcast) beside
// the source box's Chebyshev nodes.  A thread keeps K x S accumulators.  The phases'
// partial rows are summed in phase order one source at a time through the tile, so the
// workgroup's LDS is the tile and the staged multipoles.
template <int NP, int K, int S>
__global__ void __launch_bounds__(256) k_ho_m2l_src(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                    const int* __restrict__ src, const int* __restrict__ blk,
                                                    const double* __restrict__ E, const double* __restrict__ ncx,
                                                    const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                    const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                    HarmWeights hw, const double* __restrict__ mult, int64_t mstride,
                                                    double* __restrict__ local, int64_t lstride) {
    constexpr int R = NP * NP, RK = R * K, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 4 : 3;  // NC = 16 / 6
    constexpr int KS = kStride<K>;
    static_assert(NC % G == 0, "whole column groups");
    constexpr int TILE = R * LD > NPH * RK ? R * LD : NPH * RK;
    __shared__ __attribute__((aligned(16))) double XW[R * S * KS];
    __shared__ double SX[R], SY[R], TL[TILE];
    static_assert(sizeof(double) * (R * S * KS + 2 * R + TILE) <= 64 * 1024, "at most 64 KB of LDS per workgroup");
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double bx = ncx[n] + nrx[n] * T->cheb[t % NP];
    const double by = ncy[n] + nry[n] * T->cheb[t / NP];
    double c[S][K];
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) c[j][i] = 0.0;
    if constexpr (KS != K) {  // the pad entries ride along in the 16-byte reads
        for (int i = tid; i < R * S; i += 256) XW[i * KS + K] = 0.0;
    }
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const double* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const double* mj = mult + (size_t)j * mstride + (size_t)B * RK;
            for (int i = tid; i < RK; i += 256) XW[((i / K) * S + j) * KS + i % K] = hw.hw[i % K] * mj[i];
        }
        if (tid < R) {
            SX[tid] = ncx[B] + nrx[B] * T->cheb[tid % NP];
            SY[tid] = ncy[B] + nry[B] * T->cheb[tid / NP];
        }
        if (tr)
            for (int i = tid; i < R * R; i += 256) TL[(i / R) * LD + (i % R)] = Eb[i];
        __syncthreads();
        // G columns in flight per thread (their loads issued together)
#pragma unroll 1
        for (int g = 0; g < NC; g += G) {
            double ev[G];
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int s = min(ph + NPH * (g + i), R - 1);  // clamped: a valid address, skipped below
                ev[i] = tr ? TL[t * LD + s] : Eb[s * R + t];
            }
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int s = ph + NPH * (g + i);
                if (active && s < R) {
                    double xw[S][K];
#pragma unroll
                    for (int j = 0; j < S; ++j) load_charges<K>(XW + (s * S + j) * KS, xw[j]);
                    const double dy = SY[s] - by;
                    hm_rows_src<K, S, 2>(ev[i], SX[s] - bx, dy * dy, xw, c);
                }
            }
        }
    }
    // the phases' partial rows, one source at a time through the tile
#pragma unroll
    for (int j = 0; j < S; ++j) {
        __syncthreads();  // the last pair's, or the previous source's, reads of the tile are done
        if (active) {
#pragma unroll
            for (int i = 0; i < K; ++i) TL[(ph * R + t) * K + i] = c[j][i];
        }
        __syncthreads();
        double* lj = local + (size_t)j * lstride + (size_t)n * RK;
        for (int i = tid; i < RK; i += 256) {
            double v = TL[i];
#pragma unroll
            for (int p = 1; p < NPH; ++p) v += TL[p * RK + i];
            lj[i] = hw.om[i % K] * v;
        }
    }
}

// ----------------------------------------------------------------- launcher

#define ANISO_SRC_CASE(np, k, ns)                                                                               \
    case ((np) * 16 + (k)) * 8 + (ns):                                                                           \
        k_ho_m2l_src<np, k, ns><<<ntgt, 256, 0, s>>>(tgt, ptr, src, blk, E, ncx, ncy, nrx, nry, T, hw, mult,     \
                                                     mstride, local, lstride);                                   \
        break;
#define ANISO_SRC_CASES(np, k) ANISO_SRC_CASE(np, k, 1) ANISO_SRC_CASE(np, k, 2) ANISO_SRC_CASE(np, k, 4)

void launch_ho_m2l_src(int np, int K, int S, const PairList& pl, const double* E, const NodeBoxes& b,
                       const HoTables* T, const HarmWeights& hw, const double* mult, int64_t mstride, double* local,
                       int64_t lstride, hipStream_t s) {
    const auto [ntgt, tgt, ptr, src, blk] = pl;  // (the names ANISO_SRC_CASE passes on)
    const auto [ncx, ncy, nrx, nry] = b;
    if (ntgt <= 0) return;
    switch ((np * 16 + K) * 8 + S) {
        ANISO_SRC_CASES(6, 2)
        ANISO_SRC_CASES(6, 4)
        ANISO_SRC_CASES(6, 5)
        ANISO_SRC_CASES(6, 8)
        ANISO_SRC_CASES(8, 2)
        ANISO_SRC_CASES(8, 4)
        ANISO_SRC_CASES(8, 5)
        ANISO_SRC_CASES(8, 8)
        default:
            throw std::invalid_argument("multi-source M2L: unsupported order / block count / source count " +
                                        std::to_string(np) + " / " + std::to_string(K) + " / " + std::to_string(S));
    }
    HIP_LAUNCH_CHECK();
}

#undef ANISO_SRC_CASES
#undef ANISO_SRC_CASE

}  // namespace aniso
