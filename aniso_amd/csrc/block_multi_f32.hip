// block_multi_f32.hip -- the relaxed-precision block operator's M2L for several sources on a
// high-order handle (np = 6, 8): k_ho_m2l_src of block_multi.hip with the
// entry in fp32 (hm_rows_src_f32) on the float mirror of the M2L E array, under the rounding
// rules of k_ho_m2l_f32 (block_f32.hip).  What an entry costs that does not depend on the
// source is formed once in fp32; per source it spends 2K fp32 FMAs, half the fp64 kernel's
// issue cost.  A source's chain is hm_entry_f32's, so its local expansion is bit for bit
// what k_ho_m2l_f32 stores for it alone, whatever S and its slot.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"

namespace aniso {

// a source's row of staged multipoles: K floats rounded up to whole 8- or 16-byte vectors
// (K = 5: 8 floats, two 16-byte reads instead of five 4-byte ones)
template <int K>
inline constexpr int kStrideF32 = K <= 2 ? 2 : K <= 4 ? 4 : 8;

// k_ho_m2l_src's shape: one workgroup per target node, thread (row t, column phase ph), a
// transposed block through the LDS tile (row stride R + 1), the weighted multipoles of all S
// sources staged per pair as XW[column][source][KS] (a wave's lanes read one or two columns,
// so the reads broadcast), K x S accumulators per thread, and the phase sum in phase order
// one source at a time through the tile.  The source's nodes are staged as (ncx[B] - ncx[n]) +
// nrx[B] cheb in fp64 and then rounded, the thread's own offset is nrx[n] cheb; hw_b mult_j[B]
// is formed in fp64 and rounded when staged; om_i x the float sum is stored as double.  No
// atomics, no workgroup waits for another.  Columns in flight: k_ho_m2l_f32's (DESIGN.md
// §3.18.10 keeps the other form's figure).
template <int NP, int K, int S>
__global__ void __launch_bounds__(256) k_ho_m2l_src_f32(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                        const int* __restrict__ src, const int* __restrict__ blk,
                                                        const float* __restrict__ E, const double* __restrict__ ncx,
                                                        const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                        const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                        HarmWeights hw, const double* __restrict__ mult,
                                                        int64_t mstride, double* __restrict__ local, int64_t lstride) {
    constexpr int R = NP * NP, RK = R * K, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 8 : 3;  // NC = 16 / 6
    constexpr int KS = kStrideF32<K>;
    static_assert(NC % G == 0, "whole column groups");
    constexpr int TILE = R * LD > NPH * RK ? R * LD : NPH * RK;
    __shared__ __attribute__((aligned(16))) float XW[R * S * KS];
    __shared__ float SX[R], SY[R], TL[TILE];
    static_assert(sizeof(float) * (R * S * KS + 2 * R + TILE) <= 64 * 1024, "at most 64 KB of LDS per workgroup");
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double cx = ncx[n], cy = ncy[n];
    const float bx = (float)(nrx[n] * T->cheb[t % NP]);
    const float by = (float)(nry[n] * T->cheb[t / NP]);
    float c[S][K];
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) c[j][i] = 0.0f;
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const float* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const double* mj = mult + (size_t)j * mstride + (size_t)B * RK;
            for (int i = tid; i < RK; i += 256) XW[((i / K) * S + j) * KS + i % K] = (float)(hw.hw[i % K] * mj[i]);
        }
        if (tid < R) {
            SX[tid] = (float)((ncx[B] - cx) + nrx[B] * T->cheb[tid % NP]);
            SY[tid] = (float)((ncy[B] - cy) + nry[B] * T->cheb[tid / NP]);
        }
        if (tr)
            for (int i = tid; i < R * R; i += 256) TL[(i / R) * LD + (i % R)] = Eb[i];
        __syncthreads();
        // G columns in flight per thread (their loads issued together)
#pragma unroll 1
        for (int g = 0; g < NC; g += G) {
            float ev[G];
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int s = min(ph + NPH * (g + i), R - 1);  // clamped: a valid address, skipped below
                ev[i] = tr ? TL[t * LD + s] : Eb[s * R + t];
            }
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int s = ph + NPH * (g + i);
                if (active && s < R) {
                    float xw[S][K];
#pragma unroll
                    for (int j = 0; j < S; ++j)
#pragma unroll
                        for (int bb = 0; bb < K; ++bb) xw[j][bb] = XW[(s * S + j) * KS + bb];
                    const float dy = SY[s] - by;
                    hm_rows_src_f32<K, S>(ev[i], SX[s] - bx, dy * dy, xw, c);
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
            float v = TL[i];
#pragma unroll
            for (int p = 1; p < NPH; ++p) v += TL[p * RK + i];
            lj[i] = hw.om[i % K] * (double)v;
        }
    }
}

// ----------------------------------------------------------------- launcher

#define ANISO_SRC_F32_CASE(np, k, ns)                                                                            \
    case ((np) * 16 + (k)) * 8 + (ns):                                                                           \
        k_ho_m2l_src_f32<np, k, ns><<<ntgt, 256, 0, s>>>(tgt, ptr, src, blk, E, ncx, ncy, nrx, nry, T, hw, mult, \
                                                         mstride, local, lstride);                               \
        break;
#define ANISO_SRC_F32_CASES(np, k) \
    ANISO_SRC_F32_CASE(np, k, 1) ANISO_SRC_F32_CASE(np, k, 2) ANISO_SRC_F32_CASE(np, k, 4)

void launch_ho_m2l_src_f32(int np, int K, int S, const PairList& pl, const float* E, const NodeBoxes& b,
                           const HoTables* T, const HarmWeights& hw, const double* mult, int64_t mstride,
                           double* local, int64_t lstride, hipStream_t s) {
    const auto [ntgt, tgt, ptr, src, blk] = pl;  // (the names ANISO_SRC_F32_CASE passes on)
    const auto [ncx, ncy, nrx, nry] = b;
    if (ntgt <= 0) return;
    switch ((np * 16 + K) * 8 + S) {
        ANISO_SRC_F32_CASES(6, 2)
        ANISO_SRC_F32_CASES(6, 4)
        ANISO_SRC_F32_CASES(6, 5)
        ANISO_SRC_F32_CASES(6, 8)
        ANISO_SRC_F32_CASES(8, 2)
        ANISO_SRC_F32_CASES(8, 4)
        ANISO_SRC_F32_CASES(8, 5)
        ANISO_SRC_F32_CASES(8, 8)
        default:
            throw std::invalid_argument("f32 multi-source M2L: unsupported order / block count / source count " +
                                        std::to_string(np) + " / " + std::to_string(K) + " / " + std::to_string(S));
    }
    HIP_LAUNCH_CHECK();
}

#undef ANISO_SRC_F32_CASES
#undef ANISO_SRC_F32_CASE

}  // namespace aniso
