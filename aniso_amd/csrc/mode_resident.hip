// mode_resident.hip -- one mode's resident factor blocks on a high-order handle (np = 6, 8)
// and the fp64 MFMA M2L that streams them.
//
// k_ho_m2l_mode (mode_apply.hip) forms the factor (E / r) T_id(c) of every entry of every
// E block again for every chunk of columns and every pass of a solve.  It depends on the
// medium and the mode only, so here it is formed once per stored pair, kept where the E
// block is kept (same block index, same R x R doubles), and the M2L becomes
//     local(R x 16) += +-F(R x R) . mult(R x 16)
// on v_mfma_f64_16x16x4_f64 with the block as the only operand that comes from HBM.
//
// In-block layout: 4 x 4 microtiles of 16 doubles = one 128-B line each, microtile (A, B)
// of the MT x MT grid (MT = R / 4) at line A * MT + B, element (a, b) of the block
// (a: point of the owner = the stored target, b: point of the source) at offset
// 4 * (a % 4) + (b % 4) of microtile (a / 4, b / 4).  The MFMA's A operand gives lane
// (r = lane & 15, h = lane >> 4) row r of the wave's 16-row tile and k index h of the step:
//   straight:   lane (r, h) reads row (r % 4) of microtiles (row / 4, 4 kg + h), kg = 0 ..:
//               one 32-B load per four k-steps, the k index of step (kg, e) being
//               16 kg + 4 h + e; a wave's load covers 16 whole lines;
//   transposed: the partner end of a V pair needs F^T with the sign (-1)^id
//               (T_id(-c) = (-1)^id T_id(c), r unchanged: the stored bits serve both ends).
//               Lane (r, h) reads column (row % 4) of microtiles (4 kg + h, row / 4): four
//               8-B loads at stride 32 B, and the four lanes of a microtile read its whole
//               line over the four loads.
//   np = 6 (MT = 9): two full groups and one tail step on microtile column (row) 8, whose k
//               index is 32 + h; the third 16-row tile holds rows 32 .. 35 and zeros.
// The B operand is the source's multipole, staged per pair in LDS as [k][16 columns] with
// the rows of one step adjacent (512 B, no bank conflict), double-buffered: one barrier
// per pair.  The 16 columns come from up to two expansion buffers of the mode kernels'
// layout [node][R][K]: columns 0 .. KA-1 of multA, 8 .. 8+KB-1 of multB, the others zero.
// A column never meets another in an MFMA, so its bits do not depend on the others.
// One workgroup per target node, pairs in list order, no atomics: repeats are bitwise equal.
// A form that also keeps the next pair's block in flight across the barrier (16 / 9 more
// doubles per lane, 4 waves per SIMD) measured the same spans: the launch is bound by the
// bytes it moves, each stored V block once from each end, not by latency.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"
#include "kernels.hpp"
#include "mode_factor.hpp"

namespace aniso {

typedef double f64x4r __attribute__((ext_vector_type(4)));

// the blocks of mode id from the E blocks, one workgroup per stored pair (owner: its
// target node, other: its source node); E[pair][s * R + t] as launch_ho_cache_att leaves it
template <int NP>
__global__ void __launch_bounds__(256) k_ho_mode_blocks(const int* __restrict__ owner, const int* __restrict__ other,
                                                        const double* __restrict__ E, const double* __restrict__ ncx,
                                                        const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                        const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                        int id, double* __restrict__ F) {
    constexpr int R = NP * NP, MT = R / 4;
    __shared__ double TX[R], TY[R], SX[R], SY[R];
    const int tid = threadIdx.x;
    const int n = owner[blockIdx.x], B = other[blockIdx.x];
    if (tid < R) {
        TX[tid] = ncx[n] + nrx[n] * T->cheb[tid % NP];
        TY[tid] = ncy[n] + nry[n] * T->cheb[tid / NP];
        SX[tid] = ncx[B] + nrx[B] * T->cheb[tid % NP];
        SY[tid] = ncy[B] + nry[B] * T->cheb[tid / NP];
    }
    __syncthreads();
    const double* Eb = E + (size_t)blockIdx.x * (R * R);
    double* Fb = F + (size_t)blockIdx.x * (R * R);
    for (int i = tid; i < R * R; i += 256) {
        const int s = i / R, t = i % R;
        const double dy = SY[s] - TY[t];
        const double f = mode_factor<false>(Eb[i], SX[s] - TX[t], dy * dy, id);
        Fb[((t >> 2) * MT + (s >> 2)) * 16 + (t & 3) * 4 + (s & 3)] = f;
    }
}

// LDS row of k index b of the staged multipole: within a full group of 16 the rows of one
// MFMA step (k = 16 kg + 4 h + e, h = 0 .. 3) are adjacent
template <int FULL>
__device__ __forceinline__ int stage_row(int b) {
    return b < FULL ? ((b & ~15) | ((b & 3) << 2) | ((b >> 2) & 3)) : b;
}

template <int NP>
__global__ void __launch_bounds__(64 * ((NP * NP + 15) / 16))
    k_ho_m2l_resident(const int* __restrict__ tgt, const int64_t* __restrict__ ptr, const int* __restrict__ src,
                      const int* __restrict__ blk, const double* __restrict__ F, double sgn,
                      const double* __restrict__ multA, int KA, const double* __restrict__ multB, int KB,
                      double* __restrict__ localA, double* __restrict__ localB) {
    constexpr int R = NP * NP, MT = R / 4, NT = (R + 15) / 16, KG = MT / 4, TAIL = MT % 4, NTH = 64 * NT;
    constexpr int STEPS = 4 * KG + TAIL, FULL = 16 * KG, NX = R * 16 / NTH;
    static_assert(TAIL <= 1, "at most one tail microtile column");
    static_assert(NX * NTH == R * 16, "whole staging rounds");
    __shared__ double X[2][R * 16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, h = lane >> 4;
    const int row = 16 * w + r;
    const bool rowOk = row < R;
    const int n = tgt[blockIdx.x];
    f64x4r acc = {0.0, 0.0, 0.0, 0.0};
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    // the A operand of pair e: this lane's row of the block, one value per MFMA step
    auto load_a = [&](int64_t e, double (&a)[STEPS]) {
        const int b = blk[e];
        const bool tr = b < 0;  // (workgroup-uniform)
        const double* Fb = F + (size_t)(tr ? ~b : b) * (R * R);
        if (!rowOk) {
#pragma unroll
            for (int i = 0; i < STEPS; ++i) a[i] = 0.0;
        } else if (!tr) {
            const double* p = Fb + ((row >> 2) * MT + h) * 16 + (row & 3) * 4;
#pragma unroll
            for (int kg = 0; kg < KG; ++kg) {
                const f64x4r v = __builtin_nontemporal_load(reinterpret_cast<const f64x4r*>(p + kg * 64));
#pragma unroll
                for (int i = 0; i < 4; ++i) a[4 * kg + i] = v[i];
            }
            if constexpr (TAIL) a[4 * KG] = __builtin_nontemporal_load(p + (4 * KG - h) * 16 + h);
        } else {
            const double* p = Fb + (h * MT + (row >> 2)) * 16 + (row & 3);
#pragma unroll
            for (int kg = 0; kg < KG; ++kg)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a[4 * kg + i] = sgn * __builtin_nontemporal_load(p + kg * (4 * MT * 16) + 4 * i);
            if constexpr (TAIL) a[4 * KG] = sgn * __builtin_nontemporal_load(p + (4 * KG - h) * (MT * 16) + 4 * h);
        }
    };
    int buf = 0;
    for (int64_t e = p0; e < p1; ++e, buf ^= 1) {
        double a[STEPS];
        load_a(e, a);
        // the source's multipole, 16 columns wide (the block loads above are in flight)
        const int B = src[e];
        double xv[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int k = (tid + i * NTH) >> 4, j = tid & 15;
            double v = 0.0;
            if (j < KA) v = multA[((size_t)B * R + k) * KA + j];
            else if (j >= 8 && j - 8 < KB) v = multB[((size_t)B * R + k) * KB + (j - 8)];
            xv[i] = v;
        }
        double* Xb = X[buf];
#pragma unroll
        for (int i = 0; i < NX; ++i) Xb[stage_row<FULL>((tid + i * NTH) >> 4) * 16 + (tid & 15)] = xv[i];
        __syncthreads();  // (the other buffer is rewritten only after the next barrier)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 * kg + i], Xb[(16 * kg + 4 * i + h) * 16 + r], acc, 0, 0, 0);
        if constexpr (TAIL) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 * KG], Xb[(FULL + h) * 16 + r], acc, 0, 0, 0);
    }
    // accumulator element i of lane (r, h): row h + 4 i of the tile, column r
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = 16 * w + h + 4 * i;
        if (t >= R) continue;
        if (r < KA) localA[((size_t)n * R + t) * KA + r] = acc[i];
        else if (r >= 8 && r - 8 < KB) localB[((size_t)n * R + t) * KB + (r - 8)] = acc[i];
    }
}

void launch_ho_mode_blocks(int np, int id, int64_t npairs, const int* owner, const int* other, const double* E,
                           const NodeBoxes& b, const HoTables* T, double* F, hipStream_t s) {
    if (npairs <= 0) return;
    if (id < 0) throw std::invalid_argument("resident mode blocks: negative mode");
    if (np == 6) k_ho_mode_blocks<6><<<(unsigned)npairs, 256, 0, s>>>(owner, other, E, b.cx, b.cy, b.rx, b.ry, T, id, F);
    else if (np == 8) k_ho_mode_blocks<8><<<(unsigned)npairs, 256, 0, s>>>(owner, other, E, b.cx, b.cy, b.rx, b.ry, T, id, F);
    else throw std::invalid_argument("resident mode blocks: np must be 6 or 8");
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2l_resident(int np, int id, const PairList& pl, const double* F, const double* multA, int KA,
                            const double* multB, int KB, double* localA, double* localB, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (id < 0) throw std::invalid_argument("resident mode apply: negative mode");
    if (KA < 1 || KA > 8 || KB < 0 || KB > 8 || (KB > 0 && (!multB || !localB)))
        throw std::invalid_argument("resident mode apply: unsupported column counts " + std::to_string(KA) + " + " +
                                    std::to_string(KB));
    const double sgn = (id & 1) ? -1.0 : 1.0;
    if (np == 6)
        k_ho_m2l_resident<6><<<pl.ntgt, 192, 0, s>>>(pl.tgt, pl.ptr, pl.src, pl.blk, F, sgn, multA, KA, multB, KB, localA,
                                                     localB);
    else if (np == 8)
        k_ho_m2l_resident<8><<<pl.ntgt, 256, 0, s>>>(pl.tgt, pl.ptr, pl.src, pl.blk, F, sgn, multA, KA, multB, KB, localA,
                                                     localB);
    else
        throw std::invalid_argument("resident mode apply: np must be 6 or 8");
    HIP_LAUNCH_CHECK();
}

}  // namespace aniso
