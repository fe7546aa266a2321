// block_f32.hip -- the relaxed-precision block operator of a high-order handle (np = 6, 8;
// DESIGN.md §3.18.8): k_ho_m2l of high_order.hip and the unstaged harmonic near field
// k_near_hm of harmonic.hip with the entry -- 1 / r, the recurrence for T_0 .. T_{K-1}, the
// products and the accumulators -- in fp32 (hm_entry_f32), on the float mirrors of the two
// E arrays (k_cache_f32 of mode_apply_f32.hip, same indexing).  Everything around them is
// the fp64 code: the weighted multipole hw_b x_b(s) and the weighted charges are formed in
// fp64 and rounded when they are staged, the local expansion and the near field's `out`
// are stored as double.
//
// The rules of mode_apply_f32.hip hold: no absolute coordinate is subtracted in fp32 (the
// M2L stages the source's nodes relative to the target's centre, the near field takes every
// point relative to the target leaf's centre, both in fp64 and then rounded); every sum
// runs in a fixed order and there are no atomics, so repeats are bitwise equal.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"

namespace aniso {

typedef float flt4 __attribute__((ext_vector_type(4)));

// ----------------------------------------------------------------- M2L

// k_ho_m2l in fp32: the same workgroup per target node, thread (row t, column phase ph),
// LDS tile for a transposed block and phase sum in phase order.  The source's nodes are
// staged as (ncx[B] - ncx[n]) + nrx[B] cheb in fp64 and then rounded; the thread's own offset
// is nrx[n] cheb.  om_i x the sum is stored as double.  One pair per barrier round, as the
// fp64 kernel (staging more pairs lost on the mode kernel).  Columns in
// flight, measured at 1M points, ks = 5: np = 8, G = 4 / 8: 3.31 / 3.21
// ms, so 8; np = 6, G = 3 / 6: 4.56 / 4.68 ms, so the fp64 kernel's 3.
template <int NP, int K>
__global__ void __launch_bounds__(256) k_ho_m2l_f32(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                    const int* __restrict__ src, const int* __restrict__ blk,
                                                    const float* __restrict__ E, const double* __restrict__ ncx,
                                                    const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                    const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                    HarmWeights hw, const double* __restrict__ mult,
                                                    double* __restrict__ local) {
    constexpr int R = NP * NP, RK = R * K, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 8 : 3;  // NC = 16 / 6
    static_assert(NC % G == 0, "whole column groups");
    constexpr int TILE = R * LD > NPH * RK ? R * LD : NPH * RK;
    __shared__ float XW[RK], SX[R], SY[R], TL[TILE];
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double cx = ncx[n], cy = ncy[n];
    const float bx = (float)(nrx[n] * T->cheb[t % NP]);
    const float by = (float)(nry[n] * T->cheb[t / NP]);
    float c[K];
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = 0.0f;
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const float* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
        for (int i = tid; i < RK; i += 256) XW[i] = (float)(hw.hw[i % K] * mult[(size_t)B * RK + i]);
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
                    float xw[K];
#pragma unroll
                    for (int bb = 0; bb < K; ++bb) xw[bb] = XW[s * K + bb];
                    const float dy = SY[s] - by;
                    hm_entry_f32<K, false>(ev[i], SX[s] - bx, dy * dy, xw, c);
                }
            }
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < K; ++i) TL[(ph * R + t) * K + i] = c[i];
    }
    __syncthreads();
    for (int i = tid; i < RK; i += 256) {
        float v = TL[i];
#pragma unroll
        for (int p = 1; p < NPH; ++p) v += TL[p * RK + i];
        local[(size_t)n * RK + i] = hw.om[i % K] * (double)v;
    }
}

// ----------------------------------------------------------------- near field

template <int CTRL>
__device__ __forceinline__ float dpp_blk_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// k_near_hm (whole operator, near field on) in fp32: the same lanes per leaf, row quads and
// column phases; a row quad of one column is one 16-B load, U columns in flight (measured at
// 1M points, ks = 5, U = 4 / 2: 0.358 / 0.350 ms at np = 6 and 0.931 / 0.830 ms at np = 8, so
// 2, which also keeps K = 8 at three waves per SIMD).  Every
// point is taken relative to the target leaf's centre (ncx, ncy of the leaf's node) in fp64
// and then rounded; the weighted charges hw_b f_b are formed in fp64 and rounded.  out is
// stored as double, the sigma_t diagonal, om and the scale applied in fp64.
template <int K, int G, int U>
__global__ void __launch_bounds__(256) k_near_hm_f32(int nl, const int4* __restrict__ leafInfo,
                                                     const int64_t* __restrict__ nearPtsPtr,
                                                     const int* __restrict__ nearPts,
                                                     const int64_t* __restrict__ nearKOff, const float* __restrict__ E,
                                                     const double* __restrict__ ncx, const double* __restrict__ ncy,
                                                     const double* __restrict__ pxT, const double* __restrict__ pyT,
                                                     const double* __restrict__ sigDiag, HarmWeights hw,
                                                     const double* __restrict__ fT, const int* __restrict__ operm,
                                                     int64_t obase, int64_t ldo, double scale,
                                                     double* __restrict__ out) {
    static_assert(G == 16 || G == 64, "leaf group of 16 or 64 lanes");
    constexpr int KS = kStride<K>;
    const int gl = threadIdx.x & (G - 1);
    const int li = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G);
    const bool active = li < nl;
    int4 info = make_int4(0, 0, 0, 0);
    int64_t pb = 0, koff = 0;
    double cx = 0.0, cy = 0.0;
    if (active) {
        info = leafInfo[li];
        pb = nearPtsPtr[li];
        koff = nearKOff[li];
        cx = ncx[info.x];
        cy = ncy[info.x];
    }
    const int nT = info.z, S = info.w;
    const int64_t tb = info.y;
    const int nq = (nT + 3) >> 2;  // row quads: the column stride in 16-B units
    int lpc = 4;                   // lanes per column (G = 16: leaves <= 16 points, 4 quads)
    if constexpr (G == 64) {
        lpc = 1;
        while (lpc < nq && lpc < kWave) lpc <<= 1;
    }
    const int cps = G / lpc, cph = gl / lpc;
    for (int rc = 0; rc < nq || rc == 0; rc += G) {  // > 64 row quads: leaves over 256 points
        const int rq = rc + (gl & (lpc - 1));
        const bool rowOk = active && rq < nq;
        float tx[4], ty[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = min(4 * rq + j, max(nT - 1, 0));  // padded rows: E is zero there
            tx[j] = rowOk ? (float)(pxT[tb + t] - cx) : 0.0f;
            ty[j] = rowOk ? (float)(pyT[tb + t] - cy) : 0.0f;
        }
        float a[4][K];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < K; ++i) a[j][i] = 0.0f;
        if (rowOk) {
            const flt4* kc = reinterpret_cast<const flt4*>(E + koff) + rq;
            for (int c0 = cph; c0 < S; c0 += U * cps) {
                int ix[U];
#pragma unroll
                for (int u = 0; u < U; ++u) ix[u] = nearPts[pb + min(c0 + u * cps, S - 1)];
                flt4 kk[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int sc = c0 + u * cps;
                    const flt4* p = kc + (size_t)min(sc, S - 1) * nq;
                    kk[u] = sc < S ? __builtin_nontemporal_load(p) : flt4{0.0f, 0.0f, 0.0f, 0.0f};
                }
                float sx[U], sy[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    sx[u] = (float)(pxT[ix[u]] - cx);
                    sy[u] = (float)(pyT[ix[u]] - cy);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double f[K];
                    load_charges<K>(fT + (size_t)ix[u] * KS, f);
                    float xw[K];
#pragma unroll
                    for (int b = 0; b < K; ++b) xw[b] = (float)(hw.hw[b] * f[b]);
                    const float e4[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float dy = sy[u] - ty[j];
                        hm_entry_f32<K, true>(e4[j], sx[u] - tx[j], dy * dy, xw, a[j]);
                    }
                }
            }
        }
        // sum over the column phases
        if constexpr (G == 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    float v = a[j][i];
                    v += dpp_blk_f32<0x124>(v);  // row_ror:4
                    v += dpp_blk_f32<0x128>(v);  // row_ror:8
                    a[j][i] = v;
                }
        } else {
            for (int off = lpc; off < kWave; off <<= 1)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < K; ++i) a[j][i] += __shfl_xor(a[j][i], off);
        }
        if (rowOk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = 4 * rq + j;
                const bool mine = (G == 16) ? (cph == j) : (cph == 0);
                if (!mine || t >= nT) continue;
                const int64_t k = tb + t;
                double f[K];
                load_charges<K>(fT + (size_t)k * KS, f);
                const double sd = sigDiag[k];
                const int64_t oi = out_index(operm, obase, k);
#pragma unroll
                for (int i = 0; i < K; ++i)
                    out[(size_t)i * ldo + oi] = hw.om[i] * scale * __builtin_fma(hw.dw[i] * sd, f[i], (double)a[j][i]);
            }
        }
        if constexpr (G == 16) break;
    }
}

// ----------------------------------------------------------------- launchers

#define ANISO_BLOCK_F32_DISPATCH_K(k, CALL)                                                                 \
    switch (k) {                                                                                            \
        case 2: { constexpr int KK = 2; CALL; } break;                                                      \
        case 4: { constexpr int KK = 4; CALL; } break;                                                      \
        case 5: { constexpr int KK = 5; CALL; } break;                                                      \
        case 8: { constexpr int KK = 8; CALL; } break;                                                      \
        default:                                                                                            \
            throw std::invalid_argument("f32 block operator: unsupported block count " + std::to_string(k)); \
    }

void launch_near_hm_f32(int K, const NearList& nl, const float* E, const NodeBoxes& b, const TreePoints& pts,
                        const double* sigDiag, const HarmWeights& hw, const double* fT, double scale,
                        const OutRows& o, hipStream_t s) {
    if (nl.nl <= 0) return;
    if (nl.maxLeaf <= 16) {
        ANISO_BLOCK_F32_DISPATCH_K(K, (k_near_hm_f32<KK, 16, 2><<<blocks_for((int64_t)nl.nl * 16, 256), 256, 0, s>>>(
                                          nl.nl, nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, E, b.cx, b.cy, pts.px, pts.py,
                                          sigDiag, hw, fT, o.perm, o.base, o.ld, scale, o.out)));
    } else {
        ANISO_BLOCK_F32_DISPATCH_K(K, (k_near_hm_f32<KK, 64, 2><<<blocks_for((int64_t)nl.nl * 64, 256), 256, 0, s>>>(
                                          nl.nl, nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, E, b.cx, b.cy, pts.px, pts.py,
                                          sigDiag, hw, fT, o.perm, o.base, o.ld, scale, o.out)));
    }
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2l_f32(int np, int K, const PairList& pl, const float* E, const NodeBoxes& b, const HoTables* T,
                       const HarmWeights& hw, const double* mult, double* local, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (np == 6) {
        ANISO_BLOCK_F32_DISPATCH_K(K, (k_ho_m2l_f32<6, KK><<<pl.ntgt, 256, 0, s>>>(
                                          pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, hw, mult, local)));
    } else if (np == 8) {
        ANISO_BLOCK_F32_DISPATCH_K(K, (k_ho_m2l_f32<8, KK><<<pl.ntgt, 256, 0, s>>>(
                                          pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, hw, mult, local)));
    } else {
        throw std::invalid_argument("f32 block operator: np must be 6 or 8");
    }
    HIP_LAUNCH_CHECK();
}

#undef ANISO_BLOCK_F32_DISPATCH_K

}  // namespace aniso
