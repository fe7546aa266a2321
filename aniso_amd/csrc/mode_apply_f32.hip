// mode_apply_f32.hip -- the reduced-precision operator of a high-order handle (np = 6, 8;
// DESIGN.md §3.18.5): k_ho_m2l_mode and k_near_mode of mode_apply.hip with the entry's
// factor (E / r) T_id(c), the products and the accumulators in fp32, on float mirrors of
// the two E arrays (k_cache_f32, same indexing).  Everything around them stays the fp64
// code: the multipole is read as double and rounded when it is staged, the local
// expansion and the near field's `out` are stored as double.
//
// No absolute coordinate is subtracted in fp32: at 1M points a leaf is 1e-3 wide and
// float(0.5) - float(0.5 + 1e-3) keeps four digits.  The geometry is formed relative to
// the pair in fp64 and then rounded: the M2L stages the source's nodes relative to the
// target's centre, the near field takes every point relative to the target leaf's centre.
// Every sum runs in a fixed order and there are no atomics: repeats are bitwise equal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "device_common.hpp"

namespace aniso {

typedef float flt4 __attribute__((ext_vector_type(4)));

// v_rsq_f32 (1 ulp) and one Newton step (without it the M2L launch is 1 % shorter at 1M
// points, DESIGN.md §3.18.5: not worth the digit)
__device__ __forceinline__ float rsqrt_f32(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    return y * __builtin_fmaf(-0.5f * x * y, y, 1.5f);
}

// mode_factor in fp32.  guard0: r = 0 is the point itself, where E = 0; the floor keeps
// 1 / r finite in fp32's range (1e-30 is a separation of 1e-15, below any two points)
template <bool guard0>
__device__ __forceinline__ float mode_factor_f32(float e, float dx, float dy2, int id) {
    float r2 = __builtin_fmaf(dx, dx, dy2);
    if constexpr (guard0) r2 = __builtin_fmaxf(r2, 1e-30f);
    const float ri = rsqrt_f32(r2);
    const float c = dx * ri, c2 = c + c;
    float t0 = 1.0f, t1 = c;
#pragma nounroll
    for (int n = 1; n < id; ++n) {
        const float t = __builtin_fmaf(c2, t1, -t0);
        t0 = t1;
        t1 = t;
    }
    return (e * ri) * (id == 0 ? 1.0f : t1);
}

// ----------------------------------------------------------------- the mirrors

// both E arrays rounded to float in one launch: a (na entries) then b (nb entries)
__global__ void __launch_bounds__(256) k_cache_f32(int64_t na, const double* __restrict__ a, float* __restrict__ af,
                                                   int64_t nb, const double* __restrict__ b, float* __restrict__ bf) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += stride) {
        if (i < na) af[i] = (float)a[i];
        else bf[i - na] = (float)b[i - na];
    }
}

void launch_cache_f32(int64_t na, const double* a, float* af, int64_t nb, const double* b, float* bf, hipStream_t s) {
    if (na + nb <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(na + nb, 256), 1 << 16);
    k_cache_f32<<<grid, 256, 0, s>>>(na, a, af, nb, b, bf);
    HIP_LAUNCH_CHECK();
}

// ----------------------------------------------------------------- M2L

// k_ho_m2l_mode in fp32: the same workgroup per target node, thread (row t, column phase
// ph) and phase sum.  The source's nodes are staged relative to the target's centre,
// (ncx[B] - ncx[n]) + nrx[B] cheb in fp64 and then rounded; the thread's own offset is
// nrx[n] cheb.  G = 4 / 3 columns in flight and one pair per barrier round, as the fp64
// kernel: the launch is bound by the latency of the E loads, which more resident waves hide
// and more loads per thread do not.  Measured at 1M points, K = 8:
// np = 8, G = 4 / 8 / 16 (80 / 94 / 168 VGPRs): 2.76 / 2.96 / 3.82 ms; np = 6, G = 3 / 6: 4.76
// / 5.39 ms; 4 and 8 pairs staged per round (27 and 54 KB of LDS): 7.5 and 13.3 ms.
template <int NP, int K>
__global__ void __launch_bounds__(256) k_ho_m2l_mode_f32(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                         const int* __restrict__ src, const int* __restrict__ blk,
                                                         const float* __restrict__ E, const double* __restrict__ ncx,
                                                         const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                         const double* __restrict__ nry,
                                                         const HoTables* __restrict__ T, int id,
                                                         const double* __restrict__ mult, double* __restrict__ local) {
    constexpr int R = NP * NP, RK = R * K, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 4 : 3;  // NC = 16 / 6
    static_assert(NC % G == 0, "whole column groups");
    constexpr int TILE = R * LD > NPH * RK ? R * LD : NPH * RK;
    __shared__ float X[RK], SX[R], SY[R], TL[TILE];
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double cx = ncx[n], cy = ncy[n];
    const float bx = (float)(nrx[n] * T->cheb[t % NP]);
    const float by = (float)(nry[n] * T->cheb[t / NP]);
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0f;
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const float* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
        for (int i = tid; i < RK; i += 256) X[i] = (float)mult[(size_t)B * RK + i];
        if (tid < R) {
            SX[tid] = (float)((ncx[B] - cx) + nrx[B] * T->cheb[tid % NP]);
            SY[tid] = (float)((ncy[B] - cy) + nry[B] * T->cheb[tid / NP]);
        }
        if (tr)
            for (int i = tid; i < R * R; i += 256) TL[(i / R) * LD + (i % R)] = Eb[i];
        __syncthreads();
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
                    const float dy = SY[s] - by;
                    const float f = mode_factor_f32<false>(ev[i], SX[s] - bx, dy * dy, id);
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = __builtin_fmaf(f, X[s * K + k], acc[k]);
                }
            }
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int k = 0; k < K; ++k) TL[(ph * R + t) * K + k] = acc[k];
    }
    __syncthreads();
    for (int i = tid; i < RK; i += 256) {
        float v = TL[i];
#pragma unroll
        for (int p = 1; p < NPH; ++p) v += TL[p * RK + i];
        local[(size_t)n * RK + i] = (double)v;
    }
}

// ----------------------------------------------------------------- near field

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// k_near_mode in fp32: the same lanes per leaf, row quads and column phases; a row quad
// of one column is one 16-B load, U = 2 columns in flight (4 take K = 8 from 132 to 190
// VGPRs, two waves per SIMD).  Every point is taken
// relative to the target leaf's centre (ncx, ncy of the leaf's node) in fp64 and then
// rounded.  The charges are read as double; out is stored as double, the sigma_t diagonal
// and the scale applied in fp64.
template <int K, int G>
__global__ void __launch_bounds__(256) k_near_mode_f32(int nl, const int4* __restrict__ leafInfo,
                                                       const int64_t* __restrict__ nearPtsPtr,
                                                       const int* __restrict__ nearPts,
                                                       const int64_t* __restrict__ nearKOff, const float* __restrict__ E,
                                                       const double* __restrict__ ncx, const double* __restrict__ ncy,
                                                       const double* __restrict__ pxT, const double* __restrict__ pyT,
                                                       const double* __restrict__ sigDiag, int id,
                                                       const double* __restrict__ fT, const int* __restrict__ operm,
                                                       int64_t obase, int64_t ldo, double scale,
                                                       double* __restrict__ out) {
    static_assert(G == 16 || G == 64, "leaf group of 16 or 64 lanes");
    constexpr int KS = kStride<K>, U = 2;
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
            for (int k = 0; k < K; ++k) a[j][k] = 0.0f;
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
                    double xd[K];
                    load_charges<K>(fT + (size_t)ix[u] * KS, xd);
                    float x[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) x[k] = (float)xd[k];
                    const float e4[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float dy = sy[u] - ty[j];
                        const float f = mode_factor_f32<true>(e4[j], sx[u] - tx[j], dy * dy, id);
#pragma unroll
                        for (int k = 0; k < K; ++k) a[j][k] = __builtin_fmaf(f, x[k], a[j][k]);
                    }
                }
            }
        }
        // sum over the column phases
        if constexpr (G == 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float v = a[j][k];
                    v += dpp_f32<0x124>(v);  // row_ror:4
                    v += dpp_f32<0x128>(v);  // row_ror:8
                    a[j][k] = v;
                }
        } else {
            for (int off = lpc; off < kWave; off <<= 1)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int k = 0; k < K; ++k) a[j][k] += __shfl_xor(a[j][k], off);
        }
        if (rowOk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = 4 * rq + j;
                const bool mine = (G == 16) ? (cph == j) : (cph == 0);
                if (!mine || t >= nT) continue;
                const int64_t kp = tb + t;
                double x[K];
                load_charges<K>(fT + (size_t)kp * KS, x);
                const double sd = id == 0 ? sigDiag[kp] : 0.0;
                const int64_t oi = out_index(operm, obase, kp);
#pragma unroll
                for (int k = 0; k < K; ++k)
                    out[(size_t)k * ldo + oi] = scale * __builtin_fma(sd, x[k], (double)a[j][k]);
            }
        }
        if constexpr (G == 16) break;
    }
}

// ----------------------------------------------------------------- launchers

#define ANISO_MODE_DISPATCH_K(k, CALL)                                                                    \
    switch (k) {                                                                                          \
        case 2: { constexpr int KK = 2; CALL; } break;                                                    \
        case 4: { constexpr int KK = 4; CALL; } break;                                                    \
        case 5: { constexpr int KK = 5; CALL; } break;                                                    \
        case 8: { constexpr int KK = 8; CALL; } break;                                                    \
        default:                                                                                          \
            throw std::invalid_argument("f32 mode apply: unsupported column count " + std::to_string(k)); \
    }

void launch_near_mode_f32(int K, int id, const NearList& nl, const float* E, const NodeBoxes& b,
                          const TreePoints& pts, const double* sigDiag, const double* fT, double scale,
                          const OutRows& o, hipStream_t s) {
    if (nl.nl <= 0) return;
    if (id < 0) throw std::invalid_argument("f32 mode apply: negative mode");
    if (nl.maxLeaf <= 16) {
        ANISO_MODE_DISPATCH_K(K, (k_near_mode_f32<KK, 16><<<blocks_for((int64_t)nl.nl * 16, 256), 256, 0, s>>>(
                                     nl.nl, nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, E, b.cx, b.cy, pts.px, pts.py, sigDiag,
                                     id, fT, o.perm, o.base, o.ld, scale, o.out)));
    } else {
        ANISO_MODE_DISPATCH_K(K, (k_near_mode_f32<KK, 64><<<blocks_for((int64_t)nl.nl * 64, 256), 256, 0, s>>>(
                                     nl.nl, nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, E, b.cx, b.cy, pts.px, pts.py, sigDiag,
                                     id, fT, o.perm, o.base, o.ld, scale, o.out)));
    }
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2l_mode_f32(int np, int K, int id, const PairList& pl, const float* E, const NodeBoxes& b,
                            const HoTables* T, const double* mult, double* local, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (id < 0) throw std::invalid_argument("f32 mode apply: negative mode");
    if (np == 6) {
        ANISO_MODE_DISPATCH_K(K, (k_ho_m2l_mode_f32<6, KK><<<pl.ntgt, 256, 0, s>>>(
                                     pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, id, mult, local)));
    } else if (np == 8) {
        ANISO_MODE_DISPATCH_K(K, (k_ho_m2l_mode_f32<8, KK><<<pl.ntgt, 256, 0, s>>>(
                                     pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, id, mult, local)));
    } else {
        throw std::invalid_argument("f32 mode apply: np must be 6 or 8");
    }
    HIP_LAUNCH_CHECK();
}

#undef ANISO_MODE_DISPATCH_K

}  // namespace aniso
