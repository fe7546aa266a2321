// mode_apply.hip -- one mode applied to K vectors on the mode-shared E caches of a
// high-order handle (np = 6, 8):
//     out[k] = sum over sources of (E / r) T_id(c) x[k],   c = cos of the pair's angle.
//
// The block kernels (k_near_hm, k_ho_m2l) form K modes of one entry and mix K inputs
// into them; their offset form serves a single mode of one vector as an 8-row pass that
// runs both windows' recurrences and keeps one row.  Here the entry's factor
// (E / r) T_id(c) -- the geometry, 1/r with two Newton steps and one recurrence up to
// id -- is formed once and applied to the K columns with one FMA each.  There are no
// harmonic weights: the staged multipole is the P2M's own and the stored local is the
// plain sum, so P2M, M2M, L2L and L2P of high_order.hip run unchanged around the M2L.
// k_ho_m2l_mode_wide forms it once for 16 columns in two expansion buffers.
// A lean np = 4 handle runs the same near field and the rank-16 M2L k_m2l_mode16 between
// the up and down tiers of apply.hip.
// Every sum runs in a fixed order and there are no atomics: repeats are bitwise equal.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"
#include "mode_factor.hpp"

namespace aniso {

// ----------------------------------------------------------------- M2L

// k_ho_m2l for one mode and K columns: one workgroup per target node, thread (row t,
// column phase ph) of the NPH = 256 / R phases, G columns in flight; a V pair stored once
// by its smaller id is read transposed through the LDS tile (row stride R + 1); the
// source's multipole and Chebyshev nodes are staged in LDS per pair; the phases' partial
// rows are summed through LDS in phase order.
template <int NP, int K>
__global__ void __launch_bounds__(256) k_ho_m2l_mode(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                     const int* __restrict__ src, const int* __restrict__ blk,
                                                     const double* __restrict__ E, const double* __restrict__ ncx,
                                                     const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                     const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                     int id, const double* __restrict__ mult,
                                                     double* __restrict__ local) {
    constexpr int R = NP * NP, RK = R * K, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 4 : 3;  // NC = 16 / 6
    static_assert(NC % G == 0, "whole column groups");
    constexpr int TILE = R * LD > NPH * RK ? R * LD : NPH * RK;
    __shared__ double X[RK], SX[R], SY[R], TL[TILE];
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double bx = ncx[n] + nrx[n] * T->cheb[t % NP];
    const double by = ncy[n] + nry[n] * T->cheb[t / NP];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const double* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
        for (int i = tid; i < RK; i += 256) X[i] = mult[(size_t)B * RK + i];
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
                    const double dy = SY[s] - by;
                    const double f = mode_factor<false>(ev[i], SX[s] - bx, dy * dy, id);
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = __builtin_fma(f, X[s * K + k], acc[k]);
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
        double v = TL[i];
#pragma unroll
        for (int p = 1; p < NPH; ++p) v += TL[p * RK + i];
        local[(size_t)n * RK + i] = v;
    }
}

// k_ho_m2l_mode for 8 + KB columns in two expansion buffers (the column convention of
// k_ho_m2l_resident: columns 0 .. 7 in multA / localA as [node][R][8], columns 8 .. 8+KB-1
// in multB / localB as [node][R][KB]).  The factor of an entry is
// formed once and applied to all 8 + KB columns.  Thread shape, entry order (s = ph +
// NPH g ascending within a pair, pairs in list order) and the phase-order sum are
// k_ho_m2l_mode's, so a column's bits are what k_ho_m2l_mode<NP, 8> / <NP, KB> gives it.
// The phases' partial rows go through the tile in two rounds, the first half's and then the
// second's: the tile keeps its 8-column size.
template <int NP, int KB>
__global__ void __launch_bounds__(256) k_ho_m2l_mode_wide(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                          const int* __restrict__ src, const int* __restrict__ blk,
                                                          const double* __restrict__ E, const double* __restrict__ ncx,
                                                          const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                          const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                          int id, const double* __restrict__ multA,
                                                          const double* __restrict__ multB, double* __restrict__ localA,
                                                          double* __restrict__ localB) {
    constexpr int KA = 8, R = NP * NP, RA = R * KA, RB = R * KB, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 4 : 3;  // NC = 16 / 6
    static_assert(NC % G == 0, "whole column groups");
    static_assert(KB >= 1 && KB <= KA, "the second half is no wider than the first");
    constexpr int TILE = R * LD > NPH * RA ? R * LD : NPH * RA;
    __shared__ double XA[RA], XB[RB], SX[R], SY[R], TL[TILE];
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double bx = ncx[n] + nrx[n] * T->cheb[t % NP];
    const double by = ncy[n] + nry[n] * T->cheb[t / NP];
    double accA[KA], accB[KB];
#pragma unroll
    for (int k = 0; k < KA; ++k) accA[k] = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) accB[k] = 0.0;
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const double* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
        for (int i = tid; i < RA; i += 256) XA[i] = multA[(size_t)B * RA + i];
        for (int i = tid; i < RB; i += 256) XB[i] = multB[(size_t)B * RB + i];
        if (tid < R) {
            SX[tid] = ncx[B] + nrx[B] * T->cheb[tid % NP];
            SY[tid] = ncy[B] + nry[B] * T->cheb[tid / NP];
        }
        if (tr)
            for (int i = tid; i < R * R; i += 256) TL[(i / R) * LD + (i % R)] = Eb[i];
        __syncthreads();
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
                    const double dy = SY[s] - by;
                    const double f = mode_factor<false>(ev[i], SX[s] - bx, dy * dy, id);
#pragma unroll
                    for (int k = 0; k < KA; ++k) accA[k] = __builtin_fma(f, XA[s * KA + k], accA[k]);
#pragma unroll
                    for (int k = 0; k < KB; ++k) accB[k] = __builtin_fma(f, XB[s * KB + k], accB[k]);
                }
            }
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int k = 0; k < KA; ++k) TL[(ph * R + t) * KA + k] = accA[k];
    }
    __syncthreads();
    for (int i = tid; i < RA; i += 256) {
        double v = TL[i];
#pragma unroll
        for (int p = 1; p < NPH; ++p) v += TL[p * RA + i];
        localA[(size_t)n * RA + i] = v;
    }
    __syncthreads();  // the first half's partials are read
    if (active) {
#pragma unroll
        for (int k = 0; k < KB; ++k) TL[(ph * R + t) * KB + k] = accB[k];
    }
    __syncthreads();
    for (int i = tid; i < RB; i += 256) {
        double v = TL[i];
#pragma unroll
        for (int p = 1; p < NPH; ++p) v += TL[p * RB + i];
        localB[(size_t)n * RB + i] = v;
    }
}

// ----------------------------------------------------------------- M2L, rank 16

// PG blocks of one wave's pair list, as lane (s, q) holds them: rows 4q .. 4q+3 of column s
// of each E block, the K columns of entry s of each source's multipole, the source nodes
template <int K, int PG>
struct M16Group {
    double e4[PG][4];
    double xm[PG][K];
    int B[PG];
};

// issue the loads of blocks j0 .. j0 + PG - 1 of the wave's cnt pairs (mySrc / myBlk: lane
// j holds pair j).  A block past cnt is a valid clamp with E = 0: its factor is 0.
template <int K, int PG>
__device__ __forceinline__ void m16_load(M16Group<K, PG>& g, int j0, int cnt, int mySrc, int myBlk, int s, int q,
                                         const double* __restrict__ E, const double* __restrict__ mult) {
#pragma unroll
    for (int i = 0; i < PG; ++i) {
        const int b = __builtin_amdgcn_readlane(myBlk, min(j0 + i, cnt - 1));
        const bool tr = b < 0;
        const double* p = E + (size_t)(tr ? ~b : b) * 256 + (tr ? 64 * q + s : 16 * s + 4 * q);
        const int st = tr ? 16 : 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) g.e4[i][j] = j0 + i < cnt ? p[j * st] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < PG; ++i) {
        g.B[i] = __builtin_amdgcn_readlane(mySrc, min(j0 + i, cnt - 1));
        const double* m = mult + ((size_t)g.B[i] * kRank + s) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) g.xm[i][k] = m[k];
    }
}

// k_m2l_hm for one mode and K columns (np = 4): one wave per target node, four targets per
// workgroup; every directed pair's 2 KB E block read once as 64 lanes x 32 B (column-major:
// lane (s, q) holds column s, rows 4q .. 4q+3), a pair listed as ~blk read transposed
// (stride 16).  Two groups of PG blocks rotate: the next group's loads are issued before
// the current group's arithmetic (the rank-16 M2L is bound by load latency, DESIGN.md
// §3.10), so 2 PG blocks are in flight per wave.  Per entry the factor (E / r) T_id(c) and
// one FMA per column; the 16 columns are summed with k_m2l_hm's __shfl_xor tree.  The
// stored local is the plain sum (no harmonic weights): the rank-16 up and down tiers run
// unchanged around it.  Every target of the list is stored, one with no pair as zero.
template <int K, int PG, int WPE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) k_m2l_mode16(int ntgt, const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                    const int* __restrict__ src, const int* __restrict__ blk,
                                                    const double* __restrict__ E, const double* __restrict__ ncx,
                                                    const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                    const double* __restrict__ nry, const Params* __restrict__ P, int id,
                                                    const double* __restrict__ mult, double* __restrict__ local) {
    const int wave =
        __builtin_amdgcn_readfirstlane((int)blockIdx.x * (int)(blockDim.x / kWave) + (int)(threadIdx.x / kWave));
    const int lane = threadIdx.x & (kWave - 1);
    if (wave >= ntgt) return;
    const int n = tgt[wave];
    const int s = lane >> 2, q = lane & 3;
    double bx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bx[j] = ncx[n] + nrx[n] * P->cheb[j];
    const double by = ncy[n] + nry[n] * P->cheb[q];
    const double chx = P->cheb[s & 3], chy = P->cheb[s >> 2];
    double c[4][K];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) c[j][k] = 0.0;
    // a group's arithmetic: dx = source minus target, so an odd mode keeps its sign
    auto apply = [&](const M16Group<K, PG>& g) {
#pragma unroll
        for (int i = 0; i < PG; ++i) {
            const double ax = ncx[g.B[i]] + nrx[g.B[i]] * chx;
            const double dy = (ncy[g.B[i]] + nry[g.B[i]] * chy) - by;
            const double dy2 = dy * dy;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double f = mode_factor<false>(g.e4[i][j], ax - bx[j], dy2, id);
#pragma unroll
                for (int k = 0; k < K; ++k) c[j][k] = __builtin_fma(f, g.xm[i][k], c[j][k]);
            }
        }
    };
    const int64_t p0 = ptr[wave], p1 = ptr[wave + 1];
    for (int64_t cb = p0; cb < p1; cb += kWave) {
        const int cnt = (int)min<int64_t>(kWave, p1 - cb);
        const int mySrc = lane < cnt ? src[cb + lane] : 0;
        const int myBlk = lane < cnt ? blk[cb + lane] : 0;
        M16Group<K, PG> ga, gb;
        m16_load<K, PG>(ga, 0, cnt, mySrc, myBlk, s, q, E, mult);
        for (int j0 = 0; j0 < cnt; j0 += 2 * PG) {
            const bool more = j0 + PG < cnt;  // (wave-uniform)
            if (more) m16_load<K, PG>(gb, j0 + PG, cnt, mySrc, myBlk, s, q, E, mult);
            apply(ga);
            if (j0 + 2 * PG < cnt) m16_load<K, PG>(ga, j0 + 2 * PG, cnt, mySrc, myBlk, s, q, E, mult);
            if (more) apply(gb);
        }
    }
    // sum over the 16 columns (lane bits 2..5); row t = 4q' + j is entry j of the lanes
    // with q == q' (lane 4t + (t >> 2) holds row t = s), as k_m2l_hm
#pragma unroll
    for (int off = 4; off < kWave; off <<= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) c[j][k] += __shfl_xor(c[j][k], off);
    const int jr = s & 3, srcLane = 4 * s + (s >> 2);
    double* dst = local + ((size_t)n * kRank + s) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double sel = jr == 0 ? c[0][k] : jr == 1 ? c[1][k] : jr == 2 ? c[2][k] : c[3][k];
        const double v = __shfl(sel, srcLane);
        if ((k & 3) == q) dst[k] = v;
    }
}

// ----------------------------------------------------------------- near field

// k_near_hm for one mode and K columns: directed E blocks (column-major nT4 x S per
// target leaf, rows padded to a multiple of 4), G lanes per target leaf (G = 16: leaves
// <= 16 points, 4 leaves per wave; else 64), lane (row quad rq, column phase) computes
// rows 4rq .. 4rq+3 for its columns, U = 2 columns in flight; the row loop serves leaves over
// 256 points.  out (stored, not added) = scale * (sum over sources + the sigma_t
// diagonal, present for id = 0 only).
template <int K, int G>
__global__ void __launch_bounds__(256) k_near_mode(int nl, const int4* __restrict__ leafInfo,
                                                   const int64_t* __restrict__ nearPtsPtr,
                                                   const int* __restrict__ nearPts, const int64_t* __restrict__ nearKOff,
                                                   const double* __restrict__ E, const double* __restrict__ pxT,
                                                   const double* __restrict__ pyT, const double* __restrict__ sigDiag,
                                                   int id, const double* __restrict__ fT,
                                                   const int* __restrict__ operm, int64_t obase, int64_t ldo,
                                                   double scale, double* __restrict__ out) {
    static_assert(G == 16 || G == 64, "leaf group of 16 or 64 lanes");
    // (2 columns in flight, as k_near_hm's offset form: 112 .. 198 VGPRs for K = 2 .. 8; with 4
    // the 16 entries' 1/r chains take K = 8 to 256 VGPRs, one wave per SIMD)
    constexpr int KS = kStride<K>, U = 2;
    const int gl = threadIdx.x & (G - 1);
    const int li = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G);
    const bool active = li < nl;
    int4 info = make_int4(0, 0, 0, 0);
    int64_t pb = 0, koff = 0;
    if (active) {
        info = leafInfo[li];
        pb = nearPtsPtr[li];
        koff = nearKOff[li];
    }
    const int nT = info.z, S = info.w;
    const int64_t tb = info.y;
    const int nq = (nT + 3) >> 2;  // row quads
    const int cstr = 2 * nq;       // column stride in 16-B units
    int lpc = 4;                   // lanes per column (G = 16: leaves <= 16 points, 4 quads)
    if constexpr (G == 64) {
        lpc = 1;
        while (lpc < nq && lpc < kWave) lpc <<= 1;
    }
    const int cps = G / lpc, cph = gl / lpc;
    for (int rc = 0; rc < nq || rc == 0; rc += G) {  // > 64 row quads: leaves over 256 points
        const int rq = rc + (gl & (lpc - 1));
        const bool rowOk = active && rq < nq;
        double tx[4], ty[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = min(4 * rq + j, max(nT - 1, 0));  // padded rows: E is zero there
            tx[j] = rowOk ? pxT[tb + t] : 0.0;
            ty[j] = rowOk ? pyT[tb + t] : 0.0;
        }
        double a[4][K];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) a[j][k] = 0.0;
        if (rowOk) {
            const dbl2* kc = reinterpret_cast<const dbl2*>(E + koff) + 2 * rq;
            for (int c0 = cph; c0 < S; c0 += U * cps) {
                int ix[U];
#pragma unroll
                for (int u = 0; u < U; ++u) ix[u] = nearPts[pb + min(c0 + u * cps, S - 1)];
                dbl2 kk[U][2];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int sc = c0 + u * cps;
                    const dbl2* p = kc + (size_t)min(sc, S - 1) * cstr;
                    const bool ok = sc < S;
                    kk[u][0] = ok ? __builtin_nontemporal_load(p) : dbl2{0.0, 0.0};
                    kk[u][1] = ok ? __builtin_nontemporal_load(p + 1) : dbl2{0.0, 0.0};
                }
                double sx[U], sy[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    sx[u] = pxT[ix[u]];
                    sy[u] = pyT[ix[u]];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double x[K];
                    load_charges<K>(fT + (size_t)ix[u] * KS, x);
                    const double e4[4] = {kk[u][0].x, kk[u][0].y, kk[u][1].x, kk[u][1].y};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double dy = sy[u] - ty[j];
                        const double f = mode_factor<true>(e4[j], sx[u] - tx[j], dy * dy, id);
#pragma unroll
                        for (int k = 0; k < K; ++k) a[j][k] = __builtin_fma(f, x[k], a[j][k]);
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
                    double v = a[j][k];
                    v += dpp_f64<0x124>(v);  // row_ror:4
                    v += dpp_f64<0x128>(v);  // row_ror:8
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
                for (int k = 0; k < K; ++k) out[(size_t)k * ldo + oi] = scale * __builtin_fma(sd, x[k], a[j][k]);
            }
        }
        if constexpr (G == 16) break;
    }
}

// ----------------------------------------------------------------- launchers

#define ANISO_MODE_DISPATCH_K(k, CALL)                                                                \
    switch (k) {                                                                                      \
        case 2: { constexpr int KK = 2; CALL; } break;                                                \
        case 4: { constexpr int KK = 4; CALL; } break;                                                \
        case 5: { constexpr int KK = 5; CALL; } break;                                                \
        case 8: { constexpr int KK = 8; CALL; } break;                                                \
        default:                                                                                      \
            throw std::invalid_argument("mode apply: unsupported column count " + std::to_string(k)); \
    }

void launch_near_mode(int K, int id, const NearList& nl, const double* E, const TreePoints& pts,
                      const double* sigDiag, const double* fT, double scale, const OutRows& o, hipStream_t s) {
    if (nl.nl <= 0) return;
    if (id < 0) throw std::invalid_argument("mode apply: negative mode");
    if (nl.maxLeaf <= 16) {
        ANISO_MODE_DISPATCH_K(K, (k_near_mode<KK, 16><<<blocks_for((int64_t)nl.nl * 16, 256), 256, 0, s>>>(
                                     nl.nl, nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, E, pts.px, pts.py, sigDiag, id, fT,
                                     o.perm, o.base, o.ld, scale, o.out)));
    } else {
        ANISO_MODE_DISPATCH_K(K, (k_near_mode<KK, 64><<<blocks_for((int64_t)nl.nl * 64, 256), 256, 0, s>>>(
                                     nl.nl, nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, E, pts.px, pts.py, sigDiag, id, fT,
                                     o.perm, o.base, o.ld, scale, o.out)));
    }
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2l_mode(int np, int K, int id, const PairList& pl, const double* E, const NodeBoxes& b,
                        const HoTables* T, const double* mult, double* local, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (id < 0) throw std::invalid_argument("mode apply: negative mode");
    if (np == 6) {
        ANISO_MODE_DISPATCH_K(K, (k_ho_m2l_mode<6, KK><<<pl.ntgt, 256, 0, s>>>(
                                     pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, id, mult, local)));
    } else if (np == 8) {
        ANISO_MODE_DISPATCH_K(K, (k_ho_m2l_mode<8, KK><<<pl.ntgt, 256, 0, s>>>(
                                     pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, id, mult, local)));
    } else {
        throw std::invalid_argument("mode apply: np must be 6 or 8");
    }
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2l_mode_wide(int np, int KB, int id, const PairList& pl, const double* E, const NodeBoxes& b,
                             const HoTables* T, const double* multA, const double* multB, double* localA,
                             double* localB, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (id < 0) throw std::invalid_argument("mode apply: negative mode");
    if (!multA || !multB || !localA || !localB) throw std::invalid_argument("wide mode apply: a NULL expansion buffer");
    if (np == 6) {
        ANISO_MODE_DISPATCH_K(KB, (k_ho_m2l_mode_wide<6, KK><<<pl.ntgt, 256, 0, s>>>(
                                      pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, id, multA, multB,
                                      localA, localB)));
    } else if (np == 8) {
        ANISO_MODE_DISPATCH_K(KB, (k_ho_m2l_mode_wide<8, KK><<<pl.ntgt, 256, 0, s>>>(
                                      pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, T, id, multA, multB,
                                      localA, localB)));
    } else {
        throw std::invalid_argument("mode apply: np must be 6 or 8");
    }
    HIP_LAUNCH_CHECK();
}

void launch_m2l_mode16(int K, int id, const PairList& pl, const double* E, const NodeBoxes& b, const Params* P,
                       const double* mult, double* local, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (id < 0) throw std::invalid_argument("mode apply: negative mode");
    const unsigned nb = blocks_for((int64_t)pl.ntgt * kWave, 256);
    // one block per group, two groups: 2 blocks in flight per wave at 4 (K = 2), 3 (K = 4, 5) and
    // 2 (K = 8) waves per SIMD, the most each instance holds without scratch
    ANISO_MODE_DISPATCH_K(K, (k_m2l_mode16<KK, 1, (KK <= 2 ? 4 : KK <= 5 ? 3 : 2)><<<nb, 256, 0, s>>>(
                                 pl.ntgt, pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy, b.rx, b.ry, P, id, mult,
                                 local)));
    HIP_LAUNCH_CHECK();
}

#undef ANISO_MODE_DISPATCH_K

}  // namespace aniso
