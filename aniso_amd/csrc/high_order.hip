// high_order.hip -- the far field of a high-order handle (np = 6, 8):
// the mode-shared block apply of harmonic.hip at Chebyshev rank R = np^2 = 36 / 64.
//
// Reference behaviour (file:line under lowrank/aniso): bbfmm.h:476-505 takes np from the
// config; P2M bbfmm.h:737-748, M2M 855-859, M2L 1051-1065, L2L 1070-1071, L2P 1104.
//
// The near field and the corrections do not depend on the order and stay the kernels of
// harmonic.hip / apply.hip; the lists (targets, pairs, leaves, levels) are the host's,
// independent of the rank.  Layouts: expansions [node][R][K] with entry r = ix + np iy
// (x fastest, as at rank 16); E blocks R x R column-major (pair R^2 + s R + t: source
// column s, target row t), so one column is 288 / 512 contiguous bytes.  The transfer
// S_x (x) S_y is applied as two 1-D transforms with the np x np matrices HoTables::S.
// Every sum runs in a fixed order and there are no atomics: the applies are bitwise
// repeatable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"
#include "line_integral.hpp"

namespace aniso {

void ho_tables(int np, HoTables* t) {
    if (np < 2 || np > kMaxNP) throw std::invalid_argument("high-order tables: np out of range");
    *t = HoTables{};
    for (int i = 0; i < np; ++i) t->cheb[i] = -std::cos((i + 0.5) * M_PI / np);
    auto poly = [&](double s, double* T) {
        T[0] = 1.0;
        T[1] = s;
        for (int l = 2; l < np; ++l) T[l] = 2.0 * s * T[l - 1] - T[l - 2];
    };
    double T[kMaxNP];
    for (int i = 0; i < np; ++i) {
        poly(t->cheb[i], T);
        for (int l = 0; l < np; ++l) t->tnode[i + l * np] = T[l];
    }
    // S[b][c np + p]: the weight of parent node p at child node c of half b
    // (bbfmm.h:597-693, as Params::R at rank 16: R = S[b1] (x) S[b0])
    for (int b = 0; b < 2; ++b)
        for (int c = 0; c < np; ++c) {
            poly((b ? 0.5 : -0.5) + 0.5 * t->cheb[c], T);
            for (int p = 0; p < np; ++p) {
                double acc = 0.0;
                for (int l = 0; l < np; ++l) acc += T[l] * t->tnode[p + l * np];
                t->S[b][c * np + p] = (2.0 * acc - 1.0) * (1.0 / np);
            }
        }
}

// Chebyshev interpolant S(s, c_i) of order NP (cheb_weights' arithmetic)
template <int NP>
__device__ __forceinline__ void ho_cheb_weights(const HoTables* __restrict__ T, double s, double (&S)[NP]) {
    double Tl[NP];
    Tl[0] = 1.0;
    Tl[1] = s;
#pragma unroll
    for (int l = 2; l < NP; ++l) Tl[l] = 2.0 * s * Tl[l - 1] - Tl[l - 2];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < NP; ++l) acc += Tl[l] * T->tnode[i + l * NP];
        S[i] = (2.0 * acc - 1.0) * (1.0 / NP);
    }
}

// ----------------------------------------------------------------- E cache

// E[t][s] = e^-tau between Chebyshev node s of the pair's source box and node t of its
// target box (k_cache_att_m2l at rank R), column-major: consecutive threads write
// consecutive rows of one column.
template <int NP>
__global__ void __launch_bounds__(256) k_ho_cache_att(int64_t total, const int* __restrict__ pairTgt,
                                                      const int* __restrict__ src, const double* __restrict__ ncx,
                                                      const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                      const double* __restrict__ nry, const double* __restrict__ stcoef,
                                                      const Params* __restrict__ P, const HoTables* __restrict__ T,
                                                      double* __restrict__ E) {
    constexpr int R = NP * NP;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t p = e / (R * R);
    const int rem = (int)(e - p * (R * R));
    const int s = rem / R, t = rem - s * R;
    const int tn = pairTgt[p], sn = src[p];
    const double bx = ncx[tn] + nrx[tn] * T->cheb[t % NP];
    const double by = ncy[tn] + nry[tn] * T->cheb[t / NP];
    const double ax = ncx[sn] + nrx[sn] * T->cheb[s % NP];
    const double ay = ncy[sn] + nry[sn] * T->cheb[s / NP];
    E[e] = pair_kernel(P, stcoef, kAttMode, ax, ay, bx, by);
}

// ----------------------------------------------------------------- up pass

// P2M (bbfmm.h:737-748): one wave per leaf.  64 points at a time: lane p forms its
// point's weights S_x, S_y and loads its weighted charges (fT, launch_prepare) into
// LDS; lane r = ix + NP iy then sums its entry over the points in order.
template <int NP, int K>
__global__ void __launch_bounds__(64) k_ho_p2m(const int4* __restrict__ leafInfo, const double* __restrict__ ncx,
                                               const double* __restrict__ ncy, const double* __restrict__ nrx,
                                               const double* __restrict__ nry, const double* __restrict__ pxT,
                                               const double* __restrict__ pyT, const double* __restrict__ fT,
                                               const HoTables* __restrict__ T, double* __restrict__ mult) {
    constexpr int R = NP * NP, KS = kStride<K>;
    static_assert(R <= 64, "one lane per expansion entry");
    __shared__ double W[64][2 * NP + 1];
    __shared__ double F[64][K];
    const int4 info = leafInfo[blockIdx.x];
    const int n = info.x, nT = info.z;
    const int64_t tb = info.y;
    const double cx = ncx[n], cy = ncy[n], irx = 1.0 / nrx[n], iry = 1.0 / nry[n];
    const int r = threadIdx.x, ix = r % NP, iy = (r / NP) % NP;
    double acc[K];
#pragma unroll
    for (int b = 0; b < K; ++b) acc[b] = 0.0;
    for (int c0 = 0; c0 < nT; c0 += 64) {
        const int p = c0 + (int)threadIdx.x;
        __syncthreads();
        if (p < nT) {
            const int64_t kp = tb + p;
            double Sx[NP], Sy[NP], f[K];
            ho_cheb_weights<NP>(T, (pxT[kp] - cx) * irx, Sx);
            ho_cheb_weights<NP>(T, (pyT[kp] - cy) * iry, Sy);
            load_charges<K>(fT + (size_t)kp * KS, f);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                W[threadIdx.x][i] = Sx[i];
                W[threadIdx.x][NP + i] = Sy[i];
            }
#pragma unroll
            for (int b = 0; b < K; ++b) F[threadIdx.x][b] = f[b];
        }
        __syncthreads();
        const int cnt = min(64, nT - c0);
        if (r < R)
            for (int q = 0; q < cnt; ++q) {
                const double w = W[q][ix] * W[q][NP + iy];
#pragma unroll
                for (int b = 0; b < K; ++b) acc[b] = __builtin_fma(w, F[q][b], acc[b]);
            }
    }
    if (r < R) {
#pragma unroll
        for (int b = 0; b < K; ++b) mult[((size_t)n * R + r) * K + b] = acc[b];
    }
}

// M2M (bbfmm.h:855-859) of one level: one workgroup per parent.  The four children's
// multipoles (zero for an empty child: child < 0) go to LDS, are transformed along x
// with S[q & 1], then along y with S[q >> 1] and summed over the children in order.
template <int NP, int K>
__global__ void __launch_bounds__(256) k_ho_m2m(const int* __restrict__ nodes, const int4* __restrict__ child,
                                                const HoTables* __restrict__ T, double* __restrict__ mult) {
    constexpr int R = NP * NP, RK = R * K;
    __shared__ double C[4 * RK], X[4 * RK], S[2 * R];
    const int n = nodes[blockIdx.x];
    const int4 c4 = child[n];
    const int ch[4] = {c4.x, c4.y, c4.z, c4.w};
    for (int i = threadIdx.x; i < 2 * R; i += blockDim.x) S[i] = T->S[i / R][i % R];
    for (int it = threadIdx.x; it < 4 * RK; it += blockDim.x) {
        const int q = it / RK, e = it - q * RK;
        C[it] = ch[q] >= 0 ? mult[(size_t)ch[q] * RK + e] : 0.0;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < 4 * RK; it += blockDim.x) {
        const int q = it / RK, e = it - q * RK, rr = e / K, b = e - rr * K, cy = rr / NP, px = rr - cy * NP;
        const double* Sq = S + (q & 1) * R + px;
        const double* Cq = C + q * RK + (cy * NP) * K + b;
        double acc = 0.0;
#pragma unroll
        for (int cxi = 0; cxi < NP; ++cxi) acc = __builtin_fma(Sq[cxi * NP], Cq[cxi * K], acc);
        X[it] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < RK; e += blockDim.x) {
        const int rr = e / K, b = e - rr * K, py = rr / NP, px = rr - py * NP;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double* Sq = S + (q >> 1) * R + py;
            const double* Xq = X + q * RK + px * K + b;
#pragma unroll
            for (int cyi = 0; cyi < NP; ++cyi) acc = __builtin_fma(Sq[cyi * NP], Xq[cyi * NP * K], acc);
        }
        mult[(size_t)n * RK + e] = acc;
    }
}

// ----------------------------------------------------------------- M2L

// The kernels' harmonic weights with the pass window (i0 = b0 = 0: the whole operator
// of at most kMaxRhs blocks)
struct HoHarm : HarmWeights {
    int i0, b0;
};

// Harmonic M2L over V then X (k_m2l_hm at rank R): one workgroup per target node, every
// pair's E block read ONCE for all modes.  Thread (row t, column phase ph) of the NPH =
// 256 / R phases owns target row t and walks the columns s = ph, ph + NPH, ...: a wave's
// loads of a stored block are whole contiguous columns.  A V pair stored once by its
// smaller id is read transposed (blk < 0: E(t, s) = E_stored(s, t)): the workgroup copies
// the block into an LDS tile with coalesced loads and the threads read their rows from
// the tile (row stride R + 1: no bank conflict), instead of R-strided global loads.
// Per pair the source's weighted multipole hw_b x_b(s) and its Chebyshev nodes are
// staged in LDS.  The phases' partial rows are summed through LDS in phase order.
template <int NP, int K>
__global__ void __launch_bounds__(256) k_ho_m2l(const int* __restrict__ tgt, const int64_t* __restrict__ ptr,
                                                const int* __restrict__ src, const int* __restrict__ blk,
                                                const double* __restrict__ E, const double* __restrict__ ncx,
                                                const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                const double* __restrict__ nry, const HoTables* __restrict__ T,
                                                HoHarm hw, const double* __restrict__ mult,
                                                double* __restrict__ local) {
    constexpr int R = NP * NP, RK = R * K, NPH = 256 / R, NC = (R + NPH - 1) / NPH, LD = R + 1;
    constexpr int G = NP == 8 ? 4 : 3;  // NC = 16 / 6
    static_assert(NC % G == 0, "whole column groups");
    constexpr int TILE = R * LD > NPH * RK ? R * LD : NPH * RK;
    __shared__ double XW[RK], SX[R], SY[R], TL[TILE];
    const int tid = threadIdx.x, t = tid % R, ph = tid / R;
    const bool active = ph < NPH;
    const int n = tgt[blockIdx.x];
    const double bx = ncx[n] + nrx[n] * T->cheb[t % NP];
    const double by = ncy[n] + nry[n] * T->cheb[t / NP];
    double c[1][K];
#pragma unroll
    for (int i = 0; i < K; ++i) c[0][i] = 0.0;
    const int64_t p0 = ptr[blockIdx.x], p1 = ptr[blockIdx.x + 1];
    for (int64_t e = p0; e < p1; ++e) {
        const int B = src[e], b = blk[e];
        const bool tr = b < 0;
        const double* Eb = E + (size_t)(tr ? ~b : b) * (R * R);
        __syncthreads();  // the previous pair's LDS reads are done
        for (int i = tid; i < RK; i += 256) XW[i] = hw.hw[i % K] * mult[(size_t)B * RK + i];
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
                    double xw[K];
#pragma unroll
                    for (int bb = 0; bb < K; ++bb) xw[bb] = XW[s * K + bb];
                    const double dy = SY[s] - by;
                    const double e1[1] = {ev[i]}, dx1[1] = {SX[s] - bx}, dy1[1] = {dy * dy};
                    hm_rows_win<K, false, 2>(e1, dx1, dy1, hw.i0, hw.b0, xw, c);
                }
            }
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < K; ++i) TL[(ph * R + t) * K + i] = c[0][i];
    }
    __syncthreads();
    for (int i = tid; i < RK; i += 256) {
        double v = TL[i];
#pragma unroll
        for (int p = 1; p < NPH; ++p) v += TL[p * RK + i];
        local[(size_t)n * RK + i] = hw.om[i % K] * v;
    }
}

// ----------------------------------------------------------------- down pass

// L2L (bbfmm.h:1070-1071) of one level: one workgroup per child, local[child] +=
// S[slot >> 1] (x) S[slot & 1] total[parent], the parent's total being complete (the
// levels run top-down).
template <int NP, int K>
__global__ void __launch_bounds__(256) k_ho_l2l(const int* __restrict__ nodes, const int* __restrict__ parent,
                                                const int* __restrict__ slot, const HoTables* __restrict__ T,
                                                double* __restrict__ local) {
    constexpr int R = NP * NP, RK = R * K;
    __shared__ double PT[RK], X[RK], S[2 * R];
    const int n = nodes[blockIdx.x], p = parent[n], q = slot[n];
    for (int i = threadIdx.x; i < 2 * R; i += blockDim.x) S[i] = T->S[i / R][i % R];
    for (int e = threadIdx.x; e < RK; e += blockDim.x) PT[e] = local[(size_t)p * RK + e];
    __syncthreads();
    for (int e = threadIdx.x; e < RK; e += blockDim.x) {  // along x: X[py][cx]
        const int rr = e / K, b = e - rr * K, py = rr / NP, cxi = rr - py * NP;
        const double* Sq = S + (q & 1) * R + cxi * NP;
        const double* Pq = PT + (py * NP) * K + b;
        double acc = 0.0;
#pragma unroll
        for (int px = 0; px < NP; ++px) acc = __builtin_fma(Sq[px], Pq[px * K], acc);
        X[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < RK; e += blockDim.x) {  // along y: child[cy][cx]
        const int rr = e / K, b = e - rr * K, cyi = rr / NP, cxi = rr - cyi * NP;
        const double* Sq = S + (q >> 1) * R + cyi * NP;
        const double* Xq = X + cxi * K + b;
        double acc = 0.0;
#pragma unroll
        for (int py = 0; py < NP; ++py) acc = __builtin_fma(Sq[py], Xq[py * NP * K], acc);
        local[(size_t)n * RK + e] += acc;
    }
}

// L2P (bbfmm.h:1104): one wave per leaf, one point per lane, added to what the near
// field and the corrections stored (as k_down_tier: xsub fuses aniso.m's x - mforward(x)).
template <int NP, int K>
__global__ void __launch_bounds__(64) k_ho_l2p(const int4* __restrict__ leafInfo, const double* __restrict__ ncx,
                                               const double* __restrict__ ncy, const double* __restrict__ nrx,
                                               const double* __restrict__ nry, const double* __restrict__ pxT,
                                               const double* __restrict__ pyT, const HoTables* __restrict__ T,
                                               const double* __restrict__ local, const int* __restrict__ operm,
                                               int64_t obase, int64_t ldo, double scale, double* __restrict__ out,
                                               const double* __restrict__ xsub, int64_t ldx) {
    constexpr int R = NP * NP, RK = R * K;
    __shared__ double L[RK], W[2 * NP][64];
    const int4 info = leafInfo[blockIdx.x];
    const int n = info.x, nT = info.z;
    const int64_t tb = info.y;
    for (int e = threadIdx.x; e < RK; e += blockDim.x) L[e] = local[(size_t)n * RK + e];
    __syncthreads();
    const double cx = ncx[n], cy = ncy[n], irx = 1.0 / nrx[n], iry = 1.0 / nry[n];
    for (int p = threadIdx.x; p < nT; p += blockDim.x) {
        const int64_t kpos = tb + p;
        double Sx[NP], Sy[NP], v[K];
        ho_cheb_weights<NP>(T, (pxT[kpos] - cx) * irx, Sx);
        ho_cheb_weights<NP>(T, (pyT[kpos] - cy) * iry, Sy);
#pragma unroll
        for (int i = 0; i < NP; ++i) {  // the lane's weights in its own LDS column: the loop below indexes them
            W[i][threadIdx.x] = Sx[i];
            W[NP + i][threadIdx.x] = Sy[i];
        }
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] = 0.0;
#pragma unroll 2
        for (int e = 0; e < R; ++e) {  // (rolled: unrolled it keeps R x K LDS values live and spills)
            const double w = W[e % NP][threadIdx.x] * W[NP + e / NP][threadIdx.x];
#pragma unroll
            for (int i = 0; i < K; ++i) v[i] = __builtin_fma(w, L[e * K + i], v[i]);
        }
        const int64_t o = out_index(operm, obase, kpos);
        if (xsub) {
#pragma unroll
            for (int i = 0; i < K; ++i)
                out[(size_t)i * ldo + o] = xsub[(size_t)i * ldx + o] - (out[(size_t)i * ldo + o] + scale * v[i]);
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i) out[(size_t)i * ldo + o] += scale * v[i];
        }
    }
}

// ----------------------------------------------------------------- launchers

#define ANISO_HO_DISPATCH(np, k, CALL)                                                                       \
    switch ((np) * 16 + (k)) {                                                                               \
        case 6 * 16 + 2: { constexpr int NN = 6, KK = 2; CALL; } break;                                      \
        case 6 * 16 + 4: { constexpr int NN = 6, KK = 4; CALL; } break;                                      \
        case 6 * 16 + 5: { constexpr int NN = 6, KK = 5; CALL; } break;                                      \
        case 6 * 16 + 8: { constexpr int NN = 6, KK = 8; CALL; } break;                                      \
        case 8 * 16 + 2: { constexpr int NN = 8, KK = 2; CALL; } break;                                      \
        case 8 * 16 + 4: { constexpr int NN = 8, KK = 4; CALL; } break;                                      \
        case 8 * 16 + 5: { constexpr int NN = 8, KK = 5; CALL; } break;                                      \
        case 8 * 16 + 8: { constexpr int NN = 8, KK = 8; CALL; } break;                                      \
        default:                                                                                             \
            throw std::invalid_argument("high-order apply: unsupported order / block count " +               \
                                        std::to_string(np) + " / " + std::to_string(k));                     \
    }

void launch_ho_cache_att(int np, int64_t npairs, const int* pairTgt, const int* src, const NodeBoxes& b,
                         const double* stcoef, const Params* P, const HoTables* T, double* E, hipStream_t s) {
    if (npairs <= 0) return;
    const int64_t total = npairs * np * np * np * np;
    if (blocks_for(total, 256) > 0x7fffffffu) throw std::invalid_argument("high-order E cache: too many pairs for one launch");
    if (np == 6) k_ho_cache_att<6><<<blocks_for(total, 256), 256, 0, s>>>(total, pairTgt, src, b.cx, b.cy, b.rx, b.ry, stcoef, P, T, E);
    else if (np == 8) k_ho_cache_att<8><<<blocks_for(total, 256), 256, 0, s>>>(total, pairTgt, src, b.cx, b.cy, b.rx, b.ry, stcoef, P, T, E);
    else throw std::invalid_argument("high-order E cache: np must be 6 or 8");
    HIP_LAUNCH_CHECK();
}

void launch_ho_p2m(int np, int K, int nl, const int4* leafInfo, const NodeBoxes& b, const TreePoints& pts,
                   const double* fT, const HoTables* T, double* mult, hipStream_t s) {
    if (nl <= 0) return;
    ANISO_HO_DISPATCH(np, K, (k_ho_p2m<NN, KK><<<nl, 64, 0, s>>>(leafInfo, b.cx, b.cy, b.rx, b.ry, pts.px, pts.py, fT, T,
                                                                  mult)));
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2m(int np, int K, int nn, const int* nodes, const int4* child, const HoTables* T, double* mult,
                   hipStream_t s) {
    if (nn <= 0) return;
    ANISO_HO_DISPATCH(np, K, (k_ho_m2m<NN, KK><<<nn, 256, 0, s>>>(nodes, child, T, mult)));
    HIP_LAUNCH_CHECK();
}

void launch_ho_m2l(int np, int K, const PairList& pl, const double* E, const NodeBoxes& b, const HoTables* T,
                   const HarmWeights& hw, const HarmWindow* win, const double* mult, double* local, hipStream_t s) {
    if (pl.ntgt <= 0) return;
    if (win && K != kMaxRhs) throw std::invalid_argument("high-order M2L: the offset form takes 8 blocks per pass");
    HoHarm a;
    static_cast<HarmWeights&>(a) = hw;
    a.i0 = win ? win->i0 : 0;
    a.b0 = win ? win->b0 : 0;
    ANISO_HO_DISPATCH(np, K, (k_ho_m2l<NN, KK><<<pl.ntgt, 256, 0, s>>>(pl.tgt, pl.ptr, pl.src, pl.blk, E, b.cx, b.cy,
                                                                        b.rx, b.ry, T, a, mult, local)));
    HIP_LAUNCH_CHECK();
}

void launch_ho_l2l(int np, int K, int nn, const int* nodes, const int* parent, const int* slot, const HoTables* T,
                   double* local, hipStream_t s) {
    if (nn <= 0) return;
    ANISO_HO_DISPATCH(np, K, (k_ho_l2l<NN, KK><<<nn, 256, 0, s>>>(nodes, parent, slot, T, local)));
    HIP_LAUNCH_CHECK();
}

void launch_ho_l2p(int np, int K, int nl, const int4* leafInfo, const NodeBoxes& b, const TreePoints& pts,
                   const HoTables* T, const double* local, double scale, const OutRows& o, hipStream_t s) {
    if (nl <= 0) return;
    ANISO_HO_DISPATCH(np, K, (k_ho_l2p<NN, KK><<<nl, 64, 0, s>>>(leafInfo, b.cx, b.cy, b.rx, b.ry, pts.px, pts.py, T,
                                                                  local, o.perm, o.base, o.ld, scale, o.out, o.minuend,
                                                                  o.minuendLd)));
    HIP_LAUNCH_CHECK();
}

#undef ANISO_HO_DISPATCH

}  // namespace aniso
