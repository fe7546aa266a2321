// direct.hip -- direct (all-pairs) evaluation of the integral operator at chosen
// target points (DESIGN.md "Accuracy of the method"): no tree, no interaction lists,
// no translations, no caches.
//
//   y_t = sum_j pair_kernel(m, x_j, x_t) f_j          over all N sources j
//
// with f = input x quadrature weight (x sigma_s where the apply multiplies it), the
// same charges the near field of the apply multiplies.  It is what the apply computes
// on a one-leaf tree (maxLevel = 0), so it measures the far-field approximation of any
// other tree -- at nt x N line integrals per call.
//
// Harmonic form (harmonic.hip's identity): the modes share e^-tau / r, and cos(m th)
// = T_m(c), c = dx / r, so ONE line integral and one 1 / r per (target, source) pair
// serve every mode.  For aniso.m's mixes, out_i = sum_j w_|j| K_|i+j| x_|j|, and
// 2 T_i T_b = T_{i+b} + T_|i-b|:
//     out_i += (e^-tau / r) T_i(c) S,   S = sum_b hw_b T_b(c) f_b,
// hw_0 = w_0, hw_b = 2 w_b (the mixes' row 0: hw_b = mix[b][0][b]).  A single mode id
// is the same with one input row, hw = [1] and the one output degree id.  The r = 0
// entry (sigma_t at the point, mode 0 only) is added apart: dw_i f_i sigma_t(x_t).
//
// Shape: one workgroup = one target x 1,024 consecutive sources in tree order (a
// wave's 64 sources are neighbours in space: walks of similar length towards the
// target).  Per-thread fp64 partial sums, then a fixed-order reduction: wave shuffles,
// the workgroup's four waves in order, one partial per (target, source block), and a
// second kernel that sums a target's partials in a fixed order.  No atomics: a repeat
// gives the same bits, and a target's value does not depend on the other targets of
// the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "line_integral.hpp"

namespace aniso {

constexpr int kDirThreads = 256;
constexpr int kDirPerThread = 4;  // sources per thread: a workgroup covers 1,024 tree positions
constexpr int kDirBlock = kDirThreads * kDirPerThread;

int64_t direct_blocks(int64_t N) { return (N + kDirBlock - 1) / kDirBlock; }

static __device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// KO output rows (Chebyshev degrees m0 .. m0 + KO - 1, the first nout of them live)
// of targets t0 .. t0 + gridDim.y - 1 from all nb input rows.
template <int KO>
__global__ void __launch_bounds__(kDirThreads) k_direct(DirectArgs a) {
    __shared__ double red[kDirThreads / kWave][KO];
    const int tl = blockIdx.y;
    const int64_t tk = a.iperm[a.tg[a.t0 + tl]];  // the target's tree position
    const double bx = a.pxT[tk], by = a.pyT[tk];
    double acc[KO];
#pragma unroll
    for (int r = 0; r < KO; ++r) acc[r] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * kDirBlock + threadIdx.x;
    for (int it = 0; it < kDirPerThread; ++it) {
        const int64_t k = base + (int64_t)it * kDirThreads;
        if (k >= a.N) break;
        const int64_t o = a.perm[k];
        const double wk = a.sigT ? a.sigT[k] * a.wT[k] : a.wT[k];
        if (k == tk) {  // r = 0: sigma_t at the point, mode 0 only
            const double st = sigma_eval(a.P, a.stcoef, bx, by);
#pragma unroll
            for (int r = 0; r < KO; ++r)
                if (r < a.nout && a.dw[r] != 0.0) acc[r] += st * a.dw[r] * (a.x[(size_t)(a.drow0 + r) * a.ldx + o] * wk);
            continue;
        }
        const double ax = a.pxT[k], ay = a.pyT[k];
        const double ddx = ax - bx, ddy = ay - by;
        const double ir = 1.0 / sqrt(ddx * ddx + ddy * ddy);
        const double c = ddx * ir, c2 = 2.0 * c;
        // S = sum_b hw_b T_b(c) f_b
        double tp = 1.0, tc = c;  // T_b, T_{b+1}
        double S = 0.0;
        for (int b = 0; b < a.nb; ++b) {
            S += a.hw[b] * tp * (a.x[(size_t)b * a.ldx + o] * wk);
            const double tn = c2 * tc - tp;
            tp = tc;
            tc = tn;
        }
        const double gS = pair_kernel(a.P, a.stcoef, kAttMode, ax, ay, bx, by) * ir * S;
        tp = 1.0;
        tc = c;
        for (int m = 0; m < a.m0; ++m) {
            const double tn = c2 * tc - tp;
            tp = tc;
            tc = tn;
        }
#pragma unroll
        for (int r = 0; r < KO; ++r) {
            acc[r] += gS * tp;
            const double tn = c2 * tc - tp;
            tp = tc;
            tc = tn;
        }
    }
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
    for (int r = 0; r < KO; ++r) {
        const double v = wave_sum_fixed(acc[r]);
        if (lane == 0) red[w][r] = v;
    }
    __syncthreads();
    if (threadIdx.x < KO) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kDirThreads / kWave; ++q) v += red[q][threadIdx.x];
        a.part[((size_t)tl * gridDim.x + blockIdx.x) * KO + threadIdx.x] = v;
    }
}

// One wave per (target, output row): the target's nblk partials in a fixed order, then
// the value itself: scale x sum + the corrections read out at the target, or (minuend)
// x - that.
template <int KO>
__global__ void __launch_bounds__(kWave) k_direct_reduce(DirectArgs a, int64_t nblk) {
    const int tl = blockIdx.x, r = blockIdx.y;
    const int lane = threadIdx.x;
    double v = 0.0;
    for (int64_t b = lane; b < nblk; b += kWave) v += a.part[((size_t)tl * nblk + b) * KO + r];
    v = wave_sum_fixed(v);
    if (lane != 0) return;
    const int64_t t = a.t0 + tl, o = a.tg[t];
    const int row = a.orow0 + r;
    v = v * a.scale + a.corr[(size_t)(a.crow0 + r) * a.ldc + o];
    if (a.minuend) v = a.minuend[(size_t)row * a.ldm + o] - v;
    a.out[(size_t)row * a.ldo + t] = v;
}

int direct_rows(int nout) {
    for (int c : {1, 2, 4, 8, 16, 32})
        if (nout <= c) return c;
    return 32;
}

#define ANISO_DIRECT_KO(ko, CALL)                                  \
    switch (ko) {                                                  \
        case 1: { constexpr int KO = 1; CALL; } break;             \
        case 2: { constexpr int KO = 2; CALL; } break;             \
        case 4: { constexpr int KO = 4; CALL; } break;             \
        case 8: { constexpr int KO = 8; CALL; } break;             \
        case 16: { constexpr int KO = 16; CALL; } break;           \
        case 32: { constexpr int KO = 32; CALL; } break;           \
        default: throw std::invalid_argument("direct evaluation: unsupported row count " + std::to_string(ko)); \
    }

void launch_direct(int KO, int ntl, const DirectArgs& a, hipStream_t s) {
    if (ntl <= 0 || a.N <= 0) return;
    if (a.nout < 1 || a.nout > KO) throw std::invalid_argument("direct evaluation: live rows outside the window");
    const int64_t nblk = direct_blocks(a.N);
    const dim3 grid((unsigned)nblk, (unsigned)ntl);
    ANISO_DIRECT_KO(KO, (k_direct<KO><<<grid, kDirThreads, 0, s>>>(a)));
    HIP_LAUNCH_CHECK();
    const dim3 rgrid((unsigned)ntl, (unsigned)a.nout);
    ANISO_DIRECT_KO(KO, (k_direct_reduce<KO><<<rgrid, kWave, 0, s>>>(a, nblk)));
    HIP_LAUNCH_CHECK();
}

}  // namespace aniso
