// solver.hip -- the callers of the hot path: main.cpp's
// forwardOperator u - K_0(sigma_s .* u) (main.cpp:125-136) and the restarted
// GMRES(m) that drives it (gmres.cpp:53-169), with every vector resident in HBM.
// BLAS-1 reductions use a fixed two-level tree so results are deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <exception>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "aniso_op.hpp"
#include "arnoldi.hpp"
#include "arnoldi16.hpp"
#include "arnoldi_cols.hpp"
#include "device_common.hpp"
#include "gmres_driver.hpp"
#include "kernels.hpp"

namespace aniso {

constexpr int kRedBlocks = 512;

// y = alpha x + beta y
__global__ void k_axpby(int64_t n, double alpha, const double* __restrict__ x, double beta, double* __restrict__ y) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = alpha * x[i] + beta * y[i];
}

// z = x - y
__global__ void k_sub(int64_t n, const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ z) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = x[i] - y[i];
}

__global__ void __launch_bounds__(256) k_dot_partial(int64_t n, const double* __restrict__ x,
                                                     const double* __restrict__ y, double* __restrict__ part) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += x[i] * y[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(256) k_dot_final(int nb, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

static unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

// ---- Krylov kernels of the block solve (aniso.m:159-173): classical Gram-Schmidt
// with one reorthogonalisation (CGS2) on device-resident bases.  Every reduction
// has a fixed order (per-block partials, then one block per output), so a solve is
// bitwise reproducible; no host round trip sits inside a step except reading the
// Hessenberg column for the Givens rotations.
constexpr int kDotGroup = 8;  // basis vectors reduced together per pass over w

// part[k * gridDim.x + blk] = sum over this block's chunk of V[k][j] w[j], k < nv
__global__ void __launch_bounds__(256) k_mdot_partial(int64_t n, int nv, const double* __restrict__ V, int64_t ldv,
                                                      const double* __restrict__ w, double* __restrict__ part) {
    __shared__ double red[kDotGroup][256];
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t j0 = (int64_t)blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    for (int k0 = 0; k0 < nv; k0 += kDotGroup) {
        double acc[kDotGroup];
#pragma unroll
        for (int g = 0; g < kDotGroup; ++g) acc[g] = 0.0;
        for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
            const double wj = w[j];
#pragma unroll
            for (int g = 0; g < kDotGroup; ++g)
                if (k0 + g < nv) acc[g] = __builtin_fma(V[(size_t)(k0 + g) * ldv + j], wj, acc[g]);
        }
#pragma unroll
        for (int g = 0; g < kDotGroup; ++g) red[g][threadIdx.x] = acc[g];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o)
#pragma unroll
                for (int g = 0; g < kDotGroup; ++g) red[g][threadIdx.x] += red[g][threadIdx.x + o];
            __syncthreads();
        }
        if ((int)threadIdx.x < kDotGroup && k0 + (int)threadIdx.x < nv)
            part[(size_t)(k0 + threadIdx.x) * gridDim.x + blockIdx.x] = red[threadIdx.x][0];
        __syncthreads();
    }
}

// out[k] (+)= sum_b part[k * nb + b]: one block per k, a fixed order
__global__ void __launch_bounds__(256) k_mdot_final(int nb, const double* __restrict__ part, int accumulate,
                                                    double* __restrict__ out) {
    __shared__ double r[256];
    const int k = blockIdx.x;
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) a += part[(size_t)k * nb + b];
    r[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) r[threadIdx.x] += r[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = accumulate ? out[k] + r[0] : r[0];
}

// w[j] += sign * sum_{k < nv} c[k] V[k][j]
__global__ void __launch_bounds__(256) k_maxpy(int64_t n, int nv, const double* __restrict__ V, int64_t ldv,
                                               const double* __restrict__ c, double sign, double* __restrict__ w) {
    extern __shared__ double cs[];
    for (int k = threadIdx.x; k < nv; k += 256) cs[k] = sign * c[k];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double a = w[j];
    for (int k = 0; k < nv; ++k) a = __builtin_fma(cs[k], V[(size_t)k * ldv + j], a);
    w[j] = a;
}

// y = a x
__global__ void k_scale(int64_t n, double a, const double* __restrict__ x, double* __restrict__ y) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) y[j] = a * x[j];
}

// y = x / sqrt(*nrm2) (a norm computed on the device; 0 stays 0)
__global__ void k_scale_rsqrt(int64_t n, const double* __restrict__ x, const double* __restrict__ nrm2,
                              double* __restrict__ y) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double s = *nrm2 > 0.0 ? 1.0 / sqrt(*nrm2) : 0.0;
    if (j < n) y[j] = x[j] * s;
}

// orig[perm[k]] = tree[k] (the inverse of launch_permute)
__global__ void k_unpermute(int64_t n, const int* __restrict__ perm, const double* __restrict__ tree,
                            double* __restrict__ orig) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) orig[perm[k]] = tree[k];
}

// ---- the CGS2 sweeps with the basis held in registers (nv <= 48 vectors): one read of
// V per sweep.  Each thread owns elements j of its block's chunk;
// the per-block sums of the NV products reduce by xor shuffles inside a wave and then
// over the 4 waves in a fixed order (deterministic).
template <int NV>
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// per-block sums of acc[k] (k < nv) into part[k * gridDim.x + blockIdx.x], and with SQ
// of acc[NA - 1] into row nv: wave sums by xor shuffles, then the 4 waves in a fixed order
template <int NA, bool SQ>
__device__ __forceinline__ void block_partials(const double (&acc)[NA], int nv, double* red, double* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int ND = SQ ? NA - 1 : NA;
#pragma unroll
    for (int k = 0; k < ND; ++k)
        if (k < nv) {
            const double v = wave_sum<0>(acc[k]);
            if (lane == 0) red[wv * NA + k] = v;
        }
    if constexpr (SQ) {
        const double v = wave_sum<0>(acc[NA - 1]);
        if (lane == 0) red[wv * NA + NA - 1] = v;
    }
    __syncthreads();
    const int rows = SQ ? nv + 1 : nv;
    for (int k = threadIdx.x; k < rows; k += blockDim.x) {
        const int i = SQ && k == nv ? NA - 1 : k;
        part[(size_t)k * gridDim.x + blockIdx.x] = ((red[i] + red[NA + i]) + red[2 * NA + i]) + red[3 * NA + i];
    }
}

// pass 1: part[k][blk] = sum over the block's chunk of V[k][j] w[j]
template <int NV>
__global__ void __launch_bounds__(256) k_cgs_dot(int64_t n, int nv, const double* __restrict__ V, int64_t ldv,
                                                 const double* __restrict__ w, double* __restrict__ part) {
    __shared__ double red[4 * NV];
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t j0 = (int64_t)blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        double v[NV];  // every load of the element in flight before the products
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = k < nv ? V[(size_t)k * ldv + j] : 0.0;
        const double wj = w[j];
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (k < nv) acc[k] = __builtin_fma(v[k], wj, acc[k]);
    }
    block_partials<NV, false>(acc, nv, red, part);
}

// pass 2 / 3: w[j] -= sum_k c[k] V[k][j] (k_maxpy's order), then the products of the
// updated w with the same V[k][j] (DOT: the reorthogonalisation's h = V^T w, rows
// 0 .. nv-1) and its square (||w||^2: row nv with DOT, row 0 without)
template <int NV, bool DOT>
__global__ void __launch_bounds__(256) k_cgs_update(int64_t n, int nv, const double* __restrict__ V, int64_t ldv,
                                                    const double* __restrict__ c, double* __restrict__ w,
                                                    double* __restrict__ part) {
    constexpr int NA = DOT ? NV + 1 : 1;
    __shared__ double red[4 * NA];
    __shared__ double cs[NV];
    for (int k = threadIdx.x; k < nv; k += blockDim.x) cs[k] = -c[k];
    __syncthreads();
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t j0 = (int64_t)blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        double v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = k < nv ? V[(size_t)k * ldv + j] : 0.0;
        double a = w[j];
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (k < nv) a = __builtin_fma(cs[k], v[k], a);
        w[j] = a;
        if constexpr (DOT) {
#pragma unroll
            for (int k = 0; k < NV; ++k)
                if (k < nv) acc[k] = __builtin_fma(v[k], a, acc[k]);
        }
        acc[NA - 1] = __builtin_fma(a, a, acc[NA - 1]);
    }
    if constexpr (DOT) block_partials<NA, true>(acc, nv, red, part);
    else block_partials<1, false>(acc, 1, red, part);
}

constexpr int kCgsMaxRegs = 48;  // basis vectors the register-held sweeps take

constexpr int kMdotBlocks = 2048;  // partial sums per reduction (per-block chunks of ~2.5K elements at 1M x 5)

struct Krylov {
    int64_t n;
    hipStream_t s;
    double* part;  // kMdotBlocks x (restart + 1)
    // out[0 .. nv) (+)= V[0 .. nv)^T w
    void mdot(int nv, const double* V, int64_t ldv, const double* w, double* out, bool accumulate) {
        k_mdot_partial<<<kMdotBlocks, 256, 0, s>>>(n, nv, V, ldv, w, part);
        k_mdot_final<<<nv, 256, 0, s>>>(kMdotBlocks, part, accumulate ? 1 : 0, out);
    }
    void maxpy(int nv, const double* V, int64_t ldv, const double* c, double sign, double* w) {
        k_maxpy<<<nblk(n), 256, (size_t)nv * sizeof(double), s>>>(n, nv, V, ldv, c, sign, w);
    }
    // the three sweeps of a CGS2 step over nv basis vectors: h = V^T w; w -= V h with
    // h2 = V^T w from the same read of V; w -= V h2 with ||w||^2 (one read of V each
    // for nv <= kCgsMaxRegs, else the two-pass kernels above)
    template <typename F>
    static void nv_dispatch(int nv, F&& f) {
        if (nv <= 8) f(std::integral_constant<int, 8>{});
        else if (nv <= 16) f(std::integral_constant<int, 16>{});
        else if (nv <= 32) f(std::integral_constant<int, 32>{});
        else f(std::integral_constant<int, kCgsMaxRegs>{});
    }
    void dot(int nv, const double* V, int64_t ldv, const double* w, double* out) {
        if (nv > kCgsMaxRegs) return mdot(nv, V, ldv, w, out, false);
        nv_dispatch(nv, [&](auto c) {
            k_cgs_dot<decltype(c)::value><<<kMdotBlocks, 256, 0, s>>>(n, nv, V, ldv, w, part);
        });
        k_mdot_final<<<nv, 256, 0, s>>>(kMdotBlocks, part, 0, out);
    }
    // w -= V c, then out[k] = V_k . w (k < nv) and out[nv] = w . w
    void updateDot(int nv, const double* V, int64_t ldv, const double* c, double* w, double* out) {
        if (nv > kCgsMaxRegs) {
            maxpy(nv, V, ldv, c, -1.0, w);
            mdot(nv, V, ldv, w, out, false);
            return mdot(1, w, ldv, w, out + nv, false);
        }
        nv_dispatch(nv, [&](auto cc) {
            k_cgs_update<decltype(cc)::value, true><<<kMdotBlocks, 256, 0, s>>>(n, nv, V, ldv, c, w, part);
        });
        k_mdot_final<<<nv + 1, 256, 0, s>>>(kMdotBlocks, part, 0, out);
    }
    void updateNorm(int nv, const double* V, int64_t ldv, const double* c, double* w, double* nrm2) {
        if (nv > kCgsMaxRegs) {
            maxpy(nv, V, ldv, c, -1.0, w);
            return mdot(1, w, ldv, w, nrm2, false);
        }
        nv_dispatch(nv, [&](auto cc) {
            k_cgs_update<decltype(cc)::value, false><<<kMdotBlocks, 256, 0, s>>>(n, nv, V, ldv, c, w, part);
        });
        k_mdot_final<<<1, 256, 0, s>>>(kMdotBlocks, part, 0, nrm2);
    }
};

struct DeviceBlas {
    int64_t n;
    hipStream_t s;
    double* part;
    double* res;
    double dot(const double* x, const double* y) {
        k_dot_partial<<<kRedBlocks, 256, 0, s>>>(n, x, y, part);
        k_dot_final<<<1, 256, 0, s>>>(kRedBlocks, part, res);
        double h = 0;
        HIP_CHECK(hipMemcpyAsync(&h, res, sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        return h;
    }
    double nrm2(const double* x) { return std::sqrt(dot(x, x)); }
    void axpby(double a, const double* x, double b, double* y) { k_axpby<<<nblk(n), 256, 0, s>>>(n, a, x, b, y); }
};

// forwardOperator (main.cpp:125-136): out = u - K_0(sigma_s .* u)
void Operator::forwardDev(const double* u, double* out, hipStream_t s) {
    if (plan.nranks != 1) throw std::logic_error("forward operator on a sharded handle: gather first");
    ensureDevice();
    apply(u, false, dSigmaT.as<double>(), 0, dTmp2.as<double>(), false, s, kStageAll);  // sigma_s .* u inside the up pass
    k_sub<<<nblk(geo.N), 256, 0, s>>>(geo.N, u, dTmp2.as<double>(), out);
}

// main.cpp:121-141: rhs = K_0 q; GMRES(forwardOperator, x, rhs, m, maxit, tol).
// Mirrors gmres.cpp:53-169 (MGS, Givens, restart with Update).  Returns the
// iteration count j on convergence and -j otherwise; hist gets the residual
// printed at the start of every inner iteration plus the final one.
int Operator::gmresHost(const double* q, double* xh, int m, int maxit, double tol, double* hist, int maxhist,
                        double* finalResid) {
    refuseHighOrder("aniso_gmres");
    if (m < 1 || maxit < 0) throw std::invalid_argument("GMRES needs m >= 1 and maxit >= 0");
    needResident(0, "aniso_gmres");
    if (!modeCached(0)) throw std::runtime_error("GMRES before cache(0)");
    ensureDevice();
    const int64_t N = geo.N;
    hipStream_t s = own;
    DevBuf bq, bb, br, bp, bx, bpart, bres;
    bq.upload(q, N * sizeof(double));
    bx.upload(xh, N * sizeof(double));
    bb.alloc(N * sizeof(double));
    br.alloc(N * sizeof(double));
    bp.alloc(N * sizeof(double));
    bpart.alloc(kRedBlocks * sizeof(double));
    bres.alloc(sizeof(double));
    std::vector<DevBuf> v(m + 1);
    for (auto& vi : v) vi.alloc(N * sizeof(double));
    DeviceBlas B{N, s, bpart.as<double>(), bres.as<double>()};
    double* b = bb.as<double>();
    double* r = br.as<double>();
    double* p = bp.as<double>();
    double* x = bx.as<double>();
    mappingDev(bq.as<double>(), 0, b, s, kStageAll);  // rhs = apply_mapping(charge)
    const int ld = m + 1;
    std::vector<double> H((size_t)ld * ld, 0.0), sv(ld, 0.0), cs(ld, 0.0), sn(ld, 0.0);
    int nh = 0, ret;
    auto rot = [](double& dx, double& dy, double c, double sn_) {
        double t = c * dx + sn_ * dy;
        dy = -sn_ * dx + c * dy;
        dx = t;
    };
    auto gen = [](double dx, double dy, double& c, double& sn_) {
        if (dy == 0.0) { c = 1.0; sn_ = 0.0; }
        else if (std::fabs(dy) > std::fabs(dx)) { double t = dx / dy; sn_ = 1.0 / std::sqrt(1.0 + t * t); c = t * sn_; }
        else { double t = dy / dx; c = 1.0 / std::sqrt(1.0 + t * t); sn_ = t * c; }
    };
    auto update = [&](int k) {  // Update (gmres.cpp:12-24)
        std::vector<double> y(sv.begin(), sv.begin() + k + 1);
        for (int i = k; i >= 0; i--) {
            y[i] /= H[i + (size_t)i * ld];
            for (int j2 = i - 1; j2 >= 0; j2--) y[j2] -= H[j2 + (size_t)i * ld] * y[i];
        }
        for (int j2 = 0; j2 <= k; j2++) B.axpby(y[j2], v[j2].as<double>(), 1.0, x);
    };
    double normb = B.nrm2(b);
    forwardDev(x, p, s);
    k_sub<<<nblk(N), 256, 0, s>>>(N, b, p, r);
    double beta = B.nrm2(r), resid;
    if (normb == 0.0) normb = 1;
    int i = 0, j = 1;
    if ((resid = beta / normb) <= tol) {
        ret = 0;
        goto done;
    }
    while (j <= maxit) {
        HIP_CHECK(hipMemcpyAsync(v[0].p, r, N * sizeof(double), hipMemcpyDeviceToDevice, s));
        B.axpby(0.0, r, 1.0 / beta, v[0].as<double>());
        std::fill(sv.begin(), sv.end(), 0.0);
        sv[0] = beta;
        for (i = 0; i < m && j <= maxit; i++, j++) {
            if (hist && nh < maxhist) hist[nh++] = resid;
            forwardDev(v[i].as<double>(), p, s);
            for (int k = 0; k <= i; k++) {
                double h = B.dot(p, v[k].as<double>());
                H[k + (size_t)i * ld] = h;
                B.axpby(-h, v[k].as<double>(), 1.0, p);
            }
            double hn = B.nrm2(p);
            H[(i + 1) + (size_t)i * ld] = hn;
            HIP_CHECK(hipMemcpyAsync(v[i + 1].p, p, N * sizeof(double), hipMemcpyDeviceToDevice, s));
            B.axpby(0.0, p, 1.0 / hn, v[i + 1].as<double>());
            for (int k = 0; k < i; k++) rot(H[k + (size_t)i * ld], H[(k + 1) + (size_t)i * ld], cs[k], sn[k]);
            gen(H[i + (size_t)i * ld], H[(i + 1) + (size_t)i * ld], cs[i], sn[i]);
            rot(H[i + (size_t)i * ld], H[(i + 1) + (size_t)i * ld], cs[i], sn[i]);
            rot(sv[i], sv[i + 1], cs[i], sn[i]);
            if ((resid = std::fabs(sv[i + 1]) / normb) < tol) {
                update(i);
                ret = j;
                goto done;
            }
        }
        update(i - 1);
        forwardDev(x, p, s);
        k_sub<<<nblk(N), 256, 0, s>>>(N, b, p, r);
        beta = B.nrm2(r);
        if ((resid = beta / normb) < tol) {
            ret = j;
            goto done;
        }
    }
    ret = -j;
done:
    if (hist && nh < maxhist) hist[nh++] = resid;
    if (finalResid) *finalResid = resid;
    HIP_CHECK(hipMemcpyAsync(xh, x, N * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    checkDeviceErrors();
    return ret;
}

// The CGS2 sweeps as library primitives for a caller's own Krylov loop (the sharded
// GMRES of aniso_amd.solve.gmres_dist reduces their outputs over the ranks between
// the calls): out[k] = V_k . w; and w -= V c followed by out[k] = V_k . w, out[nv] =
// w . w (dots) or out[0] = w . w.  Device pointers, on stream s.
void Operator::krylovDot(int64_t n, int nv, const double* V, int64_t ldv, const double* w, double* out,
                         hipStream_t s) {
    if (n < 0 || nv < 1 || ldv < n) throw std::invalid_argument("krylov dot: bad sizes");
    ensureDevice();
    dKryPart.alloc(std::max(dKryPart.bytes, (size_t)kMdotBlocks * (nv + 2) * sizeof(double)));
    Krylov kr{n, s, dKryPart.as<double>()};
    kr.dot(nv, V, ldv, w, out);
}

void Operator::krylovUpdate(int64_t n, int nv, const double* V, int64_t ldv, const double* c, double* w,
                            double* out, bool dots, hipStream_t s) {
    if (n < 0 || nv < 1 || ldv < n) throw std::invalid_argument("krylov update: bad sizes");
    ensureDevice();
    dKryPart.alloc(std::max(dKryPart.bytes, (size_t)kMdotBlocks * (nv + 2) * sizeof(double)));
    Krylov kr{n, s, dKryPart.as<double>()};
    if (dots) kr.updateDot(nv, V, ldv, c, w, out);
    else kr.updateNorm(nv, V, ldv, c, w, out);
}

// ---- DCGS2 Arnoldi on a never-rewritten basis (arnoldi.hpp): the library primitives
// (aniso_arnoldi_*) and the block solve on them.  dKryPart holds the sweeps' partial
// sums (arn::kParts per row).
int64_t arn_state_doubles(int m) { return arn::Layout(m).total; }

static void check_arnoldi(int m, int j) {
    if (m < 1 || j < 0 || j >= m) throw std::invalid_argument("arnoldi: need 0 <= j < m");
}

// the small kernels' fast paths stage up to ~100 KB of LDS: their dynamic limit is
// raised once per device (a function attribute binds to the device current at the
// call), checked, before any launch of them on that device
static void arn_small_kernel_attrs() {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) throw_hip(e, __FILE__, __LINE__);
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return;
    for (const void* f : {(const void*)arn::k_arn_coef, (const void*)arn::k_arn_column}) {
        e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024);
        if (e != hipSuccess) throw_hip(e, __FILE__, __LINE__);
    }
    done.fetch_or(bit, std::memory_order_acq_rel);
}

// dKryPart for sweeps of `rows` rows.  DevBuf::alloc frees and reallocates (a device
// synchronisation) on every size change, so it grows geometrically; the Arnoldi entry
// points that know the restart length size it for the whole cycle at once
void Operator::arnoldiParts(int rows) {
    arn_small_kernel_attrs();
    const size_t need = (size_t)arn::kParts * (rows + 2) * sizeof(double);
    if (need > dKryPart.bytes) dKryPart.alloc(std::max(need, 2 * dKryPart.bytes));
}

void Operator::arnoldiBegin(int64_t n, int m, const double* V, int64_t ldv, double* st, const double* rr,
                            double normb, double* status, hipStream_t s) {
    if (m < 1 || n < 0 || ldv < n || !(normb > 0.0)) throw std::invalid_argument("arnoldi begin: bad sizes or |b|");
    ensureDevice();
    if (rr) {
        arn::k_arn_begin<<<1, arn::kThreads, 0, s>>>(m, st, rr, 1, normb, status);
        HIP_LAUNCH_CHECK();
        return;
    }
    arnoldiParts(m + 2);
    arn::launch_project(n, 1, V, ldv, V, dKryPart.as<double>(), s);
    arn::k_arn_begin<<<1, arn::kThreads, 0, s>>>(m, st, dKryPart.as<double>(), arn::kParts, normb, status);
    HIP_LAUNCH_CHECK();
}

void Operator::arnoldiStep(int64_t n, int m, int j, double* V, int64_t ldv, const double* w, double* st,
                           double* status, hipStream_t s) {
    check_arnoldi(m, j);
    if (n < 0 || ldv < n) throw std::invalid_argument("arnoldi step: bad sizes");
    ensureDevice();
    arnoldiParts(m + 2);
    double* part = dKryPart.as<double>();
    arn::launch_project(n, j + 1, V, ldv, w, part, s);
    arn::k_arn_coef<<<1, arn::kThreads, arn::coef_lds(j), s>>>(m, j, st, part, arn::kParts);
    HIP_LAUNCH_CHECK();
    arn::launch_update(n, j + 1, V, ldv, w, st, m, part, s);
    arn::k_arn_column<<<1, arn::kThreads, arn::column_lds(j), s>>>(m, j, st, part, arn::kParts, status);
    HIP_LAUNCH_CHECK();
}

void Operator::arnoldiProject(int64_t n, int j, const double* V, int64_t ldv, const double* w, double* out,
                              hipStream_t s) {
    if (n < 0 || j < 0 || ldv < n) throw std::invalid_argument("arnoldi project: bad sizes");
    ensureDevice();
    arnoldiParts(j + 1);
    arn::launch_project(n, j + 1, V, ldv, w, dKryPart.as<double>(), s);
    arn::k_arn_rows<<<1, arn::kThreads, (size_t)(j + 1) * sizeof(double), s>>>(dKryPart.as<double>(), arn::kParts,
                                                                                 j + 1, out);
    HIP_LAUNCH_CHECK();
}

void Operator::arnoldiCoef(int m, int j, double* st, const double* red, hipStream_t s) {
    check_arnoldi(m, j);
    ensureDevice();
    arn_small_kernel_attrs();
    arn::k_arn_coef<<<1, arn::kThreads, arn::coef_lds(j), s>>>(m, j, st, red, 1);
    HIP_LAUNCH_CHECK();
}

void Operator::arnoldiUpdate(int64_t n, int m, int j, double* V, int64_t ldv, const double* w, const double* st,
                             double* out, hipStream_t s) {
    check_arnoldi(m, j);
    if (n < 0 || ldv < n) throw std::invalid_argument("arnoldi update: bad sizes");
    ensureDevice();
    arnoldiParts(m + 2);
    arn::launch_update(n, j + 1, V, ldv, w, st, m, dKryPart.as<double>(), s);
    arn::k_arn_rows<<<1, arn::kThreads, (size_t)(j + 2) * sizeof(double), s>>>(dKryPart.as<double>(), arn::kParts,
                                                                                 j + 2, out);
    HIP_LAUNCH_CHECK();
}

void Operator::arnoldiColumn(int m, int j, double* st, const double* red, double* status, hipStream_t s) {
    check_arnoldi(m, j);
    ensureDevice();
    arn_small_kernel_attrs();
    arn::k_arn_column<<<1, arn::kThreads, arn::column_lds(j), s>>>(m, j, st, red, 1, status);
    HIP_LAUNCH_CHECK();
}

void Operator::arnoldiSolution(int64_t n, int m, int used, const double* V, int64_t ldv, double* st, double* x,
                               hipStream_t s) {
    if (m < 1 || used < 0 || used > m || n < 0 || ldv < n) throw std::invalid_argument("arnoldi solution: bad sizes");
    ensureDevice();
    if (used == 0) return;
    arn::k_arn_solve<<<1, arn::kThreads, arn::solve_lds(used), s>>>(m, used, st);
    HIP_LAUNCH_CHECK();
    if (n > 0)
        arn::k_arn_axpy<<<nblk(n), arn::kThreads, (size_t)used * sizeof(double), s>>>(n, used, V, ldv,
                                                                                        st + arn::Layout(m).y, x);
    HIP_LAUNCH_CHECK();
}

// The restarted GMRES of one system (GmresSystem, gmres_driver.hpp), the loop of the block
// solve and of its sharded form: MATLAB's semantics as described at blockSolveDev, g.x
// updated in place.  Returns the total step count (negative if not converged); hist gets
// the relative residual estimate after every step, *relresOut the final one.  hs: the
// status words {relres, r', steps, -} that startCycle and step store.  Every decision is
// taken from those words, which the sharded solve's kernels compute from all-reduced sums:
// no rank takes a branch of its own.
int Operator::gmresRestarted(const GmresSystem& g, StatusBlock& hs, double tol, int maxit, double* hist, int maxhist,
                             double* relresOut, hipStream_t s) {
    const int64_t L = g.L;
    const int m = g.m;
    double* const V = g.V;
    *relresOut = 0.0;
    if (g.normb == 0.0) {  // b = 0: x = 0
        if (L > 0) HIP_CHECK(hipMemsetAsync(g.x, 0, L * sizeof(double), s));
        return 0;
    }
    bool xZero = g.xZero;
    // r = b - A x into V[0], then the cycle's start; returns |r| / |b|
    auto residual = [&] {
        for (int tries = 0;; ++tries) {
            if (xZero) {
                if (L > 0) HIP_CHECK(hipMemcpyAsync(V, g.b, L * sizeof(double), hipMemcpyDeviceToDevice, s));
            } else {
                g.matvec(g.x);
                if (L > 0) k_sub<<<nblk(L), 256, 0, s>>>(L, g.b, g.w, V);
            }
            g.startCycle();
            hs.sync(s);
            // a residual whose matvec ran on an invalid fused launch is redone, once
            if (!g.spoiled() || tries > 0) return hs.p[0];
        }
    };
    int nh = 0, total = 0;
    double relres = residual();
    bool conv = relres <= tol;
    LookAhead la;
    // the relaxed rule: `est` is the latest estimate the host holds (a residual is never relaxed)
    double est = relres;
    auto arnoldiMatvec = [&](const double* v) {
        if (g.matvecLow && g.relax > 0.0 && est <= g.relax) g.matvecLow(v);
        else g.matvec(v);
    };
    for (int cyc = 0; cyc < maxit && !conv; ++cyc) {
        if (hs.p[1] == 0.0) break;  // |r| = 0 in floating point
        int used = 0;
        bool ahead = false;  // the matvec of V[j] is already enqueued
        la.clear();
        est = relres;  // the cycle's explicit relres
        for (int j = 0; j < m; ++j) {
            if (!ahead) arnoldiMatvec(V + (size_t)j * L);
            g.step(j);
            hs.post(s);
            // the next step's matvec before the host reads the status, unless this step is
            // predicted to converge (LookAhead); sharded, every rank holds the same
            // estimates: all ranks enqueue it, or none
            ahead = j + 1 < m && !la.near(tol);
            if (ahead) arnoldiMatvec(V + (size_t)(j + 1) * L);
            hs.wait();
            if (g.spoiled()) {
                // this step's matvec (or the look-ahead one) ran on an invalid fused launch:
                // the cycle ends before this step (columns 0 .. j - 1 are valid) and restarts
                // from its update on the tier launches
                ahead = false;
                break;
            }
            const double rel = hs.p[0], rnext = hs.p[1];
            if (hs.p[2] != (double)(j + 1))  // the column kernel of this step did not run
                throw std::runtime_error("block solve: Arnoldi step " + std::to_string(j) + " left no status");
            ++total;
            used = j + 1;
            relres = rel;
            est = rel;
            la.push(rel);
            if (hist && nh < maxhist) hist[nh++] = rel;
            if (rel <= tol || rnext == 0.0) break;  // converged (estimate) or lucky breakdown
        }
        arnoldiSolution(L, m, used, V, L, g.st, g.x, s);  // x += P T R^-1 g
        xZero = xZero && used == 0;
        relres = residual();
        conv = relres <= tol;
    }
    *relresOut = relres;
    return conv ? total : -std::max(total, 1);
}

// aniso.m:159-173: u = gmres(A, rhs, restart, tol, maxit) with A(x) = x - mforward(x)
// (aniso.m:155) on the nb = ks stacked blocks.  MATLAB's restarted GMRES semantics:
// x0 = the given guess, at most maxit cycles of at most `restart` steps, converged
// when ||rhs - A x|| / ||rhs|| <= tol (the estimate inside a cycle, confirmed by the
// explicit residual at its end).  The vectors are permuted once into tree order and
// every Krylov vector ((restart + 1) x ks x N doubles) stays in HBM; the Arnoldi
// process is DCGS2 on the device (arnoldi.hpp): per step the matvec, two sweeps over
// the basis and two one-block kernels; the host reads one status word per step
// while the GPU already runs the next step's matvec.  rhs / x: device, original
// order, block b at b * N.  Returns the total step count (negative if not converged);
// hist gets the relative residual estimate after every step.
int Operator::blockSolveDev(const double* rhs, double* x, int restart, double tol, int maxit, double* hist,
                            int maxhist, double* relresOut, hipStream_t s) {
    return blockSolveRun(rhs, x, restart, tol, maxit, 0.0, nullptr, hist, maxhist, relresOut, s);
}

// The relaxed solve.  What the handle rules out first (np = 4, a shard,
// ks > 8), then the arguments, then the state: nothing of this touches the device.
int Operator::blockSolveRelaxedDev(const double* rhs, double* x, int restart, double tol, int maxit, double relax,
                                   double* hist, int maxhist, double* relresOut, hipStream_t s) {
    const char* const what = "aniso_block_solve_relaxed_dev";
    blockOpF32Refuse(what);
    if (restart < 1 || maxit < 1 || !(tol > 0.0))
        throw std::invalid_argument(std::string(what) + " needs restart >= 1, maxit >= 1, tol > 0");
    if (std::isnan(relax)) throw std::invalid_argument(std::string(what) + ": relax is NaN");
    blockOpF32Ready(what);
    if (relax < 0.0) relax = kRelaxFactor * tol;
    relaxedCalls.clear();
    return blockSolveRun(rhs, x, restart, tol, maxit, relax, &relaxedCalls, hist, maxhist, relresOut, s);
}

int Operator::blockSolveRelaxedHost(const double* rhs, double* x, int restart, double tol, int maxit, double relax,
                                    double* hist, int maxhist, double* relres) {
    const char* const what = "aniso_block_solve_relaxed";
    blockOpF32Refuse(what);
    if (restart < 1 || maxit < 1 || !(tol > 0.0))
        throw std::invalid_argument(std::string(what) + " needs restart >= 1, maxit >= 1, tol > 0");
    if (std::isnan(relax)) throw std::invalid_argument(std::string(what) + ": relax is NaN");
    blockOpF32Ready(what);
    ensureDevice();
    const size_t bytes = (size_t)ks * geo.N * sizeof(double);
    DevBuf db, dx;
    db.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(db.p, rhs, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, x, bytes, hipMemcpyHostToDevice, own));
    const int it = blockSolveRelaxedDev(db.as<double>(), dx.as<double>(), restart, tol, maxit, relax, hist, maxhist,
                                        relres, own);
    HIP_CHECK(hipMemcpyAsync(x, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return it;
}

int Operator::blockSolveRun(const double* rhs, double* x, int restart, double tol, int maxit, double relax,
                            std::vector<int>* rec, double* hist, int maxhist, double* relresOut, hipStream_t s) {
    refuseHoShard("aniso_block_solve");
    checkBlockLimit(false);
    if (plan.nranks != 1) throw std::logic_error("block solve on a sharded handle");
    if (!coeffSet) throw std::runtime_error("block solve before setCoeff");
    for (int m = 0; m < kernelSize; ++m)
        if (!modes[m].tables) throw std::runtime_error("block solve before cache(" + std::to_string(m) + ")");
    if (!harmonicReady())  // the matvec streams the per-mode operators
        for (int m = 0; m < kernelSize; ++m) needResident(m, "the block solve without the mode-shared caches");
    if (restart < 1 || maxit < 1 || !(tol > 0.0)) throw std::invalid_argument("block solve needs restart >= 1, maxit >= 1, tol > 0");
    ensureDevice();
    checkDeviceErrors();
    const int64_t N = geo.N, L = (int64_t)ks * N;
    const int m = restart;
    const arn::Layout lay(m);
    DevBuf bB, bX, bW, bV, bSt;
    auto allocAll = [&] {
        bB.alloc(L * sizeof(double));
        bX.alloc(L * sizeof(double));
        bW.alloc(L * sizeof(double));
        bV.alloc((size_t)(m + 1) * L * sizeof(double));
        bSt.alloc((size_t)lay.total * sizeof(double));
        arnoldiParts(m + 2);
    };
    if (relax > 0.0) {
        // the relaxed solve: every buffer, then the float mirrors (their own message), before
        // the first launch
        try {
            allocAll();
        } catch (const std::exception& e) {
            throw std::runtime_error("relaxed block solve: the Krylov basis of (restart + 1) x ks x N = " +
                                     std::to_string(m + 1) + " x " + std::to_string(ks) + " x " + std::to_string(N) +
                                     " doubles (" + std::to_string((size_t)(m + 1) * L * sizeof(double)) +
                                     " bytes) and 3 x " + std::to_string(L * sizeof(double)) +
                                     " bytes of work vectors could not be allocated: " + e.what());
        }
        cacheF32();
    } else {
        allocAll();
    }
    double *b = bB.as<double>(), *xt = bX.as<double>(), *w = bW.as<double>();
    double* V = bV.as<double>();
    double* st = bSt.as<double>();
    const int* perm = dPerm.as<int>();
    for (int k = 0; k < ks; ++k) {  // tree order: the operator needs no permutation gathers
        launch_permute(N, perm, rhs + (size_t)k * N, b + (size_t)k * N, s);
        launch_permute(N, perm, x + (size_t)k * N, xt + (size_t)k * N, s);
    }
    // the status word {relres, r', steps} in mapped host memory: the column kernel
    // stores it there and the host waits for an event behind it, not a stream drain
    StatusBlock hs;
    hs.alloc(4);
    double* stat = hs.dev;
    auto sumsq = [&](const double* v) {  // |v|^2 on the host (once per solve)
        arnoldiProject(L, 0, v, L, v, stat, s);
        hs.sync(s);
        return hs.p[0];
    };
    // a fused-launch time-out (recoverTopTimeout) re-runs the apply it spoiled on the
    // tier launches, and the rest of the solve keeps them
    ScopedFlag restore(forceUnfused), own(ownTimeline);
    ownTimeline = true;  // the look-ahead matvec may be enqueued after a spoiled one: recovered in the driver
    GmresSystem g{L, m, 0.0, false, b, xt, w, V, st};
    g.normb = std::sqrt(sumsq(b));
    // A 0 = 0: a zero initial guess needs no matvec for its residual
    g.xZero = g.normb > 0.0 && sumsq(xt) == 0.0;
    g.matvec = [&](const double* v) {
        blockOpDev(2, v, N, w, N, true, s);
        if (rec) rec->push_back(64);
    };
    if (relax > 0.0) {
        g.relax = relax;
        g.matvecLow = [&](const double* v) {
            blockOpDev(2, v, N, w, N, true, s, NAN, nullptr, 0, nullptr, nullptr, ApplyPrec::F32);
            if (rec) rec->push_back(32);
        };
    }
    g.startCycle = [&] { arnoldiBegin(L, m, V, L, st, nullptr, g.normb, stat, s); };
    g.step = [&](int j) { arnoldiStep(L, m, j, V, L, w, st, stat, s); };
    g.spoiled = [&] { return recoverTopTimeout(s); };
    double relres = 0.0;
    const int its = gmresRestarted(g, hs, tol, maxit, hist, maxhist, &relres, s);
    for (int k = 0; k < ks; ++k)
        k_unpermute<<<nblk(N), 256, 0, s>>>(N, perm, xt + (size_t)k * N, x + (size_t)k * N);
    HIP_CHECK(hipStreamSynchronize(s));
    ownTimeline = false;
    checkDeviceErrors();  // every apply was checked at its recovery point: a flag here is new
    if (relresOut) *relresOut = relres;
    return its;
}

// ---- the block solve across ranks: the small device pieces beside the
// sharded matvec and the DCGS2 sweeps
// dst[r * ldd + i] = src[r * lds + i] for i < len; blockIdx.y = the row r
__global__ void __launch_bounds__(256) k_rows_copy(int64_t len, const double* __restrict__ src, int64_t lds,
                                                   double* __restrict__ dst, int64_t ldd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < len) dst[(size_t)blockIdx.y * ldd + i] = src[(size_t)blockIdx.y * lds + i];
}

// an all-reduce entry that counts the ranks in trouble: `add` plus 1 if this rank's
// sticky device-failure word (err: the fused launch's time-out flag, may be null) is set
__global__ void k_flag_put(const unsigned* __restrict__ err, double add, double* __restrict__ slot) {
    if (threadIdx.x == 0) *slot = add + (err && *(const volatile unsigned*)err != 0 ? 1.0 : 0.0);
}

// n (<= 64) all-reduced words into the mapped status
__global__ void k_words(const double* __restrict__ src, int n, double* __restrict__ dst) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
}

static void rows_copy(int rows, int64_t len, const double* src, int64_t lds, double* dst, int64_t ldd, hipStream_t s) {
    if (rows < 1 || len < 1) return;
    k_rows_copy<<<dim3(nblk(len), (unsigned)rows), 256, 0, s>>>(len, src, lds, dst, ldd);
    HIP_LAUNCH_CHECK();
}

// blockSolveDev's loop (gmresRestarted) on this rank's compact owned vectors (L = ks x
// owned, contiguous rows), every rank of the communicator together.  The matvec is the one-call sharded
// operator: V[j] goes into the own-range columns of the handle's (ks, N) input with one
// strided copy, and the operator writes its owned output straight into w.  A step is
//   project -> k_arn_rows -> all-reduce (j + 1) -> k_arn_coef(P = 1) -> update ->
//   k_arn_rows -> all-reduce (j + 2 sums + the failure flag) -> k_arn_column(P = 1),
// a cycle starts with project(V0, V0) -> all-reduce (|r|^2 + the flag) -> k_arn_begin.
// No rank may take a branch of its own: every decision below reads all-reduced values
// (the status words the begin / column kernels compute from the reduced sums are
// bit-identical on every rank if the all-reduce delivers the same bits to every rank),
// never a local norm.  What one rank alone can refuse -- arguments, cache state, the
// allocations -- is evaluated before the first collective and summed as a flag in it:
// either every rank starts, or every rank returns with no further collective.  A
// device-side time-out is not recovered locally (a restart on the tier launches would
// change one rank's collectives): the flag travels in each step's second all-reduce and
// in each cycle start's, reaches the host with the status word, and ends the call on
// every rank at the same step.
int Operator::blockSolveShardedDev(const double* rhs, int64_t ldr, double* x, int64_t ldx, int restart, double tol,
                                   int maxit, double* hist, int maxhist, double* relresOut, hipStream_t s) {
    refuseHighPlain("aniso_block_solve_sharded_dev");
    if (hoShard) checkBlockLimit(true);  // (ks is the same on every rank, commInitHigh: all return alike, no collective)
    if (!comm) throw std::logic_error("sharded block operator before aniso_comm_init");
    ensureDevice();
    const int64_t N = geo.N, ob = plan.ownBegin, owned = plan.ownEnd - plan.ownBegin, L = (int64_t)ks * owned;
    const int m = restart;
    // the all-reduce buffer first: a rank that refuses still takes part in the opening collective
    {
        const size_t need = (size_t)((restart >= 1 && restart < (1 << 24) ? restart : 1) + 8) * sizeof(double);
        if (dShRed.bytes < need) dShRed.alloc(need);
    }
    double* red = dShRed.as<double>();
    DevBuf bB, bX, bW, bV, bSt;
    StatusBlock hs;
    unsigned* errDev = nullptr;
    // ---- everything that can fail on this rank alone
    std::exception_ptr refused;
    try {
        if (!rhs || !x) throw std::invalid_argument("sharded block solve: rhs or x is NULL");
        if (ldr < owned || ldx < owned) throw std::invalid_argument("sharded block solve: leading dimension below the owned size");
        if (restart < 1 || maxit < 1 || !(tol > 0.0))
            throw std::invalid_argument("block solve needs restart >= 1, maxit >= 1, tol > 0");
        prepareShardedMatvec();
        checkDeviceErrors();
        bB.alloc(L * sizeof(double));
        bX.alloc(L * sizeof(double));
        bW.alloc(L * sizeof(double));
        bV.alloc((size_t)(m + 1) * L * sizeof(double));
        bSt.alloc((size_t)arn::Layout(m).total * sizeof(double));
        if (dShIn.bytes < (size_t)ks * N * sizeof(double)) {
            dShIn.alloc((size_t)ks * N * sizeof(double));
            HIP_CHECK(hipMemsetAsync(dShIn.p, 0, dShIn.bytes, s));  // outside the own range: the exchange's halo
        }
        arnoldiParts(m + 2);
        hs.alloc(4);
        HIP_CHECK(hipHostGetDevicePointer((void**)&errDev, topErr, 0));
    } catch (...) {
        refused = std::current_exception();
    }
    double *b = bB.as<double>(), *xt = bX.as<double>(), *w = bW.as<double>();
    double* V = bV.as<double>();
    double* st = bSt.as<double>();
    double* xin = dShIn.as<double>();
    // ---- the opening all-reduce: {ranks that refuse, |b|^2, |x0|^2}
    HIP_CHECK(hipMemsetAsync(red, 0, 3 * sizeof(double), s));
    k_flag_put<<<1, 64, 0, s>>>(nullptr, refused ? 1.0 : 0.0, red);
    HIP_LAUNCH_CHECK();
    if (!refused) {
        rows_copy(ks, owned, rhs, ldr, b, owned, s);
        rows_copy(ks, owned, x, ldx, xt, owned, s);
        arnoldiProject(L, 0, b, L, b, red + 1, s);
        arnoldiProject(L, 0, xt, L, xt, red + 2, s);
    }
    comm->allreduce(red, 3, s);
    double opening[3] = {0.0, 0.0, 0.0};
    HIP_CHECK(hipMemcpyAsync(opening, red, sizeof(opening), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (refused) std::rethrow_exception(refused);
    if (opening[0] != 0.0)
        throw std::invalid_argument("sharded block solve: another rank refused the call (its own error says why); "
                                    "no rank started and nothing was changed");
    ScopedFlag ownTl(ownTimeline);
    ownTimeline = true;  // the applies' entry checks leave the failure flag to the all-reduces below
    double* const stat = hs.dev;
    GmresSystem g{L, m, std::sqrt(opening[1]), false, b, xt, w, V, st};
    g.xZero = g.normb > 0.0 && opening[2] == 0.0;  // A 0 = 0: no matvec for the first residual
    // w = A v: v (compact) into the own-range columns of the (ks, N) input, the owned output into w
    g.matvec = [&](const double* v) {
        rows_copy(ks, owned, v, owned, xin + ob, N, s);
        blockOpShardedOwned(2, xin, N, w, owned, s);
    };
    // the failure flag behind n reduced sums, all-reduced with them; then the flag's sum
    // beside the status words that `then` stores
    auto reduceFlagged = [&](int n, auto&& then) {
        k_flag_put<<<1, 64, 0, s>>>(errDev, 0.0, red + n);
        HIP_LAUNCH_CHECK();
        comm->allreduce(red, (size_t)n + 1, s);
        then();
        k_words<<<1, 64, 0, s>>>(red + n, 1, stat + 3);
        HIP_LAUNCH_CHECK();
    };
    g.startCycle = [&] {  // |r|^2 summed over the ranks
        arnoldiProject(L, 0, V, L, V, red, s);
        reduceFlagged(1, [&] { arnoldiBegin(L, m, V, L, st, red, g.normb, stat, s); });
    };
    g.step = [&](int j) {  // the library's sweeps (aniso_arnoldi_*), their sums reduced over the ranks
        arnoldiProject(L, j, V, L, w, red, s);
        comm->allreduce(red, (size_t)j + 1, s);
        arnoldiCoef(m, j, st, red, s);
        arnoldiUpdate(L, m, j, V, L, w, st, red, s);
        reduceFlagged(j + 2, [&] { arnoldiColumn(m, j, st, red, stat, s); });
    };
    // the all-reduced failure flag beside the status words: never recovered, see above
    g.spoiled = [&]() -> bool {
        if (hs.p[3] == 0.0) return false;
        HIP_CHECK(hipStreamSynchronize(s));  // (a look-ahead matvec may be in flight; every rank enqueued it)
        *(volatile unsigned*)topErr = 0;
        throw std::runtime_error("sharded block solve: a rank reported a device-side failure (a hand-off time-out of "
                                 "its fused top-of-tree launch); every rank left the solve at the same step and x "
                                 "is unchanged");
    };
    double relres = 0.0;
    const int its = gmresRestarted(g, hs, tol, maxit, hist, maxhist, &relres, s);
    rows_copy(ks, owned, xt, owned, x, ldx, s);
    HIP_CHECK(hipStreamSynchronize(s));
    if (relresOut) *relresOut = relres;
    return its;
}

// ---- the 16-column Arnoldi of arnoldi16.hpp as functions on a caller's buffers: the
// mixed solves below and the development entries aniso_arnoldi16_* run these.  They
// only check and launch: the device and the small kernels' LDS limit are made ready
// once per call by arnoldi16Ready (the entries) or mixedPrepare (the solves), not per step
void Operator::arnoldi16Ready() {
    ensureDevice();
    arn_small_kernel_attrs();
}

void arn16_work_doubles(int m, int64_t* state, int64_t* part) {
    *state = (int64_t)arn16::KC * arn::Layout(m).total;
    *part = (int64_t)arn16::kParts * arn16::KC * (m + 2);
}

static void check_arnoldi16(int64_t n16, int m, int j, int64_t ldv) {
    if (m < 1 || m > arn16::kMaxBasis)
        throw std::invalid_argument("arnoldi16: restart must be in [1, " + std::to_string(arn16::kMaxBasis) + "]");
    if (j < 0 || j >= m) throw std::invalid_argument("arnoldi16: need 0 <= j < m");
    if (n16 < 0 || n16 % arn16::KC != 0 || ldv < n16)
        throw std::invalid_argument("arnoldi16: n16 must be 16 x the points and the row stride at least n16");
}

static arn::ColArgs cols16(int m) {
    arn::ColArgs ca = arn16::kCols;
    ca.sts = arn::Layout(m).total;
    return ca;
}

// cycle start: V[0] = fp32(r - sub) (sub: fp32, may be null), its norm per column against
// scale[c]; status (may be null): per column {|V0_c| / scale_c, |V0_c|, 0, -}
void Operator::arnoldi16Begin(int64_t n16, int m, const double* r, const float* sub, const double* scale, float* V,
                              double* st, double* part, double* status, hipStream_t s) {
    using namespace arn16;
    check_arnoldi16(n16, m, 0, n16);
    if (sub) k16_sub_norm<float><<<kParts, kT, 0, s>>>(n16, r, sub, nullptr, V, part);
    else k16_sub_norm<double><<<kParts, kT, 0, s>>>(n16, r, nullptr, nullptr, V, part);
    HIP_LAUNCH_CHECK();
    arn::k_arn_begin<<<KC, arn::kThreads, 0, s>>>(m, st, part, kParts, 1.0, status, cols16(m), scale);
    HIP_LAUNCH_CHECK();
}

// step j with w = A V[j] (not row j + 1 of V): row j + 1 written; status per column {estimate, r', j + 1, -}
void Operator::arnoldi16Step(int64_t n16, int m, int j, float* V, int64_t ldv, const float* w, double* st,
                             double* part, double* status, hipStream_t s) {
    using namespace arn16;
    check_arnoldi16(n16, m, j, ldv);
    // sweep B writes row j + 1 while it reads w
    const float* vn = V + (size_t)(j + 1) * ldv;
    if (w < vn + n16 && vn < w + n16) throw std::invalid_argument("arnoldi16: w overlaps row j + 1 of V");
    const arn::ColArgs ca = cols16(m);
    launch_project16(n16, j + 1, V, ldv, w, part, s);
    HIP_LAUNCH_CHECK();
    arn::k_arn_coef<<<KC, arn::kThreads, arn::coef_lds(j), s>>>(m, j, st, part, kParts, ca);
    HIP_LAUNCH_CHECK();
    launch_update16(n16, j + 1, V, ldv, w, st, ca.sts, m, part, s);
    HIP_LAUNCH_CHECK();
    arn::k_arn_column<<<KC, arn::kThreads, arn::column_lds(j), s>>>(m, j, st, part, kParts, status, ca);
    HIP_LAUNCH_CHECK();
}

// x += the cycle's correction over its first `used` steps (x: n16 doubles, point-major)
void Operator::arnoldi16Solution(int64_t n16, int m, int used, const float* V, int64_t ldv, double* st, double* x,
                                 hipStream_t s) {
    using namespace arn16;
    check_arnoldi16(n16, m, 0, ldv);
    if (used < 0 || used > m) throw std::invalid_argument("arnoldi16: need 0 <= used <= m");
    if (used == 0 || n16 == 0) return;
    const int64_t sts = arn::Layout(m).total;
    arn::k_arn_solve<<<KC, arn::kThreads, arn::solve_lds(used), s>>>(m, used, st, sts);
    HIP_LAUNCH_CHECK();
    k16_axpy<<<nblk(n16), 256, (size_t)used * KC * sizeof(double), s>>>(n16, used, V, ldv, st, sts, m, x);
    HIP_LAUNCH_CHECK();
}

// Config 5 (main.cpp:121-141 for 16 right-hand sides): A X = B with
// A(u) = u - K_0(sigma_s .* u), fp64 iterative refinement over fp32 inner GMRES(m)
// solves -- the algorithm of aniso_amd.solve.gmres_mixed, every step in the library:
//   outer: R = B - A64 X (the fp64 16-RHS MFMA operator), rel_c = |R_c| / |B_c|; stop
//          when every rel_c <= tol (or after maxOuter refinements); X += inner(R);
//   inner: GMRES(m) per column on an fp32 basis (arnoldi16.hpp: the DCGS2 Arnoldi of
//          the block solve, 16 columns in lockstep), the fp32 16-RHS MFMA operator,
//          to |g_c| <= innerTol |R_c| for every column, at most maxCycles cycles.
// B, X: 16 rows of N doubles (original order, strides ldb / ldx; X is written, the
// initial guess is 0); device pointers, stream s.  Returns the inner steps; *outer the
// refinements; rel: the 16 final relative residuals.
int Operator::solve16Mixed(const double* B, int64_t ldb, double* X, int64_t ldx, int m, double tol, double innerTol,
                           int maxOuter, int maxCycles, int* outerOut, double* rel, hipStream_t s) {
    mixedCheckState("16-RHS solve", "aniso_solve16_mixed_dev");
    mixedCheckArgs("16-RHS solve", arn16::kMaxRows - 1, m, tol, innerTol, maxOuter, maxCycles, ldb, ldx);
    mixedPrepare(m);
    int longest = 0;
    return mixedGroup(B, ldb, X, ldx, arn16::KC, m, tol, innerTol, maxOuter, maxCycles, outerOut, &longest, rel, s);
}

// The same for any number of right-hand sides and any restart up to arn16::kMaxBasis
// (main.cpp:141 runs GMRES(80)): the rows are solved in groups of 16, in order, on the
// work buffers of one group; a short last group is padded with zero columns (a zero
// column's solution is 0 and its relres 0).  *outerOut: the largest refinement count
// of a group; returns the sum of the groups' inner steps; *longest: the most steps any
// inner cycle took; rel: nrhs entries (may be null).  Arguments are checked before the
// handle's state, both before the device is touched.
int Operator::solveMixed(int nrhs, const double* B, int64_t ldb, double* X, int64_t ldx, int m, double tol,
                         double innerTol, int maxOuter, int maxCycles, int* outerOut, int* longest, double* rel,
                         hipStream_t s) {
    if (nrhs < 1) throw std::invalid_argument("mixed solve: nrhs must be at least 1");
    mixedCheckArgs("mixed solve", arn16::kMaxBasis, m, tol, innerTol, maxOuter, maxCycles, ldb, ldx);
    mixedCheckState("mixed solve", "aniso_solve_mixed_dev");
    mixedPrepare(m);
    int outer = 0, inner = 0, longestAll = 0;
    for (int r0 = 0; r0 < nrhs; r0 += arn16::KC) {
        const int rows = std::min(arn16::KC, nrhs - r0);
        int o = 0, lc = 0;
        double rel16[arn16::KC];
        inner += mixedGroup(B + (size_t)r0 * ldb, ldb, X + (size_t)r0 * ldx, ldx, rows, m, tol, innerTol, maxOuter,
                            maxCycles, &o, &lc, rel16, s);
        outer = std::max(outer, o);
        longestAll = std::max(longestAll, lc);
        if (rel) std::copy(rel16, rel16 + rows, rel + r0);
    }
    if (outerOut) *outerOut = outer;
    if (longest) *longest = longestAll;
    return inner;
}

// what one rank's handle must be for the mixed solves, and their arguments (mMax: the
// entry's restart bound); neither touches the device
void Operator::mixedCheckState(const char* what, const char* entry) const {
    const std::string w(what);
    refuseHighOrder(entry);
    if (plan.nranks != 1) throw std::logic_error(w + " on a sharded handle");
    if (!coeffSet) throw std::runtime_error(w + " before setCoeff");
    needResident(0, entry);
    if (!modes[0].resident) throw std::runtime_error(w + " before cache(0)");
}

void Operator::mixedCheckArgs(const char* what, int mMax, int m, double tol, double innerTol, int maxOuter,
                              int maxCycles, int64_t ldb, int64_t ldx) const {
    const std::string w(what);
    if (m < 1 || m > mMax) throw std::invalid_argument(w + ": restart must be in [1, " + std::to_string(mMax) + "]");
    if (!(tol > 0.0) || !(innerTol > 0.0) || maxOuter < 0 || maxCycles < 1)
        throw std::invalid_argument(w + " needs tol, inner_tol > 0, max_outer >= 0, max_cycles >= 1");
    if (ldb < geo.N || ldx < geo.N) throw std::invalid_argument(w + ": leading dimension below N");
}

// the work buffers of one group of 16 columns at restart m, the mapped status block and
// its event: kept on the handle between solves (grown, never shrunk), allocated before
// anything is launched
void Operator::mixedPrepare(int m) {
    using namespace arn16;
    ensureDevice();
    checkDeviceErrors();
    const int64_t n16 = KC * geo.N;
    auto grow = [](DevBuf& b, size_t bytes) {
        if (b.bytes < bytes) b.alloc(bytes);
    };
    const size_t basis = (size_t)(m + 1) * n16 * sizeof(float);
    try {
        grow(s16V, basis);
    } catch (const std::exception& e) {
        throw std::runtime_error("mixed solve: the fp32 Krylov basis of (m + 1) x 16 x N = " + std::to_string(m + 1) +
                                 " x 16 x " + std::to_string(geo.N) + " floats (" + std::to_string(basis) +
                                 " bytes) could not be allocated: " + e.what());
    }
    grow(s16B, n16 * sizeof(double));
    grow(s16X, n16 * sizeof(double));
    grow(s16R, n16 * sizeof(double));
    grow(s16W, n16 * sizeof(double));
    grow(s16D, n16 * sizeof(double));
    grow(s16Df, n16 * sizeof(float));
    grow(s16W32, n16 * sizeof(float));
    int64_t stDoubles = 0, partDoubles = 0;
    arn16_work_doubles(m, &stDoubles, &partDoubles);
    grow(s16St, (size_t)stDoubles * sizeof(double));
    grow(s16Part, (size_t)partDoubles * sizeof(double));
    grow(s16R0, KC * sizeof(double));
    // status words in mapped host memory: per column {relres, r', steps, -}, then 16 sums
    if (!s16Stat)
        HIP_CHECK(hipHostMalloc((void**)&s16Stat, 5 * KC * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    if (!s16Ev) HIP_CHECK(hipEventCreateWithFlags(&s16Ev, hipEventDisableTiming));
    arn_small_kernel_attrs();
}

// one group: `nrows` <= 16 rows of B and X, the columns from nrows on zero (mixedPrepare
// before it).  An exception leaves after the stream has drained: no kernel still writes
// to the handle's buffers when the caller sees the error.
int Operator::mixedGroup(const double* B, int64_t ldb, double* X, int64_t ldx, int nrows, int m, double tol,
                         double innerTol, int maxOuter, int maxCycles, int* outerOut, int* longest, double* rel,
                         hipStream_t s) {
    try {
        return mixedGroupRun(B, ldb, X, ldx, nrows, m, tol, innerTol, maxOuter, maxCycles, outerOut, longest, rel, s);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
}

int Operator::mixedGroupRun(const double* B, int64_t ldb, double* X, int64_t ldx, int nrows, int m, double tol,
                            double innerTol, int maxOuter, int maxCycles, int* outerOut, int* longest, double* rel,
                            hipStream_t s) {
    using namespace arn16;
    const int64_t N = geo.N, n16 = KC * N;
    double *Bt = s16B.as<double>(), *Xt = s16X.as<double>(), *R = s16R.as<double>(), *W = s16W.as<double>();
    double *D = s16D.as<double>(), *st = s16St.as<double>(), *part = s16Part.as<double>(), *r0d = s16R0.as<double>();
    float *Df = s16Df.as<float>(), *W32 = s16W32.as<float>(), *V = s16V.as<float>();
    const int* perm = dPerm.as<int>();
    StatusBlock hs;
    hs.view(s16Stat, s16Ev);
    double* stat = hs.dev;
    double* sums = stat + 4 * KC;
    const double* hsums = hs.p + 4 * KC;
    auto colsums = [&] {  // the one-row partials in `part` -> hsums[c]
        k16_rows<<<KC, arn::kThreads, 0, s>>>(part, sums);
        HIP_LAUNCH_CHECK();
        hs.sync(s);
    };
    const unsigned g16 = nblk(n16);
    k16_gather<<<g16, 256, 0, s>>>(N, perm, B, ldb, nrows, Bt);
    k16_sub_norm<double><<<kParts, kT, 0, s>>>(n16, Bt, nullptr, R, nullptr, part);  // R = B (X = 0)
    HIP_LAUNCH_CHECK();
    HIP_CHECK(hipMemsetAsync(Xt, 0, n16 * sizeof(double), s));
    colsums();
    double bn[KC], rn[KC], r0[KC];
    for (int c = 0; c < KC; ++c) bn[c] = std::sqrt(hsums[c]);
    int outer = 0, inner = 0, longestCycle = 0;
    for (;; ++outer) {
        if (outer > 0) {
            mrhs64Dev(0, true, Xt, W, s);  // W = X - K_0(sigma_s .* X), fp64
            k16_sub_norm<double><<<kParts, kT, 0, s>>>(n16, Bt, W, R, nullptr, part);
            HIP_LAUNCH_CHECK();
            colsums();
        }
        bool all = true;
        for (int c = 0; c < KC; ++c) {
            rn[c] = std::sqrt(hsums[c]);
            rel[c] = bn[c] > 0.0 ? rn[c] / bn[c] : 0.0;
            all = all && rel[c] <= tol;
        }
        if (all || outer == maxOuter) break;
        for (int c = 0; c < KC; ++c) r0[c] = rn[c] > 0.0 ? rn[c] : 1.0;
        HIP_CHECK(hipMemcpyAsync(r0d, r0, KC * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(D, 0, n16 * sizeof(double), s));
        int its = 0;
        for (int cyc = 0; cyc < maxCycles; ++cyc) {
            // the cycle's residual R - A32 D into V[0] (fp32) and its norm per column
            if (its > 0) {
                k16_round<<<g16, 256, 0, s>>>(n16, D, Df);
                forwardF32Dev(Df, W32, s);
            }
            arnoldi16Begin(n16, m, R, its > 0 ? W32 : nullptr, r0d, V, st, part, stat, s);
            hs.sync(s);
            bool done = true;
            for (int c = 0; c < KC; ++c) done = done && hs.p[4 * c] <= innerTol;
            if (done) break;
            int used = 0;
            bool ahead = false;
            LookAhead la;
            for (int j = 0; j < m; ++j) {
                float* vj = V + (size_t)j * n16;
                if (!ahead) forwardF32Dev(vj, W32, s);
                arnoldi16Step(n16, m, j, V, n16, W32, st, part, stat, s);
                hs.post(s);
                // the next step's matvec before the host reads the estimates (as gmresRestarted)
                ahead = j + 1 < m && !la.near(innerTol);
                if (ahead) forwardF32Dev(V + (size_t)(j + 1) * n16, W32, s);
                hs.wait();
                double worst = 0.0;
                for (int c = 0; c < KC; ++c) {
                    if (hs.p[4 * c + 2] != (double)(j + 1))
                        throw std::runtime_error("16-RHS solve: Arnoldi step " + std::to_string(j) + " left no status");
                    worst = std::max(worst, hs.p[4 * c]);
                }
                ++its;
                used = j + 1;
                la.push(worst);
                if (worst <= innerTol) break;
            }
            longestCycle = std::max(longestCycle, used);
            arnoldi16Solution(n16, m, used, V, n16, st, D, s);
        }
        k16_add<<<g16, 256, 0, s>>>(n16, D, Xt);
        HIP_LAUNCH_CHECK();
        inner += its;
    }
    k16_scatter<<<g16, 256, 0, s>>>(N, perm, Xt, X, ldx, nrows);
    HIP_LAUNCH_CHECK();
    HIP_CHECK(hipStreamSynchronize(s));
    checkDeviceErrors();
    if (outerOut) *outerOut = outer;
    if (longest) *longest = longestCycle;
    return inner;
}

// ---- the multi-source forward solve (main.cpp:121-141 for several
// sources): u_k - K_0(sigma_s u_k) = b_k, b_k = K_0 q_k or q_k, on every unsharded handle
// whose mode 0 is ready -- np = 6, 8 and np = 4 lean or resident -- through modeApplyDev.
// Each column is blockSolveDev's restarted GMRES (DCGS2 Arnoldi, arnoldi.hpp) with a
// basis, a state block and a convergence of its own; the columns of a group of
// arn::kNarrowCols (arn::kMaxCols with the wide setting on) run in
// lockstep and share one operator call per step, on exactly the rows still active.

// the GMRES parameters of the lockstep multi-column solves (w: the entry's name)
static void checkColsSolveParams(const std::string& w, int restart, double tol, int maxit) {
    if (restart < 1 || restart > 400)
        throw std::invalid_argument(w + ": restart must be in [1, 400], got " + std::to_string(restart));
    if (!(tol > 0.0)) throw std::invalid_argument(w + ": tol must be > 0");
    if (maxit < 0) throw std::invalid_argument(w + ": maxit must be >= 0, got " + std::to_string(maxit));
}

// everything that can be refused before the device is touched (false: nothing to do)
bool Operator::forwardSolveMultiCheck(const char* what, int nrhs, const void* q, int64_t ldq, const void* x,
                                      int64_t ldx, const int* iters, int restart, double tol, int maxit,
                                      const MixedParams* mixed) const {
    const std::string w(what);
    const int64_t N = geo.N;
    if (nrhs < 0) throw std::invalid_argument(w + ": nrhs must be >= 0, got " + std::to_string(nrhs));
    if (ldq < N) throw std::invalid_argument(w + ": ldq = " + std::to_string(ldq) + " is below N = " + std::to_string(N));
    if (ldx < N) throw std::invalid_argument(w + ": ldx = " + std::to_string(ldx) + " is below N = " + std::to_string(N));
    checkColsSolveParams(w, restart, tol, maxit);
    if (mixed && !(mixed->innerTol > 0.0 && mixed->innerTol < 1.0))
        throw std::invalid_argument(w + ": inner_tol must be in (0, 1)");
    if (mixed && mixed->maxOuter < 1)
        throw std::invalid_argument(w + ": max_outer must be >= 1, got " + std::to_string(mixed->maxOuter));
    if (nrhs > 0 && !q) throw std::invalid_argument(w + ": q is NULL");
    if (nrhs > 0 && !x) throw std::invalid_argument(w + ": x is NULL");
    if (nrhs > 0 && !iters) throw std::invalid_argument(w + ": iters is NULL");
    if (nrhs > 0 && mixed && !mixed->outer) throw std::invalid_argument(w + ": outer is NULL");
    if (nrhs == 0) return false;
    const char* qb = static_cast<const char*>(q);
    const char* xb = static_cast<const char*>(x);
    const size_t qs = ((size_t)(nrhs - 1) * ldq + N) * sizeof(double), xs = ((size_t)(nrhs - 1) * ldx + N) * sizeof(double);
    if (qb < xb + xs && xb < qb + qs) throw std::invalid_argument(w + ": q and x overlap");
    // the handle's state, as aniso_forward_multi_dev (mixed: as aniso_forward_multi_f32_dev)
    return modeApplyCheck(what, 0, nrhs, q, ldq, x, ldx, false, mixed != nullptr);
}

int Operator::forwardSolveMultiDev(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x, int64_t ldx,
                                   int restart, double tol, int maxit, int* iters, double* relres, double* hist,
                                   int maxhist, hipStream_t s) {
    if (!forwardSolveMultiCheck("aniso_forward_solve_multi_dev", nrhs, q, ldq, x, ldx, iters, restart, tol, maxit))
        return 0;
    return forwardSolveMultiRun(nrhs, q, ldq, rhsIsSource, x, ldx, restart, tol, maxit, 0.0, iters, relres, hist, maxhist,
                                nullptr, s);
}

// forwardSolveMultiDev's body (the arguments checked); relax > 0: the relaxed rule of
// DESIGN.md §3.18.10 with mode 0's f32 pass as the low operator (chunks of 8 whatever the
// group size), every call recorded in rec
int Operator::forwardSolveMultiRun(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x, int64_t ldx,
                                   int restart, double tol, int maxit, double relax, int* iters, double* relres,
                                   double* hist, int maxhist, std::vector<std::pair<int, int>>* rec, hipStream_t s) {
    ensureDevice();
    checkDeviceErrors();
    // the group size: 16 with the wide setting on (a step's live columns are one operator
    // call: one wide chunk while more than 8 are live)
    const int G = wideOn ? arn::kMaxCols : arn::kNarrowCols;
    const int64_t N = geo.N;
    const int m = restart, gmax = std::min(nrhs, G);
    const std::string g = std::to_string(gmax);
    const std::string tail =
        gmax > arn::kNarrowCols ? "work buffers (aniso_set_wide(h, 0) halves both: groups of 8)" : "work buffers";
    ColsWork cw;
    cw.alloc(N, G, gmax, m, false,
             "forward solve: the Krylov bases of (restart + 1) x " + g + " x N = " + std::to_string(m + 1) + " x " + g +
                 " x " + std::to_string(N),
             tail.c_str());
    if (relax > 0.0) cacheF32();  // the float mirrors, if this is their first use: before anything is launched
    arn_small_kernel_attrs();
    solveCalls.clear();
    const double* sigS = sigmaSTree();
    // the shared loop over mode 0's x - K_0(sigma_s x)
    ColsSolve cs{N, "forward solve",
                 [&](int nrows, const double* in, double* w) { modeApplyDev(0, nrows, in, N, sigS, true, w, N, s); }};
    if (relax > 0.0) {
        cs.Alow = [&](int nrows, const double* in, double* w) {
            modeApplyDev(0, nrows, in, N, sigS, true, w, N, s, false, ApplyPrec::F32);
        };
        cs.relax = relax;
    }
    cs.rec = rec;
    int steps = 0;
    try {
        for (int r0 = 0; r0 < nrhs; r0 += G) {
            const int ng = std::min(G, nrhs - r0);
            const double* qg = q + (size_t)r0 * ldq;
            // the group's right-hand sides
            if (rhsIsSource) modeApplyDev(0, ng, qg, ldq, nullptr, false, cw.B.as<double>(), N, s);
            else
                HIP_CHECK(hipMemcpy2DAsync(cw.B.p, N * sizeof(double), qg, ldq * sizeof(double), N * sizeof(double), ng,
                                           hipMemcpyDeviceToDevice, s));
            steps += colsSolveGroup(cs, cw, ng, x + (size_t)r0 * ldx, ldx, m, tol, maxit, iters + r0,
                                    relres ? relres + r0 : nullptr, hist ? hist + (size_t)r0 * maxhist : nullptr,
                                    hist ? maxhist : 0, s);
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);  // no kernel still writes the buffers freed here
        throw;
    }
    return steps;
}

// one group's buffers at row length L (ColsWork, gmres_driver.hpp)
void ColsWork::alloc(int64_t L, int group, int gmax, int m, bool ownX, const std::string& head, const char* tail,
                     const std::function<void()>& more) {
    if (group < 1 || group > arn::kMaxCols || gmax > group)
        throw std::logic_error("a solve group of " + std::to_string(gmax) + " of " + std::to_string(group) + " columns");
    const int64_t sts = arn::Layout(m).total, pc = (int64_t)(m + 2) * arn::kParts;
    const size_t row = (size_t)gmax * L * sizeof(double), basis = (size_t)(m + 1) * row;
    const size_t rest = (size_t)((ownX ? 4 : 3) * L + sts + pc + 1) * gmax * sizeof(double);
    try {
        V.alloc(basis);
        B.alloc(row);
        In.alloc(row);
        W.alloc(row);
        if (ownX) X.alloc(row);
        st.alloc((size_t)gmax * sts * sizeof(double));
        part.alloc((size_t)gmax * pc * sizeof(double));
        dNb.alloc((size_t)gmax * sizeof(double));
        if (more) more();
    } catch (const std::exception& e) {
        throw std::runtime_error(head + " doubles (" + std::to_string(basis) + " bytes) and " + std::to_string(rest) +
                                 " bytes of " + tail + " could not be allocated: " + e.what());
    }
    hs.alloc(6 * group);
    G = group;
}

// The lockstep loop of one group (ColsSolve) on the buffers cw: every column a restarted
// GMRES of its own on vectors of cs.L doubles; cw.B holds the right-hand sides.
int Operator::colsSolveGroup(const ColsSolve& cs, ColsWork& cw, int ng, double* x, int64_t ldx, int m, double tol,
                             int maxit, int* iters, double* relres, double* hist, int maxhist, hipStream_t s) {
    const int G = cw.G;  // the group size: the status block's stride
    if (ng > G)
        throw std::logic_error(std::string(cs.what) + ": " + std::to_string(ng) + " columns in a group of " +
                               std::to_string(G));
    const int64_t N = cs.L;  // the row length
    const std::string what(cs.what);
    const arn::Layout lay(m);
    const int64_t sts = lay.total, pc = (int64_t)(m + 2) * arn::kParts, vc = (int64_t)(m + 1) * N;
    const arn::ColArgs ca{sts, pc, arn::kParts, 4};
    const unsigned nb = nblk(N);
    double *V = cw.V.as<double>(), *B = cw.B.as<double>(), *In = cw.In.as<double>(), *W = cw.W.as<double>();
    double *st = cw.st.as<double>(), *part = cw.part.as<double>(), *dNb = cw.dNb.as<double>();
    double *hstat = cw.hs.p, *stat = cw.hs.dev;
    struct Col {
        int total = 0, used = 0, nh = 0;
        bool done = false, conv = false, frozen = false, xzero = false;
        double normb = 0.0, rel = 0.0, r = 0.0;
        double est = 0.0;  // the latest relative-residual estimate: the cycle's explicit relres, then each step's
    } col[arn::kMaxCols];
    auto slot = [&](int c) {
        arn::ColSlot sl{};
        sl.V = V + (size_t)c * vc;
        sl.b = B + (size_t)c * N;
        sl.part = part + (size_t)c * pc;
        sl.st = st + (size_t)c * sts;
        sl.x = x + (size_t)c * ldx;
        sl.w = sl.x;
        return sl;
    };
    // f(c0, len) over the maximal runs of consecutive columns in `cols` (ascending): the
    // small kernels address a launch's columns by a stride
    auto runs = [&](const std::vector<int>& cols, auto&& f) {
        for (size_t i = 0; i < cols.size();) {
            size_t k = i + 1;
            while (k < cols.size() && cols[k] == cols[k - 1] + 1) ++k;
            f(cols[i], (int)(k - i));
            i = k;
        }
    };
    // A on the rows `src` of table t (nrows of them), W's compact rows out: one operator call
    // (low: on the relaxed rule's f32 operator)
    auto op = [&](const arn::ColTable& t, int nrows, int row, int64_t ldv, bool low) {
        arn::k_arn_gather_cols<<<dim3(nb, nrows), arn::kThreads, 0, s>>>(N, row, ldv, t, In);
        HIP_LAUNCH_CHECK();
        (low ? cs.Alow : cs.A)(nrows, In, W);
        solveCalls.push_back(nrows);
        if (cs.rec) cs.rec->emplace_back(low ? 32 : 64, nrows);
    };
    const bool relaxed = cs.Alow && cs.relax > 0.0;
    {  // |b|^2 and |x|^2 per column
        arn::ColTable tb{}, tx{};
        for (int c = 0; c < ng; ++c) {
            tb.c[c] = slot(c);
            tb.c[c].V = B + (size_t)c * N;
            tb.c[c].w = tb.c[c].V;
            tx.c[c] = slot(c);
            tx.c[c].V = tx.c[c].x;
        }
        arn::launch_project_cols(N, 1, N, tb, ng, s);
        arn::k_arn_sums_cols<<<ng, arn::kThreads, 0, s>>>(tb, stat + 4 * G);
        arn::launch_project_cols(N, 1, N, tx, ng, s);
        arn::k_arn_sums_cols<<<ng, arn::kThreads, 0, s>>>(tx, stat + 5 * G);
        HIP_LAUNCH_CHECK();
        cw.hs.sync(s);
    }
    double normbs[arn::kMaxCols] = {};
    for (int c = 0; c < ng; ++c) {
        Col& k = col[c];
        k.normb = std::sqrt(hstat[4 * G + c]);
        k.xzero = hstat[5 * G + c] == 0.0;  // A 0 = 0: no operator row for its first residual
        normbs[c] = k.normb > 0.0 ? k.normb : 1.0;
        if (!(k.normb > 0.0)) {  // b = 0: x = 0
            HIP_CHECK(hipMemsetAsync(x + (size_t)c * ldx, 0, N * sizeof(double), s));
            k.done = k.conv = true;
        }
    }
    HIP_CHECK(hipMemcpyAsync(dNb, normbs, ng * sizeof(double), hipMemcpyHostToDevice, s));
    // r = b - A x into V[0] of the columns `cols`, and their cycle's start
    auto residual = [&](const std::vector<int>& cols) {
        if (cols.empty()) return;
        arn::ColTable t{}, tg{};
        int nop = 0;
        for (size_t a = 0; a < cols.size(); ++a) {
            const int c = cols[a];
            t.c[a] = slot(c);
            if (!col[c].xzero) {
                tg.c[nop] = t.c[a];
                tg.c[nop].V = t.c[a].x;
                t.c[a].w = W + (size_t)nop * N;
                ++nop;
            }  // else w = x = 0: r = b
            hstat[4 * c + 2] = -1.0;
        }
        if (nop > 0) op(tg, nop, 0, 0, false);  // every residual is fp64
        arn::k_arn_resid_cols<<<dim3(nb, (unsigned)cols.size()), arn::kThreads, 0, s>>>(N, t);
        HIP_LAUNCH_CHECK();
        for (size_t a = 0; a < cols.size(); ++a) t.c[a].w = t.c[a].V;
        arn::launch_project_cols(N, 1, N, t, (int)cols.size(), s);
        runs(cols, [&](int c0, int len) {
            arn::k_arn_begin<<<len, arn::kThreads, 0, s>>>(m, st + (size_t)c0 * sts, part + (size_t)c0 * pc, arn::kParts,
                                                           1.0, stat + 4 * c0, ca, dNb + c0);
        });
        HIP_LAUNCH_CHECK();
        cw.hs.sync(s);
        for (int c : cols) {
            if (hstat[4 * c + 2] != 0.0) throw std::runtime_error(what + ": a cycle's start left no status");
            col[c].rel = hstat[4 * c];
            col[c].r = hstat[4 * c + 1];
            col[c].conv = col[c].rel <= tol;
            col[c].est = col[c].rel;
        }
    };
    std::vector<int> act, live;
    for (int c = 0; c < ng; ++c)
        if (!col[c].done) act.push_back(c);
    residual(act);
    for (int cyc = 0; cyc < maxit; ++cyc) {
        act.clear();
        for (int c = 0; c < ng; ++c)
            if (!col[c].done && !col[c].conv && col[c].r != 0.0) act.push_back(c);
        if (act.empty()) break;
        for (int c : act) {
            col[c].used = 0;
            col[c].frozen = false;
        }
        for (int j = 0; j < m; ++j) {
            live.clear();
            for (int c : act)
                if (!col[c].frozen) live.push_back(c);
            if (live.empty()) break;
            const int nl = (int)live.size();
            arn::ColTable t{};
            for (int a = 0; a < nl; ++a) {
                t.c[a] = slot(live[a]);
                t.c[a].w = W + (size_t)a * N;
                hstat[4 * live[a] + 2] = -1.0;
            }
            // the relaxed rule, per group: f32 iff every live column's latest estimate is <= relax
            bool low = relaxed;
            for (int a = 0; low && a < nl; ++a) low = col[live[a]].est <= cs.relax;
            op(t, nl, j, N, low);
            arn::launch_project_cols(N, j + 1, N, t, nl, s);
            runs(live, [&](int c0, int len) {
                arn::k_arn_coef<<<len, arn::kThreads, arn::coef_lds(j), s>>>(m, j, st + (size_t)c0 * sts,
                                                                              part + (size_t)c0 * pc, arn::kParts, ca);
            });
            HIP_LAUNCH_CHECK();
            arn::launch_update_cols(N, j + 1, N, m, t, nl, s);
            runs(live, [&](int c0, int len) {
                arn::k_arn_column<<<len, arn::kThreads, arn::column_lds(j), s>>>(
                    m, j, st + (size_t)c0 * sts, part + (size_t)c0 * pc, arn::kParts, stat + 4 * c0, ca);
            });
            HIP_LAUNCH_CHECK();
            cw.hs.sync(s);
            for (int c : live) {
                Col& k = col[c];
                if (hstat[4 * c + 2] != (double)(j + 1))
                    throw std::runtime_error(what + ": Arnoldi step " + std::to_string(j) + " left no status");
                const double rel = hstat[4 * c], rnext = hstat[4 * c + 1];
                ++k.total;
                k.used = j + 1;
                k.est = rel;
                if (hist && k.nh < maxhist) hist[(size_t)c * maxhist + k.nh++] = rel;
                k.frozen = rel <= tol || rnext == 0.0;  // converged (estimate) or lucky breakdown
            }
        }
        // x += P T R^-1 g, every column with its own row count
        arn::ColTable tu{};
        int nu = 0, maxUsed = 0;
        for (int c : act)
            if (col[c].used > 0) {
                arn::k_arn_solve<<<1, arn::kThreads, arn::solve_lds(col[c].used), s>>>(m, col[c].used,
                                                                                        st + (size_t)c * sts);
                tu.c[nu] = slot(c);
                tu.c[nu].used = col[c].used;
                maxUsed = std::max(maxUsed, col[c].used);
                col[c].xzero = false;
                ++nu;
            }
        HIP_LAUNCH_CHECK();
        if (nu > 0) {
            arn::k_arn_axpy_cols<<<dim3(nb, nu), arn::kThreads, (size_t)maxUsed * sizeof(double), s>>>(N, N, m, tu);
            HIP_LAUNCH_CHECK();
        }
        residual(act);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    checkDeviceErrors();
    int steps = 0;
    for (int c = 0; c < ng; ++c) {
        const Col& k = col[c];
        iters[c] = k.conv ? k.total : -std::max(k.total, 1);
        if (relres) relres[c] = k.rel;
        steps += k.total;
    }
    return steps;
}

// N x k column-major host arrays: one staging copy each way
int Operator::forwardSolveMultiHost(const double* Q, int k, bool rhsIsSource, double* X, int restart, double tol,
                                    int maxit, int* iters, double* relres) {
    if (!forwardSolveMultiCheck("aniso_forward_solve_multi", k, Q, geo.N, X, geo.N, iters, restart, tol, maxit)) return 0;
    ensureDevice();
    const size_t bytes = (size_t)k * geo.N * sizeof(double);
    DevBuf dq, dx;
    dq.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(dq.p, Q, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, X, bytes, hipMemcpyHostToDevice, own));
    const int steps = forwardSolveMultiDev(k, dq.as<double>(), geo.N, rhsIsSource, dx.as<double>(), geo.N, restart, tol,
                                           maxit, iters, relres, nullptr, 0, own);
    HIP_CHECK(hipMemcpyAsync(X, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return steps;
}

// ---- the multi-source forward solve in mixed precision: high-order
// handles.  Per group of arn::kNarrowCols columns an fp64 refinement loop around colsSolveGroup
// over the f32 operator: the Krylov vectors stay double, only the operator is inexact.
//   r = b - A x (fp64; a zero guess costs no pass); until every column is done:
//     a column is converged at |r| <= tol |b| (what confirms a column of the fp64 solve);
//     d from A~ d = r / |r| (zero guess, innerTol, restart, maxit cycles; an inner solve
//     that stops short still contributes its d); x += |r| d; one fp64 pass over exactly the
//     active columns for the new residuals.
// A column stops when it has converged, at maxOuter, or when a refinement does not reduce
// its fp64 residual (the previous iterate is put back).
int Operator::forwardSolveMultiMixedDev(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x,
                                        int64_t ldx, int restart, double tol, double innerTol, int maxit,
                                        int maxOuter, int* iters, int* outer, double* relres, hipStream_t s) {
    const MixedParams mp{innerTol, maxOuter, outer};
    if (!forwardSolveMultiCheck("aniso_forward_solve_multi_mixed_dev", nrhs, q, ldq, x, ldx, iters, restart, tol, maxit,
                                &mp))
        return 0;
    ensureDevice();
    checkDeviceErrors();
    constexpr int G = arn::kNarrowCols;  // (the f32 operator has no wide chunk: groups of 8 whatever the setting)
    const int64_t N = geo.N;
    const int m = restart, gmax = std::min(nrhs, G);
    const std::string g = std::to_string(gmax);
    const size_t row = (size_t)gmax * N * sizeof(double);
    const unsigned nbp = std::min(nblk(N), 1024u);  // partial sums per norm
    ColsWork cw;
    DevBuf Bt, R, D, Xp, dPart, dNrm;  // the true right-hand sides, residuals, corrections, previous iterates
    cw.alloc(N, G, gmax, m, false,
             "mixed forward solve: the Krylov bases of (restart + 1) x " + g + " x N = " + std::to_string(m + 1) +
                 " x " + g + " x " + std::to_string(N),
             ("work buffers and 4 x " + std::to_string(row) + " bytes of refinement vectors").c_str(), [&] {
                 Bt.alloc(row);
                 R.alloc(row);
                 D.alloc(row);
                 Xp.alloc(row);
                 dPart.alloc((size_t)nbp * sizeof(double));
                 dNrm.alloc(G * sizeof(double));
             });
    cacheF32();  // the float mirrors, if this is their first use: before anything is launched
    arn_small_kernel_attrs();
    solveCalls.clear();
    mixedCalls.clear();
    const double* sigS = sigmaSTree();
    double *bt = Bt.as<double>(), *r = R.as<double>(), *d = D.as<double>(), *xp = Xp.as<double>();
    double *W = cw.W.as<double>(), *In = cw.In.as<double>(), *Bn = cw.B.as<double>(), *nrm = dNrm.as<double>();
    const size_t rb = (size_t)N * sizeof(double);
    const ColsSolve cs{N, "mixed forward solve", [&](int nrows, const double* in, double* w) {
                           modeApplyDev(0, nrows, in, N, sigS, true, w, N, s, false, ApplyPrec::F32);
                           mixedCalls.push_back({32, nrows});
                       }};
    // |v_a|^2 of n vectors (fixed-order sums) to the host
    double hn[G];
    auto norms2 = [&](int n, auto&& vec) {
        for (int a = 0; a < n; ++a) {
            const double* v = vec(a);
            k_dot_partial<<<nbp, 256, 0, s>>>(N, v, v, dPart.as<double>());
            k_dot_final<<<1, 256, 0, s>>>((int)nbp, dPart.as<double>(), nrm + a);
        }
        HIP_LAUNCH_CHECK();
        HIP_CHECK(hipMemcpyAsync(hn, nrm, n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    };
    // W[a] = A x[cols[a]] in fp64: one pass over exactly these columns
    auto pass64 = [&](const std::vector<int>& cols, double* xg, int64_t ld) {
        for (size_t a = 0; a < cols.size(); ++a)
            HIP_CHECK(hipMemcpyAsync(In + a * N, xg + (size_t)cols[a] * ld, rb, hipMemcpyDeviceToDevice, s));
        modeApplyDev(0, (int)cols.size(), In, N, sigS, true, W, N, s);
        mixedCalls.push_back({64, (int)cols.size()});
    };
    int steps = 0;
    try {
        for (int r0 = 0; r0 < nrhs; r0 += G) {
            const int ng = std::min(G, nrhs - r0);
            const double* qg = q + (size_t)r0 * ldq;
            double* xg = x + (size_t)r0 * ldx;
            if (rhsIsSource) {
                modeApplyDev(0, ng, qg, ldq, nullptr, false, bt, N, s);
                mixedCalls.push_back({64, ng});
            } else {
                HIP_CHECK(hipMemcpy2DAsync(bt, rb, qg, ldq * sizeof(double), rb, ng, hipMemcpyDeviceToDevice, s));
            }
            struct Col {
                int total = 0, outer = 0;
                bool done = false, conv = false;
                double normb = 0.0, rel = 0.0, nr = 0.0;
            } col[G];
            norms2(ng, [&](int c) { return bt + (size_t)c * N; });
            for (int c = 0; c < ng; ++c) col[c].normb = std::sqrt(hn[c]);
            norms2(ng, [&](int c) { return xg + (size_t)c * ldx; });
            std::vector<int> act, first;
            for (int c = 0; c < ng; ++c) {
                if (!(col[c].normb > 0.0)) {  // b = 0: x = 0
                    HIP_CHECK(hipMemsetAsync(xg + (size_t)c * ldx, 0, rb, s));
                    col[c].done = col[c].conv = true;
                    continue;
                }
                act.push_back(c);
                if (hn[c] != 0.0) first.push_back(c);  // A 0 = 0: a zero guess costs no pass
                else HIP_CHECK(hipMemcpyAsync(r + (size_t)c * N, bt + (size_t)c * N, rb, hipMemcpyDeviceToDevice, s));
            }
            if (!first.empty()) {
                pass64(first, xg, ldx);
                for (size_t a = 0; a < first.size(); ++a)
                    k_sub<<<nblk(N), 256, 0, s>>>(N, bt + (size_t)first[a] * N, W + a * N, r + (size_t)first[a] * N);
                HIP_LAUNCH_CHECK();
            }
            norms2((int)act.size(), [&](int a) { return r + (size_t)act[a] * N; });
            for (size_t a = 0; a < act.size(); ++a) {
                Col& k = col[act[a]];
                k.nr = std::sqrt(hn[a]);
                k.rel = k.nr / k.normb;
            }
            for (;;) {
                act.clear();
                for (int c = 0; c < ng; ++c) {
                    Col& k = col[c];
                    if (k.done) continue;
                    k.conv = k.rel <= tol;
                    if (k.conv || k.outer >= maxOuter) k.done = true;
                    else act.push_back(c);
                }
                if (act.empty()) break;
                const int na = (int)act.size();
                // the residuals at unit norm: the fp32 staging never sees their scale
                for (int a = 0; a < na; ++a)
                    k_scale<<<nblk(N), 256, 0, s>>>(N, 1.0 / col[act[a]].nr, r + (size_t)act[a] * N, Bn + (size_t)a * N);
                HIP_LAUNCH_CHECK();
                HIP_CHECK(hipMemsetAsync(d, 0, (size_t)na * rb, s));
                int it[G];
                colsSolveGroup(cs, cw, na, d, N, m, innerTol, maxit, it, nullptr, nullptr, 0, s);
                for (int a = 0; a < na; ++a) {
                    const int c = act[a];
                    col[c].total += maxit == 0 ? 0 : std::abs(it[a]);
                    ++col[c].outer;
                    HIP_CHECK(hipMemcpyAsync(xp + (size_t)c * N, xg + (size_t)c * ldx, rb, hipMemcpyDeviceToDevice, s));
                    k_axpby<<<nblk(N), 256, 0, s>>>(N, col[c].nr, d + (size_t)a * N, 1.0, xg + (size_t)c * ldx);
                }
                HIP_LAUNCH_CHECK();
                pass64(act, xg, ldx);
                for (int a = 0; a < na; ++a)
                    k_sub<<<nblk(N), 256, 0, s>>>(N, bt + (size_t)act[a] * N, W + (size_t)a * N, d + (size_t)a * N);
                HIP_LAUNCH_CHECK();
                norms2(na, [&](int a) { return d + (size_t)a * N; });  // (the corrections are spent: d holds b - A x)
                for (int a = 0; a < na; ++a) {
                    const int c = act[a];
                    Col& k = col[c];
                    const double nr = std::sqrt(hn[a]);
                    if (nr < k.nr) {
                        k.nr = nr;
                        k.rel = nr / k.normb;
                        HIP_CHECK(hipMemcpyAsync(r + (size_t)c * N, d + (size_t)a * N, rb, hipMemcpyDeviceToDevice, s));
                    } else {  // no reduction: the previous iterate is kept and the column stops
                        HIP_CHECK(hipMemcpyAsync(xg + (size_t)c * ldx, xp + (size_t)c * N, rb, hipMemcpyDeviceToDevice, s));
                        k.done = true;
                    }
                }
            }
            HIP_CHECK(hipStreamSynchronize(s));
            checkDeviceErrors();
            for (int c = 0; c < ng; ++c) {
                const Col& k = col[c];
                iters[r0 + c] = k.conv ? k.total : -std::max(k.total, 1);
                outer[r0 + c] = k.outer;
                if (relres) relres[r0 + c] = k.rel;
                steps += k.total;
            }
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);  // no kernel still writes the buffers freed here
        throw;
    }
    return steps;
}

// N x k column-major host arrays: one staging copy each way
int Operator::forwardSolveMultiMixedHost(const double* Q, int k, bool rhsIsSource, double* X, int restart, double tol,
                                         double innerTol, int maxit, int maxOuter, int* iters, int* outer,
                                         double* relres) {
    const MixedParams mp{innerTol, maxOuter, outer};
    if (!forwardSolveMultiCheck("aniso_forward_solve_multi_mixed", k, Q, geo.N, X, geo.N, iters, restart, tol, maxit, &mp))
        return 0;
    ensureDevice();
    const size_t bytes = (size_t)k * geo.N * sizeof(double);
    DevBuf dq, dx;
    dq.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(dq.p, Q, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, X, bytes, hipMemcpyHostToDevice, own));
    const int steps = forwardSolveMultiMixedDev(k, dq.as<double>(), geo.N, rhsIsSource, dx.as<double>(), geo.N, restart,
                                                tol, innerTol, maxit, maxOuter, iters, outer, relres, own);
    HIP_CHECK(hipMemcpyAsync(X, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return steps;
}

// ---- the block solve for several sources (aniso.m:159-173 per source):
// forwardSolveMultiDev's scheme on vectors of ks * N doubles, groups of kBlockGroup sources
// sharing one blockOpMultiDev(2, ...) per step on the sources still active.

constexpr int kBlockGroup = 4;  // sources per group: one chunk of blockOpMultiDev

bool Operator::blockSolveMultiCheck(const char* what, int nsrc, const void* q, int64_t ldq, const void* x, int64_t ldx,
                                    const int* iters, int restart, double tol, int maxit) const {
    checkColsSolveParams(what, restart, tol, maxit);
    if (nsrc > 0 && !iters) throw std::invalid_argument(std::string(what) + ": iters is NULL");
    return blockOpMultiCheck(what, 2, nsrc, q, ldq, x, ldx);  // the rows, their overlap and the handle's state
}

int Operator::blockSolveMultiDev(int nsrc, const double* q, int64_t ldq, bool rhsIsCharge, double* x, int64_t ldx,
                                 int restart, double tol, int maxit, int* iters, double* relres, double* hist,
                                 int maxhist, hipStream_t s) {
    if (!blockSolveMultiCheck("aniso_block_solve_multi_dev", nsrc, q, ldq, x, ldx, iters, restart, tol, maxit)) return 0;
    return blockSolveMultiRun("multi-source block solve", nsrc, q, ldq, rhsIsCharge, x, ldx, restart, tol, maxit, 0.0,
                              iters, relres, hist, maxhist, nullptr, s);
}

// blockSolveMultiDev's body (the arguments checked); relax > 0: the relaxed rule of DESIGN.md
// §3.18.10 with blockOpMultiF32Dev(2, ...) as the low operator, every call recorded in rec
int Operator::blockSolveMultiRun(const char* what, int nsrc, const double* q, int64_t ldq, bool rhsIsCharge, double* x,
                                 int64_t ldx, int restart, double tol, int maxit, double relax, int* iters,
                                 double* relres, double* hist, int maxhist, std::vector<std::pair<int, int>>* rec,
                                 hipStream_t s) {
    ensureDevice();
    checkDeviceErrors();
    constexpr int G = arn::kNarrowCols;
    static_assert(kBlockGroup <= G, "a group fits the column tables");
    const int64_t N = geo.N, L = (int64_t)ks * N;
    const int m = restart, gmax = std::min(nsrc, kBlockGroup);
    const std::string g = std::to_string(gmax);
    ColsWork cw;  // X: the group's guesses as compact vectors
    cw.alloc(L, G, gmax, m, true,
             std::string(what) + ": the Krylov bases of (restart + 1) x " + g + " x ks x N = " +
                 std::to_string(m + 1) + " x " + g + " x " + std::to_string(ks) + " x " + std::to_string(N),
             "work rows", [&] {
                 if (highOrder() && ks <= kMaxRhs) blockMultiReserve(gmax == 3 ? 4 : gmax);
             });
    DevBuf &bB = cw.B, &bX = cw.X;
    if (relax > 0.0) cacheF32();  // the float mirrors, if this is their first use: before anything is launched
    arn_small_kernel_attrs();
    solveCalls.clear();
    ColsSolve cs{L, what, [&](int nrows, const double* in, double* w) { blockOpMultiDev(2, nrows, in, N, w, N, s); }};
    if (relax > 0.0) {
        cs.Alow = [&](int nrows, const double* in, double* w) { blockOpMultiF32Dev(2, nrows, in, N, w, N, s); };
        cs.relax = relax;
    }
    cs.rec = rec;
    int steps = 0;
    try {
        for (int r0 = 0; r0 < nsrc; r0 += kBlockGroup) {
            const int ng = std::min(kBlockGroup, nsrc - r0);
            const double* qg = q + (size_t)r0 * ks * ldq;
            double* xg = x + (size_t)r0 * ks * ldx;
            // the group's guesses as compact vectors, its right-hand sides (aniso.m:160)
            HIP_CHECK(hipMemcpy2DAsync(bX.p, N * sizeof(double), xg, ldx * sizeof(double), N * sizeof(double),
                                       (size_t)ng * ks, hipMemcpyDeviceToDevice, s));
            if (rhsIsCharge) {
                blockOpMultiDev(0, ng, qg, ldq, bB.as<double>(), N, s);
                solveCalls.push_back(ng);
                if (rec) rec->emplace_back(64, ng);
            } else {
                HIP_CHECK(hipMemcpy2DAsync(bB.p, N * sizeof(double), qg, ldq * sizeof(double), N * sizeof(double),
                                           (size_t)ng * ks, hipMemcpyDeviceToDevice, s));
            }
            steps += colsSolveGroup(cs, cw, ng, bX.as<double>(), L, m, tol, maxit, iters + r0,
                                    relres ? relres + r0 : nullptr, hist ? hist + (size_t)r0 * maxhist : nullptr,
                                    hist ? maxhist : 0, s);
            HIP_CHECK(hipMemcpy2DAsync(xg, ldx * sizeof(double), bX.p, N * sizeof(double), N * sizeof(double),
                                       (size_t)ng * ks, hipMemcpyDeviceToDevice, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));  // the buffers are freed on return
    } catch (...) {
        (void)hipStreamSynchronize(s);  // no kernel still writes the buffers freed here
        throw;
    }
    return steps;
}

// (ks N) x nsrc column-major host arrays: one staging copy each way
int Operator::blockSolveMultiHost(const double* Q, int nsrc, bool rhsIsCharge, double* X, int restart, double tol,
                                  int maxit, int* iters, double* relres) {
    if (!blockSolveMultiCheck("aniso_block_solve_multi", nsrc, Q, geo.N, X, geo.N, iters, restart, tol, maxit)) return 0;
    ensureDevice();
    const size_t bytes = (size_t)nsrc * ks * geo.N * sizeof(double);
    DevBuf dq, dx;
    dq.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(dq.p, Q, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, X, bytes, hipMemcpyHostToDevice, own));
    const int steps = blockSolveMultiDev(nsrc, dq.as<double>(), geo.N, rhsIsCharge, dx.as<double>(), geo.N, restart, tol,
                                         maxit, iters, relres, nullptr, 0, own);
    HIP_CHECK(hipMemcpyAsync(X, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return steps;
}

// ---- the relaxed multi-source solves ----

// What the handle itself rules out (np = 4, a shard; the block solve: ks > 8), then NaN: before
// the arguments, the state and the device.  Returns the relax in force (< 0: the default).
double Operator::multiRelaxedEnter(const char* what, bool block, double tol, double relax) const {
    if (block) {
        blockOpF32Refuse(what);
    } else {
        if (!highOrder())
            throw std::logic_error(std::string(what) + ": the f32 mode operator is built for np = 6, 8; the "
                                                       "reduced-precision route of an np = 4 handle is aniso_solve_mixed_dev");
        refuseHoShard(what);
        if (plan.nranks > 1) throw std::logic_error(std::string(what) + " on a sharded handle (use an unsharded handle)");
    }
    if (std::isnan(relax)) throw std::invalid_argument(std::string(what) + ": relax is NaN");
    return relax < 0.0 ? kRelaxFactor * tol : relax;
}

int Operator::blockSolveMultiRelaxedDev(int nsrc, const double* q, int64_t ldq, bool rhsIsCharge, double* x,
                                        int64_t ldx, int restart, double tol, int maxit, double relax, int* iters,
                                        double* relres, double* hist, int maxhist, hipStream_t s) {
    const char* const what = "aniso_block_solve_multi_relaxed_dev";
    relax = multiRelaxedEnter(what, true, tol, relax);
    multiCalls.clear();
    if (!blockSolveMultiCheck(what, nsrc, q, ldq, x, ldx, iters, restart, tol, maxit)) return 0;
    blockOpF32Ready(what);
    return blockSolveMultiRun("relaxed multi-source block solve", nsrc, q, ldq, rhsIsCharge, x, ldx, restart, tol, maxit,
                              relax, iters, relres, hist, maxhist, &multiCalls, s);
}

// (ks N) x nsrc column-major host arrays: one staging copy each way
int Operator::blockSolveMultiRelaxedHost(const double* Q, int nsrc, bool rhsIsCharge, double* X, int restart,
                                         double tol, int maxit, double relax, int* iters, double* relres) {
    const char* const what = "aniso_block_solve_multi_relaxed";
    multiRelaxedEnter(what, true, tol, relax);
    multiCalls.clear();
    if (!blockSolveMultiCheck(what, nsrc, Q, geo.N, X, geo.N, iters, restart, tol, maxit)) return 0;
    blockOpF32Ready(what);
    ensureDevice();
    const size_t bytes = (size_t)nsrc * ks * geo.N * sizeof(double);
    DevBuf dq, dx;
    dq.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(dq.p, Q, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, X, bytes, hipMemcpyHostToDevice, own));
    const int steps = blockSolveMultiRelaxedDev(nsrc, dq.as<double>(), geo.N, rhsIsCharge, dx.as<double>(), geo.N,
                                                restart, tol, maxit, relax, iters, relres, nullptr, 0, own);
    HIP_CHECK(hipMemcpyAsync(X, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return steps;
}

int Operator::forwardSolveMultiRelaxedDev(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x,
                                          int64_t ldx, int restart, double tol, int maxit, double relax, int* iters,
                                          double* relres, double* hist, int maxhist, hipStream_t s) {
    const char* const what = "aniso_forward_solve_multi_relaxed_dev";
    relax = multiRelaxedEnter(what, false, tol, relax);
    multiCalls.clear();
    if (!forwardSolveMultiCheck(what, nrhs, q, ldq, x, ldx, iters, restart, tol, maxit)) return 0;
    return forwardSolveMultiRun(nrhs, q, ldq, rhsIsSource, x, ldx, restart, tol, maxit, relax, iters, relres, hist,
                                maxhist, &multiCalls, s);
}

// N x k column-major host arrays: one staging copy each way
int Operator::forwardSolveMultiRelaxedHost(const double* Q, int k, bool rhsIsSource, double* X, int restart,
                                           double tol, int maxit, double relax, int* iters, double* relres) {
    const char* const what = "aniso_forward_solve_multi_relaxed";
    multiRelaxedEnter(what, false, tol, relax);
    multiCalls.clear();
    if (!forwardSolveMultiCheck(what, k, Q, geo.N, X, geo.N, iters, restart, tol, maxit)) return 0;
    ensureDevice();
    const size_t bytes = (size_t)k * geo.N * sizeof(double);
    DevBuf dq, dx;
    dq.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(dq.p, Q, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, X, bytes, hipMemcpyHostToDevice, own));
    const int steps = forwardSolveMultiRelaxedDev(k, dq.as<double>(), geo.N, rhsIsSource, dx.as<double>(), geo.N, restart,
                                                  tol, maxit, relax, iters, relres, nullptr, 0, own);
    HIP_CHECK(hipMemcpyAsync(X, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return steps;
}

// the same on host pointers (the MEX shim's 'solve' op): one staging copy each way
int Operator::blockSolveHost(const double* rhs, double* x, int restart, double tol, int maxit, double* hist,
                             int maxhist, double* relres) {
    checkBlockLimit(false);
    ensureDevice();
    const size_t bytes = (size_t)ks * geo.N * sizeof(double);
    DevBuf db, dx;
    db.alloc(bytes);
    dx.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(db.p, rhs, bytes, hipMemcpyHostToDevice, own));
    HIP_CHECK(hipMemcpyAsync(dx.p, x, bytes, hipMemcpyHostToDevice, own));
    const int it = blockSolveDev(db.as<double>(), dx.as<double>(), restart, tol, maxit, hist, maxhist, relres, own);
    HIP_CHECK(hipMemcpyAsync(x, dx.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    return it;
}

}  // namespace aniso
