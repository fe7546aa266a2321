// kernels.hip -- hand-written CDNA4 (gfx950) kernels for the device-side cache
// build of the anisotropic RTE integral operator (the apply kernels are in
// apply.hip).
//
// Reference behaviour (file:line under lowrank/aniso):
//   cache build  bbfmm.h:949-1039, KernelFactory.cpp:67-207, 240-267
// Both bbfmm instances (imag (e^-tau - 1) cos(m th)/r and real cos(m th)/r) share
// tree, lists, charges and translation operators, so one pass with the summed
// kernel e^-tau cos(m th)/r computes their sum (DESIGN.md "Merged kernels").
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>

#include "device_common.hpp"
#include "line_integral.hpp"

namespace aniso {

__global__ void k_permute(int64_t N, const int* __restrict__ perm, const double* __restrict__ orig,
                          double* __restrict__ tree) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < N) tree[k] = orig[perm[k]];
}

// ----------------------------------------------------------------- cache build

// downPassCache's M2L blocks (bbfmm.h:959-975, 782-804) for all stored (target,
// source) pairs, K[t][s] = kernel(cheb_s(src), cheb_t(tgt)), column-major
// (pair*256 + s*16 + t), the layout k_m2l streams; pairTgt = ~target marks a
// canonical block (same layout, also read transposed).
__global__ void __launch_bounds__(256) k_cache_m2l(int64_t total, const int* __restrict__ pairTgt,
                                                   const int* __restrict__ src, const double* __restrict__ ncx,
                                                   const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                   const double* __restrict__ nry, const double* __restrict__ stcoef,
                                                   const Params* __restrict__ P, int mode, double* __restrict__ K) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int64_t p = e >> 8;
    const int s = (int)((e >> 4) & 15), t = (int)(e & 15);
    int tn = pairTgt[p];
    const int sn = src[p];
    if (tn < 0) tn = ~tn;
    double bx = ncx[tn] + nrx[tn] * P->cheb[t & 3];
    double by = ncy[tn] + nry[tn] * P->cheb[t >> 2];
    double ax = ncx[sn] + nrx[sn] * P->cheb[s & 3];
    double ay = ncy[sn] + nry[sn] * P->cheb[s >> 2];
    K[e] = pair_kernel(P, stcoef, mode, ax, ay, bx, by);
}

// Mode-shared M2L cache: E[t][s] = e^-tau(cheb_s(src), cheb_t(tgt))
// for every directed (target, source) pair, column-major (pair*256 + s*16 + t), the
// layout k_m2l_hm streams (lane (column s, row quad) reads 32 contiguous bytes).
__global__ void __launch_bounds__(256) k_cache_att_m2l(int64_t total, const int* __restrict__ pairTgt,
                                                       const int* __restrict__ src, const double* __restrict__ ncx,
                                                       const double* __restrict__ ncy, const double* __restrict__ nrx,
                                                       const double* __restrict__ nry,
                                                       const double* __restrict__ stcoef,
                                                       const Params* __restrict__ P, double* __restrict__ E) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int64_t p = e >> 8;
    const int s = (int)((e >> 4) & 15), t = (int)(e & 15);
    const int tn = pairTgt[p], sn = src[p];
    double bx = ncx[tn] + nrx[tn] * P->cheb[t & 3];
    double by = ncy[tn] + nry[tn] * P->cheb[t >> 2];
    double ax = ncx[sn] + nrx[sn] * P->cheb[s & 3];
    double ay = ncy[sn] + nry[sn] * P->cheb[s >> 2];
    E[e] = pair_kernel(P, stcoef, kAttMode, ax, ay, bx, by);
}

// The mode-0 diagonal of the merged kernel, sigma_t at each point (evaluate(a),
// KernelFactory.cpp:260), tree order: the r = 0 entry the mode-shared near field
// adds apart from its blocks.
__global__ void k_sigma_diag(int64_t N, const double* __restrict__ pxT, const double* __restrict__ pyT,
                             const double* __restrict__ stcoef, const Params* __restrict__ P,
                             double* __restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < N) out[k] = sigma_eval(P, stcoef, pxT[k], pyT[k]);
}

// downPassCache's U/W blocks (bbfmm.h:991-1011): per target leaf, column-major
// nT4 x S (nT rounded up to a multiple of 4, zero rows) over the concatenated source points of its U then W members.
__global__ void __launch_bounds__(256) k_cache_near(int nl, const int* __restrict__ leaves,
                                                    const int64_t* __restrict__ nearPtr,
                                                    const int* __restrict__ nearSrc,
                                                    const int64_t* __restrict__ nearKOff,
                                                    const int64_t* __restrict__ begin,
                                                    const int64_t* __restrict__ count, const double* __restrict__ pxT,
                                                    const double* __restrict__ pyT, const double* __restrict__ stcoef,
                                                    const Params* __restrict__ P, int mode, int maxSrc,
                                                    double* __restrict__ K) {
    extern __shared__ int64_t shi[];
    int64_t* sBeg = shi;
    int* sOff = reinterpret_cast<int*>(shi + maxSrc);
    const int li = blockIdx.x;
    if (li >= nl) return;
    const int n = leaves[li];
    const int nT = (int)count[n];
    const int64_t tb = begin[n];
    const int64_t j0 = nearPtr[li];
    const int ns = (int)(nearPtr[li + 1] - j0);
    if (threadIdx.x == 0) {
        int off = 0;
        for (int j = 0; j < ns; ++j) {
            int s = nearSrc[j0 + j];
            sBeg[j] = begin[s];
            sOff[j] = off;
            off += (int)count[s];
        }
        sOff[ns] = off;
    }
    __syncthreads();
    const int S = sOff[ns];
    double* Kl = K + nearKOff[li];
    const int nTs = (nT + 3) & ~3;  // rows padded to a multiple of 4 (32-B row quads in k_near)
    const int64_t total = (int64_t)nTs * S;
    for (int64_t e = threadIdx.x; e < total; e += blockDim.x) {
        int sc = (int)(e / nTs), t = (int)(e - (int64_t)sc * nTs);
        if (t >= nT) {
            Kl[e] = 0.0;
            continue;
        }
        int j = 0;
        while (sOff[j + 1] <= sc) ++j;
        int64_t sp = sBeg[j] + (sc - sOff[j]);
        int64_t tp = tb + t;
        Kl[e] = pair_kernel(P, stcoef, mode, pxT[sp], pyT[sp], pxT[tp], pyT[tp]);
    }
}

__global__ void k_line_integrals(int n, const double* __restrict__ seg, const double* __restrict__ stcoef,
                                 const Params* __restrict__ P, double* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = line_integral(P, stcoef, seg[4 * i], seg[4 * i + 1], seg[4 * i + 2], seg[4 * i + 3]);
}

// ----------------------------------------------------------------- launchers

void launch_cache_m2l(int64_t npairs, const int* pairTgt, const int* src, const NodeBoxes& b, const double* stcoef,
                      const Params* P, int mode, double* K, hipStream_t s) {
    if (npairs <= 0) return;
    int64_t total = npairs * 256;
    k_cache_m2l<<<blocks_for(total, 256), 256, 0, s>>>(total, pairTgt, src, b.cx, b.cy, b.rx, b.ry, stcoef, P, mode,
                                                       K);
    HIP_LAUNCH_CHECK();
}

void launch_cache_att_m2l(int64_t npairs, const int* pairTgt, const int* src, const NodeBoxes& b,
                          const double* stcoef, const Params* P, double* E, hipStream_t s) {
    if (npairs <= 0) return;
    int64_t total = npairs * 256;
    k_cache_att_m2l<<<blocks_for(total, 256), 256, 0, s>>>(total, pairTgt, src, b.cx, b.cy, b.rx, b.ry, stcoef, P,
                                                           E);
    HIP_LAUNCH_CHECK();
}

void launch_sigma_diag(int64_t N, const double* pxT, const double* pyT, const double* stcoef, const Params* P,
                       double* out, hipStream_t s) {
    if (N <= 0) return;
    k_sigma_diag<<<blocks_for(N, 256), 256, 0, s>>>(N, pxT, pyT, stcoef, P, out);
    HIP_LAUNCH_CHECK();
}

void launch_cache_near(int nl, const int* leaves, const int64_t* nearPtr, const int* nearSrc, const int64_t* nearKOff,
                       const int64_t* begin, const int64_t* count, const TreePoints& pts, const double* stcoef,
                       const Params* P, int mode, int maxSrc, double* K, hipStream_t s) {
    if (nl <= 0) return;
    size_t shm = (size_t)maxSrc * sizeof(int64_t) + (size_t)(maxSrc + 1) * sizeof(int);
    k_cache_near<<<nl, 256, shm, s>>>(nl, leaves, nearPtr, nearSrc, nearKOff, begin, count, pts.px, pts.py, stcoef, P,
                                      mode, maxSrc, K);
    HIP_LAUNCH_CHECK();
}


void launch_permute(int64_t N, const int* perm, const double* orig, double* tree, hipStream_t s) {
    if (N <= 0) return;
    k_permute<<<blocks_for(N, 256), 256, 0, s>>>(N, perm, orig, tree);
    HIP_LAUNCH_CHECK();
}

void launch_line_integrals(int n, const double* seg, const double* stcoef, const Params* P, double* out,
                           hipStream_t s) {
    if (n <= 0) return;
    k_line_integrals<<<blocks_for(n, 256), 256, 0, s>>>(n, seg, stcoef, P, out);
    HIP_LAUNCH_CHECK();
}

// ---- halo exchange of the sharded apply (comm.hpp)
__global__ void k_halo_pack(int64_t n, int nb, const int64_t* __restrict__ pos, const int64_t* __restrict__ base,
                            const int64_t* __restrict__ stride, const double* __restrict__ x, int64_t ldx,
                            double* __restrict__ buf) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (int b = 0; b < nb; ++b) buf[base[j] + b * stride[j]] = x[(size_t)b * ldx + pos[j]];
}

__global__ void k_halo_unpack(int64_t n, int nb, const int64_t* __restrict__ pos, const int64_t* __restrict__ base,
                              const int64_t* __restrict__ stride, const double* __restrict__ buf,
                              double* __restrict__ x, int64_t ldx) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (int b = 0; b < nb; ++b) x[(size_t)b * ldx + pos[j]] = buf[base[j] + b * stride[j]];
}

void launch_halo_pack(int64_t n, int nb, const int64_t* pos, const int64_t* base, const int64_t* stride,
                      const double* x, int64_t ldx, double* buf, hipStream_t s) {
    if (n <= 0) return;
    k_halo_pack<<<blocks_for(n, 256), 256, 0, s>>>(n, nb, pos, base, stride, x, ldx, buf);
    HIP_LAUNCH_CHECK();
}

void launch_halo_unpack(int64_t n, int nb, const int64_t* pos, const int64_t* base, const int64_t* stride,
                        const double* buf, double* x, int64_t ldx, hipStream_t s) {
    if (n <= 0) return;
    k_halo_unpack<<<blocks_for(n, 256), 256, 0, s>>>(n, nb, pos, base, stride, buf, x, ldx);
    HIP_LAUNCH_CHECK();
}

// ---- the gathered input of a sharded high-order matvec: a rank's part of
// the all-gather is its owned slice of the nb rows, row b at b * stride (stride: the largest
// owned count of any rank).  Grid: x over the positions of a slice, y the row, z the part.
__global__ void k_slice_pack(int64_t own, const double* __restrict__ xo, int64_t ldx, int64_t stride,
                             double* __restrict__ buf) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (k < own) buf[b * stride + k] = xo[b * ldx + k];
}

// parts p0 + blockIdx.z (all but `skip`, the rank's own) into [cuts[p], cuts[p + 1]) of the rows of x
__global__ void k_slice_unpack(int p0, int skip, const int64_t* __restrict__ cuts, int nb, int64_t stride,
                               const double* __restrict__ buf, double* __restrict__ x, int64_t ldx) {
    const int p = p0 + (int)blockIdx.z;
    if (p == skip) return;
    const int64_t lo = cuts[p], cnt = cuts[p + 1] - lo;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (k < cnt && k < stride) x[b * ldx + lo + k] = buf[((int64_t)p * nb + b) * stride + k];
}

void launch_slice_pack(int64_t own, int nb, const double* xo, int64_t ldx, int64_t stride, double* buf,
                       hipStream_t s) {
    if (own <= 0 || nb <= 0) return;
    if (own > stride) throw std::invalid_argument("slice pack: the owned count exceeds the part's row stride");
    k_slice_pack<<<dim3(blocks_for(own, 256), (unsigned)nb), 256, 0, s>>>(own, xo, ldx, stride, buf);
    HIP_LAUNCH_CHECK();
}

void launch_slice_unpack(int p0, int p1, int skip, const int64_t* cuts, int nb, int64_t stride, const double* buf,
                         double* x, int64_t ldx, hipStream_t s) {
    // (nothing to do: no part but the skipped one, or every rank owns nothing)
    if (p1 <= p0 || nb <= 0 || stride <= 0 || (p1 - p0 == 1 && p0 == skip)) return;
    if (p1 - p0 > 65535) throw std::invalid_argument("slice unpack: more than 65535 parts");
    k_slice_unpack<<<dim3(blocks_for(stride, 256), (unsigned)nb, (unsigned)(p1 - p0)), 256, 0, s>>>(p0, skip, cuts, nb,
                                                                                                 stride, buf, x, ldx);
    HIP_LAUNCH_CHECK();
}


}  // namespace aniso
