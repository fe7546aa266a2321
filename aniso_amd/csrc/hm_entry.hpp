// hm_entry.hpp -- one entry of the mode-shared ("harmonic") block apply:
// the per-entry device functions shared by the rank-16 kernels (harmonic.hip) and the
// high-order ones (high_order.hip).  None of them depends on the Chebyshev order.
#pragma once

#include <hip/hip_runtime.h>

namespace aniso {

// 1/sqrt(x) to full double precision: v_rsq_f64 (about 2^-22 relative) and two
// Newton steps.  x = 0 gives a non-finite value; callers select it away.
__device__ __forceinline__ double rsqrt_f64(double x) {
    double y = __builtin_amdgcn_rsq(x);
    double h = x * y;
    double e = __builtin_fma(-h, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    h = x * y;
    e = __builtin_fma(-h, y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
}

// NR Newton steps after v_rsq_f64: one step leaves a relative error of about
// 1.5 eps0^2 (eps0 ~ 2^-22 for v_rsq_f64), i.e. ~1e-13 per kernel entry, far inside
// the 1e-10 parity tolerance; two steps give full double precision.
template <int NR>
__device__ __forceinline__ double rsqrt_nr(double x) {
    if constexpr (NR >= 2) {
        return rsqrt_f64(x);
    } else {
        const double y = __builtin_amdgcn_rsq(x);
        const double e = __builtin_fma(-(x * y), y, 1.0);
        return __builtin_fma(0.5 * y, e, y);
    }
}

// T_0 .. T_{K-1} at c (cos(b theta) for c = cos theta)
template <int K>
__device__ __forceinline__ void cheb_T(double c, double (&T)[K]) {
    T[0] = 1.0;
    if constexpr (K > 1) T[1] = c;
    const double c2 = c + c;
#pragma unroll
    for (int i = 2; i < K; ++i) T[i] = __builtin_fma(c2, T[i - 1], -T[i - 2]);
}

// One entry: E at (dx, dy) from the source, harmonic-weighted source charges xw;
// o[i] += T_i(c) (E / r) V.  guard0: r = 0 possible (near field): r^2 is raised to
// 1e-300 there, so 1/r stays finite and the entry adds exactly 0 through E = 0 (the
// mode-shared cache stores 0 at r = 0, kernels.hip pair_kernel): one v_max_f64
// instead of a compare and two selects per entry, the same bits elsewhere.
template <int K, bool guard0, int NR = 2>
__device__ __forceinline__ void hm_entry(double e, double dx, double dy2, const double (&xw)[K], double (&o)[K]) {
    double r2 = __builtin_fma(dx, dx, dy2);
    if constexpr (guard0) r2 = __builtin_fmax(r2, 1e-300);
    const double ri = rsqrt_nr<NR>(r2);
    const double c = dx * ri;
    double T[K];
    cheb_T<K>(c, T);
    double v = xw[0];
#pragma unroll
    for (int b = 1; b < K; ++b) v = __builtin_fma(T[b], xw[b], v);
    const double av = (e * ri) * v;
#pragma unroll
    for (int i = 0; i < K; ++i) o[i] = __builtin_fma(T[i], av, o[i]);
}

// The offset form of hm_entry (more than kMaxRhs blocks): one pass
// of the block operator takes K input blocks b0 .. b0 + K - 1 to K output blocks
// i0 .. i0 + K - 1,
//     o[i] += T_{i0+i}(c) (E / r) V,   V = sum_b T_{b0+b}(c) xw[b]   (xw[b] = hw_{b0+b} x_{b0+b}).
// i0 and b0 are wave-uniform run-time values: for each window the three-term recurrence
// runs from (T_0, T_1) to the window's start in a uniform loop and the window is then
// unrolled from its two seeds.  The input window is consumed into V before the output
// window is formed, so two values of T per row are live at a time.
// A lane's J rows (4 in the rank-16 kernels, 1 in the high-order M2L) share the uniform
// loops: J independent chains.
template <int K, bool guard0, int NR = 2, int J = 4>
__device__ __forceinline__ void hm_rows_win(const double (&e)[J], const double (&dx)[J], const double (&dy2)[J], int i0,
                                            int b0, const double (&xw)[K], double (&o)[J][K]) {
    static_assert(K >= 2, "a window holds at least T_n and T_{n+1}");
    double c2[J], er[J], t0[J], t1[J], v[J];
    auto step = [&](int j) {  // (T_n, T_{n+1}) -> (T_{n+1}, T_{n+2}); returns T_{n+2}
        const double t = __builtin_fma(c2[j], t1[j], -t0[j]);
        t0[j] = t1[j];
        t1[j] = t;
        return t;
    };
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double r2 = __builtin_fma(dx[j], dx[j], dy2[j]);
        if constexpr (guard0) r2 = __builtin_fmax(r2, 1e-300);
        const double ri = rsqrt_nr<NR>(r2);
        const double c = dx[j] * ri;
        c2[j] = c + c;
        er[j] = e[j] * ri;
        t0[j] = 1.0;
        t1[j] = c;
    }
#pragma nounroll
    for (int n = 0; n < b0; ++n)
#pragma unroll
        for (int j = 0; j < J; ++j) (void)step(j);
#pragma unroll
    for (int j = 0; j < J; ++j) v[j] = __builtin_fma(t1[j], xw[1], t0[j] * xw[0]);
#pragma unroll
    for (int b = 2; b < K; ++b)
#pragma unroll
        for (int j = 0; j < J; ++j) v[j] = __builtin_fma(step(j), xw[b], v[j]);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        v[j] *= er[j];  // (E / r) V
        t0[j] = 1.0;
        t1[j] = 0.5 * c2[j];
    }
#pragma nounroll
    for (int n = 0; n < i0; ++n)
#pragma unroll
        for (int j = 0; j < J; ++j) (void)step(j);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        o[j][0] = __builtin_fma(t0[j], v[j], o[j][0]);
        o[j][1] = __builtin_fma(t1[j], v[j], o[j][1]);
    }
#pragma unroll
    for (int i = 2; i < K; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) o[j][i] = __builtin_fma(step(j), v[j], o[j][i]);
}

// One entry for S sources and the whole operator (i0 = b0 = 0, at most kMaxRhs blocks;
// DESIGN.md §3.18.3).  What does not depend on the source -- r^2, 1/r, c, T_0 .. T_{K-1}
// and E / r -- is formed once; per source s
//     V_s = (E / r) sum_b T_b(c) xw[s][b],   o[s][i] += T_i(c) V_s.
// A source's chain is hm_rows_win's at i0 = b0 = 0 with one row, operation by operation,
// and reads nothing of another source: its bits depend neither on S nor on its slot.
template <int K, int S, int NR = 2>
__device__ __forceinline__ void hm_rows_src(double e, double dx, double dy2, const double (&xw)[S][K],
                                            double (&o)[S][K]) {
    static_assert(K >= 2, "at least T_0 and T_1");
    const double r2 = __builtin_fma(dx, dx, dy2);
    const double ri = rsqrt_nr<NR>(r2);
    const double c = dx * ri, c2 = c + c, er = e * ri;
    double T[K];
    T[0] = 1.0;
    T[1] = c;
#pragma unroll
    for (int i = 2; i < K; ++i) T[i] = __builtin_fma(c2, T[i - 1], -T[i - 2]);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double v = __builtin_fma(T[1], xw[s][1], T[0] * xw[s][0]);
#pragma unroll
        for (int b = 2; b < K; ++b) v = __builtin_fma(T[b], xw[s][b], v);
        v *= er;  // (E / r) V
#pragma unroll
        for (int i = 0; i < K; ++i) o[s][i] = __builtin_fma(T[i], v, o[s][i]);
    }
}

// ---- the fp32 entry of the relaxed-precision block operator (block_f32.hip)

// 1/sqrt(x) in fp32: v_rsq_f32 (1 ulp) and one Newton step
__device__ __forceinline__ float rsqrt_nr_f32(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    return y * __builtin_fmaf(-0.5f * x * y, y, 1.5f);
}

// hm_rows_win at i0 = b0 = 0 with one row, operation by operation, in fp32: the whole
// operator of at most kMaxRhs blocks.  guard0: r = 0 is the point itself, where E = 0; the
// floor keeps 1 / r finite in fp32's range (1e-30 is a separation of 1e-15, below any two
// points).
template <int K, bool guard0>
__device__ __forceinline__ void hm_entry_f32(float e, float dx, float dy2, const float (&xw)[K], float (&o)[K]) {
    static_assert(K >= 2, "at least T_0 and T_1");
    float r2 = __builtin_fmaf(dx, dx, dy2);
    if constexpr (guard0) r2 = __builtin_fmaxf(r2, 1e-30f);
    const float ri = rsqrt_nr_f32(r2);
    const float c = dx * ri, c2 = c + c, er = e * ri;
    float T[K];
    T[0] = 1.0f;
    T[1] = c;
#pragma unroll
    for (int i = 2; i < K; ++i) T[i] = __builtin_fmaf(c2, T[i - 1], -T[i - 2]);
    float v = __builtin_fmaf(T[1], xw[1], xw[0]);
#pragma unroll
    for (int b = 2; b < K; ++b) v = __builtin_fmaf(T[b], xw[b], v);
    v *= er;  // (E / r) V
#pragma unroll
    for (int i = 0; i < K; ++i) o[i] = __builtin_fmaf(T[i], v, o[i]);
}

// One entry in fp32 for S sources (block_multi_f32.hip): hm_rows_src's
// sharing -- r^2, 1 / r, c, T_0 .. T_{K-1} and E / r formed once -- around hm_entry_f32<K,
// false>'s chain per source, operation by operation (it starts with fmaf(T_1, xw[1], xw[0])).
// A source reads nothing of another source: its bits are hm_entry_f32's, whatever S and its
// slot.
template <int K, int S>
__device__ __forceinline__ void hm_rows_src_f32(float e, float dx, float dy2, const float (&xw)[S][K],
                                                float (&o)[S][K]) {
    static_assert(K >= 2, "at least T_0 and T_1");
    const float r2 = __builtin_fmaf(dx, dx, dy2);
    const float ri = rsqrt_nr_f32(r2);
    const float c = dx * ri, c2 = 2.0f * c, er = e * ri;  // (2 c: c + c exactly, with no add to contract)
    float T[K];
    T[0] = 1.0f;
    T[1] = c;
#pragma unroll
    for (int i = 2; i < K; ++i) T[i] = __builtin_fmaf(c2, T[i - 1], -T[i - 2]);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        float v = __builtin_fmaf(T[1], xw[s][1], xw[s][0]);
#pragma unroll
        for (int b = 2; b < K; ++b) v = __builtin_fmaf(T[b], xw[s][b], v);
        // T_0 = 1: hm_entry_f32's o[0] = fmaf(1, v er, o[0]) is an add of the product v er, which
        // the build's floating-point contraction fuses in every instance of k_ho_m2l_f32.  Written
        // out here, so that no instance of this function can come out otherwise.
        o[s][0] = __builtin_fmaf(v, er, o[s][0]);
        v *= er;  // (E / r) V
#pragma unroll
        for (int i = 1; i < K; ++i) o[s][i] = __builtin_fmaf(T[i], v, o[s][i]);
    }
}

}  // namespace aniso
