// line_integral.hpp -- the pair kernel of the integral operator on the device: sigma_t's
// line integral between two points (the DDA walk over the crossed squares) and the
// merged kernel e^-tau cos(m th) / r built on it.  Shared by the cache-build kernels
// (kernels.hip) and the direct evaluation at chosen targets (direct.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"

namespace aniso {

// std::tr1::legendre recurrence (libstdc++ __poly_legendre_p), values P_0..P_{d-1}
__device__ __forceinline__ void legendre_all(int d, double x, double* P) {
    P[0] = 1.0;
    if (d < 2) return;
    if (x == 1.0 || x == -1.0) {
        for (int l = 1; l < d; ++l) P[l] = (x == -1.0 && (l & 1)) ? -1.0 : 1.0;
        return;
    }
    P[1] = x;
    for (int l = 2; l < d; ++l) P[l] = 2.0 * x * P[l - 1] - P[l - 2] - (x * P[l - 1] - P[l - 2]) / (double)l;
}

// integral_helper (KernelFactory.cpp:174-190): d-point Gauss rule on one piece
// lying in one square; sigma_t's Legendre expansion is evaluated at GLOBAL
// coordinates (reference quirk).  stcoef already carries 1/legendreNorms.
static __device__ double sigma_piece(const Params* __restrict__ P, const double* __restrict__ stcoef, double xa,
                                     double ya, double xb, double yb) {
    const int sz = P->sz, d = P->d, d2 = P->d2;
    double mx = (xa + xb) / 2, my = (ya + yb) / 2;
    int col = (int)floor(mx * sz), row = (int)floor(my * sz);
    col = col < 0 ? 0 : (col >= sz ? sz - 1 : col);
    row = row < 0 ? 0 : (row >= sz ? sz - 1 : row);
    const double* c = stcoef + (size_t)(col * sz + row) * d2;
    double ret = 0.0;
    double Px[kMaxD], Py[kMaxD];
    for (int i = 0; i < d; ++i) {
        double x = mx + (xa - xb) / 2 * P->gx[i];
        double y = my + (ya - yb) / 2 * P->gx[i];
        legendre_all(d, x, Px);
        legendre_all(d, y, Py);
        double dot = 0.0;
        for (int n = 0; n < d; ++n) {
            double rowdot = 0.0;
            for (int k = 0; k < d; ++k) rowdot += Py[k] * c[n * d + k];
            dot += Px[n] * rowdot;
        }
        ret += dot * P->gw[i];
    }
    double ddx = xa - xb, ddy = ya - yb;
    return ret * sqrt(ddx * ddx + ddy * ddy) / 2.0;
}

// lineIntegral (KernelFactory.cpp:67-166).  The reference splits the segment at
// midpoints and grid lines and applies the Gauss rule per piece; the integrand is
// a polynomial of degree <= 2d-2 inside every square, so the d-point rule is exact
// on any piece inside one square and the value is independent of where the pieces
// are cut.  We walk the grid cells the segment crosses (DDA) instead: same
// integral, no recursion, bounded loop (one iteration per crossed square).
static __device__ double line_integral(const Params* __restrict__ P, const double* __restrict__ stcoef, double x0,
                                       double y0, double x1, double y1) {
    const int sz = P->sz;
    const double dx = P->dx;
    int c0 = (int)floor(x0 * sz), r0 = (int)floor(y0 * sz);
    int c1 = (int)floor(x1 * sz), r1 = (int)floor(y1 * sz);
    if (c0 == c1 && r0 == r1) return sigma_piece(P, stcoef, x0, y0, x1, y1);
    const double ddx = x1 - x0, ddy = y1 - y0;
    const double INF = 1e300;
    double tmx = INF, tdx = INF, tmy = INF, tdy = INF;
    if (ddx != 0.0) {
        double xb = (ddx > 0 ? (c0 + 1) : c0) * dx;
        tmx = (xb - x0) / ddx;
        tdx = dx / fabs(ddx);
    }
    if (ddy != 0.0) {
        double yb = (ddy > 0 ? (r0 + 1) : r0) * dx;
        tmy = (yb - y0) / ddy;
        tdy = dx / fabs(ddy);
    }
    double t0 = 0.0, sum = 0.0, xa = x0, ya = y0;
    const int guard = abs(c1 - c0) + abs(r1 - r0) + 4;
    for (int it = 0; it < guard; ++it) {
        double tn = fmin(fmin(tmx, tmy), 1.0);
        bool last = tn >= 1.0;
        double xb = last ? x1 : x0 + tn * ddx;
        double yb = last ? y1 : y0 + tn * ddy;
        if (tn > t0) sum += sigma_piece(P, stcoef, xa, ya, xb, yb);
        if (last) return sum;
        if (tmx <= tn) tmx += tdx;
        if (tmy <= tn) tmy += tdy;
        t0 = tn;
        xa = xb;
        ya = yb;
    }
    return sum + sigma_piece(P, stcoef, xa, ya, x1, y1);
}

// evaluate (KernelFactory.cpp:193-207): sigma_t at a point, global-coordinate Legendre
static __device__ double sigma_eval(const Params* __restrict__ P, const double* __restrict__ stcoef, double x,
                                    double y) {
    const int sz = P->sz, d = P->d;
    int col = (int)floor(x * sz), row = (int)floor(y * sz);
    col = col < 0 ? 0 : (col >= sz ? sz - 1 : col);
    row = row < 0 ? 0 : (row >= sz ? sz - 1 : row);
    const double* c = stcoef + (size_t)(col * sz + row) * P->d2;
    double Px[kMaxD], Py[kMaxD];
    legendre_all(d, x, Px);
    legendre_all(d, y, Py);
    double s = 0.0;
    for (int n = 0; n < d; ++n)
        for (int k = 0; k < d; ++k) s += Px[n] * Py[k] * c[n * d + k];
    return s;
}

// imag_m + real_m (makeKernels, KernelFactory.cpp:240-267); a = source, b = target.
// m = kAttMode: the mode-independent factor e^-tau alone (0 at r = 0), the entry of
// the mode-shared cache.
static __device__ double pair_kernel(const Params* __restrict__ P, const double* __restrict__ stcoef, int m, double ax,
                                     double ay, double bx, double by) {
    double ddx = ax - bx, ddy = ay - by;
    double dist = sqrt(ddx * ddx + ddy * ddy);
    if (m == kAttMode) return dist == 0.0 ? 0.0 : exp(-line_integral(P, stcoef, ax, ay, bx, by));
    if (dist == 0.0) return m == 0 ? sigma_eval(P, stcoef, ax, ay) : 0.0;
    double gk = (m == 0) ? 1.0 / dist : cos(m * atan2(ddy, ddx)) / dist;
    double tau = line_integral(P, stcoef, ax, ay, bx, by);
    return exp(-tau) * gk;
}

}  // namespace aniso
