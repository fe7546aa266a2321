// mode_factor.hpp -- one entry's factor of a single mode on the mode-shared E caches, shared by
// the mode kernels (mode_apply.hip: formed on the fly) and the resident per-mode blocks
// (mode_resident.hip: formed once, stored).
#pragma once

#include "hm_entry.hpp"

namespace aniso {

// (E / r) T_id(c) at (dx, dy^2) from the source (dx: source minus target, as hm_entry
// takes it; T_id is odd in c for odd id).  id is wave-uniform: the three-term recurrence
// runs from (T_0, T_1) in a uniform loop.  guard0 as in hm_entry: r = 0 adds E = 0.
template <bool guard0>
__device__ __forceinline__ double mode_factor(double e, double dx, double dy2, int id) {
    double r2 = __builtin_fma(dx, dx, dy2);
    if constexpr (guard0) r2 = __builtin_fmax(r2, 1e-300);
    const double ri = rsqrt_nr<2>(r2);
    const double c = dx * ri, c2 = c + c;
    double t0 = 1.0, t1 = c;
#pragma nounroll
    for (int n = 1; n < id; ++n) {
        const double t = __builtin_fma(c2, t1, -t0);
        t0 = t1;
        t1 = t;
    }
    return (e * ri) * (id == 0 ? 1.0 : t1);
}

}  // namespace aniso
