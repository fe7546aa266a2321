// mode_near_resident.hip -- one mode's resident near-field factor blocks on a high-order
// handle (np = 6, 8) and the fp64 MFMA near field that streams them.
//
// k_near_mode (mode_apply.hip) forms the factor (E / r) T_id(c) of every stored near entry
// again for every chunk of columns and every pass of a solve.  It depends on the medium and
// the mode only, so here it is formed once per stored entry (k_near_mode_blocks, the same
// mode_factor<true> call on the same data) and the near field of a target leaf becomes
//     out(nT x 16) = scale . (F(nT x S) . X(S x 16) + sigma_t diagonal for id = 0)
// on v_mfma_f64_16x16x4_f64 with F as the only operand that comes from HBM.
//
// Layout of a leaf's block (nT targets, S sources; nq = ceil(nT / 4) row quads, NG =
// ceil(S / 16) source groups; 16 nq NG . 4 doubles at the leaf's offset of Plan::nearFOff):
// 16-row tiles, tile t at t . 256 NG (every tile but the last holds 4 row quads, tile t holds
// qt = min(4, nq - 4 t)); within a tile [group g][row quad q < qt][h = 0 .. 3] 4 x 4
// microtiles of 16 doubles = one 128-B line each, element (row a, source e) of microtile
// (g, q, h) -- target 16 t + 4 q + a, source 16 g + 4 h + e -- at offset 4 a + e.  Rows past
// nT and sources past S are stored as exact zeros; rows are padded to a multiple of 4 only
// (as the E blocks are), sources to a multiple of 16.  The MFMA's A operand gives lane
// (r = lane & 15, h = lane >> 4) row r of the tile and k index h of the step: the lane reads
// row r % 4 of microtile (g, r / 4, h), one 32-B load per four k-steps, the k index of step
// (g, e) being source 16 g + 4 h + e.  A wave's load of one group covers qt whole 512-B
// runs (2 KB for a full tile), and every stored line is fetched by exactly one wave.
// The B operand is the charges of the leaf's sources, gathered through nearPts from up to two
// fT buffers of k_prepare's layout (columns 0 .. KA-1 of fTA, 8 .. 8+KB-1 of fTB, the others
// zero) and staged in LDS as [k][16 columns] with the rows of one step adjacent (512 B, no
// bank conflict), GC groups = 4 GC MFMA steps per barrier, double-buffered; the gather (16 B
// per lane: two columns of a source) runs a chunk ahead of the barrier that publishes it
// (its positions two), in registers.
// One workgroup per target leaf, wave w serves tiles w, w + NW, ...: NW = 4 with a loop over
// tiles for leaves of more than four, NW = 1 where no leaf has more than 16 points -- the
// workgroup is then one wave and its barrier orders that wave's own LDS traffic only.
// A column never meets another in an MFMA, every sum runs in source order, there are no
// atomics: a column's bits do not depend on the other columns and repeats are bitwise equal.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "device_common.hpp"
#include "hm_entry.hpp"
#include "kernels.hpp"
#include "mode_factor.hpp"

namespace aniso {

typedef double f64x4n __attribute__((ext_vector_type(4)));

// the near blocks of mode id from the directed near E blocks (column-major nT4 x S per leaf,
// as k_near_mode reads them), one workgroup per target leaf, destination-driven: every
// double of the leaf's block is written once, the padding as zero
__global__ void __launch_bounds__(256) k_near_mode_blocks(const int4* __restrict__ leafInfo,
                                                          const int64_t* __restrict__ nearPtsPtr,
                                                          const int* __restrict__ nearPts,
                                                          const int64_t* __restrict__ nearKOff,
                                                          const int64_t* __restrict__ nearFOff,
                                                          const double* __restrict__ E, const double* __restrict__ pxT,
                                                          const double* __restrict__ pyT, int id,
                                                          double* __restrict__ F) {
    const int4 info = leafInfo[blockIdx.x];
    const int nT = info.z, S = info.w;
    const int64_t tb = info.y, pb = nearPtsPtr[blockIdx.x];
    const int nq = (nT + 3) >> 2, nT4 = 4 * nq, NG = (S + 15) >> 4;
    const double* Eb = E + nearKOff[blockIdx.x];
    double* Fb = F + nearFOff[blockIdx.x];
    const int64_t total = (int64_t)nT4 * 16 * NG, tileSz = (int64_t)NG * 256;
    for (int64_t d = threadIdx.x; d < total; d += 256) {
        const int tile = (int)(d / tileSz);
        const int rem = (int)(d - tile * tileSz);
        const int qt = min(4, nq - 4 * tile);
        const int g = rem / (qt * 64), r2 = rem - g * (qt * 64);
        const int q = r2 >> 6, h = (r2 >> 4) & 3, a = (r2 >> 2) & 3, e = r2 & 3;
        const int t = 16 * tile + 4 * q + a, s = 16 * g + 4 * h + e;
        double f = 0.0;
        if (t < nT && s < S) {
            const int64_t sp = nearPts[pb + s];
            const double dy = pyT[sp] - pyT[tb + t];
            f = mode_factor<true>(Eb[(size_t)s * nT4 + t], pxT[sp] - pxT[tb + t], dy * dy, id);
        }
        Fb[d] = f;
    }
}

// (waves per SIMD: NW = 1 holds two chunks' block loads, 150 registers, and its LDS allows 3.25;
// NW = 4 takes 136 registers unless held to 4)
template <int NW, int GC>
__global__ void __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 1 ? 3 : 4)))
    k_near_resident(const int4* __restrict__ leafInfo, const int64_t* __restrict__ nearPtsPtr,
                    const int* __restrict__ nearPts, const int64_t* __restrict__ nearFOff, const double* __restrict__ F,
                    const double* __restrict__ sigDiag, const double* __restrict__ fTA, int KA, int KSA,
                    const double* __restrict__ fTB, int KB, int KSB, const int* __restrict__ operm, int64_t obase,
                    double scale, double* __restrict__ outA, int64_t ldoA, double* __restrict__ outB, int64_t ldoB) {
    constexpr int NR = 2 * GC / NW;  // staging rounds of one wave per chunk: a round is two MFMA steps' 8 x 16 rows
    static_assert(NR * NW == 2 * GC, "whole staging rounds");
    constexpr bool AHEAD = NW == 1;  // one-tile leaves: the next chunk's block loads in flight as well
    __shared__ double X[2][GC * 256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, h = lane >> 4;
    const int4 info = leafInfo[blockIdx.x];
    const int nT = info.z, S = info.w;
    const int64_t tb = info.y, pb = nearPtsPtr[blockIdx.x];
    const int nq = (nT + 3) >> 2, NTL = (nq + 3) >> 2, NG = (S + 15) >> 4;
    const double* Fb = F + nearFOff[blockIdx.x];
    // this lane's column of the 16: its charge buffer, row stride and column there (null: a zero column)
    const bool colA = r < KA, colB = r >= 8 && r - 8 < KB;
    const double* fc = colA ? fTA + r : colB ? fTB + (r - 8) : nullptr;
    const int ksc = colA ? KSA : KSB;
    // the charges of the chunk at group g0, 16 columns wide.  The gather's lane (rr = lane >> 3,
    // cp = lane & 7) loads columns 2 cp, 2 cp + 1 of one source as 16 B (a row of fT is whole
    // 16-B vectors, the pad entry of an odd K zero); round p = w + NW it is LDS rows 8 p + rr =
    // 16 gi + 4 e + hh of group gi = p / 2, steps e = 2 (p % 2) + rr / 4, hh = rr % 4: sources
    // 16 gi + 4 hh + e, a wave's store 1 KB in a run.  The tree positions are loaded a chunk
    // ahead of the charges and the charges a chunk ahead of their use, so neither gather waits
    // in front of the barrier (past the last chunk both wrap to the first: the next tile pass
    // reads the same sources again)
    const int cp = lane & 7, rr = lane >> 3;
    const double* gc = 2 * cp < KA ? fTA + 2 * cp : (cp >= 4 && 2 * cp - 8 < KB) ? fTB + (2 * cp - 8) : nullptr;
    const int gks = cp < 4 ? KSA : KSB;
    int ix[NR];
    dbl2 xv[NR];
    auto load_ix = [&](int g0) {
#pragma unroll
        for (int it = 0; it < NR; ++it) {
            const int p = w + NW * it, s = 16 * (g0 + (p >> 1)) + 4 * (rr & 3) + 2 * (p & 1) + (rr >> 2);
            ix[it] = (gc && s < S) ? nearPts[pb + s] : -1;
        }
    };
    auto load_x = [&]() {
#pragma unroll
        for (int it = 0; it < NR; ++it)
            xv[it] = ix[it] >= 0 ? *reinterpret_cast<const dbl2*>(gc + (size_t)ix[it] * gks) : dbl2{0.0, 0.0};
    };
    auto next = [&](int g0) { return g0 + GC < NG ? g0 + GC : 0; };
    load_ix(0);
    load_x();
    load_ix(next(0));
    int buf = 0;
    for (int tile0 = 0; tile0 < NTL; tile0 += NW) {  // (workgroup-uniform)
        const int tile = tile0 + w;
        const bool has = tile < NTL;  // (wave-uniform)
        const int qt = has ? min(4, nq - 4 * tile) : 0;
        const bool aOk = (r >> 2) < qt;
        const double* Fl = Fb + (size_t)tile * NG * 256 + ((r >> 2) * 4 + h) * 16 + (r & 3) * 4;
        f64x4n acc = {0.0, 0.0, 0.0, 0.0};
        // the A operand of the chunk at group g0: this lane's row of its GC groups
        auto load_a = [&](int g0, f64x4n (&a)[GC]) {
#pragma unroll
            for (int gi = 0; gi < GC; ++gi) {
                a[gi] = f64x4n{0.0, 0.0, 0.0, 0.0};
                if (aOk && g0 + gi < NG)
                    a[gi] = __builtin_nontemporal_load(reinterpret_cast<const f64x4n*>(Fl + (size_t)(g0 + gi) * qt * 64));
            }
        };
        f64x4n a[GC], an[GC];
        if constexpr (AHEAD) load_a(0, an);
        for (int g0 = 0; g0 < NG; g0 += GC, buf ^= 1) {
            if constexpr (AHEAD) {
#pragma unroll
                for (int gi = 0; gi < GC; ++gi) a[gi] = an[gi];
                load_a(g0 + GC, an);  // (past the last group: zeros, nothing is read)
            } else {
                load_a(g0, a);
            }
            double* Xb = X[buf];
#pragma unroll
            for (int it = 0; it < NR; ++it)
                *reinterpret_cast<dbl2*>(Xb + (8 * (w + NW * it) + rr) * 16 + 2 * cp) = xv[it];
            load_x();                    // the next chunk's charges ...
            load_ix(next(next(g0)));     // ... and the positions of the one after it
            __syncthreads();  // (the other buffer is rewritten only after the next barrier)
            if (has) {
#pragma unroll
                for (int gi = 0; gi < GC; ++gi)
                    if (g0 + gi < NG) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[gi][e], Xb[((4 * gi + e) * 4 + h) * 16 + r], acc, 0,
                                                                       0, 0);
                    }
            }
        }
        // accumulator element i of lane (r, h): row h + 4 i of the tile, column r
        if (has && fc) {
            double* const out = colA ? outA : outB;
            const int64_t co = colA ? (int64_t)r * ldoA : (int64_t)(r - 8) * ldoB;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = 16 * tile + h + 4 * i;
                if (t >= nT) continue;
                const int64_t kp = tb + t;
                double v = acc[i];
                if (sigDiag) v = __builtin_fma(sigDiag[kp], fc[(size_t)kp * ksc], v);
                out[co + out_index(operm, obase, kp)] = scale * v;
            }
        }
    }
}

void launch_near_mode_blocks(int id, const NearList& nl, const int64_t* nearFOff, const double* E,
                             const TreePoints& pts, double* F, hipStream_t s) {
    if (nl.nl <= 0) return;
    if (id < 0) throw std::invalid_argument("resident near blocks: negative mode");
    k_near_mode_blocks<<<nl.nl, 256, 0, s>>>(nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, nearFOff, E, pts.px, pts.py, id, F);
    HIP_LAUNCH_CHECK();
}

void launch_near_resident(int id, const NearList& nl, const double* F, const double* sigDiag, const double* fTA,
                          int KA, const double* fTB, int KB, double scale, const OutRows& oA, const OutRows& oB,
                          hipStream_t s) {
    if (nl.nl <= 0) return;
    if (id < 0) throw std::invalid_argument("resident near field: negative mode");
    auto compiled = [](int k) { return k == 2 || k == 4 || k == 5 || k == 8; };
    if (!compiled(KA) || (KB != 0 && !compiled(KB)) || (KB > 0 && (!fTB || !oB.out)))
        throw std::invalid_argument("resident near field: unsupported column counts " + std::to_string(KA) + " + " +
                                    std::to_string(KB));
    auto stride = [](int k) { return k % 2 == 0 ? k : k + 1; };  // kStride<K>
    const double* sd = id == 0 ? sigDiag : nullptr;
    if (nl.maxLeaf <= 16)
        k_near_resident<1, 3><<<nl.nl, 64, 0, s>>>(nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, F, sd, fTA, KA, stride(KA), fTB,
                                                   KB, stride(KB), oA.perm, oA.base, scale, oA.out, oA.ld, oB.out, oB.ld);
    else
        k_near_resident<4, 4><<<nl.nl, 256, 0, s>>>(nl.leafInfo, nl.ptsPtr, nl.pts, nl.off, F, sd, fTA, KA, stride(KA), fTB,
                                                    KB, stride(KB), oA.perm, oA.base, scale, oA.out, oA.ld, oB.out, oB.ld);
    HIP_LAUNCH_CHECK();
}

}  // namespace aniso
