// kernels.hpp -- device-side parameter block and kernel declarations.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aniso {

constexpr int kNP = 4;          // Chebyshev order per dimension (np); rank = 16
constexpr int kRank = kNP * kNP;
constexpr int kMaxD = 6;        // quadRule supported on the GPU path

// Small read-only tables shared by all kernels of one operator (lives in HBM,
// served from L1/L2: a few KB).
struct Params {
    int sz, d, d2, nsq;
    double dx;
    double gx[kMaxD], gw[kMaxD];            // volume Gauss rule (line integral)
    double cheb[kNP];                       // -cos((i+1/2) pi / np)
    double tnode[kNP * kNP];                // T_l(c_i) at [i + l*np]
    double R[4][kRank * kRank];             // M2M / L2L transfer, col-major
    double interp[kMaxD * kMaxD * kMaxD * kMaxD];  // d2 x d2 col-major
    double sqrtW[kMaxD * kMaxD];
    double coefScale[kMaxD * kMaxD];        // 1 / legendreNorms
    double legB[kMaxD * kMaxD * kMaxD];     // Taylor-shifted Legendre coefficients
};

constexpr int kMaxRhs = 8;  // right-hand sides of one batched apply

// One mode term of a batched apply (device-side table, one entry per term): the
// mode's cached operators and its K x K mix (rhs i = sum_b mix[i][b] base b).
struct ModeArgs {
    const double* Km2l;   // stored M2L blocks (column-major 16 x 16)
    const double* Knear;  // near-field blocks
    const double* C;      // stencil weights (d2 x 9 x d2)
    const double* mu;     // singular moments
    double sgn;           // (-1)^m: K_{B<-A} = sgn K_{A<-B}^T
    double pad;
    double mix[kMaxRhs][kMaxRhs];
};

// Harmonic weights of a block apply (harmonic.hip): the mixes of
// aniso.m's forward / mforward, out_i = sum_j w_|j| K_|i+j| x_|j|, as hw_b = w_0
// (b = 0) or 2 w_b, dw_i = the mode-0 (diagonal) weight of output i, and om_i = 0
// for an output the mixes leave empty (a padded right-hand side).
struct HarmWeights {
    double hw[kMaxRhs];
    double dw[kMaxRhs];
    double om[kMaxRhs];
};

// One pass of a block operator of more than kMaxRhs blocks: the
// harmonic kernels' offset form takes input blocks b0 .. b0 + 7 to output blocks
// i0 .. i0 + 7 (hw / dw / om hold the pass's 8 weights); multiples of kMaxRhs.
struct HarmWindow {
    int i0, b0;
};

enum StageMask : int {
    kStageFar = 1,      // M2L + L2L + L2P (both kernels)
    kStageNear = 2,     // U/W near field (both kernels)
    kStageStencil = 4,  // nearRemoval + refineAddOn
    kStageSing = 8,     // singularAddOn
    kStageAll = 15,
    kStageForward = 16,  // 16-RHS fp64 operator (f64op.hip): Y = X - K (sigma_s X) instead of Y = K X
};

// ---- views of the plan's device arrays, as the launchers of the un-fused applies take them
// (Operator's accessors build them): one type per argument group, so a
// swapped group does not compile.
// the pair lists of the mode-shared caches (Plan::attPtr / attSrc / attBlk over m2lTgt)
struct PairList {
    int ntgt;
    const int* tgt;
    const int64_t* ptr;
    const int* src;
    const int* blk;
};
struct NodeBoxes {  // per node: centre and half widths
    const double *cx, *cy, *rx, *ry;
};
struct TreePoints {  // the points in tree order
    const double *px, *py;
};
// the directed near lists of the target leaves (maxLeaf: the largest, in points); off: per
// leaf its first stored entry, Plan::nearKOff for the E blocks or nearFOff for resident near blocks
struct NearList {
    int nl, maxLeaf;
    const int4* leafInfo;
    const int64_t* ptsPtr;
    const int* pts;
    const int64_t* off;
};
// The output rows of an apply (Operator::outRows): perm / base place a tree position in `out`
// (perm = the permutation writes the original-order vector out[perm[k]]; perm = nullptr the
// owned tree-order slice out[k - base]), ld = the stride between rows; the last writer stores
// minuend - (...) where minuend is set.
struct OutRows {
    double* out;
    const double* minuend;
    const int* perm;
    int64_t ld, base, minuendLd;
    bool tree;
};

constexpr int kTierThreads = 256;  // workgroup of the down pass tasks
// up pass tasks: 256 threads (P2M holds 16 products per lane, ~94 VGPRs = 5 waves
// per SIMD), so four workgroups fit per CU and 1,024 tasks run in one round
constexpr int kUpThreads = 256;

// ---- apply kernels (apply.hip), batched over K right-hand sides.
// K is a runtime argument dispatched to compiled instances (rhs_supported); the
// operator pads other counts with zero right-hand sides (rhs_padded).  Vectors are
// [K][ld] (rhs-major); tree-order work arrays fT/cT are [N][K], expansions
// [node][16][K].  `mix` is a K x K row-major matrix: the kernels of one mode
// apply it to the base inputs on the fly (rhs i = sum_b mix[i][b] base b).
bool rhs_supported(int k);
int rhs_padded(int k);  // smallest supported count >= k, or -1
int rhs_stride(int k);  // row stride (doubles) of the tree-order charge arrays fT / cT
void launch_prepare(int K, int64_t N, const double* xin, int64_t ldi, int treeIn, const int* perm,
                    const double* sigT, const double* wT, double* fT, double* cT, hipStream_t s);
size_t up_tier_lds(int maxTask, int K);
size_t down_tier_lds(int maxTask, int maxLeaves, int maxNear, int maxChain, int K);
// taskList (nullptr: tasks taskBase .. taskBase + ntask - 1): the tasks to run.
// Sharded applies (all may be null): rootSlot / recv -- children that
// are tier-0 roots with a slot are read from the all-gathered records recv (and
// stored to mult for the M2L); sendSlot / send -- a task root with a send slot also
// stores its record into this rank's all-gather buffer.
void launch_up_tier(int K, int ntask, int taskBase, const int* taskList, int maxTask, const int4* desc,
                    const int* grpFix, const int* node, const int4* code, const double4* geom, const int2* leafRange,
                    const double* pxT, const double* pyT, const double* xin, int64_t ldi, int treeIn, const int* perm,
                    const double* sigT, const double* wT, double* fT, double* cT, const Params* P, double* mult,
                    const int* rootSlot, const double* recv, const int* sendSlot, double* send, hipStream_t s,
                    unsigned* zeroCnt = nullptr);
// config 5's fp32 operator (f32op.hip): node expansions as 64 lanes x float4
// (void* below), vectors point-major N x 16 floats
void launch32_p2m(int nleaf, const int* leaves, const int64_t* begin, const int64_t* count, const double* ncx,
                  const double* ncy, const double* nrx, const double* nry, const double* pxT, const double* pyT,
                  const float* X, const double* sigT, const double* wT, const Params* P, void* mult, float* fT,
                  float* cT, hipStream_t s);
void launch32_m2m(int nn, const int* nodes, const int4* child, const int64_t* count, const void* Rup, void* mult,
                  hipStream_t s);
void launch32_m2l(int ntgt, const int* tgt, const int64_t* ptr, const int* src, const void* K32, const void* mult,
                  void* local, hipStream_t s);
void launch32_l2l(int nn, const int* nodes, const int* parent, const int* slot, const void* Rdn, void* local,
                  hipStream_t s);
void launch32_leaf(int nleaf, const int4* leafInfo, const int64_t* nearPtr, const int* nearPts, const int64_t* koff,
                   const void* Knear, const int* level, const double* ncx, const double* ncy, const double* nrx,
                   const double* nry, const double* pxT, const double* pyT, const Params* P, const void* local,
                   const float* fT, const float* X, float scale, int flags, float* Y, hipStream_t s);
void launch32_corr(int d, int64_t N, const int* perm, const int* iperm, const float* cT, const float* fT,
                   const double* C, const double* mu, const Params* P, int flags, float scale, float* Y,
                   hipStream_t s);
void launch32_conv_m2l(int64_t npairs, const double* Kd, void* K32, hipStream_t s);
void launch32_conv_near(int nl, const int4* info, const int64_t* koffD, const int64_t* koff, const int* srcCount,
                        const double* Kd, void* K32, hipStream_t s);
// the fp64 16-right-hand-side operator on MFMA (f64op.hip): the same plan and
// layouts as the fp32 one, expansions as 64 lanes x 4 doubles
void launch64_p2m(int nleaf, const int* leaves, const int64_t* begin, const int64_t* count, const double* ncx,
                  const double* ncy, const double* nrx, const double* nry, const double* pxT, const double* pyT,
                  const double* X, const double* sigT, const double* wT, const Params* P, void* mult, double* fT,
                  double* cT, hipStream_t s);
void launch64_m2m(int nn, const int* nodes, const int4* child, const int64_t* count, const void* Rup, void* mult,
                  hipStream_t s);
void launch64_m2l(int ntgt, const int* tgt, const int64_t* ptr, const int* src, const void* K64, const void* mult,
                  void* local, hipStream_t s);
void launch64_l2l(int nn, const int* nodes, const int* parent, const int* slot, const void* Rdn, void* local,
                  hipStream_t s);
void launch64_leaf(int nleaf, const int4* leafInfo, const int64_t* nearPtr, const int* nearPts, const int64_t* koff,
                   const void* Knear, const int* level, const double* ncx, const double* ncy, const double* nrx,
                   const double* nry, const double* pxT, const double* pyT, const Params* P, const void* local,
                   const double* fT, const double* X, double scale, int flags, double* Y, hipStream_t s);
void launch64_corr(int d, int64_t N, const int* perm, const int* iperm, const double* cT, const double* fT,
                   const double* C, const double* mu, const Params* P, int flags, double scale, double* Y,
                   hipStream_t s);
void launch64_lane_major(int64_t npairs, double* K, hipStream_t s);
void launch64_conv_near(int nl, const int4* info, const int64_t* koffD, const int64_t* koff, const int* srcCount,
                        const double* Kd, void* K64, hipStream_t s);
void launch64_gather16(int64_t N, int k, const int* perm, const double* Q, double* X16, hipStream_t s);
void launch64_scatter16(int64_t N, int k, const int* perm, const double* Y16, double* Out, hipStream_t s);
// the tier-0 root records of a sharded apply without upper tiers, scattered back
// from the all-gather (mult[nodes[j]] = recv[j] where nodes[j] >= 0)
void launch_roots_unpack(int K, int nslots, const int* nodes, const double* recv, double* mult, hipStream_t s);
// All terms in one launch: local = sum over the terms (stored), transposed
// canonical products summed over the terms into their partial slots (stored).
void launch_m2l(int K, int ntgt, const int* tgt, const int64_t* ptr, const int* nDir, const int* canonBase,
                const int* outSlot, const int* src, const ModeArgs* tab, int nterm, const double* mult, int maxCanon,
                double* partial, double* local, hipStream_t s);
void launch_m2l_gather(int K, int ntgt, const int* tgt, const int* inPtr, const double* partial, double* local,
                       hipStream_t s);
// Output index mode of k_near / k_down_tier / k_corr: operm = perm writes the
// original-order vector out[perm[k]]; operm = nullptr writes the owned tree-order
// slice out[k - obase].  ldo = the stride between right-hand sides of out.
// near field with symmetric U storage (K = 1 handles): partial products to `partial`
void launch_near_sym(int K, int nl, const int4* leafInfo, const int64_t* nearPtsPtr, const int* nearPts,
                     const int64_t* nearKOff, const int2* nearSym, const double* Kop, const double* fT,
                     const double* mix, const int* operm, int64_t obase, int64_t ldo, int maxS, int flags, double sgn,
                     double scale, int accum, double* partial, double* out, hipStream_t s);
// near field with directed storage, all terms in one launch (out stored, or added
// with accum); maxLeaf = the largest target leaf (points)
void launch_near(int K, int nl, int maxLeaf, const int4* leafInfo, const int64_t* nearPtsPtr, const int* nearPts,
                 const int64_t* nearKOff, const ModeArgs* tab, int nterm, const double* fT, const int* operm,
                 int64_t obase, int64_t ldo, int flags, double scale, int accum, double* out, hipStream_t s);
void launch_down_tier(int K, int ntask, int maxTask, int maxLeaves, const int4* desc, const int* grpFix,
                      const int4* dn, const double* local, const Params* P, const int* leafSlot, const int* leafBegin,
                      const int2* leafNear, const double4* leafGeom, const double* pxT, const double* pyT,
                      const int* operm, int64_t obase, int64_t ldo, const int* nearOff, int maxNear,
                      const double* nearPart, const int2* chain, int maxChain, int flags, double scale, double* out,
                      const double* xsub, int64_t ldx,
                      hipStream_t s, const double* hpart = nullptr, const int* chainFold = nullptr);
// corrections of all terms in one launch, added to out: Wc / Wm the terms'
// stencil and singular tables folded with their mixes (Operator::corrTable)
void launch_corr(int K, int d, int64_t b, int64_t e, const int* perm, const int* iperm, const double* cT,
                 const double* fT, const double* Wc, const double* Wm, const Params* P, int flags, double scale,
                 bool treeOut, int64_t ldo, double* out, hipStream_t s);
// harmonic block apply (harmonic.hip): all modes from the mode-shared E caches
void launch_m2l_hm(int K, const PairList& pl, const double* E, const NodeBoxes& b, const Params* P,
                   const HarmWeights& hw, const double* mult, double* local, hipStream_t s,
                   const HarmWindow* win = nullptr);  // win: the offset form (K = 8)
// the clustered M2L's arguments (harmonic.hip k_m2l_hc, k_top_m2l_hc)
struct HcArgs {
    const int* clPtr;
    const int* tgt;
    const int64_t* ptr;
    const int* ndir;
    const int* src;
    const int* blk;
    const int* slot;
    const double* E;
    const double* ncx;
    const double* ncy;
    const double* nrx;
    const double* nry;
    const Params* P;
    HarmWeights hw;
    const double* mult;
    double* local;
    // the halo form (Plan::hmHaloPtr): cluster c's halo slots h = haloPtr[c] ..
    // haloPtr[c+1] - 1 go to partial haloPos[h] of hpart (16 x K doubles each, stored
    // scaled, receiver-contiguous: the down pass adds them to the locals)
    const int* haloPtr = nullptr;
    const int* haloPos = nullptr;
    double* hpart = nullptr;
    // the deterministic sums (k_m2l_hc only): per node the bound W of
    // its weighted multipole (k_node_wmax), per cluster the host's geometric bound, the
    // largest stored E (device scalar).  wmax == nullptr: the ds_add_f64 sums
    const double* wmax = nullptr;
    const double* clBound = nullptr;
    const double* emax = nullptr;
};
// The fused top-of-tree + clustered M2L launch (harmonic.hip k_top_m2l_hc, DESIGN.md
// §3.10): blocks 0 .. nUp - 1 run the up tasks of tiers 1 .. ntier - 1 (tier k's
// tasks wait until tier k - 1 has finished), the other blocks are the clusters, a
// cluster whose sources include upper-tier multipoles waiting for that tier.
constexpr int kMaxTopTiers = 8;
struct UpArgs {  // one up task's inputs (up_task.hpp)
    int maxTask;
    const int4* desc;
    const int* grpFix;
    const int* node;
    const int4* code;
    const double4* geom;
    const int2* leafRange;
    const double* pxT;
    const double* pyT;
    const double* xin;
    int64_t ldi;
    int treeIn;
    const int* perm;
    const double* sigT;
    const double* wT;
    double* fT;
    double* cT;
    const Params* P;
    double* mult;
    const int* rootSlot;
};
struct TopArgs {
    int nUp;                      // up-task blocks
    int ntier;                    // tiers 1 .. ntier - 1 run in the launch
    int blk0[kMaxTopTiers + 1];   // first block of tier k; blk0[ntier] = nUp
    int task0[kMaxTopTiers];      // first task of tier k
    const int* clWait;            // per cluster: the upper tier it waits for (0: none)
    unsigned* cnt;                // finished tasks per tier (zeroed by tier 0)
    const double* recv1;          // sharded phase 2: the gathered tier-0 roots tier 1 reads
    unsigned spinLimit;           // polls of a tier's counter before the waiting block computes the tier itself
                                  // (0: at once -- tests only)
    unsigned* steals;             // persistent count of tier tasks computed by a waiting block (aniso_stats)
    unsigned* err;                // host-visible sticky flag (kept for the ABI; the launch no longer sets it)
    int64_t* trace;               // development (ANISO_TOP_TRACE=1): per block {start, waited, end, hw id}
};
// the fused corrections of the staged near field (d = 1; harmonic.hip k_near_hs)
struct NearCorr {  // the fused corrections of k_near_hs (d = 1), or ignored when rows == nullptr
    const uint16_t* rows;
    const int* perm;
    const int* iperm;
    const double* cT;
    const double* Wc;
    const double* Wm;
    const Params* P;
};
// the staged near field's arguments (harmonic.hip k_near_hs): 16 leaves per group
struct NearHsArgs {
    int nl;                  // target leaves
    int nsMax;               // largest source table (rows)
    const int4* leafInfo;
    const int64_t* nearPtsPtr;
    const uint16_t* nearLoc;
    const int64_t* nsPtr;
    const int* nsPts;
    const int64_t* nearKOff;
    const double* E;
    const double* pxT;
    const double* pyT;
    const double* sigDiag;
    HarmWeights hw;
    const double* fT;
    const int* operm;
    int64_t obase;
    int64_t ldo;
    int flags;
    double scale;
    double* out;
    NearCorr nc;
    // charges from the apply's input (xin != nullptr): f = x sigma_s w and c = x
    // sigma_s formed here (as up_task does), so the near field needs nothing from the
    // up pass and can run beside it; else fT / cT (and nc.cT) as the up pass wrote them
    const double* xin = nullptr;
    int64_t ldi = 0;
    int treeIn = 0;
    const int* perm = nullptr;
    const double* sigT = nullptr;
    const double* wT = nullptr;
    // the 16-leaf groups to run (ngrp of them; nullptr: all, in order): a sharded
    // apply's one-collective form runs the groups that read only the own range before
    // the exchange and the rest after it (Plan::nearGrpEarly / nearGrpLate)
    const int* grpList = nullptr;
    int ngrp = 0;
    // the bottom up tier in the staged near field (one GPU, serial schedule;
    // Plan::nearUpGrp): every 16-leaf group is one tier-0 subtree (its
    // 16 leaves, their 4 parents, the root).  Its lanes form the leaves' P2M from the
    // charges the epilogue loads, the workgroup the subtree's M2M, into upMult (the
    // multipoles of an up tier; the tier launch is skipped).  upGrp: per group
    // kNearUpInts ints -- per leaf (parent slot << 2 | quadrant), per parent its
    // quadrant, the 4 parent nodes, the root node.  zeroCnt: the fused top-of-tree
    // launch's counters, zeroed here instead of by the skipped tier launch.
    double* upMult = nullptr;
    const int* upGrp = nullptr;
    const Params* upP = nullptr;
    const double* upNcx = nullptr;
    const double* upNcy = nullptr;
    const double* upNrx = nullptr;
    const double* upNry = nullptr;
    unsigned* zeroCnt = nullptr;
};
constexpr int kNearUpInts = 25;
// LDS the fused up tail needs in the group's table region (doubles): 256 points x
// (8 Chebyshev weights + K charges), then the 4 parents' 16 x K
inline size_t near_up_lds_doubles(int K) { return (size_t)256 * (8 + K) + 4 * 16 * K; }
bool top_fused_enabled();
void launch_top_m2l_hc(int K, int ncl, int maxCl, const UpArgs& u, const TopArgs& t, const HcArgs& a, hipStream_t s);
// whether launch_near_hm would run the staged near field with fused corrections
bool near_hs_fusable(int nl, int maxLeaf, int nsMax, const uint16_t* nearLoc, const NearCorr* corr, int flags);
void launch_m2l_hc(int K, int ncl, int maxCl, const HcArgs& a, hipStream_t s);
// the deterministic cluster sums' bounds: out[n] = max over node n's 16 columns of
// sum_b |hw_b mult_b|; out[0] = max |x|
void launch_node_wmax(int K, int nnodes, const double* mult, const HarmWeights& hw, double* out, hipStream_t s);
void launch_abs_max(int64_t n, const double* x, double* out, hipStream_t s);
// returns true when the corrections were fused (the caller skips launch_corr)
bool launch_near_hm(int K, const NearList& list, const double* E, const TreePoints& pts, const double* sigDiag,
                    const HarmWeights& hw, const double* fT, int flags, double scale, const OutRows& o,
                    const uint16_t* nearLoc, const int64_t* nsPtr, const int* nsPts, int nsMax, const NearCorr* corr,
                    hipStream_t s,
                    const NearHsArgs* in = nullptr,  // in->xin: the staged kernel's charges from the input
                    const HarmWindow* win = nullptr);  // win: the offset form (K = 8)
// out[i] = a[i] (add == 0) or out[i] += a[i], rows i < nrhs of n entries: the sum over a block operator's passes
void launch_add_rows(int64_t n, int nrhs, const double* a, int64_t lda, double* out, int64_t ldo, int add,
                     hipStream_t s);
void launch_sub_slice(int64_t n, int nrhs, const double* x, int64_t ldx, const double* a, int64_t lda, double* y,
                      int64_t ldy, hipStream_t s);

// ---- high-order handles (high_order.hip): np = 6 or 8, rank R = np^2.
// The order-dependent tables, apart from the rank-16 Params: the Chebyshev nodes,
// T_l(c_i) at [i + l np], and the 1-D transfer S[b][c np + p] = the weight of parent node
// p at child node c of half b (M2M / L2L apply S[y half] (x) S[x half] as two transforms).
constexpr int kMaxNP = 8;
struct HoTables {
    double cheb[kMaxNP];
    double tnode[kMaxNP * kMaxNP];
    double S[2][kMaxNP * kMaxNP];
};
void ho_tables(int np, HoTables* t);  // host
// E[pair][s][t] = e^-tau between the pair's Chebyshev nodes (R x R doubles per stored pair)
void launch_ho_cache_att(int np, int64_t npairs, const int* pairTgt, const int* src, const NodeBoxes& b,
                         const double* stcoef, const Params* P, const HoTables* T, double* E, hipStream_t s);
// expansions [node][R][K]; leafInfo as Plan::leafInfo; fT from launch_prepare
void launch_ho_p2m(int np, int K, int nl, const int4* leafInfo, const NodeBoxes& b, const TreePoints& pts,
                   const double* fT, const HoTables* T, double* mult, hipStream_t s);
// one level: child[n] = the four children of node n (< 0: empty, contributes nothing)
void launch_ho_m2m(int np, int K, int nn, const int* nodes, const int4* child, const HoTables* T, double* mult,
                   hipStream_t s);
// the pair lists of the mode-shared plan (Plan::attPtr / attSrc / attBlk over m2lTgt);
// win: the offset form (K = 8); local = om_i x the unscaled sums, as k_m2l_hm stores them
void launch_ho_m2l(int np, int K, const PairList& pl, const double* E, const NodeBoxes& b, const HoTables* T,
                   const HarmWeights& hw, const HarmWindow* win, const double* mult, double* local, hipStream_t s);
// one level, top-down: local[n] += L2L of its parent's (complete) local
void launch_ho_l2l(int np, int K, int nn, const int* nodes, const int* parent, const int* slot, const HoTables* T,
                   double* local, hipStream_t s);
// out += scale * L2P (o.minuend: out = minuend - (out + scale * L2P)), output modes as k_down_tier
void launch_ho_l2p(int np, int K, int nl, const int4* leafInfo, const NodeBoxes& b, const TreePoints& pts,
                   const HoTables* T, const double* local, double scale, const OutRows& o, hipStream_t s);
// ---- one mode on K columns on the mode-shared caches (mode_apply.hip): a
// high-order handle, or a lean mode of an np = 4 one.  K in {2, 4, 5, 8}, the entry's factor
// (E / r) T_id(c) formed once for all K columns.
// launch_near_hm's unstaged kernel for mode id: out (stored) = scale * (near field + the
// sigma_t diagonal when id = 0); fT from launch_prepare
void launch_near_mode(int K, int id, const NearList& nl, const double* E, const TreePoints& pts,
                      const double* sigDiag, const double* fT, double scale, const OutRows& o, hipStream_t s);
// launch_ho_m2l for mode id: mult as launch_ho_p2m / _m2m leave it, local = the plain sums
void launch_ho_m2l_mode(int np, int K, int id, const PairList& pl, const double* E, const NodeBoxes& b,
                        const HoTables* T, const double* mult, double* local, hipStream_t s);
// the same for 8 + KB columns with one factor formation per entry:
// columns 0 .. 7 from multA / to localA ([node][R][8]), 8 .. 8+KB-1 from multB / to localB
// ([node][R][KB]), KB = 2, 4, 5 or 8; a column's bits are launch_ho_m2l_mode's
void launch_ho_m2l_mode_wide(int np, int KB, int id, const PairList& pl, const double* E, const NodeBoxes& b,
                             const HoTables* T, const double* multA, const double* multB, double* localA,
                             double* localB, hipStream_t s);
// The resident per-mode blocks of a high-order handle (mode_resident.hip):
// F[pair] = (E / r) T_id(c) of every stored pair (owner / other: its target and source node),
// R x R doubles per pair in 4 x 4 microtiles, and launch_ho_m2l_mode on them as an fp64 MFMA
// product for 16 columns: columns 0 .. KA-1 from multA / to localA ([node][R][KA]), columns
// 8 .. 8+KB-1 from multB / to localB (KB = 0: none), 1 <= KA <= 8, 0 <= KB <= 8.
void launch_ho_mode_blocks(int np, int id, int64_t npairs, const int* owner, const int* other, const double* E,
                           const NodeBoxes& b, const HoTables* T, double* F, hipStream_t s);
void launch_ho_m2l_resident(int np, int id, const PairList& pl, const double* F, const double* multA, int KA,
                            const double* multB, int KB, double* localA, double* localB, hipStream_t s);
// The resident near blocks of one mode (mode_near_resident.hip):
// F = mode_factor<true> of every stored entry of the directed near E blocks, per leaf at
// nearFOff in 16-row tiles of 4 x 4 microtiles (rows padded to 4, sources to 16, the padding
// zero), and launch_near_mode on them as an fp64 MFMA product for 16 columns: columns
// 0 .. KA-1 from fTA ([tree position][kStride<KA>]) to oA, columns 8 .. 8+KB-1 from fTB to
// oB (KB = 0: none, oB = OutRows{}; oA's perm and base place both), KA and KB in {2, 4, 5, 8}.
// out (stored) as launch_near_mode's.  launch_near_mode_blocks: nl.off = nearKOff, the E blocks'.
void launch_near_mode_blocks(int id, const NearList& nl, const int64_t* nearFOff, const double* E,
                             const TreePoints& pts, double* F, hipStream_t s);
void launch_near_resident(int id, const NearList& nl, const double* F, const double* sigDiag, const double* fTA,
                          int KA, const double* fTB, int KB, double scale, const OutRows& oA, const OutRows& oB,
                          hipStream_t s);
// The reduced-precision operator of a high-order handle (mode_apply_f32.hip, DESIGN.md
// §3.18.5): both E arrays rounded to float with the same indexing (one launch), and
// launch_near_mode / launch_ho_m2l_mode on the mirrors with the factor, the products and the
// accumulators in fp32 (the boxes: the near field takes its points relative to the target
// leaf's centre).  Charges, multipoles, locals and `out` stay double.
void launch_cache_f32(int64_t na, const double* a, float* af, int64_t nb, const double* b, float* bf, hipStream_t s);
void launch_near_mode_f32(int K, int id, const NearList& nl, const float* E, const NodeBoxes& b,
                          const TreePoints& pts, const double* sigDiag, const double* fT, double scale,
                          const OutRows& o, hipStream_t s);
void launch_ho_m2l_mode_f32(int np, int K, int id, const PairList& pl, const float* E, const NodeBoxes& b,
                            const HoTables* T, const double* mult, double* local, hipStream_t s);
// The relaxed-precision block operator of a high-order handle (block_f32.hip, DESIGN.md
// §3.18.8): launch_near_hm's unstaged kernel (whole operator, near field on) and
// launch_ho_m2l (no window) on the same mirrors, the entry of all K modes in fp32.
void launch_near_hm_f32(int K, const NearList& nl, const float* E, const NodeBoxes& b, const TreePoints& pts,
                        const double* sigDiag, const HarmWeights& hw, const double* fT, double scale,
                        const OutRows& o, hipStream_t s);
void launch_ho_m2l_f32(int np, int K, const PairList& pl, const float* E, const NodeBoxes& b, const HoTables* T,
                       const HarmWeights& hw, const double* mult, double* local, hipStream_t s);
// launch_m2l_hm for mode id on a rank-16 (np = 4) handle: mult [node][16][K] as the up tiers
// leave it, local = the plain sums of every listed target (the down tiers read them as they
// are); ntgt = 0 launches nothing.  A column's bits do not depend on K or on its slot.
void launch_m2l_mode16(int K, int id, const PairList& pl, const double* E, const NodeBoxes& b, const Params* P,
                       const double* mult, double* local, hipStream_t s);
// ---- the block operator for S sources per read of the E blocks (block_multi.hip, DESIGN.md
// §3.18.3): launch_ho_m2l (whole operator, no window) on S in {1, 2, 4} multipole buffers
// mult + j * mstride into S local buffers local + j * lstride, each [node][R][K].  A
// source's bits do not depend on S or on its slot.
void launch_ho_m2l_src(int np, int K, int S, const PairList& pl, const double* E, const NodeBoxes& b,
                       const HoTables* T, const HarmWeights& hw, const double* mult, int64_t mstride, double* local,
                       int64_t lstride, hipStream_t s);
// The same launch with the entry in fp32 on the float mirror of E (block_multi_f32.hip,
// DESIGN.md §3.18.10): a source's local expansion is launch_ho_m2l_f32's, bit for bit.
void launch_ho_m2l_src_f32(int np, int K, int S, const PairList& pl, const float* E, const NodeBoxes& b,
                           const HoTables* T, const HarmWeights& hw, const double* mult, int64_t mstride,
                           double* local, int64_t lstride, hipStream_t s);

// ---- cache build and helpers (kernels.hip)
void launch_cache_m2l(int64_t npairs, const int* pairTgt, const int* src, const NodeBoxes& b, const double* stcoef,
                      const Params* P, int mode, double* K, hipStream_t s);
void launch_cache_near(int nl, const int* leaves, const int64_t* nearPtr, const int* nearSrc, const int64_t* nearKOff,
                       const int64_t* begin, const int64_t* count, const TreePoints& pts, const double* stcoef,
                       const Params* P, int mode, int maxSrc, double* K, hipStream_t s);
// mode-shared cache: pair_kernel's mode argument kAttMode gives
// e^-tau alone (0 at r = 0); launch_cache_near takes it as well
constexpr int kAttMode = -1;
void launch_cache_att_m2l(int64_t npairs, const int* pairTgt, const int* src, const NodeBoxes& b,
                          const double* stcoef, const Params* P, double* E, hipStream_t s);
void launch_sigma_diag(int64_t N, const double* pxT, const double* pyT, const double* stcoef, const Params* P,
                       double* out, hipStream_t s);
void launch_permute(int64_t N, const int* perm, const double* orig, double* tree, hipStream_t s);
// halo exchange of an nb-block vector (comm.hpp): element j of a position list goes
// to / comes from buf[base[j] + b * stride[j]] for block b, vector entry x[b * ldx + pos[j]]
void launch_halo_pack(int64_t n, int nb, const int64_t* pos, const int64_t* base, const int64_t* stride,
                      const double* x, int64_t ldx, double* buf, hipStream_t s);
void launch_halo_unpack(int64_t n, int nb, const int64_t* pos, const int64_t* base, const int64_t* stride,
                        const double* buf, double* x, int64_t ldx, hipStream_t s);
// the gathered input of a sharded high-order matvec.  pack: the own slice xo
// (own positions of nb rows at stride ldx) into one contiguous part, row b at b * stride
// (stride >= own: the largest owned count of any rank).  unpack: parts p0 .. p1 - 1 of buf
// (part p at p * nb * stride), all but `skip`, into [cuts[p], cuts[p + 1]) of the rows of x.
// Zero-size launches (a rank or a peer that owns nothing) are skipped.
void launch_slice_pack(int64_t own, int nb, const double* xo, int64_t ldx, int64_t stride, double* buf,
                       hipStream_t s);
void launch_slice_unpack(int p0, int p1, int skip, const int64_t* cuts, int nb, int64_t stride, const double* buf,
                         double* x, int64_t ldx, hipStream_t s);
// the one-collective exchange's pack (send) or unpack (receive) in one launch: root
// records (nRoot parts of rec doubles at rootOff in buf; unpack: to rootDst in roots,
// and this rank's own record from ownRoots), input positions (pos / base / stride as
// the halo exchange, nb blocks of x), multipole rows (node / nodeBase, len doubles)
struct OxArgs {
    int64_t nRoot = 0, rec = 0;
    const int64_t* rootOff = nullptr;
    const int64_t* rootDst = nullptr;
    double* roots = nullptr;           // pack: this rank's records (read); unpack: the slot layout (written)
    const double* ownRoots = nullptr;  // unpack: this rank's records, copied to its own slot
    int64_t ownDst = 0;
    int64_t nPts = 0;
    int nb = 0;
    const int64_t* pos = nullptr;
    const int64_t* base = nullptr;
    const int64_t* stride = nullptr;
    double* x = nullptr;
    int64_t ldx = 0;
    int64_t nNode = 0;
    int len = 0;
    const int* node = nullptr;
    const int64_t* nodeBase = nullptr;
    double* mult = nullptr;
    double* buf = nullptr;
    // unpack, the upper multipoles as partial sums (Plan::xUpPartial): node sumNode[j]
    // = the sum of its records sumSrc[sumPtr[j] .. sumPtr[j + 1]) in that order (>= 0:
    // offset into buf, < 0: ~offset into ownRec), len doubles each
    int64_t nSum = 0;
    const int* sumNode = nullptr;
    const int* sumPtr = nullptr;
    const int64_t* sumSrc = nullptr;
    const double* ownRec = nullptr;
};
void launch_ox(const OxArgs& a, bool pack, hipStream_t s);
void launch_spin_us(int us, int blocks, hipStream_t s);  // development: a stand-in exchange latency
// the pack launch with the upper multipoles as partial sums (apply.hip k_ox_pack_up):
// one workgroup per task of Plan::xUpTask (kUpTaskInts ints each) stores its records
// into rec and into each of nPeer parts at peerOff (doubles into a.buf), the rest pack
// a's input positions and multipole rows (a.nRoot must be 0)
void launch_ox_pack_up(int K, int ntask, const int* task, const double* mult, const Params* P, double* rec,
                       int nPeer, const int64_t* peerOff, const OxArgs& a, hipStream_t s);


// ---- direct evaluation at chosen targets (direct.hip)
// One launch: targets tg[t0 .. t0 + ntl) (original indices, device) against all N
// sources, the live output rows of one window.  Input rows x[b * ldx + original index],
// b < nb, weighted by hw[b]; output row r of the window has Chebyshev degree m0 + r, the
// r = 0 weight dw[r] on input row drow0 + r, and goes to out[(orow0 + r) * ldo + t] as
//   scale * sum + corr[(crow0 + r) * ldc + tg[t]],  or minuend[(orow0 + r) * ldm + tg[t]] - that.
struct DirectArgs {
    int64_t N = 0;
    int nb = 0, m0 = 0, drow0 = 0, nout = 0, orow0 = 0, crow0 = 0;
    const double* x = nullptr;
    int64_t ldx = 0;
    const double* hw = nullptr;  // device, nb entries
    const double* dw = nullptr;  // device, nout entries
    const int* perm = nullptr;
    const int* iperm = nullptr;
    const double* sigT = nullptr;  // sigma_s in tree order, or nullptr
    const double* wT = nullptr;
    const double* pxT = nullptr;
    const double* pyT = nullptr;
    const double* stcoef = nullptr;
    const Params* P = nullptr;
    const int64_t* tg = nullptr;
    int64_t t0 = 0;
    double* part = nullptr;  // ntl x direct_blocks(N) x KO doubles
    double scale = 0.0;
    const double* corr = nullptr;
    int64_t ldc = 0;
    const double* minuend = nullptr;
    int64_t ldm = 0;
    double* out = nullptr;
    int64_t ldo = 0;
};
int64_t direct_blocks(int64_t N);  // source blocks (partials per target and row)
int direct_rows(int nout);         // the compiled window (1, 2, 4, 8, 16, 32) holding nout rows, at most 32
void launch_direct(int KO, int ntl, const DirectArgs& a, hipStream_t s);

// host-callable device helpers used by tests through the C ABI
void launch_line_integrals(int n, const double* seg, const double* stcoef, const Params* P, double* out,
                           hipStream_t s);

}  // namespace aniso
