// aniso_op.hpp -- the MI355X operator behind the C ABI (one per handle).
//
// Host state (geometry, tree, plan) is built by the constructor without touching
// the GPU; device buffers are created on first use (setCoeff), on the HIP device
// that is current at that moment.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <map>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "comm.hpp"
#include "host.hpp"
#include "kernels.hpp"

namespace aniso {

int64_t arn_state_doubles(int m);  // the Arnoldi state block of restart length m (arnoldi.hpp)
// the 16-column Arnoldi's state blocks and sweep partials at restart m (arnoldi16.hpp), in doubles
void arn16_work_doubles(int m, int64_t* state, int64_t* part);

struct StatusBlock;  // gmres_driver.hpp: what the solves of solver.hip share
struct GmresSystem;
struct ColsWork;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~DevBuf();
    void alloc(size_t nbytes);
    void upload(const void* host, size_t nbytes);
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

struct ModeCache {
    DevBuf Knear, Km2l, C, mu;
    std::vector<double> hostC, hostMu;  // the correction tables (folded per batched apply)
    // two readiness notions: the correction tables C / mu are built
    // (enough for the harmonic block apply and its passes, which read the mode-shared
    // caches), and the mode's own operators Km2l / Knear are built (everything that
    // streams them).  resident implies tables; setCoeff clears both.
    bool tables = false, resident = false;
};

// Correction tables of one batched apply: every term's stencil / singular table
// folded with its mix (launch_corr).
struct CorrFold {
    DevBuf Wc, Wm;
};

struct StageTimes {
    float exch = 0, up = 0, m2l = 0, gather = 0, near = 0, down = 0, corr = 0, total = 0;
};

// The exchange form of a one-collective sharded matvec, filled in by
// shardedExchange for the applies of its two phase callbacks.
struct ExchangeForm {
    bool oneX = false;       // the two phases run around the one grouped exchange
    bool upPartial = false;  // the upper multipoles travel as partial sums (Plan::xUpPartial on every rank)
};

// The precision of an apply's M2L and near field on a high-order handle (an argument of
// modeApplyDev and a member of ApplyCall, not Operator state): F32 runs mode_apply_f32.hip
// (one mode) or block_f32.hip (the block operator) on the float mirrors.
enum class ApplyPrec { F64, F32 };

// Everything about one applyBlock call that is not the operator's state (default: a
// whole apply, no pass, no exchange).
struct ApplyCall {
    // phase 0: the whole apply (input valid everywhere, every up task); 1 / 2: the
    // two halves of a sharded apply (forwardTreeBegin / End); 3: phase 2 again for
    // another output window of a sharded pass (blockOpShardedPasses), on the
    // multipoles already in dMult: no unpack, no upper tier
    int phase = 0;
    double* rootsSend = nullptr;        // phase 1: this rank's tier-0 root records
    const double* rootsRecv = nullptr;  // phase 2: every rank's
    void phased(int ph, double* send, const double* recv) { phase = ph; rootsSend = send; rootsRecv = recv; }
    // x - mforward(x) fused into the down pass (blockOpDev, which = 2): x at the output positions
    const double* minuend = nullptr;
    int64_t minuendLd = 0;
    // one pass of a block operator of more than kMaxRhs blocks, or a lean mapping
    // (blockPass, leanMapping, blockOpShardedPasses): its window and harmonic weights
    bool pass = false;
    HarmWindow win{0, 0};
    HarmWeights hw{};
    bool shardedPass = false;  // inside blockOpShardedPasses: phase 2 keeps the pending state for its repeats
    // the apply of a sharded high-order matvec (blockOpShardedHigh, blockOpDev in tree order):
    // the only applies a handle made by createSharded at np = 6, 8 runs
    bool hoShard = false;
    // F32: the M2L and the unstaged near field of a high-order handle on the float mirrors
    // (blockOpF32Dev and the relaxed block solve; the caller has built the mirrors)
    ApplyPrec prec = ApplyPrec::F64;
    ExchangeForm exch;
};

// The K input rows of an apply (tree: in tree order; sigT: sigma_s in tree order, multiplied
// into the charges, or nullptr); its output rows are kernels.hpp's OutRows (Operator::outRows).
struct InRows {
    const double* x;
    int64_t ld;
    bool tree;
    const double* sigT;
};
// One half of a mode chunk on a high-order handle (Operator::modeChunkHigh): K compiled columns
struct ModeHalf {
    int K;
    InRows in;
    OutRows o;
};

// The resident factor blocks of one kind per mode id (Operator::cacheMode / cacheModeNear)
struct ResidentBlocks {
    std::map<int, DevBuf> blocks;
    const double* find(int id) const {  // nullptr: mode id has none
        const auto it = blocks.find(id);
        return it == blocks.end() ? nullptr : it->second.as<double>();
    }
    void free(int id);  // id = -1: all
    int64_t bytes() const;
};

class Operator {
public:
    // shardRank / shardRanks: the shard of a handle made by aniso_create_sharded at np = 6, 8
    // (shardRanks = 0: a plain handle; np = 4 ignores them, its shard is set by setShard;
    // the entry point checks the pair, and Plan::build once more)
    Operator(int sz, int d, int ks, double g, int ns, int np, int maxLevel, int shardRank = 0, int shardRanks = 0);
    ~Operator();

    // --- the reference's MEX ops (AnisoWrapper.cpp:10-136)
    int64_t numNodes() const { return geo.N; }
    void getNodes(double* xy) const;
    void setCoeff(const double* sigma_s, const double* sigma_t);
    void cache(int id);
    // every mode made ready for the block operator on the mode-shared caches, without
    // per-mode operators (a lean handle)
    void cacheBlock();
    // device bytes of the operator caches: per-mode Km2l + Knear over all modes, the
    // mode-shared caches
    void cacheBytes(int64_t bytes[2]) const;
    // float mirrors of the mode-shared caches' M2L blocks and directed near blocks (same
    // indexing), read by the f32 mode applies of a high-order handle.  They
    // live until setCoeff, a rebuild of the shared caches or the handle's end; the f32 applies
    // build them on first use.  cacheF32Bytes: their device bytes, 0 when there are none.
    void cacheF32();
    int64_t cacheF32Bytes() const { return (int64_t)(dAttM2LF.bytes + dAttNearF.bytes); }
    // one mode's resident factor blocks on a high-order handle (np = 6, 8; mode_resident.hip,
    // DESIGN.md §3.18.6): F_id = (E / r) T_id(c) of every stored pair, indexed as the E blocks
    // and as large as they are, built in one launch.  While mode id is resident the fp64 mode
    // applies run the MFMA M2L on them, up to 16 columns per chunk.  Several modes may be
    // resident; they live until cacheModeFree (id = -1: all), setCoeff, a rebuild of the shared
    // caches or the handle's end.  cacheModeBytes: their device bytes over all modes.
    void cacheMode(int id);
    void cacheModeFree(int id);
    int64_t cacheModeBytes() const;
    // one mode's resident near-field factor blocks on a high-order handle (np = 6, 8;
    // mode_near_resident.hip): F_id = (E / r) T_id(c) of every stored entry
    // of the directed near E blocks, in 16-row tiles of 4 x 4 microtiles at Plan::nearFOff,
    // built in one launch.  While mode id is near-resident the fp64 mode applies run the MFMA
    // near field on them for a full 8-column chunk (2, 4 and 5 columns keep k_near_mode: no
    // gain measured on mode 0), and a 16-column chunk (which exists while the M2L blocks of
    // cacheMode are resident too, or with setWide(1)) runs one near launch for all its columns.  Independent of
    // the M2L blocks; same lifetime rules.  cacheModeNearBytes: their device bytes over all modes.
    void cacheModeNear(int id);
    void cacheModeNearFree(int id);
    int64_t cacheModeNearBytes() const;
    // 16 columns per pass on an unsharded high-order handle, off by
    // default.  On: the fp64 mode applies form one chunk of up to 16 columns whenever more
    // than 8 remain, on every mode -- a mode without resident M2L blocks runs the wide mode
    // kernel, one factor formation per entry for all 16 columns -- and the forward solve runs
    // lockstep groups of 16.  The f32 entries, the mixed solve, the block operator and its
    // solves are not affected.  A setting, not a cache: it survives setCoeff, cache rebuilds
    // and the cacheMode*Free calls.  on = 1 is refused (logic_error) on np = 4 and on shards
    // before the device is touched; on = 0 is accepted everywhere.
    void setWide(int on);
    bool wide() const { return wideOn; }
    void mappingHost(const double* charge, int id, double* out);
    void mappingBatchedHost(const double* Q, int k, int id, double* Out);  // N x k column-major
    // One mode on nrhs vectors wherever the mode is ready: rows of N
    // doubles in original order, strides ldx, ldo >= N, unsharded handles.
    //     out[k] = K_id (sigT .* x[k])          (sigT: tree-order sigma_s, or nullptr)
    //     out[k] = x[k] - K_id (sigT .* x[k])   (minuend; x and out must not overlap)
    // A high-order handle runs chunks of 8 columns (a remainder zero-padded to 2, 4 or 8)
    // through the mode kernels of mode_apply.hip on the mode-shared caches: the entry's
    // factor is formed once per chunk.  A mode made resident by cacheMode (fp64 only) runs
    // the MFMA M2L of mode_resident.hip in their place; more than 8 remaining columns then
    // form one chunk of up to 16, two halves of the 8-column launches around one M2L; with
    // setWide(1) every mode forms such chunks, a mode without stored blocks around the wide mode
    // M2L.  np = 4: a resident mode runs applyBlock's identity
    // mix in chunks of 8; a lean mode runs the same chunks through modeApplyLean16 (the
    // near-field mode kernel and the rank-16 mode M2L between the up and down tiers), one
    // read of the shared caches per chunk.
    // modeApplyCheck raises everything that can be refused before the device is touched
    // (false: nrhs = 0, nothing to do).
    // f32: the reduced-precision entries, refused on np = 4 and on sharded handles.
    bool modeApplyCheck(const char* what, int id, int nrhs, const void* x, int64_t ldx, const void* out, int64_t ldo,
                        bool minuend, bool f32 = false) const;
    // keepCalls: append to modeApplyCalls() (a caller that cuts one call into several)
    // prec = F32 (high-order handles): the M2L and the near field in fp32 on the float mirrors
    void modeApplyDev(int id, int nrhs, const double* x, int64_t ldx, const double* sigT, bool minuend, double* out,
                      int64_t ldo, hipStream_t s, bool keepCalls = false, ApplyPrec prec = ApplyPrec::F64);
    // the compiled column count K of every operator pass of the last modeApplyDev /
    // mappingMultiHost call, in order: a mode-kernel chunk (2, 4, 5 or 8), 16 for a high-order
    // chunk of more than 8 columns (a resident mode's, or any mode's with setWide(1)), a resident
    // np = 4 mode's applyBlock chunk (1, 2, 4, 5 or 8), 8 for a per-column leanMapping pass
    const std::vector<int>& modeApplyCalls() const { return modeCalls; }
    // the near-field launches of the same call, in order: (columns: 2, 4, 5, 8, or 16 for the
    // wide launch; 1 if it ran on the resident near blocks, 0 if k_near_mode or its f32 form)
    const std::vector<std::pair<int, int>>& modeNearCalls() const { return nearCalls; }
    void mappingMultiHost(const double* Q, int k, int id, double* Out);  // N x k column-major
    const double* sigmaSTree() const { return dSigmaT.as<double>(); }    // sigma_s in tree order (device)
    void mappingDev(const double* charge, int id, double* out, hipStream_t s, int stageMask = 0x3f);
    void mappingTreeDev(const double* qTree, int id, double* outSlice, hipStream_t s);
    void forwardTreeDev(const double* xTree, double* ySlice, hipStream_t s);
    // sharded applies in two phases around the caller's all-gather of the tier-0
    // root multipoles: begin runs this rank's tier-0 up tasks (input
    // valid at the own range and plan.xHalo only), packs its roots into rootsSend
    // (plan.xRootChunk x 16 x K doubles, K = rootRhs(nrhs)) and starts the near
    // field (it writes the output); end scatters the gathered roots (nranks
    // chunks), runs the upper tiers, the M2L and the down pass.  The same x and out
    // in both calls, tree order.
    void forwardTreePhase(int phase, const double* xTree, double* ySlice, double* rootsSend, const double* rootsRecv,
                          hipStream_t s);
    static int rootRhs(int nrhs);  // right-hand sides per root record of an nrhs apply (padded count)

    // --- block operator (aniso.m:121-157)
    // out[i] = sum_t sum_b mixes[t][i][b] K_{ids[t]}(sig .* x[b]) for i, b < nrhs <= 8:
    // one up pass over the nrhs base vectors, every mode's operators streamed once
    // for all right-hand sides, one down pass.  x: nrhs vectors of all N points
    // (stride ldx; original or tree order); out: original order (owned targets) or
    // the owned tree-order slice (treeOut), stride ldo.  mixes: nterm x nrhs x nrhs.
    void applyBlockDev(int nrhs, const double* x, int64_t ldx, bool treeIn, bool useSigma, int nterm, const int* ids,
                       const double* mixes, double* out, int64_t ldo, bool treeOut, hipStream_t s,
                       int mask = 15);
    // aniso.m on nb = ks blocks of n = N points: which = 0 forward (the right-hand
    // side, aniso.m:121-136), 1 mforward (aniso.m:138-157), 2 x - mforward(x) (the
    // GMRES matvec, aniso.m:155); tree = tree-order input and owned-slice output.
    // gval / sigT (tree-order sigma_s on the device) override the handle's g and
    // sigma_s when given (NaN / nullptr: the handle's).
    void blockOpDev(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool tree, hipStream_t s,
                    double gval = NAN, const double* sigT = nullptr, int phase = 0, double* rootsSend = nullptr,
                    const double* rootsRecv = nullptr, ApplyPrec prec = ApplyPrec::F64);
    // The relaxed-precision block operator of a high-order handle (np = 6, 8, ks <= 8;
    // block_f32.hip): blockOpDev with the M2L and the unstaged near field in
    // fp32 on the float mirrors (built on first use), doubles in and out; everything around
    // the two kernels, the minuend of which = 2 included, is the fp64 code.
    // blockOpF32Refuse raises (ANISO_ERR_STATE) what the handle itself rules out -- np = 4, a
    // sharded handle, ks > 8 -- and blockOpF32Ready a call before the coefficients and the
    // caches; neither touches the device.
    void blockOpF32Refuse(const char* what) const;
    void blockOpF32Ready(const char* what) const;
    void blockOpF32Dev(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool tree, hipStream_t s);
    // host-pointer block operator (aniso.m:121-157): u and out hold nb = ks blocks of
    // N points each (block b at b * N, original order); sigmaS (N, or nullptr: the
    // handle's sigma_s) and gval (NaN: the handle's g) as aniso.m's mforward reads them
    void blockOpHost(int which, const double* u, const double* sigmaS, double gval, double* out);
    // --- direct evaluation at chosen targets (direct.hip; DESIGN.md "Accuracy of the
    // method"): what mapping / the block operator return on a one-leaf tree (maxLevel = 0),
    // at the nt points `targets` (host array of original indices, any order, repeats
    // allowed), from all N sources -- nt x N line integrals, no tree and no cache.  The
    // stencil and singular corrections come from the apply's own correction kernel, read
    // out at the targets.  out: nt entries per row (block form: ks rows at stride ldo).
    // Unsharded handles; every argument and the state are checked before the device is
    // touched, and nt = 0 returns at once.
    void mappingDirectDev(const double* charge, int id, const int64_t* targets, int64_t nt, double* out,
                          hipStream_t s);
    void mappingDirectHost(const double* charge, int id, const int64_t* targets, int64_t nt, double* out);
    void blockOpDirectDev(int which, const double* x, int64_t ldx, const int64_t* targets, int64_t nt, double* out,
                          int64_t ldo, hipStream_t s);
    void blockOpDirectHost(int which, const double* u, const int64_t* targets, int64_t nt, double* out);
    // the (2 nb - 1) mode mixes of forward (chi = false) or mforward (chi = true)
    static std::vector<double> blockMixes(int nb, double g, bool chi);
    // More than kMaxRhs blocks: the block operator runs as
    // nchunks x nchunks passes over chunks of `chunk` blocks (ks <= 8: one pass of ks).
    static void blockPassPlan(int ks, int* chunk, int* nchunks);
    // one pass (development interface): the contribution of input chunk J of x (ks x N,
    // original order) to output chunk I, out (chunk x N); which = 0 forward, 1 mforward
    void blockPassDev(int which, int I, int J, const double* x, int64_t ldx, double* out, int64_t ldo, hipStream_t s);

    // --- extensions
    void setShard(int rank, int nranks);
    // the library's own multi-GPU exchange (comm.hpp): attach a
    // communicator of this shard's rank / nranks, then blockOpShardedDev runs the
    // input's halo all-to-all, phase 1, the root all-gather and phase 2 in one call
    // (any ks: more than kMaxRhs blocks as passes, one exchange per input chunk)
    void commInit(std::unique_ptr<Collectives> c);
    // A sharded high-order handle (aniso_create_sharded at np = 6, 8): a rank
    // computes its own targets from the WHOLE input.  Its plan is Plan::build's lists for
    // (rank, nranks); P2M and M2M run over the whole tree on every rank, the near field, the
    // corrections, the M2L, L2L and L2P over the rank's lists.  commInit runs one all-gather
    // of {N, ks, np, nranks, caches ready} and builds no halo plan; a matvec gathers every
    // rank's owned slice of the ks rows into x with ONE all-gather (parts padded to the
    // largest owned count).  Everything but blockOpShardedDev, blockOpDev in tree order and
    // blockSolveShardedDev raises ANISO_ERR_STATE on such a handle (refuseHoShard).
    bool hoSharded() const { return hoShard; }
    void refuseHoShard(const char* what) const;
    // raise (ANISO_ERR_STATE) on a high-order handle made by aniso_create: the sharded routes
    void refuseHighPlain(const char* what) const;
    void blockOpShardedDev(int which, double* x, int64_t ldx, double* y, int64_t ldy, hipStream_t s);
    bool commReady() const { return comm != nullptr; }
    void getShard(int64_t* ownBegin, int64_t* ownEnd) const { *ownBegin = plan.ownBegin; *ownEnd = plan.ownEnd; }
    // sharded apply: writes only owned targets of out (original order), others untouched
    void permuteToTree(const double* orig, double* tree, hipStream_t s);
    void lineIntegrals(const double* seg, int n, double* out);
    // callers of the hot path (main.cpp:125-141)
    void forwardDev(const double* u, double* out, hipStream_t s);
    int gmresHost(const double* q, double* x, int m, int maxit, double tol, double* hist, int maxhist,
                  double* finalResid);
    // aniso.m:159-173: gmres(A, rhs, restart, tol, maxit), A = x - mforward(x), on the
    // ks stacked blocks (original order, block b at b * N); device / host pointers
    int blockSolveDev(const double* rhs, double* x, int restart, double tol, int maxit, double* hist, int maxhist,
                      double* relres, hipStream_t s);
    // blockSolveDev as inexact (relaxed) GMRES: the matvec of V[j] runs on
    // the f32 block operator iff the latest relative residual estimate the host holds when it
    // enqueues that matvec is <= relax (a cycle's start: its explicit relres; a look-ahead
    // matvec: the estimate of the step before).  Every cycle-boundary residual is fp64, so
    // convergence is blockSolveDev's.  relax = 0: blockSolveDev's launches and bits, no
    // mirrors; relax < 0: the default kRelaxFactor x tol.  Arguments are checked before the
    // handle's state, and every buffer (the mirrors included) is allocated before the first
    // launch.  blockSolveRelaxedCalls: the precision (64 / 32) of every operator pass of the
    // last relaxed solve, in order.
    static constexpr double kRelaxFactor = 1e6;
    int blockSolveRelaxedDev(const double* rhs, double* x, int restart, double tol, int maxit, double relax,
                             double* hist, int maxhist, double* relres, hipStream_t s);
    int blockSolveRelaxedHost(const double* rhs, double* x, int restart, double tol, int maxit, double relax,
                              double* hist, int maxhist, double* relres);
    const std::vector<int>& blockSolveRelaxedCalls() const { return relaxedCalls; }
    int solve16Mixed(const double* B, int64_t ldb, double* X, int64_t ldx, int m, double tol, double innerTol,
                     int maxOuter, int maxCycles, int* outer, double* rel, hipStream_t s);
    // the same for nrhs >= 1 rows in groups of 16 and a restart up to 400 (main.cpp:141's
    // GMRES(80)); *longest: the most steps of any inner cycle; rel: nrhs entries
    int solveMixed(int nrhs, const double* B, int64_t ldb, double* X, int64_t ldx, int m, double tol, double innerTol,
                   int maxOuter, int maxCycles, int* outer, int* longest, double* rel, hipStream_t s);
    // the 16-column DCGS2 Arnoldi of the mixed solves on a caller's buffers (arnoldi16.hpp;
    // aniso_arnoldi16_*): vectors point-major, n16 = 16 x points; st / part sized by
    // arn16_work_doubles(m); status: 64 doubles, per column {estimate, r', steps, -}
    void arnoldi16Ready();  // the device current and the small kernels' LDS limit raised: once per call
    void arnoldi16Begin(int64_t n16, int m, const double* r, const float* sub, const double* scale, float* V,
                        double* st, double* part, double* status, hipStream_t s);
    void arnoldi16Step(int64_t n16, int m, int j, float* V, int64_t ldv, const float* w, double* st, double* part,
                       double* status, hipStream_t s);
    void arnoldi16Solution(int64_t n16, int m, int used, const float* V, int64_t ldv, double* st, double* x,
                           hipStream_t s);
    int blockSolveHost(const double* rhs, double* x, int restart, double tol, int maxit, double* hist, int maxhist,
                       double* relres);
    // the multi-source forward solve (main.cpp:121-141 for nrhs sources):
    // u_k - K_0(sigma_s u_k) = b_k with b_k = K_0 q_k (rhsIsSource) or q_k, every column a
    // restarted GMRES of its own (blockSolveDev's semantics per column) over modeApplyDev,
    // in groups of 8 columns (16 with the wide setting on) that share one operator call per
    // step on the rows still active.  q / x: device rows of N doubles in original order at strides ldq, ldx >= N;
    // x: guess in, solution out.  iters / relres (nrhs entries) and hist (row k at k *
    // maxhist) are host arrays.  Every unsharded handle whose mode 0 is ready.  Returns the
    // steps of all columns.  forwardSolveMultiCheck raises everything that can be refused
    // before the device is touched (false: nrhs = 0, nothing to do).
    // (mixed: the mixed solve's innerTol and maxOuter, checked with the other parameters, and the
    // f32 operator's refusals)
    struct MixedParams {
        double innerTol;
        int maxOuter;
        const int* outer;
    };
    bool forwardSolveMultiCheck(const char* what, int nrhs, const void* q, int64_t ldq, const void* x, int64_t ldx,
                                const int* iters, int restart, double tol, int maxit,
                                const MixedParams* mixed = nullptr) const;
    int forwardSolveMultiDev(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x, int64_t ldx,
                             int restart, double tol, int maxit, int* iters, double* relres, double* hist, int maxhist,
                             hipStream_t s);
    int forwardSolveMultiHost(const double* Q, int k, bool rhsIsSource, double* X, int restart, double tol, int maxit,
                              int* iters, double* relres);  // N x k column-major
    // The same solve in mixed precision on a high-order handle: per group
    // of 8 columns an fp64 refinement loop -- explicit fp64 residuals, converged at
    // |r| <= tol |b| -- around colsSolveGroup over the f32 operator on the residuals scaled to
    // unit norm (zero guess, innerTol, restart, maxit cycles).  A column stops when it has
    // converged, at maxOuter refinements, or when a refinement does not reduce its fp64
    // residual (the previous iterate is kept).  iters: a column's inner steps, negative if it
    // did not converge; outer: its refinements; relres: its last explicit fp64 residual.
    // Every buffer is allocated before the first launch (x untouched on failure).
    int forwardSolveMultiMixedDev(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x, int64_t ldx,
                                  int restart, double tol, double innerTol, int maxit, int maxOuter, int* iters,
                                  int* outer, double* relres, hipStream_t s);
    int forwardSolveMultiMixedHost(const double* Q, int k, bool rhsIsSource, double* X, int restart, double tol,
                                   double innerTol, int maxit, int maxOuter, int* iters, int* outer, double* relres);
    // every operator pass of the last mixed forward solve, in order: {precision (64 / 32), columns}
    const std::vector<std::pair<int, int>>& forwardSolveMixedCalls() const { return mixedCalls; }
    // the column count of every operator call of the last forward solve, in order
    const std::vector<int>& forwardSolveCalls() const { return solveCalls; }
    // --- the block operator and its solve for several sources (aniso.m:121-173
    // for nsrc charges in one medium).  x / out: nsrc * ks device rows of N doubles in original
    // order at strides ldx, ldo >= N, row s * ks + b = block b of source s; `which` as blockOpDev's.
    // x and out must not overlap.  Unsharded handles with every mode 0 .. 2 ks - 2 ready.
    // np = 6, 8 and ks <= 8: the sources run in chunks of 4 (a remainder of 3 zero-padded to 4, of
    // 2 and 1 on the 2- and 1-source instances) through ONE M2L launch per chunk that reads every
    // stored E block once for all its sources (block_multi.hip); the near field, the corrections
    // and the up and down passes run per source on blockOpDev's launches.  np = 4 (cached or lean)
    // or ks > 8: ONE blockOpDev PER SOURCE -- correct, nothing shared.  A source's output bits do
    // not depend on how many sources the call has, which ones, or its position among them.
    // blockOpMultiCheck raises everything that can be refused before the device is touched
    // (false: nsrc = 0, nothing to do).
    bool blockOpMultiCheck(const char* what, int which, int nsrc, const void* x, int64_t ldx, const void* out,
                           int64_t ldo) const;
    void blockOpMultiDev(int which, int nsrc, const double* x, int64_t ldx, double* out, int64_t ldo, hipStream_t s);
    void blockOpMultiHost(int which, const double* U, int nsrc, double* Out);  // (ks N) x nsrc column-major
    // aniso.m:159-173 per source: b_s = forward(q_s) (rhsIsCharge, aniso.m:160) or q_s, then
    // blockSolveDev's restarted GMRES of x - mforward(x) on the source's ks * N vector.  Groups of
    // 4 sources run in lockstep (forwardSolveMultiDev's scheme at row length ks * N) and share one
    // blockOpMultiDev(2, ...) per step on exactly the sources still active.  q / x as
    // blockOpMultiDev's rows; x: guess in, solution out (untouched if the work buffers cannot be
    // allocated); iters / relres (nsrc) and hist (row s at s * maxhist) are host arrays.  Every
    // buffer is allocated before the first launch and freed on return.  Returns the steps of all
    // sources; the source count of every operator call is left in forwardSolveCalls().
    bool blockSolveMultiCheck(const char* what, int nsrc, const void* q, int64_t ldq, const void* x, int64_t ldx,
                              const int* iters, int restart, double tol, int maxit) const;
    int blockSolveMultiDev(int nsrc, const double* q, int64_t ldq, bool rhsIsCharge, double* x, int64_t ldx,
                           int restart, double tol, int maxit, int* iters, double* relres, double* hist, int maxhist,
                           hipStream_t s);
    int blockSolveMultiHost(const double* Q, int nsrc, bool rhsIsCharge, double* X, int restart, double tol, int maxit,
                            int* iters, double* relres);  // (ks N) x nsrc column-major
    // --- the relaxed-precision multi-source operator and lockstep solves (DESIGN.md §3.18.10;
    // np = 6, 8, unsharded, ks <= 8).  blockOpMultiF32Dev: blockOpMultiDev's chunking with the
    // near field and the M2L in fp32 on the float mirrors (built on first use); a source's bits
    // are blockOpF32Dev's.  The two solves are blockSolveMultiDev / forwardSolveMultiDev with
    // the relaxed rule per GROUP: a step's one operator call runs on the f32 operator iff
    // relax > 0 and the largest latest relative-residual estimate among the step's live columns
    // is <= relax (step 0 of a cycle: the cycle's explicit relres).  Every residual, and
    // forward(charge), stays fp64, so convergence and relres are decided as in the fp64 entries.
    // Under the group rule a column's bits depend on the columns beside it -- the one property
    // of the fp64 entries this gives up; identical calls still return equal bits.  relax < 0:
    // kRelaxFactor x tol; relax = 0: the fp64 entry's launches and bits, no mirrors; NaN:
    // invalid_argument.  Refusals (blockOpF32Refuse, the arguments, blockOpF32Ready) come before
    // the device is touched; the mirrors and every buffer before the first launch.
    // multiRelaxedCalls(): {64 | 32, columns} of every operator call of the last such solve.
    void blockOpMultiF32Dev(int which, int nsrc, const double* x, int64_t ldx, double* out, int64_t ldo,
                            hipStream_t s);
    int blockSolveMultiRelaxedDev(int nsrc, const double* q, int64_t ldq, bool rhsIsCharge, double* x, int64_t ldx,
                                  int restart, double tol, int maxit, double relax, int* iters, double* relres,
                                  double* hist, int maxhist, hipStream_t s);
    int blockSolveMultiRelaxedHost(const double* Q, int nsrc, bool rhsIsCharge, double* X, int restart, double tol,
                                   int maxit, double relax, int* iters, double* relres);
    int forwardSolveMultiRelaxedDev(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x, int64_t ldx,
                                    int restart, double tol, int maxit, double relax, int* iters, double* relres,
                                    double* hist, int maxhist, hipStream_t s);
    int forwardSolveMultiRelaxedHost(const double* Q, int k, bool rhsIsSource, double* X, int restart, double tol,
                                     int maxit, double relax, int* iters, double* relres);
    const std::vector<std::pair<int, int>>& multiRelaxedCalls() const { return multiCalls; }
    // the same solve on a sharded handle with a communicator, every rank together
    // (DESIGN.md §3.17): rhs / x are this rank's owned slices in tree order, ks rows of
    // `owned` doubles at strides ldr / ldx (device).  Every branch is taken from
    // all-reduced values, so the ranks issue the same collectives and return the same
    // counts; a refusal or a device-side failure of one rank ends the call on all.
    int blockSolveShardedDev(const double* rhs, int64_t ldr, double* x, int64_t ldx, int restart, double tol,
                             int maxit, double* hist, int maxhist, double* relres, hipStream_t s);
    // config 5's fp32 operator (f32op.hip): Y = X - K_0(sigma_s .* X)
    // for 16 right-hand sides, X and Y point-major (N x 16 floats, tree order), every
    // FMM translation a 16 x 16 x 16 MFMA product on fp32 caches (built from the
    // fp64 mode-0 operators at the first call).  Unsharded handles only.
    void forwardF32Dev(const float* X, float* Y, hipStream_t s, int mask = kStageAll);
    // the fp64 16-right-hand-side operator on MFMA (f64op.hip): Y = K_id X
    // (forward = false) or main.cpp's Y = X - K_0(sigma_s .* X) (forward = true, id 0);
    // X, Y point-major N x 16 doubles in tree order.  The mode's fp64 caches (directed
    // lists, A order) are built from its operators at the first call.  Unsharded only.
    void mrhs64Dev(int id, bool forward, const double* X, double* Y, hipStream_t s, int mask = kStageAll);
    // the block solve's CGS2 sweeps as primitives (aniso_krylov_dot / _update)
    void krylovDot(int64_t n, int nv, const double* V, int64_t ldv, const double* w, double* out, hipStream_t s);
    void krylovUpdate(int64_t n, int nv, const double* V, int64_t ldv, const double* c, double* w, double* out,
                      bool dots, hipStream_t s);
    // DCGS2 Arnoldi primitives on a caller's state block (arnoldi.hpp; aniso_arnoldi_*):
    // begin a cycle (V[0] = the residual; rr: its all-reduced |r|^2, or null: this rank's),
    // one step on one rank, or its parts around a caller's all-reduces (project / update
    // write this rank's row sums; coef / column take the reduced ones), and the cycle's
    // update x += P T R^-1 g
    void arnoldiBegin(int64_t n, int m, const double* V, int64_t ldv, double* st, const double* rr, double normb,
                      double* status, hipStream_t s);
    void arnoldiStep(int64_t n, int m, int j, double* V, int64_t ldv, const double* w, double* st, double* status,
                     hipStream_t s);
    void arnoldiProject(int64_t n, int j, const double* V, int64_t ldv, const double* w, double* out, hipStream_t s);
    void arnoldiCoef(int m, int j, double* st, const double* red, hipStream_t s);
    void arnoldiUpdate(int64_t n, int m, int j, double* V, int64_t ldv, const double* w, const double* st, double* out,
                       hipStream_t s);
    void arnoldiColumn(int m, int j, double* st, const double* red, double* status, hipStream_t s);
    void arnoldiSolution(int64_t n, int m, int used, const double* V, int64_t ldv, double* st, double* x,
                         hipStream_t s);
    // directed M2L pairs of the 16-right-hand-side operators (0 before their plan is built)
    int64_t mrhsM2LPairs() const { return mrhsPlanReady ? (int64_t)f32.m2lSrc.size() : 0; }
    int64_t f32Bytes() const { return f32Ready ? (int64_t)(d32Km2l.bytes + d32Knear.bytes) : 0; }
    hipStream_t stream() const { return own; }
    // raise (ANISO_ERR_RUNTIME) if a fused top-of-tree launch gave up waiting for its
    // producers since the last check: its locals, and so the apply's output, are invalid
    void checkDeviceErrors();
    // recovery from a fused-launch time-out where the library owns the timeline (the
    // host-pointer block operator, the block solve): if the flag is set, drain `s`,
    // clear it, switch the fused launch off for the rest of the call (forceUnfused)
    // and count it; the caller then re-runs the apply on the tier launches
    bool recoverTopTimeout(hipStream_t s);
    int64_t topRecoveries = 0;  // applies re-run after a time-out (aniso_stats)
    int64_t topSteals();        // tier tasks the fused launch's waiting blocks computed themselves (aniso_stats)
    int64_t oneXApplies = 0;    // sharded matvecs through the one-collective exchange (aniso_stats)
    int64_t upPartialApplies = 0;  // ... of them with the upper multipoles as partial sums (aniso_stats)
    bool nearOverlaps() const { return overlapOn(); }  // the block apply's near field on a side stream
    // the one-GPU block apply forms its bottom up tier inside the near field
    bool nearUpTier() const { return nearUpOn && plan.nearUpOk && !overlapOn(); }
    bool forceUnfused = false;
    // set while a call that recovers its own time-outs (the block solve) runs: the
    // entry checks of the applies it enqueues leave the flag to its recovery points
    bool ownTimeline = false;
    // wait for every apply enqueued by this handle (both streams), then check
    void sync();
    // development timeline of the last fused top-of-tree launch (ANISO_TOP_TRACE=1,
    // tools/top_trace.py): per block 8 values {start, waited, end (100 MHz ticks), hw id,
    // kind (-k: up tier k; else the cluster id), wait tier, targets, block reads}
    std::vector<int64_t> topTrace();
    bool harmonicReady() const { return useAtt && attReady; }
    bool clustersOn() const { return useClusters; }
    // the block apply's upper up tiers ride in the clustered M2L launch (k_top_m2l_hc);
    // ANISO_TOP_FUSED=0 runs them as launches of their own before the clusters (a rank
    // of 8: 0.262 against 0.251 ms, same-process A/B r03ls)
    bool topFusedOn() const {
        const int ntier = (int)plan.upTierTask.size() - 1;
        return useClusters && !detSums && topFusedMode != 0 && !forceUnfused && top_fused_enabled() && ntier >= 2 &&
               ntier <= kMaxTopTiers &&
               plan.upLastLeafTier == 0 && plan.hmClWait.size() + 1 == plan.hmClPtr.size();
    }
    // bitwise-reproducible applies: the clustered M2L with its LDS
    // sums in fixed point (integer adds: order-independent) and the upper up tiers as
    // launches of their own; ANISO_DET_PER_TARGET=1 keeps the round-2 form instead (one
    // wave per target, every sum in a fixed order, every block read from both ends)
    void setDeterministic(bool on) {
        if (on && highOrder())
            throw std::invalid_argument("deterministic applies: not on a high-order handle (np = " + std::to_string(np) +
                                        "): its far field sums in a fixed order and is bitwise repeatable as it is");
        if (on && ks > kMaxRhs)
            throw std::invalid_argument("deterministic applies: not with more than " + std::to_string(kMaxRhs) +
                                        " blocks (ks = " + std::to_string(ks) + ")");
        detSums = on && !detPerTarget;
        useClusters = !(on && detPerTarget);
    }
    bool deterministicOn() const { return detSums || !useClusters; }
    // a high-order handle (np = 6 or 8): every mode runs on the mode-shared
    // caches; whatever streams per-mode operators, shards or runs single stages is refused
    bool highOrder() const { return np != kNP; }
    // raise (ANISO_ERR_STATE) on a high-order handle, before anything is launched
    void refuseHighOrder(const char* what) const;
    // the mode's own operators are resident (cache(id) since the last setCoeff)
    bool modeCached(int id) const { return id >= 0 && id < kernelSize && modes[id].resident; }
    // raise (ANISO_ERR_STATE) if the mode was made ready by cacheBlock only: `what`
    // streams its operators.  A mode with no tables either is left to the caller's check.
    void needResident(int id, const char* what) const;
    int kernelSize = 0;
    // stage timing with HIP events recorded in-stream (no host sync per apply);
    // stageTimes() averages every apply recorded since setTiming(level > 0).
    // level 1: every stage; level 2: the M2L and near-field spans only (4 events per
    // block apply instead of 9 -- the timers cost 1.3 % of a block matvec, r04as)
    void setTiming(int level);
    StageTimes stageTimes();
    int timeStages = 0;

    Geometry geo;
    Tree tree;
    Plan plan;
    int ks = 0, ns = 0, np = 0, maxLevel = 0;
    double g = 0;
    bool coeffSet = false;
    std::vector<double> sigma_s, sigma_t;

    // stats
    int64_t nearEntries() const { return plan.pairsNear; }
    int64_t m2lEntries() const { return plan.pairsM2L * np * np * np * np; }
    int maxNearSources() const { return maxNearS; }

private:
    void apply(const double* charge, bool treeIn, const double* sigT, int id, double* out, bool treeOut, hipStream_t s,
               int mask);
    void applyBlock(int K, const double* x, int64_t ldx, bool treeIn, const double* sigT, int nterm, const int* ids,
                    const double* mixes, double* out, int64_t ldo, bool treeOut, hipStream_t s, int mask,
                    const ApplyCall& call);
    // blockOpDev at ks <= kMaxRhs on a call description (a sharded matvec's carries its exchange form)
    void blockOp(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool treeIo, hipStream_t s,
                 double gval, const double* sigT, ApplyCall& call);
    struct Pending {  // state between the two phases of a sharded apply
        bool active = false, nearDone = false;
        int K = 0, e0 = -1, ePack = -1, eStart = -1;
    } pend;
    // the public call that started a pending sharded apply: its _end must repeat it
    // (operation, which, vectors, strides, sigma_s, g)
    struct PendingCall {
        int kind = -1, which = -1;
        const void *x = nullptr, *out = nullptr, *sig = nullptr;
        int64_t ldx = 0, ldo = 0;
        double g = 0;
        bool operator==(const PendingCall& o) const {
            return kind == o.kind && which == o.which && x == o.x && out == o.out && sig == o.sig && ldx == o.ldx &&
                   ldo == o.ldo && (g == o.g || (std::isnan(g) && std::isnan(o.g)));
        }
    } pendCall;
    void pendingCall(int phase, const PendingCall& c);
    // ks > kMaxRhs: the passes of the block operator (blockOpDev), one pass, the limit
    void blockOpPasses(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool treeIo, hipStream_t s,
                       double gval, const double* sig);
    void blockPass(int I, int J, const std::vector<double>& mix, const double* x, int64_t ldx, bool tree,
                   const double* sig, double* out8, int64_t ldo, hipStream_t s);
    void checkBlockLimit(bool shardedCall) const;
    // pass (I, J)'s sub-block of the mixes and its harmonic weights
    void passMix(int I, int J, const std::vector<double>& mix, std::vector<double>& sub, HarmWeights& hw) const;
    // ks > kMaxRhs on a shard: per input chunk one exchange and one up pass, per output
    // chunk under it the window's near field, M2L and down pass
    // (yo: the owned slice of the output, row b at yo + b * ldo)
    void blockOpShardedPasses(int which, double* x, int64_t ldx, double* yo, int64_t ldo, bool one, hipStream_t s);
    // blockOpShardedDev with the output as its owned slice (ldo >= owned): the sharded
    // block solve's matvec writes its compact vector
    void blockOpShardedOwned(int which, double* x, int64_t ldx, double* yo, int64_t ldo, hipStream_t s);
    // the sharded matvec's rank-local checks and work buffers, ahead of any collective
    void prepareShardedMatvec(int which = 2);
    // the sharded block solve: the matvec's (ks, N) input and the all-reduce buffer,
    // kept between solves (grown, never shrunk)
    DevBuf dShIn, dShRed;
    // the exchange of one sharded matvec (or of one input chunk of its passes) around
    // the two phases: nb rows of x, the one- or the two-collective form.  The phases get
    // the call description with the exchange form filled in and add their own part.
    using PhaseFn = std::function<void(ApplyCall&)>;
    void shardedExchange(int nb, double* x, int64_t ldx, bool one, hipStream_t s, const PhaseFn& phase1,
                         const PhaseFn& phase2);
    // the far field of a high-order handle (high_order.hip): applyBlock's branch for np != 4
    void applyBlockHigh(int K, const InRows& in, int nterm, const int* ids, const double* mixes, const OutRows& o,
                        hipStream_t s, int mask, const ApplyCall& call);
    void uploadHighPlan();  // its tables and level lists (ensureDevice: they follow the tree alone)
    DevBuf dHoTab, dHoChild, dHoM2m, dHoL2l, dHoMult, dHoLocal;
    // a sharded high-order handle: every non-empty leaf (the replicated P2M; dLeafInfo keeps
    // the owned leaves), the all-gather's send part and receive buffer (ks x hgMax doubles
    // per rank, hgMax the largest owned count) and every rank's cut on the device
    bool hoShard = false;
    DevBuf dHoLeafAll, dHgSend, dHgRecv, dHgCuts;
    int hoLeafAll = 0;
    int64_t hgMax = 0;
    void commInitHigh(std::unique_ptr<Collectives> c);
    void blockOpShardedHigh(int which, double* x, int64_t ldx, double* yo, int64_t ldo, hipStream_t s);
    std::vector<int> hoM2mPtr, hoL2lPtr;  // per level: its range of dHoM2m (bottom-up) / dHoL2l (top-down)
    int hoWorkK = 0;
    // the stages of the un-fused applies, one launcher's arguments each
    OutRows outRows(double* out, int64_t ld, bool tree, const double* minuend = nullptr, int64_t minuendLd = 0) const {
        return {out, minuend, tree ? nullptr : dPerm.as<int>(), ld, tree ? plan.ownBegin : 0, minuendLd, tree};
    }
    // the plan views of kernels.hpp: the only place these buffers are cast for the launchers that take views
    PairList pairList() const {
        return {(int)plan.m2lTgt.size(), dM2LTgt.as<int>(), dAttPtr.as<int64_t>(), dAttSrc.as<int>(), dAttBlk.as<int>()};
    }
    NodeBoxes nodeBoxes() const { return {dNcx.as<double>(), dNcy.as<double>(), dNrx.as<double>(), dNry.as<double>()}; }
    TreePoints treePoints() const { return {dPxT.as<double>(), dPyT.as<double>()}; }
    NearList nearList(bool residentOff = false) const {  // residentOff: off = nearFOff, else nearKOff
        return {(int)plan.leaves.size(), plan.nearMaxLeaf, dLeafInfo.as<int4>(), dNearPtsPtr.as<int64_t>(),
                dNearPts.as<int>(), (residentOff ? dNearFOff : dNearKOff).as<int64_t>()};
    }
    void prepareCharges(int K, const InRows& in, double* fT, double* cT, hipStream_t s);
    void nearUnstaged(int K, const HarmWeights& hw, const HarmWindow* win, int mask, const OutRows& o, hipStream_t s);
    void nearUnstagedF32(int K, const HarmWeights& hw, const OutRows& o, hipStream_t s);
    void nearMode(int K, int id, const OutRows& o, hipStream_t s, ApplyPrec prec = ApplyPrec::F64);
    // a two-half chunk's near field on the resident near blocks: columns 0 .. KA-1 from
    // dFT to a.o, 8 .. 8+KB-1 from dFT2 to b.o, one launch
    void nearMode16(int id, const ModeHalf& a, const ModeHalf& b, hipStream_t s);
    void corrections(int K, const CorrFold& cf, const double* fT, const double* cT, int64_t begin, int64_t end,
                     int mask, const OutRows& o, hipStream_t s);
    // dHoMult / dHoLocal for K columns (grown, never shrunk), the locals zeroed; second: the
    // expansions of a 16-column chunk's second half (dHoMult2 / dHoLocal2)
    void hoReserve(int K, hipStream_t s, bool second = false);
    size_t hoDoubles(int K) const { return (size_t)tree.nn * np * np * K; }  // one expansion buffer
    // fT: the charges the P2M reads; allLeaves: a shard's replicated P2M
    void hoUpPass(int K, const double* fT, double* mult, bool allLeaves, hipStream_t s);
    void hoDownPass(int K, double* local, const OutRows& o, hipStream_t s);
    void upTier16(int K, int k, const int* list, int ntask, double* fT, double* cT, const double* recv, double* send,
                  unsigned* zeroCnt, const InRows& in, hipStream_t s);
    void downPass16(int K, int mask, const double* nearPart, const double* hpart, const OutRows& o, hipStream_t s);
    // groups of nb rows (stride ldx) into the first nb of each group's K rows of buf (stride N),
    // the other rows zero; and the first n points of the nb rows of one group back out
    void padRowsIn(DevBuf& buf, int groups, int nb, int K, const double* x, int64_t ldx, hipStream_t s);
    void padRowsOut(const double* group, int nb, int64_t n, double* out, int64_t ldo, hipStream_t s);
    // blockOpMultiDev's chunk of S in {1, 2, 4} sources (nreal of them present, the rest zero)
    // on a high-order handle: its S multipole and S local buffers, and the chunk's rows padded
    // to the compiled block count (grown, never shrunk: a hipFree synchronises the device)
    // prec = F32: the near field of applyBlockHigh's f32 route per source and
    // the f32 M2L (block_multi_f32.hip) on the float mirrors, every other stage unchanged
    void blockMultiChunk(int which, int S, int nreal, const double* x, int64_t ldx, double* out, int64_t ldo,
                         hipStream_t s, ApplyPrec prec = ApplyPrec::F64);
    void blockMultiReserve(int S);
    DevBuf dMsMult, dMsLocal, dMsIn, dMsOut;
    // mapping of a mode whose operators are not resident: one pass of the offset form
    // (sigT: tree-order sigma_s multiplied into the charge by the pass's launch_prepare)
    void leanMapping(const double* charge, int id, double* out, hipStream_t s, int mask, const double* sigT = nullptr);
    // modeApplyDev's chunk on a high-order handle: one half of K = 2, 4, 5 or 8 columns, or (a
    // resident mode, or the wide setting) an 8-column half and a second of 2, 4, 5 or 8 around
    // one M2L for all of them
    void modeChunkHigh(int id, int nh, const ModeHalf* h, hipStream_t s, ApplyPrec prec);
    // the most columns of one chunk of modeApplyDev: 16 on a high-order handle in fp64 with the
    // mode's M2L blocks resident or the wide setting on, else 8
    int modeChunkWidth(int id, ApplyPrec prec) const {
        return highOrder() && prec == ApplyPrec::F64 && (modeBlocks.find(id) || wideOn) ? 2 * kMaxRhs : kMaxRhs;
    }
    // nb rows of x (stride ldx) as a half of K compiled columns writing nb rows of out: in place
    // (K = nb), or through dPadIn / dPadOut with zero rows (*padded: padRowsOut is due after the chunk)
    ModeHalf stageHalf(int nb, int K, const double* x, int64_t ldx, const double* sigT, bool sub, double* out,
                       int64_t ldo, bool* padded, hipStream_t s);
    // cacheMode's and cacheModeNear's shared checks, memory policy and bookkeeping: `built` and
    // `noun` name the blocks in the messages, build(F) enqueues the launch that fills them on `own`
    void cacheResident(const char* api, const char* built, const char* noun, bool needDirected, int id,
                       ResidentBlocks& rb, size_t need, const std::function<void(double*)>& build);
    ResidentBlocks modeBlocks;  // cacheMode: resident factor blocks per mode id
    DevBuf dHoMult2, dHoLocal2;
    int hoWorkK2 = 0;
    // setWide: every mode forms 16-column chunks, resident or not (the wide mode M2L measured
    // shorter than two narrow launches at both orders)
    bool wideOn = false;
    ResidentBlocks modeNearBlocks;  // cacheModeNear: resident near factor blocks per mode id
    // the charges of a 16-column chunk's second half while one near launch serves both
    // (grown, never shrunk, as dHoMult2)
    DevBuf dFT2, dCT2;
    int workK2 = 0;
    void reserveCharges2(int K);
    // modeApplyDev's chunk of K = 2, 4, 5 or 8 columns on a lean mode of an np = 4 handle
    void modeApplyLean16(int id, int K, const InRows& in, const OutRows& o, hipStream_t s);
    // the modes of a batched apply are usable by it: tables for the harmonic launches,
    // resident operators for the per-mode stream (checked before anything is launched)
    void checkModes(int K, int nterm, const int* ids, const double* mixes, const ApplyCall& call) const;
    DevBuf dPassIn, dPassOut;  // a pass's zero-padded input chunk, its 8 output rows
    // direct evaluation: the checks shared by its entries (false: nt = 0, nothing to do),
    // the per-call device state (targets, weights, partials; the previous call's launches
    // are waited for before it is overwritten), the corrections of an input at all N points
    bool directCheck(const char* what, bool block, int id, int which, const void* in, const char* inName,
                     int64_t ldx, const int64_t* targets, int64_t nt, const void* out, int64_t ldo) const;
    void directBegin(const int64_t* targets, int64_t nt, const std::vector<double>& weights, int KO);
    void directCorr(int K, const double* x, int64_t ldx, const double* sig, int nterm, const int* ids,
                    const double* mixes, double* corr, hipStream_t s);
    void directSweep(int KO, DirectArgs a, int64_t nt, hipStream_t s);
    DevBuf dDirTg, dDirW, dDirPart, dDirCorr, dDirF, dDirC, dDirIn, dDirOut;
    hipEvent_t evDirect = nullptr;
    // Targets per launch.  One launch is targets x ceil(N / 1024) workgroups, each walking
    // 1,024 line integrals.  Measured at 1M points (sz = 1024, d = 1), 256 targets per call,
    // mode form: 4 per launch 1.00 s, 16 0.93 s, 32 0.916 s, 64 0.911 s, all 256 in one
    // launch 0.873 s.  32 keeps a launch at 0.11 s for 5 % over the single launch of 0.87 s
    // (DESIGN.md "Accuracy of the method").  ANISO_DIRECT_TARGETS, read when the handle is
    // created, overrides it (tests: a small value exercises the chunking at small N).
    int directChunk = 32;
    // a pass's input chunk, rows b0 .. of x: {pointer, leading dimension}, in place or in dPassIn
    std::pair<double*, int64_t> stagePassInput(double* x, int64_t ldx, int b0, hipStream_t s);
    void ensureWork(int K);  // work arrays for K right-hand sides
    const ModeArgs* modeTable(int K, int nterm, const int* ids, const double* mixes);
    // harmonic (mode-shared) block apply, DESIGN.md §3.9: the E caches of every
    // directed M2L pair and near block, built at the first cache() of a block handle
    bool harmonicWeights(int K, int nterm, const int* ids, const double* mixes, HarmWeights& hw) const;
    void buildAttCache();
    bool useAtt = false, attReady = false;
    DevBuf dAttM2L, dAttNear, dSigDiag, dAttPtr, dAttSrc, dAttBlk, dAttOwner, dAttOther;
    DevBuf dAttM2LF, dAttNearF;    // their float mirrors (cacheF32; none: empty)
    void dropCacheF32();
    DevBuf dAttMax;                // max |E| of dAttM2L (the deterministic sums' bound)
    DevBuf dHmClBound, dNodeWmax;  // the deterministic sums: per cluster, per node
    DevBuf dHmClPtr, dHmTgt, dHmPtr, dHmSrc, dHmBlk, dHmSlot, dHmNDir;  // cluster plan
    DevBuf dHmHaloPtr, dHmHaloPos, dHmPart, dDnChainFold;  // the halo form (Plan::hmHaloPtr)
    DevBuf dHmClWait, dTopCnt;  // fused top-of-tree launch: per-cluster wait tier, per-tier counters
    DevBuf dTopSteals;          // tier tasks computed by waiting blocks of the fused launch (persistent)
    DevBuf dTopTrace;           // ANISO_TOP_TRACE=1: the launch's per-block timeline
    DevBuf dKryPart;            // partial sums of the Krylov primitives
    // config 5's library solve (solve16Mixed): its vectors and fp32 basis, kept between
    // solves (grown, never shrunk: a hipFree synchronises the device)
    DevBuf s16B, s16X, s16R, s16W, s16D, s16Df, s16W32, s16V, s16St, s16Part, s16R0;
    double* s16Stat = nullptr;   // their mapped status block (80 doubles) and its event
    hipEvent_t s16Ev = nullptr;
    void mixedCheckState(const char* what, const char* entry) const;
    void mixedCheckArgs(const char* what, int mMax, int m, double tol, double innerTol, int maxOuter, int maxCycles,
                        int64_t ldb, int64_t ldx) const;
    void mixedPrepare(int m);
    int mixedGroup(const double* B, int64_t ldb, double* X, int64_t ldx, int nrows, int m, double tol,
                   double innerTol, int maxOuter, int maxCycles, int* outer, int* longest, double* rel, hipStream_t s);
    int mixedGroupRun(const double* B, int64_t ldb, double* X, int64_t ldx, int nrows, int m, double tol,
                      double innerTol, int maxOuter, int maxCycles, int* outer, int* longest, double* rel,
                      hipStream_t s);
    // One group of ng <= cw.G (8 or 16) independent columns of row length L in lockstep, the loop
    // the forward solve and the multi-source block solve share: B holds the right-hand sides
    // (compact rows of L), x the guesses / solutions (rows at stride ldx), A(nrows, In, W) is one
    // operator call on nrows compact rows.  `what` names the solve in its error messages.
    struct ColsSolve {
        int64_t L;
        const char* what;
        std::function<void(int, const double*, double*)> A;
        // the relaxed rule: Alow serves a step's call iff relax > 0 and the
        // largest latest estimate among the step's live columns is <= relax; residuals stay on A
        std::function<void(int, const double*, double*)> Alow = nullptr;
        double relax = 0.0;
        std::vector<std::pair<int, int>>* rec = nullptr;  // {64 | 32, columns} per operator call
    };
    // the bodies of the multi-source solves, relaxed (relax > 0) or not
    int blockSolveMultiRun(const char* what, int nsrc, const double* q, int64_t ldq, bool rhsIsCharge, double* x,
                           int64_t ldx, int restart, double tol, int maxit, double relax, int* iters, double* relres,
                           double* hist, int maxhist, std::vector<std::pair<int, int>>* rec, hipStream_t s);
    int forwardSolveMultiRun(int nrhs, const double* q, int64_t ldq, bool rhsIsSource, double* x, int64_t ldx,
                             int restart, double tol, int maxit, double relax, int* iters, double* relres,
                             double* hist, int maxhist, std::vector<std::pair<int, int>>* rec, hipStream_t s);
    // what the relaxed multi entries check before the device is touched; returns the relax in force
    double multiRelaxedEnter(const char* what, bool block, double tol, double relax) const;
    std::vector<std::pair<int, int>> multiCalls;  // multiRelaxedCalls()
    int colsSolveGroup(const ColsSolve& cs, ColsWork& cw, int ng, double* x, int64_t ldx, int m, double tol, int maxit,
                       int* iters, double* relres, double* hist, int maxhist, hipStream_t s);
    // the restarted GMRES of one system: the loop blockSolveDev and blockSolveShardedDev share
    int gmresRestarted(const GmresSystem& g, StatusBlock& hs, double tol, int maxit, double* hist, int maxhist,
                       double* relres, hipStream_t s);
    std::vector<int> solveCalls;
    std::vector<std::pair<int, int>> mixedCalls;  // forwardSolveMixedCalls()
    std::vector<int> modeCalls;  // modeApplyCalls()
    std::vector<int> relaxedCalls;  // blockSolveRelaxedCalls()
    // blockSolveDev's body; relax > 0: the relaxed rule, rec: where every pass is recorded
    int blockSolveRun(const double* rhs, double* x, int restart, double tol, int maxit, double relax,
                      std::vector<int>* rec, double* hist, int maxhist, double* relres, hipStream_t s);
    std::vector<std::pair<int, int>> nearCalls;  // modeNearCalls()
    void arnoldiParts(int rows);  // dKryPart for sweeps of `rows` rows
    bool topTraceOn = false;
    int topFusedMode = 1;  // ANISO_TOP_FUSED=0: the upper up tiers as launches of their own
    // the staged near field forms its charges from the input and forks at the start
    // of the block apply, beside the up pass (ANISO_NEAR_EARLY=0: after it, from fT)
    bool nearEarly = true;
    // the bottom up tier inside the staged near field on one GPU (Plan::nearUpOk, serial
    // schedule; ANISO_NEAR_UP=0: its own launch)
    bool nearUpOn = true;
    DevBuf dNearUpGrp;
    int topTraceBlocks = 0;
    // the attached communicator and its halo exchange plan (commInit): per element of
    // the send / receive position lists its tree position and its place in the
    // peer-major buffers (base + b * stride for block b); doubles per peer
    std::unique_ptr<Collectives> comm;
    DevBuf dHxSendPos, dHxSendBase, dHxSendStride, dHxRecvPos, dHxRecvBase, dHxRecvStride, dHxSendBuf, dHxRecvBuf;
    DevBuf dXRootsSend, dXRootsRecv;
    std::vector<int64_t> hxScount, hxSoff, hxRcount, hxRoff;
    int64_t hxNsend = 0, hxNrecv = 0;
    // the one-collective exchange (Plan::xOneOk; ANISO_ONE_EXCHANGE=0 keeps the halo
    // all-to-all before phase 1): per peer one buffer part = the tier-0 root records,
    // its input positions (block-major, as the halo exchange), its multipole rows
    // (16 x K each)
    DevBuf dOxSendPos, dOxSendBase, dOxSendStride, dOxRecvPos, dOxRecvBase, dOxRecvStride;
    DevBuf dOxSendNode, dOxSendNodeBase, dOxRecvNode, dOxRecvNodeBase, dOxSendBuf, dOxRecvBuf, dXOwnT0Tasks;
    DevBuf dOxRootSend, dOxRootRecv, dOxRootDst;  // the root records' place in each peer part
    DevBuf dNearGrpEarly, dNearGrpLate;           // Plan::nearGrpEarly / nearGrpLate
    int64_t oxRootParts = 0;
    std::vector<int64_t> oxScount, oxSoff, oxRcount, oxRoff;
    int64_t oxNsendPts = 0, oxNrecvPts = 0, oxNsendNodes = 0, oxNrecvNodes = 0;
    bool oxReady = false, oneXOn = true;
    // the upper multipoles as partial sums (Plan::xUpPartial on every rank): the parts
    // carry every rank's records instead of the roots; the unpack sums each upper
    // node's records (oxUpSumNode / Ptr / Src: >= 0 an offset into the receive buffer,
    // < 0 ~offset into this rank's own records)
    bool oxUp = false;
    DevBuf dXUpTask, dXUpRec, dOxUpSumNode, dOxUpSumPtr, dOxUpSumSrc;
    int64_t oxUpSums = 0;
    bool oneExchangeUsable(int which);
    bool cachesReady() const;
    bool oneExchangeLocal() const;  // this rank's (shard- and process-dependent) part, gathered at commInit
    // sticky time-out flag of the fused launch's in-kernel hand-offs, in host-visible
    // memory (the kernel stores 1 there when a wait gives up; checked at every API
    // entry and by sync(); read on the device only by the sharded block solve, which
    // sums it over the ranks inside its all-reduces)
    unsigned* topErr = nullptr;
    // ANISO_TOP_SPIN_LIMIT: polls of a tier counter (~1 us each) before a waiting block of
    // the fused launch computes the tier itself (tests: 0 makes every waiter compute)
    unsigned topSpinLimit = 1u << 16;
    bool useClusters = true;
    bool detSums = false;       // the clustered M2L's fixed-point sums (setDeterministic)
    bool detPerTarget = false;  // ANISO_DET_PER_TARGET
    void detBounds();           // dHmClBound from the plan (once)
    std::map<std::string, DevBuf> modeTabs;
    const CorrFold& corrTable(int K, int nterm, const int* ids, const double* mixes);
    std::map<std::string, CorrFold> corrTabs;
    int workK = 0;

    void ensureDevice();
  public:
    int deviceId() const { return device; }
  private:
    void uploadPlan();
    int device = -1;
    hipStream_t own = nullptr;
    // side stream of the harmonic block apply: near field + corrections run beside
    // the M2L (both HBM-bound, neither saturates alone)
    hipStream_t side = nullptr;
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    // x - mforward(x) fused into the down pass (ApplyCall::minuend)
    bool fuseSub = true;
    // the near field beside the up pass and the M2L on a side stream: -1 (default) on a
    // shard only -- one GPU runs them serially, 1.190 against 1.202 ms per block matvec
    // (same-process A/B, r05r; 1.148 against 1.162, r04ar): each kernel alone keeps
    // the load path busy, and the fork and join cost more than the overlap saves; a
    // rank of 8 overlaps (0.208 against 0.229 ms, r04ar).  ANISO_OVERLAP=0/1 forces it.
    int overlap = -1;
    bool overlapOn() const { return overlap < 0 ? plan.nranks > 1 : overlap != 0; }
    // stage timing: events recorded in-stream, (stage, start, end) spans per apply
    std::vector<hipEvent_t> evPool;
    int evUsed = 0;
    struct Span {
        int stage, a, b;
    };
    std::vector<Span> spans;
    int applies = 0;
    int mark(hipStream_t s);
    // The spans of one apply on stream s: a stage ends where end(stage) stands and starts at the
    // previous mark.  Level 1 records every stage, level 2 the roofline stages only (M2L, 2; near
    // field, 4): one that follows another stage has startRoofline() before it.  total(): the
    // span from the first mark (none: no total) to the last, and the apply is counted.
    struct StageSpans {
        Operator& op;
        const hipStream_t s;
        const bool tr = op.timeStages != 0, tm = op.timeStages == 1;
        int first, prev;  // the apply's first mark and its latest (-1: none): a new one, or the caller's (resumes)
        StageSpans(Operator& o, hipStream_t st) : op(o), s(st) { first = prev = tr ? op.mark(s) : -1; }
        StageSpans(Operator& o, hipStream_t st, int e0, int e) : op(o), s(st), first(e0), prev(e) {}  // resumes
        void start() { if (tr) prev = op.mark(s); }
        void startRoofline() { if (tr && !tm) prev = op.mark(s); }
        void end(int stage) {
            if (!(tm || (tr && (stage == 2 || stage == 4)))) return;
            const int e = op.mark(s);
            if (prev >= 0) op.spans.push_back({stage, prev, e});
            prev = e;
        }
        void total() {
            if (tr && !tm && first >= 0) prev = op.mark(s);
            if (tr && first >= 0 && prev >= 0) op.spans.push_back({7, first, prev});
            if (tr) ++op.applies;
        }
    };
    int maxNearS = 0;
    // geometry / tree on device
    DevBuf dPxT, dPyT, dPerm, dW, dNcx, dNcy, dNrx, dNry, dBegin, dCount, dParent, dSlot, dChild, dIsLeaf;
    DevBuf dLeaves, dNearPtr, dNearSrc, dNearKOff, dNearFOff, dM2LTgt, dM2LPtr, dM2LSrc, dM2LPairTgt;
    DevBuf dUpTaskPtr, dUpGrpPtr, dUpGrp, dUpNode, dUpCode, dUpDesc, dUpGrpFix, dUpGeom, dUpLeaf;                       // up-pass tiers
    DevBuf dDnTaskPtr, dDnGrpPtr, dDnGrp, dDnNode, dDnLeafPtr, dDnLeafSlot, dDnLeafIdx, dDnLeafPts, dDnPtsRange, dDnDesc, dDnGrpFix, dDnLeafGeom;  // down
    DevBuf dLeafInfo, dNearPtsPtr, dNearPts;
    DevBuf dNsPtr, dNsPts, dNearLoc;  // near field sources staged per workgroup (k_near_hs)
    DevBuf dNearCorrRow;              // d = 1: the stencil's table rows (corrections fused into k_near_hs)
    DevBuf dXT0Tasks, dXRootRecv, dXRootSlot, dXSendSlot;  // sharded up pass (plan.buildExchange)
    DevBuf dM2LNDir, dM2LCanonBase, dM2LInPtr, dM2LOutSlot, dM2LPart;  // symmetric M2L
    DevBuf dNearSym, dNearPart, dDnLeafNear, dDnNearPtr, dDnNearOff, dDnChainPtr, dDnChain;              // symmetric near field
    DevBuf dParams, dStCoef;
    DevBuf dCharge, dOut, dFT, dCT, dMult, dLocal, dSigmaS, dTmp, dTmp2;
    DevBuf dWT, dSigmaT, dIperm, dTmpS;  // tree-order path
    DevBuf dPadIn, dPadOut, dBlk;       // block operator: padded right-hand sides, x - mforward(x)
    DevBuf dHostIn, dHostOut, dSigAlt;  // host-pointer block operator: staging, sigma_s override
    std::vector<ModeCache> modes;
    Params hostP{};  // the parameter block uploaded to dParams
    // fp32 operator (buildF32): leaves with their directed U/W sources (padded to 16
    // columns), M2M / L2L levels, directed M2L pairs
    void buildF32();
    bool f32Ready = false;
    void buildMrhsPlan();  // the directed lists both 16-RHS operators share (f32 plan below)
    bool mrhsPlanReady = false;
    struct Mrhs64Cache {
        DevBuf Km2l, Knear;
    };
    std::map<int, Mrhs64Cache> m64;  // fp64 16-RHS caches per mode id
    void buildMrhs64(int id);
    size_t mrhs64Bytes();  // HBM a buildMrhs64 would allocate
    DevBuf d64Rup, d64Rdn, d64Mult, d64Local, d64FT, d64CT;
    DevBuf d32PairTgt, d32SrcPtr, d32SrcNodes, d32KoffD, d32SrcCount;  // cache-build inputs of the 16-RHS plan
    struct F32Plan {
        std::vector<int> leaves;
        std::vector<std::array<int, 4>> leafInfo;  // node, begin, count, padded sources
        std::vector<int64_t> nearPtr, koff, koffD, srcPtr;
        std::vector<int> nearPts, srcNodes, srcCount;
        std::vector<std::vector<int>> m2m, l2l;  // per level: M2M bottom-up, L2L top-down
        std::vector<int> m2lTgt, m2lSrc, m2lPairTgt;
        std::vector<int64_t> m2lPtr;
        int64_t nearTiles = 0, nearD = 0;
        int maxSrc = 1;
    } f32;
    DevBuf d32Leaves, d32LeafInfo, d32NearPtr, d32NearPts, d32Koff, d32Tgt, d32Ptr, d32Src;
    DevBuf d32Km2l, d32Knear, d32Rup, d32Rdn, d32Mult, d32Local, d32FT, d32CT, d32Level;
    std::vector<DevBuf> d32LevelNodes;  // m2m levels then l2l levels
};

}  // namespace aniso
