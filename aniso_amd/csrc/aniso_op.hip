// aniso_op.hip -- host orchestration of the MI355X operator (one per handle).
//
// Lifecycle mirrors the reference's MEX ops (AnisoWrapper.cpp:10-136):
//   Operator()  <- 'new'       geometry + quadtree + lists on the host (no GPU)
//   setCoeff    <- 'setCoeff'  sigma coefficients; uploads geometry/tree to HBM
//   cache(m)    <- 'cache'     device-side build of the merged pair operators
//   mapping*    <- 'mapping'   one apply, all stages on the GPU
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>

#include "aniso_op.hpp"
#include "kernels.hpp"

namespace aniso {

[[noreturn]] void throw_hip(hipError_t e, const char* file, int line) {
    throw std::runtime_error(std::string("HIP error ") + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ") at " +
                             file + ":" + std::to_string(line));
}

#define HIP_CHECK(x)                                         \
    do {                                                     \
        hipError_t e__ = (x);                                \
        if (e__ != hipSuccess) throw_hip(e__, __FILE__, __LINE__); \
    } while (0)

DevBuf::~DevBuf() {
    if (p) (void)hipFree(p);
}

void DevBuf::alloc(size_t nbytes) {
    if (p && bytes == nbytes) return;
    if (p) {
        HIP_CHECK(hipFree(p));
        p = nullptr;
    }
    // a failed allocation leaves an empty buffer (p = null, bytes = 0), never a size without
    // memory behind it: callers that grow a kept buffer compare `bytes` only
    bytes = 0;
    if (nbytes) {
        const hipError_t e = hipMalloc(&p, nbytes);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();  // the next launch check must not report this again
            throw_hip(e, __FILE__, __LINE__);
        }
    }
    bytes = nbytes;
}

void DevBuf::upload(const void* host, size_t nbytes) {
    alloc(nbytes);
    if (nbytes) HIP_CHECK(hipMemcpy(p, host, nbytes, hipMemcpyHostToDevice));
}

template <class T>
static void up(DevBuf& b, const std::vector<T>& v) {
    b.upload(v.data(), v.size() * sizeof(T));
}

static int host_threads() {
    unsigned n = std::thread::hardware_concurrency();
    return n ? (int)std::min(n, 16u) : 4;
}

// the K x K mix of one mode applied to K columns
static std::vector<double> identityMix(int K) {
    std::vector<double> mix((size_t)K * K, 0.0);
    for (int i = 0; i < K; ++i) mix[(size_t)i * K + i] = 1.0;
    return mix;
}

Operator::Operator(int sz, int d, int ks_, double g_, int ns_, int np_, int maxLevel_, int shardRank, int shardRanks)
    : ks(ks_), ns(ns_), np(np_), maxLevel(maxLevel_), g(g_) {
    if (ks < 1) throw std::invalid_argument("kernel size must be >= 1");
    if (np != 4 && np != 6 && np != 8)
        throw std::invalid_argument("np must be 4, 6 or 8 on the MI355X path (Chebyshev rank 16, 36 or 64), got " +
                                    std::to_string(np));
    if (d < 1 || d > kMaxD) throw std::invalid_argument("quadRule must be in 1..6 on the MI355X path");
    if (maxLevel < 0) throw std::invalid_argument("maxLevel must be >= 0");
    kernelSize = 2 * ks - 1;
    geo.build(sz, d, ns);
    tree.build(geo.px.data(), geo.py.data(), geo.N, np * np, maxLevel, host_threads());
    // symmetric U storage pays for single right-hand sides; a block handle (ks > 1,
    // the aniso.m operator) reads every near block directed.
    // ANISO_NEAR_SYMMETRIC=0/1 overrides.
    plan.nearSymmetric = ks == 1;
    if (const char* e = std::getenv("ANISO_NEAR_SYMMETRIC")) plan.nearSymmetric = e[0] == '1';
    plan.maxCanon = ks == 1 ? kMaxCanon : kMaxCanonBlock;
    // ANISO_UPPER_PARTIAL=0: a sharded one-collective matvec exchanges the tier-0 roots
    // and runs the upper up tiers on every rank (the round-4 form)
    if (const char* e = std::getenv("ANISO_UPPER_PARTIAL")) plan.xUpPartialIn = std::atoi(e) != 0;
    if (highOrder()) {  // the mode-shared caches only (ks = 1 too), directed near lists, no rank-16 schedules
        plan.nearSymmetric = false;
        plan.listsOnly = true;
        hoShard = shardRanks != 0;  // the rank's own lists; setShard keeps refusing
    }
    if (hoShard) plan.build(tree, np, shardRank, shardRanks);
    else plan.build(tree, np, 0, 1);
    if (!highOrder()) {
        plan.buildExchange(tree, geo.sz, geo.d2);
        plan.buildTopWait(tree);
    }
    // block handles apply aniso.m's operator through the mode-shared E caches
    // (DESIGN.md §3.9); ANISO_HARMONIC=0 keeps the per-mode operator stream
    useAtt = ks > 1 && !plan.nearSymmetric;
    if (const char* e = std::getenv("ANISO_HARMONIC")) useAtt = useAtt && e[0] != '0';
    if (highOrder()) useAtt = true;
    if (const char* e = std::getenv("ANISO_OVERLAP")) overlap = std::atoi(e);
    if (const char* e = std::getenv("ANISO_FUSE_SUB")) fuseSub = e[0] != '0';
    if (const char* e = std::getenv("ANISO_TOP_SPIN_LIMIT")) topSpinLimit = (unsigned)std::strtoul(e, nullptr, 10);
    if (const char* e = std::getenv("ANISO_TOP_TRACE")) topTraceOn = std::atoi(e) != 0;
    if (const char* e = std::getenv("ANISO_NEAR_EARLY")) nearEarly = std::atoi(e) != 0;
    if (const char* e = std::getenv("ANISO_ONE_EXCHANGE")) oneXOn = std::atoi(e) != 0;
    if (const char* e = std::getenv("ANISO_DET_PER_TARGET")) detPerTarget = std::atoi(e) != 0;
    if (const char* e = std::getenv("ANISO_NEAR_UP")) nearUpOn = std::atoi(e) != 0;
    if (const char* e = std::getenv("ANISO_TOP_FUSED")) topFusedMode = std::atoi(e) != 0 ? 1 : 0;
    if (const char* e = std::getenv("ANISO_DIRECT_TARGETS")) directChunk = std::min(std::max(std::atoi(e), 1), 65535);
    sigma_s.assign(geo.N, 0.0);
    sigma_t.assign(geo.N, 0.0);
    modes.resize(kernelSize);
}

Operator::~Operator() {
    if (device >= 0) {
        int prev = -1;  // restore the caller's device (the destructor runs from Python __del__)
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        if (comm) {  // the communicator before the streams its collectives ran on
            (void)hipDeviceSynchronize();
            comm.reset();
        }
        for (auto& e : evPool) (void)hipEventDestroy(e);
        if (evFork) (void)hipEventDestroy(evFork);
        if (evJoin) (void)hipEventDestroy(evJoin);
        if (evDirect) (void)hipEventDestroy(evDirect);
        if (side) (void)hipStreamDestroy(side);
        if (own) (void)hipStreamDestroy(own);
        if (topErr) (void)hipHostFree(topErr);
        if (s16Stat) (void)hipHostFree(s16Stat);
        if (s16Ev) (void)hipEventDestroy(s16Ev);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
}

void Operator::getNodes(double* xy) const {
    for (int64_t i = 0; i < geo.N; ++i) {
        xy[i] = geo.px[i];
        xy[i + geo.N] = geo.py[i];
    }
}

void Operator::setShard(int rank, int nranks) {
    if (highOrder() && nranks > 1)
        throw std::invalid_argument("aniso_set_shard: a high-order handle (np = " + std::to_string(np) +
                                    ") is unsharded only, got nranks = " + std::to_string(nranks));
    if (comm) {  // a communicator belongs to one shard layout; drain its collectives first
        if (device >= 0) HIP_CHECK(hipDeviceSynchronize());
        comm.reset();
        oxReady = false;
    }
    plan.build(tree, np, rank, nranks);
    if (!highOrder()) {
        plan.buildExchange(tree, geo.sz, geo.d2);
        plan.buildTopWait(tree);
    }
    pend = Pending();
    for (auto& m : modes) {
        m.Knear.alloc(0);
        m.Km2l.alloc(0);
        m.tables = m.resident = false;
    }
    f32Ready = false;
    mrhsPlanReady = false;
    m64.clear();
    if (device >= 0) uploadPlan();
    if (device >= 0 && hoShard) uploadHighPlan();  // (rank 0 of 1: its L2L lists follow the own range)
}

void Operator::refuseHighPlain(const char* what) const {
    if (highOrder() && !hoShard)
        throw std::logic_error(std::string(what) + ": a high-order handle (np = " + std::to_string(np) +
                               ") made by aniso_create is unsharded only; aniso_create_sharded makes the handle "
                               "of one rank of a sharded high-order operator");
}

void Operator::refuseHoShard(const char* what) const {
    if (hoShard)
        throw std::logic_error(std::string(what) + ": a sharded high-order handle (aniso_create_sharded, np = " +
                               std::to_string(np) + ", rank " + std::to_string(plan.rank) + " of " +
                               std::to_string(plan.nranks) + ") runs aniso_block_op_sharded_dev, aniso_block_op_dev in "
                               "tree order and aniso_block_solve_sharded_dev only");
}

void Operator::ensureDevice() {
    if (device >= 0) {
        HIP_CHECK(hipSetDevice(device));
        return;
    }
    HIP_CHECK(hipGetDevice(&device));
    HIP_CHECK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    // side stream at normal priority (a high-priority one measured slower, r01f; the
    // lowest priority 11-25 % slower, r04l; a CU-masked one serialised the two streams
    // on a rank of 8: 0.455 against 0.235 ms, r06q)
    HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&evFork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&evJoin, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&evDirect, hipEventDisableTiming));
    HIP_CHECK(hipHostMalloc((void**)&topErr, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent));
    *(volatile unsigned*)topErr = 0;
    // tree-order coordinates
    std::vector<double> pxT(geo.N), pyT(geo.N);
    for (int64_t k = 0; k < geo.N; ++k) {
        pxT[k] = geo.px[tree.perm[k]];
        pyT[k] = geo.py[tree.perm[k]];
    }
    up(dPxT, pxT);
    up(dPyT, pyT);
    up(dPerm, tree.perm);
    up(dW, geo.w);
    std::vector<double> wT(geo.N);
    for (int64_t k = 0; k < geo.N; ++k) wT[k] = geo.w[tree.perm[k]];
    up(dWT, wT);
    std::vector<int> iperm(geo.N);
    for (int64_t k = 0; k < geo.N; ++k) iperm[tree.perm[k]] = (int)k;
    up(dIperm, iperm);
    up(dNcx, tree.ncx);
    up(dNcy, tree.ncy);
    up(dNrx, tree.nrx);
    up(dNry, tree.nry);
    up(dBegin, tree.begin);
    up(dCount, tree.count);
    up(dParent, tree.parent);
    up(dSlot, tree.slot);
    std::vector<int4> ch(tree.nn);
    for (int i = 0; i < tree.nn; ++i) ch[i] = make_int4(tree.child[i][0], tree.child[i][1], tree.child[i][2], tree.child[i][3]);
    for (auto& c : ch) {  // leaves: point children at self (never dereferenced for non-leaves)
        if (c.x < 0) c = make_int4(0, 0, 0, 0);
    }
    up(dChild, ch);
    // parameter block
    Params P;
    std::memset(&P, 0, sizeof(P));
    P.sz = geo.sz;
    P.d = geo.d;
    P.d2 = geo.d2;
    P.nsq = geo.nsq;
    P.dx = geo.dx;
    for (int i = 0; i < geo.d; ++i) {
        P.gx[i] = geo.gx[i];
        P.gw[i] = geo.gw[i];
    }
    // Chebyshev nodes / polynomials / transfer operators (bbfmm.h:597-693)
    for (int i = 0; i < kNP; ++i) P.cheb[i] = -std::cos((i + 0.5) * M_PI / kNP);
    for (int i = 0; i < kNP; ++i) {
        double T[kNP];
        T[0] = 1.0;
        T[1] = P.cheb[i];
        for (int l = 2; l < kNP; ++l) T[l] = 2.0 * P.cheb[i] * T[l - 1] - T[l - 2];
        for (int l = 0; l < kNP; ++l) P.tnode[i + l * kNP] = T[l];
    }
    double S[2 * kNP][kNP];
    for (int k = 0; k < 2 * kNP; ++k) {
        double s = (k < kNP) ? -0.5 + 0.5 * P.cheb[k] : 0.5 + 0.5 * P.cheb[k - kNP];
        double T[kNP];
        T[0] = 1.0;
        T[1] = s;
        for (int l = 2; l < kNP; ++l) T[l] = 2.0 * s * T[l - 1] - T[l - 2];
        for (int i = 0; i < kNP; ++i) {
            double acc = 0.0;
            for (int l = 0; l < kNP; ++l) acc += T[l] * P.tnode[i + l * kNP];
            S[k][i] = (2.0 * acc - 1.0) * (1.0 / kNP);
        }
    }
    for (int id = 0; id < 4; ++id) {
        int b0 = id & 1, b1 = (id >> 1) & 1;
        for (int i = 0; i < kNP; ++i)
            for (int j = 0; j < kNP; ++j)
                for (int k = 0; k < kNP; ++k)
                    for (int l = 0; l < kNP; ++l)
                        P.R[id][(i * kNP + j) + (k * kNP + l) * kRank] = S[b1 * kNP + i][k] * S[b0 * kNP + j][l];
    }
    const int d2 = geo.d2;
    for (int i = 0; i < d2 * d2; ++i) P.interp[i] = geo.interp[i];
    for (int i = 0; i < d2; ++i) P.sqrtW[i] = geo.sqrtW[i];
    CorrTables ct;
    ct.build(geo, 0);
    for (size_t i = 0; i < ct.legB.size(); ++i) P.legB[i] = ct.legB[i];
    for (int i = 0; i < d2; ++i) P.coefScale[i] = ct.coefScale[i];
    dParams.upload(&P, sizeof(P));
    hostP = P;
    // work arrays
    dCharge.alloc(geo.N * sizeof(double));
    dOut.alloc(geo.N * sizeof(double));
    dTmp.alloc(geo.N * sizeof(double));
    dTmp2.alloc(geo.N * sizeof(double));
    dTmpS.alloc(geo.N * sizeof(double));
    ensureWork(1);
    uploadPlan();
    if (highOrder()) uploadHighPlan();
}

// The order-dependent tables and the level lists of a high-order handle's far field
// (high_order.hip): per node its children (-1: empty or none), the parents of each level
// bottom-up (M2M), the nodes of each level >= 2 top-down (L2L).  The levels are those of
// the 16-right-hand-side plan (buildMrhsPlan); the leaves, the M2L targets and their
// pairs are the plan's own lists.
void Operator::uploadHighPlan() {
    HoTables tab;
    ho_tables(np, &tab);
    dHoTab.upload(&tab, sizeof(tab));
    const Tree& t = tree;
    std::vector<int4> ch(t.nn);
    for (int i = 0; i < t.nn; ++i) {
        int c[4];
        for (int q = 0; q < 4; ++q) {
            c[q] = t.isLeaf[i] ? -1 : t.child[i][q];
            if (c[q] >= 0 && t.isEmpty[c[q]]) c[q] = -1;
            if (c[q] >= 0 && (t.parent[c[q]] != i || t.slot[c[q]] != q))
                throw std::logic_error("high-order plan: child slot mismatch");
        }
        ch[i] = make_int4(c[0], c[1], c[2], c[3]);
    }
    up(dHoChild, ch);
    const int D = t.maxLevel;
    std::vector<std::vector<int>> m2m(D + 1), l2l(D + 1);
    // a sharded handle (hoShard): the up pass covers the whole tree on every rank, the L2L
    // only the nodes that intersect the own range -- no other local is ever read
    auto mine = [&](int n) {
        return !hoShard || (t.begin[n] < plan.ownEnd && t.begin[n] + t.count[n] > plan.ownBegin);
    };
    for (int i = 0; i < t.nn; ++i) {
        if (t.isEmpty[i] || t.parent[i] < 0) continue;
        if (!t.isLeaf[i]) m2m[t.level[i]].push_back(i);
        if (t.level[i] >= 2 && mine(i)) l2l[t.level[i]].push_back(i);
    }
    if (hoShard) {  // every non-empty leaf, as Plan::leafInfo's {node, begin, count, -}: the replicated P2M
        std::vector<int4> all;
        for (int i = 0; i < t.nn; ++i)
            if (t.isLeaf[i] && !t.isEmpty[i]) all.push_back(make_int4(i, (int)t.begin[i], (int)t.count[i], 0));
        hoLeafAll = (int)all.size();
        up(dHoLeafAll, all);
    }
    std::vector<int> a, b;
    hoM2mPtr.assign(1, 0);
    for (int l = D; l >= 1; --l) {
        a.insert(a.end(), m2m[l].begin(), m2m[l].end());
        hoM2mPtr.push_back((int)a.size());
    }
    hoL2lPtr.assign(1, 0);
    for (int l = 2; l <= D; ++l) {
        b.insert(b.end(), l2l[l].begin(), l2l[l].end());
        hoL2lPtr.push_back((int)b.size());
    }
    up(dHoM2m, a);
    up(dHoL2l, b);
}

// Per-right-hand-side work arrays, sized for the largest K used so far:
// fT/cT [N][K], multipoles and locals [node][16][K], M2L and near partials.
void Operator::ensureWork(int K) {
    if (K <= workK) return;
    workK = K;
    dFT.alloc((size_t)geo.N * rhs_stride(K) * sizeof(double));
    dCT.alloc((size_t)geo.N * rhs_stride(K) * sizeof(double));
    dMult.alloc((size_t)tree.nn * kRank * K * sizeof(double));
    dLocal.alloc((size_t)tree.nn * kRank * K * sizeof(double));
    HIP_CHECK(hipMemset(dMult.p, 0, dMult.bytes));
    HIP_CHECK(hipMemset(dLocal.p, 0, dLocal.bytes));
    dM2LPart.alloc((size_t)std::max(plan.m2lCanon, 1) * kRank * K * sizeof(double));
    dNearPart.alloc((size_t)std::max<int64_t>(plan.nearPartTotal, 1) * K * sizeof(double));
}

static std::vector<int4> to_int4(const std::vector<std::array<int, 4>>& v) {
    std::vector<int4> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = make_int4(v[i][0], v[i][1], v[i][2], v[i][3]);
    return o;
}

void Operator::uploadPlan() {
    up(dLeaves, plan.leaves);
    up(dNearPtr, plan.nearPtr);
    up(dNearSrc, plan.nearSrc);
    up(dNearKOff, plan.nearKOff);
    up(dNearFOff, plan.nearFOff);
    up(dM2LTgt, plan.m2lTgt);
    up(dM2LPtr, plan.m2lPtr);
    up(dM2LSrc, plan.m2lSrc);
    std::vector<int> pairTgt(plan.m2lSrc.size());
    for (size_t i = 0; i < plan.m2lTgt.size(); ++i)
        for (int64_t p = plan.m2lPtr[i]; p < plan.m2lPtr[i + 1]; ++p)  // ~target: canonical (column-major) block
            pairTgt[p] = p < plan.m2lPtr[i] + plan.m2lNDir[i] ? plan.m2lTgt[i] : ~plan.m2lTgt[i];
    up(dM2LPairTgt, pairTgt);
    up(dM2LNDir, plan.m2lNDir);
    if (useAtt) {
        up(dAttPtr, plan.attPtr);
        up(dAttSrc, plan.attSrc);
        up(dAttBlk, plan.attBlk);
        std::vector<int> own(plan.attOwner), oth(plan.attOther);  // stored blocks, then the cluster plan's copies
        own.insert(own.end(), plan.hmCopyOwner.begin(), plan.hmCopyOwner.end());
        oth.insert(oth.end(), plan.hmCopyOther.begin(), plan.hmCopyOther.end());
        up(dAttOwner, own);
        up(dAttOther, oth);
        up(dHmClPtr, plan.hmClPtr);
        up(dHmTgt, plan.hmTgt);
        up(dHmPtr, plan.hmPtr);
        up(dHmSrc, plan.hmSrc);
        up(dHmBlk, plan.hmBlk);
        up(dHmSlot, plan.hmSlot);
        up(dHmNDir, plan.hmNDir);
        up(dHmClWait, plan.hmClWait);
        up(dHmHaloPtr, plan.hmHaloPtr);
        up(dHmHaloPos, plan.hmHaloPos);
        dHmClBound.alloc(0);  // the deterministic sums' bounds follow the plan (detBounds)
        dTopCnt.alloc((kMaxTopTiers + 1) * sizeof(unsigned));
        dTopSteals.alloc(sizeof(unsigned));
        HIP_CHECK(hipMemset(dTopSteals.p, 0, sizeof(unsigned)));
        attReady = false;
        dropCacheF32();
        modeBlocks.blocks.clear();
        modeNearBlocks.blocks.clear();
    }
    up(dM2LCanonBase, plan.m2lCanonBase);
    up(dM2LInPtr, plan.m2lInPtr);
    up(dM2LOutSlot, plan.m2lOutSlot);
    dM2LPart.alloc((size_t)std::max(plan.m2lCanon, 1) * kRank * workK * sizeof(double));
    std::vector<int2> ns(plan.nearSym.size());
    for (size_t i = 0; i < ns.size(); ++i) ns[i] = make_int2(plan.nearSym[i][0], plan.nearSym[i][1]);
    up(dNearSym, ns);
    up(dDnLeafNear, plan.dnLeafNear);
    up(dDnDesc, to_int4(plan.dnDesc));
    up(dDnGrpFix, plan.dnGrpFix);
    up(dDnLeafGeom, plan.dnLeafGeom);
    up(dDnChainPtr, plan.dnChainPtr);
    up(dDnChain, plan.dnChain);
    up(dDnChainFold, plan.dnChainFold);
    up(dDnNearPtr, plan.dnNearPtr);
    up(dDnNearOff, plan.dnNearOff);
    dNearPart.alloc((size_t)std::max<int64_t>(plan.nearPartTotal, 1) * workK * sizeof(double));
    up(dLeafInfo, to_int4(plan.leafInfo));
    up(dNearPtsPtr, plan.nearPtsPtr);
    up(dNearPts, plan.nearPts);
    up(dXT0Tasks, plan.xT0Tasks);
    up(dXOwnT0Tasks, plan.xOwnT0Tasks);
    up(dXUpTask, plan.xUpTask);
    up(dNearUpGrp, plan.nearUpGrp);
    up(dNearGrpEarly, plan.nearGrpEarly);
    up(dNearGrpLate, plan.nearGrpLate);
    up(dXRootRecv, plan.xRootRecv);
    up(dNsPtr, plan.nsPtr);
    up(dNsPts, plan.nsPts);
    up(dNearLoc, plan.nearLoc);
    up(dNearCorrRow, plan.nearCorrRow);
    up(dXRootSlot, plan.xRootSlot);
    up(dXSendSlot, plan.xSendSlot);
    up(dUpTaskPtr, plan.upTaskPtr);
    up(dUpGrpPtr, plan.upGrpPtr);
    up(dUpGrp, plan.upGrp);
    up(dUpNode, plan.upNode);
    up(dUpCode, to_int4(plan.upCode));
    up(dUpDesc, to_int4(plan.upDesc));
    up(dUpGrpFix, plan.upGrpFix);
    up(dUpGeom, plan.upGeom);
    up(dUpLeaf, plan.upLeaf);
    up(dDnTaskPtr, plan.dnTaskPtr);
    up(dDnGrpPtr, plan.dnGrpPtr);
    up(dDnGrp, plan.dnGrp);
    up(dDnNode, to_int4(plan.dnNode));
    up(dDnLeafPtr, plan.dnLeafPtr);
    up(dDnLeafSlot, plan.dnLeafSlot);
    up(dDnLeafIdx, plan.dnLeafIdx);
    up(dDnLeafPts, plan.dnLeafPts);
    up(dDnPtsRange, plan.dnPtsRange);
    // a task's expansions live in LDS (<= 4 levels: 85 nodes); a workgroup may use all 160 KiB
    if (up_tier_lds(plan.upMaxTask, 1) > 160 * 1024 ||
        down_tier_lds(plan.dnMaxTask, plan.dnMaxLeaves, plan.dnMaxNear, plan.dnMaxChain, 1) > 160 * 1024)
        throw std::logic_error("up/down pass task exceeds one workgroup's LDS");
    maxNearS = 1;
    for (size_t li = 0; li < plan.leaves.size(); ++li) {
        int64_t S = 0;
        for (int64_t j = plan.nearPtr[li]; j < plan.nearPtr[li + 1]; ++j) S += tree.count[plan.nearSrc[j]];
        maxNearS = std::max<int>(maxNearS, (int)S);
    }
}

// setCoeff (AnisoWrapper.cpp:46-69): sigma copies + interpolation() (KernelFactory.cpp:212-227);
// singPrecompute() lives in Geometry; the device keeps sigma_t's coefficients / legendreNorms.
void Operator::setCoeff(const double* ss, const double* st) {
    ensureDevice();
    std::memcpy(sigma_s.data(), ss, geo.N * sizeof(double));
    std::memcpy(sigma_t.data(), st, geo.N * sizeof(double));
    const int d2 = geo.d2;
    std::vector<double> coef((size_t)geo.nsq * d2);
    std::vector<double> lt(d2);
    for (int i = 0; i < geo.nsq; ++i) {
        for (int j = 0; j < d2; ++j) lt[j] = geo.sqrtW[j] * st[(size_t)i * d2 + j];
        for (int r = 0; r < d2; ++r) {
            double s = 0.0;
            for (int k = 0; k < d2; ++k) s += geo.interp[r + (size_t)k * d2] * lt[k];
            coef[(size_t)i * d2 + r] = s / geo.lnorm[r];
        }
    }
    up(dStCoef, coef);
    up(dSigmaS, sigma_s);
    std::vector<double> sT(geo.N);
    for (int64_t k = 0; k < geo.N; ++k) sT[k] = sigma_s[tree.perm[k]];
    up(dSigmaT, sT);
    for (auto& m : modes) m.tables = m.resident = false;
    attReady = false;
    dropCacheF32();    // the float mirrors are rounded from the shared caches of sigma_t
    modeBlocks.blocks.clear();  // ... and the resident mode blocks are formed from them
    modeNearBlocks.blocks.clear();
    f32Ready = false;  // config 5's fp32 caches are rounded from the mode-0 operators of sigma_t
    m64.clear();       // ... and the fp64 16-RHS caches are the modes' operators
    coeffSet = true;
}

// cache(Id) (AnisoWrapper.cpp:72-90): runKernelsCache + runKernelsCacheSing
// (merged operators, built on the GPU), refineAddOnCache + singularAddCache
// (translation-invariant stencil tables, built on the host).
void Operator::cache(int id) {
    if (id < 0 || id >= kernelSize)
        throw std::out_of_range("kernel id " + std::to_string(id) + " out of range [0, " + std::to_string(kernelSize) + ")");
    if (!coeffSet) throw std::runtime_error("cache called before setCoeff");
    ensureDevice();
    ModeCache& mc = modes[id];
    if (highOrder()) {  // the mode's tables on the mode-shared caches: no Km2l / Knear
        if (!attReady) buildAttCache();
        HIP_CHECK(hipDeviceSynchronize());  // queued work may still read the folded tables
        CorrTables ct;
        ct.build(geo, id);
        up(mc.C, ct.C);
        up(mc.mu, ct.mu);
        mc.hostC = ct.C;
        mc.hostMu = ct.mu;
        corrTabs.clear();
        mc.tables = true;
        return;
    }
    if (id == 0) f32Ready = false;  // rebuilt from the new mode-0 operators at the next fp32 apply
    m64.erase(id);
    mc.Knear.alloc((size_t)plan.nearKTotal * sizeof(double));
    mc.Km2l.alloc((size_t)plan.storedM2L * 256 * sizeof(double));
    const Params* P = dParams.as<Params>();
    int maxSrc = 1;
    for (size_t li = 0; li < plan.leaves.size(); ++li)
        maxSrc = std::max<int>(maxSrc, (int)(plan.nearPtr[li + 1] - plan.nearPtr[li]));
    launch_cache_m2l(plan.storedM2L, dM2LPairTgt.as<int>(), dM2LSrc.as<int>(), nodeBoxes(), dStCoef.as<double>(), P, id,
                     mc.Km2l.as<double>(), own);
    launch_cache_near((int)plan.leaves.size(), dLeaves.as<int>(), dNearPtr.as<int64_t>(), dNearSrc.as<int>(),
                      dNearKOff.as<int64_t>(), dBegin.as<int64_t>(), dCount.as<int64_t>(), treePoints(),
                      dStCoef.as<double>(), P, id, maxSrc, mc.Knear.as<double>(), own);
    if (useAtt && !attReady) buildAttCache();
    CorrTables ct;
    ct.build(geo, id);
    up(mc.C, ct.C);
    up(mc.mu, ct.mu);
    mc.hostC = ct.C;
    mc.hostMu = ct.mu;
    HIP_CHECK(hipStreamSynchronize(own));  // folded tables may still be read by queued work
    corrTabs.clear();
    HIP_CHECK(hipStreamSynchronize(own));
    mc.tables = mc.resident = true;
}

// cacheBlock: every mode made usable by the block operator on the mode-shared caches
// (DESIGN.md §3.9.2): those caches once, and per mode the host-built correction tables
// only -- no Km2l / Knear.  The operator buffers of modes that are not resident (left
// by an earlier setCoeff) are freed, so afterwards a mode holds operators only if
// cache(id) built them since the last setCoeff.
void Operator::cacheBlock() {
    if (ks < 2 && !highOrder()) throw std::invalid_argument("aniso_cache_block: a handle of one block (ks = 1) has no block operator on the mode-shared caches; use aniso_cache(id)");
    if (plan.nearSymmetric)
        throw std::invalid_argument("aniso_cache_block: symmetric near storage (ANISO_NEAR_SYMMETRIC=1) runs the block operator on the per-mode operators; use aniso_cache(id)");
    if (!useAtt)
        throw std::invalid_argument("aniso_cache_block: the mode-shared caches are off (ANISO_HARMONIC=0), the block operator streams the per-mode operators; use aniso_cache(id)");
    if (!coeffSet) throw std::runtime_error("aniso_cache_block called before setCoeff");
    ensureDevice();
    if (!attReady) buildAttCache();
    // queued work (on the caller's streams too) may still read the stale operators or
    // the folded tables
    HIP_CHECK(hipDeviceSynchronize());
    for (int id = 0; id < kernelSize; ++id) {
        ModeCache& mc = modes[id];
        if (!mc.resident) {
            mc.Knear.alloc(0);
            mc.Km2l.alloc(0);
        }
        if (mc.tables) continue;
        CorrTables ct;
        ct.build(geo, id);
        up(mc.C, ct.C);
        up(mc.mu, ct.mu);
        mc.hostC = ct.C;
        mc.hostMu = ct.mu;
    }
    corrTabs.clear();
    for (auto& mc : modes) mc.tables = true;
}

void Operator::cacheBytes(int64_t bytes[2]) const {
    bytes[0] = 0;
    for (const auto& mc : modes) bytes[0] += (int64_t)(mc.Km2l.bytes + mc.Knear.bytes);
    bytes[1] = (int64_t)(dAttM2L.bytes + dAttNear.bytes + dSigDiag.bytes);
}

void Operator::dropCacheF32() {
    dAttM2LF.alloc(0);
    dAttNearF.alloc(0);
}

// The float mirrors of dAttM2L and dAttNear: one conversion launch.
void Operator::cacheF32() {
    if (!highOrder())
        throw std::logic_error("aniso_cache_f32: an np = 4 handle has no f32 mode operator (its reduced-precision "
                               "route is aniso_solve_mixed_dev)");
    refuseHoShard("aniso_cache_f32");
    if (!coeffSet || !attReady || !modes[0].tables)
        throw std::runtime_error("aniso_cache_f32 before aniso_set_coeff and aniso_cache(0) or aniso_cache_block");
    // (an array without entries -- a tree without M2L pairs -- has no mirror to build)
    if ((dAttM2LF.p || !dAttM2L.bytes) && (dAttNearF.p || !dAttNear.bytes)) return;
    ensureDevice();
    const size_t na = dAttM2L.bytes / sizeof(double), nb = dAttNear.bytes / sizeof(double);
    try {
        dAttM2LF.alloc(na * sizeof(float));
        dAttNearF.alloc(nb * sizeof(float));
    } catch (const std::exception& e) {
        dropCacheF32();
        throw std::runtime_error("aniso_cache_f32: the float mirrors of " + std::to_string(na * sizeof(float)) + " + " +
                                 std::to_string(nb * sizeof(float)) + " bytes could not be allocated: " + e.what());
    }
    launch_cache_f32((int64_t)na, dAttM2L.as<double>(), dAttM2LF.as<float>(), (int64_t)nb, dAttNear.as<double>(),
                     dAttNearF.as<float>(), own);
    HIP_CHECK(hipStreamSynchronize(own));
}

void Operator::setWide(int on) {
    if (on != 0 && on != 1) throw std::invalid_argument("aniso_set_wide: on must be 0 or 1, got " + std::to_string(on));
    if (on) {
        if (!highOrder())
            throw std::logic_error("aniso_set_wide: the 16-column chunks and solve groups are built for np = 6, 8; an "
                                   "np = 4 handle keeps chunks and groups of 8");
        refuseHoShard("aniso_set_wide");
        if (plan.nranks > 1) throw std::logic_error("aniso_set_wide on a sharded handle (use an unsharded handle)");
    }
    wideOn = on != 0;
}

// One mode's resident factor blocks of either kind: one launch.
// Everything that can be refused is refused before the device is touched.
void ResidentBlocks::free(int id) {
    if (blocks.empty() || (id >= 0 && !blocks.count(id))) return;
    HIP_CHECK(hipDeviceSynchronize());  // queued applies (on the caller's streams too) may still read them
    if (id < 0) blocks.clear();
    else blocks.erase(id);
}

int64_t ResidentBlocks::bytes() const {
    int64_t b = 0;
    for (const auto& m : blocks) b += (int64_t)m.second.bytes;
    return b;
}

void Operator::cacheResident(const char* api, const char* built, const char* noun, bool needDirected, int id,
                             ResidentBlocks& rb, size_t need, const std::function<void(double*)>& build) {
    const std::string a(api), what = a + ": the " + noun;
    if (id < 0 || id >= kernelSize)
        throw std::out_of_range(a + ": kernel id " + std::to_string(id) + " out of range [0, " +
                                std::to_string(kernelSize) + ")");
    if (!highOrder())
        throw std::logic_error(a + ": the " + built + " are built for np = 6, 8; the resident route of an np = 4 handle "
                                   "is aniso_cache(h, id)");
    refuseHoShard(api);
    if (plan.nranks > 1) throw std::logic_error(a + " on a sharded handle (use an unsharded handle)");
    if (!coeffSet || !attReady || !modes[id].tables)
        throw std::runtime_error(a + " before aniso_set_coeff and aniso_cache(" + std::to_string(id) +
                                 ") or aniso_cache_block");
    if (needDirected && plan.nearPartTotal != 0)
        throw std::logic_error(a + ": the near E blocks are not stored directed");
    if (rb.blocks.count(id)) return;
    ensureDevice();
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    const std::string sizes = std::to_string(need) + " bytes for mode " + std::to_string(id) + ", " +
                              std::to_string(freeB) + " bytes of HBM free";
    if (need + (size_t)(1ull << 30) > freeB)  // keep a GiB of headroom
        throw std::runtime_error(what + " do not fit with a GiB to spare: " + sizes);
    DevBuf F;
    try {
        F.alloc(need);
    } catch (const std::exception& e) {
        throw std::runtime_error(what + " could not be allocated: " + sizes + ": " + e.what());
    }
    build(F.as<double>());
    HIP_CHECK(hipStreamSynchronize(own));
    rb.blocks.emplace(id, std::move(F));
}

// (as many bytes as the E blocks: F_id of every stored pair)
void Operator::cacheMode(int id) {
    const size_t need = dAttM2L.bytes, rank = (size_t)np * np;
    cacheResident("aniso_cache_mode", "resident mode blocks", "resident blocks", false, id, modeBlocks, need,
                  [&](double* F) {
                      launch_ho_mode_blocks(np, id, (int64_t)(need / (rank * rank * sizeof(double))), dAttOwner.as<int>(),
                                            dAttOther.as<int>(), dAttM2L.as<double>(), nodeBoxes(),
                                            dHoTab.as<HoTables>(), F, own);
                  });
}

void Operator::cacheModeFree(int id) {
    if (id < -1 || id >= kernelSize)
        throw std::out_of_range("aniso_cache_mode_free: kernel id " + std::to_string(id) + " out of range [-1, " +
                                std::to_string(kernelSize) + ")");
    modeBlocks.free(id);
}

int64_t Operator::cacheModeBytes() const { return modeBlocks.bytes(); }

// One mode's resident near blocks: the directed near E blocks with the
// sources of every leaf padded to 16, one launch.
void Operator::cacheModeNear(int id) {
    cacheResident("aniso_cache_mode_near", "resident near blocks", "resident near blocks", true, id, modeNearBlocks,
                  (size_t)plan.nearFTotal * sizeof(double), [&](double* F) {
                      launch_near_mode_blocks(id, nearList(), dNearFOff.as<int64_t>(), dAttNear.as<double>(),
                                              treePoints(), F, own);
                  });
}

void Operator::cacheModeNearFree(int id) {
    if (id < -1 || id >= kernelSize)
        throw std::out_of_range("aniso_cache_mode_near_free: kernel id " + std::to_string(id) + " out of range [-1, " +
                                std::to_string(kernelSize) + ")");
    modeNearBlocks.free(id);
}

int64_t Operator::cacheModeNearBytes() const { return modeNearBlocks.bytes(); }

void Operator::refuseHighOrder(const char* what) const {
    if (highOrder())
        throw std::logic_error(std::string(what) + ": a high-order handle (np = " + std::to_string(np) +
                               ") runs on the mode-shared caches only (aniso_mapping, the block operator, its passes and "
                               "solve, the direct forms); use an np = 4 handle");
}

void Operator::needResident(int id, const char* what) const {
    refuseHighOrder(what);
    if (id < 0 || id >= kernelSize || !modes[id].tables || modes[id].resident) return;
    throw std::logic_error(std::string(what) + " needs the operators of kernel id " + std::to_string(id) +
                           " resident: aniso_cache_block builds none, call aniso_cache(" + std::to_string(id) +
                           ") before it");
}

// The mode-shared caches: E = e^-tau for every directed M2L pair
// (column-major 16 x 16) and near block (the directed near layout), and sigma_t at
// every point (the mode-0 diagonal).  Built once per setCoeff on a block handle.
void Operator::buildAttCache() {
    dropCacheF32();
    modeBlocks.blocks.clear();
    modeNearBlocks.blocks.clear();
    const Params* P = dParams.as<Params>();
    const int64_t npairs = (int64_t)(plan.attOwner.size() + plan.hmCopyOwner.size());  // stored blocks + copies
    const size_t rank = (size_t)np * np;
    dAttM2L.alloc((size_t)npairs * rank * rank * sizeof(double));
    // the near blocks in the layout the harmonic near field reads: directed
    const std::vector<int64_t>& nptr = plan.nearPtr;
    dAttNear.alloc((size_t)plan.nearKTotal * sizeof(double));
    dSigDiag.alloc((size_t)geo.N * sizeof(double));
    int maxSrc = 1;
    for (size_t li = 0; li < plan.leaves.size(); ++li) maxSrc = std::max<int>(maxSrc, (int)(nptr[li + 1] - nptr[li]));
    if (highOrder())
        launch_ho_cache_att(np, npairs, dAttOwner.as<int>(), dAttOther.as<int>(), nodeBoxes(), dStCoef.as<double>(), P,
                            dHoTab.as<HoTables>(), dAttM2L.as<double>(), own);
    else
        launch_cache_att_m2l(npairs, dAttOwner.as<int>(), dAttOther.as<int>(), nodeBoxes(), dStCoef.as<double>(), P,
                             dAttM2L.as<double>(), own);
    launch_cache_near((int)plan.leaves.size(), dLeaves.as<int>(), dNearPtr.as<int64_t>(), dNearSrc.as<int>(),
                      dNearKOff.as<int64_t>(), dBegin.as<int64_t>(), dCount.as<int64_t>(), treePoints(),
                      dStCoef.as<double>(), P, kAttMode, maxSrc, dAttNear.as<double>(), own);
    launch_sigma_diag(geo.N, dPxT.as<double>(), dPyT.as<double>(), dStCoef.as<double>(), P, dSigDiag.as<double>(),
                      own);
    if (!highOrder()) {  // the deterministic sums' bound: rank 16 only
        if (!dAttMax.bytes) dAttMax.alloc(sizeof(double));
        launch_abs_max(npairs * 256, dAttM2L.as<double>(), dAttMax.as<double>(), own);
    }
    HIP_CHECK(hipStreamSynchronize(own));
    attReady = true;
}

// The deterministic sums' geometric bound per cluster (harmonic.hip hc_det_scale):
// 2 x 16 columns x the most pair products one of its LDS slots receives x the largest
// 1 / gap over its pairs (gap: the boxes' separation along the wider axis, a lower
// bound on the distance of any two of their Chebyshev nodes).
void Operator::detBounds() {
    const int ncl = (int)plan.hmClPtr.size() - 1;
    if (ncl <= 0 || dHmClBound.bytes >= (size_t)ncl * sizeof(double)) return;
    std::vector<double> bound(ncl);
    std::vector<int> cnt;
    for (int c = 0; c < ncl; ++c) {
        const int c0 = plan.hmClPtr[c], nt = plan.hmClPtr[c + 1] - c0;
        const int nh = plan.hmHaloPtr.empty() ? 0 : plan.hmHaloPtr[c + 1] - plan.hmHaloPtr[c];
        cnt.assign(nt + nh, 0);
        double ig = 0.0;
        for (int ti = 0; ti < nt; ++ti) {
            const int t = plan.hmTgt[c0 + ti];
            const int64_t p0 = plan.hmPtr[c0 + ti], pd = p0 + plan.hmNDir[c0 + ti], p1 = plan.hmPtr[c0 + ti + 1];
            for (int64_t e = p0; e < p1; ++e) {
                const int n = plan.hmSrc[e];
                const double gx = std::fabs(tree.ncx[t] - tree.ncx[n]) - tree.nrx[t] - tree.nrx[n];
                const double gy = std::fabs(tree.ncy[t] - tree.ncy[n]) - tree.nry[t] - tree.nry[n];
                const double gap = std::max(gx, gy);
                if (!(gap > 0.0)) throw std::logic_error("deterministic M2L: a V-list pair of touching boxes");
                ig = std::max(ig, 1.0 / gap);
                ++cnt[ti];
                if (e >= pd) ++cnt.at(plan.hmSlot[e]);
            }
        }
        const int most = cnt.empty() ? 0 : *std::max_element(cnt.begin(), cnt.end());
        bound[c] = 2.0 * 16.0 * most * ig;
    }
    up(dHmClBound, bound);
}

// Do the terms of a batched apply have aniso.m's harmonic structure (harmonic.hip)?
// Terms must be modes 0, 1, ..., nterm-1 with mix[m][i][b] = sum over j with |j| = b,
// |i + j| = m of w_b; w comes from output row 0 (mix[b][0][b] = hw_b).  Rows that are
// all zero (padded right-hand sides) are masked out.
bool Operator::harmonicWeights(int K, int nterm, const int* ids, const double* mixes, HarmWeights& hw) const {
    if (!useAtt || !attReady || plan.nearPartTotal > 0 || K < 2 || K > kMaxRhs || nterm > 2 * K - 1) return false;
    if (!(K == 2 || K == 4 || K == 5 || K == 8)) return false;
    for (int t = 0; t < nterm; ++t)
        if (ids[t] != t) return false;
    std::memset(&hw, 0, sizeof(hw));
    auto mx = [&](int m, int i, int b) { return m < nterm ? mixes[((size_t)m * K + i) * K + b] : 0.0; };
    double mag = 0.0;
    for (int t = 0; t < nterm * K * K; ++t) mag = std::max(mag, std::fabs(mixes[t]));
    for (int i = 0; i < K; ++i) {
        bool any = false;
        for (int m = 0; m < nterm; ++m)
            for (int b = 0; b < K; ++b) any = any || mx(m, i, b) != 0.0;
        hw.om[i] = any ? 1.0 : 0.0;
    }
    if (hw.om[0] == 0.0) return false;
    for (int b = 0; b < K; ++b) hw.hw[b] = mx(b, 0, b);
    std::vector<double> want((size_t)(2 * K - 1) * K * K, 0.0);
    for (int i = 0; i < K; ++i)
        for (int j = -(K - 1); j <= K - 1; ++j) {
            const int b = std::abs(j), m = std::abs(i + j);
            want[((size_t)m * K + i) * K + b] += b == 0 ? hw.hw[0] : 0.5 * hw.hw[b];
        }
    for (int i = 0; i < K; ++i) {
        if (hw.om[i] == 0.0) continue;
        hw.dw[i] = want[((size_t)0 * K + i) * K + i];
        for (int m = 0; m < 2 * K - 1; ++m)
            for (int b = 0; b < K; ++b)
                if (std::fabs(want[((size_t)m * K + i) * K + b] - mx(m, i, b)) > 1e-13 * mag) return false;
    }
    return true;
}

void Operator::mappingHost(const double* charge, int id, double* out) {
    refuseHoShard("aniso_mapping");
    if (id < 0 || id >= kernelSize) throw std::out_of_range("kernel id out of range");
    if (!modes[id].tables) throw std::runtime_error("mapping on kernel id " + std::to_string(id) + " before cache(" + std::to_string(id) + ")");
    ensureDevice();
    HIP_CHECK(hipMemcpyAsync(dCharge.p, charge, geo.N * sizeof(double), hipMemcpyHostToDevice, own));
    if (plan.nranks > 1) HIP_CHECK(hipMemsetAsync(dOut.p, 0, dOut.bytes, own));
    mappingDev(dCharge.as<double>(), id, dOut.as<double>(), own, kStageAll);
    HIP_CHECK(hipMemcpyAsync(out, dOut.p, geo.N * sizeof(double), hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    checkDeviceErrors();
}

// k right-hand sides of one mode: up to 8 per batched apply (identity mix), or, for
// more than 8 on an unsharded handle, 16 per apply of the fp64 MFMA operator
// (f64op.hip; zero columns pad the last chunk).  That operator keeps its own fp64
// copy of the mode's operators on the directed lists (mrhs64Bytes: about 6 GB per
// mode at 1M points, 24 GB at 4M), freed by setCoeff / cache(id): it is used only
// when that copy fits in the free HBM, else the 8-column batches run.
void Operator::mappingBatchedHost(const double* Q, int k, int id, double* Out) {
    refuseHighOrder("aniso_mapping_batched");
    if (k == 0) return;
    needResident(id, "aniso_mapping_batched");
    ensureDevice();
    const int64_t N = geo.N;
    bool mfma = k > 8 && plan.nranks == 1;
    if (mfma && !m64.count(id) && id >= 0 && id < kernelSize && modes[id].resident) {
        // the plan first (mrhs64Bytes builds and uploads it), then the free HBM it leaves
        const size_t need = mrhs64Bytes() + (size_t)64 * N * sizeof(double);  // + the four 16-column staging buffers
        size_t freeB = 0, totalB = 0;
        HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
        mfma = need + (size_t)(1ull << 30) <= freeB;  // keep a GiB of headroom
    }
    if (mfma) {
        if (id < 0 || id >= kernelSize) throw std::out_of_range("kernel id out of range");
        if (!modes[id].resident)
            throw std::runtime_error("mapping on kernel id " + std::to_string(id) + " before cache(" + std::to_string(id) + ")");
        DevBuf dq, dout, x16, y16;
        dq.alloc((size_t)16 * N * sizeof(double));
        dout.alloc((size_t)16 * N * sizeof(double));
        x16.alloc((size_t)16 * N * sizeof(double));
        y16.alloc((size_t)16 * N * sizeof(double));
        for (int j0 = 0; j0 < k; j0 += 16) {
            const int kc = std::min(16, k - j0);
            HIP_CHECK(hipMemcpyAsync(dq.p, Q + (size_t)j0 * N, (size_t)kc * N * sizeof(double), hipMemcpyHostToDevice,
                                     own));
            launch64_gather16(N, kc, dPerm.as<int>(), dq.as<double>(), x16.as<double>(), own);
            mrhs64Dev(id, false, x16.as<double>(), y16.as<double>(), own);
            launch64_scatter16(N, kc, dPerm.as<int>(), y16.as<double>(), dout.as<double>(), own);
            HIP_CHECK(hipMemcpyAsync(Out + (size_t)j0 * N, dout.p, (size_t)kc * N * sizeof(double),
                                     hipMemcpyDeviceToHost, own));
            HIP_CHECK(hipStreamSynchronize(own));
        }
        checkDeviceErrors();
        return;
    }
    const int kb = std::min(k, 8);
    DevBuf dq, dout;
    dq.alloc((size_t)kb * N * sizeof(double));
    dout.alloc((size_t)kb * N * sizeof(double));
    for (int j0 = 0; j0 < k; j0 += kb) {
        const int nb = std::min(kb, k - j0);
        HIP_CHECK(hipMemcpyAsync(dq.p, Q + (size_t)j0 * N, (size_t)nb * N * sizeof(double), hipMemcpyHostToDevice, own));
        if (plan.nranks > 1) HIP_CHECK(hipMemsetAsync(dout.p, 0, dout.bytes, own));
        ApplyCall call;
        applyBlock(nb, dq.as<double>(), N, false, nullptr, 1, &id, identityMix(nb).data(), dout.as<double>(), N, false,
                   own, kStageAll, call);
        HIP_CHECK(hipMemcpyAsync(Out + (size_t)j0 * N, dout.p, (size_t)nb * N * sizeof(double), hipMemcpyDeviceToHost,
                                 own));
        HIP_CHECK(hipStreamSynchronize(own));
        checkDeviceErrors();
    }
}

// mapping (AnisoWrapper.cpp:92-136) on device pointers, enqueued on stream s.
// Only owned targets of `out` are written when the operator is sharded.
void Operator::mappingDev(const double* charge, int id, double* out, hipStream_t s, int mask) {
    refuseHoShard("aniso_mapping_dev");
    if (id >= 0 && id < kernelSize && modes[id].tables && !modes[id].resident) {
        leanMapping(charge, id, out, s, mask);
        return;
    }
    apply(charge, false, nullptr, id, out, false, s, mask);
}

// mapping(id) of a mode made ready by cacheBlock only: served from
// the mode-shared caches as one pass of the offset form (§3.9.1).  The charge is row 0
// of a zero-padded 8-row input with the harmonic weights hw = [1, 0, ..., 0], the
// window is i0 = 8 (id / 8), b0 = 0, and om masks every output row but id - i0:
//     out = (E / r) T_id(c) charge
// over the M2L and the near field, with mode id's correction stencils and, for id = 0,
// the sigma_t diagonal (dw).  The launches are the pass's; the stage mask is not
// supported on this route.
void Operator::leanMapping(const double* charge, int id, double* out, hipStream_t s, int mask, const double* sigT) {
    constexpr int K = kMaxRhs;
    if (mask != kStageAll) refuseHighOrder("a per-stage apply");
    if (mask != kStageAll)
        throw std::logic_error("mapping stages on kernel id " + std::to_string(id) +
                               ": its operators are not resident (aniso_cache_block builds none); call aniso_cache(" +
                               std::to_string(id) + ") before a per-stage apply");
    if (!(useAtt && attReady && plan.nearPartTotal == 0)) needResident(id, "aniso_mapping");
    ensureDevice();
    const int64_t N = geo.N;
    const int i0 = K * (id / K), row = id - i0;
    dPassIn.alloc((size_t)K * N * sizeof(double));
    dPassOut.alloc((size_t)K * N * sizeof(double));
    HIP_CHECK(hipMemsetAsync(dPassIn.p, 0, dPassIn.bytes, s));
    HIP_CHECK(hipMemcpyAsync(dPassIn.p, charge, N * sizeof(double), hipMemcpyDeviceToDevice, s));
    double* const orow = dPassOut.as<double>() + (size_t)row * N;
    // a shard writes its owned targets only: the others keep the caller's values
    if (plan.nranks > 1) HIP_CHECK(hipMemcpyAsync(orow, out, N * sizeof(double), hipMemcpyDeviceToDevice, s));
    ApplyCall call;
    call.pass = true;
    call.win = HarmWindow{i0, 0};
    call.hw.hw[0] = 1.0;
    call.hw.om[row] = 1.0;
    call.hw.dw[row] = id == 0 ? 1.0 : 0.0;
    std::vector<double> sub((size_t)K * K, 0.0);  // the correction fold: mode id, input row 0 to output row `row`
    sub[(size_t)row * K] = 1.0;
    applyBlock(K, dPassIn.as<double>(), N, false, sigT, 1, &id, sub.data(), dPassOut.as<double>(), N, false, s,
               kStageAll, call);
    HIP_CHECK(hipMemcpyAsync(out, orow, N * sizeof(double), hipMemcpyDeviceToDevice, s));
}

// mapping on a tree-order input (all N) into the owned tree-order slice
// out[k - ownBegin], k in [ownBegin, ownEnd): no permutation gathers, and the
// slices of the shards concatenate to the tree-order output.
void Operator::mappingTreeDev(const double* qTree, int id, double* outSlice, hipStream_t s) {
    needResident(id, "aniso_mapping_tree_dev");
    apply(qTree, true, nullptr, id, outSlice, true, s, kStageAll);
}

// main.cpp forwardOperator (main.cpp:125-136) in tree order: y = x - K_0(sigma_s x)
// on the owned slice, x tree-ordered (all N).
void Operator::forwardTreeDev(const double* xTree, double* ySlice, hipStream_t s) {
    forwardTreePhase(0, xTree, ySlice, nullptr, nullptr, s);
}

void Operator::forwardTreePhase(int phase, const double* xTree, double* ySlice, double* rootsSend,
                                const double* rootsRecv, hipStream_t s) {
    refuseHighOrder("the forward operator");
    needResident(0, "the forward operator");
    if (!modeCached(0)) throw std::runtime_error("forward operator before cache(0)");
    ensureDevice();
    pendingCall(phase, PendingCall{0, 0, xTree, ySlice, dSigmaT.p, geo.N, 0, 0.0});
    const double one = 1.0;
    const int id = 0;
    ApplyCall call;
    call.phased(phase, rootsSend, rootsRecv);
    applyBlock(1, xTree, geo.N, true, dSigmaT.as<double>(), 1, &id, &one, dTmpS.as<double>(), geo.N, true, s,
               kStageAll, call);
    if (phase == 1) return;
    const int64_t n = plan.ownEnd - plan.ownBegin;
    launch_sub_slice(n, 1, xTree + plan.ownBegin, n, dTmpS.as<double>(), n, ySlice, n, s);
}

void Operator::apply(const double* charge, bool treeIn, const double* sigT, int id, double* out, bool treeOut,
                     hipStream_t s, int mask) {
    const double one = 1.0;
    ApplyCall call;
    applyBlock(1, charge, geo.N, treeIn, sigT, 1, &id, &one, out, geo.N, treeOut, s, mask, call);
}

void Operator::applyBlockDev(int nrhs, const double* x, int64_t ldx, bool treeIn, bool useSigma, int nterm,
                             const int* ids, const double* mixes, double* out, int64_t ldo, bool treeOut,
                             hipStream_t s, int mask) {
    refuseHoShard("aniso_apply_block_dev");
    if (useSigma && !coeffSet) throw std::runtime_error("block apply with sigma_s before setCoeff");
    ensureDevice();
    ApplyCall call;
    applyBlock(nrhs, x, ldx, treeIn, useSigma ? dSigmaT.as<double>() : nullptr, nterm, ids, mixes, out, ldo, treeOut,
               s, mask, call);
}

int Operator::mark(hipStream_t s) {
    if (evUsed == (int)evPool.size()) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        evPool.push_back(e);
    }
    HIP_CHECK(hipEventRecord(evPool[evUsed], s));
    return evUsed++;
}

// Device table of the mode terms of a batched apply (operator pointers, sign and
// K x K mix per term).  Tables are cached by content: a block operator reuses one
// table every call, so no upload sits on the apply's path.
const ModeArgs* Operator::modeTable(int K, int nterm, const int* ids, const double* mixes) {
    std::vector<ModeArgs> tab(nterm);
    std::memset(tab.data(), 0, tab.size() * sizeof(ModeArgs));
    for (int t = 0; t < nterm; ++t) {
        const ModeCache& mc = modes[ids[t]];
        ModeArgs& m = tab[t];
        m.Km2l = mc.Km2l.as<double>();
        m.Knear = mc.Knear.as<double>();
        m.C = mc.C.as<double>();
        m.mu = mc.mu.as<double>();
        m.sgn = (ids[t] % 2 == 0) ? 1.0 : -1.0;  // K_{B<-A} = (-1)^m K_{A<-B}^T
        for (int i = 0; i < K; ++i)
            for (int b = 0; b < K; ++b) m.mix[i][b] = mixes[((size_t)t * K + i) * K + b];
    }
    std::string key(reinterpret_cast<const char*>(tab.data()), tab.size() * sizeof(ModeArgs));
    auto it = modeTabs.find(key);
    if (it != modeTabs.end()) return it->second.as<ModeArgs>();
    if (modeTabs.size() >= 64) {  // bound the cache; hipFree waits for work that may still read a table
        HIP_CHECK(hipDeviceSynchronize());
        modeTabs.clear();
    }
    DevBuf& buf = modeTabs[key];
    buf.upload(tab.data(), tab.size() * sizeof(ModeArgs));
    return buf.as<ModeArgs>();
}

// The correction tables of a batched apply, folded over its terms on the host:
// Wc[tq][q9][c][i][b] = sum_t mix_t[i][b] C_t[tq][q9][c] and
// Wm[tq][i][b][a][bb] = sum_t mix_t[i][b] mu_t[tq][a][bb] (k_corr).  Cached by
// content, like the mode table.
const CorrFold& Operator::corrTable(int K, int nterm, const int* ids, const double* mixes) {
    std::string key(reinterpret_cast<const char*>(&K), sizeof(int));
    key.append(reinterpret_cast<const char*>(ids), nterm * sizeof(int));
    key.append(reinterpret_cast<const char*>(mixes), (size_t)nterm * K * K * sizeof(double));
    auto it = corrTabs.find(key);
    if (it != corrTabs.end()) return it->second;
    const int d = geo.d, d2 = geo.d2;
    std::vector<double> wc((size_t)d2 * 9 * d2 * K * K, 0.0), wm((size_t)d2 * K * K * d2, 0.0);
    for (int t = 0; t < nterm; ++t) {
        const ModeCache& mc = modes[ids[t]];
        for (int i = 0; i < K; ++i)
            for (int b = 0; b < K; ++b) {
                const double w = mixes[((size_t)t * K + i) * K + b];
                if (w == 0.0) continue;
                for (int tq = 0; tq < d2; ++tq) {
                    for (int q = 0; q < 9 * d2; ++q)  // (q9, c)
                        wc[(((size_t)tq * 9 * d2 + q) * K + i) * K + b] += w * mc.hostC[(size_t)tq * 9 * d2 + q];
                    for (int ab = 0; ab < d * d; ++ab)
                        wm[(((size_t)tq * K + i) * K + b) * d2 + ab] += w * mc.hostMu[(size_t)tq * d * d + ab];
                }
            }
    }
    if (corrTabs.size() >= 64) {  // bound the cache; hipFree waits for work that may still read a table
        HIP_CHECK(hipDeviceSynchronize());
        corrTabs.clear();
    }
    CorrFold& f = corrTabs[key];
    up(f.Wc, wc);
    up(f.Wm, wm);
    return f;
}

// nterm K x K mixes in the top-left corners of Kp x Kp ones (zero right-hand sides pad the rest)
static std::vector<double> padMixes(int K, int Kp, int nterm, const double* mixes) {
    std::vector<double> mp((size_t)nterm * Kp * Kp, 0.0);
    for (int t = 0; t < nterm; ++t)
        for (int i = 0; i < K; ++i)
            for (int b = 0; b < K; ++b) mp[((size_t)t * Kp + i) * Kp + b] = mixes[((size_t)t * K + i) * K + b];
    return mp;
}

// the mode ids 0 .. nm - 1 of a block operator's terms
static std::vector<int> modeIds(int nm) {
    std::vector<int> ids(nm);
    for (int m = 0; m < nm; ++m) ids[m] = m;
    return ids;
}

constexpr double kScale = M_1_PI / 2.0;  // AnisoWrapper.cpp:129-130

// ---- the stages of the un-fused applies ----
// One stream, every sum in a fixed order: the weighted charges; the near field, which stores
// the output rows; the corrections, which add to them; the up pass; one M2L launch; the down
// pass, the last writer of the rows (it carries the minuend).

void Operator::prepareCharges(int K, const InRows& in, double* fT, double* cT, hipStream_t s) {
    launch_prepare(K, geo.N, in.x, in.ld, in.tree ? 1 : 0, dPerm.as<int>(), in.sigT, dWT.as<double>(), fT, cT, s);
}

void Operator::nearUnstaged(int K, const HarmWeights& hw, const HarmWindow* win, int mask, const OutRows& o,
                            hipStream_t s) {
    launch_near_hm(K, nearList(), dAttNear.as<double>(), treePoints(), dSigDiag.as<double>(), hw, dFT.as<double>(), mask,
                   kScale, o, nullptr, nullptr, nullptr, 0, nullptr, s, nullptr, win);
}

void Operator::nearUnstagedF32(int K, const HarmWeights& hw, const OutRows& o, hipStream_t s) {
    launch_near_hm_f32(K, nearList(), dAttNearF.as<float>(), nodeBoxes(), treePoints(), dSigDiag.as<double>(), hw,
                       dFT.as<double>(), kScale, o, s);
}

void Operator::nearMode(int K, int id, const OutRows& o, hipStream_t s, ApplyPrec prec) {
    if (prec == ApplyPrec::F32) {
        launch_near_mode_f32(K, id, nearList(), dAttNearF.as<float>(), nodeBoxes(), treePoints(), dSigDiag.as<double>(),
                             dFT.as<double>(), kScale, o, s);
        nearCalls.emplace_back(K, 0);  // (the f32 entries ignore the resident near blocks)
        return;
    }
    // the stored near blocks serve the full chunk only: at 2, 4 and 5 columns k_near_mode's span
    // on mode 0 is as short or shorter at both orders (measured)
    if (const double* F = K == kMaxRhs ? modeNearBlocks.find(id) : nullptr) {
        launch_near_resident(id, nearList(true), F, dSigDiag.as<double>(), dFT.as<double>(), K, nullptr, 0, kScale, o,
                             OutRows{}, s);
        nearCalls.emplace_back(K, 1);
        return;
    }
    launch_near_mode(K, id, nearList(), dAttNear.as<double>(), treePoints(), dSigDiag.as<double>(), dFT.as<double>(),
                     kScale, o, s);
    nearCalls.emplace_back(K, 0);
}

void Operator::nearMode16(int id, const ModeHalf& a, const ModeHalf& b, hipStream_t s) {
    const double* F = modeNearBlocks.find(id);
    if (!F || a.o.perm != b.o.perm || a.o.base != b.o.base)
        throw std::logic_error("a 16-column near launch without resident near blocks or with two output orders");
    launch_near_resident(id, nearList(true), F, dSigDiag.as<double>(), dFT.as<double>(), a.K, dFT2.as<double>(), b.K,
                         kScale, a.o, b.o, s);
    nearCalls.emplace_back(2 * kMaxRhs, 1);
}

void Operator::reserveCharges2(int K) {
    if (K <= workK2) return;
    workK2 = K;
    dFT2.alloc((size_t)geo.N * rhs_stride(K) * sizeof(double));
    dCT2.alloc((size_t)geo.N * rhs_stride(K) * sizeof(double));
}

void Operator::corrections(int K, const CorrFold& cf, const double* fT, const double* cT, int64_t begin, int64_t end,
                           int mask, const OutRows& o, hipStream_t s) {
    launch_corr(K, geo.d, begin, end, dPerm.as<int>(), dIperm.as<int>(), cT, fT, cf.Wc.as<double>(), cf.Wm.as<double>(),
                dParams.as<Params>(), mask, kScale, o.tree, o.ld, o.out, s);
}

void Operator::hoReserve(int K, hipStream_t s, bool second) {
    DevBuf& mult = second ? dHoMult2 : dHoMult;
    DevBuf& local = second ? dHoLocal2 : dHoLocal;
    int& have = second ? hoWorkK2 : hoWorkK;
    if (K > have) {
        mult.alloc(hoDoubles(K) * sizeof(double));
        local.alloc(hoDoubles(K) * sizeof(double));
        have = K;
    }
    // nodes that are no M2L target (the root, empty nodes) keep zero locals; a smaller K
    // re-uses the buffers with its own strides
    HIP_CHECK(hipMemsetAsync(local.p, 0, hoDoubles(K) * sizeof(double), s));
}

void Operator::hoUpPass(int K, const double* fT, double* mult, bool allLeaves, hipStream_t s) {
    const int nl = allLeaves ? hoLeafAll : (int)plan.leaves.size();
    launch_ho_p2m(np, K, nl, (allLeaves ? dHoLeafAll : dLeafInfo).as<int4>(), nodeBoxes(), treePoints(), fT,
                  dHoTab.as<HoTables>(), mult, s);
    for (size_t l = 0; l + 1 < hoM2mPtr.size(); ++l)
        launch_ho_m2m(np, K, hoM2mPtr[l + 1] - hoM2mPtr[l], dHoM2m.as<int>() + hoM2mPtr[l], dHoChild.as<int4>(),
                      dHoTab.as<HoTables>(), mult, s);
}

void Operator::hoDownPass(int K, double* local, const OutRows& o, hipStream_t s) {
    const HoTables* T = dHoTab.as<HoTables>();
    for (size_t l = 0; l + 1 < hoL2lPtr.size(); ++l)
        launch_ho_l2l(np, K, hoL2lPtr[l + 1] - hoL2lPtr[l], dHoL2l.as<int>() + hoL2lPtr[l], dParent.as<int>(),
                      dSlot.as<int>(), T, local, s);
    launch_ho_l2p(np, K, (int)plan.leaves.size(), dLeafInfo.as<int4>(), nodeBoxes(), treePoints(), T, local, kScale, o, s);
}

// tier k: `list` (nullptr: every task of the tier) names ntask tasks; fT / cT (nullptr: none)
// receive the charges its P2M forms; recv / send: the tier-0 roots of a sharded apply
void Operator::upTier16(int K, int k, const int* list, int ntask, double* fT, double* cT, const double* recv,
                        double* send, unsigned* zeroCnt, const InRows& in, hipStream_t s) {
    launch_up_tier(K, ntask, plan.upTierTask[k], list, plan.upTierMaxTask[k], dUpDesc.as<int4>(), dUpGrpFix.as<int>(),
                   dUpNode.as<int>(), dUpCode.as<int4>(), dUpGeom.as<double4>(), dUpLeaf.as<int2>(), dPxT.as<double>(),
                   dPyT.as<double>(), in.x, in.ld, in.tree ? 1 : 0, dPerm.as<int>(), in.sigT, dWT.as<double>(), fT, cT,
                   dParams.as<Params>(), dMult.as<double>(), recv ? dXRootSlot.as<int>() : nullptr, recv,
                   send ? dXSendSlot.as<int>() : nullptr, send, s, zeroCnt);
}

// L2L + L2P + the gathered partials (nearPart: transposed near products; hpart: the clustered
// M2L's halo), once for the sum over the terms
void Operator::downPass16(int K, int mask, const double* nearPart, const double* hpart, const OutRows& o,
                          hipStream_t s) {
    launch_down_tier(K, (int)plan.dnDesc.size() / 3, plan.dnMaxTask, plan.dnMaxLeaves, dDnDesc.as<int4>(),
                     dDnGrpFix.as<int>(), dDnNode.as<int4>(), dLocal.as<double>(), dParams.as<Params>(),
                     dDnLeafSlot.as<int>(), dDnLeafPts.as<int>(), dDnLeafNear.as<int2>(), dDnLeafGeom.as<double4>(),
                     dPxT.as<double>(), dPyT.as<double>(), o.perm, o.base, o.ld, dDnNearOff.as<int>(), plan.dnMaxNear,
                     nearPart, dDnChain.as<int2>(), plan.dnMaxChain, mask, kScale, o.out, o.minuend, o.minuendLd, s,
                     hpart, dDnChainFold.as<int>());
}

void Operator::padRowsIn(DevBuf& buf, int groups, int nb, int K, const double* x, int64_t ldx, hipStream_t s) {
    const int64_t N = geo.N;
    HIP_CHECK(hipMemsetAsync(buf.p, 0, (size_t)groups * K * N * sizeof(double), s));
    for (int j = 0; j < groups; ++j)
        HIP_CHECK(hipMemcpy2DAsync(buf.as<double>() + (size_t)j * K * N, N * sizeof(double), x + (size_t)j * nb * ldx,
                                   ldx * sizeof(double), N * sizeof(double), nb, hipMemcpyDeviceToDevice, s));
}

void Operator::padRowsOut(const double* group, int nb, int64_t n, double* out, int64_t ldo, hipStream_t s) {
    HIP_CHECK(hipMemcpy2DAsync(out, ldo * sizeof(double), group, geo.N * sizeof(double), n * sizeof(double), nb,
                               hipMemcpyDeviceToDevice, s));
}

// One batched apply: the up pass over the K base vectors, then per term t (mode
// ids[t], mix mixes[t]) the near field, the corrections, the M2L stream and its
// gather, each accumulating; then one down pass.  sigT (sigma_s in tree order, or
// nullptr) multiplies the inputs at their tree positions.
//
// phase 1 / 2 split a sharded apply around the caller's all-gather of the tier-0
// root multipoles: phase 1 runs this rank's tier-0 up tasks only
// (plan.xT0Tasks), packs its roots into rootsSend and starts the near field and
// corrections (they need only the weighted charges of the rank's own and halo
// points); phase 2 scatters rootsRecv, runs the upper tiers (every rank), the M2L
// and the down pass.  `call` says which of these, and what else, this call is (ApplyCall).
void Operator::applyBlock(int K, const double* x, int64_t ldx, bool treeIn, const double* sigT, int nterm,
                          const int* ids, const double* mixes, double* out, int64_t ldo, bool treeOut, hipStream_t s,
                          int mask, const ApplyCall& call) {
    const int phase = call.phase;
    double* const rootsSend = call.rootsSend;
    const double* const rootsRecv = call.rootsRecv;
    if (!(call.hoShard && treeIn && treeOut)) refuseHoShard("a block apply");  // before anything is staged
    if (K < 1 || K > 8) throw std::invalid_argument("block apply supports 1..8 right-hand sides, got " + std::to_string(K));
    checkDeviceErrors();
    if (nterm < 1) throw std::invalid_argument("block apply needs at least one mode term");
    checkModes(K, nterm, ids, mixes, call);
    if (phase != 0 && !treeIn) throw std::invalid_argument("a sharded (two-phase) apply takes tree-order input");
    if (phase == 1 && plan.xRootChunk > 0 && !rootsSend) throw std::invalid_argument("sharded apply: null roots_send");
    if (phase == 2 && plan.xRootChunk > 0 && !rootsRecv) throw std::invalid_argument("sharded apply: null roots_recv");
    if (phase >= 2 && !(pend.active && pend.K == rootRhs(K)))
        throw std::logic_error("sharded apply: end without a matching begin");
    if (phase == 3 && !(call.shardedPass && call.pass)) throw std::logic_error("sharded apply: a repeated phase 2 outside a pass");
    ensureDevice();
    const int64_t nOut = treeOut ? plan.ownEnd - plan.ownBegin : geo.N;
    if (ldx < geo.N || ldo < nOut) throw std::invalid_argument("block apply: leading dimension too small");
    // (a high-order handle's harmonic launches start at 2 blocks: ks = 1 runs as 2 with a zero one)
    const bool padHigh = highOrder() && K == 1 && !call.pass;
    if (!rhs_supported(K) || padHigh) {  // pad with zero right-hand sides to the next compiled count
        const int Kp = padHigh ? 2 : rhs_padded(K);
        dPadIn.alloc((size_t)Kp * geo.N * sizeof(double));
        dPadOut.alloc((size_t)Kp * geo.N * sizeof(double));
        if (phase != 2) padRowsIn(dPadIn, 1, K, Kp, x, ldx, s);  // phase 2 reads what phase 1 staged
        const std::vector<double> mp = padMixes(K, Kp, nterm, mixes);
        applyBlock(Kp, dPadIn.as<double>(), geo.N, treeIn, sigT, nterm, ids, mp.data(), dPadOut.as<double>(), geo.N,
                   treeOut, s, mask, call);
        if (phase != 1) padRowsOut(dPadOut.as<double>(), K, nOut, out, ldo, s);
        return;
    }
    ensureWork(K);
    const InRows in{x, ldx, treeIn, sigT};
    const OutRows o = outRows(out, ldo, treeOut, call.minuend, call.minuendLd);
    if (highOrder()) {
        applyBlockHigh(K, in, nterm, ids, mixes, o, s, mask, call);
        return;
    }
    if (up_tier_lds(plan.upMaxTask, K) > 160 * 1024 ||
        down_tier_lds(plan.dnMaxTask, plan.dnMaxLeaves, plan.dnMaxNear, plan.dnMaxChain, K) > 160 * 1024)
        throw std::logic_error("up/down pass task exceeds one workgroup's LDS at " + std::to_string(K) + " right-hand sides");
    const Params* P = dParams.as<Params>();
    const bool tr = timeStages != 0;  // the roofline spans: M2L (stage 2), near field (4)
    const bool tm = timeStages == 1;  // every stage
    auto span = [&](int stage, int a, int b) {
        if (a >= 0 && b >= 0) spans.push_back({stage, a, b});
    };
    HarmWeights hw;
    // one pass of a block operator of more than kMaxRhs blocks (blockPass): its weights
    // come with it, and it runs the plain harmonic launches in their offset form; without
    // the mode-shared caches the pass's sub-mixes take the per-mode stream like any mix
    const HarmWindow* const win = call.pass && useAtt && attReady && plan.nearPartTotal == 0 ? &call.win : nullptr;
    if (win) hw = call.hw;
    if (call.shardedPass && !(win && phase != 0)) throw std::logic_error("sharded pass: not the offset harmonic form");
    const bool harmonic = win ? true : harmonicWeights(K, nterm, ids, mixes, hw);
    // the harmonic block apply runs its near field + corrections (they write `out`)
    // on a side stream beside the M2L (it writes the locals), forked as soon as the
    // weighted charges are complete: after the last up tier with a P2M leaf
    const ModeArgs* tab = win ? nullptr : modeTable(K, nterm, ids, mixes);  // (the harmonic launches read no mode table)
    const CorrFold& cf = corrTable(K, nterm, ids, mixes);
    const NearCorr nc{dNearCorrRow.as<uint16_t>(), dPerm.as<int>(), dIperm.as<int>(), dCT.as<double>(),
                      cf.Wc.as<double>(), cf.Wm.as<double>(), P};
    const int ntier = (int)plan.upTierTask.size() - 1;  // 0: a lone leaf
    // a sharded one-collective matvec with the upper multipoles as partial sums
    // (blockOpShardedDev, Plan::xUpPartial): phase 1 forms this rank's records, the
    // exchange's unpack sums them, phase 2 runs no up tier
    const bool upPartial = call.exch.oneX && call.exch.upPartial && phase != 0;
    // the upper tiers ride in the M2L launch (k_top_m2l_hc) when every leaf is in the
    // bottom tier: the near field then forks after it
    const bool topFused = harmonic && (mask & kStageFar) && topFusedOn() && !upPartial && !win;
    const bool fork = harmonic && overlapOn();
    const hipStream_t sn = fork ? side : s;
    // the staged near field with its fused corrections forms its charges from the
    // input itself (NearHsArgs::xin), so it needs nothing from the up pass: it forks
    // at the start of the apply, beside the latency-bound up tiers, and the up pass
    // stores no fT / cT (ANISO_NEAR_EARLY=0: it forks after the up pass and reads them)
    const bool nearIn = harmonic && nearEarly && plan.nearCorrOk && (mask & kStageNear) &&
                        near_hs_fusable((int)plan.leaves.size(), plan.nearMaxLeaf, plan.nsMax,
                                        dNearLoc.as<uint16_t>(), &nc, mask);
    // the one-collective exchange (blockOpShardedDev): phase 1 runs the own tier-0
    // tasks only and leaves the near field to phase 2, after the exchange
    const bool oneX = call.exch.oneX && phase != 0;
    if (oneX && !(harmonic && nearIn))
        throw std::logic_error("one-collective exchange: the apply is not the harmonic one with its near field from the input");
    double* const fTw = nearIn ? nullptr : dFT.as<double>();
    double* const cTw = nearIn ? nullptr : dCT.as<double>();
    // the near field forks after the whole up pass on one GPU: forked after the
    // bottom tier it starved the latency-bound upper tiers the M2L waits on (up pass
    // 0.25 -> 0.14 ms, 644 -> 660 block matvec/s); a sharded apply starts it in
    // phase 1, beside the root exchange (8 shards: 0.317 vs 0.327 ms per rank)
    const int forkTier = phase == 0 && !topFused ? std::max(ntier - 1, 0) : plan.upLastLeafTier;
    // one up tier; a sharded apply's bottom tier runs this rank's tasks only (list)
    // and stores its tier-0 roots into send, its next tier reads the gathered ones
    auto upTier = [&](int k, const int* list, int ntask, const double* recv, double* send) {
        unsigned* const zeroCnt = topFused && k == 0 ? dTopCnt.as<unsigned>() : nullptr;
        upTier16(K, k, list, ntask, fTw, cTw, recv, send, zeroCnt, in, s);
        if (fork && !nearIn && k == forkTier) HIP_CHECK(hipEventRecord(evFork, s));
    };
    auto tierTasks = [&](int k) { return plan.upTierTask[k + 1] - plan.upTierTask[k]; };
    NearHsArgs nin{};  // nearIn: the input the near field forms its charges from
    if (nearIn) {
        nin.xin = x;
        nin.ldi = ldx;
        nin.treeIn = treeIn ? 1 : 0;
        nin.perm = dPerm.as<int>();
        nin.sigT = sigT;
        nin.wT = dWT.as<double>();
    }
    // the bottom up tier inside the staged near field (one GPU, serial: the near field
    // runs first, so tier 1 -- in the fused launch or its own -- finds the tier-0 roots)
    // (K <= 5: the 4-wave near kernel with the tail spills at K = 8)
    const bool nearUp = phase == 0 && nearIn && !fork && nearUpTier() && ntier >= 1 && K <= 5;
    if (nearUp) {
        nin.upMult = dMult.as<double>();
        nin.upGrp = dNearUpGrp.as<int>();
        nin.upP = P;
        nin.upNcx = dNcx.as<double>();
        nin.upNcy = dNcy.as<double>();
        nin.upNrx = dNrx.as<double>();
        nin.upNry = dNry.as<double>();
        nin.zeroCnt = topFused ? dTopCnt.as<unsigned>() : nullptr;
    }
    // near field + corrections (they need only fT / cT, or with nearIn the input)
    auto nearStage = [&] {
        if (fork) HIP_CHECK(hipStreamWaitEvent(side, evFork, 0));
        StageSpans ns(*this, sn);
        bool corrFused = false;
        if (harmonic) {
            // the corrections ride in the staged near kernel (d = 1, its table holds
            // every stencil neighbour; Plan::nearCorrRow)
            corrFused = launch_near_hm(K, nearList(), dAttNear.as<double>(), treePoints(), dSigDiag.as<double>(), hw,
                                       dFT.as<double>(), mask, kScale, o, dNearLoc.as<uint16_t>(), dNsPtr.as<int64_t>(),
                                       dNsPts.as<int>(), plan.nsMax, plan.nearCorrOk ? &nc : nullptr, sn, &nin, win);
        } else if (plan.nearPartTotal > 0) {
            // symmetric U storage (K = 1 handles): one launch per term; the transposed
            // products go to partials summed over the terms
            for (int t = 0; t < nterm; ++t) {
                const int id = ids[t];
                // K_{B<-A} = (-1)^m K_{A<-B}^T for the merged kernel; Id = m
                const double sgn = (id % 2 == 0) ? 1.0 : -1.0;
                launch_near_sym(K, (int)plan.leaves.size(), dLeafInfo.as<int4>(), dNearPtsPtr.as<int64_t>(),
                                dNearPts.as<int>(), dNearKOff.as<int64_t>(), dNearSym.as<int2>(),
                                modes[id].Knear.as<double>(), dFT.as<double>(), mixes + (size_t)t * K * K, o.perm,
                                o.base, ldo, maxNearS, mask, sgn, kScale, t > 0 ? 1 : 0, dNearPart.as<double>(), out,
                                s);
            }
        } else {  // directed storage: all terms in one launch
            launch_near(K, (int)plan.leaves.size(), plan.nearMaxLeaf, dLeafInfo.as<int4>(), dNearPtsPtr.as<int64_t>(),
                        dNearPts.as<int>(), dNearKOff.as<int64_t>(), tab, nterm, dFT.as<double>(), o.perm, o.base, ldo,
                        mask, kScale, 0, out, s);
        }
        ns.end(4);
        if (!corrFused)
            corrections(K, cf, dFT.as<double>(), dCT.as<double>(), plan.ownBegin, plan.ownEnd, mask, o, sn);
        ns.end(6);
        if (fork) HIP_CHECK(hipEventRecord(evJoin, side));
    };
    const bool clustered = harmonic && useClusters && !win;  // a pass: the per-target launch (its offset form)
    const int ncl = (int)plan.hmClPtr.size() - 1;
    HcArgs hca{dHmClPtr.as<int>(), dHmTgt.as<int>(), dHmPtr.as<int64_t>(), dHmNDir.as<int>(), dHmSrc.as<int>(),
                     dHmBlk.as<int>(), dHmSlot.as<int>(), dAttM2L.as<double>(), dNcx.as<double>(), dNcy.as<double>(),
                     dNrx.as<double>(), dNry.as<double>(), P, hw, dMult.as<double>(), dLocal.as<double>()};
    const bool halo = !plan.hmHaloNode.empty();
    if (halo) {  // the halo form: partials of the cross-cluster partner products (Plan::hmHaloPtr)
        const size_t hb = plan.hmHaloNode.size() * kRank * K * sizeof(double);
        if (dHmPart.bytes < hb) dHmPart.alloc(hb);
        hca.haloPtr = dHmHaloPtr.as<int>();
        hca.haloPos = dHmHaloPos.as<int>();
        hca.hpart = dHmPart.as<double>();
    }
    auto m2lClusters = [&](int c0, int c1, hipStream_t st) {
        HcArgs a = hca;
        if (detSums) {  // fixed-point cluster sums: the bounds of this apply's multipoles first
            detBounds();
            const int nn = (int)tree.ncx.size();
            if (dNodeWmax.bytes < (size_t)nn * sizeof(double)) dNodeWmax.alloc((size_t)nn * sizeof(double));
            launch_node_wmax(K, nn, dMult.as<double>(), hw, dNodeWmax.as<double>(), st);
            a.wmax = dNodeWmax.as<double>();
            a.clBound = dHmClBound.as<double>() + c0;
            a.emax = dAttMax.as<double>();
        }
        a.clPtr += c0;
        if (a.haloPtr) a.haloPtr += c0;
        launch_m2l_hc(K, c1 - c0, plan.hmMaxLds, a, st);
    };
    int e0 = -1;
    int eStart = -1;  // the apply's first event: the total span covers every stage
    bool nearDone = false;
    // a sharded pass (blockOpShardedPasses): its phase 1 serves every output window of the
    // input chunk, so nothing that depends on the window -- the near field and the
    // corrections write `out` -- is issued there; every near group runs in phase 2
    const bool passShard = win && phase != 0;
    if (phase < 2) {
        // up pass: tiers bottom-up; its P2M also forms the weighted charges fT (tree
        // order) the near field and the corrections read
        e0 = tm ? mark(s) : -1;
        eStart = e0;
        if (nearIn && oneX && !plan.nearGrpEarly.empty() && !passShard) {
            // one-collective form: the groups that read only the own range start now,
            // beside the own tier-0 tasks; the rest waits for the exchange (phase 2)
            nin.grpList = dNearGrpEarly.as<int>();
            nin.ngrp = (int)plan.nearGrpEarly.size();
            if (fork) HIP_CHECK(hipEventRecord(evFork, s));
            nearStage();
            if (!fork && tm) e0 = mark(s);
        }
        // the fork point is the start of the apply, but the near field's launch is issued
        // after the bottom up tier's, so the dispatcher tends to hand the up tasks their
        // workgroup slots first (0.6-1.2 % per block matvec on one GPU, 1.6 % on a rank
        // of 8, r04z)
        const bool nearAfterUp = nearIn && !oneX && fork && phase == 0 && ntier >= 1;
        if (nearIn && !oneX && !passShard) {  // the near field first: beside the up pass (fork) or before it (serial)
            if (fork) HIP_CHECK(hipEventRecord(evFork, s));
            if (!nearAfterUp) {
                nearStage();
                nearDone = true;
            }
            if (!fork && tm) e0 = mark(s);  // serial: the up span starts after the near field
        }
        if (ntier < 1) {  // a lone leaf: no up pass
            prepareCharges(K, in, dFT.as<double>(), dCT.as<double>(), s);
            if (fork) HIP_CHECK(hipEventRecord(evFork, s));
        }
        if (phase == 1 && ntier >= 1) {
            if (oneX)
                upTier(0, dXOwnT0Tasks.as<int>(), (int)plan.xOwnT0Tasks.size(), nullptr,
                       upPartial ? nullptr : rootsSend);
            else upTier(0, dXT0Tasks.as<int>(), (int)plan.xT0Tasks.size(), nullptr, rootsSend);
        }
        for (int k = nearUp ? 1 : 0; k < (topFused ? 1 : ntier) && phase == 0; ++k) {
            upTier(k, nullptr, tierTasks(k), nullptr, nullptr);
            if (k == 0 && nearAfterUp) {
                nearStage();
                nearDone = true;
            }
        }
        if (phase == 1) {
            const int ep = tm ? mark(s) : -1;
            span(1, e0, ep);
            if ((ntier < 1 || forkTier == 0) && !nearDone && !oneX && !passShard) {
                nearStage();
                nearDone = true;
            }
            pend.active = true;
            pend.nearDone = nearDone;
            pend.K = K;
            pend.e0 = e0;
            pend.eStart = eStart;
            pend.ePack = ep;
            return;
        }
    } else {
        e0 = pend.e0;
        eStart = pend.eStart;
        nearDone = pend.nearDone;
        pend.active = call.shardedPass;  // a sharded pass repeats its phase 2 per output window (phase 3)
        const int ex = tm ? mark(s) : -1;
        if (phase == 2) span(0, pend.ePack, ex);  // the caller's root exchange
        else eStart = ex;                         // a repeat's total span is its own
        if (oneX && !nearDone) {  // the rest of the near field after the one exchange (it filled the input's halo)
            // (a pass: every group here, in one launch)
            const bool late = !passShard;
            nin.grpList = late ? dNearGrpLate.as<int>() : nullptr;
            nin.ngrp = late ? (int)plan.nearGrpLate.size() : 0;
            if (fork) HIP_CHECK(hipEventRecord(evFork, s));
            nearStage();
            nin.grpList = nullptr;
            nin.ngrp = 0;
            nearDone = true;
        }
        if (phase == 3) {  // the chunk's multipoles are in dMult since its phase 2
        } else if (upPartial) {  // the exchange's unpack summed the upper multipoles
        } else if (topFused) {  // the upper tiers run inside the M2L launch below
        } else if (ntier >= 2) {  // the first upper tier reads the gathered roots (and stores them for the M2L)
            upTier(1, nullptr, tierTasks(1), rootsRecv, nullptr);
            for (int k = 2; k < ntier; ++k) upTier(k, nullptr, tierTasks(k), nullptr, nullptr);
        } else {
            launch_roots_unpack(K, (int)plan.xRootRecv.size(), dXRootRecv.as<int>(), rootsRecv, dMult.as<double>(),
                                s);
        }
        e0 = ex;  // the up span of phase 2: upper tiers
    }
    const int ep = tr ? mark(s) : -1;
    span(1, e0, ep);
    StageSpans sp(*this, s, eStart, ep);  // the tail's spans: M2L, gather, down pass, total
    if (!nearDone) {
        // a sharded pass in the two-collective form: the side stream waits here, behind the
        // previous window's k_add_rows, which reads the rows this near field writes
        if (passShard && fork) HIP_CHECK(hipEventRecord(evFork, s));
        nearStage();
        if (sn == s) sp.start();  // serial (ANISO_OVERLAP=0): the M2L span starts after the near field
    }
    if (mask & kStageFar) {
        if (topFused) {
            // the launch's LDS holds the largest task of tiers >= 1 only (tier 0 runs apart)
            // (sizing it for the 85-node tier-0 tasks too cost 0.3-0.5 %, r04j)
            const UpArgs ua{plan.upMaxTaskFrom(1), dUpDesc.as<int4>(), dUpGrpFix.as<int>(), dUpNode.as<int>(),
                            dUpCode.as<int4>(), dUpGeom.as<double4>(), dUpLeaf.as<int2>(), dPxT.as<double>(),
                            dPyT.as<double>(), x, ldx, treeIn ? 1 : 0, dPerm.as<int>(), sigT, dWT.as<double>(),
                            fTw, cTw, P, dMult.as<double>(),
                            phase == 2 ? dXRootSlot.as<int>() : nullptr};
            TopArgs ta{};
            const int u1 = plan.upTierTask[1];
            ta.nUp = plan.upTierTask[ntier] - u1;
            ta.ntier = ntier;
            for (int k = 1; k <= ntier; ++k) ta.blk0[k] = plan.upTierTask[k] - u1;
            for (int k = 1; k < ntier; ++k) ta.task0[k] = plan.upTierTask[k];
            ta.clWait = dHmClWait.as<int>();
            ta.cnt = dTopCnt.as<unsigned>();
            ta.recv1 = phase == 2 ? rootsRecv : nullptr;
            ta.spinLimit = topSpinLimit;
            ta.steals = dTopSteals.as<unsigned>();
            HIP_CHECK(hipHostGetDevicePointer((void**)&ta.err, topErr, 0));
            if (topTraceOn) {
                topTraceBlocks = ta.nUp + ncl;
                if (dTopTrace.bytes < (size_t)topTraceBlocks * 4 * sizeof(int64_t))
                    dTopTrace.alloc((size_t)topTraceBlocks * 4 * sizeof(int64_t));
                ta.trace = dTopTrace.as<int64_t>();
            }
            launch_top_m2l_hc(K, ncl, plan.hmMaxLds, ua, ta, hca, s);
        } else if (clustered) {
            m2lClusters(0, ncl, s);
        } else if (harmonic) {
            launch_m2l_hm(K, pairList(), dAttM2L.as<double>(), nodeBoxes(), P, hw, dMult.as<double>(), dLocal.as<double>(),
                          s, win);
        } else {
            launch_m2l(K, (int)plan.m2lTgt.size(), dM2LTgt.as<int>(), dM2LPtr.as<int64_t>(), dM2LNDir.as<int>(),
                       dM2LCanonBase.as<int>(), dM2LOutSlot.as<int>(), dM2LSrc.as<int>(), tab, nterm,
                       dMult.as<double>(), plan.m2lMaxCanon, dM2LPart.as<double>(), dLocal.as<double>(), s);
        }
    }
    sp.end(2);
    if (!harmonic && (mask & kStageFar) && plan.m2lCanon > 0) {
        launch_m2l_gather(K, (int)plan.m2lTgt.size(), dM2LTgt.as<int>(), dM2LInPtr.as<int>(), dM2LPart.as<double>(),
                          dLocal.as<double>(), s);
        sp.end(3);
    }
    if (fork) HIP_CHECK(hipStreamWaitEvent(s, evJoin, 0));
    // down pass (owned part), once for the sum over the terms (it is linear in the locals and
    // the partials).  The near partials: a single-RHS symmetric plan's
    if (mask & (kStageFar | kStageNear))
        downPass16(K, mask, !harmonic && plan.nearPartTotal > 0 ? dNearPart.as<double>() : nullptr,
                   halo && clustered ? dHmPart.as<double>() : nullptr, o, s);
    sp.end(5);
    sp.total();  // (at level 2 this route has no first mark, so no total: DESIGN.md §3.18.4)
}

// applyBlock on a high-order handle (np = 6, 8): the harmonic block apply
// with the far field of high_order.hip, as the un-fused sequence above.  The unstaged
// harmonic near field (it and the corrections do not depend on the order), and one M2L
// launch that reads every stored E block once for all modes (o.minuend: x - mforward(x)).
void Operator::applyBlockHigh(int K, const InRows& in, int nterm, const int* ids, const double* mixes, const OutRows& o,
                              hipStream_t s, int mask, const ApplyCall& call) {
    // a shard: only the matvec of a handle made by createSharded (call.hoShard), on the rank's
    // own lists below -- the whole input in tree order in, the owned slice out
    if (call.phase != 0 || (plan.nranks > 1 && !(hoShard && call.hoShard))) refuseHighOrder("a sharded apply");
    if (hoShard && !(call.hoShard && in.tree && o.tree)) refuseHoShard("a block apply");
    if (mask != kStageAll) refuseHighOrder("a per-stage apply");
    if (!attReady) throw std::runtime_error("high-order apply before cache()");
    HarmWeights hw;
    const HarmWindow* const win = call.pass ? &call.win : nullptr;
    if (win) hw = call.hw;
    else if (!harmonicWeights(K, nterm, ids, mixes, hw))
        refuseHighOrder("a block apply whose mixes are not aniso.m's forward / mforward");
    // the relaxed-precision operator (block_f32.hip): the whole operator on an unsharded
    // handle whose mirrors the caller has built
    const bool f32 = call.prec == ApplyPrec::F32;
    if (f32 && (win || hoShard || (dAttM2L.bytes && !dAttM2LF.p) || (dAttNear.bytes && !dAttNearF.p)))
        throw std::logic_error("the f32 block operator: a pass, a shard, or no float mirrors");
    hoReserve(K, s);
    const CorrFold& cf = corrTable(K, nterm, ids, mixes);
    StageSpans sp(*this, s);
    prepareCharges(K, in, dFT.as<double>(), dCT.as<double>(), s);
    if (f32) nearUnstagedF32(K, hw, o, s);
    else nearUnstaged(K, hw, win, mask, o, s);
    sp.end(4);
    corrections(K, cf, dFT.as<double>(), dCT.as<double>(), plan.ownBegin, plan.ownEnd, mask, o, s);
    sp.end(6);
    // (a shard: the up pass over every leaf of the tree -- the M2L reads any node's multipole)
    hoUpPass(K, dFT.as<double>(), dHoMult.as<double>(), hoShard, s);
    sp.end(1);
    sp.startRoofline();
    if (f32)
        launch_ho_m2l_f32(np, K, pairList(), dAttM2LF.as<float>(), nodeBoxes(), dHoTab.as<HoTables>(), hw,
                          dHoMult.as<double>(), dHoLocal.as<double>(), s);
    else
        launch_ho_m2l(np, K, pairList(), dAttM2L.as<double>(), nodeBoxes(), dHoTab.as<HoTables>(), hw, win,
                      dHoMult.as<double>(), dHoLocal.as<double>(), s);
    sp.end(2);
    hoDownPass(K, dHoLocal.as<double>(), o, s);
    sp.end(5);
    sp.total();
}

// ---- one mode on several vectors ----

bool Operator::modeApplyCheck(const char* what, int id, int nrhs, const void* x, int64_t ldx, const void* out,
                              int64_t ldo, bool minuend, bool f32) const {
    const std::string w(what);
    if (nrhs < 0) throw std::invalid_argument(w + ": nrhs must be >= 0, got " + std::to_string(nrhs));
    if (ldx < geo.N) throw std::invalid_argument(w + ": ldx = " + std::to_string(ldx) + " is below N = " + std::to_string(geo.N));
    if (ldo < geo.N) throw std::invalid_argument(w + ": ldo = " + std::to_string(ldo) + " is below N = " + std::to_string(geo.N));
    if (nrhs > 0 && !x) throw std::invalid_argument(w + ": x is NULL");
    if (nrhs > 0 && !out) throw std::invalid_argument(w + ": out is NULL");
    if (id < 0 || id >= kernelSize)
        throw std::out_of_range(w + ": kernel id " + std::to_string(id) + " out of range [0, " + std::to_string(kernelSize) + ")");
    if (nrhs == 0) return false;
    if (minuend) {  // the near field stores `out` before the down pass reads x at the same points
        const char* xb = static_cast<const char*>(x);
        const char* ob = static_cast<const char*>(out);
        const size_t xs = ((size_t)(nrhs - 1) * ldx + geo.N) * sizeof(double), os = ((size_t)(nrhs - 1) * ldo + geo.N) * sizeof(double);
        if (xb < ob + os && ob < xb + xs) throw std::invalid_argument(w + ": x and out overlap");
    }
    if (f32 && !highOrder())
        throw std::logic_error(w + ": the f32 mode operator is built for np = 6, 8; the reduced-precision route of an "
                                   "np = 4 handle is aniso_solve_mixed_dev");
    refuseHoShard(what);
    if (plan.nranks > 1)
        throw std::logic_error(w + " on a sharded handle: it writes every target (use an unsharded handle)");
    if (!coeffSet)
        throw std::runtime_error(w + " before aniso_set_coeff and aniso_cache(" + std::to_string(id) + ") or aniso_cache_block");
    const ModeCache& mc = modes[id];
    const bool shared = useAtt && attReady && plan.nearPartTotal == 0;  // the mode-shared caches serve it
    if (!mc.tables || !(highOrder() ? attReady : (mc.resident || shared)))
        throw std::runtime_error(w + " on kernel id " + std::to_string(id) + " before aniso_cache(" + std::to_string(id) +
                                 ") or aniso_cache_block");
    return true;
}

// One chunk on a high-order handle: applyBlockHigh's sequence with the mode kernels in place of
// launch_near_hm and launch_ho_m2l, and the corrections of mode id (identity fold; o.minuend:
// x - K_id(...)), on one half of 2, 4, 5 or 8 columns or on an 8-column half and a second one
// (a resident mode, or the wide setting) around ONE M2L for all their columns.  Half i has
// expansion buffers of its own, the block path's dHoMult / dHoLocal and dHoMult2 / dHoLocal2.
// The variation points:
//   near field -- f32: launch_near_mode_f32 per half; two halves with the mode's near blocks
//     resident: one launch for all 16 columns; otherwise nearMode per half;
//   M2L -- f32: the f32 mode kernel (one half only); the mode's M2L blocks resident: the MFMA
//     launch on them; two halves without them: the wide mode kernel on the E blocks (one factor
//     formation per entry, §3.18.9); otherwise the mode kernel;
//   order -- per half (charges, near field, corrections, up pass, then the next half: they share
//     dFT / dCT, the second half's charges are formed after the first's up pass has read them), or
//     per stage where the near launch is joint (the second half's charges live in dFT2 / dCT2;
//     same stage ids, each stage once for both halves).
void Operator::modeChunkHigh(int id, int nh, const ModeHalf* h, hipStream_t s, ApplyPrec prec) {
    const bool f32 = prec == ApplyPrec::F32, two = nh == 2;
    const double* F = f32 ? nullptr : modeBlocks.find(id);  // (the f32 entries ignore the resident blocks)
    if (two && (f32 || (!F && !wideOn)))
        throw std::logic_error("a 16-column mode chunk without resident blocks or the wide setting");
    const bool joint = two && modeNearBlocks.find(id);
    ensureWork(h[0].K);
    for (int i = 0; i < nh; ++i) hoReserve(h[i].K, s, i == 1);
    if (joint) reserveCharges2(h[1].K);
    double* const fT[2] = {dFT.as<double>(), (joint ? dFT2 : dFT).as<double>()};
    double* const cT[2] = {dCT.as<double>(), (joint ? dCT2 : dCT).as<double>()};
    double* const mult[2] = {dHoMult.as<double>(), dHoMult2.as<double>()};
    double* const local[2] = {dHoLocal.as<double>(), dHoLocal2.as<double>()};
    StageSpans sp(*this, s);
    // one round of the stages before the M2L per half, or one for both halves around the joint near launch
    const int step = joint ? 2 : 1;
    for (int i0 = 0; i0 < nh; i0 += step) {
        const int i1 = i0 + step;
        for (int i = i0; i < i1; ++i) prepareCharges(h[i].K, h[i].in, fT[i], cT[i], s);
        if (joint) nearMode16(id, h[0], h[1], s);
        else nearMode(h[i0].K, id, h[i0].o, s, prec);
        sp.end(4);
        for (int i = i0; i < i1; ++i) {
            // (corrTable may drop its folds when it adds one: the second half's is taken after the first's launch)
            const CorrFold& cf = corrTable(h[i].K, 1, &id, identityMix(h[i].K).data());
            corrections(h[i].K, cf, fT[i], cT[i], plan.ownBegin, plan.ownEnd, kStageAll, h[i].o, s);
        }
        sp.end(6);
        for (int i = i0; i < i1; ++i) hoUpPass(h[i].K, fT[i], mult[i], false, s);
        sp.end(1);
    }
    sp.startRoofline();
    if (f32)
        launch_ho_m2l_mode_f32(np, h[0].K, id, pairList(), dAttM2LF.as<float>(), nodeBoxes(), dHoTab.as<HoTables>(),
                               mult[0], local[0], s);
    else if (F)
        launch_ho_m2l_resident(np, id, pairList(), F, mult[0], h[0].K, two ? mult[1] : nullptr, two ? h[1].K : 0,
                               local[0], two ? local[1] : nullptr, s);
    else if (two)
        launch_ho_m2l_mode_wide(np, h[1].K, id, pairList(), dAttM2L.as<double>(), nodeBoxes(), dHoTab.as<HoTables>(),
                                mult[0], mult[1], local[0], local[1], s);
    else
        launch_ho_m2l_mode(np, h[0].K, id, pairList(), dAttM2L.as<double>(), nodeBoxes(), dHoTab.as<HoTables>(), mult[0],
                           local[0], s);
    sp.end(2);
    for (int i = 0; i < nh; ++i) hoDownPass(h[i].K, local[i], h[i].o, s);
    sp.end(5);
    sp.total();
}

// One chunk on a lean mode of an np = 4 handle: one pass of the offset form as leanMapping
// ends up running it, as the un-fused sequence, with the mode kernels in place of the offset
// near field and M2L: the corrections of mode id (identity fold), the rank-16 up tiers on the
// K plain columns, the mode M2L (plain sums into dLocal) and the down tiers (o.minuend:
// x - K_id(...), original order).
void Operator::modeApplyLean16(int id, int K, const InRows& in, const OutRows& o, hipStream_t s) {
    ensureWork(K);
    if (up_tier_lds(plan.upMaxTask, K) > 160 * 1024 ||
        down_tier_lds(plan.dnMaxTask, plan.dnMaxLeaves, plan.dnMaxNear, plan.dnMaxChain, K) > 160 * 1024)
        throw std::logic_error("up/down pass task exceeds one workgroup's LDS at " + std::to_string(K) + " right-hand sides");
    const CorrFold& cf = corrTable(K, 1, &id, identityMix(K).data());
    const int ntier = (int)plan.upTierTask.size() - 1;  // 0: a lone leaf
    StageSpans sp(*this, s);
    prepareCharges(K, in, dFT.as<double>(), dCT.as<double>(), s);
    nearMode(K, id, o, s);
    sp.end(4);
    corrections(K, cf, dFT.as<double>(), dCT.as<double>(), plan.ownBegin, plan.ownEnd, kStageAll, o, s);
    sp.end(6);
    // (the up tiers form their charges from the input again and store none: launch_prepare did)
    for (int k = 0; k < ntier; ++k)
        upTier16(K, k, nullptr, plan.upTierTask[k + 1] - plan.upTierTask[k], nullptr, nullptr, nullptr, nullptr,
                 nullptr, in, s);
    sp.end(1);
    sp.startRoofline();
    launch_m2l_mode16(K, id, pairList(), dAttM2L.as<double>(), nodeBoxes(), dParams.as<Params>(), dMult.as<double>(),
                      dLocal.as<double>(), s);
    sp.end(2);
    downPass16(K, kStageAll, nullptr, nullptr, o, s);
    sp.end(5);
    sp.total();
}

// zero rows pad the half to its compiled count, as applyBlock pads (the buffers grow and never
// shrink: a solve's active columns change the count)
ModeHalf Operator::stageHalf(int nb, int K, const double* x, int64_t ldx, const double* sigT, bool sub, double* out,
                             int64_t ldo, bool* padded, hipStream_t s) {
    *padded = K != nb;
    if (!*padded) return {K, InRows{x, ldx, false, sigT}, outRows(out, ldo, false, sub ? x : nullptr, ldx)};
    const int64_t N = geo.N;
    const size_t pb = (size_t)K * N * sizeof(double);
    if (dPadIn.bytes < pb) dPadIn.alloc(pb);
    if (dPadOut.bytes < pb) dPadOut.alloc(pb);
    padRowsIn(dPadIn, 1, nb, K, x, ldx, s);
    return {K, InRows{dPadIn.as<double>(), N, false, sigT},
            outRows(dPadOut.as<double>(), N, false, sub ? dPadIn.as<double>() : nullptr, N)};
}

void Operator::modeApplyDev(int id, int nrhs, const double* x, int64_t ldx, const double* sigT, bool minuend,
                            double* out, int64_t ldo, hipStream_t s, bool keepCalls, ApplyPrec prec) {
    if (!modeApplyCheck("mode apply", id, nrhs, x, ldx, out, ldo, minuend, prec == ApplyPrec::F32)) return;
    checkDeviceErrors();
    ensureDevice();
    if (prec == ApplyPrec::F32) cacheF32();  // (built on first use)
    if (!keepCalls) {
        modeCalls.clear();
        nearCalls.clear();
    }
    const int64_t N = geo.N;
    // a lean mode of an np = 4 handle on the mode-shared caches (leanMapping's conditions;
    // the mode kernels read the directed near blocks)
    const bool lean16 = !highOrder() && !modes[id].resident && useAtt && attReady && plan.nearPartTotal == 0;
    // its down tiers are the last writer of every point and fuse the forward form's
    // subtraction; a lone leaf has none and goes through the buffer below
    const bool viaBuffer = minuend && !highOrder() && !(lean16 && !plan.dnDesc.empty());
    if (highOrder() || lean16) {
        double* dst = out;
        int64_t ldd = ldo;
        if (viaBuffer) {
            if (dBlk.bytes < (size_t)nrhs * N * sizeof(double)) dBlk.alloc((size_t)nrhs * N * sizeof(double));
            dst = dBlk.as<double>();
            ldd = N;
        }
        const bool sub = minuend && !viaBuffer;
        // a chunk: up to 8 columns as one half, or (a width of 16) 9 .. 16 as an 8-column half
        // and a second one; a half of no compiled count is zero-padded to the next one
        const int width = modeChunkWidth(id, prec);
        for (int j0 = 0; j0 < nrhs;) {
            const int nc = std::min(width, nrhs - j0), nh = nc > kMaxRhs ? 2 : 1;
            ModeHalf h[2];
            int nb[2], padHalf = -1;
            for (int i = 0; i < nh; ++i) {
                const size_t r = (size_t)j0 + i * kMaxRhs;
                nb[i] = std::min(kMaxRhs, nc - i * kMaxRhs);
                const int K = nb[i] == 1 ? 2 : rhs_padded(nb[i]);  // (the mode kernels start at 2 columns)
                bool padded = false;
                h[i] = stageHalf(nb[i], K, x + r * ldx, ldx, sigT, sub, dst + r * ldd, ldd, &padded, s);
                if (padded) padHalf = i;  // (at most one: the first of two halves is full)
            }
            if (lean16) modeApplyLean16(id, h[0].K, h[0].in, h[0].o, s);
            else modeChunkHigh(id, nh, h, s, prec);
            if (padHalf >= 0)
                padRowsOut(dPadOut.as<double>(), nb[padHalf], N, dst + ((size_t)j0 + padHalf * kMaxRhs) * ldd, ldd, s);
            modeCalls.push_back(nh == 2 ? 2 * kMaxRhs : h[0].K);
            j0 += nc;
        }
        if (viaBuffer) launch_sub_slice(N, nrhs, x, ldx, dBlk.as<double>(), N, out, ldo, s);
        return;
    }
    // np = 4.  The forward form goes through a buffer: the applies store K_id(...) there
    // and the subtraction writes `out`
    double* dst = out;
    int64_t ldd = ldo;
    if (minuend) {
        dBlk.alloc((size_t)nrhs * N * sizeof(double));
        dst = dBlk.as<double>();
        ldd = N;
    }
    if (modes[id].resident) {  // mappingBatchedHost's 8-column branch on device pointers
        for (int j0 = 0; j0 < nrhs; j0 += kMaxRhs) {
            const int nb = std::min(kMaxRhs, nrhs - j0);
            ApplyCall call;
            applyBlock(nb, x + (size_t)j0 * ldx, ldx, false, sigT, 1, &id, identityMix(nb).data(),
                       dst + (size_t)j0 * ldd, ldd, false, s, kStageAll, call);
            modeCalls.push_back(rootRhs(nb));  // (applyBlock pads the chunk to the next compiled count)
        }
    } else {  // a lean mode the mode kernels do not serve: one pass of the offset form per column
        for (int j = 0; j < nrhs; ++j) {
            leanMapping(x + (size_t)j * ldx, id, dst + (size_t)j * ldd, s, kStageAll, sigT);
            modeCalls.push_back(kMaxRhs);
        }
    }
    if (minuend) launch_sub_slice(N, nrhs, x, ldx, dBlk.as<double>(), N, out, ldo, s);
}

// N x k column-major host arrays through modeApplyDev, 8 columns at a time
void Operator::mappingMultiHost(const double* Q, int k, int id, double* Out) {
    if (!modeApplyCheck("aniso_mapping_multi", id, k, Q, geo.N, Out, geo.N, false)) return;
    ensureDevice();
    const int64_t N = geo.N;
    const int kb = std::min(k, modeChunkWidth(id, ApplyPrec::F64));
    DevBuf dq, dout;
    dq.alloc((size_t)kb * N * sizeof(double));
    dout.alloc((size_t)kb * N * sizeof(double));
    modeCalls.clear();
    nearCalls.clear();
    for (int j0 = 0; j0 < k; j0 += kb) {
        const int nb = std::min(kb, k - j0);
        HIP_CHECK(hipMemcpyAsync(dq.p, Q + (size_t)j0 * N, (size_t)nb * N * sizeof(double), hipMemcpyHostToDevice, own));
        modeApplyDev(id, nb, dq.as<double>(), N, nullptr, false, dout.as<double>(), N, own, true);
        HIP_CHECK(hipMemcpyAsync(Out + (size_t)j0 * N, dout.p, (size_t)nb * N * sizeof(double), hipMemcpyDeviceToHost,
                                 own));
        HIP_CHECK(hipStreamSynchronize(own));
        checkDeviceErrors();
    }
}

// The modes of a batched apply: every one needs its correction tables; the per-mode
// stream (any apply that is not the harmonic one or a pass) needs their operators too.
// Raised before anything is staged or launched.
void Operator::checkModes(int K, int nterm, const int* ids, const double* mixes, const ApplyCall& call) const {
    bool lean = false;
    for (int t = 0; t < nterm; ++t) {
        if (ids[t] < 0 || ids[t] >= kernelSize) throw std::out_of_range("kernel id out of range");
        if (!modes[ids[t]].tables)
            throw std::runtime_error("mapping on kernel id " + std::to_string(ids[t]) + " before cache(" + std::to_string(ids[t]) + ")");
        lean = lean || !modes[ids[t]].resident;
    }
    if (!lean || highOrder()) return;  // (a high-order apply checks its own form, applyBlockHigh)
    if (call.pass && useAtt && attReady && plan.nearPartTotal == 0) return;  // a pass: the mode-shared caches
    HarmWeights hw;
    bool harmonic = false;
    if (rhs_supported(K)) {
        harmonic = harmonicWeights(K, nterm, ids, mixes, hw);
    } else if (K >= 1 && K <= kMaxRhs) {  // as applyBlock pads it
        const int Kp = rhs_padded(K);
        harmonic = harmonicWeights(Kp, nterm, ids, padMixes(K, Kp, nterm, mixes).data(), hw);
    }
    if (harmonic) return;
    for (int t = 0; t < nterm; ++t) needResident(ids[t], "a block apply down the per-mode operator stream");
}

int Operator::rootRhs(int nrhs) { return rhs_supported(nrhs) ? nrhs : rhs_padded(nrhs); }

// aniso.m forward / mforward mixes (aniso.m:121-157).  Output block iid takes,
// for every j in [-(nb-1), nb-1], mode m = |iid + j| of input block |j| with
// weight chi_|j| (mforward; 1 for forward).  Per mode m the pairs (iid, b = |j|)
// are j = m - iid and j = -m - iid (one j when m = 0).
std::vector<double> Operator::blockMixes(int nb, double g, bool chi) {
    if (nb < 1) throw std::invalid_argument("block count must be >= 1");
    const int nm = 2 * nb - 1;
    std::vector<double> mix((size_t)nm * nb * nb, 0.0);
    const double gN = std::pow(g, nb);
    for (int iid = 0; iid < nb; ++iid)
        for (int j = -(nb - 1); j <= nb - 1; ++j) {
            const int b = std::abs(j), m = std::abs(iid + j);
            const double w = chi ? (std::pow(g, b) - gN) / (1.0 - gN) : 1.0;
            mix[((size_t)m * nb + iid) * nb + b] += w;
        }
    return mix;
}

void Operator::blockOpDev(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool treeIo,
                          hipStream_t s, double gval, const double* sigT, int phase, double* rootsSend,
                          const double* rootsRecv, ApplyPrec prec) {
    if (which < 0 || which > 2) throw std::invalid_argument("block operator: which must be 0, 1 or 2");
    if (prec == ApplyPrec::F32) blockOpF32Refuse("the f32 block operator");
    if (phase != 0) refuseHighOrder("the two-phase block operator");
    // a sharded high-order handle: the matvec of blockOpShardedHigh for a caller who gathered
    // the input -- the whole vector in tree order in, the owned slice out
    if (hoShard && !treeIo) refuseHoShard("aniso_block_op_dev in original order");
    checkBlockLimit(phase != 0);
    if (!coeffSet) throw std::runtime_error("block operator before setCoeff");
    ensureDevice();
    if (ks > kMaxRhs) {  // more blocks than one harmonic launch holds: P x P passes of 8
        blockOpPasses(which, x, ldx, out, ldo, treeIo, s, std::isnan(gval) ? g : gval,
                      sigT ? sigT : dSigmaT.as<double>());
        return;
    }
    ApplyCall call;
    call.phased(phase, rootsSend, rootsRecv);
    call.hoShard = hoShard;
    call.prec = prec;
    if (hoShard && plan.ownEnd == plan.ownBegin) return;  // a rank that owns nothing
    blockOp(which, x, ldx, out, ldo, treeIo, s, gval, sigT, call);
}

// ---- the relaxed-precision block operator ----

void Operator::blockOpF32Refuse(const char* what) const {
    const std::string w(what);
    if (!highOrder())
        throw std::logic_error(w + ": the f32 block operator is built for np = 6, 8; the reduced-precision route of an "
                                   "np = 4 handle is aniso_solve_mixed_dev");
    refuseHoShard(what);
    if (plan.nranks > 1) throw std::logic_error(w + " on a sharded handle (use an unsharded handle)");
    if (ks > kMaxRhs)
        throw std::logic_error(w + ": ks = " + std::to_string(ks) + " blocks run as passes of " +
                               std::to_string(kMaxRhs) + ", and the passes have no f32 form");
}

void Operator::blockOpF32Ready(const char* what) const {
    bool ready = coeffSet && attReady;
    for (int m = 0; ready && m < kernelSize; ++m) ready = modes[m].tables;
    if (!ready)
        throw std::runtime_error(std::string(what) + " before aniso_set_coeff and aniso_cache_block (or aniso_cache of "
                                                     "every mode)");
}

void Operator::blockOpF32Dev(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool treeIo,
                             hipStream_t s) {
    const char* const what = "aniso_block_op_f32_dev";
    if (which < 0 || which > 2) throw std::invalid_argument("block operator: which must be 0, 1 or 2");
    blockOpF32Refuse(what);
    blockOpF32Ready(what);
    if (ldx < geo.N || ldo < geo.N) throw std::invalid_argument("block apply: leading dimension too small");
    cacheF32();  // the float mirrors, if this is their first use: before anything is launched
    blockOpDev(which, x, ldx, out, ldo, treeIo, s, NAN, nullptr, 0, nullptr, nullptr, ApplyPrec::F32);
}

void Operator::blockOp(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool treeIo, hipStream_t s,
                       double gval, const double* sigT, ApplyCall& call) {
    const int phase = call.phase;
    const int nb = ks, nm = 2 * ks - 1;
    const auto mix = blockMixes(nb, std::isnan(gval) ? g : gval, which != 0);
    const double* sig = sigT ? sigT : dSigmaT.as<double>();
    pendingCall(phase, PendingCall{1, which, x, out, sig, ldx, ldo, std::isnan(gval) ? g : gval});
    const std::vector<int> ids = modeIds(nm);
    if (which < 2) {
        applyBlock(nb, x, ldx, treeIo, which != 0 ? sig : nullptr, nm, ids.data(), mix.data(), out, ldo, treeIo, s,
                   kStageAll, call);
        return;
    }
    // x - mforward(x) on the owned targets (aniso.m:155)
    const int64_t nOut = treeIo ? plan.ownEnd - plan.ownBegin : geo.N;
    if (!treeIo && plan.nranks != 1) throw std::logic_error("block matvec in original order on a sharded handle: use tree order");
    const double* xo = x + (treeIo ? plan.ownBegin : 0);  // x at the output positions
    if (fuseSub && rhs_supported(nb) && (highOrder() ? nb > 1 : !plan.dnDesc.empty())) {
        // the down pass, last writer of every owned point, stores x - (near + corr + far)
        call.minuend = xo;
        call.minuendLd = ldx;
        applyBlock(nb, x, ldx, treeIo, sig, nm, ids.data(), mix.data(), out, ldo, treeIo, s, kStageAll, call);
        return;
    }
    if (phase != 2) dBlk.alloc((size_t)nb * nOut * sizeof(double));
    applyBlock(nb, x, ldx, treeIo, sig, nm, ids.data(), mix.data(), dBlk.as<double>(), nOut, treeIo, s, kStageAll,
               call);
    if (phase != 1) launch_sub_slice(nOut, nb, xo, ldx, dBlk.as<double>(), nOut, out, ldo, s);
}

// ---- more than kMaxRhs blocks ----
//
// aniso.m loops over any number of blocks (aniso.m:139-157); the harmonic kernels hold
// kMaxRhs.  The identity of harmonic.hip does not depend on the block count, so the
// blocks are cut into P = ceil(ks / 8) chunks of 8 (the last zero-padded) and the
// operator into P x P passes: pass (I, J) adds to output rows 8 I .. 8 I + 7
//     (E / r) T_{8I+i}(c) sum_{b < 8} hw_{8J+b} T_{8J+b}(c) x_{8J+b},
// over the M2L and the near field, with the correction stencils folded from the
// (2 ks - 1) x 8 x 8 sub-block of the mixes and the r = 0 diagonal term only at I == J.
// Every pass reads the mode-shared E caches once (P^2 reads per block apply) and no
// per-mode operator cache.

void Operator::blockPassPlan(int ks, int* chunk, int* nchunks) {
    if (ks < 1) throw std::invalid_argument("block count must be >= 1");
    *chunk = ks <= kMaxRhs ? ks : kMaxRhs;
    *nchunks = ks <= kMaxRhs ? 1 : (ks + kMaxRhs - 1) / kMaxRhs;
}

// ks > kMaxRhs runs on an unsharded handle, or on a shard through the library's own
// exchange (blockOpShardedDev, which does not come here); the phase-0 entry points of
// a sharded handle and the caller-driven two-phase forms are refused, before anything
// is launched or any pending-call state is set
void Operator::checkBlockLimit(bool shardedCall) const {
    if (ks > kMaxRhs && hoShard)
        throw std::invalid_argument("block operator: ks = " + std::to_string(ks) + " blocks on a sharded high-order handle "
                                    "(its matvec holds at most " + std::to_string(kMaxRhs) + " blocks)");
    if (ks > kMaxRhs && (plan.nranks > 1 || shardedCall))
        throw std::invalid_argument("block operator: ks = " + std::to_string(ks) + " blocks on a sharded handle (more than " +
                                    std::to_string(kMaxRhs) + " blocks run on unsharded handles, and on shards through "
                                    "aniso_block_op_sharded_dev only)");
}

void Operator::passMix(int I, int J, const std::vector<double>& mix, std::vector<double>& sub, HarmWeights& hw) const {
    constexpr int K = kMaxRhs;
    const int nm = 2 * ks - 1, i0 = I * K, b0 = J * K;
    auto mx = [&](int m, int i, int b) { return i < ks && b < ks ? mix[((size_t)m * ks + i) * ks + b] : 0.0; };
    sub.assign((size_t)nm * K * K, 0.0);
    for (int m = 0; m < nm; ++m)
        for (int i = 0; i < K; ++i)
            for (int b = 0; b < K; ++b) sub[((size_t)m * K + i) * K + b] = mx(m, i0 + i, b0 + b);
    // the pass's harmonic weights straight from the block weights: output row 0 holds
    // hw_B at mode B (w_0, or 2 w_B: j = B and j = -B), the mode-0 weight of row i is w_i
    std::memset(&hw, 0, sizeof(hw));
    for (int b = 0; b < K; ++b) hw.hw[b] = b0 + b < ks ? mx(b0 + b, 0, b0 + b) : 0.0;
    for (int i = 0; i < K; ++i) {
        hw.om[i] = i0 + i < ks ? 1.0 : 0.0;
        hw.dw[i] = I == J ? mx(0, i0 + i, i0 + i) : 0.0;
    }
}

// One pass: input chunk J of x (ks rows) to the 8 rows out8 of output chunk I.  sig:
// sigma_s in tree order, or nullptr (forward).  mix: blockMixes(ks, g, chi).
void Operator::blockPass(int I, int J, const std::vector<double>& mix, const double* x, int64_t ldx, bool tree,
                         const double* sig, double* out8, int64_t ldo, hipStream_t s) {
    constexpr int K = kMaxRhs;
    const int nm = 2 * ks - 1, i0 = I * K, b0 = J * K;
    const int64_t N = geo.N;
    if (ldx < N || ldo < N) throw std::invalid_argument("block apply: leading dimension too small");
    std::vector<double> sub;
    ApplyCall call;
    call.pass = true;
    call.win = HarmWindow{i0, b0};
    passMix(I, J, mix, sub, call.hw);
    const std::vector<int> ids = modeIds(nm);
    const std::pair<double*, int64_t> in = stagePassInput(const_cast<double*>(x), ldx, b0, s);  // (read only)
    applyBlock(K, in.first, in.second, tree, sig, nm, ids.data(), sub.data(), out8, ldo, tree, s, kStageAll, call);
}

// The chunk's rows of x (from row b0); the last chunk zero-padded to kMaxRhs rows in dPassIn.
std::pair<double*, int64_t> Operator::stagePassInput(double* x, int64_t ldx, int b0, hipStream_t s) {
    constexpr int K = kMaxRhs;
    const int64_t N = geo.N;
    const int nin = std::min(K, ks - b0);
    double* const xin = x + (size_t)b0 * ldx;
    if (nin == K) return {xin, ldx};
    dPassIn.alloc((size_t)K * N * sizeof(double));
    padRowsIn(dPassIn, 1, nin, K, xin, ldx, s);
    return {dPassIn.as<double>(), N};
}

void Operator::blockOpPasses(int which, const double* x, int64_t ldx, double* out, int64_t ldo, bool treeIo,
                             hipStream_t s, double gval, const double* sig) {
    constexpr int K = kMaxRhs;
    const int P = (ks + K - 1) / K;
    const int64_t N = geo.N;
    if (ldx < N || ldo < N) throw std::invalid_argument("block apply: leading dimension too small");
    const auto mix = blockMixes(ks, gval, which != 0);
    dPassOut.alloc((size_t)K * N * sizeof(double));
    double* acc = out;
    int64_t lda = ldo;
    if (which == 2) {  // x - mforward(x): the passes sum into dBlk
        dBlk.alloc((size_t)ks * N * sizeof(double));
        acc = dBlk.as<double>();
        lda = N;
    }
    for (int I = 0; I < P; ++I)
        for (int J = 0; J < P; ++J) {
            blockPass(I, J, mix, x, ldx, treeIo, which != 0 ? sig : nullptr, dPassOut.as<double>(), N, s);
            launch_add_rows(N, std::min(K, ks - I * K), dPassOut.as<double>(), N, acc + (size_t)I * K * lda, lda,
                            J > 0 ? 1 : 0, s);
        }
    if (which == 2) launch_sub_slice(N, ks, x, ldx, dBlk.as<double>(), N, out, ldo, s);
}

void Operator::blockPassDev(int which, int I, int J, const double* x, int64_t ldx, double* out, int64_t ldo,
                            hipStream_t s) {
    if (which < 0 || which > 1) throw std::invalid_argument("block pass: which must be 0 or 1");
    refuseHoShard("aniso_block_pass_dev");
    if (plan.nranks > 1) throw std::invalid_argument("block pass: unsharded handles only");
    int chunk = 0, P = 0;
    blockPassPlan(ks, &chunk, &P);
    if (I < 0 || I >= P || J < 0 || J >= P) throw std::invalid_argument("block pass: chunk index out of range");
    if (!coeffSet) throw std::runtime_error("block operator before setCoeff");
    ensureDevice();
    if (P == 1) {  // one pass is the operator itself
        blockOpDev(which, x, ldx, out, ldo, false, s);
        return;
    }
    const auto mix = blockMixes(ks, g, which != 0);
    blockPass(I, J, mix, x, ldx, false, which != 0 ? dSigmaT.as<double>() : nullptr, out, ldo, s);
}

void Operator::blockOpHost(int which, const double* u, const double* sigmaS, double gval, double* out) {
    refuseHoShard("the host block operator");
    checkBlockLimit(false);
    if (plan.nranks != 1) throw std::logic_error("host block operator on a sharded handle");
    if (!coeffSet) throw std::runtime_error("block operator before setCoeff");
    ensureDevice();
    const int64_t N = geo.N;
    const size_t bytes = (size_t)ks * N * sizeof(double);
    dHostIn.alloc(bytes);
    dHostOut.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(dHostIn.p, u, bytes, hipMemcpyHostToDevice, own));
    const double* sigT = nullptr;
    if (sigmaS) {
        std::vector<double> sT(N);
        for (int64_t k = 0; k < N; ++k) sT[k] = sigmaS[tree.perm[k]];
        HIP_CHECK(hipStreamSynchronize(own));  // a previous call may still read dSigAlt
        dSigAlt.upload(sT.data(), N * sizeof(double));
        sigT = dSigAlt.as<double>();
    }
    blockOpDev(which, dHostIn.as<double>(), N, dHostOut.as<double>(), N, false, own, gval, sigT);
    HIP_CHECK(hipMemcpyAsync(out, dHostOut.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    if (recoverTopTimeout(own)) {  // the fused launch timed out: the same apply on the tier launches
        struct Restore {
            bool& f;
            ~Restore() { f = false; }
        } restore{forceUnfused};
        blockOpDev(which, dHostIn.as<double>(), N, dHostOut.as<double>(), N, false, own, gval, sigT);
        HIP_CHECK(hipMemcpyAsync(out, dHostOut.p, bytes, hipMemcpyDeviceToHost, own));
        HIP_CHECK(hipStreamSynchronize(own));
    }
    checkDeviceErrors();
}

// ---- the block operator for several sources ----

bool Operator::blockOpMultiCheck(const char* what, int which, int nsrc, const void* x, int64_t ldx, const void* out,
                                 int64_t ldo) const {
    const std::string w(what);
    const int64_t N = geo.N;
    if (nsrc < 0) throw std::invalid_argument(w + ": nsrc must be >= 0, got " + std::to_string(nsrc));
    if (which < 0 || which > 2) throw std::invalid_argument(w + ": which must be 0, 1 or 2, got " + std::to_string(which));
    if (ldx < N) throw std::invalid_argument(w + ": the input stride " + std::to_string(ldx) + " is below N = " + std::to_string(N));
    if (ldo < N) throw std::invalid_argument(w + ": the output stride " + std::to_string(ldo) + " is below N = " + std::to_string(N));
    if (nsrc > 0 && !x) throw std::invalid_argument(w + ": the input is NULL");
    if (nsrc > 0 && !out) throw std::invalid_argument(w + ": the output is NULL");
    if (nsrc == 0) return false;
    {  // a source's near field stores its output rows before the next source's input rows are read
        const char* xb = static_cast<const char*>(x);
        const char* ob = static_cast<const char*>(out);
        const size_t rows = (size_t)nsrc * ks - 1;
        const size_t xs = (rows * ldx + N) * sizeof(double), os = (rows * ldo + N) * sizeof(double);
        if (xb < ob + os && ob < xb + xs) throw std::invalid_argument(w + ": the input and output rows overlap");
    }
    refuseHoShard(what);
    if (plan.nranks > 1)
        throw std::logic_error(w + " on a sharded handle: it writes every target (use an unsharded handle)");
    if (!coeffSet) throw std::runtime_error(w + " before aniso_set_coeff and aniso_cache_block");
    const bool shared = useAtt && attReady && plan.nearPartTotal == 0;  // the mode-shared caches serve a lean mode
    for (int m = 0; m < 2 * ks - 1; ++m) {
        const ModeCache& mc = modes[m];
        if (!mc.tables || !(highOrder() ? attReady : (mc.resident || shared)))
            throw std::runtime_error(w + " before mode " + std::to_string(m) + " of 0 .. " + std::to_string(2 * ks - 2) +
                                     " is ready: call aniso_cache_block (or aniso_cache for every mode)");
    }
    return true;
}

// the chunk's buffers for S sources: S multipole and S local buffers beside dHoMult / dHoLocal,
// and the rows of a block count that is not compiled padded with zero blocks
void Operator::blockMultiReserve(int S) {
    const int K = ks == 1 ? 2 : rhs_padded(ks);
    const size_t exp = (size_t)S * tree.nn * np * np * K * sizeof(double);
    ensureWork(K);
    if (dMsMult.bytes < exp) dMsMult.alloc(exp);
    if (dMsLocal.bytes < exp) dMsLocal.alloc(exp);
    if (K != ks) {
        const size_t pad = (size_t)S * K * geo.N * sizeof(double);
        if (dMsIn.bytes < pad) dMsIn.alloc(pad);
        if (dMsOut.bytes < pad) dMsOut.alloc(pad);
    }
}

// One chunk on a high-order handle: applyBlockHigh's launch sequence with launch_prepare, the
// near field, the corrections, P2M and M2M per source (each into its own multipole buffer),
// ONE M2L launch for the chunk, then L2L and L2P per source, the last writer of its rows
// (which = 2: x - mforward(x) through the L2P's minuend).  An absent source (nreal < S) is a
// zero multipole buffer whose locals nobody reads.
void Operator::blockMultiChunk(int which, int S, int nreal, const double* x, int64_t ldx, double* out, int64_t ldo,
                               hipStream_t s, ApplyPrec prec) {
    const int nb = ks, nm = 2 * ks - 1, K = nb == 1 ? 2 : rhs_padded(nb);
    const int64_t N = geo.N;
    std::vector<double> mix = blockMixes(nb, g, which != 0);
    if (K != nb) mix = padMixes(nb, K, nm, mix.data());
    const std::vector<int> ids = modeIds(nm);
    HarmWeights hw;
    if (!harmonicWeights(K, nm, ids.data(), mix.data(), hw))
        throw std::logic_error("multi-source block operator: the mode-shared caches are not ready");
    const double* sigT = which != 0 ? dSigmaT.as<double>() : nullptr;
    // the relaxed-precision chunk: applyBlockHigh's f32 near field per source
    // and the f32 M2L, on the mirrors the caller has built; every other stage is the fp64 one
    const bool f32 = prec == ApplyPrec::F32;
    if (f32 && ((dAttM2L.bytes && !dAttM2LF.p) || (dAttNear.bytes && !dAttNearF.p)))
        throw std::logic_error("the f32 multi-source block operator: no float mirrors");
    blockMultiReserve(S);
    const size_t exp = hoDoubles(K);
    const CorrFold& cf = corrTable(K, nm, ids.data(), mix.data());
    // source j's rows: the caller's, or its K rows of the padded buffers (stride N)
    const bool padded = K != nb;
    const double* const xs = padded ? dMsIn.as<double>() : x;
    double* const os = padded ? dMsOut.as<double>() : out;
    const int64_t ldi = padded ? N : ldx, ldw = padded ? N : ldo;
    const size_t rows = padded ? K : nb;
    auto rowsIn = [&](int j) { return InRows{xs + j * rows * ldi, ldi, false, sigT}; };
    auto rowsOut = [&](int j) {
        return outRows(os + j * rows * ldw, ldw, false, which == 2 ? xs + j * rows * ldi : nullptr, ldi);
    };
    StageSpans sp(*this, s);
    if (padded) padRowsIn(dMsIn, nreal, nb, K, x, ldx, s);
    // nodes that are no M2L target (the root, empty nodes) keep zero locals
    HIP_CHECK(hipMemsetAsync(dMsLocal.p, 0, (size_t)S * exp * sizeof(double), s));
    if (nreal < S)
        HIP_CHECK(hipMemsetAsync(dMsMult.as<double>() + (size_t)nreal * exp, 0, (size_t)(S - nreal) * exp * sizeof(double), s));
    for (int j = 0; j < nreal; ++j) {
        const OutRows o = rowsOut(j);
        sp.start();
        prepareCharges(K, rowsIn(j), dFT.as<double>(), dCT.as<double>(), s);
        if (f32) nearUnstagedF32(K, hw, o, s);
        else nearUnstaged(K, hw, nullptr, kStageAll, o, s);
        sp.end(4);
        corrections(K, cf, dFT.as<double>(), dCT.as<double>(), plan.ownBegin, plan.ownEnd, kStageAll, o, s);
        sp.end(6);
        hoUpPass(K, dFT.as<double>(), dMsMult.as<double>() + (size_t)j * exp, false, s);
        sp.end(1);
    }
    sp.start();
    if (f32)
        launch_ho_m2l_src_f32(np, K, S, pairList(), dAttM2LF.as<float>(), nodeBoxes(), dHoTab.as<HoTables>(), hw,
                              dMsMult.as<double>(), (int64_t)exp, dMsLocal.as<double>(), (int64_t)exp, s);
    else
        launch_ho_m2l_src(np, K, S, pairList(), dAttM2L.as<double>(), nodeBoxes(), dHoTab.as<HoTables>(), hw,
                          dMsMult.as<double>(), (int64_t)exp, dMsLocal.as<double>(), (int64_t)exp, s);
    sp.end(2);
    for (int j = 0; j < nreal; ++j) {
        const OutRows o = rowsOut(j);
        hoDownPass(K, dMsLocal.as<double>() + (size_t)j * exp, o, s);
        if (padded) padRowsOut(o.out, nb, N, out + (size_t)j * nb * ldo, ldo, s);
    }
    sp.end(5);
    sp.total();
}

void Operator::blockOpMultiDev(int which, int nsrc, const double* x, int64_t ldx, double* out, int64_t ldo,
                               hipStream_t s) {
    if (!blockOpMultiCheck("multi-source block operator", which, nsrc, x, ldx, out, ldo)) return;
    checkDeviceErrors();
    ensureDevice();
    if (!highOrder() || ks > kMaxRhs) {  // nothing shared: the existing operator per source
        for (int j = 0; j < nsrc; ++j)
            blockOpDev(which, x + (size_t)j * ks * ldx, ldx, out + (size_t)j * ks * ldo, ldo, false, s);
        return;
    }
    for (int j0 = 0; j0 < nsrc; j0 += 4) {
        const int n = std::min(4, nsrc - j0);
        blockMultiChunk(which, n == 3 ? 4 : n, n, x + (size_t)j0 * ks * ldx, ldx, out + (size_t)j0 * ks * ldo, ldo, s);
    }
}

// The relaxed-precision operator for several sources: blockOpMultiDev's
// chunking on the f32 chunk.  What the handle rules out, the arguments and the state are
// raised before the device is touched; the mirrors are built on first use, before any launch.
void Operator::blockOpMultiF32Dev(int which, int nsrc, const double* x, int64_t ldx, double* out, int64_t ldo,
                                  hipStream_t s) {
    const char* const what = "aniso_block_op_multi_f32_dev";
    blockOpF32Refuse(what);
    if (!blockOpMultiCheck(what, which, nsrc, x, ldx, out, ldo)) return;
    blockOpF32Ready(what);
    checkDeviceErrors();
    ensureDevice();
    cacheF32();
    for (int j0 = 0; j0 < nsrc; j0 += 4) {
        const int n = std::min(4, nsrc - j0);
        blockMultiChunk(which, n == 3 ? 4 : n, n, x + (size_t)j0 * ks * ldx, ldx, out + (size_t)j0 * ks * ldo, ldo, s,
                        ApplyPrec::F32);
    }
}

// (ks N) x nsrc column-major host arrays: one staging copy each way
void Operator::blockOpMultiHost(int which, const double* U, int nsrc, double* Out) {
    if (!blockOpMultiCheck("aniso_block_op_multi", which, nsrc, U, geo.N, Out, geo.N)) return;
    ensureDevice();
    const size_t bytes = (size_t)nsrc * ks * geo.N * sizeof(double);
    DevBuf du, dout;
    du.alloc(bytes);
    dout.alloc(bytes);
    HIP_CHECK(hipMemcpyAsync(du.p, U, bytes, hipMemcpyHostToDevice, own));
    blockOpMultiDev(which, nsrc, du.as<double>(), geo.N, dout.as<double>(), geo.N, own);
    HIP_CHECK(hipMemcpyAsync(Out, dout.p, bytes, hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    checkDeviceErrors();
}

// ---- direct evaluation at chosen targets (direct.hip) ----
//
// The direct sum over all N sources gives the near field a one-leaf tree would compute;
// the stencil and singular corrections do not depend on the tree, so they come from the
// apply's own correction kernel (launch_corr on the charges launch_prepare forms, at all
// N points) and are read out at the targets by the direct kernel's reduction.

bool Operator::directCheck(const char* what, bool block, int id, int which, const void* in, const char* inName,
                           int64_t ldx, const int64_t* targets, int64_t nt, const void* out, int64_t ldo) const {
    const std::string w(what);
    refuseHoShard(what);
    if (plan.nranks > 1)
        throw std::logic_error(w + " on a sharded handle: a direct sum needs every source (use an unsharded handle)");
    if (block) {
        if (which < 0 || which > 2) throw std::invalid_argument(w + ": which must be 0, 1 or 2");
    } else if (id < 0 || id >= kernelSize) {
        throw std::out_of_range(w + ": kernel id " + std::to_string(id) + " out of range [0, " + std::to_string(kernelSize) + ")");
    }
    if (nt < 0) throw std::invalid_argument(w + ": nt must be >= 0, got " + std::to_string(nt));
    if (block && ldo < nt)
        throw std::invalid_argument(w + ": ldo = " + std::to_string(ldo) + " is below nt = " + std::to_string(nt));
    if (block && nt > 0 && ldx < geo.N)
        throw std::invalid_argument(w + ": ldx = " + std::to_string(ldx) + " is below N = " + std::to_string(geo.N));
    if (nt == 0) return false;
    if (!in) throw std::invalid_argument(w + ": " + inName + " is NULL");
    if (!targets) throw std::invalid_argument(w + ": targets is NULL");
    if (!out) throw std::invalid_argument(w + ": out is NULL");
    for (int64_t t = 0; t < nt; ++t)
        if (targets[t] < 0 || targets[t] >= geo.N)
            throw std::invalid_argument(w + ": targets[" + std::to_string(t) + "] = " + std::to_string(targets[t]) +
                                        " is outside [0, N = " + std::to_string(geo.N) + ")");
    if (!coeffSet) throw std::runtime_error(w + " before setCoeff");
    for (int m = block ? 0 : id; m < (block ? kernelSize : id + 1); ++m)
        if (!modes[m].tables)
            throw std::runtime_error(w + " on kernel id " + std::to_string(m) + " before cache(" + std::to_string(m) +
                                     ") or aniso_cache_block");
    return true;
}

// The call's device state: the targets, the weights (hw then dw) and room for one
// launch's partials.  The buffers are the handle's, so the previous direct call's
// launches (on whatever stream) are waited for first.
void Operator::directBegin(const int64_t* targets, int64_t nt, const std::vector<double>& weights, int KO) {
    HIP_CHECK(hipEventSynchronize(evDirect));
    if (dDirTg.bytes < (size_t)nt * sizeof(int64_t)) dDirTg.alloc((size_t)nt * sizeof(int64_t));
    HIP_CHECK(hipMemcpy(dDirTg.p, targets, (size_t)nt * sizeof(int64_t), hipMemcpyHostToDevice));
    if (dDirW.bytes < weights.size() * sizeof(double)) dDirW.alloc(weights.size() * sizeof(double));
    HIP_CHECK(hipMemcpy(dDirW.p, weights.data(), weights.size() * sizeof(double), hipMemcpyHostToDevice));
    const size_t pb = (size_t)std::min<int64_t>(nt, directChunk) * direct_blocks(geo.N) * KO * sizeof(double);
    if (dDirPart.bytes < pb) dDirPart.alloc(pb);
}

// corr (K rows of N, original order) += the stencil and singular corrections of the K
// input rows under the terms' mixes: the apply's charges and its correction kernel.
void Operator::directCorr(int K, const double* x, int64_t ldx, const double* sig, int nterm, const int* ids,
                          const double* mixes, double* corr, hipStream_t s) {
    const int64_t N = geo.N;
    const size_t cb = (size_t)N * rhs_stride(K) * sizeof(double);
    if (dDirF.bytes < cb) {
        dDirF.alloc(cb);
        dDirC.alloc(cb);
    }
    const CorrFold& cf = corrTable(K, nterm, ids, mixes);
    prepareCharges(K, InRows{x, ldx, false, sig}, dDirF.as<double>(), dDirC.as<double>(), s);
    corrections(K, cf, dDirF.as<double>(), dDirC.as<double>(), 0, N, kStageStencil | kStageSing,
                outRows(corr, N, false), s);
}

// One window's rows for every target, a bounded number of targets per launch.
void Operator::directSweep(int KO, DirectArgs a, int64_t nt, hipStream_t s) {
    a.N = geo.N;
    a.perm = dPerm.as<int>();
    a.iperm = dIperm.as<int>();
    a.wT = dWT.as<double>();
    a.pxT = dPxT.as<double>();
    a.pyT = dPyT.as<double>();
    a.stcoef = dStCoef.as<double>();
    a.P = dParams.as<Params>();
    a.tg = dDirTg.as<int64_t>();
    a.part = dDirPart.as<double>();
    a.scale = M_1_PI / 2.0;  // AnisoWrapper.cpp:129-130
    a.corr = dDirCorr.as<double>();
    a.ldc = geo.N;
    for (int64_t t0 = 0; t0 < nt; t0 += directChunk) {
        a.t0 = t0;
        launch_direct(KO, (int)std::min<int64_t>(directChunk, nt - t0), a, s);
    }
}

void Operator::mappingDirectDev(const double* charge, int id, const int64_t* targets, int64_t nt, double* out,
                                hipStream_t s) {
    if (!directCheck("aniso_mapping_direct", false, id, 0, charge, "charge", geo.N, targets, nt, out, nt)) return;
    ensureDevice();
    checkDeviceErrors();
    const int64_t N = geo.N;
    directBegin(targets, nt, {1.0, id == 0 ? 1.0 : 0.0}, 1);
    if (dDirCorr.bytes < (size_t)N * sizeof(double)) dDirCorr.alloc((size_t)N * sizeof(double));
    HIP_CHECK(hipMemsetAsync(dDirCorr.p, 0, (size_t)N * sizeof(double), s));
    const double one = 1.0;
    directCorr(1, charge, N, nullptr, 1, &id, &one, dDirCorr.as<double>(), s);
    DirectArgs a;
    a.nb = 1;
    a.m0 = id;
    a.nout = 1;
    a.x = charge;
    a.ldx = N;
    a.hw = dDirW.as<double>();
    a.dw = dDirW.as<double>() + 1;
    a.out = out;
    a.ldo = nt;
    directSweep(1, a, nt, s);
    HIP_CHECK(hipEventRecord(evDirect, s));
}

void Operator::mappingDirectHost(const double* charge, int id, const int64_t* targets, int64_t nt, double* out) {
    if (!directCheck("aniso_mapping_direct", false, id, 0, charge, "charge", geo.N, targets, nt, out, nt)) return;
    ensureDevice();
    HIP_CHECK(hipMemcpyAsync(dCharge.p, charge, geo.N * sizeof(double), hipMemcpyHostToDevice, own));
    HIP_CHECK(hipEventSynchronize(evDirect));  // dDirOut may still be written
    if (dDirOut.bytes < (size_t)nt * sizeof(double)) dDirOut.alloc((size_t)nt * sizeof(double));
    mappingDirectDev(dCharge.as<double>(), id, targets, nt, dDirOut.as<double>(), own);
    HIP_CHECK(hipMemcpyAsync(out, dDirOut.p, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    checkDeviceErrors();
}

void Operator::blockOpDirectDev(int which, const double* x, int64_t ldx, const int64_t* targets, int64_t nt,
                                double* out, int64_t ldo, hipStream_t s) {
    if (!directCheck("aniso_block_op_direct", true, 0, which, x, "x", ldx, targets, nt, out, ldo)) return;
    ensureDevice();
    checkDeviceErrors();
    constexpr int K = kMaxRhs;
    const int64_t N = geo.N;
    const int nm = 2 * ks - 1, P = (ks + K - 1) / K;
    const auto mix = blockMixes(ks, g, which != 0);
    const double* sig = which != 0 ? dSigmaT.as<double>() : nullptr;
    // the harmonic weights from the mixes, as passMix reads them: row 0 holds hw_b at
    // mode b, the mode-0 weight of output row i is its diagonal weight
    std::vector<double> wts(2 * (size_t)ks);
    for (int b = 0; b < ks; ++b) {
        wts[b] = mix[((size_t)b * ks + 0) * ks + b];
        wts[ks + b] = mix[((size_t)0 * ks + b) * ks + b];
    }
    const int KO = direct_rows(std::min(ks, 32));
    directBegin(targets, nt, wts, KO);
    // the corrections, chunk by chunk of 8 rows (any ks): input chunk J into output chunk I
    const size_t cb = (size_t)P * K * N * sizeof(double);
    if (dDirCorr.bytes < cb) dDirCorr.alloc(cb);
    HIP_CHECK(hipMemsetAsync(dDirCorr.p, 0, cb, s));
    const std::vector<int> ids = modeIds(nm);
    std::vector<double> sub;
    HarmWeights unused;
    for (int J = 0; J < P; ++J) {
        const int nin = std::min(K, ks - J * K);
        const double* xin = x + (size_t)J * K * ldx;
        int64_t ldi = ldx;
        if (nin < K) {  // the last chunk zero-padded to 8 rows
            if (dDirIn.bytes < (size_t)K * N * sizeof(double)) dDirIn.alloc((size_t)K * N * sizeof(double));
            padRowsIn(dDirIn, 1, nin, K, xin, ldx, s);
            xin = dDirIn.as<double>();
            ldi = N;
        }
        for (int I = 0; I < P; ++I) {
            passMix(I, J, mix, sub, unused);
            if (std::all_of(sub.begin(), sub.end(), [](double v) { return v == 0.0; })) continue;
            directCorr(K, xin, ldi, sig, nm, ids.data(), sub.data(), dDirCorr.as<double>() + (size_t)I * K * N, s);
        }
    }
    // the direct sums: every output row from ONE line integral per pair (windows of up to
    // 32 rows: more than 32 blocks repeat the walk per window)
    for (int i0 = 0; i0 < ks; i0 += KO) {
        DirectArgs a;
        a.nb = ks;
        a.m0 = a.drow0 = a.orow0 = a.crow0 = i0;
        a.nout = std::min(KO, ks - i0);
        a.x = x;
        a.ldx = ldx;
        a.sigT = sig;
        a.hw = dDirW.as<double>();
        a.dw = dDirW.as<double>() + ks + i0;
        a.minuend = which == 2 ? x : nullptr;  // x - mforward(x) (aniso.m:155)
        a.ldm = ldx;
        a.out = out;
        a.ldo = ldo;
        directSweep(KO, a, nt, s);
    }
    HIP_CHECK(hipEventRecord(evDirect, s));
}

void Operator::blockOpDirectHost(int which, const double* u, const int64_t* targets, int64_t nt, double* out) {
    if (!directCheck("aniso_block_op_direct", true, 0, which, u, "u", geo.N, targets, nt, out, nt)) return;
    ensureDevice();
    const int64_t N = geo.N;
    dHostIn.alloc((size_t)ks * N * sizeof(double));
    HIP_CHECK(hipMemcpyAsync(dHostIn.p, u, (size_t)ks * N * sizeof(double), hipMemcpyHostToDevice, own));
    HIP_CHECK(hipEventSynchronize(evDirect));  // dDirOut may still be written
    if (dDirOut.bytes < (size_t)ks * nt * sizeof(double)) dDirOut.alloc((size_t)ks * nt * sizeof(double));
    blockOpDirectDev(which, dHostIn.as<double>(), N, targets, nt, dDirOut.as<double>(), nt, own);
    HIP_CHECK(hipMemcpyAsync(out, dDirOut.p, (size_t)ks * nt * sizeof(double), hipMemcpyDeviceToHost, own));
    HIP_CHECK(hipStreamSynchronize(own));
    checkDeviceErrors();
}

void Operator::setTiming(int level) {
    if (level < 0 || level > 2) throw std::invalid_argument("timing level must be 0, 1 or 2");
    timeStages = level;
    if (level) {
        evUsed = 0;
        spans.clear();
        applies = 0;
        ensureDevice();
        while (evPool.size() < 512) {  // events for ~50 applies created here, not inside a timed region
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            evPool.push_back(e);
        }
    }
}

std::vector<int64_t> Operator::topTrace() {
    sync();
    std::vector<int64_t> out;
    if (!topTraceOn || topTraceBlocks == 0) return out;
    std::vector<int64_t> raw((size_t)topTraceBlocks * 4);
    HIP_CHECK(hipMemcpy(raw.data(), dTopTrace.p, raw.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int ntier = (int)plan.upTierTask.size() - 1;
    const int u1 = plan.upTierTask[1], nUp = plan.upTierTask[ntier] - u1;
    out.reserve((size_t)topTraceBlocks * 8);
    for (int b = 0; b < topTraceBlocks; ++b) {
        out.insert(out.end(), raw.begin() + 4 * b, raw.begin() + 4 * b + 4);
        if (b < nUp) {
            int k = 1;
            while (k + 1 < ntier && b >= plan.upTierTask[k + 1] - u1) ++k;
            out.insert(out.end(), {(int64_t)-k, (int64_t)(k - 1), 0, 0});
        } else {
            const int c = b - nUp, t0 = plan.hmClPtr[c], t1 = plan.hmClPtr[c + 1];
            out.insert(out.end(), {(int64_t)c, (int64_t)plan.hmClWait[c], (int64_t)(t1 - t0),
                                   (int64_t)(plan.hmPtr[t1] - plan.hmPtr[t0])});
        }
    }
    return out;
}

StageTimes Operator::stageTimes() {
    StageTimes r;
    if (applies == 0 || spans.empty()) return r;
    HIP_CHECK(hipEventSynchronize(evPool[spans.back().b]));
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const Span& sp : spans) {
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, evPool[sp.a], evPool[sp.b]));
        acc[sp.stage] += t;
    }
    for (double& a : acc) a /= applies;
    r.exch = (float)acc[0];
    r.up = (float)acc[1];
    r.m2l = (float)acc[2];
    r.gather = (float)acc[3];
    r.near = (float)acc[4];
    r.down = (float)acc[5];
    r.corr = (float)acc[6];
    r.total = (float)acc[7];
    return r;
}

void Operator::lineIntegrals(const double* seg, int n, double* out) {
    if (!coeffSet) throw std::runtime_error("line integrals before setCoeff");
    if (n < 0) throw std::invalid_argument("n must be >= 0");
    if (n == 0) return;
    ensureDevice();
    DevBuf ds, dout;
    ds.upload(seg, (size_t)n * 4 * sizeof(double));
    dout.alloc((size_t)n * sizeof(double));
    launch_line_integrals(n, ds.as<double>(), dStCoef.as<double>(), dParams.as<Params>(), dout.as<double>(), own);
    HIP_CHECK(hipStreamSynchronize(own));
    HIP_CHECK(hipMemcpy(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------- fp32 operator
// (f32op.hip).  The plan is the unsharded tree's: every non-empty
// leaf with its directed U then W sources (bbfmm.h:1081-1099), M2M levels bottom-up
// (bbfmm.h:855-859), every non-empty node's V then X pairs (bbfmm.h:1051-1065), L2L
// levels top-down (bbfmm.h:1070-1071).  The caches are the fp64 mode-0 operators
// (k_cache_m2l / k_cache_near on these directed lists) rounded to fp32.
void Operator::buildMrhsPlan() {
    if (plan.nranks != 1) throw std::logic_error("16-right-hand-side operator on a sharded handle");
    if (mrhsPlanReady) return;
    ensureDevice();
    F32Plan& f = f32;
    f = F32Plan();
    const Tree& t = tree;
    std::vector<int> lv;
    for (int i = 0; i < t.nn; ++i)
        if (t.isLeaf[i] && !t.isEmpty[i]) lv.push_back(i);
    std::sort(lv.begin(), lv.end(), [&](int a, int b) { return t.begin[a] < t.begin[b]; });
    f.nearPtr.push_back(0);
    f.srcPtr.push_back(0);
    for (int n : lv) {
        int64_t S = 0;
        const int64_t s0 = (int64_t)f.srcNodes.size();
        for (int64_t k = t.uPtr[n]; k < t.uPtr[n + 1]; ++k)
            if (!t.isEmpty[t.uIdx[k]]) f.srcNodes.push_back(t.uIdx[k]);
        for (int64_t k = t.wPtr[n]; k < t.wPtr[n + 1]; ++k)
            if (!t.isEmpty[t.wIdx[k]]) f.srcNodes.push_back(t.wIdx[k]);
        for (size_t k = s0; k < f.srcNodes.size(); ++k) {
            const int b = f.srcNodes[k];
            for (int64_t q = 0; q < t.count[b]; ++q) f.nearPts.push_back((int)(t.begin[b] + q));
            S += t.count[b];
        }
        f.maxSrc = std::max<int>(f.maxSrc, (int)(f.srcNodes.size() - s0));
        const int64_t Sp = (S + 15) & ~(int64_t)15;
        for (int64_t q = S; q < Sp; ++q) f.nearPts.push_back((int)t.begin[n]);  // zero columns
        const int nT = (int)t.count[n];
        f.leaves.push_back(n);
        f.leafInfo.push_back({n, (int)t.begin[n], nT, (int)Sp});
        f.srcCount.push_back((int)S);
        f.koff.push_back(f.nearTiles);
        f.koffD.push_back(f.nearD);
        f.nearTiles += (int64_t)((nT + 15) / 16) * (Sp / 16) * 64;
        f.nearD += S * ((nT + 3) & ~3);
        f.nearPtr.push_back((int64_t)f.nearPts.size());
        f.srcPtr.push_back((int64_t)f.srcNodes.size());
    }
    const int D = t.maxLevel;
    f.m2m.assign(std::max(D, 1), {});
    f.l2l.assign(D + 1, {});
    for (int i = 0; i < t.nn; ++i) {
        if (t.isEmpty[i] || t.parent[i] < 0) continue;
        if (!t.isLeaf[i]) f.m2m[t.level[i]].push_back(i);
        if (t.level[i] >= 2) f.l2l[t.level[i]].push_back(i);
        f.m2lTgt.push_back(i);
    }
    f.m2lPtr.push_back(0);
    for (int n : f.m2lTgt) {
        for (int64_t k = t.vPtr[n]; k < t.vPtr[n + 1]; ++k)
            if (!t.isEmpty[t.vIdx[k]]) f.m2lSrc.push_back(t.vIdx[k]);
        for (int64_t k = t.xPtr[n]; k < t.xPtr[n + 1]; ++k)
            if (!t.isEmpty[t.xIdx[k]]) f.m2lSrc.push_back(t.xIdx[k]);
        f.m2lPtr.push_back((int64_t)f.m2lSrc.size());
        for (int64_t p = f.m2lPtr[f.m2lPtr.size() - 2]; p < f.m2lPtr.back(); ++p) f.m2lPairTgt.push_back(n);
    }
    // device lists
    up(d32Leaves, f.leaves);
    std::vector<int4> li(f.leafInfo.size());
    for (size_t i = 0; i < li.size(); ++i)
        li[i] = make_int4(f.leafInfo[i][0], f.leafInfo[i][1], f.leafInfo[i][2], f.leafInfo[i][3]);
    up(d32LeafInfo, li);
    up(d32NearPtr, f.nearPtr);
    up(d32NearPts, f.nearPts);
    up(d32Koff, f.koff);
    up(d32Tgt, f.m2lTgt);
    up(d32Ptr, f.m2lPtr);
    up(d32Src, f.m2lSrc);
    up(d32Level, t.level);
    up(d32PairTgt, f.m2lPairTgt);
    up(d32SrcPtr, f.srcPtr);
    up(d32SrcNodes, f.srcNodes);
    up(d32KoffD, f.koffD);
    up(d32SrcCount, f.srcCount);
    d32LevelNodes.clear();
    d32LevelNodes.resize(f.m2m.size() + f.l2l.size());
    for (size_t l = 0; l < f.m2m.size(); ++l) up(d32LevelNodes[l], f.m2m[l]);
    for (size_t l = 0; l < f.l2l.size(); ++l) up(d32LevelNodes[f.m2m.size() + l], f.l2l[l]);
    // transfer operators in A order: Rup = R_q^T (M2M), Rdn = R_q (L2L); fp32 lane l,
    // element e: k = 4 (l >> 4) + e; fp64: k = (l >> 4) + 4 e (each MFMA's own order)
    std::vector<float> rup(4 * 256), rdn(4 * 256);
    std::vector<double> rup64(4 * 256), rdn64(4 * 256);
    for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 64; ++l)
            for (int e = 0; e < 4; ++e) {
                const int i = l & 15, k = 4 * (l >> 4) + e, k64 = (l >> 4) + 4 * e;
                rup[q * 256 + l * 4 + e] = (float)hostP.R[q][k + i * 16];
                rdn[q * 256 + l * 4 + e] = (float)hostP.R[q][i + k * 16];
                rup64[q * 256 + l * 4 + e] = hostP.R[q][k64 + i * 16];
                rdn64[q * 256 + l * 4 + e] = hostP.R[q][i + k64 * 16];
            }
    up(d32Rup, rup);
    up(d32Rdn, rdn);
    up(d64Rup, rup64);
    up(d64Rdn, rdn64);
    mrhsPlanReady = true;
}

// config 5's fp32 caches: the fp64 mode-0 blocks on the directed lists, rounded
void Operator::buildF32() {
    needResident(0, "the fp32 operator");
    if (!modeCached(0)) throw std::runtime_error("fp32 operator before cache(0)");
    buildMrhsPlan();
    const F32Plan& f = f32;
    const Tree& t = tree;
    d32Mult.alloc((size_t)t.nn * 256 * sizeof(float));
    d32Local.alloc((size_t)t.nn * 256 * sizeof(float));
    d32FT.alloc((size_t)geo.N * 16 * sizeof(float));
    d32CT.alloc((size_t)geo.N * 16 * sizeof(float));
    const Params* P = dParams.as<Params>();
    {
        const int64_t np_ = (int64_t)f.m2lSrc.size();
        DevBuf tmp;
        tmp.alloc((size_t)std::max<int64_t>(np_, 1) * 256 * sizeof(double));
        d32Km2l.alloc((size_t)std::max<int64_t>(np_, 1) * 256 * sizeof(float));
        launch_cache_m2l(np_, d32PairTgt.as<int>(), d32Src.as<int>(), nodeBoxes(), dStCoef.as<double>(), P, 0,
                         tmp.as<double>(), own);
        launch32_conv_m2l(np_, tmp.as<double>(), d32Km2l.p, own);
        HIP_CHECK(hipStreamSynchronize(own));
    }
    {
        DevBuf tmp;
        tmp.alloc((size_t)std::max<int64_t>(f.nearD, 1) * sizeof(double));
        d32Knear.alloc((size_t)std::max<int64_t>(f.nearTiles, 1) * 4 * sizeof(float));
        launch_cache_near((int)f.leaves.size(), d32Leaves.as<int>(), d32SrcPtr.as<int64_t>(), d32SrcNodes.as<int>(),
                          d32KoffD.as<int64_t>(), dBegin.as<int64_t>(), dCount.as<int64_t>(), treePoints(),
                          dStCoef.as<double>(), P, 0, f.maxSrc, tmp.as<double>(), own);
        launch32_conv_near((int)f.leaves.size(), d32LeafInfo.as<int4>(), d32KoffD.as<int64_t>(),
                           d32Koff.as<int64_t>(), d32SrcCount.as<int>(), tmp.as<double>(), d32Knear.p, own);
        HIP_CHECK(hipStreamSynchronize(own));
    }
    f32Ready = true;
}

// the fp64 16-RHS caches of mode id (f64op.hip): the mode's blocks on the directed
// lists, the M2L blocks rearranged in place into A order, the near blocks as tiles
// Built into a local cache, entered into m64 only once every allocation and kernel
// has succeeded: a failed build (out of HBM, a fault) leaves no half-built entry for
// the next call to launch on (ANISO_FAULT_INJECT=mrhs64 makes it throw after its
// allocations, for the test of that path).
size_t Operator::mrhs64Bytes() {
    buildMrhsPlan();
    const F32Plan& f = f32;
    size_t b = (size_t)std::max<int64_t>((int64_t)f.m2lSrc.size(), 1) * 256 * sizeof(double);
    b += (size_t)std::max<int64_t>(f.nearTiles, 1) * 4 * sizeof(double);
    b += (size_t)std::max<int64_t>(f.nearD, 1) * sizeof(double);  // the build's temporary
    if (!d64Mult.p) b += 2 * (size_t)tree.nn * 256 * sizeof(double) + 2 * (size_t)geo.N * 16 * sizeof(double);
    return b;
}

void Operator::buildMrhs64(int id) {
    buildMrhsPlan();
    const F32Plan& f = f32;
    const Params* P = dParams.as<Params>();
    d64Mult.alloc((size_t)tree.nn * 256 * sizeof(double));
    d64Local.alloc((size_t)tree.nn * 256 * sizeof(double));
    d64FT.alloc((size_t)geo.N * 16 * sizeof(double));
    d64CT.alloc((size_t)geo.N * 16 * sizeof(double));
    Mrhs64Cache c;
    const int64_t np_ = (int64_t)f.m2lSrc.size();
    c.Km2l.alloc((size_t)std::max<int64_t>(np_, 1) * 256 * sizeof(double));
    launch_cache_m2l(np_, d32PairTgt.as<int>(), d32Src.as<int>(), nodeBoxes(), dStCoef.as<double>(), P, id,
                     c.Km2l.as<double>(), own);
    launch64_lane_major(np_, c.Km2l.as<double>(), own);
    {
        DevBuf tmp;
        tmp.alloc((size_t)std::max<int64_t>(f.nearD, 1) * sizeof(double));
        c.Knear.alloc((size_t)std::max<int64_t>(f.nearTiles, 1) * 4 * sizeof(double));
        launch_cache_near((int)f.leaves.size(), d32Leaves.as<int>(), d32SrcPtr.as<int64_t>(), d32SrcNodes.as<int>(),
                          d32KoffD.as<int64_t>(), dBegin.as<int64_t>(), dCount.as<int64_t>(), treePoints(),
                          dStCoef.as<double>(), P, id, f.maxSrc, tmp.as<double>(), own);
        launch64_conv_near((int)f.leaves.size(), d32LeafInfo.as<int4>(), d32KoffD.as<int64_t>(),
                           d32Koff.as<int64_t>(), d32SrcCount.as<int>(), tmp.as<double>(), c.Knear.p, own);
        HIP_CHECK(hipStreamSynchronize(own));
    }
    if (const char* e = std::getenv("ANISO_FAULT_INJECT"))
        if (std::string(e) == "mrhs64") throw std::runtime_error("fp64 16-RHS cache build failed (ANISO_FAULT_INJECT)");
    m64.emplace(id, std::move(c));
}

void Operator::mrhs64Dev(int id, bool forward, const double* X, double* Y, hipStream_t s, int mask) {
    refuseHighOrder("the 16-RHS fp64 operator");
    if (plan.nranks != 1) throw std::logic_error("16-right-hand-side operator on a sharded handle");
    if (id < 0 || id >= kernelSize) throw std::out_of_range("kernel id out of range");
    if (forward && id != 0) throw std::invalid_argument("the forward operator is mode 0's (main.cpp:125-136)");
    needResident(id, "the 16-RHS fp64 operator");
    if (!modes[id].resident)
        throw std::runtime_error("16-RHS fp64 operator on kernel id " + std::to_string(id) + " before cache(" +
                                 std::to_string(id) + ")");
    ensureDevice();
    checkDeviceErrors();
    if (!m64.count(id)) buildMrhs64(id);
    const Mrhs64Cache& c = m64.at(id);
    const Params* P = dParams.as<Params>();
    const F32Plan& f = f32;
    const double scale = M_1_PI / 2.0;  // AnisoWrapper.cpp:129-130
    const bool tm = timeStages;
    const int e0 = tm ? mark(s) : -1;
    launch64_p2m((int)f.leaves.size(), d32Leaves.as<int>(), dBegin.as<int64_t>(), dCount.as<int64_t>(),
                 dNcx.as<double>(), dNcy.as<double>(), dNrx.as<double>(), dNry.as<double>(), dPxT.as<double>(),
                 dPyT.as<double>(), X, forward ? dSigmaT.as<double>() : nullptr, dWT.as<double>(), P, d64Mult.p,
                 d64FT.as<double>(), d64CT.as<double>(), s);
    for (int l = (int)f.m2m.size() - 1; l >= 1; --l)
        launch64_m2m((int)f.m2m[l].size(), d32LevelNodes[l].as<int>(), dChild.as<int4>(), dCount.as<int64_t>(),
                     d64Rup.p, d64Mult.p, s);
    const int e1 = tm ? mark(s) : -1;
    if (tm) spans.push_back({1, e0, e1});
    if (mask & kStageFar) {
        launch64_m2l((int)f.m2lTgt.size(), d32Tgt.as<int>(), d32Ptr.as<int64_t>(), d32Src.as<int>(), c.Km2l.p,
                     d64Mult.p, d64Local.p, s);
        const int e2 = tm ? mark(s) : -1;
        if (tm) spans.push_back({2, e1, e2});
        for (size_t l = 2; l < f.l2l.size(); ++l)
            launch64_l2l((int)f.l2l[l].size(), d32LevelNodes[f.m2m.size() + l].as<int>(), dParent.as<int>(),
                         dSlot.as<int>(), d64Rdn.p, d64Local.p, s);
    }
    const int e3 = tm ? mark(s) : -1;
    launch64_leaf((int)f.leaves.size(), d32LeafInfo.as<int4>(), d32NearPtr.as<int64_t>(), d32NearPts.as<int>(),
                  d32Koff.as<int64_t>(), c.Knear.p, d32Level.as<int>(), dNcx.as<double>(), dNcy.as<double>(),
                  dNrx.as<double>(), dNry.as<double>(), dPxT.as<double>(), dPyT.as<double>(), P, d64Local.p,
                  d64FT.as<double>(), X, scale, (mask & kStageAll) | (forward ? kStageForward : 0), Y, s);
    const int e4 = tm ? mark(s) : -1;
    if (tm) spans.push_back({4, e3, e4});
    // corrections: Y -= scale' corr with scale' = scale (forward: X - K x) or -scale (mapping: K x)
    launch64_corr(geo.d, geo.N, dPerm.as<int>(), dIperm.as<int>(), d64CT.as<double>(), d64FT.as<double>(),
                  modes[id].C.as<double>(), modes[id].mu.as<double>(), P, mask, forward ? scale : -scale, Y, s);
    if (tm) {
        const int e5 = mark(s);
        spans.push_back({6, e4, e5});
        spans.push_back({7, e0, e5});
        ++applies;
    }
}

void Operator::forwardF32Dev(const float* X, float* Y, hipStream_t s, int mask) {
    refuseHighOrder("the fp32 operator");
    if (plan.nranks != 1) throw std::logic_error("fp32 operator on a sharded handle");
    if (!f32Ready) buildF32();
    ensureDevice();
    const Params* P = dParams.as<Params>();
    const F32Plan& f = f32;
    const float scale = (float)(M_1_PI / 2.0);  // AnisoWrapper.cpp:129-130
    const bool tm = timeStages;
    const int e0 = tm ? mark(s) : -1;
    launch32_p2m((int)f.leaves.size(), d32Leaves.as<int>(), dBegin.as<int64_t>(), dCount.as<int64_t>(),
                 dNcx.as<double>(), dNcy.as<double>(), dNrx.as<double>(), dNry.as<double>(), dPxT.as<double>(),
                 dPyT.as<double>(), X, dSigmaT.as<double>(), dWT.as<double>(), P, d32Mult.p, d32FT.as<float>(),
                 d32CT.as<float>(), s);
    for (int l = (int)f.m2m.size() - 1; l >= 1; --l)
        launch32_m2m((int)f.m2m[l].size(), d32LevelNodes[l].as<int>(), dChild.as<int4>(), dCount.as<int64_t>(),
                     d32Rup.p, d32Mult.p, s);
    const int e1 = tm ? mark(s) : -1;
    if (tm) spans.push_back({1, e0, e1});
    if (mask & kStageFar) {
        launch32_m2l((int)f.m2lTgt.size(), d32Tgt.as<int>(), d32Ptr.as<int64_t>(), d32Src.as<int>(), d32Km2l.p,
                     d32Mult.p, d32Local.p, s);
        const int e2 = tm ? mark(s) : -1;
        if (tm) spans.push_back({2, e1, e2});
        for (size_t l = 2; l < f.l2l.size(); ++l)
            launch32_l2l((int)f.l2l[l].size(), d32LevelNodes[f.m2m.size() + l].as<int>(), dParent.as<int>(),
                         dSlot.as<int>(), d32Rdn.p, d32Local.p, s);
    }
    const int e3 = tm ? mark(s) : -1;
    launch32_leaf((int)f.leaves.size(), d32LeafInfo.as<int4>(), d32NearPtr.as<int64_t>(), d32NearPts.as<int>(),
                  d32Koff.as<int64_t>(), d32Knear.p, d32Level.as<int>(), dNcx.as<double>(), dNcy.as<double>(),
                  dNrx.as<double>(), dNry.as<double>(), dPxT.as<double>(), dPyT.as<double>(), P, d32Local.p,
                  d32FT.as<float>(), X, scale, mask, Y, s);
    const int e4 = tm ? mark(s) : -1;
    if (tm) spans.push_back({4, e3, e4});
    launch32_corr(geo.d, geo.N, dPerm.as<int>(), dIperm.as<int>(), d32CT.as<float>(), d32FT.as<float>(),
                  modes[0].C.as<double>(), modes[0].mu.as<double>(), P, mask, scale, Y, s);
    if (tm) {
        const int e5 = mark(s);
        spans.push_back({6, e4, e5});
        spans.push_back({7, e0, e5});
        ++applies;
    }
}

// Attach a communicator (every rank together) and build the halo exchange: each rank
// receives, from the owner of each position of its halo (plan.xHalo), that position;
// what it sends to peer p is p's halo inside its own range, so every rank's halo
// ranges are exchanged once (one all-gather of the counts, one of the ranges).
void Operator::commInit(std::unique_ptr<Collectives> c) {
    refuseHighPlain("aniso_comm_init");
    if (hoShard) {
        commInitHigh(std::move(c));
        return;
    }
    if (!c) throw std::invalid_argument("null communicator");
    if (c->nranks != plan.nranks || c->rank != plan.rank)
        throw std::logic_error("communicator rank / size (" + std::to_string(c->rank) + " of " +
                               std::to_string(c->nranks) + ") differ from the handle's shard (" +
                               std::to_string(plan.rank) + " of " + std::to_string(plan.nranks) + ")");
    ensureDevice();
    if (comm && device >= 0) HIP_CHECK(hipDeviceSynchronize());  // collectives in flight on the old one
    comm.reset();
    const int P = c->nranks, me = c->rank;
    DevBuf a, b;
    // every rank's lists (one all-gather of the counts, one of the padded lists); a
    // loopback communicator (development: one rank's schedule on one GPU) has no
    // peers, so their lists come from their plans built here
    struct PeerLists {
        std::vector<double> halo, oneHalo, needNodes, ok, upRec;
    };
    std::vector<PeerLists> peerLists;
    if (c->loopback()) {
        peerLists.resize(P);
        for (int r = 0; r < P; ++r) {
            Plan q;  // the same plan inputs (Plan::build keeps these), rank r's shard
            if (r != me) {
                q.nearSymmetric = plan.nearSymmetric;
                q.maxCanon = plan.maxCanon;
                q.xUpPartialIn = plan.xUpPartialIn;
                q.build(tree, np, r, P);
                q.buildExchange(tree, geo.sz, geo.d2);
            }
            const Plan& src = r == me ? plan : q;
            peerLists[r].halo.assign(src.xHalo.begin(), src.xHalo.end());
            peerLists[r].oneHalo.assign(src.xOneHalo.begin(), src.xOneHalo.end());
            peerLists[r].needNodes.assign(src.xNeedNodes.begin(), src.xNeedNodes.end());
            peerLists[r].ok = {(r == me ? oneExchangeLocal() : src.xOneOk) ? 1.0 : 0.0, src.xUpPartial ? 1.0 : 0.0,
                               cachesReady() ? 1.0 : 0.0};
            peerLists[r].upRec.assign(src.xUpRecNode.begin(), src.xUpRecNode.end());
        }
    }
    auto gatherList = [&](std::vector<double> PeerLists::*field, const std::vector<double>& mineV,
                          std::vector<std::vector<double>>& allV) {
        allV.assign(P, {});
        if (!peerLists.empty()) {
            for (int r = 0; r < P; ++r) allV[r] = peerLists[r].*field;
            return;
        }
        double n = (double)mineV.size();
        a.alloc(sizeof(double));
        b.alloc((size_t)P * sizeof(double));
        HIP_CHECK(hipMemcpy(a.p, &n, sizeof(double), hipMemcpyHostToDevice));
        c->allgather(a.as<double>(), b.as<double>(), 1, own);
        HIP_CHECK(hipStreamSynchronize(own));
        std::vector<double> cnt(P);
        HIP_CHECK(hipMemcpy(cnt.data(), b.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost));
        size_t m = 1;
        for (double x : cnt) m = std::max(m, (size_t)x);
        std::vector<double> pad(m, -1.0);
        std::copy(mineV.begin(), mineV.end(), pad.begin());
        a.alloc(m * sizeof(double));
        b.alloc((size_t)P * m * sizeof(double));
        HIP_CHECK(hipMemcpy(a.p, pad.data(), m * sizeof(double), hipMemcpyHostToDevice));
        c->allgather(a.as<double>(), b.as<double>(), m, own);
        HIP_CHECK(hipStreamSynchronize(own));
        std::vector<double> flat((size_t)P * m);
        HIP_CHECK(hipMemcpy(flat.data(), b.p, flat.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int r = 0; r < P; ++r)
            allV[r].assign(flat.begin() + (size_t)r * m, flat.begin() + (size_t)r * m + (size_t)cnt[r]);
    };
    std::vector<std::vector<double>> haloAll;
    gatherList(&PeerLists::halo, std::vector<double>(plan.xHalo.begin(), plan.xHalo.end()), haloAll);
    const auto cuts = shard_cuts(tree, P);
    if (cuts[me] != plan.ownBegin || cuts[me + 1] != plan.ownEnd) throw std::logic_error("shard cuts disagree with the plan");
    // the rows of one exchange: the blocks, or one chunk of a block operator of more than
    // kMaxRhs blocks (blockOpShardedPasses: every input chunk reuses this layout)
    const int nb = std::min(ks, kMaxRhs);
    auto ranges = [&](int r) {  // rank r's halo ranges
        std::vector<std::pair<int64_t, int64_t>> v;
        for (size_t i = 0; i + 1 < haloAll[r].size(); i += 2) v.push_back({(int64_t)haloAll[r][i], (int64_t)haloAll[r][i + 1]});
        return v;
    };
    auto intersect = [](const std::vector<std::pair<int64_t, int64_t>>& rs, int64_t lo, int64_t hi,
                        std::vector<int64_t>& out) {
        for (const auto& r : rs)
            for (int64_t k = std::max(r.first, lo); k < std::min(r.second, hi); ++k) out.push_back(k);
    };
    std::vector<int64_t> spos, sbase, sstr, rpos, rbase, rstr;
    hxScount.assign(P, 0);
    hxSoff.assign(P, 0);
    hxRcount.assign(P, 0);
    hxRoff.assign(P, 0);
    const auto myHalo = ranges(me);
    for (int p = 0; p < P; ++p) {
        hxSoff[p] = (int64_t)spos.size() * nb;
        hxRoff[p] = (int64_t)rpos.size() * nb;
        if (p == me) continue;
        std::vector<int64_t> sp, rp;
        intersect(ranges(p), plan.ownBegin, plan.ownEnd, sp);  // p's halo inside my range
        intersect(myHalo, cuts[p], cuts[p + 1], rp);           // my halo inside p's range
        for (size_t i = 0; i < sp.size(); ++i) {
            spos.push_back(sp[i]);
            sbase.push_back(hxSoff[p] + (int64_t)i);
            sstr.push_back((int64_t)sp.size());
        }
        for (size_t i = 0; i < rp.size(); ++i) {
            rpos.push_back(rp[i]);
            rbase.push_back(hxRoff[p] + (int64_t)i);
            rstr.push_back((int64_t)rp.size());
        }
        hxScount[p] = (int64_t)sp.size() * nb;
        hxRcount[p] = (int64_t)rp.size() * nb;
    }
    hxNsend = (int64_t)spos.size();
    hxNrecv = (int64_t)rpos.size();
    up(dHxSendPos, spos);
    up(dHxSendBase, sbase);
    up(dHxSendStride, sstr);
    up(dHxRecvPos, rpos);
    up(dHxRecvBase, rbase);
    up(dHxRecvStride, rstr);
    dHxSendBuf.alloc((size_t)std::max<int64_t>(hxNsend * nb, 1) * sizeof(double));
    dHxRecvBuf.alloc((size_t)std::max<int64_t>(hxNrecv * nb, 1) * sizeof(double));
    const int64_t rec = (int64_t)plan.xRootChunk * kRank * rootRhs(nb);
    dXRootsSend.alloc((size_t)std::max<int64_t>(rec, 1) * sizeof(double));
    dXRootsRecv.alloc((size_t)std::max<int64_t>(rec * P, 1) * sizeof(double));
    HIP_CHECK(hipMemset(dXRootsSend.p, 0, dXRootsSend.bytes));
    // ---- the one-collective layout: every rank's needed multipoles (node lists, one
    // all-gather of the counts and one of the lists) and its input ranges (as above)
    oxReady = false;
    std::vector<std::vector<double>> oksAll;
    // every rank's shard- and process-dependent part of the decision (its plan, its
    // staged near field, its knobs): the one-collective form only where all of them
    // hold, so that oxReady, and with it the collectives each matvec issues, is the
    // same on every rank (oneExchangeUsable adds only rank-independent checks)
    // (and whether its plan has the upper multipoles as partial sums: only if every
    // rank's has, since the parts then carry records instead of roots)
    // (and whether it has cached every mode: a sharded matvec on a rank without its
    // caches could only fail on that rank while its peers wait inside the exchange, so
    // comm_init fails on EVERY rank instead, after this gather)
    gatherList(&PeerLists::ok, {oneExchangeLocal() ? 1.0 : 0.0, plan.xUpPartial ? 1.0 : 0.0, cachesReady() ? 1.0 : 0.0},
               oksAll);
    bool allOk = true, allUp = true;
    for (int r = 0; r < P; ++r) {
        const auto& o = oksAll[r];
        if (o.size() < 3 || o[2] < 0.5)
            throw std::logic_error("comm_init: rank " + std::to_string(r) +
                                   " has not cached every mode; every rank caches its modes before comm_init");
        allOk = allOk && o[0] > 0.5;
        allUp = allUp && o[1] > 0.5;
    }
    oxUp = false;
    if (allOk) {  // every rank decides alike: all take part in the same collectives
        std::vector<std::vector<double>> oneAll, nodesAll, upAll;
        gatherList(&PeerLists::oneHalo, std::vector<double>(plan.xOneHalo.begin(), plan.xOneHalo.end()), oneAll);
        gatherList(&PeerLists::needNodes, std::vector<double>(plan.xNeedNodes.begin(), plan.xNeedNodes.end()), nodesAll);
        if (allUp)
            gatherList(&PeerLists::upRec, std::vector<double>(plan.xUpRecNode.begin(), plan.xUpRecNode.end()), upAll);
        const int RK = kRank * rootRhs(nb);
        // the partial-sum records: (node, rank, record, source offset), summed per node in
        // (rank, record) order; this rank's own from its record buffer (~offset)
        struct UpSum {
            int node, rank, j;
            int64_t src;
        };
        std::vector<UpSum> sums;
        const int64_t myRec = allUp ? (int64_t)plan.xUpRecNode.size() * RK : 0;
        if (allUp)
            for (size_t j = 0; j < plan.xUpRecNode.size(); ++j)
                sums.push_back({plan.xUpRecNode[j], me, (int)j, ~((int64_t)j * RK)});
        auto ownerOf = [&](int n) {
            return (int)(std::upper_bound(cuts.begin() + 1, cuts.end() - 1, tree.begin[n]) - (cuts.begin() + 1));
        };
        auto pts = [&](int r, int64_t lo, int64_t hi, std::vector<int64_t>& out) {  // rank r's ranges inside [lo, hi)
            for (size_t i = 0; i + 1 < oneAll[r].size(); i += 2)
                for (int64_t k = std::max((int64_t)oneAll[r][i], lo); k < std::min((int64_t)oneAll[r][i + 1], hi); ++k)
                    out.push_back(k);
        };
        auto nodes = [&](int r, int owner, std::vector<int>& out) {  // rank r's needed nodes owned by `owner`
            for (double v : nodesAll[r])
                if (ownerOf((int)v) == owner) out.push_back((int)v);
        };
        std::vector<int64_t> sp_, sb_, ss_, rp_, rb_, rs_, snb, rnb;
        std::vector<int> sn_, rn_;
        oxScount.assign(P, 0);
        oxSoff.assign(P, 0);
        oxRcount.assign(P, 0);
        oxRoff.assign(P, 0);
        // per peer part: the tier-0 root records (rec doubles, every peer gets this
        // rank's), the input positions (block-major), the multipole rows -- one send
        // and one receive per peer
        std::vector<int64_t> rtS, rtR, rtD;
        int64_t so = 0, ro = 0;
        for (int p = 0; p < P; ++p) {
            oxSoff[p] = so;
            oxRoff[p] = ro;
            if (p == me) continue;
            if (allUp) {  // this rank's records to p; p's records from it
                if (myRec > 0) {
                    rtS.push_back(so);
                    so += myRec;
                }
                for (size_t j = 0; j < upAll[p].size(); ++j)
                    sums.push_back({(int)upAll[p][j], p, (int)j, ro + (int64_t)j * RK});
                ro += (int64_t)upAll[p].size() * RK;
            } else if (rec > 0) {
                rtS.push_back(so);
                rtR.push_back(ro);
                rtD.push_back((int64_t)p * rec);
                so += rec;
                ro += rec;
            }
            std::vector<int64_t> sp, rp;
            std::vector<int> sn, rn;
            pts(p, plan.ownBegin, plan.ownEnd, sp);  // p's positions inside my range
            pts(me, cuts[p], cuts[p + 1], rp);       // mine inside p's range
            nodes(p, me, sn);                        // p's nodes in my subtrees
            nodes(me, p, rn);                        // mine in p's
            for (size_t i = 0; i < sp.size(); ++i) {
                sp_.push_back(sp[i]);
                sb_.push_back(so + (int64_t)i);
                ss_.push_back((int64_t)sp.size());
            }
            for (size_t i = 0; i < rp.size(); ++i) {
                rp_.push_back(rp[i]);
                rb_.push_back(ro + (int64_t)i);
                rs_.push_back((int64_t)rp.size());
            }
            const int64_t sn0 = so + (int64_t)sp.size() * nb, rn0 = ro + (int64_t)rp.size() * nb;
            for (size_t j = 0; j < sn.size(); ++j) {
                sn_.push_back(sn[j]);
                snb.push_back(sn0 + (int64_t)j * RK);
            }
            for (size_t j = 0; j < rn.size(); ++j) {
                rn_.push_back(rn[j]);
                rnb.push_back(rn0 + (int64_t)j * RK);
            }
            so += (int64_t)sp.size() * nb + (int64_t)sn.size() * RK;
            ro += (int64_t)rp.size() * nb + (int64_t)rn.size() * RK;
            oxScount[p] = so - oxSoff[p];
            oxRcount[p] = ro - oxRoff[p];
        }
        if (allUp) {
            std::sort(sums.begin(), sums.end(), [](const UpSum& a, const UpSum& b) {
                return a.node != b.node ? a.node < b.node : a.rank != b.rank ? a.rank < b.rank : a.j < b.j;
            });
            std::vector<int> sNode, sPtr(1, 0);
            std::vector<int64_t> sSrc;
            for (size_t i = 0; i < sums.size(); ++i) {
                if (i == 0 || sums[i].node != sums[i - 1].node) {
                    if (i > 0) sPtr.push_back((int)sSrc.size());
                    sNode.push_back(sums[i].node);
                }
                sSrc.push_back(sums[i].src);
            }
            if (!sums.empty()) sPtr.push_back((int)sSrc.size());
            oxUpSums = (int64_t)sNode.size();
            up(dOxUpSumNode, sNode);
            up(dOxUpSumPtr, sPtr);
            up(dOxUpSumSrc, sSrc);
            dXUpRec.alloc((size_t)std::max<int64_t>(myRec, 1) * sizeof(double));
            oxUp = true;
        }
        oxRootParts = (int64_t)rtS.size();
        up(dOxRootSend, rtS);
        up(dOxRootRecv, rtR);
        up(dOxRootDst, rtD);
        oxNsendPts = (int64_t)sp_.size();
        oxNrecvPts = (int64_t)rp_.size();
        oxNsendNodes = (int64_t)sn_.size();
        oxNrecvNodes = (int64_t)rn_.size();
        if (oxNrecvNodes != (int64_t)plan.xNeedNodes.size())
            throw std::logic_error("one-collective exchange: a needed multipole has no owner");
        up(dOxSendPos, sp_);
        up(dOxSendBase, sb_);
        up(dOxSendStride, ss_);
        up(dOxRecvPos, rp_);
        up(dOxRecvBase, rb_);
        up(dOxRecvStride, rs_);
        up(dOxSendNode, sn_);
        up(dOxSendNodeBase, snb);
        up(dOxRecvNode, rn_);
        up(dOxRecvNodeBase, rnb);
        dOxSendBuf.alloc((size_t)std::max<int64_t>(so, 1) * sizeof(double));
        dOxRecvBuf.alloc((size_t)std::max<int64_t>(ro, 1) * sizeof(double));
        oxReady = true;
    }
    if (c->loopback()) {
        // no peer ever fills the receive buffers: zeros stand in for the peers' data, so a
        // rank's schedule runs on finite values (an iteration on it -- the sharded block
        // solve -- would otherwise spread whatever the allocation held)
        for (DevBuf* b : {&dHxRecvBuf, &dXRootsRecv, &dOxRecvBuf})
            if (b->p) HIP_CHECK(hipMemset(b->p, 0, b->bytes));
    }
    comm = std::move(c);
}

// commInit on a sharded high-order handle: no halo plan -- a matvec gathers
// the whole input, and every rank derives every rank's range from shard_cuts.  ONE small
// all-gather of {N, ks, np, nranks, caches ready} makes the call fail on every rank when the
// ranks' handles disagree or one has not cached its modes (each rank compares every record
// with its own, so a single odd rank fails all of them).  A loopback communicator has no
// peers: their records are taken to be this rank's.
void Operator::commInitHigh(std::unique_ptr<Collectives> c) {
    if (!c) throw std::invalid_argument("null communicator");
    if (c->nranks != plan.nranks || c->rank != plan.rank)
        throw std::logic_error("communicator rank / size (" + std::to_string(c->rank) + " of " +
                               std::to_string(c->nranks) + ") differ from the handle's shard (" +
                               std::to_string(plan.rank) + " of " + std::to_string(plan.nranks) + ")");
    ensureDevice();
    if (comm && device >= 0) HIP_CHECK(hipDeviceSynchronize());  // collectives in flight on the old one
    comm.reset();
    const int P = c->nranks, me = c->rank;
    constexpr int kRec = 5;
    const double mine[kRec] = {(double)geo.N, (double)ks, (double)np, (double)P, cachesReady() ? 1.0 : 0.0};
    std::vector<double> all((size_t)P * kRec);
    if (c->loopback()) {
        for (int r = 0; r < P; ++r) std::copy(mine, mine + kRec, all.begin() + (size_t)r * kRec);
    } else {
        DevBuf a, b;
        a.upload(mine, sizeof(mine));
        b.alloc(all.size() * sizeof(double));
        c->allgather(a.as<double>(), b.as<double>(), kRec, own);
        HIP_CHECK(hipStreamSynchronize(own));
        HIP_CHECK(hipMemcpy(all.data(), b.p, all.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (int r = 0; r < P; ++r) {
        const double* o = all.data() + (size_t)r * kRec;
        if (!std::equal(o, o + 4, mine))
            throw std::logic_error("comm_init: rank " + std::to_string(r) + "'s handle (N, ks, np, nranks = " +
                                   std::to_string((int64_t)o[0]) + ", " + std::to_string((int)o[1]) + ", " +
                                   std::to_string((int)o[2]) + ", " + std::to_string((int)o[3]) + ") differs from rank " +
                                   std::to_string(me) + "'s");
    }
    for (int r = 0; r < P; ++r)  // (after the comparison: every rank names the same first rank)
        if (all[(size_t)r * kRec + 4] < 0.5)
            throw std::logic_error("comm_init: rank " + std::to_string(r) +
                                   " has not cached every mode; every rank caches its modes before comm_init");
    const auto cuts = shard_cuts(tree, P);
    if (cuts[me] != plan.ownBegin || cuts[me + 1] != plan.ownEnd) throw std::logic_error("shard cuts disagree with the plan");
    hgMax = 0;
    for (int r = 0; r < P; ++r) hgMax = std::max(hgMax, cuts[r + 1] - cuts[r]);
    up(dHgCuts, cuts);
    // the parts of the matvec's all-gather: min(ks, 8) rows of hgMax doubles per rank (the
    // padding behind a shorter rank's rows is never unpacked; zeroed once so that a
    // host-staged transport moves finite values)
    const size_t part = (size_t)std::min(ks, kMaxRhs) * (size_t)hgMax;
    dHgSend.alloc(std::max<size_t>(part, 1) * sizeof(double));
    dHgRecv.alloc(std::max<size_t>(part * P, 1) * sizeof(double));
    HIP_CHECK(hipMemset(dHgSend.p, 0, dHgSend.bytes));
    HIP_CHECK(hipMemset(dHgRecv.p, 0, dHgRecv.bytes));
    oxReady = false;
    comm = std::move(c);
}

// The sharded matvec of a high-order handle: pack the own slice of the ks rows, ONE
// all-gather (every part padded to the largest owned count: the same count on every rank,
// which an all-gather needs; the cuts are balanced to within a frontier node, so the
// padding is small unless ranks own nothing), unpack every peer's part into its range of x -- x then holds the whole
// vector -- and the apply on the rank's own lists.  A loopback communicator moves the own
// part only (the caller supplies the rest of x), and it alone is unpacked.  A rank that
// owns nothing takes part in the collective and launches nothing else.
void Operator::blockOpShardedHigh(int which, double* x, int64_t ldx, double* yo, int64_t ldo, hipStream_t s) {
    const int P = plan.nranks, me = plan.rank;
    const int64_t owned = plan.ownEnd - plan.ownBegin;
    const bool tm = timeStages == 1;
    const int e0 = tm ? mark(s) : -1;
    launch_slice_pack(owned, ks, x + plan.ownBegin, ldx, hgMax, dHgSend.as<double>(), s);
    const int e1 = tm ? mark(s) : -1;
    comm->allgather(dHgSend.as<double>(), dHgRecv.as<double>(), (size_t)ks * (size_t)hgMax, s);
    const int e2 = tm ? mark(s) : -1;
    if (comm->loopback()) launch_slice_unpack(me, me + 1, -1, dHgCuts.as<int64_t>(), ks, hgMax, dHgRecv.as<double>(), x, ldx, s);
    else launch_slice_unpack(0, P, me, dHgCuts.as<int64_t>(), ks, hgMax, dHgRecv.as<double>(), x, ldx, s);
    if (tm) {  // stage 0: the pack; stage 3 (the rank-16 M2L gather, unused here): the unpack
        const int e3 = mark(s);
        spans.push_back({0, e0, e1});
        spans.push_back({3, e2, e3});
    }
    if (owned == 0) return;
    ApplyCall call;
    call.hoShard = true;
    blockOp(which, x, ldx, yo, ldo, true, s, NAN, nullptr, call);
}

// Can this sharded matvec take the one-collective exchange?  Its phase 1 must leave
// nothing to the halo: the harmonic block apply with the near field formed from the
// input (run in phase 2, after the exchange) and no padded right-hand sides -- exactly
// applyBlock's `harmonic && nearIn` for this call.  The decision must be the same on
// every rank (the ranks issue matching collectives), so it is split: the part that
// depends on a rank's shard or process (oneExchangeLocal) is all-gathered at commInit
// into oxReady; what is left here depends only on the problem (ks, g, which) and on
// the mode caches, which every rank builds alike before a block matvec.
bool Operator::oneExchangeLocal() const {
    // (more than kMaxRhs blocks: the exchange carries one chunk of kMaxRhs rows)
    if (!plan.xOneOk || !oneXOn || !useAtt || !rhs_supported(std::min(ks, kMaxRhs)) || !nearEarly ||
        !plan.nearCorrOk || plan.nearPartTotal > 0)
        return false;
    const NearCorr probe{dNearCorrRow.as<uint16_t>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return near_hs_fusable((int)plan.leaves.size(), plan.nearMaxLeaf, plan.nsMax, dNearLoc.as<uint16_t>(), &probe,
                           kStageAll);
}

// every mode cached (and the mode-shared caches built, where the handle uses them):
// what a sharded block matvec needs on every rank
bool Operator::cachesReady() const {
    const bool shared = useAtt && attReady;  // a lean handle (cacheBlock) is ready: the block operator reads these
    for (int m = 0; m < kernelSize; ++m)
        if (!modes[m].tables || !(shared || modes[m].resident)) return false;
    return !useAtt || attReady;
}

bool Operator::oneExchangeUsable(int which) {
    if (!oxReady) return false;  // (the mode caches are ready on every rank: prepareShardedMatvec)
    const int nm = 2 * ks - 1;
    const auto mix = blockMixes(ks, g, which != 0);
    HarmWeights hw;
    return harmonicWeights(ks, nm, modeIds(nm).data(), mix.data(), hw);
}

void Operator::blockOpShardedDev(int which, double* x, int64_t ldx, double* y, int64_t ldy, hipStream_t s) {
    refuseHighPlain("aniso_block_op_sharded_dev");
    if (!comm) throw std::logic_error("sharded block operator before aniso_comm_init");
    if (ldx < geo.N || ldy < geo.N) throw std::invalid_argument("sharded block operator: leading dimension below N");
    blockOpShardedOwned(which, x, ldx, y + plan.ownBegin, ldy, s);
}

// the same with the output given as its owned slice: row b of the result starts at
// yo + b * ldo (ldo >= owned).  The public call passes y + own_begin at stride ldy; the
// sharded block solve its compact (ks, owned) vector.
void Operator::blockOpShardedOwned(int which, double* x, int64_t ldx, double* yo, int64_t ldo, hipStream_t s) {
    prepareShardedMatvec(which);
    checkDeviceErrors();
    if (hoShard) {  // one all-gather of the input, then the rank's own targets
        blockOpShardedHigh(which, x, ldx, yo, ldo, s);
        return;
    }
    const bool one = ks > kMaxRhs ? oxReady : oneExchangeUsable(which);
    auto phase = [&](ApplyCall& call, int ph) {
        call.phased(ph, ph == 1 ? dXRootsSend.as<double>() : nullptr, ph == 2 ? dXRootsRecv.as<double>() : nullptr);
        blockOp(which, x, ldx, yo, ldo, true, s, NAN, nullptr, call);
    };
    if (ks > kMaxRhs)  // P input chunks, each with one exchange and P output windows
        blockOpShardedPasses(which, x, ldx, yo, ldo, one, s);
    else
        shardedExchange(
            ks, x, ldx, one, s, [&](ApplyCall& call) { phase(call, 1); }, [&](ApplyCall& call) { phase(call, 2); });
    if (one) {
        ++oneXApplies;
        if (oxUp) ++upPartialApplies;
    }
}

// What a sharded block matvec (blockOpShardedOwned; `which` as blockOpDev's) can refuse,
// or fail to allocate, on one rank alone -- raised here, before its first collective (or,
// for the sharded block solve, before the caller's): the state checks of the matvec and
// every work buffer it sizes on its way.
void Operator::prepareShardedMatvec(int which) {
    if (!comm) throw std::logic_error("sharded block operator before aniso_comm_init");
    if (which < 0 || which > 2) throw std::invalid_argument("block operator: which must be 0, 1 or 2");
    if (!coeffSet) throw std::runtime_error("block operator before setCoeff");
    constexpr int K = kMaxRhs;
    if (hoShard) {  // one apply of ks <= 8 blocks on the high-order launches: no tiers, no passes
        checkBlockLimit(true);
        if (!cachesReady())
            throw std::logic_error("sharded block operator before cache(): every rank caches its modes first");
        ensureDevice();
        const int Kp = ks == 1 ? 2 : rootRhs(ks);
        if (Kp != ks) {
            dPadIn.alloc((size_t)Kp * geo.N * sizeof(double));
            dPadOut.alloc((size_t)Kp * geo.N * sizeof(double));
        }
        if (which == 2 && !(fuseSub && rhs_supported(ks) && ks > 1))
            dBlk.alloc((size_t)ks * (plan.ownEnd - plan.ownBegin) * sizeof(double));
        ensureWork(Kp);
        return;
    }
    if (ks > K && useAtt && !attReady)
        throw std::logic_error("sharded block operator before cache(): every rank caches its modes first");
    if (ks > K && (!useAtt || plan.nearPartTotal != 0))
        throw std::invalid_argument("sharded block operator: ks = " + std::to_string(ks) + " blocks (more than " +
                                    std::to_string(kMaxRhs) + ") run as passes over the mode-shared caches with directed "
                                    "near storage; this handle has " +
                                    (!useAtt ? "no mode-shared caches (ANISO_HARMONIC=0)" : "symmetric near storage"));
    if (!cachesReady())  // (a set_coeff since comm_init: the applies would fail in checkModes, between two collectives)
        throw std::logic_error("sharded block operator before cache(): every rank caches its modes first");
    ensureDevice();
    const int64_t N = geo.N, own = plan.ownEnd - plan.ownBegin;
    const int Kp = ks > K ? K : rootRhs(ks);  // the right-hand sides of one apply
    if (up_tier_lds(plan.upMaxTask, Kp) > 160 * 1024 ||
        down_tier_lds(plan.dnMaxTask, plan.dnMaxLeaves, plan.dnMaxNear, plan.dnMaxChain, Kp) > 160 * 1024)
        throw std::logic_error("up/down pass task exceeds one workgroup's LDS at " + std::to_string(Kp) + " right-hand sides");
    if (ks > K) {
        dPassOut.alloc((size_t)K * N * sizeof(double));
        if (ks % K) dPassIn.alloc((size_t)K * N * sizeof(double));
    } else if (Kp != ks) {
        dPadIn.alloc((size_t)Kp * N * sizeof(double));
        dPadOut.alloc((size_t)Kp * N * sizeof(double));
    }
    // x - mforward(x) where the down pass does not subtract: the operator's value goes to dBlk
    if (which == 2 && !(ks <= K && fuseSub && rhs_supported(ks) && !plan.dnDesc.empty()))
        dBlk.alloc((size_t)ks * own * sizeof(double));
    ensureWork(Kp);
}

// More than kMaxRhs blocks on a shard.  The input chunk J is the
// outer loop: its 8 rows of x (the last chunk zero-padded) take one exchange and one
// up pass, exactly the sharded apply at K = 8 -- the chunk's multipoles then stand in
// dMult and its halo in the input.  Under it every output chunk I runs only what
// depends on the window {8 I, 8 J}: near field + corrections, the per-target M2L and
// the down pass (phase 2 for I = 0, its repeat -- phase 3 -- after it), into the
// (8, owned) scratch that k_add_rows sums into the owned slice of rows 8 I ...  A
// matvec so issues P exchanges, not P^2.  Every rank takes the same route: the form
// is commInit's all-gathered decision (`one` = oxReady), and everything that can fail on one
// rank alone was checked, and every work buffer sized, by prepareShardedMatvec.
void Operator::blockOpShardedPasses(int which, double* x, int64_t ldx, double* yo, int64_t ldy, bool one,
                                    hipStream_t s) {
    constexpr int K = kMaxRhs;
    const int P = (ks + K - 1) / K, nm = 2 * ks - 1;
    const int64_t N = geo.N, own = plan.ownEnd - plan.ownBegin;
    const auto mix = blockMixes(ks, g, which != 0);
    const double* sig = which != 0 ? dSigmaT.as<double>() : nullptr;
    const std::vector<int> ids = modeIds(nm);
    double* acc = yo;
    int64_t lda = ldy;
    if (which == 2) {  // x - mforward(x): the passes sum into dBlk
        acc = dBlk.as<double>();
        lda = own;
    }
    struct ClearPending {  // phase 2 of a pass leaves the pending state active for its repeats
        Pending& p;
        ~ClearPending() { p.active = false; }
    } clearPending{pend};
    std::vector<double> sub;
    for (int J = 0; J < P; ++J) {
        const int b0 = J * K, nin = std::min(K, ks - b0);
        // (the last chunk zero-padded: the exchange fills the copy's halo)
        const std::pair<double*, int64_t> in = stagePassInput(x, ldx, b0, s);
        double* const xin = in.first;
        const int64_t ldin = in.second;
        auto pass = [&](ApplyCall& call, int I, int phase) {
            call.phased(phase, phase == 1 ? dXRootsSend.as<double>() : nullptr,
                        phase == 2 ? dXRootsRecv.as<double>() : nullptr);
            call.pass = true;
            call.shardedPass = true;
            call.win = HarmWindow{I * K, b0};
            passMix(I, J, mix, sub, call.hw);
            applyBlock(K, xin, ldin, true, sig, nm, ids.data(), sub.data(), dPassOut.as<double>(), own, true, s,
                       kStageAll, call);
        };
        shardedExchange(
            K, xin, ldin, one, s, [&](ApplyCall& call) { pass(call, 0, 1); },
            [&](ApplyCall& call) {
                // the caller's x has its halo filled for every row
                if (nin < K) padRowsOut(xin, nin, N, x + (size_t)b0 * ldx, ldx, s);
                for (int I = 0; I < P; ++I) {
                    pass(call, I, I == 0 ? 2 : 3);
                    launch_add_rows(own, std::min(K, ks - I * K), dPassOut.as<double>(), own, acc + (size_t)I * K * lda,
                                    lda, J > 0 ? 1 : 0, s);
                }
            });
    }
    if (which == 2) launch_sub_slice(own, ks, x + plan.ownBegin, ldx, dBlk.as<double>(), own, yo, ldy, s);
}

void Operator::shardedExchange(int nb, double* x, int64_t ldx, bool one, hipStream_t s,
                               const PhaseFn& phase1, const PhaseFn& phase2) {
    const int64_t rec = (int64_t)plan.xRootChunk * kRank * rootRhs(nb);
    ApplyCall call;
    if (one) {
        // phase 1 (own tier-0 subtrees), then ONE grouped exchange: the roots to every
        // rank, and from each owner the input positions and multipoles this rank reads;
        // then phase 2 (near field, upper tiers + M2L, down pass)
        ExchangeForm& form = call.exch;
        form.oneX = true;
        form.upPartial = oxUp;
        if (oxUp && oxRootParts > 63) throw std::logic_error("partial-sum records: more than 63 peer parts");
        const int RK = kRank * rootRhs(nb);
        // one pack launch (this rank's roots -- or its partial-sum records -- into
        // every peer's part, the input positions and the multipole rows each peer
        // reads), one all-to-all-v, one unpack launch (the peers' roots into the slot
        // layout and the own roots -- or every upper node's records summed -- the
        // input's halo, the multipoles)
        phase1(call);
        // (built after phase 1, which may size the work buffers, dMult)
        OxArgs pk;
        pk.nRoot = oxRootParts;
        pk.rec = oxUp ? (int64_t)plan.xUpRecNode.size() * RK : rec;
        pk.rootOff = dOxRootSend.as<int64_t>();
        pk.roots = oxUp ? dXUpRec.as<double>() : dXRootsSend.as<double>();
        pk.nPts = oxNsendPts;
        pk.nb = nb;
        pk.pos = dOxSendPos.as<int64_t>();
        pk.base = dOxSendBase.as<int64_t>();
        pk.stride = dOxSendStride.as<int64_t>();
        pk.x = x;
        pk.ldx = ldx;
        pk.nNode = oxNsendNodes;
        pk.len = RK;
        pk.node = dOxSendNode.as<int>();
        pk.nodeBase = dOxSendNodeBase.as<int64_t>();
        pk.mult = dMult.as<double>();
        pk.buf = dOxSendBuf.as<double>();
        if (oxUp) {  // the pack launch forms this rank's records (its first workgroups)
            OxArgs pr = pk;
            pr.nRoot = 0;
            launch_ox_pack_up(rootRhs(nb), (int)(plan.xUpTask.size() / Plan::kUpTaskInts), dXUpTask.as<int>(),
                              dMult.as<double>(), dParams.as<Params>(), dXUpRec.as<double>(), (int)oxRootParts,
                              dOxRootSend.as<int64_t>(), pr, s);
        } else {
            launch_ox(pk, true, s);
        }
        comm->alltoallv(dOxSendBuf.as<double>(), oxScount.data(), oxSoff.data(), dOxRecvBuf.as<double>(),
                        oxRcount.data(), oxRoff.data(), s);
        OxArgs uk = pk;
        uk.rootOff = dOxRootRecv.as<int64_t>();
        uk.rootDst = dOxRootDst.as<int64_t>();
        uk.roots = dXRootsRecv.as<double>();
        uk.ownRoots = rec > 0 ? dXRootsSend.as<double>() : nullptr;
        uk.ownDst = (int64_t)plan.rank * rec;
        uk.nPts = oxNrecvPts;
        uk.pos = dOxRecvPos.as<int64_t>();
        uk.base = dOxRecvBase.as<int64_t>();
        uk.stride = dOxRecvStride.as<int64_t>();
        uk.nNode = oxNrecvNodes;
        uk.node = dOxRecvNode.as<int>();
        uk.nodeBase = dOxRecvNodeBase.as<int64_t>();
        uk.buf = dOxRecvBuf.as<double>();
        if (oxUp) {
            uk.nRoot = 0;
            uk.ownRoots = nullptr;
            uk.nSum = oxUpSums;
            uk.sumNode = dOxUpSumNode.as<int>();
            uk.sumPtr = dOxUpSumPtr.as<int>();
            uk.sumSrc = dOxUpSumSrc.as<int64_t>();
            uk.ownRec = dXUpRec.as<double>();
        }
        launch_ox(uk, false, s);
        phase2(call);
        return;
    }
    // the input's halo from its owners
    launch_halo_pack(hxNsend, nb, dHxSendPos.as<int64_t>(), dHxSendBase.as<int64_t>(), dHxSendStride.as<int64_t>(),
                     x, ldx, dHxSendBuf.as<double>(), s);
    comm->alltoallv(dHxSendBuf.as<double>(), hxScount.data(), hxSoff.data(), dHxRecvBuf.as<double>(),
                    hxRcount.data(), hxRoff.data(), s);
    launch_halo_unpack(hxNrecv, nb, dHxRecvPos.as<int64_t>(), dHxRecvBase.as<int64_t>(), dHxRecvStride.as<int64_t>(),
                       dHxRecvBuf.as<double>(), x, ldx, s);
    // phase 1, the tier-0 root all-gather, phase 2 (the owned slice of y)
    phase1(call);
    if (rec > 0) comm->allgather(dXRootsSend.as<double>(), dXRootsRecv.as<double>(), (size_t)rec, s);
    phase2(call);
}

void Operator::checkDeviceErrors() {
    if (!topErr || ownTimeline) return;
    if (*(volatile unsigned*)topErr == 0) return;
    *(volatile unsigned*)topErr = 0;
    throw std::runtime_error(
        "hand-off time-out in the fused top-of-tree M2L launch (k_top_m2l_hc): a cluster gave up waiting for the "
        "upper up tiers, so the output of an apply enqueued earlier on this handle is invalid");
}

bool Operator::recoverTopTimeout(hipStream_t s) {
    if (!topErr || *(volatile unsigned*)topErr == 0) return false;
    HIP_CHECK(hipStreamSynchronize(s));  // every launch that could still raise it has finished
    *(volatile unsigned*)topErr = 0;
    forceUnfused = true;
    ++topRecoveries;
    return true;
}

int64_t Operator::topSteals() {
    if (device < 0 || !dTopSteals.p) return 0;
    HIP_CHECK(hipSetDevice(device));
    unsigned v = 0;
    HIP_CHECK(hipMemcpy(&v, dTopSteals.p, sizeof(unsigned), hipMemcpyDeviceToHost));
    return v;
}

void Operator::sync() {
    if (device < 0) return;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipDeviceSynchronize());
    checkDeviceErrors();
}

// The two phases of a sharded apply must come from the same public call: an _end
// that does not repeat its _begin (another operation, block-operator kind, vectors,
// strides or coefficients) would run on the other call's weighted charges.
void Operator::pendingCall(int phase, const PendingCall& c) {
    if (phase == 1) {
        pendCall = c;
    } else if (phase == 2) {
        if (!pend.active || !(pendCall == c))
            throw std::logic_error("sharded apply: end does not match the pending begin (operation, which, x, out, "
                                   "strides and coefficients must repeat)");
    }
}

void Operator::permuteToTree(const double* orig, double* treeOut, hipStream_t s) {
    ensureDevice();
    launch_permute(geo.N, dPerm.as<int>(), orig, treeOut, s);
}

}  // namespace aniso
