// gmres_driver.hpp -- what the restarted-GMRES solves of solver.hip share on the host
// (DESIGN.md §3.17): the mapped status block, the look-ahead rule, the hooks of the
// single-system driver (Operator::gmresRestarted) and the buffers of the lockstep
// multi-column solves (Operator::colsSolveGroup).  No device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>

#include "aniso_op.hpp"

namespace aniso {

[[noreturn]] void throw_hip(hipError_t e, const char* file, int line);
#define HIP_CHECK(x)                                               \
    do {                                                           \
        hipError_t e__ = (x);                                      \
        if (e__ != hipSuccess) throw_hip(e__, __FILE__, __LINE__); \
    } while (0)

// n status doubles in mapped, coherent host memory and a timing-disabled event: the small
// kernels store their status words there (dev), and the host waits for the event recorded
// behind them, not a stream drain, before it reads them (p).
struct StatusBlock {
    double *p = nullptr, *dev = nullptr;
    hipEvent_t ev = nullptr;
    bool owned = true;
    StatusBlock() = default;
    StatusBlock(const StatusBlock&) = delete;
    ~StatusBlock() {
        if (owned && p) (void)hipHostFree(p);
        if (owned && ev) (void)hipEventDestroy(ev);
    }
    void alloc(int n) {
        HIP_CHECK(hipHostMalloc((void**)&p, n * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_CHECK(hipHostGetDevicePointer((void**)&dev, p, 0));
    }
    // a view of words and an event that outlive it (the mixed solve's, kept on the handle)
    void view(double* host, hipEvent_t e) {
        owned = false;
        p = host;
        ev = e;
        HIP_CHECK(hipHostGetDevicePointer((void**)&dev, p, 0));
    }
    void post(hipStream_t s) const { HIP_CHECK(hipEventRecord(ev, s)); }
    void wait() const { HIP_CHECK(hipEventSynchronize(ev)); }
    void sync(hipStream_t s) const { post(s), wait(); }  // nothing enqueued in between
};

// puts a flag back to what it was when the scope ends
struct ScopedFlag {
    bool& f;
    bool v;
    explicit ScopedFlag(bool& flag) : f(flag), v(flag) {}
    ~ScopedFlag() { f = v; }
};

// The look-ahead rule of the Arnoldi loops.  The next step's matvec goes in before the host
// reads this step's status: the GPU runs it while the host decides (wasted once per cycle,
// at the step that converges) -- except where the residual estimate is predicted to reach
// tol at this step: geometric extrapolation of the cycle's last two estimates, 10x margin.
struct LookAhead {
    double last = 0.0, prev = 0.0;
    int n = 0;  // estimates of this cycle
    void clear() { n = 0; }
    void push(double rel) {
        prev = last;
        last = rel;
        ++n;
    }
    bool near(double tol) const {
        if (n >= 2) return last * std::min(1.0, last / prev) <= 10.0 * tol;
        return n == 1 && last <= 10.0 * tol;
    }
};

// One system A x = b for Operator::gmresRestarted: vectors of L doubles (V: m + 1 of them;
// st: the Arnoldi state of arn::Layout(m)) and the four places where the unsharded and the
// sharded block solve differ.  The hooks enqueue on the solve's stream.
struct GmresSystem {
    int64_t L;
    int m;
    double normb;  // |b|, over all ranks
    bool xZero;    // the guess is 0 (A 0 = 0: its residual needs no matvec)
    double *b, *x, *w, *V, *st;
    std::function<void(const double*)> matvec;  // w = A v
    std::function<void()> startCycle;           // |V[0]|^2 reduced, k_arn_begin, the status store
    std::function<void(int)> step;              // Arnoldi step j on w = A V[j], up to the status store
    // after the host has waited for the status.  true: what it waited for ran on an invalid
    // fused launch and was recovered (recoverTopTimeout); a solve that cannot recover throws
    std::function<bool()> spoiled;
    // the relaxed solve: w = A~ v on the reduced-precision operator, taken
    // for the Arnoldi matvec of V[j] iff the latest relative residual estimate the host holds
    // when it enqueues it is <= relax.  None (the sharded and the plain solves): matvec always.
    std::function<void(const double*)> matvecLow = nullptr;
    double relax = 0.0;
};

// One group's buffers of the lockstep multi-column solves (colsSolveGroup) at row length L,
// gmax columns and restart m; X (ownX): the guesses / solutions as compact rows where the
// caller's are not.  hs: per column {estimate, r', steps, -}, then |b|^2 and |x|^2 per column,
// for G columns: the solve's group size (arn::kNarrowCols or arn::kMaxCols), gmax <= G.
struct ColsWork {
    DevBuf V, B, In, W, X, st, part, dNb;
    StatusBlock hs;
    int G = 0;
    // everything before anything is launched; a failure, of `more` (the caller's further
    // allocations) too, is raised as
    //   <head> doubles (<basis> bytes) and <rest> bytes of <tail> could not be allocated: <why>
    void alloc(int64_t L, int group, int gmax, int m, bool ownX, const std::string& head, const char* tail,
               const std::function<void()>& more = nullptr);
};

}  // namespace aniso
