#!/usr/bin/env python3
"""bench.py -- GMRES matvec throughput of the MI355X path at 1M quadrature points.

Workload (BASELINE.json metric "GMRES matvec/s & pair-interactions/s at 1M quad
points"; configs[2] = SURVEY.md §8(d) config 3): the aniso.m / demo.m problem --
sz=1024, d=1, ns=10, np=4, maxLevel=20, ks=5 Fourier blocks (9 modes), g=0.8,
N = 1,048,576 points, sigma_s = 20, sigma_a = 0.2 (demo.m:15-16), the Gaussian
charge in block 0 (demo.m:24-29) -- and its GMRES matvec x - mforward(x)
(aniso.m:138-157, 155): 45 mode-applies of the reference per matvec, computed as
ONE harmonic block apply (one up pass over the 5 blocks, one read
of the mode-shared e^-tau caches for all 9 modes and 5 outputs, the per-mode
correction stencils, one down pass).  A "step" is one block
matvec; steps are chained (v <- A v) with every vector resident in HBM, in tree
order (a fixed relabelling of the unknowns: no permutation gathers on the data
path).  fp64 throughout.  --workload mode0 instead times main.cpp's matvec
u - K_0(sigma_s .* u) (main.cpp:125-136) with main.cpp's coefficients; the block
run also reports that number as `mode0_matvec_per_s` under --full.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) sets up, warms up, times the K
steps and prints the result line: the headline rate, `ms_per_step`, the setup times and
the roofline of the two spans its timed region records.  --dump-outputs DIR then also
writes the last timed step's output, the (blocks, N) fp64 iterate in tree order (N > 1:
the rank's owned slice), as DIR/matvec_out.npy; the inputs are fixed, so two builds run
with the same arguments can be compared entry for entry.  Every other leg below runs
only with --full.

N GPUs (one process per GPU, RCCL over xGMI; `bench.py --gpus N` run bare starts its
N ranks itself under torch.distributed.run, and under a launcher WORLD_SIZE must equal
--gpus): the targets are sharded by FMM subtree (strong scaling: total work fixed).
Each rank forms the multipoles of its own tier-0 subtrees and its partial sums of the
upper tiers, then ONE grouped all-to-all-v per matvec (the library's own exchange,
aniso_block_op_sharded_dev over RCCL) brings it the upper multipoles,
the multipoles below the root level and the input points it reads from each owner;
it then computes its targets into its slice of the next iterate.  Config 4 (one
right-hand side) keeps the two-collective form: a halo all-to-all and the tier-0
root all-gather.

Reported on the same JSON line (all but the roofline only with --full):
  roofline      HBM roofline of the dominant kernel (the clustered M2L with the upper up
                tiers, k_top_m2l_hc, one launch per matvec) and of the near-field sweep,
                timed with HIP events
                on the streams they run on over the timed region;
  cpu_baseline  the CPU oracle (a faithful port of the reference apply, timed with
                the reference's per-use heap traffic repeated) on this host's cores at
                the full workload size (modes 0 and 1);
  rel_err_vs_cpu  GPU vs CPU oracle on those inputs, plus the 45-term block
                composition at sz=256;
  mode0_matvec_per_s, deterministic_matvec_per_s  secondary legs on the same
                operator, measured before the headline leg;
  config2, config4, config5  BASELINE's other configs:
                129,600 points at d = 3 (matvec/s, roofline, rel_err vs the oracle),
                4M points sharded over the run's GPUs (matvec/s, per-rank roofline), the
                16-RHS fp32 mixed-precision solve (seconds, iterations, rel_err vs fp64
                GMRES); config2 and config5 on one GPU only;
  stage_ms      the M2L and near-field spans of the timed region; with --full every
                stage, from 5 more steps after it (stage_pass).
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip table (spec); 6.29 TB/s measured copy
FP64_VALU_PEAK_TF = 78.6  # MI355X fp64 vector (spec): half the 157.3 TF fp32 vector rate of the chip table
FP32_MATRIX_PEAK_TF = 157.3  # MI355X_MICROARCH.md chip table: fp32-input MFMA = the fp32 vector rate
FP64_MATRIX_PEAK_TF = 78.6  # MI355X dense fp64 MFMA (spec; equal to the fp64 vector peak on CDNA4)


def main_coeffs(xy):
    """main.cpp:34-40"""
    x = xy[:, 0]
    ss = 16 * 0.5 * (1 - np.cos(2 * np.pi * x))
    return ss, ss + 0.2


def demo_coeffs(xy):
    """demo.m:15-16 through aniso.m:96-100: sigma_s = 20, sigma_t = sigma_s + 0.2"""
    ss = np.full(xy.shape[0], 20.0)
    return ss, ss + 0.2


def gaussian(xy):
    """main.cpp:29-32 / demo.m:24"""
    return np.exp(-25 * ((xy[:, 0] - 0.5) ** 2 + (xy[:, 1] - 0.5) ** 2))


def ref_pairs(sz, d, ns, s):
    """Reference pair interactions per mode-apply: 2 P_U + 2 P_M + P_rem + P_R + P_S."""
    N = sz * sz * d * d
    p_rem = d ** 4 * (3 * sz - 2) ** 2
    p_r = 16 * d ** 4 * ((3 * sz - 2) ** 2 - sz ** 2)
    p_s = 8 * ns * ns * N
    return 2 * s["near_entries"] + 2 * s["m2l_entries"] + p_rem + p_r + p_s


def ref_bytes(sz, d, ns, s):
    """Reference cached-operator stream per mode-apply: 8 (2P_U + 2P_M + P_R + P_S) + 8 * 6N."""
    N = sz * sz * d * d
    p_r = 16 * d ** 4 * ((3 * sz - 2) ** 2 - sz ** 2)
    return 8 * (2 * s["near_entries"] + 2 * s["m2l_entries"] + p_r + 8 * ns * ns * N) + 8 * 6 * N


def _round_key(path):
    """Profiles are named r<round><letters>_...: r04at comes after r04n (a < b < ... < z <
    aa < ab ...), so order by round, then by the letters' length, then the letters."""
    m = re.match(r"r(\d+)([a-z]*)_", os.path.basename(path))
    return (int(m.group(1)), len(m.group(2)), m.group(2)) if m else (-1, 0, "")


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` (a name prefix with the template arguments that
    pick the kernel family) from the newest committed rocprofv3 PMC summary that holds
    it (profiles/rNN_pmc_summary.json, made by tools/profile_round.sh +
    tools/pmc_summary.py on this same bench command; FETCH_SIZE doubled per the gfx950
    correction).  Among that summary's instantiations of the family, the one the bench
    launched most often -- the shipped variant -- is taken.  Returns (bytes, source,
    kernel name)."""
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json")), key=_round_key)
    for f in reversed(files):
        ks = json.load(open(f))["kernels"]
        hits = [(v.get("launches", 0), n, v) for n, v in ks.items() if n == kernel or n.startswith(kernel)]
        if hits:
            _, name, k = max(hits, key=lambda h: h[0])
            return int(k["traffic_bytes"]), os.path.relpath(f, ROOT), name
    return None, None, None


def mfma_busy(kernel):
    """MFMA pipe busy % of `kernel` from the newest committed counter summary that holds
    it (profiles/rNN*_mfma_summary.json or profiles/rNN*/mfma_summary.json, made by
    tools/f32op_prof.sh / f64op_prof.sh + tools/counter_summary.py:
    SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs))."""
    import glob

    files = glob.glob(os.path.join(ROOT, "profiles", "r*_mfma_summary.json")) + \
        glob.glob(os.path.join(ROOT, "profiles", "r*", "mfma_summary.json"))
    files.sort(key=lambda f: _round_key(os.path.relpath(f, os.path.join(ROOT, "profiles")).replace("/", "_")))
    for f in reversed(files):
        for n, v in json.load(open(f)).items():
            if n.split("<")[0].endswith("::" + kernel) and "mfma_util_pct" in v:
                return round(v["mfma_util_pct"], 2), os.path.relpath(f, ROOT)
    return None, None


def block_ref(o, U, ss, g):
    """aniso.m:138-157 x - mforward(x) composed from oracle mode applies (45 in the
    reference's loop; each distinct (block, mode) product computed once here)."""
    nb = U.shape[0]
    out = np.zeros_like(U)
    memo = {}
    for i in range(-(nb - 1), 1):
        for j in range(-(nb - 1), nb):
            b, m = abs(j), abs(i - j)
            if (b, m) not in memo:
                memo[(b, m)] = o.mapping(U[b] * ss, m)
            out[abs(i)] += (g ** b - g ** nb) / (1 - g ** nb) * memo[(b, m)]
    return U - out


def fwd_roofline(st, times, nb=1):
    """HBM roofline of the per-mode (single-RHS handle) apply's two streams, timed by the
    apply's HIP stage events: the M2L (k_m2l: 2 KB per stored merged block, the multipole
    read and local written per target, the transposed product per canonical pair) and the
    near field (8 B per stored near entry)."""
    m2l_b = 2048.0 * st["stored_m2l"] + 2.0 * 128.0 * nb * st["m2l_targets"] + 128.0 * nb * st["m2l_canon"]
    near_b = 8.0 * st["stored_near"]
    out = {}
    for k, b, ms in (("m2l", m2l_b, times["m2l"]), ("near", near_b, times["near"])):
        gbs = b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        out[k] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "frac": round(gbs / HBM_PEAK_GBS, 4), "kernel_ms": round(ms, 5), "algorithmic_bytes": int(b)}
    return out


def stage_pass(op, step, n=5):
    """Per-stage times of n more steps after a timed region.  The timed region itself
    records only the M2L and near-field spans (aniso_set_timing level 2, the roofline
    kernels' durations); a timer between every stage costs 1.3 % of a block matvec
    (DESIGN.md §4, r04as), so the full stage split comes from this untimed pass."""
    op.set_timing(1)
    for _ in range(n):
        step()
    full = op.stage_times()
    op.set_timing(0)
    return full


def merge_stage_times(roof, full):
    """stage_ms: the M2L and near spans of the timed region, the rest from stage_pass."""
    out = dict(full)
    out["m2l"], out["near"] = roof["m2l"], roof["near"]
    return out


def config2_leg(args, with_cpu):
    """BASELINE configs[1]: sz = 120 (N = 129,600), d = 3, ns = 8,
    maxLevel = 5, mode 0, main.cpp's coefficients; main.cpp's GMRES matvec
    u - K_0(sigma_s .* u) (main.cpp:125-136), chained in tree order on one GPU, with the
    roofline of its M2L and near-field streams; rel_err: one mapping(q, 0) against the
    CPU oracle at the same full size (its cache build is ~20 s of the CPU leg)."""
    import torch

    import aniso_amd

    op = aniso_amd.Aniso(120, 3, 1, args.g, 8, 4, 5)
    xy = op.getNodes()
    ss, st = main_coeffs(xy)
    op.setCoeff(ss, st)
    op.cache(0)
    perm = torch.tensor(op.tree_perm(), device="cuda", dtype=torch.int64)
    x = torch.tensor(gaussian(xy), device="cuda")[perm]
    y = torch.zeros_like(x)
    for _ in range(3):
        op.forward_tree_dev(x, y)
        x, y = y, x
    op.set_timing(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        op.forward_tree_dev(x, y)
        x, y = y, x
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    times = merge_stage_times(op.stage_times(), stage_pass(op, lambda: op.forward_tree_dev(x, y)))
    stats = op.stats()
    leg = {"workload": "configs[1]: sz=120 (N=129600), d=3, ns=8, np=4, maxLevel=5 (bbfmm depth 5), mode 0: main.cpp "
                       "GMRES matvec u - K_0(sigma_s .* u), main.cpp coefficients, chained, tree order",
           "N": op.N, "matvec_per_s": round(args.steps / el, 3), "ms_per_step": round(1e3 * el / args.steps, 4),
           "steps": args.steps, "stage_ms": {k: round(v, 5) for k, v in times.items()},
           "roofline": fwd_roofline(stats, times), "rel_err_vs_cpu": None}
    if with_cpu:
        from oracle.oracle_py import Oracle

        o = Oracle(120, 3, 1, args.g, 8, 4, 5)
        o.setCoeff(ss, st)
        o.cache(0)
        q = gaussian(xy) * ss + np.random.default_rng(7).uniform(-0.1, 0.1, op.N)
        ref = o.mapping(q, 0)
        o.close()
        got = op.mapping(q, 0)
        leg["rel_err_vs_cpu"] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    op.close()
    return leg


def config5_leg(args):
    """BASELINE configs[4]: the configs[2] geometry (N = 1M),
    mode 0, 16 right-hand sides b_k = K_0 q_k (q_k Gaussian bumps centred by
    mt19937_64(seed = k)): aniso_amd.solve.gmres_mixed -- the Krylov basis and inner
    operator in fp32 (16-RHS MFMA operator), fp64 iterative refinement on the fp64 MFMA
    operator to ||r|| / ||b|| <= 1e-12 -- timed after a warm-up solve; rel_err against 16
    fp64 device GMRES(80) solves (main.cpp:121-141, aniso_gmres) of the same systems."""
    import torch

    import aniso_amd
    from aniso_amd.solve import config5_charges, gmres_mixed, rhs_block

    a = aniso_amd.Aniso(args.sz, args.d, 1, args.g, args.ns, 4, args.max_level)
    xy = a.getNodes()
    a.setCoeff(*main_coeffs(xy))
    a.cache(0)
    Q = np.stack([config5_charges(xy, s) for s in range(16)])
    B = rhs_block(a, torch.tensor(Q, device="cuda"))
    gmres_mixed(a, B, tol=1e-12)  # warm-up: builds the fp32 and fp64 16-RHS caches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X, outer, inner, rel = gmres_mixed(a, B, tol=1e-12, m=40, inner_tol=1e-6)
    torch.cuda.synchronize()
    t_mixed = time.perf_counter() - t0
    Xh = X.cpu().numpy()
    # the fp64 reference: aniso_gmres solves A x = K_0 q (it forms rhs = K_0 q itself,
    # main.cpp:123), the same systems as B = K_0 Q above
    errs, its = [], []
    t0 = time.perf_counter()
    for k in range(16):
        it, x, _, _ = a.gmres(Q[k], m=80, maxit=400, tol=1e-12)
        its.append(it)
        errs.append(float(np.linalg.norm(Xh[k] - x) / np.linalg.norm(x)))
    t_ref = time.perf_counter() - t0
    # north_star's "MFMA utilisation on M2L": the two MFMA operators' M2L launches (k32_m2l,
    # k64_m2l: one 16 x 16 x 16 product per directed pair, 2 x 16^3 flops) timed by the
    # operators' HIP stage events over 5 applies each; the MFMA pipe's busy share from
    # the newest committed PMC pass of the same kernels (SQ_VALU_MFMA_BUSY_CYCLES)
    mfma = {}
    pairs = a.stats()["mrhs_m2l_pairs"]
    flops = 2.0 * 16 ** 3 * pairs
    for kern, dt, fn, peak in (("k32_m2l", torch.float32, a.forward_f32_dev, FP32_MATRIX_PEAK_TF),
                               ("k64_m2l", torch.float64, a.forward16_f64_dev, FP64_MATRIX_PEAK_TF)):
        Xm = torch.rand((a.N, 16), dtype=dt, device="cuda")
        Ym = torch.empty_like(Xm)
        fn(Xm, Ym)
        a.set_timing(1)
        for _ in range(5):
            fn(Xm, Ym)
        ms = a.stage_times()["m2l"]
        a.set_timing(0)
        tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        busy, bsrc = mfma_busy(kern)
        # the bound from the counters: the kernel's PMC HBM bytes per launch over its
        # time against HBM peak, beside its flops against the MFMA peak -- the larger
        # fraction of peak is what bounds it
        traffic, tsrc, _ = pmc_traffic(f"aniso::{kern}")
        hbm_gbs = traffic / (ms * 1e-3) / 1e9 if traffic and ms > 0 else None
        hbm_frac = hbm_gbs / HBM_PEAK_GBS if hbm_gbs else None
        bound = ("hbm" if hbm_frac is not None and hbm_frac > tf / peak else "mfma") if hbm_frac is not None else None
        mfma[kern] = {"bound": bound, "achieved": round(tf, 2), "peak": peak,
                      "unit": "TFLOP/s", "frac": round(tf / peak, 4), "kernel_ms": round(ms, 5),
                      "algorithmic_flops": int(flops), "directed_pairs": int(pairs),
                      "mfma_busy_pct": busy, "mfma_busy_source": bsrc,
                      "traffic": traffic, "traffic_source": tsrc,
                      "hbm_GBps_from_traffic": round(hbm_gbs, 1) if hbm_gbs else None,
                      "hbm_frac_from_traffic": round(hbm_frac, 4) if hbm_frac else None}
    leg = {"workload": "configs[4]: configs[2] geometry (N=1048576, d=1, ns=10), mode 0, 16 RHS, fp32 mixed precision: "
                       "fp32 Krylov basis + fp32 16-RHS MFMA inner operator, fp64 refinement on the fp64 MFMA operator",
           "seconds": round(t_mixed, 4), "outer_refinements": outer, "inner_iterations": inner,
           "final_rel_residual_max": float(rel.max()), "rel_err_vs_fp64_gmres_max": max(errs),
           "fp64_gmres_16_solves_s": round(t_ref, 4), "fp64_gmres_iterations": its, "mfma_m2l": mfma}
    a.close()
    return leg


SOCKET_CORES = 64  # physical cores of one socket of the GPU box's CPU (AMD EPYC 9575F)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cgroup_cpu_quota():
    """The job's CPU quota from its cgroup (v2 cpu.max "quota period", or v1
    cfs_quota_us / cfs_period_us): (cpus, raw text), or (None, reason)."""
    try:
        raw = open("/sys/fs/cgroup/cpu.max").read().strip()
        q, p = raw.split()[:2]
        return (None if q == "max" else round(int(q) / int(p), 2)), f"cpu.max={raw}"
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return (None if q < 0 else round(q / p, 2)), f"cfs_quota_us={q} cfs_period_us={p}"
    except (OSError, ValueError):
        return None, "no cgroup cpu quota readable"


def cpu_baseline(args, coeffs, op, block_check):
    """The CPU oracle (oracle/, a faithful port of the reference apply incl. its
    per-apply tree rebuild) timed on this host at the FULL workload size: one mode
    cached at a time (the reference caches all 9: ~190 GB at 1M points), modes 0
    and 1 (an even and an odd mode; every mode streams the same caches), one warm-up
    and --cpu-reps timed applies each in two timing modes on the same caches:
      reference_alloc -- the oracle repeats the reference's per-use heap traffic
        (oracle_set_reference_alloc: Vector load(d^2) + ddot per Duffy point,
        KernelFactory.cpp:847-855; two Vectors per target and neighbour,
        :684-685; the cached block deep-copied per use, bbfmm.h:1053).  On the d = 1
        aniso.m geometry this reproduces the reference's recorded rate (sz = 256:
        2.14 vs 2.19 mode-applies/s at 8 threads, profiles/r03_calibration_refalloc.log),
        so it is the reported baseline;
      port -- the same arithmetic without that heap traffic (5-8x faster than the
        reference's record on d = 1; within 8 % of it on the d = 3 cases).
    One block matvec = ks (2 ks - 1) = 45 mode-applies (aniso.m's loop).  The same
    inputs go through the HIP path (op.mapping, host pointers) for rel_err per mode
    at full size.  block_check(sz) runs the 45-term composition x - mforward(x)
    against the oracle at sz (default 256).
    Returns (baseline dict, {"mode0": err, "mode1": err, "block_sz256": err})."""
    from oracle.oracle_py import Oracle

    block = args.workload == "block"
    ks = args.ks if block else 1
    modes = [0, 1] if block else [0]
    o = Oracle(args.sz, args.d, ks, args.g, args.ns, 4, args.max_level)
    xy = o.getNodes()
    ss, st = coeffs(xy)
    o.setCoeff(ss, st)
    u = gaussian(xy) * ss + np.random.default_rng(3).uniform(-0.1, 0.1, o.N)
    per_mode, port_mode, t_cache, errs, spread = {}, {}, 0.0, {}, {}
    for m in modes:
        t0 = time.time()
        o.cache(m)
        t_cache += time.time() - t0
        o.set_reference_alloc(False)
        ref = o.mapping(u, m)  # warm-up (and the check's reference)
        for alloc, dst in ((False, port_mode), (True, per_mode)):
            o.set_reference_alloc(alloc)
            ts = []
            while len(ts) < args.cpu_reps:
                t1 = time.perf_counter()
                o.mapping(u, m)
                ts.append(time.perf_counter() - t1)
            dst[m] = float(np.median(ts))
            spread[(m, alloc)] = (min(ts), max(ts))
        o.set_reference_alloc(False)
        o.uncache(m)
        got = op.mapping(u, m)
        errs[f"mode{m}"] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    o.close()
    if block:
        errs["block_sz256"] = block_check(args.cpu_check_sz)
    t_apply = float(np.mean(list(per_mode.values())))
    t_port = float(np.mean(list(port_mode.values())))
    per_matvec = ks * (2 * ks - 1) if block else 1  # aniso.m's loop: ks x (2ks-1) mapping calls per mforward
    cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    quota, quota_raw = cgroup_cpu_quota()
    try:
        visible = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        visible = os.cpu_count() or 1
    return {
        "value": 1.0 / (per_matvec * t_apply),
        "unit": "matvec/s",
        "cores": cores,
        "kind": "port",
        "timing_mode": "reference_alloc",
        "cpu_model": cpu_model(),
        "sample": (f"oracle mode-apply at the full workload size N={o.N} (tree rebuilt per apply as in the reference, "
                   f"the reference's per-use heap vectors and block copies repeated), modes {modes} one cached at a "
                   f"time, median of {args.cpu_reps} applies each after a warm-up: "
                   + ", ".join(f"mode {m} {t * 1e3:.0f} ms" for m, t in per_mode.items())
                   + f"; one matvec = {per_matvec} mode-applies (the reference's loop); cache build {t_cache:.1f} s "
                   f"not timed; OMP threads={cores}"),
        # OpenMP threads: OMP_NUM_THREADS as the GPU box sets it for one GPU's job (16: the
        # box's CPU share per GPU; the reference's own runs used one thread per core)
        "thread_policy": (f"OMP_NUM_THREADS={cores} (the job's CPU share on the GPU box, set by the box and left "
                          f"as set: one GPU's job may use 16 CPUs); {visible} CPUs visible to the process, "
                          f"os.cpu_count()={os.cpu_count()}; cgroup quota: {quota_raw}"),
        "cgroup_cpu_quota": quota,
        "mode_apply_s": {str(m): round(t, 4) for m, t in per_mode.items()},
        "mode_apply_spread_s": {f"{m}{'' if a else '_port'}": [round(lo, 4), round(hi, 4)]
                                for (m, a), (lo, hi) in spread.items()},
        "reps_per_mode": args.cpu_reps,
        "port_value": 1.0 / (per_matvec * t_port),
        # SURVEY §8(d) / BASELINE.md name one socket's physical cores (64 on the EPYC
        # 9575F); the box gives one GPU's job 16 CPUs and its OMP_NUM_THREADS is left as
        # set, so the 64-core figure is the measured rate scaled linearly: an upper bound
        # on the reference's rate at 64 threads (its own runs scale sub-linearly)
        "socket_cores": SOCKET_CORES,
        "value_linear_to_socket": 1.0 / (per_matvec * t_apply) * SOCKET_CORES / max(cores, 1),
        "port_mode_apply_s": {str(m): round(t, 4) for m, t in port_mode.items()},
    }, errs


def free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n):
    """`bench.py --gpus N` run bare: N ranks of this same command under
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1); rank 0 prints
    the JSON line.  Returns the launcher's exit code."""
    import subprocess

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL (the box's driver)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)  # 50 x 1.2 ms: the steady state, seconds of run time
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary leg: the mode-0 and deterministic matvecs, the per-stage "
                         "timing pass, GMRES, the block solve, configs 2, 4 and 5, --verify and the CPU baseline "
                         "(their own switches below choose among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output (fp64, tree order) to DIR/matvec_out.npy")
    ap.add_argument("--workload", default="block", choices=["block", "mode0"])
    ap.add_argument("--sz", type=int, default=1024)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--ns", type=int, default=10)
    ap.add_argument("--ks", type=int, default=5)
    ap.add_argument("--g", type=float, default=0.8)
    ap.add_argument("--max-level", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3,
                    help="timed oracle applies per mode and timing mode (after one warm-up)")
    ap.add_argument("--cpu-check-sz", type=int, default=256, help="sz of the 45-term block composition check")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend for N>1 (gloo = CPU-staged rehearsal)")
    ap.add_argument("--same-device", action="store_true",
                    help="all ranks on cuda:0 (rehearse the sharded path on a one-GPU box; use --backend gloo)")
    ap.add_argument("--verify", action="store_true", help="check the sharded matvec against an unsharded operator")
    ap.add_argument("--comm", default="native", choices=["native", "python"],
                    help="N>1 exchange: the library's own (one C call per matvec, RCCL or gloo callbacks) or "
                         "aniso_amd.dist.ShardExchange between the two phases")
    ap.add_argument("--gmres", type=int, default=30,
                    help="steps of the GMRES leg (aniso_amd.solve.gmres_dist over this run's matvec; 0: skip)")
    ap.add_argument("--no-solve", action="store_true", help="skip the one-GPU aniso.m solve (aniso_block_solve)")
    ap.add_argument("--config4-sz", type=int, default=2048,
                    help="secondary leg: BASELINE configs[3] (4M points, mode 0, sharded over the run's GPUs); 0 skips")
    ap.add_argument("--config2", type=int, default=1,
                    help="secondary leg (one GPU): BASELINE configs[1], 129,600 points, d=3, maxLevel 5; 0 skips")
    ap.add_argument("--config5", type=int, default=1,
                    help="secondary leg (one GPU): BASELINE configs[4], 16-RHS fp32 mixed-precision solve; 0 skips")
    args = ap.parse_args()
    if args.verify and not args.full:
        ap.error("--verify is a secondary leg: run it with --full")

    # --gpus N > 1 without a launcher: start N ranks under torch.distributed.run as a
    # child process and exit with its code (before torch or HIP is touched here, so
    # nothing in this process has initialised the GPU); under a launcher the world
    # size must agree with --gpus
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    if world_env is not None and int(world_env) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}", file=sys.stderr)
        sys.exit(2)

    import torch
    import torch.distributed as dist

    import aniso_amd
    from aniso_amd import dist as adist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = 0 if args.same_device else local
    torch.cuda.set_device(dev)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group("gloo")

    block = args.workload == "block"
    ks = args.ks if block else 1
    nb = ks if block else 1
    coeffs = demo_coeffs if block else main_coeffs
    # setup, timed per step: create (geometry, quadtree, interaction
    # lists, the cluster plan), the shard's plan, setCoeff (device upload of the
    # plan and coefficients), cache (every mode's operators and the mode-shared E
    # caches, built on the device), the communicator
    setup = {}
    t0 = time.perf_counter()
    op = aniso_amd.Aniso(args.sz, args.d, ks, args.g, args.ns, 4, args.max_level)
    setup["create"] = time.perf_counter() - t0
    N = op.N
    xy = op.getNodes()
    ss, st = coeffs(xy)
    full_stats = op.stats()
    perm = torch.tensor(op.tree_perm(), device="cuda", dtype=torch.int64)
    if world > 1:
        # sharded apply: own subtrees + halo up pass, one all-gather
        # of the tier-0 root multipoles mid-apply, one halo all-to-all per iterate
        t0 = time.perf_counter()
        op.set_shard(rank, world)
        setup["set_shard"] = time.perf_counter() - t0
        xchg = adist.ShardExchange(op, rank, world, nb, "cuda", args.backend)
        xchg0 = adist.ShardExchange(op, rank, world, 1, "cuda", args.backend) if block else xchg
        ob, oe = xchg.own
    t0 = time.perf_counter()
    op.setCoeff(ss, st)
    torch.cuda.synchronize()
    setup["set_coeff"] = time.perf_counter() - t0
    native = world > 1 and block and args.comm == "native"
    modes = list(range(2 * ks - 1))
    t0 = time.time()
    for m in modes:
        op.cache(m)
    torch.cuda.synchronize()
    t_cache = time.time() - t0
    setup["cache"] = t_cache
    # the library's communicator after the caches: comm_init all-gathers every rank's
    # readiness and fails on every rank if one has not cached
    t0 = time.perf_counter()
    coll = adist.native_comm_init(op, world, args.backend) if native else None  # noqa: F841 (kept alive)
    if native:
        setup["comm_init"] = time.perf_counter() - t0
    setup["total"] = sum(setup.values())
    # GMRES vectors live in tree order (a fixed relabelling of the unknowns): the
    # operator then needs no permutation gathers, and the shards' output slices
    # concatenate to the next iterate.  Block 0 holds the Gaussian (demo.m:27-29).
    v = torch.zeros(nb, N, dtype=torch.float64, device="cuda")
    v[0] = torch.tensor(gaussian(xy), device="cuda")[perm]
    w = torch.zeros_like(v)

    def local_apply(x, y):
        if block:
            op.block_op_dev(2, x, y, tree=True)
        else:
            op.forward_tree_dev(x[0], y[0])

    def matvec(x, y):
        if world == 1:
            local_apply(x, y)
            return
        if native:
            # one library call: x's halo all-to-all, phase 1, the root all-gather, phase 2
            op.block_op_sharded_dev(2, x, y)
            return
        # phase 1 (own + halo up tasks, near field), the root all-gather, phase 2
        # (upper tiers, M2L, down pass into the owned slice of y), the halo of y
        if block:
            yo = y[:, ob:oe]
            op.block_op_begin_dev(2, x, yo, xchg.roots_send)
            xchg.roots_allgather()
            op.block_op_end_dev(2, x, yo, xchg.roots_recv, world)
        else:
            op.forward_tree_begin_dev(x[0], y[0, ob:oe], xchg.roots_send)
            xchg.roots_allgather()
            op.forward_tree_end_dev(x[0], y[0, ob:oe], xchg.roots_recv, world)
        xchg.halo(y)

    def timed(fn, steps, warmup):
        nonlocal v, w
        for _ in range(warmup):
            fn(v, w)
            v, w = w, v
        op.set_timing(2)  # the roofline kernels' spans only (stage_pass: the rest)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn(v, w)
            v, w = w, v
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        el = time.perf_counter() - t0
        roof = op.stage_times()  # per-apply averages over the timed region (HIP events)
        if args.full:
            times = merge_stage_times(roof, stage_pass(op, lambda: fn(v, w)))
        else:
            op.set_timing(0)
            times = {"m2l": roof["m2l"], "near": roof["near"]}
        if world > 1:
            t = torch.tensor([el], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, times

    # the secondary legs (main.cpp's mode-0 operator, the bitwise-deterministic block
    # matvec) run first, so the headline leg below measures the GPU in the steady
    # state a long GMRES solve runs in
    sec = {}
    if block and args.full:
        def mode0(x, y):
            if world == 1:
                op.forward_tree_dev(x[0], y[0])
                return
            op.forward_tree_begin_dev(x[0], y[0, ob:oe], xchg0.roots_send)
            xchg0.roots_allgather()
            op.forward_tree_end_dev(x[0], y[0, ob:oe], xchg0.roots_recv, world)
            xchg0.halo(y[0:1])

        el0, t0s = timed(mode0, args.steps, 2)
        sec["mode0_matvec_per_s"] = round(args.steps / el0, 3)
        sec["mode0_stage_ms"] = {k: round(v_, 5) for k, v_ in t0s.items()}
        op.set_deterministic(True)
        eld, tds = timed(matvec, args.steps, 2)
        op.set_deterministic(False)
        sec["deterministic_matvec_per_s"] = round(args.steps / eld, 3)
        sec["deterministic_stage_ms"] = {k: round(v_, 5) for k, v_ in tds.items()}
    elapsed, times = timed(matvec, args.steps, args.warmup)
    if args.dump_outputs:
        # v is the last timed step's output (stage_pass wrote w only)
        os.makedirs(args.dump_outputs, exist_ok=True)
        last = v if world == 1 else v[:, ob:oe]
        name = "matvec_out.npy" if world == 1 else f"matvec_out_rank{rank}.npy"
        np.save(os.path.join(args.dump_outputs, name), last.cpu().numpy())
    my_stats = op.stats()
    ms = 1e3 * elapsed / args.steps
    value = args.steps / elapsed
    # dominant kernel: the M2L stream, one launch per matvec.
    # Harmonic block apply (k_m2l_hm, §3.9): the mode-shared E block of every
    # directed pair (2 KB) once, plus the multipoles read and the locals written per
    # target node (16 x nb doubles each).  Per-mode stream (k_m2l): the stored merged
    # operators of every mode term, the same per-target bytes per term, one
    # transposed partial (16 x nb doubles) per canonical pair and term.
    # Clustered (k_m2l_hc, §3.10): every stored block is read once for both ends (the
    # halo form; block_reads = the stored blocks).  The algorithmic bytes count every
    # stored block once.
    harmonic = block and my_stats["harmonic"] == 1
    if harmonic and my_stats["hm_clusters"] > 0:
        m2l_bytes = 2048.0 * my_stats["att_m2l_blocks"] + 2.0 * 128.0 * nb * my_stats["m2l_targets"]
        # the upper up tiers ride in the same launch (k_top_m2l_hc, §3.10); their
        # bytes (~1,400 small nodes) are not counted
        kn = "k_top_m2l_hc" if my_stats["top_fused"] else "k_m2l_hc"
        kname, pmc_name = f"{kn}<{nb}>", f"void aniso::{kn}<{nb},"
    elif harmonic:
        m2l_bytes = 2048.0 * my_stats["att_m2l_blocks"] + 2.0 * 128.0 * nb * my_stats["m2l_targets"]
        kname, pmc_name = f"k_m2l_hm<{nb}>", f"void aniso::k_m2l_hm<{nb},"
    else:
        terms = len(modes) if block else 1
        m2l_bytes = terms * (2048.0 * my_stats["stored_m2l"] + 2.0 * 128.0 * nb * my_stats["m2l_targets"]
                             + 128.0 * nb * my_stats["m2l_canon"])
        kname = f"k_m2l<{nb}> ({terms} mode terms)"
        pmc_name = f"void aniso::k_m2l<{nb}, {4 if nb <= 2 else 2}>"
    m2l_ms = times["m2l"]
    achieved = m2l_bytes / (m2l_ms * 1e-3) / 1e9 if m2l_ms > 0 else 0.0
    traffic, tsrc, tkern = (pmc_traffic(pmc_name) if world == 1 and args.sz == 1024 and args.d == 1
                            else (None, None, None))
    roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "kernel": kname,
                "kernel_ms": round(m2l_ms, 5), "algorithmic_bytes": int(m2l_bytes), "traffic_source": tsrc,
                "traffic_kernel": tkern}
    if harmonic:
        # the harmonic M2L is fp64-VALU work per matrix entry: r^2,
        # 1/r, c = dx/r, T_2..T_{K-1}, V = sum_b T_b xw_b, (E/r) V, K output FMAs =
        # 6K flops per directed entry (FMA = 2), 256 entries per directed pair
        flops = 6.0 * nb * 256.0 * my_stats["m2l_pairs"]
        tf = flops / (m2l_ms * 1e-3) / 1e12 if m2l_ms > 0 else 0.0
        roofline["e_block_reads"] = my_stats["hm_block_reads"] if my_stats["hm_clusters"] > 0 else my_stats["m2l_pairs"]
        roofline["compute"] = {"bound": "fp64_valu", "achieved": round(tf, 2), "peak": FP64_VALU_PEAK_TF,
                               "unit": "TFLOP/s", "frac": round(tf / FP64_VALU_PEAK_TF, 4),
                               "algorithmic_flops": int(flops)}
    if harmonic:
        # the near-field sweep (k_near_hm): the directed e^-tau entry of
        # every (target, source) point pair once (8 B each), timed by its own HIP events
        # on the side stream it runs on (overlapped with the M2L)
        near_ms = times["near"]
        # the launch's full algorithmic bytes (verdict r05: the E stream alone left its fused
        # work uncounted): the directed E entries (8 B each); every point's data once
        # (x, y, the nb input charges, sigma_s, the quadrature weight: the source table's
        # and the epilogue's reads); the 16-bit source-row and correction-stencil row
        # indices; sigma_t at each point (the r = 0 diagonal); the nb outputs per target;
        # with the up tail (one GPU), the bottom-tier multipoles it writes (16 x nb doubles
        # per node)
        n_pts = my_stats["N"] if world == 1 else (oe - ob)
        parts = {"E_entries": 8.0 * my_stats["stored_near"],
                 "points_once": 8.0 * (4 + nb) * n_pts,
                 "row_indices": 2.0 * (my_stats["near_loc_entries"] + my_stats["near_corr_rows"]),
                 "sigma_t_diag": 8.0 * n_pts,
                 "outputs": 8.0 * nb * n_pts,
                 "up_tail_multipoles": (8.0 * 16 * nb * my_stats["near_up_nodes"]
                                        if my_stats["near_up_tier"] and world == 1 else 0.0)}
        near_bytes = sum(parts.values())
        near_gbs = near_bytes / (near_ms * 1e-3) / 1e9 if near_ms > 0 else 0.0
        # leaves <= 16 points (this geometry) run k_near_hs (sources staged in LDS)
        nkern = "k_near_hs" if my_stats["max_leaf"] <= 16 else "k_near_hm"
        ntraffic, nsrc, nkname = (pmc_traffic(f"void aniso::{nkern}<{nb},") if world == 1 and args.sz == 1024
                                  and args.d == 1 else (None, None, None))
        roofline["near"] = {"bound": "hbm", "achieved": round(near_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(near_gbs / HBM_PEAK_GBS, 4), "traffic": ntraffic,
                            "traffic_source": nsrc, "traffic_kernel": nkname,
                            "kernel": f"{nkern}<{nb}>", "kernel_ms": round(near_ms, 5),
                            "algorithmic_bytes": int(near_bytes),
                            "algorithmic_bytes_parts": {k: int(v_) for k, v_ in parts.items()},
                            "traffic_over_algorithmic": (round(ntraffic / near_bytes, 3) if ntraffic else None),
                            "overlapped_with": roofline["kernel"] if my_stats.get("near_overlap") else None}
        roofline["m2l_rsqrt"] = "v_rsq_f64 + 1 Newton step (~1e-13 relative per entry); near field 2 steps (full fp64)"
    applies = ks * (2 * ks - 1) if block else 1  # the reference's mapping calls per matvec
    cfg = (f"configs[2] (1M points, d=1, ns=10, np=4, maxLevel=20, g={args.g}): aniso.m GMRES block matvec "
           f"x - mforward(x), {ks} blocks x {2 * ks - 1} modes = {applies} mode-applies per matvec"
           if block else "configs[2] geometry, main.cpp GMRES matvec of mode 0")
    line = {
        "metric": ("GMRES matvec/s at 1M quad points (aniso.m block matvec, g=0.8, 45 mode-applies)" if block
                   else "GMRES matvec/s at 1M quadrature points (main.cpp forwardOperator, mode 0)"),
        "value": round(value, 3),
        "unit": "matvec/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms, 4),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": ("synthetic: demo.m coefficients (sigma_s=20, sigma_a=0.2), Gaussian charge in block 0, chained matvecs"
                 if block else "synthetic: main.cpp coefficient functions and Gaussian source, chained matvecs"),
        "config": {"workload": cfg, "N": N, "sz": args.sz, "d": args.d, "ns": args.ns, "np": 4, "ks": ks,
                   "g": args.g, "maxLevel": args.max_level, "rhs_per_apply": nb,
                   "parallelism": f"fmm-subtree-shard x{world}" if world > 1 else "single-gpu"},
        "mode_applies_per_s": round(value * applies, 1),
        # BASELINE's "pair-interactions/s" as the reference counts them: its per-mode
        # pairs x 45 mode-applies.  The harmonic path never forms them (one
        # mode-shared entry serves all modes), so these two are
        # reference-equivalent rates, not achieved throughput; kernel_entries_per_s is
        # what the kernels evaluate (M2L block reads x 256 + near-field entries)
        "ref_equivalent_pair_interactions_per_s": round(value * applies * ref_pairs(args.sz, args.d, args.ns,
                                                                                    full_stats), 1),
        "ref_equivalent_stream_GBps": round(value * applies * ref_bytes(args.sz, args.d, args.ns, full_stats) / 1e9, 1),
        "kernel_entries_per_s": (round(value * (256.0 * roofline["e_block_reads"] + my_stats["stored_near"]), 1)
                                 if harmonic and world == 1 else None),
        "stage_ms": {k: round(v_, 5) for k, v_ in times.items()},
        "cache_build_s": round(t_cache, 3),
        "setup_s": {k: round(v_, 3) for k, v_ in setup.items()},
        "roofline": roofline,
    }
    one_x = world > 1 and native and op.stats()["one_exchange_applies"] > 0
    if world > 1:
        line["exchange"] = {"root_allgather_bytes_per_rank": 8 * xchg.C * xchg.R,
                            "halo_bytes_received": xchg.halo_bytes(), "backend": args.backend,
                            "comm": ("library (aniso_block_op_sharded_dev: halo all-to-all, phase 1, root all-gather, "
                                     "phase 2 in one call)" if native else "aniso_amd.dist.ShardExchange")}
        if one_x:  # own tier-0 subtrees, then ONE grouped exchange
            o1 = op.shard_exchange_one()
            line["exchange"].update({
                "comm": "library (aniso_block_op_sharded_dev: own tier-0 subtrees, then one grouped send/receive "
                        "of the roots, the multipoles below the root level and the input each rank reads, then "
                        "phase 2)",
                "collectives_per_matvec": 1,
                "halo_bytes_received": 8 * nb * o1["halo_points"] + 8 * xchg.R * o1["need_nodes"],
                "multipoles_received": o1["need_nodes"], "input_points_received": o1["halo_points"]})
    line.update(sec)  # mode-0 operator and deterministic block matvec (measured before the headline leg)
    if args.full and args.gmres > 0 and block:
        # GMRES over this run's (possibly sharded) block matvec: aniso_amd.solve.gmres_dist
        # on the library's DCGS2 Arnoldi (two all-reduces of its inner products per step on
        # N > 1), one cycle of exactly --gmres steps (tol 0) from x0 = 0 (no matvec for its
        # residual); the final explicit residual adds one matvec
        from aniso_amd.solve import gmres_dist

        rhs0 = torch.zeros(nb, N, dtype=torch.float64, device="cuda")
        rhs0[0] = torch.tensor(gaussian(xy), device="cuda")[perm]
        if world == 1:
            gb = rhs0

            def gapply(x, y):
                op.block_op_dev(2, x, y, tree=True)
            gred = None
        else:
            gb = rhs0[:, ob:oe].contiguous()
            gapply = adist.native_block_matvec(op, nb, "cuda") if native else adist.sharded_block_matvec(op, xchg)
            gred = xchg.allreduce
        # warm-up: one cycle of the same length (its Krylov basis allocation is then reused,
        # and the GPU enters the timed cycle busy, not after an idle gap: a cold start ran
        # the first steps' kernels at lower clocks, r06i trace)
        gmres_dist(gapply, gb, restart=args.gmres, tol=0.0, maxit=1, allreduce=gred, kry=op)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        tg = time.perf_counter()
        _, _, grel = gmres_dist(gapply, gb, restart=args.gmres, tol=0.0, maxit=1, allreduce=gred, kry=op)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        gel = time.perf_counter() - tg
        if world > 1:
            t = torch.tensor([gel], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            gel = float(t.item())
        line["gmres"] = {"steps": args.gmres, "steps_per_s": round(args.gmres / gel, 3),
                         "ms_per_step": round(1e3 * gel / args.gmres, 4), "matvecs": args.gmres + 1,
                         "relres_after": grel,
                         "method": "aniso_amd.solve.gmres_dist: restarted GMRES on the library's DCGS2 Arnoldi "
                                   "(aniso_arnoldi_*: two sweeps over the Krylov basis per step, Hessenberg matrix, "
                                   "rotations and residual estimate on the device; 2 all-reduces per step on N > 1), "
                                   "the next matvec enqueued before the host reads the step's estimate; tol 0 so "
                                   "exactly `steps` Arnoldi steps are timed"}
    if args.full and args.config4_sz > 0 and block:
        # BASELINE configs[3]: sz = 2048 (4,194,304 points), d = 1, mode 0 -- main.cpp's GMRES
        # matvec u - K_0(sigma_s .* u), the configuration BASELINE names for 8 GPUs --
        # sharded over this run's ranks like the headline (the library's one-call exchange at
        # N > 1); its per-N rates give the strong scaling of the multi-GPU config
        setup4 = {}
        t0 = time.perf_counter()
        op4 = aniso_amd.Aniso(args.config4_sz, args.d, 1, args.g, args.ns, 4, args.max_level)
        setup4["create"] = time.perf_counter() - t0
        xy4 = op4.getNodes()
        perm4 = torch.tensor(op4.tree_perm(), device="cuda", dtype=torch.int64)
        if world > 1:
            t0 = time.perf_counter()
            op4.set_shard(rank, world)
            setup4["set_shard"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        op4.setCoeff(*main_coeffs(xy4))
        torch.cuda.synchronize()
        setup4["set_coeff"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        op4.cache(0)
        torch.cuda.synchronize()
        setup4["cache"] = time.perf_counter() - t0
        if world > 1:
            t0 = time.perf_counter()
            coll4 = adist.native_comm_init(op4, world, args.backend)  # noqa: F841 (kept alive)
            setup4["comm_init"] = time.perf_counter() - t0
        setup4["total"] = sum(setup4.values())
        x4 = torch.zeros(1, op4.N, dtype=torch.float64, device="cuda")
        x4[0] = torch.tensor(gaussian(xy4), device="cuda")[perm4]
        y4 = torch.zeros_like(x4)

        def step4(a, b):
            if world == 1:
                op4.block_op_dev(2, a, b, tree=True)  # ks = 1: x - K_0(sigma_s x), main.cpp:125-136
            else:
                op4.block_op_sharded_dev(2, a, b)

        for _ in range(2):
            step4(x4, y4)
            x4, y4 = y4, x4
        op4.set_timing(2)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        for _ in range(args.steps):
            step4(x4, y4)
            x4, y4 = y4, x4
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        el4 = time.perf_counter() - t4
        times4 = merge_stage_times(op4.stage_times(), stage_pass(op4, lambda: step4(x4, y4)))
        if world > 1:
            t = torch.tensor([el4], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el4 = float(t.item())
        line["config4"] = {"workload": "configs[3]: sz=2048 (N=4194304), d=1, ns=10, mode 0: main.cpp GMRES matvec "
                                       "u - K_0(sigma_s .* u), sharded by FMM subtree over the run's GPUs",
                           "N": op4.N, "matvec_per_s": round(args.steps / el4, 3),
                           "ms_per_step": round(1e3 * el4 / args.steps, 4), "steps": args.steps,
                           "scaling": "strong", "n_gpus": world,
                           "stage_ms": {k: round(v_, 5) for k, v_ in times4.items()},
                           "setup_s": {k: round(v_, 3) for k, v_ in setup4.items()},
                           # this rank's M2L and near-field streams (its shard's stored blocks)
                           "roofline": fwd_roofline(op4.stats(), times4)}
        del op4
    if args.verify:
        # one matvec of a fixed block vector through this (possibly sharded) path vs
        # an unsharded operator on the same device
        U = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (nb, N)), device="cuda")
        got = torch.zeros_like(U)
        Ut = U[:, perm].contiguous()
        xin = Ut.clone()
        if world > 1:  # the input holds the rank's own range only (NaN elsewhere)
            xin.fill_(float("nan"))
            xin[:, ob:oe] = Ut[:, ob:oe]
            if not native:
                for lo, hi in xchg.halos[rank]:
                    xin[:, lo:hi] = Ut[:, lo:hi]
        matvec(xin, got)  # tree order in and out
        ref_op = aniso_amd.Aniso(args.sz, args.d, ks, args.g, args.ns, 4, args.max_level)
        ref_op.setCoeff(ss, st)
        for m in modes:
            ref_op.cache(m)
        ref = torch.zeros_like(U)
        if block:
            ref_op.block_op_dev(2, U, ref)  # original order, unsharded
        else:
            ref_op.forward_dev(U[0], ref[0])
        torch.cuda.synchronize()
        ref = ref[:, perm]
        b_, e_ = (ob, oe) if world > 1 else (0, N)
        # owned slice of every rank vs the unsharded operator; the halo the exchange filled
        # (native: the input's, from the owners; python: the output's, after the matvec)
        sq = torch.tensor([float(torch.sum((got[:, b_:e_] - ref[:, b_:e_]) ** 2)),
                           float(torch.sum(ref[:, b_:e_] ** 2))], dtype=torch.float64)
        if world > 1:
            ranges = op.shard_one_halo() if one_x else xchg.halos[rank]
            hal = [torch.arange(int(lo), int(hi), device="cuda") for lo, hi in ranges]
            if hal:
                hi_ = torch.cat(hal)
                if native:
                    line["verify_halo_rel_err"] = float(torch.linalg.norm(xin[:, hi_] - Ut[:, hi_])
                                                        / torch.linalg.norm(Ut[:, hi_]))
                else:
                    line["verify_halo_rel_err"] = float(torch.linalg.norm(got[:, hi_] - ref[:, hi_])
                                                        / torch.linalg.norm(ref[:, hi_]))
            sq = sq.to("cuda") if args.backend == "nccl" else sq
            dist.all_reduce(sq)
        line["verify_rel_err_vs_unsharded"] = float((sq[0] / sq[1]) ** 0.5)
        del ref_op
    if args.full and world == 1 and block and not args.no_solve:
        # aniso.m:159-173 as the MATLAB caller runs it: rhs = forward(charge), u = gmres(A,
        # rhs, 400, 1e-11, 400), A(u) = u - mforward(u), through aniso_block_solve_dev
        # (Krylov basis of 401 x 5 x N doubles in HBM; wall time incl. its allocation)
        charge = torch.zeros(nb, N, dtype=torch.float64, device="cuda")
        charge[0] = torch.tensor(gaussian(xy), device="cuda")
        rhs = torch.zeros_like(charge)
        op.block_op_dev(0, charge, rhs)
        u = torch.zeros_like(charge)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        its, shist, srel = op.block_solve_dev(rhs, u, 400, 1e-11, 400)
        sel = time.perf_counter() - ts
        line["block_solve"] = {"call": "gmres(A, rhs, 400, 1e-11, 400), A(u) = u - mforward(u) (aniso.m:159-173)",
                               "iterations": its, "relres": srel, "seconds": round(sel, 4),
                               "ms_per_iteration": round(1e3 * sel / max(abs(its), 1), 4)}
    # BASELINE's one-GPU configs[1] and configs[4] (after the block solve: their handles'
    # allocations would otherwise be recycled into the solve's 16.8 GB Krylov basis)
    if args.full and world == 1 and block and args.config2:
        line["config2"] = config2_leg(args, with_cpu=not args.no_cpu)
    if args.full and world == 1 and block and args.config5:
        line["config5"] = config5_leg(args)
    if args.full and rank == 0 and world == 1 and not args.no_cpu:
        def block_check(sz):
            """x - mforward(x) (aniso.m:155) at sz: HIP harmonic block apply vs the
            oracle's per-mode composition (45 mapping calls in the reference)."""
            from oracle.oracle_py import Oracle

            o = Oracle(sz, args.d, ks, args.g, args.ns, 4, args.max_level)
            a = aniso_amd.Aniso(sz, args.d, ks, args.g, args.ns, 4, args.max_level)
            cs = coeffs(a.getNodes())
            a.setCoeff(*cs)
            o.setCoeff(*cs)
            for m in modes:
                a.cache(m)
                o.cache(m)
            U = np.random.default_rng(0).uniform(-1, 1, (ks, a.N))
            U[0] += gaussian(a.getNodes())
            ref = block_ref(o, U, cs[0], args.g)
            got = a.block_op(2, U)
            o.close()
            a.close()
            return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))

        base, errs = cpu_baseline(args, coeffs, op, block_check)
        line["cpu_baseline"] = base
        line["rel_err_vs_cpu"] = max(errs.values())
        line["rel_err_vs_cpu_detail"] = errs
        line["speedup_vs_cpu"] = round(value / base["value"], 1)
    else:
        line["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
