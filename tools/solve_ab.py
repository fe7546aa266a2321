"""A/B record of the library's GMRES solves, for changes that must not move a bit: small
cases that cross every branch of the host-side drivers in aniso_amd/csrc/solver.hip (the
zero-guess shortcut, restarts with the explicit residual, a zero right-hand side, the
not-converged return, the sharded solve's collectives, padded groups of the mixed solve,
columns that freeze at different steps in the multi-column solves).

usage: solve_ab.py dump FILE.npz      run the cases, write iters / hist / relres / solutions
       solve_ab.py compare A.npz B.npz   per case: is every array np.array_equal

ANISO_LIB selects the library build a dump runs on (default: the tree's).  A case that the
default handle does not reproduce bit for bit between two dumps of one build (the np = 4
clustered apply sums with floating-point atomics) has a twin "<case>.det" on a handle with
set_deterministic(True) where the handle accepts it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

G = 0.8


def main_coeffs(xy):  # main.cpp:34-40
    ss = 16 * 0.5 * (1 - np.cos(2 * np.pi * xy[:, 0]))
    return ss, ss + 0.2


def block_cases(out, torch, aniso_amd, det):
    """block_solve_dev: sz 32, d 1, ks 5, np 4, every mode cached."""
    a = aniso_amd.Aniso(32, 1, 5, G, 10, 4, 20)
    a.setCoeff(*main_coeffs(a.getNodes()))
    for m in range(9):
        a.cache(m)
    if det:
        a.set_deterministic(True)
    rng = np.random.default_rng(5)
    rhs = torch.tensor(rng.uniform(-1, 1, (5, a.N)), device="cuda")
    guess = torch.tensor(0.1 * rng.uniform(-1, 1, (5, a.N)), device="cuda")
    zero = torch.zeros_like(rhs)
    cases = {
        "block.one_cycle_zero_guess": (rhs, zero, dict(restart=400, tol=1e-11, maxit=3)),
        "block.restart8_guess": (rhs, guess, dict(restart=8, tol=1e-11, maxit=60)),
        "block.zero_rhs": (zero, guess, dict(restart=8, tol=1e-11, maxit=3)),
        "block.maxit1_not_converged": (rhs, zero, dict(restart=8, tol=1e-300, maxit=1)),
    }
    for name, (b, x0, kw) in cases.items():
        x = x0.clone()
        its, hist, rel = a.block_solve_dev(b, x, **kw)
        torch.cuda.synchronize()
        rec(out, name + (".det" if det else ""), iters=its, hist=hist, relres=rel, x=x.cpu().numpy())


def sharded_cases(out, torch, det):
    """block_solve_sharded_dev: sz 32, ks 5, two thread-ranks, restart 8 and 60."""
    from test_gpu_sharded_solve import _Ranks, _tree_rhs
    from test_gpu_sharded_passes import _handle

    full = _handle(32, 1, 5, 20, None)
    ranks = _Ranks(32, 5, 2, full.coef)
    if det:
        try:
            for h in ranks.hs:
                h.set_deterministic(True)
        except Exception as ex:  # noqa: BLE001 -- a handle that does not accept it has no twin
            print("sharded .det cases left out:", ex)
            return
    B = torch.tensor(_tree_rhs(full.N, 5, 3), device="cuda")
    for restart in (8, 60):
        res = ranks.solve(B, restart=restart, tol=1e-11, maxit=40)
        for r, runs in enumerate(res):
            one = runs[0]
            rec(out, f"sharded.restart{restart}.rank{r}" + (".det" if det else ""), iters=one["iters"],
                hist=one["hist"], relres=one["relres"], x=one["x"].cpu().numpy(), collectives=np.array(one["calls"]))


def mixed_cases(out, torch, aniso_amd):
    """solve_mixed_dev: sz 32, m 8 (the inner cycles restart), 3 rows and 17 (a padded second group)."""
    a = aniso_amd.Aniso(32, 1, 1, G, 10, 4, 20)
    a.setCoeff(*main_coeffs(a.getNodes()))
    a.cache(0)
    rng = np.random.default_rng(7)
    for nrhs in (3, 17):
        B = torch.tensor(rng.uniform(-1, 1, (nrhs, a.N)), device="cuda")
        X = torch.zeros_like(B)
        outer, inner, longest, rel = a.solve_mixed_dev(B, X, m=8, tol=1e-12, inner_tol=1e-6)
        torch.cuda.synchronize()
        rec(out, f"mixed.nrhs{nrhs}", outer=outer, inner=inner, longest=longest, relres=rel, x=X.cpu().numpy())


def forward_multi_cases(out, torch, aniso_amd):
    """forward_solve_multi_dev: sz 32 at np 4 and 6, 9 columns (a group of 8 and one more), one
    of them zero, of different difficulty, two with a guess; restart 6."""
    for np_ in (4, 6):
        a = aniso_amd.Aniso(32, 1, 3, G, 10, np_, 20)
        xy = a.getNodes()
        a.setCoeff(*main_coeffs(xy))
        a.cache_block()
        rng = np.random.default_rng(11)
        x, y = xy[:, 0], xy[:, 1]
        Q = np.array([np.exp(-25 * ((x - 0.5) ** 2 + (y - 0.5) ** 2)), rng.uniform(-1, 1, a.N),
                      np.exp(-200.0 * ((x - 0.2) ** 2 + (y - 0.7) ** 2)), np.ones(a.N),
                      1e-3 * rng.uniform(-1, 1, a.N), (x > 0.5).astype(np.float64), np.zeros(a.N),
                      rng.uniform(-1, 1, a.N), x * y])
        X0 = np.zeros_like(Q)
        X0[1] = 0.1 * rng.uniform(-1, 1, a.N)
        X0[6] = 0.1 * rng.uniform(-1, 1, a.N)  # the zero column: its solution is set to 0
        for src in (True, False):
            X = torch.tensor(X0, device="cuda")
            its, rel, hist = a.forward_solve_multi_dev(torch.tensor(Q, device="cuda"), X, restart=6, tol=1e-12,
                                                       maxit=40, rhs_is_source=src)
            torch.cuda.synchronize()
            rec(out, f"forward_multi.np{np_}.{'source' if src else 'rhs'}", iters=its, relres=rel, hist=hist,
                x=X.cpu().numpy(), calls=a.forward_solve_calls())


def block_multi_cases(out, torch, aniso_amd):
    """block_solve_multi_dev: sz 32, ks 3, np 6, 5 sources (a group of 4 and one more), restart 6."""
    a = aniso_amd.Aniso(32, 1, 3, G, 10, 6, 20)
    a.setCoeff(*main_coeffs(a.getNodes()))
    a.cache_block()
    rng = np.random.default_rng(13)
    Q = rng.uniform(-1, 1, (5, 3, a.N))
    Q[3] *= 1e-3
    Q[1, 1:] = 0.0
    for charge in (True, False):
        X = torch.zeros(15, a.N, dtype=torch.float64, device="cuda")
        its, rel, hist = a.block_solve_multi_dev(torch.tensor(Q.reshape(15, a.N), device="cuda"), X, restart=6,
                                                 tol=1e-11, maxit=40, rhs_is_charge=charge)
        torch.cuda.synchronize()
        rec(out, f"block_multi.{'charge' if charge else 'rhs'}", iters=its, relres=rel, hist=hist,
            x=X.cpu().numpy(), calls=a.forward_solve_calls())


def rec(out, case, **arrays):
    for k, v in arrays.items():
        out[f"{case}/{k}"] = np.asarray(v)
    it = np.atleast_1d(arrays.get("iters", arrays.get("inner")))
    print(f"{case}: steps {it.tolist()}", flush=True)


def dump(path):
    import torch

    import aniso_amd

    assert torch.cuda.is_available(), "dump needs the GPU"
    print("library:", aniso_amd.LIB_PATH, flush=True)
    out = {}
    for det in (False, True):
        block_cases(out, torch, aniso_amd, det)
        sharded_cases(out, torch, det)
    mixed_cases(out, torch, aniso_amd)
    forward_multi_cases(out, torch, aniso_amd)
    block_multi_cases(out, torch, aniso_amd)
    np.savez(path, **out)
    print(f"wrote {len(out)} arrays to {path}")


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    cases = sorted({k.split("/")[0] for k in list(A.keys()) + list(B.keys())})
    same = 0
    for c in cases:
        notes = []
        for k in sorted(k for k in set(A.keys()) | set(B.keys()) if k.split("/")[0] == c):
            name = k.split("/")[1]
            if k not in A or k not in B:
                notes.append(f"{name}: only in one file")
                continue
            a, b = A[k], B[k]
            if a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)):
                continue
            if a.shape == b.shape and a.dtype.kind == "f":
                d = float(np.max(np.abs(a - b)))
                notes.append(f"{name}: max |a - b| = {d:.3e} ({d / max(float(np.max(np.abs(b))), 1e-300):.3e} of max |b|)")
            else:
                notes.append(f"{name}: {a.tolist() if a.size < 20 else a.shape} vs {b.tolist() if b.size < 20 else b.shape}")
        same += not notes
        print(f"{c:44s} {'IDENTICAL' if not notes else 'DIFFERS  ' + '; '.join(notes)}")
    print(f"{same} of {len(cases)} cases bit-identical")
    return 0 if same == len(cases) else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
