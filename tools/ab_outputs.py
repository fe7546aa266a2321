"""Outputs of two builds of the library on the same block matvecs, compared.

ANISO_LIB selects the build when the package is imported, so each build runs in a process
of its own and saves its outputs; a third call compares the two files:

    ANISO_LIB=<other build> python tools/ab_outputs.py run a.npz
    python tools/ab_outputs.py run b.npz
    python tools/ab_outputs.py compare a.npz b.npz

Every case is block_op_dev(2, ...) in tree order (sharded cases: the owned slices of every
rank), once on a default handle and once after set_deterministic(1).  compare: the
deterministic outputs must be bitwise equal, the default ones (their LDS sums are not
run-to-run reproducible) equal to 1e-13 relative, the tolerance the suite uses between forms.
Cases: small trees with 64-target clusters (halo form), 2 / 3 / 5 / 8 blocks at 256 x 256,
the two-phase rank schedule and the one-call sharded matvec (ranks as threads) at 3 and 8
ranks, and the 1M-point matvec (--no-large skips it)."""
import os
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def coeffs(xy, seed):
    rng = np.random.default_rng(seed)
    ss = rng.uniform(0.5, 6.0, xy.shape[0])
    return ss, ss + rng.uniform(0.1, 2.0, xy.shape[0])


def handle(aniso_amd, sz, d, ks, ml, coef=None, shard=None, det=False):
    a = aniso_amd.Aniso(sz, d, ks, 0.8, 10, 4, ml)
    if shard:
        a.set_shard(*shard)
    a.setCoeff(*(coef if coef else coeffs(a.getNodes(), 3)))
    for m in range(2 * ks - 1):
        a.cache(m)
    a.set_deterministic(det)
    return a


def unsharded(torch, aniso_amd, sz, d, ks, ml, det):
    a = handle(aniso_amd, sz, d, ks, ml, det=det)
    X = torch.tensor(np.random.default_rng(sz + ks).uniform(-1, 1, (ks, a.N)), device="cuda")
    out = torch.zeros_like(X)
    a.block_op_dev(2, X, out, tree=True)
    a.sync()
    return out.cpu().numpy()


def two_phase(torch, aniso_amd, sz, ks, world, det):
    """every rank's begin / end around the root all-gather, played by concatenation"""
    coef, X, hs, sends = None, None, [], []
    for r in range(world):
        if coef is None:
            probe = aniso_amd.Aniso(sz, 1, ks, 0.8, 10, 4, 20)
            coef = coeffs(probe.getNodes(), 12)
            X = torch.tensor(np.random.default_rng(world).uniform(-1, 1, (ks, probe.N)), device="cuda")
        sh = handle(aniso_amd, sz, 1, ks, 20, coef, (r, world), det)
        b, e = sh.shard()
        ex = sh.shard_exchange(ks)
        y = torch.zeros(ks, max(e - b, 1), dtype=torch.float64, device="cuda")
        rs = torch.zeros(max(ex["root_chunk"] * ex["root_record"], 1), dtype=torch.float64, device="cuda")
        sh.block_op_begin_dev(2, X, y, rs)
        hs.append((sh, y, b, e))
        sends.append(rs[: ex["root_chunk"] * ex["root_record"]])
    recv = torch.cat(sends) if sends[0].numel() else torch.zeros(1, dtype=torch.float64, device="cuda")
    got = torch.zeros_like(X)
    for sh, y, b, e in hs:
        sh.block_op_end_dev(2, X, y, recv, world)
        got[:, b:e] = y[:, : e - b]
    torch.cuda.synchronize()
    return got.cpu().numpy()


class ThreadCollectives:
    """aniso_collectives between the handles of one process, one thread per rank,
    host-staged through shared slots and a barrier"""

    def __init__(self, aniso_amd, world, rank, shared):
        self.world, self.rank, self.sh, self.lib = world, rank, shared, aniso_amd
        self.struct = aniso_amd.Collectives(None, aniso_amd.COLL_ALLGATHER(self._ag), aniso_amd.COLL_ALLTOALLV(self._a2a),
                                            aniso_amd.COLL_ALLREDUCE(self._ar))

    def _host(self, ptr, n):
        buf = np.empty(int(n), dtype=np.float64)
        if n:
            self.lib.memcpy(buf.ctypes.data, ptr, 8 * int(n))
        return buf

    def _put(self, ptr, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if arr.size:
            self.lib.memcpy(ptr, arr.ctypes.data, 8 * arr.size)

    def _guard(self, fn):
        try:
            fn()
            return 0
        except Exception as ex:  # noqa: BLE001 -- the library turns the status into its error
            self.sh["errors"].append(repr(ex))
            self.sh["bar"].abort()
            return 1

    def _round(self, mine, take):
        def run():
            self.sh["slot"][self.rank] = mine()
            self.sh["bar"].wait()
            take()
            self.sh["bar"].wait()
        return self._guard(run)

    def _ag(self, ctx, send, recv, count, stream):
        return self._round(lambda: self._host(send, count),
                           lambda: self._put(recv, np.concatenate([self.sh["slot"][r] for r in range(self.world)])))

    def _a2a(self, ctx, send, sc, so, recv, rc, ro, stream):
        def take():
            for p in range(self.world):
                if p != self.rank and int(rc[p]):
                    self._put(recv + 8 * int(ro[p]), self.sh["slot"][p][self.rank])
        return self._round(lambda: [self._host(send + 8 * int(so[p]), int(sc[p])) for p in range(self.world)], take)

    def _ar(self, ctx, buf, count, stream):
        return self._round(lambda: self._host(buf, count),
                           lambda: self._put(buf, np.sum([self.sh["slot"][r] for r in range(self.world)], axis=0)))


def native(torch, aniso_amd, sz, ks, world, det):
    """the library's one-call sharded matvec, each rank's input valid at its own range only"""
    probe = aniso_amd.Aniso(sz, 1, ks, 0.8, 10, 4, 20)
    coef = coeffs(probe.getNodes(), 2)
    X = torch.tensor(np.random.default_rng(world).uniform(-1, 1, (ks, probe.N)), device="cuda")
    hs = [handle(aniso_amd, sz, 1, ks, 20, coef, (r, world), det) for r in range(world)]
    shared = dict(bar=threading.Barrier(world, timeout=60), slot=[None] * world, errors=[])
    colls = [ThreadCollectives(aniso_amd, world, r, shared) for r in range(world)]
    outs = [None] * world

    def run(r):
        try:
            h = hs[r]
            h.comm_init_callbacks(colls[r].struct)
            b, e = h.shard()
            x = torch.full_like(X, float("nan"))
            x[:, b:e] = X[:, b:e]
            y = torch.zeros_like(X)
            h.block_op_sharded_dev(2, x, y)
            h.sync()
            outs[r] = y[:, b:e].clone()
        except Exception as ex:  # noqa: BLE001
            shared["errors"].append(repr(ex))
            shared["bar"].abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    if shared["errors"]:
        raise RuntimeError(shared["errors"])
    return torch.cat(outs, dim=1).cpu().numpy()


def run(path, large):
    import torch

    import aniso_amd

    res = {}
    for det in (False, True):
        tag = "det" if det else "default"
        for sz, d, ks, ml, sym in [(32, 1, 5, 20, "1"), (19, 2, 3, 20, "1"), (64, 1, 2, 20, "0"), (40, 1, 5, 3, "1"),
                                   (24, 1, 8, 20, "1")]:
            os.environ.update(ANISO_SYMMETRIC=sym, ANISO_HM_HALO="1", ANISO_HM_CLDEPTH="3")
            res[f"{tag}/halo-{sz}-{d}-{ks}-{ml}-{sym}"] = unsharded(torch, aniso_amd, sz, d, ks, ml, det)
        for k in ("ANISO_SYMMETRIC", "ANISO_HM_HALO", "ANISO_HM_CLDEPTH"):
            del os.environ[k]
        for ks in (2, 3, 5, 8):
            res[f"{tag}/256-ks{ks}"] = unsharded(torch, aniso_amd, 256, 1, ks, 20, det)
        for world in (3, 8):
            res[f"{tag}/two-phase-256-w{world}"] = two_phase(torch, aniso_amd, 256, 5, world, det)
        for sz, world in ((96, 3), (512, 8)):
            res[f"{tag}/native-{sz}-w{world}"] = native(torch, aniso_amd, sz, 5, world, det)
        if large:
            res[f"{tag}/1M-ks5"] = unsharded(torch, aniso_amd, 1024, 1, 5, 20, det)
        print(tag, "done", flush=True)
    np.savez(path, **res)
    print("saved", len(res), "outputs from", aniso_amd.LIB_PATH)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    bad = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        assert np.isfinite(x).all() and np.isfinite(y).all(), k
        rel = float(np.linalg.norm(x - y) / np.linalg.norm(x))
        ok = np.array_equal(x, y) if k.startswith("det/") else rel <= 1e-13
        bad += not ok
        print(f"{'ok  ' if ok else 'FAIL'} {k}: rel {rel:.3e}{' bitwise' if np.array_equal(x, y) else ''}")
    print("all equal" if not bad else f"{bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], "--no-large" not in sys.argv)
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
