"""Wall time of tb_model.kpm_eigs / tbk_kpm_eigs and where it goes:

  A  the spinful Kane-Mele flake of 24 x 22 cells (2112 states), window (-0.3, 0.3), n_search = 64, degree = 512;
  B  an open Haldane flake of L x L cells (default 100: 20 000 states), the gap window (-0.35, 0.35), degree = 512, n_search
     doubled from 128 until the subspace is no longer saturated (the tables are built with NumPy and go to tbk_sparse_upload);
  C  the only comparison there is: the dense solve_all(eig_vectors=True) of a Kane-Mele flake of 16 x 32 cells (2048 states, the
     dense limit), every eigenpair, on the same build.

Every call is warmed up once (code objects, workspace) and then timed `--repeat` times with a host clock around the call, which
ends in a device synchronisation; the median and the runs are printed.  One more call of A and B runs with the library's
per-launch event brackets: the share of the kernel time in the filter (kpm_eigs_load, kpm_series_step, kpm_series_guard)
against the subspace kernels (kpm_eigs_hy, kpm_eigs_gram, kpm_eigs_rotate, kpm_eigs_resid, kpm_series_gather), kpm_reduce, which
serves both and is given by itself, and the two dense solves (every other scope).

    python profiles/kpm_eigs_probe.py [--flake 100] [--repeat 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from kpm_probe import _lib, haldane_supercell_tables  # noqa: E402
import helpers as hp  # noqa: E402
import pythtb_amd as tb  # noqa: E402

FILTER = ("kpm_eigs_load", "kpm_series_step", "kpm_series_guard", "kpm_series_const")
SUBSPACE = ("kpm_eigs_hy", "kpm_eigs_gram", "kpm_eigs_rotate", "kpm_eigs_resid", "kpm_series_gather")


def km_flake(nx, ny):
    m = hp.kane_mele(tb.tb_model)
    return hp.quiet(lambda: m.cut_piece(nx, 0, glue_edgs=False).cut_piece(ny, 1, glue_edgs=False))


def open_haldane(ctx, L):
    """the L x L supercell of kpm_probe without the bonds that leave it: dim_k = 0"""
    t = haldane_supercell_tables(L)
    keep = np.all(t["hop_R"] == 0, axis=1)
    n = len(t["orb"])
    orb = np.zeros((n, 0))
    hi, hj, ha = (np.ascontiguousarray(t[key][keep]) for key in ("hop_i", "hop_j", "hop_amp"))
    h = C.c_void_p()
    _lib.check(_lib.lib.tbk_sparse_upload(ctx.handle, 0, n, 1, _lib.dptr(orb), _lib.dptr(t["onsite"].view(float)), len(hi), _lib.iptr(hi),
                                          _lib.iptr(hj), None, _lib.dptr(ha.view(float)), C.byref(h)))
    return h, n


def raw_eigs(sp, n, window, bounds, n_search, degree):
    nf, ev, vec = C.c_int(0), np.zeros(n_search), np.empty((n_search, n), dtype=complex)
    res, info = np.zeros(n_search), np.zeros(4, dtype=np.int32)
    _lib.check(_lib.lib.tbk_kpm_eigs(sp, None, window[0], window[1], bounds[0], bounds[1], n_search, degree, 1e-10, 40, 0, C.byref(nf),
                                     _lib.dptr(ev), _lib.dptr(vec.view(float)), _lib.dptr(res), _lib.iptr(info)))
    return ev[:nf.value], vec[:nf.value], res[:nf.value], info


def timed(call, repeat):
    call()
    runs = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        runs.append(time.perf_counter() - t0)
    return float(np.median(runs)), runs


def shares(ctx, call):
    ctx.prof_enable(1)
    ctx.prof_reset()
    call()
    rep = ctx.prof_report()
    ctx.prof_enable(0)
    ctx.prof_reset()
    ms = {name: v["total_ms"] for name, v in rep.items()}
    filt = sum(ms.get(k, 0.0) for k in FILTER)
    sub = sum(ms.get(k, 0.0) for k in SUBSPACE)
    red = ms.get("kpm_reduce", 0.0)
    total = sum(ms.values())
    return dict(kernel_ms=total, filter_ms=filt, subspace_ms=sub, reduce_ms=red, dense_and_other_ms=total - filt - sub - red,
                scopes={k: dict(ms=v["total_ms"], launches=v["launches"]) for k, v in rep.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flake", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    rows = []

    m = km_flake(24, 22)
    call = lambda: m.kpm_eigs((-0.3, 0.3), n_search=64, degree=512, return_info=True)
    ev, _, info = call()
    med, runs = timed(call, a.repeat)
    rows.append(dict(case="A", nsta=m._nsta, n_search=64, degree=512, found=len(ev), applications=info["applications"], wall_s=med,
                     wall_runs=runs, **shares(ctx, call)))
    print(json.dumps(rows[-1]), flush=True)

    sp, n = open_haldane(ctx, a.flake)
    g = np.zeros(2)
    _lib.check(_lib.lib.tbk_sparse_info(sp, None, None, None, _lib.dptr(g)))
    bnd = (g[0] - 0.01 * (g[1] - g[0]), g[1] + 0.01 * (g[1] - g[0]))
    ns = 128
    while True:
        try:
            ev, vec, res, info = raw_eigs(sp, n, (-0.35, 0.35), bnd, ns, 512)
            break
        except _lib.TbkError as e:
            if "raise n_search" not in str(e) or ns >= 2048:
                raise
            print("n_search = %d is saturated" % ns, flush=True)
            ns *= 2
    call = lambda: raw_eigs(sp, n, (-0.35, 0.35), bnd, ns, 512)
    med, runs = timed(call, a.repeat)
    rows.append(dict(case="B", nsta=n, n_search=ns, degree=512, found=len(ev), applications=int(info[0]), strong=int(info[2]),
                     worst_residual=float(res.max()) if len(res) else 0.0,
                     orthonormality=float(np.abs(vec.conj() @ vec.T - np.identity(len(ev))).max()) if len(ev) else 0.0, wall_s=med,
                     wall_runs=runs, **shares(ctx, call)))
    print(json.dumps(rows[-1]), flush=True)
    _lib.check(_lib.lib.tbk_sparse_free(sp))

    d = km_flake(16, 32)
    call = lambda: d.solve_all(eig_vectors=True)
    med, runs = timed(call, a.repeat)
    rows.append(dict(case="C", nsta=d._nsta, what="dense solve_all(eig_vectors=True), every eigenpair", wall_s=med, wall_runs=runs))
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
