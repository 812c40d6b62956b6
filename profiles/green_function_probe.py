#!/usr/bin/env python3
"""Wall times of the Green's-function calls on one device: green_function_mesh for Haldane (n = 2) on a
256 x 256 mesh, the w90 silicon model (n = 8) on 32 x 32 x 32 and the 4 x 4 Haldane supercell (n = 32) on 64 x 64, each at
(nw = 256, R = 0), (nw = 16, 9 lattice vectors) and (nw = 1, the same 9 vectors); beside each the time of density_matrix_mesh on
the same mesh and R list (both run the lattice sum of tbk_lat_dev.h: G at nw = 1 is the same walk with complex weights) and
the ratio; then the 64 x 64 impurity LDOS map of Haldane 256 x 256 at 16 frequencies.

Method: every call ends in a device synchronise (it downloads its result), so a host clock around calls is their time.  Each case
is warmed up once (model upload, scratch growth, code objects); the warm-up sets the number N of back-to-back calls that fill a
window of about WINDOW_MS, and a window of N calls is timed REPS times, alternating with the density-matrix partner's; the line
gives the median time per call and the spread (min, max) over the windows, and N.  A second pass with the tbk_prof_* brackets
gives the kernel times by label, in a run of its own.  One JSON line per case.

    python profiles/green_function_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import pythtb_amd as tb  # noqa: E402
import helpers as hp  # noqa: E402
from pythtb_amd import _lib, w90  # noqa: E402

QUICK = "--quick" in sys.argv
REPS = 7
WINDOW_MS = 100.0
ETA = 0.05


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def timed(fns):
    """ms per call of every function of `fns`, from REPS windows of N back-to-back calls each, alternating:
    {name: ([ms, ...], N)}."""
    ctx = _lib.default_context()
    count = {}
    for k, fn in fns.items():
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        once = (time.perf_counter() - t0) * 1e3
        count[k] = int(min(2000, max(1, round(WINDOW_MS / once))))
    out = {k: ([], count[k]) for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(count[k]):
                fn()
            out[k][0].append((time.perf_counter() - t0) * 1e3 / count[k])
    return out


def stats(res):
    ms, count = res
    return dict(calls_per_window=count, median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def kernels(fn):
    ctx = _lib.default_context()
    ctx.prof_reset()
    ctx.prof_enable(1)
    fn()
    ctx.sync()
    kern = {k: round(v["total_ms"], 3) for k, v in ctx.prof_report().items()}
    ctx.prof_enable(0)
    return kern


def green_cases(name, m, mesh):
    if QUICK:
        mesh = [max(2, x // 4) for x in mesh]
    d = m._dim_k
    ev = m.solve_all_mesh(mesh)
    lo, hi = float(ev.min()), float(ev.max())
    unit = np.identity(d, dtype=int)
    nine = np.concatenate([np.zeros((1, d), dtype=int), unit, -unit, unit + np.roll(unit, 1, axis=0), -unit - np.roll(unit, 1, axis=0)])[:9]
    zero = np.zeros((1, d), dtype=int)
    mu = 0.5 * (lo + hi)
    for nw, rs in ((256, zero), (16, nine), (1, nine), (1, zero)):
        w = np.linspace(lo, hi, nw) if nw > 1 else np.array([mu])
        g = lambda: m.green_function_mesh(mesh, w, ETA, rs)
        dm = lambda: m.density_matrix_mesh(mesh, mu, 0.05, rs)
        t = timed(dict(green=g, density_matrix=dm))
        rec = dict(case="%s_nw%d_nR%d" % (name, nw, len(rs)), n=m._nsta, mesh=list(mesh), green=stats(t["green"]),
                   density_matrix=stats(t["density_matrix"]),
                   ratio=round(float(np.median(t["green"][0]) / np.median(t["density_matrix"][0])), 2), green_kernels_ms=kernels(g),
                   density_matrix_kernels_ms=kernels(dm))
        print(json.dumps(rec), flush=True)


def ldos_map(m, mesh):
    if QUICK:
        mesh = [max(2, x // 4) for x in mesh]
    side = min(64, mesh[0])
    grid = np.array([[a, b] for a in range(-side // 2, side // 2) for b in range(-side // 2, side // 2)])
    w = np.linspace(-1.0, 1.0, 16)
    f = lambda: m.impurity_ldos_mesh(mesh, w, ETA, [(0, [0, 0])], [2.0], R_list=grid)
    t = timed(dict(ldos=f))
    print(json.dumps(dict(case="haldane_ldos_map_%dx%d_nw16" % (side, side), mesh=list(mesh), ldos=stats(t["ldos"]), kernels_ms=kernels(f))),
          flush=True)


hal = hp.haldane(tb.tb_model, delta=0.2)
green_cases("haldane_256x256", hal, [256, 256])
silicon = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
green_cases("silicon_32x32x32", silicon, [32, 32, 32])
green_cases("haldane4x4_64x64", quiet(hal.make_supercell, [[4, 0], [0, 4]]), [64, 64])
ldos_map(hal, [256, 256])
