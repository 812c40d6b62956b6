#!/usr/bin/env python3
"""Wall times of the unfolding calls on one device, each beside solve_all(k, eig_vectors=True) of the same
supercell k list (what a host-side projection would have to download):

    haldane10x10_nw512   the 10 x 10 Haldane supercell (200 states, on-site disorder), a 300-point path, 512 frequencies
    haldane10x10_nw1     the same at one frequency
    haldane32x32_nw1024  the 32 x 32 supercell (2048 states), a 64-point path, 1024 frequencies
    silicon_id_nw512     the identity case of the 8-state w90 silicon model (fat bands), 300 points, 512 frequencies

per case: unfolded_spectral total and per_state, unfolded_bands per_state, the solve; the ratio of each to the solve; the kernel
times by label from the tbk_prof_* brackets (a pass of its own); the bytes the call returns against the bytes of eigenvectors
the solve downloads.

Method (that of green_function_probe.py): every call ends in a device synchronise (it downloads its result), so a host clock around
calls is their time.  Each function is warmed up once; the warm-up sets the number N of back-to-back calls that fill a window of
about WINDOW_MS, and a window of N calls is timed REPS times, the functions of a case alternating; the line gives the median time
per call and the spread (min, max) over the windows, and N.  One JSON line per case.

The 2048-state case times unfolded_spectral(per_state=True) and the solve only (a call on 64 points takes 40 s: the time budget of a run decides --big-points).

    python profiles/unfold_probe.py [--quick] [--big-points N]
    (--quick: 4 x 4 and 8 x 8 supercells, a quarter of the points; --big-points: the points of the 2048-state path, default 64)"""
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
BIG_POINTS = int(sys.argv[sys.argv.index("--big-points") + 1]) if "--big-points" in sys.argv else 64
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


def case(name, m, S, k, nw, only=None):
    n, nk = m._nsta, len(k)
    per = list(m._per)
    K = np.ascontiguousarray(k @ np.array(S, dtype=float)[np.ix_(per, per)].T)
    ev = m.solve_all(K)
    w = np.linspace(float(ev.min()), float(ev.max()), nw) if nw > 1 else np.array([0.5 * float(ev.min() + ev.max())])
    fns = dict(spectral=lambda: m.unfolded_spectral(k, w, ETA, S),
               spectral_per_state=lambda: m.unfolded_spectral(k, w, ETA, S, per_state=True),
               bands_per_state=lambda: m.unfolded_bands(k, S, per_state=True),
               solve=lambda: m.solve_all(K, eig_vectors=True))
    if only:
        fns = {key: fns[key] for key in only}
    t = timed(fns)
    solve = float(np.median(t["solve"][0]))
    ng = m.unfolded_spectral(k[:1], w[:1], ETA, S, per_state=True).shape[-1]
    rec = dict(case=name, n=n, nk=nk, nw=nw, ng=ng)
    for key in fns:
        rec[key] = stats(t[key])
        if key != "solve":
            rec[key]["ratio_to_solve"] = round(float(np.median(t[key][0])) / solve, 3)
    rec["kernels_ms"] = {key: kernels(fns[key]) for key in ("spectral_per_state", "bands_per_state", "solve") if key in fns}
    rec["bytes_returned"] = dict(spectral=8 * nk * nw, spectral_per_state=8 * nk * nw * ng, bands_per_state=8 * n * nk * (ng + 1),
                                 eigenvectors_of_the_solve=16 * n * n * nk)
    print(json.dumps(rec), flush=True)


def path(m, nk):
    return m.k_path([[0.0, 0.0], [2.0 / 3.0, 1.0 / 3.0], [0.5, 0.5], [0.0, 0.0]], nk, report=False)[0]


def disordered(m, seed):
    m.set_onsite(list(np.random.default_rng(seed).uniform(-0.25, 0.25, m._norb)), mode="add")
    return m


hal = hp.haldane(tb.tb_model, delta=0.2)
a, b = (4, 8) if QUICK else (10, 32)
scale = 4 if QUICK else 1
sc = disordered(quiet(hal.make_supercell, [[a, 0], [0, a]]), 1)
case("haldane%dx%d_nw512" % (a, a), sc, [[a, 0], [0, a]], path(hal, 300 // scale), 512)
case("haldane%dx%d_nw1" % (a, a), sc, [[a, 0], [0, a]], path(hal, 300 // scale), 1)
silicon = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
ks = np.random.default_rng(2).uniform(-0.5, 0.5, (300 // scale, 3))
case("silicon_id_nw512", silicon, np.identity(3, dtype=int), ks, 512)
big = disordered(quiet(hal.make_supercell, [[b, 0], [0, b]]), 2)
case("haldane%dx%d_nw1024" % (b, b), big, [[b, 0], [0, b]], path(hal, BIG_POINTS // scale), 1024, only=("spectral_per_state", "solve"))
