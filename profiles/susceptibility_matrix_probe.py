#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of susceptibility_matrix_mesh beside the scalar
susceptibility_mesh in the same process, on the workloads of profiles/susceptibility_probe.py: a static 64 x 64 q-map and a
256-frequency cut along a q path of 64 points, for Haldane (n = 2) on a 256 x 256 mesh and for the w90 silicon model (n = 8) on a
32 x 32 x 32 mesh -- the full matrix (all states), and the RPA with an on-site U on top.  The scalar call, with the same two
eigen-solves per (chunk, q), is the yardstick.  Prints one JSON line per call: the wall time, the kernel times by label, the sum of
the chi_* / chim_* brackets (the stages of the unit) and of all the others (the k generator and the solves), and per workload the
ratio matrix / scalar of the wall times.

    python profiles/susceptibility_matrix_probe.py [--quick]      (--quick: an 8 x 8 q-map and 8 path points)"""
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
NMAP, NPATH, NW = (8, 8, 256) if QUICK else (64, 64, 256)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def call(name, fn, extra):
    ctx = _lib.default_context()
    fn()                                   # warm-up (model upload, scratch growth, code objects)
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ms = (time.perf_counter() - t0) * 1e3
    ctx.prof_reset()
    ctx.prof_enable(1)
    fn()
    ctx.sync()
    kern = {k: round(v["total_ms"], 3) for k, v in ctx.prof_report().items()}
    ctx.prof_enable(0)
    chi = sum(v for k, v in kern.items() if k.startswith("chi"))
    rest = sum(v for k, v in kern.items() if not k.startswith("chi"))
    rec = dict(case=name, call_ms=round(ms, 2), kernels_ms=kern, chi_stages_ms=round(chi, 3), solves_ms=round(rest, 3))
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return ms


def workloads(name, m, mesh, mu, kT):
    d, n = m._dim_k, m._nsta
    g = np.arange(NMAP) / NMAP
    qmap = np.zeros((NMAP * NMAP, d))
    qmap[:, 0] = np.repeat(g, NMAP)
    qmap[:, 1] = np.tile(g, NMAP)
    path = np.zeros((NPATH, d))
    path[:, 0] = 0.5 * (1 + np.arange(NPATH)) / NPATH           # (0, 0) -> (1/2, 1/2), without q = 0
    path[:, 1] = path[:, 0]
    w = np.linspace(0.0, 6.0, NW)
    u = 0.5 * np.eye(n)
    info = dict(n=n, na=n, mesh=list(mesh))
    for tag, qs, kw in (("static_map", qmap, {}), ("omega_path", path, {"omega": w, "eta": 0.05})):
        ex = dict(info, nq=len(qs), nw=len(kw.get("omega", ())))
        t_s = call("%s_%s_scalar" % (name, tag), lambda: m.susceptibility_mesh(mesh, qs, fermi_level=mu, kT=kT, **kw), ex)
        t_m = call("%s_%s_matrix" % (name, tag), lambda: m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, **kw), ex)
        t_r = call("%s_%s_matrix_rpa" % (name, tag),
                   lambda: m.susceptibility_matrix_mesh(mesh, qs, fermi_level=mu, kT=kT, interaction=u, return_det=True, **kw), ex)
        print(json.dumps(dict(case="%s_%s" % (name, tag), matrix_over_scalar=round(t_m / t_s, 2), rpa_over_matrix=round(t_r / t_m, 3))),
              flush=True)


workloads("haldane_256x256", hp.haldane(tb.tb_model, delta=0.2), [256, 256], 0.3, 0.05)
silicon = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
workloads("silicon_32x32x32", silicon, [32, 32, 32], 6.0, 0.05)
