#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of susceptibility_mesh on its two workloads:
a static 64 x 64 q-map and a 256-frequency cut along a q path of 64 points, for Haldane (n = 2) on a 256 x 256 mesh and for the
w90 silicon model on a 32 x 32 x 32 mesh, with and without matrix elements.  Prints one JSON line per call: the wall time, the
kernel times by label, the sum of the chi_* brackets (the stages this unit adds) and the sum of all the others (the k generator
and the two eigen-solves per (chunk, q)), and that share.  Then the same solver launches alone: one solve_all_mesh of the same
mesh with and without eigenvectors under the same brackets -- times (1 + nq) it is the floor of the design, which solves at k
once per chunk and at k + q once per (chunk, q).

    python profiles/susceptibility_probe.py [--quick]      (--quick: an 8 x 8 q-map and 8 path points)"""
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
    chi = sum(v for k, v in kern.items() if k.startswith("chi_"))
    rest = sum(v for k, v in kern.items() if not k.startswith("chi_"))
    rec = dict(case=name, call_ms=round(ms, 2), kernels_ms=kern, chi_stages_ms=round(chi, 3), solves_ms=round(rest, 3))
    if chi + rest > 0.0:
        rec["solve_share_of_kernel_time"] = round(rest / (chi + rest), 3)
    rec.update(extra)
    print(json.dumps(rec), flush=True)


def workloads(name, m, mesh, mu, kT):
    d = m._dim_k
    g = np.arange(NMAP) / NMAP
    qmap = np.zeros((NMAP * NMAP, d))
    qmap[:, 0] = np.repeat(g, NMAP)
    qmap[:, 1] = np.tile(g, NMAP)
    path = np.zeros((NPATH, d))
    path[:, 0] = 0.5 * (1 + np.arange(NPATH)) / NPATH           # (0, 0) -> (1/2, 1/2), without q = 0
    path[:, 1] = path[:, 0]
    w = np.linspace(0.0, 6.0, NW)
    info = dict(n=m._nsta, mesh=list(mesh))
    for me in (True, False):
        tag = "%s_%s" % (name, "me" if me else "bands")
        call(tag + "_static_map", lambda: m.susceptibility_mesh(mesh, qmap, fermi_level=mu, kT=kT, matrix_elements=me),
             dict(info, nq=len(qmap), nw=0))
        call(tag + "_omega_path", lambda: m.susceptibility_mesh(mesh, path, w, 0.05, fermi_level=mu, kT=kT, matrix_elements=me),
             dict(info, nq=len(path), nw=NW))
    for vec in (True, False):
        call("%s_solve_alone_%s" % (name, "vectors" if vec else "values"), lambda: m.solve_all_mesh(mesh, eig_vectors=vec), info)


workloads("haldane_256x256", hp.haldane(tb.tb_model, delta=0.2), [256, 256], 0.3, 0.05)
silicon = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
workloads("silicon_32x32x32", silicon, [32, 32, 32], 6.0, 0.05)
