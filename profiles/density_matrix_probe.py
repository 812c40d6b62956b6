#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of the occupied-state calls: one step of a
mean-field loop -- fermi_level_mesh, then density_matrix_mesh on a short list of lattice vectors -- and thermodynamics_mesh
at 256 levels, for Haldane (n = 2) on a 256 x 256 mesh, its 4 x 4 supercell (n = 32) on 64 x 64 and the w90 silicon model on
32 x 32 x 32.  Prints one JSON line per call: the wall time, the kernel times by label, the sum of the occ_* and dm_* brackets (the
stages this unit adds) and the sum of all the others (the k generator and the eigen-solve), and that share.  Then the solver
alone under the same brackets: one solve_all_mesh of the same mesh with and without eigenvectors.

    python profiles/density_matrix_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
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
    own = sum(v for k, v in kern.items() if k.startswith(("occ_", "dm_")))
    rest = sum(v for k, v in kern.items() if not k.startswith(("occ_", "dm_")))
    rec = dict(case=name, call_ms=round(ms, 2), kernels_ms=kern, occ_stages_ms=round(own, 3), solves_ms=round(rest, 3))
    if own + rest > 0.0:
        rec["solve_share_of_kernel_time"] = round(rest / (own + rest), 3)
    rec.update(extra)
    print(json.dumps(rec), flush=True)


def workloads(name, m, mesh, nel, kT):
    if QUICK:
        mesh = [max(2, x // 4) for x in mesh]
    d = m._dim_k
    unit = np.identity(d, dtype=int)
    rs = np.concatenate([np.zeros((1, d), dtype=int), unit, -unit])           # R = 0 and the nearest neighbours
    info = dict(n=m._nsta, mesh=list(mesh))
    mu = m.fermi_level_mesh(mesh, nel, kT=kT)
    for t in (0.0, kT):
        tag = "%s_kT%g" % (name, t)
        call(tag + "_fermi_level", lambda: m.fermi_level_mesh(mesh, nel, kT=t), dict(info, nfill=1))
        call(tag + "_fermi_level_16", lambda: m.fermi_level_mesh(mesh, np.full(16, nel), kT=t), dict(info, nfill=16))
        call(tag + "_density_matrix", lambda: m.density_matrix_mesh(mesh, mu, t, rs), dict(info, nR=len(rs)))
        call(tag + "_density_matrix_R0", lambda: m.density_matrix_mesh(mesh, mu, t), dict(info, nR=1))
        call(tag + "_thermodynamics_256", lambda: m.thermodynamics_mesh(mesh, np.linspace(mu - 1.0, mu + 1.0, 256), t),
             dict(info, nmu=256))
    for vec in (True, False):
        call("%s_solve_alone_%s" % (name, "vectors" if vec else "values"), lambda: m.solve_all_mesh(mesh, eig_vectors=vec), info)


hal = hp.haldane(tb.tb_model, delta=0.2)
workloads("haldane_256x256", hal, [256, 256], 1.0, 0.05)
workloads("haldane4x4_64x64", quiet(hal.make_supercell, [[4, 0], [0, 4]]), [64, 64], 16.0, 0.05)
silicon = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
workloads("silicon_32x32x32", silicon, [32, 32, 32], 4.0, 0.05)
