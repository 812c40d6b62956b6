#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of orbital_magnetization_mesh beside
berry_curvature_mesh's Fermi scan on the same mesh: Haldane 2048^2 (n = 2), Kane-Mele 1024^2 (n = 4), cubic16 65^3 (n = 16)
and w90 silicon 48^3 (n = 8), each with 512 levels spread over the spectrum.  Per model: the curvature scan, the T = 0 scan,
the kT = 0.05 scan and the band set.  Prints one JSON line per call, with the thermal scan's (orb_kt) time per (record, level) in ps."""
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


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def case(name, fn, reps, records=None, nmu=None):
    ctx = _lib.default_context()
    fn()                                   # warm-up (model upload, scratch growth, code objects)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ms = (time.perf_counter() - t0) / reps * 1e3
    ctx.prof_reset()
    ctx.prof_enable(1)
    fn()
    ctx.sync()
    kern = {k: round(v["total_ms"] * 1e3, 1) for k, v in ctx.prof_report().items()}
    ctx.prof_enable(0)
    row = dict(case=name, call_ms=round(ms, 3), kernels_us=kern)
    if records and "orb_kt" in kern:
        row["kt_ps_per_record_level"] = round(kern["orb_kt"] * 1e6 / (records * nmu), 3)
    print(json.dumps(row), flush=True)


MODELS = {
    "haldane_2048^2": lambda: (hp.haldane(tb.tb_model, 0.2), [2048, 2048], [0], 3),
    "kane_mele_1024^2": lambda: (hp.kane_mele(tb.tb_model), [1024, 1024], [0, 1], 3),
    "cubic16_65^3": lambda: (hp.cubic16(tb.tb_model), [65, 65, 65], list(range(8)), 2),
    "silicon_48^3": lambda: (quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model), [48, 48, 48],
                             [0, 1, 2, 3], 2),
}

for name in sys.argv[1:] or list(MODELS):
    m, mesh, occ, reps = MODELS[name]()
    e = m.solve_all_mesh([16] * len(mesh))
    levels = np.linspace(e.min(), e.max(), 512)
    records = int(np.prod(mesh)) * m._nsta
    case(name + " curv_fermi512", lambda: m.berry_curvature_mesh(mesh, fermi_levels=levels), reps)
    case(name + " orb_t0_512", lambda: m.orbital_magnetization_mesh(mesh, fermi_levels=levels), reps)
    case(name + " orb_kT0.05_512", lambda: m.orbital_magnetization_mesh(mesh, fermi_levels=levels, kT=0.05), reps, records, 512)
    case(name + " orb_occ", lambda: m.orbital_magnetization_mesh(mesh, occ=occ), reps)
