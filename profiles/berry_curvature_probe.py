#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of the Berry-curvature calls:
Haldane 2048^2 mesh integral (n = 2, fused), Kane-Mele 4096 x 512 (n = 4), cubic16 per band on 64^3, the Haldane 4 x 4
supercell on 256^2 (n = 32) and a 512-level Fermi scan of w90 silicon on 48^3.  Prints one JSON line per case."""
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


def case(name, fn, reps):
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
    print(json.dumps(dict(case=name, call_ms=round(ms, 3), kernels_us=kern)), flush=True)


hal = hp.haldane(tb.tb_model, 0.2)
km = hp.kane_mele(tb.tb_model)
cub = hp.cubic16(tb.tb_model)
sc4 = quiet(hal.make_supercell, [[4, 0], [0, 4]])
si = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
e_si = si.solve_all_mesh([16, 16, 16])
levels = np.linspace(e_si.min(), e_si.max(), 512)

case("haldane_2048^2_occ0", lambda: hal.berry_curvature_mesh([2048, 2048], occ=[0]), 10)
case("haldane_2048^2_per_band", lambda: hal.berry_curvature_mesh([2048, 2048]), 10)
case("kane_mele_4096x512_occ01", lambda: km.berry_curvature_mesh([4096, 512], occ=[0, 1]), 3)
case("cubic16_64^3_per_band", lambda: cub.berry_curvature_mesh([64, 64, 64]), 2)
case("haldane_4x4_256^2_occ16", lambda: sc4.berry_curvature_mesh([256, 256], occ=list(range(16))), 2)
case("silicon_48^3_fermi512", lambda: si.berry_curvature_mesh([48, 48, 48], fermi_levels=levels), 2)
