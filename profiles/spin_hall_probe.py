#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of spin_hall_conductivity_mesh beside berry_curvature_mesh on the same
case in the same process: Kane-Mele 4096 x 512 (n = 4), a 16-state and a 32-state spinful random model
and the 64-state 4 x 4 supercell of Kane-Mele (the wide form).  Prints one JSON line per call and one per case with the ratio
of the spin call's contraction brackets to the charge call's."""
import contextlib
import io
import json
import os
import sys
import time

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import pythtb_amd as tb  # noqa: E402
import helpers as hp  # noqa: E402
from pythtb_amd import _lib  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def call(name, fn, reps):
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
    return kern


def case(name, m, mesh, occ, reps):
    charge = call(name + "_charge", lambda: m.berry_curvature_mesh(mesh, occ=occ), reps)
    spin = call(name + "_spin_z", lambda: m.spin_hall_conductivity_mesh(mesh, 2, occ=occ), reps)
    ratios = {}
    for stage in ("lds", "wsp", "contract", "occ_sum"):
        if "curv_" + stage in charge and "spin_curv_" + stage in spin:
            ratios[stage] = round(spin["spin_curv_" + stage] / charge["curv_" + stage], 3)
    print(json.dumps(dict(case=name, n=m._nsta, spin_over_charge=ratios)), flush=True)


km = hp.kane_mele(tb.tb_model)
case("kane_mele_4096x512", km, [4096, 512], [0, 1], 3)
case("random_n16_256^2", hp.random_model(tb.tb_model, 8, 2, 2, 33), [256, 256], list(range(8)), 2)
case("random_n32_128^2", hp.random_model(tb.tb_model, 16, 2, 2, 34), [128, 128], list(range(16)), 2)
case("kane_mele_4x4_n64_32^2", quiet(km.make_supercell, [[4, 0], [0, 4]]), [32, 32], list(range(32)), 2)
