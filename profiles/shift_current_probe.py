#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of shift_current_mesh and injection_current_mesh
beside optical_conductivity_mesh on the same model, mesh and frequencies: Kane-Mele 4096 x 512 (n = 4), cubic16 64^3 (n = 16), a random
32-state model on 96^2 (the LDS pair kernel at its largest matrices) and a random 72-state model on 32^2 (the wide pair kernels), each
with 512 frequencies across the spectrum, the Fermi level at mid-spectrum, kT = 0.05, the full tensor.  Prints one JSON line per call and
the ratio of the new pair stage (shift_pairs + shift_wide) to the pair stage of optical_conductivity_mesh (opt_pairs + opt_wide)."""
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
from pythtb_amd import _lib  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def case(name, fn, reps, stage):
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
    rep = ctx.prof_report()
    kern = {k: round(v["total_ms"] * 1e3, 1) for k, v in rep.items()}
    ctx.prof_enable(0)
    pair = sum(kern.get(k, 0.0) for k in stage)
    print(json.dumps(dict(case=name, call_ms=round(ms, 3), kernels_us=kern, launches={k: v["launches"] for k, v in rep.items()},
                          pair_stage_us=round(pair, 1))), flush=True)
    return pair


MODELS = {
    "kane_mele_4096x512": lambda: (hp.kane_mele(tb.tb_model), [4096, 512], 2),
    "cubic16_64^3": lambda: (hp.cubic16(tb.tb_model), [64, 64, 64], 2),
    "random32_96^2": lambda: (hp.random_model(tb.tb_model, 32, 2, 1, 43), [96, 96], 2),
    "random72_32^2": lambda: (hp.random_model(tb.tb_model, 72, 2, 1, 45), [32, 32], 2),
}

for name in sys.argv[1:] or list(MODELS):
    m, mesh, reps = MODELS[name]()
    e = m.solve_all_mesh([8] * len(mesh))
    omega = np.linspace(0.0, e.max() - e.min(), 512)
    mu = float(np.median(e))
    opt = case(name + " optics", lambda: m.optical_conductivity_mesh(mesh, omega, 0.05, fermi_level=mu, kT=0.05), reps,
               ("opt_pairs", "opt_wide"))
    for label, call in (("shift", m.shift_current_mesh), ("injection", m.injection_current_mesh)):
        new = case(name + " " + label, lambda: call(mesh, omega, 0.05, fermi_level=mu, kT=0.05), reps, ("shift_pairs", "shift_wide"))
        if opt:
            print(json.dumps(dict(case=name, call=label, pair_stage_over_optics=round(new / opt, 3))), flush=True)
