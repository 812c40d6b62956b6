#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of optical_conductivity_mesh: Haldane 2048^2
(n = 2), Kane-Mele 4096 x 512 (n = 4), w90 silicon 48^3 mid-gap (n = 8, d = 3), cubic16 64^3 with 8 bands occupied
(n = 16, d = 3), the Haldane 4 x 4 supercell on 256^2 (n = 32) and a 40-cell Haldane ribbon on 4096 k (n = 80, dim_k = 1).
Prints one JSON line per case: the call time, the kernel times, the pairs with c != 0 and the frequency kernel's time per
(pair, frequency) in ps.  Optional arguments: case names to run (default all)."""
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


def live_pairs(m, mesh, mu):
    """Pairs with c != 0 at kT = 0: per k, (levels <= mu) x (levels > mu)."""
    e = m.solve_all_mesh(mesh)
    occ = (e <= mu).sum(axis=0)
    return int(np.sum(occ * (m._nsta - occ)))


def case(name, m, mesh, nw, mu, eta, reps):
    ctx = _lib.default_context()
    w = np.linspace(-4.0, 4.0, nw)
    fn = lambda: m.optical_conductivity_mesh(mesh, w, eta, fermi_level=mu)  # noqa: E731
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
    pairs = live_pairs(m, mesh, mu)
    ps = kern.get("opt_omega", 0.0) * 1e6 / (pairs * nw) if pairs else None
    print(json.dumps(dict(case=name, call_ms=round(ms, 3), pairs=pairs, nomega=nw, kernels_us=kern,
                          omega_ps_per_pair_freq=None if ps is None else round(ps, 3))), flush=True)


CASES = {
    "haldane_2048^2": lambda: (hp.haldane(tb.tb_model, 0.2), [2048, 2048], 512, 0.0, 0.02, 3),
    "kane_mele_4096x512": lambda: (hp.kane_mele(tb.tb_model), [4096, 512], 512, 0.0, 0.02, 3),
    "silicon_48^3": lambda: (quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model), [48, 48, 48],
                             512, None, 0.02, 2),
    "cubic16_64^3": lambda: (hp.cubic16(tb.tb_model), [64, 64, 64], 256, 0.0, 0.02, 2),
    "haldane_4x4_256^2": lambda: (quiet(hp.haldane(tb.tb_model, 0.2).make_supercell, [[4, 0], [0, 4]]), [256, 256], 256, 0.0,
                                  0.02, 2),
    "haldane_ribbon40_4096": lambda: (quiet(hp.haldane(tb.tb_model, 0.2).cut_piece, 40, 1), [4096], 512, 0.0, 0.02, 2),
}

for name in sys.argv[1:] or list(CASES):
    m, mesh, nw, mu, eta, reps = CASES[name]()
    if mu is None:                         # mid-gap of the four valence bands
        e = m.solve_all_mesh([16, 16, 16])
        mu = 0.5 * (e[3].max() + e[4].min())
    case(name, m, mesh, nw, mu, eta, reps)
