#!/usr/bin/env python3
"""Landauer transmission by the recursive Green's function sweep (transmission) beside its NumPy restatement
(tests/landauer_ref.py) on a subsample of the same inputs.  Per case one JSON line: the call's wall time and HIP-event time, the
per-kernel times of the library's profiling brackets, the mean decimation steps of the leads, the time per (k, omega, layer) of
the transmission kernel, and the restatement's time per (k, omega, layer) on the subsample.  No speed figure existed for this path
before it was added: the numbers are recorded, not compared with a threshold.    python profiles/landauer_probe.py [case ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as hp  # noqa: E402
import landauer_ref as lr  # noqa: E402
import pythtb_amd as tb  # noqa: E402
from pythtb_amd import _lib  # noqa: E402

ctx = _lib.default_context()
ETA = 0.01


def timed(fn, reps=2):
    """Best of `reps` after one warm-up: (wall ms, HIP-event ms, per-kernel ms, result)."""
    out = fn()
    best = None
    for _ in range(reps):
        ctx.prof_enable(1)
        ctx.prof_reset()
        t0 = time.perf_counter()
        ctx.timer_begin()
        out = fn()
        ev = ctx.timer_end()
        wall = (time.perf_counter() - t0) * 1e3
        rep = ctx.prof_report()
        ctx.prof_enable(0)
        if best is None or wall < best[0]:
            best = (wall, ev, {k: round(v["total_ms"], 3) for k, v in rep.items()}, out)
    return best


def case(name):
    T = tb.tb_model
    if name == "haldane_ribbon":       # the ribbon of 8 cells as the crystal: N = 16, no k
        m, fd, nk, nw, M, mesh = hp.quiet(hp.haldane(T, delta=0.2).cut_piece, 8, 1), 0, 1, 4096, 32, None
    elif name == "kane_mele":
        m, fd, nk, nw, M, mesh = hp.kane_mele(T), 0, 1024, 256, 8, None
    elif name == "cubic16":
        m, fd, nk, nw, M, mesh = hp.cubic16(T), 2, 32 * 32, 64, 4, [32, 32]
    elif name == "random36":
        m, fd, nk, nw, M, mesh = hp.random_model(T, 18, 3, 2, seed=4, rmax=1), 0, 16 * 16, 16, 4, [16, 16]
    else:
        raise SystemExit("unknown case " + name)
    lo, hi = (-3.2, 3.2) if name in ("haldane_ribbon", "kane_mele") else (-4.0, 4.0)
    om = np.linspace(lo, hi, nw)
    dev = lr.disordered(m, fd, M, seed=1)
    if m._dim_k == 1:
        k = None
    elif mesh is None:
        k = (np.arange(nk) / nk).reshape(-1, 1)
    else:
        k = hp.quiet(m.cut_piece, 1, fd).k_uniform_mesh(mesh)
    wall, ev, kern, out = timed(lambda: m.transmission(k, om, ETA, fd, device=dev, return_info=True))
    N = m.principal_layer(fd) * m._nsta
    sweep = sum(v for kname, v in kern.items() if kname.startswith("land_") and kname not in ("land_blocks", "land_rows"))
    # the restatement on a subsample: at most 4 k x 4 omega of the same inputs
    ks = None if k is None else k[::max(1, nk // 4)][:4]
    oms = om[::max(1, nw // 4)][:4]
    t0 = time.perf_counter()
    want, _ = lr.transmission(m, ks, oms, ETA, fd, dev)
    ref_s = time.perf_counter() - t0
    got = m.transmission(ks, oms, ETA, fd, device=dev)
    rec = dict(case=name, N=N, layers=M, nk=nk, nomega=nw, eta=ETA, wall_ms=round(wall, 2), event_ms=round(ev, 2), kernels_ms=kern,
               mean_steps=round(float(out[1].mean()), 2), max_T=round(float(out[0].max()), 4),
               ns_per_point_layer=round(sweep * 1e6 / (nk * nw * M), 3),
               wall_ns_per_point_layer=round(wall * 1e6 / (nk * nw * M), 3),
               numpy_points=int(want.size), numpy_ns_per_point_layer=round(ref_s * 1e9 / (want.size * M), 1),
               max_abs_diff_on_subsample=float(np.abs(got - want).max()))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    for c in (sys.argv[1:] or ["haldane_ribbon", "kane_mele", "cubic16", "random36"]):
        case(c)
