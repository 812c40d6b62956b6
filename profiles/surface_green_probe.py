#!/usr/bin/env python3
"""Edge spectra by iterative decimation (surface_spectral / surface_dos_mesh) beside the ribbon route for the
same picture: cut_piece(64, fin_dir) + solve_all with eigenvectors on the same k of the surface zone.  Per case one JSON line: the
call's wall time and HIP-event time, the per-kernel times of the library's profiling brackets, the mean decimation steps, the
real multiply-adds per step and problem implied by the decimation kernel's time, and the ribbon's time (null with the reason where the
ribbon cannot be built or solved).  The ribbon is timed on THIS build: the change that added the surface calls touches neither
`cut_piece` nor the eigen-solver, so the time is that of the parent commit's route.  Two of the four cases can never yield a ratio --
the ribbon of the 36-state model has 2304 states, beyond the solver's 2048, and the ribbon of cubic16 is not built (see ribbon_time)
-- and report `ribbon: null`.    python profiles/surface_green_probe.py [case ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as hp  # noqa: E402
import pythtb_amd as tb  # noqa: E402
from pythtb_amd import _lib  # noqa: E402

ctx = _lib.default_context()
RIBBON_CELLS = 64
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


def ribbon_time(m, fin_dir, k):
    """cut_piece(RIBBON_CELLS) + solve_all(eig_vectors=True) on the k list, or (None, reason)."""
    nhop = len(m._hoppings) * RIBBON_CELLS
    nsta = m._nsta * RIBBON_CELLS
    if nsta > _lib.MAX_NSTA:
        return None, "ribbon of %d states is beyond the solver's %d" % (nsta, _lib.MAX_NSTA)
    # cut_piece adds every hopping with set_hop(mode="add"), which walks the list so far: nhop^2 / 2 comparisons of a few
    # microseconds each.  An estimate, not a measurement: 4000 hoppings are ~10^7 comparisons, about half a minute; the 56 832 of
    # cubic16 would be 1.6 10^9, hours.
    if nhop > 4000:
        return None, "cut_piece of %d hoppings is quadratic in their number (estimated, not measured): not built" % nhop
    rib = hp.quiet(m.cut_piece, RIBBON_CELLS, fin_dir)
    if nsta * nsta * 16 * len(k) > 8 << 30:
        return None, "eigenvectors of %d k-points of a %d-state ribbon do not fit one call" % (len(k), nsta)
    wall, ev, kern, _ = timed(lambda: rib.solve_all(k, eig_vectors=True), reps=1)
    return dict(states=nsta, wall_ms=round(wall, 2), event_ms=round(ev, 2), kernels_ms=kern), None


def case(name):
    T = tb.tb_model
    if name == "haldane":
        m, fd, nk, nw, mesh = hp.haldane(T, delta=0.2), 0, 2048, 1024, None
    elif name == "kane_mele":
        m, fd, nk, nw, mesh = hp.kane_mele(T), 0, 1024, 512, None
    elif name == "cubic16":
        m, fd, nk, nw, mesh = hp.cubic16(T), 2, 64 * 64, 128, [64, 64]
    elif name == "random36":
        m, fd, nk, nw, mesh = hp.random_model(T, 18, 3, 2, seed=4, rmax=1), 0, 32 * 32, 32, [32, 32]
    else:
        raise SystemExit("unknown case " + name)
    lo, hi = (-3.2, 3.2) if name in ("haldane", "kane_mele") else (-4.0, 4.0)
    om = np.linspace(lo, hi, nw)
    if mesh is None:
        k = (np.arange(nk) / nk).reshape(-1, 1)
        call = lambda: m.surface_spectral(k, om, ETA, fd, return_info=True)  # noqa: E731
    else:
        k = hp.quiet(m.cut_piece, 1, fd).k_uniform_mesh(mesh)
        call = lambda: m.surface_dos_mesh(mesh, om, ETA, fd)  # noqa: E731
    wall, ev, kern, out = timed(call)
    N = m.principal_layer(fd) * m._nsta
    if mesh is None:
        steps = float(out[1].mean())
    else:   # the steps of a sample of the mesh
        steps = float(m.surface_spectral(k[::max(1, nk // 64)], om, ETA, fd, return_info=True)[1].mean())
    dec = sum(v for kname, v in kern.items() if kname.startswith("sgf_") and kname not in ("sgf_blocks", "sgf_rows"))
    rib, why = ribbon_time(m, fd, k)
    rec = dict(case=name, N=N, nk=nk, nomega=nw, eta=ETA, wall_ms=round(wall, 2), event_ms=round(ev, 2), kernels_ms=kern,
               mean_steps=round(steps, 2), ns_per_problem_step=round(dec * 1e6 / (nk * nw * max(steps, 1.0)), 3),
               ribbon=rib, ribbon_missing=why, ratio_ribbon_over_decimation=(round(rib["wall_ms"] / wall, 3) if rib else None))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    for c in (sys.argv[1:] or ["haldane", "kane_mele", "cubic16", "random36"]):
        case(c)
