#!/usr/bin/env python3
"""Times of tb_model.wannier_mesh: the projection-only call (max_iter = 0) and the time per iteration of the
descent, beside one solve_all_mesh(eig_vectors=True) of the same mesh (which the call contains, minus the download of the vectors).

Cases: Haldane in its trivial phase (delta = 0.7, t2 = 0.1) on 256 x 256, the lower band; the w90 silicon model (8 states) on
32 x 32 x 32, the four valence bands; the 4 x 4 supercell of the same Haldane model (32 states) on 64 x 64, the sixteen lower bands.
The trial functions are the nw dominant eigenvectors of the occupied-state projector at R = 0 (density_matrix_mesh at mid-gap): local,
and never orthogonal to the bands.  The hopping table is asked for on the lattice vectors with |R_a| <= 1 only, so that the Fourier
sum and the Python table do not enter.  Per case, in a fresh child process under its own time limit: a warm-up, then WINDOWS windows,
each timing solve_all_mesh, the projection-only call (both repeated until 0.1 s have passed), a run of NT iterations and a run of
2 NT iterations; the time per iteration of a window is the difference of the two runs over NT (solve, projection, model and copies
cancel).  One JSON line each with the medians and the spread; then the kernel time by label from a run under the event brackets.

    python profiles/wannier_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
import contextlib
import io
import itertools
import json
import os
import subprocess
import sys
import time

import numpy as np

_ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("haldane_256x256", "silicon_32x32x32", "haldane4x4_64x64")
WINDOWS, LIMIT_S = 5, 300
NT = {"haldane_256x256": 192, "silicon_32x32x32": 64, "haldane4x4_64x64": 64}       # iterations of a window's short run: 0.1 s or more


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(name, quick):
    sys.path.insert(0, _ROOT)
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import pythtb_amd as tb
    import helpers as hp
    from pythtb_amd import w90
    hal = hp.haldane(tb.tb_model, delta=0.7, t2abs=0.1)
    q = 4 if quick else 1
    if name == "haldane_256x256":
        return hal, [256 // q, 256 // q], 1
    if name == "silicon_32x32x32":
        return quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model), [32 // q, 32 // q, 32 // q], 4
    return quiet(hal.make_supercell, [[4, 0], [0, 4]]), [64 // q, 64 // q], 16


def repeat(fn):
    """Seconds per call of fn, over as many calls as 0.1 s hold (at least one)."""
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= 0.1:
            return dt / n, dt


def child(name, quick):
    m, mesh, nw = build(name, quick)
    from pythtb_amd import _lib
    n, dk = m._nsta, m._dim_k
    coarse = [max(3, x // 4) for x in mesh]
    mu = m.fermi_level_mesh(coarse, float(nw))
    P = np.array(m.density_matrix_mesh(coarse, mu)).reshape(n, n)
    val, vec = np.linalg.eigh(P)
    trial = vec[:, -nw:]
    bands = list(range(nw))
    R = [list(r) for r in itertools.product((-1, 0, 1), repeat=dk)]

    def run(nt):
        t = time.perf_counter()
        res = m.wannier_mesh(mesh, trial, bands, max_iter=nt, check_every=max(nt, 1), R_list=R)
        return time.perf_counter() - t, res

    nt = NT[name]
    try:
        m._wannier_bvectors(np.array(mesh, dtype=np.int32))
    except Exception as e:                                           # (an fcc lattice: the closed-form star has a zero weight)
        print(json.dumps({"case": name, "not_measured": " ".join(str(e).split())}), flush=True)
        return 0
    run(2), m.solve_all_mesh(mesh, eig_vectors=True)
    per, proj, solve, short = [], [], [], []
    res = None
    for _ in range(WINDOWS):
        s, ws = repeat(lambda: m.solve_all_mesh(mesh, eig_vectors=True))
        p, wp = repeat(lambda: run(0))
        t1, _ = run(nt)
        t2, res = run(2 * nt)
        solve.append(s), proj.append(p), per.append((t2 - t1) / nt), short.append(min(ws, wp, t1))
    med = lambda v: round(1e3 * float(np.median(v)), 4)
    rng = lambda v: [round(1e3 * min(v), 4), round(1e3 * max(v), 4)]
    print(json.dumps({"case": name, "mesh": mesh, "nsta": n, "nw": nw, "nt": nt, "shortest_window_s": round(min(short), 4),
                      "solve_all_mesh_vectors_ms": med(solve), "solve_min_max": rng(solve), "projection_call_ms": med(proj),
                      "projection_min_max": rng(proj), "iteration_ms": med(per), "iteration_min_max": rng(per), "sv_min": res.sv_min,
                      "omega_projection": float(res.history[0]), "omega_after_%d" % (2 * nt): res.omega}), flush=True)
    ctx = _lib.default_context()
    ctx.prof_reset()
    ctx.prof_enable(1)
    run(16)
    rep = ctx.prof_report()
    ctx.prof_enable(0)
    kern = {k: round(v["total_ms"] / (16.0 if k in ("wan_step",) else 17.0 if k == "wan_spread" else 1.0), 4) for k, v in rep.items()}
    print(json.dumps({"case": name, "kernel_ms (per iteration: wan_step, wan_spread; per call: the rest)": kern}), flush=True)


def main():
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        return child(sys.argv[sys.argv.index("--child") + 1], quick)
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + (["--quick"] if quick else [])
        try:
            r = subprocess.run(cmd, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": name, "error": "time limit"}), flush=True)
            return 1
        if r.returncode != 0:                                        # nothing more on the device after a failure
            print(json.dumps({"case": name, "error": "exit status %d" % r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
