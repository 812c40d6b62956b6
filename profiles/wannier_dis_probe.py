#!/usr/bin/env python3
"""Times of tb_model.wannier_disentangle_mesh: the time per disentanglement iteration beside the time per
iteration of section 34's descent in the same call and beside one solve_all_mesh(eig_vectors=True) of the same mesh.

Cases: the 4 x 4 supercell of the trivial Haldane model (32 states) on 64 x 64, 8 functions from the 16 lower bands, no windows;
the w90 silicon model (8 states, fcc) on 32 x 32 x 32 through b_vectors="shells", 4 functions from all 8 bands with the valence bands
frozen (the frozen window ends in the middle of the gap of the mesh).  The trial functions are the nw dominant eigenvectors of the
occupied-state projector at R = 0 (density_matrix_mesh, the Fermi level at nw electrons): local, and never orthogonal to the low
bands.  The hopping table is asked for on the lattice vectors with |R_a| <= 1 only.  Per case, in a fresh child process under its own
time limit: a warm-up, then WINDOWS windows, each timing solve_all_mesh (repeated until 0.1 s have passed), the calls with
(dis_iter, max_iter) = (NT, 0), (2 NT, 0) and (NT, NT); the time per disentanglement iteration of a window is the difference of the
first two over NT, the time per descent iteration the difference of the third and the first over NT (solve, overlaps, start, gauge,
model and copies cancel).  One JSON line each with the medians and the spread; then the kernel time by label from a run under the
event brackets.

    python profiles/wannier_dis_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
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
CASES = ("haldane4x4_64x64", "silicon_32x32x32")
WINDOWS, LIMIT_S = 5, 300
NT = {"haldane4x4_64x64": 32, "silicon_32x32x32": 32}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(name, quick):
    """(model, mesh, nw, bands, keywords of the call)."""
    sys.path.insert(0, _ROOT)
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import pythtb_amd as tb
    import helpers as hp
    from pythtb_amd import w90
    q = 4 if quick else 1
    if name == "haldane4x4_64x64":
        hal = hp.haldane(tb.tb_model, delta=0.7, t2abs=0.1)
        return quiet(hal.make_supercell, [[4, 0], [0, 4]]), [64 // q, 64 // q], 8, list(range(16)), {}
    m = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
    mesh = [32 // q, 32 // q, 32 // q]
    ev = m.solve_all_mesh(mesh)
    ev = np.asarray(ev).reshape(m._nsta, -1)
    top, bottom = ev[3].max(), ev[4].min()
    kw = dict(b_vectors="shells")
    if bottom > top:                                               # the valence bands frozen: the window ends in the gap of the mesh
        kw["frozen"] = (float(ev.min()) - 1.0, 0.5 * float(top + bottom))
    return m, mesh, 4, list(range(8)), kw


def repeat(fn):
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= 0.1:
            return dt / n, dt


def child(name, quick):
    m, mesh, nw, bands, kw = build(name, quick)
    from pythtb_amd import _lib
    n, dk = m._nsta, m._dim_k
    coarse = [max(3, x // 4) for x in mesh]
    mu = m.fermi_level_mesh(coarse, float(nw))
    P = np.array(m.density_matrix_mesh(coarse, mu)).reshape(n, n)
    val, vec = np.linalg.eigh(P)
    trial = vec[:, -nw:]
    R = [list(r) for r in itertools.product((-1, 0, 1), repeat=dk)]

    def run(nd, nt):
        t = time.perf_counter()
        res = m.wannier_disentangle_mesh(mesh, trial, bands, dis_iter=nd, max_iter=nt, check_every=max(nd, nt, 1), R_list=R, **kw)
        return time.perf_counter() - t, res

    nt = NT[name]
    run(2, 2), m.solve_all_mesh(mesh, eig_vectors=True)
    dis, des, solve, base = [], [], [], []
    res = None
    for _ in range(WINDOWS):
        s, _w = repeat(lambda: m.solve_all_mesh(mesh, eig_vectors=True))
        t1, _r = run(nt, 0)
        t2, res = run(2 * nt, 0)
        t3, _r = run(nt, nt)
        solve.append(s), base.append(t1), dis.append((t2 - t1) / nt), des.append((t3 - t1) / nt)
    med = lambda v: round(1e3 * float(np.median(v)), 4)
    rng = lambda v: [round(1e3 * min(v), 4), round(1e3 * max(v), 4)]
    print(json.dumps({"case": name, "mesh": mesh, "nsta": n, "nb": len(bands), "nw": nw, "nbv": len(res.b_weights), "nt": nt,
                      "frozen": list(kw.get("frozen", ())), "n_frozen_min_max": [int(res.n_frozen.min()), int(res.n_frozen.max())],
                      "solve_all_mesh_vectors_ms": med(solve), "solve_min_max": rng(solve), "call_with_%d_iterations_ms" % nt: med(base),
                      "dis_iteration_ms": med(dis), "dis_iteration_min_max": rng(dis), "descent_iteration_ms": med(des),
                      "descent_iteration_min_max": rng(des), "sv_min": res.sv_min, "dis_gap_min": res.dis_gap_min,
                      "omega_i_start": float(res.dis_history[0]), "omega_i_after_%d" % (2 * nt): float(res.dis_history[-1])}), flush=True)
    ctx = _lib.default_context()
    ctx.prof_reset()
    ctx.prof_enable(1)
    run(16, 0)
    rep = ctx.prof_report()
    ctx.prof_enable(0)
    kern = {k: round(v["total_ms"] / (16.0 if k == "wdis_step" else 1.0), 4) for k, v in rep.items()}
    print(json.dumps({"case": name, "kernel_ms (per iteration: wdis_step; per call: the rest)": kern}), flush=True)


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
