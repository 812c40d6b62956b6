#!/usr/bin/env python3
"""Time per iteration of tb_model.bdg_mesh and, beside it, the whole-matrix density stage the pair stage
replaces: density_matrix_mesh(res.model, 0, kT, R_list) of the same mesh -- one eigen-solve with vectors of the Nambu model and
occ_dm_stage over its nR (2 nsta)^2 entries -- and density_matrix_pairs_mesh of the triples the loop consumes.

Cases: spinful Haldane (n = 4, Nambu 8) on 256 x 256 with U = -2; the w90 silicon model (n = 8, Nambu 16) on 32 x 32 x 32 and the
4 x 4 Haldane supercell (n = 32, Nambu 64) on 64 x 64 with an attraction of -0.5 between neighbouring orbitals of the cell at
R = 0 (o, o + 1); Hartree and pairing, kT = 0.05, 0.4 electrons per state, Anderson mixing over 4 pairs.  Per case, in a fresh child
process under its own time limit: a warm-up, then WINDOWS windows, each timing a run of NT iterations and a run of 2 NT iterations
(the time per iteration of a window is the difference over NT: upload, final scan and copies cancel) and NC calls of each of the two
density calls on the Nambu model of the result.  One JSON line with the medians and the spread; then, from a separate run of 16
iterations under the per-launch event brackets, the kernel time per iteration by label.

    python profiles/bdg_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
import contextlib
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

_ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("haldane_spinful_256x256", "silicon_32x32x32", "haldane4x4_64x64")
WINDOWS, LIMIT_S = 5, 300
NT = {"haldane_spinful_256x256": 320, "silicon_32x32x32": 96, "haldane4x4_64x64": 24}      # iterations of a window's short run: 0.1 s or more
NC = {"haldane_spinful_256x256": 64, "silicon_32x32x32": 32, "haldane4x4_64x64": 8}        # density calls of a window


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(name, quick):
    sys.path.insert(0, _ROOT)
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import pythtb_amd as tb
    import helpers as hp
    from pythtb_amd import w90
    q = 4 if quick else 1
    if name == "haldane_spinful_256x256":
        m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=2)
        m.set_onsite([-0.2, 0.2])
        for amp, i, j, R in ((-1.0, 0, 1, [0, 0]), (-1.0, 1, 0, [1, 0]), (-1.0, 1, 0, [0, 1]), (0.15j, 0, 0, [1, 0]), (0.15j, 1, 1, [1, -1]),
                             (0.15j, 1, 1, [0, 1]), (-0.15j, 1, 1, [1, 0]), (-0.15j, 0, 0, [1, -1]), (-0.15j, 0, 0, [0, 1])):
            m.set_hop(amp, i, j, R)
        return m, [256 // q, 256 // q], dict(U=-2.0)
    if name == "silicon_32x32x32":
        m = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
        mesh = [32 // q, 32 // q, 32 // q]
    else:
        m = quiet(hp.haldane(tb.tb_model, delta=0.2).make_supercell, [[4, 0], [0, 4]])
        mesh = [64 // q, 64 // q]
    zero = [0] * m._dim_r
    return m, mesh, dict(interaction=[(-0.5, o, o + 1, zero) for o in range(m._nsta - 1)])


def child(name, quick):
    m, mesh, inter = build(name, quick)
    from pythtb_amd import _lib
    n, kT = m._nsta, 0.05
    kw = dict(inter, n_electrons=0.4 * n, kT=kT, mixing=0.5, history=4, tol=0.0)

    def run(nt):
        t = time.perf_counter()
        res = m.bdg_mesh(mesh, max_iter=nt, check_every=nt, **kw)
        return time.perf_counter() - t, res

    nt, nc = NT[name], NC[name]
    res = run(2)[1]
    run(2)
    nambu = res.model
    ab, Rs, _ = m._mf_entries("bdg_mesh", inter.get("interaction"), inter.get("U"))
    Rl = np.unique(np.vstack([np.zeros((1, m._dim_k), dtype=np.int32), Rs]), axis=0)
    pairs = [(a, a, None) for a in range(n)] + [(int(a), n + int(b), R) for (a, b), R in zip(ab, Rs)]

    def whole(calls):
        t = time.perf_counter()
        for _ in range(calls):
            nambu.density_matrix_mesh(mesh, 0.0, kT, Rl)
        return (time.perf_counter() - t) / calls

    def selected(calls):
        t = time.perf_counter()
        for _ in range(calls):
            nambu.density_matrix_pairs_mesh(mesh, 0.0, kT, pairs)
        return (time.perf_counter() - t) / calls

    whole(2), selected(2)
    per, wh, se = [], [], []
    for _ in range(WINDOWS):
        t1, t2 = run(nt)[0], run(2 * nt)[0]
        per.append((t2 - t1) / nt)
        wh.append(whole(nc))
        se.append(selected(nc))
    ms = lambda v: round(1e3 * float(np.median(v)), 4)
    out = {"case": name, "mesh": mesh, "nsta": n, "nambu": 2 * n, "triples": len(pairs), "nR": int(len(Rl)), "nt": nt,
           "window_s": round(float(np.median(per)) * nt, 4), "iteration_ms": ms(per),
           "iteration_ms_min_max": [round(1e3 * min(per), 4), round(1e3 * max(per), 4)],
           "density_matrix_mesh_ms": ms(wh), "density_matrix_mesh_ms_min_max": [round(1e3 * min(wh), 4), round(1e3 * max(wh), 4)],
           "density_matrix_pairs_mesh_ms": ms(se), "density_matrix_pairs_mesh_ms_min_max": [round(1e3 * min(se), 4), round(1e3 * max(se), 4)]}
    print(json.dumps(out), flush=True)
    ctx = _lib.default_context()
    for label, fn in (("bdg_mesh", lambda: run(16)), ("density_matrix_mesh", lambda: whole(16)), ("density_matrix_pairs_mesh", lambda: selected(16))):
        ctx.prof_reset()
        ctx.prof_enable(1)
        fn()
        kern = {k: round(v["total_ms"] / 16.0, 4) for k, v in ctx.prof_report().items()}
        ctx.prof_enable(0)
        print(json.dumps({"case": name, "call": label, "kernel_ms_per_iteration_or_call": kern}), flush=True)


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
