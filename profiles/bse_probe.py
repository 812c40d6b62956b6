#!/usr/bin/env python3
"""Time per Lanczos step and per application of the exciton operator (tb_model.exciton_spectrum_mesh) and,
beside it, one solve_all_mesh(eig_vectors=True) of the same mesh and one density_matrix_pairs_mesh call with the operator's triples
(which moves the selected eigenvectors once, where an application moves them twice).

Cases: spinless Haldane (n = 2, 1 x 1 bands) on 256 x 256 with a nearest-neighbour V = 1 (repulsive between electrons: attractive
between electron and hole); the w90 silicon model (n = 8, 4 x 4 bands) on 32 x 32 x 32 and the 4 x 4 Haldane supercell (n = 32,
8 x 8 bands) on 64 x 64 with V = 0.5 between neighbouring orbitals of the cell at R = 0.  Per case, in a fresh child process under
its own time limit: a warm-up, then WINDOWS windows, each timing a run of NT steps and a run of 2 NT steps of ONE Lanczos run
(dirs=(0, 0)): the time per step of a window is the difference over NT, so that the mesh solve, the setup and the copies cancel.
The time per application is the sum of the operator's four kernels per step from a separate run under the per-launch event
brackets.  One JSON line with the medians and the spread, the bytes one application moves by the count of section 37
(2 x 16 B x N n (nv + nc) + 3 x 16 B x N_t) and the rate that makes of the application time.

    python profiles/bse_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
import contextlib
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

_ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("haldane_256x256", "silicon_32x32x32", "haldane4x4_64x64")
WINDOWS, LIMIT_S = 5, 300
NT = {"haldane_256x256": 2048, "silicon_32x32x32": 1024, "haldane4x4_64x64": 512}      # steps of a window's short run: 0.1 s or more
NC = {"haldane_256x256": 32, "silicon_32x32x32": 16, "haldane4x4_64x64": 8}          # calls of a window of the two calls beside it
APPLY = ("bse_pair", "bse_rows", "bse_fields", "bse_project")


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
    if name == "haldane_256x256":
        m = hp.haldane(tb.tb_model, delta=0.7)
        return m, [256 // q, 256 // q], 1, dict(interaction=[(1.0, 0, 1, [0, 0]), (1.0, 1, 0, [1, 0]), (1.0, 1, 0, [0, 1])])
    if name == "silicon_32x32x32":
        m = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
        mesh, nb = [32 // q, 32 // q, 32 // q], 4
    else:
        m = quiet(hp.haldane(tb.tb_model, delta=0.7).make_supercell, [[4, 0], [0, 4]])
        mesh, nb = [64 // q, 64 // q], 8
    zero = [0] * m._dim_r
    return m, mesh, nb, dict(interaction=[(0.5, o, o + 1, zero) for o in range(m._nsta - 1)], valence=nb, conduction=nb)


def child(name, quick):
    m, mesh, nb, kw = build(name, quick)
    from pythtb_amd import _lib
    n, nk = m._nsta, int(np.prod(mesh))
    nocc = n // 2
    kw["fermi_level"] = float(np.ravel(m.fermi_level_mesh(mesh, float(nocc)))[0])

    def run(nt):
        t = time.perf_counter()
        res = m.exciton_spectrum_mesh(mesh, omega=[1.0], eta=0.1, dirs=(0, 0), n_steps=nt, **kw)
        return time.perf_counter() - t, res

    nt, nc = NT[name], NC[name]
    run(2), run(2)
    ab, Rs, _ = m._mf_entries("exciton_spectrum_mesh", kw["interaction"], None)
    pairs = [(int(a), int(b), R) for (a, b), R in zip(ab, Rs)] + [(int(b), int(a), -R) for (a, b), R in zip(ab, Rs)]
    pairs += [(int(a), int(a), None) for a in sorted(set(ab.reshape(-1).tolist()))]

    def solve(calls):
        t = time.perf_counter()
        for _ in range(calls):
            m.solve_all_mesh(mesh, eig_vectors=True)
        return (time.perf_counter() - t) / calls

    def selected(calls):
        t = time.perf_counter()
        for _ in range(calls):
            m.density_matrix_pairs_mesh(mesh, kw["fermi_level"], 0.0, pairs)
        return (time.perf_counter() - t) / calls

    solve(1), selected(2)
    per, so, se = [], [], []
    for _ in range(WINDOWS):
        t1, t2 = run(nt)[0], run(2 * nt)[0]
        per.append((t2 - t1) / nt)
        so.append(solve(max(1, nc // 8)))
        se.append(selected(nc))
    ctx = _lib.default_context()
    ctx.prof_reset()
    ctx.prof_enable(1)
    run(16)
    kern = {k: round(v["total_ms"] / 16.0, 4) for k, v in ctx.prof_report().items() if k.startswith("bse_")}
    ctx.prof_enable(0)
    apply_ms = sum(kern.get(k, 0.0) for k in APPLY)
    nt_all = nk * nb * nb
    moved = 2 * 16 * nk * n * 2 * nb + 3 * 16 * nt_all
    ms = lambda v: round(1e3 * float(np.median(v)), 4)
    print(json.dumps({"case": name, "mesh": mesh, "nsta": n, "bands": [nb, nb], "transitions": nt_all, "sums": len(pairs), "nt": nt,
                      "window_s": round(float(np.median(per)) * nt, 4), "lanczos_step_ms": ms(per),
                      "lanczos_step_ms_min_max": [round(1e3 * min(per), 4), round(1e3 * max(per), 4)], "application_kernels_ms": round(apply_ms, 4),
                      "application_bytes": moved, "application_GB_per_s": round(moved / (apply_ms * 1e-3) / 1e9, 1) if apply_ms else None,
                      "solve_all_mesh_vectors_ms": ms(so), "density_matrix_pairs_mesh_ms": ms(se), "kernel_ms_per_step": kern}), flush=True)


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
