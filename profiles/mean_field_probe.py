#!/usr/bin/env python3
"""Time per iteration of tb_model.mean_field_mesh beside the same iteration written with the public calls it
replaces (set_onsite, fermi_level_mesh, density_matrix_mesh at R = 0 -- two eigen-solves, one flatten and upload, two round trips).

Cases: Haldane (n = 2) on 256 x 256, the w90 silicon model (n = 8) on 32 x 32 x 32, the 4 x 4 Haldane supercell (n = 32) on 64 x 64;
the interaction couples neighbouring orbitals of the cell at R = 0 (o, o + 1), strength 0.5, kT = 0.05, half filling.  Variants:
Hartree only (fock=False; the public-call loop is timed beside it) and with the Fock term on the same bonds, each in the resident and
(TBK_MF_RESIDENT_MAX=1) the two-pass form.  Per (case, variant), in a fresh child process under its own time limit: a warm-up, then
WINDOWS windows, each timing a run of NT iterations, a run of 2 NT iterations and -- Hartree only -- NT iterations of the public-call
loop, interleaved; the time per iteration of a window is the difference of the two runs over NT (upload, start pass, final scan and
copies cancel).  One JSON line each with the medians, the spread and the ratio; then, from a separate run of 16 iterations under the
per-launch event brackets, the kernel time per iteration by label.

    python profiles/mean_field_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
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
VARIANTS = ("hartree_resident", "hartree_twopass", "fock_resident", "fock_twopass")
WINDOWS, LIMIT_S = 5, 300
NT = {"haldane_256x256": 256, "silicon_32x32x32": 192, "haldane4x4_64x64": 64}      # iterations of a window's short run: 0.1 s or more


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(name, quick):
    sys.path.insert(0, _ROOT)
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import pythtb_amd as tb
    import helpers as hp
    from pythtb_amd import w90
    hal = hp.haldane(tb.tb_model, delta=0.2)
    q = 4 if quick else 1
    if name == "haldane_256x256":
        return hal, [256 // q, 256 // q]
    if name == "silicon_32x32x32":
        return quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model), [32 // q, 32 // q, 32 // q]
    return quiet(hal.make_supercell, [[4, 0], [0, 4]]), [64 // q, 64 // q]


def child(name, variant, quick):
    m, mesh = build(name, quick)
    from pythtb_amd import _lib
    n, kT, V = m._nsta, 0.05, 0.5
    nel = n / 2.0
    zero = [0] * m._dim_r
    inter = [(V, o, o + 1, zero) for o in range(n - 1)]
    fock = variant.startswith("fock")
    start = 0.5 + 0.1 * np.cos(np.arange(float(n)))
    base = np.array(m._site_energies, dtype=float).copy()

    def run(nt):
        t = time.perf_counter()
        m.mean_field_mesh(mesh, inter, n_electrons=nel, kT=kT, start=start, fock=fock, mixing=0.5, history=4, tol=0.0, max_iter=nt,
                          check_every=nt)
        return time.perf_counter() - t

    def public(nt):
        occ = start.copy()
        t = time.perf_counter()
        for _ in range(nt):
            eps = base.copy()
            eps[:-1] += V * occ[1:]
            eps[1:] += V * occ[:-1]
            m.set_onsite(list(eps), mode="reset")
            mu = m.fermi_level_mesh(mesh, nel, kT=kT)
            occ = 0.5 * occ + 0.5 * np.real(np.diagonal(m.density_matrix_mesh(mesh, mu, kT)))
        dt = time.perf_counter() - t
        m.set_onsite(list(base), mode="reset")
        return dt

    nt = NT[name]
    run(2), run(2)
    if not fock:
        public(2)
    per, pub = [], []
    for _ in range(WINDOWS):
        t1, t2 = run(nt), run(2 * nt)
        per.append((t2 - t1) / nt)
        if not fock:
            pub.append(public(nt) / nt)
    out = {"case": name, "variant": variant, "mesh": mesh, "nsta": n, "nt": nt, "window_s": round(float(np.median(per)) * nt, 4),
           "iteration_ms": round(1e3 * float(np.median(per)), 4), "iteration_ms_min_max": [round(1e3 * min(per), 4), round(1e3 * max(per), 4)]}
    if pub:
        out["public_calls_ms"] = round(1e3 * float(np.median(pub)), 4)
        out["ratio_public_over_driver"] = round(float(np.median(pub)) / float(np.median(per)), 3)
    print(json.dumps(out), flush=True)
    ctx = _lib.default_context()
    ctx.prof_reset()
    ctx.prof_enable(1)
    run(16)
    kern = {k: round(v["total_ms"] / 16.0, 4) for k, v in ctx.prof_report().items()}
    ctx.prof_enable(0)
    print(json.dumps({"case": name, "variant": variant, "kernel_ms_per_iteration": kern}), flush=True)


def main():
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        return child(sys.argv[i + 1], sys.argv[i + 2], quick)
    for name in CASES:
        for variant in VARIANTS:
            env = dict(os.environ)
            if variant.endswith("twopass"):
                env["TBK_MF_RESIDENT_MAX"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, variant] + (["--quick"] if quick else [])
            try:
                r = subprocess.run(cmd, env=env, timeout=LIMIT_S)
            except subprocess.TimeoutExpired:
                print(json.dumps({"case": name, "variant": variant, "error": "time limit"}), flush=True)
                return 1
            if r.returncode != 0:                                    # nothing more on the device after a failure
                print(json.dumps({"case": name, "variant": variant, "error": "exit status %d" % r.returncode}), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
