#!/usr/bin/env python3
"""Per-call wall time and per-kernel times (tbk_prof_*) of quantum_geometric_tensor_mesh on the cases
of berry_curvature_probe.py, whose curv2_plane / curv_lds brackets are the yardstick: Haldane 2048^2 (n = 2), Kane-Mele
4096 x 512 with occ = [0, 1], cubic16 per band on 64^3, the Haldane 4 x 4 supercell on 256^2 (n = 32) and w90 silicon on
48^3.  Prints one JSON line per case.

Without --case every case runs in a child process of its own under its own time limit, one after the other, and the first
one that fails (or runs out of time) ends the probe: nothing more is started on the device behind a failure."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

_HERE = os.path.abspath(__file__)
_ROOT = os.path.join(os.path.dirname(_HERE), "..")
CASES = {   # name: (repetitions, time limit in seconds)
    "haldane_2048^2_occ0": (10, 120),
    "haldane_2048^2_per_band": (10, 120),
    "kane_mele_4096x512_occ01": (3, 180),
    "cubic16_64^3_per_band": (2, 180),
    "haldane_4x4_256^2_occ16": (2, 180),
    "silicon_48^3_occ4": (2, 180),
}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def run_case(name):
    sys.path.insert(0, _ROOT)
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import pythtb_amd as tb
    import helpers as hp
    from pythtb_amd import _lib, w90

    hal = hp.haldane(tb.tb_model, 0.2)
    if name == "haldane_2048^2_occ0":
        fn = lambda: hal.quantum_geometric_tensor_mesh([2048, 2048], occ=[0])   # noqa: E731
    elif name == "haldane_2048^2_per_band":
        fn = lambda: hal.quantum_geometric_tensor_mesh([2048, 2048])   # noqa: E731
    elif name == "kane_mele_4096x512_occ01":
        km = hp.kane_mele(tb.tb_model)
        fn = lambda: km.quantum_geometric_tensor_mesh([4096, 512], occ=[0, 1])   # noqa: E731
    elif name == "cubic16_64^3_per_band":
        cub = hp.cubic16(tb.tb_model)
        fn = lambda: cub.quantum_geometric_tensor_mesh([64, 64, 64])   # noqa: E731
    elif name == "haldane_4x4_256^2_occ16":
        sc4 = quiet(hal.make_supercell, [[4, 0], [0, 4]])
        fn = lambda: sc4.quantum_geometric_tensor_mesh([256, 256], occ=list(range(16)))   # noqa: E731
    else:
        si = quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model)
        fn = lambda: si.quantum_geometric_tensor_mesh([48, 48, 48], occ=[0, 1, 2, 3])   # noqa: E731
    reps = CASES[name][0]
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=list(CASES))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        sys.exit(0)
    for name, (_, limit) in CASES.items():
        try:
            rc = subprocess.run([sys.executable, _HERE, "--case", name], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(case=name, failed=rc)), flush=True)
            sys.exit(rc if rc > 0 else 1)
