#!/usr/bin/env python3
"""Time per step of tb_model.propagate_mesh beside its floor: every step holds one eigen-solve with
eigenvectors of the shifted mesh, so one such solve of the same mesh -- generated and solved on the device in the same chunks, nothing
downloaded, what solve_all_mesh(..., eig_vectors=True) does before its copy -- is the least a step can take.

Cases: Haldane (n = 2, the lower band) on 256 x 256, the w90 silicon model (n = 8, four bands) on 32 x 32 x 32, and the 4 x 4 Haldane
supercell (n = 32, 16 bands) on 64 x 64.  Per case, in a fresh child process under its own time limit: after a warm-up, WINDOWS windows,
each timing a run of NT steps, a run of 2 NT steps and NT chunked solves, interleaved (NT per case, so that a window lasts 0.1 s or
more); the time per step of a window is the difference of the two runs over NT (the start, the first measurement and the copies
cancel).  One JSON line per case with the medians over the windows, the spread, and the ratio of a step to the solve; then, from a
separate run of 16 steps under the per-launch event brackets (tbk_prof_*), the kernel time per step by label.

    python profiles/td_probe.py [--quick]      (--quick: meshes of a quarter of the points per axis)"""
import contextlib
import ctypes as C
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
STEPS = {"haldane_256x256": 4096, "silicon_32x32x32": 256, "haldane4x4_64x64": 64}   # steps of a window's short run: 0.1 s or more


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build(name):
    sys.path.insert(0, _ROOT)
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import pythtb_amd as tb
    import helpers as hp
    from pythtb_amd import w90
    hal = hp.haldane(tb.tb_model, delta=0.2)
    if name == "haldane_256x256":
        return hal, [256, 256], [0]
    if name == "silicon_32x32x32":
        return quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model), [32, 32, 32], list(range(4))
    return quiet(hal.make_supercell, [[4, 0], [0, 4]]), [64, 64], list(range(16))


def solver(m, mesh):
    """A function that generates and solves the mesh on the device in the chunks of the propagation, and waits for it."""
    from pythtb_amd import _lib
    lib, ctx = _lib.lib, _lib.default_context()
    n, dk = m._nsta, m._dim_k
    nk = int(np.prod(mesh))
    chunk = min(max(1, (32 << 20) // (n * n * 16)), nk)                     # kubo_chunk_len
    bufs = []
    for nbytes in (chunk * dk * 8, chunk * n * 8, chunk * n * n * 16):
        p = C.c_void_p()
        _lib.check(lib.tbk_dev_alloc(ctx.handle, nbytes, C.byref(p)))
        bufs.append(p)
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    h = m._device_model()

    def run():
        for first in range(0, nk, chunk):
            cnt = min(chunk, nk - first)
            _lib.check(lib.tbk_k_uniform_mesh_range_dev(ctx.handle, dk, _lib.iptr(mesh32), first, cnt, bufs[0]))
            _lib.check(lib.tbk_solve_list_dev_checked(h, bufs[0], cnt, bufs[1], bufs[2]))
        ctx.sync()
    return run


def child(name, quick):
    m, mesh, occ = build(name)
    if quick:
        mesh = [max(2, x // 4) for x in mesh]
    from pythtb_amd import _lib
    ctx = _lib.default_context()
    dk = m._dim_k
    NT = REPS = STEPS[name]
    t = np.arange(2 * NT + 1) * 0.05
    amp = np.array([0.05, 0.05j, 0.0][:dk]) if dk > 1 else np.array([0.05])
    kap = m.laser_shift(t, amp, 3.0, envelope="flat")
    solve = solver(m, mesh)

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()                                                                 # (both end in a device synchronisation)
        return (time.perf_counter() - t0) * 1e3

    short = lambda: m.propagate_mesh(mesh, kap[:NT + 1], 0.05, occ=occ)
    long_ = lambda: m.propagate_mesh(mesh, kap, 0.05, occ=occ)
    many = lambda: [solve() for _ in range(REPS)]
    for fn in (short, long_, many):                                          # warm-up: upload, scratch growth, code objects
        fn()
    step, sol = [], []
    for _ in range(WINDOWS):
        a, b, s = timed(short), timed(long_), timed(many)
        step.append((b - a) / NT)
        sol.append(s / REPS)
    rec = dict(case=name, n=m._nsta, mesh=list(mesh), nprop=len(occ), steps_timed=NT, windows=WINDOWS,
               step_ms_median=round(float(np.median(step)), 4), step_ms_min=round(min(step), 4), step_ms_max=round(max(step), 4),
               solve_ms_median=round(float(np.median(sol)), 4), solve_ms_min=round(min(sol), 4), solve_ms_max=round(max(sol), 4))
    rec["step_over_solve"] = round(rec["step_ms_median"] / rec["solve_ms_median"], 3)
    print(json.dumps(rec), flush=True)
    ctx.prof_reset()
    ctx.prof_enable(1)
    m.propagate_mesh(mesh, kap[:17], 0.05, occ=occ)
    ctx.sync()
    kern = {k: round(v["total_ms"] / 16.0, 4) for k, v in ctx.prof_report().items()}
    ctx.prof_enable(0)
    print(json.dumps(dict(case=name, kernel_ms_per_step=kern)), flush=True)


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    if "--case" in sys.argv:
        child(sys.argv[sys.argv.index("--case") + 1], quick)
        sys.exit(0)
    bad = 0
    for name in CASES:                                                       # a fresh process and a time limit per GPU step
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name] + (["--quick"] if quick else [])
        try:
            rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(case=name, failed=rc)), flush=True)
            bad = 1
            break                                                            # nothing more on the GPU after a failure
    sys.exit(bad)
