"""Time per Chebyshev step of tbk_kpm_apply_series (k_kpm_step with the series epilogue, nset coefficient sets) against the bare
step of tbk_kpm_moments (the same kernel with the dot-product epilogue) on the same periodic Haldane supercell of about 10^6
states (nvec = 8, 256 sparse products each),
and the traffic model of DESIGN.md section 23:

    bytes per step = nnz * 20 (value + column) + nsta * NV * 16 * (3 + 2 nset)
                     (the gather of T_m v counted once, T_m-1 v read, the write, and every accumulator read and written)

The two calls alternate in one process; kernel times are the library's per-launch event brackets (a call of its own each), wall
times per step come from unbracketed calls and include the launch gaps.  The tables and the upload are those of kpm_probe.py.

    python profiles/kpm_series_probe.py [--sizes 707] [--steps 256] [--sets 1,4] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import time

import numpy as np

from kpm_probe import COPY_RATE, NV, _lib, haldane_supercell_tables, moments, upload


def apply_series(sp, k, coeffs, bounds, n, nvec=NV, seed=1):
    out = np.empty((len(k), coeffs.shape[0], nvec, n), dtype=complex)
    _lib.check(_lib.lib.tbk_kpm_apply_series(sp, _lib.dptr(k), len(k), coeffs.shape[1], coeffs.shape[0], _lib.dptr(coeffs.view(float)),
                                             bounds[0], bounds[1], nvec, None, None, seed, _lib.dptr(out.view(float))))
    return out


def bracketed(ctx, call, name):
    ctx.prof_enable(1)
    ctx.prof_reset()
    call()
    rep = ctx.prof_report()
    ctx.prof_enable(0)
    ctx.prof_reset()
    return rep[name]["total_ms"] * 1e-3 / rep[name]["launches"], rep


def wall_per_step(long_call, short_call, steps):
    w0 = time.perf_counter()
    long_call()
    w1 = time.perf_counter()
    short_call()
    w2 = time.perf_counter()
    return ((w1 - w0) - (w2 - w1)) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="707")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--sets", default="1,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    k = np.array([[0.137, 0.731]])
    steps = a.steps
    rows = []
    for L in [int(s) for s in a.sizes.split(",")]:
        sp = upload(ctx, haldane_supercell_tables(L))
        n, nnz, g = C.c_int(0), C.c_int64(0), np.zeros(2)
        _lib.check(_lib.lib.tbk_sparse_info(sp, None, C.byref(n), C.byref(nnz), _lib.dptr(g)))
        pad = 0.01 * (g[1] - g[0])
        bnd = (g[0] - pad, g[1] + pad)
        rng = np.random.default_rng(1)
        nsets = [int(s) for s in a.sets.split(",")]
        table = (rng.standard_normal((max(nsets), steps + 1)) + 1j * rng.standard_normal((max(nsets), steps + 1))) / np.sqrt(steps + 1)
        calls = {"kpm_step": (lambda: moments(sp, k, 2 * steps, bnd), lambda: moments(sp, k, 2, bnd), steps - 1)}
        for ns in nsets:
            c, c2 = np.ascontiguousarray(table[:ns]), np.ascontiguousarray(table[:ns, :2])
            calls["kpm_series_step nset=%d" % ns] = (lambda c=c: apply_series(sp, k, c, bnd, n.value),
                                                     lambda c2=c2: apply_series(sp, k, c2, bnd, n.value), steps - 1)
        for long_call, short_call, _ in calls.values():           # warm-up: code objects, workspace
            short_call()
            long_call()
        kernel = {name: [] for name in calls}
        wall = {name: [] for name in calls}
        for _ in range(3):                                         # alternating
            for name, (long_call, short_call, nstep) in calls.items():
                t, _rep = bracketed(ctx, long_call, name.split()[0])
                kernel[name].append(t)
                wall[name].append(wall_per_step(long_call, short_call, nstep))
        for name in calls:
            ns = int(name.split("=")[1]) if "=" in name else 0
            model_bytes = nnz.value * 20 + n.value * NV * 16 * (3 + 2 * ns)
            tk_, tw = float(np.median(kernel[name])), float(np.median(wall[name]))
            row = dict(L=L, nsta=n.value, nnz=nnz.value, kernel=name, steps=steps, kernel_us_per_step=tk_ * 1e6,
                       kernel_us_runs=[t * 1e6 for t in kernel[name]], wall_us_per_step=tw * 1e6,
                       wall_us_runs=[t * 1e6 for t in wall[name]], model_bytes_per_step=model_bytes,
                       model_rate_kernel=model_bytes / tk_, fraction_of_copy_kernel=model_bytes / tk_ / COPY_RATE)
            rows.append(row)
            print(json.dumps(row), flush=True)
        _lib.check(_lib.lib.tbk_sparse_free(sp))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
