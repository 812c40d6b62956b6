"""Time per Chebyshev step of tbk_kpm_moments on periodic Haldane supercells of about 2 10^3, 10^5 and 2 10^6 states
(nvec = 8, M = 512: 256 sparse products), against the traffic model of DESIGN.md section 21:

    bytes per step = nnz * 20 (value + column) + nsta * NV * 16 * 3 (the gather of alpha_m counted once, alpha_m-1 read, the write)

The tables are built with NumPy (a model of 10^6 cells does not go through set_hop) and handed to tbk_sparse_upload directly.
Two figures per size: the kernel time of k_kpm_step from the library's per-launch event brackets (a call of its own), and the
wall time per step of an unbracketed call, which includes the launch gaps.  Past the 256 MiB cache the rate is also given as a
fraction of the measured plain-copy rate of the device, 6.29 TB/s (float4 copy).

At L = --double-size (224) one more figure: the wall time of a whole tbk_kpm_double_moments call with
--double-moments (64) moments, 8 vectors, one k, directions (0, 1).

    python profiles/kpm_probe.py [--sizes 32,224,1000] [--moments 512] [--double-size 224] [--double-moments 64] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pythtb_amd import _lib  # noqa: E402

COPY_RATE = 6.29e12
NV = 8


def haldane_supercell_tables(L, delta=0.2, t=-1.0, t2abs=0.15):
    """tables of the L x L supercell of the Haldane model (dim_k = 2, 2 L^2 orbitals, 9 L^2 hops)"""
    x, y = [a.reshape(-1) for a in np.meshgrid(np.arange(L), np.arange(L), indexing="ij")]
    cell = lambda cx, cy: (cx % L) * L + (cy % L)
    tau = np.array([[1.0 / 3.0, 1.0 / 3.0], [2.0 / 3.0, 2.0 / 3.0]])
    orb = np.empty((L * L, 2, 2))
    for o in range(2):
        orb[:, o, 0] = (x + tau[o, 0]) / L
        orb[:, o, 1] = (y + tau[o, 1]) / L
    onsite = np.zeros((L * L, 2), dtype=complex)
    onsite[:, 0], onsite[:, 1] = -delta, delta
    t2 = t2abs * 1j
    hops = [(t, 0, 1, 0, 0), (t, 1, 0, 1, 0), (t, 1, 0, 0, 1), (t2, 0, 0, 1, 0), (t2, 1, 1, 1, -1), (t2, 1, 1, 0, 1),
            (t2.conjugate(), 1, 1, 1, 0), (t2.conjugate(), 0, 0, 1, -1), (t2.conjugate(), 0, 0, 0, 1)]
    hi, hj, hR, ha = [], [], [], []
    for amp, i, j, dx, dy in hops:
        hi.append(2 * cell(x, y) + i)
        hj.append(2 * cell(x + dx, y + dy) + j)
        hR.append(np.stack([(x + dx) // L, (y + dy) // L], axis=1))
        ha.append(np.full(L * L, amp, dtype=complex))
    return dict(orb=np.ascontiguousarray(orb.reshape(-1, 2)), onsite=np.ascontiguousarray(onsite.reshape(-1)),
                hop_i=np.ascontiguousarray(np.concatenate(hi), dtype=np.int32), hop_j=np.ascontiguousarray(np.concatenate(hj), dtype=np.int32),
                hop_R=np.ascontiguousarray(np.concatenate(hR), dtype=np.int32), hop_amp=np.ascontiguousarray(np.concatenate(ha)))


def upload(ctx, t):
    h = C.c_void_p()
    _lib.check(_lib.lib.tbk_sparse_upload(ctx.handle, 2, len(t["orb"]), 1, _lib.dptr(t["orb"]), _lib.dptr(t["onsite"].view(float)),
                                          len(t["hop_i"]), _lib.iptr(t["hop_i"]), _lib.iptr(t["hop_j"]), _lib.iptr(t["hop_R"].reshape(-1)),
                                          _lib.dptr(t["hop_amp"].view(float)), C.byref(h)))
    return h


def moments(sp, k, M, bounds, nvec=NV, seed=1):
    mu = np.empty((len(k), nvec, M))
    _lib.check(_lib.lib.tbk_kpm_moments(sp, _lib.dptr(k), len(k), M, bounds[0], bounds[1], nvec, None, None, seed, _lib.dptr(mu)))
    return mu


def double_moments(sp, k, M, bounds, nvec=NV, seed=1):
    mu = np.empty((len(k), nvec, M, M), dtype=complex)
    _lib.check(_lib.lib.tbk_kpm_double_moments(sp, _lib.dptr(k), len(k), M, bounds[0], bounds[1], 0, 1, nvec, None, None, seed,
                                               _lib.dptr(mu.view(float))))
    return mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,224,1000")
    ap.add_argument("--moments", type=int, default=512)
    ap.add_argument("--double-size", type=int, default=224)
    ap.add_argument("--double-moments", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    k = np.array([[0.137, 0.731]])
    M = a.moments
    rows = []
    for L in [int(s) for s in a.sizes.split(",")]:
        t0 = time.perf_counter()
        tab = haldane_supercell_tables(L)
        t1 = time.perf_counter()
        sp = upload(ctx, tab)
        t2 = time.perf_counter()
        n, nnz, g = C.c_int(0), C.c_int64(0), np.zeros(2)
        _lib.check(_lib.lib.tbk_sparse_info(sp, None, C.byref(n), C.byref(nnz), _lib.dptr(g)))
        pad = 0.01 * (g[1] - g[0])
        bnd = (g[0] - pad, g[1] + pad)
        moments(sp, k, 4, bnd)                                   # warm-up: code objects, workspace
        moments(sp, k, M, bnd)
        wall = []
        for _ in range(3):
            w0 = time.perf_counter()
            moments(sp, k, M, bnd)
            wM = time.perf_counter() - w0
            w0 = time.perf_counter()
            moments(sp, k, 2, bnd)
            w2 = time.perf_counter() - w0
            wall.append((wM - w2) / (M // 2 - 1))
        ctx.prof_enable(1)
        ctx.prof_reset()
        mu = moments(sp, k, M, bnd)
        rep = ctx.prof_report()
        ctx.prof_enable(0)
        ctx.prof_reset()
        step = rep["kpm_step"]
        t_kernel = step["total_ms"] * 1e-3 / step["launches"]
        model_bytes = nnz.value * 20 + n.value * NV * 16 * 3
        footprint = nnz.value * 20 + n.value * NV * 16 * 2
        row = dict(L=L, nsta=n.value, nnz=nnz.value, moments=M, steps=step["launches"], build_s=t1 - t0, upload_s=t2 - t1,
                   kernel_us_per_step=t_kernel * 1e6, wall_us_per_step=float(np.median(wall)) * 1e6,
                   wall_us_per_step_runs=[w * 1e6 for w in wall], model_bytes_per_step=model_bytes, footprint_bytes=footprint,
                   model_rate_kernel=model_bytes / t_kernel, model_rate_wall=model_bytes / float(np.median(wall)),
                   fraction_of_copy_kernel=model_bytes / t_kernel / COPY_RATE, past_cache=footprint > (256 << 20),
                   values_us=rep["kpm_values"]["total_ms"] * 1e3, max_abs_mu=float(np.abs(mu).max()),
                   kernels={kk: vv for kk, vv in rep.items()})
        if L == a.double_size:
            double_moments(sp, k, a.double_moments, bnd)         # warm-up: workspace
            runs = []
            for _ in range(3):
                w0 = time.perf_counter()
                double_moments(sp, k, a.double_moments, bnd)
                runs.append((time.perf_counter() - w0) * 1e3)
            row.update(double_moments=a.double_moments, double_ms=float(np.median(runs)), double_ms_runs=runs)
        rows.append(row)
        print(json.dumps(row), flush=True)
        _lib.check(_lib.lib.tbk_sparse_free(sp))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
