#!/usr/bin/env python3
"""A fixed list of kernel-polynomial calls (kpm_vectors, kpm_moments, kpm_double_moments, kpm_apply, kpm_evolve,
local_chern_marker) that reaches every kernel of DESIGN.md sections 21 to 23 with all three kinds of start vectors, every output
saved to one .npz:

    TBK_LIBRARY=<libtbk.so> python profiles/kpm_bits.py out.npz      run the calls with that library (a fresh process each)
    python profiles/kpm_bits.py --compare a.npz b.npz                compare two runs as uint64 views (NaN and infinity patterns too)

Two builds that claim the same results must give equal files: the comparison has no tolerance (DESIGN.md sections 14 and 24).
The operators are those of tests/test_kpm.py::GPU_CASES (63, 64 and 65 rows, an empty row, spin blocks, long rows, dim_k = 0) and
the long ring of its grid-stride test; 257 moments or coefficients cross one rollover of the partial-sum slots, 17 and 33 double
moments the tile of 16 twice."""
import ctypes as C
import os
import sys

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kubo_bits import compare  # noqa: E402

NVECS = (1, 3, 8, 9)
ORDERS = (1, 2, 3, 64, 257)      # n_moments of kpm_moments, ncoef of kpm_apply
NSETS = (1, 4)
DOUBLE_ORDERS = (1, 17, 33)
SEED = 20240229


def main(path):
    import pythtb_amd as tb
    import kpm_ref as kr
    import test_kpm as tk
    L = tb._lib
    out = {}

    def keep(name, a):
        assert name not in out
        out[name] = np.ascontiguousarray(np.asarray(a)).view(float)

    rng = np.random.default_rng(2025)
    coef = rng.standard_normal((max(NSETS), max(ORDERS))) + 1j * rng.standard_normal((max(NSETS), max(ORDERS)))
    coef *= 0.5 ** np.arange(max(ORDERS)).clip(max=40)
    for name, nk in tk.GPU_CASES:
        m = tk.model(name)
        n, dk = m._nsta, m._dim_k
        k = tk.kpoints(m, nk)
        V = rng.standard_normal((max(NVECS), n)) + 1j * rng.standard_normal((max(NVECS), n))
        keep(name + " vectors", m.kpm_vectors(11, seed=SEED, first=3))
        for nvec in NVECS:
            states = [(7 * i) % n for i in range(nvec)]
            starts = (("random", dict(n_vectors=nvec, seed=SEED)), ("states", dict(states=states)), ("vectors", dict(vectors=V[:nvec])))
            for how, kw in starts:
                tag = "%s nvec%d %s " % (name, nvec, how)
                for M in ORDERS:
                    keep(tag + "moments M%d" % M, m.kpm_moments(M, k, **kw)[0])
                    for nset in NSETS:
                        keep(tag + "apply ncoef%d nset%d" % (M, nset), m.kpm_apply(coef[:nset, :M], k, **kw)[0])
                if dk > 0:
                    for dirs in ((0, 0),) if dk == 1 else ((0, dk - 1), (dk - 1, 0)):
                        for M in DOUBLE_ORDERS:
                            keep(tag + "double %s M%d" % (dirs, M), m.kpm_double_moments(M, dirs, k, **kw)[0])
        keep(name + " evolve", m.kpm_evolve([0.0, 0.7, 11.0], k, vectors=V[:3])[0])
        keep(name + " evolve states", m.kpm_evolve(2.5, k, states=[0, n - 1])[0])
        if dk == 0 and m._dim_r >= 2:
            for M in ORDERS:
                keep(name + " marker M%d" % M, m.local_chern_marker(0.05, M))
            keep(name + " marker states", m.local_chern_marker(0.05, 64, states=[n - 1, 0, 5], dirs=(1, 0)))
        print(name, len(out), flush=True)
    fl = tk.model("flake10x12")           # 240 states: a marker over 30 blocks
    keep("flake10x12 marker", fl.local_chern_marker(0.0, 257))
    # the long ring: the row tiles past 2048 workgroups, through the C interface
    (tab, kq, bnd, vec, rcoef), _ = tk.ring_reference()
    n, sp, kk = kr.RING_N, C.c_void_p(), np.array([[kq], [0.77]])
    L.check(L.lib.tbk_sparse_upload(L.default_context().handle, 1, n, 1, L.dptr(tab["orb"]), L.dptr(tab["onsite"].view(float)), n,
                                    L.iptr(tab["hop_i"]), L.iptr(tab["hop_j"]), L.iptr(tab["hop_R"].reshape(-1)),
                                    L.dptr(tab["hop_amp"].view(float)), C.byref(sp)))
    states = np.array([0, n - 1, 65536, 65535, 32, 31, 4099, 77, 12345], dtype=np.int32)
    for how, nvec, vp, stp in (("random", 9, None, None), ("states", 9, None, L.iptr(states)), ("vectors", 9, L.dptr(vec.view(float)), None),
                               ("random", 3, None, None)):
        tag = "ring nvec%d %s " % (nvec, how)
        mu = np.empty((2, nvec, 257))
        L.check(L.lib.tbk_kpm_moments(sp, L.dptr(kk), 2, 257, bnd[0], bnd[1], nvec, vp, stp, SEED, L.dptr(mu)))
        keep(tag + "moments", mu)
        for nset in NSETS:
            o = np.empty((2, nset, nvec, n), dtype=complex)
            c = np.ascontiguousarray(coef[:nset, :5])
            L.check(L.lib.tbk_kpm_apply_series(sp, L.dptr(kk), 2, 5, nset, L.dptr(c.view(float)), bnd[0], bnd[1], nvec, vp, stp, SEED,
                                               L.dptr(o.view(float))))
            keep(tag + "apply nset%d" % nset, o)
        d = np.empty((2, nvec, 17, 17), dtype=complex)
        L.check(L.lib.tbk_kpm_double_moments(sp, L.dptr(kk), 2, 17, bnd[0], bnd[1], 0, 0, nvec, vp, stp, SEED, L.dptr(d.view(float))))
        keep(tag + "double", d)
    L.check(L.lib.tbk_sparse_free(sp))
    np.savez(path, **out)
    print("saved %d arrays to %s (library %s)" % (len(out), path, os.environ.get("TBK_LIBRARY", "default")))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
