#!/usr/bin/env python3
"""A fixed list of calls through the lattice sum of weighted projectors (DESIGN.md sections 27, 30 and 33: density_matrix_mesh,
green_function_mesh, impurity_ldos_mesh, mean_field_mesh) on the small models of tests/test_density_matrix.py -- one, two and four
entries per lane, the ragged 63-point batch, two selections, the tiled form, the two two-chunk cases of each test file -- every
output saved to one .npz:

    TBK_LIBRARY=<libtbk.so> python profiles/lattice_sum_bits.py out.npz      run the calls with that library (a fresh process each)
    python profiles/lattice_sum_bits.py --compare a.npz b.npz                compare two runs as uint64 views

Two builds that claim the same results must give equal files: the comparison has no tolerance."""
import os
import sys

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))

from kubo_bits import compare  # noqa: E402

MODELS = ["square_1", "haldane_2a", "chain3_3", "kane_mele_4", "cubic16_16", "haldane3x3_18", "haldane4x4_32", "chain3x11_33"]
SELECTIONS = {"cubic16_16": [11, 2, 15, 7, 0], "chain3x11_33": [32, 5, -16, 0, 20]}
ETA = 0.05


def main():
    import dm_ref as dmr
    import test_density_matrix as tdm
    import test_green_function as tgf
    import test_mean_field as tmf
    from helpers import quiet

    out = {}
    for name in MODELS:
        m, mesh, target = tdm.build(name)
        ev = dmr.levels(m, mesh)
        if target is None:
            target = tdm.widest_gap(ev)
        rs = tdm.r_list(mesh)
        out[name + " D kT=0"] = m.density_matrix_mesh(mesh, tdm.safe_mu(ev, target), 0.0, rs)
        out[name + " D kT=0.05"] = m.density_matrix_mesh(mesh, target + 0.11, 0.05, rs)
        lo, width = ev.min(), ev.max() - ev.min()
        for nw in (1, 3, 5):
            w = lo + width * (np.array([0.7, 0.2, 0.7]) if nw == 3 else np.linspace(-0.1, 1.05, nw + 1)[1:])
            out["%s G nw=%d" % (name, nw)] = m.green_function_mesh(mesh, w, ETA, rs)
            if name in SELECTIONS:
                out["%s G nw=%d selected" % (name, nw)] = m.green_function_mesh(mesh, w, ETA, rs, states=SELECTIONS[name])
        w = np.array([lo + 0.3 * width, ev.max() + 0.5, lo + 0.5 * width])
        sites = tgf.three_sites(m) if name in ("haldane_2a", "kane_mele_4") else [(0, [0] * len(mesh)), (m._nsta - 1, [1] + [0] * (len(mesh) - 1))]
        v = tgf.hermitian(np.random.default_rng(11), len(sites), 0.4)
        probes = None if m._nsta <= 32 else [s for s in range(m._nsta) if s != 17][::-1]
        l0, dl = m.impurity_ldos_mesh(mesh, w, 0.1, sites, v, R_list=rs[:5], states=probes)
        out[name + " ldos0"], out[name + " dldos"] = l0, dl
    # the two-chunk cases: 40 states on 37 x 37 (tiled, two launches per chunk), 32 states on 46 x 46 (512 k-groups)
    m40, m32 = (quiet(tdm.haldane().make_supercell, s) for s in ([[5, 0], [0, 4]], [[4, 0], [0, 4]]))
    r40 = np.array([[0, 0], [1, 0], [-1, 2], [37, 0]] + [[a, b] for a in (-2, 3) for b in (-1, 0, 1, 2, 40)])
    r32 = np.array([[0, 0], [0, -1], [47, 3], [0, 46], [1, 1]])
    out["two chunks tiled D"] = m40.density_matrix_mesh([37, 37], 0.2, tdm.KT, r40)
    out["two chunks tiled G"] = m40.green_function_mesh([37, 37], np.array([0.2, -1.3]), ETA, r40)
    ev = dmr.levels(m32, [46, 46])
    out["two chunks lds D"] = m32.density_matrix_mesh([46, 46], tdm.safe_mu(ev, tdm.widest_gap(ev)), 0.0, r32)
    out["two chunks lds G"] = m32.green_function_mesh([46, 46], np.array([0.4, -2.1]), ETA, r32)
    for name in ("n4", "n18", "n33"):
        for kT in (0.05, 0.0):
            m, mesh, kw, nel = tmf.path_cases()[name]
            res = m.mean_field_mesh(mesh, tol=0.0, max_iter=3, **dict(kw, n_electrons=nel, kT=kT, mixing=0.5, history=0))
            for what in ("history", "residuals", "field", "density"):
                out["mean field %s kT=%g %s" % (name, kT, what)] = np.asarray(getattr(res, what))
            out["mean field %s kT=%g energy" % (name, kT)] = np.array([res.energy, res.fermi_level])
    np.savez(sys.argv[1], **{k: np.ascontiguousarray(np.asarray(v, dtype=complex if np.iscomplexobj(v) else float)) for k, v in out.items()})
    print("saved %d arrays to %s (library %s)" % (len(out), sys.argv[1], os.environ.get("TBK_LIBRARY", "default")))


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == "--compare" else main())
