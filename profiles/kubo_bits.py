#!/usr/bin/env python3
"""A fixed list of Kubo-formula calls (berry_curvature*, orbital_moment, orbital_magnetization_mesh, optical_conductivity_mesh,
spin_berry_curvature, spin_hall_conductivity_mesh, band_velocity, anomalous_transport_mesh, drude_weight_mesh, shift_current*,
injection_current_mesh, quantum_geometric_tensor*, susceptibility_mesh, thermodynamics_mesh, fermi_level_mesh, density_matrix_mesh,
dos_mesh) that reaches every routed form of DESIGN.md sections 11 to 13, 15 to 17, 20, 26 and 27, every output saved to one .npz:

    TBK_LIBRARY=<libtbk.so> python profiles/kubo_bits.py out.npz      run the calls with that library (a fresh process each)
    python profiles/kubo_bits.py --compare a.npz b.npz                compare two runs as uint64 views (NaN and infinity patterns too)

Two builds that claim the same results must give equal files: the comparison has no tolerance."""
import contextlib
import io
import itertools
import os
import sys

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))


def compare(fa, fb):
    a, b = np.load(fa), np.load(fb)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x.view(np.uint64), y.view(np.uint64)):
            n = int(np.sum(x.view(np.uint64) != y.view(np.uint64))) if x.shape == y.shape else -1
            print("DIFFERENT %s: %d of %d words" % (name, n, x.view(np.uint64).size))
            bad.append(name)
    print("%d arrays compared, %d different or missing" % (len(set(a.files) | set(b.files)), len(bad)))
    return 1 if bad else 0


def main():
    import pythtb_amd as tb  # noqa: E402
    import helpers as hp  # noqa: E402
    from pythtb_amd import w90  # noqa: E402


    def quiet(fn, *a, **k):
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a, **k)


    def supercell(s):
        return quiet(hp.haldane(tb.tb_model, 0.2).make_supercell, [[s, 0], [0, s]])


    # name -> (model, occupied bands, 2-D or 3-D mesh); the number of states routes the form
    MODELS = {
        "haldane_n2": (lambda: hp.haldane(tb.tb_model, 0.2), [0], [96, 80]),
        "random_n3": (lambda: hp.random_model(tb.tb_model, 3, 2, 1, 11), [0], [40, 36]),
        "kane_mele_n4": (lambda: hp.kane_mele(tb.tb_model), [0, 1], [48, 40]),
        "silicon_n8": (lambda: quiet(w90(os.path.join(_ROOT, "tests", "golden", "w90_silicon"), "silicon").model), [0, 1, 2, 3], [12, 10, 8]),
        "cubic16_n16": (lambda: hp.cubic16(tb.tb_model), list(range(8)), [24, 24, 16]),   # two chunks
        "haldane_4x4_n32": (lambda: supercell(4), list(range(16)), [24, 20]),
        "random_n36": (lambda: hp.random_model(tb.tb_model, 36, 2, 1, 12), list(range(18)), [12, 10]),
        "random_n80": (lambda: hp.random_model(tb.tb_model, 40, 2, 2, 13), list(range(40)), [8, 6]),
        # three directions at the last size of the LDS forms (80 KiB in k_opt_pairs and k_qgt_lds<3>) and at the first wide size
        "random3d_n32": (lambda: hp.random_model(tb.tb_model, 16, 3, 2, 14), list(range(16)), [6, 5, 4]),
        "random3d_n33": (lambda: hp.random_model(tb.tb_model, 33, 3, 1, 15), list(range(16)), [4, 3, 2]),
    }

    out = {}


    def keep(name, a):
        assert name not in out
        out[name] = np.ascontiguousarray(np.asarray(a)).view(float)


    def keep_all(name, arrays):
        for i, a in enumerate(arrays):
            keep("%s %d" % (name, i), a)


    rng = np.random.default_rng(2024)
    for name, (make, occ, mesh) in MODELS.items():
        m = make()
        dk = m._dim_k
        e = m.solve_all_mesh([6] * dk)
        lo, hi = float(e.min()), float(e.max())
        few = np.linspace(lo - 0.1, hi + 0.1, 37)
        # more levels than one window of either Fermi kernel, unsorted, with ties
        many = rng.permutation(np.concatenate([np.linspace(lo, hi, 4000), np.linspace(lo, hi, 500), np.full(500, 0.5 * (lo + hi))]))
        k = rng.random((70, dk))
        for dirs in ([(0, 1), (1, 2), (2, 0)] if dk == 3 else [(0, 1), (1, 0)]):
            tag = "%s d%d%d " % ((name,) + dirs)
            keep(tag + "curv list", m.berry_curvature(k, dirs=dirs))
            keep(tag + "curv list occ", m.berry_curvature(k, occ=occ, dirs=dirs))
            keep(tag + "orb list", m.orbital_moment(k, dirs=dirs))
            keep(tag + "orb list occ", m.orbital_moment(k, occ=occ, dirs=dirs))
            keep(tag + "curv mesh", m.berry_curvature_mesh(mesh, dirs=dirs))
            keep(tag + "curv mesh occ", m.berry_curvature_mesh(mesh, occ=occ, dirs=dirs))
            keep(tag + "curv mesh fermi", m.berry_curvature_mesh(mesh, dirs=dirs, fermi_levels=few))
            keep(tag + "orb mesh occ", m.orbital_magnetization_mesh(mesh, occ=occ, dirs=dirs))
            keep(tag + "orb mesh fermi", m.orbital_magnetization_mesh(mesh, fermi_levels=few, dirs=dirs))
            keep(tag + "orb mesh kT", m.orbital_magnetization_mesh(mesh, fermi_levels=few, kT=0.05, dirs=dirs))
            keep_all(tag + "transport", m.anomalous_transport_mesh(mesh, few, 0.05, dirs=dirs))
            if m._nspin == 2:
                keep(tag + "spin curv list", m.spin_berry_curvature(k, dirs=dirs))
                keep(tag + "spin curv list occ", m.spin_berry_curvature(k, spin=0, occ=occ, dirs=dirs))
                keep(tag + "spin hall mesh", m.spin_hall_conductivity_mesh(mesh, dirs=dirs))
                keep(tag + "spin hall mesh occ", m.spin_hall_conductivity_mesh(mesh, spin=0, occ=occ, dirs=dirs))
                keep(tag + "spin hall mesh fermi", m.spin_hall_conductivity_mesh(mesh, dirs=dirs, fermi_levels=few))
        keep(name + " velocity", m.band_velocity(k))
        keep(name + " drude", m.drude_weight_mesh(mesh, few, 0.05))
        if name in ("haldane_n2", "kane_mele_n4", "silicon_n8"):
            keep(name + " curv mesh fermi5000", m.berry_curvature_mesh(mesh, fermi_levels=many))
            keep(name + " orb mesh fermi5000", m.orbital_magnetization_mesh(mesh, fermi_levels=many))
            # the thermal scan over twenty tiles of levels
            keep(name + " orb mesh kT5000", m.orbital_magnetization_mesh(mesh, fermi_levels=many, kT=0.05))
            keep_all(name + " transport kT5000", m.anomalous_transport_mesh(mesh, many, 0.05))
            keep(name + " drude kT5000", m.drude_weight_mesh(mesh, many, 0.05))
        omega = np.linspace(-1.0, 0.5 * (hi - lo), 23)
        mu = 0.5 * (lo + hi) + 0.013
        for kT in (0.0, 0.05):
            for dirs in ((0, 0), (0, 1), None):
                keep("%s optics %s kT%g" % (name, dirs, kT),
                     m.optical_conductivity_mesh(mesh, omega, 0.03, fermi_level=mu, kT=kT, dirs=dirs))
        one = (dk - 1, 0, dk - 1)
        keep(name + " shift list", m.shift_current(k, occ, one))
        keep(name + " shift list aaa", m.shift_current(k, occ, (0, 0, 0)))
        for kT in (0.0, 0.05):
            for dirs in (None, one):
                keep("%s shift %s kT%g" % (name, dirs, kT), m.shift_current_mesh(mesh, omega, 0.03, fermi_level=mu, kT=kT, dirs=dirs))
                keep("%s injection %s kT%g" % (name, dirs, kT),
                     m.injection_current_mesh(mesh, omega, 0.03, fermi_level=mu, kT=kT, dirs=dirs))
        keep(name + " qgt list", m.quantum_geometric_tensor(k))
        keep(name + " qgt list occ", m.quantum_geometric_tensor(k, occ=occ))
        keep(name + " qgt mesh", m.quantum_geometric_tensor_mesh(mesh))
        keep(name + " qgt mesh occ", m.quantum_geometric_tensor_mesh(mesh, occ=occ))
        # the susceptibility and the occupied-state calls (sections 26 and 27): q = 0, a mesh vector and a general q
        qs = np.array([[0.0] * dk, [1.0 / mesh[0]] + [0.0] * (dk - 1), [0.37, 0.21, 0.11][:dk]])
        nocc = len(occ)
        for kT in (0.0, 0.05):
            for me in (True, False):
                keep("%s chi static me%d kT%g" % (name, me, kT), m.susceptibility_mesh(mesh, qs, fermi_level=mu, kT=kT, matrix_elements=me))
                for w in (omega, np.linspace(-1.0, hi - lo, 1030)) if name == "haldane_n2" else (omega,):
                    keep("%s chi w%d me%d kT%g" % (name, len(w), me, kT),
                         m.susceptibility_mesh(mesh, qs, w, 0.03, fermi_level=mu, kT=kT, matrix_elements=me))
            keep("%s thermo kT%g" % (name, kT), m.thermodynamics_mesh(mesh, few, kT=kT))
            if name in ("haldane_n2", "kane_mele_n4", "silicon_n8"):
                keep("%s thermo5000 kT%g" % (name, kT), m.thermodynamics_mesh(mesh, many, kT=kT))
            keep("%s density matrix kT%g" % (name, kT),
                 m.density_matrix_mesh(mesh, mu, kT=kT, R_list=list(itertools.product((-1, 0, 1), repeat=dk))))
        nkp = int(np.prod(mesh))
        keep_all(name + " fermi level kT0", m.fermi_level_mesh(mesh, [nocc, (nocc * nkp - 1) / nkp, (nocc * nkp + 1) / nkp], return_edges=True))
        keep(name + " fermi level kT0.05", m.fermi_level_mesh(mesh, [nocc, nocc - 0.37, nocc + 0.21], kT=0.05))
        if name in ("haldane_n2", "silicon_n8"):
            keep_all(name + " dos", m.dos_mesh(mesh, bins=50, range=(lo, hi)))
        print(name, len(out), flush=True)

    # one dimension: the whole-mesh forms alone (sections 16 and 20)
    m = hp.chain3(tb.tb_model, -1.3, 0.4, 0.7)
    k = rng.random((70, 1))
    keep("chain3 qgt list", m.quantum_geometric_tensor(k))
    keep("chain3 qgt list occ", m.quantum_geometric_tensor(k, occ=[0]))
    keep("chain3 qgt mesh", m.quantum_geometric_tensor_mesh([500]))
    keep("chain3 qgt mesh occ", m.quantum_geometric_tensor_mesh([500], occ=[0]))
    keep("chain3 drude", m.drude_weight_mesh([500], np.linspace(-3.0, 3.0, 37), 0.05))
    keep("chain3 velocity", m.band_velocity(k))
    print("chain3", len(out), flush=True)

    np.savez(sys.argv[1], **out)
    print("saved %d arrays to %s (library %s)" % (len(out), sys.argv[1], os.environ.get("TBK_LIBRARY", "default")))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
