#!/usr/bin/env python3
"""A fixed list of calls through the three drivers of the density-density interaction (DESIGN.md sections 33, 36, 37 and 38:
mean_field_mesh, bdg_mesh, exciton_apply_mesh / exciton_states_mesh / exciton_spectrum_mesh) on the small iteration-path models of
tests/test_mean_field.py, tests/test_bdg.py and tests/test_excitons.py -- both filling forms, kT = 0 and > 0, linear and Anderson
mixing, the resident and the two-pass form, one, two and three channels, one and two chunks, bonds at R = 0 and R != 0 -- every
output saved to one .npz:

    TBK_LIBRARY=<libtbk.so> python profiles/mean_field_bits.py out.npz      run the calls with that library (a fresh process each)
    python profiles/mean_field_bits.py --compare a.npz b.npz                compare two runs as uint64 views

Two builds that claim the same results must give equal files: the comparison has no tolerance."""
import os
import sys

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))

from kubo_bits import compare  # noqa: E402

MF_KEEP = ("field", "_x", "residuals", "history", "density")
BDG_KEEP = ("field", "_x", "residuals", "history", "anomalous")


def main():
    import test_bdg as tbd
    import test_excitons as tex
    import test_mean_field as tmf

    out = {}

    def keep(tag, res, arrays, scalars):
        for what in arrays:
            out["%s %s" % (tag, what)] = np.asarray(getattr(res, what))
        out[tag + " scalars"] = np.array([getattr(res, s) for s in scalars], dtype=float)

    mf_scalars = ("energy", "entropy", "free_energy", "band_energy", "n_electrons", "fermi_level")
    for name in ("n4", "n18", "n33"):
        m, mesh, kw, nel = tmf.path_cases()[name]
        for kT in (0.0, 0.05):
            for history, iters in ((0, 3), (0, 6), (4, 3), (4, 6)):
                for fill in (dict(n_electrons=nel), dict(fermi_level=0.1)):
                    tag = "mf %s kT=%g history=%d max_iter=%d %s" % (name, kT, history, iters, list(fill)[0])
                    keep(tag, m.mean_field_mesh(mesh, **dict(kw, tol=0.0, max_iter=iters, kT=kT, mixing=0.5, history=history, **fill)),
                         MF_KEEP, mf_scalars)
        two = tmf.with_knob(1, lambda: m.mean_field_mesh(mesh, **dict(kw, tol=0.0, max_iter=6, kT=0.05, mixing=0.5, history=4,
                                                                      n_electrons=nel)))
        assert not two.resident
        keep("mf %s two-pass" % name, two, MF_KEEP, mf_scalars)

    bdg_scalars = ("energy", "entropy", "free_energy", "grand_potential", "gap", "n_electrons", "fermi_level")
    for name in ("hubbard_kT", "chain_fock", "haldane_all", "n9", "n17", "n20"):
        m, mesh, kw, nel, mu = tbd.path_cases()[name]
        start = 0.5 + 0.1 * np.cos(np.arange(float(m._nsta)))
        start = start.reshape(m._norb, 2) if m._nspin == 2 else start
        for fill in (dict(n_electrons=nel), dict(fermi_level=mu)):
            tag = "bdg %s %s" % (name, list(fill)[0])
            keep(tag, m.bdg_mesh(mesh, **dict(kw, tol=0.0, max_iter=6, start=start, history=0, mixing=0.5, **fill)), BDG_KEEP, bdg_scalars)
        keep("bdg %s anderson" % name, m.bdg_mesh(mesh, **dict(kw, tol=0.0, max_iter=6, start=start, history=4, mixing=0.5, n_electrons=nel)),
             BDG_KEEP, bdg_scalars)

    rng = np.random.default_rng(11)
    for name in ("chain2", "honey", "honey-R", "spinful"):
        m, mesh, kw = tex.case(name)
        nv, nc = kw.get("valence", 1), kw.get("conduction", 1)
        shape = (3,) + tuple(mesh) + (nv, nc)
        Y, gaps = m.exciton_apply_mesh(mesh, vectors=rng.standard_normal(shape) + 1j * rng.standard_normal(shape), **kw)
        out["bse %s apply" % name], out["bse %s gaps" % name] = Y, gaps
        st = m.exciton_states_mesh(mesh, **kw)
        out["bse %s energies" % name], out["bse %s dipoles" % name], out["bse %s norm" % name] = st.energies, st.dipoles, st.dipole_norm
        out["bse %s gap" % name] = np.array([st.gap, st.binding])
        sp = m.exciton_spectrum_mesh(mesh, omega=np.linspace(0.0, 3.0, 7), eta=0.05, n_steps=16, return_coefficients=True, **kw)
        c = sp.coefficients
        out["bse %s chi" % name], out["bse %s alpha" % name], out["bse %s beta" % name] = sp.chi, c.alpha, c.beta
        out["bse %s norm2" % name], out["bse %s used" % name] = c.norm2, np.asarray(c.n_used, dtype=float)
    np.savez(sys.argv[1], **{k: np.ascontiguousarray(np.asarray(v, dtype=complex if np.iscomplexobj(v) else float)) for k, v in out.items()})
    print("saved %d arrays to %s (library %s)" % (len(out), sys.argv[1], os.environ.get("TBK_LIBRARY", "default")))


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == "--compare" else main())
