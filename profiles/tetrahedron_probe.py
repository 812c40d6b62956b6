"""The tetrahedron calls beside the eigen-solve alone, in one process: tetrahedron_dos_mesh (256 energies, without and with the
projected DOS of every state) and tetrahedron_fermi_level_mesh on Haldane 256 x 256 and on an 8-state random model on 32 x 32 x 32,
with solve_all_mesh (eigenvalues only) and, for the projected DOS, the solve with eigenvectors.  Best of 5 after one untimed call,
wall time of the Python call in ms, one JSON line.  The figures of DESIGN.md section 29 come from one run of this script."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pythtb_amd as tb
from pythtb_amd import _lib
import helpers as hp
ctx = _lib.default_context()
def timed(f, rep=5):
    f(); ctx.sync()
    best = 1e9
    for _ in range(rep):
        ctx.sync(); t = time.perf_counter(); f(); ctx.sync(); best = min(best, time.perf_counter() - t)
    return round(best * 1e3, 3)
out = {}
for name, m, mesh, nel in (("haldane_256x256", hp.haldane(tb.tb_model, delta=0.2), [256, 256], 0.8),
                           ("random8_32x32x32", hp.random_model(tb.tb_model, 8, 3, 1, 21), [32, 32, 32], 3.3)):
    ev = m.solve_all_mesh(mesh)
    en = np.linspace(ev.min() - 0.1, ev.max() + 0.1, 256)
    sel = list(range(m._nsta))
    r = {"solve_evals_ms": timed(lambda: m.solve_all_mesh(mesh)),
         "solve_evecs_ms": timed(lambda: m.solve_all_mesh(mesh, eig_vectors=True)),
         "dos_ms": timed(lambda: m.tetrahedron_dos_mesh(mesh, en)),
         "dos_per_band_ms": timed(lambda: m.tetrahedron_dos_mesh(mesh, en, per_band=True)),
         "dos_pdos_ms": timed(lambda: m.tetrahedron_dos_mesh(mesh, en, states=sel)),
         "weights_ms": timed(lambda: m.tetrahedron_weights_mesh(mesh, float(en[100]))),
         "fermi_ms": timed(lambda: m.tetrahedron_fermi_level_mesh(mesh, nel)),
         "fermi_n1_ms": timed(lambda: m.tetrahedron_fermi_level_mesh(mesh, 1.0))}
    mu = m.tetrahedron_fermi_level_mesh(mesh, nel)
    r["N_at_mu_minus_n"] = float(m.tetrahedron_dos_mesh(mesh, [mu])[1][0] - nel)
    out[name] = r
print(json.dumps(out))
