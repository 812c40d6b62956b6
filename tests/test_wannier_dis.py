"""tb_model.wannier_disentangle_mesh and the b-vector shell search against tests/wdis_ref.py and against exact
identities.

Bound.  1e-10 A max(1, 1 / sv_min^2): sv_min is the reference's smallest singular value of the projection inside the final subspace,
asserted >= 0.1 (the Loewdin factor amplifies the rounding of A' by its inverse square); A is the amplification of a 1e-9 change of
one trial amplitude between two REFERENCE runs, floored at 1 and asserted <= 1e4 (the rule of tests/test_wannier.py and
tests/test_mean_field.py).  The reference's smallest selection gap is asserted >= 1e-3: below it the choice of the subspace is
ill-conditioned.  The eigenvector basis inside the subspace is arbitrary, so only the projector (up to the phases of the band
eigenvectors: its moduli and cyclic triple products), Omega_I and what follows the gauge step are compared.  DESIGN.md section 35
lists the measured deviations next to the bounds."""
import os
import subprocess

import numpy as np
import pytest

import helpers as hp
import wan_ref as wr
import wdis_ref as wd
from helpers import quiet
from oracle import tb_oracle as orc

import pythtb_amd as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- models (the builders of tests/test_wannier.py)
def honeycomb(delta, nspin=1):
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=nspin)
    m.set_onsite([-delta, delta])
    m.set_hop(-1.0, 0, 1, [0, 0])
    m.set_hop(-1.0, 1, 0, [1, 0])
    m.set_hop(-1.0, 1, 0, [0, 1])
    return m


def spinful_honeycomb():
    m = honeycomb(0.7, nspin=2)
    m.set_onsite([0.0, 0.0, 0.0, 0.15], 0, mode="add")
    m.set_onsite([0.0, 0.0, 0.0, 0.10], 1, mode="add")
    m.set_hop([0.0, 0.0, 0.12j, 0.05], 0, 1, [1, 0], mode="add", allow_conjugate_pair=True)
    return m


def chain(norb, pot=0.6):
    m = quiet(tb.tb_model, 1, 1, [[1.0]], [[(o + 0.25) / norb] for o in range(norb)])
    m.set_onsite([pot * np.cos(2.4 * o + 0.3) for o in range(norb)])
    for o in range(norb):
        t = -1.0 - 0.2 * (o % 2)
        if o + 1 < norb:
            m.set_hop(t, o, o + 1, [0])
        else:
            m.set_hop(t, o, 0, [1])
    return m


def cubic8():
    orb = [[0.25 + 0.5 * x, 0.2 + 0.5 * y, 0.3 + 0.5 * z] for x in range(2) for y in range(2) for z in range(2)]
    m = quiet(tb.tb_model, 3, 3, np.eye(3), orb)
    idx = lambda x, y, z: (x * 2 + y) * 2 + z
    m.set_onsite([(-1.5 if (x + y + z) % 2 == 0 else 1.5) + 0.1 * idx(x, y, z) for x in range(2) for y in range(2) for z in range(2)])
    for x in range(2):
        for y in range(2):
            for z in range(2):
                i = idx(x, y, z)
                for d, t in ((0, -1.0), (1, -0.8), (2, -0.6)):
                    p = [x, y, z]
                    R = [0, 0, 0]
                    p[d] += 1
                    if p[d] == 2:
                        p[d], R[d] = 0, 1
                    m.set_hop(t * (1.0 + 0.1 * p[d]), i, idx(*p), R)
    return m


FCC = [[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]
BCC = [[-0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, -0.5]]
HEX = [[1.0, 0.0, 0.0], [-0.5, np.sqrt(3.0) / 2.0, 0.0], [0.0, 0.0, 1.6]]
TRICLINIC = [[1.0, 0.0, 0.0], [0.3, 1.1, 0.0], [-0.2, 0.25, 0.9]]


def fcc3():
    """Three orbitals on an fcc lattice: the closed-form star has zero weights here, the shell search finds four vectors."""
    m = quiet(tb.tb_model, 3, 3, FCC, [[0.0, 0.0, 0.0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5]])
    m.set_onsite([-1.0, 0.6, 1.2])
    m.set_hop(-0.5, 0, 1, [0, 0, 0])
    m.set_hop(-0.3, 2, 1, [0, 0, 0])
    for a in range(3):
        e = [1 if d == a else 0 for d in range(3)]
        m.set_hop(-0.5, 0, 1, [-x for x in e])
        m.set_hop(-0.3, 2, 1, e)
        m.set_hop(0.1, 0, 0, e)
        m.set_hop(-0.15, 2, 2, e)
    return m


CHAIN_TRIAL = [[(1.0, 0, [0]), (0.3, 1, [0])], [(1.0, 2, [0]), (-0.4, 3, [0])]]


def blocks(width, count, last=None):
    out = [[(1.0, o, [0]) for o in range(i * width, (i + 1) * width)] for i in range(count)]
    if last is not None:
        out[-1] = [(1.0, o, [0]) for o in range((count - 1) * width, last)]
    return out


_BANDS = {}


def band_ranges(m, mesh):
    """(min, max) over the mesh of every band, from the oracle's Hamiltonian."""
    key = (id(m), tuple(mesh))
    if key not in _BANDS:
        ev = np.linalg.eigvalsh(orc.ham_batch(m, wr.mesh_points(m, mesh)))
        _BANDS[key] = (ev.min(axis=0), ev.max(axis=0))
    return _BANDS[key]


def mid(m, mesh, j):
    lo, hi = band_ranges(m, mesh)
    return 0.5 * (lo[j] + hi[j])


def below(m, mesh):
    return band_ranges(m, mesh)[0][0] - 1.0


_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = dict(chain6=lambda: chain(6), spinful=spinful_honeycomb, cubic=cubic8, chain33=lambda: chain(33),
                             chain40=lambda: chain(40), fcc=fcc3)[name]()
    return _MODELS[name]


def cases():
    """name -> (model, mesh, trial, bands, keywords).  'mid band j' is the midpoint of band j's range on the mesh."""
    c6, sp, cub, c33, c40 = model("chain6"), model("spinful"), model("cubic"), model("chain33"), model("chain40")
    low = [0, 3, 5, 6]
    out = {
        "chain6": (c6, [12], CHAIN_TRIAL, [0, 1, 2, 3], dict(dis_iter=40)),
        "chain6-frozen": (c6, [12], CHAIN_TRIAL, [0, 1, 2, 3],
                          dict(dis_iter=40, frozen=(below(c6, [12]), band_ranges(c6, [12])[1][0] + 1e-3))),
        "chain6-window": (c6, [12], CHAIN_TRIAL, [0, 1, 2, 3], dict(dis_iter=40, window=(below(c6, [12]), mid(c6, [12], 3)))),
        "spinful-frozen": (sp, [6, 5], [0, 1], [0, 1, 2, 3], dict(dis_iter=40, frozen=(below(sp, [6, 5]), mid(sp, [6, 5], 1)))),
        "spinful-both": (sp, [6, 5], [0, 1], [0, 1, 2, 3],
                         dict(dis_iter=40, frozen=(below(sp, [6, 5]), mid(sp, [6, 5], 1)), window=(below(sp, [6, 5]), mid(sp, [6, 5], 3)))),
        "cubic": (cub, [4, 3, 5], low, list(range(8)),
                  dict(dis_iter=20, window=(below(cub, [4, 3, 5]), mid(cub, [4, 3, 5], 6)), frozen=(below(cub, [4, 3, 5]), mid(cub, [4, 3, 5], 2)))),
        "chain33": (c33, [8], blocks(8, 4, last=33), list(range(8)), dict(dis_iter=40)),
        "chain40-32": (c40, [6], blocks(3, 12), list(range(32)), dict(dis_iter=20, frozen=(below(c40, [6]), mid(c40, [6], 5)))),
        "chain40-24": (c40, [6], blocks(5, 6), list(range(24)),
                       dict(dis_iter=20, window=(below(c40, [6]), mid(c40, [6], 20)), frozen=(below(c40, [6]), mid(c40, [6], 3)))),
        "fcc": (model("fcc"), [4, 4, 4], [0], [0, 1], dict(dis_iter=20, b_vectors="shells")),
    }
    return out


CASES = ["chain6", "chain6-frozen", "chain6-window", "spinful-frozen", "spinful-both", "cubic", "chain33", "chain40-32", "chain40-24"]
KEYS = ("centers", "spreads", "hoppings", "history", "dis_history", "projector")
_REF = {}


def ref_pair(name, **extra):
    """(reference run, amplification A) of a case, computed once per set of keywords and shared: A from a second reference run with the
    first trial amplitude changed by 1e-9."""
    key = (name, tuple(sorted(extra.items())))
    if key not in _REF:
        m, mesh, trial, bands, kw = cases()[name]
        kw = dict(kw, **extra)
        terms = wr.trial_terms(m, trial)
        pert = [[(a, s, R) for a, s, R in fn] for fn in terms]
        a0, s0, R0 = pert[0][0]
        pert[0][0] = (a0 + 1e-9, s0, R0)
        full = lambda fn: [(a, s, np.array(R)) for a, s, R in fn]
        ref = wd.run(m, mesh, [full(f) for f in terms], bands, **kw)
        ref2 = wd.run(m, mesh, [full(f) for f in pert], bands, **kw)
        A = max(1.0, max(np.max(np.abs(ref2[k] - ref[k])) for k in KEYS) / 1e-9)
        _REF[key] = (ref, A)
    return _REF[key]


def bound_of(ref, A):
    assert A <= 1e4, A
    assert ref["sv_min"] >= 0.1, ref["sv_min"]
    assert ref["dis_gap_min"] >= 1e-3, ref["dis_gap_min"]
    return 1e-10 * A * max(1.0, 1.0 / ref["sv_min"] ** 2)


def compare(res, ref, bound, tag):
    # the projector in the band basis: every band's eigenvector carries a phase of its solver's choosing, P_ab -> e^{i(t_a - t_b)} P_ab,
    # so its moduli and its cyclic triple products P_ab P_bc P_ca are compared, which no such phase changes
    P, Pr = res.gauge @ res.gauge.conj().transpose(0, 2, 1), ref["projector"]
    triple = lambda X: np.einsum("kab,kbc,kca->kabc", X, X, X)
    d = {
        "dis_history": np.max(np.abs(res.dis_history - ref["dis_history"])),
        "projector": max(np.max(np.abs(np.abs(P) - np.abs(Pr))), np.max(np.abs(triple(P) - triple(Pr)))),
        "centers": np.max(np.abs(res.centers - ref["centers"])),
        "spreads": np.max(np.abs(res.spreads - ref["spreads"])),
        "omega_i": abs(res.omega_i - ref["omega_i"]),
        "omega_od": abs(res.omega_od - ref["omega_od"]),
        "omega_d": abs(res.omega_d - ref["omega_d"]),
        "sv_min": abs(res.sv_min - ref["sv_min"]),
        "sv_min_projection": abs(res.sv_min_projection - ref["sv_min_projection"]),
        "hoppings": np.max(np.abs(res.hoppings - ref["hoppings"])),
        "history": np.max(np.abs(res.history - ref["history"])),
    }
    print("%s: bound %.2e; " % (tag, bound) + ", ".join("%s %.2e" % kv for kv in d.items()))
    print("%s: Omega_I %.6f -> %.6f, sv_min %.3f, gap %.3e (reference %.3e), n_window %d..%d, n_frozen %d..%d" % (
        tag, res.dis_history[0], res.dis_history[-1], res.sv_min, res.dis_gap_min, ref["dis_gap_min"], res.n_window.min(),
        res.n_window.max(), res.n_frozen.min(), res.n_frozen.max()))
    assert np.array_equal(res.R_list, ref["R_list"])
    assert np.array_equal(res.n_window, ref["n_window"]) and np.array_equal(res.n_frozen, ref["n_frozen"])
    assert max(d.values()) <= bound, d
    if np.isfinite(ref["dis_gap_min"]):                                                # eigenvalues of Z: at most sum_{+-b} w_b, not O(1)
        scale = max(1.0, 2.0 * float(np.sum(ref["b_weights"])))
        assert abs(res.dis_gap_min - ref["dis_gap_min"]) <= bound * scale, (res.dis_gap_min, ref["dis_gap_min"])
    else:
        assert res.dis_gap_min == np.inf


def call(name, **extra):
    m, mesh, trial, bands, kw = cases()[name]
    return m.wannier_disentangle_mesh(mesh, trial, bands, **dict(kw, **extra))


# ---------------------------------------------------------------- CPU
def test_argument_errors_without_gpu():
    m = chain(6)
    for kw, pat in ((dict(window=(1.0, 0.0)), "window"), (dict(window=(0.0, np.inf)), "window"), (dict(window=(0.0,)), "window"),
                    (dict(window="ab"), "window"), (dict(frozen=(np.nan, 1.0)), "frozen"), (dict(frozen=(2.0, 1.0)), "frozen"),
                    (dict(frozen=[0.0, 1.0, 2.0]), "frozen"), (dict(dis_iter=-1), "dis_iter"), (dict(dis_iter=65537), "dis_iter"),
                    (dict(dis_iter=1.5), "dis_iter"), (dict(dis_mixing=0.0), "dis_mixing"), (dict(dis_mixing=1.5), "dis_mixing"),
                    (dict(dis_mixing=np.nan), "dis_mixing"), (dict(dis_tol=-1.0), "dis_tol"), (dict(dis_tol=np.nan), "dis_tol"),
                    (dict(b_vectors="stars"), "b_vectors"), (dict(b_vectors=None), "b_vectors"), (dict(max_iter=-1), "max_iter"),
                    (dict(check_every=0), "check_every")):
        with pytest.raises(Exception, match=pat):
            m.wannier_disentangle_mesh([12], CHAIN_TRIAL, [0, 1, 2, 3], **kw)
    with pytest.raises(Exception, match="b_vectors"):
        m.wannier_mesh([12], CHAIN_TRIAL, [0, 1], b_vectors="shell")
    with pytest.raises(Exception, match="more trial functions"):
        m.wannier_disentangle_mesh([12], CHAIN_TRIAL, [0])
    # the two residency caps: the candidate states (N_k nsta nb) and their overlaps (N_k nbv nb^2), each where section 34's cap holds
    with pytest.raises(Exception, match="candidate states stay resident"):
        m.wannier_disentangle_mesh([2 ** 23], [0], [0, 1], R_list=[[0]])
    with pytest.raises(Exception, match="overlaps stay resident"):
        cubic8().wannier_disentangle_mesh([64, 64, 128], [0, 3, 5, 6], list(range(8)), R_list=[[0, 0, 0]])


def test_wdis_check_program():
    """make wdis-check: the host-only checks, caps, plans and the 32 x 32 eigen-solver, as a stand-alone program under the sanitizers."""
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "pythtb_amd", "csrc"), "wdis-check"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "wdis_plan_check: ok" in res.stdout


@pytest.mark.parametrize("lat, mesh, count, equal", [
    (FCC, [4, 4, 4], 4, True), (BCC, [4, 4, 4], 6, True), (FCC, [4, 4, 6], 6, False), (HEX, [6, 6, 4], 4, False),
    (TRICLINIC, [5, 6, 4], 6, False), (hp.LAT, [12, 12], 3, True)])
def test_shell_rule(lat, mesh, count, equal):
    lat = np.array(lat, dtype=float)
    dk = lat.shape[0]
    m = quiet(tb.tb_model, dk, dk, lat, [[0.0] * dk])
    steps, w, b = m._wannier_bvectors(np.array(mesh, dtype=np.int32), "shells")
    print("%s: steps %s, weights %s" % (mesh, steps.tolist(), w))
    assert len(w) == count and len(w) <= 6 and np.all(w > 0.0) and np.all(np.abs(steps) <= 1)
    assert np.max(np.abs(2.0 * np.einsum("b,bi,bj->ij", w, b, b) - np.eye(dk))) <= 1e-12
    rs, rw, rb = wd.shells(lat, mesh)
    assert np.array_equal(steps, rs) and np.max(np.abs(w - rw)) <= 1e-12 * np.max(rw) and np.max(np.abs(b - rb)) <= 1e-14 * np.max(np.abs(rb))
    if equal:
        assert np.max(np.abs(w - w[0])) <= 1e-12 * w[0]
    if dk == 3 and mesh == [4, 4, 4] and count == 4:
        assert steps.tolist() == [[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    if dk == 2:                                                                        # the three vectors of the closed form
        cs, cw, cb = m._wannier_bvectors(np.array(mesh, dtype=np.int32))
        assert sorted(map(tuple, steps.tolist())) == sorted(map(tuple, cs.tolist()))


def test_shell_rule_refuses_the_skew_lattice():
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.9, 0.2]], [[0.0, 0.0]])
    with pytest.raises(Exception, match="too skewed"):
        m._wannier_bvectors(np.array([6, 6], dtype=np.int32), "shells")
    with pytest.raises(Exception, match="too skewed"):
        m.wannier_disentangle_mesh([6, 6], [0], [0], b_vectors="shells")
    with pytest.raises(ValueError):
        wd.shells([[1.0, 0.0], [0.9, 0.2]], [6, 6])


def test_fcc_refuses_the_closed_form_star():
    m = model("fcc")
    with pytest.raises(Exception, match="too skewed"):
        m.wannier_mesh([4, 4, 4], [0], [0])
    with pytest.raises(Exception, match="too skewed"):
        m.wannier_disentangle_mesh([4, 4, 4], [0], [0, 1])


# ---------------------------------------------------------------- GPU: against the reference
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_against_reference(name):
    ref, A = ref_pair(name)
    bound = bound_of(ref, A)
    res = call(name, return_gauge=True)
    kw = cases()[name][4]
    assert res.dis_iterations == kw["dis_iter"] and not res.dis_converged and res.iterations == 0
    compare(res, ref, bound, "%s (A = %.2f)" % (name, A))
    assert res.dis_history[-1] <= res.dis_history[0] and ref["dis_history"][-1] <= ref["dis_history"][0]
    assert abs(res.dis_history[-1] - res.omega_i) <= bound                            # Omega_I of the subspace is that of its functions
    rows = np.where(~ref["window_mask"])
    assert np.all(res.gauge[rows[0], rows[1], :] == 0.0)                              # zero rows for bands outside the window


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6-frozen", "spinful-both"])
def test_descent_after_disentanglement(name):
    ref, A = ref_pair(name, max_iter=20, check_every=5)
    res = call(name, max_iter=20, check_every=5, return_gauge=True)
    assert res.iterations == 20 and res.history.shape == (5,) and res.dis_history.shape == (9,)
    compare(res, ref, bound_of(ref, A), "%s with the descent (A = %.2f)" % (name, A))
    assert np.all(np.diff(res.history) <= 1e-13), res.history


@pytest.mark.gpu
def test_mixing_against_reference():
    ref, A = ref_pair("chain6-window", dis_mixing=0.5)
    res = call("chain6-window", dis_mixing=0.5, return_gauge=True)
    compare(res, ref, bound_of(ref, A), "chain6-window at mixing 0.5 (A = %.2f)" % A)
    plain = ref_pair("chain6-window")[0]
    assert np.max(np.abs(plain["dis_history"][1:] - ref["dis_history"][1:])) > 1e-6      # the mixing does change the path


# ---------------------------------------------------------------- GPU: exact identities
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6-frozen", "spinful-frozen", "spinful-both", "cubic", "chain40-32", "chain40-24"])
def test_frozen_window_is_exact(name):
    m, mesh, trial, bands, kw = cases()[name]
    ref = ref_pair(name)[0]
    res = call(name, return_gauge=True)
    k = m.k_uniform_mesh(mesh)
    evw = np.asarray(res.model.solve_all(k)).T                                        # (N_k, nw)
    evg = np.linalg.eigvalsh(np.einsum("kbm,kb,kbn->kmn", res.gauge.conj(), ref["energies"], res.gauge))
    worst_m = worst_g = 0.0
    count = 0
    for q, b in zip(*np.where(ref["frozen_mask"])):
        e = ref["energies"][q, b]
        worst_m = max(worst_m, np.min(np.abs(evw[q] - e)))
        worst_g = max(worst_g, np.min(np.abs(evg[q] - e)))
        count += 1
    print("%s: %d frozen eigenvalues; off the model's by %.2e, off the gauge's by %.2e" % (name, count, worst_m, worst_g))
    assert count > 0 and worst_m <= 1e-10 and worst_g <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain", "spinful"])
def test_full_subspace_agrees_with_wannier_mesh(name):
    m, mesh, trial, bands = {"chain": (chain(4), [16], CHAIN_TRIAL, [0, 1]), "spinful": (model("spinful"), [6, 5], [0, 1], [0, 1])}[name]
    a = m.wannier_mesh(mesh, trial, bands, max_iter=10, check_every=5, return_functions=True, return_gauge=True)
    b = m.wannier_disentangle_mesh(mesh, trial, bands, dis_iter=10, max_iter=10, check_every=5, return_functions=True, return_gauge=True)
    assert a.sv_min >= 0.1
    bound = 1e-10 * max(1.0, 1.0 / a.sv_min ** 2)
    d = {key: np.max(np.abs(np.asarray(getattr(a, key)) - np.asarray(getattr(b, key))))
         for key in ("centers", "spreads", "omega_i", "omega_od", "omega_d", "sv_min", "hoppings", "history", "functions", "gauge")}
    print("%s, nw = nb: bound %.2e; " % (name, bound) + ", ".join("%s %.2e" % kv for kv in d.items()))
    assert max(d.values()) <= bound, d
    assert b.dis_gap_min == np.inf and abs(b.sv_min_projection - a.sv_min) <= bound
    assert np.max(np.abs(b.dis_history - b.dis_history[0])) <= 1e-12
    p = m.wannier_mesh(mesh, trial, bands)
    assert abs(b.dis_history[0] - p.omega_i) <= bound


@pytest.mark.gpu
def test_omega_i_does_not_depend_on_the_trial_gauge():
    name = "chain6-frozen"
    m, mesh, trial, bands, kw = cases()[name]
    ref, A = ref_pair(name)
    mat = np.zeros((6, 2), dtype=complex)
    for w, fn in enumerate(CHAIN_TRIAL):
        for amp, s, R in fn:
            mat[s, w] = amp
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
    a = m.wannier_disentangle_mesh(mesh, mat, bands, **kw)
    b = m.wannier_disentangle_mesh(mesh, mat @ Q, bands, **kw)
    d = np.max(np.abs(a.dis_history - b.dis_history))
    print("Omega_I under a rotation of the trial functions: %.2e (A = %.2f)" % (d, A))
    assert A <= 1e4 and d <= 1e-10 * A


# ---------------------------------------------------------------- GPU: determinism
@pytest.mark.gpu
def test_two_calls_give_the_same_bits_and_short_runs_are_prefixes():
    kw = dict(max_iter=20, check_every=5, return_functions=True, return_gauge=True)
    a = call("spinful-both", dis_iter=20, **kw)
    b = call("spinful-both", dis_iter=20, **kw)
    for key in ("centers", "spreads", "hoppings", "history", "dis_history", "functions", "gauge", "n_window", "n_frozen"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    assert (a.omega_i, a.omega_od, a.omega_d, a.sv_min, a.sv_min_projection, a.dis_gap_min) == \
        (b.omega_i, b.omega_od, b.omega_d, b.sv_min, b.sv_min_projection, b.dis_gap_min)
    c = call("spinful-both", dis_iter=10, check_every=5)
    assert c.dis_history.shape == (3,) and a.dis_history.shape == (5,)
    assert np.array_equal(c.dis_history, a.dis_history[:3])
    d = call("spinful-both", dis_iter=20, max_iter=10, check_every=5)
    assert d.history.shape == (3,) and np.array_equal(d.history, a.history[:3]) and np.array_equal(d.dis_history, a.dis_history)
    e = call("chain40-32", return_gauge=True)                                          # the 32 x 32 solver
    f = call("chain40-32", return_gauge=True)
    assert np.array_equal(e.gauge, f.gauge) and np.array_equal(e.dis_history, f.dis_history)


# ---------------------------------------------------------------- GPU: the shell search on an fcc lattice
@pytest.mark.gpu
def test_shells_on_fcc_against_reference():
    m = model("fcc")
    with pytest.raises(Exception, match="too skewed"):
        m.wannier_mesh([4, 4, 4], [0], [0])
    # one function from one band: wdis_ref with nw = nb and no windows is section 34's projection
    ref = wd.run(m, [4, 4, 4], [0], [0], dis_iter=0, b_vectors="shells")
    assert ref["sv_min"] >= 0.1
    bound = 1e-10 * max(1.0, 1.0 / ref["sv_min"] ** 2)
    res = m.wannier_mesh([4, 4, 4], [0], [0], b_vectors="shells")
    d = {key: np.max(np.abs(np.asarray(getattr(res, key)) - ref[key]))
         for key in ("centers", "spreads", "omega_i", "omega_od", "omega_d", "sv_min", "hoppings", "history")}
    print("fcc, one band: sv_min %.3f, Omega %.5f, bound %.2e; " % (res.sv_min, res.omega, bound) + ", ".join("%s %.2e" % kv for kv in d.items()))
    assert max(d.values()) <= bound, d
    assert len(res.b_weights) == 4 and np.max(np.abs(res.b_vectors - ref["b_vectors"])) <= 1e-13
    ref2, A = ref_pair("fcc")
    res2 = call("fcc", return_gauge=True)
    compare(res2, ref2, bound_of(ref2, A), "fcc, two bands (A = %.2f)" % A)
    assert res2.dis_history[-1] <= res2.dis_history[0]
