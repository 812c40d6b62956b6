"""tb_model.wannier_mesh against tests/wan_ref.py and against exact identities.

Bounds.  Projection (max_iter = 0): 1e-10 max(1, 1 / sv_min^2) with sv_min from the reference, asserted >= 0.1 -- the Loewdin factor
(A+ A)^-1/2 amplifies the rounding of A by the inverse square of its smallest singular value.  Iterated runs: 1e-10 A, with A the
amplification of a 1e-9 change of one trial amplitude between two REFERENCE runs (floored at 1, asserted <= 1e4), the rule of
tests/test_mean_field.py.  Identities: each bound stands next to its test (DESIGN.md section 34 lists them with the measured values)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as hp
import wan_ref as wr
from helpers import quiet

import pythtb_amd as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- models
def honeycomb(delta, nspin=1):
    m = quiet(tb.tb_model, 2, 2, hp.LAT, hp.ORB, nspin=nspin)
    m.set_onsite([-delta, delta])
    m.set_hop(-1.0, 0, 1, [0, 0])
    m.set_hop(-1.0, 1, 0, [1, 0])
    m.set_hop(-1.0, 1, 0, [0, 1])
    return m


def spinful_honeycomb():
    """Gapped honeycomb with a spin-dependent hop and a Zeeman term: two non-degenerate lower bands."""
    m = honeycomb(0.7, nspin=2)
    m.set_onsite([0.0, 0.0, 0.0, 0.15], 0, mode="add")
    m.set_onsite([0.0, 0.0, 0.0, 0.10], 1, mode="add")
    m.set_hop([0.0, 0.0, 0.12j, 0.05], 0, 1, [1, 0], mode="add", allow_conjugate_pair=True)
    return m


def chain(norb, pot=0.6):
    """The chain of tests/test_mean_field.py: norb orbitals evenly spaced, alternating hops, an incommensurate potential."""
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
    """2 x 2 x 2 orbitals in a cubic cell at staggered on-site energies, nearest-neighbour hops of three strengths."""
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


CHAIN_TRIAL = [[(1.0, 0, [0]), (0.3, 1, [0])], [(1.0, 2, [0]), (-0.4, 3, [0])]]


def projection_cases():
    """name -> (model, mesh, trial, bands)."""
    c33 = chain(33)
    cub = cubic8()
    low = [i for i in range(8) if (i // 4 + (i // 2) % 2 + i % 2) % 2 == 0]
    return {
        "honeycomb": (honeycomb(0.7), [12, 12], [0], [0]),
        "spinful": (spinful_honeycomb(), [6, 5], [0, 1], [0, 1]),
        "chain": (chain(4), [16], CHAIN_TRIAL, [0, 1]),
        "chain-3-2": (chain(4), [16], CHAIN_TRIAL, [0, 1, 2]),
        "chain33": (c33, [8], [[(1.0, o, [0]) for o in blk] for blk in (range(0, 8), range(8, 16), range(16, 24), range(24, 33))],
                    [0, 1, 2, 3]),
        "cubic": (cub, [4, 3, 5], low, [0, 1, 2, 3]),
        "shifted": (chain(4), [16], [[(1.0, 0, [0]), (0.3, 3, [-1])], [(1.0, 2, [0]), (-0.4, 3, [0]), (0.1j, 0, [1])]], [0, 1]),
    }


_REF = {}


def ref_run(name, **kw):
    """The reference run of a case, computed once per set of keywords and shared."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        m, mesh, trial, bands = projection_cases()[name]
        _REF[key] = wr.run(m, mesh, trial, bands, **kw)
    return _REF[key]


def compare(res, ref, bound, tag, functions=False):
    d = {
        "centers": np.max(np.abs(res.centers - ref["centers"])),
        "spreads": np.max(np.abs(res.spreads - ref["spreads"])),
        "omega_i": abs(res.omega_i - ref["omega_i"]),
        "omega_od": abs(res.omega_od - ref["omega_od"]),
        "omega_d": abs(res.omega_d - ref["omega_d"]),
        "sv_min": abs(res.sv_min - ref["sv_min"]),
        "hoppings": np.max(np.abs(res.hoppings - ref["hoppings"])),
        "history": np.max(np.abs(res.history - ref["history"])),
    }
    if functions:
        d["functions"] = np.max(np.abs(res.functions - ref["functions"]))
    print("%s: bound %.2e; " % (tag, bound) + ", ".join("%s %.2e" % kv for kv in d.items()))
    assert np.array_equal(res.R_list, ref["R_list"])
    assert max(d.values()) <= bound, d


# ---------------------------------------------------------------- CPU
def test_argument_errors_without_gpu():
    m = honeycomb(0.7)
    flat = quiet(tb.tb_model, 0, 2, hp.LAT, hp.ORB)
    with pytest.raises(Exception, match="dim_k"):
        flat.wannier_mesh([4], [0], [0])
    for bad in ([12, 2], [12], [2, 12]):
        with pytest.raises(Exception):
            m.wannier_mesh(bad, [0], [0])
    with pytest.raises(Exception, match="at least 3"):
        m.wannier_mesh([12, 2], [0], [0])
    with pytest.raises(Exception, match="more trial functions"):
        m.wannier_mesh([6, 6], [0, 1], [0])
    big = chain(40)
    with pytest.raises(Exception, match="at most 16 trial"):
        big.wannier_mesh([8], list(range(17)), list(range(20)))
    with pytest.raises(Exception, match="at most 32 bands"):
        big.wannier_mesh([8], [0], list(range(33)))
    with pytest.raises(Exception, match="twice"):
        m.wannier_mesh([6, 6], [0], [0, 0])
    with pytest.raises(Exception, match="out of range"):
        m.wannier_mesh([6, 6], [0], [2])
    with pytest.raises(Exception, match="out of range"):
        m.wannier_mesh([6, 6], [2], [0])
    with pytest.raises(Exception, match="out of range"):
        m.wannier_mesh([6, 6], [[(1.0, -1, [0, 0])]], [0])
    with pytest.raises(Exception, match="dim_r integers"):
        m.wannier_mesh([6, 6], [[(1.0, 0, [0])]], [0])
    with pytest.raises(Exception, match="stay resident"):
        m.wannier_mesh([8192, 8192], [0], [0])
    with pytest.raises(Exception, match="4096"):
        m.wannier_mesh([6, 6], [0], [0], R_list=np.zeros((4097, 2), dtype=int))
    for kw, pat in ((dict(tol=-1.0), "tol"), (dict(tol=np.nan), "tol"), (dict(max_iter=-1), "max_iter"), (dict(max_iter=65537), "max_iter"),
                    (dict(max_iter=1.5), "max_iter"), (dict(check_every=0), "check_every")):
        with pytest.raises(Exception, match=pat):
            m.wannier_mesh([6, 6], [0], [0], **kw)


def test_wan_check_program():
    """make wan-check: the host-only checks, caps, plans and the small eigen-solver, as a stand-alone program under the sanitizers."""
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "pythtb_amd", "csrc"), "wan-check"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "wan_plan_check: ok" in res.stdout


@pytest.mark.parametrize("lat, mesh", [
    (hp.LAT, [12, 12]), (hp.LAT, [8, 10]), (np.eye(3), [4, 3, 5]),
    ([[1.0, 0.0, 0.0], [0.3, 1.1, 0.0], [-0.2, 0.25, 0.9]], [5, 6, 4]), ([[1.3]], [7])])
def test_bvector_completeness(lat, mesh):
    lat = np.array(lat, dtype=float)
    dk = lat.shape[0]
    m = quiet(tb.tb_model, dk, dk, lat, [[0.0] * dk])
    steps, w, b = m._wannier_bvectors(np.array(mesh, dtype=np.int32))
    assert len(w) <= 6 and np.all(w > 0.0) and np.all(np.abs(steps) <= 1)
    assert np.max(np.abs(2.0 * np.einsum("b,bi,bj->ij", w, b, b) - np.eye(dk))) <= 1e-14
    rs, rw, rb = wr.bvectors(lat, mesh)
    assert np.array_equal(steps, rs) and np.max(np.abs(w - rw)) <= 1e-14 * np.max(rw) and np.max(np.abs(b - rb)) <= 1e-14
    if dk == 2 and mesh == [12, 12]:
        assert len(w) == 3 and np.max(np.abs(w - w[0])) <= 1e-14 * w[0]            # the three weights of the honeycomb star are equal


def test_bvector_too_skewed():
    m = quiet(tb.tb_model, 2, 2, [[1.0, 0.0], [0.9, 0.2]], [[0.0, 0.0]])           # a_0 . a_1 = 0.9 against |a_1|^2 = 0.85
    with pytest.raises(Exception, match="too skewed"):
        m._wannier_bvectors(np.array([6, 6], dtype=np.int32))
    with pytest.raises(Exception, match="too skewed"):
        m.wannier_mesh([6, 6], [0], [0])


# ---------------------------------------------------------------- GPU: against the reference
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["honeycomb", "spinful", "chain", "chain-3-2", "chain33", "cubic", "shifted"])
def test_projection_against_reference(name):
    m, mesh, trial, bands = projection_cases()[name]
    ref = ref_run(name, functions=True)
    assert ref["sv_min"] >= 0.1, ref["sv_min"]
    bound = 1e-10 * max(1.0, 1.0 / ref["sv_min"] ** 2)
    res = m.wannier_mesh(mesh, trial, bands, return_functions=True)
    assert res.iterations == 0 and not res.converged and res.history.shape == (1,)
    compare(res, ref, bound, name, functions=True)
    assert abs(res.omega - (res.omega_i + res.omega_od + res.omega_d)) <= 1e-14 * max(1.0, res.omega)
    assert abs(np.sum(res.spreads) - res.omega) <= 1e-12 * max(1.0, res.omega)


def test_trial_forms_agree_on_the_reference():
    """The three accepted forms of a trial function give the same term lists (the reference's parser against the package's)."""
    m = chain(4)
    mat = np.zeros((4, 2), dtype=complex)
    mat[0, 0], mat[1, 0], mat[2, 1], mat[3, 1] = 1.0, 0.3, 1.0, -0.4
    a = m._wannier_args([16], mat, [0, 1], 0, 0.0, 10, None)
    b = m._wannier_args([16], CHAIN_TRIAL, [0, 1], 0, 0.0, 10, None)
    for key in ("tptr", "tstate", "tR", "tamp"):
        assert np.array_equal(a[key], b[key])
    c = m._wannier_args([16], [0, 2], [0, 1], 0, 0.0, 10, None)
    assert np.array_equal(c["tstate"], [0, 2]) and np.array_equal(c["tptr"], [0, 1, 2]) and np.array_equal(c["R"], wr.torus([16]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain", "spinful"])
def test_iterated_against_reference(name):
    m, mesh, trial, bands = projection_cases()[name]
    terms = wr.trial_terms(m, trial)
    pert = [[(a, s, R) for a, s, R in fn] for fn in terms]
    a0, s0, R0 = pert[0][0]
    pert[0][0] = (a0 + 1e-9, s0, R0)
    full = lambda fn: [(a, s, np.array(R)) for a, s, R in fn]
    ref = wr.run(m, mesh, [full(f) for f in terms], bands, max_iter=20, check_every=5)
    ref2 = wr.run(m, mesh, [full(f) for f in pert], bands, max_iter=20, check_every=5)
    A = max(1.0, max(np.max(np.abs(ref2[k] - ref[k])) for k in ("centers", "spreads", "hoppings", "history")) / 1e-9)
    assert A <= 1e4, A
    res = m.wannier_mesh(mesh, trial, bands, max_iter=20, check_every=5)
    assert res.iterations == 20 and res.history.shape == (5,)
    compare(res, ref, 1e-10 * A, "%s iterated (A = %.2f)" % (name, A))
    assert np.all(np.diff(res.history) <= 1e-13), res.history


# ---------------------------------------------------------------- GPU: exact identities
@pytest.mark.gpu
def test_single_band_centre_is_the_berry_phase():
    m = chain(4)
    res = m.wannier_mesh([16], [0], [0])
    w = tb.wf_array(m, [17])
    w.solve_on_grid([0.0])
    phase = w.berry_phase([0], 0, contin=False)
    x = res.centers[0, 0] / 1.0                                                       # reduced: the lattice constant is 1
    d = (2.0 * np.pi * x - phase + np.pi) % (2.0 * np.pi) - np.pi
    print("2 pi x = %.12f, Berry phase = %.12f, difference %.2e" % (2.0 * np.pi * x, phase, d))
    assert abs(d) <= 1e-10


@pytest.mark.gpu
def test_omega_i_is_gauge_invariant():
    m = chain(4)
    a = m.wannier_mesh([16], CHAIN_TRIAL, [0, 1])
    b = m.wannier_mesh([16], [[(1.0, 1, [0]), (0.2j, 0, [0])], [(1.0, 3, [0]), (0.5, 2, [0])]], [0, 1])
    c = m.wannier_mesh([16], CHAIN_TRIAL, [0, 1], max_iter=20, check_every=20)
    print("Omega_I: %.15f, %.15f, after 20 iterations %.15f" % (a.omega_i, b.omega_i, c.omega_i))
    assert abs(a.omega_i - b.omega_i) <= 1e-10 and abs(a.omega_i - c.omega_i) <= 1e-10
    assert c.omega < a.omega


@pytest.mark.gpu
@pytest.mark.parametrize("name, mesh", [("honeycomb", [12, 12]), ("chain", [9])])
def test_full_torus_model_reproduces_the_bands(name, mesh):
    if name == "honeycomb":
        m, trial, bands = honeycomb(0.7), [0, 1], [0, 1]
    else:
        m, trial, bands = chain(4), [0, 1, 2, 3], [0, 1, 2, 3]
    res = m.wannier_mesh(mesh, trial, bands)
    k = m.k_uniform_mesh(mesh)
    ev = m.solve_all(k)
    evw = res.model.solve_all(k)
    print("%s: bands of the Wannier model against the model's, %.2e" % (name, np.max(np.abs(ev[bands] - evw))))
    assert np.max(np.abs(ev[bands] - evw)) <= 1e-10


@pytest.mark.gpu
def test_functions_are_orthonormal_on_the_torus():
    m, mesh, trial, bands = projection_cases()["chain"]
    res = m.wannier_mesh(mesh, trial, bands, max_iter=5, check_every=5, return_functions=True)
    N, nw = mesh[0], 2
    w = res.functions                                                                 # (nR, nsta, nw), R = -7 .. 8
    worst = 0.0
    for s in range(N):                                                                # the translate by s cells on the torus
        ws = np.roll(w, s, axis=0)
        ov = np.einsum("rjm,rjn->mn", w.conj(), ws)
        worst = max(worst, np.max(np.abs(ov - (np.eye(nw) if s == 0 else 0.0))))
    print("orthonormality of the functions and their translates: %.2e" % worst)
    assert worst <= 1e-12


@pytest.mark.gpu
def test_haldane_both_bands_localise_onto_the_orbitals():
    m = hp.haldane(tb.tb_model, delta=0.2, t2abs=0.3)
    rng = np.random.default_rng(1)
    Q, _ = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
    a = m.wannier_mesh([8, 8], Q, [0, 1])
    assert abs(a.omega_i) <= 1e-12
    res = m.wannier_mesh([8, 8], Q, [0, 1], max_iter=300, check_every=100)
    pos = np.array(hp.ORB) @ np.array(hp.LAT)
    d = min(np.max(np.abs(res.centers - pos)), np.max(np.abs(res.centers - pos[::-1])))
    print("Haldane, both bands: Omega %.3e -> %.3e, centres off the orbitals by %.2e" % (a.omega, res.omega, d))
    assert res.omega < 1e-10 and abs(res.omega_i) <= 1e-12
    assert d <= 1e-6


# ---------------------------------------------------------------- GPU: obstruction
@pytest.mark.gpu
def test_chern_band_refuses_a_trial_function():
    m = hp.haldane(tb.tb_model, delta=0.2, t2abs=0.3)
    with pytest.raises(Exception, match="trial functions are singular on the bands at k ="):
        m.wannier_mesh([12, 12], [0], [0])
    trivial = hp.haldane(tb.tb_model, delta=0.7, t2abs=0.1)
    res = trivial.wannier_mesh([12, 12], [0], [0])
    assert res.sv_min > 0.1


# ---------------------------------------------------------------- GPU: determinism
@pytest.mark.gpu
def test_two_calls_give_the_same_bits_and_a_short_run_is_a_prefix():
    m, mesh, trial, bands = projection_cases()["spinful"]
    a = m.wannier_mesh(mesh, trial, bands, max_iter=20, return_functions=True, return_gauge=True)
    b = m.wannier_mesh(mesh, trial, bands, max_iter=20, return_functions=True, return_gauge=True)
    for key in ("centers", "spreads", "hoppings", "history", "functions", "gauge"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    assert (a.omega_i, a.omega_od, a.omega_d, a.sv_min) == (b.omega_i, b.omega_od, b.omega_d, b.sv_min)
    c = m.wannier_mesh(mesh, trial, bands, max_iter=10)
    assert c.history.shape == (2,) and a.history.shape == (3,)
    assert np.array_equal(c.history, a.history[:2])
