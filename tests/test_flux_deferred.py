"""The deferred Berry-flux total (TBK_FLUX_DEFER, default 1): tbk_berry_flux_async leaves the sum of its partials pending and the
next row-kernel mesh solve of the same array does it in one extra workgroup; tbk_berry_flux_result, and every call that would
overwrite the partials or the totals, launches the stand-alone k_flux_reduce first.  Both forms share one summation function, so
"equal" below means the same float64 bits, and "stand-alone" means the same calls under TBK_FLUX_DEFER=0.

The Haldane model of tests/helpers.py through the C ABI, as multi.GridSlab drives it.  TBK_FLUX_TI=1 gives small meshes many
partials: [9, 9] 2, [700, 400] 1224 (more than 1024: one load per virtual thread), [1500, 760] 4872 (the second trip of the
stride-4096 loop); [130, 67] runs with the default tile height."""
import ctypes as C

import numpy as np
import pytest

import helpers as hp

pytestmark = pytest.mark.gpu

START = [-0.5, -0.5]
OCC0 = np.array([0], dtype=np.int32)
OCC1 = np.array([1], dtype=np.int32)
# (mesh, TBK_FLUX_TI)
SIZES = {"a": ([9, 9], 1), "b": ([700, 400], 1), "c": ([1500, 760], 1), "d": ([130, 67], -1)}


@pytest.fixture(scope="module")
def tb():
    import pythtb_amd
    pythtb_amd._lib.default_context()
    return pythtb_amd


@pytest.fixture(scope="module")
def models(tb):
    return {d: hp.haldane(tb.tb_model, d) for d in (0.0, 0.7, 1.2)}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def slab(tb, model, mesh, row0=0, global_n0=None):
    """multi.GridSlab plus the calls it does not wrap: flux along given directions / with plaquettes, sampled eigenvectors."""
    from pythtb_amd import _lib, multi

    class Slab(multi.GridSlab):
        def solve_with(self, other_model, start=START):
            self.hm = other_model._device_model()
            self.solve(start)

        def flux_dirs(self, occ32, d0, d1, want_plaq):
            self._lib.check(self.lib.tbk_berry_flux_async(self.h, self._lib.iptr(occ32), len(occ32), d0, d1, 1 if want_plaq else 0))

        def result(self, nslices=1, nplaq=0):
            t = np.zeros(nslices)
            p = np.zeros(nplaq) if nplaq else None
            self._lib.check(self.lib.tbk_berry_flux_result(self.h, self._lib.dptr(t), self._lib.dptr(p)))
            return t, p

        def points(self, idx):
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            out = np.zeros((len(idx), self.n, self.n), dtype=np.complex128)
            self._lib.check(self.lib.tbk_wfs_download_points(self.h, idx.ctypes.data_as(C.POINTER(C.c_int64)), len(idx),
                                                             self._lib.dptr(out)))
            return out

    return Slab(_lib.lib, _lib, _lib.default_context(), model, mesh, row0, global_n0)


def standalone(tb, model, mesh, ti, occ=OCC0, row0=0, global_n0=None):
    """solve; flux; result with the reduction launched inside tbk_berry_flux_async."""
    from pythtb_amd import _lib
    with _lib.knob("TBK_FLUX_TI", ti), _lib.knob("TBK_FLUX_DEFER", 0):
        g = slab(tb, model, mesh, row0, global_n0)
        g.solve(START)
        g.flux(occ)
        tot = g.flux_total()
        g.free()
    return tot


_REF = {}


def reference(tb, models, size, delta=0.0, occ=0):
    key = (size, delta, occ)
    if key not in _REF:
        mesh, ti = SIZES[size]
        _REF[key] = standalone(tb, models[delta], mesh, ti, OCC1 if occ else OCC0)
    return _REF[key]


def check_default_path(tb, model, mesh, ti, ref, row0=0, global_n0=None):
    from pythtb_amd import _lib
    with _lib.knob("TBK_FLUX_TI", ti):
        g = slab(tb, model, mesh, row0, global_n0)
        g.solve(START)
        g.flux(OCC0)
        g.solve(START)                       # carries the reduction
        folded = g.flux_total()
        g.solve(START)
        g.flux(OCC0)
        plain = g.flux_total()               # nothing folded: the result call launches the reduction
        g.free()
    assert same(folded, ref), (folded, ref)
    assert same(plain, ref), (plain, ref)


@pytest.mark.parametrize("size", sorted(SIZES))
def test_default_path_equals_standalone(tb, models, size):
    mesh, ti = SIZES[size]
    ref = reference(tb, models, size)
    assert np.isfinite(ref).all()
    if size != "a":
        assert round(float(ref[0]) / (2 * np.pi)) == -1     # (the Haldane model at delta = 0: Chern number -1)
    check_default_path(tb, models[0.0], mesh, ti, ref)


@pytest.mark.parametrize("delta", [0.7, 1.2])
@pytest.mark.parametrize("size", ["b", "d"])
def test_carried_total_is_the_old_one(tb, models, size, delta):
    """delta = 0.7 is still the Chern phase (|delta| < 3 sqrt(3) |t2| = 0.78): its total may round to the first model's bits, as it
    does at [130, 67].  delta = 1.2 is the trivial phase, total ~ 0: there a total handed to the wrong call cannot go unnoticed."""
    from pythtb_amd import _lib
    mesh, ti = SIZES[size]
    first, second = reference(tb, models, size, 0.0), reference(tb, models, size, delta)
    if delta > 1.0:
        assert abs(first[0] + 2 * np.pi) < 1e-9 and abs(second[0]) < 1e-9
    with _lib.knob("TBK_FLUX_TI", ti):
        g = slab(tb, models[0.0], mesh)
        g.solve(START)
        g.flux(OCC0)
        g.solve_with(models[delta])          # the array now holds the second model; the carried total is the first model's
        got_first = g.flux_total()
        g.flux(OCC0)
        got_second = g.flux_total()
        g.free()
    assert same(got_first, first), (got_first, first)
    assert same(got_second, second), (got_second, second)


@pytest.mark.parametrize("size", ["b", "d"])
def test_overwrites_flush_first(tb, models, size):
    from pythtb_amd import _lib
    mesh, ti = SIZES[size]
    ref1 = reference(tb, models, size, 0.0, occ=1)
    with _lib.knob("TBK_FLUX_TI", ti):
        g = slab(tb, models[0.0], mesh)
        g.solve(START)
        g.flux(OCC0)
        g.flux(OCC1)
        got = g.flux_total()
        g.free()
        with _lib.knob("TBK_FLUX_DEFER", 0):
            f = slab(tb, models[0.0], mesh)
            f.solve_flux(START, OCC0)
            fused_ref = f.flux_total()
            f.free()
        g = slab(tb, models[0.0], mesh)
        g.solve(START)
        g.flux(OCC0)
        g.solve_flux(START, OCC0)
        fused = g.flux_total()
        g.free()
    assert same(got, ref1), (got, ref1)
    assert same(fused, fused_ref), (fused, fused_ref)


def test_fallbacks_slices_and_plaquettes(tb, models):
    """More than one slice, or plaquettes requested: the reduction is launched at once, as before."""
    from pythtb_amd import _lib
    lib = _lib.lib
    # a 3-D array [9, 9, 17] of Haldane states: plane i2 holds the model with delta = 0.05 i2 on the 9 x 9 mesh
    planes = []
    for i2 in range(17):
        w = tb.wf_array(hp.haldane(tb.tb_model, 0.05 * i2), [9, 9])
        w.solve_on_grid(START)
        planes.append(np.asarray(w.to_host()).reshape(9, 9, 2, 2))
    host = np.ascontiguousarray(np.stack(planes, axis=2), dtype=np.complex128)     # [9][9][17][band][comp]
    out = {}
    for defer in (1, 0):
        with _lib.knob("TBK_FLUX_DEFER", defer):
            h = C.c_void_p()
            m32 = np.array([9, 9, 17], dtype=np.int32)
            _lib.check(lib.tbk_wfs_create(_lib.default_context().handle, 3, _lib.iptr(m32), 2, 2, C.byref(h)))
            _lib.check(lib.tbk_wfs_upload(h, _lib.dptr(host)))
            _lib.check(lib.tbk_berry_flux_async(h, _lib.iptr(OCC0), 1, 0, 1, 0))
            t3 = np.zeros(17)
            _lib.check(lib.tbk_berry_flux_result(h, _lib.dptr(t3), None))
            _lib.check(lib.tbk_wfs_free(h))
            g = slab(tb, models[0.0], [130, 67])
            g.solve(START)
            g.flux_dirs(OCC0, 0, 1, True)
            g.solve(START)
            t2, p2 = g.result(1, 129 * 66)
            g.free()
            out[defer] = (t3, t2, p2)
    # (the total of a closed plane is 2 pi times an integer whatever the mesh; across the planes the integer changes with delta)
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0] / (2 * np.pi) - np.round(out[0][0] / (2 * np.pi))).max() < 1e-9
    assert same(out[1][0], out[0][0])
    assert same(out[1][1], out[0][1])
    assert same(out[1][2], out[0][2])
    assert same(out[0][1], reference(tb, models, "d"))


def test_slab_window(tb, models):
    """Rows [37, 167) of a global mesh of 300 rows."""
    mesh, row0, g_n0 = [130, 67], 37, 300
    ref = standalone(tb, models[0.0], mesh, 1, row0=row0, global_n0=g_n0)
    assert not same(ref, standalone(tb, models[0.0], mesh, 1))
    check_default_path(tb, models[0.0], mesh, 1, ref, row0, g_n0)


def test_free_with_a_pending_reduction(tb, models):
    from pythtb_amd import _lib
    mesh, ti = SIZES["b"]
    with _lib.knob("TBK_FLUX_TI", ti):
        g = slab(tb, models[0.0], mesh)
        g.solve(START)
        g.flux(OCC0)
        assert _lib.lib.tbk_wfs_free(g.h) == 0
    check_default_path(tb, models[0.0], mesh, ti, reference(tb, models, "b"))


def test_the_fold_is_really_taken(tb, models):
    from pythtb_amd import _lib
    ctx = _lib.default_context()
    mesh, ti = SIZES["b"]
    counts, totals = {}, {}
    for defer in (None, 0):
        with _lib.knob("TBK_FLUX_TI", ti), _lib.knob("TBK_FLUX_DEFER", defer):
            g = slab(tb, models[0.0], mesh)
            g.solve(START)                   # (tables and buffers allocated before the counted launches)
            ctx.sync()
            ctx.prof_enable(1)
            ctx.prof_reset()
            try:
                for _ in range(3):
                    g.solve(START)
                    g.flux(OCC0)
                totals[defer] = g.flux_total()
                rep = ctx.prof_report()
            finally:
                ctx.prof_enable(0)
                ctx.prof_reset()
            g.free()
        counts[defer] = (rep["flux_reduce"]["launches"], rep["solve_grid"]["launches"], rep["berry_flux"]["launches"])
    assert counts[None] == (1, 3, 3), counts
    assert counts[0] == (3, 3, 3), counts
    assert same(totals[None], totals[0]) and same(totals[0], reference(tb, models, "b"))


@pytest.mark.parametrize("size", ["b", "d"])
def test_solve_that_carried_a_reduction_is_unchanged(tb, models, size):
    from pythtb_amd import _lib
    mesh, ti = SIZES[size]
    idx = np.unique(np.concatenate([np.random.default_rng(11).integers(0, mesh[0] * mesh[1], 500),
                                    [0, mesh[1] - 1, mesh[0] * mesh[1] - 1]]))
    with _lib.knob("TBK_FLUX_TI", ti):
        g = slab(tb, models[0.7], mesh)
        g.solve(START)
        gaps_plain, vec_plain = g.gaps(), g.points(idx)
        g.solve_with(models[0.0])
        g.flux(OCC0)
        g.solve_with(models[0.7])            # carries the reduction
        gaps_carry, vec_carry = g.gaps(), g.points(idx)
        tot = g.flux_total()
        g.free()
    assert same(gaps_carry, gaps_plain)
    assert np.array_equal(vec_carry.view(np.uint64), vec_plain.view(np.uint64))
    assert np.abs(vec_plain).max() > 0.1
    assert same(tot, reference(tb, models, size))


def _fresh_copy(tb, w, model, mesh):
    """A new wf_array (a new device array: none of its buffers sized yet) holding the vectors of `w`."""
    f = tb.wf_array(model, mesh)
    f._wfs = np.array(w.to_host())
    return f


def test_one_array_buffers_grow_and_shrink_3d(tb):
    """The per-array buffers (totals and counters, partials, plaquettes) of ONE array through planes of 20, 8 and 9 slices, with
    and without plaquettes, each route sizing them after another has: every result equals, bit for bit, the same call on a fresh
    array holding the same vectors."""
    mesh = [9, 8, 20]
    m = hp.random_model(tb.tb_model, 2, 3, 1, seed=77, nhop=8, rmax=1)
    w = tb.wf_array(m, mesh)
    w.solve_on_grid([0.01, 0.02, 0.03])
    calls = [((0, 1), False), ((1, 2), True), ((0, 2), False), ((0, 1), True), ((1, 2), False)]
    nsl = {(0, 1): 20, (1, 2): 9, (0, 2): 8}
    for dirs, ind in calls:
        got = np.asarray(w.berry_flux([0], list(dirs), individual_phases=ind))
        ref = np.asarray(_fresh_copy(tb, w, m, mesh).berry_flux([0], list(dirs), individual_phases=ind))
        assert got.shape[0] == nsl[dirs] and got.shape == ref.shape
        assert np.isfinite(ref).all() and np.abs(ref).max() > 1e-6
        assert same(got, ref), (dirs, ind)


def test_one_array_buffers_grow_and_shrink_2d(tb, models):
    """The same on a 2-D array, alternating the fused solve (its own partials and gap minima), plaquettes, and the row kernel at
    two tile heights (TBK_FLUX_TI: 4 rows, 80 partials; 24 rows, 16)."""
    from pythtb_amd import _lib
    mesh, m = [33, 40], models[0.0]
    w = tb.wf_array(m, mesh)

    for _ in range(2):
        gaps, tot = w.solve_on_grid_flux(START, [0])
        rgaps, rtot = tb.wf_array(m, mesh).solve_on_grid_flux(START, [0])
        assert same(gaps, rgaps) and same(tot, rtot) and round(tot / (2 * np.pi)) == -1
        plaq = w.berry_flux([0], individual_phases=True)
        assert plaq.shape == (32, 39) and same(plaq, _fresh_copy(tb, w, m, mesh).berry_flux([0], individual_phases=True))
        for ti in (4, 24):
            with _lib.knob("TBK_FLUX_TI", ti):
                assert same(w.berry_flux([0]), _fresh_copy(tb, w, m, mesh).berry_flux([0])), ti
