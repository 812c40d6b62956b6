#!/usr/bin/env python3
"""A fixed list of solve_on_grid, solve_on_grid_flux, berry_flux and k-list solves that reaches every route the mesh-solve driver
(solve_window_impl, tbk_solve.hip), the flux driver (tbk_berry_flux_async, tbk_berry.hip) and launch_wave choose, every output
saved to one .npz:

    TBK_LIBRARY=<libtbk.so> python profiles/solve_flux_bits.py out.npz      run the calls with that library (a fresh process each)
    python profiles/solve_flux_bits.py --compare a.npz b.npz                compare two runs as uint64 views

Two builds that claim the same results must give equal files: the comparison has no tolerance (profiles/kubo_bits.py is the same
for the Kubo calls).  The list: solve_on_grid of 1 to 4 states at last-axis hopping ranges 0 to 5 (k_grid_rows<N, 0..4> and the
generic instance), a window with an offset, the periodic-image column solved on its own (TBK_GRID_IMG=0), k_grid_small
(TBK_GRID_KERNEL=1), TBK_GRID_SEG, 5 to 96 states on small meshes and in a window; solve_on_grid_flux of 2 and 4 states with one
and two bands; berry_flux on the row kernel, the slices kernel, the generic kernel and the three determinant routes (lanes,
chain-wave, and the workgroup LU through TBK_DET_BIG_FROM), each with and without plaquettes, on one slice and on several; the
deferred total flushed by the result call and carried by a following solve; and the supplied-matrix solves of
tests/test_regimes.py in every forced regime, forwards and backwards, so that the shared workspace is regrown between regimes."""
import contextlib
import io
import os
import sys

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))

from kubo_bits import compare  # noqa: E402  (the same comparison)


def main():
    import pythtb_amd as tb
    import helpers as hp
    import test_regimes as tr
    from pythtb_amd import _lib, multi

    out = {}

    def keep(name, a):
        assert name not in out, name
        if a is not None:
            out[name] = np.ascontiguousarray(np.asarray(a, dtype=None if np.iscomplexobj(a) else float)).view(float)

    def ranged(n, pm, seed):
        """n states on a square lattice, hoppings [1, r] for r = 0..pm: range pm along the last axis exactly."""
        rng = np.random.default_rng(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            m = tb.tb_model(2, 2, [[1.0, 0.0], [0.0, 1.0]], rng.random((n, 2)))
        m.set_onsite(list(rng.standard_normal(n)))
        for r in range(pm + 1):
            for i in range(n):
                m.set_hop(complex(rng.standard_normal(), rng.standard_normal()), i, (i + 1 + r) % n, [1, r])
        return m

    def solve(name, m, mesh, start, **window):
        w = tb.wf_array(m, mesh)
        gaps = w.solve_on_grid_window(start, **window) if window else w.solve_on_grid(start)
        keep(name + " gaps", gaps)
        keep(name + " vectors", w.to_host())
        return w

    # ---- solve_on_grid, up to 4 states: the row kernel per (states, range), its window and image forms, k_grid_small
    for n in (1, 2, 3, 4):
        for pm in range(6):
            m = ranged(n, pm, 100 * n + pm)
            solve("rows n%d pm%d" % (n, pm), m, [9, 70], [0.1, -0.3])
        m = ranged(n, 1, 100 * n + 1)
        solve("rows n%d 3 chunks" % n, m, [5, 131], [0.1, -0.3])
        solve("rows n%d window" % n, m, [4, 40], [0.1, -0.3], offset=[3, 30], global_mesh=[9, 70])         # ends at the global end
        solve("rows n%d window inside" % n, m, [4, 40], [0.1, -0.3], offset=[3, 7], global_mesh=[9, 70])
        for knob, val in (("TBK_GRID_IMG", 0), ("TBK_GRID_KERNEL", 1), ("TBK_GRID_SEG", 1), ("TBK_GRID_SEG", 100), ("TBK_GRID_OCC", 3)):
            with _lib.knob(knob, val):
                solve("rows n%d %s=%d" % (n, knob, val), m, [5, 131], [0.1, -0.3])
        m3 = hp.random_model(tb.tb_model, n, 3, 1, seed=50 + n, nhop=5 * n, rmax=1)
        solve("rows n%d 3-D" % n, m3, [5, 6, 66], [0.13, -0.21, 0.37])
    print("solve_on_grid up to 4 states", len(out), flush=True)

    # ---- solve_on_grid beyond 4 states: launch_wave's regimes on a mesh, whole and as a window
    for n, mesh in ((5, [9, 70]), (12, [6, 41]), (12, [40, 60]), (17, [5, 6]), (17, [48, 50]), (30, [5, 7]), (48, [4, 5]), (96, [3, 4])):
        m = hp.random_model(tb.tb_model, n, 2, 1, seed=300 + n, rmax=1)
        tag = "wave n%d %dx%d" % (n, mesh[0], mesh[1])
        solve(tag, m, mesh, [0.05, 0.07])
        solve(tag + " window", m, [mesh[0] - 1, mesh[1] - 2], [0.05, 0.07], offset=[1, 1], global_mesh=mesh)
    print("solve_on_grid beyond 4 states", len(out), flush=True)

    # ---- solve_on_grid_flux: 2 and 4 states, one and two bands
    for name, m, occs in (("haldane", hp.haldane(tb.tb_model, 0.2), ([0], [1], [0, 1])), ("kane_mele", hp.kane_mele(tb.tb_model), ([0], [0, 1]))):
        for mesh in ([65, 65], [130, 200]):
            for occ in occs:
                for knob, val in ((None, None), ("TBK_GRID_SEG", 2), ("TBK_FUSED_SUM", 0), ("TBK_FUSED_OCC", 3)):
                    w = tb.wf_array(m, mesh)
                    with _lib.knob(knob, val) if knob else contextlib.nullcontext():
                        gaps, tot = w.solve_on_grid_flux([-0.5, -0.5], occ)
                    tag = "fused %s %dx%d occ%s %s" % (name, mesh[0], mesh[1], occ, knob)
                    keep(tag + " gaps", gaps)
                    keep(tag + " total", [tot])
                    keep(tag + " vectors", w.to_host())
    print("solve_on_grid_flux", len(out), flush=True)

    # ---- berry_flux: every route, with and without plaquettes, one slice and several
    def flux(name, w, occ, pairs):
        for dirs in pairs:
            keep("%s dirs%s total" % (name, dirs), w.berry_flux(occ, list(dirs)))
            keep("%s dirs%s plaquettes" % (name, dirs), w.berry_flux(occ, list(dirs), individual_phases=True))

    pairs3 = [(0, 1), (1, 0), (0, 2), (1, 2)]
    for n, nspin, occ in ((1, 1, [0]), (2, 1, [0]), (2, 1, [0, 1]), (3, 1, [0, 2]), (2, 2, [0, 1]), (2, 2, [1, 2, 3])):
        tag = "flux n%dx%d occ%s" % (n, nspin, occ)
        m = hp.random_model(tb.tb_model, n, 2, nspin, seed=400 + 10 * n + nspin, nhop=4 * n, rmax=1)
        w = tb.wf_array(m, [70, 131])
        w.solve_on_grid([0.01, 0.02])
        flux(tag + " rows", w, occ, [(0, 1), (1, 0)])
        for ti in (1, 24):
            with _lib.knob("TBK_FLUX_TI", ti):
                flux(tag + " rows ti%d" % ti, w, occ, [(0, 1)])
        with _lib.knob("TBK_FLUX_FUSED", 1):
            flux(tag + " rows summed in the kernel", w, occ, [(0, 1)])
        m = hp.random_model(tb.tb_model, n, 3, nspin, seed=410 + 10 * n + nspin, nhop=4 * n, rmax=1)
        w = tb.wf_array(m, [9, 8, 70])
        w.solve_on_grid([0.01, 0.02, 0.03])
        flux(tag + " 3-D", w, occ, pairs3)                      # (0, 1), (1, 0): the slices kernel
        with _lib.knob("TBK_FLUX_SLICES", 0):
            flux(tag + " 3-D no slices kernel", w, occ, [(0, 1)])
    for n, nocc, knobs in ((6, 3, {}), (6, 3, {"TBK_CHAIN_WAVE": 2}), (6, 3, {"TBK_CHAIN_WAVE": 0}), (6, 3, {"TBK_DET_BIG_FROM": 2}),
                           (16, 8, {}), (16, 8, {"TBK_CHAIN_WAVE": 0}), (16, 5, {}), (12, 7, {"TBK_DET_BIG_FROM": 4}), (20, 10, {}),
                           (9, 9, {"TBK_CHAIN_WAVE": 0})):
        tag = "flux n%d nocc%d %s" % (n, nocc, "+".join("%s=%s" % kv for kv in knobs.items()) or "default")
        for mesh, start, pairs in (([23, 37], [0.01, 0.02], [(0, 1), (1, 0)]), ([5, 6, 19], [0.01, 0.02, 0.03], pairs3)):
            m = hp.random_model(tb.tb_model, n, len(mesh), 1, seed=500 + n + len(mesh), rmax=1)
            w = tb.wf_array(m, mesh)
            w.solve_on_grid(start)
            with tr.knobs(knobs):
                flux("%s %d-D" % (tag, len(mesh)), w, list(range(nocc)), pairs)
    print("berry_flux", len(out), flush=True)

    # ---- the deferred total: flushed by the result call, carried by a following solve, overwritten by the next flux call
    lib, ctx = _lib.lib, _lib.default_context()
    occ0, occ1 = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    for mesh, ti in (([9, 9], 1), ([700, 400], 1), ([130, 67], -1)):
        for defer in (1, 0):
            with _lib.knob("TBK_FLUX_TI", ti), _lib.knob("TBK_FLUX_DEFER", defer):
                tag = "deferred %dx%d ti%d defer%d " % (mesh[0], mesh[1], ti, defer)
                g = multi.GridSlab(lib, _lib, ctx, hp.haldane(tb.tb_model, 0.0), mesh)
                g.solve([-0.5, -0.5])
                g.flux(occ0)
                keep(tag + "flushed", g.flux_total())
                g.flux(occ0)
                g.solve([-0.45, -0.5])
                keep(tag + "carried", g.flux_total())
                keep(tag + "gaps of the carrying solve", g.gaps())
                g.flux(occ0)
                g.flux(occ1)
                keep(tag + "overwritten", g.flux_total())
                g.flux(occ1)
                g.solve_flux([-0.5, -0.5], occ0)
                keep(tag + "before a fused solve", g.flux_total())
                g.free()
    print("deferred totals", len(out), flush=True)

    # ---- supplied matrices and k lists through every regime; forwards, then backwards: the workspace is regrown between regimes
    cases = [(r, True) for r in tr.REGIMES] + [(r, False) for r in tr.EVAL_ONLY]
    for rnd, order in (("a", cases), ("b", cases[::-1])):
        for i, ((n, nk, kn, _), vectors) in enumerate(order):
            h = tr._matrices(n, nk, 1000 + n)
            with tr.knobs(kn):
                ev, vec = tr._eigh_batch(h, vectors=vectors)
            keep("eigh %s%d n%d evals" % (rnd, i, n), ev)
            keep("eigh %s%d n%d vectors" % (rnd, i, n), vec)
    rng = np.random.default_rng(7)
    for n in (2, 4, 5, 12, 17, 30, 48, 96):
        m = hp.random_model(tb.tb_model, n, 2, 1, seed=300 + n, rmax=1)
        for nk in (3, 2000, 40):
            k = rng.random((nk, 2))
            ev, vec = m.solve_all(k, eig_vectors=True)
            keep("list n%d nk%d evals" % (n, nk), ev)
            keep("list n%d nk%d vectors" % (n, nk), vec)
            keep("list n%d nk%d evals only" % (n, nk), m.solve_all(k))
        keep("list n%d uniform mesh" % n, m.solve_all_mesh([7, 9]))
    print("k lists", len(out), flush=True)

    np.savez(sys.argv[1], **out)
    print("saved %d arrays to %s (library %s)" % (len(out), sys.argv[1], os.environ.get("TBK_LIBRARY", "default")))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
