// tbk_wdis.h -- the host-only part of tbk_wdis.hip (disentangled Wannier functions with energy windows on uniform k meshes, DESIGN.md
// section 35): the argument checks and caps of tbk_wannier_dis_mesh beyond those of tbk_wannier_mesh (tbk_wan.h, whose wan_check runs
// first), the partitions of the new kernels and the layout of the workspace behind the one of section 34.  No device call:
// check/wdis_plan_check.cpp drives it on the host alone (make wdis-check).
//
// Caps beyond tbk_wan.h's:  the candidate eigenvectors V_bands[N_k][nb][nsta] stay resident, N_k nsta nb <= kTdStateCap = 2^26 c128
// (this takes the place of section 34's N_k nsta nw: M0 needs both k and k + b, which may fall in different solve chunks);  the
// overlaps M0[N_k][nbv][nb][nb] take N_k nbv nb^2 <= 2^26 c128;  0 <= dis_iter <= 65536;  0 < dis_mixing <= 1;  dis_tol >= 0;  the
// windows are absent or finite ordered pairs.
//
// Partition, a function of (mesh, nsta, nb, nw, the number of b-vectors) alone -- NOT of dis_iter, dis_tol, dis_mixing, check_every
// or the windows:
//   k_wdis_overlap   one (point, b-vector) item per workgroup of 256 lanes: lane t owns the entries t, t + 256, ... of the nb^2, both
//                    sides staged through LDS in tiles of WDIS_OV_TJ components, rows of WDIS_OV_TJ + 1
//   k_wdis_select, k_wdis_gauge, k_wdis_reduce   one wavefront per point or item
//   G                k-groups of the sum of Omega_I: wan_groups(N_k), the groups and slices of k_wan_sum
// Z_in is kept only when dis_mixing < 1 (a buffer's size, not a partition).
#pragma once
#include "tbk_wan.h"
#include "tbk_small_eig32.h"

#define WDIS_OV_TJ 32                                      // components per LDS tile of the M0 kernel
#define WDIS_OV_ROWS (2 * WAN_NB_MAX)                      // rows of WDIS_OV_TJ + 1 c128 in that tile
#define WDIS_OV_EPL (WAN_NB_MAX * WAN_NB_MAX / 256)        // entries per lane of the M0 kernel
#define WDIS_LDS_A (SE32_NMAX * SE32_LD)                   // c128 of the wavefront kernels' blocks: Z | P
#define WDIS_LDS_C (2 * WAN_NB_MAX * SE_LD)                // ... two nb x nw panels, or the compacted matrix
static const int64_t kWdisOverlapCap = (int64_t)1 << 26;  // c128 of M0
static const size_t kWdisLdsBudget = (size_t)64 << 10;    // static LDS per workgroup (of the CU's 160 KiB)

struct WdisArgs {
    int have_window = 0, have_frozen = 0;
    double window[2] = {0.0, 0.0}, frozen[2] = {0.0, 0.0};
    int dis_iter = 0, check_every = 10;
    double dis_mixing = 1.0, dis_tol = 0.0;
};

// the rules of the disentanglement itself; wan_check (tbk_wan.h) has taken the mesh, the bands, the trial terms, the star and the descent
static int wdis_check(const char* fn, int n, int64_t npts, int nb, int nbv, const WdisArgs& D) {
    TBK_REQUIRE(npts * n * nb <= kTdStateCap, TBK_EINVAL,
                "%s: %lld points x %d bands x %d components = %lld c128 of candidate states stay resident (at most %lld): coarsen the mesh", fn,
                (long long)npts, nb, n, (long long)(npts * n * nb), (long long)kTdStateCap);
    TBK_REQUIRE(npts * nbv * nb * nb <= kWdisOverlapCap, TBK_EINVAL,
                "%s: %lld points x %d b-vectors x %d^2 = %lld c128 of overlaps stay resident (at most %lld): coarsen the mesh", fn,
                (long long)npts, nbv, nb, (long long)(npts * nbv * nb * nb), (long long)kWdisOverlapCap);
    if (D.have_window)
        TBK_REQUIRE(std::isfinite(D.window[0]) && std::isfinite(D.window[1]) && D.window[0] <= D.window[1], TBK_EINVAL,
                    "%s: window = (%.17g, %.17g) (a finite pair lo <= hi)", fn, D.window[0], D.window[1]);
    if (D.have_frozen)
        TBK_REQUIRE(std::isfinite(D.frozen[0]) && std::isfinite(D.frozen[1]) && D.frozen[0] <= D.frozen[1], TBK_EINVAL,
                    "%s: frozen = (%.17g, %.17g) (a finite pair lo <= hi)", fn, D.frozen[0], D.frozen[1]);
    TBK_REQUIRE(D.dis_iter >= 0 && D.dis_iter <= kWanIterMax, TBK_EINVAL, "%s: dis_iter=%d (0..%d)", fn, D.dis_iter, kWanIterMax);
    TBK_REQUIRE(D.dis_mixing > 0.0 && D.dis_mixing <= 1.0, TBK_EINVAL, "%s: dis_mixing=%.17g (in (0, 1])", fn, D.dis_mixing);
    TBK_REQUIRE(D.dis_tol >= 0.0 && std::isfinite(D.dis_tol), TBK_EINVAL, "%s: dis_tol=%.17g (finite, >= 0)", fn, D.dis_tol);
    TBK_REQUIRE(D.check_every >= 1, TBK_EINVAL, "%s: check_every=%d (at least 1)", fn, D.check_every);
    return TBK_OK;
}

// static LDS of the kernels of tbk_wdis.hip, in bytes (the arrays they declare)
static inline size_t wdis_lds_overlap() { return (size_t)WDIS_OV_ROWS * (WDIS_OV_TJ + 1) * sizeof(cd); }
static inline size_t wdis_lds_select() {
    return (size_t)(2 * WDIS_LDS_A + WDIS_LDS_C) * sizeof(cd) + (size_t)(SE32_W + SE32_NMAX) * sizeof(double) + 4 * SE32_NMAX * sizeof(int);
}
static inline size_t wdis_lds_gauge() { return (size_t)(2 * WAN_NB_MAX * SE_LD + 5 * SE_NMAX * SE_LD) * sizeof(cd); }
static inline size_t wdis_lds_reduce() { return (size_t)(WDIS_LDS_A + 3 * WAN_NB_MAX * SE_LD) * sizeof(cd); }

// the workspace behind section 34's (WanPlan::total): offsets from the start of the one block
struct WdisPlan {
    WanPlan wan;                                              // the plan of section 34 for the same (mesh, nsta, nb, nw, nbv)
    int G = 0, nq = 0;
    int keep_zin = 0;
    enum { VB, AM, M0, UD0, UD1, ZIN, WIN, FRZ, NWIN, NFRZ, GAP, SVP, OPART, DISH, DISD, NBUF };
    size_t off[NBUF + 1];
    size_t total = 0;
};
static WdisPlan wdis_plan(int n, int dk, int64_t npts, const int32_t* mesh, int nb, int nw, int nbv, int64_t nterm, int max_iter, int nR,
                          int want_fn, int dis_iter, double dis_mixing) {
    WdisPlan p;
    const size_t D = sizeof(double), C = sizeof(cd);
    p.wan = wan_plan(n, dk, npts, mesh, nb, nw, nbv, nterm, max_iter, nR, want_fn);
    p.G = p.wan.G, p.nq = p.wan.nq;
    p.keep_zin = dis_mixing < 1.0 ? 1 : 0;
    size_t b[WdisPlan::NBUF];
    b[WdisPlan::VB] = (size_t)npts * nb * n * C;
    b[WdisPlan::AM] = (size_t)npts * nb * nw * C;
    b[WdisPlan::M0] = (size_t)npts * nbv * nb * nb * C;
    b[WdisPlan::UD0] = (size_t)npts * nb * nw * C;
    b[WdisPlan::UD1] = (size_t)npts * nb * nw * C;
    b[WdisPlan::ZIN] = p.keep_zin ? (size_t)npts * nb * nb * C : 0;
    b[WdisPlan::WIN] = (size_t)npts * sizeof(uint32_t);
    b[WdisPlan::FRZ] = (size_t)npts * sizeof(uint32_t);
    b[WdisPlan::NWIN] = (size_t)npts * sizeof(int32_t);
    b[WdisPlan::NFRZ] = (size_t)npts * sizeof(int32_t);
    b[WdisPlan::GAP] = (size_t)npts * D;
    b[WdisPlan::SVP] = (size_t)npts * D;
    b[WdisPlan::OPART] = (size_t)p.G * p.nq * D;
    b[WdisPlan::DISH] = (size_t)(dis_iter + 1) * D;
    b[WdisPlan::DISD] = (size_t)(dis_iter + 1) * D;
    p.off[0] = al256(p.wan.total);
    for (int i = 0; i < WdisPlan::NBUF; ++i) p.off[i + 1] = p.off[i] + al256(b[i]);
    p.total = p.off[WdisPlan::NBUF];
    return p;
}
