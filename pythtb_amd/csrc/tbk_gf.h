// tbk_gf.h -- the host-only part of tbk_gf.hip (the lattice Green's function G(R, w) on k meshes, the T-matrix of a local impurity and
// the LDOS around it): the argument checks of tbk_green_function_mesh, tbk_impurity_t_matrix_mesh and
// tbk_impurity_ldos_mesh, the caps, the internal problem of the two impurity calls (the union of the probe and site states, the
// lattice vectors between probes and sites reduced modulo the mesh and de-duplicated, the index tables of the contraction), the plan
// of a call -- the chunk, k-groups, points per batch, frequency and R tiles -- and the layout of the scratch block.  No device call:
// check/gf_plan_check.cpp drives it on the host alone (make gf-check).
//
// Every partition here is a function of (mesh, n, dim_k) alone -- NOT of the number of frequencies, lattice vectors or selected
// states: a frequency or an R is worked through with the same groups whatever stands beside it, so it gives the same bits alone and
// inside a longer list.
#pragma once
#include <array>
#include <map>
#include "tbk_occ.h"

#define GF_WB 4                                          // frequencies per workgroup of the Green's-function kernels
#define GF_RB 2                                          // lattice vectors per workgroup
static const int kGfSelMax = 32;                         // selected states of tbk_green_function_mesh and probe states of the LDOS
static const int kGfSiteMax = 16;                        // sites of an impurity
static const int kGfSelIntMax = kGfSelMax + kGfSiteMax;  // states of the internal selection of tbk_impurity_ldos_mesh
static const int kGfIntRMax = 16384;                     // internal lattice vectors of an impurity call, after the reduction
static const int64_t kGfOutCap = (int64_t)1 << 22;       // nw nR na^2 of tbk_green_function_mesh at most (64 MiB of c128)
static const int64_t kGfIntCap = (int64_t)1 << 23;       // nw nR_int na_int^2 of an impurity call at most (128 MiB of c128)
static const int64_t kGfLdosCap = (int64_t)1 << 24;      // nw nR na doubles of dldos at most
static const int64_t kGfPartCap = (int64_t)1 << 22;      // c128 of group partials per launch (64 MiB)
static const int kGfGroupsMax = 512;                     // k-groups of a chunk

// ---------------------------------------------------------------- checks
static int gf_mesh_omega_check(const char* fn, int dk, int n, const int32_t* mesh, int nw, const double* omega, double eta, int64_t& npts) {
    int rc = occ_mesh_check(fn, dk, n, mesh, npts);
    if (rc) return rc;
    TBK_REQUIRE(omega, TBK_EINVAL, "%s: null omega", fn);
    return kubo_omega_check(fn, nw, omega, eta);
}
// nsel = 0 and sel = null: all states (na = n); else 1..kGfSelMax distinct indices in [0, n)
static int gf_sel_check(const char* fn, int n, int nsel, const int32_t* sel, int& na) {
    if (!sel) {
        TBK_REQUIRE(nsel == 0, TBK_EINVAL, "%s: nsel=%d without a selection", fn, nsel);
        na = n;
        return TBK_OK;
    }
    TBK_REQUIRE(nsel >= 1 && nsel <= kGfSelMax, TBK_EINVAL, "%s: nsel=%d (1..%d selected states)", fn, nsel, kGfSelMax);
    for (int i = 0; i < nsel; ++i) {
        TBK_REQUIRE(sel[i] >= 0 && sel[i] < n, TBK_EINVAL, "%s: selected state %d is %d (0..%d)", fn, i, sel[i], n - 1);
        for (int j = 0; j < i; ++j) TBK_REQUIRE(sel[j] != sel[i], TBK_EINVAL, "%s: state %d is selected twice", fn, sel[i]);
    }
    na = nsel;
    return TBK_OK;
}
static int gf_green_check(const char* fn, int dk, int n, const int32_t* mesh, int nw, const double* omega, double eta, int nR,
                          const int32_t* R, int nsel, const int32_t* sel, int64_t& npts, int& na) {
    int rc = gf_mesh_omega_check(fn, dk, n, mesh, nw, omega, eta, npts);
    if (!rc) rc = lat_R_check(fn, dk, nR, R);
    if (!rc) rc = gf_sel_check(fn, n, nsel, sel, na);
    if (rc) return rc;
    TBK_REQUIRE((int64_t)nw * nR * na * na <= kGfOutCap, TBK_EINVAL, "%s: nw * nR * na^2 = %lld (at most %lld): split omega or R_list", fn,
                (long long)nw * nR * na * na, (long long)kGfOutCap);
    return TBK_OK;
}
// a lattice vector reduced modulo the mesh: every component in [0, N_a)
static inline std::array<int32_t, 3> gf_reduce(int dk, const int32_t* mesh, const int64_t* R) {
    std::array<int32_t, 3> r{0, 0, 0};
    for (int d = 0; d < dk; ++d) {
        int64_t x = R[d] % mesh[d];
        if (x < 0) x += mesh[d];
        r[d] = (int32_t)x;
    }
    return r;
}
// the sites (state, R) of an impurity: 1..kGfSiteMax of them, distinct as sites of the torus; the potential V[ns][ns] (c128) finite
// and Hermitian to 1e-12 of its largest entry
static int gf_sites_check(const char* fn, int dk, int n, const int32_t* mesh, int ns, const int32_t* st, const int32_t* R, const double* V) {
    TBK_REQUIRE(ns >= 1 && ns <= kGfSiteMax && st && R, TBK_EINVAL, "%s: %d sites (1..%d)", fn, ns, kGfSiteMax);
    for (int a = 0; a < ns; ++a) {
        TBK_REQUIRE(st[a] >= 0 && st[a] < n, TBK_EINVAL, "%s: the state of site %d is %d (0..%d)", fn, a, st[a], n - 1);
        for (int d = 0; d < dk; ++d)
            TBK_REQUIRE(R[a * dk + d] > -kOccRAbsMax && R[a * dk + d] < kOccRAbsMax, TBK_EINVAL,
                        "%s: the lattice vector of site %d has a component of 2^30 or more", fn, a);
    }
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b < a; ++b) {
            int64_t d[3] = {0, 0, 0};
            for (int c = 0; c < dk; ++c) d[c] = (int64_t)R[a * dk + c] - R[b * dk + c];
            const std::array<int32_t, 3> r = gf_reduce(dk, mesh, d);
            TBK_REQUIRE(st[a] != st[b] || r[0] || r[1] || r[2], TBK_EINVAL, "%s: sites %d and %d coincide modulo the mesh", fn, b, a);
        }
    TBK_REQUIRE(V, TBK_EINVAL, "%s: null potential", fn);
    double big = 0.0;
    for (int i = 0; i < 2 * ns * ns; ++i) {
        TBK_REQUIRE(std::isfinite(V[i]), TBK_EINVAL, "%s: the potential is not finite", fn);
        big = std::max(big, fabs(V[i]));
    }
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b <= a; ++b) {
            const double dr = V[2 * (a * ns + b)] - V[2 * (b * ns + a)], di = V[2 * (a * ns + b) + 1] + V[2 * (b * ns + a) + 1];
            TBK_REQUIRE(fabs(dr) <= 1e-12 * big && fabs(di) <= 1e-12 * big, TBK_EINVAL, "%s: the potential is not Hermitian at (%d, %d)", fn, a,
                        b);
        }
    return TBK_OK;
}

// ---------------------------------------------------------------- the internal problem of the impurity calls
// What the two impurity calls ask of the Green's-function kernels.  The mesh cannot tell lattice vectors apart that differ by a
// period, so every difference is reduced modulo the mesh and kept once (in order of first appearance; index 0 is R = 0).
//   sel[na]          the internal selection: the probe states in the order given, then the site states not among them
//   R[nR][dk]        the internal lattice vectors
//   pos_site[ns]     the place of site a's state in sel;  pos_probe[np]: the place of probe state a in sel (= a)
//   pair[a][b]       the index of R_b - R_a:  g_ab = G_{i_a i_b}(R_b - R_a)
//   out[r][b], in[r][c]   the indices of R_b - R_r and R_r - R_c for probe cell r (LDOS only)
struct GfImpurity {
    int ns = 0, np = 0, nprobe = 0, na = 0, nR = 0;
    std::vector<int32_t> sel, R, pos_site, pos_probe, pair, out, in;
};
static GfImpurity gf_impurity_build(int dk, const int32_t* mesh, int ns, const int32_t* st, const int32_t* Rs, int nprobe, const int32_t* Rp,
                                    int np, const int32_t* probe) {
    GfImpurity g;
    g.ns = ns, g.np = np, g.nprobe = nprobe;
    for (int a = 0; a < np; ++a) {
        g.sel.push_back(probe[a]);
        g.pos_probe.push_back(a);
    }
    for (int a = 0; a < ns; ++a) {
        int at = -1;
        for (size_t i = 0; i < g.sel.size(); ++i)
            if (g.sel[i] == st[a]) at = (int)i;
        if (at < 0) {
            at = (int)g.sel.size();
            g.sel.push_back(st[a]);
        }
        g.pos_site.push_back(at);
    }
    g.na = (int)g.sel.size();
    std::map<std::array<int32_t, 3>, int> seen;
    auto index = [&](const int32_t* to, const int32_t* from) {
        int64_t d[3] = {0, 0, 0};
        for (int c = 0; c < dk; ++c) d[c] = (int64_t)to[c] - from[c];
        const std::array<int32_t, 3> r = gf_reduce(dk, mesh, d);
        auto it = seen.find(r);
        if (it != seen.end()) return it->second;
        const int at = (int)seen.size();
        seen.emplace(r, at);
        for (int c = 0; c < dk; ++c) g.R.push_back(r[c]);
        return at;
    };
    const int32_t zero[3] = {0, 0, 0};
    index(zero, zero);
    g.pair.resize((size_t)ns * ns);
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b < ns; ++b) g.pair[(size_t)a * ns + b] = index(Rs + b * dk, Rs + a * dk);
    g.out.resize((size_t)nprobe * ns);
    g.in.resize((size_t)nprobe * ns);
    for (int r = 0; r < nprobe; ++r)
        for (int b = 0; b < ns; ++b) {
            g.out[(size_t)r * ns + b] = index(Rs + b * dk, Rp + (int64_t)r * dk);
            g.in[(size_t)r * ns + b] = index(Rp + (int64_t)r * dk, Rs + b * dk);
        }
    g.nR = (int)seen.size();
    return g;
}
// the caps of an impurity call on its internal problem; nrows = nw nprobe np, the doubles of dldos (0: the T-matrix call)
static int gf_impurity_caps(const char* fn, const GfImpurity& g, int nw, int64_t nrows) {
    TBK_REQUIRE(g.na <= kGfSelIntMax, TBK_EINVAL, "%s: %d internal states (at most %d)", fn, g.na, kGfSelIntMax);
    TBK_REQUIRE(g.nR <= kGfIntRMax, TBK_EINVAL, "%s: %d distinct lattice vectors between probes and sites (at most %d): split R_list", fn, g.nR,
                kGfIntRMax);
    TBK_REQUIRE((int64_t)nw * g.nR * g.na * g.na <= kGfIntCap, TBK_EINVAL,
                "%s: nw * nR_int * na_int^2 = %lld (%d internal lattice vectors, %d internal states; at most %lld): split omega or R_list", fn,
                (long long)nw * g.nR * g.na * g.na, g.nR, g.na, (long long)kGfIntCap);
    TBK_REQUIRE(nrows <= kGfLdosCap, TBK_EINVAL, "%s: nw * nR * na = %lld (at most %lld): split omega or R_list", fn, (long long)nrows,
                (long long)kGfLdosCap);
    return TBK_OK;
}

// ---------------------------------------------------------------- the plan
// the partition of tbk_lat.h with na states kept and GF_WB x GF_RB (frequency, lattice vector) pairs per workgroup, and
struct GfPlan : LatPart {
    int na = 0, nab = 0;    // selected states and entries of a block
    int WT = 0, RT = 0;     // frequencies and lattice vectors per launch: part[G][WT][RT][nab] stays under kGfPartCap.  Every R where
                            // a frequency's partials fit, then as many frequencies as fit; else one block of frequencies and RT < nR
    int64_t part_cd = 0, acc_cd = 0;
    // the scratch block: 256 leading bytes, omega, the R list, the selection, acc[nw][nR][nab], part, the caller's extra bytes, then
    // the chunk workspace
    size_t off_om = 0, off_R = 0, off_sel = 0, off_acc = 0, off_part = 0, off_x = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};
static GfPlan gf_plan(int n, int dk, int64_t npts, int nw, int nR, int na, size_t extra) {
    GfPlan p;
    const int64_t nab = (int64_t)na * na;
    static_cast<LatPart&>(p) = lat_partition(n, na, npts, GF_WB * GF_RB, kGfPartCap, kGfGroupsMax);
    p.na = na, p.nab = (int)nab;
    const int64_t one = (int64_t)p.G * nR * nab;                  // part of one frequency, every R
    if (one <= kGfPartCap) {
        int64_t wt = kGfPartCap / one;
        if (wt >= GF_WB) wt -= wt % GF_WB;
        p.WT = (int)std::min<int64_t>(wt, nw);
        p.RT = nR;
    } else {
        p.WT = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nw, (int64_t)GF_WB, kGfPartCap / ((int64_t)p.G * nab)}));
        int64_t rt = std::max<int64_t>(1, kGfPartCap / ((int64_t)p.G * nab * p.WT));
        if (rt >= GF_RB) rt -= rt % GF_RB;
        p.RT = (int)std::min<int64_t>(rt, nR);
    }
    p.part_cd = (int64_t)p.G * p.WT * p.RT * nab;
    p.acc_cd = (int64_t)nw * nR * nab;
    p.cw = KuboChunks(n, dk, p.chunk, 0, 0, 0);
    p.off_om = 256;
    p.off_R = p.off_om + al256((size_t)nw * sizeof(double));
    p.off_sel = p.off_R + al256((size_t)nR * dk * sizeof(int32_t));
    p.off_acc = p.off_sel + al256((size_t)na * sizeof(int32_t));
    p.off_part = p.off_acc + al256((size_t)p.acc_cd * sizeof(cd));
    p.off_x = p.off_part + al256((size_t)p.part_cd * sizeof(cd));
    p.off_chunks = p.off_x + al256(extra);
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}

// the extra bytes of an impurity call behind part: the potential, the tables, T per frequency, det, the singular flags, and for
// the LDOS the two results.  Offsets from GfPlan.off_x.
struct GfImpLayout {
    size_t off_v = 0, off_tab = 0, off_t = 0, off_det = 0, off_flag = 0, off_ldos0 = 0, off_dldos = 0, total = 0;
    size_t tab_pos_site = 0, tab_pair = 0, tab_out = 0, tab_in = 0, tab_ints = 0;   // places (in int32) inside the one table upload
};
static GfImpLayout gf_imp_layout(int ns, int nw, int nprobe, int np) {
    GfImpLayout l;
    l.tab_pos_site = 0;
    l.tab_pair = l.tab_pos_site + (size_t)ns;
    l.tab_out = l.tab_pair + (size_t)ns * ns;
    l.tab_in = l.tab_out + (size_t)nprobe * ns;
    l.tab_ints = l.tab_in + (size_t)nprobe * ns;
    l.off_v = 0;
    l.off_tab = l.off_v + al256((size_t)ns * ns * sizeof(cd));
    l.off_t = l.off_tab + al256(l.tab_ints * sizeof(int32_t));
    l.off_det = l.off_t + al256((size_t)nw * ns * ns * sizeof(cd));
    l.off_flag = l.off_det + al256((size_t)nw * sizeof(cd));
    l.off_ldos0 = l.off_flag + al256((size_t)nw * sizeof(int32_t));
    l.off_dldos = l.off_ldos0 + al256((size_t)nw * np * sizeof(double));
    l.total = l.off_dldos + al256((size_t)nw * nprobe * np * sizeof(double));
    return l;
}
