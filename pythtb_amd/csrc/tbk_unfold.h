// tbk_unfold.h -- the host-only part of tbk_unfold.hip (band unfolding: the weights of the eigenstates of a supercell on the Bloch sums of
// the primitive cell and the spectral function A(k, w) in the primitive zone): the argument checks of
// tbk_unfold_bands_list and tbk_unfold_spectral_list, the caps, the group tables, the plan of a call -- the chunk, the band tiles and
// lane shares of the projection, the accumulator tile of the broadening -- and the layout of the scratch block.  No device call:
// check/unfold_plan_check.cpp drives it on the host alone (make unfold-check).
//
// Caps:  nsta <= 2048 (the dense solver);  ng <= kUnfGroupsMax = 64 groups;  the result -- nsta nk ngo doubles of weights, or
// nk nw ngo doubles of A, ngo = ng per group and 1 for the total -- at most kUnfOutCap = 2^24 doubles (128 MiB).
//
// Tiling, a function of (nsta, ng, nw, nk) alone:
//   chunk   points per solve: kubo_chunk_len(nsta, nk), for the spectral function shortened so that the chunk's weights
//           W[chunk][nsta][ngo] stay under kUnfWBytes = 64 MiB
//   BT      bands per LDS load of the projection: min(nsta, 2048 / nsta), at least 1 -- a workgroup is (point, tile of BT bands)
//   NGP, L, BB   the lanes of a workgroup are BB bands x NGP group slots (the power of two >= ng) x L shares (min(32, 256 / NGP)):
//           share l of group g adds the members l, l + L, ... of the group in that order, then one lane adds the L shares in index order
//   GT      accumulators per lane of the broadening: the first of 1, 4, 16, 64 that holds ngo; a workgroup is (point, block of
//           UNF_FB = 256 frequencies), the bands go through LDS in strips of UNF_SB = 32
// In these kernels a point's numbers depend on nothing but that point's eigenpairs, a frequency's on nothing but that frequency: a
// frequency gives the same bits alone and inside a longer list, in any slot, and so does a point wherever the solver's route is the same.
#pragma once
#include "tbk_kubo.h"

#define UNF_FB 256                                        // frequencies per workgroup of k_unfold_spectral, a lane each
#define UNF_SB 32                                         // bands per strip of k_unfold_spectral
static const int kUnfStatesMax = 2048;                    // the dense solver's limit
static const int kUnfGroupsMax = 64;                      // groups (primitive orbitals x spin)
static const int kUnfLdsCd = 2048;                        // c128 of eigenvector components in LDS (32 KiB)
static const int64_t kUnfOutCap = (int64_t)1 << 24;       // doubles of a result
static const size_t kUnfWBytes = (size_t)64 << 20;        // bytes of a chunk's weights between the two kernels

// ---------------------------------------------------------------- checks
// k_sc[nk][dk] the supercell's k (solved as given), group[n] in [-1, ng) with at least one >= 0, phase_k[nk][dk] and delta[norb][dk]
// both given or both null, inv_nc = 1 / N_c; nw = 0: the bands call (no frequencies)
static int unf_check(const char* fn, int dk, int n, int norb, int64_t nk, const double* k_sc, int ng, const int32_t* group, const double* phase_k,
                     const double* delta, double inv_nc, int per_state, int nw, const double* omega, double eta) {
    TBK_REQUIRE(dk >= 1 && dk <= 3, TBK_EINVAL, "%s: dim_k=%d (k lists of 1, 2 or 3 dimensions)", fn, dk);
    TBK_REQUIRE(n >= 1 && n <= kUnfStatesMax, TBK_EINVAL,
                "%s: nsta=%d (at most %d, the dense solver's limit; kpm_unfolded_spectral unfolds larger supercells)", fn, n, kUnfStatesMax);
    TBK_REQUIRE(nk >= 1 && k_sc, TBK_EINVAL, "%s: nk=%lld (at least one k-point)", fn, (long long)nk);
    TBK_REQUIRE(ng >= 1 && ng <= kUnfGroupsMax, TBK_EINVAL, "%s: ng=%d (1..%d groups)", fn, ng, kUnfGroupsMax);
    TBK_REQUIRE(group, TBK_EINVAL, "%s: null group", fn);
    bool any = false;
    for (int j = 0; j < n; ++j) {
        TBK_REQUIRE(group[j] >= -1 && group[j] < ng, TBK_EINVAL, "%s: group[%d]=%d (-1..%d)", fn, j, group[j], ng - 1);
        any = any || group[j] >= 0;
    }
    TBK_REQUIRE(any, TBK_EINVAL, "%s: no state belongs to a group", fn);
    TBK_REQUIRE((phase_k == nullptr) == (delta == nullptr), TBK_EINVAL, "%s: phase_k and delta go together", fn);
    TBK_REQUIRE(std::isfinite(inv_nc) && inv_nc > 0.0, TBK_EINVAL, "%s: inv_nc must be finite and > 0", fn);
    const int64_t ngo = per_state ? ng : 1;
    const int64_t rows = nw ? (int64_t)nw : (int64_t)n;
    if (nw) {
        TBK_REQUIRE(omega, TBK_EINVAL, "%s: null omega", fn);
        int rc = kubo_omega_check(fn, nw, omega, eta);
        if (rc) return rc;
    }
    TBK_REQUIRE(nk <= kUnfOutCap && nk * rows * ngo <= kUnfOutCap, TBK_EINVAL, "%s: nk * %s * ng = %lld (at most %lld): split k_list or omega", fn,
                nw ? "nw" : "nsta", (long long)(nk * rows * ngo), (long long)kUnfOutCap);
    for (int64_t j = 0; j < nk * dk; ++j) {
        TBK_REQUIRE(std::isfinite(k_sc[j]), TBK_EINVAL, "%s: k-point %lld is not finite", fn, (long long)(j / dk));
        TBK_REQUIRE(!phase_k || std::isfinite(phase_k[j]), TBK_EINVAL, "%s: phase k-point %lld is not finite", fn, (long long)(j / dk));
    }
    if (delta)
        for (int j = 0; j < norb * dk; ++j) TBK_REQUIRE(std::isfinite(delta[j]), TBK_EINVAL, "%s: the displacement of orbital %d is not finite", fn, j / dk);
    return TBK_OK;
}

// ---------------------------------------------------------------- the group tables
// idx[off[g] .. off[g + 1]) = the states of group g in ascending order; states of group -1 appear nowhere
struct UnfGroups {
    std::vector<int32_t> off, idx;
};
static UnfGroups unf_groups(int n, int ng, const int32_t* group) {
    UnfGroups t;
    t.off.assign((size_t)ng + 1, 0);
    for (int j = 0; j < n; ++j)
        if (group[j] >= 0) ++t.off[(size_t)group[j] + 1];
    for (int g = 0; g < ng; ++g) t.off[(size_t)g + 1] += t.off[(size_t)g];
    t.idx.resize((size_t)t.off[(size_t)ng]);
    std::vector<int32_t> at(t.off.begin(), t.off.end() - 1);
    for (int j = 0; j < n; ++j)
        if (group[j] >= 0) t.idx[(size_t)at[(size_t)group[j]]++] = j;
    return t;
}

// ---------------------------------------------------------------- the plan
struct UnfPlan {
    int n = 0, ng = 0, ngo = 0;   // states, groups, groups of the result (1: the total)
    int64_t nk = 0, chunk = 0, nchunks = 0;
    int BT = 0, ntile = 0;        // bands per LDS load of k_unfold_weights and band tiles of a point
    int NGP = 0, L = 0, BB = 0;   // group slots, shares per group, bands side by side: BB NGP L <= 256
    int GT = 0;                   // accumulators per lane of k_unfold_spectral (0: the bands call)
    int nwb = 0;                  // blocks of UNF_FB frequencies
    int64_t out_d = 0;            // doubles of the result
    // the scratch block: 256 leading bytes, the solver's k list, the primitive k list and the displacements (phases only), omega, the
    // group offsets, the group members, the eigenvalues (bands call), the result, then the chunk workspace with the chunk's phases
    // ph[chunk][n] (extra 0) and weights W[chunk][n][ngo] (extra 1, spectral call)
    size_t off_k = 0, off_pk = 0, off_delta = 0, off_om = 0, off_goff = 0, off_idx = 0, off_ev = 0, off_out = 0, off_chunks = 0, total = 0;
    KuboChunks cw;
};
static UnfPlan unf_plan(int n, int dk, int norb, int64_t nk, int ng, int per_state, int nw, bool phases, int nidx) {
    UnfPlan p;
    p.n = n, p.ng = ng, p.ngo = per_state ? ng : 1, p.nk = nk;
    p.chunk = kubo_chunk_len(n, nk);
    if (nw) p.chunk = std::min<int64_t>(p.chunk, std::max<int64_t>(1, (int64_t)(kUnfWBytes / ((size_t)n * p.ngo * sizeof(double)))));
    p.nchunks = (nk + p.chunk - 1) / p.chunk;
    p.BT = std::max(1, std::min(n, kUnfLdsCd / n));
    p.ntile = (n + p.BT - 1) / p.BT;
    p.NGP = 1;
    while (p.NGP < ng) p.NGP *= 2;
    p.L = std::min(32, 256 / p.NGP);
    p.BB = 256 / (p.NGP * p.L);
    p.GT = !nw ? 0 : (p.ngo <= 1 ? 1 : (p.ngo <= 4 ? 4 : (p.ngo <= 16 ? 16 : 64)));
    p.nwb = (nw + UNF_FB - 1) / UNF_FB;
    p.out_d = nk * (nw ? (int64_t)nw : (int64_t)n) * p.ngo;
    const size_t D = sizeof(double);
    p.cw = KuboChunks(n, dk, p.chunk, phases ? (size_t)p.chunk * n * sizeof(cd) : 0, nw ? (size_t)p.chunk * n * p.ngo * D : 0, 0);
    p.off_k = 256;
    p.off_pk = p.off_k + al256((size_t)nk * dk * D);
    p.off_delta = p.off_pk + al256(phases ? (size_t)nk * dk * D : 0);
    p.off_om = p.off_delta + al256(phases ? (size_t)norb * dk * D : 0);
    p.off_goff = p.off_om + al256((size_t)nw * D);
    p.off_idx = p.off_goff + al256((size_t)(ng + 1) * sizeof(int32_t));
    p.off_ev = p.off_idx + al256((size_t)nidx * sizeof(int32_t));
    p.off_out = p.off_ev + al256(nw ? 0 : (size_t)n * nk * D);
    p.off_chunks = p.off_out + al256((size_t)p.out_d * D);
    p.total = p.off_chunks + p.cw.bytes();
    return p;
}
