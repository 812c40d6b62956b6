// tbk_int.h -- the state-indexed density-density interaction list V_ab(R) that tbk_mean_field_mesh, tbk_bdg_mesh and the exciton calls
// take (DESIGN.md sections 33, 36, 37 and 38): the rules of one entry and the one walk over the list.  Host only, no device call;
// check/mf_plan_check.cpp drives the walk directly (make mf-check).
#pragma once
#include <array>
#include <map>
#include "tbk_occ.h"

// the rules of entry e = (a, b, R, V): both states in range, V finite, |R| < 2^30, no self-interaction
static int int_entry_check(const char* fn, int dk, int n, int e, const int32_t* ab, const int32_t* R, const double* V) {
    const int a = ab[2 * e], b = ab[2 * e + 1];
    TBK_REQUIRE(a >= 0 && a < n && b >= 0 && b < n, TBK_EINVAL, "%s: interaction %d has a state index out of range", fn, e);
    TBK_REQUIRE(std::isfinite(V[e]), TBK_EINVAL, "%s: interaction %d is not finite", fn, e);
    bool zero = true;
    for (int d = 0; d < dk; ++d) {
        const int32_t r = R[(int64_t)e * dk + d];
        TBK_REQUIRE(r > -kOccRAbsMax && r < kOccRAbsMax, TBK_EINVAL, "%s: interaction %d has a lattice component of 2^30 or more", fn, e);
        zero = zero && r == 0;
    }
    TBK_REQUIRE(!(a == b && zero), TBK_EINVAL, "%s: interaction %d couples state %d to itself (a self-interaction)", fn, e, a);
    return TBK_OK;
}

// An entry (a, b, R) stands for the bond and its mirror (b, a, -R): given twice in either form it is refused.  What the walk leaves:
struct IntBonds {
    int nocc = 0, nR = 0;
    std::vector<int> occ_par;            // [n]: the place of a among the states some V touches, ascending a; -1 where none does
    std::vector<int32_t> Rl;             // [nR][dk]: R = 0 first, then the entries' vectors in order of first appearance
    std::vector<int> ent_r;              // [nint]: the index of an entry's R in Rl
    std::vector<double> rowsum;          // [n]: sum_b,R |V_ab(R)| (both directions of every bond)
};
static int int_bonds(const char* fn, int dk, int n, int nint, const int32_t* ab, const int32_t* R, const double* V, IntBonds& B) {
    B = IntBonds();
    B.occ_par.assign((size_t)n, -1);
    B.rowsum.assign((size_t)n, 0.0);
    B.Rl.assign((size_t)dk, 0);
    B.ent_r.resize((size_t)nint);
    std::map<std::array<int, 6>, int> seen;
    std::map<std::array<int, 4>, int> rid;
    rid[{0, 0, 0, 0}] = 0;
    for (int e = 0; e < nint; ++e) {
        const int a = ab[2 * e], b = ab[2 * e + 1];
        std::array<int, 4> r{0, 0, 0, 0};
        for (int d = 0; d < dk; ++d) r[d] = R[(int64_t)e * dk + d];
        const std::array<int, 6> k1{a, b, r[0], r[1], r[2], r[3]}, k2{b, a, -r[0], -r[1], -r[2], -r[3]};
        TBK_REQUIRE(!seen.count(k1) && !seen.count(k2), TBK_EINVAL, "%s: interaction %d repeats the bond of interaction %d (a bond is given once)",
                    fn, e, seen.count(k1) ? seen[k1] : seen[k2]);
        seen[k1] = e;
        B.occ_par[a] = B.occ_par[b] = 0;
        auto it = rid.find(r);
        if (it == rid.end()) {
            it = rid.emplace(r, (int)rid.size()).first;
            B.Rl.insert(B.Rl.end(), r.begin(), r.begin() + dk);
        }
        B.ent_r[e] = it->second;
        B.rowsum[a] += fabs(V[e]);
        B.rowsum[b] += fabs(V[e]);
    }
    B.nR = (int)rid.size();
    for (int a = 0; a < n; ++a)
        if (B.occ_par[a] == 0) B.occ_par[a] = B.nocc++;
    return TBK_OK;
}
