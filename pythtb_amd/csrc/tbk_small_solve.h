// tbk_small_solve.h -- the small complex solve that k_chim_rpa (tbk_chim.hip) and k_gf_tmatrix (tbk_gf.hip,
// section 30) share: one matrix per workgroup of ONE wavefront, M = [A | B] (na rows of 2 na columns) in LDS, Gaussian elimination
// with partial pivoting (pivot: the largest |.|^2 of the column, the lowest row winning ties), back substitution, det = the signed
// product of the pivots.  Device only.
#pragma once
#include "tbk_internal.h"

// On entry M holds [A | B] and every lane of the wavefront has passed a barrier behind its writes.  Returns false -- for every lane
// alike -- at a pivot of squared modulus exactly 0 (M is then half eliminated and det is not meaningful); else M[r][na + c] =
// (A^-1 B)[r][c], det = det A, and every lane has passed a barrier behind the last write.
template <int NMAX>
__device__ __forceinline__ bool small_solve(cd (&M)[NMAX][2 * NMAX + 1], const int na, const int t, cd& det) {
    const int w2 = 2 * na;
    cd d{1.0, 0.0};
    for (int k = 0; k < na; ++k) {
        int piv = k;                                               // (every lane finds the same pivot from the same values)
        double best = cabs2(M[k][k]);
        for (int r = k + 1; r < na; ++r) {
            const double m2 = cabs2(M[r][k]);
            if (m2 > best) best = m2, piv = r;
        }
        if (best == 0.0) return false;
        __syncthreads();
        if (piv != k) {
            for (int c = t; c < w2; c += 64) {
                const cd x = M[k][c];
                M[k][c] = M[piv][c];
                M[piv][c] = x;
            }
            d = cd{-d.x, -d.y};
            __syncthreads();
        }
        const cd pv = M[k][k];
        d = cmul(d, pv);
        const cd inv{pv.x / best, -pv.y / best};
        // rows below k, columns right of k: lane (r, c); column k itself (the factors) and row k are only read
        const int nr = na - 1 - k, nc = w2 - 1 - k;
        for (int e = t; e < nr * nc; e += 64) {
            const int r = k + 1 + e / nc, c = k + 1 + e % nc;
            M[r][c] = csub(M[r][c], cmul(cmul(M[r][k], inv), M[k][c]));
        }
        __syncthreads();
    }
    // back substitution, one lane per column of the right-hand side
    if (t < na) {
        for (int r = na - 1; r >= 0; --r) {
            cd s = M[r][na + t];
            for (int c = r + 1; c < na; ++c) s = csub(s, cmul(M[r][c], M[c][na + t]));
            const cd pv = M[r][r];
            const double m2 = cabs2(pv);
            M[r][na + t] = cmul(s, cd{pv.x / m2, -pv.y / m2});
        }
    }
    __syncthreads();
    det = d;
    return true;
}
