// tbk_small_eig32.h -- the Hermitian eigen-solver of the disentanglement (tbk_wdis.hip): one matrix of at
// most 32 x 32 per wavefront, A and Q in LDS (rows of SE32_LD), complex Jacobi in round-robin (tournament) order.  A sweep is
// m - 1 rounds (m = n rounded up to even) of m / 2 disjoint pairs: index m - 1 stays, the others turn by one per round, and a pair
// that holds the padding index of an odd n is skipped.  Every angle of a round comes from the same LDS snapshot (lane i < m / 2
// works out pair i and leaves c, s, e^{i theta} and a flag in the small table W); then the column update A <- A J, Q <- Q J with
// J the product of the round's rotations, a lane per (row, pair), then the row update A <- J+ A, a lane per (pair, column), so that
// all 64 lanes work where the 16 x 16 routine of tbk_small_eig.h keeps at most n busy.  The threshold rule is that routine's: a pair
// is rotated when |a_pq| exceeds 1e-18 of the Frobenius norm the matrix came in with, and the sweeps end after the first one that
// rotates nothing.  Every lane takes every decision from the same LDS values, so the wavefront never diverges on them.
//
// Host and device: the host plays the wavefront with one lane (check/wdis_plan_check.cpp); the items of a phase touch disjoint
// entries, so one lane walking them in order computes what 64 lanes compute side by side.
#pragma once
#include "tbk_small_eig.h"

#define SE32_NMAX 32
#define SE32_LD 33          // odd row length
#define SE32_SWEEPS 40
#define SE32_W (5 * (SE32_NMAX / 2))   // doubles of the round's table: c, s, Re and Im e^{i theta}, rotated

// the pair i of round r for m (even) indices: p < q; (m - 1, r) for i = 0, else ((r + i) mod (m - 1), (r - i) mod (m - 1))
__host__ __device__ inline void se32_pair(const int m, const int r, const int i, int& p, int& q) {
    const int a = i == 0 ? m - 1 : (r + i) % (m - 1);
    const int b = i == 0 ? r : (r - i + (m - 1)) % (m - 1);
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// On entry A (Hermitian, n x n in rows of SE32_LD) is written and every lane has passed a barrier behind the writes.  On return
// A = Q diag(lam) Q+ of the matrix that came in, lam[j] = Re A[j][j] in no particular order, the columns of Q orthonormal, and every
// lane has passed a barrier behind the last write.  W: SE32_W doubles of LDS.  lane / nl: this lane and the number of lanes playing
// (64 | 1).  Returns the number of sweeps taken (SE32_SWEEPS + 1: the last allowed sweep still rotated).
__host__ __device__ inline int small_eig_jacobi32(cd* A, cd* Q, double* W, const int n, const int lane, const int nl) {
    for (int e = lane; e < n * n; e += nl) Q[(e / n) * SE32_LD + e % n] = cd{e / n == e % n ? 1.0 : 0.0, 0.0};
    double f2 = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) f2 += cabs2(A[r * SE32_LD + c]);
    const double thr = 1e-18 * sqrt(f2);
    const int m = (n + 1) & ~1, np = m / 2;
    SE_SYNC();
    int sweep = 0;
    for (; sweep < SE32_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < m - 1; ++r) {
            for (int i = lane; i < np; i += nl) {                  // the round's angles, all from this snapshot
                int p, q;
                se32_pair(m, r, i, p, q);
                double c = 1.0, s = 0.0, px = 1.0, py = 0.0, flag = 0.0;
                if (q < n) {
                    const cd apq = A[p * SE32_LD + q];
                    const double g = sqrt(cabs2(apq));
                    if (g > thr) {
                        const double app = A[p * SE32_LD + p].x, aqq = A[q * SE32_LD + q].x;
                        const double tau = (aqq - app) / (2.0 * g);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                        px = apq.x / g, py = apq.y / g;            // e^{i theta}
                        flag = 1.0;
                    }
                }
                W[5 * i] = c, W[5 * i + 1] = s, W[5 * i + 2] = px, W[5 * i + 3] = py, W[5 * i + 4] = flag;
            }
            SE_SYNC();
            int any = 0;
            for (int i = 0; i < np; ++i) any += W[5 * i + 4] != 0.0;   // (uniform: every lane reads the same values)
            if (any) {
                rotated += any;
                // X <- X J, J's columns of a pair: p: c e_p - s e^{-i theta} e_q;  q: s e_p + c e^{-i theta} e_q
                for (int e = lane; e < n * np; e += nl) {
                    const int row = e % n, i = e / n;
                    if (W[5 * i + 4] == 0.0) continue;
                    int p, q;
                    se32_pair(m, r, i, p, q);
                    const double c = W[5 * i], s = W[5 * i + 1];
                    const cd phc{W[5 * i + 2], -W[5 * i + 3]};
                    const cd xp = A[row * SE32_LD + p], xq = cmul(A[row * SE32_LD + q], phc);
                    A[row * SE32_LD + p] = cd{c * xp.x - s * xq.x, c * xp.y - s * xq.y};
                    A[row * SE32_LD + q] = cd{s * xp.x + c * xq.x, s * xp.y + c * xq.y};
                    const cd yp = Q[row * SE32_LD + p], yq = cmul(Q[row * SE32_LD + q], phc);
                    Q[row * SE32_LD + p] = cd{c * yp.x - s * yq.x, c * yp.y - s * yq.y};
                    Q[row * SE32_LD + q] = cd{s * yp.x + c * yq.x, s * yp.y + c * yq.y};
                }
                SE_SYNC();
                // A <- J+ A
                for (int e = lane; e < n * np; e += nl) {
                    const int k = e % n, i = e / n;
                    if (W[5 * i + 4] == 0.0) continue;
                    int p, q;
                    se32_pair(m, r, i, p, q);
                    const double c = W[5 * i], s = W[5 * i + 1];
                    const cd ph{W[5 * i + 2], W[5 * i + 3]};
                    const cd xp = A[p * SE32_LD + k], xq = cmul(A[q * SE32_LD + k], ph);
                    A[p * SE32_LD + k] = cd{c * xp.x - s * xq.x, c * xp.y - s * xq.y};
                    A[q * SE32_LD + k] = cd{s * xp.x + c * xq.x, s * xp.y + c * xq.y};
                }
                SE_SYNC();
                for (int i = lane; i < np; i += nl) {              // the rotated pairs are zero and their diagonal real, exactly
                    if (W[5 * i + 4] == 0.0) continue;
                    int p, q;
                    se32_pair(m, r, i, p, q);
                    A[p * SE32_LD + q] = cd{0.0, 0.0};
                    A[q * SE32_LD + p] = cd{0.0, 0.0};
                    A[p * SE32_LD + p].y = 0.0;
                    A[q * SE32_LD + q].y = 0.0;
                }
            }
            SE_SYNC();                                             // (behind the last reads of W and the last writes of A)
        }
        if (!rotated) break;
    }
    return sweep + 1;
}
