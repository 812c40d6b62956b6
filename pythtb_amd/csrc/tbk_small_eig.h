// tbk_small_eig.h -- the small Hermitian eigen-solver of tbk_wan.hip: the Loewdin factor (A+A)^-1/2 and the
// unitary step e^{dW} both come from it.  One matrix of at most 16 x 16 per wavefront, A and Q in LDS (rows of SE_LD), cyclic complex
// Jacobi in the fixed pair order (0,1), (0,2), ..., (n-2,n-1): a pair is rotated when |a_pq| exceeds 1e-18 of the Frobenius norm the
// matrix came in with, and the sweeps end after the first one that rotates nothing (SE_SWEEPS at most).  Every lane takes every
// decision from the same LDS values, so the wavefront never diverges on them.
//
// Host and device: the host plays the wavefront with one lane (check/wan_plan_check.cpp holds the arithmetic against matrices with
// known spectra); SE_SYNC is the workgroup barrier on the device -- the workgroup IS the wavefront -- and nothing on the host.
#pragma once
#include "tbk_internal.h"

#define SE_NMAX 16
#define SE_LD 17            // odd row length: a column walk of 16 lanes touches 16 different bank groups
#define SE_SWEEPS 40

#if defined(__HIP_DEVICE_COMPILE__)
#define SE_SYNC() __syncthreads()
#else
#define SE_SYNC() ((void)0)
#endif

// On entry A (Hermitian, n x n in rows of SE_LD) is written and every lane has passed a barrier behind the writes.  On return
// A = Q diag(lam) Q+ of the matrix that came in, lam[j] = Re A[j][j] in no particular order, the columns of Q orthonormal, and every
// lane has passed a barrier behind the last write.  lane / nl: this lane and the number of lanes playing (64 | 1).  Returns the
// number of sweeps taken (SE_SWEEPS + 1: the last allowed sweep still rotated).
__host__ __device__ inline int small_eig_jacobi(cd* A, cd* Q, const int n, const int lane, const int nl) {
    for (int e = lane; e < n * n; e += nl) Q[(e / n) * SE_LD + e % n] = cd{e / n == e % n ? 1.0 : 0.0, 0.0};
    double f2 = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) f2 += cabs2(A[r * SE_LD + c]);
    const double thr = 1e-18 * sqrt(f2);
    SE_SYNC();
    int sweep = 0;
    for (; sweep < SE_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const cd apq = A[p * SE_LD + q];
                const double g = sqrt(cabs2(apq));
                if (!(g > thr)) continue;                          // (uniform: every lane reads the same value)
                ++rotated;
                const double app = A[p * SE_LD + p].x, aqq = A[q * SE_LD + q].x;
                const double tau = (aqq - app) / (2.0 * g);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                const cd ph{apq.x / g, apq.y / g};                 // e^{i theta}
                const cd phc = cconj(ph);
                SE_SYNC();                                         // everyone has read a_pq, a_pp, a_qq
                // X <- X J, J's columns: p: c e_p - s e^{-i theta} e_q;  q: s e_p + c e^{-i theta} e_q
                for (int r = lane; r < n; r += nl) {
                    const cd xp = A[r * SE_LD + p], xq = cmul(A[r * SE_LD + q], phc);
                    A[r * SE_LD + p] = cd{c * xp.x - s * xq.x, c * xp.y - s * xq.y};
                    A[r * SE_LD + q] = cd{s * xp.x + c * xq.x, s * xp.y + c * xq.y};
                    const cd yp = Q[r * SE_LD + p], yq = cmul(Q[r * SE_LD + q], phc);
                    Q[r * SE_LD + p] = cd{c * yp.x - s * yq.x, c * yp.y - s * yq.y};
                    Q[r * SE_LD + q] = cd{s * yp.x + c * yq.x, s * yp.y + c * yq.y};
                }
                SE_SYNC();
                // A <- J+ A
                for (int k = lane; k < n; k += nl) {
                    const cd xp = A[p * SE_LD + k], xq = cmul(A[q * SE_LD + k], ph);
                    A[p * SE_LD + k] = cd{c * xp.x - s * xq.x, c * xp.y - s * xq.y};
                    A[q * SE_LD + k] = cd{s * xp.x + c * xq.x, s * xp.y + c * xq.y};
                }
                SE_SYNC();
                if (lane == 0) {                                   // the rotated pair is zero and the diagonal real, exactly
                    A[p * SE_LD + q] = cd{0.0, 0.0};
                    A[q * SE_LD + p] = cd{0.0, 0.0};
                    A[p * SE_LD + p].y = 0.0;
                    A[q * SE_LD + q].y = 0.0;
                }
                SE_SYNC();
            }
        if (!rotated) break;
    }
    return sweep + 1;
}
