// tbk_chi_dev.h -- the device code that the two susceptibility units share (tbk_chi.hip; tbk_chim.hip, section
// 28): the occupation weights of an ordered pair (n at k, m at k + q) and the k + q kernel.  The library is built without relocatable
// device code, so the kernel is static: each unit that launches it holds its own definition and host stub.
#pragma once
#include "tbk_kubo.h"

// ---------------------------------------------------------------- occupation weights
// f_n - f_m without cancellation: sinh h / (cosh h + cosh u), h = (E_m - E_n) / 2kT, u = ((E_n + E_m) / 2 - mu) / kT, by tbk_kubo.h's
// FermiPair
__device__ __forceinline__ double chi_fdiff(const double en, const double em, const double mu, const double kT) {
    if (kT == 0.0) return (en <= mu ? 1.0 : 0.0) - (em <= mu ? 1.0 : 0.0);
    const double h = 0.5 * (em - en) / kT;
    const FermiPair p(fabs(h), fabs((0.5 * (en + em) - mu) / kT));
    const double mag = -p.num() / p.den;
    return h < 0.0 ? -mag : mag;
}
// L = -(f_n - f_m) / (E_n - E_m) = (sinh h / h) / (2 kT (cosh h + cosh u)): smooth through h = 0, where it is -f'(E)
__device__ __forceinline__ double chi_static_weight(const double en, const double em, const double mu, const double kT) {
    if (kT == 0.0) {
        const bool fn = en <= mu, fm = em <= mu;
        return fn == fm ? 0.0 : (fn ? 1.0 : -1.0) / (em - en);
    }
    const double a = fabs(0.5 * (em - en) / kT);
    const FermiPair p(a, fabs((0.5 * (en + em) - mu) / kT));
    const double s = a < 1e-4 ? (1.0 + a * a * (1.0 / 6.0)) * exp(-p.M) : -p.num() / (2.0 * a);
    return s / (kT * p.den);
}

// ---------------------------------------------------------------- k + q
static __global__ __launch_bounds__(256) void k_chi_kq(const double* __restrict__ k, const double* __restrict__ q, const int64_t nk, const int dk,
                                                double* __restrict__ kq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nk * dk) return;
    kq[i] = k[i] + q[i % dk];
}
