// tbk_mesh_phase.h -- the lattice and orbital phases of the real-space sums over a k mesh, shared by the density matrix (tbk_occ.hip,
// DESIGN.md section 27) and the lattice Green's function (tbk_gf.hip, section 30).  Device only.
#pragma once
#include "tbk_kubo.h"

struct OccMesh {
    int N[3];   // the mesh, 1 beyond dim_k
    int dk;
};
// e^{-2 pi i k.R} at point idx of the mesh: per axis the exact integer m = i_a R_a mod N_a, then sincospi(-2 m / N_a)
__device__ __forceinline__ cd dm_phase(const OccMesh& M, const int64_t idx, const int32_t* __restrict__ R) {
    int ii[3];
    mesh_point(M.N, idx, ii);
    cd ph{1.0, 0.0};
    for (int d = 0; d < M.dk; ++d) {
        int64_t mm = ((int64_t)ii[d] * (int64_t)R[d]) % M.N[d];
        if (mm < 0) mm += M.N[d];
        if (mm == 0) continue;
        double sn, cs;
        sincospi(-2.0 * ((double)mm / (double)M.N[d]), &sn, &cs);
        ph = cmul_x(ph, cd{cs, sn});
    }
    return ph;
}
__device__ __forceinline__ cd dm_orb_phase(const ModelView& mv, const double* __restrict__ k, const int64_t ik, const int o) {
    double kk[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < mv.dim_k; ++d) kk[d] = k[ik * mv.dim_k + d];
    return expi2pi(kdot(kk, mv.orb[o]));
}
