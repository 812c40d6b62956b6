// tbk_occ_dev.h -- the two device-resident stages of tbk_occ.hip (DESIGN.md sections 27 and 33), shared by its own entry points and
// the mean-field driver (tbk_mf.hip), and the selected-entry stage of tbk_pairs_dm.hip (section 36) beside them.  All work on
// device-resident inputs, leave their results on the device and neither copy nor synchronise.
#pragma once
#include "tbk_occ.h"
#include "tbk_lat_dev.h"

// f and, where wanted, the entropy term s = -f ln f - (1 - f) ln(1 - f) of x = (E - mu) / kT (tbk_kubo.h's fermi_terms)
__device__ __forceinline__ double occ_fermi(const double e, const double mu, const double kT, double* s) {
    if (kT == 0.0) {
        if (s) *s = 0.0;
        return e <= mu ? 1.0 : 0.0;
    }
    const FermiTerms ft = fermi_terms((e - mu) / kT);
    if (s) *s = ft.entropy();
    return ft.f();
}

// the buffers of the Fermi selection, all on the device: part[2 nfill G] doubles; mu, lo, hi, target [nfill]; edges [2 nfill]
struct OccFermiBufs {
    double* part;
    double* mu;
    uint64_t* lo;
    uint64_t* hi;
    const double* target;
    double* edges;
};
// The bisection on the resident levels e_dev[nlev] (G = occ_scan_groups(nlev)): arms the brackets on the device, runs the kOccSteps
// passes and ends with the Fermi level of every filling in B.mu -- kT > 0: the first double whose occupation reaches the target (B.hi
// holds its key); kT = 0: the midpoint of B.edges = (e_{c-1}, e_c), formed on the device.
int occ_fermi_stage(tbk_ctx* ctx, const double* e_dev, int64_t nlev, int G, int nfill, double kT, const OccFermiBufs& B);

// The density-matrix accumulation of ONE chunk [first, first + cnt) given its eigenpairs (ec[n][cnt], vc[n][cnt][n]) and k points kp:
// weights at the Fermi level *mu_dev (device memory) where mu_dev is not null, else at mu; then the partials of the plan's k-groups
// and acc[R][i][j] (+)= their sum in index order (accumulate = 0: the first chunk of a pass stores).  fw: cnt * n doubles.
int occ_dm_stage(tbk_ctx* ctx, const ModelView& mv, const OccDmPlan& pl, const OccMesh& M, int64_t first, int64_t cnt, const double* kp,
                 const double* ec, const cd* vc, const double* mu_dev, double mu, double kT, double* fw, const int32_t* R_dev, int nR,
                 cd* part, cd* acc, int accumulate);

// tbk_pairs_dm.hip: selected entries of the same accumulation for ONE chunk, no whole matrix formed --
// acc[p] (+)= sum over the chunk's points of [sum_n f_n v_n[i_p] conj(v_n[j_p])] e^{-2 pi i k.(R_p + tau_j - tau_i)} for the nt triples
// (ij[nt][2], R[nt][dim_k], device memory): the partials of the plan's k-groups into part[G][min(TL, nt)], launch range after launch
// range of TL triples, then their sum in index order.  Weights at *mu_dev where mu_dev is not null, else at mu.
struct PdmPart;
int occ_pairs_stage(tbk_ctx* ctx, const ModelView& mv, const PdmPart& pl, const OccMesh& M, int64_t first, int64_t cnt, const double* kp,
                    const double* ec, const cd* vc, const double* mu_dev, double mu, double kT, const int32_t* ij_dev, const int32_t* R_dev,
                    int64_t nt, cd* part, cd* acc, int accumulate);

// tbk_occ.hip: the thermal sums N, E, S of nmu Fermi levels over the resident levels, part[j][3][G] (the driver's final energies)
__global__ __launch_bounds__(256) void k_occ_scan(const double* __restrict__ ev, const int64_t nlev, const int G, const double* __restrict__ mu,
                                                  const int nmu, const double kT, double* __restrict__ part);

// tbk_pairs_dm.hip: acc[row] (+)= sum_g part[g][row], a wavefront per row (a double), the groups in a fixed order (the exciton
// operator of tbk_bse.hip reduces its group partials with it)
__global__ __launch_bounds__(256) void k_pairs_rows(const double* __restrict__ part, const int G, const int64_t nrows, const int accumulate,
                                                    double* __restrict__ acc);
