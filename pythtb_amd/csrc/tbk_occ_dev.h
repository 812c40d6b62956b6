// tbk_occ_dev.h -- the two device-resident stages of tbk_occ.hip (DESIGN.md sections 27 and 33), shared by its own entry points and
// the mean-field driver (tbk_mf.hip).  Both work on device-resident inputs, leave their results on the device and neither copy nor
// synchronise.
#pragma once
#include "tbk_occ.h"
#include "tbk_lat_dev.h"

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

// tbk_occ.hip: the thermal sums N, E, S of nmu Fermi levels over the resident levels, part[j][3][G] (the driver's final energies)
__global__ __launch_bounds__(256) void k_occ_scan(const double* __restrict__ ev, const int64_t nlev, const int G, const double* __restrict__ mu,
                                                  const int nmu, const double kT, double* __restrict__ part);
