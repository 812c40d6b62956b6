// tbk_pairs_dm.hip -- selected entries of the real-space density matrix on uniform k meshes.
//
// For a list of triples (i, j, R) -- state indices and a lattice vector -- with the eigenpairs, the occupation rule and the phase
// convention of tbk_density_matrix_mesh (tbk_occ.hip),
//   D_ij(R) = (1 / N_k) sum_k [sum_n f_n u_n[i] conj(u_n[j])] e^{-2 pi i k.(R + tau_j - tau_i)} = <c+_{j,R} c_{i,0}>
// without forming any matrix: what a self-consistency loop needs is the few entries its interaction couples, not nR n^2 of them.
//
// occ_pairs_stage, per chunk of the mesh (tbk_kubo.h's chunks, eigenvectors on the device):
//   k_pairs_dm   workgroup (k-group g, tile of PDM_TILE = 64 triples): lane l of each of the four wavefronts owns triple l of the tile.
//                The group's eigenvectors go through LDS stage by stage (tbk_pairs_dm.h: every band of P points up to 45 states, NB
//                bands of one point beyond), copied as whole runs of 16-byte elements, with the stage's weights f[band][point] beside
//                them.  Up to 45 states wavefront w takes the points w, w + 4, ... of a stage and every band in order; beyond, the bands
//                b = w (mod 4) of the point.  A band of weight 0 is skipped -- the weight is the same in every lane of the wavefront.  A
//                finished P_ij(k) is multiplied by the phase, formed per (lane, point) from the exact integer (i_a R_a mod N_a) and
//                k.(tau_i - tau_j), and added to the lane's accumulator, which is carried over all the group's points.  At the end the four
//                wavefronts' accumulators are added in index order through LDS: part[g][triple].
//   k_pairs_rows   acc[triple] (+)= sum_g part[g][triple], a wavefront per real number, the groups in a fixed order, chunk after chunk
//                in stream order
// No floating-point atomics, and nothing in the partition or in a lane's operations depends on the list: two calls give the same bits, and
// a triple gives the same bits alone and inside any list, at any place in it.
#include <math.h>
#include "tbk_pairs_dm.h"
#include "tbk_occ_dev.h"

// e^{-2 pi i k.R} at point idx of the mesh, R in registers: the arithmetic of dm_phase (tbk_lat_dev.h), axis by axis
__device__ __forceinline__ cd pdm_axis(const cd ph, const int i, const int R, const int N) {
    int64_t mm = ((int64_t)i * (int64_t)R) % N;
    if (mm < 0) mm += N;
    if (mm == 0) return ph;
    double sn, cs;
    sincospi(-2.0 * ((double)mm / (double)N), &sn, &cs);
    return cmul_x(ph, cd{cs, sn});
}

// orb: the model's orbital table (ModelView::orb; the whole view would cost the kernel 40 scalar registers it has no use for)
__global__ __launch_bounds__(256) void k_pairs_dm(const double4* __restrict__ orb, const int n, const int dk, const double* __restrict__ k,
                                                  const double2* __restrict__ evec, const double* __restrict__ lev, const int64_t nk,
                                                  const int64_t first, const OccMesh M,
                                                  const int G, const double* __restrict__ mu_dev, const double mu_val, const double kT,
                                                  const int32_t* __restrict__ ij, const int32_t* __restrict__ R, const int64_t ntl,
                                                  cd* __restrict__ part) {
    __shared__ double2 U[PDM_LDS_CD];
    __shared__ double gs[PDM_ROWS];
    __shared__ cd red[4][PDM_TILE];
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const PdmStage st = pdm_stage(n);
    const int g = blockIdx.x;
    const int64_t tr = (int64_t)blockIdx.y * PDM_TILE + l;
    const bool live = tr < ntl;
    const int64_t tt = live ? tr : 0;                              // (a lane beyond the list reads triple 0 and stores nothing)
    const int i = ij[2 * tt], j = ij[2 * tt + 1];
    const int r0 = R[tt * dk], r1 = dk > 1 ? R[tt * dk + 1] : 0, r2 = dk > 2 ? R[tt * dk + 2] : 0;
    const double4 ti = orb[i], tj = orb[j];
    const double4 dtau{ti.x - tj.x, ti.y - tj.y, ti.z - tj.z, 0.0};
    const double mu = mu_dev ? mu_dev[0] : mu_val;
    const bool pts = st.P > 1;                                     // the wavefronts share the points of a stage, else the bands
    const int64_t p0 = (int64_t)g * nk / G, p1 = (int64_t)(g + 1) * nk / G;
    cd acc{0.0, 0.0}, pij{0.0, 0.0};
    for (int64_t b0 = p0; b0 < p1; b0 += st.P) {
        const int np = (int)min((int64_t)st.P, p1 - b0), run = np * n;
        for (int bb0 = 0; bb0 < n; bb0 += st.NB) {
            const int nb = min(st.NB, n - bb0);
            __syncthreads();                                       // (the previous stage is consumed)
            for (int e = t; e < nb * np; e += 256) {
                const int b = e / np, p = e - b * np;
                gs[e] = occ_fermi(lev[(int64_t)(bb0 + b) * nk + b0 + p], mu, kT, nullptr);
            }
#pragma unroll 4
            for (int e = t; e < nb * run; e += 256) {               // band b of the stage: one run of np n elements
                const int b = e / run, r = e - b * run;
                U[e] = evec[((int64_t)(bb0 + b) * nk + b0) * n + r];
            }
            __syncthreads();
            if (!live) continue;
            const int bs = pts ? 0 : ((w - bb0) & 3), bstep = pts ? 1 : 4;
            for (int p = pts ? w : 0; p < np; p += pts ? 4 : 1) {
                if (bb0 == 0) pij = cd{0.0, 0.0};
                for (int b = bs; b < nb; b += bstep) {
                    const double f = gs[b * np + p];
                    if (f == 0.0) continue;                        // (uniform over the wavefront)
                    const double2* u = U + (b * np + p) * n;
                    const double2 a = u[i], c = u[j];
                    cfmac_x(pij, cd{a.x * f, a.y * f}, cd{c.x, c.y});   // += f u[i] conj(u[j])
                }
                if (bb0 + nb < n) continue;                        // (more bands of this point to come)
                const int64_t ik = b0 + p;
                int ii[3];
                mesh_point(M.N, first + ik, ii);
                double kk[4] = {0.0, 0.0, 0.0, 0.0};
                kk[0] = k[ik * dk];
                if (dk > 1) kk[1] = k[ik * dk + 1];
                if (dk > 2) kk[2] = k[ik * dk + 2];
                cd ph = expi2pi(kdot(kk, dtau));                   // e^{-2 pi i k.(tau_j - tau_i)}
                ph = pdm_axis(ph, ii[0], r0, M.N[0]);
                ph = pdm_axis(ph, ii[1], r1, M.N[1]);
                ph = pdm_axis(ph, ii[2], r2, M.N[2]);
                cfma_x(acc, pij, ph);
            }
        }
    }
    red[w][l] = acc;
    __syncthreads();
    if (w == 0 && live) {
        cd s = red[0][l];
        s = cadd(s, red[1][l]);
        s = cadd(s, red[2][l]);
        s = cadd(s, red[3][l]);
        part[(int64_t)g * ntl + tr] = s;
    }
}

// acc[row] (+)= sum_g part[g][row], one WAVEFRONT per row (a double: the real or the imaginary part of a triple): lane l adds the groups
// l, l + 64, ... in order, a shuffle tree adds the lanes.  The loop's few dozen rows of up to 512 groups would leave k_group_rows_lanes
// (a lane per row, the groups one after the other) waiting on 512 loads in a chain; the shape is the same for every list.
__global__ __launch_bounds__(256) void k_pairs_rows(const double* __restrict__ part, const int G, const int64_t nrows, const int accumulate,
                                                    double* __restrict__ acc) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;                                      // (a whole wavefront)
    double s = 0.0;
    for (int g = threadIdx.x & 63; g < G; g += 64) s += part[(int64_t)g * nrows + row];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) acc[row] = accumulate ? acc[row] + s : s;
}

// ---------------------------------------------------------------- host side: the stage (tbk_occ_dev.h)
int occ_pairs_stage(tbk_ctx* ctx, const ModelView& mv, const PdmPart& pl, const OccMesh& M, int64_t first, int64_t cnt, const double* kp,
                    const double* ec, const cd* vc, const double* mu_dev, double mu, double kT, const int32_t* ij_dev, const int32_t* R_dev,
                    int64_t nt, cd* part, cd* acc, int accumulate) {
    const int dk = mv.dim_k;
    for (int64_t t0 = 0; t0 < nt; t0 += pl.TL) {
        const int64_t ntl = std::min<int64_t>(pl.TL, nt - t0);
        {
            ProfScope ps(ctx, "pairs_dm");
            hipLaunchKernelGGL(k_pairs_dm, dim3((unsigned)pl.G, (unsigned)((ntl + PDM_TILE - 1) / PDM_TILE)), dim3(256), 0, ctx->stream, mv.orb,
                               mv.nsta, dk, kp, (const double2*)vc, ec, cnt, first, M, pl.G, mu_dev, mu, kT, ij_dev + 2 * t0, R_dev + t0 * dk,
                               ntl, part);
            TBK_HIP(hipGetLastError());
        }
        ProfScope ps(ctx, "pairs_rows");
        hipLaunchKernelGGL(k_pairs_rows, dim3((unsigned)((2 * ntl + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)part, pl.G, 2 * ntl,
                           accumulate, (double*)(acc + t0));
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

// ---------------------------------------------------------------- host side
extern "C" int tbk_density_matrix_pairs_mesh(tbk_model* m, const int32_t* mesh, double mu, double kT, int64_t nt, const int32_t* ij,
                                             const int32_t* R, double* out) {
    const char* fn = "tbk_density_matrix_pairs_mesh";
    TBK_REQUIRE(m && mesh && out, TBK_EINVAL, "%s: null argument", fn);
    const int dk = m->dim_k, n = m->nsta;
    int64_t npts;
    int rc = pdm_check(fn, dk, n, mesh, mu, kT, nt, ij, R, npts);
    if (rc) return rc;
    const PdmPlan pl = pdm_plan(n, dk, npts, nt, true);
    tbk_ctx* ctx = m->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    void* base = nullptr;
    rc = tbk_ctx_scratch(ctx, pl.total, &base);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)base;
    int32_t* ij_dev = (int32_t*)(b + pl.off_ij);
    int32_t* R_dev = (int32_t*)(b + pl.off_R);
    cd* acc = (cd*)(b + pl.off_acc);
    cd* part = (cd*)(b + pl.off_part);
    KuboChunks cw = pl.cw;
    cw.base = b + pl.off_chunks;
    TBK_HIP(hipMemcpyAsync(ij_dev, ij, (size_t)nt * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TBK_HIP(hipMemcpyAsync(R_dev, R, (size_t)nt * dk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    OccMesh M{{1, 1, 1}, dk};
    for (int d = 0; d < dk; ++d) M.N[d] = mesh[d];
    rc = kubo_for_chunks(m, cw, nullptr, mesh, npts, [&](int64_t first, int64_t cnt, const double* kp, const double* ec, const cd* vc) -> int {
        return occ_pairs_stage(ctx, m->view, pl, M, first, cnt, kp, ec, vc, nullptr, mu, kT, ij_dev, R_dev, nt, part, acc, first > 0 ? 1 : 0);
    });
    if (rc) return rc;
    TBK_HIP(hipMemcpyAsync(out, acc, (size_t)nt * sizeof(cd), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    const double nk = (double)npts;
    for (int64_t i = 0; i < 2 * nt; ++i) out[i] /= nk;
    return TBK_OK;
}
