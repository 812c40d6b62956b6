// tbk_lat_dev.h -- the lattice sum of weighted projectors over a k mesh, device side:
//   X_ij(R[, w]) = sum_k e^{-2 pi i k.(R + tau_j - tau_i)} sum_n c_n(k[, w]) u_n[i] conj(u_n[j])
// the density matrix (tbk_occ.hip: c_n a real Fermi weight) and the lattice Green's function (tbk_gf.hip: c_n = 1 / (w + i eta - E_n)
// over a block of frequencies).  The two kernels and their launch are templates over a weight policy Wt and are instantiated in the
// unit that launches them.  Wt gives
//   WB, RB      frequencies and lattice vectors per workgroup (the accumulators of a lane: WB x RB per entry)
//   GROUP_X     the grid is (blocks of frequencies and lattice vectors [x tiles], k-groups); true: the k-groups run along x.  The
//               device hands consecutive workgroups to its eight XCDs in turn, so with the groups along x (and a multiple of 8 of them)
//               the blocks of one k-group meet in one L2 and its eigenvectors are fetched once; along y the grid takes 2^31 - 1 blocks
//   NSEL        0: every state in order; else the most selected states (Wt then has sel, na, all: the selection on the device, its
//               length, and whether it is every state in order)
//   W           the staged weight: double or cd
//   freq(w)     frequency w (0.0 where there is none), weight(om, x): c_n from the level's value x = lev[n][ik] at frequency om
//   empty(c)    a state whose first weight c adds nothing: it is skipped, and -- the weights falling with the level -- ends a point of
//               the tiled form where it leads a strip
//   add<FULL>(pij, a, b, c, nwl)   pij[w] += c[w] a conj(b) for the block's nwl frequencies (FULL: nwl = WB, no test)
//   kLabel      the ProfScope labels of the lds form, the tiled form and the group sum
// The lattice and orbital phases are formed from exact integers.  A frequency or lattice vector beyond the last of a workgroup's block
// is skipped by branches that are uniform over the workgroup: every entry goes through the same operations whatever stands beside it.
#pragma once
#include "tbk_lat.h"

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

// Up to 32 states.  Workgroup (block of WB frequencies and RB lattice vectors, k-group g): batches of P points.  A batch's weights, orbital phases and lattice phases are staged first, then the kept components of its eigenvectors as
// W[p][b][a] = u_b[sel a] e^{2 pi i k.tau_{sel a}} (every state in order: through kubo_lds_load; a selection: gathered).  The lanes
// take entries (i, j) and shares of the batch's points by lat_lane (tbk_lat.h); the shares are added in index order through LDS at the
// end.  Every lane of a wavefront reads the same state b at the same time, W_b[j] at consecutive addresses, W_b[i] and the weights as
// broadcasts: no bank conflict at 16 or 32 states (the 16-way conflict of k_chi_pairs comes from lanes on different rows).  Writes
// part[g][w][R][i][j].
template <class Wt, int ES>
__global__ __launch_bounds__(256) void k_lat_lds(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                 const double* __restrict__ lev, const int64_t nk, const int64_t first, const OccMesh M,
                                                 const int P, const int G, const Wt wt, const int nw, const int32_t* __restrict__ R,
                                                 const int nr, cd* __restrict__ part) {
    constexpr int WB = Wt::WB, RB = Wt::RB;
    constexpr bool SEL = Wt::NSEL > 0;
    typedef typename Wt::W W;
    __shared__ cd U[OCC_LDS_CD];
    __shared__ W gs[OCC_LDS_PN * WB];
    __shared__ cd eph[OCC_LDS_PN];
    __shared__ cd phs[64 * RB];
    __shared__ int ssel[SEL ? Wt::NSEL : 1];
    const int n = mv.nsta, t = threadIdx.x;
    int na = n;
    bool all = true;
    if constexpr (SEL) {
        na = wt.na, all = wt.all;
        if (t < na) ssel[t] = wt.sel[t];
    }
    const int nab = na * na, ns = n * na;
    const int nrb = (nr + RB - 1) / RB;
    const int bid = Wt::GROUP_X ? blockIdx.y : blockIdx.x, g = Wt::GROUP_X ? blockIdx.x : blockIdx.y;
    const int wb = bid / nrb, w0 = wb * WB, r0 = (bid - wb * nrb) * RB;
    const int nwl = WB == 1 ? 1 : min(WB, nw - w0), nrl = min(RB, nr - r0);   // the block's own frequencies and lattice vectors
    const int64_t p0 = (int64_t)g * nk / G, p1 = (int64_t)(g + 1) * nk / G;
    const LatLane ln = lat_lane(ES, nab, t);
    double om[WB];
#pragma unroll
    for (int w = 0; w < WB; ++w) om[w] = wt.freq(min(w0 + w, nw - 1));
    cd acc[ES][WB][RB];
#pragma unroll
    for (int s = 0; s < ES; ++s)
#pragma unroll
        for (int w = 0; w < WB; ++w)
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[s][w][r] = cd{0.0, 0.0};
    if constexpr (SEL) __syncthreads();
    for (int64_t b0 = p0; b0 < p1; b0 += P) {
        const int np = (int)std::min<int64_t>(P, p1 - b0);
        for (int e = t; e < np * n; e += 256) {
            const int p = e / n, b = e - p * n;
            const double x = lev[(int64_t)b * nk + b0 + p];
#pragma unroll
            for (int w = 0; w < WB; ++w)
                if (w < nwl) gs[e * WB + w] = wt.weight(om[w], x);
        }
        for (int e = t; e < np * na; e += 256) {
            const int p = e / na, a = e - p * na;
            eph[e] = dm_orb_phase(mv, k, b0 + p, SEL ? ssel[a] : a);
        }
        for (int e = t; e < np * nrl; e += 256) {
            const int p = e / nrl, r = e - p * nrl;
            phs[p * RB + r] = dm_phase(M, first + b0 + p, R + (int64_t)(r0 + r) * M.dk);
        }
        __syncthreads();
        if (all) {
            kubo_lds_load(U, evec, nk, b0, np, n, ns, [&](const int e) {
                const int p = e / ns, r = e - p * ns, i = r % n;
                U[e] = cmul_x(U[e], eph[p * n + i]);
            });
        } else {
            for (int e = t; e < np * ns; e += 256) {
                const int p = e / ns, rr = e - p * ns, b = rr / na, a = rr - b * na;
                U[e] = cmul_x(evec[((int64_t)b * nk + b0 + p) * n + ssel[a]], eph[p * na + a]);
            }
        }
        __syncthreads();
        if (ln.live) {
#pragma unroll
            for (int s = 0; s < ES; ++s) {
                const int el = ln.el0 + 256 * s;
                if (el >= nab) continue;
                int i, j;
                lat_entry(el, na, i, j);
                for (int p = ln.q; p < np; p += ln.Q) {
                    const cd* Wp = U + p * ns;
                    const W* gp = gs + p * n * WB;
                    cd pij[WB];
#pragma unroll
                    for (int w = 0; w < WB; ++w) pij[w] = cd{0.0, 0.0};
                    if (nwl == WB) {                               // (a full block: no test in the loop; the same operations)
                        for (int b = 0; b < n; ++b) {
                            if (Wt::empty(gp[b * WB])) continue;
                            Wt::template add<true>(pij, Wp[b * na + i], Wp[b * na + j], gp + b * WB, nwl);
                        }
                    } else {
                        for (int b = 0; b < n; ++b) {
                            if (Wt::empty(gp[b * WB])) continue;
                            Wt::template add<false>(pij, Wp[b * na + i], Wp[b * na + j], gp + b * WB, nwl);
                        }
                    }
#pragma unroll
                    for (int w = 0; w < WB; ++w)
#pragma unroll
                        for (int r = 0; r < RB; ++r)
                            if (w < nwl && r < nrl) cfma_x(acc[s][w][r], pij[w], phs[p * RB + r]);
                }
            }
        }
        __syncthreads();                                           // (the batch is consumed)
    }
    if (ES == 1 && ln.Q > 1) {                                     // the shares of the points, one (frequency, R) after the other
        cd* buf = U;                                               // 256 <= OCC_LDS_CD
#pragma unroll
        for (int w = 0; w < WB; ++w)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (w >= nwl || r >= nrl) continue;                 // (uniform over the workgroup)
                buf[t] = acc[0][w][r];
                __syncthreads();
                if (t < nab) {
                    cd s = buf[t];
                    for (int qq = 1; qq < ln.Q; ++qq) s = cadd(s, buf[qq * nab + t]);
                    part[(((int64_t)g * nw + w0 + w) * nr + r0 + r) * nab + t] = s;
                }
                __syncthreads();
            }
        return;
    }
#pragma unroll
    for (int s = 0; s < ES; ++s) {
        const int el = ln.el0 + 256 * s;
        if (!ln.live || el >= nab) continue;
#pragma unroll
        for (int w = 0; w < WB; ++w)
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (w < nwl && r < nrl) part[(((int64_t)g * nw + w0 + w) * nr + r0 + r) * nab + el] = acc[s][w][r];
    }
}

// 33 .. 2048 states.  Workgroup (16 x 16 tile (ti, tj) of the kept block of P(k[, w]) x block of WB frequencies and RB lattice vectors,
// k-group g): lane (ty, tx) owns the entry (16 ti + ty, 16 tj + tx).  Per point the states go through LDS in
// strips of 16 (their kept components of the tile's rows and of its columns, both read along the components) with the strip's
// weights; the orbital phases are applied to the finished P_ij.
template <class Wt>
__global__ __launch_bounds__(256) void k_lat_tile(const ModelView mv, const double* __restrict__ k, const cd* __restrict__ evec,
                                                  const double* __restrict__ lev, const int64_t nk, const int64_t first, const OccMesh M,
                                                  const int T, const int G, const Wt wt, const int nw, const int32_t* __restrict__ R,
                                                  const int nr, cd* __restrict__ part) {
    constexpr int WB = Wt::WB, RB = Wt::RB;
    constexpr bool SEL = Wt::NSEL > 0;
    typedef typename Wt::W W;
    __shared__ cd As[16][16], Bs[16][16], eo[32], phs[RB];
    __shared__ W gs[16][WB];
    __shared__ int so[SEL ? 32 : 1];
    const int n = mv.nsta, t = threadIdx.x, tx = t & 15, ty = t >> 4;
    int na = n;
    if constexpr (SEL) na = wt.na;
    const int bid = Wt::GROUP_X ? blockIdx.y : blockIdx.x, g = Wt::GROUP_X ? blockIdx.x : blockIdx.y;
    const int tiles = T * T, blk = bid / tiles, tile = bid - blk * tiles;
    const int ti = tile / T, tj = tile - ti * T;
    const int nrb = (nr + RB - 1) / RB;
    const int wb = blk / nrb, w0 = wb * WB, r0 = (blk - wb * nrb) * RB;
    const int nwl = WB == 1 ? 1 : min(WB, nw - w0), nrl = min(RB, nr - r0);   // the block's own frequencies and lattice vectors
    const int i = ti * 16 + ty, j = tj * 16 + tx;
    const int64_t p0 = (int64_t)g * nk / G, p1 = (int64_t)(g + 1) * nk / G;
    // the state of row x (x < 16) or column x - 16 of the tile; -1 beyond the kept block
    auto state = [&](const int x) {
        if constexpr (SEL) {
            return so[x];
        } else {
            const int pos = x < 16 ? ti * 16 + x : tj * 16 + x - 16;
            return pos < n ? pos : -1;
        }
    };
    if constexpr (SEL) {
        if (t < 32) {
            const int pos = t < 16 ? ti * 16 + t : tj * 16 + t - 16;
            so[t] = pos < na ? wt.sel[pos] : -1;
        }
    }
    const double omt = wt.freq(min(w0 + (t & (WB - 1)), nw - 1));   // (the frequency this lane stages the weights of)
    cd acc[WB][RB];
#pragma unroll
    for (int w = 0; w < WB; ++w)
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[w][r] = cd{0.0, 0.0};
    if constexpr (SEL) __syncthreads();
    for (int64_t ik = p0; ik < p1; ++ik) {
        if (t < 32) {
            const int o = state(t);
            eo[t] = o >= 0 ? dm_orb_phase(mv, k, ik, o) : cd{0.0, 0.0};
        } else if (t < 32 + nrl) {
            phs[t - 32] = dm_phase(M, first + ik, R + (int64_t)(r0 + t - 32) * M.dk);
        }
        cd pij[WB];
#pragma unroll
        for (int w = 0; w < WB; ++w) pij[w] = cd{0.0, 0.0};
        for (int b0 = 0; b0 < n; b0 += 16) {
            __syncthreads();                                       // (the previous strip is consumed; eo and phs are staged)
            if (t < 16 * WB) {
                const int bb = t / WB;
                gs[bb][t & (WB - 1)] = b0 + bb < n ? wt.weight(omt, lev[(int64_t)(b0 + bb) * nk + ik]) : W{};
            }
            const int b = b0 + ty;
            const cd* u = evec + ((int64_t)(b < n ? b : 0) * nk + ik) * n;
            const int sa = state(tx), sb = state(16 + tx);
            As[ty][tx] = (b < n && sa >= 0) ? u[sa] : cd{0.0, 0.0};
            Bs[ty][tx] = (b < n && sb >= 0) ? u[sb] : cd{0.0, 0.0};
            __syncthreads();
            if (Wt::empty(gs[0][0])) break;                        // (uniform: every later state adds nothing either)
            if (nwl == WB) {                                       // (a full block: no test in the loop; the same operations)
#pragma unroll
                for (int bb = 0; bb < 16; ++bb) {
                    if (Wt::empty(gs[bb][0])) continue;
                    Wt::template add<true>(pij, As[bb][ty], Bs[bb][tx], gs[bb], nwl);
                }
            } else {
#pragma unroll
                for (int bb = 0; bb < 16; ++bb) {
                    if (Wt::empty(gs[bb][0])) continue;
                    Wt::template add<false>(pij, As[bb][ty], Bs[bb][tx], gs[bb], nwl);
                }
            }
        }
#pragma unroll
        for (int w = 0; w < WB; ++w) {
            if (w >= nwl) continue;
            const cd pw = cmul_x(cmul_x(pij[w], eo[ty]), cconj(eo[16 + tx]));
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r < nrl) cfma_x(acc[w][r], pw, phs[r]);
        }
        __syncthreads();                                           // (eo and phs are read)
    }
    if (i < na && j < na)
#pragma unroll
        for (int w = 0; w < WB; ++w)
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (w < nwl && r < nrl) part[(((int64_t)g * nw + w0 + w) * nr + r0 + r) * na * na + (int64_t)i * na + j] = acc[w][r];
}

// ---------------------------------------------------------------- host side
// a chunk [first, first + cnt) of the mesh on the device: its k points, eigenvectors vc[n][cnt][n] and the levels' values lev[n][cnt]
// the weights are formed from
struct LatChunk {
    ModelView mv;
    const double* kp;
    const cd* vc;
    const double* lev;
    int64_t cnt, first;
    OccMesh M;
};
// One launch tile of a chunk -- nw frequencies (those of wt) times the nr lattice vectors at Rp, of nR in all: the partials of the
// plan's k-groups into part[G][nw][nr][na^2], then acc (+)= their sum in index order.  acc points at the tile's first entry in
// acc[..][nR][na^2]: the rows of a tile of nr < nR lattice vectors are runs of acc, one per frequency.
template <class Wt>
static int lat_launch(tbk_ctx* ctx, const LatPart& pl, const LatChunk& c, const Wt& wt, int na, int nw, const int32_t* Rp, int nr, int nR,
                      cd* part, cd* acc, int accumulate) {
    const int64_t blocks = (int64_t)((nw + Wt::WB - 1) / Wt::WB) * ((nr + Wt::RB - 1) / Wt::RB);
    auto grid = [&](const int64_t nb) { return Wt::GROUP_X ? dim3((unsigned)pl.G, (unsigned)nb) : dim3((unsigned)nb, (unsigned)pl.G); };
    if (pl.lds) {
        ProfScope ps(ctx, Wt::kLabel[0]);
        const auto kern = pl.ES == 1 ? k_lat_lds<Wt, 1> : (pl.ES == 2 ? k_lat_lds<Wt, 2> : k_lat_lds<Wt, 4>);
        hipLaunchKernelGGL(kern, grid(blocks), dim3(256), 0, ctx->stream, c.mv, c.kp, c.vc, c.lev, c.cnt, c.first,
                           c.M, pl.P, pl.G, wt, nw, Rp, nr, part);
        TBK_HIP(hipGetLastError());
    } else {
        ProfScope ps(ctx, Wt::kLabel[1]);
        hipLaunchKernelGGL(k_lat_tile<Wt>, grid(blocks * pl.T * pl.T), dim3(256), 0, ctx->stream, c.mv, c.kp, c.vc,
                           c.lev, c.cnt, c.first, c.M, pl.T, pl.G, wt, nw, Rp, nr, part);
        TBK_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, Wt::kLabel[2]);
    const int64_t nrow = (int64_t)nr * na * na * 2;
    const int64_t run = nr == nR ? nw * nrow : nrow;               // (every R: the tile is one run of acc)
    hipLaunchKernelGGL(k_group_rows_lanes, dim3(nblk(nw * nrow)), dim3(256), 0, ctx->stream, (const double*)part, pl.G, nw * nrow, run,
                       (int64_t)nR * na * na * 2, accumulate, (double*)acc);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
