// tbk_kpm.hip -- kernel polynomial method: Chebyshev moments of the sparse H(k).
//
// The dense path of this library stops at TBK_MAX_NSTA states because every quantity starts from a full diagonalisation.  Here
// the hopping table the model already holds is kept as what it is, a sparse matrix (CSR over states), and the DOS / LDOS come from
// mu_m = <v|T_m(H~)|v> / <v|v>, H~ = (H - b) / a, by the three-term recursion alpha_{m+1} = 2 H~ alpha_m - alpha_{m-1}: one sparse
// product per step, two moments per product (mu_2m = 2 <alpha_m|alpha_m> - mu_0, mu_2m+1 = 2 <alpha_m+1|alpha_m> - mu_1).
// No reference counterpart (PythTB 1.8 has no sparse operator); Weisse, Wellein, Alvermann, Fehske, Rev. Mod. Phys. 78, 275.
//
// Layouts.  CSR: row_ptr[n + 1] (int64), col[nnz] (int32, sorted within a row), amp[nnz], R[nnz] (int4) and the row of every entry;
// the value at k is amp exp(2 pi i k.(R + orb_col - orb_row)), the convention of _gen_ham (pythtb.py:874-925).
// Vectors: alpha[row][NV] c128, the vector index fastest, NV = 8: a matrix entry is read once per 8 vectors and the gathered row of
// alpha is one contiguous 128-byte segment.  A call with more vectors runs block after block; a short block is padded with zeros.
//
// Launches.  One plain launch per Chebyshev step on the context's stream, one host synchronisation at the end of the call; no grid
// barrier, no persistent kernel.  The dot products go through per-workgroup partial sums and a fixed-order reduce kernel (no
// floating-point atomics): the moments are bit-identical from run to run.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "tbk_kpm.h"

// ------------------------------------------------------------------ host assembly
namespace {
struct RawEntry {
    int32_t col;
    int32_t R[4];
    cd amp;
};
inline bool raw_less(const RawEntry& x, const RawEntry& y) {
    if (x.col != y.col) return x.col < y.col;
    for (int d = 0; d < 4; ++d)
        if (x.R[d] != y.R[d]) return x.R[d] < y.R[d];
    return false;
}
inline bool raw_same(const RawEntry& x, const RawEntry& y) {
    return x.col == y.col && x.R[0] == y.R[0] && x.R[1] == y.R[1] && x.R[2] == y.R[2] && x.R[3] == y.R[3];
}
struct SparseHost {
    int n = 0;
    int64_t nnz = 0;
    std::vector<int64_t> row_ptr;
    std::vector<RawEntry> ent;      // the first nnz are the merged entries, rows in order, (col, R) sorted within a row
    std::vector<double> orb4;
    double gmin = 0.0, gmax = 0.0;
    double vbound[4] = {0.0, 0.0, 0.0, 0.0};   // largest row sum of |dH/dk_d|, d < dim_k
};
}  // namespace

// The CSR form of the tables tbk_model_upload takes: the on-site blocks, every hop and its Hermitian conjugate, spin blocks expanded
// to scalar entries, equal (row, col, R) summed, exact zeros dropped.  Bucketed by row (two passes over the tables), then sorted and
// merged row by row: linear in the table size, no node-based container (a flake of 10^6 orbitals has 10^7 entries).
static int sparse_flatten(int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                          const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp, SparseHost& S) {
    TBK_REQUIRE(dim_k >= 0 && dim_k <= TBK_MAX_DIM, TBK_EINVAL, "tbk_sparse: dim_k=%d", dim_k);
    TBK_REQUIRE(nspin == 1 || nspin == 2, TBK_EINVAL, "tbk_sparse: nspin=%d", nspin);
    TBK_REQUIRE(norb >= 1 && (int64_t)norb * nspin <= (int64_t)0x7fffffff, TBK_EINVAL, "tbk_sparse: norb=%d", norb);
    TBK_REQUIRE(nhop >= 0, TBK_EINVAL, "tbk_sparse: nhop=%lld", (long long)nhop);
    TBK_REQUIRE(onsite && (dim_k == 0 || orb), TBK_EINVAL, "tbk_sparse: null table");
    TBK_REQUIRE(nhop == 0 || (hop_i && hop_j && hop_amp && (dim_k == 0 || hop_R)), TBK_EINVAL, "tbk_sparse: null hopping table");
    const int ns = nspin, n = norb * nspin;
    for (int64_t h = 0; h < nhop; ++h)
        TBK_REQUIRE(hop_i[h] >= 0 && hop_i[h] < norb && hop_j[h] >= 0 && hop_j[h] < norb, TBK_EINVAL,
                    "tbk_sparse: hop %lld has orbital index out of range", (long long)h);
    S.n = n;
    std::vector<int64_t>& ptr = S.row_ptr;
    std::vector<int64_t> start;
    try {
        ptr.assign((size_t)n + 1, 0);
        for (int a = 0; a < n; ++a) ptr[a + 1] = ns;                      // the on-site block
        for (int64_t h = 0; h < nhop; ++h)
            for (int s = 0; s < ns; ++s) {
                ptr[(int64_t)hop_i[h] * ns + s + 1] += ns;                // ham[i,s,j,t] += amp E_R
                ptr[(int64_t)hop_j[h] * ns + s + 1] += ns;                // ham[j,t,i,s] += conj(amp) E_-R   (pythtb.py:919-924)
            }
        for (int a = 0; a < n; ++a) ptr[a + 1] += ptr[a];
        S.ent.resize((size_t)ptr[n]);
        start.assign(ptr.begin(), ptr.end() - 1);
    } catch (const std::bad_alloc&) {
        tbk_set_error("tbk_sparse: out of host memory");
        return TBK_ENOMEM;
    }
    std::vector<RawEntry>& ent = S.ent;
    std::vector<int64_t> fill(start);
    auto put = [&](int row, int col, const int* R, int sign, cd amp) {
        RawEntry& e = ent[(size_t)fill[row]++];
        e.col = col;
        for (int d = 0; d < 4; ++d) e.R[d] = d < dim_k ? sign * R[d] : 0;
        e.amp = amp;
    };
    const int zeroR[4] = {0, 0, 0, 0};
    for (int o = 0; o < norb; ++o)
        for (int s = 0; s < ns; ++s)
            for (int t = 0; t < ns; ++t) {   // the upper part of the Hermitian on-site block and its mirror, as tbk_model_upload reads it
                const double* p = onsite + 2 * (((int64_t)o * ns + std::min(s, t)) * ns + std::max(s, t));
                put(o * ns + s, o * ns + t, zeroR, 1, cd{p[0], s == t ? 0.0 : (s < t ? p[1] : -p[1])});
            }
    for (int64_t h = 0; h < nhop; ++h) {
        int R[4] = {0, 0, 0, 0};
        for (int d = 0; d < dim_k; ++d) R[d] = hop_R[h * dim_k + d];
        for (int s = 0; s < ns; ++s)
            for (int t = 0; t < ns; ++t) {
                const double* p = hop_amp + 2 * ((h * ns + s) * ns + t);
                const int a = hop_i[h] * ns + s, b = hop_j[h] * ns + t;
                put(a, b, R, 1, cd{p[0], p[1]});
                put(b, a, R, -1, cd{p[0], -p[1]});
            }
    }
    // sort and merge row by row, compacting in place (the write position never passes the row being read)
    int64_t w = 0;
    double gmin = INFINITY, gmax = -INFINITY;
    for (int a = 0; a < n; ++a) {
        const int64_t e0 = start[a], e1 = ptr[a + 1];
        std::stable_sort(ent.begin() + e0, ent.begin() + e1, raw_less);   // equal keys are summed in table order
        const int64_t w0 = w;
        double diag = 0.0, rad = 0.0, vrow[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t e = e0; e < e1;) {
            RawEntry m = ent[(size_t)e];
            int64_t f = e + 1;
            for (; f < e1 && raw_same(ent[(size_t)f], m); ++f) m.amp = cadd(m.amp, ent[(size_t)f].amp);
            e = f;
            if (m.amp.x == 0.0 && m.amp.y == 0.0) continue;
            const bool onsite_term = m.col == a && m.R[0] == 0 && m.R[1] == 0 && m.R[2] == 0 && m.R[3] == 0;
            if (onsite_term) {
                diag += m.amp.x;
                rad += fabs(m.amp.y);       // zero for a Hermitian table
            } else {
                rad += sqrt(cabs2(m.amp));
            }
            for (int d = 0; d < dim_k; ++d)   // |(dH/dk_d)_ab| = 2 pi |amp| |(R + orb_b - orb_a)_d| at every k
                vrow[d] += 2.0 * M_PI * sqrt(cabs2(m.amp)) *
                           fabs((double)m.R[d] + orb[(int64_t)(m.col / ns) * dim_k + d] - orb[(int64_t)(a / ns) * dim_k + d]);
            ent[(size_t)w++] = m;
        }
        ptr[a] = w0;
        gmin = std::min(gmin, diag - rad);
        gmax = std::max(gmax, diag + rad);
        for (int d = 0; d < dim_k; ++d) S.vbound[d] = std::max(S.vbound[d], vrow[d]);
    }
    ptr[n] = w;
    S.nnz = w;
    S.gmin = gmin;
    S.gmax = gmax;
    S.orb4.assign((size_t)n * 4, 0.0);
    for (int a = 0; a < n; ++a)
        for (int d = 0; d < dim_k; ++d) S.orb4[(size_t)a * 4 + d] = orb[(int64_t)(a / ns) * dim_k + d];
    return TBK_OK;
}

extern "C" int tbk_sparse_flatten_host(int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                                       const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                                       int64_t cap, int64_t* nnz, int64_t* row_ptr, int32_t* col, int32_t* ent_R, double* ent_amp,
                                       double* gershgorin) {
    TBK_REQUIRE(nnz, TBK_EINVAL, "tbk_sparse_flatten_host: null nnz");
    SparseHost S;
    int rc = sparse_flatten(dim_k, norb, nspin, orb, onsite, nhop, hop_i, hop_j, hop_R, hop_amp, S);
    if (rc) return rc;
    *nnz = S.nnz;
    if (gershgorin) {
        gershgorin[0] = S.gmin;
        gershgorin[1] = S.gmax;
    }
    if (cap >= S.nnz && row_ptr && col && ent_R && ent_amp) {
        for (int a = 0; a <= S.n; ++a) row_ptr[a] = S.row_ptr[a];
        for (int64_t e = 0; e < S.nnz; ++e) {
            const RawEntry& m = S.ent[(size_t)e];
            col[e] = m.col;
            for (int d = 0; d < 4; ++d) ent_R[e * 4 + d] = m.R[d];
            ent_amp[2 * e] = m.amp.x;
            ent_amp[2 * e + 1] = m.amp.y;
        }
    }
    return TBK_OK;
}

extern "C" int tbk_sparse_velocity_bounds_host(int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                                               const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                                               double* vbound) {
    TBK_REQUIRE(vbound, TBK_EINVAL, "tbk_sparse_velocity_bounds_host: null vbound");
    SparseHost S;
    int rc = sparse_flatten(dim_k, norb, nspin, orb, onsite, nhop, hop_i, hop_j, hop_R, hop_amp, S);
    if (rc) return rc;
    for (int d = 0; d < 4; ++d) vbound[d] = S.vbound[d];
    return TBK_OK;
}

extern "C" int tbk_sparse_upload(tbk_ctx* ctx, int dim_k, int norb, int nspin, const double* orb, const double* onsite,
                                 int64_t nhop, const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R,
                                 const double* hop_amp, tbk_sparse** out) {
    TBK_REQUIRE(ctx && out, TBK_EINVAL, "tbk_sparse_upload: null ctx/out");
    SparseHost S;
    {
        int rc = sparse_flatten(dim_k, norb, nspin, orb, onsite, nhop, hop_i, hop_j, hop_R, hop_amp, S);
        if (rc) return rc;
    }
    const size_t n = (size_t)S.n, nnz = (size_t)S.nnz;
    const size_t o_ptr = 0, o_col = o_ptr + up256((n + 1) * 8), o_row = o_col + up256(nnz * 4), o_amp = o_row + up256(nnz * 4),
                 o_R = o_amp + up256(nnz * 16), o_orb = o_R + up256(nnz * 16), total = o_orb + up256(n * 32);
    std::vector<unsigned char> host;
    try {
        host.assign(total, 0);
    } catch (const std::bad_alloc&) {
        tbk_set_error("tbk_sparse_upload: out of host memory");
        return TBK_ENOMEM;
    }
    memcpy(host.data() + o_ptr, S.row_ptr.data(), (n + 1) * 8);
    int32_t* hc = (int32_t*)(host.data() + o_col);
    int32_t* hr = (int32_t*)(host.data() + o_row);
    cd* ha = (cd*)(host.data() + o_amp);
    int32_t* hR = (int32_t*)(host.data() + o_R);
    for (size_t a = 0; a < n; ++a)
        for (int64_t e = S.row_ptr[a]; e < S.row_ptr[a + 1]; ++e) {
            const RawEntry& m = S.ent[(size_t)e];
            hc[e] = m.col;
            hr[e] = (int32_t)a;
            ha[e] = m.amp;
            for (int d = 0; d < 4; ++d) hR[e * 4 + d] = m.R[d];
        }
    memcpy(host.data() + o_orb, S.orb4.data(), n * 32);
    tbk_sparse* sp = new (std::nothrow) tbk_sparse();
    TBK_REQUIRE(sp, TBK_ENOMEM, "tbk_sparse_upload: out of host memory");
    sp->ctx = ctx;
    sp->dim_k = dim_k;
    sp->nsta = S.n;
    sp->nnz = S.nnz;
    sp->gmin = S.gmin;
    sp->gmax = S.gmax;
    for (int d = 0; d < 4; ++d) sp->vbound[d] = S.vbound[d];
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&sp->blob, total);
    if (e == hipSuccess) e = hipMemcpyAsync(sp->blob, host.data(), total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        if (sp->blob) hipFree(sp->blob);
        delete sp;
        tbk_set_error("tbk_sparse_upload: %zu bytes of tables: %s", total, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? TBK_ENOMEM : TBK_EHIP;
    }
    unsigned char* base = (unsigned char*)sp->blob;
    sp->row_ptr = (const int64_t*)(base + o_ptr);
    sp->col = (const int32_t*)(base + o_col);
    sp->row_of = (const int32_t*)(base + o_row);
    sp->amp = (const cd*)(base + o_amp);
    sp->R = (const int4*)(base + o_R);
    sp->orb = (const double4*)(base + o_orb);
    *out = sp;
    return TBK_OK;
}

extern "C" int tbk_sparse_free(tbk_sparse* sp) {
    if (!sp) return TBK_OK;
    hipSetDevice(sp->ctx->device);
    hipStreamSynchronize(sp->ctx->stream);
    if (sp->blob) hipFree(sp->blob);
    delete sp;
    return TBK_OK;
}

extern "C" int tbk_sparse_info(tbk_sparse* sp, int* dim_k, int* nsta, int64_t* nnz, double* gershgorin) {
    TBK_REQUIRE(sp, TBK_EINVAL, "tbk_sparse_info: null operator");
    if (dim_k) *dim_k = sp->dim_k;
    if (nsta) *nsta = sp->nsta;
    if (nnz) *nnz = sp->nnz;
    if (gershgorin) {
        gershgorin[0] = sp->gmin;
        gershgorin[1] = sp->gmax;
    }
    return TBK_OK;
}

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_kpm_randvec(const int nsta, const uint64_t seed, const int64_t first, const int64_t count,
                                                     cd* __restrict__ out) {
    const int64_t total = count * nsta;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
        out[e] = kpm_random_phase(seed, (uint64_t)(first + e / nsta), (uint64_t)(e % nsta));
}

// The doubling identities on dots[step] = (A_step[NV], B_step[NV]), A_j = <alpha_j|alpha_j>, B_j = Re <alpha_j|alpha_j-1>:
// mu_0 = 1, mu_1 = B_1 / A_0, mu_2j = (2 A_j - A_0) / A_0, mu_2j-1 = (2 B_j - B_1) / A_0  ->  mu[v][m], v < nv
template <int NV>
__global__ __launch_bounds__(256) void k_kpm_finish(const int nv, const int nmom, const double* __restrict__ dots,
                                                    double* __restrict__ mu) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nv * nmom) return;
    const int v = idx / nmom, m = idx % nmom;
    const double a0 = dots[v];
    double r;
    if (m == 0) {
        r = a0 / a0;
    } else if (m == 1) {
        r = dots[2 * NV + NV + v] / a0;
    } else if ((m & 1) == 0) {
        r = (2.0 * dots[(int64_t)(m / 2) * 2 * NV + v] - a0) / a0;
    } else {
        r = (2.0 * dots[(int64_t)((m + 1) / 2) * 2 * NV + NV + v] - dots[2 * NV + NV + v]) / a0;
    }
    mu[(int64_t)v * nmom + m] = r;
}

// ------------------------------------------------------------------ host entry points
int kpm_values_at(const tbk_sparse* sp, const double* k_dev, cd* val) {
    tbk_ctx* ctx = sp->ctx;
    ProfScope ps(ctx, "kpm_values");
    hipLaunchKernelGGL(k_kpm_values<false>, dim3(kpm_stream_grid(sp->nnz)), dim3(256), 0, ctx->stream, sp->nnz, sp->dim_k, 0, 0, k_dev,
                       sp->col, sp->row_of, sp->amp, sp->R, sp->orb, val, (cd*)nullptr, (cd*)nullptr);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

extern "C" int tbk_kpm_vectors(tbk_sparse* sp, uint64_t seed, int64_t first, int64_t count, double* out) {
    TBK_REQUIRE(sp && (out || count == 0), TBK_EINVAL, "tbk_kpm_vectors: null argument");
    TBK_REQUIRE(first >= 0 && count >= 0, TBK_EINVAL, "tbk_kpm_vectors: first=%lld count=%lld", (long long)first, (long long)count);
    if (count == 0) return TBK_OK;
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)count * sp->nsta * sizeof(cd);
    void* ws = nullptr;
    int rc = tbk_ctx_scratch(ctx, bytes, &ws);
    if (rc) return rc;
    {
        ProfScope ps(ctx, "kpm_randvec");
        hipLaunchKernelGGL(k_kpm_randvec, dim3(kpm_stream_grid(count * sp->nsta)), dim3(256), 0, ctx->stream, sp->nsta, seed, first,
                           count, (cd*)ws);
        TBK_HIP(hipGetLastError());
    }
    TBK_HIP(hipMemcpyAsync(out, ws, bytes, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    return TBK_OK;
}

extern "C" int tbk_kpm_moments(tbk_sparse* sp, const double* k, int64_t nk, int n_moments, double emin, double emax, int nvec,
                               const double* vectors, const int32_t* states, uint64_t seed, double* mu) {
    constexpr int NV = KPM_NV, NC = 2 * NV;
    TBK_REQUIRE(sp && mu, TBK_EINVAL, "tbk_kpm_moments: null argument");
    int rc = kpm_check_args("tbk_kpm_moments", sp, "n_moments", n_moments, nvec, vectors, states, emin, emax, k, &nk);
    if (rc) return rc;
    if (nk == 0) return TBK_OK;
    const int dim_k = sp->dim_k, n = sp->nsta;
    tbk_ctx* ctx = sp->ctx;
    TBK_HIP(hipSetDevice(ctx->device));
    const double a = 0.5 * (emax - emin), b = 0.5 * (emax + emin), inv_a = 1.0 / a;
    const int nsteps = n_moments / 2;                 // alpha_1 .. alpha_nsteps; step 0 is the norm of alpha_0
    const KpmPlan P = kpm_plan(n, nsteps);
    KpmStart start(sp, k, nk, nvec, vectors, states, seed);
    cd *val_dev, *cur, *prev;
    double *part, *dots, *mu_dev;
    size_t total;
    rc = kpm_workspace(ctx, [&](KpmCarve& c) {
        c.take(val_dev, dim_k > 0 ? (size_t)sp->nnz : 0);
        c.take(cur, (size_t)n * NV);
        c.take(prev, (size_t)n * NV);
        c.take(part, P.part_len());
        c.take(dots, (size_t)(nsteps + 1) * NC);
        c.take(mu_dev, (size_t)nk * nvec * n_moments);
        start.carve(c);
    }, &total);
    if (rc) return rc;
    rc = start.upload(ctx);
    if (rc) return rc;
    for (int64_t q = 0; q < nk; ++q) {
        const cd* val = sp->amp;
        if (dim_k > 0) {
            rc = kpm_values_at(sp, start.k_at(q), val_dev);
            if (rc) return rc;
            val = val_dev;
        }
        for (int v0 = 0; v0 < nvec; v0 += NV) {
            const int nv = std::min(NV, nvec - v0);
            rc = start.launch(ctx, P.nwg, q, v0, nv, cur, part);
            if (rc) return rc;
            rc = kpm_run_steps(ctx, P, nsteps, cur, prev, part, dots, [&](int j, const cd* x, cd* y, double* pj) {
                ProfScope ps(ctx, "kpm_step");
                if (j == 1)
                    hipLaunchKernelGGL((k_kpm_step<NV, true, KpmDots>), dim3(P.nwg), dim3(256), 0, ctx->stream, n, sp->row_ptr, sp->col, val,
                                       x, nullptr, y, b, inv_a, KpmDots{pj});
                else
                    hipLaunchKernelGGL((k_kpm_step<NV, false, KpmDots>), dim3(P.nwg), dim3(256), 0, ctx->stream, n, sp->row_ptr, sp->col, val,
                                       x, nullptr, y, b, inv_a, KpmDots{pj});
                TBK_HIP(hipGetLastError());
                return TBK_OK;
            });
            if (rc) return rc;
            ProfScope ps(ctx, "kpm_finish");
            hipLaunchKernelGGL((k_kpm_finish<NV>), dim3((unsigned)((nv * n_moments + 255) / 256)), dim3(256), 0, ctx->stream, nv, n_moments,
                               dots, mu_dev + ((size_t)q * nvec + v0) * n_moments);
            TBK_HIP(hipGetLastError());
        }
    }
    const size_t nmu = (size_t)nk * nvec * n_moments;
    TBK_HIP(hipMemcpyAsync(mu, mu_dev, nmu * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    // divergence guard: |T_m(x)| <= 1 only inside [-1, 1]; outside, the recursion grows without limit (a floating-point outcome)
    for (size_t i = 0; i < nmu; ++i)
        if (!(fabs(mu[i]) <= 1.0 + 1e-6)) {
            tbk_set_error("tbk_kpm_moments: moment %lld of sample %lld is %g: the bounds (%.17g, %.17g) do not contain the spectrum "
                          "(Gershgorin interval of this operator: (%.17g, %.17g))",
                          (long long)(i % (size_t)n_moments), (long long)(i / (size_t)n_moments), mu[i], emin, emax, sp->gmin, sp->gmax);
            return TBK_EINVAL;
        }
    return TBK_OK;
}
