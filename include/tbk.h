/* tbk.h -- C ABI of libtbk: the MI355X (gfx950) k-mesh tight-binding kernels.
 *
 * This is the drop-in boundary for PythTB's k-space hot path.  The reference
 * (PythTB 1.8.0, one pure-Python file) has no FFI of its own, so each entry
 * point below names the reference routine whose results it reproduces
 * (file:line in /root/reference/pythtb.py).  The Python side that binds these
 * with ctypes lives in pythtb_amd/_lib.py; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a TBK_E* code otherwise;
 *     tbk_last_error() gives a thread-local message for the last failure.
 *   - plain pointers and sizes only.  "c128" = interleaved (re,im) doubles.
 *     Pointers are HOST pointers unless the parameter name ends in _dev.
 *   - state index n = 2*orbital+spin for nspin=2 (the reshape of pythtb.py:933).
 *   - a handle is bound to one device and one HIP stream; calls on a handle are
 *     synchronous from the caller's view unless the name ends in _async.
 *     Handles are not thread-safe (neither are the reference's objects).
 */
#ifndef TBK_H
#define TBK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TBK_OK 0
#define TBK_EINVAL 1   /* bad argument (shape, range, null)            */
#define TBK_EHIP 2     /* a HIP runtime call failed                    */
#define TBK_ENOMEM 3   /* device or host allocation failed             */
#define TBK_EUNSUPPORTED 4 /* size outside what this build handles     */
#define TBK_ECOMM 5    /* RCCL not loadable / communicator failure     */
#define TBK_ENOCONV 6  /* an iterative kernel hit its sweep limit      */

#define TBK_MAX_DIM 4      /* dim_k, dim_arr <= 4      (pythtb.py:99)   */
#define TBK_MAX_NSTA 2048  /* states per k in this build                */
#define TBK_MAX_NOCC 16    /* largest band set of the per-thread Berry kernels (used up to 8 bands, 2 for Wilson-loop eigenphases); larger sets take the workgroup-level paths, any size */

typedef struct tbk_ctx tbk_ctx;     /* device + stream + workspaces          */
typedef struct tbk_model tbk_model; /* flattened hopping table on the device */
typedef struct tbk_wfs tbk_wfs;     /* device-resident wf_array._wfs         */

const char* tbk_last_error(void);
int tbk_version(void);
int tbk_device_count(int* count);
/* TBK_* environment knobs are parsed once, on first use; re-read them after changing one */
int tbk_knobs_reload(void);
/* 1 if this library was built with -DTBK_DIAG (ablation branches compiled into the kernels), else 0 */
int tbk_build_has_diagnostics(void);

/* ---- context -------------------------------------------------------- */
int tbk_ctx_create(int device, tbk_ctx** out);
int tbk_ctx_destroy(tbk_ctx* ctx);
int tbk_ctx_sync(tbk_ctx* ctx);
int tbk_ctx_device_info(tbk_ctx* ctx, char* name, int name_cap, int* compute_units,
                        int64_t* hbm_bytes);

/* raw device memory for callers that keep inputs/outputs resident (bench) */
int tbk_dev_alloc(tbk_ctx* ctx, int64_t bytes, void** ptr_dev);
int tbk_dev_free(tbk_ctx* ctx, void* ptr_dev);
int tbk_dev_upload(tbk_ctx* ctx, void* dst_dev, const void* src, int64_t bytes);
int tbk_dev_download(tbk_ctx* ctx, void* dst, const void* src_dev, int64_t bytes);

/* HIP-event timing on the context's stream (the stream kernels run on).
 * tbk_timer_*: one bracket around arbitrary calls.  tbk_prof_*: per-kernel
 * brackets recorded inside the library around every launch while enabled. */
int tbk_timer_begin(tbk_ctx* ctx);
int tbk_timer_end(tbk_ctx* ctx, double* elapsed_ms);
/* period: 0 = off, 1 = bracket every launch, N = bracket every N-th launch (an event
 * record costs about 3 us of stream time, so timed loops sample)                     */
int tbk_prof_enable(tbk_ctx* ctx, int period);
int tbk_prof_reset(tbk_ctx* ctx);
/* median duration of an EMPTY bracket (two event records, nothing between them)        */
int tbk_prof_calibrate(tbk_ctx* ctx, int reps, double* median_ms);
int tbk_prof_count(tbk_ctx* ctx, int* n_kernels);
int tbk_prof_get(tbk_ctx* ctx, int index, char* name, int name_cap, int64_t* launches,
                 double* total_ms);

/* ---- model tables (tb_model._site_energies/_hoppings, pythtb.py:171-180,
 *      :475-478; consumed by _gen_ham :874-925) ------------------------ */
/* orb:     norb x dim_k  reduced orbital coordinates, periodic components only
 *          (_orb[:, _per], :912-914)
 * onsite:  norb x nspin x nspin c128 (nspin=1: the real site energy as c128)
 * hop_R:   nhop x dim_k  integer lattice vectors, periodic components only
 * hop_amp: nhop x nspin x nspin c128 (the block of _val_to_block :517-560)  */
int tbk_model_upload(tbk_ctx* ctx, int dim_k, int norb, int nspin, const double* orb,
                     const double* onsite, int64_t nhop, const int32_t* hop_i,
                     const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                     tbk_model** out);
int tbk_model_free(tbk_model* model);
/* Host-only introspection of what tbk_model_upload builds (no device needed): the merged term list of
 * S_ab(k) = sum_t amp_t exp(2 pi i k.R_t), a <= b, slot = a*n - a(a-1)/2 + (b-a), in the order the kernels
 * read it.  term_cap = capacity of term_slot[], term_R[][4], term_amp[] (c128); *nterm = number of terms
 * (call with term_cap = 0 to size).  info[4] = {pmax, nR, nnz, nslot}.  For tests and sanitizer builds.   */
int tbk_model_flatten_host(int dim_k, int norb, int nspin, const double* orb, const double* onsite,
                           int64_t nhop, const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R,
                           const double* hop_amp, int64_t term_cap, int64_t* nterm, int32_t* term_slot,
                           int32_t* term_R, double* term_amp, int32_t* info);
/* The same with pinned keys pin[npin][6] = {a, b, R[4]} in STATE indices: terms that keep their slot (and cell, and lattice-vector
 * table entry) at amplitude zero; a pin on the diagonal (a == b) pins R and -R.  npin = 0 is tbk_model_flatten_host.  The mean-field
 * driver uploads its private model this way.                                                                 */
int tbk_model_flatten_host_pinned(int dim_k, int norb, int nspin, const double* orb, const double* onsite,
                                  int64_t nhop, const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R,
                                  const double* hop_amp, int64_t npin, const int32_t* pin, int64_t term_cap, int64_t* nterm,
                                  int32_t* term_slot, int32_t* term_R, double* term_amp, int32_t* info);
int tbk_model_info(tbk_model* model, int* dim_k, int* nsta, int64_t* nterm);

/* Host-only: continuity of Berry phases along the first index of a result array (berry_phase(contin=True), pythtb.py:2980-3036).
 * tbk_one_phase_cont  = _one_phase_cont  (pythtb.py:3876-3889): pha[n] unwrapped by 2 pi steps, the first entry anchored at clos.
 * tbk_array_phases_cont = _array_phases_cont (pythtb.py:3891-3921): arr[n0][nb] eigenphase sets; set i is matched greedily to the
 * previous (already continuous) set by distance on the unit circle -- the LAST index among equal minima, like the reference's <= --
 * and unwrapped; clos[nb] anchors set 0.  `stride` = doubles between consecutive sets / entries (a column of a larger array).
 * No device call, no context.                                                                                                   */
int tbk_one_phase_cont(const double* pha, int64_t n, int64_t stride, double clos, double* out, int64_t out_stride);
int tbk_array_phases_cont(const double* arr, int64_t n0, int nb, int64_t stride, const double* clos, double* out,
                          int64_t out_stride);

/* ---- H(k) and eigen-solve ------------------------------------------- */
/* _gen_ham (pythtb.py:874-925) for nk points: ham_out[nk][nsta][nsta] c128.
 * k: nk x dim_k reduced coordinates (ignored when dim_k == 0).            */
int tbk_gen_ham(tbk_model* model, const double* k, int64_t nk, double* ham_out);

/* solve_all (pythtb.py:955-1079) = _gen_ham + _sol_ham (:927-953) fused:
 * eval[nsta][nk] ascending per k; evec[nsta][nk][nsta] c128 (rows are
 * eigenvectors, band-major) or NULL for eigenvalues only.                  */
int tbk_solve_list(tbk_model* model, const double* k, int64_t nk, double* eval, double* evec);
/* same, all buffers already on the device (no PCIe in the call)           */
int tbk_solve_list_dev(tbk_model* model, const double* k_dev, int64_t nk, double* eval_dev,
                       double* evec_dev);
/* tbk_solve_list_dev followed by the read (and reset) of the context's sticky solver status -- one host synchronisation:
 * TBK_ENOCONV where numpy.linalg.eigh would raise (pythtb.py:939-944: an iteration limit, a NaN model); a rotation-record
 * overflow of the direct solvers is repeated once on the Jacobi kernels.  What every caller that hands results on (a gather,
 * a download) must use: the unchecked form leaves the status set for the next checked call on the context.               */
int tbk_solve_list_dev_checked(tbk_model* model, const double* k_dev, int64_t nk, double* eval_dev,
                               double* evec_dev);

/* _sol_ham (pythtb.py:927-953) on caller-supplied Hermitian matrices
 * ham[nk][n][n] c128 -> eval[n][nk], evec[n][nk][n] (or NULL).            */
int tbk_eigh_batch(tbk_ctx* ctx, int n, const double* ham, int64_t nk, double* eval,
                   double* evec);

/* Which of the eigen-solver's regimes a batch would take (host only, no device): the dispatch of _sol_ham's replacement is
 * ONE table of (states, eigenvectors?, input form, batch window) rows with the measured crossovers as data
 * (tbk_solve.hip, kRegimeRules).  form: 0 k list, 1 regular mesh, 2 supplied matrices; nk: matrices of the call; batch:
 * matrices of the global mesh (= nk for lists); compute_units <= 0: 256.  Returns a static name ("trig", "blocked", "big",
 * "reg", "ql16", "qlw", "row16", "wg_lds", "wg_global", "wave", "ql_small", "closed_form"); *note_out (nullable) the
 * measurement behind the matching row.                                                                                  */
const char* tbk_solver_regime(int n, int with_vectors, int form, int64_t nk, int64_t batch,
                              int compute_units, int has_rblocks, const char** note_out);

/* ---- wf_array storage (pythtb.py:2388-2419): _wfs[k1..kD][state][comp] */
int tbk_wfs_create(tbk_ctx* ctx, int dim_arr, const int32_t* mesh, int nsta_arr, int ncomp,
                   tbk_wfs** out);
int tbk_wfs_free(tbk_wfs* wfs);
int tbk_wfs_upload(tbk_wfs* wfs, const double* host_c128);
int tbk_wfs_download(tbk_wfs* wfs, double* host_c128);
int tbk_wfs_device_ptr(tbk_wfs* wfs, void** ptr_dev, int64_t* bytes);
/* wf_array.choose_states (pythtb.py:2568-2608) on the device: dst (same mesh and ncomp, nsta_arr = nb) receives the
 * states bands[0..nb) of src.  Band planes are contiguous in HBM, so this is nb device-to-device copies.            */
int tbk_wfs_copy_bands(tbk_wfs* dst, tbk_wfs* src, const int32_t* bands, int nb);
/* wf_array.__getitem__/__setitem__ (pythtb.py:2644-2672) on a resident array: copy the states of
 * npoints mesh points (row-major mesh indices) to/from host[npoints][nsta_arr][ncomp] c128 without
 * moving the rest of the array.                                                              */
int tbk_wfs_download_points(tbk_wfs* wfs, const int64_t* point_index, int64_t npoints, double* host_c128);
int tbk_wfs_upload_points(tbk_wfs* wfs, const int64_t* point_index, int64_t npoints, const double* host_c128);
/* bytes and calls of wf_array traffic across PCIe since the last reset (whole-array upload/download
 * and the per-point forms): lets callers and tests assert that a script causes no re-uploads. */
int tbk_ctx_transfer_stats(tbk_ctx* ctx, int64_t* h2d_bytes, int64_t* d2h_bytes, int64_t* h2d_calls,
                           int64_t* d2h_calls, int reset);
/* diagnostics of the eigen-solver since the last reset: `listed_matrices` = matrices of 9..16 states that the direct kernels
 * (k_e16 / k_tw16_*) could not finish themselves (three or more eigenvalues of a block within gaptol, a failed residual)
 * and handed to the QL-replay fallback.  Results are the same either way; the count tells a regression of the in-kernel
 * repairs from a healthy launch without timing anything.  Synchronises the context's stream.  (No reference counterpart:
 * numpy.linalg.eigh, pythtb.py:939-947, has one path.)                                                              */
int tbk_ctx_solver_stats(tbk_ctx* ctx, int64_t* listed_matrices, int reset);

/* solve_on_grid (pythtb.py:2421-2532): every mesh point i_d < N_d-1 solved at
 * start_k[d] + i_d/(N_d-1); the points with i_d == N_d-1 are the impose_pbc
 * images (:2729-2747), produced in the same launch by solving k(i_d=0) again
 * and multiplying by pbc_phase[d][comp] (c128, = exp(-2 pi i orb[:,per[d]])).
 * min_gaps[nsta-1] = min over solved points of E[b+1]-E[b] (:2495,:2530).
 * Slab form for k-sharding along mesh axis 0: the handle holds rows
 * [row0, row0+mesh[0]) of a global mesh whose axis-0 size is global_n0
 * (pass row0=0, global_n0=mesh[0] for the whole mesh).                     */
int tbk_wfs_solve_grid(tbk_wfs* wfs, tbk_model* model, const double* start_k,
                       const double* pbc_phase, int64_t row0, int64_t global_n0,
                       double* min_gaps);
/* Launch-only forms (no host synchronisation, no PCIe traffic): results stay
 * in device buffers owned by the handle until the matching *_result call.  */
int tbk_wfs_solve_grid_async(tbk_wfs* wfs, tbk_model* model, const double* start_k,
                             const double* pbc_phase, int64_t row0, int64_t global_n0);
int tbk_wfs_solve_grid_result(tbk_wfs* wfs, double* min_gaps);
/* General sharding window: the handle holds the points [offset[d], offset[d]+mesh[d]) of a
 * global mesh of global_mesh[d] points along every axis d (k-sharding of Berry strings
 * cuts an axis other than 0).  Results through tbk_wfs_solve_grid_result.              */
int tbk_wfs_solve_window_async(tbk_wfs* wfs, tbk_model* model, const double* start_k,
                               const double* pbc_phase, const int64_t* offset,
                               const int64_t* global_mesh);
/* solve_on_grid (:2421-2532) followed by berry_flux(occ, dirs=[0,1]) (:3068-3205, _one_flux_plane :3840-3865) in ONE pass over
 * a 2-D array of 2 or 4 states: the plaquette phases are formed from the eigenvectors while they are in registers, so the
 * array is written once and never read back.  occ: 1 or 2 bands.  Launch only; the results through
 * tbk_wfs_solve_grid_result (min gaps) and tbk_berry_flux_result (the total: same value as the two separate calls up to the
 * order of the sum).  TBK_EUNSUPPORTED where the fused kernel does not apply (other dimensions, state counts, long-ranged
 * models along the last axis): issue the two calls then.                                                              */
int tbk_wfs_solve_grid_flux_async(tbk_wfs* wfs, tbk_model* model, const double* start_k,
                                  const double* pbc_phase, int64_t row0, int64_t global_n0,
                                  const int32_t* occ, int nocc);
/* impose_pbc (:2674-2749) / impose_loop (:2751-2791) on a filled array:
 * last slice along mesh_dir = first slice * phase[comp] (phase NULL: copy) */
int tbk_wfs_impose(tbk_wfs* wfs, int mesh_dir, const double* phase_c128);

/* ---- Berry quantities ----------------------------------------------- */
/* berry_flux (pythtb.py:3068-3205) / _one_flux_plane (:3840-3865):
 * plaquette phases on the (dir0,dir1) planes for bands occ[nocc].
 * totals[n_slices]: sum over each plane (slices = remaining axes, row-major
 * in original axis order).  plaq (nullable): [n_slices][N_dir0-1][N_dir1-1].
 * The sum is a fixed-shape tree (no float atomics): bit-reproducible.       */
int tbk_berry_flux(tbk_wfs* wfs, const int32_t* occ, int nocc, int dir0, int dir1,
                   double* totals, double* plaq);

int tbk_berry_flux_async(tbk_wfs* wfs, const int32_t* occ, int nocc, int dir0, int dir1,
                         int want_plaq);
int tbk_berry_flux_result(tbk_wfs* wfs, double* totals, double* plaq);

/* berry_phase (pythtb.py:2863-3066) / _one_berry_loop (:3798-3838) for every
 * string along `dir` (strings = remaining axes, row-major in original order).
 * berry_evals == 0: out[n_strings]        = -arg det prod_i M_i
 * berry_evals != 0: out[n_strings][nocc]  = sorted -arg eig prod_i polar(M_i)
 * (the contin post-processing :3036-3065 is O(n_strings) host work).        */
int tbk_berry_phase(tbk_wfs* wfs, const int32_t* occ, int nocc, int dir, int berry_evals,
                    double* out);

/* ---- position operator / hybrid Wannier functions (first "next" row) ----
 * tb_model.position_matrix (pythtb.py:2034-2098), position_expectation (:2100-2141) and
 * position_hwf (:2143-2279), batched over nk points.
 * evec[nk][nsub][ncomp] c128: the states at each point; pos[ncomp]: reduced coordinate of
 * each component's orbital along the chosen non-periodic direction (repeated per spin).
 * xmat (nullable)  [nk][nsub][nsub] c128      X_mn = <u_m| r |u_n>
 * hwfc (nullable)  [nk][nsub]                 eigenvalues of X, ascending
 * hwf  (nullable)  [nk][nsub][nsub]  rows = eigenvectors of X on the input states, or with
 *                  orbital_basis != 0 [nk][nsub][ncomp] expanded on the orbitals (:2262-2277) */
int tbk_position_hwf(tbk_ctx* ctx, const double* evec, int64_t nk, int nsub, int ncomp,
                     const double* pos, double* xmat, double* hwfc, double* hwf, int orbital_basis);

/* The same on the states `occ[nocc]` of a RESIDENT wf_array (wf_array.position_matrix / _expectation /
 * _hwf, pythtb.py:2793-2861): nothing but the results crosses PCIe.  point_index (nullable): row-major
 * mesh indices of the npoints points wanted; NULL = every mesh point in order (npoints ignored).
 * Output shapes as above with nk = number of points, nsub = nocc.                                   */
int tbk_wfs_position_hwf(tbk_wfs* wfs, const int64_t* point_index, int64_t npoints, const int32_t* occ, int nocc,
                         const double* pos, double* xmat, double* hwfc, double* hwf, int orbital_basis);

/* ---- k generators on the device, eigenvalue reductions (third "next" row) ----
 * tb_model.k_uniform_mesh (pythtb.py:1792-1861): k_dev[prod(mesh)][dim_k], point
 * (i_0,..) row-major = (i_0/N_0, ...); dim_k 1..3 like the reference.                  */
int tbk_k_uniform_mesh_dev(tbk_ctx* ctx, int dim_k, const int32_t* mesh, double* k_dev);
/* points [first, first+count) of that list only: the chunk one rank of a k-sharded solve_all owns  */
int tbk_k_uniform_mesh_range_dev(tbk_ctx* ctx, int dim_k, const int32_t* mesh, int64_t first,
                                 int64_t count, double* k_dev);
/* interpolation step of tb_model.k_path (pythtb.py:1978-1996): nodes[n_nodes][dim_k] and
 * node_index[n_nodes] (0 .. nk-1, increasing; both computed on the host, :1926-1976)
 * -> k_dev[nk][dim_k], bit-equal to the reference's k_vec.                             */
int tbk_k_path_dev(tbk_ctx* ctx, int dim_k, int n_nodes, const double* nodes,
                   const int32_t* node_index, int64_t nk, double* k_dev);
/* solve_all(k_uniform_mesh(mesh)) with the k list generated on the device (no upload):
 * eval[n][nk], evec[n][nk][n] or NULL.                                                  */
int tbk_solve_mesh(tbk_model* model, const int32_t* mesh, double* eval, double* evec);
/* The reduction of the reference's DOS example (examples/haldane.py:96-121: histogram of
 * solve_all over a uniform mesh) without downloading the eigenvalues: counts[n][nbins] per
 * band with np.histogram's bin rule for the given edges[nbins+1] (equal-width bins, last
 * bin closed), and/or the band extrema band_min[n], band_max[n] (each nullable;
 * nbins = 0 with edges = counts = NULL computes the extrema alone).                     */
int tbk_dos_mesh(tbk_model* model, const int32_t* mesh, int nbins, const double* edges,
                 int64_t* counts, double* band_min, double* band_max);

/* ---- Berry curvature by the Kubo formula ----------
 * k in reduced coordinates, H the convention-II matrix of tbk_gen_ham.  No reference counterpart (PythTB 1.8 has only the
 * link products of berry_flux); the quantities PythTB 2 and Wannier-interpolation codes call the Berry curvature.
 * d_dir H(k) = sum_t amp 2 pi i (R + tau_j - tau_i)_dir exp(2 pi i k.(R + tau_j - tau_i)) for nk points:
 * out[nk][nsta][nsta] c128, the layout of tbk_gen_ham.  dir in [0, dim_k).                                        */
int tbk_gen_dham(tbk_model* model, const double* k, int64_t nk, int dir, double* out);
/* Omega on a k list k[nk][dim_k], dirs (dir0, dir1) distinct in [0, dim_k), dim_k >= 2.
 * occ == NULL: per band, out[nsta][nk], Omega_n = -2 Im sum_{m != n} V^a_nm V^b_mn / (E_n - E_m)^2 (pairs closer than
 *              1e-9 max(1, |E_n|, |E_m|) left out);
 * otherwise:   the manifold of the bands occ[nocc] (distinct, in [0, nsta)), out[nk], the sum over n in occ, m not in occ. */
int tbk_berry_curv_list(tbk_model* model, const double* k, int64_t nk, int dir0, int dir1,
                        const int32_t* occ, int nocc, double* out);
/* Plane means of Omega over k_uniform_mesh(mesh) (dim_k 2 or 3), generated on the device: per band out[nsta] (occ NULL,
 * nmu 0), manifold out[1] (occ given), or the T = 0 Fermi scan out[nmu], I(mu) = mean_k sum_{n: E_n(k) <= mu} Omega_n(k)
 * for nmu (1..8192) levels mu[] in any order (occ NULL).  A 3-D mesh gains a trailing axis over the remaining mesh
 * direction: out[..][N_rest].  Fixed-shape reductions: bit-reproducible.                                           */
int tbk_berry_curv_mesh(tbk_model* model, const int32_t* mesh, int dir0, int dir1, const int32_t* occ,
                        int nocc, int nmu, const double* mu, double* out);

/* ---- quantum geometric tensor and quantum metric by the Kubo formula ----------
 * Q_ab = g_ab - i Omega_ab / 2 over ALL axes a, b in [0, dim_k), dim_k 1..3: the real part of the sum whose imaginary part is
 * tbk_berry_curv_list's.  occ == NULL: per band, Q^n_ab = sum_{m != n} V^a_nm V^b_mn / (E_n - E_m)^2 with the degeneracy rule of
 * tbk_berry_curv_list; otherwise the band set occ[nocc] (distinct, in [0, nsta)), the sum over n in occ, m not in occ.
 * A (band or set, point) result is dim_k^2 doubles: g_ab for a <= b in row-major upper-triangle order, then Omega_ab for a < b
 * in the same order.  tbk_qgt_list: out[nsta][nk][dim_k^2] per band, out[nk][dim_k^2] for a set.
 * tbk_qgt_mesh: the means over the whole k_uniform_mesh(mesh) (mesh[d] >= 1, generated on the device), out[nsta][dim_k^2] or
 * out[dim_k^2].  Fixed-shape reductions: bit-reproducible.                                                         */
int tbk_qgt_list(tbk_model* model, const double* k, int64_t nk, const int32_t* occ, int nocc, double* out);
int tbk_qgt_mesh(tbk_model* model, const int32_t* mesh, const int32_t* occ, int nocc, double* out);

/* ---- spin Berry curvature and spin Hall conductivity by the Kubo formula ----------
 * For a model with nspin = 2 (state = 2 orbital + spin).  Sigma_s = 1_orb (x) (s.sigma) for the real vector spin[3] (used as
 * given, not normalised; every result is linear in it), J^{s,a} = (Sigma_s d_a H + d_a H Sigma_s) / 2 the spin current:
 *   Omega^s_n = -2 Im sum_{m != n} J^{s,a}_nm V^b_mn / (E_n - E_m)^2,   (a, b) = (dir0, dir1),
 * with the degeneracy rule, the band-set form, the Fermi scan, the shapes and the argument rules of tbk_berry_curv_list and
 * tbk_berry_curv_mesh.  With spin hbar sigma / 2, sigma^s_ab = (e / 4 pi) I^s / (2 pi) per layer for the mesh mean I^s; an
 * S_z-conserving model has I^s / (2 pi) = C_up - C_down.  A model with nspin = 1 or a non-finite spin[] is TBK_EINVAL.
 * tbk_gen_jham: J^{s,dir}(k) for nk points, out[nk][nsta][nsta] c128 (the layout of tbk_gen_dham).                  */
int tbk_gen_jham(tbk_model* model, const double* k, int64_t nk, int dir, const double spin[3], double* out);
int tbk_spin_curv_list(tbk_model* model, const double* k, int64_t nk, int dir0, int dir1,
                       const int32_t* occ, int nocc, const double spin[3], double* out);
int tbk_spin_curv_mesh(tbk_model* model, const int32_t* mesh, int dir0, int dir1, const int32_t* occ,
                       int nocc, int nmu, const double* mu, const double spin[3], double* out);

/* ---- interband optical conductivity by the Kubo formula ----------
 * k reduced, H the convention-II matrix of tbk_gen_ham, V^a = d_a H (tbk_gen_dham), E_n, |n> the eigenpairs of the solver,
 * f_n = [E_n <= mu] for kT = 0, else 1 / (1 + exp((E_n - mu) / kT)); the mean over k_uniform_mesh(mesh) (dim_k 1..3, N_k points):
 *   S_ab(w) = (i / N_k) sum_k sum_{n != m} [(f_m - f_n) / (E_m - E_n)] V^a_nm V^b_mn / (E_m - E_n - w - i eta)
 * pairs with |E_m - E_n| <= 1e-9 max(1, |E_n|, |E_m|) left out (interband only), time dependence e^{-i w t}, no spin factor.
 * Reduced units: sigma = A^T S A / ((2 pi)^2 V_c) in e^2/hbar x length^(2 - dim_k), A the periodic lattice vectors as rows,
 * V_c = sqrt(det(A A^T)); at w -> 0 the antisymmetric part Re (S_ab - S_ba) / 2 is minus the Fermi scan of tbk_berry_curv_mesh.
 * nomega (1..65536) finite frequencies omega[] in any order, eta > 0, kT >= 0, all finite.  dir0 = dir1 = -1: the full tensor,
 * out[nomega][dim_k][dim_k] c128; otherwise the one component S_{dir0 dir1}, out[nomega] c128 (dir0 == dir1 allowed).
 * Fixed partitions, no atomics: bit-reproducible.                                                                          */
int tbk_optical_cond_mesh(tbk_model* model, const int32_t* mesh, int nomega, const double* omega, double eta, double mu,
                          double kT, int dir0, int dir1, double* out);

/* ---- orbital moments and orbital magnetization by the Kubo formula ----------
 * k reduced, V^d = d_d H (tbk_gen_dham), E_n, |n> the eigenpairs of the solver, (a, b) = (dir0, dir1) distinct in [0, dim_k),
 * dim_k >= 2, P_nm = Im V^a_nm V^b_mn, Delta_nm = E_n - E_m.
 * On a k list k[nk][dim_k]:
 *   occ == NULL: per band, out[nsta][nk], m_n = sum_{m != n} P_nm / (E_m - E_n) (pairs closer than 1e-9 max(1, |E_n|, |E_m|)
 *                left out, as tbk_berry_curv_list);
 *   otherwise:   out[nk] = LC + IC of the bands occ[nocc], LC = sum_{n in occ, m not in occ} P_nm E_m / Delta^2,
 *                IC = (same) P_nm E_n / Delta^2.                                                                          */
int tbk_orb_moment_list(tbk_model* model, const double* k, int64_t nk, int dir0, int dir1, const int32_t* occ, int nocc,
                        double* out);
/* Plane means over k_uniform_mesh(mesh) (dim_k 2 or 3), generated on the device; exactly one of occ and mu[nmu]:
 *   occ given:  out[3] = (LC, IC, Omega_occ), Omega_occ = -2 sum_{n in occ, m not in occ} P_nm / Delta^2 (kT must be 0);
 *   nmu levels (1..8192, finite, any order): out[nmu], M(mu) = mean_k sum_n [f_n m_n + g_n Omega_n] with Omega_n the
 *   per-band curvature of tbk_berry_curv_list; kT = 0: f = [E_n <= mu], g = (mu - E_n) f; kT > 0: f = 1 / (1 + e^x),
 *   g = kT ln(1 + e^-x), x = (E_n - mu) / kT.
 * M_z = -(q / hbar) M / (2 pi)^2 per area for dirs (0, 1) of a 2-D cell with a1 x a2 along +z.  A 3-D mesh gains a trailing
 * axis over the remaining mesh direction: out[..][N_rest].  Fixed-shape reductions, no atomics: bit-reproducible.      */
int tbk_orb_mag_mesh(tbk_model* model, const int32_t* mesh, int dir0, int dir1, const int32_t* occ, int nocc, int nmu,
                     const double* mu, double kT, double* out);

/* ---- Fermi-surface transport ----------
 * k reduced, V^c = d_c H (tbk_gen_dham), E_n, |n> the eigenpairs of the solver, dim_k 1..3.  A group G at a k point is a maximal
 * run of consecutive sorted levels, each within 1e-9 max(1, |E|, |E'|) of its predecessor (the pair rule of tbk_berry_curv_list).
 * For band n in G: vbar^c_n = mean over m in G of <m|V^c|m>, w^{cd}_n = sum_{m in G} Re <n|V^c|m><m|V^d|n>; both group sums are
 * independent of the solver's choice of eigenvectors inside G.  x = (E_n - mu) / kT, f = 1 / (1 + e^x), -f' = -df/dE,
 * s = -f ln f - (1 - f) ln(1 - f).
 * Band velocities on a k list k[nk][dim_k]: the raw diagonal elements v^c_n = <n|V^c|n> (the derivative of an isolated band's
 * eigenvalue; inside a group only the group's trace is defined).  dir = -1: out[dim_k][nsta][nk]; dir in [0, dim_k): out[nsta][nk]. */
int tbk_band_velocity_list(tbk_model* model, const double* k, int64_t nk, int dir, double* out);
/* Plane means over k_uniform_mesh(mesh) (dim_k 2 or 3), (dir0, dir1) distinct, nmu (1..8192) finite levels in any order, kT > 0:
 *   out[2 + dim_k][nmu] = hall, nernst, dipole_0 .. dipole_{dim_k - 1}:  mean_k sum_n f_n Omega_n,  mean_k sum_n s_n Omega_n,
 *   mean_k sum_n (-f')_n Omega_n vbar^c_n, with Omega_n the per-band curvature of tbk_berry_curv_list(dir0, dir1).
 * A 3-D mesh gains a trailing axis over the remaining mesh direction: out[..][nmu][N_rest].                             */
int tbk_anom_transport_mesh(tbk_model* model, const int32_t* mesh, int dir0, int dir1, int nmu, const double* mu, double kT,
                            double* out);
/* The Drude weight, the mean over the whole k_uniform_mesh(mesh) (dim_k 1..3): out[nmu][dim_k (dim_k + 1) / 2],
 * D_cd = mean_k sum_n (-f')_n w^{cd}_n for c <= d row by row: the intraband pairs that tbk_optical_cond_mesh leaves out.
 * Both mesh calls: fixed partitions, no atomics on floating-point data: bit-reproducible.                               */
int tbk_drude_mesh(tbk_model* model, const int32_t* mesh, int nmu, const double* mu, double kT, double* out);

/* ---- shift and injection photocurrents: the interband second-order response ----------
 * k reduced, V^a = d_a H (tbk_gen_dham), W^{ab} = d_a d_b H (tbk_gen_ddham), E_n, |n> the eigenpairs of the solver, E_nm = E_n - E_m,
 * G(n) the group of band n (the rule of the transport block above), f as in tbk_optical_cond_mesh.  For G(n) != G(m):
 *   r^b_nm   = -i V^b_nm / E_nm   (0 inside a group)
 *   r^b_nm;a = (i / E_nm) [T^{ba}_nm / E_nm - W^{ba}_nm + sum_{p not in G(n) u G(m)} (V^b_np V^a_pm / E_pm - V^a_np V^b_pm / E_np)]
 *   T^{ba}_nm = sum_{p in G(n)} (V^a_np V^b_pm + V^b_np V^a_pm) - sum_{p in G(m)} (V^b_np V^a_pm + V^a_np V^b_pm)
 *   X^{abc}_nm = r^b_mn r^c_nm;a + r^c_mn r^b_nm;a
 *   Y^{abc}_nm = sum_{m' in G(m)} V^a_mm' r^c_m'n r^b_nm - sum_{n' in G(n)} r^c_mn V^a_nn' r^b_n'm
 * (groups of one: T^{ba}_nm = V^b_nm D^a_nm + V^a_nm D^b_nm and Y^{abc}_nm = D^a_mn r^b_nm r^c_mn, D^a_nm = V^a_nn - V^a_mm).  The sums
 * over (n in G1, m in G2) do not depend on the solver's choice of eigenvectors inside a group; nothing beyond that has been validated
 * for models whose in-group velocity blocks are not multiples of the identity.
 * tbk_gen_ddham: d_dir0 d_dir1 H(k) = sum_t amp (2 pi i)^2 (R + tau_j - tau_i)_dir0 (R + tau_j - tau_i)_dir1 exp(2 pi i k.(R + tau_j -
 * tau_i)) for nk points, out[nk][nsta][nsta] c128 (the layout of tbk_gen_dham); dir0 == dir1 allowed.                            */
int tbk_gen_ddham(tbk_model* model, const double* k, int64_t nk, int dir0, int dir1, double* out);
/* The k-resolved shift transition strength on a k list k[nk][dim_k] (dim_k 1..3): out[nk] = sum_{n in occ, m not in occ,
 * G(n) != G(m)} Im X^{abc}_nm for the bands occ[nocc] (distinct, in [0, nsta)); a, b, c axes in [0, dim_k), repeats allowed.     */
int tbk_shift_list(tbk_model* model, const double* k, int64_t nk, int a, int b, int c, const int32_t* occ, int nocc, double* out);
/* Means over k_uniform_mesh(mesh) (dim_k 1..3), generated on the device, with D(eps, w) = (eta / pi) [1 / ((eps - w)^2 + eta^2) +
 * 1 / ((eps + w)^2 + eta^2)]:
 *   kind 0 (shift):      K_abc(w) = mean_k sum_{E_m > E_n, G(n) != G(m)} (f_n - f_m) Im X^{abc}_nm D(E_m - E_n, w), real, K_abc = K_acb
 *   kind 1 (injection):  N_abc(w) = the same sum of Y^{abc}_nm, complex, N_acb = conj N_abc
 * Cartesian shift conductivity: sigma^{xyz} = (pi / 2) sum_abc A_ax A_by A_cz K_abc / ((2 pi)^3 V_c) in e^3/hbar^2 x length^(3 - dim_k),
 * A and V_c as in tbk_optical_cond_mesh.  nomega (1..65536) finite frequencies in any order, eta > 0, kT >= 0, all finite.
 * a = b = c = -1: the full tensor, out[nomega][dim_k][dim_k][dim_k] (doubles for kind 0, c128 for kind 1); otherwise the one
 * component, out[nomega].  One state, or kT = 0 with mu outside the spectrum: exact zeros.  Fixed partitions, no atomics:
 * bit-reproducible.                                                                                                            */
int tbk_photocurrent_mesh(tbk_model* model, const int32_t* mesh, int kind /*0 shift, 1 injection*/, int nomega, const double* omega,
                          double eta, double mu, double kT, int a, int b, int c /* all -1: full tensor */, double* out);

/* ---- surface Green's functions by iterative decimation ----------
 * No reference counterpart (the reference's route to an edge spectrum is cut_piece + solve_all on a ribbon).  `cut` is the uploaded
 * cut_piece(2 L, fin_dir) of the model, L = max(1, max |R_fin_dir|): 2 nlayer states, nlayer = L ncell the principal layer, ncell the
 * states of one unit cell; its dim_k (0..3) is the dimension of the surface zone and k[nk][dim_k] its reduced coordinates (dim_k = 0:
 * k ignored, nk = 1).  H00(k), H01(k): the top-left and top-right nlayer x nlayer blocks of that model's H(k) (tbk_gen_ham).
 * tbk_surface_blocks: h00[nk][nlayer][nlayer], h01[nk][nlayer][nlayer] c128.                                                    */
int tbk_surface_blocks(tbk_model* cut, int nlayer, const double* k, int64_t nk, double* h00, double* h01);
/* z = omega + i eta.  With es = et = e = H00, al = H01, be = H01^+ one step is g = (z - e)^-1, es += al g be, et += be g al,
 * e += al g be + be g al, al <- al g al, be <- be g be; after i steps G_0 = (z - es)^-1 (side 0: the crystal fills cells >= 0, cell 0
 * exposed), G_1 = (z - et)^-1 (side 1: cells <= 0, the last cell of the layer exposed), G_b = (z - e)^-1 (side 2: bulk).  A point
 * (k, omega) stops at the first i >= 0 with max(|al|_max, |be|_max) <= tol max(|H00|_max, |H01|_max); tol = 0: exactly max_iter steps.
 * TBK_ENOCONV (the message counts the points) when a point misses a non-zero tol after max_iter (0..64) steps.
 * nomega (1..65536) finite frequencies in any order, eta > 0, tol >= 0, all finite; nlayer <= 128 (TBK_EUNSUPPORTED beyond).
 *   mode 0: out[nk][nomega][nlayer][nlayer] c128, the Green's function of `side` (0, 1, 2)
 *   mode 1: out[3][nk][nomega], A = -(1 / pi) Im sum_s G_ss over the states of the exposed unit cell (cell 0; the last cell for side 1)
 *   mode 2: out[3][nk][nomega][ncell], that diagonal itself
 * info (nullable): [nk][nomega] steps taken.  The value at a point does not depend on the rest of the call: same bits alone, in any
 * batch, at any position.                                                                                                       */
int tbk_surface_green_list(tbk_model* cut, int nlayer, int ncell, const double* k, int64_t nk, int nomega, const double* omega,
                           double eta, double tol, int max_iter, int mode, int side, double* out, int32_t* info);
/* the mean of modes 1 (per_state = 0: out[3][nomega]) and 2 (out[3][nomega][ncell]) over k_uniform_mesh(mesh) of the surface zone
 * (dim_k 1..3), generated on the device; fixed-order sums, no atomics on floating-point data: bit-reproducible.                */
int tbk_surface_dos_mesh(tbk_model* cut, int nlayer, int ncell, const int32_t* mesh, int nomega, const double* omega, double eta,
                         double tol, int max_iter, int per_state, double* out);

/* ---- Landauer transmission through a scattering region between two leads of the crystal ----------
 * No reference counterpart.  `cut`, nlayer, k, omega, eta, tol, max_iter and the decimation as in the surface calls above.  The left
 * lead fills the layers <= 0 and the right one the layers >= nlayers + 1; with G_0 = (z - es)^-1, G_1 = (z - et)^-1 of that decimation
 *   Sigma_R = H01 G_0 H01^+ (side 0, on layer nlayers),   Sigma_L = H01^+ G_1 H01 (side 1, on layer 1),   Gamma = i (Sigma - Sigma^+).
 * `dev` is the uploaded device: a model of nlayers nlayer states (1..1024 layers) with the dim_k and the context of `cut`, whose H(k)
 * is block-tridiagonal in layers of nlayer states, D_i (i = 1..nlayers) on the diagonal and U_i = H_{i,i+1} above it; slots that join
 * layers further apart are ignored (the Python layer rejects such a device).
 * tbk_landauer_blocks: d[nk][nlayers][nlayer][nlayer], u[nk][nlayers - 1][nlayer][nlayer] c128 (u nullable for one layer).        */
int tbk_landauer_blocks(tbk_model* dev, int nlayer, int nlayers, const double* k, int64_t nk, double* d, double* u);
/* out[nk][nomega][nlayer][nlayer] c128: Sigma_R (side 0) or Sigma_L (side 1); info (nullable): [nk][nomega] decimation steps.   */
int tbk_lead_self_energy_list(tbk_model* cut, int nlayer, const double* k, int64_t nk, int nomega, const double* omega,
                              double eta, double tol, int max_iter, int side, double* out, int32_t* info);
/* T = Re Tr[Gamma_R P Gamma_L P^+], P = G_{nlayers,1} of (z - H_dev - Sigma_L (+) Sigma_R)^-1 by the forward sweep A_1 = z - D_1 -
 * Sigma_L, A_i = z - D_i - U_{i-1}^+ A_{i-1}^-1 U_{i-1}, A_nlayers additionally - Sigma_R, P_1 = A_1^-1, P_i = A_i^-1 U_{i-1}^+ P_{i-1};
 * the same eta in the leads and in the device.  out[nk][nomega] doubles, info as above.  dev = null: one pristine layer (nlayers = 1,
 * D_1 = H00).  TBK_ENOCONV as the surface calls; TBK_EUNSUPPORTED (the message says what to split) when the buffers of a call would
 * pass 4 GiB.  The value at a point does not depend on the rest of the call: same bits alone, in any batch, at any position.         */
int tbk_transmission_list(tbk_model* cut, tbk_model* dev /* null: one pristine layer */, int nlayer, int nlayers,
                          const double* k, int64_t nk, int nomega, const double* omega, double eta, double tol,
                          int max_iter, double* out, int32_t* info);
/* out[nomega]: the mean of T over k_uniform_mesh(mesh) of the surface zone (dim_k 1..3), generated on the device; fixed-order sums,
 * no atomics on floating-point data: bit-reproducible.                                                                           */
int tbk_transmission_mesh(tbk_model* cut, tbk_model* dev, int nlayer, int nlayers, const int32_t* mesh, int nomega,
                          const double* omega, double eta, double tol, int max_iter, double* out);

/* ---- kernel polynomial method: Chebyshev moments of the sparse H(k), any number of states ----------
 * No reference counterpart.  The tables are those of tbk_model_upload; the operator is CSR over the states (nsta = norb nspin rows, no
 * TBK_MAX_NSTA limit): the on-site blocks, every hop and its Hermitian conjugate, spin blocks expanded to scalar entries, entries with
 * the same (row, col, R) summed, exact zeros dropped, (col, R) ascending within a row.  The value of an entry at k is
 * amp exp(2 pi i k.(R + orb_col - orb_row)) (_gen_ham, pythtb.py:874-925).  The Gershgorin interval [min_i (d_i - r_i),
 * max_i (d_i + r_i)], d_i the real R = 0 diagonal entry and r_i the sum of the moduli of the other entries of row i, contains the
 * spectrum at every k.
 * tbk_sparse_flatten_host: host only (no device call).  *nnz = number of entries (call with cap = 0 to size); with cap >= *nnz,
 * row_ptr[nsta + 1], col[nnz], ent_R[nnz][4] (zero-padded beyond dim_k), ent_amp[nnz] c128; gershgorin[2] (nullable).          */
typedef struct tbk_sparse tbk_sparse;
int tbk_sparse_flatten_host(int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                            const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp, int64_t cap,
                            int64_t* nnz, int64_t* row_ptr, int32_t* col, int32_t* ent_R, double* ent_amp, double* gershgorin);
int tbk_sparse_upload(tbk_ctx* ctx, int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                      const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp, tbk_sparse** out);
int tbk_sparse_free(tbk_sparse* sp);
int tbk_sparse_info(tbk_sparse* sp, int* dim_k, int* nsta, int64_t* nnz, double* gershgorin);
/* Random-phase vectors number first .. first + count - 1 of `seed`: out[count][nsta] c128, element i of vector g = e^{i phi}, phi a pure
 * function of (seed, g, i) (a counter-based generator: independent of the launch and of how many vectors a call asks for).       */
int tbk_kpm_vectors(tbk_sparse* sp, uint64_t seed, int64_t first, int64_t count, double* out);
/* mu[nk][nvec][n_moments] = <v|T_m(H~(k))|v> / <v|v>, H~ = (H - b) / a with a = (emax - emin) / 2, b = (emax + emin) / 2, by the
 * recursion alpha_m+1 = 2 H~ alpha_m - alpha_m-1 and the identities mu_2m = 2 <alpha_m|alpha_m> - mu_0, mu_2m+1 = 2 <alpha_m+1|alpha_m>
 * - mu_1: n_moments / 2 sparse products per block of 8 vectors.  k[nk][dim_k] (dim_k = 0: ignored, nk = 1).  Start vectors:
 * vectors[nvec][nsta] c128, or the unit vectors at states[nvec], or (both null) the random-phase vectors number q nvec + v of `seed`
 * for the k-point with index q.  TBK_EINVAL, naming the bounds, when a moment is not finite or exceeds 1 + 1e-6 in modulus: (emin,
 * emax) does not contain the spectrum.  Fixed-order sums, no atomics on floating-point data: bit-reproducible.                  */
int tbk_kpm_moments(tbk_sparse* sp, const double* k, int64_t nk, int n_moments, double emin, double emax, int nvec,
                    const double* vectors, const int32_t* states, uint64_t seed, double* mu);
/* ---- kernel polynomial method: double moments of the Kubo-Bastin conductivity ------------------------
 * No reference counterpart.  V^a = dH/dk_a in reduced coordinates, a periodic axis in [0, dim_k): the matrix of tbk_gen_dham, with the
 * sparsity of H -- the entry of H times 2 pi i (R + orb_col - orb_row)_a.
 * mu[nk][nvec][n_moments][n_moments] c128, mu_mn = <v| V^a T_m(H~(k)) V^b T_n(H~(k)) |v> / <v|v>, a = dir_a, b = dir_b (equal
 * allowed), H~ and the start vectors as in tbk_kpm_moments (random-phase vectors number q nvec + v for the k-point with index q).
 * 3 n_moments sparse products per block of 8 vectors and a device workspace of n_moments nsta 8 x 16 bytes for the vectors
 * T_n(H~) v (TBK_ENOMEM, naming the byte count, when it cannot be had).  TBK_EINVAL for dim_k = 0, for a direction outside
 * [0, dim_k) and, naming the bounds, when a moment is not finite or exceeds (1 + 1e-6) ||V^a|| ||V^b|| in modulus, the norms bounded
 * by the largest row sum of |V|.  Fixed-order sums, no atomics on floating-point data: bit-reproducible.
 * tbk_sparse_velocity_bounds_host: host only (no device call); vbound[4] = those row-sum bounds of the tables' operator per axis
 * (zero from dim_k on).                                                                                                        */
int tbk_kpm_double_moments(tbk_sparse* sp, const double* k, int64_t nk, int n_moments, double emin, double emax, int dir_a, int dir_b,
                           int nvec, const double* vectors, const int32_t* states, uint64_t seed, double* mu);
int tbk_sparse_velocity_bounds_host(int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                                    const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                                    double* vbound);
/* ---- kernel polynomial method: operator functions and the local Chern marker ------------------------
 * out[nk][nset][nvec][nsta] c128, out_s = sum_{m < ncoef} coeffs[s][m] T_m(H~(k)) v, coeffs[nset][ncoef] c128: a function of H applied
 * to vectors (Chebyshev coefficients of a step: the Fermi projector; (2 - delta_m0) (-i)^m J_m(a t) e^{-i b t}: e^{-i H t}).  H~, the
 * bounds, the start vectors and the random-vector numbering exactly as in tbk_kpm_moments; the result is not divided by <v|v>.
 * ncoef - 1 sparse products per block of 8 vectors, every set accumulated in the same pass.  TBK_EINVAL, naming the bounds, when a
 * norm <T_j v|T_j v> is not finite or exceeds (1 + 1e-6) <v|v>: (emin, emax) does not contain the spectrum.  TBK_ENOMEM, naming the
 * byte count, when the device workspace (2 + nset vectors of nsta x 8 x 16 bytes, the values at k, the output) cannot be had.
 * Fixed-order sums, no atomics on floating-point data: bit-reproducible.
 * tbk_kpm_marker: out[nvec] c128, out_v = <s_v| F A F B F |s_v>, F = sum_m coeffs[m] T_m(H~) with REAL coeffs[ncoef] (F Hermitian),
 * A = diag(da[nsta]), B = diag(db[nsta]), s_v the unit vector at states[v]; dim_k must be 0 (TBK_EINVAL).  With the coefficients of
 * the Fermi projector and da, db two position coordinates, 4 pi Im out_v is the local Chern marker (Bianco, Resta, Phys. Rev. B 84,
 * 241106).  2 (ncoef - 1) sparse products per block of 8 states; no vector leaves the device.  Guard and errors as above.        */
int tbk_kpm_apply_series(tbk_sparse* sp, const double* k, int64_t nk, int ncoef, int nset, const double* coeffs, double emin,
                         double emax, int nvec, const double* vectors, const int32_t* states, uint64_t seed, double* out);
int tbk_kpm_marker(tbk_sparse* sp, int ncoef, const double* coeffs, double emin, double emax, const double* da, const double* db,
                   int nvec, const int32_t* states, double* out);
/* ---- kernel polynomial method: eigenpairs in an energy window ------------------------------------------
 * All eigenpairs of the sparse H(k) with e_lo <= E <= e_hi, for any number of states, by Chebyshev-filtered subspace iteration: the
 * n_search random-phase vectors number 0 .. n_search - 1 of `seed` (scaled by 1 / sqrt(nsta)) are filtered with the Jackson-damped
 * series of degree `degree` of the indicator of [e_lo - delta, e_hi + delta], delta = 2 pi a / degree, orthonormalised through their
 * Gram matrix (directions at or below 1e-12 of its largest eigenvalue are dropped), and rotated to Ritz vectors; a Ritz pair counts
 * when the norm tau of its filtered vector is >= 1/2 (a mixture of states on both sides of the window has a smaller one).  The call
 * returns when every counting pair inside the window has |H x - theta x| <= tol a AND fewer pairs count than the subspace has
 * directions; at least two filter applications are made.  k: dim_k doubles (dim_k = 0: ignored); H~, a and the bounds as in
 * tbk_kpm_moments.  n_search: a multiple of 8 in [8, min(nsta rounded down to 8, 2048)]; it must exceed the number of states in
 * the widened window.  Results: *n_found = m, eval[m] ascending, evec[m][nsta] c128 orthonormal, resid[m] (nullable); the arrays
 * have room for n_search entries.  info[4]: filter applications made, directions kept in the last orthonormalisation, pairs with
 * tau >= 1/2, pairs returned.  m = 0 is a valid answer.
 * TBK_EINVAL: an empty window (e_lo > e_hi) or one not inside (emin, emax), a bad n_search, degree (2 .. 65536), tol or max_iter
 * (< 2); bounds that do not contain the spectrum (the message of tbk_kpm_apply_series).  TBK_ENOCONV, nothing returned: the
 * subspace is saturated -- as many pairs count as it has directions, states may be missing; the message says "raise n_search" and
 * names the count -- or, after max_iter filter applications, a counting pair inside the window misses tol (the message names the
 * worst residual).  TBK_ENOMEM, naming the byte count, when the device workspace (3 n_search nsta 16 bytes for X, Y, H Y, the two
 * vectors of a series, the Gram sums and three n_search^2 matrices) cannot be had.  (degree + 2) n_search / 8 sparse products of
 * 8 vectors per filter application.  Fixed-order sums, no atomics on floating-point data: bit-reproducible.                      */
int tbk_kpm_eigs(tbk_sparse* sp, const double* k, double e_lo, double e_hi, double emin, double emax, int n_search, int degree,
                 double tol, int max_iter, uint64_t seed, int* n_found, double* eval, double* evec, double* resid, int32_t* info);

/* ---- bare (Lindhard) susceptibility at finite momentum transfer ----------
 * k and q reduced, E_n(k), u_n(k) the eigenpairs of the solver (the convention-II matrix of tbk_gen_ham: u is the cell-periodic part),
 * f as in tbk_optical_cond_mesh, M_nm(k, q) = sum_j conj(u_n(k)[j]) u_m(k+q)[j] = <psi_nk| e^{-i q.r} |psi_m,k+q> with r at the orbital
 * positions; the mean over k_uniform_mesh(mesh) (dim_k 1..3, N_k points), all n^2 ordered pairs (n = m included), no spin factor:
 *   omega given (nomega 1..65536 finite frequencies in any order, eta > 0; nq nomega <= 2^22): out[nq][nomega] c128,
 *     chi0(q, w) = -(1 / N_k) sum_k sum_{n,m} [f(E_n(k)) - f(E_m(k+q))] |M_nm|^2 / (w + i eta + E_n(k) - E_m(k+q))
 *   omega NULL (nomega = 0, eta = 0): the exact static limit, out[nq] doubles,
 *     chi0(q) = (1 / N_k) sum_k sum_{n,m} L_nm |M_nm|^2,  L = -(f_n - f_m) / (E_n - E_m) (kT = 0: 0 where f_n = f_m; kT > 0:
 *     (sinh h / h) / (2 kT (cosh h + cosh u)), h = (E_m - E_n) / 2kT, u = ((E_n + E_m) / 2 - mu) / kT, which is -f'(E) at h = 0).
 * q[nq][dim_k]: 1..65536 finite points, any real values (k + q goes through the list solver as it is).  flags: 0 replaces |M|^2 by 1
 * (the band-only Lindhard function; eigenvalue-only solves).  Per unit cell and per energy.  The chunks, groups and tiles do not
 * depend on the q list and nothing uses atomics: bit-reproducible, and a q gives the same bits alone and inside a longer list. */
#define TBK_CHI_MATRIX_ELEMENTS 1
int tbk_susceptibility_mesh(tbk_model* model, const int32_t* mesh, int nq, const double* q, int nomega, const double* omega_or_null,
                            double eta, double mu, double kT, int flags, double* out);

/* ---- the orbital-resolved susceptibility matrix and its RPA ----------
 * Every convention of tbk_susceptibility_mesh.  a, b run over nsel = 1..16 distinct STATE indices sel[] in [0, nsta) (components of the
 * eigenvector; a spinful model has 2 norb of them), in the order given; A^{nm}_a(k, q) = conj(u_n(k)[a]) u_m(k+q)[a]:
 *   omega given: chi0[nq][nomega][nsel][nsel] c128,
 *     chi0_ab(q, w) = -(1 / N_k) sum_k sum_{n,m} [f(E_n(k)) - f(E_m(k+q))] A_a conj(A_b) / (w + i eta + E_n(k) - E_m(k+q))
 *   omega NULL (nomega = 0, eta = 0): chi0[nq][nsel][nsel] c128 (Hermitian, positive semidefinite, not real in general),
 *     chi0_ab(q) = (1 / N_k) sum_k sum_{n,m} L_nm A_a conj(A_b)
 * The sum over a, b of ALL states is the scalar chi0 of tbk_susceptibility_mesh with TBK_CHI_MATRIX_ELEMENTS.
 * nq max(nomega, 1) nsel^2 <= 2^22.  v NULL (nvq = 0, chi_rpa and det NULL): chi0 alone.  v[nvq][nsel][nsel] c128, finite, nvq = 1 (one
 * interaction) or nq (a V(q)), not necessarily Hermitian: chi_rpa, shaped like chi0, is chi = (1 - chi0 V)^-1 chi0 per (q, w), by LU with
 * partial pivoting on the device, and det_or_null[nq][max(nomega, 1)] c128 is det(1 - chi0 V), the signed product of the pivots.  A pivot
 * that is exactly 0 is no error: that matrix of chi_rpa is NaN and its det is 0.  The chunks, groups, tiles and blocks do not depend on
 * the q list and nothing uses atomics: bit-reproducible, a q gives the same bits alone and inside a longer list, and chi0 has the same
 * bits with and without an interaction.                                                                                        */
int tbk_susceptibility_matrix_mesh(tbk_model* model, const int32_t* mesh, int nq, const double* q, int nomega, const double* omega_or_null,
                                   double eta, double mu, double kT, int nsel, const int32_t* sel, const double* v_or_null, int nvq,
                                   double* chi0, double* chi_rpa_or_null, double* det_or_null);

/* ---- the occupied states on k meshes: thermodynamic sums, the Fermi level of a filling, the density matrix ----
 * E_n(k), u_n(k) the eigenpairs of the solver (the convention-II matrix of tbk_gen_ham) on k_uniform_mesh(mesh) (dim_k 1..3, N_k < 2^31
 * points), f = [E <= mu] (kT = 0) or 1 / (1 + exp((E - mu) / kT)); a state counts once (no spin factor: a spinful model has 2 norb).
 * Fixed-order sums, no floating-point atomics, no partition that depends on the number of levels, fillings or lattice vectors:
 * bit-reproducible, and a level, a filling or an R gives the same bits alone and inside a longer list.
 *
 * tbk_thermodynamics_mesh: out[3][nmu] for nmu = 1..8192 finite levels in any order,
 *   N = (1 / N_k) sum f,   E = (1 / N_k) sum f E_n,   S = -(1 / N_k) sum [f ln f + (1 - f) ln(1 - f)]  (exactly 0 at kT = 0).
 *   Eigenvalues only; those of the whole mesh stay on the device.  At kT = 0, N is an integer count divided by N_k.
 *
 * tbk_fermi_level_mesh: mu_out[nfill] for nfill = 1..64 electron counts per cell; ONE eigen-solve of the mesh, then 64 bisection steps
 *   on the ordered integer key of a double, for all fillings at once, without a host synchronisation between them.
 *   kT = 0: c = n_electrons N_k must lie within 1e-6 of an integer in [1, nsta N_k - 1]; with the levels of the mesh sorted,
 *     mu = (e_{c-1} + e_c) / 2 and edges_or_null[nfill][2] = (e_{c-1}, e_c), the device's own eigenvalues.  Equal edges: the level cuts
 *     a degenerate group, and tbk_thermodynamics_mesh at that mu counts more than c.
 *   kT > 0: 0 < n_electrons < nsta; mu is the first double at which the device's occupation sum reaches n_electrons N_k
 *     (edges_or_null must be NULL).  Inside a gap at kT << gap, mu is only as determined as N(mu) is.
 *
 * tbk_density_matrix_mesh: out[nR][nsta][nsta] c128,
 *   D_ij(R) = (1 / N_k) sum_k [sum_n f_n u_n[i] conj(u_n[j])] e^{-2 pi i k.(R + tau_j - tau_i)} = <c+_{j,R} c_{i,0}>
 *   in the index layout and phase convention of the hopping table (amp, i, j, R): D_ii(0) is the occupation of state i,
 *   D_ji(-R) = conj D_ij(R), and E = Re sum conj(t_ij(R)) D_ij(R) over the whole table (both directions of every hop, on-site terms at
 *   R = 0).  R[nR][dim_k]: 1..4096 integer vectors, |R_a| < 2^30, nR nsta^2 <= 2^22.  The phase e^{-2 pi i k.R} is formed from the
 *   exact integer (i_a R_a mod N_a): an R equal to a mesh period gives D(0) bit for bit.  nsta <= 32: one kernel with the
 *   eigenvectors of a group of points in LDS; beyond: 16 x 16 tiles, plain VALU.                                                       */
int tbk_thermodynamics_mesh(tbk_model* model, const int32_t* mesh, int nmu, const double* mu, double kT, double* out);
int tbk_fermi_level_mesh(tbk_model* model, const int32_t* mesh, int nfill, const double* n_electrons, double kT, double* mu_out,
                         double* edges_or_null);
int tbk_density_matrix_mesh(tbk_model* model, const int32_t* mesh, double mu, double kT, int nR, const int32_t* R, double* out);

/* ---- the linear tetrahedron method on k meshes (no reference counterpart) ----
 * Bloechl, Jepsen, Andersen, PRB 49, 16223.  E_b(k) is the solver's b-th eigenvalue at every point of k_uniform_mesh(mesh), dim_k 1, 2
 * or 3, N_k < 2^31, periodic.  The cell with origin o is cut along the fixed diagonal o -> o + (1, .., 1) into dim_k! simplices, one per
 * permutation (a, b, c) of the axes, with corners o, o + e_a, o + e_a + e_b, o + e_a + e_b + e_c (this breaks the lattice's point
 * symmetry slightly; an axis of one or two points is allowed).  Inside a simplex each band is interpolated linearly, and
 *   w_i(E): sum_i w_i X_i = int theta(E - e) X over the simplex as a fraction of the zone,   d_i(E) = dw_i / dE
 * in closed form, the level at E occupied (f = [e <= E]); corners sorted by energy, ties by corner slot.  A band that is flat over a
 * simplex adds a step to N and nothing to g.  No spin factor.  Fixed-order sums: bit-reproducible, and an energy gives the same bits
 * alone and inside a longer list.
 *
 * tbk_tetrahedron_dos_mesh: energies[nE], 1..65536 finite values in any order.  dos = g(E) = sum d_i and idos = N(E) = sum w_i,
 *   [nE], or [nsta][nE] per band with per_band != 0 (at most 2^22 doubles each).  sel[nsel], 1..16 distinct state indices, with
 *   pdos_or_null[nsel][nE] (or [nsel][nsta][nE]) = sum d_i(E) |u_b(k_i)[a]|^2 (at most 2^22 doubles), from a second solve with
 *   eigenvectors in chunks; nsel = 0, sel = NULL and pdos_or_null = NULL: none.
 *
 * tbk_tetrahedron_weights_mesh: out[nsta][N_k], the sum of w_i(mu) over the simplices with mesh point k as corner i, so that
 *   sum_{b,k} out X_b(k) is the tetrahedron integral of X; derivative != 0: the sum of d_i(mu).  correction != 0 (dim_k = 3, not with
 *   derivative) adds Bloechl's curvature correction g_T / 40 sum_j (e_j - e_i) per tetrahedron, which leaves the sum over k unchanged.
 *
 * tbk_tetrahedron_fermi_level_mesh: one eigen-solve.  n_electrons within 1e-9 of an integer m in [1, nsta - 1] with
 *   max_k E_{m-1} < min_k E_m gives the middle of that gap; else (0 < n_electrons < nsta) the first double at which the device's own
 *   N(mu) reaches n_electrons, by rounds of up to 256 trial energies per launch on the ordered key of a double.                          */
int tbk_tetrahedron_dos_mesh(tbk_model* model, const int32_t* mesh, int nE, const double* energies, int per_band, int nsel,
                             const int32_t* sel, double* dos, double* idos, double* pdos_or_null);
int tbk_tetrahedron_weights_mesh(tbk_model* model, const int32_t* mesh, double mu, int correction, int derivative, double* out);
int tbk_tetrahedron_fermi_level_mesh(tbk_model* model, const int32_t* mesh, double n_electrons, double* mu_out);

/* ---- the lattice Green's function on k meshes, the T-matrix of a local impurity and the LDOS around it ----
 * E_n(k), u_n(k) the eigenpairs of the solver on k_uniform_mesh(mesh) (dim_k 1..3, N_k < 2^31 points), z = omega + i eta with eta > 0
 * (retarded), omega[nomega]: 1..65536 finite frequencies in any order.  In the index layout and phase convention of
 * tbk_density_matrix_mesh and of the hopping table (amp, i, j, R):
 *   G_ij(R, w) = (1 / N_k) sum_k sum_n u_n[i] conj(u_n[j]) / (z - E_n(k)) e^{-2 pi i k.(R + tau_j - tau_i)} = <i,0| (z - H)^-1 |j,R>
 * which is exactly the resolvent of the torus of the mesh (its block from cell c to cell c + R mod mesh is t(R)); the infinite crystal
 * is approached for eta above the level spacing of the mesh.  Phases from exact integers: an R equal to a mesh period gives the bits of
 * R = 0.  Fixed-order sums, no floating-point atomics, a partition that depends on (mesh, nsta, dim_k) alone: bit-reproducible, and a
 * frequency or an R gives the same bits alone and inside a longer list.  The eigenvectors never leave the device.
 *
 * tbk_green_function_mesh: out[nomega][nR][na][na] c128.  R[nR][dim_k]: 1..4096 integer vectors, |R_a| < 2^30.  sel[nsel]: 1..32
 *   distinct state indices, the block G_{sel a, sel b} at a cost of nsta na^2 per point and frequency; nsel = 0 and sel = NULL: all
 *   states (na = nsta).  nomega nR na^2 <= 2^22 (the message says "split omega or R_list").  nsta <= 32: one kernel with the selected
 *   components of the eigenvectors of a group of points in LDS; beyond: 16 x 16 tiles, plain VALU.
 *
 * tbk_impurity_t_matrix_mesh: a perturbation V on nsite = 1..16 sites (site_state[a], site_R[a][dim_k]), distinct as sites of the torus;
 *   potential[nsite][nsite] c128, finite and Hermitian.  g_ab = G_{i_a i_b}(R_b - R_a), t_out[nomega][nsite][nsite] = V (1 - g V)^-1
 *   and det_or_null[nomega] = det(1 - g V), c128, by an LU with partial pivoting per frequency on the device.  A pivot that is exactly
 *   0 is TBK_EINVAL; the message names the frequency.
 *
 * tbk_impurity_ldos_mesh: ldos0[nomega][na] = -(1 / pi) Im G_{s_a s_a}(0), the bulk LDOS of the probe states sel (nsel = 0, sel = NULL:
 *   all states, nsta <= 32), and dldos[nomega][nR][na] = -(1 / pi) Im sum_{bc} G_{s_a i_b}(R_b - R_r) T_bc G_{i_c s_a}(R_r - R_c), the
 *   change of the LDOS of state s_a in the probe cell R_r.  The G blocks are computed into device scratch for the union of the probe
 *   and site states and for the probe-site differences reduced modulo the mesh and de-duplicated (at most 16384 of them), and
 *   contracted there: nomega nR_int na_int^2 <= 2^23 and nomega nR na <= 2^24 (TBK_EINVAL beyond; split omega or R).              */
int tbk_green_function_mesh(tbk_model* model, const int32_t* mesh, int nomega, const double* omega, double eta, int nR, const int32_t* R,
                            int nsel, const int32_t* sel, double* out);
int tbk_impurity_t_matrix_mesh(tbk_model* model, const int32_t* mesh, int nomega, const double* omega, double eta, int nsite,
                               const int32_t* site_state, const int32_t* site_R, const double* potential, double* t_out,
                               double* det_or_null);
int tbk_impurity_ldos_mesh(tbk_model* model, const int32_t* mesh, int nomega, const double* omega, double eta, int nsite,
                           const int32_t* site_state, const int32_t* site_R, const double* potential, int nR, const int32_t* R, int nsel,
                           const int32_t* sel, double* ldos0, double* dldos);

/* ---- band unfolding: a supercell's eigenstates on the Bloch sums of the primitive cell ----
 * Called on the SUPERCELL model (nsta <= 2048, dim_k 1..3).  k_sc[nk][dim_k] is K = S k, the supercell's reduced k of the same Cartesian
 * vector as the primitive k, solved as given (not reduced modulo 1).  group[nsta]: the group (primitive orbital x spin) state j is an
 * image of, 0..ng-1, or -1 for none (never read into a sum); ng <= 64.  phase_k[nk][dim_k] (the primitive k) and delta[norb][dim_k]
 * (the displacement of every supercell orbital from the nearest lattice image of its ideal site, primitive reduced coordinates) go
 * together: both NULL means delta = 0 and no phase is formed.  inv_nc = 1 / N_c, N_c = |det S|.  With (E_b, u_b) the solver's eigenpairs:
 *   W[b][g](k) = inv_nc | sum_{j in g} e^{2 pi i k.delta_j} u_b[j] |^2        (members in ascending state order, a fixed partition)
 *   A[g](k, w) = sum_b W[b][g](k) (eta / pi) / ((w - E_b)^2 + eta^2)           (bands in index order)
 * per_state != 0: per group (ngo = ng); else the sums over g (ngo = 1).
 *
 * tbk_unfold_bands_list: eval_out[nsta][nk] (as tbk_solve_list) and w_out[nsta][nk][ngo]; nsta nk ngo <= 2^24.
 * tbk_unfold_spectral_list: out[nk][nomega][ngo] for omega[nomega], 1..65536 finite frequencies in any order, eta > 0;
 *   nk nomega ngo <= 2^24 (the message says "split k_list or omega").
 * The tiling is a function of (nsta, ng, nomega, nk) alone (pythtb_amd/csrc/tbk_unfold.h); no floating-point atomics: two calls give
 * the same bits, a frequency the same bits alone and inside a longer list, and a k-point too wherever the solver takes the same route
 * for both list lengths (the kernels here add no dependence on position or neighbours).  The eigenvectors never leave the device.     */
int tbk_unfold_bands_list(tbk_model* model, const double* k_sc, int64_t nk, int ng, const int32_t* group, const double* phase_k,
                          const double* delta, double inv_nc, int per_state, double* eval_out, double* w_out);
int tbk_unfold_spectral_list(tbk_model* model, const double* k_sc, int64_t nk, int ng, const int32_t* group, const double* phase_k,
                             const double* delta, double inv_nc, int nomega, const double* omega, double eta, int per_state, double* out);

/* ---- real-time propagation under a uniform time-dependent field: currents and Floquet propagators ----
 * Velocity gauge: the field is a rigid shift of every k-point, k -> k + kappa(t).  shift[nt + 1][dim_k] is kappa at the times
 * t_j = j dt (reduced coordinates, finite), 1 <= nt <= 65536, dt finite and > 0, dim_k 1..3, nsta <= 2048.  H and d_a H are the
 * convention-II matrices of tbk_gen_ham / tbk_gen_dham; (E, V) are the solver's eigenpairs.  One step j -> j + 1 is the exponential
 * midpoint rule  psi <- V diag(e^{-i E dt}) V^+ psi  with (E, V) of H(k + (kappa_j + kappa_{j+1}) / 2): exactly unitary, second order in
 * dt, independent of the solver's basis inside a degenerate group.
 *
 * tbk_propagate_mesh: on k_uniform_mesh(mesh), N_k < 2^31.  The carried states start as the eigenvectors of H(k + kappa_0): the bands
 *   occ[nocc] (distinct, weight f = 1), or -- occ_or_null = NULL, nocc = 0 -- every band with the Fermi weight f_n of (mu, kT), the
 *   conventions of tbk_thermodynamics_mesh (no spin factor, f = [E <= mu] at kT = 0); a state whose weight is exactly 0 is skipped.
 *   At every t_j, j = 0 included, with rho(k) = sum_n f_n psi_n psi_n^+:
 *     current[j][a] = (1 / N_k) sum_k tr d_a H(k + kappa_j) rho(k),     energy[j] = (1 / N_k) sum_k tr H(k + kappa_j) rho(k).
 *   kpop_or_null[nsta][N_k] = p_n(k) = sum_m f_m |<u_n(k + kappa_nt)|psi_m>|^2 and pop_or_null[nsta] = its mesh mean, from one more
 *   solve at the last time; inside a group of degenerate levels only the group's sum is defined (the solver chooses the basis).
 *   The carried states -- N_k nprop nsta c128, nprop = nocc or nsta -- stay on the device for the whole call: at most 2^26 c128
 *   (1 GiB); beyond, TBK_EINVAL whose message says "coarsen the mesh or select fewer bands".
 *
 * tbk_propagator_list: the same steps on the list k[nk][dim_k], started from the identity, no weights:
 *   u_out[k][i][j] = <i| prod_j exp(-i H(k + kappa_mid,j) dt) |j>, c128 (later steps to the left); nk nsta^2 <= 2^26.
 *
 * nsta <= 32: one step kernel with the eigenvectors, phases and carried states of a group of points in LDS; beyond: 16 x 16 tiles, plain
 * VALU.  Fixed-order sums, no floating-point atomics, a partition that depends on (mesh or nk, nsta, dim_k, nprop) alone and not on
 * nt: two calls give the same bits, and nt' < nt steps on the leading nt' + 1 shifts give the bits of the first nt' + 1 entries.        */
int tbk_propagate_mesh(tbk_model* model, const int32_t* mesh, int nt, const double* shift, double dt, int nocc,
                       const int32_t* occ_or_null, double mu, double kT, double* current, double* energy, double* pop_or_null,
                       double* kpop_or_null);
int tbk_propagator_list(tbk_model* model, const double* k, int64_t nk, int nt, const double* shift, double dt, double* u_out);

/* ---- self-consistent Hartree-Fock on a k mesh ----
 * H_int = 1/2 sum_{a,b,R} V_ab(R) n_{a,0} n_{b,R} over STATE indices (orbital * nspin + spin), decoupled with D_ij(R) = <c+_{j,R} c_{i,0}>
 * of tbk_density_matrix_mesh: the on-site energy of a gets sum V_ab(R) n_b (Hartree) and, with fock != 0, the entry (a, b, R) of the
 * hopping table gets -V_ab(R) D_ab(R) and its mirror the conjugate.  The bare model comes as the tables of tbk_model_upload: the
 * driver uploads a private copy with every field entry pinned and frees it at the end.
 *   interaction  nint >= 1 entries: int_ab[nint][2], int_R[nint][dim_k], int_V[nint]; an entry is the bond AND its mirror (b, a, -R),
 *                given once; (a, a, R = 0) is refused.  The lattice vectors of the result: R = 0, then the entries' in order of first
 *                appearance, nR <= 4096, nR nsta^2 <= 2^22.
 *   parameters   x[np]: the occupations of the states some V touches (ascending state), then with fock Re, Im of D_ab(R) of every
 *                entry in list order; np <= 2^20.
 *   filling      have_nel != 0: nel_or_mu electrons per cell (the rules of tbk_fermi_level_mesh); else the Fermi level itself.
 *   start        start_mode 0: the field of the bare model at the same filling; 1: x_start[np].
 *   mixing       0 < mixing <= 1; history 0 linear, 1..8 Anderson over that many pairs after as many linear steps; tol >= 0 on
 *                max |x_out - x_in| (0: exactly max_iter iterations); 1 <= max_iter <= 65536; the host reads the residual every
 *                check_every >= 1 iterations (one 8-byte copy) and nothing else until the end.
 * Out: x_in[np] the field the last iteration solved in, x_out[np] the field it produced, mu_out[1], dens[nR][nsta][nsta] c128 = D of the
 * last iteration, R_out[nR][dim_k], energies[5] = {E, S, E - kT S, band energy, N} per cell, res_hist[max_iter] and
 * occ_hist[max_iter][nsta] (the first `iterations` rows are written), info[5] = {iterations, converged, nR, np, resident form}.
 * Fixed-order sums, no floating-point atomics: two calls give the same bits, and max_iter = k gives the first k rows of a longer run. */
int tbk_mean_field_mesh(tbk_ctx* ctx, int dim_k, int norb, int nspin, const double* orb, const double* onsite, int64_t nhop,
                        const int32_t* hop_i, const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp,
                        const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R, const double* int_V, int fock,
                        int have_nel, double nel_or_mu, double kT, int start_mode, const double* x_start, double mixing,
                        int history, double tol, int max_iter, int check_every, double* x_in, double* x_out, double* mu_out,
                        double* dens, int32_t* R_out, double* energies, double* res_hist, double* occ_hist, int32_t* info);

/* ---- selected entries of the density matrix, and self-consistent Bogoliubov-de Gennes superconductivity ----
 * tbk_density_matrix_pairs_mesh: out[nt] c128 = D_{i_p j_p}(R_p) of tbk_density_matrix_mesh -- the same definition, phase, occupation
 *   rule and chunks -- for nt = 1..2^20 triples ij[nt][2] (state indices), R[nt][dim_k] (|R_a| < 2^30), without forming any matrix:
 *   what a self-consistency loop consumes.  The partition depends on (mesh, nsta, dim_k) alone, not on the list: two calls give the
 *   same bits, and a triple gives the same bits alone and inside any list.
 *
 * tbk_bdg_mesh: H_int of tbk_mean_field_mesh, decoupled in the Hartree, Fock and pairing channels (each on or off) on the NAMBU model
 *   of N = 2 nsta states, Psi = (c, c+): particle state a, hole state nsta + a at the same position, hole block -conj of the particle
 *   block, Fermi level 0.  With D its density matrix: n_a = D_aa(0), <c+_{b,R} c_{a,0}> = D_ab(R), F_ab(R) = <c_{b,R} c_{a,0}> =
 *   D_{a,nsta+b}(R); the pairing field of an entry (V, a, b, R) is Delta = V F_ab(R) on the hop (a -> nsta + b, R) and -Delta on
 *   (b -> nsta + a, -R).  The tables (orb[N][dim_k], onsite[N] c128, hops over N spinless orbitals) are those of the bare Nambu model
 *   without pairing: at Fermi level 0 with have_nel != 0, else at the given Fermi level nel_or_mu.
 *   parameters   x[np]: the occupations of the states some V touches (ascending), with fock Re, Im of D_ab(R) per entry, with pairing
 *                Re, Im of F_ab(R) per entry, with have_nel != 0 mu last; np <= 2^20.  x_start[np] is the first x_in.
 *   filling      have_nel != 0: any 0 < nel_or_mu < nsta, and x_out[mu] = x_in[mu] + mu_step (n_electrons - N_out), mu_step > 0.
 *   loop         mixing, history, tol, max_iter, check_every as in tbk_mean_field_mesh; nsta <= 1024, at most 4096 lattice vectors.
 * Out: x_in[np], x_out[np] of the last iteration; energies[7] = {E = <H - mu N> + mu N, S, F = E - kT S, F - mu N, N_out, mu_in,
 * min |E_n(k)| over the mesh} per cell; res_hist[max_iter], occ_hist[max_iter][nsta] (the first `iterations` rows are written);
 * info[5] = {iterations, converged, nR, np, triples}.  Fixed-order sums, no floating-point atomics: two calls give the same bits, and
 * max_iter = k gives the first k rows of a longer run.                                                                             */
int tbk_density_matrix_pairs_mesh(tbk_model* model, const int32_t* mesh, double mu, double kT, int64_t nt, const int32_t* ij,
                                  const int32_t* R, double* out);
int tbk_bdg_mesh(tbk_ctx* ctx, int dim_k, int nsta, const double* orb, const double* onsite, int64_t nhop, const int32_t* hop_i,
                 const int32_t* hop_j, const int32_t* hop_R, const double* hop_amp, const int32_t* mesh, int nint,
                 const int32_t* int_ab, const int32_t* int_R, const double* int_V, int hartree, int fock, int pairing,
                 int have_nel, double nel_or_mu, double kT, const double* x_start, double mu_step, double mixing, int history,
                 double tol, int max_iter, int check_every, double* x_in, double* x_out, double* energies, double* res_hist,
                 double* occ_hist, int32_t* info);

/* ---- excitons: the Tamm-Dancoff Bethe-Salpeter operator, its dense states and its Haydock spectrum ----
 * The bands are the model's own (for time-dependent Hartree-Fock: the model a converged tbk_mean_field_mesh produced), an insulator
 * at kT = 0: the same number n_occ of levels at or below mu at every mesh point.  The interaction is the list of
 * tbk_mean_field_mesh (a bond given once, state indices); E holds both directions of every bond, d_e = R + tau_b - tau_a.
 * Transitions t = (k, v, c) over the mesh and the selected bands, X[k][v][c], Delta_t = E_c(k) - E_v(k):
 *   H_ex = Delta + K^x - K^d,   (H_ex X)_vc(k) = Delta X_vc(k) + sum_a h_a conj(u_c[a]) u_v[a]
 *                                                - sum_e V_e F_e e^{2 pi i k.d_e} conj(u_c[a]) u_v[b]
 *   with T(k) = sum_vc X_vc(k) u_ck u_vk^+, F_e = (1/N) sum_k e^{-2 pi i k.d_e} T_ab(k), rho_b = (1/N) sum_k T_bb(k) and
 *   h_a = sum_{e: a_e = a} V_e rho_{b_e}; `direct` = 0 drops K^d, `exchange` = 0 drops K^x.
 *   bands        vsel / csel: nv / nc band indices (occupied / empty, 1..16 each); or null: the top nv occupied and the bottom nc
 *                empty bands, 0 meaning all of them.  info[3] = {n_occ, nv, nc} as resolved.
 *   dipoles      D^a_t = <u_c| dH/dk_a |u_v> / Delta_t (reduced k), S_ab = (1/N) <D^a|D^b>
 * tbk_exciton_apply_mesh: out[nb][N_t] c128 = H_ex applied to vectors[nb][N_t] (nb = 1..16, of xnv x xnc bands per point, which must
 *   be the selection's), gaps[N_t] = Delta_t; N_t <= 2^24 and N_k nsta (nv + nc) <= 2^26.
 * tbk_exciton_states_mesh: N_t <= 2048 <= cap.  H_ex is formed by applying the operator to unit vectors in blocks of 16 and solved
 *   by the dense solver: energies[N_t] ascending, dipoles[N_t][dim_k] c128 = <A^lambda|D^a>, sab[dim_k][dim_k] c128 = S_ab,
 *   vectors[N_t][N_t] c128 (or null), scal[2] = {smallest, largest Delta_t}.
 * tbk_exciton_spectrum_mesh: the Lanczos runs of a polarizability -- the full tensor (da = db = -1): one run from every D^a, then for
 *   every pair a < b one from D^a + D^b and one from D^a + i D^b, dim_k^2 runs; one component: da == db one run, else D^da, D^db,
 *   D^da + D^db, D^da + i D^db -- carried as one block through the same applications with alpha, beta, the three-term update and the
 *   breakdown rule on the device: alpha[nrun][nsteps], beta[nrun][nsteps], norm2[nrun] = |start|^2, n_used[nrun] (a run whose beta
 *   falls below 1e-10 max(largest |alpha| so far, largest Delta_t) ends there), sab, scal as above.
 * tbk_exciton_reconstruct (host only): chi_ab(omega_w) = (1/N) <D^a| (H_ex - omega_w - i eta)^-1 |D^b> from those coefficients by
 *   continued fractions: out[nw][dim_k][dim_k] c128 (da < 0) or out[nw].
 * Fixed-order sums, no floating-point atomics, partitions that depend on (mesh, nv, nc) alone: two calls give the same bits, a vector
 * gives the same bits alone and inside any block, and nsteps = k gives the first k coefficients of a longer run.                  */
int tbk_exciton_apply_mesh(tbk_model* model, const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R,
                           const double* int_V, double mu, int nv, const int32_t* vsel, int nc, const int32_t* csel, int direct,
                           int exchange, int nb, int xnv, int xnc, const double* vectors, double* out, double* gaps, int32_t* info);
int tbk_exciton_states_mesh(tbk_model* model, const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R,
                            const double* int_V, double mu, int nv, const int32_t* vsel, int nc, const int32_t* csel, int direct,
                            int exchange, int64_t cap, double* energies, double* dipoles, double* sab, double* vectors, double* scal,
                            int32_t* info);
int tbk_exciton_spectrum_mesh(tbk_model* model, const int32_t* mesh, int nint, const int32_t* int_ab, const int32_t* int_R,
                              const double* int_V, double mu, int nv, const int32_t* vsel, int nc, const int32_t* csel, int direct,
                              int exchange, int da, int db, int nsteps, double* alpha, double* beta, double* norm2, int32_t* n_used,
                              double* sab, double* scal, int32_t* info);
int tbk_exciton_reconstruct(int dim_k, int da, int db, int nsteps, const double* alpha, const double* beta, const double* norm2,
                            const int32_t* n_used, int64_t npts, int nw, const double* omega, double eta, double* out);

/* ---- projected and maximally localised Wannier functions on a k mesh ----
 * nw <= 16 functions from the nb <= 32 bands `bands` (distinct, the same at every k) of k_uniform_mesh(mesh), dim_k 1..3, every
 * N_a >= 3, nsta <= 2048, N_k nsta nw <= 2^26 (the rotated states stay on the device).
 *   trial       function w is the sum of its terms term_ptr[w] .. term_ptr[w + 1]: amplitude term_amp[t] (c128) on state term_state[t]
 *               of cell term_R[t][dim_k]; g~_w(k)[j] = sum amp e^{-2 pi i k.(R + tau_j)}, A(k) = V_bands(k)+ g~(k), U = A (A+ A)^-1/2.
 *               TBK_EINVAL "trial functions are singular on the bands at k = ..." when the smallest singular value of A over the mesh
 *               is below 1e-8.
 *   b-vectors   nbv <= 6 steps bstep[nbv][dim_k] in {-1, 0, 1} (b = sum_a step_a beta_a / N_a; -b is implied), weights bw[nbv] > 0 with
 *               2 sum_b w_b b b^T = 1, bgram[nbv][nbv] = b.b' in Cartesian coordinates.
 *   descent     max_iter >= 0 steps of Marzari-Vanderbilt steepest descent at alpha = 1 (0: the projection alone); the host reads the
 *               change of Omega every check_every iterations (one 8-byte copy) and stops when its modulus is below tol > 0.
 *   model       t_mn(R) = (1 / N_k) sum_k e^{-2 pi i k.R} [U_tot+ E U_tot]_mn for the nR vectors R[nR][dim_k] (r_user != 0: a list of the
 *               caller's, nR <= 4096; else at most the N_k vectors of the torus), in the index layout of the hopping table (amp, i, j, R).
 * Out: hop[nR][nw][nw] c128; sums[21 + 16 * 6] = {Omega_I, Omega_OD, Omega_D, Omega, the nw spreads} from [0], the smallest singular
 * value at [20], sum_k Im ln M_nn(k, b) as [nw][nbv] from [21] (r_n = -(2 / N_k) sum_b w_b b of it); hist[max_iter + 1]: Omega of the
 * projection and after every iteration (the first iterations + 1 entries are written); functions_or_null[nR][nsta][nw] c128:
 * w_n(R, j) = (1 / N_k) sum_k e^{2 pi i k.(R + tau_j)} u~_n(k)[j]; gauge_or_null[N_k][nb][nw] c128: U_tot; info[5] = {iterations, converged,
 * points per workgroup of the rotation, items per workgroup of the overlaps, k-groups of the spread sums}.
 * Fixed-order sums, no atomics, a partition that depends on (mesh, nsta, nb, nw, nbv) alone: two calls give the same bits, and
 * max_iter = m gives the first m + 1 entries of the history of a longer run.                                                        */
int tbk_wannier_mesh(tbk_model* model, const int32_t* mesh, int nb, const int32_t* bands, int nw, int64_t nterm,
                     const int32_t* term_ptr, const int32_t* term_state, const int32_t* term_R, const double* term_amp, int nbv,
                     const int32_t* bstep, const double* bw, const double* bgram, int max_iter, double tol, int check_every, int nR,
                     int r_user, const int32_t* R, double* hop, double* sums, double* hist, double* functions_or_null,
                     double* gauge_or_null, int32_t* info);

/* ---- disentangled Wannier functions with energy windows on a k mesh ----
 * tbk_wannier_mesh's arguments mean what they mean there; `bands` is the outermost candidate set, and the subspace of nw functions
 * is chosen inside it after Souza, Marzari and Vanderbilt (PRB 65, 035109).  Beyond tbk_wannier_mesh's caps: the candidate states
 * stay on the device, N_k nsta nb <= 2^26, and so do their overlaps, N_k nbv nb^2 <= 2^26.
 *   window_or_null   (lo, hi): of the candidate bands only those with lo <= E_n(k) <= hi take part at k (null: all of them);
 *                    TBK_EINVAL "... at k = ..." where fewer than nw do
 *   frozen_or_null   (lo, hi): window bands inside it are kept in the subspace whole; TBK_EINVAL "... at k = ..." where more than nw are
 *   dis_iter         0..65536 iterations (0: the projected subspace with the frozen states forced in); Z_in = dis_mixing Z_out +
 *                    (1 - dis_mixing) Z_in, 0 < dis_mixing <= 1; the host reads the change of Omega_I every check_every iterations
 *                    (one 8-byte copy) and stops when its modulus is below dis_tol > 0
 * then the gauge U0 = U_dis A' (A'+ A')^-1/2 with A' = U_dis+ A (TBK_EINVAL "trial functions are singular ..." when the smallest
 * singular value of A' over the mesh is below 1e-8) and tbk_wannier_mesh's spread, descent, model and functions.
 * Out beyond tbk_wannier_mesh's (sums[20]: the smallest singular value of A'): dis_sums[2] = {the smallest singular value of the
 * nb x nw projection over the mesh, the smallest gap over the mesh between the last selected and the first rejected eigenvalue of Z at
 * the last iteration, infinity where nothing is rejected}; dis_hist[dis_iter + 1]: Omega_I of the starting subspace and after every
 * iteration; n_window[N_k], n_frozen[N_k]; gauge_or_null[N_k][nb][nw]: U_tot, zero rows for bands outside the window;
 * info[5] = {iterations, converged, dis_iterations, dis_converged, k-groups of the sums}.
 * Fixed-order sums, no atomics, a partition that depends on (mesh, nsta, nb, nw, nbv) alone: two calls give the same bits, dis_iter = m
 * gives the first m + 1 entries of dis_hist of a longer run, and with dis_iter fixed max_iter = m the first m + 1 entries of hist.   */
int tbk_wannier_dis_mesh(tbk_model* model, const int32_t* mesh, int nb, const int32_t* bands, int nw, int64_t nterm,
                         const int32_t* term_ptr, const int32_t* term_state, const int32_t* term_R, const double* term_amp, int nbv,
                         const int32_t* bstep, const double* bw, const double* bgram, const double* window_or_null,
                         const double* frozen_or_null, int dis_iter, double dis_mixing, double dis_tol, int max_iter, double tol,
                         int check_every, int nR, int r_user, const int32_t* R, double* hop, double* sums, double* hist, double* dis_sums,
                         double* dis_hist, int32_t* n_window, int32_t* n_frozen, double* functions_or_null, double* gauge_or_null,
                         int32_t* info);

/* ---- multi-GPU: one process per GPU, k-points sharded, one gather ------
 * Thin RCCL wrappers (librccl is dlopen'ed on first use).  The 128-byte id is
 * created on rank 0 and distributed by the launcher (any out-of-band channel). */
int tbk_comm_unique_id(unsigned char id_out[128]);
int tbk_comm_init(tbk_ctx* ctx, const unsigned char id[128], int nranks, int rank);
int tbk_comm_destroy(tbk_ctx* ctx);
/* all ranks contribute count doubles from send_dev; recv_dev[nranks*count]   */
int tbk_comm_allgather_f64(tbk_ctx* ctx, const double* send_dev, double* recv_dev,
                           int64_t count);

/* uneven contributions (513 Berry strings over 8 ranks; slabs of a 257-plane mesh): rank r contributes
 * counts[r] doubles, received at recv_dev + displs[r] on every rank; counts/displs are HOST arrays of nranks
 * entries and count must equal counts[own rank].  One grouped ncclSend/ncclRecv exchange.                  */
int tbk_comm_allgatherv_f64(tbk_ctx* ctx, const double* send_dev, int64_t count, double* recv_dev,
                            const int64_t* counts, const int64_t* displs);
/* the eigenvalue gather of a sharded solve_all (ret_eval (nsta, nkp) band-major, pythtb.py:1040,1053-1067): rank r
 * holds send_dev[nrows][counts[r]] -- its contiguous chunk of the k list for every band -- and every rank receives
 * recv_dev[nrows][row_stride] with that chunk of row b at b*row_stride + displs[r].  Same single grouped exchange,
 * nrows messages per pair of ranks, so the result lands band-major with no relayout pass (config E: 16 messages of
 * 16.8 MB per pair).                                                                                              */
int tbk_comm_allgatherv_rows_f64(tbk_ctx* ctx, const double* send_dev, int64_t nrows, int64_t count,
                                 double* recv_dev, const int64_t* counts, const int64_t* displs,
                                 int64_t row_stride);
/* the ROOTED form of the same gather (the reference's ret_eval is one array on one caller,
 * pythtb.py:1040,1053-1067): only rank `root` receives recv_dev[nrows][row_stride]; on every other rank recv_dev may
 * be NULL -- those ranks send their rows to the root and allocate nothing of size nrows x row_stride (config E's
 * solve_all leg: 268 MB sent per rank instead of 2.1 GB received by each).  Grouped ncclSend / ncclRecv, at most 32
 * rows per ncclGroup (both rows forms).                                                                            */
int tbk_comm_gatherv_rows_f64(tbk_ctx* ctx, const double* send_dev, int64_t nrows, int64_t count,
                              double* recv_dev, const int64_t* counts, const int64_t* displs,
                              int64_t row_stride, int root);

#ifdef __cplusplus
}
#endif
#endif /* TBK_H */
