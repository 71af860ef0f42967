/*
 * psa_hip.h -- C ABI of libpsa_hip.so: the MI355X (gfx950) implementation of the
 * PSA spectral-energy-density hot path.
 *
 * The reference (h-walk/PSA) is pure Python and has no FFI of its own; the seam
 * this library replaces is the private method
 *
 *     SEDCalculator._calculate_sed_for_group(k_vectors_3d, group_atom_indices, mean_pos_all)
 *         -> (T, K, 3) complex64                     src/psa/core/sed_calculator.py:58-84
 *
 * plus the per-group |.|^2 accumulation of the incoherent branch of
 * SEDCalculator.calculate (sed_calculator.py:313-327).  Every entry point is
 * plain C: opaque context pointer, raw host pointers, sizes; no C++ or torch types.
 * The ctypes stub that binds it is psa_amd/_hip.py; INTEGRATION.md shows the
 * ten-line patch that routes the reference's own SEDCalculator through it.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PSA_E* code on failure;
 *     psa_last_error() returns the text for the calling thread's last failure;
 *   - host arrays are C-contiguous, owned by the caller, only read/written
 *     during the call; device memory, rocFFT plans, streams and RCCL
 *     communicators are owned by the context;
 *   - entry points may be called from any host thread (each one selects the
 *     context's device itself); calls on one context are serialised by an
 *     internal mutex (the reference GUI calls from worker threads,
 *     src/psa/gui/psa_gui.py:1015, :2246).
 */
#ifndef PSA_HIP_H
#define PSA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSA_HIP_ABI_VERSION 6

/* error codes */
#define PSA_OK          0
#define PSA_EINVAL     -1   /* bad argument (shape, NULL, out-of-range index) */
#define PSA_EHIP       -2   /* HIP runtime failure            */
#define PSA_EFFT       -3   /* rocFFT failure                 */
#define PSA_ERCCL      -4   /* RCCL failure                   */
#define PSA_ESTATE     -5   /* call sequence violated (e.g. finalize before project) */
#define PSA_ENOMEM     -6

/* data slots: which resident (T, N, 3) float32 array a projection reads.
 * sed_calculator.py:69-72 projects velocities, or positions minus their mean. */
#define PSA_SLOT_VELOCITIES 0
#define PSA_SLOT_POSITIONS  1
#define PSA_NUM_SLOTS       2

/* flags for psa_sed_project */
#define PSA_F_DISPLACEMENTS  0x1  /* data = slot - mean_pos (sed_calculator.py:70)           */
#define PSA_F_INTENSITY      0x2  /* result = sum_g sum_c |S_g|^2, float32 (T,K)  (:313-327) */
                                  /* default: complex64 (T,K,3) of the (single) group (:296-311) */

/* projection-kernel selector (diagnostics; PSA_K1_AUTO is the product path) */
#define PSA_K1_AUTO   0  /* split-precision (fp32-equivalent) MFMA kernels: "2 x f16" for groups with more
                            than 16 k-vectors -- from the group's cached split planes when it has them
                            (PSA_OPT_PLANES), splitting on the fly otherwise -- "3 x bf16" below that and
                            for arrays holding NaN/Inf; displacement mode projects a materialised
                            positions - mean array the same way */
#define PSA_K1_WAVE   1  /* LDS-staged VALU kernel with wavefront shuffle sums       */
#define PSA_K1_MFMA32 2  /* always the exact-fp32 MFMA tile kernel                   */
#define PSA_K1_SPLIT_BF16 3  /* "3 x bf16" split-precision kernel for every velocity-mode group */

typedef struct psa_ctx psa_ctx;

/* ---- library / context ------------------------------------------------ */
int         psa_abi_version(void);
const char* psa_last_error(void);
int         psa_device_count(int* count);
/* page-locked host memory for result arrays: a D2H copy into it runs at the full PCIe rate and
 * touches no fresh pages (into pageable memory configuration 5's 101 MB result took 4.5 ms of copy
 * plus as much again in page faults).  Independent of any context. */
int         psa_host_alloc(size_t bytes, void** out);
int         psa_host_free(void* p);
int         psa_create(int device, psa_ctx** out);
int         psa_destroy(psa_ctx* ctx);
int         psa_synchronize(psa_ctx* ctx);
int         psa_set_k1(psa_ctx* ctx, int selector);     /* PSA_K1_* */
/* The low-rank k-path route's fold (on in a new context): the product of the node table's lo piece with the hi plane is not
 * multiplied per node row; by the combine's linearity it equals E v_hi with E = phi L W_lo, a table as small as D, and the D
 * image holds D + E rounded once to float16.  Node rows keep two products instead of three (k1_lowrank_fold.hip for lists the
 * pair launch serves, else the two-product node pass and the D pass on the folded image).  Results move within the route's
 * per-element bound; on = 0: the route as it was, bit for bit.  A switch of its own like psa_set_k1, not a row of the option
 * table below. */
int         psa_set_k1_lowrank_fold(psa_ctx* ctx, int on);
/* The folded route's node count, 48 (a new context) or 64.  64 Chebyshev nodes interpolate the line's phases to fp64
 * rounding; 48 leave a residual of at most 4.6e-7, which the folded D image absorbs with everything else the node rows' hi
 * piece does not carry: D' = P_ref w - phi L W_hi, taken in fp64 and rounded once to float16.  Node rows fall from 128 to 96
 * (k1_lowrank_n48.hip for lists the pair launch serves, else the two-product node pass on the 48-node table and the D pass on
 * that image).  Effective only while the fold is on: with the fold off the route has 64 nodes.  Results move within the
 * route's per-element bound; 64: the folded route as it was, bit for bit.  A switch of its own, like the fold. */
int         psa_set_k1_lowrank_nodes(psa_ctx* ctx, int nodes);
/* Tunables of the product path (defaults in brackets):
 *   PSA_OPT_PLANES        [1] keep, per atom group, the group's data scaled, split into its two
 *                             float16 pieces and laid out in MFMA-fragment order ("split planes",
 *                             4 bytes per value like the float32 array, the group's atoms compacted)
 *                             and project from them; 0 = always split on the fly
 *   PSA_OPT_PLANES_BUDGET [0] bytes of HBM the plane cache may hold; 0 = 45 % of the device.  Sets
 *                             are evicted least-recently-used; a group that does not fit is
 *                             projected by the on-the-fly kernels.  The float32 slot is never dropped.
 *   PSA_OPT_PLANES_EAGER  [0] 1 = build an index-list group's planes on its first projection
 *                             (default: on the second with the same list; "all atoms" always first)
 *   PSA_OPT_PLANES_MIN_K  [17] shortest k-list for which a group's planes are BUILT (a shorter list
 *                             uses them when they exist; otherwise the "3 x bf16" kernel on the
 *                             float32 array, which is HBM-bound at the same rate) */
#define PSA_OPT_PLANES         0
#define PSA_OPT_PLANES_BUDGET  1
#define PSA_OPT_PLANES_EAGER   2
#define PSA_OPT_PLANES_MIN_K   3
/*   PSA_OPT_FOLD_PAIRS    [1] when the whole k-list is given to one device, k-vectors whose exact
 *                             negation (or an identical twin) is also in the list are not projected:
 *                             S(-k)[w] = conj S(k)[(T-w) mod T] holds bit for bit in the reference's
 *                             arithmetic (float32 phase argument odd in k, real data), so the partner's
 *                             columns are written by the epilogue from the one projection.  A k-grid
 *                             symmetric about Gamma (examples/k_grid_heatmap_example.py:33-38) costs
 *                             half its projections and FFTs.  0 = project every vector. */
#define PSA_OPT_FOLD_PAIRS     4
/*   PSA_OPT_FFT_PRIME     [1] when a trajectory of T frames becomes resident (psa_data_upload /
 *                             psa_data_alloc) a host thread builds a one-k-vector rocFFT plan of length T,
 *                             so that rocFFT's run-time kernel compilation for that length happens beside
 *                             the upload instead of inside the first calculation.  Independently of this,
 *                             psa_create points ROCFFT_RTC_CACHE_PATH (unless set) at
 *                             $PSA_CACHE_DIR | $XDG_CACHE_HOME/psa_amd | $HOME/.cache/psa_amd so that later
 *                             processes load the compiled kernels instead of compiling them again. */
#define PSA_OPT_FFT_PRIME      5
/*   PSA_OPT_K1_LOADER_WAVES [1] which form of the planes kernel projects 128-row M blocks (more than 32
 *                             k-vectors): 1 = twelve wavefronts per workgroup of which four issue all
 *                             LDS-DMA and eight only multiply (k1_planes_lw.hip), 0 = eight wavefronts
 *                             that both load and multiply (k1_planes.hip; always used for the 64- and
 *                             32-row blocks of shorter lists).  Same arithmetic, same results; the loader
 *                             form measured 2-3 % faster on every shape (round 3). */
#define PSA_OPT_K1_LOADER_WAVES 6
/*   PSA_OPT_K1_WIDE       [1] lists of more than 64 k-vectors are projected in 256-row M blocks
 *                             (k1_planes_wide.hip: eight wavefronts, a ring of 1-KiB units, 28 KiB of LDS-DMA
 *                             per 128 rows and stage instead of 40).  Same arithmetic; the float32 fold
 *                             comes every 10 stages instead of every 8.  0 = the 128-row blocks for them too. */
#define PSA_OPT_K1_WIDE         7
/*   PSA_OPT_K1_LOWRANK    [1] k-lists on one line (k-paths) are projected as 64 node rows of exact phases
 *                             (the 128-row planes kernel), one float16 product of the difference to the
 *                             reference's float32 phases with the hi plane (k1_planes_diff.hip) and a
 *                             combine; planned per group on the host (api_lowrank.hip), else the dense
 *                             kernels.  Environment PSA_K1_LOWRANK=0/1 sets it at context creation.
 *   PSA_OPT_K1_LOWRANK_MIN_K [256] shortest whole k-list (K_total) the route serves.  Environment
 *                             PSA_K1_LOWRANK_MIN_K.
 *   PSA_OPT_K1_LOWRANK_MIN_LOCAL [128] shortest part of such a list one projection launch serves (the
 *                             D pass works in 512-row blocks: a 128-vector part is a half-empty one).
 *                             A list split over calls of one process keeps the route for every part of
 *                             >= 128; psa_amd.dist sets 256 on the ranks of a k-sharded run, where a
 *                             128-vector shard is faster on the dense kernels. */
#define PSA_OPT_K1_LOWRANK      8
#define PSA_OPT_K1_LOWRANK_MIN_K 9
#define PSA_OPT_K1_LOWRANK_MIN_LOCAL 10
/*   PSA_OPT_VDOS_WORK_BYTES [1 GiB] bytes of device memory the work buffer of psa_vdos may take, whatever N and T:
 *                             the call loops over (atom block x segment block).  Must hold 32 atom pairs x 3
 *                             components x one segment: 768 L bytes. */
#define PSA_OPT_VDOS_WORK_BYTES 11
/*   PSA_OPT_MODES_WORK_BYTES [4 GiB] bytes of device memory the stacked spectra of psa_sed_modes may take (and, for
 *                             psa_sed_modes_welch, they and the segment buffer together: at least 24 B (T + L)): the call
 *                             loops over blocks of k-vectors of 24 B T bytes each (B groups x 3 components x T
 *                             complex64).  The default holds 256 k-vectors of 65536 frames and 8 sites in one block.
 *                             Any value >= 1 is accepted; a call whose single k-vector does not fit is PSA_EINVAL.
 *                             The (T,K,M) float32 result on the device is not part of the budget. */
#define PSA_OPT_MODES_WORK_BYTES 12
/*   PSA_OPT_DYNAMIC_WORK_BYTES [4 GiB] bytes of device memory the frame-dependent projections q of psa_dynamic_spectra
 *                             and its segment buffer may take together: the call loops over blocks of k-vectors of
 *                             8 NC T bytes each (NC = 1, with currents 4, series of T complex64).  Any value >= 1 is
 *                             accepted; a call whose single k-vector (and one segment of it) does not fit is PSA_EINVAL.
 *                             The (1 or 3, L, K) float32 result on the device is not part of the budget. */
#define PSA_OPT_DYNAMIC_WORK_BYTES 13
/*   PSA_OPT_K1_LOWRANK_PAIR [1] on the low-rank route (PSA_OPT_K1_LOWRANK), a launch whose D rows fill one 512-row block
 *                             (at most 256 k-vectors) projects node rows and D rows in ONE kernel launch of two balanced
 *                             workgroups per frame tile on one XCD (k1_lowrank_pair.hip) instead of the node pass and
 *                             the D pass.  Same arithmetic, bit-identical results; 0 = always the two passes.  psa_k1_lowrank_pair_launches counts the launches it served. */
#define PSA_OPT_K1_LOWRANK_PAIR 15   /* 14 is not assigned: psa_set_option refuses it as unknown */
int         psa_set_option(psa_ctx* ctx, int option, int64_t value);
/* The table those options live in (api_core.hip), row by row: the option's id, the default a new context starts it at
 * (before psa_create reads the environment) and its name as spelled above; any of the three may be null.  PSA_EINVAL past
 * the last row.  No context, no GPU. */
int         psa_option_info(int index, int32_t* option, int64_t* default_value, const char** name);
/* device name / CU count / HBM bytes of the context's GPU */
int         psa_device_info(psa_ctx* ctx, char* name, int name_len,
                            int* compute_units, int64_t* hbm_bytes);

/* ---- trajectory residency ---------------------------------------------
 * Trajectory.velocities / .positions are (T, N, 3) float32 C-order
 * (src/psa/core/trajectory.py:20-23); they stay in HBM in exactly that layout. */
/* psa_data_upload streams the array through two page-locked staging buffers (filled by a few
 * host threads, drained by hipMemcpyAsync on a copy stream) -- the source may be pageable or a
 * memory-mapped .npy cache (src/psa/io/loader.py:48-79). */
int psa_data_upload(psa_ctx* ctx, int slot, const float* host, int64_t T, int64_t N);
int psa_data_alloc(psa_ctx* ctx, int slot, int64_t T, int64_t N);
int psa_data_download(psa_ctx* ctx, int slot, float* host, int64_t t0, int64_t nt);
int psa_data_release(psa_ctx* ctx, int slot);
int psa_data_shape(psa_ctx* ctx, int slot, int64_t* T, int64_t* N);

/* Fill a slot, already allocated with psa_data_alloc, with the synthetic
 * trajectory of psa_amd/synth.py (bit-identical NumPy twin there):
 *   v[t,a,c] = noise(seed,t,a,c) + sum_m [c==mode_comp[m]] amp[m]*(ct[m,t]*ca[m,a] + st[m,t]*sa[m,a])
 * tables are (n_modes, T) / (n_modes, N) float32, host.  The slot holds frames
 * [t_offset, t_offset + T) of the synthetic trajectory (noise counter and ct/st rows of those
 * frames): a frame-sharded rank generates its own slice. */
int psa_data_fill_synthetic(psa_ctx* ctx, int slot, uint64_t seed, int64_t t_offset, int n_modes,
                            const float* amp, const int32_t* mode_comp,
                            const float* ct, const float* st,
                            const float* ca, const float* sa);

/* mean over frames of a resident slot, float32 sequential-in-t accumulation then /T:
 * bit-identical to np.mean(positions, axis=0, dtype=np.float32) (sed_calculator.py:205). */
int psa_mean_positions(psa_ctx* ctx, int slot, float* mean_host /* (N,3) */);

/* The same mean for an array that stays on the host (velocity mode does not upload positions):
 * columns split over `threads` host threads (0 = up to 16), each a sequential float32 chain over the
 * frames like NumPy's -- bit-identical to np.mean(x, axis=0, dtype=np.float32), one pass at memory
 * bandwidth.  No context, no GPU. */
int psa_host_mean_frames(const float* x /* (T, cols) */, int64_t T, int64_t cols, float* mean_out, int threads);

/* Per-atom weights (mass-weighted or charge-weighted SED): from this call on, every projection on the
 * context -- psa_sed_project, _project_upload, _calculate, _fs_project, _single_bin and the psa_debug_*
 * projections -- computes
 *     q[k,c,t] = sum_a  w[idx[a]] * d[t, idx[a], c] * P[k,a]
 * (the phase still from the unweighted mean positions; FFT, /T, |.|^2, group sums, pair folding and the
 * chiral phase unchanged) until it is cleared with w = NULL.  w: N finite float32 values, copied to the
 * device during the call; a non-finite entry is PSA_EINVAL, and so is a projection whose slot holds a
 * different number of atoms.  The weight enters the phase table, never the data: the resident arrays,
 * their split planes and the plane cache are untouched.  The float16 tables hold w * 2^-e, 2^e the
 * smallest power of two >= max|w|, and the launch multiplies 2^e back exactly.  With no weights set every
 * result is bit for bit what it is without this call. */
int psa_set_atom_weights(psa_ctx* ctx, const float* w /* N, or NULL to clear */, int64_t N);

/* Segment-averaged (Welch) intensity spectra.  For segment length L, hop H (1 <= H, 2 <= L <= T) and a real window
 * w of length L:
 *     n_seg      = 1 + (T - L) / H              (integer division; frames after the last segment are not used)
 *     U          = (1/L) sum_tau w[tau]^2        (float64 on the host; must be > 0)
 *     F_s[k,c,o] = (1/L) sum_tau w[tau] q[k,c,s H + tau] exp(-2 pi i o tau / L)
 *     I[o,k]     = 1/(n_seg U) sum_s sum_c |F_s[k,c,o]|^2,  summed over the atom groups like PSA_F_INTENSITY
 * No detrending; frequencies are np.fft.fftfreq(L, dt), two-sided, in FFT order.  With w = 1, L = T (one segment)
 * I is the PSA_F_INTENSITY result bit for bit; with w = 1 and H = L, sum_o I is the mean power of the frames used.
 * From this call on, until it is cleared with L = 0, psa_sed_project, _project_upload and _calculate produce I:
 * the projection is unchanged; after it the windowed segments are gathered (in blocks of k rows, so that the extra
 * device memory never exceeds the q buffer), transformed by a batched length-L FFT and reduced into the slab.
 *   - they require PSA_F_INTENSITY, and L <= T of the slot projected (PSA_EINVAL otherwise);
 *   - psa_sed_finalize returns (L,K) float32 (out_bytes = 4 L K); psa_slab_read / psa_slab_write rows are (nrows, L)
 *     float32; folded +-k pairs are mirrored as usual: I(-k)[o] = I(k)[(L - o) mod L];
 *   - the frame-sharded entry points (psa_sed_fs_*) refuse with PSA_EINVAL;
 *   - psa_sed_single_bin (iSED) and the psa_debug_* projections ignore the setting;
 *   - set before an upload, the FFT primer builds the plan of length L instead of T.
 * window: L finite float32 values, copied during the call.  hop < 1, L < 2, a non-finite window or U = 0 is
 * PSA_EINVAL (the previous setting is then kept). */
int psa_set_segments(psa_ctx* ctx, int64_t L, int64_t hop, const float* window /* L, copied; L = 0 clears */);

/* ---- the hot path -------------------------------------------------------
 * psa_sed_project: for each of the G atom groups, for the K_local k-vectors given,
 *     P[k,a]   = exp(i * (k . mean_pos[idx[a]]))            float32 FMA chain + sincos
 *     q[k,c,t] = sum_a  d[t, idx[a], c] * P[k,a]            split-precision f16 MFMA (fp32-equivalent), LDS-staged tiles
 *     S[k,c,w] = FFT_t(q) / T                               batched rocFFT, in place
 * and either keeps S of the (single) group as complex64, or accumulates
 * sum_c |S|^2 over groups as float32 (PSA_F_INTENSITY).  The result stays on the
 * device, k-major, as rows [k_offset, k_offset+K_local) of a K_total-row slab so
 * that k-sharded ranks produce contiguous pieces of one array.
 *
 *   mean_pos_all : (N, 3) float32 host          (sed_calculator.py:205)
 *   k_vectors    : (K_local, 3) float32 host    (rows k_offset.. of the full list)
 *   group_idx    : concatenated atom indices of all groups (int32), or NULL with
 *                  G = 1 meaning "all N atoms in order"
 *   group_off    : (G+1) int64 offsets into group_idx (ignored when group_idx NULL)
 * Without PSA_F_INTENSITY, G must be 1.
 * The first projection of a group after an upload does work that is cached afterwards: one pass for
 * the largest magnitude of the data (the power-of-two scale of the float16 kernels; per 32-atom
 * column block for index-list groups; of slot - mean in displacement mode) with a blocking
 * read-back -- psa_sed_project_upload folds it into the upload -- and, under PSA_OPT_PLANES, the
 * build of the group's split planes.  Later calls are asynchronous on the context's stream.
 */
int psa_sed_project(psa_ctx* ctx, int slot,
                    const float* mean_pos_all,
                    const float* k_vectors, int64_t K_local,
                    int64_t K_total, int64_t k_offset,
                    const int32_t* group_idx, const int64_t* group_off, int32_t G,
                    int32_t flags);

/* The same for an array that is not resident yet: uploads `host` (T,N,3) into the slot AND
 * projects, overlapped -- the array travels in chunks of frames through the staging pipeline of
 * psa_data_upload, and each chunk's frames are projected (first atom group; the projection is
 * independent per frame, sed_calculator.py:80-81) on the compute stream while the next chunk is
 * on the PCIe link; the rocFFT plan is built meanwhile on a host thread.  Further groups, the FFT
 * and the epilogue follow on the resident array.  Result and state as after psa_data_upload +
 * psa_sed_project (all K on this device). */
int psa_sed_project_upload(psa_ctx* ctx, int slot, const float* host, int64_t T, int64_t N,
                           const float* mean_pos_all, const float* k_vectors, int64_t K,
                           const int32_t* group_idx, const int64_t* group_off, int32_t G,
                           int32_t flags);

/* Transpose the K_total-row slab to the reference's layout -- (T,K,3) complex64
 * (sed_calculator.py:277) or (T,K) float32 (:280) -- and copy it to out_host
 * (may be NULL: the result then only exists on the device, see psa_result_*).
 * out_bytes is the size of the caller's buffer and must be exactly the result's
 * (24*T*K or 4*T*K): a mismatch is PSA_EINVAL, nothing is copied.
 * out_intensity (may be NULL; complex results only): (T,K) float32 = sum_c |S|^2, i.e. SED.intensity
 * (src/psa/core/sed.py:22-24) of this very result -- produced by the same pass over the result (the
 * tile is in LDS anyway) and copied beside it; out_intensity_bytes must be 4*T*K. */
int psa_sed_finalize(psa_ctx* ctx, void* out_host, size_t out_bytes,
                     float* out_intensity, size_t out_intensity_bytes);

/* one-call convenience: project all K on this device, finalize, copy out.  A complex result of
 * >= 192 k-vectors leaves block by block (project -> FFT -> transpose -> D2H on a copy stream while the
 * next block is projected).  out_intensity as for psa_sed_finalize. */
int psa_sed_calculate(psa_ctx* ctx, int slot, const float* mean_pos_all,
                      const float* k_vectors, int64_t K,
                      const int32_t* group_idx, const int64_t* group_off, int32_t G,
                      int32_t flags, void* out_host, size_t out_bytes,
                      float* out_intensity, size_t out_intensity_bytes);

/* Vibrational density of states: the power spectrum of the atoms' own series, summed over atom groups -- the
 * k-integrated companion of the SED (which sums amplitudes over atoms BEFORE the FFT; this sums powers AFTER it).
 * d[t,a,c] is the slot's data: velocities, or positions minus mean_pos_all under PSA_F_DISPLACEMENTS.  With segment
 * length L, hop H and real window win (the context's psa_set_segments setting; none set: L = H = T, win = 1) and
 * weights w_a (psa_set_atom_weights; none set: 1), for the atom groups g = 0 .. G-1:
 *     n_seg      = 1 + (T - L) / H                          (integer division, as for segments)
 *     U          = (1/L) sum_tau win[tau]^2
 *     X_s[a,c,o] = (1/L) sum_tau win[tau] d[s H + tau, a, c] exp(-2 pi i o tau / L)
 *     D[o,g,c]   = 1/(n_seg U) sum_s sum_{a in g} w_a^2 |X_s[a,c,o]|^2      o = 0 .. L/2   (L/2 + 1 rows, integer
 *                                                                            division: 32 rows for L = 63)
 * One-sided because the series are real: row o is the two-sided value at bin o, NOT doubled.  Frequencies are
 * np.fft.rfftfreq(L, dt).  No detrending.  The weight is squared so that w = sqrt(m) gives sum m |v(omega)|^2, the
 * convention of the weighted SED: for a group of one atom a, sum_c D[o,{a},c] is the PSA_F_INTENSITY result of the
 * group {a} at any k.  With win = 1 and H = L, D[0] + 2 sum_{0<o<L/2} D[o] (+ D[L/2] for even L) is the mean square of
 * the frames used.
 *   group_idx / group_off / G as for psa_sed_project (NULL with G = 1: all atoms); the groups must be DISJOINT -- a
 *   partial density of states is a partition, and one pass serves all groups; an empty group gives zeros;
 *   out_host: (G, 3, L/2+1) float32, out_bytes exactly its size.
 * PSA_EINVAL: out_bytes not exact, L > T, an index out of range, an atom listed twice, weights set for another N, a
 * work budget (PSA_OPT_VDOS_WORK_BYTES) below 768 L bytes.
 * One pass over the selected atoms' columns of the resident array per (overlapping) segment: gather and transpose
 * through LDS with mean, weight and window applied; a batched length-L rocFFT in which two atoms of one group share a
 * complex series (|X_a|^2 + |X_b|^2 = (|Z[o]|^2 + |Z[L-o]|^2) / 2, so nothing is untangled); |.|^2 summed in float64
 * per (group, component, bin), each element by one thread per launch, launches in order on the context's stream:
 * deterministic.  The slab, the k map, the plane cache and every result of the SED entry points are left as they are.
 * Stage times go to psa_last_timings: [6] gather, [3] FFT, [4] power, [7] device->host. */
int psa_vdos(psa_ctx* ctx, int slot, const float* mean_pos_all /* (N,3); read only under PSA_F_DISPLACEMENTS */,
             const int32_t* group_idx, const int64_t* group_off, int32_t G,
             int32_t flags /* PSA_F_DISPLACEMENTS or 0 */, float* out_host /* (G,3,L/2+1) */, size_t out_bytes);

/* Mode-projected SED (normal-mode decomposition): the spectra of the B basis-site groups of a crystal, contracted with
 * the polarisation vectors of M modes per k-point BEFORE the modulus is taken -- one column per phonon branch instead of
 * one per k-point.  d[t,a,c] is the slot's data: velocities, or positions minus mean_pos_all under PSA_F_DISPLACEMENTS;
 * w_a the context's atom weights (psa_set_atom_weights; none set: 1); r_a = mean_pos_all[a].  For the disjoint atom
 * groups b = 0 .. B-1 ("site b in every cell") and the mode vectors eig (K, M, B, 3) complex64, C order:
 *     q_b[k,c,t]  = sum_{a in b} w_a d[t,a,c] exp(+i k.r_a)            the projection of psa_sed_project, every route
 *     S_b[k,c,w]  = (1/T) sum_t q_b[k,c,t] exp(-2 pi i w t / T)
 *     Q[k,nu,w]   = sum_b sum_c conj(eig[k,nu,b,c]) S_b[k,c,w]
 *     Phi[w,k,nu] = |Q[k,nu,w]|^2                                      out_host (T, K, M) float32, w in FFT order
 * eig is used as given: not normalised, not required to be orthogonal, M is free (the 3 acoustic branches alone are as
 * valid as all 3B).  The sign conventions are the projection's: exp(+i k.r_a) with each atom's OWN mean position (not
 * its cell origin), and conj(eig) in the contraction; a lattice-dynamics code with another phase convention has its
 * vectors converted by the caller.  Pairs (k, -k) are not folded: each k-vector has its own vectors.  An empty group
 * contributes nothing.
 *   group_idx / group_off / B as for psa_sed_project (NULL with B = 1: all atoms); the groups must be disjoint;
 *   out_bytes exactly 4 T K M.
 * PSA_EINVAL: eig or out_host null, M < 1, a non-finite eig value, an atom in two groups, an index out of range,
 * out_bytes not exact, segments set (psa_set_segments: no segment average here), weights set for another N, a work
 * budget (PSA_OPT_MODES_WORK_BYTES) below 24 B T bytes, T > 2^31 - 64 (the contraction indexes frequencies in 32 bits).
 * Per block of k-vectors: B projections into one stacked buffer (B, kb, 3, T), one batched rocFFT of 3 B kb series,
 * one pass (modes.hip) that contracts and takes the modulus; blocks of a k-path keep PSA_OPT_K1_LOWRANK_MIN_LOCAL
 * vectors where the budget allows.  The slab, the k map and every result of the SED entry points are left as they are;
 * the call returns after the stream has drained.  Stage times go to psa_last_timings: [2] projection, [3] FFT,
 * [4] contraction, [7] device->host. */
int psa_sed_modes(psa_ctx* ctx, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                  const int32_t* group_idx, const int64_t* group_off, int32_t B,
                  const void* eig /* (K,M,B,3) complex64 */, int64_t M, int32_t flags /* PSA_F_DISPLACEMENTS or 0 */,
                  float* out_host /* (T,K,M) */, size_t out_bytes);

/* Spectral covariance of the site groups' projections: the frequency-weighted sum of the outer products of the B groups'
 * spectra -- the matrix whose eigenvectors are the mode vectors psa_sed_modes contracts with (the Green's-function
 * method: the displacement covariance of the mass-weighted site coordinates at k is k_B T D(k)^-1).  q_b, S_b, the groups,
 * the weights and the flags as for psa_sed_modes; with i = 3 b + c, n = 3 B and the weight rows g_m (n_w, T) float32 in
 * FFT order:
 *     G^(m)[k,i,j] = sum_w g_m[w] S_i[k,w] conj(S_j[k,w])              out_host (n_w, K, n, n) complex128, C order
 * g = 1 gives (1/T) sum_t q q^+ (Parseval); the weights are used as given, the bin w = 0 included.  out_bytes exactly
 * 16 n_w K n^2.  PSA_EINVAL: n_w outside 1..2, a non-finite weight, 3 B > 96, what psa_sed_modes refuses of its k-list,
 * groups (an atom in two groups, an index out of range), weights and T, a null pointer, out_bytes not exact, segments
 * set (no segment average here), a work budget (PSA_OPT_MODES_WORK_BYTES) that cannot hold one k-vector (24 B T bytes
 * and its partial sums).
 * Per block of k-vectors: psa_sed_modes' B projections and batched rocFFT, then two kernels (covariance.hip): float32
 * products and sums on the fp32 matrix cores -- at most 128 frequencies per accumulator, folded at most 32 times into a
 * second float32 sum, one partial slab per k-vector and 4096 frequencies -- and a pass that adds the slabs in float64,
 * scales by 1/T^2 in float64 and mirrors: G[j,i] is the exact conjugate of G[i,j], Im G[i,i] exactly 0.  No atomics; the
 * result does not depend on the blocking; two identical calls give the same bits.  The slab, the k map, the plane cache
 * and every result of the other entry points are left as they are.  Stage times go to psa_last_timings:
 * [2] projection, [3] FFT, [4] the covariance kernels, [7] device->host. */
int psa_sed_covariance(psa_ctx* ctx, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                       const int32_t* group_idx, const int64_t* group_off, int32_t B,
                       const float* freq_weights /* (n_w, T) */, int32_t n_w, int32_t flags /* PSA_F_DISPLACEMENTS or 0 */,
                       double* out_host /* (n_w, K, 3B, 3B, 2) */, size_t out_bytes);

/* Lorentzian fits of spectrum peaks: frequency and half width per column, on the device.  A spectrum is phi (F, C)
 * float32, C order; row i is bin i of an F-point transform, f_i = i df.  Only the positive half is used, bins
 * 1 .. ceil(F/2) - 1.  Column j has the band [lo_j, hi_j) of bins (bands (C, 2) int32, or NULL: [lo, hi) for all).
 *   1. p = the lowest bin of the band at which phi is largest; half = 0.5f phi[p]; l (r) = the number of consecutive
 *      bins below (above) p, not past the band, with phi >= half; h0 = max(1, (l + r + 1) / 2) bins;
 *      n = clamp(ceil(window_hwhm h0), 4, 2047), or clamp(half_window_bins, 4, 2047) when that is not 0; the window is
 *      [a, b) = [max(lo, p - n), min(hi, p + n + 1)).  Integer and float32 comparisons only.
 *   2. unweighted least squares of  height hwhm^2 / ((f - f0)^2 + hwhm^2) + baseline  over the window's bins, by
 *      Levenberg-Marquardt with Marquardt's diagonal scaling in the units x = (i - p) / h0, y = phi[i] / phi[p], from
 *      f0 = 0, hwhm = 1, baseline = min y, height = 1 - baseline; steps with hwhm <= 0 are rejected; at most max_iter
 *      iterations; stop when the largest step is at most 1e-6 (f0, hwhm relative to hwhm; height, baseline relative
 *      to height).  Sums and solve are float64.
 * fit (C, 6) float32: f0, hwhm (in the units of df), height, baseline, rss (units of phi^2), peak bin p.
 * info (C, 4) int32: status, iterations, a, b - a.  Status 0 converged; 1 iteration cap reached (the best so far);
 * 2 no fit -- a band of fewer than 5 bins, phi[p] <= 0 or a non-finite value in the band: the six floats are NaN, the
 * rest of info 0; 3 converged, but f0 outside [a, b) or hwhm above b - a bins.
 * PSA_EINVAL: a null spectrum or output, F < 12, C < 1, a band outside [1, ceil(F/2)) or with lo >= hi, window_hwhm <= 0,
 * half_window_bins < 0, max_iter < 1.  Two kernels (peaks.hip): one streaming pass that finds the peak bins, one
 * wavefront per column that fits from LDS; deterministic (two calls give the same bits, a column's result does not
 * depend on the other columns).  No result of another entry point is touched.  Stage times go to psa_last_timings:
 * [0] upload, [4] both kernels, [7] device->host. */
typedef struct {
    float   window_hwhm;        /* half width of the fit window in units of the peak's half width at half maximum [8] */
    int32_t half_window_bins;   /* the same in bins, overriding window_hwhm; 0 = automatic */
    int32_t max_iter;           /* iteration cap [50] */
} psa_peak_opts;
/* any spectrum: spec_host (F, C) float32 is uploaded; opts NULL = the defaults */
int psa_fit_peaks(psa_ctx* ctx, const float* spec_host, int64_t F, int64_t C, double df, const int32_t* bands, int32_t lo,
                  int32_t hi, const psa_peak_opts* opts, float* fit /* (C,6) */, int32_t* info /* (C,4) */);
/* psa_sed_modes and the fit of its (T, K M) result where it lies: psa_sed_modes' arguments and refusals, then the
 * fit's with F = T, C = K M (column k M + nu).  out_host may be NULL: the spectra are then not copied to the host. */
int psa_sed_modes_fit(psa_ctx* ctx, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                      const int32_t* group_idx, const int64_t* group_off, int32_t B, const void* eig, int64_t M,
                      int32_t flags, double df, const int32_t* bands, int32_t lo, int32_t hi, const psa_peak_opts* opts,
                      float* fit /* (K*M,6) */, int32_t* info /* (K*M,4) */, float* out_host, size_t out_bytes);

/* Welch-averaged mode spectra: the mode-projected SED with the context's segments (psa_set_segments: length L, hop H,
 * real window win; n_seg = 1 + (T - L) / H, U = (1/L) sum win^2; no detrending, two-sided, FFT order, frames after the
 * last segment unused) between the projection and the contraction.  q_b and eig as for psa_sed_modes:
 *     F_b,s[k,c,w] = (1/L) sum_tau win[tau] q_b[k,c,s H + tau] exp(-2 pi i w tau / L)
 *     Q_s[k,nu,w]  = sum_b sum_c conj(eig[k,nu,b,c]) F_b,s[k,c,w]
 *     Phi[w,k,nu]  = 1/(n_seg U) sum_s |Q_s[k,nu,w]|^2                  out_host (L, K, M) float32
 * With no segments set the call is one boxcar segment of T frames (L = T): psa_sed_modes' result.  out_bytes exactly
 * 4 L K M.  PSA_EINVAL: what psa_sed_modes refuses other than segments; L > T; a work budget
 * (PSA_OPT_MODES_WORK_BYTES) that cannot hold one k-vector of q and one (k-vector, segment) unit, 24 B (T + L) bytes
 * (24 B T with no segments set: q is then transformed in place).
 * Per block of kb k-vectors the B projections are psa_sed_modes' own (plane cache, weights, displacement mode, the
 * low-rank k-path route, its block rule); then per sub-block of bk k-vectors x bs segments: the window pass into
 * (B, bk, 3, bs, L), one batched rocFFT of 3 B bk bs series of length L, one pass (modes.hip) that contracts,
 * takes the modulus and sums the sub-block's segments on chip; the first segments of a column overwrite it, later ones
 * add to it.  q and the segment buffer share the budget; the (L,K,M) result on the device is outside it.  No atomics;
 * launches in order on the context's stream: two identical calls give the same bits.  The slab, the k map, the plane
 * cache and every result of the SED entry points are left as they are.  Stage times go to psa_last_timings:
 * [2] projection, [3] FFT, [4] window and contraction, [7] device->host. */
int psa_sed_modes_welch(psa_ctx* ctx, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                        const int32_t* group_idx, const int64_t* group_off, int32_t B,
                        const void* eig /* (K,M,B,3) complex64 */, int64_t M, int32_t flags /* PSA_F_DISPLACEMENTS or 0 */,
                        float* out_host /* (L,K,M) */, size_t out_bytes);
/* psa_sed_modes_welch and the fit of its (L, K M) result where it lies: psa_sed_modes_welch's arguments and refusals,
 * then the fit's with F = L, C = K M (column k M + nu); df is the caller's (1 / (L dt) for bins of the segment
 * transform).  out_host may be NULL: the spectra are then not copied to the host. */
int psa_sed_modes_welch_fit(psa_ctx* ctx, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                            const int32_t* group_idx, const int64_t* group_off, int32_t B, const void* eig, int64_t M,
                            int32_t flags, double df, const int32_t* bands, int32_t lo, int32_t hi, const psa_peak_opts* opts,
                            float* fit /* (K*M,6) */, int32_t* info /* (K*M,4) */, float* out_host, size_t out_bytes);

/* Dynamic structure factor and current correlations: spectra whose phase comes from the atoms' positions in every frame,
 * not from their time average -- what an inelastic neutron or X-ray measurement sees (multi-phonon lines, the
 * Debye-Waller decay with |k|, the quasi-elastic line), and the only meaningful spectra of a run whose atoms do not stay
 * at a site (a liquid, a glass, a superionic conductor).  r[t,a,:] is the positions slot as stored (no mean is
 * subtracted; PSA_F_DISPLACEMENTS does not apply), v[t,a,:] the velocities slot, w_a the context's atom weights
 * (psa_set_atom_weights; none set: 1), idx one atom set (NULL: all atoms), k_vectors (K, 3) float32.  The phase is
 * exp(+i k.r) of the float32 inputs taken as exact real numbers (the float64 definition, not a float32 FMA chain):
 *     q_0[k,t]          = sum_{a in idx} w_a exp(i k.r[t,a])                   density rho(k,t)
 *     q_c[k,t]          = sum_{a in idx} w_a v[t,a,c] exp(i k.r[t,a])          c = 1,2,3: current j(k,t), only with `currents`
 *     F_s[k,c,o]        = (1/L) sum_tau win[tau] q_c[k, s H + tau] exp(-2 pi i o tau / L)
 *     density[o,k]      = 1/(n_seg U) sum_s |F_s[k,0,o]|^2
 *     longitudinal[o,k] = 1/(n_seg U) sum_s |sum_c khat_c F_s[k,c,o]|^2        khat = k/|k| in float64 from the float32 k
 *     transverse[o,k]   = ( 1/(n_seg U) sum_s sum_c |F_s[k,c,o]|^2 - longitudinal[o,k] ) / 2
 *                       = 1/(2 n_seg U) sum_s sum_c |F_s[k,c,o] - khat_c (khat.F_s[k,.,o])|^2
 * (the kernels form the transverse part the second way, from the component of F perpendicular to khat: a sum of squares,
 * never negative, its error relative to sqrt(|F|^2 |F_perp|^2) and not to |F|^2 -- the difference of the first line loses
 * a transverse part that is small beside the longitudinal one and can come out negative)
 * with the context's segments (psa_set_segments: L, H, win; none set: L = H = T, win = 1); n_seg, U, no detrending,
 * two-sided, FFT order and the unused frames after the last segment exactly as there.  out_host is (1, L, K) float32
 * (density) or, with currents = 1, (3, L, K): density, longitudinal, transverse.  out_bytes exactly its size.
 *   - The physical S(k,omega) is density L dt / sum_a w_a^2; the factor is the caller's (psa_amd.DynamicSpectra applies it).
 *   - A k = 0 row has khat = 0: longitudinal 0, transverse (1/2) sum_c |j_c|^2.
 *   - The static part of rho at a reciprocal-lattice vector (the Bragg peak, N^2 for unit weights) sits in bin 0, and in
 *     its neighbours under a tapered window.
 *   - Pairs (k, -k) are not folded.  An empty atom set (idx non-NULL, n_g = 0) gives zeros.
 * PSA_EINVAL: a null pointer, K < 1, out_bytes not exact, the positions slot not resident, currents with the velocities
 * slot absent or of another shape, an index out of range, weights set for another N, L > T, a work budget
 * (PSA_OPT_DYNAMIC_WORK_BYTES) that cannot hold one k-vector (8 NC (T + L) bytes; 8 NC T with no segments), a non-finite
 * k, a sharded context (psa_comm_init).
 * Per block of k-vectors: one VALU kernel (dynamic.hip) over all frames -- lanes own k-vectors, a frame's atoms are staged
 * in LDS and read as broadcasts, short k-lists split the lanes over atom slices; the phase is formed in turns from
 * kappa = k / 2 pi (float64 on the host, float32 hi + lo on the device) with error-free products whose integer parts are
 * removed exactly before v_sin_f32 / v_cos_f32 --, the window pass, one batched length-L rocFFT, and a power pass that
 * contracts with khat before the modulus.  Per element of q, against the float64 evaluation q64 of the definition,
 *     |q_c[k,t] - q64_c[k,t]| <= (eps_term + (DYN_CHAIN + folds(N_g) + 4) 2^-24) sum_a |w_a| |d_a,c(t)|    d = 1 (c = 0), v_c
 * with DYN_CHAIN = 128 atoms per float32 accumulator, folds(N_g) = ceil(ceil(N_g / 2) / DYN_CHAIN) foldings into a second
 * float32 sum, and eps_term = 2 pi 1.51 2^-24 + sqrt(2) DYN_SINCOS_ERR <= 2^-18 the error of one unit-modulus term
 * (DYN_SINCOS_ERR = 2.6e-7: twice the measured error of the hardware sine and cosine, 1.253e-7; eps_term = 9.3e-7; derivation
 * in dynamic.hip, figures in DESIGN section 7), for P = sum_c |k_c r_c| / 2 pi <= 2^12 turns (2.5e4 rad).  Beyond that
 * nothing is refused and nothing breaks: the argument's error is 1.5 u + 12 u^2 P turns (u = 2^-24) for any P, so eps_term
 * becomes 2 pi (1.5 u + 12 u^2 P) + sqrt(2) DYN_SINCOS_ERR -- 1 % larger at 1e5 rad, doubled at 1.3e7 rad, where the
 * float32 positions themselves carry a phase uncertainty of order 1 rad.  No atomics: two identical calls give the same bits, and the result
 * does not depend on how the budget cuts the k-list into blocks.  The slab, the k map, the plane cache and every result
 * of the SED entry points are left as they are.  Stage times go to psa_last_timings: [2] the kernel, [3] FFT, [4] window
 * and power, [7] device->host. */
int psa_dynamic_spectra(psa_ctx* ctx, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g,
                        int32_t currents /* 0: density only, 1: all three */, float* out_host /* (1 or 3, L, K) */,
                        size_t out_bytes);

/* The same spectra on the reciprocal lattice of the simulation box, per vector or averaged over shells of |k| (the
 * powder average): what a liquid, a glass or a superionic conductor has instead of a direction.  Under periodic
 * boundaries only the commensurate vectors k = n_1 G_1 + n_2 G_2 + n_3 G_3, n integer, are legitimate, and on them the
 * phase is defined by the integers, not by a rounded k:
 *   - H is the box matrix, its rows the box vectors; its float32 entries are taken as exact numbers.
 *   - box_inverse = Hinv, the float64 inverse of H as the caller formed it (psa_amd: np.linalg.inv), 9 doubles row-major.
 *     The library and a float64 reference use the same 9 numbers.
 *   - G = 2 pi Hinv^T; its rows are G_1, G_2, G_3.
 *   - s[t,a,:] = r[t,a,:] . Hinv, on the float32 positions taken as exact: the fractional coordinates.
 *     q_0[n,t] = sum_{a in idx} w_a exp(2 pi i n.s[t,a])
 *     q_c[n,t] = sum_{a in idx} w_a v[t,a,c] exp(2 pi i n.s[t,a])                c = 1, 2, 3
 *   - F_s, density, longitudinal and transverse per vector are exactly those of psa_dynamic_spectra (segments, U,
 *     scaling, FFT order), with khat = n.G / |n.G| formed in float64.
 *   - Powder average: a bin b holds a set V_b of vectors of the FULL sphere, n = 0 never among them, and
 *         X_b[o] = (1/|V_b|) sum_{n in V_b} X_n[o]                               X = density, longitudinal, transverse.
 *     One vector of each pair (n, -n) is projected -- the half-space member, whose first non-zero index is positive --
 *     and X_{-n}[o] = X_n[(L - o) mod L] supplies the other (q(-n) = conj q(n) for real weights).  A bin with no vector
 *     is a row of zeros.
 * indices is (K, 3) int32, |n_j| <= 64 (LAT_MAX_INDEX).
 *   bin_of == NULL  the per-vector form: out_host (1 or 3, L, K) as psa_dynamic_spectra returns it; the vectors are
 *                   projected as given, n = 0 allowed, nothing folded.
 *   bin_of != NULL  the shell form: bin_of[k] in [0, n_bins) is vector k's bin, every vector a half-space member that
 *                   stands for itself and its partner; out_host (1 or 3, L, n_bins).  The sum over a shell is formed on
 *                   the device in float64, scaled by 1 / (2 n_half_b n_seg U L^2) in float64 and rounded once to float32.
 * PSA_EINVAL: a null pointer, K < 1, out_bytes not exact, a non-finite or singular box_inverse, |n_j| > 64, a bin index
 * outside [0, n_bins), a shell-form vector that is 0 or not a half-space member, and every refusal of psa_dynamic_spectra
 * that concerns the slots, the weights, the segments, the budget (PSA_OPT_DYNAMIC_WORK_BYTES, the same rule) and sharding.
 * Per block of vectors: one VALU kernel (lattice.hip) in which the phase factorises, exp(2 pi i n.s) = E_1[n_1] E_2[n_2]
 * E_3[n_3] with E_j[m] = exp(2 pi i m s_j): per staged atom the factors a tile of 512 vectors needs are evaluated once,
 * each directly from m and s_j carried as two float32 (error-free products, integer parts removed exactly), and a
 * (vector, atom, frame) unit is two float32 complex products and the accumulation -- no sine or cosine.  Per element
 *     |q_c[n,t] - q64_c[n,t]| <= (eps_lat + (LAT_CHAIN + folds(N_g) + 4) 2^-24) sum_a |w_a| |d_a,c(t)|     d = 1 (c = 0), v_c
 * with LAT_CHAIN = 128, folds(N_g) = ceil(N_g / LAT_CHAIN) and eps_lat = 3 (2 pi 2^-24 + sqrt(2) DYN_SINCOS_ERR) + 6 2^-24
 * = 2.59e-6 <= 2^-18 for every |n_j| <= 64, independent of |r| up to sum_c |Hinv_cj r_c| <= 2^12 turns (derivation in
 * lattice.hip).  No atomics: two identical calls give the same bits; the projections q do not depend on how the budget
 * cuts the list into blocks; the per-vector result depends on it as psa_dynamic_spectra's does (a budget that also cuts
 * the segments into sub-blocks adds the later ones in float32), the shell form in the order of its float64 sums alone
 * (one float32 ulp at the most).  The plan costs 4 KiB of host and device memory per tile of 512 vectors and every block
 * starts a new tile, so a budget that leaves a handful of vectors per block pays that, and a 256-lane workgroup, per
 * handful.  The result, and the shell form's float64 accumulator (8 bytes x (1 or 3) x L x n_bins), lie outside the
 * budget, as psa_dynamic_spectra's result does.  Nothing of the SED entry points' state or of psa_dynamic_spectra's is touched.  Stage times go to
 * psa_last_timings as for psa_dynamic_spectra: [2] the kernel, [3] FFT, [4] window, power or shell pass, [7] device->host. */
int psa_lattice_spectra(psa_ctx* ctx, const double* box_inverse /* 9 */, const int32_t* indices /* (K,3) */, int64_t K,
                        const int32_t* bin_of /* K or NULL */, int64_t n_bins, const int32_t* idx, int64_t n_g,
                        int32_t currents /* 0: density only, 1: all three */, float* out_host /* (1 or 3, L, K or n_bins) */,
                        size_t out_bytes);

/* The self (incoherent) part of the dynamic structure factor on that lattice: a sum over atoms of moduli where
 * psa_lattice_spectra takes the modulus of a sum over atoms -- what an incoherent scatterer (hydrogen, lithium, sodium,
 * vanadium; w_a = b_inc) shows in a quasi-elastic neutron measurement.  Hinv, s and box_inverse are those of
 * psa_lattice_spectra, the segments L, H, win, U, n_seg and the forward FFT those of psa_dynamic_spectra:
 *     z[a,n,t]     = w_a exp(2 pi i n.s[t,a])
 *     Z_s[a,n,o]   = sum_l win[l] z[a,n,sH+l] exp(-2 pi i o l / L)
 *     density[o,n] = 1/(n_seg U L^2) sum_{a in idx} sum_s |Z_s[a,n,o]|^2
 * The weights enter squared (signed weights are legal) and the result is a SUM over atoms, not a mean:
 * density L dt / sum_a w_a^2 normalises it, and sum_o density[o,n] = sum_a w_a^2 for every vector and every trajectory (Parseval
 * and U = (1/L) sum win^2; exact for one boxcar segment, else up to the segments' coverage).  With integer n a whole
 * box vector added to r changes nothing: the result is the same on wrapped and on unwrapped coordinates.
 *   bin_of == NULL  the per-vector form: out_host (L, K), the vectors as given, n = 0 allowed, nothing folded.
 *   bin_of != NULL  the shell form: out_host (L, n_bins), the mean of density over the FULL-sphere vectors of each shell;
 *                   every vector is a half-space member and -n is read at the mirrored frequency, X_{-n}[o] =
 *                   X_n[(L - o) mod L] (z_{-n} = conj z_n for a real window and real weights); bins, the empty bin and
 *                   the scale 1 / (2 n_half_b n_seg U L^2) are exactly those of psa_lattice_spectra.
 * PSA_EINVAL: everything psa_lattice_spectra refuses that does not concern velocities; the budget rule differs.  Only the
 * positions slot is read.  Work: N_g K n_seg L units of 8 bytes, N_g times what the coherent density costs after its
 * projection.  Per block (self.hip): the series kernel writes work (atoms, vectors, segments, L) complex64 -- the sine and
 * the cosine once per (atom, frame, distinct (axis, index) pair of a vector tile), two float32 complex products per unit,
 * a frame shared by overlapping segments evaluated once per segment (measured faster than sharing it) --, one batched rocFFT, and the power pass adds
 * |Z|^2, formed in float32, in float64 into an accumulator (L, K or n_bins) that lives across blocks; the last launch
 * scales in float64 and rounds once to float32.  Per series element before the window
 *     |z - z64| <= (eps_lat + 2^-24) |w_a|                                  (eps_lat: psa_lattice_spectra)
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): a block is a whole number of atom tiles (4 atoms) x vector tiles (at most 64 vectors
 * with at most 24 distinct (axis, index) pairs) x segments; segments shrink first, then vector tiles, then atom tiles; a
 * budget below 4 atoms x the largest tile's vectors x 8 L bytes is refused.  The accumulator, the chunk sums of the power
 * pass and the result lie outside it.  No atomics: two identical calls give the same bits; the series do not depend on the
 * blocking, the result in the order of its float64 sums alone (one float32 ulp at the most).  Nothing of the other entry
 * points' state is touched.  Stage times go to psa_last_timings: [6] the series kernel, [3] FFT, [4] power pass and
 * finish, [7] device->host. */
int psa_self_spectra(psa_ctx* ctx, const double* box_inverse /* 9 */, const int32_t* indices /* (K,3) */, int64_t K,
                     const int32_t* bin_of /* K or NULL */, int64_t n_bins, const int32_t* idx, int64_t n_g,
                     float* out_host /* (L, K or n_bins) */, size_t out_bytes);

/* The species-resolved (partial) spectra on that lattice: the matrix of partials S_ab(k, w), C_L^ab, C_T^ab of a system
 * of S species, which scattering lengths, charges (charge-charge and number-number, Bhatia-Thornton) or concentrations
 * combine afterwards.  H, Hinv, s, the segments, the window, U, the FFT order and khat are those of psa_lattice_spectra.
 * Species a = 0 .. S - 1 are disjoint atom lists A_a, each in the order given: idx holds them one after the other,
 * species_start (S + 1) their ascending offsets into it, species_start[0] = 0 and species_start[S] = the length of idx.
 * The weights w are the context's atom weights.
 *     q^a_0[n,t] = sum_{i in A_a} w_i exp(2 pi i n.s[t,i])        q^a_c[n,t] = sum_{i in A_a} w_i v[t,i,c] exp(2 pi i n.s[t,i])
 *     F^a = the windowed transform of q^a per segment, as for psa_lattice_spectra
 * One entry per pair a <= b, the pairs in row-major order over the upper triangle, (0,0), (0,1), .., (0,S-1), (1,1), ..:
 * P = S (S + 1) / 2.  With scale = 1 / (L^2 n_seg U)
 *     density_ab[o,n]      = scale sum_seg Re(F^a_0 conj F^b_0)
 *     longitudinal_ab[o,n] = scale sum_seg Re((khat.F^a) conj(khat.F^b))
 *     transverse_ab[o,n]   = scale 1/2 sum_seg sum_c Re(F_perp,c^a conj F_perp,c^b)        F_perp,c = F_c - khat_c (khat.F)
 * the transverse part from the perpendicular components, never as a difference of the other two.  The real part is the
 * symmetrised (ab + ba) / 2, the only part that enters sum_ab b_a b_b S_ab.  Off-diagonal entries are not doubled:
 * sum_a X_aa + 2 sum_{a<b} X_ab is the field X of the union of the species.
 *   bin_of == NULL  the per-vector form: out_host (1 or 3, P, L, K).
 *   bin_of != NULL  the shell form, exactly as for psa_lattice_spectra: half-space members only, X^ab_-n[o] =
 *                   X^ab_n[(L - o) mod L] (both factors mirrored: q^a(-n) = conj q^a(n) for real weights), float32 terms
 *                   summed in float64 over a bin's vectors, segments and both sides, scaled by 1 / (2 n_half_b n_seg U L^2)
 *                   in float64 and rounded once; an empty bin gives zeros; out_host (1 or 3, P, L, n_bins).
 * An empty species gives zeros in all of its pairs.
 * PSA_EINVAL: S < 1 or S > 8 (PARTIAL_MAX_SPECIES), a null idx or species_start, offsets that do not begin at 0 or are not
 * ascending, an atom listed in two species, an index outside [0, N), and everything psa_lattice_spectra refuses.
 * Per block of vectors q is (kb, S, NC, T): the projection kernel of psa_lattice_spectra, unchanged, runs once per species
 * on that species' list, so a species' rows are bit for bit what psa_debug_lattice_project gives for its list and carry its
 * per-element bound; the window pass and the rocFFT see S NC series per vector; the pair passes (partial.hip) then take one
 * lane per (pair, vector or bin, frequency) with the float32 term and float64 sum structure of the passes they replace.
 * The budget rule (PSA_OPT_DYNAMIC_WORK_BYTES) is psa_lattice_spectra's with S NC series per vector where it has NC.  No
 * atomics: two identical calls give the same bits, and the per-vector form does not depend on how the budget cuts the
 * list into blocks of vectors.  The result and the shell form's float64 accumulator lie outside the budget.  Nothing of
 * the other entry points' state is touched.  Stage times as for psa_lattice_spectra. */
int psa_partial_spectra(psa_ctx* ctx, const double* box_inverse /* 9 */, const int32_t* indices /* (K,3) */, int64_t K,
                        const int32_t* bin_of /* K or NULL */, int64_t n_bins, const int32_t* idx, const int64_t* species_start /* S+1 */,
                        int32_t n_species, int32_t currents /* 0: density only, 1: all three */,
                        float* out_host /* (1 or 3, P, L, K or n_bins) */, size_t out_bytes);

/* The time correlations on that lattice: the intermediate scattering function F(k,t) and the current correlations
 * C_L(k,t), C_T(k,t) -- the functions of time whose spectra psa_lattice_spectra gives -- as the LINEAR, unbiased estimator
 * (transforming a spectrum back gives the circular correlation of a segment, lag t contaminated by lag L - t).  Inputs as
 * for psa_lattice_spectra.  Segments come from psa_set_segments and must carry the boxcar window, every value exactly 1.0f;
 * with none set there is one segment of L = T frames; n_seg = 1 + (T - L) / H.  1 <= n_lags <= L.
 *     P      = the smallest power of two >= L + n_lags - 1      (the padded FFT length: part of the definition)
 *     A_s[o] = sum_{l<L} x[sH + l] exp(-2 pi i o l / P),  o = 0 .. P - 1
 *     C[t]   = (1/P) sum_o (sum_s |A_s[o]|^2) cos(2 pi o t / P)  =  Re sum_s sum_{l=0}^{L-1-t} x[sH+l+t] conj x[sH+l]
 *     F[t]   = C[t] / (n_seg (L - t)),  t = 0 .. n_lags - 1
 * for the series x of a field: density from q_0, longitudinal from khat.q, transverse 1/2 sum_c over the perpendicular
 * components q_c - khat_c (khat.q), built from the perpendicular form as in psa_lattice_spectra.  Only the real part -- per
 * vector the part even in t -- is produced.  F[0] is the mean of |x|^2 over the frames used and, with the same boxcar
 * segments, the sum over o of the matching field of psa_lattice_spectra.
 *   bin_of == NULL  the per-vector form: out_host (1 or 3, n_lags, K).
 *   bin_of != NULL  the shell form: out_host (1 or 3, n_lags, n_bins), the mean over the FULL-sphere vectors of each shell
 *                   from its half-space members (C_{-n}[t] = conj C_n[t], so the mean is real); an empty bin gives zeros.
 * PSA_EINVAL: everything psa_lattice_spectra refuses; n_lags outside [1, L]; segments whose window is not the boxcar; a
 * sharded context.  The route is psa_lattice_spectra's with every segment zero-padded to P frames (correlation.hip: the
 * first L values bit copies, the tail written for every block), the power summed where the spectra sum it -- float32 per
 * vector, float64 per shell --, and a float64 back-transform out = float32(factor[t] scale[col] sum_o X[o] tab[(o t) mod P]),
 * tab the float64 cosines from the host, factor[t] = 1 / (P n_seg (L - t)), one chain over o in a fixed order: no atomics,
 * two identical calls give the same bits.  The budget rule (PSA_OPT_DYNAMIC_WORK_BYTES) is psa_lattice_spectra's with a
 * segment buffer of P frames per series where that has L -- also without segments, where the spectra use none; the
 * refusal names P.  The power (1 or 3, P, K or n_bins), the tables and the result lie outside the budget.  Nothing of the
 * other entry points' state is touched.  Stage times go to psa_last_timings: [2] the projection, [5] the padding pass,
 * [3] FFT, [4] power or shell pass, [1] the back-transform, [7] device->host. */
int psa_lattice_correlations(psa_ctx* ctx, const double* box_inverse /* 9 */, const int32_t* indices /* (K,3) */, int64_t K,
                             const int32_t* bin_of /* K or NULL */, int64_t n_bins, const int32_t* idx, int64_t n_g,
                             int32_t currents /* 0: density only, 1: all three */, int64_t n_lags,
                             float* out_host /* (1 or 3, n_lags, K or n_bins) */, size_t out_bytes);

/* The self part in time, F_s(k,t): the sum over the atoms of the set of C_a[t] of z[a,n,.] = w_a exp(2 pi i n.s[.,a])
 * (psa_self_spectra), by the definition above: the weights enter squared, F_s(n, 0) = sum_a w_a^2 for every vector, and
 * the result is the same on wrapped and on unwrapped coordinates.  out_host (n_lags, K), or in the shell form
 * (n_lags, n_bins).  PSA_EINVAL: everything psa_self_spectra refuses, and n_lags, the window and sharding as above.  The
 * route is psa_self_spectra's with rows of P frames: the series kernel writes the first L values of a row, the padding
 * pass the P - L others, for every block; the power pass runs without the frequency mirror in the shell form too (the
 * cosine is even: the scale is 1 / n_half), one read of the transformed block instead of two.  Budget: psa_self_spectra's
 * rule with 8 P bytes per series.  Stage times: [6] the series kernel, [5] the padding pass, [3] FFT, [4] power pass,
 * [1] the back-transform, [7] device->host. */
int psa_self_correlations(psa_ctx* ctx, const double* box_inverse /* 9 */, const int32_t* indices /* (K,3) */, int64_t K,
                          const int32_t* bin_of /* K or NULL */, int64_t n_bins, const int32_t* idx, int64_t n_g, int64_t n_lags,
                          float* out_host /* (n_lags, K or n_bins) */, size_t out_bytes);

/* Real-space self dynamics: the moments of the displacement (mean-square displacement, non-Gaussian parameter) and the
 * self van Hove function of atom groups, from the positions resident in PSA_SLOT_POSITIONS as stored, wrapped or not.
 * H = box (9 doubles, rows = box vectors, r = s H), Hinv = box_inverse, the convention of psa_lattice_spectra.
 *
 * Unwrapping, float64 from the float32 positions:  d[t,a,:] = (r[t,a] - r[t-1,a]) Hinv (t >= 1),  m[t,a,j] = rint(d_j),
 *     n[t,a] = -sum_{t' <= t} m[t',a]  (int32 image counts, n[0] = 0),   u[t,a] = (r[t,a] - r[0,a]) + n[t,a] H.
 * Contract: no atom moves half a box length or more along a box axis between two stored frames -- the only convention
 * possible without image flags.  On an unwrapped trajectory m = 0 and u = r(t) - r(0).  unwrap = 0 skips the image search:
 * u = r(t) - r(0).  As evaluated (msd.hip): d_j = fma(e_z, Hinv[2][j], fma(e_y, Hinv[1][j], e_x Hinv[0][j])) with
 * e = r[t] - r[t-1], and u_c = fma(n_2, H[2][c], fma(n_1, H[1][c], fma(n_0, H[0][c], r_c[t] - r_c[0]))): four roundings, so
 *     |u - u_exact| <= 4 2^-53 (|r_c(t) - r_c(0)| + sum_j |n_j| |H_jc|).
 * The image counts are integer sums over tiles of 64 frames, a scan over the tiles and a scan inside each tile: they do not
 * depend on how the pass is cut.
 *
 * Groups g = 0 .. G-1, G <= 8: idx holds their atoms one group after the other, group_start (G + 1) their offsets; the
 * groups are disjoint, a group may be empty; idx NULL: one group of all N atoms (n_groups = 1, group_start unused).
 * Lags t = 0 .. n_lags-1, 1 <= n_lags <= T; origins O_t = {0, s, 2 s, ...: o + t <= T-1}, s = origin_step >= 1,
 * n_o(t) = (T-1-t) / s + 1 (integer division).  With D = u[o+t,a] - u[o,a]:
 *     M2_c[t,g] = 1/(N_g n_o) sum_{a in g} sum_{o in O_t} D_c^2  (c = x, y, z),   M4[t,g] = 1/(N_g n_o) sum sum (D_x^2+D_y^2+D_z^2)^2
 * out_host (n_lags, G, 4) float64: M2_x, M2_y, M2_z, M4; an empty group gives zeros.  The caller forms msd = sum_c M2_c and
 * alpha_2 = 3 M4 / (5 msd^2) - 1.
 * A direct sum over origins, no FFT.  u is stored as float64 (n_a, 3, T); the moments kernel takes a tile of 256 lags (one
 * per lane) and origin tiles of at most 1024 origins, and per atom stages float32(u[f] - u[o_0]), o_0 the tile's first
 * origin (float64 subtraction, one rounding), for at most 1280 frames, so a staged value has the size of the excursion
 * since o_0, not of the total displacement.  Per (lag, origin) in float32, each operation rounded once:
 *     D_c = b_c - a_c;   q_c = D_c D_c;   r2 = fma(D_z, D_z, fma(D_y, D_y, q_x));   M2_c += (double) q_c;   M4 += (double)(r2 r2)
 * the sums in float64 over origins, atoms, chunks of atoms and blocks, in a fixed order; the last pass divides by
 * N_g n_o(t) in float64.  No atomics: two identical calls give the same bits; another blocking regroups the float64 sums.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): u of a block, 24 T bytes per atom; a block is a whole number of atoms; a budget
 * below one atom is refused and the refusal names the bytes needed.  The partial sums, the accumulator and the result lie
 * outside it.
 * PSA_EINVAL: a null pointer, no positions resident, a box or inverse that is not finite, a singular box, an inverse that
 * is not the box's, n_groups outside [1, 8], offsets that do not begin at 0 or are not ascending, an atom in two groups, an
 * index outside [0, N), n_lags outside [1, T], origin_step < 1, unwrap not 0 or 1, out_bytes not exact, a budget below one
 * atom, a sharded context (psa_comm_init).
 * Only the positions slot is read.  Atom weights and segments set on the context are ignored, not refused; the slab, the
 * k map, the plane cache, the K1 selection, the FFT plans and every result of the other entry points are left as they
 * are.  Stage times go to psa_last_timings: [5] unwrap, [6] the moments kernel, [4] reduce and finish, [7] device->host. */
int psa_displacement_moments(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                             const int64_t* group_start /* G+1 */, int32_t n_groups, int64_t n_lags, int64_t origin_step,
                             int32_t unwrap, double* out_host /* (n_lags, G, 4): M2x, M2y, M2z, M4 */, size_t out_bytes);

/* The self van Hove function as counts: for the lags tau_j (n_vh <= 64 of them, each in [0, T-1]), the bin width dr > 0 and
 * 1 <= n_r <= 1024 bins,  counts[j,g,i] = number of (a in g, o in O_{tau_j}) with i = floor(|D| / dr) < n_r, and
 * counts[j,g,n_r] the overflow count; uint64, so sum_i counts[j,g,:] = N_g n_o(tau_j) exactly.  Unwrapping, groups,
 * origins and the budget are those of psa_displacement_moments.  D and r2 are formed as there from a_c = float32(u_c[o] -
 * u_c[o_0]) and b_c = float32(u_c[o+tau] - u_c[o_0]), o_0 the first origin of the same origin tiles; then
 *     r = sqrt(r2) (rounded once);   x = r inv_dr (rounded once), inv_dr the float32 nearest to 1/dr;
 *     bin = x < n_r ? (int) floorf(x) : n_r.
 * Per workgroup a histogram in LDS with 32-bit integer adds -- the host keeps a workgroup's samples below 2^32 --, written
 * to partials with plain stores and summed in 64-bit integers: integer adds commute, so the counts are bit-identical
 * whatever the order and the blocking.  PSA_EINVAL: everything psa_displacement_moments refuses about the context, the
 * box, the groups, origin_step, unwrap and the budget; n_vh outside [1, 64]; a lag outside [0, T-1]; dr <= 0 or not finite;
 * n_r outside [1, 1024]; out_bytes not exact.  Stage times: [5] unwrap, [6] the histogram kernel, [4] reduce,
 * [7] device->host. */
int psa_van_hove_self(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                      const int64_t* group_start /* G+1 */, int32_t n_groups, const int64_t* lags /* n_vh */, int64_t n_vh,
                      int64_t origin_step, int32_t unwrap, double dr, int32_t n_r, uint64_t* out_host /* (n_vh, G, n_r + 1) */,
                      size_t out_bytes);

/* The self-overlap per time origin and its two moments over the origins (dynamic heterogeneity): for the lags tau_j
 * (1 <= n_lags <= 256 of them, each in [0, T-1], duplicates allowed), the cut-off a > 0 and the origins o_k = k s,
 * k < n_o(tau_j) = (T-1-tau_j) / s + 1,
 *     Q[j,g,k] = #{ a in g : overlap(a, o_k, tau_j) }                       (uint32)
 *     S1[j,g]  = sum_k Q[j,g,k],   S2[j,g] = sum_k Q[j,g,k]^2               (uint64)
 * so that q(t) = S1 / (n_o N_g) and the four-point susceptibility chi_4(t) = (n_o S2 - S1^2) / (n_o^2 N_g), the variance
 * of Q over the origins used, per atom.  Groups, unwrapping, origins and the budget's blocks of atoms are those of
 * psa_van_hove_self.  overlap is the van Hove sample with one bin of width a: a_c = float32(u_c[o] - u_c[o_0]) and
 * b_c = float32(u_c[o+tau] - u_c[o_0]), o_0 the first origin of the origin tile of at most 1024 origins that holds o
 * (float64 subtraction, one rounding), D and r2 as in psa_displacement_moments, and the sample overlaps iff
 *     sqrt(r2) (rounded once) times inv_a (rounded once) < 1,   inv_a the float32 nearest to 1/a
 * -- a strict inequality, the bin 0 of psa_van_hove_self(dr = a, n_r = 1): S1[j,g] equals that count bit for bit.
 * out_sums (n_lags, G, 2) uint64: S1, S2.  out_origins, unless NULL, (n_lags, G, n_o_max) uint32 with n_o_max = n_o(the
 * smallest lag): Q, the entries at k >= n_o(tau_j) zero; origins_bytes is its size, 0 with NULL.  An empty group gives
 * zeros; every group empty gives zeros without a launch.
 * The count kernel (overlap.hip) takes a lane per origin, eight lags per workgroup and a chunk of atoms, keeps its counts
 * in registers and writes them with plain stores; an integer reduce adds a group's chunks into Q, which lives in device
 * memory across the blocks of a call; the last pass forms S1 and S2 in uint64.  No atomics anywhere: the counts are
 * bit-identical whatever the blocking.  Budget (PSA_OPT_DYNAMIC_WORK_BYTES): the table Q, 4 n_lags G n_o_max bytes, and
 * beside it u of a block, 24 T bytes per atom; a table that leaves no room for one atom is refused, and the refusal advises
 * a larger origin_step or fewer lags.
 * PSA_EINVAL: everything psa_van_hove_self refuses about the context, the box, the groups, the lags, origin_step, unwrap
 * and the budget; n_lags outside [1, 256]; a cut-off that is not positive and finite or has no float32 reciprocal;
 * out_bytes or origins_bytes not exact; N_g^2 n_o >= 2^63 (S2 could overflow); a sharded context (psa_comm_init).
 * Stage times: [5] unwrap, [6] the count kernel, [4] reduce and moments, [7] device->host. */
int psa_self_overlap(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                     const int64_t* group_start /* G+1 */, int32_t n_groups, const int64_t* lags /* n_lags */, int64_t n_lags,
                     int64_t origin_step, int32_t unwrap, double cutoff, uint64_t* out_sums /* (n_lags, G, 2): S1, S2 */,
                     size_t out_bytes, uint32_t* out_origins /* (n_lags, G, n_o_max) or NULL */, size_t origins_bytes);

/* Pair distributions: the radial distribution function g(r), its species-resolved partials and the distinct van Hove
 * function G_d(r,t), as integer counts, from the positions resident in PSA_SLOT_POSITIONS as stored, wrapped or not.
 * H = box (rows = box vectors, r = s H), Hinv = box_inverse.  Species alpha = 0 .. S-1, S <= 8, are listed like the
 * groups of psa_displacement_moments (idx, group_start; disjoint; idx NULL: one species of all N atoms).  Lags tau_j in
 * frames (n_lags <= 64 of them, each in [0, T-1]), origins O_tau = {0, s, 2 s, ...: o + tau <= T-1}, s = origin_step:
 *     counts[j,alpha,beta,i] = #{(a in alpha, b in beta, b != a, o in O_tau_j): floor(|mi(r_b(o+tau_j) - r_a(o))| / dr) = i},  i < n_r
 * and counts[j,alpha,beta,n_r] everything at or beyond r_max = n_r dr (the overflow), mi the minimum image.  tau = 0 is
 * g(r), tau > 0 is G_d(r,t).  out_host (n_lags, S, S, n_r + 1) uint64 holds every ordered species pair; the counts are
 * exact integers, sum_i counts[j,alpha,beta,:] = n_o(tau_j) N_alpha (N_beta - delta_alphabeta), and at tau = 0
 * counts[alpha,beta] = counts[beta,alpha] bit for bit.  An empty species, and a species of one atom against itself, give
 * zeros.
 * Nothing is unwrapped: within r_max at most one periodic image of b lies around a, so the minimum image of the stored
 * positions is the distance at any lag.  Served radius: with w_j = 1 / |column j of Hinv| the box's perpendicular widths,
 * rounding the fractional difference to the nearest integer gives the true minimum image of every pair closer than
 * min_j w_j / 2, whatever the tilt; r_max <= (1/2 - 2^-12) min_j w_j is served (compared with a relative slack of 2^-40),
 * anything larger refused before anything is uploaded.  A pair whose fractional difference lies within rounding (2^-24)
 * of 1/2 may take either image; both are then longer than r_max and are counted in the overflow.
 * As evaluated (pair.hip).  Per (frame, atom), float64 from the float32 position:
 *     sigma_j = fma(r_z, Hinv[2][j], fma(r_y, Hinv[1][j], r_x Hinv[0][j]));   c_j = float32(sigma_j - floor(sigma_j) - 0.5)
 * per pair, float32, every operation rounded once, h = H rounded to float32, inv_dr = float32(1 / dr):
 *     e_j = c_j(b) - c_j(a);  e_j = e_j - rintf(e_j) (exact);  d_c = fma(e_2, h[2][c], fma(e_1, h[1][c], e_0 h[0][c]))
 *     r2 = fma(d_z, d_z, fma(d_y, d_y, d_x d_x));   x = sqrt(r2) inv_dr;   bin = x < n_r ? (int) floorf(x) : n_r
 * so x carries at most (|delta d|_2 + 4.5 2^-24 |d|) / dr with |delta d_c| <= sum_j (2^-24 + 3 2^-24 |e_j|) |H_jc|.
 * A workgroup takes 256 alpha-atoms (one per lane), beta-atoms staged in LDS 256 at a time and a slab of origins, and adds
 * into a 32-bit integer histogram in LDS -- the host keeps a workgroup's samples below 2^32 --, written to partials with
 * plain stores and summed in 64-bit integers: no global atomics, no float atomics; two identical calls, any blocking and
 * any order of the atoms inside a species give the same bits.  At tau = 0 every unordered pair is evaluated once.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): c of the listed atoms at a block of origins and at their partner frames, 24 n_a
 * bytes per origin; a budget below one origin is refused and the refusal names the bytes needed.
 * PSA_EINVAL: a null pointer, no positions resident, a box or inverse that is not finite, a singular box, an inverse that
 * is not the box's, r_max beyond the served radius, n_groups outside [1, 8], offsets that do not begin at 0 or are not
 * ascending, an atom in two species, an index outside [0, N), n_lags outside [1, 64], a lag outside [0, T-1],
 * origin_step < 1, dr <= 0 or not finite, n_r outside [1, 1024], out_bytes not exact, a budget below one origin, a sharded
 * context (psa_comm_init).
 * Only the positions slot is read.  Atom weights and segments set on the context are ignored, not refused; every result
 * and plan of the other entry points is left as it is.  Stage times: [5] the fraction pass, [6] the pair kernel,
 * [4] reduce, [7] device->host. */
int psa_pair_histogram(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                       const int64_t* group_start /* S+1 */, int32_t n_groups, const int64_t* lags /* n_lags */, int64_t n_lags,
                       int64_t origin_step, double dr, int32_t n_r, uint64_t* out_host /* (n_lags, S, S, n_r + 1) */,
                       size_t out_bytes);

/* Bond-angle distributions and coordination statistics: the neighbour shell of every atom at every time origin, the
 * histogram of the angles between pairs of neighbours and the histogram of the neighbour counts, as integer counts.
 * Inputs.  The positions resident in PSA_SLOT_POSITIONS as stored; nothing is unwrapped, for the reason given at
 * psa_pair_histogram.  H = box with its inverse, and S <= 8 disjoint species (idx, group_start), as for
 * psa_pair_histogram.  r_cut (S, S) double, symmetric, every entry finite, >= 0 (0: no bond between these species) and
 * <= the served radius of psa_pair_histogram (the same relative slack of 2^-40).  Origins o = 0, s, 2 s, ... <= T-1,
 * s = origin_step, n_o = (T-1) / s + 1.  n_theta in [1, 1024].
 * Neighbour.  b in beta is a neighbour of a in alpha at origin o when b != a, r_cut[alpha,beta] > 0 and x < 1, x being
 * exactly the value psa_pair_histogram forms with dr = r_cut[alpha,beta]:
 *     c_j from the float64 prepass;   e_j = c_j(b) - c_j(a);  e_j = e_j - rintf(e_j)
 *     d_c = fma(e_2, h[2][c], fma(e_1, h[1][c], e_0 h[0][c]));   r2 = fma(d_z, d_z, fma(d_y, d_y, d_x d_x))
 *     x = sqrt(r2) float32(1 / r_cut[alpha,beta])
 * every operation rounded once.  With one scalar cut-off the number of neighbours is bit for bit the count that
 * psa_pair_histogram puts into bin 0 with dr = r_cut, n_r = 1.
 * Capacity.  A centre holds at most 64 neighbours (ANGLE_MAX_NEIGHBOURS), all species together.  A (centre, origin) with
 * more is truncated: it contributes to neither histogram -- all or nothing, never its first 64 -- and is counted in
 * truncated[alpha].
 * Coordination.  coord[alpha,beta,n], n = 0 .. 64: the number of (a in alpha, o), not truncated, with exactly n
 * neighbours of species beta.  sum_n coord[alpha,beta,n] + truncated[alpha] = n_o N_alpha for every beta, exactly.
 * Angles.  For a centre a in alpha that is not truncated, every unordered pair {b, c} of its neighbours, b in beta, c in
 * gamma, is filed under the species pair p(beta <= gamma) -- upper triangle, row-major, P = S (S + 1) / 2 pairs: (0,0),
 * (0,1), .., (0,S-1), (1,1), .. -- by the angle at a.  float32, every operation rounded once, from the d of the two legs:
 *     dot = fma(d_z(b), d_z(c), fma(d_y(b), d_y(c), d_x(b) d_x(c)));   q = r2(b) r2(c);   cos = dot / sqrt(q)
 * clamped to [-1, 1]; every step is symmetric in b <-> c bit for bit, so the order of the list cannot move a count.
 * Bins are uniform in theta over [0, pi], defined through the table cedge[i] = float32(cos(i pi / n_theta)) computed in
 * float64 and rounded once, cedge[0] = 1 and cedge[n_theta] = -1 exactly (strictly decreasing up to 1024 bins):
 * bin = the i with cedge[i+1] < cos <= cedge[i]; cos = -1 goes to the last bin; a cos that is not a number (a coincident
 * neighbour, r2 = 0) goes to the extra counter n_theta ("undefined").  angles[alpha,p,i], i <= n_theta.
 *     sum_i angles[alpha,p(beta,beta),i] = sum_n coord[alpha,beta,n] n (n - 1) / 2
 *     sum_i angles[alpha,p(beta,gamma),i] = sum over the centres that are not truncated of n_beta n_gamma   (beta < gamma)
 * exactly.
 * As evaluated (angle.hip): the fraction pass of psa_pair_histogram; a neighbour pass in which a workgroup holds 256
 * centres in registers and walks all beta-atoms staged in LDS, appending each hit {d_x, d_y, d_z, list position and
 * species} to the lane's own list and counting on beyond 64; an angle pass in which a wavefront reads a centre's list
 * once, its lanes take the pairs, and counts go by 32-bit integer adds into histograms in LDS -- the host keeps a
 * workgroup's samples below 2^32 --, written to partials with plain stores and summed in 64-bit integers.  No global
 * atomics, no float atomics; two identical calls, any budget and any order of the atoms inside a species give the same
 * bits.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block c, the counts and the lists of the listed atoms, 1040 n_a
 * bytes; a block is a whole number of origins, a budget below one origin is refused and the refusal names the bytes
 * needed.
 * PSA_EINVAL: what psa_pair_histogram refuses about the context (a sharded one among it), the box, the inverse and the
 * species; a null pointer; r_cut not symmetric, negative, not finite or beyond the served radius; origin_step < 1;
 * n_theta outside [1, 1024]; angles_bytes or coord_bytes not exact; 2^28 or more listed atoms; a budget below one origin.
 * Only the positions slot is read.  Atom weights and segments set on the context are ignored, not refused; every result
 * and plan of the other entry points is left as it is.  Stage times: [0] the tables' upload, [5] the fraction pass,
 * [6] the neighbour pass, [1] the angle pass, [4] reduce, [7] device->host. */
int psa_angle_histogram(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                        const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */, int64_t origin_step,
                        int32_t n_theta, uint64_t* angles /* (S, P, n_theta + 1) */, size_t angles_bytes,
                        uint64_t* coord /* (S, S, 65) */, size_t coord_bytes, uint64_t* truncated /* S */);

/* Steinhardt bond-orientational order parameters q_l of every atom's neighbour shell at every time origin: per species and
 * order l the histogram of q_l, as integer counts, and optionally q_l^2 of every atom as an exact integer.
 * Inputs.  The positions slot, H = box with its inverse, S <= 8 disjoint species, r_cut (S, S) and origin_step exactly as
 * for psa_angle_histogram, under the same checks and refusals.  ls: n_ls orders, strictly ascending integers in [1, 12],
 * 1 <= n_ls <= 8.  n_q in [1, 1024].
 * Neighbours and capacity.  The neighbours of a centre are bit for bit those of psa_angle_histogram, of all species
 * together (a pair of species bonds where r_cut[alpha][beta] > 0); n is their number.  A centre a in alpha at an origin is
 * left out of the histograms, all or nothing, and counted once, in the first of
 *     truncated[alpha]   it has more than 64 neighbours
 *     isolated[alpha]    it has n = 0 neighbours
 *     undefined[alpha]   it has a pair of legs whose cosine is not a number (a coincident neighbour, r2 = 0)
 * that applies: sum_i hist[alpha,j,i] + truncated[alpha] + isolated[alpha] + undefined[alpha] = n_o N_alpha exactly for every j.
 * Definition.  q_l(a)^2 = 4 pi / (2 l + 1) sum_m |1/n sum_b Y_lm(d_b / |d_b|)|^2 over the n legs d_b of a, which by the
 * addition theorem of the spherical harmonics is 1/n^2 (n + 2 sum_{b<c} P_l(cos theta_bc)), theta_bc the angle between the
 * legs b and c.  It is evaluated in that form.
 * Per unordered pair {b, c} of legs, float32, every operation rounded once:
 *     dot = fma(d_z(b), d_z(c), fma(d_y(b), d_y(c), d_x(b) d_x(c)));   q = r2(b) r2(c);   cos = dot / sqrt(q)
 * clamped to [-1, 1] -- the chain of psa_angle_histogram, from the same stored d and r2 -- and then
 *     P_0 = 1;   P_1 = cos;   P_{k+1} = __fmaf_rn(A_k, __fmul_rn(cos, P_k), -__fmul_rn(B_k, P_{k-1})),   k = 1 .. max(ls) - 1
 *     A_k = float32((2 k + 1) / (k + 1)),   B_k = float32(k / (k + 1))   (the quotients formed in float64, rounded once)
 *     t_l = __float2ll_rn(__fmul_rn(P_l, 2^24))
 * The scaling is exact; the rounding to an integer loses at most 2^-25 in P_l.  Every step is symmetric in b <-> c bit for
 * bit.
 * Per centre, 64-bit integers:  X_l = n 2^24 + 2 sum_{b<c} t_l(b, c), clamped to [0, n^2 2^24];  q_l^2 = X_l / (n^2 2^24).
 * Integer adds commute, so X_l depends on neither the order of the list, the blocking, the budget nor the order of the
 * atoms inside a species.
 * Bin.  n_q uniform bins in q over [0, 1], found with integers only: the largest i in [0, n_q - 1] with
 * i^2 n^2 2^24 <= X_l n_q^2 (both sides stay below 2^57; q = 1 is in the last bin).  No floating-point root and no
 * floating-point comparison after t_l.
 * Outputs.  hist (S, n_ls, n_q) uint64; truncated, isolated, undefined (S) uint64; optionally per atom (either pointer may
 * be NULL) x (n_o, n_a, n_ls) int64, the clamped X_l, -1 for a centre that is left out, and n (n_o, n_a) int32, the true
 * neighbour count (beyond 64 too) -- n_a the listed atoms in list order.
 * As evaluated (order.hip): the fraction pass and the neighbour pass of psa_angle_histogram; an order pass in which a
 * wavefront reads a centre's list once, its lanes take the pairs and add t_l into 64-bit integers, a 64-bit wave
 * reduction, and one lane per order bins with a 32-bit integer add in LDS -- an item's samples stay below 2^32 --, written
 * to partials with plain stores and summed in 64-bit integers.  No global atomics, no float atomics; two identical calls,
 * any budget and any order of the atoms inside a species give the same bits.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block 1040 n_a bytes as for psa_angle_histogram, plus 8 n_ls n_a
 * when x is asked for; every block's x and n are copied to the caller's arrays block by block; a budget below one origin
 * is refused and the refusal names the bytes needed.
 * PSA_EINVAL: everything psa_angle_histogram refuses about the context, the box, the species, r_cut, origin_step and the
 * budget; ls null, n_ls outside [1, 8], an order outside [1, 12] or not strictly ascending; n_q outside [1, 1024];
 * hist_bytes not exact; a null hist, truncated, isolated or undefined.
 * Not here: odd l in psa_local_order, the q_lm of other neighbour definitions, Voronoi or solid-angle-weighted neighbours,
 * cell lists (w_l, the neighbour-averaged q_l and the bonds: psa_local_order; the clusters of the solid-like atoms:
 * psa_solid_clusters).
 * Only the positions slot is read.  Atom weights and segments set on the context are ignored, not refused; every result
 * and plan of the other entry points is left as it is.  Stage times: [0] the table's upload, [5] the fraction pass,
 * [6] the neighbour pass, [1] the order pass, [4] reduce, [7] device->host. */
int psa_bond_order(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                   const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */, int64_t origin_step,
                   const int32_t* ls /* n_ls */, int32_t n_ls, int32_t n_q, uint64_t* hist /* (S, n_ls, n_q) */, size_t hist_bytes,
                   uint64_t* truncated /* S */, uint64_t* isolated /* S */, uint64_t* undefined /* S */,
                   int64_t* x /* (n_o, n_a, n_ls) or NULL */, int32_t* n /* (n_o, n_a) or NULL */);

/* Local order from the vectors q_lm of every atom's neighbour shell at every time origin: the neighbour-averaged q-bar_l of
 * Lechner and Dellago, the third-order invariants w_l and w-bar_l, and the solid-like bonds of ten Wolde, Ruiz-Montero and
 * Frenkel, as integer counts and optionally per atom.
 * Inputs.  The positions slot, H = box with its inverse, S <= 8 disjoint species, r_cut (S, S) and origin_step exactly as
 * for psa_angle_histogram, under the same checks and refusals.  The neighbours of a centre are bit for bit those of
 * psa_bond_order: all species together, at most 64, n of them with the legs d_b; the relation is symmetric bit for bit (the
 * minimum-image chain is odd in e).
 * Orders.  ls: n_ls strictly ascending EVEN orders in [2, 12], 1 <= n_ls <= 4.  For odd l the 3j symbol (l l l; m1 m2 m3)
 * is antisymmetric under an exchange of two columns, so W_l vanishes identically: an odd order is refused.
 * The vector.  With Yt_lm = sqrt(4 pi / (2 l + 1)) Y_lm (|Yt_lm| <= 1), Condon-Shortley phase included:
 *     Q_lm(a) = sum_b t_lm(b),   t = __double2ll_rn(Yt_lm(d_b / |d_b|) 2^40) for the real and the imaginary part, m = 0 .. l
 *     Q_{l,-m} = (-1)^m conj Q_lm;   q_lm = (Q_lm 2^-40) / n
 * 64-bit integers (64 x 2^40 fits), and integer adds commute: Q is the same bits for any blocking, budget and atom order.
 * The harmonics, float64, without trigonometry and without a pole; every operation rounded once, none contracted
 * (__dmul_rn, __dadd_rn, __ddiv_rn, __dsqrt_rn only):
 *     x, y, z = (double) d_x, d_y, d_z (exact);   r = sqrt(z z + (y y + x x));   u = (x / r, y / r, z / r)
 *     c_0 = 1;  c_m = c_{m-1} (u_x + i u_y):   re' = re u_x + (-(im u_y)),   im' = re u_y + im u_x
 *     Pi_mm = (2 m - 1)!! (exact);   Pi_{m+1,m} = (2 m + 1)!! u_z;
 *     Pi_lm = ((2 l - 1) (u_z Pi_{l-1,m}) + (-((l + m - 1) Pi_{l-2,m}))) / (l - m)
 *     Yt_lm = ((N_lm Pi_lm) re(c_m), (N_lm Pi_lm) im(c_m)), each then times 2^40 and rounded to the nearest integer
 *     N_lm = (-1)^m sqrt(1 / prod_{k = l-m+1 .. l+m} k), float64 on the host, the product taken in ascending k
 * A leg of length 0 makes the centre undefined (also a centre's only leg, which psa_bond_order still counts).
 * Lechner-Dellago average, float64:  q-bar_lm(a) = (q_lm(a) + sum_{b in N(a)} q_lm(b)) / (n + 1), the sum taken in list
 * order starting from q_lm(a), every q_lm(b) = (Q_lm(b) 2^-40) / n_b formed first.  qbar2 = sum_{m=-l..l} |q-bar_lm|^2 =
 * q-bar_l^2, formed as sum_{m=0..l} c_m (re re + im im) in ascending m, c_0 = 1, c_m = 2.  Its bin of n_q uniform bins in
 * q-bar over [0, 1]: the largest i < n_q with (double)(i i) <= __dmul_rn(qbar2, (double)(n_q n_q)), by bisection; no root.
 * Third-order invariants.  W_l(v) = sum_{m1+m2+m3=0} (l l l; m1 m2 m3) Re(v_m1 v_m2 v_m3), w_l(v) = W_l(v) / S^{3/2},
 * S = sum_m |v_m|^2 as above; evaluated as W / (S sqrt(S)).  w = w_l(Q(a) 2^-40) (scale invariant: no n) and wbar =
 * w_l(q-bar(a)), the w-bar_l of Lechner and Dellago.  w3j: the caller's table, per order the dense block (2 l + 1)^2 of
 * (l l l; m1 m2 -m1-m2) at [(m1 + l) (2 l + 1) + m2 + l], 0 where |m1 + m2| > l, the blocks concatenated in the order of ls
 * (w3j_count values); the terms of a block are dealt to 64 partial sums in strides of 64 and those added pairwise by a
 * butterfly (partners 32, 16, 8, 4, 2, 1 apart), an order that depends on the table alone.  Bin of n_w uniform bins over [-w_range, w_range]:
 * u = __dmul_rn(__dadd_rn(w, w_range), n_w / (2 w_range)); i = floor(u) where 0 <= u < n_w, else the value counts as
 * outside.  Where S is exactly 0 the value is undefined (NaN per atom).  w_l of a shell whose q_l is nearly 0 is noise.
 * Solid-like bonds, for the order solid_l among ls and 0 < solid_threshold <= 1:  D = Re sum_{m=-l..l} Q_lm(a) conj Q_lm(b),
 * A = sum_m |Q_lm(a)|^2, B = sum_m |Q_lm(b)|^2, float64 from the integers times 2^-40, sums over m = 0 .. l with the
 * weights c_m as above.  The bond a-b is solid-like when D > 0 and D D > thr^2 (A B): no root, no division, symmetric in
 * a <-> b bit for bit.  xi(a) = the number of such bonds, 0 .. 64.
 * Left out, all or nothing per (origin, centre), counted once in the first that applies: truncated (more than 64
 * neighbours), isolated (none), undefined (a leg of length 0), incomplete (a neighbour that is truncated or undefined).
 * Outputs.  hist (S, R) uint64, a species' row R = n_ls n_q + 2 n_ls n_w + 65 + 4 + 4 n_ls:
 *     qbar[n_ls][n_q], w[n_ls][n_w], wbar[n_ls][n_w], connections[65], truncated, isolated, undefined, incomplete,
 *     w_outside[n_ls], w_undefined[n_ls], wbar_outside[n_ls], wbar_undefined[n_ls]
 * For every order sum_i qbar[j][i] + the four counters = sum_i connections[i] + the four = n_o N_alpha; for w and wbar the
 * same with that histogram's outside and undefined added.  Optionally per atom, in list order (any may be NULL): qbar2, w,
 * wbar (n_o, n_a, n_ls) float64, NaN where the centre is left out (w, wbar: or undefined); connections (n_o, n_a) int32,
 * -1 where left out; n (n_o, n_a) int32 the true neighbour count.
 * As evaluated (qlm.hip): the fraction pass and the neighbour pass of psa_angle_histogram; a pass in which a wavefront takes
 * a centre, lane b the leg b, and a 64-bit integer wave reduction leaves Q_lm in a table (n_a, sum (l + 1), 2) int64 per
 * origin; a second pass over the same items in which a wavefront gathers its neighbours' rows of that table and counts with
 * 32-bit integer adds in LDS, written to partials with plain stores and summed in 64-bit integers.  No global atomics, no
 * float atomics; two identical calls and any budget give the same bits; a permutation of the atoms inside a species leaves
 * Q the same bits and moves the float64 values by the roundings of the reordered sums.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block 1040 n_a bytes as for psa_angle_histogram, plus 16 sum (l + 1)
 * n_a for the table, plus (24 n_ls + 8) n_a when any of qbar2, w, wbar, connections is asked for.
 * PSA_EINVAL: everything psa_angle_histogram refuses about the context, the box, the species, r_cut, origin_step and the
 * budget; ls null, n_ls outside [1, 4], an order outside [2, 12], odd, or not strictly ascending; n_q or n_w outside
 * [1, 1024]; w_range not finite or <= 0; solid_l not among ls; solid_threshold outside (0, 1]; w3j null, w3j_count not the
 * blocks' size, an entry not finite or beyond 1 in modulus; hist_bytes not exact; a null hist.
 * Only the positions slot is read; every result and plan of the other entry points is left as it is.  Stage times: [0] the
 * tables' upload, [5] the fraction pass, [6] the neighbour pass, [1] the two passes, [2] of these the second, [4] reduce,
 * [7] device->host. */
int psa_local_order(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                    const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */, int64_t origin_step,
                    const int32_t* ls /* n_ls */, int32_t n_ls, int32_t n_q, int32_t n_w, double w_range, int32_t solid_l,
                    double solid_threshold, const double* w3j /* w3j_count */, int64_t w3j_count, uint64_t* hist /* (S, R) */,
                    size_t hist_bytes, double* qbar2 /* (n_o, n_a, n_ls) or NULL */, double* w /* the same */,
                    double* wbar /* the same */, int32_t* connections /* (n_o, n_a) or NULL */, int32_t* n /* (n_o, n_a) or NULL */);

/* The first pass of psa_local_order alone at one frame: q (n_a, sum (l + 1), 2) int64, Q_lm of every listed atom, the
 * orders' columns m = 0 .. l one after the other, (re, im).  A centre that is truncated, isolated or undefined has zeros,
 * and -1 in Im Q of its first column (0 for every other centre: Y_l0 is real).  Refusals as for psa_local_order and
 * psa_debug_neighbour_lists. */
int psa_debug_qlm(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                  const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */, int64_t frame,
                  const int32_t* ls /* n_ls */, int32_t n_ls, int64_t* q /* (n_a, sum (l + 1), 2) */);

/* Solid-like clusters: the connected components of the solid atoms over the neighbour lists, per time origin -- the size
 * of the largest is the order parameter of a nucleation study, the size distribution gives its free energy.
 * Inputs.  The positions slot, H, the species, r_cut and origin_step exactly as for psa_local_order, under the same checks
 * and refusals; solid_l an even order in [2, 12], 0 < solid_threshold <= 1, min_connections in [0, 64], link 0 or 1,
 * n_sizes in [1, 4096].
 * Definition.  The neighbours are those of psa_local_order (all species together, at most 64).  xi(a) is its number of
 * solid-like bonds for the order solid_l, by its rule and its arithmetic, bit for bit; -1 for a centre that is truncated,
 * isolated, undefined or incomplete.  a is solid when xi(a) >= min_connections.  Two solid atoms a != b are joined when b
 * is in a's list or a is in b's (link 0, "neighbours": ten Wolde, Ruiz-Montero and Frenkel); with link 1 ("solid bonds")
 * the bond, in whichever list holds it, must be solid-like as well.  A cluster is a connected component of solid atoms; its
 * label is the smallest column of its members (a column: the position in the concatenated atom list); an atom that is not
 * solid has label -1 and size 0.  Per origin, on positions as stored; the lists are minimum-image, so a cluster runs
 * through the periodic boundary.
 * Outputs.  species_rows (S, 69) uint64: connections[65], truncated, isolated, undefined, incomplete -- those 69 words of
 * psa_local_order's row, the same bits.  size_counts (n_sizes + 2) uint64 over all origins: slot s in [1, n_sizes] the
 * clusters of exactly s atoms, slot n_sizes + 1 the larger ones, slot 0 stays 0; *large_atoms the atoms in the larger ones:
 * sum_s s size_counts[s] + large_atoms = sum n_solid, sum_s size_counts[s] = sum n_clusters.  Per origin (n_o) int32:
 * n_solid, n_clusters, largest (0: none) and largest_label (the smallest label among the clusters of that size, -1: none).
 * Optionally per atom, in list order (any may be NULL): labels, size_atoms (the size of the atom's cluster), connections
 * (xi), n (the true neighbour count), int32 (n_o, n_a), and bond_masks uint64 (n_o, n_a): bit b set when the bond to the
 * b-th neighbour of the list is solid-like (0 where the centre is left out).
 * As evaluated (cluster.hip): the fraction pass and the neighbour pass of psa_angle_histogram, the q_lm pass of
 * psa_local_order for the one order, then a bonds pass (xi, masks, every solid atom its own parent), a hook pass (lock-free
 * union, the larger root under the smaller: compare-and-swap on parent, path halving, every loop bounded by n_a), a flatten
 * pass (label = root; one integer add per distinct label of a wavefront on size) and a stats pass.  Integer global atomics
 * on parent and size only; a minimum and integer sums do not depend on the order, so two identical calls and any budget
 * give the same bits, and a permutation of the atoms gives the same partition.  No float atomics.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block 1040 n_a bytes as for psa_angle_histogram, plus 16 (solid_l +
 * 1) n_a for the table, plus 20 n_a (xi 4, mask 8, parent / label 4, size 4); a budget below one origin is refused and the
 * refusal names the bytes needed.
 * PSA_EINVAL: everything psa_angle_histogram refuses about the context (a sharded one among it), the box, the species,
 * r_cut, origin_step and the budget; solid_l odd or outside [2, 12]; solid_threshold outside (0, 1]; min_connections
 * outside [0, 64]; link not 0 or 1; n_sizes outside [1, 4096]; a null required output.  PSA_EHIP "cluster pass did not
 * converge": a bounded loop of the hook or flatten pass ran out (a defect, never a hang).
 * Only the positions slot is read; every result and plan of the other entry points is left as it is.  Stage times: [0] the
 * tables' upload, [5] the fraction pass, [6] the neighbour pass, [1] the q_lm, bonds, hook and flatten passes, of these [2]
 * the hook and [3] the flatten pass, [4] the species reduce, the stats pass and its reduce, [7] device->host. */
int psa_solid_clusters(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                       const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */, int64_t origin_step,
                       int32_t solid_l, double solid_threshold, int32_t min_connections, int32_t link, int32_t n_sizes,
                       uint64_t* species_rows /* (S, 69) */, uint64_t* size_counts /* n_sizes + 2 */, uint64_t* large_atoms /* 1 */,
                       int32_t* n_solid /* n_o */, int32_t* n_clusters /* n_o */, int32_t* largest /* n_o */,
                       int32_t* largest_label /* n_o */, int32_t* labels /* (n_o, n_a) or NULL */, int32_t* size_atoms /* the same */,
                       int32_t* connections /* the same */, int32_t* n /* the same */, uint64_t* bond_masks /* (n_o, n_a) or NULL */);

/* The graph passes of psa_solid_clusters alone (hook, flatten, stats) on a graph of the caller's, all n_o <= 65535 origins
 * in one block: count (n_o, n_a) int32 in [0, 64], list (n_o, n_a, 64) int32 the neighbours' columns (only the first count
 * are read), solid (n_o, n_a) uint8, bond_masks (n_o, n_a) uint64 or NULL (all ones), link, n_sizes as above.  The list
 * entries are built with the tags the neighbour pass would have written.  Lists that are not symmetric are legal: an edge
 * that only one end lists joins.  Outputs as for psa_solid_clusters without the species rows; labels and size_atoms may be
 * NULL.  PSA_EINVAL: a column outside [0, n_a), a count outside [0, 64], a self-loop, link, n_sizes, n_o or n_a out of
 * range, a graph beyond the work budget, a sharded context, a null required argument. */
int psa_debug_cluster_labels(psa_ctx* ctx, int64_t n_o, int64_t n_a, const int32_t* count /* (n_o, n_a) */,
                             const int32_t* list /* (n_o, n_a, 64) */, const uint8_t* solid /* (n_o, n_a) */,
                             const uint64_t* bond_masks /* (n_o, n_a) or NULL */, int32_t link, int32_t n_sizes,
                             uint64_t* size_counts /* n_sizes + 2 */, uint64_t* large_atoms /* 1 */, int32_t* n_solid /* n_o */,
                             int32_t* n_clusters /* n_o */, int32_t* largest /* n_o */, int32_t* largest_label /* n_o */,
                             int32_t* labels /* (n_o, n_a) or NULL */, int32_t* size_atoms /* the same */);

/* Bond persistence: how long a neighbour stays a neighbour.  The pairs listed at a time origin are tested again at later
 * frames; the counts give the intermittent and the continuous bond correlation of every species pair and the cage
 * correlation of every species, as integers.
 * Inputs.  The positions slot as stored, H = box with its inverse, S <= 8 disjoint species (idx, group_start), r_cut (S, S)
 * and origin_step exactly as for psa_angle_histogram, under the same checks and refusals.  r_break (S, S) double, symmetric
 * and finite, every entry >= r_cut's and <= the served radius, 0 exactly where r_cut is 0: a bond forms below r_cut and
 * counts as alive while it stays below r_break (hysteresis; r_break = r_cut: none).  lags: n_lags in [1, 1024] frame lags,
 * strictly ascending, each in [0, T-1] and a multiple of sample_step >= 1.  continuous: 0 or 1.
 * Origins and centres.  The origins of lag tau are O_tau = {o = 0, s, 2 s, ... : o + tau <= T-1}, s = origin_step, as for
 * psa_pair_histogram; n_o(tau) = (T-1-tau) / s + 1 is their number.  The neighbours of centre a at origin o are bit for bit
 * those of psa_angle_histogram (r_cut); n_beta(a, o) of them are of species beta.  A (centre, origin) with more than 64
 * neighbours is left out whole -- never its first 64 -- and counted in truncated[j, alpha] for every lag j whose O_tau holds
 * that origin.
 * Alive.  A listed neighbour b of a at origin o is alive at frame o + f when x < 1, x being exactly the float32 chain
 * stated at psa_angle_histogram evaluated on the centred fractions c_j of frame o + f, with float32(1 / r_break[alpha,beta])
 * in place of the reciprocal of r_cut; every operation rounded once.  At f = 0 every listed neighbour is alive: the
 * reciprocal of a larger radius is not larger, and the chain is otherwise the one that listed it.  The chain is odd in e bit
 * for bit, so alive(a, b, o, f) = alive(b, a, o, f).
 * Outputs, uint64.
 *     bonds[j, alpha, beta]      sum over o in O_tau_j and the centres a in alpha that are not truncated of n_beta(a, o)
 *     alive[j, alpha, beta]      those bonds alive at o + tau_j: the intermittent correlation is alive / bonds
 *     unbroken[j, alpha, beta]   those bonds alive at every visited frame o + v, v in {sample_step, 2 sample_step, ...},
 *                                v <= tau_j: the continuous correlation is unbroken / bonds; zeros when continuous = 0
 *     lost[j, alpha, m]          m = 0 .. 64: the (a in alpha, o in O_tau_j), not truncated, with exactly m of their listed
 *                                neighbours not alive at o + tau_j (the cage correlation: the share with m < c)
 *     truncated[j, alpha]
 * At lag 0 alive = unbroken = bonds = sum_n n coord[alpha, beta, n] of psa_angle_histogram, bit for bit;
 * sum_m lost[j, alpha, m] + truncated[j, alpha] = n_o(tau_j) N_alpha;  sum_m m lost[j, alpha, m] = sum_beta (bonds -
 * alive)[j, alpha, beta];  unbroken <= alive <= bonds (continuous = 1), exactly.
 * Optionally per atom (NULL: not asked for): alive_masks and unbroken_masks, each (n_lags, n_o(0), n_a) uint64 in list
 * order: bit i stands for the i-th neighbour in the order of psa_debug_neighbour_lists at the origin; 0 for a truncated
 * centre and for an origin outside O_tau_j; unbroken_masks is zeros when continuous = 0.
 * As evaluated (persist.hip): per block of origins the fraction pass and the neighbour pass of psa_angle_histogram; a tag
 * pass that keeps of every list the 64 tag words and sets the centre's survivor mask to its n low bits; then per visited
 * frame f -- with continuous = 1 every multiple of sample_step up to the last lag, else the listed lags alone -- the
 * fraction pass of the frames o + f for the origins of the block with o + f <= T-1 and a step pass in which a wavefront
 * takes a centre and lane i its i-th neighbour: it gathers the two atoms' fractions, runs the chain, the ballot is the alive
 * mask, the survivor mask is ANDed with it.  At a listed lag the per-species popcounts and the centre's lost count go by
 * 32-bit integer adds into counters in LDS -- the host keeps a workgroup's samples below 2^32 --, written to partials with
 * plain stores and summed in 64-bit integers into that lag's rows.  No global atomics, no float atomics; two identical
 * calls, any budget and any order of the atoms inside a species give the same bits.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block 1040 n_a bytes as for psa_angle_histogram, plus 288 n_a (the
 * tags 256, the lagged fractions 12, the survivor and the alive mask 8 each, 4 of padding); a budget below one origin is
 * refused and the refusal names the bytes needed.
 * PSA_EINVAL: everything psa_angle_histogram refuses about the context (a sharded one among it), the box, the species,
 * r_cut, origin_step and the budget; r_break below r_cut, not symmetric, not finite, beyond the served radius, or 0 where
 * r_cut is not (and the reverse); n_lags outside [1, 1024]; lags not strictly ascending, outside [0, T-1] or no multiple of
 * sample_step; sample_step < 1; continuous not 0 or 1; pair_bytes, lost_bytes, truncated_bytes or (with a per-atom output)
 * masks_bytes not exact; a null required argument.
 * Only the positions slot is read.  Atom weights and segments set on the context are ignored, not refused; every result
 * and plan of the other entry points is left as it is.  Stage times: [0] the tables' upload, [5] the origins' fraction
 * pass, [6] the neighbour pass, [1] the tag pass and every visited frame's fraction pass, step pass and reduce,
 * [7] device->host. */
int psa_bond_persistence(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                         const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */,
                         const double* r_break /* S*S */, int64_t origin_step, const int64_t* lags /* n_lags */, int32_t n_lags,
                         int64_t sample_step, int32_t continuous, uint64_t* bonds /* (n_lags, S, S) */,
                         uint64_t* alive /* the same */, uint64_t* unbroken /* the same */, size_t pair_bytes /* of each */,
                         uint64_t* lost /* (n_lags, S, 65) */, size_t lost_bytes, uint64_t* truncated /* (n_lags, S) */,
                         size_t truncated_bytes, uint64_t* alive_masks /* (n_lags, n_o(0), n_a) or NULL */,
                         uint64_t* unbroken_masks /* the same */, size_t masks_bytes /* of each */);

/* Common-neighbour analysis (Honeycutt and Andersen; Faken and Jonsson): the signature (j, k, l) of every bond of the
 * neighbour lists and the structure type -- fcc, hcp, bcc, icosahedral, other -- of every atom at every time origin, as
 * integers.
 * Inputs.  The positions slot as stored, H = box with its inverse, S <= 8 disjoint species (idx, group_start), r_cut (S, S)
 * and origin_step exactly as for psa_angle_histogram, under the same checks and refusals.  Origins o = 0, s, 2 s, ... <=
 * T-1, n_o = (T-1) / s + 1.
 * Neighbours and left-out centres.  The neighbours b_0, .., b_{n-1} of centre a at origin o are bit for bit those of
 * psa_angle_histogram, of all species together, in the order of psa_debug_neighbour_lists.  A (centre, origin) with more
 * than 64 neighbours is left out whole -- never its first 64 -- and counted in truncated[alpha].
 * Adjacency.  Two listed neighbours b_i in beta, b_j in gamma of a are bonded when the float32 chain stated at
 * psa_angle_histogram holds for them at that origin: min_image of their centred fractions, x = sqrt(r2) float32(1 /
 * r_cut[beta,gamma]), x < 1, every operation rounded once; r_cut[beta,gamma] = 0: no bond.  The chain is odd in e bit for
 * bit and r_cut is symmetric, so the adjacency is symmetric; it is "b_j is in b_i's list" wherever b_i's list is complete,
 * and it asks for no list of b_i's: a neighbour that is truncated itself changes nothing.
 * Signature of the bond a-b_i.  C_i: the listed neighbours of a that are bonded to b_i, the common neighbours.  j = |C_i|;
 * k = the number of bonds among the members of C_i; l = the number of bonds of the largest connected component of that bond
 * graph (the "longest chain" of the widely used implementations: a star of three bonds has l = 3, not 2).
 * Type of a centre with n neighbours that is not truncated:
 *     1 fcc    n = 12 and 12 x (4,2,1)
 *     2 hcp    n = 12 and 6 x (4,2,1) + 6 x (4,2,2)
 *     3 bcc    n = 14 and 8 x (6,6,6) + 6 x (4,4,4)
 *     4 ico    n = 12 and 12 x (5,5,5)
 *     0 other  anything else, n = 0 among it
 * Outputs, uint64.  signature_counts (S, 8, 16, 16): per species of the centre the bonds with signature (j, k, l), j < 8, k <
 * 16, l < 16, over all origins; signature_outside (S): the bonds whose signature does not fit.  type_counts (n_o, S, 5): the
 * centres of every species by type at every origin.  truncated (S).  Exactly:
 *     sum signature_counts[alpha] + signature_outside[alpha] = sum_beta sum_n n coord[alpha,beta,n] of psa_angle_histogram
 *     sum_t type_counts[o,alpha,t] + the centres of alpha truncated at o = N_alpha
 * Optionally per atom, in list order (NULL: not asked for): types (n_o, n_a) int32, -1 for a truncated centre; n (n_o, n_a)
 * int32, the true neighbour count (beyond 64 too); bond_signatures (n_o, n_a, 64) uint32: j | k << 8 | l << 16 of the bond
 * to the i-th neighbour in the order of psa_debug_neighbour_lists -- k and l clamped to 255 in this word (j <= 63 always;
 * such a bond lies outside the table in any case) --, 0xFFFFFFFF at and beyond n and for a truncated centre.
 * As evaluated (cna.hip): the fraction pass and the neighbour pass of psa_angle_histogram; a signature pass in which a
 * wavefront takes a centre and lane i its i-th neighbour: the lane gathers the neighbour's fractions once, the n (n - 1) / 2
 * pairs of neighbours go through rounds in which lane i tests (i, i + m mod n), m = 1 .. n / 2, each round's ballot sets both
 * ends' bits, and lane i ends with row i of the 64 x 64 adjacency as one 64-bit word; the rows are parked in LDS and the lane
 * derives its bond's signature with bit operations alone (a popcount, a flood over masks that pops every common neighbour
 * once: at most 64 steps); the type is five ballots.  Counts go by 32-bit integer adds into counters in LDS -- the host
 * keeps a workgroup's samples below 2^32 --, written to partials with plain stores and summed in 64-bit integers; a census
 * pass counts the types per origin and species by integer sums.  No global atomics, no float atomics, and nothing after the
 * adjacency is floating point: two identical calls, any budget, with or without the per-atom outputs and any order of the
 * atoms inside a species give the same bits.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block 1040 n_a bytes as for psa_angle_histogram, plus 8 n_a (the
 * types 4, 4 of padding), plus 256 n_a where bond_signatures is asked for; a budget below one origin is refused and the
 * refusal names the bytes needed.
 * PSA_EINVAL: everything psa_angle_histogram refuses about the context (a sharded one among it), the box, the species,
 * r_cut, origin_step and the budget; signature_bytes or type_bytes not exact; with types or n, atom_bytes not exact; with
 * bond_signatures, bond_bytes not exact; a null required output.
 * Only the positions slot is read.  Atom weights and segments set on the context are ignored, not refused; every result
 * and plan of the other entry points is left as it is.  Stage times: [0] the tables' upload, [5] the fraction pass, [6] the
 * neighbour pass, [1] the signature and the census pass, of these [2] the census pass, [4] reduce, [7] device->host.
 * Not served: diamond identification, signature tables resolved by the species pair of the bond (bond_signatures with the
 * lists give them on the host), cell lists, sharding.  Adaptive cut-offs per atom: psa_adaptive_common_neighbours. */
int psa_common_neighbours(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                          const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */,
                          int64_t origin_step, uint64_t* signature_counts /* (S, 8, 16, 16) */, size_t signature_bytes,
                          uint64_t* signature_outside /* S */, uint64_t* type_counts /* (n_o, S, 5) */, size_t type_bytes,
                          uint64_t* truncated /* S */, int32_t* types /* (n_o, n_a) or NULL */, int32_t* n /* the same */,
                          size_t atom_bytes /* of each */, uint32_t* bond_signatures /* (n_o, n_a, 64) or NULL */,
                          size_t bond_bytes);

/* Adaptive common-neighbour analysis (Stukowski, Modelling Simul. Mater. Sci. Eng. 20, 045021, 2012): the structure type of
 * every atom at every time origin with a cut-off of the atom's own, derived from its nearest candidates, so that r_cut is no
 * longer a radius to tune but a generous candidate radius: it must only contain the 14 nearest atoms (up to the third shell,
 * usually).
 * Inputs.  Exactly those of psa_common_neighbours, under the same checks and refusals; origins o = 0, s, 2 s, ... <= T-1.
 * Candidates.  The candidates of centre a at an origin are the list the neighbour pass of psa_angle_histogram leaves for
 * r_cut (a scalar or a symmetric (S, S) matrix, 0: not a candidate, nothing beyond max_pair_radius(box)), in the order of
 * psa_debug_neighbour_lists; n is the true count, at most 64 candidates are held.  Species play no part after this list.
 *   Truncated.  n > 64: the centre is left out whole: type -1, counted in truncated[alpha].
 *   Short.  n < 12: type other, no bonds, counted in short_centres[alpha].
 * Rank.  s_i = d_x^2 + d_y^2 + d_z^2 of leg i, float32, fma(d_z, d_z, fma(d_y, d_y, d_x d_x)): the same bits as the neighbour
 * pass's r2.  rank(i) = #{j : s_j < s_i} + #{j < i : s_j = s_i}: exact float compares on r2, no root; a tie goes to the earlier
 * list position (the lower atom column).  rho_k = sqrt(s), float32, of the candidate with rank k.
 * Test A (n >= 12).  The members are the ranks 0 .. 11.  L = rho_0 + .. + rho_11 added in ascending rank, each add rounded
 * once; r_A = L * float32(K / 12), K = (1 + sqrt 2) / 2; inv_A = 1.f / r_A, each rounded once.  Two members u, v are bonded
 * when the float32 chain stated at psa_angle_histogram gives x < 1 for them with inv_A: min_image of their centred
 * fractions, x = sqrt(r2) inv_A -- the chain of psa_common_neighbours on the same fractions, not a difference of legs (wrong
 * beyond half a box); a value that is not a number: no bond.  The signature (j, k, l) of each of the 12 bonds a-member is
 * psa_common_neighbours' own: the common neighbours among the members, the bonds among them, the bonds of the largest
 * connected component.  Type: fcc 12 x (4,2,1); hcp 6 x (4,2,1) + 6 x (4,2,2); ico 12 x (5,5,5); else other.
 * Test B (only where test A gave other and n >= 14).  The members are the ranks 0 .. 13.  P = rho_0 + .. + rho_7 and Q = rho_8
 * + .. + rho_13, each in ascending rank; L = P * float32(2 / sqrt 3) + Q, the product and the sum rounded once each (no fma);
 * r_B = L * float32(K / 14); inv_B = 1.f / r_B.  Type: bcc 8 x (6,6,6) + 6 x (4,4,4); else other.
 * Which bonds are counted.  A centre's counted bonds, and its per-atom rows, are those of the test that ran last: the 12 of A
 * or the 14 of B; its cut-off is that test's r.  Bonds and per-atom rows are indexed by rank, not by list position.
 * Everything after the adjacency is integers.  (Where rho_11 = rho_12 exactly -- the perfect bcc lattice -- test A's members
 * are decided by the tie rule; such a centre cannot come out fcc, hcp or ico there, and test B decides.)
 * Outputs, uint64.  signature_counts (S, 8, 16, 16) per species of the centre, over all origins; signature_outside (S): the
 * counted bonds whose signature does not fit (k up to 78 among 14 members); type_counts (n_o, S, 5): other, fcc, hcp, bcc,
 * ico; truncated (S); short_centres (S).  Exactly:
 *     sum_t type_counts[o,alpha,t] + the centres of alpha truncated at o = N_alpha
 *     sum signature_counts[alpha] + signature_outside[alpha] = 12 #(centres of alpha whose last test is A) + 14 #(B)
 * Optionally per atom, in list order (NULL: not asked for): types (n_o, n_a) int32, -1 for a truncated centre; n (n_o, n_a)
 * int32, the true candidate count (beyond 64 too); cutoffs (n_o, n_a) float32, the r of the test that ran last, NaN where no
 * test ran (truncated, short); nearest (n_o, n_a, 14) int32, the members' atom columns by rank, -1 beyond the members of the
 * last test; bond_signatures (n_o, n_a, 14) uint32, j | k << 8 | l << 16 of the bond to the member of that rank, 0xFFFFFFFF
 * where there is no bond.
 * As evaluated (acna.hip): the fraction pass and the neighbour pass of psa_angle_histogram; a pass in which a wavefront takes
 * a centre and lane i its i-th candidate, loaded as one float4: the 64 s_i are parked in LDS and every lane counts its rank
 * from same-address broadcast reads; a lane with a rank below 14 writes the candidate's fractions, column and rho to LDS slot
 * `rank`, lanes 0 .. 13 then are the members; the pairs of members go through the leg-pair rounds of psa_common_neighbours
 * with 12 members, then where test B runs with 14 (the branch is uniform over the wavefront); rows of the adjacency as 32-bit
 * words in LDS, the flood over masks and the type ballots as there; counts by 32-bit integer adds in LDS, partials with plain
 * stores, summed in 64-bit integers; psa_common_neighbours' census pass on the types.  No global atomics, no float atomics:
 * two identical calls, any budget, with or without the per-atom outputs give the same bits; so does any order of the atoms
 * inside a species on the counts and the types, and on the bonds as sets of (centre, member, word) -- the rank labels of
 * candidates whose r2 are exactly tied follow the list order.
 * Budget (PSA_OPT_DYNAMIC_WORK_BYTES): per origin of a block 1040 n_a bytes as for psa_angle_histogram, plus 12 n_a (the
 * types 4, 4 of padding, the cut-offs 4), plus 112 n_a where nearest or bond_signatures is asked for; a budget below one origin
 * is refused and the refusal names the bytes needed.
 * PSA_EINVAL: everything psa_common_neighbours refuses about the context (a sharded one among it), the box, the species,
 * r_cut, origin_step and the budget; signature_bytes or type_bytes not exact; with types, n or cutoffs, atom_bytes not exact
 * (4 n_o n_a); with nearest or bond_signatures, bond_bytes not exact (56 n_o n_a); a null required output.  Byte counts of
 * outputs not asked for are not read.
 * Only the positions slot is read; every result and plan of the other entry points is left as it is.  Stage times as for
 * psa_common_neighbours.
 * Not served: diamond identification, signature tables per species pair, cell lists, sharding. */
int psa_adaptive_common_neighbours(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                                   const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */,
                                   int64_t origin_step, uint64_t* signature_counts /* (S, 8, 16, 16) */, size_t signature_bytes,
                                   uint64_t* signature_outside /* S */, uint64_t* type_counts /* (n_o, S, 5) */, size_t type_bytes,
                                   uint64_t* truncated /* S */, uint64_t* short_centres /* S */,
                                   int32_t* types /* (n_o, n_a) or NULL */, int32_t* n /* the same */, float* cutoffs /* the same */,
                                   size_t atom_bytes /* of each */, int32_t* nearest /* (n_o, n_a, 14) or NULL */,
                                   uint32_t* bond_signatures /* the same */, size_t bond_bytes /* of each */);

/* Pair folding (PSA_OPT_FOLD_PAIRS) as a service for callers that split a k-list themselves
 * (psa_amd/dist.py): kmap[i] = row of k-vector i among the n_unique vectors that need projecting
 * (unique_idx[r] = position of row r's vector in the input list), with bit 31 set when vector i is
 * the exact negation of that row's vector.  No context, no GPU. */
#define PSA_KMAP_MIRROR 0x80000000u
int psa_k_pairs(const float* k_vectors, int64_t K, int32_t* kmap /* K */,
                int32_t* unique_idx /* K, first n_unique valid */, int64_t* n_unique);
/* ... and the map of a result whose slab rows the caller projected from the folded list (every rank
 * that finalizes installs it after its psa_sed_project / psa_sed_gather): psa_sed_finalize then
 * returns K_out columns, column i from slab row kmap[i] & ~PSA_KMAP_MIRROR, mirrored in frequency
 * and conjugated where bit 31 is set. */
int psa_sed_set_kmap(psa_ctx* ctx, const int32_t* kmap, int64_t K_out);

/* The low-rank plan of a k-list for one atom group (api_lowrank.hip) as a host-only service for tests:
 * *ok = 1 when the route serves; geo[14] = u (3), k0 (3), x_c, h_x, interval width, interval id, bound on
 * |D|, scale of D, bound on |E| and scale of the folded image D + E (psa_set_k1_lowrank_fold); kappa[64] the nodes, L[K * 64] the combine's real Lagrange weights and phi[K * 2] its complex64
 * row phases, C[K * 64 * 2] complex64 their product phi[j] L[j, l] rounded once from fp64: the reference the two
 * factors are checked against, which no kernel reads (any may be null).  No context, no GPU. */
int psa_lowrank_plan(const float* k_vectors, int64_t K, const float* mean_pos_all, int64_t N, const int32_t* idx,
                     int64_t n_g, int32_t* ok, double* geo, double* kappa, float* C, float* L, float* phi);
/* The same for a plan of `nodes` = 48 or 64 nodes (psa_set_k1_lowrank_nodes): kappa[nodes], L[K * nodes], C[K * nodes * 2];
 * geo[15], the 14 values above -- e_bound from this plan's L; with 48 nodes the scale of the image from d_bound + e_bound +
 * 1e-6, the cap on r_bound a launch uses -- and r_bound, with 48 nodes the fp64 maximum over the rows and the group's atoms
 * of |P_line - phi L W| (W the node rows in fp64, L and phi the float32 tables), 0 with 64. */
int psa_lowrank_plan_nodes(const float* k_vectors, int64_t K, const float* mean_pos_all, int64_t N, const int32_t* idx,
                           int64_t n_g, int32_t nodes, int32_t* ok, double* geo, double* kappa, float* C, float* L, float* phi);

/* One (k, omega) bin: S[c] = FFT_t(q)[i_w] / T for ONE k-vector and one atom group, as 3
 * complex64 -- what iSED consumes of a group's spectrum (sed_calculator.py:483, :494-499: only
 * sed[i_w, i_k, :] of the full path spectrum is used).  One pass over the trajectory and one DFT
 * dot instead of K projections and 3K FFTs.  idx NULL = all atoms. */
int psa_sed_single_bin(psa_ctx* ctx, int slot, const float* mean_pos_all, const float* k_vector,
                       const int32_t* idx, int64_t n_g, int32_t flags, int64_t i_w,
                       float* out_c64x3 /* 6 floats */);

/* Raw access to rows [row0, row0+nrows) of the k-major slab (complex64 (nrows,3,T) or float32
 * (nrows,T), whichever the last psa_sed_project produced; (nrows,L) float32 under psa_set_segments): lets a host transport stand in for
 * psa_sed_gather when no RCCL communicator can be formed, and serves checkpointing. */
int psa_slab_read(psa_ctx* ctx, int64_t row0, int64_t nrows, void* host);
int psa_slab_write(psa_ctx* ctx, int64_t row0, int64_t nrows, const void* host);

/* SED.intensity of the finalized complex result, (T,K) float32 = sum_c |S|^2 (src/psa/core/sed.py:22-24):
 * psa_sed_finalize / psa_sed_calculate leave it on the device next to the result; this copies it out
 * (out_host NULL: only makes sure it exists). */
int psa_result_intensity(psa_ctx* ctx, float* out_host /* (T,K) */, size_t out_bytes);
/* chiral phase, option "C", of components (c1, c2) of the finalized complex
 * result: (T,K) float32           (sed_calculator.py:344-350) */
int psa_result_chiral_phase(psa_ctx* ctx, int c1, int c2, float* out_host, size_t out_bytes);

/* stage timings of the last project/finalize on this context, milliseconds:
 * [0] host->device uploads  [1] phase table  [2] projection  [3] FFT
 * [4] |.|^2 / scale epilogue  [5] gather (RCCL)  [6] transpose  [7] device->host */
int psa_last_timings(psa_ctx* ctx, double* ms /* [8] */);
/* number of projection-kernel launches and their summed duration (HIP events on
 * the context's stream) since the last call of this function */
int psa_k1_stats(psa_ctx* ctx, int64_t* launches, double* total_ms);
/* projection launches of the context's life that took the low-rank route for k-paths (PSA_OPT_K1_LOWRANK) */
int psa_k1_lowrank_launches(psa_ctx* ctx, int64_t* launches);
/* ... of which the single pair launch served node rows and D rows (PSA_OPT_K1_LOWRANK_PAIR) */
int psa_k1_lowrank_pair_launches(psa_ctx* ctx, int64_t* launches);
/* The D image of that launch (k1_lowrank_pair.h) as a host-only service for tests: bytes = its size for n_stage 32-atom
 * stages, padding included; index[512 * 32 n_stage] (may be null) = the float16 element index of (row m, atom a) at
 * m * 32 n_stage + a.  No context, no GPU. */
int psa_lowrank_pair_image(int32_t n_stage, int64_t* index, int64_t* bytes);
/* The same for the folded D image of the folded pair launch (k1_lowrank_fold.h, psa_set_k1_lowrank_fold): rows 0..127 in
 * role A's part, rows 128..511 in role B's.  No context, no GPU. */
int psa_lowrank_fold_image(int32_t n_stage, int64_t* index, int64_t* bytes);
/* ... and for the D image of the 48-node pair launch (k1_lowrank_n48.h, psa_set_k1_lowrank_nodes): rows 0..159 in role A's
 * part, rows 160..511 in role B's.  No context, no GPU. */
int psa_lowrank_n48_image(int32_t n_stage, int64_t* index, int64_t* bytes);
/* Device allocations the library's contexts hold at this moment, process-wide: how many and their bytes.  A destroyed
 * context leaves none behind.  No context, no GPU. */
int psa_debug_device_buffers(int64_t* count, int64_t* bytes);
/* The table of the context's device buffers (api_core.hip), row by row: the member's name and what its bytes are read
 * as; either may be null.  PSA_EINVAL past the last row.  No context, no GPU.
 *   PSA_SCRATCH_REAL   only as float, float16, complex, double or counters that are only added to
 *   PSA_SCRATCH_INDEX  in part as an index, an offset, an address or a loop bound
 *   PSA_SCRATCH_STATE  it carries something a later call is promised: atom weights, the segment window, a cached table */
#define PSA_SCRATCH_REAL 0
#define PSA_SCRATCH_INDEX 1
#define PSA_SCRATCH_STATE 2
int psa_debug_scratch_info(int index, const char** name, int32_t* cls);
/* Shows that no result depends on what scratch memory held before.  Drains the context's streams, then sets every byte of
 * every REAL buffer's whole capacity to `byte` (0 .. 255; 0xFF is a NaN in float16, float32 and float64) and every byte
 * of every INDEX buffer to 0, whatever `byte` is: a pattern never reaches anything a kernel turns into an address or a
 * trip count.  STATE buffers, the data slots and the plane sets that exist are left alone.  The result resident on the
 * device is dropped with its buffers: psa_sed_finalize and psa_result_* answer as after psa_create.  buffers, bytes (may
 * be null): how many buffers were filled and their bytes.  The call also ARMS the context: until byte = -1 disarms it
 * (and fills nothing), every REAL or INDEX buffer the context allocates or grows, and every plane set it builds, is
 * filled the same way before its first use.  Between a call that begins a sequence (psa_sed_project, psa_sed_fs_project)
 * and the one that ends it, the sequence's intermediate results go the same way.  Not for production: a context that
 * was never armed pays one pointer test per reservation. */
int psa_debug_scratch_fill(psa_ctx* ctx, int byte, int64_t* buffers, int64_t* bytes);
/* host wall clock (ms) of work that is done once and then cached, summed since the last call:
 * [0] rocFFT plan builds (run-time compiled per (T, batch))  [1] largest-magnitude passes
 * [2] split-plane builds  [3] trajectory uploads (psa_data_upload / psa_sed_project_upload) */
int psa_oneoff_stats(psa_ctx* ctx, double* ms /* [4] */);

/* diagnostics for tests: the phase table of one group as (K,N_g) complex64, and the
 * pre-FFT projection q as (K,3,T) complex64 */
int psa_debug_phase_table(psa_ctx* ctx, const float* mean_pos_all,
                          const float* k_vectors, int64_t K,
                          const int32_t* idx, int64_t n_g, int64_t N,
                          void* out_host);
int psa_debug_project_only(psa_ctx* ctx, int slot, const float* mean_pos_all,
                           const float* k_vectors, int64_t K,
                           const int32_t* idx, int64_t n_g, int32_t flags,
                           void* out_host);
/* the same over all frames, launched as psa_sed_project launches a list that consists of these K vectors: it takes the
 * low-rank route for k-paths (PSA_OPT_K1_LOWRANK) where that call would, and psa_k1_lowrank_launches counts it.  The
 * list is taken as it is: not folded ((k, -k) pairs, twins) and not cut into k-blocks.
 * psa_debug_project_only and psa_debug_project_frames never take that route. */
int psa_debug_project_route(psa_ctx* ctx, int slot, const float* mean_pos_all,
                            const float* k_vectors, int64_t K,
                            const int32_t* idx, int64_t n_g, int32_t flags,
                            void* out_host);
/* psa_debug_project_only for frames [t_begin, t_begin + t_count) only, written into those columns of a zeroed
 * (K,3,T) slab (what a frame-sharded or streaming projection does per piece) */
int psa_debug_project_frames(psa_ctx* ctx, int slot, const float* mean_pos_all,
                             const float* k_vectors, int64_t K,
                             const int32_t* idx, int64_t n_g, int32_t flags,
                             int64_t t_begin, int64_t t_count, void* out_host);
/* the contraction kernel of psa_sed_modes alone, on spectra the caller uploads: S_host (B,K,3,T) complex64 taken as
 * they are (no division by T), eig (K,M,B,3) complex64 -> out_host (T,K,M) float32 = |sum_{b,c} conj(eig) S|^2 */
int psa_debug_mode_power(psa_ctx* ctx, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t T,
                         float* out_host);
/* the covariance kernels of psa_sed_covariance alone, on spectra the caller uploads: S_host (B,K,3,T) complex64 taken as
 * the transforms S_b (used as given), freq_weights (n_w,T), out_host (n_w,K,3B,3B) complex128 = scale sum_w g S S^+ */
int psa_debug_covariance(psa_ctx* ctx, const void* S_host /* (B, K, 3, T) complex64, used as given */, int32_t B, int64_t K,
                         int64_t T, const float* freq_weights, int32_t n_w, double scale, double* out_host);
/* the contraction kernel of psa_sed_modes_welch alone, on transformed segments the caller uploads: S_host (B,K,3,ns,L)
 * complex64 taken as they are, eig (K,M,B,3) complex64 -> out_host (L,K,M) float32 = sum_s scale |sum_{b,c} conj(eig) S_s|^2.
 * seg_block = 0: one launch; seg_block > 0: launches of at most that many segments, the later ones adding to the result
 * of the earlier (the path a budget-bound call takes) */
int psa_debug_mode_power_welch(psa_ctx* ctx, const void* S_host, const void* eig, int32_t B, int64_t K, int64_t M, int64_t L,
                               int64_t ns, int64_t seg_block, float scale, float* out_host);
/* the kernel of psa_dynamic_spectra alone, block by block under the same budget rule: out_host (K, NC, T) complex64,
 * NC = currents ? 4 : 1, the projections q before the window and the FFT (the context's segments only enter the
 * block size) */
int psa_debug_dynamic_project(psa_ctx* ctx, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g,
                              int32_t currents, void* out_host);
/* the sine and cosine of that kernel on n arguments in turns (|x| <= 2): out_host (n, 2) float32 = sin, cos of 2 pi x */
int psa_debug_dynamic_sincos(psa_ctx* ctx, const float* turns, int64_t n, float* out_host);
/* the projection kernel of psa_lattice_spectra alone (per-vector form), block by block under the same budget rule:
 * out_host (K, NC, T) complex64 in the caller's order, NC = currents ? 4 : 1 */
int psa_debug_lattice_project(psa_ctx* ctx, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx,
                              int64_t n_g, int32_t currents, void* out_host);
/* the series kernel of psa_self_spectra alone (per-vector form), block by block under the same budget rule, before the
 * window and the FFT (one boxcar segment of all T frames whatever segments the context holds): out_host (n_g, K, T)
 * complex64, atoms in the order of the set, vectors in the caller's order */
int psa_debug_self_series(psa_ctx* ctx, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx,
                          int64_t n_g, void* out_host);
/* The passes that follow the FFT in the three families above, alone, on TRANSFORMED segments the caller uploads (no
 * projection, no window, no FFT): each entry cuts the call into sub-blocks as its family's run does and goes through the
 * same host code and the same launches, so what it returns is what the run would make of these segments.  A block
 * argument of 0 means "all at once".  PSA_EINVAL: a null pointer, a size that is not positive, a negative block, an input
 * beyond 2^28 elements per sub-block, and what each entry names below.  They use their family's device buffers, which
 * hold nothing between calls.
 *   psa_debug_dynamic_power  the power pass of psa_dynamic_spectra (and of the per-vector form of psa_lattice_spectra):
 *       seg_host (K, NC, n_seg, L) complex64, NC = currents ? 4 : 1; k / |k| is formed from k_vectors as psa_dynamic_spectra
 *       forms it; out_host (currents ? 3 : 1, L, K) float32 = scale sum_s (density, longitudinal, transverse), the sum over
 *       the segments of a sub-block in one float32 chain, later sub-blocks added in float32.  Refused: k_vectors not finite.
 *   psa_debug_lattice_shell  the shell and finish passes of psa_lattice_spectra: the same seg_host with the vectors in the
 *       processing order, bin_of (K) ascending, khat (K, 3) float32 as given (may be NULL without currents); the scale of bin
 *       b is 1 / (2 n_b norm), norm = n_seg U L^2 as one double, an empty bin gives zeros; out_host (3 or 1, L, n_bins).
 *       Refused: bin_of outside [0, n_bins) or descending, norm not positive, khat not finite.
 *   psa_debug_self_power     the power, reduce and finish passes of psa_self_spectra: work_host (na, nv, n_seg, L)
 *       complex64; groups (2 (n_groups + 1)) int32: per column group its first vector and its column of the result, the
 *       last pair (nv, 0) -- a shell per group with mirror = 1, or one vector per group and any permutation of the
 *       columns with mirror = 0; scale (cols) float64; n_chunks: chunks of a block's atoms, 0 = the rule of the run;
 *       out_host (L, cols) float32.  Refused: groups that do not tile [0, nv) in ascending order, a column outside
 *       [0, cols) or used twice, n_chunks above 65535. */
int psa_debug_dynamic_power(psa_ctx* ctx, const void* seg_host, const float* k_vectors /* (K,3) */, int64_t K, int32_t currents,
                            int64_t n_seg, int64_t L, int64_t k_block, int64_t seg_block, float scale, float* out_host);
int psa_debug_lattice_shell(psa_ctx* ctx, const void* seg_host, const float* khat /* (K,3) */, const int32_t* bin_of /* K */,
                            int64_t K, int64_t n_bins, int32_t currents, int64_t n_seg, int64_t L, int64_t k_block,
                            int64_t seg_block, double norm, float* out_host);
int psa_debug_self_power(psa_ctx* ctx, const void* work_host, int64_t na, int64_t nv, int64_t n_seg, int64_t L,
                         const int32_t* groups, int64_t n_groups, int64_t cols, const double* scale, int32_t mirror,
                         int64_t n_chunks, int64_t atom_block, int64_t vec_block, int64_t seg_block, float* out_host);
/* the projections of psa_partial_spectra alone (per-vector form), block by block under the same budget rule: out_host
 * (K, S, NC, T) complex64 in the caller's order, NC = currents ? 4 : 1 */
int psa_debug_partial_project(psa_ctx* ctx, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx,
                              const int64_t* species_start, int32_t n_species, int32_t currents, void* out_host);
/* the pair pass of psa_partial_spectra alone on TRANSFORMED segments seg_host (K, S, NC, n_seg, L) complex64, through the
 * host loop of the run, as the three entries above: khat (K, 3) float32 as given (may be NULL without currents); norm =
 * n_seg U L^2 as one double.  bin_of == NULL: the per-vector form, out_host (1 or 3, P, L, K), the scale (float)(1 / norm).
 * bin_of (K) ascending: the shell and finish passes, the vectors in the processing order, out_host (1 or 3, P, L, n_bins),
 * the scale of bin b 1 / (2 n_b norm).  Refused: what psa_debug_lattice_shell refuses, and S outside [1, 8]. */
int psa_debug_partial_power(psa_ctx* ctx, const void* seg_host, const float* khat /* (K,3) */, const int32_t* bin_of /* K or NULL */,
                            int64_t K, int64_t n_bins, int32_t n_species, int32_t currents, int64_t n_seg, int64_t L,
                            int64_t k_block, int64_t seg_block, double norm, float* out_host);
/* number of plane sets in the cache and their bytes */
int psa_debug_plane_cache(psa_ctx* ctx, int64_t* n_sets, int64_t* bytes);

/* ---- k-point sharding over the GPUs of a node (one process per GPU) ------
 * rank 0 calls psa_comm_unique_id and ships the 128 bytes to the other ranks by
 * any host channel; every rank then calls psa_comm_init.  psa_sed_gather moves each
 * rank's rows of the slab to `root` over RCCL (xGMI) -- or to every rank when root is
 * -1 -- as grouped point-to-point transfers; k_offsets/k_counts are the (nranks) row
 * ranges.  After it, the receiving rank(s) call psa_sed_finalize. */
#define PSA_UNIQUE_ID_BYTES 128
int psa_comm_unique_id(void* out /* PSA_UNIQUE_ID_BYTES */);
int psa_comm_init(psa_ctx* ctx, const void* unique_id, int rank, int nranks);
int psa_comm_destroy(psa_ctx* ctx);
/* every pair of ranks trades one small stamped block in the grouped point-to-point pattern the
 * data path uses; PSA_ERCCL if anything arrives damaged.  Collective: all ranks call it. */
int psa_comm_selftest(psa_ctx* ctx);
int psa_sed_gather(psa_ctx* ctx, int root, const int64_t* k_offsets, const int64_t* k_counts);
int psa_comm_barrier(psa_ctx* ctx);

/* ---- frame sharding: one exchange step before the FFT -------------------------------
 * The projection is linear in atoms and independent per frame (sed_calculator.py:80-81), the FFT
 * runs along frames (:83).  Rank r holds only frames [t_offsets[r], +t_counts[r]) of the
 * trajectory in its slot (1/n of the array), projects ALL K k-vectors on them, then an
 * all-to-all over RCCL hands every rank the frames it lacks of ITS block of k rows
 * [k_offsets[r], +k_counts[r]); FFT and epilogue run on those rows, which end up in the same
 * k-major slab rows as with k-sharding -- psa_sed_gather / psa_sed_finalize follow unchanged.
 * Per atom group (G groups need PSA_F_INTENSITY as usual):
 *     psa_sed_fs_project   q_local (K_total,3,T_local) of the group, on the device
 *     psa_sed_fs_exchange  the all-to-all (grouped ncclSend/ncclRecv, direct links)
 *                          -- or psa_sed_fs_read / psa_sed_fs_write when a host transport stands in
 *     psa_sed_fs_finish    FFT over T_total of my rows, then complex rows into the slab or
 *                          |.|^2 accumulated into it (first_group: overwrite) */
int psa_sed_fs_project(psa_ctx* ctx, int slot, const float* mean_pos_all,
                       const float* k_vectors, int64_t K_total,
                       const int32_t* idx, int64_t n_g, int32_t flags,
                       int64_t T_total, int64_t k_offset, int64_t k_count);
int psa_sed_fs_exchange(psa_ctx* ctx, const int64_t* t_offsets, const int64_t* t_counts,
                        const int64_t* k_offsets, const int64_t* k_counts);
/* rows [k0, k0+nk) of q_local as (nk,3,T_local) complex64 */
int psa_sed_fs_read(psa_ctx* ctx, int64_t k0, int64_t nk, void* host);
/* frames [t0, t0+nt) of my rows, (k_count,3,nt) complex64 */
int psa_sed_fs_write(psa_ctx* ctx, int64_t t0, int64_t nt, const void* host);
int psa_sed_fs_finish(psa_ctx* ctx, int32_t first_group);

/* the back-transform of psa_lattice_correlations and psa_self_correlations alone, through the launch helper the runs use:
 * X_host (fields, P, cols) float64 -- with as_float32 = 1 rounded to float32 first, the per-vector pass's type -- ->
 * out_host (fields, n_lags, cols) float32 = 1 / (P n_seg (L - t)) sum_o X[f,o,col] cos(2 pi o t / P).  Any P >= 1, not only
 * powers of two.  PSA_EINVAL: a null pointer, fields outside [1, 3], P outside [1, 2^30], a size that is not positive,
 * n_lags outside [1, min(L, P)], a non-finite value, more than 2^28 elements. */
int psa_debug_correlation_transform(psa_ctx* ctx, const double* X_host, int64_t fields, int64_t P, int64_t cols, int64_t L,
                                    int64_t n_seg, int64_t n_lags, int32_t as_float32, float* out_host);

/* the unwrap pass of psa_displacement_moments and psa_van_hove_self alone, block by block under the same budget rule:
 * out_u (T, n_g, 3) float64 the unwrapped displacements of the atoms idx (NULL: all N), out_images (T, n_g, 3) int32 the
 * image counts n (may be NULL).  PSA_EINVAL: what those entries refuse about the context, the box, the indices, unwrap
 * and the budget. */
int psa_debug_unwrap(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx, int64_t n_g,
                     int32_t unwrap, double* out_u /* (T, n_g, 3) */, int32_t* out_images /* (T, n_g, 3) or NULL */);

/* the fraction pass of psa_pair_histogram alone, frame block by frame block under the same budget rule: out (T, n_g, 3)
 * float32 the centred fractional coordinates c of the atoms idx (NULL: all N).  PSA_EINVAL: what that entry refuses about
 * the context, the inverse, the indices and the budget. */
int psa_debug_pair_fractions(psa_ctx* ctx, const double* box_inverse /* 9 */, const int32_t* idx, int64_t n_g,
                             float* out /* (T, n_g, 3) */);

/* the workgroup table psa_pair_histogram builds for species of these sizes over a block of n_origins <= 65535 origins
 * (sym = 1: lag 0), on the host alone, no context: out[0] the most beta-tiles an item walks, out[1] the origin slabs,
 * out[2] the items, out[3] the most samples one item can count (256 x its beta-atoms x its origins), which stays below
 * 2^32.  PSA_EINVAL: a null pointer, n_groups outside [1, 8], a negative size, n_origins outside [1, 65535]. */
int psa_debug_pair_plan(const int64_t* sizes /* n_groups */, int32_t n_groups, int32_t sym, int64_t n_origins, int64_t* out /* 4 */);

/* the fraction pass and the neighbour pass of psa_angle_histogram alone at one frame in [0, T-1]: count (n_a) int32 the
 * true number of neighbours of every listed atom (it may exceed 64), list (n_a, 64) int32 the list positions of its
 * first 64 neighbours in ascending order, padded with -1.  PSA_EINVAL: what that entry refuses about the context, the
 * box, the species, r_cut and the budget; a frame outside [0, T-1]. */
int psa_debug_neighbour_lists(psa_ctx* ctx, const double* box /* 9 */, const double* box_inverse /* 9 */, const int32_t* idx,
                              const int64_t* group_start /* S+1 */, int32_t n_groups, const double* r_cut /* S*S */, int64_t frame,
                              int32_t* count /* n_a */, int32_t* list /* (n_a, 64) */);

#ifdef __cplusplus
}
#endif
#endif /* PSA_HIP_H */
