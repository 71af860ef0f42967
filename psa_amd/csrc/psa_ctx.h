// Internal declarations shared by the translation units of libpsa_hip.so.
// Public surface: include/psa_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "psa_hip.h"

namespace psa {

void set_error(const char* fmt, ...);

#define PSA_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            psa::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                           hipGetErrorString(e_));                                       \
            return PSA_EHIP;                                                             \
        }                                                                                \
    } while (0)

#define PSA_FFT_CHECK(expr)                                                              \
    do {                                                                                 \
        rocfft_status s_ = (expr);                                                       \
        if (s_ != rocfft_status_success) {                                               \
            psa::set_error("%s:%d: %s -> rocfft_status %d", __FILE__, __LINE__, #expr,   \
                           (int)s_);                                                     \
            return PSA_EFFT;                                                             \
        }                                                                                \
    } while (0)

#define PSA_NCCL_CHECK(expr)                                                             \
    do {                                                                                 \
        ncclResult_t r_ = (expr);                                                        \
        if (r_ != ncclSuccess) {                                                         \
            psa::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                           ncclGetErrorString(r_));                                      \
            return PSA_ERCCL;                                                            \
        }                                                                                \
    } while (0)

#define PSA_REQUIRE(cond, ...)                                                           \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            psa::set_error(__VA_ARGS__);                                                 \
            return PSA_EINVAL;                                                           \
        }                                                                                \
    } while (0)

#define PSA_TRY(expr)                                                                    \
    do {                                                                                 \
        int rc_ = (expr);                                                                \
        if (rc_ != PSA_OK) return rc_;                                                   \
    } while (0)

// grow-only device allocation, freed with its owner (release: the early free).  Every live one is counted, process-wide
// (psa_debug_device_buffers).  fill: null, or -- while psa_debug_scratch_fill has the owner armed -- the byte every new
// allocation is set to over its whole capacity before its first use; it belongs to the member, a move leaves it behind
struct DevBuf {
    void*  ptr = nullptr;
    size_t cap = 0;
    const int* fill = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            ptr = std::exchange(o.ptr, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return static_cast<T*>(ptr); }
};

// a rocFFT plan and its execution info, destroyed (info, then plan) with their owner
struct FftPlan {
    rocfft_plan           plan = nullptr;
    rocfft_execution_info info = nullptr;
    size_t                work_bytes = 0;
    FftPlan() = default;
    FftPlan(FftPlan&& o) noexcept
        : plan(std::exchange(o.plan, nullptr)), info(std::exchange(o.info, nullptr)), work_bytes(std::exchange(o.work_bytes, 0)) {}
    FftPlan& operator=(FftPlan&& o) noexcept {
        std::swap(plan, o.plan);
        std::swap(info, o.info);
        std::swap(work_bytes, o.work_bytes);
        return *this;
    }
    ~FftPlan();
};

struct DataSlot {
    DevBuf  buf;
    int64_t T = 0, N = 0;
    bool    valid = false;
    uint64_t generation = 0;             // bumped whenever the contents change
    // largest |x| of the array (float bits), computed on first use after the contents change
    bool     absmax_known = false;
    unsigned absmax_bits = 0;
    // ... and per column block of 32 atoms (host copy), for index-list groups
    bool                  blocks_known = false;
    std::vector<unsigned> block_absmax;
};

// stage timing: event pairs recorded on the context's stream, resolved lazily
struct Timed {
    int        stage;
    hipEvent_t e0, e1;
};
struct TimingState {
    std::vector<hipEvent_t> pool;
    std::vector<Timed>      pending;
    double                  acc[8] = {};
    int64_t                 k1_launches = 0;
    double                  k1_ms = 0.0;
};

// P' (phase table) lives in HBM as the LDS tile images the projection kernel DMAs in:
//   [M block][atom stage][row in block][K1_PROW floats: 32 atoms + 4 pad]
constexpr int K1_BA   = 32;   // atoms per LDS stage
constexpr int LOWRANK_NODES = 64;   // node rows of the low-rank route for k-paths (api_lowrank.hip)
constexpr int K1_VROW = 96;   // floats per staged V row (32 atoms x 3 components)
constexpr int K1_PROW = 36;   // floats per staged P' row (odd number of 16-byte slots)

__host__ __device__ inline size_t p_tile_index(int m, int a, int m_blk, int n_stage) {
    return ((size_t)(m / m_blk) * n_stage + (a / K1_BA)) * ((size_t)m_blk * K1_PROW) +
           (size_t)(m % m_blk) * K1_PROW + (a % K1_BA);
}
inline size_t p_table_floats(int M_pad, int A_pad) { return (size_t)M_pad * (A_pad / K1_BA) * K1_PROW; }

// the kernel family a projection launch goes to (make_geom in api_project.hip decides)
enum class K1Family : int {
    f32 = 0,          // the float32 kernels (k1_mfma.hip, k1_wave.hip)
    f16_fly = 2,      // "2 x f16", split on the fly (k1_pair.hip)
    bf16 = 3,         // "3 x bf16" (k1_split.hip)
    f16_planes = 4,   // "2 x f16" from the group's cached split planes (k1_planes*.hip)
};

// geometry of one projection launch (see k1_mfma.hip)
struct ProjGeom {
    int64_t T = 0;        // frames of this launch
    int64_t q_stride = 0; // frames per row of the q slab the launch writes into (>= T)
    int64_t N_tot = 0;    // atoms in the resident array
    int     n_g = 0;      // atoms in this group
    int     A_pad = 0;    // n_g rounded up to the atom stage (32)
    int     K = 0;        // k-vectors (rows of the output)
    int     M_pad = 0;    // 2K rounded up to the variant's M block
    int     m_blk = 0;    // rows of P per workgroup (variant)
    K1Family split = K1Family::f32;
    float   vscale = 0.f; // the "2 x f16" families: power of two applied to d (from the slot's or the planes' largest magnitude)
    bool    lowrank = false;  // f16_planes through the low-rank route for k-paths (api_lowrank.hip, k1_planes_diff.hip)
    int     M_pad_d = 0;      // lowrank: rows of the D image (2K rounded up to 512)
    float   dscale = 0.f;     // lowrank: power of two the D image carries
    bool    lr_pair = false;  // lowrank: node rows and D rows in one launch (k1_lowrank_pair.hip; PSA_OPT_K1_LOWRANK_PAIR)
    bool    lr_fold = false;  // lowrank: the node table's lo piece folded into the D image, two-product node rows (psa_set_k1_lowrank_fold;
                              // dscale is then the plan's dscale_fold)
    int     lr_nodes = 64;    // lowrank: Chebyshev nodes of the plan, 64 or -- only with lr_fold -- 48 (psa_set_k1_lowrank_nodes:
                              // the 48-node tables and k1_lowrank_n48.hip)
    // per-atom weights (psa_set_atom_weights), folded into the phase table: (N_tot) float32 on the device, indexed like
    // the mean positions; nullptr = none.  The float16 tables hold w 2^-e and their launches multiply qscale by
    // wscale = 2^e (the float32 and bf16 tables hold w itself)
    const float* weights = nullptr;
    float        wscale = 1.f;
};

// A group's data as cached split planes (k1_f16.h plane_index): built from one generation of one
// slot, for one atom list (or all atoms), with one power-of-two scale.
struct PlaneSet {
    DevBuf               buf;
    int                  slot = 0;
    uint64_t             generation = 0;
    bool                 all_atoms = true;
    std::vector<int32_t> idx;            // the atom list (compacted order), empty when all_atoms
    uint64_t             idx_hash = 0;
    bool                 displaced = false;   // the planes hold slot - mean (displacement mode)
    std::vector<float>   mean;                // ... with this mean (N,3)
    int64_t              T = 0, n_fg = 0;
    int                  n_g = 0, A_pad = 0;
    float                vscale = 0.f;
    uint64_t             last_use = 0;
};

// Entry of a k map (psa_ctx::kmap): output column k takes slab row (entry & ~KMAP_MIRROR); with
// KMAP_MIRROR set that row belongs to -k and is read as conj S[(T-w) mod T]  (k2_epilogue.hip)
constexpr int KMAP_MIRROR = (int)0x80000000u;

// page-locked staging buffers + copy stream of the host->device pipeline (psa_data_upload,
// psa_sed_project_upload)
struct Stager {
    void*       pin[2] = {nullptr, nullptr};
    size_t      cap = 0;
    hipEvent_t  freed[2] = {nullptr, nullptr};   // the H2D copy out of pin[i] has finished
    hipStream_t copy_stream = nullptr;
};

}  // namespace psa

enum { PSA_T_H2D = 0, PSA_T_PHASE, PSA_T_PROJECT, PSA_T_FFT, PSA_T_EPILOGUE, PSA_T_GATHER,
       PSA_T_TRANSPOSE, PSA_T_D2H, PSA_T_COUNT };

// Everything the context opens it owns: the buffers and the rocFFT plans free themselves as members, ~psa_ctx
// (api_core.hip) closes the rest first, in the order it documents.
struct psa_ctx {
    psa_ctx();                  // the options' defaults, from the table
    ~psa_ctx();
    psa_ctx(const psa_ctx&) = delete;
    psa_ctx& operator=(const psa_ctx&) = delete;

    int         device = 0;
    hipStream_t stream = nullptr;
    std::mutex  mu;
    int         k1_selector = PSA_K1_AUTO;
    int         compute_units = 0;

    // [PSA_NUM_SLOTS] is internal: positions minus their mean (displacement mode), materialised on
    // first use and kept while the positions and the mean stay the same
    psa::DataSlot slot[PSA_NUM_SLOTS + 1];
    std::vector<float> disp_mean;        // the mean the displacement array was built with
    uint64_t           disp_source = 0;  // generation of the positions slot it was built from
    // largest |positions - mean| per 32-atom column block (scale of displacement-mode planes)
    std::vector<unsigned> disp_block_absmax;
    std::vector<float>    disp_abs_mean;
    uint64_t              disp_abs_source = ~0ull;

    // per-call scratch
    psa::DevBuf d_kvec, d_mean_all, d_idx, d_mean_g, d_phase, d_qwork, d_fft_work, d_tables, d_absmax;
    psa::DevBuf d_upload_max;                 // running largest magnitude of an array being uploaded
    psa::DevBuf d_zeros;                      // 1 KiB of zeros (k1_planes_wide.hip: planes of the stages past a group's end)
    psa::DevBuf d_qrows, d_stage, d_bin;      // frame sharding: my rows before the FFT / all-to-all landing zone; one DFT bin

    // cached split planes (PSA_OPT_PLANES*)
    std::vector<std::unique_ptr<psa::PlaneSet>> planes;
    std::vector<uint64_t> seen_groups;        // hashes of index-list groups projected once already
    uint64_t plane_tick = 0, plane_call_mark = 0;   // sets touched since the mark belong to the call in progress
    int64_t  opt_planes, opt_planes_budget, opt_planes_eager, opt_planes_min_k;   // the options: defaults from the table (api_core.hip)
    psa::Stager stager;
    hipStream_t d2h_stream = nullptr;         // result blocks leave while the next block is projected
    hipEvent_t  d2h_ready = nullptr;

    // frame sharding (psa_sed_fs_*): geometry of the group in flight
    int64_t fs_T_total = 0, fs_T_local = 0, fs_K_total = 0, fs_rows_k0 = 0, fs_rows_nk = 0;
    bool    fs_intensity = false;
    // results
    psa::DevBuf d_slab;      // k-major: (K_total,3,T) c64  or (K_total,T) f32
    psa::DevBuf d_out;       // reference layout: (T,K_total,3) c64 or (T,K_total) f32
    psa::DevBuf d_aux;       // (T,K_total) f32 for intensity / chiral phase of the result
    int64_t res_T = 0, res_K = 0;           // frames; ROWS of the slab (= k-vectors projected)
    bool    res_intensity = false;
    // k-vectors of the result when pairs (k, -k) / duplicates were folded: out_K columns, column k
    // from slab row kmap[k] (KMAP_MIRROR: as the partner of that row); empty = the slab's rows as they are
    int64_t              out_K = 0;
    std::vector<int32_t> kmap;
    psa::DevBuf          d_kmap, d_cols;
    int64_t              opt_fold_pairs;
    psa::DevBuf          d_inten;                 // (T,out_K) f32: sum_c |d_out|^2 of a finalized complex result
    bool                 inten_valid = false;
    bool    slab_valid = false, out_valid = false;

    std::map<std::pair<int64_t, int64_t>, psa::FftPlan> plans;   // (T, batch)
    // rocFFT compiles the kernels of a length at run time on first use (tens to hundreds of ms): when a
    // trajectory of T frames becomes resident a host thread builds a small plan of that length, so the
    // first calculation finds the kernels compiled (and, through the per-user cache file, so does the
    // next process)
    std::thread  fft_primer;
    psa::FftPlan primed;
    int64_t      primed_T = 0;
    int64_t      opt_fft_prime;
    int64_t      opt_k1_wide;                   // PSA_OPT_K1_WIDE: 256-row M blocks (k1_planes_wide.hip) where the k-list fills them (k1_planes_block_rows)
    int64_t      opt_k1_loader_waves;           // PSA_OPT_K1_LOADER_WAVES: 128-row M blocks through k1_planes_lw.hip
    int64_t      opt_k1_lowrank;                // PSA_OPT_K1_LOWRANK: k-paths through the node rows + D pass (api_lowrank.hip)
    int64_t      opt_k1_lowrank_min_k;          // PSA_OPT_K1_LOWRANK_MIN_K: shortest whole k-list it serves
    int64_t      opt_k1_lowrank_min_local;       // PSA_OPT_K1_LOWRANK_MIN_LOCAL: shortest part of it one launch serves
    int64_t      lowrank_launches = 0;          // projection launches that took the route (psa_k1_lowrank_launches)
    int64_t      opt_k1_lowrank_pair;           // PSA_OPT_K1_LOWRANK_PAIR: lists with one 512-row D block through k1_lowrank_pair.hip
    int64_t      lowrank_pair_launches = 0;     // ... of which the pair launch served (psa_k1_lowrank_pair_launches)
    int          k1_lowrank_nodes = 48;         // psa_set_k1_lowrank_nodes: 48 or 64 Chebyshev nodes; 48 only while the fold is on (k1_lowrank_n48.hip)
    bool         k1_lowrank_fold = true;        // psa_set_k1_lowrank_fold: D' = D + E in the D image, two products per node row (k1_lowrank_fold.hip)
    // its D image, node projections, the combine's L and phi, fp64 inputs (the node table goes into d_phase);
    // released when the route is switched off
    psa::DevBuf  d_lr_diff, d_lr_qn, d_lr_L, d_lr_phi, d_lr_f64;

    // per-atom weights of every projection (psa_set_atom_weights): d_weights holds weights_N values, none when 0;
    // weights_scale = 2^e, the smallest power of two >= their largest magnitude
    psa::DevBuf  d_weights;
    int64_t      weights_N = 0;
    float        weights_scale = 1.f;

    // Welch segments of every intensity projection (psa_set_segments): length seg_L (0 = none), hop seg_hop, the window
    // (seg_L float32) in d_seg_window, seg_U = (1/L) sum w^2 in float64; d_seg: the segment buffer (at most the q buffer)
    psa::DevBuf  d_seg_window, d_seg;
    int64_t      seg_L = 0, seg_hop = 0;
    double       seg_U = 0.0;
    bool         seg_boxcar = false;                   // every window value is exactly 1.0f (the correlations need it)

    // vibrational density of states (psa_vdos, api_vdos.hip): the work buffer of one (atom block x segment block) is held
    // to opt_vdos_work_bytes (PSA_OPT_VDOS_WORK_BYTES); the pair list, the groups' pair offsets, the mean, the chunk
    // partials, the float64 accumulator and the float32 result.  All kept between calls.
    psa::DevBuf  d_vdos_work, d_vdos_pairs, d_vdos_off, d_vdos_mean, d_vdos_part, d_vdos_acc, d_vdos_out;
    int64_t      opt_vdos_work_bytes;

    // mode-projected SED (psa_sed_modes, psa_sed_modes_welch; api_modes.hip): the stacked spectra (B, kb, 3, T) of one
    // block of k-vectors, held to opt_modes_work_bytes (PSA_OPT_MODES_WORK_BYTES); the packed coefficient table
    // conj(eig); the (T, K, M) result -- (L, K, M) with segments set, which also use d_seg for the segments
    // (B, bk, 3, bs, L) of a sub-block, q and d_seg together within the budget.
    // All kept between calls.
    psa::DevBuf  d_modes_work, d_modes_coef, d_modes_out;
    int64_t      opt_modes_work_bytes;

    // spectral covariance (psa_sed_covariance; api_covariance.hip): the stacked spectra lie in d_modes_work, under the same
    // budget as the partial slabs [k][chunk][slot][pair][part][256] of a block; the weight table (n_w, T); the (n_w, K, 3B, 3B)
    // complex128 result.  All kept between calls.
    psa::DevBuf  d_cov_slab, d_cov_g, d_cov_out;

    // Lorentzian peak fits (psa_fit_peaks, psa_sed_modes_fit; api_peaks.hip): an uploaded spectrum, the per-column bands,
    // the row slices' partial maxima (value, bin, non-finite flag) and the results.  All kept between calls.
    psa::DevBuf  d_peaks_spec, d_peaks_bands, d_peaks_part, d_peaks_fit, d_peaks_info;

    // reciprocal-space spectra and time correlations (api_reciprocal.hip: what api_dynamic.hip, api_lattice.hip,
    // api_partial.hip, api_self.hip and api_correlation.hip share).  One set that every call of those families fills before
    // it reads it and none keeps for the next:
    //   work    the projections q of one block of k-vectors -- (kb, NC, T); the partial spectra's (kb, S, NC, T) --, or the
    //           self part's series of one block (atoms, vectors, segments, P); held, together with the segment buffer d_seg,
    //           to opt_dynamic_work_bytes (PSA_OPT_DYNAMIC_WORK_BYTES).  Everything below is outside that budget
    //   kappa   k / 2 pi as float32 hi and lo parts (K, 6) (psa_dynamic_spectra alone)
    //   khat    the unit vectors k / |k| (K, 3) in the order of the rows of q
    //   idx     the atom list; the partial spectra's species lists, concatenated
    //   tiles, ent, slot, dest    the plan of a lattice call: tile offsets, the tiles' entries, per vector its three
    //           entries and (dest) its row of q -- S row for S species; the self part's tiles hold two offsets each
    //   bins, scale    the shell form's bin offsets; the columns' scales in float64
    //   acc, out       the float64 accumulator that lives across the blocks of a call (zeroed by the call) and the float32
    //           result; the per-vector time correlations leave their float32 power in out
    //   groups, part   the self part's columns (first vector, column) and its chunks' float64 partial sums
    psa::DevBuf  d_rc_work, d_rc_kappa, d_rc_khat, d_rc_idx, d_rc_tiles, d_rc_ent, d_rc_slot, d_rc_dest, d_rc_bins, d_rc_scale,
                 d_rc_acc, d_rc_out, d_rc_groups, d_rc_part;
    int64_t      opt_dynamic_work_bytes;

    // time correlations on that lattice (psa_lattice_correlations, psa_self_correlations; api_correlation.hip): they run
    // the set above with zero-padded rows of P >= L + n_lags - 1 and add the back-transform's cosine table
    // (P float64), the lag factors (n_lags float64), the columns' scales (cols float64), the debug entry's uploaded power
    // and the float32 result (1 or 3, n_lags, K or n_bins).  All kept between calls.
    psa::DevBuf  d_corr_tab, d_corr_factor, d_corr_scale, d_corr_in, d_corr_out;

    // real-space structure (api_realspace.hip: what api_msd.hip, api_pair.hip and api_shell.hip share).  One set that every
    // call of the three families fills before it reads it and none keeps for the next: the atom list, the item or chunk
    // table, the workgroups' partials (uint32 histograms; float64 moments) and the accumulator that lives across the
    // blocks and lags of a call (zeroed by the call).
    psa::DevBuf  d_rs_idx, d_rs_items, d_rs_part, d_rs_acc;

    // real-space self dynamics (psa_displacement_moments, psa_van_hove_self, psa_debug_unwrap; api_msd.hip): the unwrapped
    // displacements u64 (atoms of a block, 3, T) float64, held to opt_dynamic_work_bytes; outside it the debug entry's
    // image counts, the unwrap pass's tile sums and offsets, the groups' sizes, the van Hove lags and the scaled moments.
    psa::DevBuf  d_msd_u, d_msd_img, d_msd_sums, d_msd_offs, d_msd_sizes, d_msd_lags, d_msd_out;

    // the self-overlap (psa_self_overlap; api_overlap.hip): the per-origin counts Q (n_lags, G, n_o_max) uint32, which live
    // across the blocks of a call (zeroed by the call) and count against opt_dynamic_work_bytes beside u64, and the two
    // sums over origins (n_lags, G, 2) uint64.  The lags go through d_msd_lags, the chunk partials through d_rs_part.
    psa::DevBuf  d_ov_q, d_ov_sums;

    // pair distributions (psa_pair_histogram, psa_debug_pair_fractions; api_pair.hip): the centred fractional coordinates
    // of a block of origin frames and of their partner frames (2, origins, 3, n_a) float32, held to opt_dynamic_work_bytes.
    psa::DevBuf  d_pair_c;

    // the neighbour shells (api_shell.hip's angle_work, for the entries of api_angle, api_order, api_cluster, api_persist,
    // api_cna and api_acna.hip): per origin of a block the centred fractional coordinates (3, n_a) float32, the neighbour
    // counts (n_a) int32 and the neighbour lists (n_a, 64, 4) float32 -- 1040 n_a bytes -- and behind the counts what the
    // entry's ShellLayout states, all held to opt_dynamic_work_bytes; outside it the bin edges of psa_angle_histogram.
    psa::DevBuf  d_angle_work, d_angle_edges;
    // psa_local_order, psa_debug_qlm (api_order.hip): behind the counts the table of the Q_lm (n_a, columns, 2) int64 and the
    // per-atom rows; outside the buffer the normalisations N_lm and the 3j symbols, float64, uploaded by every call.
    // psa_solid_clusters, psa_debug_cluster_labels (api_cluster.hip): the masks, xi, parent and size behind the table
    psa::DevBuf  d_local_tab;

    psa::TimingState timing;
    double oneoff_ms[4] = {0, 0, 0, 0};   // host wall clock of work done once: rocFFT plan builds, magnitude passes,
                                          // plane builds, trajectory uploads (psa_oneoff_stats)
    psa::DevBuf      d_sync;     // one float for the RCCL barrier

    // psa_debug_scratch_fill: the byte the real buffers of the table SCRATCH (api_core.hip) and new plane sets are filled
    // with while the context is armed; -1: not armed
    int scratch_byte = -1;

    ncclComm_t comm = nullptr;
    int        rank = 0, nranks = 1;
};

namespace psa {

// --- kernels_misc.hip
int launch_phase_table(psa_ctx* c, const float* d_kvec, const float* d_mean_all, const int* d_idx,
                       float* d_phase, const ProjGeom& g);
int launch_gather_mean(psa_ctx* c, const float* d_mean_all, const int* d_idx, float* d_mean_g,
                       const ProjGeom& g);
int launch_fill_synthetic(psa_ctx* c, float* d_v, int64_t T, int64_t N, uint64_t seed, int64_t t_offset, int n_modes,
                          const float* d_amp, const int* d_comp, const float* d_ct,
                          const float* d_st, const float* d_ca, const float* d_sa);
int launch_mean_over_frames(psa_ctx* c, const float* d_x, int64_t T, int64_t N, float* d_mean);
int launch_subtract_mean(psa_ctx* c, const float* d_x, const float* d_mean, float* d_out, int64_t T, int64_t N);
int launch_absmax_bits(psa_ctx* c, const float* d_x, int64_t n, unsigned* d_out, bool reset = true);
int launch_absmax_blocks(psa_ctx* c, const float* d_x, const float* d_mean, int64_t T, int64_t N, unsigned* d_out);

// K1 launchers.  The block map and its grid are in k1_tile.h, the parts of the "2 x f16" kernels and the launch of
// the planes family in k1_f16.h.
// --- k1_mfma.hip / k1_wave.hip
int  k1_mfma_block_rows(int K);                    // M block of the variant chosen for K
int  launch_k1_mfma(psa_ctx* c, const float* d_v, const float* d_phase, const int* d_idx,
                    const float* d_mean_g, float2* d_q, const ProjGeom& g, bool displacements);
int  launch_k1_wave(psa_ctx* c, const float* d_v, const float* d_phase, const int* d_idx,
                    const float* d_mean_g, float2* d_q, const ProjGeom& g, bool displacements);

// --- k1_split.hip ("3 x bf16": any velocity-mode group)
bool   k1_split_eligible(const int* d_idx, int64_t N_tot, int64_t n_g, bool displacements);
int    k1_split_block_rows(int K);
size_t pb_table_bytes(int M_pad, int A_pad);
int    launch_phase_table_split(psa_ctx* c, const float* d_kvec, const float* d_mean_all, const int* d_idx,
                                void* d_phase, const ProjGeom& g);
int    launch_k1_split(psa_ctx* c, const float* d_v, const void* d_phase, const int* d_idx, float2* d_q,
                       const ProjGeom& g);

// --- k1_pair.hip ("2 x f16": whole-trajectory groups, 2K > 64)
bool   k1_pair_eligible(const int* d_idx, int64_t N_tot, int64_t n_g, int64_t K, bool displacements);
int    k1_pair_atom_pad(int64_t n_g);
int    k1_pair_block_rows(int K);
float  k1_f16_vscale(unsigned absmax_bits);
size_t pf16_table_bytes(int M_pad, int A_pad);
int    launch_phase_table_f16(psa_ctx* c, const float* d_kvec, const float* d_mean_all, const int* d_idx,
                              void* d_phase, const ProjGeom& g);
int    launch_k1_pair(psa_ctx* c, const float* d_v, const void* d_phase, const int* d_idx, float2* d_q,
                      const ProjGeom& g);

// --- k1_planes.hip ("2 x f16" from cached split planes: every kind of group)
int    k1_planes_block_rows(int K, bool wide);
int    launch_split_planes(psa_ctx* c, const float* d_x, const float* d_mean, const int* d_idx, void* d_planes, int64_t T,
                           int64_t N_tot, int n_g, int A_pad, float vscale);
int    launch_k1_planes(psa_ctx* c, const void* d_planes, const void* d_phase, float2* d_q, const ProjGeom& g,
                        int64_t n_fg);
// --- k1_planes_lw.hip (the same with dedicated loader wavefronts; 128-row M blocks)
int    launch_k1_planes_lw(psa_ctx* c, const void* d_planes, const void* d_phase, float2* d_q, const ProjGeom& g,
                           int64_t n_fg);
// (the low-rank route's folded node rows: two products per row tile, the node table's hi piece only)
int    launch_k1_planes_lw2(psa_ctx* c, const void* d_planes, const void* d_phase, float2* d_q, const ProjGeom& g,
                            int64_t n_fg);

// --- k1_planes_wide.hip (256-row M blocks: k-lists of more than 64 vectors under PSA_OPT_K1_WIDE)
int    launch_k1_planes_wide(psa_ctx* c, const void* d_planes, const void* d_phase, float2* d_q, const ProjGeom& g,
                             int64_t n_fg);

// --- k1_planes_diff.hip (low-rank route for k-paths: tables, D pass; planned in api_lowrank.hip)
size_t pd16_table_bytes(int M_pad, int A_pad);
int    launch_lowrank_tables(psa_ctx* c, const float* d_kvec, const double* d_kline, const double* d_geo, const double* d_kappa,
                             const float* d_mean_all, const int* d_idx, void* d_diff, void* d_nodes, const ProjGeom& g, int M_pad_d,
                             float dscale, bool pair);
int    launch_k1_planes_diff(psa_ctx* c, const void* d_planes, const void* d_diff, float2* d_q, const ProjGeom& g, int64_t n_fg,
                             float dscale);
// (psa_set_k1_lowrank_fold: the node table, then the folded image D' = D + E built from its lo pieces; pair: in the layout of
// k1_lowrank_fold.h)
int    launch_lowrank_tables_fold(psa_ctx* c, const float* d_kvec, const double* d_kline, const double* d_geo, const double* d_kappa,
                                  const float* d_mean_all, const int* d_idx, const float* d_L, const float2* d_phi, void* d_diff,
                                  void* d_nodes, const ProjGeom& g, int M_pad_d, float dscale, bool pair);

// --- k1_lowrank_pair.hip (the route's node rows and D rows as one launch of balanced row pairs: one 512-row D block;
// the D image in the pair layout, launch_lowrank_tables with pair = true)
int    launch_k1_lowrank_pair(psa_ctx* c, const void* d_planes, const void* d_nodes, const void* d_diff, float2* d_qn, float2* d_q,
                              const ProjGeom& g, int64_t n_fg, float dscale);

// (psa_set_k1_lowrank_nodes = 48: the 48-node table in the same 128-row block, then the D image from its hi pieces; pair: in
// the layout of k1_lowrank_n48.h)
int    launch_lowrank_tables_n48(psa_ctx* c, const float* d_kvec, const double* d_geo, const double* d_kappa, const float* d_mean_all,
                                 const int* d_idx, const float* d_L, const float2* d_phi, void* d_diff, void* d_nodes, const ProjGeom& g,
                                 int M_pad_d, float dscale, bool pair);
// --- k1_lowrank_n48.hip (the folded launch with 48 nodes: 96 node rows + D' rows 0..159 / D' rows 160..511)
int    launch_k1_lowrank_n48(psa_ctx* c, const void* d_planes, const void* d_nodes, const void* d_diff, float2* d_qn, float2* d_q,
                             const ProjGeom& g, int64_t n_fg, float dscale);
// --- k1_lowrank_fold.hip (the same launch on the folded tables: two-product node rows + D' rows 0..127 / D' rows 128..511)
int    launch_k1_lowrank_fold(psa_ctx* c, const void* d_planes, const void* d_nodes, const void* d_diff, float2* d_qn, float2* d_q,
                              const ProjGeom& g, int64_t n_fg, float dscale);

// --- lowrank_combine.hip (the route's combine: real weights + one phase per element)
int    launch_lowrank_combine_r(psa_ctx* c, const float2* d_qn, const float* d_L, const float2* d_phi, float2* d_q, const ProjGeom& g,
                                int64_t qn_stride);

// --- k2_epilogue.hip
int launch_dft_bin(psa_ctx* c, const float2* d_q, int64_t T, int64_t bin, float2* d_out3);
// n output columns of a K_pitch-column result (T, K_pitch, 3) from rows of the k-major slab: column
// d_cols[i] (null: col_first + i) from row d_srcs[i] (null: src_first + i; KMAP_MIRROR: the partner
// -k of the row's k-vector); d_inten (may be null): sum_c |.|^2 of the same columns into (T, K_pitch)
int launch_scale_transpose_c64(psa_ctx* c, const float2* d_slab, float2* d_out, float* d_inten, int64_t T, int64_t n,
                               int64_t K_pitch, int64_t col_first, int64_t src_first, const int32_t* d_cols,
                               const int32_t* d_srcs);
int launch_intensity_accumulate(psa_ctx* c, const float2* d_q, float* d_slab_rows, int64_t T,
                                int64_t K_local, bool first_group);
int launch_transpose_f32(psa_ctx* c, const float* d_slab, float* d_out, int64_t T, int64_t K, const int32_t* d_srcs);
// Welch segments: rows [0, nk) of q (from the block's first row) x segments [s0, s0 + ns) -> windowed segment buffer
// (nk,3,ns,L); after its FFT, inv_norm sum_s sum_c |F/L|^2 into slab rows (nk, L) (first: overwrite)
int launch_segment_window(psa_ctx* c, const float2* d_q, const float* d_w, float2* d_seg, int64_t T, int64_t L, int64_t H,
                          int64_t s0, int64_t ns, int64_t nk);
// the same for n_series rows of q (n_series, T), whatever they are: (n_series, ns, L)
int launch_segment_window_rows(psa_ctx* c, const float2* d_q, const float* d_w, float2* d_seg, int64_t T, int64_t L, int64_t H,
                               int64_t s0, int64_t ns, int64_t n_series);
int launch_segment_power(psa_ctx* c, const float2* d_seg, float* d_rows, int64_t L, int64_t ns, int64_t nk, float inv_norm,
                         bool first);
// --- vdos.hip (psa_vdos: per-atom series -> power summed per atom group; two atoms share one complex series)
constexpr int VDOS_TILE_PAIRS = 32;   // atom pairs per gather tile: the unit of an atom block
// pairs [0, n_pairs) of d_pair_atoms (2 atom indices each, -1: none) x segments [s0, s0 + ns) of the resident array ->
// d_work (3, n_pairs, ns, L) complex64: w_a win[tau] (d - mean); mean, weights, win may be null
int launch_vdos_gather(psa_ctx* c, const float* d_data, const float* d_mean, const float* d_weights, const float* d_win,
                       const int* d_pair_atoms, float2* d_work, int64_t T, int64_t N, int64_t L, int64_t H, int64_t s0,
                       int64_t ns, int64_t n_pairs);
// after the FFT of d_work, the block being pairs [p0, p0 + n_pairs) of the list: acc (G,3,L) float64 rows of groups
// [g_first, g_first + n_groups) += sum over the group's rows of |Z|^2, through n_chunks partials (n_chunks, n_groups, 3, L)
int launch_vdos_power(psa_ctx* c, const float2* d_work, const int64_t* d_pair_off, double* d_part, double* d_acc, int64_t L,
                      int64_t ns, int64_t n_pairs, int64_t p0, int64_t g_first, int64_t n_groups, int64_t n_chunks);
// out (rows, L/2 + 1) float32 = scale (acc[o] + acc[(L - o) mod L])
int launch_vdos_finish(psa_ctx* c, const double* d_acc, float* d_out, int64_t L, int64_t rows, double scale);
// --- modes.hip (psa_sed_modes, psa_sed_modes_welch: contraction of the B groups' transforms with the mode vectors, fused
// with the modulus and the sum over Welch segments)
int modes_tile(int64_t M);            // modes per pass (MT) of the kernel that serves M mode vectors
// S (B, nk, 3, ns, L) complex64 unscaled transforms of ns segments of a block of nk k-vectors (psa_sed_modes: one of T
// frames, scale = 1/T^2); coef: the block's rows of the packed table [k][pass][3B][MT] complex64 = conj(eig), zero beyond
// M; out (L, K_pitch, M) float32, columns k_col0 .. k_col0 + nk - 1: (first ? 0 : out) + sum_s |sum_n coef S_s|^2 scale,
// one float32 chain in s.  L <= 2^31 - 64.
int launch_mode_power(psa_ctx* c, const float2* d_S, const float2* d_coef, float* d_out, int64_t L, int64_t ns, int64_t nk,
                      int64_t B, int64_t M, int MT, int64_t K_pitch, int64_t k_col0, float scale, bool first);
// --- covariance.hip (psa_sed_covariance: sum over frequency of g_m S_i conj(S_j) on the fp32 matrix cores)
int64_t covariance_chunks(int64_t T);                                 // frequency chunks (slabs per k-vector and tile) of T frames
int64_t covariance_slab_floats(int64_t T, int64_t n, int n_w);        // floats of one k-vector's slabs, n = 3 B rows
// S (B, nk, 3, T) complex64 unscaled transforms of a block of nk k-vectors, g (n_w, T) float32 -> slabs -> out
// (n_w, K_pitch, 3B, 3B) complex128, k-vectors k_col0 .. k_col0 + nk - 1, times `scale` in float64.  3 B <= 96, n_w 1 or 2,
// T <= 2^31 - 64, nk covariance_chunks(T) < 2^31.
int launch_covariance(psa_ctx* c, const float2* d_S, const float* d_g, float* d_slab, double2* d_out, int64_t T, int64_t nk, int64_t B,
                      int n_w, int64_t K_pitch, int64_t k_col0, double scale);
// --- peaks.hip (psa_fit_peaks: per column of a spectrum (F, C) the largest value of its band, then a Lorentzian fit)
int peaks_slices(int64_t C, int64_t rows);   // row slices peak_find splits `rows` rows of C columns into (at most 64)
// rows [row0, row_end) in n_slices slices -> (n_slices, C) partials: largest value of the column's band [lo, hi) (d_bands
// (C, 2), or null: lo, hi for all), its lowest bin, whether the band holds a non-finite value
int launch_peak_find(psa_ctx* c, const float* d_spec, int64_t C, const int32_t* d_bands, int lo, int hi, int row0, int row_end,
                     int n_slices, float* d_pmax, int* d_pidx, int* d_pflag);
// folds the partials, sets the window and fits: d_fit (C, 6) float32, d_info (C, 4) int32 as psa_fit_peaks returns them
int launch_peak_fit(psa_ctx* c, const float* d_spec, int64_t C, const int32_t* d_bands, int lo, int hi, const float* d_pmax,
                    const int* d_pidx, const int* d_pflag, int n_slices, double df, float window_hwhm, int half_window_bins,
                    int max_iter, float* d_fit, int32_t* d_info);
// --- dynamic.hip (psa_dynamic_spectra: q_c[k,t] = sum_a w_a d_a,c(t) exp(i k.r_a(t)) with the phase of every frame's own
// positions; the summation structure and the bound are in its header)
constexpr int DYN_THREADS = 256;   // lanes of a workgroup: DYN_THREADS / slices k-vectors x `slices` atom slices
constexpr int DYN_ATOMS = 512;     // atoms of one frame staged per tile
constexpr int DYN_CHAIN = 128;     // atoms one float32 accumulator sums before it is folded into the second float32 sum
constexpr int DYN_FRAMES = 4;      // frames one workgroup projects, one after the other
int dynamic_slices(int64_t K);     // atom slices the lanes of a workgroup are split into for a call of K k-vectors
// nk k-vectors (kappa: their rows of the (K, 6) table) x all T frames -> q (nk, NC, T) complex64, NC = currents ? 4 : 1;
// d_vel, d_weights, d_idx may be null (no currents, unit weights, all atoms); slices = dynamic_slices(K of the call)
int launch_dynamic_project(psa_ctx* c, const float* d_pos, const float* d_vel, const float* d_weights, const int* d_idx,
                           const float* d_kappa, float2* d_q, int64_t T, int64_t N, int64_t n_g, int64_t nk, bool currents,
                           int slices);
// after the FFT of the segment buffer (nk, NC, ns, L): out (1 or 3, L, K_pitch) float32, columns k_col0 .. k_col0 + nk - 1:
// (first ? 0 : out) + scale sum_s { |F_0|^2;  |sum_c khat_c F_c|^2;  (sum_c |F_c|^2 - |sum_c khat_c F_c|^2) / 2 }
int launch_dynamic_power(psa_ctx* c, const float2* d_seg, const float* d_khat, float* d_out, int64_t L, int64_t ns, int64_t nk,
                         bool currents, int64_t K_pitch, int64_t k_col0, float scale, bool first);
// (sin, cos)(2 pi x) of n arguments in turns by the kernel's own routine (the sweep that measures its error)
int launch_dynamic_sincos(psa_ctx* c, const float* d_turns, float2* d_out, int64_t n);
// --- lattice.hip (psa_lattice_spectra: q_c[n,t] = sum_a w_a d_a,c(t) exp(2 pi i n.s_a(t)) on the reciprocal lattice of the
// box, the phase factorised per axis; the arithmetic, the summation structure and the bound are in its header)
constexpr int LAT_THREADS = 256;       // lanes of a workgroup
constexpr int LAT_KS = 512;            // vectors of a tile: two per lane
constexpr int LAT_ATOMS = 128;         // most atoms of one frame staged per tile
constexpr int LAT_TABLE = 3584;        // entries (cos, sin) of the per-atom factor tables in LDS: atoms per tile x entries
constexpr int LAT_CHAIN = 128;         // atoms one float32 accumulator sums before it is folded into the second float32 sum
constexpr int LAT_FRAMES = 4;          // frames one workgroup projects, one after the other
constexpr int LAT_MAX_INDEX = 64;      // largest |n_j| served
constexpr int LAT_MAX_ENTRIES = 3 * (2 * LAT_MAX_INDEX + 1);   // distinct (axis, m) pairs a tile can use
// tiles tile0 .. tile0 + n_tiles - 1 of the uploaded plan x all T frames -> q (rows, NC, T) complex64 at the rows d_dest
// names; box_hi, box_lo: the 9 entries of Hinv as float32 parts (host); d_vel, d_weights, d_idx may be null
int launch_lattice_project(psa_ctx* c, const float* d_pos, const float* d_vel, const float* d_weights, const int* d_idx,
                           const float* box_hi, const float* box_lo, const int* d_tile_off, const unsigned short* d_ent,
                           const unsigned* d_slot, const int* d_dest, float2* d_q, int64_t T, int64_t N, int64_t n_g, int64_t tile0,
                           int64_t n_tiles, bool currents);
// after the FFT of the segment buffer (nb, NC, ns, L) of the vectors g0 .. g0 + nb - 1 (d_khat: their rows): acc
// (1 or 3, L, n_bins) float64 += sum over the bin's vectors and the segments of X_n[o] + X_n[(L - o) mod L], unscaled
int launch_lattice_shell(psa_ctx* c, const float2* d_seg, const float* d_khat, const int* d_bin_start, double* d_acc, int64_t L,
                         int64_t ns, int64_t g0, int64_t nb, int64_t n_bins, bool currents);
// out[i] = (float)(acc[i] scale[i mod n_bins]), n elements
int launch_lattice_finish(psa_ctx* c, const double* d_acc, const double* d_scale, float* d_out, int64_t n, int64_t n_bins);
// --- partial.hip (psa_partial_spectra: the passes after the FFT of S species' series per vector, which take the products
// F^a conj F^b of a pair of species where dynamic.hip and lattice.hip take moduli; the arithmetic is in its header)
constexpr int PARTIAL_MAX_SPECIES = 8;                                                  // most species of a call
constexpr int PARTIAL_MAX_PAIRS = PARTIAL_MAX_SPECIES * (PARTIAL_MAX_SPECIES + 1) / 2;  // pairs a <= b of them: 36
// (pair p = (a, b), a <= b, row-major over the upper triangle: (0,0), (0,1), .., (0,S-1), (1,1), ..; P = S (S + 1) / 2)
// after the FFT of the segment buffer (nk, S, NC, ns, L): out (1 or 3, P, L, K_pitch) float32, columns k_col0 .. k_col0 + nk - 1:
// (first ? 0 : out) + scale sum_s { Re F_0^a conj F_0^b;  Re (khat.F^a) conj (khat.F^b);  sum_c Re F_perp,c^a conj F_perp,c^b / 2 }
int launch_partial_power(psa_ctx* c, const float2* d_seg, const float* d_khat, float* d_out, int64_t L, int64_t ns, int64_t nk,
                         int n_species, bool currents, int64_t K_pitch, int64_t k_col0, float scale, bool first);
// the same segment buffer of the vectors g0 .. g0 + nb - 1 of the processing order: acc (1 or 3, P, L, n_bins) float64 += the
// sum over the bin's vectors and the segments of X_n[o] + X_n[(L - o) mod L], unscaled
int launch_partial_shell(psa_ctx* c, const float2* d_seg, const float* d_khat, const int* d_bin_start, double* d_acc, int64_t L,
                         int64_t ns, int64_t g0, int64_t nb, int64_t n_bins, int n_species, bool currents);
// --- self.hip (psa_self_spectra: z[a,n,t] = w_a exp(2 pi i n.s_a(t)) per atom, its power summed over the atoms; the
// arithmetic and the bound are in its header)
constexpr int SELF_THREADS = 256;      // lanes of a workgroup: SELF_ATOMS wavefronts, a lane per frame
constexpr int SELF_ATOMS = 4;          // atoms of an atom tile, one per wavefront: the unit of an atom block
constexpr int SELF_FRAMES = 64;        // frames of a frame tile: consecutive lanes, consecutive frames
constexpr int SELF_ENTRIES = 24;       // most distinct (axis, m) pairs of a vector tile: the table is 512 B per atom and entry
constexpr int SELF_KS = 64;            // most vectors of a vector tile
// Series of one block: atoms [0, na) of the list d_idx (null: atoms a0 + i) x the vectors of tiles [tile0, tile0 + n_tiles) x
// segments [s0, s0 + ns) -> work (na, nv, ns, pitch) complex64, nv the block's vectors, = win[l] w_a E_1 E_2 E_3 at frame
// s H + l, l < L <= pitch (the spectra: pitch = L; the time correlations: pitch = P, the tail left to their padding pass).  d_tile (2 (n_tiles_all + 1)): offsets of every tile into d_ent and into d_slot; v0: the block's first vector.
// d_weights, d_idx, d_win may be null (unit weights, atoms in order, no window).
int launch_self_series(psa_ctx* c, const float* d_pos, const float* d_weights, const int* d_idx, int64_t a0, const float* box_hi,
                       const float* box_lo, const int* d_tile, const unsigned short* d_ent, const unsigned* d_slot, const float* d_win,
                       float2* d_work, int64_t T, int64_t N, int64_t na, int64_t tile0, int64_t n_tiles, int64_t v0, int64_t nv,
                       int64_t L, int64_t H, int64_t s0, int64_t ns, int64_t pitch);
// After the FFT of work (na, nv, ns, L), the block's vectors being v0 .. v0 + nv - 1 of the processing order: column group
// g in [g_first, g_first + ng) owns the vectors d_groups[2 g] .. d_groups[2 g + 2] - 1 and the column d_groups[2 g + 1] of
// acc (L, cols) float64 += sum over its vectors in the block, the atoms and the segments of |Z[o]|^2 (mirror: + |Z[(L - o)
// mod L]|^2), through n_chunks partial sums over atom chunks, added in order (d_part: n_chunks ng L float64)
int launch_self_power(psa_ctx* c, const float2* d_work, const int* d_groups, double* d_part, double* d_acc, int64_t L, int64_t ns,
                      int64_t na, int64_t v0, int64_t nv, int64_t g_first, int64_t ng, int64_t cols, int64_t n_chunks, bool mirror);
// --- correlation.hip (psa_lattice_correlations, psa_self_correlations: the zero padding before the FFT and the float64
// cosine back-transform of the summed power; the arithmetic and the layouts are in its header)
constexpr int CORR_LAGS = 8;           // lags one lane of the column form carries
constexpr int CORR_COLS_MIN = 64;      // columns from which the lanes go over columns; below, over lags
// rows [0, n_rows) of d_q (n_rows, T) x segments [s0, s0 + ns) -> d_seg (n_rows, ns, P): bit copies of the L frames from
// (s0 + s) H, zeros in [L, P).  d_q null: only the tails [L, P) of d_seg are written (the rows' heads are there already)
int launch_correlation_pad(psa_ctx* c, const float2* d_q, float2* d_seg, int64_t T, int64_t L, int64_t P, int64_t H, int64_t s0,
                           int64_t ns, int64_t n_rows);
// out (fields, n_lags, cols) float32 = (float)(factor[t] scale[col] sum_o X[f, o, col] tab[(o t) mod P]), X (fields, P, cols)
// float64 or float32, tab (P) = cos(2 pi j / P), factor (n_lags), scale (cols; null: 1) float64
int launch_correlation_transform(psa_ctx* c, const double* d_X, const double* d_tab, const double* d_factor, const double* d_scale,
                                 float* d_out, int64_t fields, int64_t P, int64_t cols, int64_t n_lags);
int launch_correlation_transform(psa_ctx* c, const float* d_X, const double* d_tab, const double* d_factor, const double* d_scale,
                                 float* d_out, int64_t fields, int64_t P, int64_t cols, int64_t n_lags);
// --- msd.hip (psa_displacement_moments, psa_van_hove_self, psa_debug_unwrap: unwrapped displacements, their moments summed
// directly over time origins, the histogram of their length; the arithmetic and the layouts are in its header)
constexpr int MSD_LAGS = 256;          // lags of a lag tile, one per lane of the moments kernel's workgroup
constexpr int MSD_ORIGINS = 1024;      // most origins of an origin tile
constexpr int MSD_WINDOW = 1280;       // most frames of u64 the moments kernel stages per atom, origin tile and lag tile
constexpr int MSD_MAX_GROUPS = 8;      // most atom groups of a call
constexpr int MSD_MAX_BINS = 1024;     // most bins of a van Hove histogram (an overflow counter follows them)
constexpr int MSD_MAX_VH_LAGS = 64;    // most lags of a van Hove call
constexpr int MSD_UNWRAP_FRAMES = 64;  // frames of an unwrap tile: a lane per frame
constexpr int MSD_UNWRAP_ATOMS = 16;   // atoms of an unwrap tile, four per wavefront
int msd_origins(int64_t step);         // origins of an origin tile at this origin step: the window stays within MSD_WINDOW
// atoms [a0, a0 + na) of the list d_idx (null: atoms a0 + i) over all T frames -> d_u (na, 3, T) float64 and, unless null,
// d_img (na, 3, T) int32 image counts.  unwrap false: u = r(t) - r(0), counts 0, d_sums and d_offs unused; else both
// (ceil(T / MSD_UNWRAP_FRAMES), na, 3) int32.  box, box_inverse: H and Hinv on the host
int launch_msd_unwrap(psa_ctx* c, const float* d_pos, const int* d_idx, int64_t a0, int64_t na, const double* box,
                      const double* box_inverse, bool unwrap, int* d_sums, int* d_offs, double* d_u, int* d_img, int64_t T, int64_t N);
// d_chunks: n_chunks entries {first atom of the block, one past the last, group, 0} (int32 x 4), each of one group; n_os:
// origin slabs per chunk, the chunks listed group by group.  The moments kernel writes d_part (n_chunks, n_os, n_lags, 4)
// float64; the reduce adds a group's chunks and slabs in order to acc (n_lags, G, 4) -- group_first (G + 1, host): group
// g's chunks are group_first[g] .. group_first[g + 1] - 1
int launch_msd_moments(psa_ctx* c, const double* d_u, const void* d_chunks, int64_t n_chunks, double* d_part, int64_t T, int64_t n_lags,
                       int64_t step, int64_t n_os);
int launch_msd_moments_reduce(psa_ctx* c, const double* d_part, const int32_t* group_first, double* d_acc, int64_t n_lags, int64_t n_os,
                              int32_t G);
// out (n_lags, G, 4) = acc / (group_size[g] n_o(t)), an empty group: 0
int launch_msd_moments_finish(psa_ctx* c, const double* d_acc, const int64_t* d_group_size, double* d_out, int64_t T, int64_t n_lags,
                              int32_t G, int64_t step);
// the histogram kernel writes d_part (n_chunks, n_os, n_vh, n_r + 1) uint32 -- a chunk's atoms x the origins of a lag stay
// below 2^32 (the caller's chunk rule) --, launch_hist_reduce adds them to acc (n_vh, G, n_r + 1) uint64
int launch_msd_hist(psa_ctx* c, const double* d_u, const void* d_chunks, int64_t n_chunks, const int64_t* d_lags, int64_t n_vh,
                    unsigned* d_part, int64_t T, int64_t step, int64_t n_os, float inv_dr, int32_t n_r);
// --- overlap.hip (psa_self_overlap: per (lag, group, origin) the number of atoms still within the cut-off of where they
// were, and the first two moments of that count over the origins; the arithmetic and the layouts are in its header)
constexpr int OVERLAP_MAX_LAGS = 256;  // most lags of a call
constexpr int OVERLAP_RUN = 8;         // lags of a count workgroup: the origin side of u64 is read once for all of them
constexpr int OVERLAP_LANES = 256;     // origins of a count workgroup, one per lane: a piece of an origin tile
// d_chunks as for the moments kernel; d_lags (n_lags) the call's lags; n_o_max the origins of the smallest lag.  The count
// kernel writes d_part (n_chunks, n_lags, n_o_max) uint32 at the origins k < n_o(lag) and nowhere else; the reduce adds a
// group's chunks to q (n_lags, G, n_o_max) uint32 at those origins -- group_first as for launch_msd_moments_reduce
int launch_overlap_count(psa_ctx* c, const double* d_u, const void* d_chunks, int64_t n_chunks, const int64_t* d_lags, int64_t n_lags,
                         unsigned* d_part, int64_t T, int64_t step, int64_t n_o_max, float inv_a);
int launch_overlap_reduce(psa_ctx* c, const unsigned* d_part, const int32_t* group_first, const int64_t* d_lags, unsigned* d_q, int64_t T,
                          int64_t n_lags, int32_t G, int64_t step, int64_t n_o_max);
// sums (n_lags, G, 2) uint64 = the sums over k < n_o(lag) of q and of q^2
int launch_overlap_moments(psa_ctx* c, const unsigned* d_q, const int64_t* d_lags, unsigned long long* d_sums, int64_t T, int64_t n_lags,
                           int32_t G, int64_t step, int64_t n_o_max);
// --- hist_reduce.hip (the integer reduce of the three histogram families).  The rows of the partials that output row g
// sums, [lo[g], hi[g]), and what it multiplies the sum by: resolved by the host, passed by value
constexpr int HIST_REDUCE_MAX_ROWS = 64;   // most output rows of a launch: the ordered pairs of PAIR_MAX_SPECIES species
struct HistRows {
    int lo[HIST_REDUCE_MAX_ROWS], hi[HIST_REDUCE_MAX_ROWS], factor[HIST_REDUCE_MAX_ROWS];
};
// acc[(j n + g) cols + col] (uint64) += factor[g] sum_r part[(r n_outer + j) cols + col] (uint32), r in [lo[g], hi[g]), for
// g < n, j < n_outer, col < cols
int launch_hist_reduce(psa_ctx* c, const unsigned* d_part, const HistRows& rows, int32_t n, int64_t n_outer, int64_t cols,
                       unsigned long long* d_acc);
// --- pair.hip (psa_pair_histogram, psa_debug_pair_fractions: the histogram of minimum-image pair distances between two
// species over time origins; the arithmetic and the tiling are in its header)
constexpr int PAIR_TILE = 256;         // alpha-atoms of a workgroup, one per lane, and beta-atoms of a staged tile
constexpr int PAIR_MAX_BINS = 1024;    // most bins of a pair histogram (an overflow counter follows them)
constexpr int PAIR_MAX_LAGS = 64;      // most lags of a call
constexpr int PAIR_MAX_SPECIES = 8;    // most species of a call
// One workgroup's work: alpha-atoms [a_lo, a_lo + a_n) and beta-atoms [b_lo, b_hi) of the list, the origins slab, slab +
// n_os, ... of the block.  diag: how the beta-tile that starts at a_lo is masked (0: not, 1: list position a < b, 2: b != a)
struct PairItem {
    int a_lo, a_n, b_lo, b_hi, slab, n_os, diag, pair;
};
// frames f0 + k df, k < n_frames, of the atoms d_idx (null: all N; n_a of them) -> d_out (n_frames, 3, n_a) float32
int launch_pair_frac(psa_ctx* c, const float* d_pos, const int* d_idx, int64_t n_a, const double* box_inverse, float* d_out, int64_t f0,
                     int64_t df, int64_t n_frames, int64_t T, int64_t N);
// d_cA, d_cB (n_ob, 3, n_a): the fractions at the block's origins and at their partner frames; d_items: n_items PairItem,
// listed species pair by species pair; d_part (n_items, n_r + 1) uint32 -- an item's samples stay below 2^32 (the caller's
// rule); launch_hist_reduce adds them to acc (S, S, n_r + 1) uint64
int launch_pair_hist(psa_ctx* c, const float* d_cA, const float* d_cB, const void* d_items, int64_t n_items, unsigned* d_part,
                     const double* box, int64_t n_a, int64_t n_ob, float inv_dr, int32_t n_r);
// --- angle.hip (psa_angle_histogram, psa_debug_neighbour_lists: the neighbour shell of every atom, the angles between
// pairs of neighbours and the coordination numbers; the arithmetic and the tiling are in its header)
constexpr int ANGLE_MAX_NEIGHBOURS = 64;   // most neighbours a centre holds, all species together
constexpr int ANGLE_MAX_BINS = 1024;       // most bins of an angle histogram (the counter of undefined angles follows them)
constexpr int ANGLE_HIST_WORDS = 12288;    // 32-bit counters of a workgroup's angle histograms in LDS
constexpr int ANGLE_CENTRES = 256;         // centres of a workgroup's tile in the neighbour pass; lanes of a workgroup in both
constexpr int ANGLE_SPECIES_SHIFT = 28;    // a list entry's tag: list position | species << 28
// the species of a call as the kernels take them: offsets into the atom list, the centre tiles' first index per species,
// float32(1 / r_cut) per ordered species pair (0: no bond)
struct AngleSpecies {
    int   S, start[PAIR_MAX_SPECIES + 1], tile_first[PAIR_MAX_SPECIES + 1];
    float inv_rc[PAIR_MAX_SPECIES * PAIR_MAX_SPECIES];
};
// One workgroup's work in the angle pass: centres [a_lo, a_lo + a_n) of species `species` (a wavefront takes every
// fourth), the origins slab, slab + n_os, ...
struct AngleItem {
    int a_lo, a_n, species, slab, n_os;
};
// columns of a partial row and of a species' accumulator row: P (n_theta + 1) angle counters, S 65 coordination counters,
// the truncated centres
inline int64_t angle_row_words(int S, int n_theta) {
    return (int64_t)(S * (S + 1) / 2) * (n_theta + 1) + (int64_t)S * (ANGLE_MAX_NEIGHBOURS + 1) + 1;
}
// d_c (n_ob, 3, n_a) -> d_count (n_ob, n_a) int32, the true number of neighbours, and d_list (n_ob, n_a, 64) float4
// {d_x, d_y, d_z, tag}, the first 64 of them in the order of the atom list
int launch_angle_neighbours(psa_ctx* c, const float* d_c, int* d_count, void* d_list, const AngleSpecies& sp, const double* box,
                            int64_t n_a, int64_t n_ob);
// d_items: n_items AngleItem listed species by species; d_part (n_items, angle_row_words) uint32 -- an item's samples stay
// below 2^32 (the caller's rule); d_edges (n_theta + 1) float32; launch_hist_reduce adds them to acc (S, angle_row_words) uint64
int launch_angle_hist(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const float* d_edges,
                      unsigned* d_part, int32_t S, int64_t n_a, int64_t n_ob, int32_t n_theta);
// --- order.hip (psa_bond_order: the Steinhardt order parameters q_l of every atom's neighbour shell from the lists of the
// neighbour pass above, by the addition theorem; the arithmetic and the tiling are in its header)
constexpr int ORDER_MAX_L = 12;            // the largest order l
constexpr int ORDER_MAX_LS = 8;            // most orders of a call
constexpr int ORDER_MAX_BINS = 1024;       // most bins of a q histogram
constexpr int ORDER_SHIFT = 24;            // P_l is rounded to a multiple of 2^-24
// the orders of a call as the kernel takes them: bit l of mask is set for every l asked for (ascending: the j-th set bit
// is column j)
struct OrderLs {
    int n_l, l_max;
    unsigned mask;
};
// columns of a partial row and of a species' accumulator row: n_l n_q bins, then the truncated, the isolated and the
// undefined centres
inline int64_t order_row_words(int n_l, int n_q) { return (int64_t)n_l * n_q + 3; }
// d_count, d_list, d_items as for launch_angle_hist; d_part (n_items, order_row_words) uint32; d_x (n_ob, n_a, n_l) int64 or
// null: per centre the clamped X_l, -1 where the centre is left out
int launch_order_hist(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, unsigned* d_part,
                      long long* d_x, const OrderLs& ls, int64_t n_a, int64_t n_ob, int32_t n_q);
// --- qlm.hip (psa_local_order, psa_debug_qlm: the vectors q_lm of every atom's neighbour shell from the same lists, and from
// them the neighbour-averaged q_l, the third-order invariants w_l and the solid-like bonds; the arithmetic and the tiling
// are in its header)
constexpr int LOCAL_MAX_LS = 4;            // most orders of a call, even ones in [2, ORDER_MAX_L]
constexpr int LOCAL_MAX_BINS = 1024;       // most bins of a q-bar histogram and of a w histogram
constexpr int LOCAL_SHIFT = 40;            // a harmonic is rounded to a multiple of 2^-40
constexpr int LOCAL_MAX_COLUMNS = 40;      // sum of l + 1 over the orders of a call at most: 7 + 9 + 11 + 13
constexpr int LOCAL_NORM_WORDS = (ORDER_MAX_L + 1) * (ORDER_MAX_L + 1);   // N_lm at [l * 13 + m]
constexpr int LOCAL_W3J_WORDS = (2 * ORDER_MAX_L + 1) * (2 * ORDER_MAX_L + 1);   // a column's 3j block: (2 l + 1)^2 of them used
// the orders of a call as the kernels take them: bit l of mask is set for every l asked for (ascending: the j-th set bit is
// column j); columns = sum of l + 1; solid_l the order of the bond test
struct LocalLs {
    int      n_l, l_max, columns, solid_l;
    unsigned mask;
};
// columns of a partial row and of a species' accumulator row: n_l n_q bins of q-bar, n_l n_w of w, n_l n_w of w-bar, the 65
// connection counts, the truncated, isolated, undefined and incomplete centres, then per order w outside, w undefined, w-bar
// outside, w-bar undefined
inline int64_t local_row_words(int n_l, int n_q, int n_w) { return (int64_t)n_l * n_q + 2ll * n_l * n_w + ANGLE_MAX_NEIGHBOURS + 1 + 4 + 4ll * n_l; }
// d_count, d_list, d_items as for launch_angle_hist; d_norm LOCAL_NORM_WORDS float64; d_q (n_ob, n_a, columns, 2) int64: Q_lm,
// m = 0 .. l, of every centre; a centre that is truncated, isolated or undefined gets zeros with -1 in Im Q of its first column
int launch_qlm_sum(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const double* d_norm,
                   long long* d_q, const LocalLs& ls, int64_t n_a, int64_t n_ob);
// after launch_qlm_sum over the same items.  d_w3j (n_l, LOCAL_W3J_WORDS) float64; d_part (n_items, local_row_words) uint32;
// per atom d_atoms (3, n_ob, n_a, n_l) float64 or null: q-bar^2, w, w-bar (NaN: left out or undefined); d_xi (n_ob, n_a) int32 or null
struct LocalBins {
    int    n_q, n_w;
    double w_range, w_scale, thr2;         // [-R, R], n_w / (2 R), the squared threshold of a solid-like bond
};
int launch_local_order(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const long long* d_q,
                       const double* d_w3j, unsigned* d_part, double* d_atoms, int* d_xi, const LocalLs& ls, const LocalBins& bins,
                       int64_t n_a, int64_t n_ob);
// --- cluster.hip (psa_solid_clusters, psa_debug_cluster_labels: the connected components of the solid atoms over the same
// lists; the definition and the passes are in its header)
constexpr int CLUSTER_MAX_SIZES = 4096;    // most exact slots of the cluster-size histogram
constexpr int CLUSTER_ROW_WORDS = ANGLE_MAX_NEIGHBOURS + 1 + 4;   // a species' row: connections[65], the four left-out kinds
constexpr int CLUSTER_STATS_ORIGINS = 16;  // most origins of a workgroup of the stats pass
// the words of a stats partial and of the accumulator behind the species rows: slots 0 .. n_sizes + 1, large_atoms
inline int64_t cluster_stat_words(int n_sizes) { return (int64_t)n_sizes + 3; }
// the workgroups of the stats pass over n_ob origins and the origins each takes (at most CLUSTER_STATS_ORIGINS)
inline int64_t cluster_stat_each(int64_t n_ob) { return std::min<int64_t>(std::max<int64_t>((n_ob + 1023) / 1024, 1), CLUSTER_STATS_ORIGINS); }
inline int64_t cluster_stat_groups(int64_t n_ob) { return (n_ob + cluster_stat_each(n_ob) - 1) / cluster_stat_each(n_ob); }
// the four working arrays of the graph passes, each (n_ob, n_a): the ballot of solid bonds in list order, xi, parent (label
// after the flatten pass) and size (size_atoms after the stats pass)
struct ClusterWork {
    unsigned long long* mask;
    int *               xi, *parent, *size;
};
// after launch_qlm_sum with the single order ls.solid_l, over the same items: xi, mask, parent (own column where xi >=
// min_connections, else -1) and size = 0 of every row; d_part (n_items, CLUSTER_ROW_WORDS) uint32
int launch_cluster_bonds(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const long long* d_q,
                         unsigned* d_part, const ClusterWork& w, const LocalLs& ls, double thr2, int min_connections, int64_t n_a,
                         int64_t n_ob);
// the union of the edges (link 1: those whose mask bit is set; both_ways: also the edges a centre lists towards a later
// column, for lists that are not symmetric), then labels and sizes; d_err: set to 1 where a bounded loop ran out
int launch_cluster_hook(psa_ctx* c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items, const ClusterWork& w,
                        int link, bool both_ways, int* d_err, int64_t n_a, int64_t n_ob);
int launch_cluster_flatten(psa_ctx* c, const ClusterWork& w, int* d_err, int64_t n_a, int64_t n_ob);
// d_origin (n_ob, 4) int32: n_solid, n_clusters, largest, largest_label; d_part (cluster_stat_groups, cluster_stat_words) uint32
int launch_cluster_stats(psa_ctx* c, const ClusterWork& w, int* d_origin, unsigned* d_part, int n_sizes, int64_t n_a, int64_t n_ob);
// --- persist.hip (psa_bond_persistence: the pairs listed at an origin tested again at later frames; the arithmetic and the
// tiling are in its header)
constexpr int PERSIST_MAX_LAGS = 1024;     // most lags of a call
// columns of a partial row and of a (lag, species) accumulator row: per beta the bonds, the alive and the unbroken ones (S
// each), lost[65], the truncated centres
inline int64_t persist_row_words(int S) { return 3ll * S + ANGLE_MAX_NEIGHBOURS + 2; }
// d_count, d_list as the neighbour pass leaves them -> d_tags (n_ob, n_a, 64) int32, the tag words, and d_surv (n_ob, n_a):
// a centre's n low bits, 0 where it is truncated
int launch_persist_tags(psa_ctx* c, const int* d_count, const void* d_list, int* d_tags, unsigned long long* d_surv, int64_t n_a,
                        int64_t n_ob);
// one visited frame over the first n_ob origins of a block.  d_items as for launch_angle_hist; d_cl (n_ob, 3, n_a) the
// fractions of the lagged frames; rb: the species with float32(1 / r_break) in inv_rc; keep: d_surv &= the alive mask;
// d_part not null (a listed lag): d_alive (n_ob, n_a) and item i's persist_row_words counters at d_part + i part_stride
// (uint32) are written -- an item's samples stay below 2^32 (the caller's rule)
int launch_persist_step(psa_ctx* c, const int* d_count, const int* d_tags, const void* d_items, int64_t n_items, const float* d_cl,
                        unsigned long long* d_surv, unsigned long long* d_alive, unsigned* d_part, int64_t part_stride,
                        const AngleSpecies& rb, const double* box, int64_t n_a, int64_t n_ob, bool keep);
// --- cna.hip (psa_common_neighbours: the signature (j, k, l) of every bond of the lists and the structure type of every
// centre; the arithmetic and the tiling are in its header)
constexpr int CNA_MAX_J = 8, CNA_MAX_K = 16, CNA_MAX_L = 16;   // the signature table holds j < 8, k < 16, l < 16
constexpr int CNA_TYPES = 5;               // other, fcc, hcp, bcc, ico
// columns of a partial row and of a species' accumulator row: the table, the bonds outside it, the truncated centres
constexpr int CNA_ROW_WORDS = CNA_MAX_J * CNA_MAX_K * CNA_MAX_L + 2;
// d_c (n_ob, 3, n_a) the fractions the neighbour pass read; d_count, d_list, d_items as for launch_angle_hist; d_types (n_ob,
// n_a) int32: the type, -1 where the centre is truncated; d_sigs (n_ob, n_a, 64) uint32 or null: j | k << 8 | l << 16 in list
// order, 0xffffffff at and beyond n and for a truncated centre; d_part (n_items, CNA_ROW_WORDS) uint32 -- an item's samples
// stay below 2^32 (the caller's rule)
int launch_cna_signature(psa_ctx* c, const float* d_c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items,
                         int* d_types, unsigned* d_sigs, unsigned* d_part, const AngleSpecies& sp, const double* box, int64_t n_a,
                         int64_t n_ob);
// d_types as above -> d_out (n_ob, S, CNA_TYPES) uint64, the centres of every species by type (a truncated one in none)
int launch_cna_census(psa_ctx* c, const int* d_types, unsigned long long* d_out, const AngleSpecies& sp, int64_t n_a, int64_t n_ob);
// --- acna.hip (psa_adaptive_common_neighbours: a cut-off per centre from its nearest candidates, the signatures on its 12
// nearest and, where that gives nothing, on its 14 nearest; the arithmetic and the tiling are in its header)
constexpr int ACNA_MEMBERS_A = 12, ACNA_MEMBERS = 14;   // the members of test A (fcc, hcp, ico) and of test B (bcc)
// columns of a partial row and of a species' accumulator row: the table, the bonds outside it, the truncated, the short centres
constexpr int ACNA_ROW_WORDS = CNA_MAX_J * CNA_MAX_K * CNA_MAX_L + 3;
// d_c, d_count, d_list, d_items, d_types as for launch_cna_signature; d_cut (n_ob, n_a) float32: the cut-off of the test that
// ran last, not a number where none ran; d_near (n_ob, n_a, 14) int32 and d_sigs (n_ob, n_a, 14) uint32, both or neither: by
// rank the members' columns (-1 beyond the last test's) and their bonds' words (0xffffffff there); d_part (n_items,
// ACNA_ROW_WORDS) uint32
int launch_acna_signature(psa_ctx* c, const float* d_c, const int* d_count, const void* d_list, const void* d_items, int64_t n_items,
                          int* d_types, float* d_cut, int* d_near, unsigned* d_sigs, unsigned* d_part, const double* box, int64_t n_a,
                          int64_t n_ob);
int launch_result_intensity(psa_ctx* c, const float2* d_out, float* d_int, int64_t n_tk);
int launch_result_chiral_c(psa_ctx* c, const float2* d_out, float* d_phase, int64_t n_tk, int c1, int c2);

}  // namespace psa
