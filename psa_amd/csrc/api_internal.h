// Internal declarations shared by the api_*.hip translation units (the C ABI of libpsa_hip.so,
// include/psa_hip.h):
//   api_core.hip     context, error text, timing, rocFFT plans, options
//   api_data.hip     trajectory residency: staging pipeline, uploads, magnitude passes, mean, displacements
//   api_project.hip  the hot path: k-list folding, plane cache, geometry, the block projector, project / project_upload /
//                    calculate (pipelined) / single_bin, atom weights, segments
//   api_result.hip   results: finalize, the k map, slab access, intensity and chiral phase of a finalized result
//   api_debug.hip    diagnostics: phase table, projection without FFT, plane cache
//   api_lowrank.hip  the low-rank route for k-paths: its plan and what a launch needs on the device
//   api_shard.hip    sharding over RCCL: communicator, k-row gather, frame sharding
//   api_vdos.hip     the vibrational density of states: a second, non-projecting pass over the resident array
//   api_modes.hip    the mode-projected SED: the B site groups' spectra contracted with the mode vectors, with or without
//                    the Welch segment average between projection and contraction
//   api_covariance.hip  the spectral covariance of the B site groups' spectra: the frequency-weighted sum of their outer products
//   api_peaks.hip    Lorentzian peak fits of spectrum columns: an uploaded spectrum, or the mode spectra where they lie
//   api_reciprocal.hip  what the reciprocal-space entries below share: segments and block rule, the one run body
//                    (projection, window or padding, rocFFT, power pass, finish), the debug loops, bins, the shell pair
//   api_dynamic.hip  the dynamic structure factor and the current correlations: the phase of every frame's own positions
//   api_lattice.hip  the same spectra on the box's reciprocal lattice, per vector or averaged over shells of |k|
//   api_self.hip     the self (incoherent) part on that lattice: per-atom series, their power summed over the atoms
//   api_partial.hip  the species-resolved (partial) spectra on that lattice: one projection per species, products of pairs
//   api_correlation.hip  F(k,t), F_s(k,t), C_L(k,t), C_T(k,t) on that lattice: the spectral calls with padded segments, then
//                    the cosine back-transform of the summed power
//   api_realspace.hip  what the real-space entries share: the atom groups and their checks, the box's determinant, inverse
//                    and served radius, the histogram arguments, the atom-list upload, the rows of the integer reduce
//                    (hist_reduce.hip; the device side of the geometry: min_image.h)
//   api_msd.hip      MSD moments and the self van Hove function from unwrapped displacements
//   api_overlap.hip  the self-overlap Q(o, t) per time origin and its two moments over the origins (q(t), chi_4(t))
//   api_pair.hip     g(r), its partials and the distinct van Hove function
//   api_shell.hip    what the entries on the neighbour shells below share (api_shell.h): the call and its checks, the block
//                    rule, the layout of the work buffer, the items, the one run body over the blocks of origins
//   api_angle.hip    bond-angle distributions and coordination statistics
//   api_order.hip    the Steinhardt order parameters q_l and the local order (q-bar_l, w_l, solid-like bonds)
//   api_cluster.hip  solid-like clusters: the connected components of the solid atoms
//   api_persist.hip  bond persistence: neighbour-lifetime and cage correlations
//   api_cna.hip      common-neighbour analysis: the bonds' signatures and the atoms' structure types
//   api_acna.hip     adaptive common-neighbour analysis: a cut-off per atom from its nearest candidates
// What the K1 kernels and their launchers share: k1_tile.h (block map and grid, swizzles: every K1 kernel) and
// k1_f16.h (the "2 x f16" family: split, images, LDS-DMA, unit ring, fold, chain loop, epilogue, planes-family launch).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <unordered_map>

#include "k1_f16.h"

namespace psa {

extern thread_local std::string g_error;                 // text of the calling thread's last failure

struct HostTimer {                                    // adds its lifetime to one of ctx->oneoff_ms
    double*                               into;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit HostTimer(double* into_) : into(into_) {}
    ~HostTimer() { *into += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

struct Guard {
    std::lock_guard<std::mutex> lk;
    explicit Guard(psa_ctx* c) : lk(c->mu) {}
};

int          enter(psa_ctx* c);                          // null check + hipSetDevice
// how an entry point ends that hands the caller's arrays to the stream: they are only read or written during the call,
// whichever way it ends
inline int synchronised(psa_ctx* c, int rc, const char* entry) {
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PSA_OK) {
        set_error("hipStreamSynchronize failed after %s", entry);
        return PSA_EHIP;
    }
    return rc;
}
TimingState& timing(psa_ctx* c);
int          get_event(TimingState& ts, hipEvent_t* ev);
int          collect(psa_ctx* c, TimingState& ts);

struct StageTimer {
    psa_ctx*     c;
    TimingState& ts;
    int          stage;
    hipEvent_t   e0 = nullptr, e1 = nullptr;
    bool         ok = false;
    StageTimer(psa_ctx* c_, int stage_) : c(c_), ts(timing(c_)), stage(stage_) {
        if (get_event(ts, &e0) == PSA_OK && get_event(ts, &e1) == PSA_OK &&
            hipEventRecord(e0, c->stream) == hipSuccess)
            ok = true;
    }
    ~StageTimer() {
        if (ok && hipEventRecord(e1, c->stream) == hipSuccess) {
            ts.pending.push_back({stage, e0, e1});
            return;
        }
        for (hipEvent_t ev : {e0, e1})                    // not booked: the events go back to the pool
            if (ev) ts.pool.push_back(ev);
    }
};

int upload(psa_ctx* c, DevBuf& b, const void* host, size_t bytes);
int get_plan(psa_ctx* c, int64_t T, int64_t batch, FftPlan** out);
void prime_fft(psa_ctx* c, int64_t T);               // background build of the length's kernels (api_core.hip)
int run_fft(psa_ctx* c, float2* data, int64_t T, int64_t batch);
int check_slot(psa_ctx* c, int slot);
int validate_groups(int64_t N, const int32_t* group_idx, const int64_t* group_off, int32_t G);

// One atom group of a projection and where its data comes from: the group's index list on the host and on the device
// (nullptr: all atoms in order), and -- resolved by group_source -- the slot to launch on, whether the kernel still has to
// subtract the mean while staging, and the group's cached split planes, if any.
struct GroupView {
    int            slot = 0;
    bool           disp = false;
    int64_t        n_g = 0;
    const int*     d_idx = nullptr;
    const int32_t* h_idx = nullptr;
    PlaneSet*      ps = nullptr;
};
// group gi of (group_idx, group_off) -- nullptr: all N atoms -- whose lists have been uploaded to d_idx
inline void set_group(const psa_ctx* c, const int32_t* group_idx, const int64_t* group_off, int gi, int64_t N, GroupView* v) {
    v->n_g = group_idx ? group_off[gi + 1] - group_off[gi] : N;
    v->d_idx = group_idx ? c->d_idx.as<int>() + group_off[gi] : nullptr;
    v->h_idx = group_idx ? group_idx + group_off[gi] : nullptr;
}

// --- api_data.hip
int  slot_absmax(psa_ctx* c, int slot);
int  group_absmax(psa_ctx* c, int slot, const int32_t* h_idx, int64_t n_g, unsigned* bits);
int  displaced_absmax(psa_ctx* c, int slot, const float* mean_host, const int32_t* h_idx, int64_t n_g, unsigned* bits);
int  stager_init(psa_ctx* c, size_t chunk_bytes);
void stager_release(psa_ctx* c);
int  staged_upload(psa_ctx* c, float* dev, const float* host, int64_t T, int64_t N,
                   const std::function<int(int64_t, int64_t, hipEvent_t)>& on_chunk);
int  data_alloc_locked(psa_ctx* c, int slot, int64_t T, int64_t N);
int  materialise_displacements(psa_ctx* c, GroupView* v, const float* mean_host);

// --- api_project.hip
// what a list-level entry point was called with
struct ProjectArgs {
    int            slot;
    const float*   mean_pos_all;
    const float*   k_vectors;
    int64_t        K_local, K_total, k_offset;
    const int32_t* group_idx;
    const int64_t* group_off;
    int32_t        G, flags;
};

// make_geom's rule: the product rule; "3 x bf16" wherever it can serve (needs no scale: the streaming upload projects
// frames before the whole array has been seen); the float32 kernels only
enum class GeomRule { product, bf16_anywhere, f32_only };

size_t planes_bytes_held(psa_ctx* c);
void   drop_stale_planes(psa_ctx* c);
int    get_planes(psa_ctx* c, const GroupView& v, int64_t K_local, const float* mean_host, PlaneSet** out);
int    group_source(psa_ctx* c, GroupView* v, const float* mean_host, int64_t K);
int    make_geom(psa_ctx* c, const GroupView& v, int64_t K_local, GeomRule rule, ProjGeom* g);
int    prepare_phase(psa_ctx* c, const GroupView& v, const ProjGeom& g, int64_t k_first);
int    launch_projection(psa_ctx* c, const GroupView& v, ProjGeom g, float2* d_q, int64_t q_stride, int64_t t_begin,
                         int64_t t_count);
// The one place a projection is set up: geometry, the low-rank preparation where the caller offers that route
// (lowrank: the list the k-vectors belong to; nullptr = not offered), phase table -- for nk k-vectors from k_first of
// the uploaded list.  project_block then launches over all frames of the view's slot into d_q (nk,3,T).
int    prepare_block(psa_ctx* c, const GroupView& v, GeomRule rule, const ProjectArgs* lowrank, int64_t k_first, int64_t nk,
                     ProjGeom* g);
int    project_block(psa_ctx* c, const GroupView& v, const ProjectArgs* lowrank, int64_t k_first, int64_t nk, float2* d_q);
// The single-group entry points build their view with the host part filled ({slot, disp, n_g, nullptr, idx}; idx
// nullptr: all N atoms), check the list against the N atoms, and -- after whatever else they require -- upload the
// k-vectors, the mean and the list (nothing for an empty group), which fills the view's device part.
int    check_group_indices(const GroupView& v, int64_t N);
int    upload_single_group(psa_ctx* c, GroupView* v, int64_t N, const float* k_vectors, int64_t K, const float* mean_pos_all);
void   fold_pairs(const float* k, int64_t K, std::vector<int32_t>* kmap, std::vector<int32_t>* unique_idx);
int    install_kmap(psa_ctx* c, const std::vector<int32_t>& kmap);
// api_lowrank.hip: the plan of the low-rank route for k-paths (ok = false: the list stays on the dense kernels; why)
struct LowRankPlan {
    bool                ok = false;
    const char*         why = "";
    double              u[3] = {0, 0, 0}, k0[3] = {0, 0, 0};   // the line: k0 + kappa u
    double              x_c = 0, h_x = 0, width = 0;          // the group's centre / half-width along u; node interval width
    int64_t             interval = 0;                         // node interval [interval * width, + width)
    int                 nodes = LOWRANK_NODES;                // Chebyshev nodes: 64, or 48 (psa_set_k1_lowrank_nodes)
    double              kappa[LOWRANK_NODES] = {};            // the nodes (the first `nodes` entries)
    double              d_bound = 0;                          // bound on |P_ref - P_line|
    float               dscale = 0.f;                         // power of two the D image carries
    double              e_bound = 0;                          // bound on |E|, the node table's lo piece through the combine:
                                                              // max_j rot_j Lam_j 2^-12 from the float32 L and phi
    float               dscale_fold = 0.f;                    // power of two the folded image D + E carries (48 nodes: from
                                                              // d_bound + e_bound + LR48_R_MAX, the cap on any r_bound)
    double              r_bound = 0;                          // 48 nodes, on request: max over rows and atoms of |P_line - phi L W|
    std::vector<double> kline;                               // (K, 3) the k-vectors projected on the line
    std::vector<float>  L;                                    // (K, nodes) the combine's real Lagrange weights L_l(kappa_j)
    std::vector<float>  phi;                                  // (K) complex64, the combine's row phases exp(i kappa_j x_c)
};
// C (may be null; written only when the plan is ok): (K, 64) complex64, the product phi L rounded once from fp64 -- what
// psa_lowrank_plan reports beside the two factors.  No kernel reads it, so a launch asks for none.
// nodes: 64 or 48.  want_r (48 nodes): also r_bound, K x n_g x 48 complex products on the host -- the entry that reports the
// plan asks for it, a launch does not (its image scale takes the cap LR48_R_MAX instead).
int plan_lowrank(const float* k, int64_t K, const float* mean_all, int64_t N, const int32_t* h_idx, int64_t n_g, LowRankPlan* p,
                 float* C = nullptr, int nodes = LOWRANK_NODES, bool want_r = false);
int prepare_lowrank(psa_ctx* c, const GroupView& v, const ProjectArgs& list, int64_t k_first, int64_t nk, ProjGeom* g);
// api_modes.hip: what psa_sed_modes, psa_sed_modes_welch and their fits were called with, and their one body.  The result,
// (T, K, M) or with segments (L, K, M), is left in c->d_modes_out.  `segments`: the context's segments are honoured or
// refused.  out may be null only with `device_only` (the fits), and is then not copied to.
struct ModesArgs {
    int            slot;
    const float*   mean_pos_all;
    const float*   k_vectors;
    int64_t        K;
    const int32_t* group_idx;
    const int64_t* group_off;
    int32_t        B;
    const float*   eig;
    int64_t        M;
    int32_t        flags;
    float*         out;
    size_t         out_bytes;
};
int modes_run(psa_ctx* c, const ModesArgs& a, bool segments, bool device_only);
// the pieces of such a call, shared with psa_sed_covariance (api_covariance.hip): checks of the k-list and the site
// groups, uploads and group sources, the block rule, the B projections of a block
struct ModesCall {
    int64_t                T = 0, N = 0, K = 0, M = 0;
    int32_t                B = 0;
    int                    MT = 0;       // modes per pass of the contraction (modes_tile)
    size_t                 coef_k = 0;   // float2 per k-vector in the packed table
    int64_t                per_k = 0;    // bytes of one k-vector in the stacked buffer (B, kb, 3, T): 24 B T
    int64_t                kb_max = 0;   // most k-vectors a block may hold whatever the budget
    ProjectArgs            list;         // the call's list (the low-rank route is offered on it)
    std::vector<float>     coef;         // conj(eig) as the kernel reads it: [k][pass][3B][MT] (empty: no mode vectors)
    std::vector<GroupView> src;          // the B groups and where their data comes from
};
int     modes_check_groups(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                           const int64_t* group_off, int32_t B, int32_t flags, ModesCall* m);
int     modes_upload(psa_ctx* c, ModesCall* m);
int64_t modes_block(const psa_ctx* c, const ModesCall& m, int64_t k0, int64_t kb);
int     modes_project(psa_ctx* c, const ModesCall& m, int64_t k0, int64_t nk, float2* d_work);
// api_peaks.hip: the arguments of a fit, and the fit of a spectrum (F, C) resident on the device
struct PeakArgs {
    int64_t        F, C;
    double         df;
    const int32_t* bands;
    int32_t        lo, hi;
    psa_peak_opts  opts;
    float*         fit;
    int32_t*       info;
    int            row0 = 0, row_end = 0;      // the rows some band covers
};
int check_peak_args(const psa_peak_opts* opts, PeakArgs* a);
int peaks_run(psa_ctx* c, const float* d_spec, const PeakArgs& a);
// ---- api_reciprocal.hip: what the reciprocal-space entries (api_dynamic.hip, api_lattice.hip, api_partial.hip, api_self.hip,
// api_correlation.hip) share.  Their device buffers are the one set d_rc_* (psa_ctx.h).
// The shape of such a call: the checks of the slots, the atom set and the weights (dynamic_inputs), the context's segments
// (segment_shape), the block rule of the budget (dynamic_plan)
struct DynCall {
    int64_t T = 0, N = 0, K = 0, n_g = 0;
    int     NC = 1, slices = 1;
    int     n_species = 1;               // species whose NC series each vector holds (psa_partial_spectra; else 1)
    bool    cut = false;                 // false: one boxcar segment of T frames, q transformed in place
    int64_t L = 0, H = 0, n_seg = 0;
    int64_t n_lags = 0, P = 0;           // lags of a time-correlation call (0: spectra); the FFT length: L, or the padded one
    int64_t per_k = 0, unit = 0;         // bytes of one k-vector of q; of one (k-vector, segment) of the segment buffer:
                                         // n_species NC series each
    int64_t kb = 0, bk = 0, bs = 0;      // k-vectors per block of q; k-vectors x segments per sub-block
    std::vector<float> kappa, khat;      // (K, 6) k / 2 pi as hi xyz, lo xyz; (K, 3) k / |k|
};
int dynamic_inputs(psa_ctx* c, const char* entry, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents, DynCall* d);
// cut, L, H, n_seg and P of a call over d->T frames with d->n_lags lags; `segments` false: one boxcar segment of T frames,
// whatever the context holds
int segment_shape(const psa_ctx* c, bool segments, DynCall* d);
int dynamic_plan(psa_ctx* c, DynCall* d);
// The power part of a call, shared by the run and by the debug power entries, which differ only in where the transformed
// segments come from.  PowerPass: what every launch of the pass gets; d_bins set: the shell pass into d_acc, else
// dynamic.hip's power pass into d_out; n_species > 0: the pair passes of partial.hip on (nb, n_species, NC, ns, L).
// power_block: vectors [k0, k0 + nk) of the processing order in sub-blocks of bk vectors x bs segments; `fill` leaves the
// transformed segments (nb, NC, ns, L) of vectors k0 + k1 .. and segments s0 .. on the device and says where.
struct PowerPass {
    int          NC = 1;
    int          n_species = 0;          // 0: one series set per vector, moduli; else that many, products of pairs
    int64_t      L = 0, n_seg = 0, K = 0;
    float        scale = 0.f;
    const float* d_khat = nullptr;       // (K, 3), row 0 = vector 0 of the processing order
    float*       d_out = nullptr;
    const int*   d_bins = nullptr;
    double*      d_acc = nullptr;
    int64_t      n_bins = 0;
};
using SegFill = std::function<int(int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** d_seg)>;
int  power_block(psa_ctx* c, const PowerPass& p, int64_t k0, int64_t nk, int64_t bk, int64_t bs, const SegFill& fill);
// How a family fills q: the call's uploads (booked under PSA_T_H2D by the family), and block `block` of the call --
// vectors [k0, k0 + nk) of the processing order -- over all frames into d_q (nk, n_species NC, T)
struct BlockSource {
    std::function<int()>                                                     upload;
    std::function<int(int64_t block, int64_t k0, int64_t nk, float2* d_q)> project;
};
// The one run body of psa_dynamic_spectra, psa_lattice_spectra, psa_partial_spectra and psa_lattice_correlations after
// their checks (d planned): the out_bytes refusal, zeros for an empty atom set, the uploads and reservations, per block the
// projection, then per sub-block the window (with segments; else q in place) or -- d.n_lags set -- the zero-padding to
// d.P frames, the rocFFT and the power pass; at the end the shell form's finish pass and the copy home, or `finish`.
struct SpectraRun {
    BlockSource src;
    bool        pairs = false;           // products of pairs of the d.n_species species (partial.hip) where else moduli
    int64_t     n_bins = 0;              // > 0: the shell form
    // set: what ends a time-correlation call, handed the unscaled power where it lies (float32 per vector, float64 per shell)
    std::function<int(const float* d_power, const double* d_acc)> finish;
    float*      out_host = nullptr;
    size_t      out_bytes = 0;
};
int spectra_run(psa_ctx* c, const DynCall& d, const SpectraRun& a);
// the projection alone, block by block under the same rule: q (K, n_species NC, T) before any FFT
int debug_project_run(psa_ctx* c, const DynCall& d, const BlockSource& src, void* out_host);
// The power pass alone on transformed segments (K, series, n_seg, L) of the caller's, cut into sub-blocks of k_block
// vectors x seg_block segments (0: all): psa_debug_dynamic_power, psa_debug_lattice_shell, psa_debug_partial_power.
// bin_of null: the per-vector form with `scale`; else the shell form, the vectors sorted by bin, with the bins' scales
// 1 / (2 n_b norm).  debug_power_check: the refusals they share, and bk, bs; debug_power_run: the rest, with k / |k| in the
// order of the vectors (read with currents only)
struct DebugPower {
    const void*    seg_host = nullptr;
    const int32_t* bin_of = nullptr;
    int64_t        K = 0, n_bins = 0;
    int            n_species = 0;        // as PowerPass
    int32_t        currents = 0;
    int64_t        n_seg = 0, L = 0, k_block = 0, seg_block = 0;
    double         norm = 1.0;
    float          scale = 0.f;
    float*         out_host = nullptr;
    int64_t        bk = 0, bs = 0;
};
int debug_power_check(DebugPower* a);
int debug_power_run(psa_ctx* c, const DebugPower& a, const float* khat);
// rows [r0, r0 + nr) x segments [s0, s0 + ns) of host segments (rows, n_seg, L), packed as (nr, ns, L) and uploaded to b
int  upload_segments(psa_ctx* c, DevBuf& b, const void* host, int64_t r0, int64_t nr, int64_t n_seg, int64_t s0, int64_t ns, int64_t L);
// vectors per bin; the same of a list that comes sorted by bin, with the refusals of such a list
void bin_counts(const int32_t* bin_of, int64_t K, int64_t n_bins, std::vector<int64_t>* count);
int  sorted_bin_counts(const int32_t* bin_of, int64_t K, int64_t n_bins, std::vector<int64_t>* count);
// where each bin's vectors begin in an order sorted by bin (n_bins + 1) and the bins' scales 1 / (2 n_half n_seg U L^2), an
// empty bin: 0 (count: vectors per bin)
void lattice_bins(const std::vector<int64_t>& count, double n_seg, double U, double L, std::vector<int32_t>* bin_start,
                  std::vector<double>* scale);
// the shell form's float64 accumulator d_rc_acc, zeroed; its last launch: the n sums times the bins' scales (d_rc_scale)
// in float64, one rounding into d_out
int  shell_begin(psa_ctx* c, size_t bytes, double** d_acc);
int  shell_finish(psa_ctx* c, int64_t n, int64_t n_bins, float* d_out);

// api_lattice.hip: what the lattice families share: the refusals that concern the box and the vector list; Hinv as float32
// hi + lo; the processing order (bin_of: by (bin, n); else every run of kb vectors by n); one tile's entry list (appended to
// ent) and per vector the three entries it reads -- returns the tile's R
int  lattice_inputs(const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins);
void lattice_box_parts(const double* B, float* hi, float* lo);
void lattice_order(const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t kb, std::vector<int64_t>* order);
int  lattice_tile_entries(const int32_t* indices, const int64_t* members, int64_t nt, std::vector<uint16_t>* ent, uint32_t* slot);
// a psa_lattice_spectra call and its pieces, shared with psa_partial_spectra (api_partial.hip) and psa_lattice_correlations
// (api_correlation.hip; n_lags > 0: its padded plan)
struct LatCall {
    DynCall  d;                                      // sizes, segments, block rule (kappa unused; khat in row order)
    bool     shell = false;
    int64_t  n_bins = 0;
    float    box_hi[9], box_lo[9];
    std::vector<int64_t>  block_tile0;               // first tile of block b (n_blocks + 1)
    std::vector<int32_t>  tile_off, dest;            // (n_tiles + 1); (n_tiles LAT_KS): a vector's row of q, or -1
    std::vector<uint16_t> ent;
    std::vector<uint32_t> slot;                      // (n_tiles LAT_KS)
    std::vector<int64_t>  count;                     // (n_bins) vectors per bin
    std::vector<int32_t>  bin_start;                 // (n_bins + 1) in the processing order
    std::vector<double>   scale;                     // (n_bins) 1 / (2 n_half n_seg U L^2); an empty bin: 0
};
// the plan of a call whose d is planned: box parts, the processing order, k / |k| in row order, blocks, tiles, entries and
// the row table -- it holds row_mult x a vector's row: 1, or the species of a partial call --, the bins' counts, offsets
// and scales
int lattice_plan(const psa_ctx* c, const double* box_inverse, const int32_t* indices, const int32_t* bin_of, int64_t n_bins,
                 int64_t row_mult, LatCall* p);
// every refusal of a lattice call, the block rule and the plan
int lattice_check(psa_ctx* c, const char* entry, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
                  int64_t n_bins, const int32_t* idx, int64_t n_g, int32_t currents, int64_t n_lags, LatCall* p);
// the plan's uploads (idx null: no atom list)
int lattice_upload(psa_ctx* c, const LatCall& p, const int32_t* idx);
// block b of the plan over all frames into d_q, for one species: the atoms [a0, a0 + n_g) of the uploaded list (`listed`
// false: all atoms in order); an empty species still gets its launch, which writes its zeros
int lattice_project(psa_ctx* c, const LatCall& p, bool listed, int64_t a0, int64_t n_g, int64_t block, float2* d_q);
// the one-species source (p and idx outlive it)
BlockSource lattice_source(psa_ctx* c, const LatCall& p, const int32_t* idx);
// api_self.hip: a psa_self_spectra call and its pieces, shared with psa_self_correlations in the same way
struct SelfCall {
    DynCall  d;                                      // T, N, K, n_g; cut, L, H, n_seg, P (the rest unused)
    bool     shell = false;
    int64_t  cols = 0;
    float    box_hi[9], box_lo[9];
    std::vector<int64_t>  order;                     // the processing order: places in the caller's list
    std::vector<int32_t>  tile;                      // (2 (n_tiles + 1)): per tile its offset into ent, its first vector
    std::vector<uint16_t> ent;
    std::vector<uint32_t> slot;                      // (K) in the processing order
    std::vector<int32_t>  groups;                    // (2 (n_groups + 1)): first vector, column; the last pair ends the list
    std::vector<int64_t>  count;                     // (n_bins) vectors per bin (shell form)
    std::vector<double>   scale;                     // (cols)
    int64_t  n_tiles = 0, kt_max = 0, n_groups = 0;
    int64_t  at = 0, vt = 0, bs = 0;                 // atom tiles, vector tiles, segments per block
};
// every refusal, the plan and the block rule; `segments`: the context's segments are honoured (false: one boxcar
// segment of T frames, whatever the context holds -- the series before the window); n_lags > 0: a time-correlation call
int self_check(psa_ctx* c, const char* entry, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
               int64_t n_bins, const int32_t* idx, int64_t n_g, bool segments, int64_t n_lags, SelfCall* p);
int self_upload(psa_ctx* c, const SelfCall& p, const int32_t* idx, bool columns);
// atoms [a0, a0 + na) x tiles [t0, t0 + nt) x segments [s0, s0 + ns) into d_work (na, nv, ns, P)
int self_series(psa_ctx* c, const SelfCall& p, const int32_t* idx, int64_t a0, int64_t na, int64_t t0, int64_t nt, int64_t s0, int64_t ns,
                float2* d_work);
// The power part of a self call, shared by self_run, psa_debug_self_power and psa_self_correlations, which differ only in
// where the transformed series come from: the float64 accumulator (L, cols), zeroed; per block of Ab atoms x the vectors
// [vcut[b], vcut[b + 1]) of the processing order x bs segments the columns the block touches, the chunk rule, the power and
// reduce launches; with `finish` the finish pass into d_rc_out (else the sums stay in d_rc_acc).  The groups table
// (2 (n_groups + 1)) and the columns' scales are on the device already.  `fill` leaves the transformed block
// (na, nv, ns, L) on the device and says where.
struct SelfPower {
    int64_t        L = 0, n_seg = 0, n_atoms = 0, cols = 0, n_groups = 0;
    const int32_t* groups = nullptr;                 // the host's copy
    bool           mirror = false, finish = true;
    int64_t        Ab = 0, bs = 0, n_chunks = 0;     // atoms and segments per block; chunks of a block's atoms (0: the rule)
    const std::vector<int64_t>* vcut = nullptr;
};
using SelfFill = std::function<int(int64_t a0, int64_t na, int64_t vb, int64_t s0, int64_t ns, const float2** d_work)>;
int self_power_run(psa_ctx* c, const SelfPower& w, const SelfFill& fill);
// the blocks of a checked call, for self_run and psa_self_correlations: the vector blocks (runs of vt tiles) into vcut, the
// work buffer of one block with rows of d.P frames reserved, and everything of w but mirror and finish
int self_blocks(psa_ctx* c, const SelfCall& p, std::vector<int64_t>* vcut, SelfPower* w);

// ---- api_realspace.hip: what the real-space entries (api_msd.hip, api_pair.hip and, through api_shell.h, the entries on the
// neighbour shells) share.
// The atom groups (species) of a real-space call
struct AtomGroups {
    int64_t              T = 0, N = 0, n_a = 0, Ab = 0;   // Ab: atoms (msd) or origins (pair, shell) of a block
    int32_t              G = 1;
    bool                 listed = false;        // false: all N atoms in order, one group
    const int*           d_idx = nullptr;       // the atom list on the device once upload_atom_list has run (null: not listed)
    std::vector<int64_t> start;                 // (G + 1) the groups' offsets into the atom list
    std::vector<int64_t> size;                  // (G)
};
constexpr int64_t REALSPACE_TARGET_GROUPS = 4096;   // workgroups a launch aims at, where the work allows
// det a of a 3 x 3 matrix, refused ("<name> is singular") when it vanishes against the entries' scale; its inverse by cofactors
int  invertible_check(const double* a, const char* name, double* det);
void inverse3(const double* a, double det, double* out);
// what those entries refuse about the context (a communicator, no positions), the box and its inverse and the group
// lists (at most MSD_MAX_GROUPS, disjoint, in bounds); fills everything of p but Ab and d_idx
int group_list_check(psa_ctx* c, const char* entry, const double* box, const double* box_inverse, const int32_t* idx,
                     const int64_t* group_start, int32_t n_groups, AtomGroups* p);
// the radius `what` = r is within the served one: (1/2 - 2^-12) of the box's least perpendicular width, 1 / |column j of
// Hinv|, compared with a relative slack of 2^-40 (a caller who divides that radius by n_r and multiplies again is served)
int served_radius_check(const double* box_inverse, const char* what, double r);
// the arguments of a histogram over lags: the lags (at most max_lags, in [0, T - 1]), origin_step, the bin width and
// its float32 reciprocal (returned), the bins (at most max_bins)
int histogram_args_check(const AtomGroups& p, const int64_t* lags, int64_t n_lags, int max_lags, int64_t origin_step, double dr, int32_t n_r,
                         int max_bins, float* inv_dr);
// the atom list into d_rs_idx (nothing when the call lists none); sets p->d_idx
int upload_atom_list(psa_ctx* c, AtomGroups* p, const int32_t* idx);
// the rows of a table listed group by group -- group g's entries are first[g] .. first[g + 1] - 1, `per` rows each -- as the
// integer reduce takes them
int rows_of_groups(const int32_t* first, int n, int64_t per, HistRows* rows);
// ---- api_msd.hip: what the entries on unwrapped displacements (api_msd.hip, api_overlap.hip) share.
// group_list_check, unwrap in {0, 1}, and the block rule: p->Ab atoms of 24 T bytes each within the work budget (a budget
// below one atom is refused)
int msd_check(psa_ctx* c, const char* entry, const double* box, const double* box_inverse, const int32_t* idx,
              const int64_t* group_start, int32_t n_groups, int32_t unwrap, AtomGroups* p);
// the unwrap pass of atoms [a0, a0 + na) of the list into d_msd_u (and, with `images`, d_msd_img)
int msd_unwrap(psa_ctx* c, const AtomGroups& p, const double* box, const double* box_inverse, int64_t a0, int64_t na, bool unwrap,
               bool images);
// the chunk table of the block [a0, a0 + na): every group's part of it in runs of at most `ca` atoms, {first atom of the
// block, one past the last, group, 0}, group by group; first (G + 1): where each group's chunks begin
std::vector<int32_t> msd_chunks(const AtomGroups& p, int64_t a0, int64_t na, int64_t ca, int32_t* first);
// origin slabs and atoms per chunk of a launch with `rows` workgroups per (slab, chunk); a chunk holds at most ca_max atoms
void msd_split(const AtomGroups& p, int64_t rows, int64_t step, int64_t ca_max, int64_t* n_os, int64_t* ca);
// the atom list (d_rs_idx) and the groups' sizes (d_msd_sizes)
int msd_upload_list(psa_ctx* c, AtomGroups* p, const int32_t* idx);
int    check_weights(psa_ctx* c, int64_t N);            // the context's atom weights fit a slot of N atoms
void   set_geom_weights(const psa_ctx* c, ProjGeom* g);  // ... and go into a launch's geometry
int    begin_result(psa_ctx* c, int64_t T, int64_t K_total, int64_t k_offset, bool intensity, char** rows);

// sizes of the result in the context: one k-row of a slab over T frames; columns of the result; the whole result
inline size_t  row_bytes(int64_t T, bool intensity) { return intensity ? (size_t)T * sizeof(float) : (size_t)T * 3 * sizeof(float2); }
inline int64_t result_K(const psa_ctx* c) { return c->kmap.empty() ? c->res_K : c->out_K; }
inline size_t  result_bytes(const psa_ctx* c) { return row_bytes(c->res_T, c->res_intensity) * (size_t)result_K(c); }
inline size_t  intensity_bytes(const psa_ctx* c) { return row_bytes(c->res_T, true) * (size_t)result_K(c); }

}  // namespace psa
