// The hot path: k-list folding, plane cache, projection geometry, the block projector (phase table + projection
// launch), atom weights, segments, psa_sed_project / _project_upload / _calculate (pipelined) / _single_bin.
// (part of the C ABI of libpsa_hip.so, include/psa_hip.h; shared declarations: api_internal.h)
#include "api_internal.h"

namespace psa {

uint64_t hash_idx(const int32_t* p, int64_t n) {
    uint64_t h = 1469598103934665603ull ^ (uint64_t)n;
    for (int64_t i = 0; i < n; ++i) h = (h ^ (uint32_t)p[i]) * 1099511628211ull;
    return h;
}

// Pairs (k, -k) and repeated k-vectors of a list.  kmap[i] = index into the list of vectors that are
// actually projected (unique_idx: their positions in the input), | KMAP_MIRROR when vector i is the
// exact negation of that one.  Exact means component-wise float equality of k_i and -k_u (so -0 == 0;
// NaN never matches): then the float32 phase argument fma(kz,rz,fma(ky,ry,kx*rx)) is the exact negative
// (sed_calculator.py:78 -- rounding is symmetric), cos is even and sin odd, the data are real, hence
// q(-k) = conj q(k) and S(-k)[w] = conj S(k)[(T-w) mod T]: the partner needs no projection and no FFT
// of its own (the reference's own heat maps are symmetric about Gamma: examples/k_grid_heatmap_example.py:33-38).
void fold_pairs(const float* k, int64_t K, std::vector<int32_t>* kmap, std::vector<int32_t>* unique_idx) {
    struct Key {
        uint32_t x, y, z;
        bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; }
    };
    struct KeyHash {
        size_t operator()(const Key& a) const {
            uint64_t h = 1469598103934665603ull;
            for (uint32_t v : {a.x, a.y, a.z}) h = (h ^ v) * 1099511628211ull;
            return (size_t)h;
        }
    };
    auto bits = [](float v, bool negate) {
        if (negate) v = -v;
        if (v == 0.f) v = 0.f;                        // -0 and +0 are the same k
        uint32_t u;
        std::memcpy(&u, &v, sizeof(u));
        return u;
    };
    std::unordered_map<Key, int32_t, KeyHash> seen;   // k-vector -> its row among the projected ones
    seen.reserve((size_t)K * 2);
    kmap->assign((size_t)K, 0);
    unique_idx->clear();
    for (int64_t i = 0; i < K; ++i) {
        const float* v = k + 3 * i;
        const bool   has_nan = v[0] != v[0] || v[1] != v[1] || v[2] != v[2];
        const Key    same{bits(v[0], false), bits(v[1], false), bits(v[2], false)};
        const Key    neg{bits(v[0], true), bits(v[1], true), bits(v[2], true)};
        if (!has_nan) {
            auto it = seen.find(same);
            if (it != seen.end()) {
                (*kmap)[i] = it->second;
                continue;
            }
            it = seen.find(neg);
            if (it != seen.end()) {
                (*kmap)[i] = it->second | KMAP_MIRROR;
                continue;
            }
        }
        const int32_t row = (int32_t)unique_idx->size();
        unique_idx->push_back((int32_t)i);
        (*kmap)[i] = row;
        if (!has_nan) seen.emplace(same, row);
    }
}

// the list the projection runs on when folding pays: *uniq_k receives the vectors to project and *kmap
// the k map (the caller installs it with install_kmap after begin_result); false = project the list as it is
static bool fold_k_list(psa_ctx* c, const float* k, int64_t K, std::vector<float>* uniq_k, std::vector<int32_t>* kmap) {
    if (!c->opt_fold_pairs || K < 2 || K >= (1ll << 30)) return false;
    std::vector<int32_t> uidx;
    fold_pairs(k, K, kmap, &uidx);
    if ((int64_t)uidx.size() == K) return false;
    uniq_k->resize(uidx.size() * 3);
    for (size_t u = 0; u < uidx.size(); ++u) std::memcpy(uniq_k->data() + 3 * u, k + 3 * (size_t)uidx[u], 3 * sizeof(float));
    return true;
}

int install_kmap(psa_ctx* c, const std::vector<int32_t>& kmap) {
    c->kmap = kmap;
    c->out_K = (int64_t)kmap.size();
    c->out_valid = false;
    return upload(c, c->d_kmap, c->kmap.data(), c->kmap.size() * sizeof(int32_t));
}

size_t planes_bytes_held(psa_ctx* c) {
    size_t b = 0;
    for (auto& ps : c->planes) b += ps->buf.cap;
    return b;
}

// plane sets built from contents a slot no longer holds
void drop_stale_planes(psa_ctx* c) {
    auto& v = c->planes;
    v.erase(std::remove_if(v.begin(), v.end(),
                           [&](const std::unique_ptr<PlaneSet>& ps) {
                               const DataSlot& s = c->slot[ps->slot];
                               return !(s.valid && s.generation == ps->generation);
                           }),
            v.end());
}

// least recently used set that the call in progress has not touched; false if there is none
bool evict_one_plane_set(psa_ctx* c) {
    int victim = -1;
    for (size_t i = 0; i < c->planes.size(); ++i)
        if (c->planes[i]->last_use < c->plane_call_mark &&
            (victim < 0 || c->planes[i]->last_use < c->planes[victim]->last_use))
            victim = (int)i;
    if (victim < 0) return false;
    c->planes.erase(c->planes.begin() + victim);
    return true;
}

// The group's split planes (k1_planes.hip): found in the cache, or built now if the policy
// (PSA_OPT_PLANES*) and HBM allow; *out stays nullptr otherwise and the caller projects with the
// kernels that split on the fly.  v: the group and the slot its data is in.
// mean_host non-null: planes of slot - mean (displacement mode; the mean is also in d_mean_all).
int get_planes(psa_ctx* c, const GroupView& v, int64_t K_local, const float* mean_host, PlaneSet** out) {
    *out = nullptr;
    if (c->k1_selector != PSA_K1_AUTO || !c->opt_planes) return PSA_OK;
    const int      slot = v.slot;
    const int32_t* h_idx = v.h_idx;
    const int64_t  n_g = v.n_g;
    DataSlot&      s = c->slot[slot];
    drop_stale_planes(c);
    const bool     all = h_idx == nullptr, displaced = mean_host != nullptr;
    const uint64_t h = (all ? 0 : hash_idx(h_idx, n_g)) ^ (displaced ? 0x9E3779B97F4A7C15ull : 0);
    const size_t   n_mean = (size_t)s.N * 3;
    for (auto& ps : c->planes)
        if (ps->slot == slot && ps->all_atoms == all && ps->n_g == n_g && ps->displaced == displaced &&
            (all || (ps->idx_hash == h && std::memcmp(ps->idx.data(), h_idx, (size_t)n_g * sizeof(int32_t)) == 0)) &&
            (!displaced || (ps->mean.size() == n_mean && std::memcmp(ps->mean.data(), mean_host, n_mean * sizeof(float)) == 0))) {
            ps->last_use = ++c->plane_tick;
            *out = ps.get();
            return PSA_OK;
        }
    // nothing cached: short k-lists are not worth a set of their own (their "3 x bf16" kernel streams the
    // float32 array at the same HBM-bound rate: 4.17 vs 4.10 ms at 16 k-vectors) -- but they use one that exists
    if (K_local < c->opt_planes_min_k) return PSA_OK;
    if (!all && !c->opt_planes_eager) {              // an index list seen for the first time: not yet
        auto& seen = c->seen_groups;
        if (std::find(seen.begin(), seen.end(), h) == seen.end()) {
            seen.push_back(h);
            if (seen.size() > 256) seen.erase(seen.begin());
            return PSA_OK;
        }
    }
    unsigned bits = 0;
    if (displaced) {
        PSA_TRY(displaced_absmax(c, slot, mean_host, h_idx, n_g, &bits));
    } else if (all) {
        PSA_TRY(slot_absmax(c, slot));
        bits = s.absmax_bits;
    } else {
        PSA_TRY(group_absmax(c, slot, h_idx, n_g, &bits));
    }
    const float vscale = k1_f16_vscale(bits);
    if (!(vscale > 0.f)) return PSA_OK;              // NaN / Inf in the data: the bf16 kernel propagates them
    const int     A_pad = k1_pair_atom_pad(n_g);
    const int64_t n_fg = (s.T + 15) / 16;
    const size_t  bytes = plane_bytes(n_fg, A_pad / K1_BA);
    size_t        free_b = 0, total_b = 0;
    PSA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = c->opt_planes_budget > 0 ? (size_t)c->opt_planes_budget : (size_t)(0.45 * (double)total_b);
    if (bytes > budget) return PSA_OK;
    while (planes_bytes_held(c) + bytes > budget)
        if (!evict_one_plane_set(c)) return PSA_OK;
    const size_t reserve = (size_t)2 << 30;          // leave room for slabs, FFT work buffers, results
    while (free_b < bytes + reserve) {
        if (!evict_one_plane_set(c)) return PSA_OK;
        PSA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    }
    auto ps = std::make_unique<PlaneSet>();
    if (c->scratch_byte >= 0) ps->buf.fill = &c->scratch_byte;   // armed (psa_debug_scratch_fill)
    if (ps->buf.reserve(bytes) != PSA_OK) {
        (void)hipGetLastError();
        return PSA_OK;
    }
    {
        HostTimer ht(&c->oneoff_ms[2]);                 // timed: the stream is drained once per set
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
        PSA_TRY(launch_split_planes(c, s.buf.as<float>(), displaced ? c->d_mean_all.as<float>() : nullptr, v.d_idx, ps->buf.ptr,
                                    s.T, s.N, (int)n_g, A_pad, vscale));
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    ps->slot = slot;
    ps->generation = s.generation;
    ps->all_atoms = all;
    if (!all) ps->idx.assign(h_idx, h_idx + n_g);
    ps->idx_hash = h;
    ps->displaced = displaced;
    if (displaced) ps->mean.assign(mean_host, mean_host + n_mean);
    ps->T = s.T;
    ps->n_fg = n_fg;
    ps->n_g = (int)n_g;
    ps->A_pad = A_pad;
    ps->vscale = vscale;
    ps->last_use = ++c->plane_tick;
    *out = ps.get();
    c->planes.push_back(std::move(ps));
    return PSA_OK;
}

// Per-atom weights (psa_set_atom_weights) of a projection over a slot of N atoms: none set, or N of them
int check_weights(psa_ctx* c, int64_t N) {
    PSA_REQUIRE(c->weights_N == 0 || c->weights_N == N, "atom weights were set for %lld atoms, the trajectory has %lld",
                (long long)c->weights_N, (long long)N);
    return PSA_OK;
}

void set_geom_weights(const psa_ctx* c, ProjGeom* g) {
    g->weights = c->weights_N ? c->d_weights.as<float>() : nullptr;
    g->wscale = c->weights_N ? c->weights_scale : 1.f;
}

// geometry and kernel family of K_local k-vectors of one group (v: resolved by group_source) under the rule
int make_geom(psa_ctx* c, const GroupView& v, int64_t K_local, GeomRule rule, ProjGeom* g) {
    const int     slot = v.slot;
    const int64_t n_g = v.n_g;
    set_geom_weights(c, g);
    g->T = c->slot[slot].T;
    g->q_stride = g->T;
    g->N_tot = c->slot[slot].N;
    PSA_REQUIRE(n_g < (1ll << 30) && K_local < (1ll << 29), "group or k-list too large");
    g->n_g = (int)n_g;
    g->A_pad = (int)((n_g + 31) / 32 * 32);
    g->K = (int)K_local;
    // product path: split-precision matrix-core kernels -- "2 x f16" from the group's cached planes,
    // or splitting on the fly (more than 16 k-vectors, no NaN/Inf), "3 x bf16" for every other
    // group; exact-fp32 MFMA kernel for displacement mode when no displacement array could be made
    g->split = K1Family::f32;
    const bool autosel = c->k1_selector == PSA_K1_AUTO;
    if (v.ps && rule == GeomRule::product) {
        g->split = K1Family::f16_planes;
        g->vscale = v.ps->vscale;
        g->m_blk = k1_planes_block_rows((int)K_local, c->opt_k1_wide != 0);
        g->A_pad = v.ps->A_pad;
        g->M_pad = (int)((2 * K_local + g->m_blk - 1) / g->m_blk * g->m_blk);
        return PSA_OK;
    }
    if (rule == GeomRule::product && autosel && k1_pair_eligible(v.d_idx, g->N_tot, n_g, K_local, v.disp)) {
        unsigned bits = 0;
        if (v.h_idx) {
            PSA_TRY(group_absmax(c, slot, v.h_idx, n_g, &bits));
        } else {
            PSA_TRY(slot_absmax(c, slot));
            bits = c->slot[slot].absmax_bits;
        }
        g->vscale = k1_f16_vscale(bits);
        if (g->vscale > 0.f) g->split = K1Family::f16_fly;
    }
    if (g->split == K1Family::f32 && rule != GeomRule::f32_only && (autosel || c->k1_selector == PSA_K1_SPLIT_BF16) &&
        k1_split_eligible(v.d_idx, g->N_tot, n_g, v.disp))
        g->split = K1Family::bf16;
    if (g->split == K1Family::f16_fly) {
        g->m_blk = k1_pair_block_rows((int)K_local);
        g->A_pad = k1_pair_atom_pad(n_g);
    } else {
        g->m_blk = g->split == K1Family::bf16 ? k1_split_block_rows((int)K_local) : k1_mfma_block_rows((int)K_local);
    }
    g->M_pad = (int)((2 * K_local + g->m_blk - 1) / g->m_blk * g->m_blk);
    return PSA_OK;
}

// phase table of one group in the image its projection kernel wants (+ the group's mean positions
// for the subtract-while-staging kernels); the launch's k-vectors start at k_first of the uploaded list
int prepare_phase(psa_ctx* c, const GroupView& v, const ProjGeom& g, int64_t k_first) {
    const int*   d_idx = v.d_idx;
    const float* d_kvec = c->d_kvec.as<float>() + 3 * k_first;
    const bool   f16 = g.split == K1Family::f16_fly || g.split == K1Family::f16_planes, bf16 = g.split == K1Family::bf16;
    if (g.lowrank) {      // the D image and the node table (the plan's fp64 inputs were uploaded by prepare_lowrank)
        PSA_TRY(c->d_lr_diff.reserve(pd16_table_bytes(g.M_pad_d, g.A_pad)));
        PSA_TRY(c->d_phase.reserve(pf16_table_bytes(128, g.A_pad)));
        StageTimer    st(c, PSA_T_PHASE);
        const double* f64 = c->d_lr_f64.as<double>();
        if (g.lr_nodes == 48)     // the 48-node table, and the image of everything its hi piece does not carry
            return launch_lowrank_tables_n48(c, d_kvec, f64, f64 + 7, c->d_mean_all.as<float>(), d_idx, c->d_lr_L.as<float>(),
                                             c->d_lr_phi.as<float2>(), c->d_lr_diff.ptr, c->d_phase.ptr, g, g.M_pad_d, g.dscale, g.lr_pair);
        if (g.lr_fold)     // the folded image is built from the node table and the combine's L and phi
            return launch_lowrank_tables_fold(c, d_kvec, f64 + 7 + LOWRANK_NODES, f64, f64 + 7, c->d_mean_all.as<float>(), d_idx,
                                              c->d_lr_L.as<float>(), c->d_lr_phi.as<float2>(), c->d_lr_diff.ptr, c->d_phase.ptr, g,
                                              g.M_pad_d, g.dscale, g.lr_pair);
        return launch_lowrank_tables(c, d_kvec, f64 + 7 + LOWRANK_NODES, f64, f64 + 7, c->d_mean_all.as<float>(), d_idx,
                                     c->d_lr_diff.ptr, c->d_phase.ptr, g, g.M_pad_d, g.dscale, g.lr_pair);
    }
    PSA_TRY(c->d_phase.reserve(f16    ? pf16_table_bytes(g.M_pad, g.A_pad)
                               : bf16 ? pb_table_bytes(g.M_pad, g.A_pad)
                                      : p_table_floats(g.M_pad, g.A_pad) * sizeof(float)));
    StageTimer st(c, PSA_T_PHASE);
    if (f16)
        PSA_TRY(launch_phase_table_f16(c, d_kvec, c->d_mean_all.as<float>(), d_idx, c->d_phase.ptr, g));
    else if (bf16)
        PSA_TRY(launch_phase_table_split(c, d_kvec, c->d_mean_all.as<float>(), d_idx, c->d_phase.ptr, g));
    else
        PSA_TRY(launch_phase_table(c, d_kvec, c->d_mean_all.as<float>(), d_idx, c->d_phase.as<float>(), g));
    if (v.disp) {
        PSA_TRY(c->d_mean_g.reserve((size_t)g.A_pad * 3 * sizeof(float)));
        PSA_TRY(launch_gather_mean(c, c->d_mean_all.as<float>(), d_idx, c->d_mean_g.as<float>(), g));
    }
    return PSA_OK;
}

// projection of frames [t_begin, t_begin + t_count) of one group into columns t_begin.. of q
// (K_local,3,q_stride); the phase table is in place
static int launch_projection_once(psa_ctx* c, const GroupView& v, ProjGeom g, float2* d_q, int64_t q_stride, int64_t t_begin,
                                  int64_t t_count);

int launch_projection(psa_ctx* c, const GroupView& v, ProjGeom g, float2* d_q, int64_t q_stride, int64_t t_begin,
                      int64_t t_count) {
    // PSA_DEBUG_REPEAT_K1=n (diagnostics, tools/short_loop_timing.py): the same launch n times back to back,
    // each timed on its own (psa_k1_stats) -- the result is that of one launch
    static const int reps = [] {
        const char* e = std::getenv("PSA_DEBUG_REPEAT_K1");
        return e ? std::max(1, std::atoi(e)) : 1;
    }();
    for (int r = 0; r < reps; ++r) PSA_TRY(launch_projection_once(c, v, g, d_q, q_stride, t_begin, t_count));
    return PSA_OK;
}

static int launch_projection_once(psa_ctx* c, const GroupView& v, ProjGeom g, float2* d_q, int64_t q_stride, int64_t t_begin,
                                  int64_t t_count) {
    const DataSlot& s = c->slot[v.slot];
    const PlaneSet* ps = v.ps;
    PSA_REQUIRE(t_begin >= 0 && t_count > 0 && t_begin + t_count <= s.T && q_stride >= t_begin + t_count,
                "frame range [%lld,%lld) outside the slot", (long long)t_begin, (long long)(t_begin + t_count));
    g.T = t_count;
    g.q_stride = q_stride;
    StageTimer   st(c, PSA_T_PROJECT);
    const float* d_v = s.buf.as<float>() + (size_t)t_begin * 3 * (size_t)s.N;
    d_q += t_begin;
    if (g.split == K1Family::f16_planes) {
        PSA_REQUIRE(ps != nullptr && t_begin % 16 == 0, "planes are cut in groups of 16 frames");
        const int64_t fg0 = t_begin / 16, n_fg = ps->n_fg - fg0;        // frame groups from the launch's first frame on
        const _Float16* pl = ps->buf.as<_Float16>() + (size_t)fg0 * (size_t)(ps->A_pad / K1_BA) * PL_STAGE_ELEMS;
        // PSA_OPT_K1_LOADER_WAVES [1]: 128-row M blocks go to the loader-wavefront form of the kernel
        // (k1_planes_lw.hip; 2-3 % faster than the eight-wavefront form on every shape, round 3); 0 = never
        if (g.lowrank) {
            // node rows (the 128-row planes kernel on the node table in d_phase) -> d_lr_qn; D pass -> q; q += C Qn (C = phi L)
            ProjGeom gn = g;
            gn.K = g.lr_nodes;                                             // (48 nodes: rows 96..127 of the block are padding)
            gn.m_blk = gn.M_pad = 2 * LOWRANK_NODES;
            gn.q_stride = t_count;
            PSA_REQUIRE(g.lr_nodes == LOWRANK_NODES || (g.lr_nodes == 48 && g.lr_fold), "48 nodes only with the fold");
            PSA_REQUIRE(c->d_lr_qn.cap >= (size_t)g.lr_nodes * 3 * t_count * sizeof(float2), "node projections not reserved");
            if (g.lr_pair) {      // one 512-row D block: both in one launch of balanced row pairs (the D image is in its layout)
                PSA_TRY((g.lr_nodes == 48 ? launch_k1_lowrank_n48
                         : g.lr_fold      ? launch_k1_lowrank_fold
                                          : launch_k1_lowrank_pair)(c, pl, c->d_phase.ptr, c->d_lr_diff.ptr, c->d_lr_qn.as<float2>(), d_q,
                                                                    g, n_fg, g.dscale));
                ++c->lowrank_pair_launches;
            } else {
                PSA_TRY((g.lr_fold ? launch_k1_planes_lw2 : launch_k1_planes_lw)(c, pl, c->d_phase.ptr, c->d_lr_qn.as<float2>(), gn, n_fg));
                ProjGeom gd = g;
                gd.M_pad = g.M_pad_d;
                PSA_TRY(launch_k1_planes_diff(c, pl, c->d_lr_diff.ptr, d_q, gd, n_fg, g.dscale));
            }
            PSA_TRY(launch_lowrank_combine_r(c, c->d_lr_qn.as<float2>(), c->d_lr_L.as<float>(), c->d_lr_phi.as<float2>(), d_q, g,
                                             t_count));
            ++c->lowrank_launches;
            return PSA_OK;
        }
        if (g.m_blk == 256) return launch_k1_planes_wide(c, pl, c->d_phase.ptr, d_q, g, n_fg);
        if (g.m_blk == 128 && c->opt_k1_loader_waves) return launch_k1_planes_lw(c, pl, c->d_phase.ptr, d_q, g, n_fg);
        return launch_k1_planes(c, pl, c->d_phase.ptr, d_q, g, n_fg);
    }
    if (g.split == K1Family::f16_fly) return launch_k1_pair(c, d_v, c->d_phase.ptr, v.d_idx, d_q, g);
    if (g.split == K1Family::bf16) return launch_k1_split(c, d_v, c->d_phase.ptr, v.d_idx, d_q, g);
    if (c->k1_selector == PSA_K1_WAVE)
        return launch_k1_wave(c, d_v, c->d_phase.as<float>(), v.d_idx, c->d_mean_g.as<float>(), d_q, g, v.disp);
    return launch_k1_mfma(c, d_v, c->d_phase.as<float>(), v.d_idx, c->d_mean_g.as<float>(), d_q, g, v.disp);
}

// (api_internal.h) -- a new kernel route is wired in here and in launch_projection, nowhere else
int prepare_block(psa_ctx* c, const GroupView& v, GeomRule rule, const ProjectArgs* lowrank, int64_t k_first, int64_t nk,
                  ProjGeom* g) {
    PSA_TRY(make_geom(c, v, nk, rule, g));
    if (lowrank) PSA_TRY(prepare_lowrank(c, v, *lowrank, k_first, nk, g));
    return prepare_phase(c, v, *g, k_first);
}

int project_block(psa_ctx* c, const GroupView& v, const ProjectArgs* lowrank, int64_t k_first, int64_t nk, float2* d_q) {
    const int64_t T = c->slot[v.slot].T;
    ProjGeom      g;
    PSA_TRY(prepare_block(c, v, GeomRule::product, lowrank, k_first, nk, &g));
    return launch_projection(c, v, g, d_q, T, 0, T);
}

// Where one group's data comes from.  In order: its cached split planes -- of the velocities, or of
// positions - mean built straight from the positions (no float32 displacement array) -- else the
// float32 slot, which in displacement mode is the materialised positions - mean array (or, when HBM
// has no room for it, the positions themselves with the subtract-while-staging kernel).
// The view comes in with the caller's slot and PSA_F_DISPLACEMENTS and goes out with what the
// projection has to be launched with (slot, disp, ps).
int group_source(psa_ctx* c, GroupView* v, const float* mean_host, int64_t K) {
    PSA_TRY(get_planes(c, *v, K, v->disp ? mean_host : nullptr, &v->ps));
    if (v->ps) {
        v->disp = false;                                          // the planes already hold slot - mean
        return PSA_OK;
    }
    return materialise_displacements(c, v, mean_host);
}

// (api_internal.h)
int check_group_indices(const GroupView& v, int64_t N) {
    for (int64_t i = 0; v.h_idx && i < v.n_g; ++i)
        PSA_REQUIRE(v.h_idx[i] >= 0 && v.h_idx[i] < N, "Atom indices in basis out of bounds.");
    return PSA_OK;
}

int upload_single_group(psa_ctx* c, GroupView* v, int64_t N, const float* k_vectors, int64_t K, const float* mean_pos_all) {
    if (v->n_g == 0) return PSA_OK;
    PSA_TRY(upload(c, c->d_kvec, k_vectors, (size_t)K * 3 * sizeof(float)));
    PSA_TRY(upload(c, c->d_mean_all, mean_pos_all, (size_t)N * 3 * sizeof(float)));
    if (v->h_idx) PSA_TRY(upload(c, c->d_idx, v->h_idx, (size_t)v->n_g * sizeof(int32_t)));
    v->d_idx = v->h_idx ? c->d_idx.as<int>() : nullptr;           // (after the upload: the buffer may have moved)
    return PSA_OK;
}

int check_project_args(psa_ctx* c, const ProjectArgs& a, int64_t N) {
    PSA_REQUIRE(a.mean_pos_all != nullptr, "null mean_pos_all");
    PSA_REQUIRE(a.K_local >= 0 && a.K_total >= 1 && a.k_offset >= 0 && a.k_offset + a.K_local <= a.K_total,
                "k range [%lld,%lld) outside [0,%lld)", (long long)a.k_offset, (long long)(a.k_offset + a.K_local),
                (long long)a.K_total);
    PSA_REQUIRE(a.K_local == 0 || a.k_vectors != nullptr, "null k_vectors");
    PSA_TRY(validate_groups(N, a.group_idx, a.group_off, a.G));
    PSA_REQUIRE((a.flags & PSA_F_INTENSITY) || a.G == 1, "complex output needs exactly one atom group (got %d)", a.G);
    (void)c;
    return PSA_OK;
}

// result slab (k-major) of a calculation over T frames; returns the rows of this call
int begin_result(psa_ctx* c, int64_t T, int64_t K_total, int64_t k_offset, bool intensity, char** rows) {
    PSA_TRY(c->d_slab.reserve(row_bytes(T, intensity) * (size_t)K_total));
    c->res_T = T;
    c->res_K = K_total;
    c->res_intensity = intensity;
    c->slab_valid = true;
    c->out_valid = false;
    c->inten_valid = false;
    c->kmap.clear();
    c->out_K = K_total;
    c->plane_call_mark = c->plane_tick + 1;
    *rows = (char*)c->d_slab.ptr + row_bytes(T, intensity) * (size_t)k_offset;
    return PSA_OK;
}

int upload_project_inputs(psa_ctx* c, const ProjectArgs& a, int64_t N) {
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_kvec, a.k_vectors, (size_t)a.K_local * 3 * sizeof(float)));
    PSA_TRY(upload(c, c->d_mean_all, a.mean_pos_all, (size_t)N * 3 * sizeof(float)));
    if (a.group_idx) PSA_TRY(upload(c, c->d_idx, a.group_idx, (size_t)a.group_off[a.G] * sizeof(int32_t)));
    return PSA_OK;
}

// ---- Welch segments (psa_set_segments) --------------------------------------------------------------------------------
// A projection over T frames while segments are set: intensity only, L <= T
int check_segments(psa_ctx* c, int64_t T, int32_t flags) {
    if (c->seg_L == 0) return PSA_OK;
    PSA_REQUIRE(flags & PSA_F_INTENSITY, "segment-averaged spectra are intensities: PSA_F_INTENSITY is required while segments are set");
    PSA_REQUIRE(c->seg_L <= T, "segment length %lld exceeds the trajectory's %lld frames", (long long)c->seg_L, (long long)T);
    return PSA_OK;
}

// frequency bins of a result over T frames: L while segments are set
static int64_t result_frames(const psa_ctx* c, int64_t T) { return c->seg_L ? c->seg_L : T; }

// Blocks of the segment stage: nk k-vectors x ns segments, so that the segment buffer (3 L complex64 per k-vector and
// segment) never holds more than the q buffer (K_local,3,T).  L <= T: at least K_local (k, segment) units fit.
static void segment_blocks(const psa_ctx* c, int64_t T, int64_t K_local, int64_t* nk, int64_t* ns) {
    const int64_t n_seg = 1 + (T - c->seg_L) / c->seg_hop;
    const int64_t units = std::max<int64_t>(1, K_local * T / c->seg_L);
    if (units >= n_seg) {
        *ns = n_seg;
        *nk = std::max<int64_t>(1, std::min(K_local, units / n_seg));
    } else {
        *ns = units;
        *nk = 1;
    }
}

// In place of the length-T FFT and intensity_accumulate: q (K_local,3,T) of one group -> windowed segments -> batched
// length-L FFT -> inv_norm sum_s sum_c |F/L|^2 into the slab rows (K_local, L); first: the call's first group
static int segment_stage(psa_ctx* c, const float2* d_q, int64_t T, int64_t K_local, float* rows, bool first) {
    const int64_t L = c->seg_L, H = c->seg_hop, n_seg = 1 + (T - L) / H;
    int64_t       nk = 0, ns = 0;
    segment_blocks(c, T, K_local, &nk, &ns);
    const float inv_norm = (float)(1.0 / ((double)n_seg * c->seg_U));   // exactly 1 for w = 1, one segment
    PSA_TRY(c->d_seg.reserve((size_t)nk * 3 * (size_t)ns * (size_t)L * sizeof(float2)));
    float2* d_seg = c->d_seg.as<float2>();
    for (int64_t k0 = 0; k0 < K_local; k0 += nk) {
        const int64_t bk = std::min(nk, K_local - k0);
        for (int64_t s0 = 0; s0 < n_seg; s0 += ns) {
            const int64_t bs = std::min(ns, n_seg - s0);
            {
                StageTimer st(c, PSA_T_EPILOGUE);
                PSA_TRY(launch_segment_window(c, d_q + (size_t)k0 * 3 * (size_t)T, c->d_seg_window.as<float>(), d_seg, T, L, H, s0,
                                              bs, bk));
            }
            {
                StageTimer st(c, PSA_T_FFT);
                PSA_TRY(run_fft(c, d_seg, L, 3 * bk * bs));
            }
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_segment_power(c, d_seg, rows + (size_t)k0 * (size_t)L, L, bs, bk, inv_norm, first && s0 == 0));
        }
    }
    return PSA_OK;
}

// What follows one group's projection: the FFT of q (K_local,3,T) and, for an intensity result, its accumulation into
// the slab rows -- or, while segments are set, the segment stage.  first: the call's first group
static int spectrum_stage(psa_ctx* c, float2* d_q, int64_t T, int64_t K_local, bool intensity, float* rows, bool first) {
    if (c->seg_L) return segment_stage(c, d_q, T, K_local, rows, first);
    {
        StageTimer st(c, PSA_T_FFT);
        PSA_TRY(run_fft(c, d_q, T, 3 * K_local));
    }
    if (intensity) {
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_intensity_accumulate(c, d_q, rows, T, K_local, first));
    }
    return PSA_OK;
}

// groups [g_first, G) on the resident slot: project, then the spectrum stage
static int project_groups(psa_ctx* c, const ProjectArgs& a, int g_first, bool* first, char* rows, float2* d_q) {
    const int64_t T = c->slot[a.slot].T, N = c->slot[a.slot].N;
    for (int gi = g_first; gi < a.G; ++gi) {
        GroupView v{a.slot, (a.flags & PSA_F_DISPLACEMENTS) != 0};
        set_group(c, a.group_idx, a.group_off, gi, N, &v);
        if (v.n_g == 0) continue;                                 // sed_calculator.py:64-65, 319-321
        PSA_TRY(group_source(c, &v, a.mean_pos_all, a.K_local));
        // the phase table holds 8 bytes per (k-vector, atom): very long k-lists (a 500 x 500 grid) are
        // projected in blocks whose table stays under 2 GiB (the reference chunks k for the same reason,
        // sed_calculator.py:268-272); ordinary lists are one block
        const int64_t per_k = 8 * ((v.n_g + 63) / 64 * 64);
        int64_t       table = (int64_t)2 << 30;
        if (const char* e = std::getenv("PSA_PHASE_TABLE_MIB")) table = (int64_t)std::max(1, std::atoi(e)) << 20;
        int64_t kb = std::max<int64_t>(64, (table / per_k) / 64 * 64);
        if (a.K_local <= kb + 64) kb = a.K_local;
        for (int64_t k0 = 0; k0 < a.K_local; k0 += kb)
            PSA_TRY(project_block(c, v, &a, k0, std::min(kb, a.K_local - k0), d_q + (size_t)k0 * 3 * (size_t)T));
        PSA_TRY(spectrum_stage(c, d_q, T, a.K_local, (a.flags & PSA_F_INTENSITY) != 0, (float*)rows, *first));
        *first = false;
    }
    return PSA_OK;
}

// Start of the list-level entry points, after their checks: the list folded where the whole of it is on this device
// (k-vectors whose negation or twin is in the list are not projected; *a then names the vectors to project, kept in
// *uniq_k -- non-empty exactly when the list was folded -- with *kmap their k map), the result begun over the slot's
// frames, the k map installed, the inputs uploaded; *rows: this call's rows of the slab, *d_q: where a group's q goes
// (the rows themselves for a complex result).  An empty list stops before the upload.
static int begin_list(psa_ctx* c, ProjectArgs* a, std::vector<float>* uniq_k, std::vector<int32_t>* kmap, char** rows,
                      float2** d_q) {
    const int64_t T = c->slot[a->slot].T, N = c->slot[a->slot].N;
    const bool    intensity = (a->flags & PSA_F_INTENSITY) != 0;
    const bool folded = a->K_local == a->K_total && a->k_offset == 0 && fold_k_list(c, a->k_vectors, a->K_local, uniq_k, kmap);
    if (folded) {
        a->k_vectors = uniq_k->data();
        a->K_local = a->K_total = (int64_t)uniq_k->size() / 3;
    }
    PSA_TRY(begin_result(c, result_frames(c, T), a->K_total, a->k_offset, intensity, rows));
    if (folded) PSA_TRY(install_kmap(c, *kmap));
    if (a->K_local == 0) return PSA_OK;
    PSA_TRY(upload_project_inputs(c, *a, N));
    *d_q = (float2*)*rows;
    if (intensity) {
        PSA_TRY(c->d_qwork.reserve((size_t)a->K_local * 3 * T * sizeof(float2)));
        *d_q = c->d_qwork.as<float2>();
    }
    return PSA_OK;
}

}  // namespace psa

using namespace psa;

extern "C" {

int psa_set_atom_weights(psa_ctx* c, const float* w, int64_t N) {
    PSA_TRY(enter(c));
    Guard guard(c);
    if (w == nullptr) {
        c->weights_N = 0;
        c->weights_scale = 1.f;
        return PSA_OK;
    }
    PSA_REQUIRE(N >= 1 && N < (1ll << 31), "bad atom count %lld", (long long)N);
    float wmax = 0.f;
    for (int64_t a = 0; a < N; ++a) {
        PSA_REQUIRE(std::isfinite(w[a]), "atom weight %lld is not finite", (long long)a);
        wmax = std::max(wmax, std::fabs(w[a]));
    }
    // 2^e: the smallest power of two >= max|w| (all zero: 1), kept inside the float range
    int e = 0;
    if (wmax > 0.f) {
        const float m = std::frexp(wmax, &e);        // wmax = m 2^e, m in [0.5, 1)
        if (m == 0.5f) --e;
        e = std::min(127, std::max(-126, e));
    }
    c->weights_N = 0;                                  // (no weights if the copy fails)
    PSA_TRY(upload(c, c->d_weights, w, (size_t)N * sizeof(float)));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));   // the caller's array is only read during the call
    c->weights_N = N;
    c->weights_scale = std::ldexp(1.f, e);
    return PSA_OK;
}

int psa_set_segments(psa_ctx* c, int64_t L, int64_t hop, const float* window) {
    PSA_TRY(enter(c));
    Guard guard(c);
    if (L == 0) {
        c->seg_L = c->seg_hop = 0;
        c->seg_U = 0.0;
        return PSA_OK;
    }
    PSA_REQUIRE(L >= 2 && L < (1ll << 31), "bad segment length %lld", (long long)L);
    PSA_REQUIRE(hop >= 1, "segment hop %lld < 1", (long long)hop);
    PSA_REQUIRE(window != nullptr, "null window");
    double u = 0.0;
    bool   boxcar = true;
    for (int64_t t = 0; t < L; ++t) {
        PSA_REQUIRE(std::isfinite(window[t]), "window value %lld is not finite", (long long)t);
        u += (double)window[t] * (double)window[t];
        boxcar = boxcar && window[t] == 1.0f;
    }
    u /= (double)L;
    PSA_REQUIRE(u > 0.0, "the window is zero everywhere (U = 0)");
    c->seg_L = 0;                                      // (no segments if the copy fails)
    PSA_TRY(upload(c, c->d_seg_window, window, (size_t)L * sizeof(float)));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));   // the caller's array is only read during the call
    c->seg_L = L;
    c->seg_hop = hop;
    c->seg_U = u;
    c->seg_boxcar = boxcar;
    return PSA_OK;
}

int psa_sed_project(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors,
                    int64_t K_local, int64_t K_total, int64_t k_offset, const int32_t* group_idx,
                    const int64_t* group_off, int32_t G, int32_t flags) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_TRY(check_slot(c, slot));
    ProjectArgs   a{slot, mean_pos_all, k_vectors, K_local, K_total, k_offset, group_idx, group_off, G, flags};
    const int64_t T = c->slot[slot].T, N = c->slot[slot].N;
    PSA_TRY(check_project_args(c, a, N));
    PSA_TRY(check_weights(c, N));
    PSA_TRY(check_segments(c, T, flags));
    std::vector<float>   uniq_k;
    std::vector<int32_t> kmap;
    char*                rows = nullptr;
    float2*              d_q = nullptr;
    PSA_TRY(begin_list(c, &a, &uniq_k, &kmap, &rows, &d_q));
    if (a.K_local == 0) return PSA_OK;
    bool first = true;
    PSA_TRY(project_groups(c, a, 0, &first, rows, d_q));
    if (first)   // every group empty: the rows are zero
        PSA_HIP_CHECK(hipMemsetAsync(rows, 0, row_bytes(c->res_T, c->res_intensity) * (size_t)a.K_local, c->stream));
    return PSA_OK;
}

// Upload and project, overlapped (psa_hip.h).  The first non-empty group is projected chunk by
// chunk behind the copies, with a kernel that needs nothing from frames not yet seen: "3 x bf16"
// (no scale), or the float32 kernel that subtracts the mean while staging in displacement mode.
int psa_sed_project_upload(psa_ctx* c, int slot, const float* host, int64_t T, int64_t N, const float* mean_pos_all,
                           const float* k_vectors, int64_t K, const int32_t* group_idx, const int64_t* group_off,
                           int32_t G, int32_t flags) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(host != nullptr, "null host array");
    PSA_REQUIRE(K >= 1, "need at least one k-vector");
    Guard       guard(c);
    ProjectArgs a{slot, mean_pos_all, k_vectors, K, K, 0, group_idx, group_off, G, flags};
    PSA_REQUIRE(slot >= 0 && slot < PSA_NUM_SLOTS, "bad data slot %d", slot);
    PSA_REQUIRE(T > 0 && N > 0, "empty trajectory (T=%lld, N=%lld)", (long long)T, (long long)N);
    PSA_TRY(check_project_args(c, a, N));
    PSA_TRY(check_weights(c, N));
    PSA_TRY(check_segments(c, T, flags));
    PSA_TRY(data_alloc_locked(c, slot, T, N));
    c->slot[slot].valid = false;
    const bool         intensity = (flags & PSA_F_INTENSITY) != 0;
    const bool         disp = (flags & PSA_F_DISPLACEMENTS) != 0;
    std::vector<float>   uniq_k;
    std::vector<int32_t> kmap;
    char*                rows = nullptr;
    float2*              d_q = nullptr;
    PSA_TRY(begin_list(c, &a, &uniq_k, &kmap, &rows, &d_q));
    K = a.K_local;                                                // (of the folded list)
    // the rocFFT plan (run-time compiled on first use of a length) is built beside the upload -- with segments set,
    // the plan of the segment stage's first block
    int64_t fft_len = T, fft_batch = 3 * K;
    if (c->seg_L) {
        int64_t nk = 0, ns = 0;
        segment_blocks(c, T, K, &nk, &ns);
        fft_len = c->seg_L;
        fft_batch = 3 * nk * ns;
    }
    int         plan_rc = PSA_OK;
    std::string plan_err;
    std::thread planner([&] {
        (void)hipSetDevice(c->device);
        FftPlan* p = nullptr;
        plan_rc = get_plan(c, fft_len, fft_batch, &p);
        if (plan_rc != PSA_OK) plan_err = g_error;
    });
    struct JoinOnExit {                                           // no path leaves with the thread running
        std::thread& t;
        ~JoinOnExit() {
            if (t.joinable()) t.join();
        }
    } join_planner{planner};
    int g0 = 0;                                                   // first non-empty group
    while (g0 < G && group_idx && group_off[g0 + 1] == group_off[g0]) ++g0;
    int rc = PSA_OK;
    // the array's largest magnitude (scale of the f16 kernels on later calls) is folded chunk by chunk
    // behind the copies too: no extra pass over the array after the upload
    PSA_TRY(c->d_upload_max.reserve(sizeof(unsigned)));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_upload_max.ptr, 0, sizeof(unsigned), c->stream));
    const size_t row_floats = (size_t)N * 3;
    auto fold_max = [&](int64_t t0, int64_t nt) {
        return launch_absmax_bits(c, c->slot[slot].buf.as<float>() + (size_t)t0 * row_floats, nt * (int64_t)row_floats,
                                  c->d_upload_max.as<unsigned>(), false);
    };
    if (g0 < G) {
        GroupView v{slot, disp};                                  // no planes, the caller's slot: the array is still arriving
        set_group(c, group_idx, group_off, g0, N, &v);
        ProjGeom g;
        rc = prepare_block(c, v, disp ? GeomRule::f32_only : GeomRule::bf16_anywhere, nullptr, 0, K, &g);
        if (rc == PSA_OK) {
            StageTimer st(c, PSA_T_H2D);
            rc = staged_upload(c, c->slot[slot].buf.as<float>(), host, T, N,
                               [&](int64_t t0, int64_t nt, hipEvent_t landed) -> int {
                                   PSA_HIP_CHECK(hipStreamWaitEvent(c->stream, landed, 0));
                                   PSA_TRY(fold_max(t0, nt));
                                   return launch_projection(c, v, g, d_q, T, t0, nt);
                               });
        }
    } else {
        StageTimer st(c, PSA_T_H2D);
        rc = staged_upload(c, c->slot[slot].buf.as<float>(), host, T, N,
                           [&](int64_t t0, int64_t nt, hipEvent_t landed) -> int {
                               PSA_HIP_CHECK(hipStreamWaitEvent(c->stream, landed, 0));
                               return fold_max(t0, nt);
                           });
    }
    planner.join();
    if (rc == PSA_OK && plan_rc != PSA_OK) {
        g_error = plan_err;
        rc = plan_rc;
    }
    PSA_TRY(rc);
    c->slot[slot].valid = true;
    PSA_HIP_CHECK(hipMemcpyAsync(&c->slot[slot].absmax_bits, c->d_upload_max.ptr, sizeof(unsigned), hipMemcpyDeviceToHost,
                                 c->stream));
    bool first = true;
    if (g0 < G) {
        PSA_TRY(spectrum_stage(c, d_q, T, K, intensity, (float*)rows, true));
        first = false;
        // remaining groups on the now resident array, by the ordinary rule
        if (g0 + 1 < G) PSA_TRY(project_groups(c, a, g0 + 1, &first, rows, d_q));
    }
    if (first) PSA_HIP_CHECK(hipMemsetAsync(rows, 0, row_bytes(c->res_T, c->res_intensity) * (size_t)K, c->stream));
    if (!c->slot[slot].absmax_known) {                           // (a later group's geometry may have asked already)
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));            // the read-back above has landed
        c->slot[slot].absmax_known = true;
    }
    return PSA_OK;
}

// Blocks of k-vectors when a complex result is produced block by block so that the D2H copy of one
// block runs while the next is projected.  r = (D2H time per k-vector) / (projection time per
// k-vector) = (24 T / 55 GB/s) / (N_g T / 4.3e13 units/s) = 1.9e4 / N_g decides the shape:
//   r < 1  (projection-bound, e.g. configuration 3): what stays exposed is the LAST block's copy ->
//          one large block (efficient projection) and a last block of one 64-vector M block;
//   r >= 1 (copy-bound, e.g. the 2500-point grid on 8192 atoms): what stays exposed is the FIRST
//          block's projection -> a first block of 128, then blocks of 512.
// Lists shorter than 192 are not split (every block is at least one M block of 64).
// K_rows: k-vectors projected; K_out >= K_rows: columns of the result (folded pairs copy twice the
// columns per projected vector, which moves r up).
static std::vector<int64_t> pipeline_blocks(int64_t K_rows, int64_t K_out, int64_t n_g) {
    std::vector<int64_t> b;
    const int64_t        K = K_rows;
    const double         r = 1.9e4 / (double)std::max<int64_t>(n_g, 1) * (double)K_out / (double)std::max<int64_t>(K_rows, 1);
    if (const char* e = std::getenv("PSA_PIPELINE_BLOCKS")) {       // experiments: "192,64"
        int64_t left = K;
        for (const char* q = e; *q && left > 0;) {
            const int64_t n = std::min<int64_t>(std::max<int64_t>(1, std::atoll(q)), left);
            b.push_back(n);
            left -= n;
            while (*q && *q != ',') ++q;
            if (*q == ',') ++q;
        }
        if (left > 0) b.push_back(left);
        return b;
    }
    if (K < 192) {
        b.push_back(K);
    } else if (r < 1.0) {
        b.push_back(K - 64);
        b.push_back(64);
    } else {
        b.push_back(128);
        for (int64_t k0 = 128; k0 < K; k0 += 512) b.push_back(std::min<int64_t>(512, K - k0));
        if (b.back() < 64 && b.size() > 2) {             // fold a sliver into its neighbour
            b[b.size() - 2] += b.back();
            b.pop_back();
        }
    }
    return b;
}

// PSA_TIMELINE=1: where a pipelined calculate spends its time -- events on both streams, printed
// (ms since entry) to stderr when the call returns.  Diagnostics only (tools/e2e_timeline.py).
struct Timeline {
    bool on = std::getenv("PSA_TIMELINE") != nullptr;
    std::chrono::steady_clock::time_point t_host0 = std::chrono::steady_clock::now();
    hipEvent_t   e0 = nullptr;
    struct Mark { const char* what; int block; hipEvent_t ev; double host_ms; };
    std::vector<Mark> marks;
    double host_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count(); }
    void start(hipStream_t s) {
        if (!on) return;
        (void)hipEventCreate(&e0);
        (void)hipEventRecord(e0, s);
    }
    void mark(const char* what, int block, hipStream_t s) {
        if (!on) return;
        hipEvent_t ev = nullptr;
        (void)hipEventCreate(&ev);
        (void)hipEventRecord(ev, s);
        marks.push_back({what, block, ev, host_ms()});
    }
    void report() {
        if (!on) return;
        const double t_end = host_ms();
        std::fprintf(stderr, "[psa timeline] %-22s %5s %10s %10s\n", "event", "block", "device_ms", "issued_ms");
        for (auto& m : marks) {
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, e0, m.ev);
            std::fprintf(stderr, "[psa timeline] %-22s %5d %10.3f %10.3f\n", m.what, m.block, ms, m.host_ms);
        }
        std::fprintf(stderr, "[psa timeline] %-22s %5s %10s %10.3f\n", "return", "", "", t_end);
    }
    ~Timeline() {                                                 // whichever way the call ends
        for (auto& m : marks)
            if (m.ev) (void)hipEventDestroy(m.ev);
        if (e0) (void)hipEventDestroy(e0);
    }
};

// Complex result of one group, all K on this device, straight to the host: per block of k-vectors
// project -> FFT -> scale/transpose (+ intensity) into its columns of (T, K, 3) -> 2-D D2H on a copy
// stream (full PCIe rate at >= 1.5-KB rows: tools/probes/d2h_2d.hip), overlapped with the next block.
// Folded lists: a block's columns are its own k-vectors' and their partners' (for a grid symmetric
// about Gamma: two runs of columns per block).
static int calculate_pipelined(psa_ctx* c, const ProjectArgs& a_in, void* out_host, float* out_intensity) {
    ProjectArgs   a = a_in;
    const int64_t K_out = a.K_total;
    PSA_TRY(check_slot(c, a.slot));
    const int64_t T = c->slot[a.slot].T, N = c->slot[a.slot].N;
    PSA_TRY(check_project_args(c, a, N));
    PSA_TRY(check_weights(c, N));
    PSA_TRY(check_segments(c, T, a.flags));                       // (a complex result: refused while segments are set)
    std::vector<float>   uniq_k;
    std::vector<int32_t> kmap;
    char*                rows = nullptr;
    float2*              d_rows = nullptr;                        // the same, as q: a block's projection goes into its rows
    PSA_TRY(begin_list(c, &a, &uniq_k, &kmap, &rows, &d_rows));
    const bool    folded = !uniq_k.empty();
    const int64_t K = a.K_total;                                   // rows of the slab
    PSA_TRY(c->d_out.reserve(result_bytes(c)));
    PSA_TRY(c->d_inten.reserve(intensity_bytes(c)));
    if (!c->d2h_stream) PSA_HIP_CHECK(hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    if (!c->d2h_ready) PSA_HIP_CHECK(hipEventCreateWithFlags(&c->d2h_ready, hipEventDisableTiming));
    GroupView v{a.slot, (a.flags & PSA_F_DISPLACEMENTS) != 0};
    set_group(c, a.group_idx, a.group_off, 0, N, &v);
    if (v.n_g == 0) {
        std::memset(out_host, 0, result_bytes(c));
        if (out_intensity) std::memset(out_intensity, 0, intensity_bytes(c));
        PSA_HIP_CHECK(hipMemsetAsync(c->d_out.ptr, 0, result_bytes(c), c->stream));
        PSA_HIP_CHECK(hipMemsetAsync(c->d_inten.ptr, 0, intensity_bytes(c), c->stream));
        PSA_HIP_CHECK(hipMemsetAsync(rows, 0, row_bytes(T, false) * (size_t)K, c->stream));
        c->out_valid = c->inten_valid = true;
        return PSA_OK;
    }
    const std::vector<int64_t> blocks = pipeline_blocks(K, K_out, v.n_g);
    // columns of every block, ascending within a block: cols / srcs, block b at [first[b], first[b+1])
    std::vector<int32_t> cols, srcs;
    std::vector<size_t>  first(blocks.size() + 1, 0);
    bool                 copy_by_block = true;
    if (folded) {
        std::vector<int> block_of((size_t)K);
        {
            int64_t r0 = 0;
            for (size_t b = 0; b < blocks.size(); r0 += blocks[b], ++b)
                for (int64_t r = r0; r < r0 + blocks[b]; ++r) block_of[(size_t)r] = (int)b;
        }
        for (int64_t k = 0; k < K_out; ++k) ++first[(size_t)block_of[(size_t)(kmap[k] & ~KMAP_MIRROR)] + 1];
        for (size_t b = 0; b < blocks.size(); ++b) first[b + 1] += first[b];
        cols.resize((size_t)K_out);
        srcs.resize((size_t)K_out);
        std::vector<size_t> at(first.begin(), first.end() - 1);
        for (int64_t k = 0; k < K_out; ++k) {
            const size_t i = at[(size_t)block_of[(size_t)(kmap[k] & ~KMAP_MIRROR)]]++;
            cols[i] = (int32_t)k;
            srcs[i] = kmap[k];
        }
        for (size_t b = 0; b < blocks.size() && copy_by_block; ++b) {   // more than a few runs of columns: one copy at the end
            int runs = 0;
            for (size_t i = first[b]; i < first[b + 1]; ++i) runs += i == first[b] || cols[i] != cols[i - 1] + 1;
            copy_by_block = runs <= 8;
        }
        PSA_TRY(c->d_cols.reserve((size_t)2 * K_out * sizeof(int32_t)));
        PSA_HIP_CHECK(hipMemcpyAsync(c->d_cols.ptr, cols.data(), (size_t)K_out * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        PSA_HIP_CHECK(hipMemcpyAsync(c->d_cols.as<int32_t>() + K_out, srcs.data(), (size_t)K_out * sizeof(int32_t),
                                     hipMemcpyHostToDevice, c->stream));
    }
    PSA_TRY(group_source(c, &v, a.mean_pos_all, K));
    Timeline tl;
    tl.start(c->stream);
    const size_t pitch = (size_t)K_out * 3 * sizeof(float2);
    auto copy_columns = [&](int64_t col0, int64_t n) -> int {
        const size_t off = (size_t)col0 * 3 * sizeof(float2), width = (size_t)n * 3 * sizeof(float2);
        PSA_HIP_CHECK(hipMemcpy2DAsync((char*)out_host + off, pitch, (const char*)c->d_out.ptr + off, pitch, width, (size_t)T,
                                       hipMemcpyDeviceToHost, c->d2h_stream));
        return PSA_OK;
    };
    int64_t k0 = 0;
    for (size_t b = 0; b < blocks.size(); ++b) {
        const int64_t nk = blocks[b];
        float2*       d_q = d_rows + (size_t)k0 * 3 * (size_t)T;
        PSA_TRY(project_block(c, v, nullptr, k0, nk, d_q));
        tl.mark("projected", (int)b, c->stream);
        {
            StageTimer st(c, PSA_T_FFT);
            PSA_TRY(run_fft(c, d_q, T, 3 * nk));
        }
        tl.mark("fft done", (int)b, c->stream);
        {
            StageTimer st(c, PSA_T_TRANSPOSE);
            if (folded)
                PSA_TRY(launch_scale_transpose_c64(c, (const float2*)rows, c->d_out.as<float2>(), c->d_inten.as<float>(), T,
                                                   (int64_t)(first[b + 1] - first[b]), K_out, 0, 0,
                                                   c->d_cols.as<int32_t>() + first[b], c->d_cols.as<int32_t>() + K_out + first[b]));
            else
                PSA_TRY(launch_scale_transpose_c64(c, (const float2*)rows, c->d_out.as<float2>(), c->d_inten.as<float>(), T, nk,
                                                   K_out, k0, k0, nullptr, nullptr));
        }
        tl.mark("transposed", (int)b, c->stream);
        if (copy_by_block) {
            PSA_HIP_CHECK(hipEventRecord(c->d2h_ready, c->stream));
            PSA_HIP_CHECK(hipStreamWaitEvent(c->d2h_stream, c->d2h_ready, 0));
            tl.mark("copy can start", (int)b, c->d2h_stream);
            if (!folded) {
                PSA_TRY(copy_columns(k0, nk));
            } else {
                for (size_t i = first[b]; i < first[b + 1];) {
                    size_t j = i + 1;
                    while (j < first[b + 1] && cols[j] == cols[j - 1] + 1) ++j;
                    PSA_TRY(copy_columns(cols[i], (int64_t)(j - i)));
                    i = j;
                }
            }
            tl.mark("copied", (int)b, c->d2h_stream);
        }
        k0 += nk;
    }
    c->out_valid = c->inten_valid = true;
    if (!copy_by_block || out_intensity) {
        PSA_HIP_CHECK(hipEventRecord(c->d2h_ready, c->stream));
        PSA_HIP_CHECK(hipStreamWaitEvent(c->d2h_stream, c->d2h_ready, 0));
        if (!copy_by_block)
            PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_out.ptr, result_bytes(c), hipMemcpyDeviceToHost, c->d2h_stream));
        if (out_intensity)
            PSA_HIP_CHECK(hipMemcpyAsync(out_intensity, c->d_inten.ptr, intensity_bytes(c), hipMemcpyDeviceToHost, c->d2h_stream));
        tl.mark("intensity copied", -1, c->d2h_stream);
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->d2h_stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    tl.report();
    return PSA_OK;
}

int psa_sed_calculate(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors,
                      int64_t K, const int32_t* group_idx, const int64_t* group_off, int32_t G,
                      int32_t flags, void* out_host, size_t out_bytes, float* out_intensity, size_t out_intensity_bytes) {
    PSA_REQUIRE(K >= 1, "need at least one k-vector");
    PSA_REQUIRE(out_intensity == nullptr || !(flags & PSA_F_INTENSITY),
                "out_intensity goes with a complex result; an intensity result IS out_host");
    if (out_host && !(flags & PSA_F_INTENSITY) && G == 1 && K >= 192 && c && c->k1_selector == PSA_K1_AUTO) {
        PSA_TRY(enter(c));
        Guard guard(c);
        PSA_TRY(check_slot(c, slot));
        const size_t bytes = row_bytes(c->slot[slot].T, false) * (size_t)K, inten = row_bytes(c->slot[slot].T, true) * (size_t)K;
        PSA_REQUIRE(k_vectors != nullptr, "null k_vectors");
        PSA_REQUIRE(out_bytes == bytes, "result is %zu bytes (T=%lld, K=%lld, complex64 x 3), the caller's buffer %zu", bytes,
                    (long long)c->slot[slot].T, (long long)K, out_bytes);
        PSA_REQUIRE(out_intensity == nullptr || out_intensity_bytes == inten,
                    "intensity is (%lld,%lld) float32 = %zu bytes, the caller's buffer %zu", (long long)c->slot[slot].T,
                    (long long)K, inten, out_intensity_bytes);
        const ProjectArgs a{slot, mean_pos_all, k_vectors, K, K, 0, group_idx, group_off, G, flags};
        return calculate_pipelined(c, a, out_host, out_intensity);
    }
    PSA_TRY(psa_sed_project(c, slot, mean_pos_all, k_vectors, K, K, 0, group_idx, group_off, G, flags));
    return psa_sed_finalize(c, out_host, out_bytes, out_intensity, out_intensity_bytes);
}

int psa_k_pairs(const float* k_vectors, int64_t K, int32_t* kmap, int32_t* unique_idx, int64_t* n_unique) {
    PSA_REQUIRE(K >= 0 && K < (1ll << 30) && (K == 0 || (k_vectors && kmap && unique_idx)) && n_unique, "bad argument");
    std::vector<int32_t> m, u;
    fold_pairs(k_vectors, K, &m, &u);
    if (K) std::memcpy(kmap, m.data(), (size_t)K * sizeof(int32_t));
    if (!u.empty()) std::memcpy(unique_idx, u.data(), u.size() * sizeof(int32_t));
    *n_unique = (int64_t)u.size();
    return PSA_OK;
}

// one (k, omega) bin of one group: K = 1 projection + one DFT dot (psa_hip.h)
int psa_sed_single_bin(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vector, const int32_t* idx,
                       int64_t n_g, int32_t flags, int64_t i_w, float* out_c64x3) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_TRY(check_slot(c, slot));
    const int64_t T = c->slot[slot].T, N = c->slot[slot].N;
    PSA_REQUIRE(mean_pos_all && k_vector && out_c64x3, "null argument");
    PSA_REQUIRE(i_w >= 0 && i_w < T, "frequency bin %lld outside [0,%lld)", (long long)i_w, (long long)T);
    PSA_TRY(check_weights(c, N));
    PSA_REQUIRE(idx == nullptr || n_g >= 0, "negative group size");
    GroupView v{slot, (flags & PSA_F_DISPLACEMENTS) != 0, idx ? n_g : N, nullptr, idx};
    PSA_TRY(check_group_indices(v, N));
    if (v.n_g == 0) {
        std::memset(out_c64x3, 0, 6 * sizeof(float));
        return PSA_OK;
    }
    PSA_TRY(upload_single_group(c, &v, N, k_vector, 1, mean_pos_all));
    c->plane_call_mark = c->plane_tick + 1;
    PSA_TRY(group_source(c, &v, mean_pos_all, 1));
    PSA_TRY(c->d_qwork.reserve((size_t)3 * T * sizeof(float2)));
    PSA_TRY(project_block(c, v, nullptr, 0, 1, c->d_qwork.as<float2>()));
    PSA_TRY(c->d_bin.reserve(3 * sizeof(float2)));
    {
        StageTimer st(c, PSA_T_FFT);
        PSA_TRY(launch_dft_bin(c, c->d_qwork.as<float2>(), T, i_w, c->d_bin.as<float2>()));
    }
    PSA_HIP_CHECK(hipMemcpyAsync(out_c64x3, c->d_bin.ptr, 3 * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // extern "C"
