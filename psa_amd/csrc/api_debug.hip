// Diagnostics: the float32 phase table, the projection without its FFT (all frames or a range, or as a list of its own
// is routed), the plane cache.
// (part of the C ABI of libpsa_hip.so, include/psa_hip.h; shared declarations: api_internal.h)
#include "api_internal.h"

using namespace psa;

extern "C" {

int psa_debug_phase_table(psa_ctx* c, const float* mean_pos_all, const float* k_vectors, int64_t K,
                          const int32_t* idx, int64_t n_g, int64_t N, void* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(mean_pos_all && k_vectors && out_host && K >= 1 && n_g >= 1 && N >= 1, "bad argument");
    PSA_REQUIRE(idx != nullptr || n_g == N, "identity group must cover all atoms");
    GroupView v{0, false, n_g, nullptr, idx};                    // (no slot: only the table is made)
    PSA_TRY(check_group_indices(v, N));
    PSA_TRY(check_weights(c, N));
    ProjGeom g;
    set_geom_weights(c, &g);
    g.n_g = (int)n_g;
    g.A_pad = (int)((n_g + 31) / 32 * 32);
    g.K = (int)K;
    g.m_blk = 32;
    g.M_pad = (int)((2 * K + 31) / 32 * 32);
    PSA_TRY(upload_single_group(c, &v, N, k_vectors, K, mean_pos_all));
    PSA_TRY(c->d_phase.reserve(p_table_floats(g.M_pad, g.A_pad) * sizeof(float)));
    PSA_TRY(launch_phase_table(c, c->d_kvec.as<float>(), c->d_mean_all.as<float>(), v.d_idx, c->d_phase.as<float>(), g));
    std::vector<float> P(p_table_floats(g.M_pad, g.A_pad));
    PSA_HIP_CHECK(hipMemcpyAsync(P.data(), c->d_phase.ptr, P.size() * sizeof(float),
                                 hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    float* o = (float*)out_host;
    for (int64_t k = 0; k < K; ++k)
        for (int64_t a = 0; a < n_g; ++a) {
            o[2 * (k * n_g + a) + 0] = P[p_tile_index((int)(2 * k), (int)a, g.m_blk, g.A_pad / K1_BA)];
            o[2 * (k * n_g + a) + 1] = P[p_tile_index((int)(2 * k + 1), (int)a, g.m_blk, g.A_pad / K1_BA)];
        }
    return PSA_OK;
}

// route: the launch goes through project_block with the K vectors offered as a whole list, as project_groups hands
// psa_sed_project's list to it -- so the low-rank route for k-paths serves where its plan, the options and the group's
// planes let it, and psa_k1_lowrank_launches counts it -- over all frames of the slot.  What psa_sed_project does to a list
// before that is not done here: the list is neither folded (begin_list: pairs (k, -k), twins) nor cut into k-blocks
// (PSA_PHASE_TABLE_MIB).
static int debug_project(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                         const int32_t* idx, int64_t n_g, int32_t flags, int64_t t_begin, int64_t t_count, void* out_host,
                         bool route = false) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_TRY(check_slot(c, slot));
    const int64_t T = c->slot[slot].T, N = c->slot[slot].N;
    PSA_REQUIRE(mean_pos_all && k_vectors && out_host && K >= 1 && n_g >= 1, "bad argument");
    if (t_count < 0) t_begin = 0, t_count = T;
    PSA_REQUIRE(idx != nullptr || n_g == N, "identity group must cover all atoms");
    GroupView v{slot, (flags & PSA_F_DISPLACEMENTS) != 0, n_g, nullptr, idx};
    PSA_TRY(check_group_indices(v, N));
    PSA_TRY(check_weights(c, N));
    PSA_TRY(upload_single_group(c, &v, N, k_vectors, K, mean_pos_all));
    c->plane_call_mark = c->plane_tick + 1;
    PSA_TRY(group_source(c, &v, mean_pos_all, K));
    const size_t bytes = (size_t)K * 3 * T * sizeof(float2);
    PSA_TRY(c->d_qwork.reserve(bytes));
    if (route) {
        const ProjectArgs list{slot, mean_pos_all, k_vectors, K, K, 0, nullptr, nullptr, 1, flags};
        PSA_TRY(project_block(c, v, &list, 0, K, c->d_qwork.as<float2>()));
    } else {
        // project_block's pieces (no low-rank route), with the zero-fill where it has always been issued and the launch
        // over the caller's frame range
        ProjGeom g;
        PSA_TRY(make_geom(c, v, K, GeomRule::product, &g));
        if (t_count != T) PSA_HIP_CHECK(hipMemsetAsync(c->d_qwork.ptr, 0, bytes, c->stream));
        PSA_TRY(prepare_phase(c, v, g, 0));
        if (t_count > 0) PSA_TRY(launch_projection(c, v, g, c->d_qwork.as<float2>(), T, t_begin, t_count));
    }
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_qwork.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int psa_debug_project_only(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors,
                           int64_t K, const int32_t* idx, int64_t n_g, int32_t flags, void* out_host) {
    return debug_project(c, slot, mean_pos_all, k_vectors, K, idx, n_g, flags, 0, -1, out_host);
}

// The projection routed as a list of its own: see debug_project
int psa_debug_project_route(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                            const int32_t* idx, int64_t n_g, int32_t flags, void* out_host) {
    return debug_project(c, slot, mean_pos_all, k_vectors, K, idx, n_g, flags, 0, -1, out_host, true);
}

int psa_debug_project_frames(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                             const int32_t* idx, int64_t n_g, int32_t flags, int64_t t_begin, int64_t t_count,
                             void* out_host) {
    PSA_REQUIRE(t_begin >= 0 && t_count >= 0, "negative frame range");
    return debug_project(c, slot, mean_pos_all, k_vectors, K, idx, n_g, flags, t_begin, t_count, out_host);
}

int psa_debug_plane_cache(psa_ctx* c, int64_t* n_sets, int64_t* bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    drop_stale_planes(c);
    if (n_sets) *n_sets = (int64_t)c->planes.size();
    if (bytes) *bytes = (int64_t)planes_bytes_held(c);
    return PSA_OK;
}

}  // extern "C"
