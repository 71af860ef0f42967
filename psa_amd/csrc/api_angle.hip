// psa_angle_histogram, psa_debug_neighbour_lists: the bond-angle distributions of species triplets and the coordination
// statistics of species pairs of the neighbour shells over time origins (definition: include/psa_hip.h; kernels: angle.hip
// -- the parts it shares with the other shell passes in shell.h -- and pair.hip's fraction pass; host core: api_shell.h).
// Nothing lies behind the counts: 1040 n_a bytes per origin of a block.  Per block: the fraction pass, the neighbour pass,
// the angle pass over the items, the reduce into the accumulator that lives across blocks.
#include "api_shell.h"

namespace psa {

namespace {

int angle_run(ShellCall& s, int32_t n_theta, uint64_t* angles, size_t angles_bytes, uint64_t* coord, size_t coord_bytes, uint64_t* truncated) {
    PSA_REQUIRE(angles != nullptr && coord != nullptr && truncated != nullptr, "null output");
    PSA_TRY(shell_check(&s, "psa_angle_histogram"));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
    PSA_REQUIRE(n_theta >= 1 && n_theta <= ANGLE_MAX_BINS, "the number of bins is in [1, %d], got %d", ANGLE_MAX_BINS, (int)n_theta);
    const int    S = p.G, P = S * (S + 1) / 2, n1 = n_theta + 1, NC = ANGLE_MAX_NEIGHBOURS + 1;
    const size_t want_a = (size_t)S * (size_t)P * (size_t)n1 * sizeof(uint64_t), want_c = (size_t)S * (size_t)S * (size_t)NC * sizeof(uint64_t);
    PSA_REQUIRE(angles_bytes == want_a, "angles_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", angles_bytes, S, P, n1, want_a);
    PSA_REQUIRE(coord_bytes == want_c, "coord_bytes is %zu, the (%d,%d,%d) uint64 result has %zu", coord_bytes, S, S, NC, want_c);
    std::memset(angles, 0, want_a);
    std::memset(coord, 0, want_c);
    std::memset(truncated, 0, (size_t)S * sizeof(uint64_t));
    if (p.n_a == 0) return PSA_OK;                           // every species empty: zeros
    const int64_t      row = angle_row_words(S, n_theta);
    std::vector<float> edges((size_t)n1);
    for (int i = 0; i < n1; ++i) edges[(size_t)i] = (float)std::cos((double)i * M_PI / (double)n_theta);
    edges[0] = 1.f, edges[(size_t)n_theta] = -1.f;
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_angle_edges, edges.data(), edges.size() * sizeof(float)));
    }
    std::vector<uint64_t> acc;
    PSA_TRY(shell_run(s, row, {}, [&](const AngleWork& w, int64_t n_items, int64_t, int64_t nb) -> int {
        return launch_angle_hist(c, w.count, w.list, c->d_rs_items.ptr, n_items, c->d_angle_edges.as<float>(), c->d_rs_part.as<unsigned>(), S,
                                 p.n_a, nb, n_theta);
    }, nullptr, &acc));
    for (int a = 0; a < S; ++a) {
        const uint64_t* r = acc.data() + (size_t)a * (size_t)row;
        std::memcpy(angles + (size_t)a * (size_t)P * (size_t)n1, r, (size_t)P * (size_t)n1 * sizeof(uint64_t));
        std::memcpy(coord + (size_t)a * (size_t)S * (size_t)NC, r + (size_t)P * (size_t)n1, (size_t)S * (size_t)NC * sizeof(uint64_t));
        truncated[a] = r[(size_t)row - 1];
    }
    return PSA_OK;
}

// the fraction pass and the neighbour pass of one frame: the true counts and the first 64 list positions of every centre
int debug_lists_run(ShellCall& s, int64_t frame, int32_t* count, int32_t* list) {
    PSA_REQUIRE(count != nullptr && list != nullptr, "null output");
    AngleWork w;
    PSA_TRY(shell_check(&s, "psa_debug_neighbour_lists"));
    PSA_TRY(shell_one_frame(s, frame, {}, &w));
    psa_ctx*          c = s.c;
    const AtomGroups& p = s.p;
    if (p.n_a == 0) return PSA_OK;
    std::vector<float> h((size_t)p.n_a * ANGLE_MAX_NEIGHBOURS * 4);
    PSA_HIP_CHECK(hipMemcpyAsync(count, w.count, (size_t)p.n_a * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(h.data(), w.list, h.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int64_t a = 0; a < p.n_a; ++a)
        for (int k = 0; k < ANGLE_MAX_NEIGHBOURS; ++k) {
            int32_t tag;
            std::memcpy(&tag, &h[((size_t)a * ANGLE_MAX_NEIGHBOURS + (size_t)k) * 4 + 3], sizeof tag);
            list[(size_t)a * ANGLE_MAX_NEIGHBOURS + (size_t)k] = k < count[a] ? (tag & ((1 << ANGLE_SPECIES_SHIFT) - 1)) : -1;
        }
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_angle_histogram(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                        int32_t n_groups, const double* r_cut, int64_t origin_step, int32_t n_theta, uint64_t* angles, size_t angles_bytes,
                        uint64_t* coord, size_t coord_bytes, uint64_t* truncated) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    ShellCall s{c, box, box_inverse, idx, group_start, n_groups, r_cut, origin_step};
    return synchronised(c, angle_run(s, n_theta, angles, angles_bytes, coord, coord_bytes, truncated), "psa_angle_histogram");
}

int psa_debug_neighbour_lists(psa_ctx* c, const double* box, const double* box_inverse, const int32_t* idx, const int64_t* group_start,
                              int32_t n_groups, const double* r_cut, int64_t frame, int32_t* count, int32_t* list) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    ShellCall s{c, box, box_inverse, idx, group_start, n_groups, r_cut, 1};
    return synchronised(c, debug_lists_run(s, frame, count, list), "psa_debug_neighbour_lists");
}

}  // extern "C"
