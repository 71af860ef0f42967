// psa_vdos: the vibrational density of states of atom groups (definition: include/psa_hip.h; kernels: vdos.hip).
// A second, non-projecting pass over the resident array: blocks of (atom pairs x segments) are gathered into a work
// buffer of bounded size, transformed by the batched complex rocFFT plans of api_core.hip -- two atoms of one group per
// complex series -- and their power is summed per group in float64.  Nothing of the SED path's state is touched.
#include "api_internal.h"

namespace psa {

namespace {

struct VdosPlan {
    std::vector<int32_t> pairs;      // 2 atom indices per pair (-1: no second atom), groups one after the other
    std::vector<int64_t> pair_off;   // (n_groups + 1) pair offsets of the non-empty groups
    std::vector<int32_t> group_of;   // caller's group number of each of them
};

// Groups -> pairs.  Each group's atoms in ascending order (reads of neighbouring atoms coalesce), two per pair; groups
// must be disjoint, since one pass serves them all.
int plan_pairs(int64_t N, const int32_t* group_idx, const int64_t* group_off, int32_t G, VdosPlan* p) {
    p->pair_off.assign(1, 0);
    if (!group_idx) {
        p->pairs.resize((size_t)((N + 1) / 2) * 2);
        for (int64_t a = 0; a < (int64_t)p->pairs.size(); ++a) p->pairs[a] = a < N ? (int32_t)a : -1;
        p->pair_off.push_back((N + 1) / 2);
        p->group_of.assign(1, 0);
        return PSA_OK;
    }
    std::vector<uint8_t> seen((size_t)N, 0);
    std::vector<int32_t> atoms;
    for (int32_t g = 0; g < G; ++g) {
        atoms.assign(group_idx + group_off[g], group_idx + group_off[g + 1]);
        if (atoms.empty()) continue;
        std::sort(atoms.begin(), atoms.end());
        for (int32_t a : atoms) {
            PSA_REQUIRE(!seen[a], "atom %d is listed twice (group %d): the groups of a density of states must be disjoint",
                        (int)a, (int)g);
            seen[a] = 1;
        }
        if (atoms.size() & 1) atoms.push_back(-1);
        p->pairs.insert(p->pairs.end(), atoms.begin(), atoms.end());
        p->pair_off.push_back((int64_t)p->pairs.size() / 2);
        p->group_of.push_back(g);
    }
    return PSA_OK;
}

int vdos_run(psa_ctx* c, int slot, const float* mean_pos_all, const int32_t* group_idx, const int64_t* group_off, int32_t G,
             int32_t flags, float* out_host, size_t out_bytes) {
    PSA_TRY(check_slot(c, slot));
    const int64_t T = c->slot[slot].T, N = c->slot[slot].N;
    const bool    disp = (flags & PSA_F_DISPLACEMENTS) != 0;
    PSA_REQUIRE((flags & ~PSA_F_DISPLACEMENTS) == 0, "psa_vdos takes PSA_F_DISPLACEMENTS or 0, got flags 0x%x", (unsigned)flags);
    PSA_REQUIRE(out_host != nullptr, "null output");
    PSA_REQUIRE(!disp || mean_pos_all != nullptr, "PSA_F_DISPLACEMENTS needs mean_pos_all");
    PSA_TRY(validate_groups(N, group_idx, group_off, G));
    PSA_TRY(check_weights(c, N));
    const int64_t L = c->seg_L ? c->seg_L : T, H = c->seg_L ? c->seg_hop : T, F = L / 2 + 1;
    PSA_REQUIRE(L <= T, "segment length %lld exceeds the trajectory's %lld frames", (long long)L, (long long)T);
    PSA_REQUIRE(out_bytes == (size_t)G * 3 * (size_t)F * sizeof(float), "out_bytes is %zu, the (%d,3,%lld) float32 result has %zu",
                out_bytes, (int)G, (long long)F, (size_t)G * 3 * (size_t)F * sizeof(float));
    VdosPlan plan;
    PSA_TRY(plan_pairs(N, group_idx, group_off, G, &plan));
    const int64_t P = (int64_t)plan.pairs.size() / 2, n_groups = (int64_t)plan.group_of.size();
    std::memset(out_host, 0, out_bytes);
    if (P == 0) return PSA_OK;                         // every group empty

    // blocks: whole gather tiles of pairs x segments, the work buffer within the budget
    const int64_t n_seg = 1 + (T - L) / H, n_tiles = (P + VDOS_TILE_PAIRS - 1) / VDOS_TILE_PAIRS;
    const int64_t unit_bytes = (int64_t)VDOS_TILE_PAIRS * 3 * L * (int64_t)sizeof(float2);
    const int64_t units = c->opt_vdos_work_bytes / unit_bytes;
    PSA_REQUIRE(units >= 1, "the work budget of %lld bytes (PSA_OPT_VDOS_WORK_BYTES) cannot hold the smallest block: %d atom "
                "pairs x 3 components x one segment of %lld frames need %lld bytes", (long long)c->opt_vdos_work_bytes,
                VDOS_TILE_PAIRS, (long long)L, (long long)unit_bytes);
    int64_t ns = n_seg, tiles = 1;
    if (units >= n_seg) tiles = std::min<int64_t>({n_tiles, units / n_seg, 65535});
    else ns = units;
    const int64_t Pb = std::min(P, tiles * VDOS_TILE_PAIRS);

    PSA_TRY(upload(c, c->d_vdos_pairs, plan.pairs.data(), plan.pairs.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_vdos_off, plan.pair_off.data(), plan.pair_off.size() * sizeof(int64_t)));
    if (disp) PSA_TRY(upload(c, c->d_vdos_mean, mean_pos_all, (size_t)N * 3 * sizeof(float)));
    PSA_TRY(c->d_vdos_work.reserve((size_t)Pb * 3 * (size_t)ns * (size_t)L * sizeof(float2)));
    PSA_TRY(c->d_vdos_acc.reserve((size_t)n_groups * 3 * (size_t)L * sizeof(double)));
    PSA_TRY(c->d_vdos_out.reserve((size_t)n_groups * 3 * (size_t)F * sizeof(float)));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_vdos_acc.ptr, 0, (size_t)n_groups * 3 * (size_t)L * sizeof(double), c->stream));

    const float*   d_data = c->slot[slot].buf.as<float>();
    const float*   d_mean = disp ? c->d_vdos_mean.as<float>() : nullptr;
    const float*   d_wgt = c->weights_N ? c->d_weights.as<float>() : nullptr;
    const float*   d_win = c->seg_L ? c->d_seg_window.as<float>() : nullptr;
    float2*        d_work = c->d_vdos_work.as<float2>();
    const int64_t* off = plan.pair_off.data();
    const int64_t  n_ot = std::min<int64_t>((L + 255) / 256, 1 << 12);
    for (int64_t p0 = 0; p0 < P; p0 += Pb) {
        const int64_t nb = std::min(Pb, P - p0);
        // the groups with pairs in [p0, p0 + nb)
        const int64_t g_first = (std::upper_bound(off, off + n_groups + 1, p0) - off) - 1;
        const int64_t g_end = std::lower_bound(off, off + n_groups + 1, p0 + nb) - off;
        const int64_t ng = g_end - g_first;
        // enough workgroups for the power pass whatever L and the number of groups: the rows of a (group, component)
        // are split into chunks whose float64 partial sums are added in order
        for (int64_t s0 = 0; s0 < n_seg; s0 += ns) {
            const int64_t bs = std::min(ns, n_seg - s0);
            const int64_t n_chunks = std::max<int64_t>(1, std::min<int64_t>({64, (2048 + n_ot * 3 * ng - 1) / (n_ot * 3 * ng), nb * bs}));
            PSA_TRY(c->d_vdos_part.reserve((size_t)n_chunks * (size_t)ng * 3 * (size_t)L * sizeof(double)));
            {
                StageTimer st(c, PSA_T_TRANSPOSE);
                PSA_TRY(launch_vdos_gather(c, d_data, d_mean, d_wgt, d_win, c->d_vdos_pairs.as<int>() + 2 * p0, d_work, T, N, L, H,
                                           s0, bs, nb));
            }
            {
                StageTimer st(c, PSA_T_FFT);
                PSA_TRY(run_fft(c, d_work, L, 3 * nb * bs));
            }
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_vdos_power(c, d_work, c->d_vdos_off.as<int64_t>(), c->d_vdos_part.as<double>(),
                                      c->d_vdos_acc.as<double>(), L, bs, nb, p0, g_first, ng, n_chunks));
        }
    }
    const double U = c->seg_L ? c->seg_U : 1.0;
    const double scale = 0.5 / ((double)L * (double)L * (double)n_seg * U);
    {
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_vdos_finish(c, c->d_vdos_acc.as<double>(), c->d_vdos_out.as<float>(), L, n_groups * 3, scale));
    }
    StageTimer         st(c, PSA_T_D2H);
    const size_t       row_bytes = 3 * (size_t)F * sizeof(float);
    std::vector<float> host;
    float*             dst = out_host;
    if (n_groups != G) {                               // empty groups stay zero
        host.resize((size_t)n_groups * 3 * (size_t)F);
        dst = host.data();
    }
    PSA_HIP_CHECK(hipMemcpyAsync(dst, c->d_vdos_out.ptr, (size_t)n_groups * row_bytes, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n_groups != G)
        for (int64_t g = 0; g < n_groups; ++g)
            std::memcpy((char*)out_host + (size_t)plan.group_of[g] * row_bytes, (char*)host.data() + (size_t)g * row_bytes, row_bytes);
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_vdos(psa_ctx* c, int slot, const float* mean_pos_all, const int32_t* group_idx, const int64_t* group_off, int32_t G,
             int32_t flags, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard     guard(c);
    const int rc = vdos_run(c, slot, mean_pos_all, group_idx, group_off, G, flags, out_host, out_bytes);
    // the caller's arrays are only read during the call, whichever way it ends
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PSA_OK) {
        set_error("hipStreamSynchronize failed after psa_vdos");
        return PSA_EHIP;
    }
    return rc;
}

}  // extern "C"
