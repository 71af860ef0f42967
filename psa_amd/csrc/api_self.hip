// psa_self_spectra: the self (incoherent) dynamic structure factor on the reciprocal lattice of the simulation box, per
// vector or averaged over shells of |k| (definition: include/psa_hip.h; kernels: self.hip).  The checks are those of
// psa_lattice_spectra (slots, atom set, weights, box, indices, half-space membership in the shell form, segments) and the
// pipeline is the staged form of psa_vdos: per block the series kernel, one batched rocFFT, the power pass into a float64
// accumulator (L, K or n_bins) that lives across blocks, and at the end lattice.hip's finish pass.
//
// The plan.  The vectors are processed sorted by (n_1, n_2, n_3) -- in the shell form by (bin, n_1, n_2, n_3), so that a
// shell's vectors are one contiguous range -- and cut greedily into tiles of at most SELF_KS vectors that use at most
// SELF_ENTRIES distinct (axis, index) pairs: a tile's table must fit the series kernel's LDS.  Per tile its entries, per
// vector the three entries it reads (lattice_tile_entries, shared with api_lattice.hip).  A column of the result is a
// "group" of consecutive vectors of that order: one vector and its place in the caller's list, or a shell.
//
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W; the accumulator, the partial sums and the result are outside).
// A block is a whole number of atom tiles x vector tiles x segments and is counted in units of SELF_ATOMS atoms x the
// largest tile's vectors x one segment, 8 L bytes per series: segments shrink first, then vector tiles, then atom tiles,
// and a budget below one unit is refused.  Shared with the other reciprocal-space entries (api_reciprocal.hip): the checks of
// the slots and the atom set, the segments (segment_shape), the bins and the buffer set d_rc_*.
#include "api_internal.h"

namespace psa {

int self_check(psa_ctx* c, const char* entry, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of,
               int64_t n_bins, const int32_t* idx, int64_t n_g, bool segments, int64_t n_lags, SelfCall* p) {
    PSA_REQUIRE(box_inverse != nullptr, "null box_inverse");
    PSA_REQUIRE(indices != nullptr, "null indices");
    DynCall& d = p->d;
    PSA_TRY(dynamic_inputs(c, entry, K, idx, n_g, 0, &d));
    PSA_TRY(lattice_inputs(box_inverse, indices, K, bin_of, n_bins));
    PSA_REQUIRE(K < (1ll << 30), "too many vectors (%lld)", (long long)K);
    p->shell = bin_of != nullptr;
    p->cols = p->shell ? n_bins : K;
    d.n_lags = n_lags;
    PSA_TRY(segment_shape(c, segments, &d));
    lattice_box_parts(box_inverse, p->box_hi, p->box_lo);
    lattice_order(indices, K, bin_of, K, &p->order);

    // tiles: as many consecutive vectors as SELF_KS and the table allow
    p->slot.assign((size_t)K, 0);
    p->tile = {0, 0};
    for (int64_t k0 = 0; k0 < K;) {
        bool    used[3][2 * LAT_MAX_INDEX + 1] = {};
        int     R = 0;
        int64_t nt = 0;
        for (; k0 + nt < K && nt < SELF_KS; ++nt) {
            const int32_t* n = indices + 3 * p->order[(size_t)(k0 + nt)];
            int            more = 0;
            for (int j = 0; j < 3; ++j) more += !used[j][n[j] + LAT_MAX_INDEX];
            if (R + more > SELF_ENTRIES) break;                            // (a tile's first vector always fits: 3 entries)
            for (int j = 0; j < 3; ++j) used[j][n[j] + LAT_MAX_INDEX] = true;
            R += more;
        }
        lattice_tile_entries(indices, p->order.data() + k0, nt, &p->ent, p->slot.data() + k0);
        k0 += nt;
        p->tile.push_back((int32_t)p->ent.size());
        p->tile.push_back((int32_t)k0);
        p->kt_max = std::max(p->kt_max, nt);
    }
    p->n_tiles = (int64_t)p->tile.size() / 2 - 1;

    // columns
    const double U = d.cut ? c->seg_U : 1.0, norm = (double)d.n_seg * U * (double)d.L * (double)d.L;
    if (p->shell) {
        std::vector<int32_t> bin_start;
        bin_counts(bin_of, K, n_bins, &p->count);
        lattice_bins(p->count, norm, 1.0, 1.0, &bin_start, &p->scale);   // 1 / (2 n_half norm)
        for (int64_t b = 0; b < n_bins; ++b) {
            p->groups.push_back(bin_start[(size_t)b]);
            p->groups.push_back((int32_t)b);
        }
    } else {
        p->scale.assign((size_t)K, 1.0 / norm);
        for (int64_t v = 0; v < K; ++v) {
            p->groups.push_back((int32_t)v);
            p->groups.push_back((int32_t)p->order[(size_t)v]);
        }
    }
    p->n_groups = (int64_t)p->groups.size() / 2;
    p->groups.push_back((int32_t)K);
    p->groups.push_back(0);

    // the block rule
    const int64_t W = c->opt_dynamic_work_bytes;
    const int64_t unit = (int64_t)SELF_ATOMS * p->kt_max * d.P * (int64_t)sizeof(float2);
    const int64_t units = W / unit;
    PSA_REQUIRE(units >= 1, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold the smallest block: %d atoms x "
                "%lld vectors x one segment of %lld frames need %lld bytes", (long long)W, SELF_ATOMS, (long long)p->kt_max,
                (long long)d.P, (long long)unit);
    const int64_t n_at = (d.n_g + SELF_ATOMS - 1) / SELF_ATOMS;
    p->at = std::max<int64_t>(1, std::min<int64_t>({n_at, units, 65535}));
    p->vt = std::min<int64_t>({p->n_tiles, units / p->at, 65535});
    p->bs = std::min<int64_t>(d.n_seg, units / (p->at * p->vt));
    // (the batch of the FFT and the rows of the passes in 31 bits)
    const int64_t series = p->at * SELF_ATOMS * std::min(K, p->vt * p->kt_max);
    PSA_REQUIRE(series < (1ll << 31), "a block of %lld series is too large: lower PSA_OPT_DYNAMIC_WORK_BYTES", (long long)series);
    p->bs = std::min<int64_t>(p->bs, ((1ll << 31) - 1) / series);
    return PSA_OK;
}

int self_upload(psa_ctx* c, const SelfCall& p, const int32_t* idx, bool columns) {
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_rc_tiles, p.tile.data(), p.tile.size() * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_rc_ent, p.ent.data(), p.ent.size() * sizeof(uint16_t)));
    PSA_TRY(upload(c, c->d_rc_slot, p.slot.data(), p.slot.size() * sizeof(uint32_t)));
    if (idx) PSA_TRY(upload(c, c->d_rc_idx, idx, (size_t)p.d.n_g * sizeof(int32_t)));
    if (columns) {
        PSA_TRY(upload(c, c->d_rc_groups, p.groups.data(), p.groups.size() * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_rc_scale, p.scale.data(), p.scale.size() * sizeof(double)));
    }
    return PSA_OK;
}

int self_series(psa_ctx* c, const SelfCall& p, const int32_t* idx, int64_t a0, int64_t na, int64_t t0, int64_t nt, int64_t s0, int64_t ns,
                float2* d_work) {
    StageTimer    st(c, PSA_T_TRANSPOSE);
    const int64_t v0 = p.tile[(size_t)(2 * t0 + 1)], nv = p.tile[(size_t)(2 * (t0 + nt) + 1)] - v0;
    return launch_self_series(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(), c->weights_N ? c->d_weights.as<float>() : nullptr,
                              idx ? c->d_rc_idx.as<int>() : nullptr, a0, p.box_hi, p.box_lo, c->d_rc_tiles.as<int>(),
                              c->d_rc_ent.as<unsigned short>(), c->d_rc_slot.as<unsigned>(),
                              p.d.cut ? c->d_seg_window.as<float>() : nullptr, d_work, p.d.T, p.d.N, na, t0, nt, v0, nv, p.d.L, p.d.H, s0,
                              ns, p.d.P);
}

int self_power_run(psa_ctx* c, const SelfPower& w, const SelfFill& fill) {
    const int64_t L = w.L, cols = w.cols;
    const size_t  want = (size_t)L * (size_t)cols * sizeof(float);
    PSA_TRY(c->d_rc_acc.reserve(want * 2));
    PSA_TRY(c->d_rc_out.reserve(want));
    double* d_acc = c->d_rc_acc.as<double>();
    PSA_HIP_CHECK(hipMemsetAsync(d_acc, 0, want * 2, c->stream));

    const int*     d_groups = c->d_rc_groups.as<int>();
    const int64_t  n_ot = std::min<int64_t>((L + 255) / 256, 1 << 12);
    std::vector<int32_t> starts((size_t)w.n_groups + 1);
    for (int64_t g = 0; g <= w.n_groups; ++g) starts[(size_t)g] = w.groups[(size_t)(2 * g)];
    for (int64_t a0 = 0; a0 < w.n_atoms; a0 += w.Ab) {
        const int64_t na = std::min(w.Ab, w.n_atoms - a0);
        for (size_t vb = 0; vb + 1 < w.vcut->size(); ++vb) {
            const int64_t v0 = (*w.vcut)[vb], nv = (*w.vcut)[vb + 1] - v0;
            // the columns with vectors in [v0, v0 + nv)
            const int64_t g_first = (std::upper_bound(starts.begin(), starts.end(), (int32_t)v0) - starts.begin()) - 1;
            const int64_t g_end = std::min<int64_t>(w.n_groups, std::lower_bound(starts.begin(), starts.end(), (int32_t)(v0 + nv)) - starts.begin());
            const int64_t ng = g_end - g_first;
            // enough workgroups for the power pass whatever L and the number of columns: the block's atoms are split into
            // chunks whose float64 partial sums are added in order
            const int64_t n_chunks = w.n_chunks ? w.n_chunks
                                                : std::max<int64_t>(1, std::min<int64_t>({64, (2048 + n_ot * ng - 1) / (n_ot * ng), na}));
            PSA_TRY(c->d_rc_part.reserve((size_t)n_chunks * (size_t)ng * (size_t)L * sizeof(double)));
            for (int64_t s0 = 0; s0 < w.n_seg; s0 += w.bs) {
                const int64_t ns = std::min(w.bs, w.n_seg - s0);
                const float2* d_work = nullptr;
                PSA_TRY(fill(a0, na, (int64_t)vb, s0, ns, &d_work));
                StageTimer st(c, PSA_T_EPILOGUE);
                PSA_TRY(launch_self_power(c, d_work, d_groups, c->d_rc_part.as<double>(), d_acc, L, ns, na, v0, nv, g_first, ng, cols,
                                          n_chunks, w.mirror));
            }
        }
    }
    if (!w.finish) return PSA_OK;
    StageTimer st(c, PSA_T_EPILOGUE);
    return launch_lattice_finish(c, d_acc, c->d_rc_scale.as<double>(), c->d_rc_out.as<float>(), L * cols, cols);
}

int self_blocks(psa_ctx* c, const SelfCall& p, std::vector<int64_t>* vcut, SelfPower* w) {
    const int64_t K = p.d.K, Ab = p.at * SELF_ATOMS, nv_max = std::min(K, p.vt * p.kt_max);
    PSA_TRY(c->d_rc_work.reserve((size_t)std::min(Ab, p.d.n_g) * (size_t)nv_max * (size_t)p.bs * (size_t)p.d.P * sizeof(float2)));
    vcut->clear();                                           // a vector block is a run of vt tiles
    for (int64_t t0 = 0; t0 < p.n_tiles; t0 += p.vt) vcut->push_back(p.tile[(size_t)(2 * t0 + 1)]);
    vcut->push_back(K);
    w->L = p.d.P, w->n_seg = p.d.n_seg, w->n_atoms = p.d.n_g, w->cols = p.cols, w->n_groups = p.n_groups, w->groups = p.groups.data();
    w->Ab = Ab, w->bs = p.bs, w->vcut = vcut;
    return PSA_OK;
}

namespace {

int self_run(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
             const int32_t* idx, int64_t n_g, float* out_host, size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    SelfCall p;
    PSA_TRY(self_check(c, "psa_self_spectra", box_inverse, indices, K, bin_of, n_bins, idx, n_g, true, 0, &p));
    const int64_t L = p.d.L, cols = p.cols;
    const size_t  want = (size_t)L * (size_t)cols * sizeof(float);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%lld) float32 result has %zu", out_bytes, (long long)L, (long long)cols,
                want);
    if (p.d.n_g == 0) {                                      // an empty atom set: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(self_upload(c, p, idx, true));
    std::vector<int64_t> vcut;
    SelfPower            w;
    PSA_TRY(self_blocks(c, p, &vcut, &w));
    w.mirror = p.shell;
    float2* d_work = c->d_rc_work.as<float2>();
    PSA_TRY(self_power_run(c, w, [&](int64_t a0, int64_t na, int64_t vb, int64_t s0, int64_t ns, const float2** where) -> int {
        const int64_t t0 = vb * p.vt, nt = std::min(p.vt, p.n_tiles - t0);
        PSA_TRY(self_series(c, p, idx, a0, na, t0, nt, s0, ns, d_work));
        StageTimer st(c, PSA_T_FFT);
        PSA_TRY(run_fft(c, d_work, L, na * (vcut[(size_t)vb + 1] - vcut[(size_t)vb]) * ns));
        *where = d_work;
        return PSA_OK;
    }));
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_rc_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the series kernel alone, block by block under the same rule, one boxcar segment of all T frames and no window:
// z (n_g, K, T) before any FFT, atoms in the order of the set, vectors in the caller's order
int self_debug_series(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx, int64_t n_g,
                      void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    SelfCall p;
    PSA_TRY(self_check(c, "psa_debug_self_series", box_inverse, indices, K, nullptr, 0, idx, n_g, false, 0, &p));
    if (p.d.n_g == 0) return PSA_OK;
    PSA_TRY(self_upload(c, p, idx, false));
    const int64_t T = p.d.T, Ab = p.at * SELF_ATOMS, nv_max = std::min(K, p.vt * p.kt_max);
    const size_t  row = (size_t)T * sizeof(float2);
    PSA_TRY(c->d_rc_work.reserve((size_t)std::min(Ab, p.d.n_g) * (size_t)nv_max * row));
    std::vector<char> host;
    for (int64_t a0 = 0; a0 < p.d.n_g; a0 += Ab) {
        const int64_t na = std::min(Ab, p.d.n_g - a0);
        for (int64_t t0 = 0; t0 < p.n_tiles; t0 += p.vt) {
            const int64_t nt = std::min(p.vt, p.n_tiles - t0);
            const int64_t v0 = p.tile[(size_t)(2 * t0 + 1)], nv = p.tile[(size_t)(2 * (t0 + nt) + 1)] - v0;
            PSA_TRY(self_series(c, p, idx, a0, na, t0, nt, 0, 1, c->d_rc_work.as<float2>()));
            host.resize((size_t)na * (size_t)nv * row);
            PSA_HIP_CHECK(hipMemcpyAsync(host.data(), c->d_rc_work.ptr, host.size(), hipMemcpyDeviceToHost, c->stream));
            PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
            for (int64_t a = 0; a < na; ++a)
                for (int64_t k = 0; k < nv; ++k)
                    std::memcpy((char*)out_host + ((size_t)(a0 + a) * (size_t)K + (size_t)p.order[(size_t)(v0 + k)]) * row,
                                host.data() + ((size_t)a * (size_t)nv + (size_t)k) * row, row);
        }
    }
    return PSA_OK;
}

// the power, reduce and finish passes alone on transformed series work (na, nv, n_seg, L) of the caller's, the vectors in
// the processing order: what self_run does after its FFT, with the caller's groups table and scales, cut into blocks of
// atom_block atoms x vec_block vectors x seg_block segments (0: all)
int self_debug_power(psa_ctx* c, const void* work_host, int64_t na, int64_t nv, int64_t n_seg, int64_t L, const int32_t* groups,
                     int64_t n_groups, int64_t cols, const double* scale, int32_t mirror, int64_t n_chunks, int64_t atom_block,
                     int64_t vec_block, int64_t seg_block, float* out_host) {
    PSA_REQUIRE(work_host != nullptr && groups != nullptr && scale != nullptr && out_host != nullptr, "null argument");
    PSA_REQUIRE(na >= 1 && na < (1ll << 31) && nv >= 1 && nv < (1ll << 30) && n_seg >= 1 && L >= 1 && n_groups >= 1 && cols >= 1,
                "na, nv, n_seg, L, n_groups and cols are positive (%lld, %lld, %lld, %lld, %lld, %lld)", (long long)na, (long long)nv,
                (long long)n_seg, (long long)L, (long long)n_groups, (long long)cols);
    PSA_REQUIRE(mirror == 0 || mirror == 1, "mirror is 0 or 1, got %d", (int)mirror);
    PSA_REQUIRE(n_chunks >= 0 && n_chunks <= 65535 && atom_block >= 0 && vec_block >= 0 && seg_block >= 0,
                "n_chunks in [0, 65535], the blocks not negative");
    PSA_REQUIRE(n_groups <= nv + cols && (double)cols * (double)L < (double)(1ll << 28), "too many groups or columns");
    // the groups tile [0, nv): first vectors ascending from 0, the end entry nv; every column inside the result and used once
    PSA_REQUIRE(groups[0] == 0 && groups[2 * n_groups] == nv, "the groups do not tile [0, %lld): they run from %d to %d", (long long)nv,
                (int)groups[0], (int)groups[2 * n_groups]);
    std::vector<char> seen((size_t)cols, 0);
    for (int64_t g = 0; g < n_groups; ++g) {
        PSA_REQUIRE(groups[2 * g] <= groups[2 * g + 2], "the groups do not tile [0, %lld): group %lld begins at %d, the next at %d",
                    (long long)nv, (long long)g, (int)groups[2 * g], (int)groups[2 * g + 2]);
        const int32_t col = groups[2 * g + 1];
        PSA_REQUIRE(col >= 0 && col < cols && !seen[(size_t)col], "group %lld: column %d is outside [0, %lld) or used twice", (long long)g,
                    (int)col, (long long)cols);
        seen[(size_t)col] = 1;
    }
    for (int64_t i = 0; i < cols; ++i) PSA_REQUIRE(std::isfinite(scale[i]), "scale[%lld] is not finite", (long long)i);
    const int64_t Ab = atom_block == 0 ? na : std::min(atom_block, na), bv = vec_block == 0 ? nv : std::min(vec_block, nv),
                  bs = seg_block == 0 ? n_seg : std::min(seg_block, n_seg);
    PSA_REQUIRE((double)Ab * (double)bv * (double)bs * (double)L < (double)(1ll << 28),
                "a block of %lld x %lld x %lld x %lld elements is more than this entry serves", (long long)Ab, (long long)bv, (long long)bs,
                (long long)L);
    PSA_TRY(upload(c, c->d_rc_groups, groups, (size_t)(2 * (n_groups + 1)) * sizeof(int32_t)));
    PSA_TRY(upload(c, c->d_rc_scale, scale, (size_t)cols * sizeof(double)));
    std::vector<int64_t> vcut;
    for (int64_t v0 = 0; v0 < nv; v0 += bv) vcut.push_back(v0);
    vcut.push_back(nv);
    SelfPower w;
    w.L = L, w.n_seg = n_seg, w.n_atoms = na, w.cols = cols, w.n_groups = n_groups, w.groups = groups;
    w.mirror = mirror != 0, w.Ab = Ab, w.bs = bs, w.n_chunks = n_chunks, w.vcut = &vcut;
    std::vector<float2> part;
    const float2*       S = (const float2*)work_host;
    PSA_TRY(self_power_run(c, w, [&](int64_t a0, int64_t nab, int64_t vb, int64_t s0, int64_t ns, const float2** where) -> int {
        const int64_t v0 = vcut[(size_t)vb], nvb = vcut[(size_t)vb + 1] - v0;
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));     // the launches that read the last block have ended
        part.resize((size_t)nab * (size_t)nvb * (size_t)ns * (size_t)L);
        for (int64_t a = 0; a < nab; ++a)
            for (int64_t v = 0; v < nvb; ++v)
                std::memcpy(part.data() + ((size_t)a * (size_t)nvb + (size_t)v) * (size_t)ns * (size_t)L,
                            S + (((size_t)(a0 + a) * (size_t)nv + (size_t)(v0 + v)) * (size_t)n_seg + (size_t)s0) * (size_t)L,
                            (size_t)ns * (size_t)L * sizeof(float2));
        PSA_TRY(upload(c, c->d_rc_work, part.data(), part.size() * sizeof(float2)));
        PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
        *where = c->d_rc_work.as<float2>();
        return PSA_OK;
    }));
    const size_t want = (size_t)L * (size_t)cols * sizeof(float);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_rc_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_self_spectra(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* bin_of, int64_t n_bins,
                     const int32_t* idx, int64_t n_g, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, self_run(c, box_inverse, indices, K, bin_of, n_bins, idx, n_g, out_host, out_bytes), "psa_self_spectra");
}

int psa_debug_self_power(psa_ctx* c, const void* work_host, int64_t na, int64_t nv, int64_t n_seg, int64_t L, const int32_t* groups,
                         int64_t n_groups, int64_t cols, const double* scale, int32_t mirror, int64_t n_chunks, int64_t atom_block,
                         int64_t vec_block, int64_t seg_block, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, self_debug_power(c, work_host, na, nv, n_seg, L, groups, n_groups, cols, scale, mirror, n_chunks, atom_block,
                                            vec_block, seg_block, out_host),
                        "psa_debug_self_power");
}

int psa_debug_self_series(psa_ctx* c, const double* box_inverse, const int32_t* indices, int64_t K, const int32_t* idx, int64_t n_g,
                          void* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, self_debug_series(c, box_inverse, indices, K, idx, n_g, out_host), "psa_debug_self_series");
}

}  // extern "C"
