// What the reciprocal-space entries share (api_dynamic.hip, api_lattice.hip, api_partial.hip, api_self.hip,
// api_correlation.hip; kernels: dynamic.hip, lattice.hip, partial.hip, self.hip, correlation.hip).  Every one of them
// projects on the phase of each frame's own positions, so none touches the projection machinery or the state of the SED
// entry points, and all of them work in the one buffer set d_rc_* (psa_ctx.h), which a call fills before it reads it.
//
// The run body (spectra_run).  Per block of kb k-vectors the family's projection writes q (kb, series, T) over all frames
// of the slots, series = NC = 1 (density) or 4 (density and the three current components), times the species of a partial
// call.  Without segments q is transformed in place by one batched rocFFT and read by the power pass as (kb, series, 1, T);
// with segments it is cut, in sub-blocks of bk k-vectors x bs segments, into the segment buffer (bk, series, bs, L) by the
// window pass, transformed by one batched length-L rocFFT and reduced.  A time-correlation call copies every segment,
// zero-padded to P frames, into the segment buffer instead (with or without segments) and transforms at length P.  The
// power pass (power_block) contracts the currents with k / |k| before the modulus -- or takes the products of species
// pairs --, keeps the sum over a sub-block's segments on chip, and either overwrites the sub-block's columns of the float32
// result with the first segments and adds to them with later ones, or, in the shell form, adds the sub-block's vectors to
// the float64 accumulator, which one last launch scales and rounds.
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W; q and the segment buffer share it, everything else is outside), as for
// psa_sed_modes_welch: the segment buffer is promised min(what all K vectors' segments need, max(one (k, segment) unit,
// W / 8)), never more than W less one k-vector of q; q takes kb = the rest / (8 series T) k-vectors, and the segment
// buffer then gets whatever q left over, cut into as many k-vectors as fit x the segments that then fit.
#include <cstdio>

#include "api_internal.h"

namespace psa {

// the refusals that concern the call's shape, the slots, the atom set and the weights (`entry`: who is asking)
int dynamic_inputs(psa_ctx* c, const char* entry, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents, DynCall* d) {
    PSA_REQUIRE(K >= 1 && K < (1ll << 29), "need at least one k-vector (K = %lld)", (long long)K);
    PSA_REQUIRE(currents == 0 || currents == 1, "currents is 0 (density only) or 1 (density and currents), got %d", (int)currents);
    PSA_REQUIRE(c->comm == nullptr && c->nranks == 1, "%s is not available on a sharded context (%d ranks)", entry, c->nranks);
    const DataSlot& pos = c->slot[PSA_SLOT_POSITIONS];
    const DataSlot& vel = c->slot[PSA_SLOT_VELOCITIES];
    PSA_REQUIRE(pos.valid, "the positions slot holds no array: the phase of %s is exp(i k.r(t))", entry);
    const int64_t T = pos.T, N = pos.N;
    PSA_REQUIRE(!currents || vel.valid, "currents need the velocities slot, which holds no array");
    PSA_REQUIRE(!currents || (vel.T == T && vel.N == N), "currents need velocities of the positions' shape: (%lld, %lld, 3) against "
                "(%lld, %lld, 3)", (long long)vel.T, (long long)vel.N, (long long)T, (long long)N);
    PSA_REQUIRE(idx == nullptr || (n_g >= 0 && n_g < (1ll << 31) - DYN_ATOMS), "bad number of atoms %lld", (long long)n_g);
    for (int64_t i = 0; idx && i < n_g; ++i) PSA_REQUIRE(idx[i] >= 0 && idx[i] < N, "Atom indices in basis out of bounds.");
    PSA_TRY(check_weights(c, N));
    d->T = T, d->N = N, d->K = K, d->n_g = idx ? n_g : N;
    d->NC = currents ? 4 : 1;
    return PSA_OK;
}

// The transform length P: L for the spectra (n_lags = 0); for the time correlations the smallest power of two
// >= L + n_lags - 1, after their refusals: 1 <= n_lags <= L, and segments (cut) only with the boxcar window.
int segment_shape(const psa_ctx* c, bool segments, DynCall* d) {
    const int64_t T = d->T, n_lags = d->n_lags;
    d->cut = segments && c->seg_L != 0;
    d->L = d->cut ? c->seg_L : T, d->H = d->cut ? c->seg_hop : T;
    PSA_REQUIRE(d->L <= T, "segment length %lld exceeds the trajectory's %lld frames", (long long)d->L, (long long)T);
    d->n_seg = 1 + (T - d->L) / d->H;
    d->P = d->L;
    if (n_lags == 0) return PSA_OK;
    PSA_REQUIRE(!d->cut || c->seg_boxcar, "the time correlations need the boxcar window (every value exactly 1): a tapered window "
                "biases a correlation function");
    PSA_REQUIRE(n_lags >= 1 && n_lags <= d->L, "n_lags = %lld is outside [1, L = %lld]", (long long)n_lags, (long long)d->L);
    for (d->P = 1; d->P < d->L + n_lags - 1;) d->P *= 2;
    return PSA_OK;
}

// the context's segments, the sizes and the block rule of the budget (d->n_lags set: of a time-correlation call, whose
// segment buffer holds rows of P frames where the spectra's holds L)
int dynamic_plan(psa_ctx* c, DynCall* d) {
    const int64_t T = d->T, K = d->K;
    PSA_TRY(segment_shape(c, true, d));
    // (the time correlations pad every segment to P frames: they use the segment buffer with or without segments)
    const bool buffered = d->cut || d->n_lags != 0;

    // the budget: q (kb k-vectors) first, the segment buffer (units of one k-vector x one segment) from the rest
    const int64_t W = c->opt_dynamic_work_bytes;
    const int64_t series = (int64_t)d->n_species * d->NC;    // per vector
    d->per_k = series * T * (int64_t)sizeof(float2);
    d->unit = buffered ? series * d->P * (int64_t)sizeof(float2) : 0;
    PSA_REQUIRE(W >= d->per_k + d->unit, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold one k-vector: "
                "%d series x (%lld frames + a segment of %lld) need %lld bytes", (long long)W, (int)series, (long long)T,
                (long long)(buffered ? d->P : 0), (long long)(d->per_k + d->unit));
    int64_t seg_bytes = 0;
    if (buffered) {
        const int64_t all = (double)K * (double)d->n_seg * (double)d->unit < 9e18 ? K * d->n_seg * d->unit : INT64_MAX;
        seg_bytes = std::min(std::min(all, std::max(d->unit, W / 8)), W - d->per_k);
    }
    // (the projection's grid: at most 65535 tiles of at least one k-vector; the passes' rows in 31 bits)
    d->kb = std::min<int64_t>({(W - seg_bytes) / d->per_k, K, 65535});
    d->bk = d->kb, d->bs = 1;
    if (buffered) {
        const int64_t units = std::min((W - d->kb * d->per_k) / d->unit, d->kb * d->n_seg);
        if (units >= d->kb) d->bs = std::min(d->n_seg, units / d->kb);
        else d->bk = units;
        d->bs = std::min(d->bs, std::max<int64_t>(1, ((1ll << 31) - 1) / (d->bk * series)));
    }
    return PSA_OK;
}

int power_block(psa_ctx* c, const PowerPass& p, int64_t k0, int64_t nk, int64_t bk, int64_t bs, const SegFill& fill) {
    for (int64_t k1 = 0; k1 < nk; k1 += bk) {
        const int64_t nb = std::min(bk, nk - k1);
        for (int64_t s0 = 0; s0 < p.n_seg; s0 += bs) {
            const int64_t ns = std::min(bs, p.n_seg - s0);
            const float2* d_seg = nullptr;
            PSA_TRY(fill(k1, nb, s0, ns, &d_seg));
            StageTimer st(c, PSA_T_EPILOGUE);
            if (p.n_species > 0 && p.d_bins)
                PSA_TRY(launch_partial_shell(c, d_seg, p.d_khat + (size_t)(k0 + k1) * 3, p.d_bins, p.d_acc, p.L, ns, k0 + k1, nb, p.n_bins,
                                             p.n_species, p.NC == 4));
            else if (p.n_species > 0)
                PSA_TRY(launch_partial_power(c, d_seg, p.d_khat + (size_t)(k0 + k1) * 3, p.d_out, p.L, ns, nb, p.n_species, p.NC == 4,
                                             p.K, k0 + k1, p.scale, s0 == 0));
            else if (p.d_bins)
                PSA_TRY(launch_lattice_shell(c, d_seg, p.d_khat + (size_t)(k0 + k1) * 3, p.d_bins, p.d_acc, p.L, ns, k0 + k1, nb, p.n_bins,
                                             p.NC == 4));
            else
                PSA_TRY(launch_dynamic_power(c, d_seg, p.d_khat + (size_t)(k0 + k1) * 3, p.d_out, p.L, ns, nb, p.NC == 4, p.K, k0 + k1,
                                             p.scale, s0 == 0));
        }
    }
    return PSA_OK;
}

int upload_segments(psa_ctx* c, DevBuf& b, const void* host, int64_t r0, int64_t nr, int64_t n_seg, int64_t s0, int64_t ns, int64_t L) {
    // (the launch that read the last upload has ended before its place is written again, and `part` outlives the copy)
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<float2> part((size_t)nr * (size_t)ns * (size_t)L);
    const float2*       S = (const float2*)host;
    for (int64_t r = 0; r < nr; ++r)
        std::memcpy(part.data() + (size_t)r * (size_t)ns * (size_t)L, S + ((size_t)(r0 + r) * (size_t)n_seg + (size_t)s0) * (size_t)L,
                    (size_t)ns * (size_t)L * sizeof(float2));
    PSA_TRY(upload(c, b, part.data(), part.size() * sizeof(float2)));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

void bin_counts(const int32_t* bin_of, int64_t K, int64_t n_bins, std::vector<int64_t>* count) {
    count->assign((size_t)n_bins, 0);
    for (int64_t k = 0; k < K; ++k) ++(*count)[(size_t)bin_of[k]];
}

int sorted_bin_counts(const int32_t* bin_of, int64_t K, int64_t n_bins, std::vector<int64_t>* count) {
    for (int64_t k = 0; k < K; ++k) {
        PSA_REQUIRE(bin_of[k] >= 0 && bin_of[k] < n_bins, "bin_of[%lld] = %d is outside [0, %lld)", (long long)k, (int)bin_of[k],
                    (long long)n_bins);
        PSA_REQUIRE(k == 0 || bin_of[k - 1] <= bin_of[k], "bin_of[%lld] = %d after %d: the vectors come sorted by bin", (long long)k,
                    (int)bin_of[k], (int)bin_of[k - 1]);
    }
    bin_counts(bin_of, K, n_bins, count);
    return PSA_OK;
}

void lattice_bins(const std::vector<int64_t>& count, double n_seg, double U, double L, std::vector<int32_t>* bin_start,
                  std::vector<double>* scale) {
    const size_t n_bins = count.size();
    bin_start->assign(n_bins + 1, 0);
    scale->assign(n_bins, 0.0);
    for (size_t b = 0; b < n_bins; ++b) {
        (*bin_start)[b + 1] = (int32_t)((*bin_start)[b] + count[b]);
        if (count[b]) (*scale)[b] = 1.0 / (2.0 * (double)count[b] * n_seg * U * L * L);
    }
}

int shell_begin(psa_ctx* c, size_t bytes, double** d_acc) {
    PSA_TRY(c->d_rc_acc.reserve(bytes));
    *d_acc = c->d_rc_acc.as<double>();
    PSA_HIP_CHECK(hipMemsetAsync(*d_acc, 0, bytes, c->stream));
    return PSA_OK;
}

int shell_finish(psa_ctx* c, int64_t n, int64_t n_bins, float* d_out) {
    StageTimer st(c, PSA_T_EPILOGUE);
    return launch_lattice_finish(c, c->d_rc_acc.as<double>(), c->d_rc_scale.as<double>(), d_out, n, n_bins);
}

int spectra_run(psa_ctx* c, const DynCall& d, const SpectraRun& a) {
    const bool    shell = a.n_bins > 0, corr = d.n_lags != 0, buffered = d.cut || corr;
    const int64_t L = d.L, T = d.T, K = d.K, P = d.P, rows = d.NC == 4 ? 3 : 1, cols = shell ? a.n_bins : K;
    const int64_t series = (int64_t)d.n_species * d.NC;      // per vector
    const int     pairs = a.pairs ? d.n_species * (d.n_species + 1) / 2 : 1;
    const int64_t len = corr ? d.n_lags : L;
    const size_t  want = (size_t)rows * (size_t)pairs * (size_t)len * (size_t)cols * sizeof(float);
    char          shape[96];
    if (a.pairs) std::snprintf(shape, sizeof shape, "(%lld,%d,%lld,%lld)", (long long)rows, pairs, (long long)len, (long long)cols);
    else std::snprintf(shape, sizeof shape, "(%lld,%lld,%lld)", (long long)rows, (long long)len, (long long)cols);
    PSA_REQUIRE(a.out_bytes == want, "out_bytes is %zu, the %s float32 result has %zu", a.out_bytes, shape, want);
    if (d.n_g == 0) {                                        // an empty atom set: zeros
        std::memset(a.out_host, 0, a.out_bytes);
        return PSA_OK;
    }
    PSA_TRY(a.src.upload());
    PSA_TRY(c->d_rc_work.reserve((size_t)d.kb * (size_t)d.per_k));
    if (buffered) PSA_TRY(c->d_seg.reserve((size_t)d.bk * (size_t)d.bs * (size_t)d.unit));
    // the power: the spectra's result itself; a time-correlation call's (rows, P, cols), float32 per vector, float64 per shell
    const size_t power = (size_t)rows * (size_t)pairs * (size_t)P * (size_t)cols;
    double*      d_acc = nullptr;
    if (!corr || !shell) PSA_TRY(c->d_rc_out.reserve(power * sizeof(float)));
    if (shell) PSA_TRY(shell_begin(c, power * sizeof(double), &d_acc));

    const double U = d.cut ? c->seg_U : 1.0;
    float2*      d_q = c->d_rc_work.as<float2>();
    float2*      d_seg = buffered ? c->d_seg.as<float2>() : nullptr;
    float*       d_out = c->d_rc_out.as<float>();
    PowerPass    pass;
    pass.NC = d.NC, pass.n_species = a.pairs ? d.n_species : 0, pass.L = P, pass.n_seg = d.n_seg, pass.K = K;
    pass.scale = corr ? 1.f : (float)(1.0 / ((double)L * (double)L * (double)d.n_seg * U));
    pass.d_khat = c->d_rc_khat.as<float>(), pass.d_out = d_out;
    if (shell) pass.d_bins = c->d_rc_bins.as<int>(), pass.d_acc = d_acc, pass.n_bins = a.n_bins;
    // the transformed segments of a sub-block; without segments q is transformed where it lies: one sub-block (bk = kb) of
    // the one segment
    const SegFill fill = [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
        float2*       buf = buffered ? d_seg : d_q;
        const float2* rows_q = d_q + (size_t)k1 * (size_t)series * (size_t)T;
        if (corr) {
            StageTimer st(c, PSA_T_GATHER);
            PSA_TRY(launch_correlation_pad(c, rows_q, d_seg, T, L, P, d.H, s0, ns, nb * series));
        } else if (d.cut) {
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_segment_window_rows(c, rows_q, c->d_seg_window.as<float>(), d_seg, T, L, d.H, s0, ns, nb * series));
        }
        StageTimer st(c, PSA_T_FFT);
        PSA_TRY(run_fft(c, buf, P, series * nb * ns));
        *where = buf;
        return PSA_OK;
    };
    int64_t block = 0;
    for (int64_t k0 = 0; k0 < K; k0 += d.kb, ++block) {
        const int64_t nk = std::min(d.kb, K - k0);
        {
            StageTimer st(c, PSA_T_PROJECT);
            PSA_TRY(a.src.project(block, k0, nk, d_q));
        }
        PSA_TRY(power_block(c, pass, k0, nk, d.bk, d.bs, fill));
    }
    if (a.finish) return a.finish(d_out, d_acc);
    if (shell) PSA_TRY(shell_finish(c, (int64_t)power, a.n_bins, d_out));
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(a.out_host, d_out, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int debug_project_run(psa_ctx* c, const DynCall& d, const BlockSource& src, void* out_host) {
    if (d.n_g == 0) {
        std::memset(out_host, 0, (size_t)d.K * (size_t)d.per_k);
        return PSA_OK;
    }
    PSA_TRY(src.upload());
    PSA_TRY(c->d_rc_work.reserve((size_t)d.kb * (size_t)d.per_k));
    int64_t block = 0;
    for (int64_t k0 = 0; k0 < d.K; k0 += d.kb, ++block) {
        const int64_t nk = std::min(d.kb, d.K - k0);
        {
            StageTimer st(c, PSA_T_PROJECT);
            PSA_TRY(src.project(block, k0, nk, c->d_rc_work.as<float2>()));
        }
        PSA_HIP_CHECK(hipMemcpyAsync((char*)out_host + (size_t)k0 * (size_t)d.per_k, c->d_rc_work.ptr, (size_t)nk * (size_t)d.per_k,
                                     hipMemcpyDeviceToHost, c->stream));
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int debug_power_check(DebugPower* a) {
    const int64_t K = a->K, n_seg = a->n_seg, L = a->L;
    PSA_REQUIRE(a->currents == 0 || a->currents == 1, "currents is 0 (density only) or 1 (density and currents), got %d", (int)a->currents);
    PSA_REQUIRE(K >= 1 && K < (1ll << 29) && n_seg >= 1 && L >= 1 && a->k_block >= 0 && a->seg_block >= 0,
                "K, n_seg and L are positive, k_block and seg_block not negative (%lld, %lld, %lld, %lld, %lld)", (long long)K,
                (long long)n_seg, (long long)L, (long long)a->k_block, (long long)a->seg_block);
    const bool shell = a->bin_of != nullptr;
    PSA_REQUIRE(!shell || (a->n_bins >= 1 && a->n_bins < (1ll << 24)), "need at least one bin (n_bins = %lld)", (long long)a->n_bins);
    PSA_REQUIRE(std::isfinite(a->norm) && a->norm > 0.0, "the norm n_seg U L^2 must be positive");
    const int64_t S = a->n_species, series = std::max<int64_t>(S, 1) * (a->currents ? 4 : 1), pairs = S ? S * (S + 1) / 2 : 1;
    a->bk = a->k_block == 0 ? K : std::min(a->k_block, K), a->bs = a->seg_block == 0 ? n_seg : std::min(a->seg_block, n_seg);
    PSA_REQUIRE((double)a->bk * (double)series * (double)a->bs * (double)L < (double)(1ll << 28) &&
                    (double)pairs * (double)(shell ? a->n_bins : K) * (double)L < (double)(1ll << 28),
                "a sub-block of %lld x %lld x %lld x %lld elements is more than this entry serves", (long long)a->bk, (long long)series,
                (long long)a->bs, (long long)L);
    return PSA_OK;
}

int debug_power_run(psa_ctx* c, const DebugPower& a, const float* khat) {
    const bool    shell = a.bin_of != nullptr;
    const int     NC = a.currents ? 4 : 1;
    const int64_t K = a.K, L = a.L, S = a.n_species, series = std::max<int64_t>(S, 1) * NC, pairs = S ? S * (S + 1) / 2 : 1;
    std::vector<int64_t> count;
    if (shell) PSA_TRY(sorted_bin_counts(a.bin_of, K, a.n_bins, &count));
    for (int64_t i = 0; a.currents && i < 3 * K; ++i) PSA_REQUIRE(std::isfinite(khat[i]), "khat[%lld] is not finite", (long long)i);
    const std::vector<float> zeros((size_t)K * 3, 0.f);
    PSA_TRY(upload(c, c->d_rc_khat, a.currents ? khat : zeros.data(), (size_t)K * 3 * sizeof(float)));
    const size_t want = (size_t)(a.currents ? 3 : 1) * (size_t)pairs * (size_t)L * (size_t)(shell ? a.n_bins : K) * sizeof(float);
    PSA_TRY(c->d_rc_out.reserve(want));
    PowerPass pass;
    pass.NC = NC, pass.n_species = a.n_species, pass.L = L, pass.n_seg = a.n_seg, pass.K = K, pass.scale = a.scale;
    pass.d_khat = c->d_rc_khat.as<float>(), pass.d_out = c->d_rc_out.as<float>();
    if (shell) {
        std::vector<int32_t> bin_start;
        std::vector<double>  scale;
        lattice_bins(count, a.norm, 1.0, 1.0, &bin_start, &scale);
        PSA_TRY(upload(c, c->d_rc_bins, bin_start.data(), bin_start.size() * sizeof(int32_t)));
        PSA_TRY(upload(c, c->d_rc_scale, scale.data(), scale.size() * sizeof(double)));
        PSA_TRY(shell_begin(c, want * 2, &pass.d_acc));
        pass.d_bins = c->d_rc_bins.as<int>(), pass.n_bins = a.n_bins;
    }
    PSA_TRY(power_block(c, pass, 0, K, a.bk, a.bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
        PSA_TRY(upload_segments(c, c->d_rc_work, a.seg_host, k1 * series, nb * series, a.n_seg, s0, ns, L));
        *where = c->d_rc_work.as<float2>();
        return PSA_OK;
    }));
    if (shell) PSA_TRY(shell_finish(c, (int64_t)(want / sizeof(float)), a.n_bins, pass.d_out));
    PSA_HIP_CHECK(hipMemcpyAsync(a.out_host, c->d_rc_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace psa
