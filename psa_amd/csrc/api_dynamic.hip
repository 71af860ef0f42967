// psa_dynamic_spectra: the dynamic structure factor and the longitudinal and transverse current correlations (definition:
// include/psa_hip.h; kernels: dynamic.hip).  The phase of every term comes from the atom's position in that very frame, so
// this path shares nothing with the projection machinery of psa_sed_project -- no phase table, no planes, no matrix
// cores -- and everything after the projection with the Welch paths.  Per block of kb k-vectors: the kernel writes
// q (kb, NC, T), NC = 1 (density) or 4 (density and the three current components), over all frames of the slots; without
// segments q is transformed in place by one batched rocFFT and read by the power pass as (kb, NC, 1, T); with segments
// it is cut, in sub-blocks of bk k-vectors x bs segments, into the segment buffer (bk, NC, bs, L) by the window pass,
// transformed by one batched length-L rocFFT and reduced; the power pass contracts the currents with k / |k| before the
// modulus, keeps the sum over a sub-block's segments on chip, overwrites the sub-block's columns of the (1 or 3, L, K)
// result with the first segments and adds to them with later ones.  Nothing of the SED entry points' state is touched.
// Budget (PSA_OPT_DYNAMIC_WORK_BYTES = W; q and the segment buffer share it, the result is outside), as for
// psa_sed_modes_welch: the segment buffer is promised min(what all K vectors' segments need, max(one (k, segment) unit,
// W / 8)), never more than W less one k-vector of q; q takes kb = the rest / (8 NC T) k-vectors, and the segment buffer
// then gets whatever q left over, cut into as many k-vectors as fit x the segments that then fit.  A call whose vectors
// hold the series of S species each (psa_partial_spectra: DynCall::n_species) counts S NC series where this says NC.
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

// The transform length of a call: L for the spectra (n_lags = 0); for the time correlations the smallest power of two
// >= L + n_lags - 1, after their refusals: 1 <= n_lags <= L, and segments (cut) only with the boxcar window.
int correlation_length(const psa_ctx* c, bool cut, int64_t L, int64_t n_lags, int64_t* P) {
    *P = L;
    if (n_lags == 0) return PSA_OK;
    PSA_REQUIRE(!cut || c->seg_boxcar, "the time correlations need the boxcar window (every value exactly 1): a tapered window "
                "biases a correlation function");
    PSA_REQUIRE(n_lags >= 1 && n_lags <= L, "n_lags = %lld is outside [1, L = %lld]", (long long)n_lags, (long long)L);
    for (*P = 1; *P < L + n_lags - 1;) *P *= 2;
    return PSA_OK;
}

// the context's segments, the sizes and the block rule of the budget (d->n_lags set: of a time-correlation call, whose
// segment buffer holds rows of P frames where the spectra's holds L)
int dynamic_plan(psa_ctx* c, DynCall* d) {
    const int64_t T = d->T, K = d->K;
    d->cut = c->seg_L != 0;
    d->L = d->cut ? c->seg_L : T, d->H = d->cut ? c->seg_hop : T;
    PSA_REQUIRE(d->L <= T, "segment length %lld exceeds the trajectory's %lld frames", (long long)d->L, (long long)T);
    d->n_seg = 1 + (T - d->L) / d->H;
    PSA_TRY(correlation_length(c, d->cut, d->L, d->n_lags, &d->P));
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

namespace {

// kappa = k / 2 pi in float64 from the float32 k, as float32 hi + lo; k / |k| in float64 (k = 0: 0)
void dynamic_directions(const float* k_vectors, int64_t K, DynCall* d) {
    const double two_pi = 6.283185307179586476925286766559;
    d->kappa.resize((size_t)K * 6);
    d->khat.assign((size_t)K * 3, 0.f);
    for (int64_t k = 0; k < K; ++k) {
        const double x = k_vectors[3 * k], y = k_vectors[3 * k + 1], z = k_vectors[3 * k + 2], norm = std::sqrt(x * x + y * y + z * z);
        for (int cc = 0; cc < 3; ++cc) {
            const double kap = (double)k_vectors[3 * k + cc] / two_pi;
            const float  hi = (float)kap;
            d->kappa[(size_t)k * 6 + cc] = hi;
            d->kappa[(size_t)k * 6 + 3 + cc] = (float)(kap - (double)hi);
            if (norm > 0.0) d->khat[(size_t)k * 3 + cc] = (float)((double)k_vectors[3 * k + cc] / norm);
        }
    }
}

// every refusal, the sizes and the block rule
int dynamic_check(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents, DynCall* d) {
    PSA_REQUIRE(k_vectors != nullptr, "null k_vectors");
    PSA_TRY(dynamic_inputs(c, "psa_dynamic_spectra", K, idx, n_g, currents, d));
    for (int64_t i = 0; i < 3 * K; ++i)
        PSA_REQUIRE(std::isfinite(k_vectors[i]), "k_vectors[%lld, %lld] is not finite", (long long)(i / 3), (long long)(i % 3));
    d->slices = dynamic_slices(K);
    PSA_TRY(dynamic_plan(c, d));

    dynamic_directions(k_vectors, K, d);
    return PSA_OK;
}

int dynamic_upload(psa_ctx* c, const DynCall& d, const int32_t* idx) {
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_dyn_kappa, d.kappa.data(), d.kappa.size() * sizeof(float)));
    PSA_TRY(upload(c, c->d_dyn_khat, d.khat.data(), d.khat.size() * sizeof(float)));
    if (idx) PSA_TRY(upload(c, c->d_dyn_idx, idx, (size_t)d.n_g * sizeof(int32_t)));
    return PSA_OK;
}

// k-vectors [k0, k0 + nk) over all frames into d_q (nk, NC, T)
int dynamic_project(psa_ctx* c, const DynCall& d, const int32_t* idx, int64_t k0, int64_t nk, float2* d_q) {
    StageTimer st(c, PSA_T_PROJECT);
    return launch_dynamic_project(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(),
                                  d.NC == 4 ? c->slot[PSA_SLOT_VELOCITIES].buf.as<float>() : nullptr,
                                  c->weights_N ? c->d_weights.as<float>() : nullptr, idx ? c->d_dyn_idx.as<int>() : nullptr,
                                  c->d_dyn_kappa.as<float>() + (size_t)k0 * 6, d_q, d.T, d.N, d.n_g, nk, d.NC == 4, d.slices);
}

int dynamic_run(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents, float* out_host,
                size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    DynCall d;
    PSA_TRY(dynamic_check(c, k_vectors, K, idx, n_g, currents, &d));
    const int64_t L = d.L, T = d.T, rows = currents ? 3 : 1;
    const size_t  want = (size_t)rows * (size_t)L * (size_t)K * sizeof(float);
    PSA_REQUIRE(out_bytes == want, "out_bytes is %zu, the (%lld,%lld,%lld) float32 result has %zu", out_bytes, (long long)rows,
                (long long)L, (long long)K, want);
    if (d.n_g == 0) {                                        // an empty atom set: zeros
        std::memset(out_host, 0, out_bytes);
        return PSA_OK;
    }
    PSA_TRY(dynamic_upload(c, d, idx));
    PSA_TRY(c->d_dyn_q.reserve((size_t)d.kb * (size_t)d.per_k));
    if (d.cut) PSA_TRY(c->d_seg.reserve((size_t)d.bk * (size_t)d.bs * (size_t)d.unit));
    PSA_TRY(c->d_dyn_out.reserve(want));

    const double U = d.cut ? c->seg_U : 1.0;
    const float  scale = (float)(1.0 / ((double)L * (double)L * (double)d.n_seg * U));
    float2*      d_q = c->d_dyn_q.as<float2>();
    float2*      d_seg = d.cut ? c->d_seg.as<float2>() : nullptr;
    float*       d_out = c->d_dyn_out.as<float>();
    PowerPass    pass;
    pass.NC = d.NC, pass.L = L, pass.n_seg = d.n_seg, pass.K = K, pass.scale = scale;
    pass.d_khat = c->d_dyn_khat.as<float>(), pass.d_out = d_out;
    for (int64_t k0 = 0; k0 < K; k0 += d.kb) {
        const int64_t nk = std::min(d.kb, K - k0);
        PSA_TRY(dynamic_project(c, d, idx, k0, nk, d_q));
        // without segments q is transformed where it lies: one sub-block (bk = kb) of the one segment
        PSA_TRY(power_block(c, pass, k0, nk, d.bk, d.bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
            float2* buf = d.cut ? d_seg : d_q;
            if (d.cut) {
                StageTimer st(c, PSA_T_EPILOGUE);
                PSA_TRY(launch_segment_window_rows(c, d_q + (size_t)k1 * (size_t)d.NC * (size_t)T, c->d_seg_window.as<float>(), d_seg, T, L,
                                                   d.H, s0, ns, nb * d.NC));
            }
            StageTimer st(c, PSA_T_FFT);
            PSA_TRY(run_fft(c, buf, L, (int64_t)d.NC * nb * ns));
            *where = buf;
            return PSA_OK;
        }));
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, d_out, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the kernel alone, block by block under the same rule: q (K, NC, T) before any FFT
int dynamic_debug_project(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents,
                          void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    DynCall d;
    PSA_TRY(dynamic_check(c, k_vectors, K, idx, n_g, currents, &d));
    if (d.n_g == 0) {
        std::memset(out_host, 0, (size_t)K * (size_t)d.per_k);
        return PSA_OK;
    }
    PSA_TRY(dynamic_upload(c, d, idx));
    PSA_TRY(c->d_dyn_q.reserve((size_t)d.kb * (size_t)d.per_k));
    for (int64_t k0 = 0; k0 < K; k0 += d.kb) {
        const int64_t nk = std::min(d.kb, K - k0);
        PSA_TRY(dynamic_project(c, d, idx, k0, nk, c->d_dyn_q.as<float2>()));
        PSA_HIP_CHECK(hipMemcpyAsync((char*)out_host + (size_t)k0 * (size_t)d.per_k, c->d_dyn_q.ptr, (size_t)nk * (size_t)d.per_k,
                                     hipMemcpyDeviceToHost, c->stream));
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

// the power pass alone on transformed segments (K, NC, n_seg, L) of the caller's: what dynamic_run does after its FFT,
// cut into sub-blocks of k_block vectors x seg_block segments (0: all)
int dynamic_debug_power(psa_ctx* c, const void* seg_host, const float* k_vectors, int64_t K, int32_t currents, int64_t n_seg, int64_t L,
                        int64_t k_block, int64_t seg_block, float scale, float* out_host) {
    PSA_REQUIRE(seg_host != nullptr && k_vectors != nullptr && out_host != nullptr, "null argument");
    PSA_REQUIRE(currents == 0 || currents == 1, "currents is 0 (density only) or 1 (density and currents), got %d", (int)currents);
    PSA_REQUIRE(K >= 1 && K < (1ll << 29) && n_seg >= 1 && L >= 1 && k_block >= 0 && seg_block >= 0,
                "K, n_seg and L are positive, k_block and seg_block not negative (%lld, %lld, %lld, %lld, %lld)", (long long)K,
                (long long)n_seg, (long long)L, (long long)k_block, (long long)seg_block);
    const int     NC = currents ? 4 : 1;
    const int64_t bk = k_block == 0 ? K : std::min(k_block, K), bs = seg_block == 0 ? n_seg : std::min(seg_block, n_seg);
    PSA_REQUIRE((double)bk * NC * (double)bs * (double)L < (double)(1ll << 28) && (double)K * (double)L < (double)(1ll << 28),
                "a sub-block of %lld x %d x %lld x %lld elements is more than this entry serves", (long long)bk, NC, (long long)bs,
                (long long)L);
    for (int64_t i = 0; i < 3 * K; ++i)
        PSA_REQUIRE(std::isfinite(k_vectors[i]), "k_vectors[%lld, %lld] is not finite", (long long)(i / 3), (long long)(i % 3));
    DynCall d;
    dynamic_directions(k_vectors, K, &d);
    const size_t want = (size_t)(currents ? 3 : 1) * (size_t)L * (size_t)K * sizeof(float);
    PSA_TRY(upload(c, c->d_dyn_khat, d.khat.data(), d.khat.size() * sizeof(float)));
    PSA_TRY(c->d_dyn_out.reserve(want));
    PowerPass pass;
    pass.NC = NC, pass.L = L, pass.n_seg = n_seg, pass.K = K, pass.scale = scale;
    pass.d_khat = c->d_dyn_khat.as<float>(), pass.d_out = c->d_dyn_out.as<float>();
    PSA_TRY(power_block(c, pass, 0, K, bk, bs, [&](int64_t k1, int64_t nb, int64_t s0, int64_t ns, const float2** where) -> int {
        PSA_TRY(upload_segments(c, c->d_dyn_q, seg_host, k1 * NC, nb * NC, n_seg, s0, ns, L));
        *where = c->d_dyn_q.as<float2>();
        return PSA_OK;
    }));
    PSA_HIP_CHECK(hipMemcpyAsync(out_host, c->d_dyn_out.ptr, want, hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_dynamic_spectra(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents,
                        float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, dynamic_run(c, k_vectors, K, idx, n_g, currents, out_host, out_bytes), "psa_dynamic_spectra");
}

int psa_debug_dynamic_project(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents,
                              void* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, dynamic_debug_project(c, k_vectors, K, idx, n_g, currents, out_host), "psa_debug_dynamic_project");
}

int psa_debug_dynamic_power(psa_ctx* c, const void* seg_host, const float* k_vectors, int64_t K, int32_t currents, int64_t n_seg, int64_t L,
                            int64_t k_block, int64_t seg_block, float scale, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    return synchronised(c, dynamic_debug_power(c, seg_host, k_vectors, K, currents, n_seg, L, k_block, seg_block, scale, out_host),
                        "psa_debug_dynamic_power");
}

int psa_debug_dynamic_sincos(psa_ctx* c, const float* turns, int64_t n, float* out_host) {
    PSA_TRY(enter(c));
    Guard guard(c);
    PSA_REQUIRE(turns != nullptr && out_host != nullptr && n >= 1 && n < (1ll << 28), "bad argument");
    // (scratch of this call alone: the projections' buffer, which holds nothing between calls)
    PSA_TRY(c->d_dyn_q.reserve((size_t)n * (sizeof(float) + sizeof(float2))));
    float2* d_out = c->d_dyn_q.as<float2>();
    float*  d_in = reinterpret_cast<float*>(d_out + n);
    int     rc = PSA_OK;
    if (hipMemcpyAsync(d_in, turns, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        set_error("upload of the sweep failed");
        rc = PSA_EHIP;
    }
    if (rc == PSA_OK) rc = launch_dynamic_sincos(c, d_in, d_out, n);
    if (rc == PSA_OK && hipMemcpyAsync(out_host, d_out, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        set_error("copy of the sweep failed");
        rc = PSA_EHIP;
    }
    return synchronised(c, rc, "psa_debug_dynamic_sincos");
}

}  // extern "C"
