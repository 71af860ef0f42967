// psa_dynamic_spectra: the dynamic structure factor and the longitudinal and transverse current correlations at k-vectors
// of the caller's choosing (definition: include/psa_hip.h; kernels: dynamic.hip).  Over the shared core (api_reciprocal.hip:
// checks, segments, budget, the run body and the debug loops) this file adds what concerns arbitrary k-vectors: their
// check, kappa = k / 2 pi as float32 hi + lo and k / |k| in float64, their upload, the projection launch -- and
// psa_debug_dynamic_sincos.
#include "api_internal.h"

namespace psa {

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

// the call's uploads, and k-vectors [k0, k0 + nk) over all frames into d_q (nk, NC, T)
BlockSource dynamic_source(psa_ctx* c, const DynCall& d, const int32_t* idx) {
    BlockSource src;
    src.upload = [c, &d, idx]() -> int {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_rc_kappa, d.kappa.data(), d.kappa.size() * sizeof(float)));
        PSA_TRY(upload(c, c->d_rc_khat, d.khat.data(), d.khat.size() * sizeof(float)));
        if (idx) PSA_TRY(upload(c, c->d_rc_idx, idx, (size_t)d.n_g * sizeof(int32_t)));
        return PSA_OK;
    };
    src.project = [c, &d, idx](int64_t, int64_t k0, int64_t nk, float2* d_q) -> int {
        return launch_dynamic_project(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(),
                                      d.NC == 4 ? c->slot[PSA_SLOT_VELOCITIES].buf.as<float>() : nullptr,
                                      c->weights_N ? c->d_weights.as<float>() : nullptr, idx ? c->d_rc_idx.as<int>() : nullptr,
                                      c->d_rc_kappa.as<float>() + (size_t)k0 * 6, d_q, d.T, d.N, d.n_g, nk, d.NC == 4, d.slices);
    };
    return src;
}

int dynamic_run(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents, float* out_host,
                size_t out_bytes) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    DynCall d;
    PSA_TRY(dynamic_check(c, k_vectors, K, idx, n_g, currents, &d));
    SpectraRun a;
    a.src = dynamic_source(c, d, idx), a.out_host = out_host, a.out_bytes = out_bytes;
    return spectra_run(c, d, a);
}

// the kernel alone, block by block under the same rule: q (K, NC, T) before any FFT
int dynamic_debug_project(psa_ctx* c, const float* k_vectors, int64_t K, const int32_t* idx, int64_t n_g, int32_t currents,
                          void* out_host) {
    PSA_REQUIRE(out_host != nullptr, "null output");
    DynCall d;
    PSA_TRY(dynamic_check(c, k_vectors, K, idx, n_g, currents, &d));
    return debug_project_run(c, d, dynamic_source(c, d, idx), out_host);
}

// the power pass alone on transformed segments (K, NC, n_seg, L) of the caller's: what the run does after its FFT
int dynamic_debug_power(psa_ctx* c, const void* seg_host, const float* k_vectors, int64_t K, int32_t currents, int64_t n_seg, int64_t L,
                        int64_t k_block, int64_t seg_block, float scale, float* out_host) {
    PSA_REQUIRE(seg_host != nullptr && k_vectors != nullptr && out_host != nullptr, "null argument");
    DebugPower a{.seg_host = seg_host, .K = K, .currents = currents, .n_seg = n_seg, .L = L, .k_block = k_block, .seg_block = seg_block,
                 .scale = scale, .out_host = out_host};
    PSA_TRY(debug_power_check(&a));
    for (int64_t i = 0; i < 3 * K; ++i)
        PSA_REQUIRE(std::isfinite(k_vectors[i]), "k_vectors[%lld, %lld] is not finite", (long long)(i / 3), (long long)(i % 3));
    DynCall d;
    dynamic_directions(k_vectors, K, &d);
    return debug_power_run(c, a, d.khat.data());
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
    PSA_TRY(c->d_rc_work.reserve((size_t)n * (sizeof(float) + sizeof(float2))));
    float2* d_out = c->d_rc_work.as<float2>();
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
