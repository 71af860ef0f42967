// psa_fit_peaks / psa_sed_modes_fit / psa_sed_modes_welch_fit: Lorentzian fits of the peaks of spectrum columns
// (definition: include/psa_hip.h; kernels: peaks.hip).  The spectrum is either uploaded -- any (F, C) float32 array: an SED, a Welch-averaged SED, mode
// spectra saved earlier -- or the result of the mode projection where it lies (psa_ctx::d_modes_out), so that of a
// (T, K, M) array only 10 numbers per column cross to the host.  Nothing of the SED entry points' result state is touched.
#include "api_internal.h"

namespace psa {

int check_peak_args(const psa_peak_opts* opts, PeakArgs* a) {
    a->opts = opts ? *opts : psa_peak_opts{8.f, 0, 50};
    PSA_REQUIRE(a->fit != nullptr, "null fit");
    PSA_REQUIRE(a->info != nullptr, "null info");
    PSA_REQUIRE(a->F >= 12 && a->F < (1ll << 31), "F = %lld: a spectrum needs at least 12 (and fewer than 2^31) frequency bins",
                (long long)a->F);
    PSA_REQUIRE(a->C >= 1 && a->C < (1ll << 31), "C = %lld: need at least one column (and fewer than 2^31)", (long long)a->C);
    PSA_REQUIRE(std::isfinite(a->df) && a->df > 0.0, "df = %g must be a positive frequency step", a->df);
    PSA_REQUIRE(a->opts.window_hwhm > 0.f && std::isfinite(a->opts.window_hwhm), "window_hwhm = %g must be positive",
                (double)a->opts.window_hwhm);
    PSA_REQUIRE(a->opts.half_window_bins >= 0, "half_window_bins = %d must not be negative (0 = automatic)",
                (int)a->opts.half_window_bins);
    PSA_REQUIRE(a->opts.max_iter >= 1, "max_iter = %d: need at least one iteration", (int)a->opts.max_iter);
    const int64_t top = (a->F + 1) / 2;                              // bins 1 .. ceil(F/2) - 1: without DC and Nyquist
    if (!a->bands) {
        PSA_REQUIRE(a->lo < a->hi, "lo = %d, hi = %d: the band [lo, hi) is empty", (int)a->lo, (int)a->hi);
        PSA_REQUIRE(a->lo >= 1 && a->hi <= top, "lo = %d, hi = %d: the band must lie in [1, %lld), the positive half of %lld bins",
                    (int)a->lo, (int)a->hi, (long long)top, (long long)a->F);
        a->row0 = a->lo, a->row_end = a->hi;
        return PSA_OK;
    }
    int32_t lo_min = INT32_MAX, hi_max = 0;
    for (int64_t j = 0; j < a->C; ++j) {
        const int32_t lo = a->bands[2 * j], hi = a->bands[2 * j + 1];
        PSA_REQUIRE(lo < hi, "bands[%lld] = [%d, %d): lo >= hi, the band is empty", (long long)j, (int)lo, (int)hi);
        PSA_REQUIRE(lo >= 1 && hi <= top, "bands[%lld] = [%d, %d) must lie in [1, %lld), the positive half of %lld bins", (long long)j,
                    (int)lo, (int)hi, (long long)top, (long long)a->F);
        lo_min = std::min(lo_min, lo), hi_max = std::max(hi_max, hi);
    }
    a->row0 = lo_min, a->row_end = hi_max;
    return PSA_OK;
}

// the two kernels on a spectrum resident on the device, and the results to the host
int peaks_run(psa_ctx* c, const float* d_spec, const PeakArgs& a) {
    const int    n_slices = peaks_slices(a.C, a.row_end - a.row0);
    const size_t part = (size_t)n_slices * (size_t)a.C;
    PSA_TRY(c->d_peaks_part.reserve(part * (sizeof(float) + 2 * sizeof(int))));
    PSA_TRY(c->d_peaks_fit.reserve((size_t)a.C * 6 * sizeof(float)));
    PSA_TRY(c->d_peaks_info.reserve((size_t)a.C * 4 * sizeof(int32_t)));
    const int32_t* d_bands = nullptr;
    if (a.bands) {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_peaks_bands, a.bands, (size_t)a.C * 2 * sizeof(int32_t)));
        d_bands = c->d_peaks_bands.as<int32_t>();
    }
    float* d_pmax = c->d_peaks_part.as<float>();
    int*   d_pidx = reinterpret_cast<int*>(d_pmax + part);
    int*   d_pflag = d_pidx + part;
    {
        StageTimer st(c, PSA_T_EPILOGUE);
        PSA_TRY(launch_peak_find(c, d_spec, a.C, d_bands, a.lo, a.hi, a.row0, a.row_end, n_slices, d_pmax, d_pidx, d_pflag));
        PSA_TRY(launch_peak_fit(c, d_spec, a.C, d_bands, a.lo, a.hi, d_pmax, d_pidx, d_pflag, n_slices, a.df, a.opts.window_hwhm,
                                a.opts.half_window_bins, a.opts.max_iter, c->d_peaks_fit.as<float>(), c->d_peaks_info.as<int32_t>()));
    }
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(a.fit, c->d_peaks_fit.ptr, (size_t)a.C * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipMemcpyAsync(a.info, c->d_peaks_info.ptr, (size_t)a.C * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

namespace {

int fit_uploaded(psa_ctx* c, const float* spec_host, PeakArgs* a, const psa_peak_opts* opts) {
    PSA_REQUIRE(spec_host != nullptr, "null spec_host");
    PSA_TRY(check_peak_args(opts, a));
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_peaks_spec, spec_host, (size_t)a->F * (size_t)a->C * sizeof(float)));
    }
    return peaks_run(c, c->d_peaks_spec.as<float>(), *a);
}

// the mode spectra of `a` and their fit where they lie; `segments` as for modes_run
int fit_modes(psa_ctx* c, const ModesArgs& a, bool segments, PeakArgs* p, const psa_peak_opts* opts) {
    PSA_TRY(check_slot(c, a.slot));
    PSA_REQUIRE(a.K >= 0 && a.K < (1ll << 29) && a.M >= 0 && a.M < (1ll << 30), "bad number of k-vectors %lld or mode vectors %lld",
                (long long)a.K, (long long)a.M);
    p->F = segments && c->seg_L ? c->seg_L : c->slot[a.slot].T, p->C = a.K * a.M;
    PSA_TRY(check_peak_args(opts, p));
    PSA_TRY(modes_run(c, a, segments, true));
    return peaks_run(c, c->d_modes_out.as<float>(), *p);
}

}  // namespace

}  // namespace psa

using namespace psa;

extern "C" {

int psa_fit_peaks(psa_ctx* c, const float* spec_host, int64_t F, int64_t C, double df, const int32_t* bands, int32_t lo, int32_t hi,
                  const psa_peak_opts* opts, float* fit, int32_t* info) {
    PSA_TRY(enter(c));
    Guard    guard(c);
    PeakArgs a{F, C, df, bands, lo, hi, {}, fit, info};
    return synchronised(c, fit_uploaded(c, spec_host, &a, opts), "psa_fit_peaks");
}

int psa_sed_modes_fit(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K, const int32_t* group_idx,
                      const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags, double df, const int32_t* bands,
                      int32_t lo, int32_t hi, const psa_peak_opts* opts, float* fit, int32_t* info, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard           guard(c);
    const ModesArgs a{slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, out_host, out_bytes};
    PeakArgs        p{0, 0, df, bands, lo, hi, {}, fit, info};
    return synchronised(c, fit_modes(c, a, false, &p, opts), "psa_sed_modes_fit");
}

int psa_sed_modes_welch_fit(psa_ctx* c, int slot, const float* mean_pos_all, const float* k_vectors, int64_t K,
                            const int32_t* group_idx, const int64_t* group_off, int32_t B, const void* eig, int64_t M, int32_t flags,
                            double df, const int32_t* bands, int32_t lo, int32_t hi, const psa_peak_opts* opts, float* fit,
                            int32_t* info, float* out_host, size_t out_bytes) {
    PSA_TRY(enter(c));
    Guard           guard(c);
    const ModesArgs a{slot, mean_pos_all, k_vectors, K, group_idx, group_off, B, (const float*)eig, M, flags, out_host, out_bytes};
    PeakArgs        p{0, 0, df, bands, lo, hi, {}, fit, info};
    return synchronised(c, fit_modes(c, a, true, &p, opts), "psa_sed_modes_welch_fit");
}

}  // extern "C"
