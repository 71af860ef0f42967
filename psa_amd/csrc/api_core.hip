// Context, error text, stage / one-off timing, rocFFT plans, options.
// (part of the C ABI of libpsa_hip.so, include/psa_hip.h; shared declarations: api_internal.h)
#include "api_internal.h"

#include <unistd.h>

#include <atomic>
#include <filesystem>

namespace psa {

thread_local std::string g_error;


void set_error(const char* fmt, ...) {
    char    buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}

// live DevBuf allocations of the process (psa_debug_device_buffers): a move hands one over and changes neither
static std::atomic<int64_t> g_devbuf_count{0}, g_devbuf_bytes{0};

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return PSA_OK;
    if (ptr) {
        PSA_HIP_CHECK(hipFree(ptr));
        g_devbuf_count -= 1;
        g_devbuf_bytes -= (int64_t)cap;
        ptr = nullptr;
        cap = 0;
    }
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e != hipSuccess) {
        ptr = nullptr;
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return PSA_ENOMEM;
    }
    cap = bytes;
    g_devbuf_count += 1;
    g_devbuf_bytes += (int64_t)bytes;
    if (fill) {                                        // armed (psa_debug_scratch_fill): no byte comes as the allocator left it
        PSA_HIP_CHECK(hipMemset(ptr, *fill, cap));
        PSA_HIP_CHECK(hipDeviceSynchronize());
    }
    return PSA_OK;
}

void DevBuf::release() {
    if (ptr) {
        (void)hipFree(ptr);
        g_devbuf_count -= 1;
        g_devbuf_bytes -= (int64_t)cap;
    }
    ptr = nullptr;
    cap = 0;
}

FftPlan::~FftPlan() {
    if (info) (void)rocfft_execution_info_destroy(info);
    if (plan) (void)rocfft_plan_destroy(plan);
}

int enter(psa_ctx* c) {
    PSA_REQUIRE(c != nullptr, "null context");
    PSA_HIP_CHECK(hipSetDevice(c->device));
    return PSA_OK;
}

// ---- stage timing: event pairs on the context's stream ---------------------
TimingState& timing(psa_ctx* c) { return c->timing; }

int get_event(TimingState& ts, hipEvent_t* ev) {
    if (!ts.pool.empty()) {
        *ev = ts.pool.back();
        ts.pool.pop_back();
        return PSA_OK;
    }
    PSA_HIP_CHECK(hipEventCreate(ev));
    return PSA_OK;
}

int collect(psa_ctx* c, TimingState& ts) {
    if (ts.pending.empty()) return PSA_OK;
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (auto& p : ts.pending) {
        float ms = 0.f;
        PSA_HIP_CHECK(hipEventElapsedTime(&ms, p.e0, p.e1));
        ts.acc[p.stage] += ms;
        if (p.stage == PSA_T_PROJECT) {
            ts.k1_launches += 1;
            ts.k1_ms += ms;
        }
        ts.pool.push_back(p.e0);
        ts.pool.push_back(p.e1);
    }
    ts.pending.clear();
    return PSA_OK;
}

int upload(psa_ctx* c, DevBuf& b, const void* host, size_t bytes) {
    PSA_TRY(b.reserve(bytes ? bytes : 16));
    if (bytes) PSA_HIP_CHECK(hipMemcpyAsync(b.ptr, host, bytes, hipMemcpyHostToDevice, c->stream));
    return PSA_OK;
}

static int create_plan(psa_ctx* c, int64_t T, int64_t batch, FftPlan* p) {
    size_t len = (size_t)T;
    PSA_FFT_CHECK(rocfft_plan_create(&p->plan, rocfft_placement_inplace, rocfft_transform_type_complex_forward,
                                     rocfft_precision_single, 1, &len, (size_t)batch, nullptr));
    PSA_FFT_CHECK(rocfft_plan_get_work_buffer_size(p->plan, &p->work_bytes));
    PSA_FFT_CHECK(rocfft_execution_info_create(&p->info));
    PSA_FFT_CHECK(rocfft_execution_info_set_stream(p->info, c->stream));
    return PSA_OK;
}

// the primer's plan (T, 3) -- one k-vector -- joins the cache; its kernels serve every batch of that length
static void join_primer(psa_ctx* c) {
    if (!c->fft_primer.joinable()) return;
    HostTimer ht(&c->oneoff_ms[0]);                    // whatever of the build is still outstanding
    c->fft_primer.join();
    if (c->primed.plan) {
        c->plans.try_emplace(std::make_pair(c->primed_T, (int64_t)3), std::move(c->primed));   // (a key that is there stays)
        c->primed = FftPlan{};
    }
}

void prime_fft(psa_ctx* c, int64_t T) {
    if (!c->opt_fft_prime || c->fft_primer.joinable() || T < 2 || c->primed_T == T) return;
    for (auto& kv : c->plans)
        if (kv.first.first == T) return;
    c->primed_T = T;
    c->fft_primer = std::thread([c, T] {
        (void)hipSetDevice(c->device);
        FftPlan p;
        if (create_plan(c, T, 3, &p) == PSA_OK) c->primed = std::move(p);
    });
}

int get_plan(psa_ctx* c, int64_t T, int64_t batch, FftPlan** out) {
    join_primer(c);
    auto key = std::make_pair(T, batch);
    auto it = c->plans.find(key);
    if (it == c->plans.end()) {
        HostTimer ht(&c->oneoff_ms[0]);
        FftPlan   p;
        PSA_TRY(create_plan(c, T, batch, &p));
        it = c->plans.emplace(key, std::move(p)).first;
    }
    *out = &it->second;
    return PSA_OK;
}

int run_fft(psa_ctx* c, float2* data, int64_t T, int64_t batch) {
    FftPlan* p = nullptr;
    PSA_TRY(get_plan(c, T, batch, &p));
    if (p->work_bytes) {
        PSA_TRY(c->d_fft_work.reserve(p->work_bytes));
        PSA_FFT_CHECK(rocfft_execution_info_set_work_buffer(p->info, c->d_fft_work.ptr, p->work_bytes));
    }
    void* bufs[1] = {data};
    PSA_FFT_CHECK(rocfft_execute(p->plan, bufs, nullptr, p->info));
    return PSA_OK;
}

int check_slot(psa_ctx* c, int slot) {
    PSA_REQUIRE(slot >= 0 && slot < PSA_NUM_SLOTS, "bad data slot %d", slot);
    PSA_REQUIRE(c->slot[slot].valid, "data slot %d holds no array", slot);
    return PSA_OK;
}

int validate_groups(int64_t N, const int32_t* group_idx, const int64_t* group_off, int32_t G) {
    PSA_REQUIRE(G >= 1, "need at least one atom group");
    if (!group_idx) {
        PSA_REQUIRE(G == 1, "group_idx NULL means one group of all atoms (G must be 1)");
        return PSA_OK;
    }
    PSA_REQUIRE(group_off != nullptr, "group_off is NULL");
    PSA_REQUIRE(group_off[0] == 0, "group_off[0] must be 0");
    for (int g = 0; g < G; ++g)
        PSA_REQUIRE(group_off[g + 1] >= group_off[g], "group_off must be non-decreasing");
    for (int64_t i = 0; i < group_off[G]; ++i)
        PSA_REQUIRE(group_idx[i] >= 0 && group_idx[i] < N, "Atom indices in basis out of bounds.");
    return PSA_OK;
}

// ---- the options: the one place that says which exist, what they are called and what they start at -----------------
// (include/psa_hip.h documents them; psa_option_info hands the table to Python and to tests/test_options_host.py)
constexpr int64_t OPT_FLAG = -1;                       // Option::min of an on / off option: stored as value != 0
struct Option {
    int              id;
    const char*      name;
    int64_t psa_ctx::*field;
    int64_t          def;
    int64_t          min;                              // least value accepted, or OPT_FLAG
};
#define PSA_OPTION(id, field, def, min) {id, #id, &psa_ctx::field, def, min}
constexpr Option OPTIONS[] = {
    PSA_OPTION(PSA_OPT_PLANES, opt_planes, 1, OPT_FLAG),
    PSA_OPTION(PSA_OPT_PLANES_BUDGET, opt_planes_budget, 0, 0),
    PSA_OPTION(PSA_OPT_PLANES_EAGER, opt_planes_eager, 0, OPT_FLAG),
    PSA_OPTION(PSA_OPT_PLANES_MIN_K, opt_planes_min_k, 17, 1),
    PSA_OPTION(PSA_OPT_FOLD_PAIRS, opt_fold_pairs, 1, OPT_FLAG),
    PSA_OPTION(PSA_OPT_FFT_PRIME, opt_fft_prime, 1, OPT_FLAG),
    PSA_OPTION(PSA_OPT_K1_LOADER_WAVES, opt_k1_loader_waves, 1, OPT_FLAG),
    PSA_OPTION(PSA_OPT_K1_WIDE, opt_k1_wide, 1, OPT_FLAG),
    PSA_OPTION(PSA_OPT_K1_LOWRANK, opt_k1_lowrank, 1, OPT_FLAG),
    PSA_OPTION(PSA_OPT_K1_LOWRANK_MIN_K, opt_k1_lowrank_min_k, 256, 1),
    PSA_OPTION(PSA_OPT_K1_LOWRANK_MIN_LOCAL, opt_k1_lowrank_min_local, 128, 1),
    PSA_OPTION(PSA_OPT_VDOS_WORK_BYTES, opt_vdos_work_bytes, (int64_t)1 << 30, 1),
    PSA_OPTION(PSA_OPT_MODES_WORK_BYTES, opt_modes_work_bytes, (int64_t)4 << 30, 1),
    PSA_OPTION(PSA_OPT_DYNAMIC_WORK_BYTES, opt_dynamic_work_bytes, (int64_t)4 << 30, 1),
    PSA_OPTION(PSA_OPT_K1_LOWRANK_PAIR, opt_k1_lowrank_pair, 1, OPT_FLAG),
};
#undef PSA_OPTION

// ---- the context's device buffers: the one place that says which exist and what their bytes are read as ------------
// (psa_debug_scratch_info hands the table to Python and to tests/test_scratch_table_host.py, which holds it against the
// DevBuf members of psa_ctx; psa_debug_scratch_fill walks it.  DESIGN.md says what every state buffer carries.)
//   real   every byte is read only as a float, float16, complex, double or a counter that is only added to: a pattern in it
//          can change a number, never an address
//   index  some part of it is read as an index, an offset, an address or a loop bound: it is only ever filled with zeros
//   state  it carries something from one call to a later one that the ABI promises: never filled
struct Scratch {
    const char*      name;
    DevBuf psa_ctx::*member;
    int              cls;
};
#define PSA_SCRATCH(member, cls) {#member, &psa_ctx::member, PSA_SCRATCH_##cls}
constexpr Scratch SCRATCH[] = {
    PSA_SCRATCH(d_kvec, REAL), PSA_SCRATCH(d_mean_all, REAL), PSA_SCRATCH(d_idx, INDEX), PSA_SCRATCH(d_mean_g, REAL),
    PSA_SCRATCH(d_phase, REAL), PSA_SCRATCH(d_qwork, REAL), PSA_SCRATCH(d_fft_work, REAL),
    PSA_SCRATCH(d_tables, INDEX),                          // (the synthetic fill's table holds component numbers)
    PSA_SCRATCH(d_absmax, REAL), PSA_SCRATCH(d_upload_max, REAL), PSA_SCRATCH(d_zeros, STATE),
    PSA_SCRATCH(d_qrows, REAL), PSA_SCRATCH(d_stage, REAL), PSA_SCRATCH(d_bin, REAL),
    PSA_SCRATCH(d_slab, REAL), PSA_SCRATCH(d_out, REAL), PSA_SCRATCH(d_aux, REAL),
    PSA_SCRATCH(d_kmap, INDEX), PSA_SCRATCH(d_cols, INDEX), PSA_SCRATCH(d_inten, REAL),
    PSA_SCRATCH(d_lr_diff, REAL), PSA_SCRATCH(d_lr_qn, REAL), PSA_SCRATCH(d_lr_L, REAL), PSA_SCRATCH(d_lr_phi, REAL),
    PSA_SCRATCH(d_lr_f64, REAL),
    PSA_SCRATCH(d_weights, STATE), PSA_SCRATCH(d_seg_window, STATE), PSA_SCRATCH(d_seg, REAL),
    PSA_SCRATCH(d_vdos_work, REAL), PSA_SCRATCH(d_vdos_pairs, INDEX), PSA_SCRATCH(d_vdos_off, INDEX), PSA_SCRATCH(d_vdos_mean, REAL),
    PSA_SCRATCH(d_vdos_part, REAL), PSA_SCRATCH(d_vdos_acc, REAL), PSA_SCRATCH(d_vdos_out, REAL),
    PSA_SCRATCH(d_modes_work, REAL), PSA_SCRATCH(d_modes_coef, REAL), PSA_SCRATCH(d_modes_out, REAL),
    PSA_SCRATCH(d_cov_slab, REAL), PSA_SCRATCH(d_cov_g, REAL), PSA_SCRATCH(d_cov_out, REAL),
    PSA_SCRATCH(d_peaks_spec, REAL), PSA_SCRATCH(d_peaks_bands, INDEX),
    PSA_SCRATCH(d_peaks_part, INDEX),                      // (the partial maxima come with their bins)
    PSA_SCRATCH(d_peaks_fit, REAL), PSA_SCRATCH(d_peaks_info, REAL),
    PSA_SCRATCH(d_rc_work, REAL), PSA_SCRATCH(d_rc_kappa, REAL), PSA_SCRATCH(d_rc_khat, REAL), PSA_SCRATCH(d_rc_idx, INDEX),
    PSA_SCRATCH(d_rc_tiles, INDEX), PSA_SCRATCH(d_rc_ent, INDEX), PSA_SCRATCH(d_rc_slot, INDEX), PSA_SCRATCH(d_rc_dest, INDEX),
    PSA_SCRATCH(d_rc_bins, INDEX), PSA_SCRATCH(d_rc_scale, REAL), PSA_SCRATCH(d_rc_acc, REAL), PSA_SCRATCH(d_rc_out, REAL),
    PSA_SCRATCH(d_rc_groups, INDEX), PSA_SCRATCH(d_rc_part, REAL),
    PSA_SCRATCH(d_corr_tab, REAL), PSA_SCRATCH(d_corr_factor, REAL), PSA_SCRATCH(d_corr_scale, REAL), PSA_SCRATCH(d_corr_in, REAL),
    PSA_SCRATCH(d_corr_out, REAL),
    PSA_SCRATCH(d_rs_idx, INDEX), PSA_SCRATCH(d_rs_items, INDEX), PSA_SCRATCH(d_rs_part, REAL), PSA_SCRATCH(d_rs_acc, REAL),
    PSA_SCRATCH(d_msd_u, REAL), PSA_SCRATCH(d_msd_img, REAL), PSA_SCRATCH(d_msd_sums, REAL), PSA_SCRATCH(d_msd_offs, REAL),
    PSA_SCRATCH(d_msd_sizes, REAL),
    PSA_SCRATCH(d_msd_lags, INDEX),                        // (a lag is a frame offset)
    PSA_SCRATCH(d_msd_out, REAL),
    PSA_SCRATCH(d_ov_q, REAL), PSA_SCRATCH(d_ov_sums, REAL),
    PSA_SCRATCH(d_pair_c, REAL),
    PSA_SCRATCH(d_angle_work, INDEX),                      // (the neighbour counts lie beside the lists)
    PSA_SCRATCH(d_angle_edges, REAL), PSA_SCRATCH(d_local_tab, REAL),
    PSA_SCRATCH(d_sync, REAL),
};
#undef PSA_SCRATCH
static const int SCRATCH_ZERO = 0;                     // what an armed index buffer is filled with, whatever the byte

}  // namespace psa

psa_ctx::psa_ctx() {
    for (const psa::Option& o : psa::OPTIONS) this->*o.field = o.def;
}

// What the members do not free themselves, once nothing can be in flight: the caller has set the device; the stream is
// drained and the primer joined before anything is closed.  The buffers, the plane sets and the rocFFT plans go after
// this body, as members: the stream they were used on is idle by then.
psa_ctx::~psa_ctx() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (fft_primer.joinable()) fft_primer.join();
    if (comm) (void)ncclCommDestroy(comm);
    for (auto& p : timing.pending) {
        (void)hipEventDestroy(p.e0);
        (void)hipEventDestroy(p.e1);
    }
    for (auto ev : timing.pool) (void)hipEventDestroy(ev);
    psa::stager_release(this);
    if (d2h_stream) (void)hipStreamDestroy(d2h_stream);
    if (d2h_ready) (void)hipEventDestroy(d2h_ready);
    if (stream) (void)hipStreamDestroy(stream);
}

using namespace psa;

extern "C" {

int psa_abi_version(void) { return PSA_HIP_ABI_VERSION; }

const char* psa_last_error(void) { return g_error.c_str(); }

int psa_device_count(int* count) {
    PSA_REQUIRE(count != nullptr, "null count");
    PSA_HIP_CHECK(hipGetDeviceCount(count));
    return PSA_OK;
}

int psa_host_alloc(size_t bytes, void** out) {
    PSA_REQUIRE(out != nullptr && bytes > 0, "bad argument");
    PSA_HIP_CHECK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return PSA_OK;
}

int psa_host_free(void* p) {
    if (p) PSA_HIP_CHECK(hipHostFree(p));
    return PSA_OK;
}

int psa_create(int device, psa_ctx** out) {
    PSA_REQUIRE(out != nullptr, "null out");
    int n = 0;
    PSA_HIP_CHECK(hipGetDeviceCount(&n));
    PSA_REQUIRE(device >= 0 && device < n, "device %d out of range (%d visible)", device, n);
    PSA_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    PSA_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    PSA_REQUIRE(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0,
                "libpsa_hip is built for gfx950 (MI355X) only; device %d is %s", device,
                prop.gcnArchName);
    static std::once_flag fft_once;
    std::call_once(fft_once, [] {
        // rocFFT keeps run-time compiled kernels in a cache file only when it is told where: give it a
        // per-user one (a second process then skips the compilation: 58 -> 23 ms for T = 65536,
        // tools/fft_plan_timing.py); an explicit ROCFFT_RTC_CACHE_PATH wins
        if (!std::getenv("ROCFFT_RTC_CACHE_PATH")) {
            std::string dir;
            if (const char* e = std::getenv("PSA_CACHE_DIR")) dir = e;
            else if (const char* x = std::getenv("XDG_CACHE_HOME")) dir = std::string(x) + "/psa_amd";
            else if (const char* h = std::getenv("HOME")) dir = std::string(h) + "/.cache/psa_amd";
            if (!dir.empty()) {
                std::error_code ec;
                std::filesystem::create_directories(dir, ec);
                if (!ec && ::access(dir.c_str(), W_OK) == 0)
                    ::setenv("ROCFFT_RTC_CACHE_PATH", (dir + "/rocfft_rtc_cache.db").c_str(), 0);
            }
        }
        (void)rocfft_setup();
    });
    psa_ctx* c = new psa_ctx();                        // (the options at the table's defaults)
    c->device = device;
    c->compute_units = prop.multiProcessorCount;
    // A/B switches of the low-rank route, read once here (psa_set_option overrides them)
    if (const char* v = std::getenv("PSA_K1_LOWRANK")) c->opt_k1_lowrank = std::atoi(v) != 0;
    if (const char* v = std::getenv("PSA_K1_LOWRANK_MIN_K")) c->opt_k1_lowrank_min_k = std::max(1, std::atoi(v));
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        return PSA_EHIP;
    }
    *out = c;
    return PSA_OK;
}

int psa_destroy(psa_ctx* c) {
    if (!c) return PSA_OK;
    { Guard g(c); }                                    // a call in flight on another thread ends first
    (void)hipSetDevice(c->device);
    delete c;
    return PSA_OK;
}

int psa_debug_device_buffers(int64_t* count, int64_t* bytes) {
    PSA_REQUIRE(count != nullptr && bytes != nullptr, "null argument");
    *count = g_devbuf_count.load();
    *bytes = g_devbuf_bytes.load();
    return PSA_OK;
}

int psa_debug_scratch_info(int index, const char** name, int32_t* cls) {
    PSA_REQUIRE(index >= 0 && index < (int)std::size(SCRATCH), "no device buffer at index %d", index);
    if (name) *name = SCRATCH[index].name;
    if (cls) *cls = SCRATCH[index].cls;
    return PSA_OK;
}

int psa_debug_scratch_fill(psa_ctx* c, int byte, int64_t* buffers, int64_t* bytes) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(byte >= -1 && byte <= 255, "the fill byte is 0 .. 255, or -1 to disarm");
    Guard g(c);
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->d2h_stream) PSA_HIP_CHECK(hipStreamSynchronize(c->d2h_stream));
    if (c->stager.copy_stream) PSA_HIP_CHECK(hipStreamSynchronize(c->stager.copy_stream));
    int64_t n = 0, total = 0;
    c->scratch_byte = byte;
    for (const Scratch& s : SCRATCH) {
        DevBuf& b = c->*s.member;
        b.fill = byte < 0 || s.cls == PSA_SCRATCH_STATE ? nullptr : s.cls == PSA_SCRATCH_REAL ? &c->scratch_byte : &SCRATCH_ZERO;
        if (!b.fill || !b.ptr) continue;
        PSA_HIP_CHECK(hipMemsetAsync(b.ptr, *b.fill, b.cap, c->stream));
        n += 1;
        total += (int64_t)b.cap;
    }
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    // the result went with d_slab, d_out and d_inten: a later psa_result_* or finalize finds what it finds after psa_create
    if (byte >= 0) c->slab_valid = c->out_valid = c->inten_valid = false;
    if (buffers) *buffers = n;
    if (bytes) *bytes = total;
    return PSA_OK;
}

int psa_synchronize(psa_ctx* c) {
    PSA_TRY(enter(c));
    Guard g(c);
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int psa_set_k1(psa_ctx* c, int selector) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(selector == PSA_K1_AUTO || selector == PSA_K1_WAVE || selector == PSA_K1_MFMA32 ||
                    selector == PSA_K1_SPLIT_BF16,
                "unknown K1 selector %d", selector);
    Guard g(c);
    c->k1_selector = selector;
    return PSA_OK;
}

int psa_set_k1_lowrank_fold(psa_ctx* c, int on) {
    PSA_TRY(enter(c));
    Guard g(c);
    c->k1_lowrank_fold = on != 0;
    return PSA_OK;
}

int psa_set_k1_lowrank_nodes(psa_ctx* c, int nodes) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(nodes == 48 || nodes == 64, "the low-rank route has 48 or 64 nodes, not %d", nodes);
    Guard g(c);
    c->k1_lowrank_nodes = nodes;
    return PSA_OK;
}

int psa_set_option(psa_ctx* c, int option, int64_t value) {
    PSA_TRY(enter(c));
    Guard g(c);
    for (const Option& o : OPTIONS) {
        if (o.id != option) continue;
        if (o.min == OPT_FLAG) value = value != 0;
        else if (o.min == 0) PSA_REQUIRE(value >= 0, "negative plane budget");
        else PSA_REQUIRE(value >= o.min, "%s must be >= %lld", o.name, (long long)o.min);
        c->*o.field = value;
        // switched off: what the option kept on the device goes
        if (option == PSA_OPT_PLANES && !value) {
            PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
            c->planes.clear();
        } else if (option == PSA_OPT_K1_LOWRANK && !value) {
            PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
            for (DevBuf* b : {&c->d_lr_diff, &c->d_lr_qn, &c->d_lr_L, &c->d_lr_phi, &c->d_lr_f64}) b->release();
        }
        return PSA_OK;
    }
    set_error("unknown option %d", option);
    return PSA_EINVAL;
}

int psa_option_info(int index, int32_t* option, int64_t* default_value, const char** name) {
    PSA_REQUIRE(index >= 0 && index < (int)std::size(OPTIONS), "no option at index %d", index);
    if (option) *option = OPTIONS[index].id;
    if (default_value) *default_value = OPTIONS[index].def;
    if (name) *name = OPTIONS[index].name;
    return PSA_OK;
}

int psa_device_info(psa_ctx* c, char* name, int name_len, int* compute_units, int64_t* hbm_bytes) {
    PSA_TRY(enter(c));
    hipDeviceProp_t prop;
    PSA_HIP_CHECK(hipGetDeviceProperties(&prop, c->device));
    if (name && name_len > 0) {
        std::snprintf(name, (size_t)name_len, "%s (%s)", prop.name[0] ? prop.name : "AMD GPU",
                      prop.gcnArchName);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return PSA_OK;
}

int psa_last_timings(psa_ctx* c, double* ms) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(ms != nullptr, "null output");
    Guard guard(c);
    TimingState& ts = timing(c);
    PSA_TRY(collect(c, ts));
    for (int i = 0; i < PSA_T_COUNT; ++i) {
        ms[i] = ts.acc[i];
        ts.acc[i] = 0.0;
    }
    return PSA_OK;
}

int psa_oneoff_stats(psa_ctx* c, double* ms) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(ms != nullptr, "null output");
    Guard guard(c);
    for (int i = 0; i < 4; ++i) {
        ms[i] = c->oneoff_ms[i];
        c->oneoff_ms[i] = 0.0;
    }
    return PSA_OK;
}

int psa_k1_lowrank_launches(psa_ctx* c, int64_t* launches) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(launches != nullptr, "null argument");
    *launches = c->lowrank_launches;
    return PSA_OK;
}

int psa_k1_lowrank_pair_launches(psa_ctx* c, int64_t* launches) {
    PSA_TRY(enter(c));
    PSA_REQUIRE(launches != nullptr, "null argument");
    *launches = c->lowrank_pair_launches;
    return PSA_OK;
}

int psa_k1_stats(psa_ctx* c, int64_t* launches, double* total_ms) {
    PSA_TRY(enter(c));
    Guard guard(c);
    TimingState& ts = timing(c);
    PSA_TRY(collect(c, ts));
    if (launches) *launches = ts.k1_launches;
    if (total_ms) *total_ms = ts.k1_ms;
    ts.k1_launches = 0;
    ts.k1_ms = 0.0;
    return PSA_OK;
}

}  // extern "C"
