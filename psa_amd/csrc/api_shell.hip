// The host core of the entries on the neighbour shells (api_shell.h): their checks and the block rule, the work buffer and
// its layout, the item table, the one run body over the blocks of origins, the per-atom copies, the start of the entries of
// one frame and the tables of the q_lm pass.  Only the positions slot is read; atom weights and segments set on the context
// are ignored; nothing of the other entry points' state is touched.
#include "api_shell.h"

namespace psa {

constexpr int64_t ANGLE_PART_BYTES = 64 << 20;  // what the items' partials aim to stay below

int cutoff_symmetric(const char* name, const double* m, int S, int a, int b) {
    PSA_REQUIRE(m[a * S + b] == m[b * S + a], "%s is not symmetric: [%d][%d] = %.17g, [%d][%d] = %.17g", name, a, b, m[a * S + b], b, a,
                m[b * S + a]);
    return PSA_OK;
}

int cutoff_reciprocal(const double* box_inverse, const char* name, int a, int b, double r, float* inv) {
    char what[32];
    std::snprintf(what, sizeof what, "%s[%d][%d]", name, a, b);
    PSA_TRY(served_radius_check(box_inverse, what, r));
    *inv = r > 0.0 ? (float)(1.0 / r) : 0.f;
    PSA_REQUIRE(r == 0.0 || (std::isfinite(*inv) && *inv > 0.f), "%s = %g has no float32 reciprocal", what, r);
    return PSA_OK;
}

int shell_check(ShellCall* s, const char* entry, const ShellLayout& layout) {
    psa_ctx*      c = s->c;
    AtomGroups*   p = &s->p;
    AngleSpecies* sp = &s->sp;
    PSA_TRY(group_list_check(c, entry, s->box, s->box_inverse, s->idx, s->group_start, s->n_groups, p));
    PSA_REQUIRE(s->r_cut != nullptr, "null r_cut");
    const int    S = p->G;
    *sp = AngleSpecies{};
    sp->S = S;
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) {
            const double r = s->r_cut[a * S + b];
            PSA_REQUIRE(std::isfinite(r) && r >= 0.0, "r_cut[%d][%d] must be finite and not negative, got %g", a, b, r);
            PSA_TRY(cutoff_symmetric("r_cut", s->r_cut, S, a, b));
            PSA_TRY(cutoff_reciprocal(s->box_inverse, "r_cut", a, b, r, &sp->inv_rc[a * S + b]));
        }
    PSA_REQUIRE(p->n_a < (1ll << ANGLE_SPECIES_SHIFT), "at most 2^%d - 1 listed atoms are served, got %lld", ANGLE_SPECIES_SHIFT,
                (long long)p->n_a);
    for (int g = 0; g <= S; ++g) sp->start[g] = (int)p->start[(size_t)g];
    for (int g = 0; g < S; ++g) sp->tile_first[g + 1] = sp->tile_first[g] + (int)((p->size[(size_t)g] + ANGLE_CENTRES - 1) / ANGLE_CENTRES);
    const int64_t W = c->opt_dynamic_work_bytes, per_origin = (ANGLE_ORIGIN_BYTES + layout.bytes()) * std::max<int64_t>(p->n_a, 1);
    PSA_REQUIRE(W / per_origin >= 1, "the work budget of %lld bytes (PSA_OPT_DYNAMIC_WORK_BYTES) cannot hold the smallest block: the "
                "fractional coordinates, neighbour counts and neighbour lists of %lld atoms at one origin need %lld bytes", (long long)W,
                (long long)p->n_a, (long long)per_origin);
    PSA_REQUIRE(s->origin_step >= 1, "origin_step must be at least 1, got %lld", (long long)s->origin_step);
    s->n_o = (p->T - 1) / s->origin_step + 1;
    p->Ab = std::min<int64_t>({s->n_o, W / per_origin, 65535});
    return PSA_OK;
}

int angle_work(psa_ctx* c, int64_t n_a, int64_t B, const ShellLayout& behind, AngleWork* w) {
    const size_t rows = (size_t)B * (size_t)n_a;
    PSA_TRY(c->d_angle_work.reserve(rows * (size_t)(ANGLE_ORIGIN_BYTES + behind.bytes())));
    char* base = static_cast<char*>(c->d_angle_work.ptr);
    w->list = reinterpret_cast<float4*>(base);
    w->c = reinterpret_cast<float*>(base + rows * 16 * ANGLE_MAX_NEIGHBOURS);
    w->count = reinterpret_cast<int*>(base + rows * (16 * ANGLE_MAX_NEIGHBOURS + 12));
    w->x = behind.bytes() ? reinterpret_cast<long long*>(base + rows * (size_t)ANGLE_ORIGIN_BYTES) : nullptr;
    w->behind = behind, w->cap = rows;
    return PSA_OK;
}

std::vector<AngleItem> angle_items(const AtomGroups& p, int64_t n_ob, int64_t row, int32_t* first) {
    int64_t tiles = 0;
    for (int g = 0; g < p.G; ++g) tiles += (p.size[(size_t)g] + ANGLE_ITEM_CENTRES - 1) / ANGLE_ITEM_CENTRES;
    const int64_t target = std::max<int64_t>(1, std::min(REALSPACE_TARGET_GROUPS, ANGLE_PART_BYTES / (row * (int64_t)sizeof(uint32_t))));
    int64_t       n_os = std::max<int64_t>(1, std::min(n_ob, target / std::max<int64_t>(1, tiles)));
    n_os = std::max(n_os, (n_ob + ANGLE_MAX_SLAB - 1) / ANGLE_MAX_SLAB);
    std::vector<AngleItem> items;
    for (int g = 0; g < p.G; ++g) {
        first[g] = (int32_t)items.size();
        for (int64_t lo = p.start[(size_t)g]; lo < p.start[(size_t)g + 1]; lo += ANGLE_ITEM_CENTRES)
            for (int64_t slab = 0; slab < n_os; ++slab)
                items.push_back(AngleItem{(int)lo, (int)std::min<int64_t>(ANGLE_ITEM_CENTRES, p.start[(size_t)g + 1] - lo), g, (int)slab, (int)n_os});
    }
    first[p.G] = (int32_t)items.size();
    return items;
}

int shell_run(ShellCall& s, int64_t row, const ShellLayout& layout, const ShellPass& pass, const ShellPass& after, std::vector<uint64_t>* acc,
              int64_t tail) {
    psa_ctx*      c = s.c;
    AtomGroups&   p = s.p;
    const int     S = p.G;
    const int64_t B = p.Ab;
    int32_t                      first[PAIR_MAX_SPECIES + 1];
    const std::vector<AngleItem> items = angle_items(p, B, row, first);
    AngleWork                    w;
    HistRows                     rows;
    PSA_TRY(rows_of_groups(first, S, 1, &rows));
    PSA_TRY(upload_atom_list(c, &p, s.idx));
    {
        StageTimer st(c, PSA_T_H2D);
        PSA_TRY(upload(c, c->d_rs_items, items.data(), items.size() * sizeof(AngleItem)));
    }
    PSA_TRY(c->d_rs_part.reserve(items.size() * (size_t)row * sizeof(uint32_t)));
    const size_t acc_words = (size_t)S * (size_t)row + (size_t)tail;
    PSA_TRY(c->d_rs_acc.reserve(acc_words * sizeof(uint64_t)));
    PSA_HIP_CHECK(hipMemsetAsync(c->d_rs_acc.ptr, 0, acc_words * sizeof(uint64_t), c->stream));
    PSA_TRY(angle_work(c, p.n_a, B, layout, &w));
    const float* d_pos = c->slot[PSA_SLOT_POSITIONS].buf.as<float>();
    for (int64_t k0 = 0; k0 < s.n_o; k0 += B) {
        const int64_t nb = std::min(B, s.n_o - k0);
        {
            StageTimer st(c, PSA_T_GATHER);
            PSA_TRY(launch_pair_frac(c, d_pos, p.d_idx, p.n_a, s.box_inverse, w.c, k0 * s.origin_step, s.origin_step, nb, p.T, p.N));
        }
        {
            StageTimer st(c, PSA_T_TRANSPOSE);
            PSA_TRY(launch_angle_neighbours(c, w.c, w.count, w.list, s.sp, s.box, p.n_a, nb));
        }
        {
            StageTimer st(c, PSA_T_PHASE);
            PSA_TRY(pass(w, (int64_t)items.size(), k0, nb));
        }
        {
            StageTimer st(c, PSA_T_EPILOGUE);
            PSA_TRY(launch_hist_reduce(c, c->d_rs_part.as<unsigned>(), rows, S, 1, row, c->d_rs_acc.as<unsigned long long>()));
        }
        if (after) PSA_TRY(after(w, (int64_t)items.size(), k0, nb));
    }
    acc->resize(acc_words);
    StageTimer st(c, PSA_T_D2H);
    PSA_HIP_CHECK(hipMemcpyAsync(acc->data(), c->d_rs_acc.ptr, acc->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return PSA_OK;
}

int copy_atom_rows(psa_ctx* c, int64_t n_a, int64_t k0, int64_t nb, std::initializer_list<AtomRows> rows) {
    StageTimer   st(c, PSA_T_D2H);
    const size_t at = (size_t)k0 * (size_t)n_a, cells = (size_t)nb * (size_t)n_a;
    for (const AtomRows& r : rows)
        if (r.host != nullptr)
            PSA_HIP_CHECK(hipMemcpyAsync(static_cast<char*>(r.host) + at * r.cell, r.dev, cells * r.cell, hipMemcpyDeviceToHost, c->stream));
    return PSA_OK;
}

int shell_one_frame(ShellCall& s, int64_t frame, const ShellLayout& layout, AngleWork* w) {
    psa_ctx*    c = s.c;
    AtomGroups& p = s.p;
    PSA_REQUIRE(frame >= 0 && frame <= p.T - 1, "frame %lld is outside [0, T - 1 = %lld]", (long long)frame, (long long)(p.T - 1));
    *w = AngleWork{};
    if (p.n_a == 0) return PSA_OK;
    PSA_TRY(upload_atom_list(c, &p, s.idx));
    PSA_TRY(angle_work(c, p.n_a, 1, layout, w));
    PSA_TRY(launch_pair_frac(c, c->slot[PSA_SLOT_POSITIONS].buf.as<float>(), p.d_idx, p.n_a, s.box_inverse, w->c, frame, 0, 1, p.T, p.N));
    return launch_angle_neighbours(c, w->c, w->count, w->list, s.sp, s.box, p.n_a, 1);
}

int upload_local_tables(psa_ctx* c, const int32_t* ls, int32_t n_ls, const double* w3j) {
    std::vector<double> tab((size_t)LOCAL_NORM_WORDS + (size_t)n_ls * LOCAL_W3J_WORDS, 0.0);
    for (int l = 0; l <= ORDER_MAX_L; ++l)
        for (int m = 0; m <= l; ++m) {
            double prod = 1.0;
            for (int k = l - m + 1; k <= l + m; ++k) prod *= (double)k;
            tab[(size_t)(l * (ORDER_MAX_L + 1) + m)] = (m & 1 ? -1.0 : 1.0) * std::sqrt(1.0 / prod);
        }
    for (int j = 0; w3j != nullptr && j < n_ls; ++j) {
        const size_t side = 2 * (size_t)ls[j] + 1;
        std::memcpy(&tab[(size_t)LOCAL_NORM_WORDS + (size_t)j * LOCAL_W3J_WORDS], w3j, side * side * sizeof(double));
        w3j += side * side;
    }
    StageTimer st(c, PSA_T_H2D);
    return upload(c, c->d_local_tab, tab.data(), tab.size() * sizeof(double));
}

}  // namespace psa
