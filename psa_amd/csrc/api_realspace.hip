// What the real-space entries share on the host (api_msd.hip: MSD and the self van Hove function; api_pair.hip: g(r) and
// the distinct van Hove function; api_shell.hip: the entries on the neighbour shells): the atom groups of a call and their checks,
// the box's determinant, inverse and served radius, the arguments of a histogram over lags, the atom-list upload and the
// row ranges of the integer reduce (hist_reduce.hip).  Every refusal of these entries that does not concern one family
// alone is worded here, once.
#include "api_internal.h"

namespace psa {

static_assert(PAIR_MAX_SPECIES == MSD_MAX_GROUPS, "the species of a pair or angle call are the groups of the displacement calls");
static_assert(PAIR_MAX_SPECIES * PAIR_MAX_SPECIES <= HIST_REDUCE_MAX_ROWS, "the ordered species pairs are the most rows of a reduce");

int invertible_check(const double* a, const char* name, double* det) {
    *det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    double scale = 0.0;
    for (int i = 0; i < 9; ++i) scale = std::max(scale, std::fabs(a[i]));
    PSA_REQUIRE(std::isfinite(*det) && std::fabs(*det) > 1e-12 * scale * scale * scale, "%s is singular (determinant %g)", name, *det);
    return PSA_OK;
}

void inverse3(const double* a, double det, double* H) {
    H[0] = (a[4] * a[8] - a[5] * a[7]) / det, H[1] = (a[2] * a[7] - a[1] * a[8]) / det, H[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    H[3] = (a[5] * a[6] - a[3] * a[8]) / det, H[4] = (a[0] * a[8] - a[2] * a[6]) / det, H[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    H[6] = (a[3] * a[7] - a[4] * a[6]) / det, H[7] = (a[1] * a[6] - a[0] * a[7]) / det, H[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

int group_list_check(psa_ctx* c, const char* entry, const double* box, const double* box_inverse, const int32_t* idx,
                     const int64_t* group_start, int32_t n_groups, AtomGroups* p) {
    PSA_REQUIRE(c->comm == nullptr && c->nranks == 1, "%s is not available on a sharded context (%d ranks)", entry, c->nranks);
    const DataSlot& pos = c->slot[PSA_SLOT_POSITIONS];
    PSA_REQUIRE(pos.valid, "the positions slot holds no array: %s reads the positions", entry);
    PSA_REQUIRE(box != nullptr && box_inverse != nullptr, "null box or box_inverse");
    for (int i = 0; i < 9; ++i) PSA_REQUIRE(std::isfinite(box[i]) && std::isfinite(box_inverse[i]), "box and box_inverse must be finite");
    double det;
    PSA_TRY(invertible_check(box, "the box", &det));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double e = 0.0;
            for (int k = 0; k < 3; ++k) e += box[3 * i + k] * box_inverse[3 * k + j];
            PSA_REQUIRE(std::fabs(e - (i == j ? 1.0 : 0.0)) < 1e-6, "box_inverse is not the inverse of box: (H Hinv)[%d][%d] = %g", i, j, e);
        }
    PSA_REQUIRE(n_groups >= 1 && n_groups <= MSD_MAX_GROUPS, "the number of atom groups is in [1, %d], got %d", MSD_MAX_GROUPS,
                (int)n_groups);
    p->T = pos.T, p->N = pos.N, p->G = n_groups;
    PSA_REQUIRE(p->T >= 1 && p->T < (1ll << 31) && p->N < (1ll << 31), "a trajectory of (%lld, %lld) is more than this entry serves",
                (long long)p->T, (long long)p->N);
    if (!idx) {
        PSA_REQUIRE(n_groups == 1, "idx NULL means one group of all atoms (n_groups must be 1)");
        p->start = {0, p->N};
    } else {
        PSA_REQUIRE(group_start != nullptr, "null group_start");
        PSA_REQUIRE(group_start[0] == 0, "group_start[0] must be 0, got %lld", (long long)group_start[0]);
        for (int g = 0; g < n_groups; ++g)
            PSA_REQUIRE(group_start[g + 1] >= group_start[g], "group_start must be ascending (group %d)", g);
        PSA_REQUIRE(group_start[n_groups] < (1ll << 31), "too many atoms (%lld)", (long long)group_start[n_groups]);
        std::vector<uint8_t> seen((size_t)p->N, 0);
        for (int g = 0; g < n_groups; ++g)
            for (int64_t i = group_start[g]; i < group_start[g + 1]; ++i) {
                PSA_REQUIRE(idx[i] >= 0 && idx[i] < p->N, "Atom indices in basis out of bounds.");
                PSA_REQUIRE(!seen[(size_t)idx[i]], "atom %d is listed twice (group %d): the groups must be disjoint", (int)idx[i], g);
                seen[(size_t)idx[i]] = 1;
            }
        p->listed = true;
        p->start.assign(group_start, group_start + n_groups + 1);
    }
    p->n_a = p->start[(size_t)n_groups];
    for (int g = 0; g < n_groups; ++g) p->size.push_back(p->start[(size_t)g + 1] - p->start[(size_t)g]);
    return PSA_OK;
}

int served_radius_check(const double* inv, const char* what, double r) {
    double width = INFINITY;
    for (int j = 0; j < 3; ++j) width = std::min(width, 1.0 / std::sqrt(inv[j] * inv[j] + inv[3 + j] * inv[3 + j] + inv[6 + j] * inv[6 + j]));
    const double served = (0.5 - 0x1p-12) * width;
    PSA_REQUIRE(r <= served * (1.0 + 0x1p-40), "%s = %.17g is beyond the served radius %.17g: (1/2 - 2^-12) of the box's least "
                "perpendicular width", what, r, served);
    return PSA_OK;
}

int histogram_args_check(const AtomGroups& p, const int64_t* lags, int64_t n_lags, int max_lags, int64_t origin_step, double dr, int32_t n_r,
                         int max_bins, float* inv_dr) {
    PSA_REQUIRE(n_lags >= 1 && n_lags <= max_lags, "the number of lags is in [1, %d], got %lld", max_lags, (long long)n_lags);
    for (int64_t j = 0; j < n_lags; ++j)
        PSA_REQUIRE(lags[j] >= 0 && lags[j] <= p.T - 1, "lag %lld is outside [0, T - 1 = %lld]", (long long)lags[j], (long long)(p.T - 1));
    PSA_REQUIRE(origin_step >= 1, "origin_step must be at least 1, got %lld", (long long)origin_step);
    PSA_REQUIRE(std::isfinite(dr) && dr > 0.0, "the bin width must be positive and finite, got %g", dr);
    *inv_dr = (float)(1.0 / dr);
    PSA_REQUIRE(std::isfinite(*inv_dr) && *inv_dr > 0.f, "the bin width %g has no float32 reciprocal", dr);
    PSA_REQUIRE(n_r >= 1 && n_r <= max_bins, "the number of bins is in [1, %d], got %d", max_bins, (int)n_r);
    return PSA_OK;
}

int upload_atom_list(psa_ctx* c, AtomGroups* p, const int32_t* idx) {
    if (!p->listed) return PSA_OK;
    StageTimer st(c, PSA_T_H2D);
    PSA_TRY(upload(c, c->d_rs_idx, idx, (size_t)p->n_a * sizeof(int32_t)));
    p->d_idx = c->d_rs_idx.as<int>();
    return PSA_OK;
}

int rows_of_groups(const int32_t* first, int n, int64_t per, HistRows* rows) {
    PSA_REQUIRE(n >= 1 && n <= HIST_REDUCE_MAX_ROWS && per >= 1 && first[n] * per < (1ll << 31), "too many partial rows (%lld x %lld)",
                (long long)first[n], (long long)per);
    for (int g = 0; g < n; ++g) rows->lo[g] = (int)(first[g] * per), rows->hi[g] = (int)(first[g + 1] * per), rows->factor[g] = 1;
    return PSA_OK;
}

}  // namespace psa
