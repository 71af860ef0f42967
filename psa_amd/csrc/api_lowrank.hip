// Low-rank route for k-paths: the host plan (the device half is k1_planes_diff.hip).
//
// All vectors of a k-path lie on one line, k_j = k0 + kappa_j u.  With x_a = u.r_a,
//     exp(i k_j.r_a) = exp(i kappa_j x_c) * sum_l L_l(kappa_j) W[l, a],   W[l, a] = exp(i k0.r_a) exp(i kappa_l (x_a - x_c)),
// where kappa_l are 64 Chebyshev nodes of an interval of kappa and L_l their Lagrange polynomials: Chebyshev
// interpolation of exp(i kappa (x - x_c)) over an interval of half-width h_k, |x - x_c| <= h_x, is exact to fp64
// rounding with 64 nodes while h_k h_x <= 30.  C[j, l] = exp(i kappa_j x_c) L_l(kappa_j); the plan also carries its
// two factors on their own, L[j, l] = L_l(kappa_j) (real) and phi[j] = exp(i kappa_j x_c), for the combine that
// sums the nodes with real weights and applies the phase once per output element (lowrank_combine_r_kernel).
// What the line does not carry goes to D = P_ref - exp(i k~_j.r) (k~_j: k_j projected on the line), bounded by
//     |D| <= 2^-22 sum_i max|k_i| max|r_i|   (float32 rounding of the reference's phase argument)
//          + max_j |k_j - k~_j| max_a |r_a|  (the vectors off the line)
//          + 2^-20                           (sincosf against fp64 sincos)
// and accepted when the bound is at most 2^-13: D times the hi plane alone then misses at most 2^-25 of |v| per term.
//
// The plan is ROW-DETERMINISTIC for the lists it serves: u, k0, the node interval and hence the nodes and each row
// of C, L and phi depend on the line and the atom group, not on which part of the path a launch holds, so a list split over
// calls projects every row with the same arithmetic.  That needs a line the float32 k-vectors determine EXACTLY:
// any quantity estimated from them carries their rounding (~1e-7 relative) and lands on different grid points for
// different sub-lists.  So the route serves lines through Gamma (k0 = 0) along a small-integer (lattice) direction
// such as [110] -- u is then snapped exactly and kappa_j = k_j.u is a function of k_j alone -- and lists that lie
// on one side of Gamma: node intervals tile kappa >= 0 as [n w, (n+1) w) and kappa <= 0 as (-(n+1) w, -n w], with
// a width w fixed by the group's x-range, and every kappa of a launch must fall in one of them.  Everything else
// (paths off Gamma, non-lattice directions, lists crossing Gamma or longer than one interval) stays on the dense
// kernels.  A list that crosses Gamma declines as a whole while a part of it on one side may take the route, so
// for such lists splitting can move rows by the ~1e-7 that separates the two routes.
#include "api_internal.h"
#include "k1_lowrank_fold.h"
#include "k1_lowrank_n48.h"
#include "k1_lowrank_pair.h"

namespace psa {

namespace {
constexpr double LR_OMEGA = 30.0;                 // half-width product h_k h_x of a node interval
constexpr double LR_D_MAX = 1.0 / 8192.0;         // 2^-13
// Cap on the 48-node plan's r_bound (plan_lowrank).  The largest residual of 48-node interpolation over a whole node interval
// is a function of LR_OMEGA and the node count alone: 4.6e-7 at 30 and 48 (1.0e-3 with 40 nodes, 2.7e-5 with 44), plus the
// float32 rounding of phi and L, at most (1 + 3.5) 2^-24 = 2.7e-7.  No launch checks it -- tests/test_lowrank_n48_host.py
// holds every r_bound to it --, so a change of LR_OMEGA or of the node count has to work this number out again.
constexpr double LR48_R_MAX = 1e-6;
static_assert(LR_OMEGA == 30.0 && LOWRANK_NODES_48 == 48, "LR48_R_MAX was worked out for 48 nodes on h_k h_x = 30");
}  // namespace

int plan_lowrank(const float* k, int64_t K, const float* mean_all, int64_t N, const int32_t* h_idx, int64_t n_g, LowRankPlan* p,
                 float* C, int nodes, bool want_r) {
    *p = LowRankPlan{};
    PSA_REQUIRE(nodes == LOWRANK_NODES || nodes == LOWRANK_NODES_48, "the plan has 48 or 64 nodes");
    p->nodes = nodes;
    auto fail = [&](const char* why) {
        p->why = why;
        return PSA_OK;
    };
    if (K < 2) return fail("fewer than two k-vectors");
    if (n_g < 1) return fail("empty group");
    for (int64_t i = 0; i < 3 * K; ++i)
        if (!std::isfinite(k[i])) return fail("k-vector not finite");
    // ---- direction: the vector farthest from the first one
    double  p0[3] = {k[0], k[1], k[2]}, far = 0.0;
    int64_t jf = 0;
    for (int64_t j = 1; j < K; ++j) {
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) d2 += ((double)k[3 * j + i] - p0[i]) * ((double)k[3 * j + i] - p0[i]);
        if (d2 > far) {
            far = d2;
            jf = j;
        }
    }
    if (!(far > 0.0)) return fail("all k-vectors equal");
    double u[3], nu = std::sqrt(far);
    for (int i = 0; i < 3; ++i) u[i] = ((double)k[3 * jf + i] - p0[i]) / nu;
    {   // canonical sign: the largest component positive
        int im = 0;
        for (int i = 1; i < 3; ++i)
            if (std::fabs(u[i]) > std::fabs(u[im])) im = i;
        if (u[im] < 0)
            for (double& v : u) v = -v;
    }
    bool snapped = false;          // (a direction that is not within 1e-6 of a small-integer one is declined below)
    for (int n = 1; n <= 12 && !snapped; ++n) {    // small-integer direction: u = m / |m| with |m_i| <= n
        double m[3], mn = 0.0, dev = 0.0;
        const double s = n / std::max({std::fabs(u[0]), std::fabs(u[1]), std::fabs(u[2])});
        for (int i = 0; i < 3; ++i) {
            m[i] = std::nearbyint(u[i] * s);
            mn += m[i] * m[i];
        }
        mn = std::sqrt(mn);
        for (int i = 0; i < 3; ++i) dev = std::max(dev, std::fabs(m[i] / mn - u[i]));
        if (dev < 1e-6) {
            for (int i = 0; i < 3; ++i) u[i] = m[i] / mn + 0.0;
            snapped = true;
        }
    }
    if (!snapped) return fail("direction not a lattice direction");
    // ---- the line must pass through Gamma: then k0 = 0 exactly.  The distance of the line from Gamma is
    // estimated from the point of the list farthest from it (float32 rounding: ~1e-7 of |k|)
    {
        double kmax2 = 0.0, off2 = 0.0;
        for (int64_t j = 0; j < K; ++j) {
            double kj[3], d = 0.0, n2 = 0.0;
            for (int i = 0; i < 3; ++i) {
                kj[i] = k[3 * j + i];
                d += kj[i] * u[i];
                n2 += kj[i] * kj[i];
            }
            double o2 = 0.0;
            for (int i = 0; i < 3; ++i) o2 += (kj[i] - d * u[i]) * (kj[i] - d * u[i]);
            kmax2 = std::max(kmax2, n2);
            off2 = std::max(off2, o2);
        }
        if (!(std::sqrt(off2) <= 1e-5 * std::sqrt(kmax2))) return fail("line does not pass through Gamma");
    }
    for (int i = 0; i < 3; ++i) p->u[i] = u[i];
    // ---- the group's atoms along u
    double xmin = INFINITY, xmax = -INFINITY, rmax = 0.0, rabs[3] = {0, 0, 0};
    for (int64_t a = 0; a < n_g; ++a) {
        const int64_t src = h_idx ? h_idx[a] : a;
        if (src < 0 || src >= N) return fail("index outside the trajectory");
        const float* r = mean_all + 3 * src;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2])) return fail("mean position not finite");
        const double x = u[0] * r[0] + u[1] * r[1] + u[2] * r[2];
        xmin = std::min(xmin, x);
        xmax = std::max(xmax, x);
        rmax = std::max(rmax, std::sqrt((double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2]));
        for (int i = 0; i < 3; ++i) rabs[i] = std::max(rabs[i], (double)std::fabs(r[i]));
    }
    p->x_c = 0.5 * (xmin + xmax);
    p->h_x = std::max(0.5 * (xmax - xmin), 1e-12);
    p->width = 2.0 * LR_OMEGA / p->h_x;
    // ---- kappa, the line's vectors, the off-line residual
    p->kline.resize((size_t)3 * K);
    std::vector<double> kap((size_t)K);
    double              off = 0.0, kabs[3] = {0, 0, 0};
    for (int64_t j = 0; j < K; ++j) {
        double kj[3], kk = 0.0;
        for (int i = 0; i < 3; ++i) {
            kj[i] = k[3 * j + i];
            kk += (kj[i] - p->k0[i]) * u[i];
            kabs[i] = std::max(kabs[i], std::fabs(kj[i]));
        }
        kap[(size_t)j] = kk;
        double e2 = 0.0;
        for (int i = 0; i < 3; ++i) {
            p->kline[3 * j + i] = p->k0[i] + kk * u[i];
            e2 += (kj[i] - p->kline[3 * j + i]) * (kj[i] - p->kline[3 * j + i]);
        }
        off = std::max(off, std::sqrt(e2));
    }
    p->d_bound = 0x1p-22 * (kabs[0] * rabs[0] + kabs[1] * rabs[1] + kabs[2] * rabs[2]) + off * rmax + 0x1p-20;
    if (!(p->d_bound <= LR_D_MAX)) return fail("k-vectors not on one line (or phases too large)");
    // ---- one node interval holds every kappa: [n w, (n + 1) w] on the side kappa >= 0, [-(n + 1) w, -n w] on the
    // other (kappa = 0, Gamma itself, belongs to interval 0 of either side)
    bool pos = true, neg = true;
    for (int64_t j = 0; j < K; ++j) {
        pos = pos && kap[(size_t)j] >= 0.0;
        neg = neg && kap[(size_t)j] <= 0.0;
    }
    if (!pos && !neg) return fail("k-list crosses Gamma");
    const bool   side = pos;                                              // all kappa >= 0 (both only if all are 0)
    const double n0 = std::floor(std::fabs(kap[0]) / p->width);
    for (int64_t j = 0; j < K; ++j)
        if (std::floor(std::fabs(kap[(size_t)j]) / p->width) != n0) return fail("k-path longer than one node interval");
    p->interval = side ? (int64_t)n0 : -(int64_t)n0 - 1;
    const double mid = (p->interval + 0.5) * p->width, half = 0.5 * p->width;
    double       bw[LOWRANK_NODES];                               // (the first `nodes` entries)
    for (int l = 0; l < nodes; ++l) {
        const double th = M_PI * (2 * l + 1) / (2.0 * nodes);
        p->kappa[l] = mid + half * std::cos(th);
        bw[l] = ((l & 1) ? -1.0 : 1.0) * std::sin(th);           // barycentric weights of Chebyshev points of the first kind
    }
    // ---- L[j, l] and phi[j], each rounded from fp64 on its own; for a caller that asks, C[j, l] = exp(i kappa_j x_c)
    // L_l(kappa_j), complex64, their product rounded once
    p->L.assign((size_t)K * nodes, 0.f);
    p->phi.assign((size_t)K * 2, 0.f);
    for (int64_t j = 0; j < K; ++j) {
        const double kj = kap[(size_t)j];
        double       L[LOWRANK_NODES], den = 0.0;                     // (the first `nodes` entries)
        int          hit = -1;
        for (int l = 0; l < nodes; ++l)
            if (kj == p->kappa[l]) hit = l;
        if (hit >= 0) {
            for (int l = 0; l < nodes; ++l) L[l] = l == hit;
        } else {
            for (int l = 0; l < nodes; ++l) {
                L[l] = bw[l] / (kj - p->kappa[l]);
                den += L[l];
            }
            for (int l = 0; l < nodes; ++l) L[l] /= den;
        }
        const double cr = std::cos(kj * p->x_c), ci = std::sin(kj * p->x_c);
        p->phi[(size_t)j * 2 + 0] = (float)cr;
        p->phi[(size_t)j * 2 + 1] = (float)ci;
        for (int l = 0; l < nodes; ++l) {
            p->L[(size_t)j * nodes + l] = (float)L[l];
            if (C) {
                C[((size_t)j * nodes + l) * 2 + 0] = (float)(cr * L[l]);
                C[((size_t)j * nodes + l) * 2 + 1] = (float)(ci * L[l]);
            }
        }
    }
    // ---- scale of D: the bound lands at or below 2^14 (float16 maximum 65504)
    p->dscale = std::ldexp(1.0f, 14 - (int)std::ceil(std::log2(p->d_bound)));
    // ---- the folded image D + E (psa_set_k1_lowrank_fold): E[j, a] = phi_j sum_l L[j, l] W_lo[l, a], |W_lo| <= 2^-12 per
    // part (the residual of a float16 piece of a value <= 1), so a part of E is at most rot_j Lam_j 2^-12 with
    // rot_j = |Re phi_j| + |Im phi_j|, Lam_j = sum_l |L[j, l]| of the float32 tables the device reads
    for (int64_t j = 0; j < K; ++j) {
        double lam = 0.0;
        for (int l = 0; l < nodes; ++l) lam += std::fabs((double)p->L[(size_t)j * nodes + l]);
        const double rot = std::fabs((double)p->phi[(size_t)j * 2]) + std::fabs((double)p->phi[(size_t)j * 2 + 1]);
        p->e_bound = std::max(p->e_bound, rot * lam * 0x1p-12);
    }
    p->dscale_fold = std::ldexp(1.0f, 14 - (int)std::ceil(std::log2(p->d_bound + p->e_bound)));
    // ---- 48 nodes: the image also holds the interpolation residual R = P_line - phi L W.  |R| depends on (kappa - mid) h_x
    // and (x - x_c) / h_x alone, so its largest value over a whole node interval is one number for every plan: 4.6e-7
    // at h_k h_x = 30, plus the float32 rounding of phi and L, (1 + Lam) 2^-24 <= 2.7e-7.  A launch scales the image
    // by the cap LR48_R_MAX = 1e-6 on that; r_bound itself, the largest |R| over the launch's rows and the group's atoms,
    // costs K x n_g x 48 complex products on the host and is worked out for psa_lowrank_plan_nodes alone.
    if (nodes == LOWRANK_NODES_48) {
        p->dscale_fold = std::ldexp(1.0f, 14 - (int)std::ceil(std::log2(p->d_bound + p->e_bound + LR48_R_MAX)));
        if (want_r) {
            std::vector<double> wr((size_t)nodes), wi((size_t)nodes);
            for (int64_t a = 0; a < n_g; ++a) {
                const float* r = mean_all + 3 * (h_idx ? h_idx[a] : a);
                const double y = (u[0] * r[0] + u[1] * r[1] + u[2] * r[2]) - p->x_c;
                const double t0 = p->k0[0] * r[0] + p->k0[1] * r[1] + p->k0[2] * r[2];
                for (int l = 0; l < nodes; ++l) {
                    wr[(size_t)l] = std::cos(t0 + p->kappa[l] * y);
                    wi[(size_t)l] = std::sin(t0 + p->kappa[l] * y);
                }
                for (int64_t j = 0; j < K; ++j) {
                    double sr = 0.0, si = 0.0;
                    for (int l = 0; l < nodes; ++l) {
                        sr += (double)p->L[(size_t)j * nodes + l] * wr[(size_t)l];
                        si += (double)p->L[(size_t)j * nodes + l] * wi[(size_t)l];
                    }
                    const double pr = p->phi[(size_t)j * 2], pi = p->phi[(size_t)j * 2 + 1];
                    const double th = p->kline[3 * j] * r[0] + p->kline[3 * j + 1] * r[1] + p->kline[3 * j + 2] * r[2];
                    p->r_bound = std::max(p->r_bound, std::hypot(std::cos(th) - (pr * sr - pi * si), std::sin(th) - (pr * si + pi * sr)));
                }
            }
        }
    }
    p->ok = true;
    return PSA_OK;
}

// Decide the route of one projection launch (a group's planes, nk k-vectors from k_first of the list) and, when the
// low-rank route serves, upload what it needs: fp64 [k0 (3), u (3), x_c, kappa (64 or 48), with 64 nodes kline (nk x 3)] and the
// combine's weights L and phases phi.
// The decision depends on the list, the group and the options only -- never on how the list is split over
// calls -- as long as every part keeps PSA_OPT_K1_LOWRANK_MIN_LOCAL vectors (default 128: a 512-row D block at
// least half full).
int prepare_lowrank(psa_ctx* c, const GroupView& v, const ProjectArgs& list, int64_t k_first, int64_t nk, ProjGeom* g) {
    g->lowrank = false;
    if (!c->opt_k1_lowrank || g->split != K1Family::f16_planes || !v.ps || list.K_total < c->opt_k1_lowrank_min_k ||
        nk < c->opt_k1_lowrank_min_local)
        return PSA_OK;
    // 48 nodes only while the fold is on: with it off the route is the 64-node route on its own kernels
    const int   nodes = c->k1_lowrank_fold && c->k1_lowrank_nodes == LOWRANK_NODES_48 ? LOWRANK_NODES_48 : LOWRANK_NODES;
    LowRankPlan p;
    PSA_TRY(plan_lowrank(list.k_vectors + 3 * k_first, nk, list.mean_pos_all, c->slot[v.slot].N, v.h_idx, g->n_g, &p, nullptr, nodes));
    if (!p.ok) return PSA_OK;
    // (kline feeds the 64-node tables' P_line; the 48-node image is built from the node table and needs none)
    const bool          kline = nodes == LOWRANK_NODES;
    std::vector<double> f64((size_t)7 + nodes + (kline ? 3 * (size_t)nk : 0));
    std::memcpy(f64.data(), p.k0, 3 * sizeof(double));
    std::memcpy(f64.data() + 3, p.u, 3 * sizeof(double));
    f64[6] = p.x_c;
    std::memcpy(f64.data() + 7, p.kappa, (size_t)nodes * sizeof(double));
    if (kline) std::memcpy(f64.data() + 7 + nodes, p.kline.data(), p.kline.size() * sizeof(double));
    PSA_TRY(upload(c, c->d_lr_f64, f64.data(), f64.size() * sizeof(double)));
    PSA_TRY(upload(c, c->d_lr_L, p.L.data(), p.L.size() * sizeof(float)));
    PSA_TRY(upload(c, c->d_lr_phi, p.phi.data(), p.phi.size() * sizeof(float)));
    PSA_TRY(c->d_lr_qn.reserve((size_t)nodes * 3 * (size_t)c->slot[v.slot].T * sizeof(float2)));
    g->lowrank = true;
    g->lr_nodes = nodes;
    g->lr_fold = c->k1_lowrank_fold;                                   // D' = D + E in the image, two products per node row
    g->dscale = g->lr_fold ? p.dscale_fold : p.dscale;
    g->M_pad_d = (int)((2 * nk + 511) / 512 * 512);
    g->lr_pair = c->opt_k1_lowrank_pair && g->M_pad_d == LRP_ROWS;     // one D block: node rows and D rows in one launch
    static_assert(LRF_ROWS == LRP_ROWS && LRN_ROWS == LRP_ROWS, "the folded pair launches serve the lists the pair launch serves");
    return PSA_OK;
}

}  // namespace psa

using namespace psa;

extern "C" {

int psa_lowrank_plan(const float* k_vectors, int64_t K, const float* mean_pos_all, int64_t N, const int32_t* idx, int64_t n_g,
                     int32_t* ok, double* geo, double* kappa, float* C, float* L, float* phi) {
    PSA_REQUIRE(K >= 0 && K < (1ll << 29) && N >= 1 && n_g >= 0 && n_g <= (idx ? (int64_t)1 << 30 : N) && ok && geo &&
                    (K == 0 || k_vectors) && mean_pos_all,
                "bad argument");
    LowRankPlan p;
    PSA_TRY(plan_lowrank(k_vectors, K, mean_pos_all, N, idx, n_g, &p, C));
    *ok = p.ok;
    const double g[14] = {p.u[0],  p.u[1],    p.u[2],           p.k0[0],   p.k0[1],  p.k0[2],   p.x_c,
                          p.h_x,   p.width,   (double)p.interval, p.d_bound, p.dscale, p.e_bound, p.dscale_fold};
    std::memcpy(geo, g, sizeof(g));
    if (p.ok && kappa) std::memcpy(kappa, p.kappa, sizeof(p.kappa));
    if (p.ok && L) std::memcpy(L, p.L.data(), p.L.size() * sizeof(float));
    if (p.ok && phi) std::memcpy(phi, p.phi.data(), p.phi.size() * sizeof(float));
    return PSA_OK;
}

int psa_lowrank_plan_nodes(const float* k_vectors, int64_t K, const float* mean_pos_all, int64_t N, const int32_t* idx, int64_t n_g,
                           int32_t nodes, int32_t* ok, double* geo, double* kappa, float* C, float* L, float* phi) {
    PSA_REQUIRE(K >= 0 && K < (1ll << 29) && N >= 1 && n_g >= 0 && n_g <= (idx ? (int64_t)1 << 30 : N) && ok && geo &&
                    (K == 0 || k_vectors) && mean_pos_all && (nodes == LOWRANK_NODES || nodes == LOWRANK_NODES_48),
                "bad argument");
    LowRankPlan p;
    PSA_TRY(plan_lowrank(k_vectors, K, mean_pos_all, N, idx, n_g, &p, C, nodes, true));
    *ok = p.ok;
    const double g[15] = {p.u[0],  p.u[1],  p.u[2],  p.k0[0], p.k0[1], p.k0[2], p.x_c, p.h_x, p.width, (double)p.interval,
                          p.d_bound, p.dscale, p.e_bound, p.dscale_fold, p.r_bound};
    std::memcpy(geo, g, sizeof(g));
    if (p.ok && kappa) std::memcpy(kappa, p.kappa, (size_t)nodes * sizeof(double));
    if (p.ok && L) std::memcpy(L, p.L.data(), p.L.size() * sizeof(float));
    if (p.ok && phi) std::memcpy(phi, p.phi.data(), p.phi.size() * sizeof(float));
    return PSA_OK;
}

int psa_lowrank_n48_image(int32_t n_stage, int64_t* index, int64_t* bytes) {
    PSA_REQUIRE(n_stage >= 1 && n_stage < (1 << 20) && bytes, "bad argument");
    *bytes = (int64_t)pd16_n48_table_bytes(n_stage);
    if (index)
        for (int m = 0; m < LRN_ROWS; ++m)
            for (int a = 0; a < n_stage * K1_BA; ++a) index[(size_t)m * n_stage * K1_BA + a] = (int64_t)pd16_n48_index(m, a, n_stage);
    return PSA_OK;
}

int psa_lowrank_pair_image(int32_t n_stage, int64_t* index, int64_t* bytes) {
    PSA_REQUIRE(n_stage >= 1 && n_stage < (1 << 20) && bytes, "bad argument");
    *bytes = (int64_t)pd16_pair_table_bytes(n_stage);
    if (index)
        for (int m = 0; m < LRP_ROWS; ++m)
            for (int a = 0; a < n_stage * K1_BA; ++a) index[(size_t)m * n_stage * K1_BA + a] = (int64_t)pd16_pair_index(m, a, n_stage);
    return PSA_OK;
}

int psa_lowrank_fold_image(int32_t n_stage, int64_t* index, int64_t* bytes) {
    PSA_REQUIRE(n_stage >= 1 && n_stage < (1 << 20) && bytes, "bad argument");
    *bytes = (int64_t)pd16_fold_table_bytes(n_stage);
    if (index)
        for (int m = 0; m < LRF_ROWS; ++m)
            for (int a = 0; a < n_stage * K1_BA; ++a) index[(size_t)m * n_stage * K1_BA + a] = (int64_t)pd16_fold_index(m, a, n_stage);
    return PSA_OK;
}

}  // extern "C"
