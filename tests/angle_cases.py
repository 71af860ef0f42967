"""Input families of the bond-angle tests, the allowance of the histograms derived from the arithmetic stated at
psa_angle_histogram in include/psa_hip.h and from nothing in the code, and a NumPy twin of that arithmetic with the planted
faults the host test holds outside the allowance.

The allowance, u = 2^-24.  A leg is the pair chain of pair_cases.py with dr = r_cut: x = |d| / r_cut carries at most
`pair_cases.tolerance`, and d carries |delta d|_2 with |delta d_c| <= sum_j (u + E64 + 3 u |e_j|) |H_jc|.  A reference
neighbour pair is LEG-BORDERLINE when |x - 1| <= that tolerance.  The cosine of the legs b, c: its derivative along d_b is
sin(theta) / r_b at most, so the legs' errors move it by (|delta d_b| / r_b + |delta d_c| / r_c) (1 + 2^-10) (the factor
covers the second order, |delta d| / r of 1e-6); the float32 chain adds
    dot: three roundings of partial sums below r_b r_c                          3 u
    r2 (three roundings each, all terms positive), their product                7 u, halved by the root: 3.5 u
    the root, the quotient                                                      2 u
of |cos| <= 1, 8.5 u together, and the table's edge is rounded once, 2^-24 allowed for it:
    tol_c = (|delta d_b| / r_b + |delta d_c| / r_c) (1 + 2^-10) + 9.5 u
A reference triplet is BORDERLINE when cos - tol_c and cos + tol_c fall into different bins (by arccos, float64); a bin may
differ from the reference by the borderline triplets that can reach it.  A leg-borderline neighbour widens the allowance
of every bin its triplets can reach and of the coordination entries its centre can move between; a centre whose count
can cross the capacity, of everything it contributes and of `truncated`.  The identities among the totals hold exactly."""
import numpy as np

import angle64 as A
import pair64 as R
import pair_cases as P
from lattice_cases import CUBIC, TRICLINIC  # noqa: F401

U32 = 2.0 ** -24
CAPACITY = A.CAPACITY
BOXES = {"cubic": CUBIC, "triclinic": TRICLINIC}


def cap(n_theta):
    assert n_theta <= 256 or n_theta == 1024
    return 1e-2 if n_theta == 1024 else 2e-3


# ---- input families -----------------------------------------------------------------------------------------------------
# name: (box, atoms, frames, r_cut): random walks of 0.05 box per frame
FAMILIES = {"cubic130": ("cubic", 130, 12, 6.0), "triclinic130": ("triclinic", 130, 12, 6.0), "cubic37": ("cubic", 37, 40, 8.0),
            "triclinic257": ("triclinic", 257, 4, 5.0)}


def family(name, seed=11):
    """(positions (T, N, 3) float32, box, r_cut)"""
    box, n, t, rc = FAMILIES[name]
    return P.walk(n, t, seed, box=BOXES[box])["wrapped"], BOXES[box], rc


def two_species(n_atoms):
    """the last 40 atoms (of few: the last third) and the rest"""
    cut = n_atoms - (40 if n_atoms > 100 else n_atoms // 3)
    return [np.arange(0, cut), np.arange(cut, n_atoms)]


def three_species(n_atoms, seed=3):
    """an empty species between two shuffled ones; the last two atoms of the shuffle are in none"""
    order = np.random.default_rng(seed).permutation(n_atoms)
    return [order[: n_atoms // 3], np.zeros(0, np.int64), order[n_atoms // 3: max(n_atoms - 2, n_atoms // 3)]]


def matrix_cutoff(r_cut, n_species):
    """a symmetric matrix with a zero entry (the last species does not bond to itself) and two different cut-offs"""
    rc = np.full((n_species, n_species), float(r_cut))
    rc[0, 0] = 0.8 * r_cut
    rc[-1, -1] = 0.0 if n_species > 1 else rc[-1, -1]
    return rc


def ball(n_inside, n_frames, r_cut, box=CUBIC, seed=5, n_outside=0):
    """`n_inside` atoms in a ball of radius r_cut / 2 (every one a neighbour of every other), `n_outside` far from it and
    from each other's cut-off spheres' overlap: frozen"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_inside, 3))
    v *= (0.5 * r_cut * rng.uniform(0.0, 1.0, (n_inside, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    H = np.asarray(box, np.float32).astype(np.float64)
    centre = np.array([0.3, 0.4, 0.5]) @ H
    far = (np.array([0.8, 0.9, 0.1]) @ H)[None] + 0.05 * rng.standard_normal((n_outside, 3))
    pos = np.concatenate([centre[None] + v, far]).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(pos, (n_frames,) + pos.shape))


def sphere(n_on, r, box=CUBIC, seed=6):
    """one frame: a centre and `n_on` atoms on a sphere of radius r around it (a Fibonacci spiral)"""
    i = np.arange(n_on) + 0.5
    z, phi = 1.0 - 2.0 * i / n_on, np.pi * (1.0 + 5.0 ** 0.5) * i
    v = r * np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    H = np.asarray(box, np.float32).astype(np.float64)
    centre = np.array([0.5, 0.5, 0.5]) @ H
    return np.concatenate([centre[None], centre[None] + v]).astype(np.float32)[None]


def diamond(n_frames):
    """512 atoms of the diamond lattice, a = 21.72 / 4, in the cubic box of 21.72, frozen: (positions, the two
    zincblende sublattices as species)"""
    a = float(np.float32(21.72)) / 4.0
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    cell = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 1, 3)
    first = (cell + fcc[None]).reshape(-1, 3) * a
    pos = np.concatenate([first, first + 0.25 * a]).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(pos, (n_frames, 512, 3))), [np.arange(256), np.arange(256, 512)]


def walk_case():
    """(positions (5, 70, 3) float32, box, the species of 67 and 3 atoms, r_cut): five frames that reach every branch of the
    centre walk the passes over the neighbour lists share -- items of 64, 3 and 3 centres (the last wavefront of a short item
    has no centre at all); centres with 0, 1, 2 (one round, counted once), an odd number, exactly 64 and 65 neighbours (atom 0
    in its sphere, one atom of which leaves in the frames 1, 2 and 4); a coincident pair (67, 68), with a third atom in reach
    (a leg of length 0 among two) and without (one leg).  `walk_counts` names the counts the frames hold"""
    H = CUBIC.astype(np.float64)
    centre = np.array([0.3, 0.3, 0.3]) @ H
    ring = sphere(65, 3.0)[0, 1:].astype(np.float64) - sphere(65, 3.0)[0, 0].astype(np.float64)
    rng = np.random.default_rng(21)
    away = [np.array(f) @ H for f in ([0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.8, 0.8, 0.2], [0.8, 0.8, 0.8])]   # 10 apart and more
    frames = []
    for f in range(5):
        shell = centre[None] + ring + (0.0 if f == 0 else 0.02 * rng.standard_normal(ring.shape))
        if f in (1, 2, 4):
            shell[64] = away[0]                                               # 64 neighbours are left
        pair = away[2] + (0.0 if f == 0 else 0.1 * f)
        third = away[3] if f in (1, 2) else pair + np.array([1.0, 0.5, -0.25])
        second = pair + np.array([0.0, 0.75, 0.0]) if f == 3 else pair    # frame 3: no two atoms at one place
        frames.append(np.concatenate([centre[None], shell, away[1][None], pair[None], second[None], third[None]]))
    return np.asarray(frames, np.float32), CUBIC, [np.arange(67), np.arange(67, 70)], 3.5


def walk_counts(n):
    """does `n` (5, 70), the true neighbour counts of `walk_case`, hold what its docstring names?"""
    n = np.asarray(n)
    odd = (n[:, 1:66] % 2 == 1) & (n[:, 1:66] > 2)
    return (n[[0, 3], 0].tolist() == [65, 65] and n[[1, 2, 4], 0].tolist() == [64, 64, 64] and np.all(n[:, 66] == 0) and odd.any()
            and np.all(n[[1, 2, 4], 65] == 0) and np.all(n[[1, 2], 67:69] == 1) and np.all(n[[1, 2], 69] == 0)
            and np.all(n[[0, 3, 4], 67:70] == 2))


# ---- the allowance ------------------------------------------------------------------------------------------------------
def reference(positions, box, groups, r_cut, step, n_theta):
    """one pass of the brute force: dict of the reference counts `angles` (S, P, n_theta + 1), `coord` (S, S, 65),
    `truncated` (S,), the allowances `angles_allowed`, `coord_allowed`, `truncated_allowed` of the same shapes, the numbers
    of `triplets`, of `borderline` triplets and of `leg_borderline` neighbour pairs, `most` the most neighbours of a
    centre, `lists` per origin the per-centre (sure neighbours, leg-borderline ones), and `cross` (S, P) the sum over the
    centres that are not truncated of n_beta n_gamma (beta < gamma; n (n - 1) / 2 on the diagonal)"""
    S = len(groups)
    n_p = S * (S + 1) // 2
    rc = A.cutoffs(r_cut, S)
    atoms, spec = A.species_of(groups)
    n = atoms.size
    out = dict(angles=np.zeros((S, n_p, n_theta + 1), np.int64), coord=np.zeros((S, S, CAPACITY + 1), np.int64),
               truncated=np.zeros(S, np.int64), triplets=0, borderline=0, leg_borderline=0, most=0, lists=[],
               cross=np.zeros((S, n_p), np.int64))
    out["angles_allowed"], out["coord_allowed"], out["truncated_allowed"] = (np.zeros_like(out[k]) for k in ("angles", "coord", "truncated"))
    if n == 0:
        out["lists"] = [[] for _ in range(0, np.shape(positions)[0], step)]
        return out
    e64 = P.sigma_error(positions, box)
    aH = np.abs(R.box64(box)[0])
    cut = rc[spec[:, None], spec[None, :]]
    off = ~np.eye(n, dtype=bool)
    for o in range(0, np.shape(positions)[0], step):
        e, d, r = A.frame_pairs(positions[o], box, atoms)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(cut > 0.0, r / cut, np.inf)
            tol = np.where(cut > 0.0, P.tolerance(e.reshape(-1, 3), d.reshape(-1, 3), r.ravel(), box, np.where(cut > 0.0, cut, 1.0).ravel(),
                                                  e64).reshape(n, n), 0.0)
        dd = (U32 + e64 + 3.0 * U32 * np.abs(e)) @ aH
        dd = np.sqrt((dd * dd).sum(axis=2))                                  # |delta d|_2 of every leg
        edge = (np.abs(x - 1.0) <= tol) & off
        sure = (x < 1.0) & off & ~edge
        is_nb = (r < cut) & off
        frame_lists = []
        for a in range(n):
            al = spec[a]
            s_nb, b_nb, nb = np.flatnonzero(sure[a]), np.flatnonzero(edge[a]), np.flatnonzero(is_nb[a])
            frame_lists.append((s_nb, b_nb))
            out["leg_borderline"] += b_nb.size
            out["most"] = max(out["most"], nb.size)
            crossing = s_nb.size <= CAPACITY < s_nb.size + b_nb.size
            if crossing:
                out["truncated_allowed"][al] += 1
            # the reference's own contribution
            if nb.size > CAPACITY:
                out["truncated"][al] += 1
            else:
                for be in range(S):
                    out["coord"][al, be, int((spec[nb] == be).sum())] += 1
            # everything the centre could contribute: all pairs among the sure and the leg-borderline neighbours
            every = np.concatenate([s_nb, b_nb])
            if s_nb.size > CAPACITY:
                continue                                                   # truncated whatever the rounding
            for be in range(S):
                lo_n, k = int((spec[s_nb] == be).sum()), int((spec[b_nb] == be).sum())
                if k or crossing:
                    out["coord_allowed"][al, be, lo_n:min(lo_n + k, CAPACITY) + 1] += 1
            j, k = np.triu_indices(every.size, 1)
            if j.size == 0:
                continue
            bj, bk = every[j], every[k]
            rb, rk = r[a, bj], r[a, bk]
            zero = (rb == 0.0) | (rk == 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                cos = np.where(zero, 0.0, (d[a, bj] * d[a, bk]).sum(axis=1) / (rb * rk))
                tol_c = np.where(zero, 0.0, (dd[a, bj] / rb + dd[a, bk] / rk) * (1.0 + 2.0 ** -10) + 9.5 * U32)
            mid = np.where(zero, n_theta, A.theta_bin(cos, n_theta))
            first, last = A.theta_bin(cos + tol_c, n_theta), A.theta_bin(cos - tol_c, n_theta)
            first, last = np.where(zero, n_theta, first), np.where(zero, n_theta, last)
            lo, hi = np.minimum(spec[bj], spec[bk]), np.maximum(spec[bj], spec[bk])
            row = lo * S - lo * (lo - 1) // 2 + hi - lo
            in_ref = is_nb[a, bj] & is_nb[a, bk] & (nb.size <= CAPACITY)
            loose = (j >= s_nb.size) | (k >= s_nb.size) | crossing         # a leg-borderline leg, or a centre that may be truncated
            np.add.at(out["angles"][al], (row[in_ref], mid[in_ref]), 1)
            np.add.at(out["cross"][al], row[in_ref], 1)
            out["triplets"] += int(in_ref.sum())
            out["borderline"] += int((in_ref & (first != last)).sum())
            for t in np.flatnonzero((first != last) | loose):
                out["angles_allowed"][al, row[t], first[t]:last[t] + 1] += 1
        out["lists"].append(frame_lists)
    return out


def check(got, ref, what=""):
    """the counts (angles, coord, truncated) of a route inside the allowance of `reference`; prints what moved"""
    angles, coord, trunc = (np.asarray(g).astype(np.int64) for g in got)
    moved = [int(np.abs(angles - ref["angles"]).sum()), int(np.abs(coord - ref["coord"]).sum()), int(np.abs(trunc - ref["truncated"]).sum())]
    print(f"{what}: {ref['borderline']} borderline of {ref['triplets']} triplets, {ref['leg_borderline']} leg-borderline, most neighbours "
          f"{ref['most']}; counts moved: angles {moved[0]}, coordination {moved[1]}, truncated {moved[2]}")
    return (np.all(np.abs(angles - ref["angles"]) <= ref["angles_allowed"]) and np.all(np.abs(coord - ref["coord"]) <= ref["coord_allowed"])
            and np.all(np.abs(trunc - ref["truncated"]) <= ref["truncated_allowed"]))


def identities(got, sizes, n_o):
    """the exact identities of the definition that the counts alone can show"""
    angles, coord, trunc = (np.asarray(g).astype(np.int64) for g in got)
    S = coord.shape[0]
    n = np.arange(CAPACITY + 1)
    ok = np.array_equal(coord.sum(axis=2) + trunc[:, None], np.broadcast_to((n_o * np.asarray(sizes, np.int64))[:, None], (S, S)))
    for al in range(S):
        for be in range(S):
            ok = ok and angles[al, A.pair_row(be, be, S)].sum() == (coord[al, be] * n * (n - 1) // 2).sum()
    return bool(ok)


# ---- a NumPy twin of the stated arithmetic, with the planted faults -----------------------------------------------------
FAULTS = ("no_image", "orthogonal_only", "one_cutoff", "diagonal_doubled", "self_included", "angle_at_b", "cos_bins", "bin_shift",
          "first_64")


def cos_edges(n_theta):
    edge = np.cos(np.arange(n_theta + 1) * (np.pi / n_theta)).astype(np.float32)
    edge[0], edge[n_theta] = 1.0, -1.0
    return edge


def table_bin(cos, edge):
    """the i with edge[i + 1] < cos <= edge[i]; -1 in the last bin"""
    n_theta = edge.size - 1
    return n_theta - 1 - np.searchsorted(edge[:n_theta][::-1], cos, side="left")


def _cos32(db, dc):
    """the float32 chain of two legs (m, 3): (cos, not a number)"""
    r2b = P._fma32(db[:, 2], db[:, 2], P._fma32(db[:, 1], db[:, 1], db[:, 0] * db[:, 0]))
    r2c = P._fma32(dc[:, 2], dc[:, 2], P._fma32(dc[:, 1], dc[:, 1], dc[:, 0] * dc[:, 0]))
    dot = P._fma32(db[:, 2], dc[:, 2], P._fma32(db[:, 1], dc[:, 1], db[:, 0] * dc[:, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dot / np.sqrt(r2b * r2c)
    return np.clip(cos, np.float32(-1.0), np.float32(1.0)), np.isnan(cos)


def model(positions, box, groups, r_cut, step, n_theta, fault=None):
    """(angles, coord, truncated) int64 as the stated float32 arithmetic gives them.  Faults: FAULTS"""
    S = len(groups)
    n_p = S * (S + 1) // 2
    rc = A.cutoffs(r_cut, S)
    if fault == "one_cutoff":
        rc = np.full_like(rc, rc.max())
    atoms, spec = A.species_of(groups)
    n = atoms.size
    angles, coord, trunc = np.zeros((S, n_p, n_theta + 1), np.int64), np.zeros((S, S, CAPACITY + 1), np.int64), np.zeros(S, np.int64)
    if n == 0:
        return angles, coord, trunc
    c = P.fractions_model(positions, box)
    h = R.box64(box)[0].astype(np.float32)
    if fault == "orthogonal_only":
        h = np.diag(np.diag(h))
    with np.errstate(divide="ignore"):
        inv = np.where(rc > 0.0, 1.0 / rc, 0.0).astype(np.float32)[spec[:, None], spec[None, :]]
    edge = cos_edges(n_theta)
    for o in range(0, c.shape[0], step):
        f = c[o][atoms]
        e = (f[None, :, :] - f[:, None, :]).astype(np.float32)              # e[a, b] = c(b) - c(a)
        if fault != "no_image":
            e = e - np.rint(e)
        d = np.stack([P._fma32(e[..., 2], h[2, k], P._fma32(e[..., 1], h[1, k], e[..., 0] * h[0, k])) for k in range(3)], -1)
        r2 = P._fma32(d[..., 2], d[..., 2], P._fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        near = (np.sqrt(r2) * inv < np.float32(1.0)) & (inv > 0)
        if fault != "self_included":
            near &= ~np.eye(n, dtype=bool)
        for a in range(n):
            al = spec[a]
            nb = np.flatnonzero(near[a])
            if nb.size > CAPACITY:
                trunc[al] += 1
                if fault != "first_64":
                    continue
                nb = nb[:CAPACITY]
            for be in range(S):
                coord[al, be, int((spec[nb] == be).sum())] += 1
            j, k = np.triu_indices(nb.size, 1)
            if j.size == 0:
                continue
            db, dc = d[a, nb[j]], d[a, nb[k]]
            if fault == "angle_at_b":
                db, dc = -db, (dc - db).astype(np.float32)
            cos, bad = _cos32(db, dc)
            if fault == "cos_bins":
                bins = np.minimum(np.floor((1.0 - cos.astype(np.float64)) * 0.5 * n_theta).astype(np.int64), n_theta - 1)
            else:
                bins = table_bin(np.where(bad, np.float32(0.0), cos), edge)
            if fault == "bin_shift":
                bins = np.minimum(bins + 1, n_theta - 1)
            bins = np.where(bad, n_theta, bins)
            lo, hi = np.minimum(spec[nb[j]], spec[nb[k]]), np.maximum(spec[nb[j]], spec[nb[k]])
            row = lo * S - lo * (lo - 1) // 2 + hi - lo
            np.add.at(angles[al], (row, bins), 1)
            if fault == "diagonal_doubled":
                same = lo == hi
                np.add.at(angles[al], (row[same], bins[same]), 1)
    return angles, coord, trunc
