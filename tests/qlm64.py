"""float64 reference of the local-order tests, by the definition of include/psa_hip.h at psa_local_order and by another route
than the kernel's: the neighbours by the brute force of tests/angle64.py; the harmonics from spherical angles -- associated
Legendre functions in cos(theta) = d_z / r with sin(theta) = hypot(d_x, d_y) / r (no sqrt(1 - cos^2), no arccos: a reference
through arccos is off by 7e-9 for a leg 1e-7 off the z axis), e^{i m phi} from arctan2 --; the full complex vectors over m in
[-l, l]; the 3j symbols from the integral of three harmonics by Gauss-Legendre quadrature, which shares nothing with Racah's
formula (sympy's symbols are held against both in tests/test_qlm_host.py)."""
import functools
import math

import numpy as np

import angle64 as A
import order64 as O

CAPACITY = A.CAPACITY


def harmonics(legs, l):
    """Yt_lm = sqrt(4 pi / (2 l + 1)) Y_lm of the legs' directions, Condon-Shortley phase included: (n, 2 l + 1) complex, column
    m + l"""
    d = np.asarray(legs, np.float64).reshape(-1, 3)
    r = np.sqrt((d * d).sum(axis=1))
    ct, st, phi = d[:, 2] / r, np.hypot(d[:, 0], d[:, 1]) / r, np.arctan2(d[:, 1], d[:, 0])
    out = np.zeros((d.shape[0], 2 * l + 1), complex)
    for m in range(l + 1):
        pmm = (-1.0) ** m * float(np.prod(np.arange(2 * m - 1, 0, -2))) * st ** m          # P_m^m
        prev, cur = np.zeros_like(ct), pmm
        for k in range(m + 1, l + 1):
            prev, cur = cur, ((2 * k - 1) * ct * cur - (k + m - 1) * prev) / (k - m)
        y = math.sqrt(math.factorial(l - m) / math.factorial(l + m)) * cur * np.exp(1j * m * phi)
        out[:, l + m] = y
        out[:, l - m] = (-1.0) ** m * np.conj(y)
    return out


@functools.lru_cache(maxsize=None)
def three_j(l):
    """(2 l + 1, 2 l + 1): (l l l; m1 m2 -m1-m2) at [m1 + l, m2 + l] from the integral of three harmonics,
    int Y_lm1 Y_lm2 Y_lm3 = sqrt((2 l + 1)^3 / 4 pi) (l l l; 0 0 0) (l l l; m1 m2 m3), by a quadrature that is exact for it; the
    sign of (l l l; 0 0 0), (-1)^(3 l / 2), and its modulus fixed through sum (3j)^2 = 1.  Even l."""
    x, wx = np.polynomial.legendre.leggauss(2 * l + 2)
    n_phi = 4 * l + 2
    phi = 2.0 * np.pi * np.arange(n_phi) / n_phi
    ct, ph = np.repeat(x, n_phi), np.tile(phi, x.size)
    st = np.sqrt((1.0 - ct) * (1.0 + ct))
    y = harmonics(np.stack([st * np.cos(ph), st * np.sin(ph), ct], 1), l)
    w = np.repeat(wx, n_phi) * (2.0 * np.pi / n_phi)
    out = np.zeros((2 * l + 1, 2 * l + 1))
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            if abs(m1 + m2) <= l:
                out[m1 + l, m2 + l] = (w * y[:, m1 + l] * y[:, m2 + l] * y[:, l - m1 - m2]).sum().real
    out /= math.sqrt((out * out).sum())
    return out * ((-1.0) ** (3 * l // 2) * np.sign(out[l, l]))


def three_j_zero(l):
    """(l l l; 0 0 0) in closed form, even l: (-1)^g sqrt((l!)^3 / (3 l + 1)!) g! / ((g - l)!)^3 with g = 3 l / 2"""
    g, f = 3 * l // 2, math.factorial
    return (-1.0) ** g * math.sqrt(f(l) ** 3 / f(3 * l + 1)) * f(g) / f(g - l) ** 3


def w_form(v, l):
    """W_l(v) = sum_{m1+m2+m3=0} (l l l; m1 m2 m3) v_m1 v_m2 v_m3 of a full vector (2 l + 1,), column m + l: the real part"""
    t = three_j(l)
    total = 0.0
    for m1 in range(-l, l + 1):
        for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
            total += t[m1 + l, m2 + l] * (v[m1 + l] * v[m2 + l] * v[l - m1 - m2])
    return float(np.real(total))


def w_hat(legs, l):
    """w_l of one shell: W_l(sum_b Yt) / (sum_m |.|^2)^(3/2)"""
    v = harmonics(legs, l).sum(axis=0)
    return w_form(v, l) / float((np.abs(v) ** 2).sum()) ** 1.5


def per_atom(positions, box, groups, r_cut, step, ls, solid_l, threshold):
    """by the definition, per origin o and listed atom a (list order):
    `v`[j] (n_o, n_a, 2 l + 1) complex = sum_b Yt_lm(d_b) (Q 2^-40 without the rounding), `vbar`[j] the averaged q-bar_lm;
    `n`, `why` (n_o, n_a): 0 counted, 1 truncated, 2 isolated, 3 undefined, 4 incomplete; `lists` per origin the neighbours of
    every atom; `D`, `AB` per origin dicts (a, b) -> D and A B of the bond at order solid_l"""
    atoms, _ = A.species_of(groups)
    origins = range(0, np.shape(positions)[0], step)
    n_o, n_a = len(origins), atoms.size
    v = [np.zeros((n_o, n_a, 2 * l + 1), complex) for l in ls]
    vbar = [np.zeros((n_o, n_a, 2 * l + 1), complex) for l in ls]
    count, why = np.zeros((n_o, n_a), np.int64), np.zeros((n_o, n_a), np.int64)
    lists, bonds = [], []
    js = list(ls).index(solid_l)
    for o, f in enumerate(origins):
        if n_a == 0:
            lists.append([]), bonds.append({})
            continue
        d, r, near = O.frame_shells(positions[f], box, groups, r_cut)
        nbs = [np.flatnonzero(near[a]) for a in range(n_a)]
        lists.append(nbs)
        for a, nb in enumerate(nbs):
            count[o, a] = nb.size
            why[o, a] = 1 if nb.size > CAPACITY else 2 if nb.size == 0 else 3 if np.any(r[a, nb] == 0.0) else 0
            if why[o, a] == 0:
                for j, l in enumerate(ls):
                    v[j][o, a] = harmonics(d[a, nb], l).sum(axis=0)
        own = why[o].copy()
        for a, nb in enumerate(nbs):
            if own[a] == 0 and np.any((own[nb] == 1) | (own[nb] == 3)):
                why[o, a] = 4
        frame_bonds = {}
        for a, nb in enumerate(nbs):
            if why[o, a]:
                continue
            for j in range(len(ls)):
                vbar[j][o, a] = (v[j][o, a] / nb.size + (v[j][o, nb] / count[o, nb][:, None]).sum(axis=0)) / (nb.size + 1)
            va = v[js][o, a]
            for b in nb:
                vb = v[js][o, b]
                frame_bonds[(a, int(b))] = (float(np.real(np.vdot(vb, va))), float(np.vdot(va, va).real * np.vdot(vb, vb).real))
        bonds.append(frame_bonds)
    return dict(v=v, vbar=vbar, n=count, why=why, lists=lists, bonds=bonds)
