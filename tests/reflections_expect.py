"""Expectation of the baked-light pass with a reflection probe set (gi_render_baked_reflections_*; include/gi_hip.h states the definition): the
numpy statement of its step 5 -- containment, edge distance, weight, exit distance, projected direction, the blend and the fall-back to the
nearest probe -- written from the header alone, one IEEE operation at a time in the header's order, so that given identical first hits the
specular term is the device's bit for bit.  First hits come from the oracle as in baked_expect (sample_hits).  Shared by the GPU tests and the
CPU tests."""
import numpy as np

import baked_expect as be

ROUTES = ("fallback", "single", "blended")          # by the number of probes with w > 0: none, one, two or more
MAX_PROBES = 64


def texel_of(D, n):
    """The texel (f n + row) n + col of a cube of face n each direction D [m][3] falls into, by step 5's rule of gi_render_baked_*, with the
    library's answers for what is no direction: a NaN coordinate goes to column (row) 0, one beyond the face to the border, a NaN or zero size
    to face +X."""
    D = np.asarray(D, np.float64)
    A = np.where(D < 0.0, -D, D)
    axis = np.zeros(len(D), np.int64)
    size = A[:, 0]
    c = A[:, 1] > size
    axis, size = np.where(c, 1, axis), np.where(c, A[:, 1], size)
    c = A[:, 2] > size
    axis, size = np.where(c, 2, axis), np.where(c, A[:, 2], size)
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, z = D[:, 0] / size, D[:, 1] / size, D[:, 2] / size
    neg = np.take_along_axis(D, axis[:, None], 1)[:, 0] < 0.0
    f = 2 * axis + neg
    a = np.choose(f, [-z, z, x, x, x, -x])
    b = np.choose(f, [-y, -y, z, -z, -y, -y])

    def coord(q):
        with np.errstate(invalid="ignore"):
            v = ((q + 1.0) * 0.5) * float(n)
            inside = (v >= 1.0) & (v < float(n))
            return np.where(v >= 1.0, np.where(inside, np.floor(np.where(inside, v, 0.0)), float(n - 1)), 0.0).astype(np.int64)

    return (f * n + coord(b)) * n + coord(a)


def probe_terms(pr, P, R):
    """One probe row pr [10] against the hits P [m][3] and directions R [m][3]: (inside [m], w [m], D [m][3], t [m])."""
    pos, lo, hi, fade = pr[0:3], pr[3:6], pr[6:9], pr[9]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inside = np.ones(len(P), bool)
        for a in range(3):
            inside &= (lo[a] <= P[:, a]) & (P[:, a] <= hi[a])
        edge = P[:, 0] - lo[0]
        for v in (hi[0] - P[:, 0], P[:, 1] - lo[1], hi[1] - P[:, 1], P[:, 2] - lo[2], hi[2] - P[:, 2]):
            edge = np.where(v < edge, v, edge)
        if fade > 0.0:
            q = edge / fade
            w = np.where(q < 1.0, q, 1.0)
        else:
            w = np.ones(len(P))
        t = np.zeros(len(P))
        have = np.zeros(len(P), bool)
        for a in range(3):
            Ra = R[:, a]
            on = Ra != 0.0
            v = (np.where(Ra > 0.0, hi[a], lo[a]) - P[:, a]) / Ra
            take = on & (~have | (v < t))
            t = np.where(take, v, t)
            have |= on
        Q = P + t[:, None] * R
        D = Q - pos
        bad = ~np.isfinite(D).all(1) | (D == 0.0).all(1)
    return inside, w, np.where(bad[:, None], R, D), t


def nearest(probes, P):
    """k* [m]: the probe with the least ((dx dx + dy dy) + dz dz), the first of equals, a NaN never less, 0 when none is less than infinity."""
    best = np.zeros(len(P), np.int64)
    bd = np.full(len(P), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, pr in enumerate(probes):
            d = P - pr[0:3]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            less = d2 < bd
            bd, best = np.where(less, d2, bd), np.where(less, k, best)
    return best


def lookup_detail(probes, chains, face, levels, P, R, level):
    """Step 5 on hits P [m][3], directions R [m][3] and levels level [m] (or one number): a dict of S [m][3], route [m] (index into ROUTES),
    inside [K][m], w [K][m], texel [K][m] (inside a chain, the level's offset included), kstar [m] and fallback_texel [m]."""
    probes = np.asarray(probes, np.float64).reshape(-1, 10)
    chains = np.asarray(chains, np.float64)
    P, R = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(R, np.float64).reshape(-1, 3)
    level = np.broadcast_to(np.asarray(level, np.int64), (len(P),))
    K, m = len(probes), len(P)
    assert 1 <= K <= MAX_PROBES and chains.shape == (K, be.chain_offsets(face, levels)[-1], 3)
    off = np.asarray(be.chain_offsets(face, levels))[level]
    n_of = face >> level

    def texels(D):
        t = np.zeros(m, np.int64)
        for l in np.unique(level):
            sel = level == l
            t[sel] = texel_of(D[sel], face >> int(l))
        assert (t < 6 * n_of * n_of).all() and (t >= 0).all()
        return off + t

    acc, W = np.zeros((m, 3)), np.zeros(m)
    inside_all, w_all, tex_all = np.zeros((K, m), bool), np.zeros((K, m)), np.zeros((K, m), np.int64)
    for k, pr in enumerate(probes):
        inside, w, D, _ = probe_terms(pr, P, R)
        tx = texels(D)
        v = chains[k][tx]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = np.where(inside[:, None], acc + w[:, None] * v, acc)
            W = np.where(inside, W + w, W)
        inside_all[k], w_all[k], tex_all[k] = inside, w, tx
    kstar = nearest(probes, P)
    fb_tex = texels(R)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where((W > 0.0)[:, None], acc / W[:, None], chains[kstar, fb_tex])
    count = (inside_all & (w_all > 0.0)).sum(0)
    assert ((count > 0) == (W > 0.0)).all()
    return {"S": S, "route": np.minimum(count, 2), "inside": inside_all, "w": w_all, "texel": tex_all, "kstar": kstar, "fallback_texel": fb_tex}


def lookup(probes, chains, face, levels, P, R, level):
    """(S [m][3], route [m] of "fallback" / "single" / "blended") of step 5."""
    d = lookup_detail(probes, chains, face, levels, P, R, level)
    return d["S"], np.array(ROUTES)[d["route"]]


def specular_inputs(g, tables, levels, exponents):
    """(sel, R, level) of the samples of g (baked_expect.sample_hits) on the mirror or glossy lobe: their rows, step 5's R and the level read."""
    rough = tables["mats"][np.where(g["hit"], g["mat"], 0), 0]
    lobe = np.where(g["hit"], be.lobe_of(rough), -1)
    sel = np.flatnonzero((lobe == 0) | (lobe == 1))
    level = np.where(lobe[sel] == 0, 0, be.level_table(tables["mats"][:, 0], levels, exponents)[g["mat"][sel]])
    return sel, be.reflect(g["d"][sel], g["Nf"][sel]), level


def sample_specular(g, tables, probes, chains, exponents, face=be.CHAIN_FACE, levels=be.CHAIN_LEVELS):
    """(specular [n][3], route [n]: index into ROUTES, -1 where the sample has no specular term) of one sample from its first hits g."""
    n = len(g["hit"])
    specular, route = np.zeros((n, 3)), np.full(n, -1, np.int64)
    sel, R, level = specular_inputs(g, tables, levels, exponents)
    if len(sel):
        d = lookup_detail(probes, chains, face, levels, g["P"][sel], R, level)
        specular[sel] = g["albedo"][sel] * d["S"]
        route[sel] = d["route"]
    return specular, route


def flips_under_perturbation(g, tables, probes, face, levels, exponents, ulps=4):
    """How many specular samples change a containment, their route or a texel they read when every component of P and of R moves by `ulps`
    ulp, up or down (all 64 sign patterns): the room the statement has on these frames.  Returns (flipped, asked)."""
    sel, R, level = specular_inputs(g, tables, levels, exponents)
    if not len(sel):
        return 0, 0
    P = g["P"][sel]
    chains = np.zeros((len(probes), be.chain_offsets(face, levels)[-1], 3))

    def facts(P_, R_):
        d = lookup_detail(probes, chains, face, levels, P_, R_, level)
        return d["inside"], d["route"], np.where(d["inside"], d["texel"], -1), np.where(d["route"] == 0, d["fallback_texel"], -1), np.where(d["route"] == 0, d["kstar"], -1)

    base = facts(P, R)
    flipped = np.zeros(len(sel), bool)
    signs = [(a, b, c) for a in (1.0, -1.0) for b in (1.0, -1.0) for c in (1.0, -1.0)]
    for sp in signs:
        for sr in signs:
            got = facts(P + np.array(sp) * ulps * np.spacing(np.abs(P)), R + np.array(sr) * ulps * np.spacing(np.abs(R)))
            for a, b in zip(base, got):
                flipped |= (a != b).reshape(-1, len(sel)).any(0) if a.ndim == 2 else (a != b)
    return int(flipped.sum()), len(sel)


# ---------------------------------------------------------------------------------------------------------------- inputs of the tests
KS = (1, 2, 5)
# Box fractions of the scene's root box per probe: (lo xyz, hi xyz, position inside the probe's box xyz, fade as a share of the scene box's
# shortest edge).  Probe 0 has no fade band.  The boxes overlap in the scene's middle (blended), leave its outer parts to one probe (single) and
# its far corners to none (fallback); no face passes within a few ulp of a first hit of the GPU tests' frames -- tests/test_reflections_cpu.py
# checks that on the oracle's hits.
PROBE_FRACTIONS = (
    ((-0.07, -0.11, -0.05), (0.61, 0.83, 0.67), (0.45, 0.40, 0.55), 0.0),
    ((0.33, 0.09, 0.21), (1.09, 1.13, 1.06), (0.50, 0.60, 0.35), 0.12),
    ((0.13, -0.06, 0.29), (0.87, 0.57, 1.08), (0.60, 0.50, 0.50), 0.07),
    ((-0.09, 0.37, -0.08), (0.71, 1.07, 0.59), (0.35, 0.55, 0.45), 0.2),
    ((0.41, 0.23, 0.17), (0.79, 0.77, 0.73), (0.50, 0.50, 0.50), 0.03),
)


def random_probes(tables, K, seed=0):
    """The table [K][10] of the tests' set for a scene: PROBE_FRACTIONS' first rows (further rows, for K > 5, are drawn from `seed` in the same
    ranges), scaled to the scene's root box."""
    b = tables["node_bbox"][0]
    size = b[3:6] - b[0:3]
    rs = np.random.default_rng(seed)
    out = np.zeros((K, 10))
    for k in range(K):
        if k < len(PROBE_FRACTIONS):
            lo, hi, at, fade = (np.asarray(q, np.float64) for q in PROBE_FRACTIONS[k])
        else:
            lo, hi, at, fade = rs.uniform(-0.1, 0.4, 3), rs.uniform(0.6, 1.1, 3), rs.uniform(0.3, 0.7, 3), rs.uniform(0.02, 0.2)
        out[k, 3:6] = b[0:3] + lo * size
        out[k, 6:9] = b[0:3] + hi * size
        out[k, 0:3] = out[k, 3:6] + at * (out[k, 6:9] - out[k, 3:6])
        out[k, 9] = fade * size.min()
    return out


def random_chains(K, seed, face=be.CHAIN_FACE, levels=be.CHAIN_LEVELS):
    """K chains from be.random_chain, as lists of levels."""
    return [be.random_chain(seed + 31 * k, face, levels) for k in range(K)]


def flat_chains(chains):
    """[K][texels][3] of chains given as lists of levels."""
    return np.ascontiguousarray(np.stack([np.concatenate([c.reshape(-1, 3) for c in chain]) for chain in chains]))


def direction_chain(face=be.CHAIN_FACE, levels=be.CHAIN_LEVELS):
    """A chain whose every texel holds the unit direction of its own centre."""
    import gi_raytracer_amd as gi
    return [gi.cube_directions(face >> l) for l in range(levels)]


def scene_box_probe(tables):
    """One probe at the middle of the scene's root box, the box its own, no fade."""
    b = tables["node_bbox"][0]
    return np.concatenate([0.5 * (b[0:3] + b[3:6]), b[0:3], b[3:6], [0.0]]).reshape(1, 10)


def angle_between(a, b):
    """The angle [m] between vectors a and b [m][3] of any length, by atan2 of |a x b| and a . b."""
    c = np.cross(a, b)
    return np.arctan2(np.sqrt((c * c).sum(-1)), (a * b).sum(-1))
