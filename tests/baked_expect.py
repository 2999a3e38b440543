"""Expectation of the baked-light pass (gi_render_baked_*; include/gi_hip.h states the definition): the numpy statement of its steps 3 to 7 -- the
lobe, the level table, the probe grid's cell, the SH9 irradiance factors, the trilinear step, the cube texel, the sums -- on first hits taken from
the oracle as occlusion_expect.sample_geometry takes them (Oracle.primary_ray, Oracle.trace, albedo via features_expect).  Shared by the GPU
tests and the CPU tests.

Every operation is written in the header's order, one IEEE operation at a time, so that given identical first hits the diffuse term is the
device's bit for bit, and the specular term wherever the texel is the same.  Valid for scenes whose alpha test cannot depend on the draw
(features_expect.DRAW_FREE_SCENES)."""
import numpy as np

import gi_raytracer_amd as gi

import features_expect as fe
import oracle_lib as ol

DIRECT, DIFFUSE, SPECULAR, EMISSIVE = gi.BAKED_DIRECT, gi.BAKED_DIFFUSE, gi.BAKED_SPECULAR, gi.BAKED_EMISSIVE
K_BAND = np.array([1.0] + [0.6666666666666666] * 3 + [0.25] * 5)
MIRROR_BELOW, GLOSSY_BELOW = .001, .9


# ---------------------------------------------------------------------------------------------------------------- steps 3 to 5, one function each
def lobe_of(roughness):
    """0 mirror (specular from level 0), 1 glossy (specular from the material's level), 2 diffuse."""
    r = np.asarray(roughness, np.float64)
    return np.where(r < MIRROR_BELOW, 0, np.where(r < GLOSSY_BELOW, 1, 2))


def level_table(roughness, levels, exponents):
    """level_of_material: 0 for a mirror and for a chain of one level; else the l of 1 .. levels-1 whose exponents[l] is nearest to
    log2(1 / roughness + 1), ties to the lower l."""
    out = np.zeros(len(roughness), np.int32)
    for m, r in enumerate(np.asarray(roughness, np.float64)):
        if levels <= 1 or r < MIRROR_BELOW or r != r:
            continue
        with np.errstate(divide="ignore"):
            want = np.log2(1.0 / r + 1.0)
        d = [abs(float(exponents[l]) - want) for l in range(1, levels)]
        out[m] = 1 + int(np.argmin(d))                  # argmin: the first of equals
    return out


def grid_cell(p, gmin, gmax, n):
    """(i0, i1, t) of one axis: g = ((p - gmin) / (gmax - gmin)) * n - 0.5 clamped to [0, n - 1], i0 = floor(g), i1 = min(i0 + 1, n - 1), t = g - i0."""
    g = ((np.asarray(p, np.float64) - gmin) / (gmax - gmin)) * float(n) - 0.5
    g = np.where(g > 0.0, np.where(g < float(n - 1), g, float(n - 1)), 0.0)
    i0 = np.floor(g).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), g - i0.astype(np.float64)


def sh9_factor(n):
    """F [..][9] = k_j * Y_j(n) with the literals of GI_BAKE_SH9."""
    n = np.asarray(n, np.float64)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    Y = [np.full(x.shape, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x, 1.0925484305920792 * (x * y),
         1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0), 1.0925484305920792 * (x * z), 0.5462742152960396 * (x * x - y * y)]
    return np.stack([K_BAND[j] * Y[j] for j in range(9)], -1)


def probe_value(c, F):
    """D_c [n][3] = the sum over j, ascending from +0.0, of F_j * c_j[ch], for probes c [n][9][3]."""
    d = np.zeros((len(c), 3))
    for j in range(9):
        d = d + F[:, j][:, None] * c[:, j]
    return d


def irradiance(sh, box, P, Nf):
    """D [n][3] at the points P under the normals Nf from sh [nz][ny][nx][9][3] in box (min xyz, max xyz): evaluate at the eight probes, then
    a + t * (b - a) along x, then y, then z, then clamp at 0 from below."""
    nz, ny, nx = sh.shape[:3]
    box = np.asarray(box, np.float64).reshape(6)
    F = sh9_factor(Nf)
    (x0, x1, tx), (y0, y1, ty), (z0, z1, tz) = (grid_cell(P[:, k], box[k], box[3 + k], n) for k, n in enumerate((nx, ny, nz)))

    def lerp(a, b, t):
        return a + t[:, None] * (b - a)

    dz = []
    for iz in (z0, z1):
        dy = []
        for iy in (y0, y1):
            dy.append(lerp(probe_value(sh[iz, iy, x0], F), probe_value(sh[iz, iy, x1], F), tx))
        dz.append(lerp(dy[0], dy[1], ty))
    d = lerp(dz[0], dz[1], tz)
    return np.where(d < 0.0, 0.0, d)


def reflect(d, nf):
    """R = d - (Nf * dot(Nf, d)) * 2.0 with dot = (Nf.x d.x + Nf.y d.y) + Nf.z d.z."""
    dt = (nf[:, 0] * d[:, 0] + nf[:, 1] * d[:, 1]) + nf[:, 2] * d[:, 2]
    return d - (nf * dt[:, None]) * 2.0


def chain_offsets(face, levels):
    """Texels before each level, and after the last."""
    off = [0]
    for l in range(levels):
        off.append(off[-1] + 6 * (face >> l) ** 2)
    return off


def chain_texel(R, level, face, levels):
    """The row of the whole chain [texels][3] each R reads at its level: gi.cube_texel_of states the texel inside the level."""
    off = chain_offsets(face, levels)
    t = np.zeros(len(R), np.int64)
    for l in range(levels):
        sel = level == l
        if sel.any():
            t[sel] = off[l] + gi.cube_texel_of(R[sel], face >> l)
    return t


# ---------------------------------------------------------------------------------------------------------------- first hits from the oracle
def sample_hits(oracle, tables, w, h, s):
    """First hits of sample s of every pixel (row-major): hit [n] bool, ent, mat [n], P, d, Nf, albedo [n][3] (rows of misses are 0)."""
    rays, idx = fe.sample_rays(oracle, w, h, s)
    hit, ent, mat, albedo, normal, _, _ = fe.sample_features(oracle, tables, rays)
    res = oracle.trace(rays)[2]
    N = normal
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        nh = N * inv[:, None]
    dn = (nh[:, 0] * rays[:, 3] + nh[:, 1] * rays[:, 4]) + nh[:, 2] * rays[:, 5]
    nf = np.where((dn > 0)[:, None], -nh, nh)
    nf = np.where(hit[:, None], nf, 0.0)
    return {"hit": hit, "ent": ent, "mat": mat, "P": np.where(hit[:, None], res[:, 0:3], 0.0), "d": rays[:, 3:6], "Nf": nf, "albedo": albedo, "idx": idx}


def sample_terms(g, tables, sh=None, box=None, chain=None, exponents=None):
    """(diffuse [n][3], specular [n][3], texel [n] = the chain row read or -1, lobe [n] (-1 on a miss)) of one sample from its first hits g:
    steps 3 to 5, a term without data being +0.0.  chain: the list of levels."""
    n = len(g["hit"])
    rough = tables["mats"][np.where(g["hit"], g["mat"], 0), 0]
    lobe = np.where(g["hit"], lobe_of(rough), -1)
    diffuse, specular, texel = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1, np.int64)
    sel = np.flatnonzero(lobe == 2)
    if sh is not None and len(sel):
        diffuse[sel] = g["albedo"][sel] * irradiance(sh, box, g["P"][sel], g["Nf"][sel])
    sel = np.flatnonzero((lobe == 0) | (lobe == 1))
    if chain is not None and len(sel):
        face, levels = chain[0].shape[1], len(chain)
        table = level_table(tables["mats"][:, 0], levels, exponents)
        level = np.where(lobe[sel] == 0, 0, table[g["mat"][sel]])
        flat = np.concatenate([c.reshape(-1, 3) for c in chain])
        texel[sel] = chain_texel(reflect(g["d"][sel], g["Nf"][sel]), level, face, levels)
        specular[sel] = g["albedo"][sel] * flat[texel[sel]]
    return diffuse, specular, texel, lobe


def fold(per_sample):
    """Step 7's sums: per channel over s in ascending order from +0.0, divided once by n."""
    acc = np.zeros_like(per_sample[0])
    for v in per_sample:
        acc = acc + v
    return acc / float(len(per_sample))


def texel_flips_under_perturbation(g, tables, face, levels, exponents, ulps=4):
    """How many specular samples read another texel when every component of R moves by `ulps` ulp, up or down: the room the statement has on
    these frames.  Returns (flipped, asked)."""
    rough = tables["mats"][np.where(g["hit"], g["mat"], 0), 0]
    lobe = np.where(g["hit"], lobe_of(rough), -1)
    sel = np.flatnonzero((lobe == 0) | (lobe == 1))
    if not len(sel):
        return 0, 0
    level = np.where(lobe[sel] == 0, 0, level_table(tables["mats"][:, 0], levels, exponents)[g["mat"][sel]])
    R = reflect(g["d"][sel], g["Nf"][sel])
    base = chain_texel(R, level, face, levels)
    flipped = np.zeros(len(sel), bool)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                flipped |= chain_texel(R + np.array([sx, sy, sz]) * ulps * np.spacing(np.abs(R)), level, face, levels) != base
    return int(flipped.sum()), len(sel)


# ---------------------------------------------------------------------------------------------------------------- scenes and inputs of the tests
ROUGHNESSES = (1.0, 0.5, 0.0005, 0.05)          # diffuse, glossy (wide lobe), mirror, glossy (narrow lobe): material m gets entry m % 4
CHAIN_FACE, CHAIN_LEVELS, CHAIN_EXPONENTS = 8, 3, (0, 5, 1)
GRIDS = ((1, 1, 1), (2, 2, 2), (3, 2, 4))       # nx, ny, nz


def with_roughnesses(scene, roughnesses=ROUGHNESSES):
    """The scene again through the scene builders, material m with roughness roughnesses[m % len]: same entities in the same order, same lights and
    ambient colour.  The camera is the caller's to carry over (scene.settings).  Scenes without textures and fog only."""
    t = scene.tables()
    assert not len(t["tex_kind"]) and not len(t["fog"])
    s = gi.Scene()
    for m, row in enumerate(t["mats"]):
        assert s.add_material(roughnesses[m % len(roughnesses)], row[1], row[2], row[3:6], row[6:9]) == m
    kind = t["ent_kind"]
    i = 0
    while i < len(kind):
        if kind[i] == 1:
            s.add_sphere(t["tri_pos"][i, 0], t["tri_pos"][i, 1, 0], int(t["tri_mat"][i]))
            i += 1
            continue
        j = i
        while j < len(kind) and kind[j] != 1:
            j += 1
        s.add_triangles(t["tri_pos"][i:j], t["tri_nrm"][i:j], t["tri_uv"][i:j], t["tri_mat"][i:j])
        i = j
    for l in t["lights"]:
        s.add_light(l[0:3], l[3:6], l[6])
    s.set_ambient(t["ambient"])
    return s.rebuild()


def oracle_with_camera(scene, st):
    """parity_checks.oracle_for with the camera of the settings st."""
    t = scene.tables()
    o = ol.Oracle().set_scene(t["tri_pos"], t["tri_nrm"], t["tri_uv"], t["tri_mat"], t["mats"], t["lights"][:, :7], t["ambient"], kind=t["ent_kind"])
    o.set_camera(list(st.cam_pos), list(st.cam_up), list(st.cam_forward), st.sensor_diag, st.focal_dist)
    return o.build_octree()


def inner_box(tables, shrink=0.3):
    """A grid box inside the scene's root box, `shrink` of its size cut off at either end of every axis: first hits outside it clamp."""
    b = tables["node_bbox"][0]
    d = b[3:6] - b[0:3]
    return np.concatenate([b[0:3] + shrink * d, b[3:6] - shrink * d])


def random_sh(grid, seed):
    nx, ny, nz = grid
    return np.random.default_rng(seed).uniform(-0.3, 1.0, (nz, ny, nx, 9, 3))


def random_chain(seed, face=CHAIN_FACE, levels=CHAIN_LEVELS):
    rs = np.random.default_rng(seed)
    return [rs.uniform(0.0, 2.0, (6, face >> l, face >> l, 3)) for l in range(levels)]
