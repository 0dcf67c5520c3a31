"""Float64 restatement of the path integrator — TEST INFRASTRUCTURE, built on tests/ref_bruteforce.py.

Same conventions as ref_bruteforce (every ray against every triangle, textbook Moller-Trumbore, float64), extended from the primary
hit to every vertex of a path: next-event estimation to the projector and the spot at each vertex, cosine-weighted bounces about the
(geometric) normal faced to the incoming ray, throughput times pi f, Mitsuba's Russian roulette, and the counter-based random numbers
of DESIGN.md 4.4 — stated here so that a GPU render can be compared per pixel with the same paths.  Flat-shaded scenes without
base-colour textures.
"""
import numpy as np

from tests import ref_bruteforce as bf

EPS = bf.EPS


def path_key(seed):
    seed_key = bf._hash32(np.uint64((seed + 0x9E3779B9) & 0xFFFFFFFF))
    return bf._hash32(seed_key ^ np.uint64(0x5BD1E995))


def path_u(key, idx, v, dim):
    """the path's random number of sample idx, vertex v (1 = the primary hit), dimension dim (0, 1: direction, 2: roulette)"""
    h = bf._hash32(np.asarray(idx, np.uint64) ^ key)
    r = bf._hash32((h + np.uint64(4 * v + dim)) & 0xFFFFFFFF)
    return (r >> 8).astype(np.float64) / 16777216.0


def cosine_dir(n, u0, u1):
    """sqrt(u0) (cos, sin)(2 pi u1), sqrt(1 - u0) in the frame of Duff et al. 2017 about the unit normals n [N,3]"""
    s, t = bf._onb(n)
    r, ph = np.sqrt(u0), 2.0 * np.pi * u1
    x, y, z = r * np.cos(ph), r * np.sin(ph), np.sqrt(np.maximum(1.0 - u0, 0.0))
    return x[:, None] * s + y[:, None] * t + z[:, None] * n


def _emitters(sd, tris, rows, P, n, Po, d):
    """next-event estimation at the points P (normal n faced to the incoming direction d, lifted origins Po) — ref_bruteforce's
    _shade_terms for arbitrary rays: projector factor per channel (BSDF included), bilinear taps and weights, spot radiance"""
    N = len(P)
    out = {"pfac": np.zeros((N, 3)), "taps": None, "w": None, "spot": np.zeros((N, 3))}
    if sd.proj.enabled:
        tw = bf._m(sd.proj.to_world, 4)
        w2l = np.linalg.inv(tw)
        pl = P @ w2l[:3, :3].T + w2l[:3, 3]
        q = np.concatenate([pl, np.ones((N, 1))], 1) @ bf._m(sd.proj.camera_to_sample, 4).T
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = q[:, 0] / q[:, 3], q[:, 1] / q[:, 3]
        ppos, axis = tw[:3, 3], tw[:3, 2]
        wi = ppos - P
        wi = wi / np.linalg.norm(wi, axis=1, keepdims=True)
        cos_s, cos_p = (n * wi).sum(1), -(wi @ axis)
        lit = (pl[:, 2] > 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (cos_s > 0) & (cos_p > 0)
        if sd.shadows and lit.any():
            sel = np.where(lit)[0]
            lit[sel[bf.any_hit(np.broadcast_to(ppos, (len(sel), 3)), Po[sel] - ppos, tris, 1.0 - 10.0 * EPS)]] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            fac = (np.pi * sd.proj.scale / (pl[:, 2] ** 2 * cos_p))[:, None] * bf.bsdf_cos(rows, n, -d, wi)
        out["pfac"] = np.where(lit[:, None], fac, 0.0)
        out["taps"], out["w"] = bf._bilinear_setup(np.where(lit, u, 0.5), np.where(lit, v, 0.5), sd.proj.tex_w, sd.proj.tex_h)
    if sd.spot.enabled:
        tw = bf._m(sd.spot.to_world, 4)
        spos = tw[:3, 3]
        wi = spos - P
        d2 = (wi * wi).sum(1)
        wi = wi / np.sqrt(d2)[:, None]
        ll = (-wi) @ np.linalg.inv(tw)[:3, :3].T
        ang = np.arccos(np.clip(ll[:, 2] / np.linalg.norm(ll, axis=1), -1, 1))
        cutoff, beam = np.deg2rad(sd.spot.cutoff_deg), np.deg2rad(sd.spot.beam_width_deg)
        fall = np.where(ang <= beam, 1.0, np.where(ang < cutoff, (cutoff - ang) / (cutoff - beam), 0.0))
        lit = ((n * wi).sum(1) > 0) & (fall > 0)
        if sd.shadows and lit.any():
            sel = np.where(lit)[0]
            lit[sel[bf.any_hit(np.broadcast_to(spos, (len(sel), 3)), Po[sel] - spos, tris, 1.0 - 10.0 * EPS)]] = False
        f = np.where(lit[:, None], (fall / d2)[:, None] * bf.bsdf_cos(rows, n, -d, wi), 0.0)
        out["spot"] = f * np.asarray(list(sd.spot.intensity), np.float64)[None]
    return out


def path_vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth=5):
    """every vertex of every sample's path: a list of (sample indices, throughput [n,3], _emitters' terms and "shape": the hit shapes) in vertex order"""
    mats = np.asarray(mats, np.float64)
    tris = bf.world_triangles(verts, tri_idx)
    v0, e1, e2 = tris
    key = path_key(seed)
    o, d, nt, ft = bf.camera_rays(sd.cam, spp, True, seed)
    idx = np.arange(len(d), dtype=np.uint64)
    beta = np.ones((len(d), 3))
    out = []
    for v in range(1, max_depth):
        t, prim = bf.intersect(o, d, tris, nt, ft)
        hit = prim >= 0
        idx, o, d, beta, t, prim = idx[hit], o[hit], d[hit], beta[hit], t[hit], prim[hit]
        if len(idx) == 0:
            break
        P = o + t[:, None] * d
        n = np.cross(e1[prim], e2[prim])
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(((n * d).sum(1) > 0)[:, None], -n, n)
        Po = P + n * ((1.0 + np.abs(P).max(1)) * EPS)[:, None]
        rows = mats[np.asarray(tri_shape)[prim]]
        e = _emitters(sd, tris, rows, P, n, Po, d)
        e["shape"] = np.asarray(tri_shape)[prim]  # (the shape every sample's vertex lies on)
        out.append((idx, beta.copy(), e))
        if v + 1 >= max_depth:
            break
        wo = cosine_dir(n, path_u(key, idx, v, 0), path_u(key, idx, v, 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.pi * bf.bsdf_cos(rows, n, -d, wo) / (n * wo).sum(1)[:, None]
        beta = beta * f
        bmax = beta.max(1)
        keep = bmax > 0
        if v >= rr_depth:
            q = np.minimum(bmax, 0.95)
            keep &= path_u(key, idx, v, 2) < q
            beta = beta / np.where(keep, q, 1.0)[:, None]
        idx, o, d, beta = idx[keep], Po[keep], wo[keep], beta[keep]
        nt, ft = np.zeros(len(idx)), np.full(len(idx), np.inf)
    return out


def _tex_value(sd, tex, e):
    (x0, x1, y0, y1), (w00, w01, w10, w11) = e["taps"], e["w"]
    tex = np.asarray(tex, np.float64)
    if tex.ndim == 2 or tex.shape[-1] == 1:
        t2 = tex.reshape(tex.shape[0], tex.shape[1])
        tv = w00 * t2[y0, x0] + w01 * t2[y0, x1] + w10 * t2[y1, x0] + w11 * t2[y1, x1]
        return tv[:, None] * np.asarray(list(sd.proj.color), np.float64)[None]
    return w00[:, None] * tex[y0, x0] + w01[:, None] * tex[y0, x1] + w10[:, None] * tex[y1, x0] + w11[:, None] * tex[y1, x1]


def sample_radiance(verts, tri_idx, tri_shape, sd, mats, tex, spp, seed, max_depth, rr_depth=5):
    """[W*H*spp, 3]: every sample's path radiance"""
    L = np.zeros((sd.cam.width * sd.cam.height * spp, 3))
    for idx, beta, e in path_vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth):
        rad = e["spot"].copy()
        if sd.proj.enabled:
            rad += _tex_value(sd, tex, e) * e["pfac"]
        L[idx.astype(np.int64)] += beta * rad
    return L


def render_fwd(verts, tri_idx, tri_shape, sd, mats, tex, spp, seed, max_depth, rr_depth=5, gaussian_stddev=None):
    W, H = sd.cam.width, sd.cam.height
    L = sample_radiance(verts, tri_idx, tri_shape, sd, mats, tex, spp, seed, max_depth, rr_depth)
    if gaussian_stddev is not None:
        num, den, _ = bf._film_splat(W, H, spp, seed, gaussian_stddev, values=L)
        return np.where(den[..., None] > 0, num / np.where(den > 0, den, 1.0)[..., None], 0.0)
    return L.reshape(H, W, spp, 3).mean(2)


def render_bwd(verts, tri_idx, tri_shape, sd, mats, spp, seed, gimg, max_depth, rr_depth=5, gaussian_stddev=None):
    """d <img, gimg> / d tex, [tex_h, tex_w, channels]"""
    W, H = sd.cam.width, sd.cam.height
    gimg = np.asarray(gimg, np.float64).reshape(H, W, 3)
    if gaussian_stddev is not None:
        _, den, _ = bf._film_splat(W, H, spp, seed, gaussian_stddev)
        G = np.where(den[..., None] > 0, gimg / np.where(den > 0, den, 1.0)[..., None], 0.0)
        _, _, q = bf._film_splat(W, H, spp, seed, gaussian_stddev, gather=G)
    else:
        q = np.repeat(gimg.reshape(-1, 3), spp, axis=0) / spp
    tc = sd.proj.tex_channels
    gt = np.zeros((sd.proj.tex_h, sd.proj.tex_w, tc))
    color = np.asarray(list(sd.proj.color), np.float64)
    for idx, beta, e in path_vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth):
        cw = q[idx.astype(np.int64)] * beta * e["pfac"]
        (x0, x1, y0, y1), ws = e["taps"], e["w"]
        for (yy, xx), w in zip(((y0, x0), (y0, x1), (y1, x0), (y1, x1)), ws):
            if tc == 1:
                np.add.at(gt[..., 0], (yy, xx), (cw * color[None]).sum(1) * w)
            else:
                for ch in range(3):
                    np.add.at(gt[..., ch], (yy, xx), cw[:, ch] * w)
    return gt
