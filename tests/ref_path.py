"""Float64 restatement of the path integrator — TEST INFRASTRUCTURE, built on tests/ref_bruteforce.py.

Same conventions as ref_bruteforce (every ray against every triangle, textbook Moller-Trumbore, float64), extended from the primary
hit to every vertex of a path: next-event estimation to the projector and the spot at each vertex, cosine-weighted bounces, throughput
times pi f, Mitsuba's Russian roulette, and the counter-based random numbers of DESIGN.md 4.4 — stated here so that a GPU render can be
compared per pixel with the same paths.

`walk` is the one statement of that walk; tests/ref_lights.py, tests/ref_sun.py and tests/ref_prb.py call it and tests/ref_ambient.py takes
its vertices from `Surface`.  It knows both normals of DESIGN.md 4.3 / 4.4 and the base-colour textures (`smooth`: one flag per shape,
`vert_uv`: [n_verts, 2], `base_tex`: a list of [h, w, 3]):
  * the geometric normal n_g, faced to the incoming ray, lifts the point (Po) and must see every emitter (n_g . wi > 0);
  * the shading normal n_s of a smooth shape is the normalised barycentric mix of the angle-weighted vertex normals, faced by the sign of
    its own cosine with the ray (n_g stands in where the mix has no length); BSDF and emitter cosines are n_s';
  * the bounce is drawn about n_s; the path ends if n_g . wo <= 0, else beta *= pi f / (n_s . wo) with f in the frame of n_s;
  * a textured row's base colour is its texture at the hit's interpolated uv, at every vertex, for beta and for the emitters' terms.
On a flat shape without a texture the two normals are one array and every value is what the walk gave before it knew the difference.
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


# the rules of DESIGN.md 4.3 / 4.4 that a walk can get wrong one at a time.  `swap` names ONE of them and the walk then makes that mistake: what
# tests/test_shading_walk_cpu.py compares with the true walk (swap = None) to show that the bounds of the GPU tests see each of them
SWAPS = ("bounce_about_ng", "no_ng_wo_test", "emitter_cosine_from_ng", "no_geometric_side", "texture_at_vertex_1_only", "ns_not_refaced")


class Surface:
    """a scene's triangles with what DESIGN.md 4.3 reads at a hit: both normals, the lifted point, the material rows under their textures"""

    def __init__(self, verts, tri_idx, tri_shape, smooth=None, vert_uv=None, base_tex=None, swap=None):
        assert swap is None or swap in SWAPS, swap
        self.verts, self.tri_idx, self.tri_shape = np.asarray(verts, np.float64), np.asarray(tri_idx), np.asarray(tri_shape)
        self.tris = bf.world_triangles(verts, tri_idx)
        self.flags = self.vn = None
        if smooth is not None and any(smooth):
            self.flags = np.asarray([bool(f) for f in smooth])
            self.vn = bf.vertex_normals(self.verts, self.tri_idx, use=self.flags[self.tri_shape])
        self.vert_uv = None if vert_uv is None else np.asarray(vert_uv, np.float64)
        self.base_tex, self.swap = base_tex, swap

    def frame(self, P, d, prim):
        """-> (n_g faced to the ray d, n_s faced by its own cosine, the lifted point Po) at the hits P of the triangles prim"""
        _, e1, e2 = self.tris
        ng = np.cross(e1[prim], e2[prim])
        ng = ng / np.linalg.norm(ng, axis=1, keepdims=True)
        ng = np.where(((ng * d).sum(1) > 0)[:, None], -ng, ng)
        Po = P + ng * ((1.0 + np.abs(P).max(1)) * EPS)[:, None]
        if self.vn is None:
            return ng, ng, Po
        idx = self.tri_idx[prim]
        wa, wb, wc = bf._barycentric(self.verts, idx, P)
        ni = wa[:, None] * self.vn[idx[:, 0]] + wb[:, None] * self.vn[idx[:, 1]] + wc[:, None] * self.vn[idx[:, 2]]
        nil = np.linalg.norm(ni, axis=1)
        use = self.flags[self.tri_shape[prim]] & (nil > 0)
        ni = ni / np.where(nil > 0, nil, 1.0)[:, None]
        if self.swap != "ns_not_refaced":
            ni = np.where(((ni * d).sum(1) > 0)[:, None], -ni, ni)
        return ng, np.where(use[:, None], ni, ng), Po

    def rows(self, mats, P, prim, v=1, base_tex=None):
        """the material rows of the hits; a textured row's base colour (column 15 = 1 + texture index) is its texture at the interpolated uv"""
        rows = mats[self.tri_shape[prim]]
        base_tex = self.base_tex if base_tex is None else base_tex
        if base_tex is None or rows.shape[1] != 16 or (self.swap == "texture_at_vertex_1_only" and v > 1):
            return rows
        rows = rows.copy()
        idx = self.tri_idx[prim]
        wa, wb, wc = bf._barycentric(self.verts, idx, P)
        uv = wa[:, None] * self.vert_uv[idx[:, 0]] + wb[:, None] * self.vert_uv[idx[:, 1]] + wc[:, None] * self.vert_uv[idx[:, 2]]
        for k, tex in enumerate(base_tex):
            sel = rows[:, 15] == k + 1
            if sel.any():
                rows[sel, :3] = bf.sample_texture(tex, uv[sel, 0], uv[sel, 1])
        return rows


class Vertex:
    """one vertex of every live sample's path: v (1 = the primary hit), idx (the sample indices), beta [n, 3], P, ng, ns, Po, d (the ray that found
    it), rows (the material rows under their textures), shape, prim, tris (the scene's triangles, for shadow rays)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def walk(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth=5, use_jitter=True, *, smooth=None, vert_uv=None, base_tex=None,
         mats0=None, base_tex0=None, swap=None):
    """the walk of DESIGN.md 4.4 without any emitter: yields a Vertex per v = 1 .. max_depth - 1.  mats0 (tests/ref_prb.py's frozen roulette): the
    survival decisions and q_v come from the throughput of the rows mats0 (under base_tex0 where given), the yielded one is that of mats"""
    mats = np.asarray(mats, np.float64)
    frozen = mats0 is not None
    mats0 = np.asarray(mats0, np.float64) if frozen else None
    surf = Surface(verts, tri_idx, tri_shape, smooth, vert_uv, base_tex, swap)
    key = path_key(seed)
    o, d, nt, ft = bf.camera_rays(sd.cam, spp, use_jitter, seed)
    idx = np.arange(len(d), dtype=np.uint64)
    beta, beta0 = np.ones((len(d), 3)), np.ones((len(d), 3))
    for v in range(1, max_depth):
        t, prim = bf.intersect(o, d, surf.tris, nt, ft)
        hit = prim >= 0
        idx, o, d, beta, beta0, t, prim = idx[hit], o[hit], d[hit], beta[hit], beta0[hit], t[hit], prim[hit]
        if len(idx) == 0:
            return
        P = o + t[:, None] * d
        ng, ns, Po = surf.frame(P, d, prim)
        rows = surf.rows(mats, P, prim, v)
        yield Vertex(v=v, idx=idx, beta=beta.copy(), P=P, ng=ng, ns=ns, Po=Po, d=d, rows=rows, shape=surf.tri_shape[prim], prim=prim, tris=surf.tris)
        if v + 1 >= max_depth:
            return
        wo = cosine_dir(ng if swap == "bounce_about_ng" else ns, path_u(key, idx, v, 0), path_u(key, idx, v, 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            cos_o = (ns * wo).sum(1)[:, None]
            beta = beta * (np.pi * bf.bsdf_cos(rows, ns, -d, wo) / cos_o)
            beta0 = beta0 * (np.pi * bf.bsdf_cos(surf.rows(mats0, P, prim, v, base_tex0), ns, -d, wo) / cos_o) if frozen else beta
        bmax = beta0.max(1)
        keep = bmax > 0
        if swap != "no_ng_wo_test":
            keep &= (ng * wo).sum(1) > 0
        if v >= rr_depth:
            q = np.minimum(bmax, 0.95)
            keep &= path_u(key, idx, v, 2) < q
            qs = np.where(keep, q, 1.0)[:, None]
            beta, beta0 = beta / qs, beta0 / qs
        idx, o, d, beta, beta0 = idx[keep], Po[keep], wo[keep], beta[keep], beta0[keep]
        nt, ft = np.zeros(len(idx)), np.full(len(idx), np.inf)


def _emitters(sd, tris, rows, P, ng, ns, Po, d, swap=None):
    """next-event estimation at the points P (geometric normal ng and shading normal ns, each faced as Surface.frame says; lifted origins Po) —
    ref_bruteforce's _shade_terms for arbitrary rays: projector factor per channel (BSDF included), bilinear taps and weights, spot radiance"""
    N = len(P)
    n = ng if swap == "emitter_cosine_from_ng" else ns  # (the normal of the cosines and of the BSDF's frame)
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
        if swap != "no_geometric_side":
            lit &= (ng * wi).sum(1) > 0
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
        if swap != "no_geometric_side":
            lit &= (ng * wi).sum(1) > 0
        if sd.shadows and lit.any():
            sel = np.where(lit)[0]
            lit[sel[bf.any_hit(np.broadcast_to(spos, (len(sel), 3)), Po[sel] - spos, tris, 1.0 - 10.0 * EPS)]] = False
        f = np.where(lit[:, None], (fall / d2)[:, None] * bf.bsdf_cos(rows, n, -d, wi), 0.0)
        out["spot"] = f * np.asarray(list(sd.spot.intensity), np.float64)[None]
    return out


def path_vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth=5, **shading):
    """every vertex of every sample's path: a list of (sample indices, throughput [n,3], _emitters' terms and "shape": the hit shapes) in vertex
    order.  shading: walk's smooth, vert_uv, base_tex, mats0, base_tex0 and swap"""
    out = []
    for x in walk(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, **shading):
        e = _emitters(sd, x.tris, x.rows, x.P, x.ng, x.ns, x.Po, x.d, shading.get("swap"))
        e["shape"] = x.shape  # (the shape every sample's vertex lies on)
        out.append((x.idx, x.beta, e))
    return out


def _tex_value(sd, tex, e):
    (x0, x1, y0, y1), (w00, w01, w10, w11) = e["taps"], e["w"]
    tex = np.asarray(tex, np.float64)
    if tex.ndim == 2 or tex.shape[-1] == 1:
        t2 = tex.reshape(tex.shape[0], tex.shape[1])
        tv = w00 * t2[y0, x0] + w01 * t2[y0, x1] + w10 * t2[y1, x0] + w11 * t2[y1, x1]
        return tv[:, None] * np.asarray(list(sd.proj.color), np.float64)[None]
    return w00[:, None] * tex[y0, x0] + w01[:, None] * tex[y0, x1] + w10[:, None] * tex[y1, x0] + w11[:, None] * tex[y1, x1]


def sample_radiance(verts, tri_idx, tri_shape, sd, mats, tex, spp, seed, max_depth, rr_depth=5, **shading):
    """[W*H*spp, 3]: every sample's path radiance (shading: path_vertices')"""
    L = np.zeros((sd.cam.width * sd.cam.height * spp, 3))
    for idx, beta, e in path_vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, **shading):
        rad = e["spot"].copy()
        if sd.proj.enabled:
            rad += _tex_value(sd, tex, e) * e["pfac"]
        L[idx.astype(np.int64)] += beta * rad
    return L


def render_fwd(verts, tri_idx, tri_shape, sd, mats, tex, spp, seed, max_depth, rr_depth=5, gaussian_stddev=None, **shading):
    W, H = sd.cam.width, sd.cam.height
    L = sample_radiance(verts, tri_idx, tri_shape, sd, mats, tex, spp, seed, max_depth, rr_depth, **shading)
    if gaussian_stddev is not None:
        num, den, _ = bf._film_splat(W, H, spp, seed, gaussian_stddev, values=L)
        return np.where(den[..., None] > 0, num / np.where(den > 0, den, 1.0)[..., None], 0.0)
    return L.reshape(H, W, spp, 3).mean(2)


def render_bwd(verts, tri_idx, tri_shape, sd, mats, spp, seed, gimg, max_depth, rr_depth=5, gaussian_stddev=None, **shading):
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
    for idx, beta, e in path_vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, **shading):
        cw = q[idx.astype(np.int64)] * beta * e["pfac"]
        (x0, x1, y0, y1), ws = e["taps"], e["w"]
        for (yy, xx), w in zip(((y0, x0), (y0, x1), (y1, x0), (y1, x1)), ws):
            if tc == 1:
                np.add.at(gt[..., 0], (yy, xx), (cw * color[None]).sum(1) * w)
            else:
                for ch in range(3):
                    np.add.at(gt[..., ch], (yy, xx), cw[:, ch] * w)
    return gt
