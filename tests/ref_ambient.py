"""Float64 restatement of the constant emitter — TEST INFRASTRUCTURE, built on tests/ref_bruteforce.py and tests/ref_path.py.

Written from DESIGN.md 4.8, not from the kernels: every ray against every triangle (no tree), the walk of DESIGN.md 4.4 (ref_path's random numbers,
cosine-weighted bounces, roulette) with its escapes reported, and the closing ray at the walk's last vertex.  A sample gains the radiance L_a
  - when its camera ray hits nothing in (nt, ft]                                                     (vertex 0: the background),
  - times the throughput behind the bounce at vertex v when that bounce's ray hits nothing in (0, inf) (vertex v; v + 1 < max_depth: the walk's own
    secondary ray, v + 1 = max_depth: the closing ray, an occlusion test along the bounce the walk would make).
Both normals and the base-colour textures are ref_path.Surface's (`shading`: ref_path.walk's smooth, vert_uv, base_tex and swap): the bounce — the
closing one included — is drawn about n_s, ends where n_g . wo <= 0 and weighs by pi f / (n_s . wo).  The image it returns is the emitter's part
alone: the render is linear in the emitters.

round32: every quantity the walk hands from one step to the next (ray origins and directions, lifted points, bounce weights, throughputs) is rounded
to float32 — a model of evaluating the same statement in single precision, for the test that the caps of the GPU comparison leave room for that.
"""
import numpy as np

from tests import ref_bruteforce as bf
from tests import ref_path as rp

EPS = bf.EPS


def _r(x, round32):
    return np.asarray(x, np.float32).astype(np.float64) if round32 else x


def sample_radiance(verts, tri_idx, tri_shape, sd, mats, radiance, spp, seed, max_depth=2, rr_depth=5, use_jitter=True, parts=None, round32=False, *,
                    smooth=None, vert_uv=None, base_tex=None, swap=None):
    """[W*H*spp, 3]: what the constant emitter of radiance (r, g, b) adds to every sample.  parts (a dict): vertex -> that vertex's share of the result
    (0: the background), and under "closing" the number of closing rays cast, under "escaped" the number of rays of any kind that hit nothing"""
    La = np.asarray(radiance, np.float64).reshape(3)
    mats = np.asarray(mats, np.float64)
    surf = rp.Surface(verts, tri_idx, tri_shape, smooth, vert_uv, base_tex, swap)
    tris = surf.tris
    key = rp.path_key(seed)
    o, d, nt, ft = bf.camera_rays(sd.cam, spp, use_jitter, seed)
    o, d = _r(o, round32), _r(d, round32)
    L = np.zeros((sd.cam.width * sd.cam.height * spp, 3))
    if parts is not None:
        parts.update({v: np.zeros_like(L) for v in range(max_depth)})
        parts["closing"] = parts["escaped"] = 0

    def gain(v, idx, beta):
        L[idx.astype(np.int64)] += beta * La[None]
        if parts is not None:
            parts[v][idx.astype(np.int64)] += beta * La[None]
            parts["escaped"] += len(idx)

    idx = np.arange(len(d), dtype=np.uint64)
    beta = np.ones((len(d), 3))
    for v in range(1, max_depth):
        t, prim = bf.intersect(o, d, tris, nt, ft)
        hit = prim >= 0
        gain(v - 1, idx[~hit], beta[~hit])  # (v = 1: the camera ray — the background; else the bounce ray of vertex v - 1, beta the throughput behind it)
        idx, o, d, beta, t, prim = idx[hit], o[hit], d[hit], beta[hit], t[hit], prim[hit]
        if len(idx) == 0:
            break
        P = _r(o + t[:, None] * d, round32)
        ng, ns, Po = surf.frame(P, d, prim)
        Po = _r(Po, round32)
        rows = surf.rows(mats, P, prim, v)
        # the bounce the walk makes, or would make, at this vertex: about n_s, alive on the geometric side
        wo = _r(rp.cosine_dir(ng if swap == "bounce_about_ng" else ns, rp.path_u(key, idx, v, 0), rp.path_u(key, idx, v, 1)), round32)
        cos_o = (ns * wo).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = _r(np.pi * bf.bsdf_cos(rows, ns, -d, wo) / cos_o[:, None], round32)
        keep = (ng * wo).sum(1) > 0 if swap != "no_ng_wo_test" else np.ones(len(idx), bool)
        nb = np.where(keep[:, None], beta * f, 0.0)
        bmax = nb.max(1)
        keep &= bmax > 0
        if v >= rr_depth:
            q = np.minimum(bmax, 0.95)
            keep &= rp.path_u(key, idx, v, 2) < q
            nb = nb / np.where(keep, q, 1.0)[:, None]
        idx, o, d, beta = idx[keep], Po[keep], wo[keep], _r(nb[keep], round32)
        nt, ft = np.zeros(len(idx)), np.full(len(idx), np.inf)
        if v + 1 >= max_depth:  # the closing ray: that bounce as an occlusion test
            free = ~bf.any_hit(o, d, tris, np.inf)
            if parts is not None:
                parts["closing"] += len(idx)
            gain(v, idx[free], beta[free])
    return L


def film(sd, L, spp, seed, gaussian_stddev=None):
    W, H = sd.cam.width, sd.cam.height
    if gaussian_stddev is not None:
        num, den, _ = bf._film_splat(W, H, spp, seed, gaussian_stddev, values=L)
        return np.where(den[..., None] > 0, num / np.where(den > 0, den, 1.0)[..., None], 0.0)
    return L.reshape(H, W, spp, 3).mean(2)


def render_ambient(verts, tri_idx, tri_shape, sd, mats, radiance, spp, seed, max_depth=2, rr_depth=5, gaussian_stddev=None, use_jitter=True, parts=None,
                   round32=False, **shading):
    """[H, W, 3]: the constant emitter's part of the image — image(main, lights, ambient) - image(main, lights)"""
    L = sample_radiance(verts, tri_idx, tri_shape, sd, mats, radiance, spp, seed, max_depth, rr_depth, use_jitter, parts, round32, **shading)
    return film(sd, L, spp, seed, gaussian_stddev)
