"""Float64 restatement of the extra emitters — TEST INFRASTRUCTURE, built on tests/ref_bruteforce.py and tests/ref_path.py.

Written from DESIGN.md 4.7, not from the kernels: every ray against every triangle (no tree), the walk of DESIGN.md 4.4 (ref_path's random numbers,
cosine-weighted bounces, roulette), and at every vertex the n lights of a [n, 24] table (include/ffx.h FFX_RENDER_LIGHTS): direction and lit test,
the spot's falloff in the light's local frame, the shadow ray from the light to the lifted point, radiance beta I fall / d^2 (base A + B) / pi.
Flat-shaded scenes without base-colour textures (ng = ns).  The image it returns is the lights' part alone: the render is linear in the emitters.
"""
import numpy as np

from tests import ref_bruteforce as bf
from tests import ref_path as rp

EPS = bf.EPS
TYPE_POINT, TYPE_SPOT = 0.0, 1.0


def table_row(kind, to_world, intensity, cutoff_deg=20.0, beam_width_deg=15.0):
    """one record of the table in float64: to_world 0..15 row-major, intensity 16..18, cutoff 19, beam width 20, type 21, 22..23 zero"""
    r = np.zeros(24)
    r[:16] = np.asarray(to_world, np.float64).reshape(16)
    r[16:19] = np.asarray(intensity, np.float64)
    r[19], r[20], r[21] = cutoff_deg, beam_width_deg, TYPE_SPOT if kind == "spot" else TYPE_POINT
    return r


def light_terms(row, tris, rows, P, n, Po, d, shadows):
    """one light at the points P (normal n — geometric and shading — faced to the incoming direction d, lifted points Po, material rows `rows`):
    -> (radiance per channel [N,3] at throughput 1, {"faces": the lit test passed, "fall": the falloff, "occluded": the shadow ray hit})"""
    row = np.asarray(row, np.float64)
    tw = row[:16].reshape(4, 4)
    Lk = tw[:3, 3]
    wi = Lk - P
    d2 = (wi * wi).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        wi = wi / np.sqrt(d2)[:, None]
    faces = (d2 > 0) & ((n * wi).sum(1) > 0)  # (ns = ng here: both tests are this one)
    fall = np.ones(len(P))
    if row[21] != TYPE_POINT:
        local = (-wi) @ np.linalg.inv(tw[:3, :3]).T
        with np.errstate(divide="ignore", invalid="ignore"):
            ang = np.arccos(np.clip(local[:, 2] / np.linalg.norm(local, axis=1), -1.0, 1.0))
        cutoff, beam = np.deg2rad(row[19]), np.deg2rad(row[20])
        fall = np.where(ang <= beam, 1.0, np.where(ang < cutoff, (cutoff - ang) / (cutoff - beam), 0.0))
    lit = faces & (fall > 0)
    occluded = np.zeros(len(P), bool)
    if shadows and lit.any():
        sel = np.where(lit)[0]
        occluded[sel] = bf.any_hit(np.broadcast_to(Lk, (len(sel), 3)), Po[sel] - Lk, tris, 1.0 - 10.0 * EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (fall / d2)[:, None] * bf.bsdf_cos(rows, n, -d, wi)  # (bsdf_cos = (base A + B) / pi, A = n . wi and B = 0 for a Lambert row)
    rad = np.where((lit & ~occluded)[:, None], f, 0.0) * row[16:19][None]
    return rad, {"faces": faces, "fall": fall, "occluded": occluded}


def vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth=2, rr_depth=5, use_jitter=True):
    """the walk of DESIGN.md 4.4 without any emitter: yields (v, sample indices, throughput [n,3], P, n, Po, d, rows) per vertex v = 1 .. max_depth - 1"""
    mats = np.asarray(mats, np.float64)
    tris = bf.world_triangles(verts, tri_idx)
    _, e1, e2 = tris
    key = rp.path_key(seed)
    o, d, nt, ft = bf.camera_rays(sd.cam, spp, use_jitter, seed)
    idx = np.arange(len(d), dtype=np.uint64)
    beta = np.ones((len(d), 3))
    for v in range(1, max_depth):
        t, prim = bf.intersect(o, d, tris, nt, ft)
        hit = prim >= 0
        idx, o, d, beta, t, prim = idx[hit], o[hit], d[hit], beta[hit], t[hit], prim[hit]
        if len(idx) == 0:
            return
        P = o + t[:, None] * d
        n = np.cross(e1[prim], e2[prim])
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(((n * d).sum(1) > 0)[:, None], -n, n)
        Po = P + n * ((1.0 + np.abs(P).max(1)) * EPS)[:, None]
        rows = mats[np.asarray(tri_shape)[prim]]
        yield v, idx, beta.copy(), P, n, Po, d, rows
        if v + 1 >= max_depth:
            return
        wo = rp.cosine_dir(n, rp.path_u(key, idx, v, 0), rp.path_u(key, idx, v, 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.pi * bf.bsdf_cos(rows, n, -d, wo) / (n * wo).sum(1)[:, None]
        beta = beta * f
        bmax = beta.max(1)
        keep = bmax > 0
        if v >= rr_depth:
            q = np.minimum(bmax, 0.95)
            keep &= rp.path_u(key, idx, v, 2) < q
            beta = beta / np.where(keep, q, 1.0)[:, None]
        idx, o, d, beta = idx[keep], Po[keep], wo[keep], beta[keep]
        nt, ft = np.zeros(len(idx)), np.full(len(idx), np.inf)


def sample_radiance(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth=2, rr_depth=5, use_jitter=True, stats=None):
    """[W*H*spp, 3]: what the lights of the [n, 24] table add to every sample.  stats (a dict): per light k the counts over all vertices of the
    samples that face it ("faces"), of those with a positive falloff ("lit") and of those whose shadow ray hit ("occluded"), and "min_fall"; under
    "direct" the part of L that comes from vertex 1"""
    lights = np.asarray(lights, np.float64).reshape(-1, 24)
    tris = bf.world_triangles(verts, tri_idx)
    L = np.zeros((sd.cam.width * sd.cam.height * spp, 3))
    direct = np.zeros_like(L)
    if stats is not None:
        stats.update({k: {"faces": 0, "lit": 0, "occluded": 0, "min_fall": np.inf} for k in range(len(lights))})
    for v, idx, beta, P, n, Po, d, rows in vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, use_jitter):
        for k, row in enumerate(lights):
            rad, info = light_terms(row, tris, rows, P, n, Po, d, bool(sd.shadows & 1))
            L[idx.astype(np.int64)] += beta * rad
            if v == 1:
                direct[idx.astype(np.int64)] += beta * rad
            if stats is not None:
                s = stats[k]
                s["faces"] += int(info["faces"].sum())
                s["lit"] += int((info["faces"] & (info["fall"] > 0)).sum())
                s["occluded"] += int(info["occluded"].sum())
                if info["faces"].any():
                    s["min_fall"] = min(s["min_fall"], float(info["fall"][info["faces"]].min()))
    if stats is not None:
        stats["direct"] = direct
    return L


def film(sd, L, spp, seed, gaussian_stddev=None):
    W, H = sd.cam.width, sd.cam.height
    if gaussian_stddev is not None:
        num, den, _ = bf._film_splat(W, H, spp, seed, gaussian_stddev, values=L)
        return np.where(den[..., None] > 0, num / np.where(den > 0, den, 1.0)[..., None], 0.0)
    return L.reshape(H, W, spp, 3).mean(2)


def render_lights(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth=2, rr_depth=5, gaussian_stddev=None, use_jitter=True, stats=None):
    """[H, W, 3]: the lights' part of the image — image(proj, spot, lights) - image(proj, spot)"""
    L = sample_radiance(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth, rr_depth, use_jitter, stats)
    return film(sd, L, spp, seed, gaussian_stddev)
