"""Float64 restatement of the extra emitters — TEST INFRASTRUCTURE, built on tests/ref_bruteforce.py and tests/ref_path.py.

Written from DESIGN.md 4.7, not from the kernels: every ray against every triangle (no tree), the walk of DESIGN.md 4.4 (ref_path's random numbers,
cosine-weighted bounces, roulette), and at every vertex the n lights of a [n, 24] table (include/ffx.h FFX_RENDER_LIGHTS): direction and lit test,
the spot's falloff in the light's local frame, the shadow ray from the light to the lifted point, radiance beta I fall / d^2 (base A + B) / pi.
The walk is ref_path.walk: shading normals and base-colour textures as it states them (`shading`: its smooth, vert_uv, base_tex and swap); a light
must lie on the geometric side (n_g . wi > 0) and its cosine and the BSDF's frame are the shading normal's.  The image it returns is the lights'
part alone: the render is linear in the emitters.
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


def light_terms(row, tris, rows, P, ng, ns, Po, d, shadows, swap=None):
    """one light at the points P (geometric normal ng and shading normal ns as ref_path.Surface.frame faces them, lifted points Po, material rows
    `rows`): -> (radiance per channel [N,3] at throughput 1, {"faces": the lit test passed, "fall": the falloff, "occluded": the shadow ray hit})"""
    row = np.asarray(row, np.float64)
    n = ng if swap == "emitter_cosine_from_ng" else ns  # (the normal of the cosine and of the BSDF's frame)
    tw = row[:16].reshape(4, 4)
    Lk = tw[:3, 3]
    wi = Lk - P
    d2 = (wi * wi).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        wi = wi / np.sqrt(d2)[:, None]
    faces = (d2 > 0) & ((n * wi).sum(1) > 0)
    if swap != "no_geometric_side":
        faces &= (ng * wi).sum(1) > 0
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


def vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth=2, rr_depth=5, use_jitter=True, **shading):
    """ref_path.walk, the walk of DESIGN.md 4.4 without any emitter: yields (v, sample indices, throughput [n,3], P, ng, ns, Po, d, rows) per vertex
    v = 1 .. max_depth - 1"""
    for x in rp.walk(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, use_jitter, **shading):
        yield x.v, x.idx, x.beta, x.P, x.ng, x.ns, x.Po, x.d, x.rows


def sample_radiance(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth=2, rr_depth=5, use_jitter=True, stats=None, **shading):
    """[W*H*spp, 3]: what the lights of the [n, 24] table add to every sample.  stats (a dict): per light k the counts over all vertices of the
    samples that face it ("faces"), of those with a positive falloff ("lit") and of those whose shadow ray hit ("occluded"), and "min_fall"; under
    "direct" the part of L that comes from vertex 1"""
    lights = np.asarray(lights, np.float64).reshape(-1, 24)
    tris = bf.world_triangles(verts, tri_idx)
    L = np.zeros((sd.cam.width * sd.cam.height * spp, 3))
    direct = np.zeros_like(L)
    if stats is not None:
        stats.update({k: {"faces": 0, "lit": 0, "occluded": 0, "min_fall": np.inf} for k in range(len(lights))})
    for v, idx, beta, P, ng, ns, Po, d, rows in vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, use_jitter, **shading):
        for k, row in enumerate(lights):
            rad, info = light_terms(row, tris, rows, P, ng, ns, Po, d, bool(sd.shadows & 1), shading.get("swap"))
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


def render_lights(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth=2, rr_depth=5, gaussian_stddev=None, use_jitter=True, stats=None, **shading):
    """[H, W, 3]: the lights' part of the image — image(proj, spot, lights) - image(proj, spot)"""
    L = sample_radiance(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth, rr_depth, use_jitter, stats, **shading)
    return film(sd, L, spp, seed, gaussian_stddev)
