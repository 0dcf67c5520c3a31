"""Float64 restatement of the directional emitter — TEST INFRASTRUCTURE, built on tests/ref_lights.py's walk (ref_path's
random numbers, cosine-weighted bounces, roulette) and tests/ref_bruteforce.py's every-ray-against-every-triangle intersection.

Written from DESIGN.md 4.9, not from the kernels.  A record of type 2 in a [n, 24] table (include/ffx.h FFX_LIGHT_DIRECTIONAL): the direction of travel
is to_world's 3 x 3 applied to (0, 0, 1), normalised; wi = -dir at every vertex; the vertex is lit when the faced normal sees wi; with shadows one ray
from the lifted point along wi over (0, 3e38), occluded iff it hits anything; radiance beta E (base A + B) / pi — no falloff, no 1 / d^2.  Records of
the other types are ref_lights'.  Shading normals and base-colour textures are ref_path.walk's (`shading`: its smooth, vert_uv, base_tex and swap): the
sun must lie on the geometric side (n_g . wi > 0), its cosine and the BSDF's frame are the shading normal's.  The image it returns is the table's
part alone.
"""
import numpy as np

from tests import ref_bruteforce as bf
from tests import ref_lights as rl

TYPE_DIRECTIONAL = 2.0
T_MAX = 3.0e38


def table_row(to_world, irradiance):
    """one directional record in float64: to_world 0..15 row-major, irradiance 16..18, type 21 = 2, zeros elsewhere"""
    r = np.zeros(24)
    r[:16] = np.asarray(to_world, np.float64).reshape(16)
    r[16:19] = np.asarray(irradiance, np.float64)
    r[21] = TYPE_DIRECTIONAL
    return r


def direction(row):
    """the direction of travel of a record, or None where the frame's +Z does not normalise to a finite unit vector"""
    z = np.asarray(row, np.float64)[:16].reshape(4, 4)[:3, 2]
    with np.errstate(all="ignore"):
        d = z / np.sqrt((z * z).sum())
    return d if np.isfinite(d).all() and abs((d * d).sum() - 1.0) < 1e-6 else None


def sun_terms(row, tris, rows, P, ng, ns, Po, d, shadows, swap=None):
    """one directional record at the points P (geometric normal ng and shading normal ns as ref_path.Surface.frame faces them, lifted points Po,
    material rows): -> (radiance per channel [N,3] at throughput 1, {"faces": the lit test passed, "occluded": the shadow ray hit})"""
    N = len(P)
    n = ng if swap == "emitter_cosine_from_ng" else ns  # (the normal of the cosine and of the BSDF's frame)
    dir_ = direction(row)
    if dir_ is None:
        return np.zeros((N, 3)), {"faces": np.zeros(N, bool), "occluded": np.zeros(N, bool)}
    wi = np.broadcast_to(-dir_, (N, 3))
    faces = (n * wi).sum(1) > 0
    if swap != "no_geometric_side":
        faces &= (ng * wi).sum(1) > 0
    occluded = np.zeros(N, bool)
    if shadows and faces.any():
        sel = np.where(faces)[0]
        occluded[sel] = bf.any_hit(Po[sel], wi[sel], tris, T_MAX)
    f = bf.bsdf_cos(rows, n, -d, wi)  # (= (base A + B) / pi, A = n . wi and B = 0 for a Lambert row)
    rad = np.where((faces & ~occluded)[:, None], f, 0.0) * np.asarray(row, np.float64)[16:19][None]
    return rad, {"faces": faces, "occluded": occluded}


def sample_radiance(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth=2, rr_depth=5, use_jitter=True, stats=None, **shading):
    """[W*H*spp, 3]: what the records of the [n, 24] table — any of the three types — add to every sample.  stats (a dict): per record k the counts over
    all vertices of the samples that face it ("faces") and of those whose shadow ray hit ("occluded"); under "direct" the part from vertex 1"""
    lights = np.asarray(lights, np.float64).reshape(-1, 24)
    tris = bf.world_triangles(verts, tri_idx)
    L = np.zeros((sd.cam.width * sd.cam.height * spp, 3))
    direct = np.zeros_like(L)
    if stats is not None:
        stats.update({k: {"faces": 0, "occluded": 0} for k in range(len(lights))})
    for v, idx, beta, P, ng, ns, Po, d, rows in rl.vertices(verts, tri_idx, tri_shape, sd, mats, spp, seed, max_depth, rr_depth, use_jitter, **shading):
        for k, row in enumerate(lights):
            terms = sun_terms if row[21] == TYPE_DIRECTIONAL else rl.light_terms
            rad, info = terms(row, tris, rows, P, ng, ns, Po, d, bool(sd.shadows & 1), shading.get("swap"))
            L[idx.astype(np.int64)] += beta * rad
            if v == 1:
                direct[idx.astype(np.int64)] += beta * rad
            if stats is not None:
                stats[k]["faces"] += int(info["faces"].sum())
                stats[k]["occluded"] += int(info["occluded"].sum())
    if stats is not None:
        stats["direct"] = direct
    return L


def render_sun(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth=2, rr_depth=5, gaussian_stddev=None, use_jitter=True, stats=None, **shading):
    """[H, W, 3]: the table's part of the image — image(proj, spot, table) - image(proj, spot)"""
    L = sample_radiance(verts, tri_idx, tri_shape, sd, mats, lights, spp, seed, max_depth, rr_depth, use_jitter, stats, **shading)
    return rl.film(sd, L, spp, seed, gaussian_stddev)
