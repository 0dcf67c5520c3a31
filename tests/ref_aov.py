"""float64 restatement of the AOV block (include/ffx.h FFX_RENDER_AOV) on tests/ref_bruteforce.py's pieces: per sample the primary hit's
depth, position, geometric and shading normal (neither faced to the viewer), texture coordinates (not wrapped), base colour, shape and triangle id —
zeros for a miss — and the film over them: the box film's mean, or the gaussian film's sum(w a) / sum(w)."""
import numpy as np

from tests import ref_bruteforce as rb

FLOATS = 17
CHANNELS = {"depth": (0, 1), "position": (1, 3), "geo_normal": (4, 3), "sh_normal": (7, 3), "uv": (10, 2), "albedo": (12, 3), "shape_index": (15, 1),
            "prim_index": (16, 1)}


def trace(verts, tri_idx, cam, spp, seed):
    """the jittered camera rays of a render and their closest hits -> (o, d, nt, t, prim): the part of aov_samples that does not depend on materials,
    flags or texture coordinates (scenes that share geometry and camera share it)"""
    tris = rb.world_triangles(np.asarray(verts, np.float64), np.asarray(tri_idx))
    o, d, nt, ft = rb.camera_rays(cam, spp, True, seed)
    t, prim = rb.intersect(o, d, tris, nt, ft)
    return o, d, nt, t, prim


def aov_samples(verts, tri_idx, tri_shape, cam, spp, seed, mats, smooth=None, vert_uv=None, base_tex=None, traced=None):
    """-> [W * H * spp, 17], sample idx = (y W + x) spp + s as everywhere.  mats: [n_shapes, 3 | 16]; smooth: one flag per shape; vert_uv: [n_verts, 2]
    or None (uv 0); base_tex: list of [h, w, 3] for rows whose column 15 is 1 + index; traced: trace(...) of the same geometry, camera, spp and seed"""
    verts, tri_idx, tri_shape = np.asarray(verts, np.float64), np.asarray(tri_idx), np.asarray(tri_shape)
    mats = np.asarray(mats, np.float64)
    _, e1, e2 = rb.world_triangles(verts, tri_idx)
    o, d, nt, t, prim = traced if traced is not None else trace(verts, tri_idx, cam, spp, seed)
    hit = prim >= 0
    pr = np.maximum(prim, 0)
    t = np.where(hit, t, 0.0)
    P = o + t[:, None] * d
    ng = np.cross(e1[pr], e2[pr])
    nl = np.linalg.norm(ng, axis=1, keepdims=True)
    ng = ng / np.where(nl > 0, nl, 1.0)
    shape = tri_shape[pr]
    idx = tri_idx[pr]
    wa, wb, wc = rb._barycentric(verts, idx, P)
    ns = ng
    if smooth is not None and any(smooth):
        fl = np.asarray([bool(f) for f in smooth])
        vn = rb.vertex_normals(verts, tri_idx, use=fl[tri_shape])
        ni = wa[:, None] * vn[idx[:, 0]] + wb[:, None] * vn[idx[:, 1]] + wc[:, None] * vn[idx[:, 2]]
        nil = np.linalg.norm(ni, axis=1)
        use = fl[shape] & (nil > 0)
        ns = np.where(use[:, None], ni / np.where(nil > 0, nil, 1.0)[:, None], ng)
    uv = np.zeros((len(P), 2))
    if vert_uv is not None:
        uvs = np.asarray(vert_uv, np.float64)
        uv = wa[:, None] * uvs[idx[:, 0]] + wb[:, None] * uvs[idx[:, 1]] + wc[:, None] * uvs[idx[:, 2]]
    rows = mats[shape]
    albedo = rows[:, :3].copy()
    if base_tex is not None and rows.shape[1] == 16:
        for k, tex in enumerate(base_tex):
            sel = hit & (rows[:, 15] == k + 1)
            if sel.any():
                albedo[sel] = rb.sample_texture(tex, uv[sel, 0], uv[sel, 1])
    out = np.concatenate([(t - nt)[:, None], P, ng, ns, uv, albedo, shape[:, None].astype(np.float64), prim[:, None].astype(np.float64)], 1)
    assert out.shape[1] == FLOATS
    return np.where(hit[:, None], out, 0.0)


def film(a, cam, spp, seed, gaussian_stddev=None):
    """per-sample values [W * H * spp, k] through the film -> [H, W, k]: the box film's mean, or the gaussian film's sum(w a) / sum(w)"""
    W, H = cam.width, cam.height
    if gaussian_stddev is None:
        return a.reshape(H, W, spp, a.shape[1]).mean(2)
    num, den, _ = rb._film_splat(W, H, spp, seed, gaussian_stddev, values=a)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den[..., None] > 0, num / den[..., None], 0.0)


def aov_block(verts, tri_idx, tri_shape, cam, spp, seed, mats, smooth=None, vert_uv=None, base_tex=None, gaussian_stddev=None, traced=None):
    """-> [H, W, 17]: the samples through the film"""
    return film(aov_samples(verts, tri_idx, tri_shape, cam, spp, seed, mats, smooth, vert_uv, base_tex, traced), cam, spp, seed, gaussian_stddev)
