"""The oracle's Mitsuba half (K7 / K8 / K9, parity-unpinned against Mitsuba itself) against an independent
float64 brute-force restatement (tests/ref_bruteforce.py: no BVH, textbook Moller-Trumbore, written from
SURVEY App. A / DESIGN §4 and not from the oracle's source).  Removes the "same author, same mistake" hole between
the oracle and the HIP kernels; it cannot replace Mitsuba."""
import ctypes as C

import numpy as np
import pytest

from fireflies_amd import _abi, scene_desc, scenes
from tests import ref_bruteforce as bf
from tests.support import material_rows


def _world(sc, frame=0, xforms=None):
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    S = len(sc.meshes)
    xf = np.tile(np.eye(4, dtype=np.float32), (S, 1, 1)) if xforms is None else xforms
    offs = (off + np.minimum(frame, nfr - 1) * stride).astype(np.int32)
    verts = pool.astype(np.float64).copy()
    gidx = tris + offs[shape][:, None]
    for s in range(S):
        used = np.unique(gidx[shape == s])
        verts[used] = pool[used].astype(np.float64) @ xf[s][:3, :3].T.astype(np.float64) + xf[s][:3, 3]
    return pool, tris, shape, off, offs, xf, alb, verts, gidx


def _xf(S, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(S):
        a = rng.uniform(-0.15, 0.15)
        R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
        T = np.eye(4)
        T[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        out.append(T @ R @ np.diag([rng.uniform(0.8, 1.2), 1.0, 1.0, 1.0]))
    return np.asarray(out, np.float32)


@pytest.mark.parametrize("which", ["hello_world", "vocalfold"])
def test_oracle_agrees_with_an_independent_bruteforce_restatement(oracle, which):
    if which == "hello_world":
        sc, spp, xf, frame = scenes.hello_world(48, 40), 2, None, 0
    else:
        sc, spp, frame = scenes.vocalfold(width=24, height=24, tex=32, frames=3, n_fold=12, tube=(12, 16)), 4, 1
        xf = _xf(len(sc.meshes), 3)
    pool, tris, shape, off, offs, xf, alb, verts, gidx = _world(sc, frame, xf)
    go = oracle.Geometry(pool, tris, shape, off)
    go.update(xf, offs)
    cam = scene_desc.camera_from_sensor(sc.camera)
    # ---- K7: depth and ids, un-jittered and jittered
    for jit in (0, 1):
        t_o, s_o, p_o = go.trace_primary(cam, spp, jit, seed=5)
        t_b, s_b, p_b = bf.trace_primary(verts, gidx, shape, cam, spp, bool(jit), 5)
        same = (p_o == p_b) & (s_o == s_b)
        assert same.mean() >= 0.998, f"{which} jitter={jit}: {1 - same.mean():.2e} of the rays hit a different primitive"
        assert (p_o >= 0).mean() > 0.3
        np.testing.assert_allclose(t_o[same], t_b[same], rtol=2e-5, atol=2e-6)
    # ---- K8: radiance
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    rng = np.random.default_rng(1)
    if sc.projector is not None:
        tex = rng.random((sc.projector.height, sc.projector.width)).astype(np.float32)
    else:
        tex = np.zeros((1, 1), np.float32)
    img_o = go.render_fwd(sd, alb, tex, spp, seed=9)
    img_b = bf.render_fwd(verts, gidx, shape, sd, alb, tex, spp, 9)
    scale = float(img_b.max())
    assert scale > 0.01
    err = np.abs(img_o - img_b)
    # fp32 vs fp64: a sample on an edge (hit or shadow test) can flip: allow 1 % of the pixels an outlier of <= 1.5 / spp
    assert (err > 2e-4 * scale).mean() <= 1e-2, f"{which}: {(err > 2e-4 * scale).mean():.3f} of the pixel channels differ"
    assert err.max() <= 1.5 * scale / spp
    assert abs(float(img_o.mean()) - float(img_b.mean())) <= 2e-3 * float(img_b.mean())
    # without shadows too (the shadow test is the part most sensitive to the lifted origin)
    sd0 = scene_desc.scene_desc(sc, tex_channels=1, shadows=False)
    e0 = np.abs(go.render_fwd(sd0, alb, tex, spp, seed=9) - bf.render_fwd(verts, gidx, shape, sd0, alb, tex, spp, 9))
    assert (e0 > 2e-4 * scale).mean() <= 1e-2 and e0.max() <= 1.5 * scale / spp
    # ---- K9: texture gradient
    if sc.projector is not None:
        gimg = rng.standard_normal((sc.camera.height, sc.camera.width, 3)).astype(np.float32)
        gt_o = go.render_bwd(sd, alb, spp, 9, gimg)[..., 0]
        gt_b = bf.render_bwd(verts, gidx, shape, sd, alb, spp, 9, gimg)
        gs = float(np.abs(gt_b).max())
        assert gs > 0
        gerr = np.abs(gt_o - gt_b)
        assert (gerr > 1e-3 * gs).mean() <= 1e-2 and gerr.max() <= 0.5 * gs
        # the adjoint identity ties K8 and K9 together in the brute-force version itself
        base = bf.render_fwd(verts, gidx, shape, sd, alb, np.zeros_like(tex), spp, 9)
        lhs = float(((img_b - base) * gimg).sum())
        rhs = float((tex.astype(np.float64) * gt_b).sum())
        assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs), 1e-12)


def _oracle_material_eval(oracle, row, n, wv, wl):
    fn = oracle.api().lib.ffx_oracle_material_eval
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 1 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    row = np.ascontiguousarray(row, np.float32)
    n, wv, wl = (np.ascontiguousarray(a, np.float32) for a in (n, wv, wl))
    ab = np.zeros((n.shape[0], 2), np.float32)
    assert fn(row.ctypes.data, row.size, n.ctypes.data, wv.ctypes.data, wl.ctypes.data, n.shape[0], ab.ctypes.data) == 0
    return ab


def _dirs(k, seed):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((k, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)

    def hemi():
        v = rng.standard_normal((k, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        c = (v * n).sum(1, keepdims=True)
        v = np.where(c < 0, v - 2 * c * n, v)  # mirrored into the normal's hemisphere
        return v

    return n.astype(np.float32), hemi().astype(np.float32), hemi().astype(np.float32)


def test_principled_bsdf_closed_forms(oracle):
    """known answers of the principled model at normal incidence and its energy-free limits"""
    n = np.array([[0.0, 0.0, 1.0]], np.float32)
    # wi = wo = n: Schlick weights vanish -> diffuse lobe is exactly Lambert's base/pi; the GGX lobe is F0 / (4 pi alpha^2)
    rough, specular = 0.5, 0.5
    eta = 2.0 / (1.0 - np.sqrt(0.08 * specular)) - 1.0  # 1.5
    row = material_rows(1, 0, roughness=rough, anisotropic=0.0, metallic=0.0, spec_trans=0.0, eta=eta, spec_tint=0.0, sheen=0.0, sheen_tint=0.0,
                        flatness=0.0, clearcoat=0.0, clearcoat_gloss=0.0)[0]
    ab = _oracle_material_eval(oracle, row, n, n, n)[0]
    F0 = ((eta - 1) / (eta + 1)) ** 2
    assert ab[0] == pytest.approx(1.0, rel=1e-6)  # pi * (1/pi) * cos
    assert ab[1] == pytest.approx(np.pi * F0 / (4 * np.pi * rough**4), rel=1e-5)
    # specular = 0 -> eta = 1: no specular lobe at all (index-matched), whatever the roughness
    row0 = row.copy()
    row0[_abi.MAT_ETA] = 1.0
    nn, wv, wl = _dirs(64, 1)
    ab0 = _oracle_material_eval(oracle, row0, nn, wv, wl)
    assert np.all(ab0[:, 1] == 0)
    # metallic = 1 kills diffuse and sheen: A carries only base * (1 - Schlick weight) of the metal's Fresnel term
    rowm = row.copy()
    rowm[_abi.MAT_METALLIC] = 1.0
    abm = _oracle_material_eval(oracle, rowm, n, n, n)[0]
    assert abm[0] == pytest.approx(np.pi / (4 * np.pi * rough**4), rel=1e-5) and abs(abm[1]) < 1e-7
    # Lambert rows and 3-float rows: A = cos_o, B = 0
    lam = material_rows(1, 0, model=0.0)[0]
    abl = _oracle_material_eval(oracle, lam, nn, wv, wl)
    np.testing.assert_allclose(abl[:, 0], (nn * wl).sum(1), rtol=1e-6, atol=1e-7)
    assert np.all(abl[:, 1] == 0)
    # below the horizon on either side: nothing
    down = -n
    assert np.all(_oracle_material_eval(oracle, row, n, n, down) == 0) and np.all(_oracle_material_eval(oracle, row, n, down, n) == 0)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_principled_bsdf_matches_the_rgb_restatement(oracle, seed):
    """base_color * A + B of the oracle against the lobe-by-lobe RGB evaluation of tests/ref_bruteforce.py (float64)"""
    k = 4000
    n, wv, wl = _dirs(k, 10 + seed)
    fixed = [{}, {"anisotropic": 0.0, "clearcoat": 0.0, "sheen": 0.0, "flatness": 0.0, "spec_tint": 0.0},
             {"metallic": 0.0, "spec_trans": 0.0}, {"eta": 1.0}][seed]
    row = material_rows(1, seed, **fixed)[0]
    ab = _oracle_material_eval(oracle, row, n, wv, wl).astype(np.float64)
    got = (row[None, :3].astype(np.float64) * ab[:, :1] + ab[:, 1:2]) / np.pi
    want = bf.bsdf_cos(np.repeat(row[None].astype(np.float64), k, 0), n.astype(np.float64), wv.astype(np.float64), wl.astype(np.float64))
    assert want.max() > 0.05
    np.testing.assert_allclose(got, want, rtol=3e-4, atol=1e-6)


def test_oracle_render_with_principled_materials_agrees_with_bruteforce(oracle):
    sc, spp, frame = scenes.vocalfold(width=24, height=24, tex=32, frames=3, n_fold=12, tube=(12, 16)), 4, 1
    xf = _xf(len(sc.meshes), 3)
    pool, tris, shape, off, offs, xf, alb, verts, gidx = _world(sc, frame, xf)
    go = oracle.Geometry(pool, tris, shape, off)
    go.update(xf, offs)
    mats = material_rows(len(sc.meshes), 7)
    mats[-1, _abi.MAT_MODEL] = 0.0  # one Lambert shape among the principled ones
    rng = np.random.default_rng(1)
    tex = rng.random((sc.projector.height, sc.projector.width)).astype(np.float32)
    for shadows in (True, False):
        sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows)
        sd.mat_stride = _abi.MAT_STRIDE
        img_o = go.render_fwd(sd, mats, tex, spp, seed=9)
        img_b = bf.render_fwd(verts, gidx, shape, sd, mats, tex, spp, 9)
        scale = float(img_b.max())
        err = np.abs(img_o - img_b)
        assert scale > 0.01
        assert (err > 5e-4 * scale).mean() <= 1e-2 and err.max() <= 1.5 * scale / spp
        assert abs(float(img_o.mean()) - float(img_b.mean())) <= 2e-3 * float(img_b.mean())
    # the Lambert image differs: the materials do something
    sd3 = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    assert np.abs(go.render_fwd(sd3, mats[:, :3].copy(), tex, spp, seed=9) - img_b).max() > 0.02 * scale
    # K9 (replay and cached) with material rows
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    sd.mat_stride = _abi.MAT_STRIDE
    gimg = rng.standard_normal((sc.camera.height, sc.camera.width, 3)).astype(np.float32)
    gt_o = go.render_bwd(sd, mats, spp, 9, gimg)[..., 0]
    gt_b = bf.render_bwd(verts, gidx, shape, sd, mats, spp, 9, gimg)
    gs = float(np.abs(gt_b).max())
    gerr = np.abs(gt_o - gt_b)
    assert gs > 0 and (gerr > 1e-3 * gs).mean() <= 1e-2 and gerr.max() <= 0.5 * gs
    img_c, cache = go.render_fwd_cache(sd, mats, tex, spp, seed=9)
    np.testing.assert_array_equal(img_c, go.render_fwd(sd, mats, tex, spp, seed=9))
    gt_c = go.render_bwd_cached(sd, mats, cache, spp, gimg)[..., 0]
    np.testing.assert_allclose(gt_c, gt_o, rtol=1e-5, atol=1e-6 * gs)


def test_vertex_normals_of_a_sphere_are_radial_and_match_the_float64_restatement(oracle):
    """ffx_smooth: the update re-derives angle-weighted vertex normals from the posed vertices [EXT Mitsuba
    recompute_vertex_normals].  Closed form: on a tessellated sphere they point along the radius (to the tessellation's
    accuracy), also after a rigid motion and a uniform scale; under a NON-uniform scale they follow the deformed surface
    (normal ~ M^-T r), which is why they are recomputed from positions and not transformed.  And the oracle's float32 values
    (asin-based unit_angle) equal the float64 restatement (arccos) of tests/ref_bruteforce.py."""
    v, t = scenes.make_uv_sphere((0.0, 0.0, 0.0), 1.0, 24, 12)
    pool, tris = v.astype(np.float32), t.astype(np.int32)
    shape, off = np.zeros(len(tris), np.int32), np.zeros(1, np.int32)
    go = oracle.Geometry(pool, tris, shape, off, smooth=[True])
    a = 0.7
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    T = np.eye(4)
    T[:3, 3] = (0.3, -0.2, 2.0)
    for M in (np.eye(4), T @ R @ np.diag([1.7, 1.7, 1.7, 1.0]), T @ R @ np.diag([2.0, 1.0, 0.5, 1.0])):
        go.update(M.astype(np.float32)[None])
        body = np.abs(pool[:, 2]) < 0.99  # (the uv-sphere's pole rings are coincident vertices with zero-area faces: ill-defined)
        vn = go.vertex_normals.astype(np.float64)[body]
        world = pool.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        want = bf.vertex_normals(world, tris)[body]
        np.testing.assert_allclose(vn, want, rtol=0, atol=3e-6)
        expect = pool.astype(np.float64)[body] @ np.linalg.inv(M[:3, :3])  # rows: (M^-T r)^T
        expect /= np.linalg.norm(expect, axis=1, keepdims=True)
        ca = (vn * expect).sum(1)  # (the winding of make_uv_sphere decides inward or outward: one sign for the whole mesh)
        assert np.abs(ca).min() > 0.985 and (np.sign(ca) == np.sign(ca[0])).all()  # within the tessellation's accuracy (24 x 12 facets)
        np.testing.assert_allclose(np.linalg.norm(vn, axis=1), 1.0, atol=1e-6)
    # a flat shape next to a smooth one: rows exist, nothing is accumulated
    pool2 = np.concatenate([pool, pool + 3.0]).astype(np.float32)
    tris2, shape2 = np.concatenate([tris, tris]), np.concatenate([shape, shape + 1])
    g2 = oracle.Geometry(pool2, tris2, shape2, np.array([0, len(pool)], np.int32), smooth=[False, True])
    assert np.all(g2.vertex_normals[: len(pool)] == 0) and np.allclose(np.linalg.norm(g2.vertex_normals[len(pool):], axis=1), 1.0, atol=1e-6)


def test_oracle_render_with_interpolated_normals_agrees_with_bruteforce(oracle):
    """shading normals (SURVEY 8a a14 / VERDICT r2 missing 2): oracle vs the float64 brute force with per-shape flags — a
    smooth and a flat shape in one scene, Lambert and principled rows, shadows on and off, forward and adjoint; the image
    differs from the flat-shaded one and is smoother across facet edges."""
    sc, spp, frame = scenes.vocalfold(width=28, height=24, tex=32, frames=3, n_fold=12, tube=(12, 16)), 4, 1
    xf = _xf(len(sc.meshes), 5)
    pool, tris, shape, off, offs, xf, alb, verts, gidx = _world(sc, frame, xf)
    rng = np.random.default_rng(2)
    tex = rng.random((sc.projector.height, sc.projector.width)).astype(np.float32)
    mats = material_rows(len(sc.meshes), 9, anisotropic=0.0)
    for smooth in ([True, True], [False, True]):
        go = oracle.Geometry(pool, tris, shape, off, smooth=smooth)
        go.update(xf, offs)
        for rows, stride in ((alb, 0), (mats, _abi.MAT_STRIDE)):
            for shadows in (True, False):
                sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows)
                sd.mat_stride = stride
                img_o = go.render_fwd(sd, rows, tex, spp, seed=4)
                img_b = bf.render_fwd(verts, gidx, shape, sd, rows, tex, spp, 4, smooth=smooth)
                scale = float(img_b.max())
                err = np.abs(img_o - img_b)
                assert scale > 0.01
                assert (err > 5e-4 * scale).mean() <= 1e-2 and err.max() <= 1.5 * scale / spp, (smooth, stride, shadows, err.max() / scale)
                assert abs(float(img_o.mean()) - float(img_b.mean())) <= 2e-3 * float(img_b.mean())
        sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
        gimg = rng.standard_normal((sc.camera.height, sc.camera.width, 3)).astype(np.float32)
        gt_o = go.render_bwd(sd, alb, spp, 4, gimg)[..., 0]
        gt_b = bf.render_bwd(verts, gidx, shape, sd, alb, spp, 4, gimg, smooth=smooth)
        gs = float(np.abs(gt_b).max())
        gerr = np.abs(gt_o - gt_b)
        assert gs > 0 and (gerr > 1e-3 * gs).mean() <= 1e-2 and gerr.max() <= 0.5 * gs
        img_c, cache = go.render_fwd_cache(sd, alb, tex, spp, seed=4)
        gt_c = go.render_bwd_cached(sd, alb, cache, spp, gimg)[..., 0]
        np.testing.assert_allclose(gt_c, gt_o, rtol=1e-5, atol=1e-6 * gs)
    # flat shading is something else
    gf = oracle.Geometry(pool, tris, shape, off)
    gf.update(xf, offs)
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    flat = gf.render_fwd(sd, alb, tex, spp, seed=4)
    go = oracle.Geometry(pool, tris, shape, off, smooth=[True, True])
    go.update(xf, offs)
    smooth_img = go.render_fwd(sd, alb, tex, spp, seed=4)
    assert np.abs(flat - smooth_img).max() > 0.02 * float(flat.max())


@pytest.mark.parametrize("which", ["hello_world", "vocalfold"])
def test_gaussian_reconstruction_filter_oracle_agrees_with_bruteforce(oracle, which):
    """ffx_scene_desc.rfilter = gaussian (hdrfilm's default, which the reference's scenes get): the oracle's two-level sums
    (a pixel's own samples per window entry, then the 25 incoming sums) against the brute force's film formed from absolute sample
    positions and pixel centres — image and texture gradient — plus: the means of the two films agree (weights normalised), the adjoint
    identity holds inside the brute force and in the oracle, the filtered image differs from the box image (the field is actually
    read), a narrower filter, the fp16 film, and the box-only entry points refuse the scene."""
    if which == "hello_world":
        sc, spp, xf, frame = scenes.hello_world(40, 32), 3, None, 0
    else:
        sc, spp, frame = scenes.vocalfold(width=24, height=20, tex=32, frames=3, n_fold=12, tube=(12, 16)), 5, 1
        xf = _xf(len(sc.meshes), 4)
    pool, tris, shape, off, offs, xf, alb, verts, gidx = _world(sc, frame, xf)
    go = oracle.Geometry(pool, tris, shape, off)
    go.update(xf, offs)
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    rng = np.random.default_rng(2)
    tex = rng.random((sc.projector.height, sc.projector.width)).astype(np.float32) if sc.projector is not None else np.zeros((1, 1), np.float32)
    img_box = go.render_fwd(sd, alb, tex, spp, seed=11)
    sd.rfilter, sd.rfilter_stddev = _abi.RFILTER_GAUSSIAN, 0.0  # (0: the default, 0.5)
    img_o = go.render_fwd(sd, alb, tex, spp, seed=11)
    img_b = bf.render_fwd(verts, gidx, shape, sd, alb, tex, spp, 11, gaussian_stddev=0.5)
    scale = float(img_b.max())
    assert scale > 0.01 and float(np.abs(img_o - img_box).max()) > 0.02 * scale
    err = np.abs(img_o - img_b)
    # (a sample that flips on an edge now spreads over its 5x5 window: a few more pixels carry a part of it)
    assert (err > 3e-4 * scale).mean() <= 5e-2, f"{which}: {(err > 3e-4 * scale).mean():.3f} of the pixel channels differ"
    assert err.max() <= 1.5 * scale / spp
    assert abs(float(img_o.mean()) - float(img_b.mean())) <= 2e-3 * float(img_b.mean())
    # a narrower filter too (stddev 0.3: radius 1.2, window entries at distance 2 get no weight)
    sd.rfilter_stddev = 0.3
    e3 = np.abs(go.render_fwd(sd, alb, tex, spp, seed=11) - bf.render_fwd(verts, gidx, shape, sd, alb, tex, spp, 11, gaussian_stddev=0.3))
    assert (e3 > 3e-4 * scale).mean() <= 5e-2 and e3.max() <= 1.5 * scale / spp
    sd.rfilter_stddev = 0.5
    # the fp16 film rounds the filtered value once
    np.testing.assert_array_equal(go.render_fwd(sd, alb, tex, spp, seed=11, fp16=True), img_o.astype(np.float16))
    if sc.projector is None:
        return
    gimg = rng.standard_normal((sc.camera.height, sc.camera.width, 3)).astype(np.float32)
    gt_o = go.render_bwd(sd, alb, spp, 11, gimg)[..., 0]
    gt_b = bf.render_bwd(verts, gidx, shape, sd, alb, spp, 11, gimg, gaussian_stddev=0.5)
    gs = float(np.abs(gt_b).max())
    assert gs > 0
    gerr = np.abs(gt_o - gt_b)
    assert (gerr > 1e-3 * gs).mean() <= 2e-2 and gerr.max() <= 0.5 * gs
    base = bf.render_fwd(verts, gidx, shape, sd, alb, np.zeros_like(tex), spp, 11, gaussian_stddev=0.5)
    lhs, rhs = float(((img_b - base) * gimg).sum()), float((tex.astype(np.float64) * gt_b).sum())
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs), 1e-12)
    # ... and in the oracle (float32: looser)
    base_o = go.render_fwd(sd, alb, np.zeros_like(tex), spp, seed=11).astype(np.float64)
    lhs_o, rhs_o = float(((img_o - base_o) * gimg).sum()), float((tex.astype(np.float64) * gt_o).sum())
    assert abs(lhs_o - rhs_o) <= 2e-4 * max(abs(lhs_o), abs(rhs_o))
    # the filtered film's adjoint cache (ABI 7): the same image, and from its records — no tracing — the re-traced adjoint's gradient
    # (same arithmetic, same order of the double sums: bit for bit)
    img_c, cache = go.render_fwd_cache(sd, alb, tex, spp, seed=11)
    np.testing.assert_array_equal(img_c, img_o)
    np.testing.assert_array_equal(go.render_bwd_cached(sd, alb, cache, spp, gimg, seed=11)[..., 0], gt_o)
    assert not np.array_equal(go.render_bwd_cached(sd, alb, cache, spp, gimg, seed=12)[..., 0], gt_o)  # (the weights come from the seed's jitter)
    # every box-only render call refuses the filter instead of rendering a box
    import ctypes as C

    a = oracle.api()
    cbuf, ibuf = np.zeros(a.lib.ffx_render_cache_bytes_sd(C.byref(sd), spp), np.uint8), np.zeros((sc.camera.height, sc.camera.width, 3), np.float32)
    albc, texc = np.ascontiguousarray(alb, np.float32), np.ascontiguousarray(tex, np.float32)
    rc = a.lib.ffx_render_fwd_cache(go.blob.ctypes.data, C.byref(go.info), C.byref(sd), albc.ctypes.data, texc.ctypes.data, spp, 11, 0, ibuf.ctypes.data, cbuf.ctypes.data, None)
    assert rc == -3 and b"reconstruction filter" in a.lib.ffx_last_error()
