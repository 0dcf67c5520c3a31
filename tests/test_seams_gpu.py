"""Every walk of libffx_hip.so held to a TREE-FREE reference at seams (boxes can only be hit more often than in exact
arithmetic; the triangle test alone decides).  The references are the oracle in its tree_free() mode — every box test skipped — and
tie_scenes.tri_hit_all_pairs; tests/test_seams_cpu.py pins the one against the other and proves that the fixtures of
tests/seam_scenes.py produce the rays a box without an absolute pad term is never entered by.  NO ray is left out anywhere in this file.
Run with `-m gpu`."""
import numpy as np
import pytest
import torch

from fireflies_amd import ops, scenes, scene_desc
from tests import seam_scenes as ss
from tests.conftest import assert_image_close
from tests.gpu_support import WALK_KNOBS, Env, dev, grad_close, host, splat_tex
from tests.support import bits

pytestmark = pytest.mark.gpu

# the five walk variants the tile bins, the wide tree walk, the octant walk's switch, the per-lane walk and the bins' fallback are reached by —
# and a sixth: with FFX_WIDE=0 alone the tile bins stay on and answer K7 again, so the binary octant TREE walk itself runs only with both off
WALKS = {"default": {}, "FFX_BINS=0": {"FFX_BINS": "0"}, "FFX_WIDE=0": {"FFX_WIDE": "0"}, "FFX_TRAVERSAL=lane": {"FFX_TRAVERSAL": "lane"}, "FFX_BIN_CAP=0": {"FFX_BIN_CAP": "0"},
         "FFX_BINS=0 FFX_WIDE=0": {"FFX_BINS": "0", "FFX_WIDE": "0"}}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need a HIP device"


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in WALK_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _geoms(oracle, sc):
    """-> (oracle geometry, a function that builds the device geometry afresh, albedo rows)"""
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    xf = np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1))
    go = oracle.Geometry(pool, tris, shape, off)
    go.update(xf, off.astype(np.int32))

    def fresh():
        gd = ops.DeviceGeometry(pool, tris, shape, off)
        gd.update(xf, off.astype(np.int32))
        return gd
    return go, fresh, alb


def _k7_findings(what, got, want):
    (t, s, p), (tw, sw, pw) = got, want
    assert t.shape == tw.shape and s.shape == sw.shape and p.shape == pw.shape
    bad = []
    dp = np.nonzero(p != pw)[0]
    if dp.size:
        r = int(dp[0])
        bad.append(f"{what}: prim differs on {dp.size} of {p.size} rays; first: ray {r} prim {p[r]} t {t[r]!r}, tree-free prim {pw[r]} t {tw[r]!r}")
    if (bits(t) != bits(tw)).any():
        bad.append(f"{what}: t bits differ on {int((bits(t) != bits(tw)).sum())} rays")
    if (s != sw).any():
        bad.append(f"{what}: shape differs on {int((s != sw).sum())} rays")
    return bad


# ------------------------------------------------------------------ K7 trace_primary: the ridges, every pitched camera, every walk
@pytest.mark.parametrize("name", list(ss.CAM_FIXTURES))
def test_k7_every_walk_equals_the_tree_free_oracle_on_the_ridges(oracle, monkeypatch, name):
    """t bits, shape and prim of EVERY ray of the 48 pitched 2048x2 cameras, through each of the six walk variants (the geometry built afresh under
    each environment).  Without an absolute term in the leaf pad the tree walks return the neighbour across the seam on 105 rays of
    wobbled_far (tests/test_seams_cpu.py)."""
    mesh, eye, fov = ss.CAM_FIXTURES[name]()
    go, fresh, _ = _geoms(oracle, scenes.SceneData([mesh], None))
    cams = [scene_desc.camera_from_sensor(c) for c in ss.pitched_cameras(eye, fov=fov)]
    with oracle.tree_free():
        want = [go.trace_primary(c, 1, 0, 0) for c in cams]
    assert all((w[2][ss.FILM_W:] >= 0).mean() > 0.85 for w in want)  # (what must hit and what may miss: tests/test_seams_cpu.py)
    bad = []
    for walk, env in WALKS.items():
        with Env(monkeypatch, env):
            gd = fresh()
            for k, c, w in zip(ss.KS, cams, want):
                bad += _k7_findings(f"{walk} k={k:+.2f}", tuple(host(a) for a in gd.trace_primary(c, 1, 0, seed=0)), w)
    assert not bad, f"{name}: {len(bad)} findings:\n  " + "\n  ".join(bad[:16])


# ------------------------------------------------------------------ K7 trace_rays: the non-apex test on the per-lane walk
@pytest.mark.parametrize("name", list(ss.RAY_FIXTURES))
def test_trace_rays_on_grazing_rays_equals_the_all_pairs_reference(name):
    """40 000 rays that cross the sheet a few ulp of their length beside the seam: t bits and prim equal the float32 all-pairs reference on
    every ray (the tree returned the neighbour on 105 / 136 / 30 / 6 of them before the leaf pad had an absolute term)"""
    mesh, eye = ss.RAY_FIXTURES[name]()
    o, d, k = ss.grazing_rays(eye)
    t_ref, p_ref = ss.all_pairs(mesh, o, d)
    assert (p_ref >= 0).mean() > 0.99
    pool, tris, shape, off, *_ = scenes.flatten(scenes.SceneData([mesh], None))
    gd = ops.DeviceGeometry(pool, tris, shape, off)
    gd.update(np.eye(4, dtype=np.float32)[None])
    t, s, p = (host(a) for a in gd.trace_rays(dev(o), dev(d)))
    bad = _k7_findings(name, (t, s, p), (t_ref, np.where(p_ref >= 0, 0, -1).astype(np.int32), p_ref))
    assert not bad, "\n  ".join(bad)


# ------------------------------------------------------------------ the small stock scenes: K7, K8 and K9 through every walk
_STOCK = {}


def _stock(oracle, name):
    """-> per scene, computed once and never modified: the scene, geometries, texture, and per pitched camera of ss.RENDER_KS the tree-free
    oracle's image and texture gradient at 8 spp"""
    if name not in _STOCK:
        sc, eye, target = ss.stock(name)
        go, fresh, alb = _geoms(oracle, sc)
        tex = splat_tex(sc)
        gimg = np.random.default_rng(1).standard_normal((ss.FILM_H, ss.FILM_W, 3)).astype(np.float32)
        cams = dict(zip(ss.KS, ss.pitched_cameras(eye, target=target)))
        ref = {}
        for k in ss.RENDER_KS:
            sd = scene_desc.scene_desc(ss.with_camera(sc, cams[k]), shadows=True)
            with oracle.tree_free():
                ref[k] = (sd, go.render_fwd(sd, alb, host(tex), 8, seed=3), go.render_bwd(sd, alb, 8, 3, gimg))
        _STOCK[name] = (sc, go, fresh, alb, tex, gimg, cams, ref)
    return _STOCK[name]


@pytest.mark.parametrize("name", ["vocalfold", "colon"])
def test_k7_every_walk_equals_the_tree_free_oracle_on_the_stock_scenes(oracle, monkeypatch, name):
    """the 48 pitched cameras in the scenes' plane of symmetry, where the tubes' seams and the lips' edges lie: every ray, every walk"""
    sc, go, fresh, *_, cams, _ = _stock(oracle, name)
    cs = [scene_desc.camera_from_sensor(c) for c in cams.values()]
    with oracle.tree_free():
        want = [go.trace_primary(c, 1, 0, 0) for c in cs]
    bad = []
    for walk, env in WALKS.items():
        with Env(monkeypatch, env):
            gd = fresh()
            for k, c, w in zip(cams, cs, want):
                bad += _k7_findings(f"{walk} k={k:+.2f}", tuple(host(a) for a in gd.trace_primary(c, 1, 0, seed=0)), w)
    assert not bad, f"{name}: {len(bad)} findings:\n  " + "\n  ".join(bad[:16])


@pytest.mark.parametrize("name", ["vocalfold", "colon"])
def test_renders_and_texture_gradients_of_every_walk_equal_each_other_and_the_tree_free_oracle(oracle, monkeypatch, name):
    """render_fwd with shadows on at 8 spp (primary rays of a pitched camera; shadow rays of a projector beside the plane and of a spot IN it)
    and render_bwd under each of the six variants, every image and every gradient within the radiance / gradient bounds of
    tests/test_ties_gpu.py of the TREE-FREE oracle's.  The five variants of the wave-packet kernels give the same image bit for bit and the
    same deterministic texture gradient bit for bit.  (The render comparisons are not shown to detect the defect the K7 tests detect: with a
    leaf pad without the absolute term the hits of these fixtures differ, their images on these cameras did not.)  FFX_TRAVERSAL=lane is another KERNEL, not only another walk: it adds a pixel's samples
    in sequence where the packet kernels combine them in a fixed tree, and it has no deterministic adjoint (ops.render_bwd refuses) — its
    image is held to the default's within the bound tests/test_hip_parity.py::test_k9_cached_adjoint_matches_retrace_and_oracle holds the
    per-lane forward to the packet kernel's cache-writing forward with under FFX_TRAVERSAL=lane (assert_close, rtol 1e-4, atol 1e-5 of the
    image's maximum; the number of pixel channels whose bits differ is printed), its float-atomic gradient to the oracle's; its HITS are held
    bit for bit by the K7 tests above, on the same cameras."""
    sc, go, fresh, alb, tex, gimg, cams, ref = _stock(oracle, name)
    bad = []
    for k, (sd, img_o, gt_o) in ref.items():
        assert float(img_o.max()) > 0.01
        first = None
        for walk, env in WALKS.items():
            lane = env.get("FFX_TRAVERSAL") == "lane"
            with Env(monkeypatch, env):
                gd = fresh()
                img = gd.render_fwd(sd, dev(alb), tex, 8, seed=3)
                gt = gd.render_bwd(sd, dev(alb), 8, 3, dev(gimg), deterministic=not lane)
            assert_image_close(host(img), img_o, 8, what=f"{name} k={k:+.2f} {walk}")
            grad_close(host(gt), gt_o, f"{name} k={k:+.2f} {walk}", 2e-4)
            if first is None:
                first = (walk, img, gt)
            elif lane:
                print(f"{name} k={k:+.2f}: the per-lane kernel's image differs from the default's in the bits of {int((img != first[1]).sum())} of {img.numel()} pixel channels")
                torch.testing.assert_close(img, first[1], rtol=1e-4, atol=1e-5 * float(first[1].max()))
            else:
                if not torch.equal(img, first[1]):
                    bad.append(f"k={k:+.2f} {walk}: {int((img != first[1]).any(-1).sum())} pixels differ from the {first[0]} walk's")
                if not torch.equal(gt, first[2]):
                    bad.append(f"k={k:+.2f} {walk}: {int((gt != first[2]).sum())} texels of the gradient differ from the {first[0]} walk's")
    assert not bad, f"{name}:\n  " + "\n  ".join(bad)


# ------------------------------------------------------------------ the recorded lane
def test_recorded_vocal_fold_lane_bins_and_the_wide_tree_walk_agree_on_all_67m_rays(monkeypatch):
    """the full vocal fold at 512 x 512 x 256 spp, seed 1: K7 under the default (tile bins) and under FFX_BINS=0 (the wide tree walk), t, shape
    and prim kept on the device, torch.equal on all 67 108 864 rays.  Before the leaf pad had an absolute term ONE ray differed — pixel
    (93, 255): bins prim 9854 at t = 3.5131609, every tree walk prim 9729 at t = 3.5131612.  The colon's recorded lane
    (1024 x 1024 x 256 spp, seed 2, pixel (180, 511)) is left out: it needs 3 GB per output."""
    sc = scenes.vocalfold()
    pool, tris, shape, off, *_ = scenes.flatten(sc)
    cam = scene_desc.camera_from_sensor(sc.camera)
    out = []
    for env in ({}, {"FFX_BINS": "0"}):
        with Env(monkeypatch, env):
            gd = ops.DeviceGeometry(pool, tris, shape, off)
            gd.update(np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)))
            out.append(gd.trace_primary(cam, 256, 1, seed=1))
    (t0, s0, p0), (t1, s1, p1) = out
    assert t0.numel() == 512 * 512 * 256 and float((p0 >= 0).float().mean()) > 0.9
    if not torch.equal(p0, p1):
        r = torch.nonzero(p0 != p1).flatten()
        i = int(r[0])
        pytest.fail(f"{r.numel()} rays differ; first: ray {i} (pixel {i // 256 % 512}, {i // 256 // 512}) bins prim {int(p0[i])} t {float(t0[i])!r}, tree prim {int(p1[i])} t {float(t1[i])!r}")
    assert torch.equal(t0.view(torch.int32), t1.view(torch.int32)) and torch.equal(s0, s1)
