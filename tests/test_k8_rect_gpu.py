"""The plain-scene instances of the packet render kernel take each pixel's bin rectangle from tables the library builds once per film
(fireflies_amd/csrc/ffx_rect.h, ffx_trace.hip rect_tables / bins_primary<..., RECT>) instead of forming it per pixel.  The tables hold the bits the
generic instance computes (tests/test_pixel_rect_cpu.py), so everything here is bit equality against the generic instance (FFX_K8_PLAIN=0), which
reads no table: the forward and the forward + adjoint, which read the tables, and the cache-writing plain forward, which keeps the per-pixel
arithmetic and only receives the new trailing kernel argument; films that share one process (each with its own key of the cache); and a film no table is kept for, which takes the generic instance and still renders the oracle's image.

Scene: tests/k8_scenes.py (the vocal fold of tests/test_k8_plain_gpu.py) on films of 64 x 48, 37 x 29 (odd sizes, a part-filled last tile in both
directions) and 8 x 8 (smaller than one block of the kernel's tile enumeration)."""
import numpy as np
import pytest
import torch

from tests import k8_scenes
from tests.conftest import assert_image_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILMS = [(64, 48), (37, 29), (8, 8)]
_SCENES = {}


def _scene(film):
    """one workload per film for the whole module (the tests pose it themselves and leave nothing else behind)"""
    if film not in _SCENES:
        wl, tex = k8_scenes.workload(width=film[0], height=film[1])
        _SCENES[film] = (wl, tex.unsqueeze(-1).contiguous())
    return _SCENES[film]


def _counted(fn):
    """fn() -> (its result, launches of the plain instances, launches of the generic ones), from ops.k8_launch_counters"""
    from fireflies_amd import ops

    k = ops.k8_launch_counters()
    p0, g0 = int(k[0]), int(k[1])
    out = fn()
    torch.cuda.synchronize()
    return out, int(k[0]) - p0, int(k[1]) - g0


def _both(monkeypatch, fn, n=1, what=""):
    """fn() under the default launcher and under FFX_K8_PLAIN=0 -> (plain result, generic result); the counters must show n launches of the plain
    instance in the first case and n of the generic one in the second"""
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    out_p, n_plain, n_gen = _counted(fn)
    assert (n_plain, n_gen) == (n, 0), f"{what}: the default launch takes the plain instance"
    monkeypatch.setenv("FFX_K8_PLAIN", "0")
    out_g, n_plain, n_gen = _counted(fn)
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    assert (n_plain, n_gen) == (0, n), f"{what}: FFX_K8_PLAIN=0 keeps the generic instance"
    return out_p, out_g


def _lattices(W, H, seed=5):
    """gradient images that are non-zero on a pixel lattice 16 apart in x and 12 in y, moved over all offsets the film has (tests/test_k8_plain_gpu.py:
    every texel is then written by one wave, and the fused adjoint's float atomics leave the sum that wave's program order makes)"""
    g = torch.from_numpy(np.where(np.random.default_rng(seed).random((H, W, 3)) < 0.5, -1.0, 1.0).astype(np.float32) / (H * W * 3)).to(DEV)
    out = []
    for oy in range(min(12, H)):
        for ox in range(min(16, W)):
            l = torch.zeros_like(g)
            l[oy::12, ox::16] = g[oy::12, ox::16]
            out.append(l)
    return out


@pytest.mark.parametrize("spp", [64, 40])
@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_table_fed_plain_instances_render_the_generic_instances_bits(film, spp, monkeypatch):
    """three poses: the forward's image, the fused forward + adjoint's image and texture gradient under every lattice, and the cache-writing forward's
    image, plain against generic, raw float32"""
    from fireflies_amd import mi, ops

    W, H = film
    wl, tex3 = _scene(film)
    geom = wl.mi_scene.geom
    lattices = _lattices(W, H)
    n_nz = 0
    for seed in (11, 12, 13):
        k8_scenes.pose(wl, seed)
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        what = f"{W} x {H}, {spp} spp, pose {seed}"
        img_p, img_g = _both(monkeypatch, lambda: mi.render(wl.mi_scene, spp=spp, seed=seed).torch().clone(), 1, what + ", forward")
        assert img_p.dtype == torch.float32 and img_p.shape[:2] == (H, W) and torch.equal(img_p, img_g), what + ": image"
        assert bool(torch.isfinite(img_p).all())
        if film == (64, 48):
            assert float(img_p.max()) > 0.02
        adj_p, adj_g = _both(monkeypatch, lambda: [geom.render_fwd_adjoint(sd, mats, tex3, spp, seed, g) for g in lattices], len(lattices), what + ", forward + adjoint")
        assert all(torch.equal(i, img_p) for i, _ in adj_p) and all(torch.equal(i, img_p) for i, _ in adj_g), what + ": image of the fused launch"
        gt_p, gt_g = torch.stack([g for _, g in adj_p]), torch.stack([g for _, g in adj_g])
        assert torch.equal(gt_p, gt_g), what + f": texture gradient, pixel lattices ({int((gt_p != gt_g).sum())} of {int((gt_g != 0).sum())} values differ)"
        n_nz += int((gt_g != 0).sum())

        def cached():
            buf = torch.full((ops.render_cache_bytes_sd(sd, spp),), 0xA5, dtype=torch.uint8, device=DEV)
            return geom.render_fwd(sd, mats, tex3, spp, seed, cache=buf)

        ic_p, ic_g = _both(monkeypatch, cached, 1, what + ", cache-writing forward")
        assert torch.equal(ic_p, ic_g) and torch.equal(ic_p, img_p), what + ": image of the cache-writing forward"
    assert n_nz > (1000 if film == (64, 48) else 0), "the lattices reach lit texels"


def test_films_that_share_a_process_keep_their_own_tables(monkeypatch):
    """two films rendered alternately give the images they give alone (the generic instance's, which reads no table); then renders of eight further
    films, each with a key of its own, and the first two again, whose tables are still theirs (a table is never freed or moved).  The films of this
    module stay well below the cache's 32 keys: a process that used them all would render every later film through the generic instance — the path
    of the film without a table below —, which the tests of other modules that run in this process must not meet"""
    from fireflies_amd import mi

    a, b = (64, 48), (37, 29)
    alone = {}
    monkeypatch.setenv("FFX_K8_PLAIN", "0")
    for film in (a, b):
        wl, _ = _scene(film)
        k8_scenes.pose(wl, 17)
        alone[film], n_plain, n_gen = _counted(lambda: mi.render(wl.mi_scene, spp=64, seed=3).torch().clone())
        assert (n_plain, n_gen) == (0, 1)
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)

    def alternately(rounds):
        for _ in range(rounds):
            for film in (a, b):
                wl, _ = _scene(film)
                img, n_plain, n_gen = _counted(lambda: mi.render(wl.mi_scene, spp=64, seed=3).torch().clone())
                assert (n_plain, n_gen) == (1, 0)
                assert torch.equal(img, alone[film]), f"film {film[0]} x {film[1]} between renders of the other"

    alternately(3)
    for w in range(9, 17):  # eight more keys: 9 x 8 ... 16 x 8
        wl, _ = k8_scenes.workload(width=w, height=8)
        k8_scenes.pose(wl, 17)
        img_p, n_plain, n_gen = _counted(lambda: mi.render(wl.mi_scene, spp=64, seed=3).torch().clone())
        assert (n_plain, n_gen) == (1, 0)
        monkeypatch.setenv("FFX_K8_PLAIN", "0")
        img_g = mi.render(wl.mi_scene, spp=64, seed=3).torch().clone()
        monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
        assert torch.equal(img_p, img_g), f"film {w} x 8"
    alternately(2)


def test_a_film_without_a_table_takes_the_generic_instance(oracle, monkeypatch):
    """the library keeps no table for a film beyond FFX_RECT_MAX_SIDE = 4096 pixels a side: 4097 x 2 renders through the generic instance — the
    oracle's image at the suite's bound for this scene's box film (1e-4 of the scale for all but 1e-3 of the pixel channels) —, while 4096 x 2, which
    differs in nothing else, takes the plain instance and renders the generic one's bits"""
    from fireflies_amd import mi, scenes

    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    wl, tex = k8_scenes.workload(width=4096, height=2)
    k8_scenes.pose(wl, 21)
    img_p, img_g = _both(monkeypatch, lambda: mi.render(wl.mi_scene, spp=64, seed=21).torch().clone(), 1, "4096 x 2")
    assert torch.equal(img_p, img_g) and float(img_p.max()) > 0.0

    wl, tex = k8_scenes.workload(width=4097, height=2)
    k8_scenes.pose(wl, 21)
    img, n_plain, n_gen = _counted(lambda: mi.render(wl.mi_scene, spp=64, seed=21).torch().clone())
    assert (n_plain, n_gen) == (0, 1), "4097 x 2: no table, the generic instance"
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(wl.data)
    go = oracle.Geometry(wl.mi_scene.geom.src_verts.cpu().numpy(), tris, shape, off)
    go.update(wl.mi_scene._xforms.numpy(), wl.mi_scene._offs)
    sd = wl.mi_scene.scene_desc(tex_channels=1)
    ref = go.render_fwd(sd, wl.mi_scene._albedo_host, tex.cpu().numpy(), 64, seed=21).astype(np.float32)
    scale, _ = assert_image_close(img.cpu().numpy(), ref, 64, frac=1e-3, rel=1e-4, what="4097 x 2, generic instance")
    assert scale > 0.0
