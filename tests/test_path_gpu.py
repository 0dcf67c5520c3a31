"""The path integrator on the GPU: the default is untouched, the kernels agree per pixel with the float64 restatement
(tests/ref_path.py) on the same random numbers, light that arrives by a bounce only, the adjoint's identities, autograd, the optimiser's
route, the refusals and a full-size render."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, workloads
from fireflies_amd import functional as Fn
from fireflies_amd._lib import api
from fireflies_amd.optim import PatternOptimizer
from tests import gpu_support as gpu
from tests import ref_path as rp
from tests.corner_scenes import path_corner, relay
from tests.gpu_support import DEV
from tests.support import FFX_ERR_ARG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gaussian", [False, True])
def test_max_depth_2_is_the_default_render_bitwise(gaussian):
    ms, sd, _ = gpu.load(path_corner(True), gaussian, 1)
    tex = gpu.rand_tex(sd)
    mats = ms.materials_arg(sd)
    ref = ms.geom.render_fwd(sd, mats, tex, 16, 3)
    assert torch.equal(ms.geom.render_fwd(sd, mats, tex, 16, 3, max_depth=2), ref)
    assert torch.equal(Fn.render(tex, ms.geom, sd, mats, 16, 3, max_depth=2), ref)
    ms._params["tex.data"] = tex[..., 0].clone()
    a = mi.render(ms, spp=16, seed=3).torch().clone()
    for it in (mi.load_dict({"type": "path", "max_depth": 2}), mi.load_dict({"type": "direct"})):
        assert torch.equal(mi.render(ms, spp=16, seed=3, integrator=it).torch(), a)
    gimg = torch.randn(ref.shape, device=DEV)
    assert torch.allclose(ms.geom.render_bwd(sd, mats, 16, 3, gimg, max_depth=2), ms.geom.render_bwd(sd, mats, 16, 3, gimg), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("gaussian", [False, True])
def test_the_fp16_film_of_a_path_render_is_the_fp32_image_rounded(gaussian):
    """k_path_fwd's fp16 store (box film) and k_rf_gather's behind it (gaussian film): the pixel's fp32 value converted with round-to-nearest-even, as
    Tensor.half() converts — the fp32 render's image bit for bit.  24 x 24, 16 spp, max_depth 3"""
    ms, sd, _ = gpu.load(path_corner(False), gaussian, 1)
    tex = gpu.rand_tex(sd, 1)
    mats = ms.materials_arg(sd)
    half = ms.geom.render_fwd(sd, mats, tex, 16, 7, fp16=True, max_depth=3)
    assert half.dtype == torch.float16 and float(half.float().max()) > 0
    assert torch.equal(half, ms.geom.render_fwd(sd, mats, tex, 16, 7, max_depth=3).half())


@pytest.mark.parametrize("depth,principled,tc,gaussian", [(3, False, 1, False), (4, True, 3, True), (3, True, 1, True), (4, False, 3, False)])
def test_path_render_matches_float64_restatement(depth, principled, tc, gaussian):
    ms, sd, world = gpu.load(path_corner(principled), gaussian, tc)
    alb = ms.albedo.cpu().numpy().astype(np.float64)
    tex = gpu.rand_tex(sd, 1)
    spp, seed = 16, 7
    mats = ms.materials_arg(sd)
    img = ms.geom.render_fwd(sd, mats, tex, spp, seed, max_depth=depth).cpu().numpy().astype(np.float64)
    tex_np = tex.cpu().numpy()
    stddev = 0.5 if gaussian else None
    ref = rp.render_fwd(*world, sd, alb, tex_np, spp, seed, depth, gaussian_stddev=stddev)
    ref2 = rp.render_fwd(*world, sd, alb, tex_np, spp, seed, 2, gaussian_stddev=stddev)
    indirect = ref - ref2
    scale = float(ref.max())
    assert indirect.mean() > 0.05 * ref.mean() > 0  # (the bounces matter in this scene)
    err = np.abs(img - ref)
    # fp32 vs fp64: a hit, a shadow test or the path after a bounce can flip on an edge for a few samples
    assert (err > 2e-3 * scale).mean() <= 0.04, float((err > 2e-3 * scale).mean())
    assert np.median(err) <= 1e-4 * scale
    # the image's sum to 1 % of its indirect part: a missing pi or cosine in the bounce is a factor, not a percent
    assert abs(img.sum() - ref.sum()) <= 0.01 * indirect.sum(), (img.sum(), ref.sum(), indirect.sum())
    # the adjoint: the same paths replayed
    gimg = np.where(np.random.default_rng(2).random(img.shape) < 0.5, -1.0, 1.0).astype(np.float32) / img.size
    gt = ms.geom.render_bwd(sd, mats, spp, seed, torch.from_numpy(gimg).to(DEV), max_depth=depth).cpu().numpy().astype(np.float64)
    gt_ref = rp.render_bwd(*world, sd, alb, spp, seed, gimg, depth, gaussian_stddev=stddev)
    gs = np.abs(gt_ref).sum()
    assert gs > 0 and np.abs(gt - gt_ref).sum() <= 0.03 * gs, (np.abs(gt - gt_ref).sum(), gs)


@pytest.mark.parametrize("gaussian", [False, True])
def test_light_that_arrives_by_a_bounce_only(gaussian):
    ms, sd, _ = gpu.load(relay(), gaussian, 1)
    tex = gpu.rand_tex(sd, 4)
    mats = ms.materials_arg(sd)
    spp, seed = 32, 5
    gimg = torch.rand((sd.cam.height, sd.cam.width, 3), device=DEV)
    img2 = ms.geom.render_fwd(sd, mats, tex, spp, seed, max_depth=2)
    assert float(img2.abs().max()) == 0.0
    assert float(ms.geom.render_bwd(sd, mats, spp, seed, gimg, max_depth=2).abs().max()) == 0.0
    img3 = ms.geom.render_fwd(sd, mats, tex, spp, seed, max_depth=3)
    gt3 = ms.geom.render_bwd(sd, mats, spp, seed, gimg, max_depth=3)
    assert float(img3.min()) >= 0.0 and float(img3.mean()) > 0.0 and float(gt3.abs().sum()) > 0.0
    # the render is linear in the texture and the adjoint is its transpose: <gimg, render(tex)> = <gtex, tex>
    lhs, rhs = float((gimg.double() * img3.double()).sum()), float((gt3.double() * tex.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize("gaussian", [False, True])
def test_path_autograd_equals_render_bwd_and_forward_is_deterministic(gaussian):
    ms, sd, _ = gpu.load(path_corner(True), gaussian, 1)
    mats = ms.materials_arg(sd)
    tex = gpu.rand_tex(sd, 2)
    a = ms.geom.render_fwd(sd, mats, tex, 64, 11, max_depth=4)
    b = ms.geom.render_fwd(sd, mats, tex, 64, 11, max_depth=4)
    assert torch.equal(a, b)
    assert not torch.equal(a, ms.geom.render_fwd(sd, mats, tex, 64, 11, max_depth=4, rr_depth=1))  # (the roulette runs)
    gw = torch.randn(a.shape, device=DEV)
    leaf = tex.clone().requires_grad_(True)
    img = Fn.render(leaf, ms.geom, sd, mats, 64, 11, max_depth=4)
    assert torch.equal(img.detach(), a)
    (img * gw).sum().backward()
    torch.testing.assert_close(leaf.grad, ms.geom.render_bwd(sd, mats, 64, 11, gw, max_depth=4), rtol=1e-5, atol=1e-8)
    # mi.render with the integrator: the same kernels
    ms._params["tex.data"] = tex[..., 0].clone()
    assert torch.equal(mi.render(ms, spp=64, seed=11, integrator=mi.load_dict({"type": "path", "max_depth": 4})).torch(), a)


def _small():
    return workloads.vocalfold(device=DEV, width=64, height=56, tex=96, grid=6, frames=5, n_fold=20, tube=(20, 24))


def test_pattern_optimizer_path_steps_match_autograd():
    def custom(img):
        return (img[..., 1] - 0.05).square().mean() + 0.1 * img[..., 0].mean()

    it = mi.load_dict({"type": "path", "max_depth": 3})
    for loss_fn, S in ((None, 1), (custom, 2)):
        runs = []
        for which in ("step", "step_autograd"):
            wl = _small()
            kw = {} if loss_fn is None else {"loss_fn": loss_fn}
            opt = PatternOptimizer(wl.mi_scene, wl.ff_scene, wl.laser, sigma=10.0, tex_size=(96, 96), spp=4, lr=5e-3, samples_per_step=S, base_seed=5,
                                   integrator=it, **kw)
            assert opt._route(wl.mi_scene.scene_desc(tex_channels=1), [0]) == "retrace"
            losses = [float(getattr(opt, which)()["loss"]) for _ in range(3)]
            if which == "step":
                assert opt.step_paths == {"fused": 0, "cache_k9": 0, "retrace": 3 * S} and opt._cache is None
            runs.append((losses, wl.laser._rays.detach().clone()))
        np.testing.assert_allclose(runs[0][0], runs[1][0], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(runs[0][1], runs[1][1], rtol=1e-5, atol=2e-6)


def test_path_refusals():
    ms, sd, _ = gpu.load(path_corner(False), False, 1)
    mats = ms.materials_arg(sd)
    tex = gpu.rand_tex(sd)
    g = ms.geom
    gimg = torch.ones((sd.cam.height, sd.cam.width, 3), device=DEV)
    cache = torch.empty(ops.render_cache_bytes_sd(sd, 4), dtype=torch.uint8, device=DEV)
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            g.render_fwd(sd, mats, tex, 4, 0, max_depth=bad)
        with pytest.raises(ValueError):
            g.render_bwd(sd, mats, 4, 0, gimg, max_depth=bad)
    with pytest.raises(ValueError):
        g.render_fwd(sd, mats, tex, 4, 0, cache=cache, max_depth=3)
    with pytest.raises(ValueError):
        g.render_fwd_adjoint(sd, mats, tex, 4, 0, gimg, max_depth=3)
    with pytest.raises(ValueError):
        g.render_bwd_cached(sd, mats, cache, 4, gimg, max_depth=3)
    with pytest.raises(ValueError):
        g.render_bwd(sd, mats, 4, 0, gimg, deterministic=True, max_depth=3)
    os.environ["FFX_DETERMINISTIC"] = "1"
    try:
        with pytest.raises(ValueError):
            Fn.render(tex.clone().requires_grad_(True), g, sd, mats, 4, 0, max_depth=3)
        wl = _small()
        with pytest.raises(ValueError):
            PatternOptimizer(wl.mi_scene, wl.ff_scene, wl.laser, tex_size=(96, 96), spp=4, integrator=mi.load_dict({"type": "path", "max_depth": 3}))
    finally:
        os.environ.pop("FFX_DETERMINISTIC", None)
    # the C ABI: the calls without the path integrator refuse its bits, the ones with it refuse depths outside 2 .. 8
    img = torch.empty((sd.cam.height, sd.cam.width, 3), device=DEV)
    gtex = torch.zeros_like(tex)
    blob, strm = C.c_void_p(g.blob.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m = C.c_void_p(mats.data_ptr()) if mats is not None else None
    p = C.c_void_p
    rc = api().call_rc("ffx_render_fwd_cache", blob, C.byref(g.info), C.byref(sd), m, p(tex.data_ptr()), 4, 0, _abi.render_path(3, 5), p(img.data_ptr()),
                       p(cache.data_ptr()), strm, allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    work = torch.empty(api().lib.ffx_render_bwd_det_bytes(C.byref(sd)), dtype=torch.uint8, device=DEV)
    rc = api().call_rc("ffx_render_bwd_det", blob, C.byref(g.info), C.byref(sd), m, 4, 0, _abi.render_path(3, 5), p(gimg.data_ptr()), p(gtex.data_ptr()),
                       p(work.data_ptr()), strm, allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    rc = api().call_rc("ffx_render_fwd", blob, C.byref(g.info), C.byref(sd), m, p(tex.data_ptr()), 4, 0, 9 << _abi.RENDER_MAX_DEPTH_SHIFT, p(img.data_ptr()), strm,
                       allow=(FFX_ERR_ARG,))
    assert rc == FFX_ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("gaussian", [False, True])
def test_full_size_vocalfold_path_render(gaussian):
    wl = workloads.vocalfold(device=DEV)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach()
    if gaussian:
        wl.mi_scene.rfilter = "gaussian"
    sd = wl.mi_scene.scene_desc(tex_channels=1)
    assert (sd.cam.width, sd.cam.height) == (512, 512)
    mats, t3, geom = wl.mi_scene.materials_arg(sd), tex.unsqueeze(-1).contiguous(), wl.mi_scene.geom
    img2 = geom.render_fwd(sd, mats, t3, 64, 1)
    geom.render_fwd(sd, mats, t3, 64, 1, max_depth=3)  # (warm-up)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    img3 = geom.render_fwd(sd, mats, t3, 64, 1, max_depth=3)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(img3).all())
    m2, m3 = float(img2.double().mean()), float(img3.double().mean())
    assert m3 >= m2 * (1.0 - 1e-5), (m2, m3)
    assert dt < 5.0, dt
