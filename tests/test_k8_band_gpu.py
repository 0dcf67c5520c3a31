"""The plain-scene instance's launch-proven diets (ffx_trace.hip: cam_ray<BAND> — the camera's operand band, ffx_band.h — and the 32-bit offsets on
scalar bases, at32): for a camera the launch proves in band the plain-scene instance renders the generic instance's image and fused adjoint bit for
bit — the generic instance keeps the IEEE forms and the 64-bit addresses — at narrow, ordinary and very wide fields of view, on full and partly
filled passes, and on textures whose clamped taps meet all four borders; a camera outside the band is not a plain scene and takes the generic
instance.

Scene: tests/k8_scenes.py's vocal fold on a 24 x 16 film (96 tiles: many workgroups, 16 is no multiple of a tile bin's side), 64 spp (a full
pass) and 40 spp (the last 24 lanes of the pass idle)."""
import numpy as np
import pytest
import torch

from tests import k8_scenes

pytestmark = pytest.mark.gpu

W, H = 24, 16


@pytest.fixture(scope="module")
def scene():
    wl, tex = k8_scenes.workload(width=W, height=H, tex=64)
    k8_scenes.pose(wl, 11)
    sd = wl.mi_scene.scene_desc(tex_channels=1)
    return wl, sd, wl.mi_scene.materials_arg(sd), tex.unsqueeze(-1).contiguous()


_GIMG = None


def _gimg():
    """one gradient image per pixel of the film, non-zero at that pixel alone ([H * W, H, W, 3]): the fused adjoint adds to the texture with float
    atomics, one wave per pixel, and texels that several pixels reach are summed in the order the waves arrive (tests/test_k8_plain_gpu.py: two launches
    of the SAME instance differ in last bits) — with one pixel per launch every texel has one writer, whatever the texture's size, and every pixel's
    contribution is compared"""
    global _GIMG
    if _GIMG is None:
        g = np.where(np.random.default_rng(5).random((H, W, 3)) < 0.5, -1.0, 1.0).astype(np.float32) / (H * W * 3)
        m = np.zeros((H * W, H * W, 3), np.float32)
        m[np.arange(H * W), np.arange(H * W)] = g.reshape(-1, 3)
        _GIMG = torch.from_numpy(m.reshape(H * W, H, W, 3)).to(k8_scenes.DEV)
    return _GIMG


def _both(geom, sd, mats, tex3, spp, seed, monkeypatch):
    """image and per-pixel gradients of the default launch and of FFX_K8_PLAIN=0, with the launch counters' differences (plain, generic) of each"""
    from fireflies_amd import ops

    res = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
        else:
            monkeypatch.setenv("FFX_K8_PLAIN", env)
        c0 = ops.k8_instance_launches()
        img = geom.render_fwd(sd, mats, tex3, spp, seed)
        adj = [geom.render_fwd_adjoint(sd, mats, tex3, spp, seed, g) for g in _gimg()]
        torch.cuda.synchronize()
        c1 = ops.k8_instance_launches()
        res.append((img, adj, (c1[0] - c0[0], c1[1] - c0[1])))
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    return res


def _assert_same_bits(res, what, plain):
    (img_d, adj_d, n_d), (img_g, adj_g, n_g) = res
    n = 1 + len(adj_d)
    assert n_d == ((n, 0) if plain else (0, n)), f"{what}: the default launches take the {'plain-scene' if plain else 'generic'} instance"
    assert n_g == (0, n), f"{what}: FFX_K8_PLAIN=0 keeps the generic instance"
    gt_d, gt_g = sum(g for _, g in adj_d), sum(g for _, g in adj_g)  # (for the figures; the bits are compared launch by launch)
    print(f"{what}: {int((img_d != img_g).sum())} of {img_g.numel()} image values differ, {int((gt_d != gt_g).sum())} of {int((gt_g != 0).sum())} non-zero "
          f"gradient values differ; image max {float(img_g.max()):.4f}")
    assert img_d.dtype == torch.float32 and torch.equal(img_d, img_g), f"{what}: image"
    assert all(torch.equal(i, img_d) for i, _ in adj_d) and all(torch.equal(i, img_g) for i, _ in adj_g), f"{what}: image of the fused launch"
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(adj_d, adj_g)), f"{what}: gtex of the fused forward + adjoint"
    if plain:
        assert int((gt_g != 0).sum()) > 0, f"{what}: the gradient reaches the texture"
    return img_g, gt_g


@pytest.mark.parametrize("spp", [64, 40])
@pytest.mark.parametrize("fov", [20.0, 90.0, 170.0])
def test_in_band_cameras_render_the_generic_instances_bits(scene, fov, spp, monkeypatch):
    wl, sd, mats, tex3 = scene
    sd2 = k8_scenes.with_camera(sd, k8_scenes.camera_to_sample(sd, fov))
    img, gt = _assert_same_bits(_both(wl.mi_scene.geom, sd2, mats, tex3, spp, 3, monkeypatch), f"fov {fov:g}, {spp} spp", plain=True)
    assert float(img.max()) > 0.0


@pytest.mark.parametrize("case", ["nonuniform_w", "s2c_scaled_up", "s2c_scaled_down"])
def test_out_of_band_cameras_take_the_generic_instance(scene, case, monkeypatch):
    """a homogeneous w that varies over the film; sample-to-camera rows times 2^50 / 2^-50 (|np|^2 = 2^+-100 times the sensor's): the launch cannot
    prove the band, the generic instance renders — under either setting of FFX_K8_PLAIN, the same launch"""
    wl, sd, mats, tex3 = scene
    K = k8_scenes.camera_to_sample(sd, 60.0)
    K2 = {"nonuniform_w": lambda: k8_scenes.nonuniform_w(K), "s2c_scaled_up": lambda: k8_scenes.scaled_s2c(K, 50), "s2c_scaled_down": lambda: k8_scenes.scaled_s2c(K, -50)}[case]()
    sd2 = k8_scenes.with_camera(sd, K2)
    img, _ = _assert_same_bits(_both(wl.mi_scene.geom, sd2, mats, tex3, 64, 3, monkeypatch), case, plain=False)
    assert torch.isfinite(img).all() and float(img.max()) > 0.0
    if case == "s2c_scaled_up":  # the same rays: powers of two scale exactly (scaled down, squares of small components turn denormal), the image is the unscaled camera's
        ref = wl.mi_scene.geom.render_fwd(k8_scenes.with_camera(sd, K), mats, tex3, 64, 3)
        assert torch.equal(img, ref), f"{case}: image of the unscaled camera"


@pytest.mark.parametrize("tw,th", [(7, 5), (500, 500)])
def test_texture_edges(scene, tw, th, monkeypatch):
    """a 7 x 5 texture (every footprint within a few texels of a border: taps clamped at all four) and a 500 x 500 one (row offsets beyond 16 bits),
    bright everywhere: the probe and the gather read every tap"""
    wl, sd, mats, _ = scene
    sd2, tex3 = k8_scenes.with_texture(k8_scenes.with_camera(sd, k8_scenes.camera_to_sample(sd, 90.0)), tw, th)
    img, gt = _assert_same_bits(_both(wl.mi_scene.geom, sd2, mats, tex3, 64, 3, monkeypatch), f"texture {tw} x {th}", plain=True)
    assert float(img.max()) > 0.0
    # which taps the film's samples reach: the adjoint of an all-positive gradient image is non-zero exactly at the texels some lit sample taps
    # (a coverage figure of this test's scene, from one more launch: dense sums depend on arrival order and are not compared)
    dense = torch.full((H, W, 3), 1.0 / (H * W * 3), device=k8_scenes.DEV)
    _, g = wl.mi_scene.geom.render_fwd_adjoint(sd2, mats, tex3, 64, 3, dense)
    g = g[..., 0]
    print(f"texture {tw} x {th}: texels tapped {int((g != 0).sum())} of {g.numel()}; border rows / columns tapped: top {int((g[0] != 0).sum())}, "
          f"bottom {int((g[-1] != 0).sum())}, left {int((g[:, 0] != 0).sum())}, right {int((g[:, -1] != 0).sum())}")
    if (tw, th) == (7, 5):  # every footprint is within a few texels of a border: clamped taps on all four sides are read and written
        assert bool((g[0] != 0).any()) and bool((g[-1] != 0).any()) and bool((g[:, 0] != 0).any()) and bool((g[:, -1] != 0).any())
