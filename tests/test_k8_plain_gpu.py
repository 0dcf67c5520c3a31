"""The packet render kernel's plain-scene instance (ffx_trace.hip k_render_fwd_pk<..., PLAIN>, picked by the launcher's plain_scene): for a scene
the host proves plain it renders the generic instance's image and fused adjoint BIT FOR BIT, the launcher's counters say which instance ran, and
every feature the instance leaves out routes the launch to the generic one — whose image is still the oracle's.

Scene: the vocal fold at 64 x 48, two shapes, 8 x 8 fold lips in an 8 x 16 tube, a 4 x 4 laser on a 64^2 texture: the smallest that still has
bins for the three apexes, envelope-settled and hard shadow packets, lit and dark projector footprints."""
import random

import numpy as np
import pytest
import torch

from tests.conftest import assert_image_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAT = "mat-Default OBJ.brdf_0."


def _workload(**kw):
    from fireflies_amd import workloads

    wl = workloads.vocalfold(device=DEV, width=64, height=48, tex=64, grid=4, frames=4, n_fold=8, tube=(8, 16), entity_device="cpu", **kw)
    tex = workloads.build_texture(wl).detach().contiguous()
    wl.params["tex.data"] = tex
    return wl, tex


def _pose(wl, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    wl.ff_scene.randomize()


def _render(wl, spp, seed, **kw):
    """mi.render -> (image on the host as the film's raw values, launches of the plain-scene instance, launches of the generic one)"""
    from fireflies_amd import mi, ops

    p0, g0 = ops.k8_instance_launches()
    s0 = wl.mi_scene.render_paths["k8_plain"]
    img = mi.render(wl.mi_scene, spp=spp, seed=seed, **kw).torch()
    torch.cuda.synchronize()
    p1, g1 = ops.k8_instance_launches()
    assert wl.mi_scene.render_paths["k8_plain"] - s0 == p1 - p0  # the scene's own counter follows the library's
    return img, p1 - p0, g1 - g0


def _oracle_image(oracle, wl, tex, spp, seed, smooth=None, fp16=False):
    from fireflies_amd import scenes

    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(wl.data)
    go = oracle.Geometry(wl.mi_scene.geom.src_verts.cpu().numpy(), tris, shape, off, smooth=smooth)
    go.update(wl.mi_scene._xforms.numpy(), wl.mi_scene._offs)
    sd = wl.mi_scene.scene_desc(tex_channels=1)
    return go.render_fwd(sd, wl.mi_scene._albedo_host, tex.cpu().numpy(), spp, seed=seed, fp16=fp16).astype(np.float32)


def test_plain_instance_renders_the_generic_instances_bits(monkeypatch):
    """three randomised poses at 64 spp: image of the default launch == image under FFX_K8_PLAIN=0, raw float32; the same for the image and the
    texture gradient of the fused forward + adjoint; the counters show the plain instance in the first case and the generic one in the second.

    The fused adjoint adds to the texture with float atomics, one wave per pixel: under a gradient image that is non-zero everywhere, texels that
    several pixels reach are summed in the order the waves arrive, and two launches of the SAME instance differ in last bits (measured on this
    scene, MI355X: 31 to 53 of ~3500 texels between two launches of the generic instance; the test prints both counts).  So the bits are compared under gradient images that are non-zero on a lattice of pixels
    16 apart in x and 12 in y — their footprints, 5 texels (2.3 degrees of the projector) wide, lie about 15 degrees apart, more than twice the
    parallax the scene's depth range can produce between camera and projector (0.25 apart) — and the lattice is moved over all 192 offsets: every
    pixel's contribution is compared, each texel is written by one wave, and the sum is what that wave's program order makes it."""
    from fireflies_amd import ops

    wl, tex = _workload()
    geom, tex3 = wl.mi_scene.geom, tex.unsqueeze(-1).contiguous()
    H, W = 48, 64
    gfull = torch.from_numpy(np.where(np.random.default_rng(5).random((H, W, 3)) < 0.5, -1.0, 1.0).astype(np.float32) / (H * W * 3)).to(DEV)
    lattices = []
    for oy in range(12):
        for ox in range(16):
            g = torch.zeros_like(gfull)
            g[oy::12, ox::16] = gfull[oy::12, ox::16]
            lattices.append(g)
    for seed in (11, 12, 13):
        _pose(wl, seed)
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
        img_p, n_plain, n_gen = _render(wl, 64, seed)
        assert (n_plain, n_gen) == (1, 0), "the default launch of a plain scene takes the plain-scene instance"
        c0 = ops.k8_instance_launches()
        adj_p = [geom.render_fwd_adjoint(sd, mats, tex3, 64, seed, g) for g in lattices]
        ia_p, gd_p = geom.render_fwd_adjoint(sd, mats, tex3, 64, seed, gfull)
        torch.cuda.synchronize()
        c1 = ops.k8_instance_launches()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (len(lattices) + 1, 0), "fused adjoint: plain-scene instance"
        monkeypatch.setenv("FFX_K8_PLAIN", "0")
        img_g, n_plain, n_gen = _render(wl, 64, seed)
        assert (n_plain, n_gen) == (0, 1), "FFX_K8_PLAIN=0 keeps the generic instance"
        adj_g = [geom.render_fwd_adjoint(sd, mats, tex3, 64, seed, g) for g in lattices]
        ia_g, gd_g = geom.render_fwd_adjoint(sd, mats, tex3, 64, seed, gfull)
        _, gd_g2 = geom.render_fwd_adjoint(sd, mats, tex3, 64, seed, gfull)
        torch.cuda.synchronize()
        c2 = ops.k8_instance_launches()
        assert (c2[0] - c1[0], c2[1] - c1[1]) == (0, len(lattices) + 3), "fused adjoint under FFX_K8_PLAIN=0: generic instance"
        assert img_p.dtype == torch.float32 and torch.equal(img_p, img_g), f"pose {seed}: image"
        assert torch.equal(ia_p, ia_g) and torch.equal(ia_p, img_p), f"pose {seed}: image of the fused launch"
        gt_p, gt_g = torch.stack([g for _, g in adj_p]), torch.stack([g for _, g in adj_g])
        print(f"pose {seed}: {int((img_p != img_g).sum())} image values differ; lattice gradients: {int((gt_p != gt_g).sum())} of {int((gt_g != 0).sum())} differ; "
              f"dense gradient image (not asserted): {int((gd_p != gd_g).sum())} of {int((gd_g != 0).sum())} differ, {int((gd_g2 != gd_g).sum())} between two launches "
              f"of the generic instance")
        assert all(torch.equal(i, img_p) for i, _ in adj_p) and all(torch.equal(i, img_p) for i, _ in adj_g)
        assert torch.equal(gt_p, gt_g), f"pose {seed}: texture gradient of the fused launch, pixel lattices"
        assert float(img_p.max()) > 0.02 and int((gt_g != 0).sum()) > 1000


ROUTES = {
    "sheen": dict(params={"sheen.value": 0.6}),
    "clearcoat": dict(params={"clearcoat.value": 0.7}),
    "anisotropic": dict(params={"anisotropic.value": 0.5}),
    "smooth": dict(smooth=[False, True]),
    "fp16": dict(render={"fp16": True}),
    "spp65": dict(spp=65),
    "gaussian": dict(rfilter="gaussian"),
    "device_table": dict(env={"FFX_HOST_MATERIALS": "0"}),
}


@pytest.mark.parametrize("case", sorted(ROUTES))
def test_anything_not_plain_takes_the_generic_instance(case, oracle, monkeypatch):
    """each feature the plain-scene instance leaves out, one at a time: the launcher's counter shows the generic instance, and the image is the oracle's
    (tolerances: the suite's own for this scene and oracle — box film 1e-4 of the scale for all but 1e-3 of the pixel channels; optional lobes 2e-4 /
    2e-3 as for the colon's mucosa, fp16 2e-3 = four half-precision ulps; gaussian film 2 % of the channels, whose weights differ from the oracle's
    five expf in the last bits — as tests/test_hip_parity.py's small gaussian films)"""
    from fireflies_amd import scenes

    c = ROUTES[case]
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    if "smooth" in c:
        make = scenes.vocalfold

        def smooth_vocalfold(**kw):
            data = make(**kw)
            for m, s in zip(data.meshes, c["smooth"]):
                m.smooth = s
            return data

        monkeypatch.setattr(scenes, "vocalfold", smooth_vocalfold)
    wl, tex = _workload()
    if "smooth" in c:
        assert wl.mi_scene.geom.smooth == c["smooth"]
    if "rfilter" in c:
        wl.mi_scene.rfilter = c["rfilter"]
    _pose(wl, 21)
    for k, v in c.get("params", {}).items():
        wl.params[MAT + k] = v
    if "params" in c:
        wl.params.update()
        col = scenes.MAT_COLUMN[next(iter(c["params"])).split(".")[0]]
        assert (wl.mi_scene._albedo_host[:, col] > 0).all()
    spp, rkw = c.get("spp", 64), c.get("render", {})
    img, n_plain, n_gen = _render(wl, spp, 21, **rkw)
    assert n_plain == 0 and n_gen == 1, f"{case}: generic instance"
    ref = _oracle_image(oracle, wl, tex, spp, 21, smooth=c.get("smooth"), fp16=bool(rkw.get("fp16")))
    frac, rel = 1e-3, 1e-4
    if "params" in c:
        frac, rel = 2e-3, 2e-4
    if rkw.get("fp16"):
        frac, rel = 2e-3, 2e-3
    if "rfilter" in c:
        frac = 0.02
    scale, _ = assert_image_close(img.float().cpu().numpy(), ref, spp, frac=frac, rel=rel, what=case)
    assert scale > 0.02


@pytest.mark.parametrize("spp", [1, 3, 33, 64])
def test_sample_counts_around_the_pixel_block_kernel(spp, monkeypatch):
    """below 33 samples per pixel the pixel-block kernel renders (neither counter moves) and FFX_K8_PLAIN changes nothing; from 33 on the packet kernel
    does — 33: its last 31 lanes idle — and the plain-scene instance's image is the generic one's, bit for bit"""
    wl, tex = _workload()
    _pose(wl, 31)
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    img_d, n_plain, n_gen = _render(wl, spp, 7)
    assert (n_plain, n_gen) == ((0, 0) if spp <= 32 else (1, 0))
    monkeypatch.setenv("FFX_K8_PLAIN", "0")
    img_g, n_plain, n_gen = _render(wl, spp, 7)
    assert (n_plain, n_gen) == ((0, 0) if spp <= 32 else (0, 1))
    assert torch.equal(img_d, img_g) and float(img_d.max()) > 0.02
