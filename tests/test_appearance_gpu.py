"""The appearance adjoint on the GPU: d loss / d base colour per material row, d loss / d spot intensity and d loss / d base-colour
texture against central differences of the GPU forward and of the float64 restatement (tests/ref_path.py at max_depth 2), the texture gradient with the
bit set, mi.render's leaves end to end, two inverse renderings, a full-size render and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, scene_desc, workloads
from fireflies_amd._lib import api
from tests import gpu_support as gpu
from tests import ref_path as rp
from tests.corner_scenes import appearance_corner, base_texture
from tests.gpu_support import DEV
from tests.support import copy_desc

pytestmark = pytest.mark.gpu



@pytest.mark.parametrize("principled,tint,gaussian", [(False, False, False), (True, False, True), (True, True, False), (True, True, True)])
def test_row_gradients_match_central_differences(principled, tint, gaussian):
    ms, sd, world = gpu.load(appearance_corner(principled, tint), gaussian, 1)
    assert sd.n_mat_h > 0
    tex, gimg = gpu.rand_tex(sd, 1), gpu.rand_gimg(sd, 2)
    spp, seed, h = 16, 7, 1e-2
    gtex, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex)
    g = app.rows.double().cpu().numpy()
    rows = ms._albedo_host.copy()
    tex_np, gimg_np = tex.cpu().numpy(), gimg.double().cpu().numpy()
    stddev = 0.5 if gaussian else None
    fd_gpu, fd_ref = np.zeros_like(g), np.zeros_like(g)
    for i in range(rows.shape[0]):
        for k in range(3):
            lo, hi = rows.copy(), rows.copy()
            lo[i, k] -= h
            hi[i, k] += h
            fd_gpu[i, k] = (gpu.loss(ms, sd, hi, tex, spp, seed, gimg) - gpu.loss(ms, sd, lo, tex, spp, seed, gimg)) / (2 * h)
            ref = [float((rp.render_fwd(*world[:3], sd, r.astype(np.float64), tex_np, spp, seed, 2, gaussian_stddev=stddev) * gimg_np).sum()) for r in (hi, lo)]
            fd_ref[i, k] = (ref[0] - ref[1]) / (2 * h)
    scale = np.abs(fd_gpu).max()
    assert scale > 0 and (np.abs(g).sum(1) > 0).sum() >= 3
    assert np.abs(g - fd_gpu).max() <= 1e-3 * scale, (g, fd_gpu)
    assert np.abs(g - fd_ref).max() <= 1e-3 * np.abs(fd_ref).max(), (g, fd_ref)


def test_spot_intensity_gradient_is_the_finite_difference():
    ms, sd, _ = gpu.load(appearance_corner(True, True), False, 1)
    assert sd.shadows & 1
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    spp, seed, h = 16, 3, 0.5
    _, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex)
    for c in range(3):
        lo, hi = copy_desc(sd), copy_desc(sd)
        lo.spot.intensity[c] -= h
        hi.spot.intensity[c] += h
        ls = [float((ms.geom.render_fwd(s, None, tex, spp, seed).double() * gimg.double()).sum()) for s in (hi, lo)]
        fd = (ls[0] - ls[1]) / (2 * h)
        assert fd > 0 and abs(float(app.spot[c]) - fd) <= 1e-3 * fd, (c, float(app.spot[c]), fd)


@pytest.mark.parametrize("gaussian", [False, True])
def test_base_texture_directional_derivative(gaussian):
    ms, sd, _ = gpu.load(appearance_corner(False, tint=True, base_tex=base_texture()), gaussian, 1)
    assert sd.n_base_tex == 1
    t = ms._base_tex[0][1]  # (the description points at this tensor)
    tex, gimg = gpu.rand_tex(sd, 6), gpu.rand_gimg(sd, 7)
    spp, seed, h = 16, 9, 1e-2
    _, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex)
    assert app.rows[0].abs().max() == 0  # (the floor's row: its base colour is the texture)
    g = app.base_tex[0]
    assert tuple(g.shape) == (8, 8, 3) and float(g.abs().sum()) > 0
    orig = t.clone()
    for s in range(3):
        v = torch.randn(t.shape, generator=torch.Generator().manual_seed(s)).to(DEV)
        ls = []
        for sign in (1, -1):
            t.copy_(orig + sign * h * v)
            ls.append(float((ms.geom.render_fwd(sd, None, tex, spp, seed).double() * gimg.double()).sum()))
        t.copy_(orig)
        fd = (ls[0] - ls[1]) / (2 * h)
        dd = float((g.double() * v.double()).sum())
        assert abs(dd - fd) <= 1e-3 * max(abs(fd), float((g.double().abs() * v.double().abs()).sum()) * 1e-2), (dd, fd)


@pytest.mark.parametrize("gaussian,tc", [(False, 1), (True, 3)])
def test_texture_gradient_with_the_bit_is_unchanged(gaussian, tc):
    ms, sd, _ = gpu.load(appearance_corner(True, True), gaussian, tc)
    tex, gimg = gpu.rand_tex(sd, 8), gpu.rand_gimg(sd, 9)
    ref = ms.geom.render_bwd(sd, None, 16, 2, gimg)
    gtex, _ = ms.geom.render_bwd(sd, None, 16, 2, gimg, appearance=True, tex=tex)
    assert float(ref.abs().max()) > 0
    assert torch.allclose(gtex, ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()))


def test_mi_render_leaves_end_to_end():
    ms, sd, _ = gpu.load(appearance_corner(True, shared=True), False, 3)
    p = mi.traverse(ms)
    spp, seed = 16, 4
    tex = gpu.rand_tex(sd, 10)
    gimg = gpu.rand_gimg(sd, 11)
    base, inten = p["mat-Floor.brdf_0.base_color.value"].t.clone(), p["emit-Spot.intensity.value"].t.clone()
    sd = ms.scene_desc(tex_channels=3)
    gtex_ref, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex)
    b_leaf, i_leaf, t_leaf = gpu.leaf(base.tolist()), gpu.leaf(inten.tolist()), tex.clone().requires_grad_(True)
    p["mat-Floor.brdf_0.base_color.value"] = b_leaf
    p["emit-Spot.intensity.value"] = i_leaf
    p["tex.data"] = t_leaf
    p.update()
    img = mi.render(ms, spp=spp, seed=seed).torch()
    (img * gimg).sum().backward()
    rows = ms._material_meshes["mat-Floor"]
    assert len(rows) == 2
    assert torch.allclose(b_leaf.grad, app.rows[rows].sum(0), rtol=1e-4, atol=1e-6)
    assert torch.allclose(i_leaf.grad, app.spot, rtol=1e-4, atol=1e-6)
    assert torch.allclose(t_leaf.grad, ms.geom.render_bwd(sd, None, spp, seed, gimg), rtol=1e-5, atol=1e-6 * float(gtex_ref.abs().max()))
    # the forward is today's image
    p["mat-Floor.brdf_0.base_color.value"] = mi.Color3f(base)
    assert not p._leaves.get("mat-Floor.brdf_0.base_color.value")
    p["emit-Spot.intensity.value"] = mi.Color3f(inten)
    p["tex.data"] = tex
    p.update()
    assert not p._leaves
    plain = mi.render(ms, spp=spp, seed=seed).torch()
    assert not plain.requires_grad and torch.equal(plain, img.detach())


def test_inverse_rendering_recovers_base_colour_and_intensity():
    ms, sd, _ = gpu.load(appearance_corner(False), False, 1)
    p = mi.traverse(ms)
    p["tex.data"] = gpu.rand_tex(sd, 12)[..., 0].contiguous()
    p.update()
    spp, seed = 16, 5
    target = mi.render(ms, spp=spp, seed=seed).torch().clone()
    key_b, key_i = "mat-Cube.brdf_0.base_color.value", "emit-Spot.intensity.value"
    b_true, i_true = p[key_b].t.clone(), p[key_i].t.clone()
    b = gpu.fit(ms, key_b, (b_true + torch.tensor([0.15, -0.2, 0.1])).tolist(), target, spp, seed, 0.03, 300)
    assert float((b.cpu() - b_true.cpu()).abs().max()) < 1e-2, (b, b_true)
    p[key_b] = mi.Color3f(b_true)
    p.update()
    i = gpu.fit(ms, key_i, (i_true * 0.6).tolist(), target, spp, seed, 0.2, 300)
    assert float(((i.cpu() - i_true.cpu()) / i_true.cpu()).abs().max()) < 1e-2, (i, i_true)


def test_full_size_vocalfold_base_colour_gradient():
    wl = workloads.vocalfold(device=DEV)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    ms = wl.mi_scene
    tex = workloads.build_texture(wl).detach()
    sd = ms.scene_desc(tex_channels=1)
    assert (sd.cam.width, sd.cam.height) == (512, 512)
    mats, t3, spp, seed = ms.materials_arg(sd), tex.unsqueeze(-1).contiguous(), 64, 1
    gimg = torch.full((512, 512, 3), 1.0 / (512 * 512), device=DEV)
    _, app = ms.geom.render_bwd(sd, mats, spp, seed, gimg, appearance=True, tex=t3)
    g = app.rows.double().cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(app.spot.cpu().numpy()).all()
    i, k = np.unravel_index(np.abs(g).argmax(), g.shape)
    rows = ms._albedo_host.copy()
    h = 1e-2
    ls = []
    for sign in (1, -1):
        r = rows.copy()
        r[i, k] += sign * h
        s2 = copy_desc(sd)
        if sd.n_mat_h > 0:
            scene_desc.set_host_materials(s2, r)
            m2 = None
        else:
            m2 = torch.from_numpy(r).to(DEV)
        ls.append(float((ms.geom.render_fwd(s2, m2, t3, spp, seed).double() * gimg.double()).sum()))
    fd = (ls[0] - ls[1]) / (2 * h)
    assert abs(g[i, k] - fd) <= 1e-3 * abs(fd) + 1e-7, (g[i, k], fd)


def test_refusals():
    ms, sd, _ = gpu.load(appearance_corner(False), False, 1)
    p = mi.traverse(ms)
    tex, gimg = gpu.rand_tex(sd), gpu.rand_gimg(sd)
    g = ms.geom
    p["tex.data"] = tex[..., 0].contiguous()
    p["mat-Cube.brdf_0.base_color.value"] = gpu.leaf([0.8, 0.4, 0.3])
    p.update()
    with pytest.raises(ValueError):
        mi.render(ms, spp=4, integrator=mi.load_dict({"type": "path", "max_depth": 3}))
    with pytest.raises(ValueError):
        g.render_bwd(sd, None, 4, 0, gimg, appearance=True, tex=tex, max_depth=3)
    os.environ["FFX_DETERMINISTIC"] = "1"
    try:
        with pytest.raises(ValueError):
            mi.render(ms, spp=4)
        with pytest.raises(ValueError):
            g.render_bwd(sd, None, 4, 0, gimg, appearance=True, tex=tex)
    finally:
        os.environ.pop("FFX_DETERMINISTIC", None)
    # the C ABI: the bit with path bits, the bit on the cache and deterministic entries
    n_app = _abi.appearance_floats(sd.n_shapes)
    out = torch.zeros(tex.numel() + n_app, device=DEV)
    src = torch.cat([gimg.reshape(-1), tex.reshape(-1)])
    img = torch.empty((sd.cam.height, sd.cam.width, 3), device=DEV)
    blob, strm, pp = C.c_void_p(g.blob.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p
    A = _abi.RENDER_GRAD_APPEARANCE
    rc = api().call_rc("ffx_render_bwd", blob, C.byref(g.info), C.byref(sd), None, 4, 0, A | _abi.render_path(3, 5), pp(src.data_ptr()), pp(out.data_ptr()), strm,
                       allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    cache = torch.empty(max(int(api().lib.ffx_render_cache_bytes_sd(C.byref(sd), 4)), 64), dtype=torch.uint8, device=DEV)
    rc = api().call_rc("ffx_render_fwd_cache", blob, C.byref(g.info), C.byref(sd), None, pp(tex.data_ptr()), 4, 0, A, pp(img.data_ptr()), pp(cache.data_ptr()), strm,
                       allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    rc = api().call_rc("ffx_render_bwd_cached", C.byref(sd), None, pp(cache.data_ptr()), 4, pp(gimg.data_ptr()), pp(out.data_ptr()), None, A, None, strm,
                       allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    rc = api().call_rc("ffx_render_fwd", blob, C.byref(g.info), C.byref(sd), None, pp(tex.data_ptr()), 4, 0, A, pp(img.data_ptr()), strm,
                       allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    work = torch.empty(api().lib.ffx_render_bwd_det_bytes(C.byref(sd)), dtype=torch.uint8, device=DEV)
    rc = api().call_rc("ffx_render_bwd_det", blob, C.byref(g.info), C.byref(sd), None, 4, 0, A, pp(gimg.data_ptr()), pp(out.data_ptr()), pp(work.data_ptr()), strm,
                       allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
