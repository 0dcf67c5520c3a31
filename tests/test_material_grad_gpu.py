"""The BSDF adjoint (FFX_RENDER_GRAD_MATERIAL) on the GPU: d loss / d the principled parameters of every material row against central
differences of the float64 restatement (tests/ref_path.py / tests/ref_bruteforce.py at max_depth 2) and of the GPU forward, the texture gradient and
the appearance block with the bit set, mi.render's BSDF leaves end to end, two inverse renderings, a full-size render and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, scene_desc, scenes, workloads
from fireflies_amd._lib import api
from tests import ref_bruteforce as rb
from tests import gpu_support as gpu
from tests import ref_path as rp
from tests import support
from tests.corner_scenes import EVERY_LOBE, NAMES, R0, base_texture, case, corner
from tests.gpu_support import DEV
from tests.support import FFX_ERR_ARG, copy_desc

pytestmark = pytest.mark.gpu


def _case(name, gaussian):
    sc, base_tex = case(name)
    ms, sd, world = gpu.load(sc, gaussian, 1)
    return sc, ms, sd, world, base_tex


@pytest.mark.parametrize("name,gaussian", [("defaults", False), ("defaults", True), ("every_lobe", False), ("every_lobe", True), ("textured", False)])
def test_every_parameter_matches_the_float64_restatement(name, gaussian):
    sc, ms, sd, world, base_tex = _case(name, gaussian)
    assert sd.n_mat_h > 0
    tex, gimg = gpu.rand_tex(sd, 1), gpu.rand_gimg(sd, 2)
    spp, seed = 16, 7
    _, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex, material=True)
    g = app.material.double().cpu().numpy()
    assert g.shape == (4, 11) and np.isfinite(g).all()
    rows = ms._albedo_host.astype(np.float64)
    tex_np, gimg_np = tex.cpu().numpy(), gimg.double().cpu().numpy()
    stddev = 0.5 if gaussian else None
    if base_tex is None:
        def f(r):
            return float((rp.render_fwd(*world, sd, r, tex_np, spp, seed, 2, gaussian_stddev=stddev) * gimg_np).sum())
    else:
        vuv = np.zeros((world[0].shape[0], 2))
        vuv[:4] = sc.meshes[0].uv

        def f(r):
            return float((rb.render_fwd(*world, sd, r, tex_np, spp, seed, vert_uv=vuv, base_tex=[base_tex.astype(np.float64)], gaussian_stddev=stddev)
                          * gimg_np).sum())
    lam = rows[:, scenes.MAT_COLUMN["model"]] == 0
    assert lam.sum() == 2 and np.abs(g[lam]).max() == 0  # (Lambert rows: 0 for every parameter)
    fd = np.zeros_like(g)
    for i in np.flatnonzero(~lam):
        for j in range(11):
            fd[i, j] = support.fd(f, rows, i, R0 + j, 1e-4)
    for j in range(11):
        scale = np.abs(fd[:, j]).max()
        assert np.abs(g[:, j] - fd[:, j]).max() <= 2e-3 * scale + 1e-9, (NAMES[j], g[:, j], fd[:, j])
    assert (np.abs(g) > 0).sum() >= (8 if name == "defaults" else 16)


@pytest.mark.parametrize("name,gaussian", [("defaults", False), ("every_lobe", True), ("textured", True)])
def test_every_parameter_matches_the_gpu_forward(name, gaussian):
    _, ms, sd, _, _ = _case(name, gaussian)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    spp, seed = 16, 5
    _, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex, material=True)
    g = app.material.double().cpu().numpy()
    rows = ms._albedo_host.copy()

    def f(r):
        return gpu.loss(ms, sd, r.astype(np.float32), tex, spp, seed, gimg)

    scale = np.abs(g).max()  # (the float32 loss resolves a column only relative to the largest gradient: the float64 test checks each column)
    for i in (0, 2):
        for j in range(11):
            fd = support.fd(f, rows.astype(np.float64), i, R0 + j, 1e-2)
            assert abs(g[i, j] - fd) <= 1e-2 * scale, (i, NAMES[j], g[i, j], fd, scale)


@pytest.mark.parametrize("gaussian,tc", [(False, 1), (True, 3)])
def test_nothing_else_moves(gaussian, tc):
    ms, sd, _ = gpu.load(corner(EVERY_LOBE, {}, base_tex=base_texture()), gaussian, tc)
    tex, gimg = gpu.rand_tex(sd, 8), gpu.rand_gimg(sd, 9)
    gtex0 = ms.geom.render_bwd(sd, None, 16, 2, gimg)
    gtex1, app1 = ms.geom.render_bwd(sd, None, 16, 2, gimg, appearance=True, tex=tex)
    gtex2, app2 = ms.geom.render_bwd(sd, None, 16, 2, gimg, appearance=True, tex=tex, material=True)
    assert app1.material is None and app2.material is not None
    # the texture gradient comes from the launches of a call without the bits; they sum with float atomics, whose order varies from run to run:
    # bit-identical where two plain calls are, else within that spread
    if torch.equal(ms.geom.render_bwd(sd, None, 16, 2, gimg), gtex0):
        assert torch.equal(gtex2, gtex0) and torch.equal(gtex1, gtex0)
    else:
        assert torch.allclose(gtex2, gtex0, rtol=1e-5, atol=1e-6 * float(gtex0.abs().max()))
    for a, b in [(app1.rows, app2.rows), (app1.spot, app2.spot), (app1.base_tex[0], app2.base_tex[0])]:
        assert float(a.abs().max()) > 0
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * float(a.abs().max()))


def test_mi_render_leaves_end_to_end():
    ms, sd, _ = gpu.load(corner(dict(EVERY_LOBE, anisotropic=0.0, clearcoat=0.0), {"roughness": 0.6}, shared=True), False, 3)
    p = mi.traverse(ms)
    spp, seed = 16, 4
    tex, gimg = gpu.rand_tex(sd, 10), gpu.rand_gimg(sd, 11)
    p["tex.data"] = tex
    p.update()
    sd = ms.scene_desc(tex_channels=3)
    gtex_ref, app = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex, material=True)
    plain0 = mi.render(ms, spp=spp, seed=seed).torch().clone()
    F, Y = "mat-Floor.brdf_0.", "mat-WallY.brdf_0."
    keys = {F + "roughness.value": 0.4, F + "metallic.value": 0.3, F + "clearcoat.value": 0.0, F + "anisotropic.value": 0.0, F + "specular": 0.6,
            Y + "eta": float(p[Y + "eta"])}
    leaves = {k: gpu.leaf(v) for k, v in keys.items()}
    base = p[F + "base_color.value"].t.clone()
    b_leaf, t_leaf = gpu.leaf(base.tolist()), tex.clone().requires_grad_(True)
    for k, v in leaves.items():
        p[k] = v
    p[F + "base_color.value"] = b_leaf
    p["tex.data"] = t_leaf
    p.update()
    img = mi.render(ms, spp=spp, seed=seed).torch()
    assert torch.equal(img.detach(), plain0)
    (img * gimg).sum().backward()
    rows = ms._material_meshes["mat-Floor"]
    assert len(rows) == 2
    M = app.material
    for k, leaf in leaves.items():
        name = k.split("brdf_0.")[1].replace(".value", "")
        col = scenes.MAT_COLUMN["eta" if name == "specular" else name] - R0
        r = ms._material_meshes[k.split(".")[0]]
        want = M[r, col].sum() * (scenes.specular_to_eta_grad(0.6) if name == "specular" else 1.0)
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape, k
        assert torch.allclose(leaf.grad, want.reshape(leaf.shape), rtol=1e-4, atol=1e-6 * float(M.abs().max())), (k, leaf.grad, want)
        assert float(want.abs()) > 0, k
    assert torch.allclose(b_leaf.grad, app.rows[rows].sum(0), rtol=1e-4, atol=1e-6)
    assert torch.allclose(t_leaf.grad, gtex_ref, rtol=1e-5, atol=1e-6 * float(gtex_ref.abs().max()))
    # specular and eta of one material in one update: specular drives the row, the eta leaf gets 0
    s_leaf, e_leaf = gpu.leaf(0.6), gpu.leaf(1.7)
    p[F + "specular"] = s_leaf
    p[F + "eta"] = e_leaf
    p.update()
    (mi.render(ms, spp=spp, seed=seed).torch() * gimg).sum().backward()
    assert float(e_leaf.grad) == 0.0 and float(s_leaf.grad) != 0.0
    assert abs(float(ms._albedo_host[rows[0], scenes.MAT_COLUMN["eta"]]) - scenes.specular_to_eta(0.6)) < 1e-6
    # plain values again: today's image, no leaves
    for k, v in keys.items():
        p[k] = mi.Float(v)
    p[F + "eta"] = mi.Float(scenes.specular_to_eta(0.6))
    p[F + "specular"] = mi.Float(0.6)
    p[F + "base_color.value"] = mi.Color3f(base)
    p["tex.data"] = tex
    p.update()
    assert not p._leaves
    plain = mi.render(ms, spp=spp, seed=seed).torch()
    assert not plain.requires_grad and torch.equal(plain, plain0)


def test_specular_at_zero_is_the_finite_limit():
    ms, sd, _ = gpu.load(corner({"roughness": 0.3, "specular": 0.0}, {"roughness": 0.6}), False, 1)
    p = mi.traverse(ms)
    tex, gimg = gpu.rand_tex(sd, 12), gpu.rand_gimg(sd, 13)
    p["tex.data"] = tex[..., 0].contiguous()
    leaf = gpu.leaf(0.0)
    p["mat-Floor.brdf_0.specular"] = leaf
    p.update()
    assert float(ms._albedo_host[0, scenes.MAT_COLUMN["eta"]]) == 1.0
    (mi.render(ms, spp=16, seed=3).torch() * gimg).sum().backward()
    g = float(leaf.grad)
    assert np.isfinite(g) and g > 0
    rows = ms._albedo_host.copy()
    sd = ms.scene_desc(tex_channels=1)
    ls = []
    for s in (0.0, 1e-3, 2e-3):
        r = rows.copy()
        r[0, scenes.MAT_COLUMN["eta"]] = scenes.specular_to_eta(s)
        ls.append(gpu.loss(ms, sd, r, tex, 16, 3, gimg))
    fd = (-3 * ls[0] + 4 * ls[1] - ls[2]) / 2e-3
    assert abs(g - fd) <= 2e-2 * abs(fd), (g, fd)


def test_inverse_rendering_recovers_roughness_and_metallic():
    ms, sd, _ = gpu.load(corner({"roughness": 0.35, "metallic": 0.2, "specular": 0.6}, {"roughness": 0.6}), False, 1)
    p = mi.traverse(ms)
    p["tex.data"] = gpu.rand_tex(sd, 14)[..., 0].contiguous()
    p.update()
    spp, seed = 16, 5
    target = mi.render(ms, spp=spp, seed=seed).torch().clone()
    r = float(gpu.fit(ms, "mat-Floor.brdf_0.roughness.value", 0.55, target, spp, seed, 0.02, 300))
    assert abs(r - 0.35) < 2e-2, r
    p["mat-Floor.brdf_0.roughness.value"] = mi.Float(0.35)
    p.update()
    m = float(gpu.fit(ms, "mat-Floor.brdf_0.metallic.value", 0.4, target, spp, seed, 0.02, 300))
    assert abs(m - 0.2) < 2e-2, m


def test_full_size_vocalfold_material_gradient():
    wl = workloads.vocalfold(device=DEV)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    ms = wl.mi_scene
    p = mi.traverse(ms)
    mat = next(m for m, pr in ms._material_principled.items() if pr)
    rng = np.random.default_rng(0)
    for name, hi in [("clearcoat.value", 1.0), ("clearcoat_gloss.value", 1.0), ("metallic.value", 0.5), ("specular", 1.0), ("roughness.value", 1.0),
                     ("anisotropic.value", 1.0), ("sheen.value", 0.5), ("spec_trans.value", 0.4), ("flatness.value", 1.0)]:
        p[f"{mat}.brdf_0.{name}"] = mi.Float(float(rng.uniform(0.0, hi)))
    p.update()
    tex = workloads.build_texture(wl).detach()
    sd = ms.scene_desc(tex_channels=1)
    assert (sd.cam.width, sd.cam.height) == (512, 512)
    mats, t3, spp, seed = ms.materials_arg(sd), tex.unsqueeze(-1).contiguous(), 64, 1
    gimg = torch.full((512, 512, 3), 1.0 / (512 * 512), device=DEV)
    _, app = ms.geom.render_bwd(sd, mats, spp, seed, gimg, appearance=True, tex=t3, material=True)
    g = app.material.double().cpu().numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    i, j = np.unravel_index(np.abs(g).argmax(), g.shape)
    rows = ms._albedo_host.copy()

    def f(r):
        s2 = copy_desc(sd)
        if sd.n_mat_h > 0:
            scene_desc.set_host_materials(s2, r.astype(np.float32))
            m2 = None
        else:
            m2 = torch.from_numpy(r.astype(np.float32)).to(DEV)
        return float((ms.geom.render_fwd(s2, m2, t3, spp, seed).double() * gimg.double()).sum())

    fd = support.fd(f, rows.astype(np.float64), i, R0 + j, 1e-2)
    assert abs(g[i, j] - fd) <= 1e-2 * abs(fd) + 1e-7, (NAMES[j], g[i, j], fd)


def test_refusals():
    ms, sd, _ = gpu.load(corner({"roughness": 0.35}, {}), False, 1)
    p = mi.traverse(ms)
    tex, gimg = gpu.rand_tex(sd), gpu.rand_gimg(sd)
    g = ms.geom
    p["tex.data"] = tex[..., 0].contiguous()
    p["mat-Floor.brdf_0.roughness.value"] = gpu.leaf(0.35)
    p.update()
    with pytest.raises(ValueError):
        mi.render(ms, spp=4, integrator=mi.load_dict({"type": "path", "max_depth": 3}))
    with pytest.raises(ValueError):
        g.render_bwd(sd, None, 4, 0, gimg, material=True)
    os.environ["FFX_DETERMINISTIC"] = "1"
    try:
        with pytest.raises(ValueError):
            mi.render(ms, spp=4)
    finally:
        os.environ.pop("FFX_DETERMINISTIC", None)
    n = tex.numel() + _abi.appearance_floats(sd.n_shapes) + _abi.material_floats(sd.n_shapes)
    out = torch.zeros(n, device=DEV)
    src = torch.cat([gimg.reshape(-1), tex.reshape(-1)])
    img = torch.empty((sd.cam.height, sd.cam.width, 3), device=DEV)
    blob, strm, pp = C.c_void_p(g.blob.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p
    A, M = _abi.RENDER_GRAD_APPEARANCE, _abi.RENDER_GRAD_MATERIAL
    rc = api().call_rc("ffx_render_bwd", blob, C.byref(g.info), C.byref(sd), None, 4, 0, M, pp(src.data_ptr()), pp(out.data_ptr()), strm, allow=(FFX_ERR_ARG,))
    assert rc == FFX_ERR_ARG
    rc = api().call_rc("ffx_render_bwd", blob, C.byref(g.info), C.byref(sd), None, 4, 0, A | M | _abi.render_path(3, 5), pp(src.data_ptr()), pp(out.data_ptr()),
                       strm, allow=(_abi.FFX_ERR_UNSUPPORTED,))
    assert rc == _abi.FFX_ERR_UNSUPPORTED
    cache = torch.empty(max(int(api().lib.ffx_render_cache_bytes_sd(C.byref(sd), 4)), 64), dtype=torch.uint8, device=DEV)
    for flags in (M, A | M):
        rc = api().call_rc("ffx_render_fwd", blob, C.byref(g.info), C.byref(sd), None, pp(tex.data_ptr()), 4, 0, flags, pp(img.data_ptr()), strm,
                           allow=(_abi.FFX_ERR_UNSUPPORTED,))
        assert rc == _abi.FFX_ERR_UNSUPPORTED
        rc = api().call_rc("ffx_render_fwd_cache", blob, C.byref(g.info), C.byref(sd), None, pp(tex.data_ptr()), 4, 0, flags, pp(img.data_ptr()),
                           pp(cache.data_ptr()), strm, allow=(_abi.FFX_ERR_UNSUPPORTED,))
        assert rc == _abi.FFX_ERR_UNSUPPORTED
        rc = api().call_rc("ffx_render_bwd_cached", C.byref(sd), None, pp(cache.data_ptr()), 4, pp(gimg.data_ptr()), pp(out.data_ptr()), None, flags, None, strm,
                           allow=(_abi.FFX_ERR_UNSUPPORTED,))
        assert rc == _abi.FFX_ERR_UNSUPPORTED
        work = torch.empty(api().lib.ffx_render_bwd_det_bytes(C.byref(sd)), dtype=torch.uint8, device=DEV)
        rc = api().call_rc("ffx_render_bwd_det", blob, C.byref(g.info), C.byref(sd), None, 4, 0, flags, pp(gimg.data_ptr()), pp(out.data_ptr()),
                           pp(work.data_ptr()), strm, allow=(_abi.FFX_ERR_UNSUPPORTED,))
        assert rc == _abi.FFX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
