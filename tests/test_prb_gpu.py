"""The `prb` integrator (FFX_RENDER_GRAD_PRB) on the GPU: its forward is the path forward bit for bit; the appearance and material
blocks at max_depth 3 and 4 against central differences of the GPU forward on the same paths (roulette off) and of the float64 restatement with the
roulette detached (tests/ref_prb.py); the texture gradient of the same launch against render_bwd's; light that arrives by a bounce only; mi.render's
leaves end to end; an inverse rendering at depth 3; a full-size render."""
import numpy as np
import pytest
import torch

from fireflies_amd import mi, scene_desc, scenes, workloads
from fireflies_amd import functional as Fn
from tests import corner_scenes as cs
from tests import gpu_support as gpu
from tests import ref_path as rp
from tests import ref_prb
from tests import support
from tests.corner_scenes import NAMES, R0
from tests.gpu_support import DEV
from tests.support import copy_desc

pytestmark = pytest.mark.gpu


def _scene(name, gaussian, **kw):
    """cs.scene(name) loaded with a 1-channel texture -> (scene, loaded scene, description, world arrays, the floor's base texture or None)"""
    sc = cs.scene(name, **kw)
    ms, sd, world = gpu.load(sc, gaussian, 1)
    return sc, ms, sd, world, sc.meshes[0].base_tex



def _blocks(ms, sd, spp, seed, gimg, tex, depth, rr, material=True):
    if depth == 2:  # (the existing direct-light adjoint)
        return ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex, material=material)
    return ms.geom.render_bwd_prb(sd, None, spp, seed, gimg, tex, depth, rr, material=material)


@pytest.mark.parametrize("gaussian", [False, True])
def test_prb_forward_is_the_path_forward_bitwise(gaussian):
    _, ms, sd, _, _ = _scene("defaults", gaussian)
    tex = gpu.rand_tex(sd)
    ms._params["tex.data"] = tex[..., 0].clone()
    for depth, rr in ((3, 5), (4, 1), (2, 5)):
        a = mi.render(ms, spp=16, seed=3, integrator=mi.load_dict({"type": "path", "max_depth": depth, "rr_depth": rr})).torch().clone()
        b = mi.render(ms, spp=16, seed=3, integrator=mi.load_dict({"type": "prb", "max_depth": depth, "rr_depth": rr})).torch()
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
        assert torch.equal(ms.geom.render_fwd(sd, None, tex, 16, 3, max_depth=depth, rr_depth=rr), a)
        assert torch.equal(Fn.render(tex, ms.geom, sd, None, 16, 3, max_depth=depth, rr_depth=rr), a)
    # with a tex.data leaf only (what PatternOptimizer differentiates) prb is path: same image, same texture gradient
    leaf = tex[..., 0].clone().requires_grad_(True)
    ms._params["tex.data"] = leaf
    gimg = gpu.rand_gimg(sd, 1)
    grads = []
    for t in ("path", "prb"):
        leaf.grad = None
        img = mi.render(ms, spp=16, seed=3, integrator=mi.load_dict({"type": t, "max_depth": 3})).torch()
        (img * gimg).sum().backward()
        grads.append((img.detach().clone(), leaf.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.allclose(grads[0][1], grads[1][1], rtol=1e-5, atol=1e-6 * float(grads[0][1].abs().max()))


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("name,gaussian", [("lambert", False), ("lambert", True), ("defaults", False), ("defaults", True), ("every_lobe", False),
                                           ("every_lobe", True), ("textured", False), ("textured", True)])
def test_blocks_match_central_differences_of_the_gpu_forward(name, gaussian, depth):
    """roulette off (rr_depth = max_depth): no parameter moves a path, so central differences of render_fwd(max_depth) walk identical paths.
    Tolerances: the existing direct-light tests' — rows 1e-3 of the largest difference, spot 1e-3, the base texture's directional derivative as
    tests/test_appearance_gpu.py, material columns 2e-3 scale + 1e-9 per column.  The float32 image leaves an ABSOLUTE noise floor in a difference
    (rounding of the loss / 2h, the same for every column whatever its size), which is above 2e-3 of the small columns: it is measured in the same
    run as the largest column error of the EXISTING direct-light adjoint against the same differences at max_depth 2, and a column may miss its
    2e-3 bound by at most twice that floor.  Every figure is printed before it is asserted.  Measured (MI355X, five-point differences at
    h = 1e-2): 127 of the 132 columns of the 12 principled cases are inside 2e-3 scale + 1e-9 on their own; the other five are the sheen_tint
    column (gradient 2e-3 .. 6e-3), errors 9e-6 .. 3e-5 against 2e-3 scale = 4e-6 .. 1e-5, with depth-2 floors of 5e-5 .. 1.3e-4 in the same runs."""
    _, ms, sd, _, bt = _scene(name, gaussian)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    spp, seed, rr = 16, 5, depth
    rows = ms._albedo_host.astype(np.float64)
    gtex, app = _blocks(ms, sd, spp, seed, gimg, tex, depth, rr)
    # 4. the texture gradient of the same launch is render_bwd's
    gtex_ref = ms.geom.render_bwd(sd, None, spp, seed, gimg, max_depth=depth, rr_depth=rr)
    ts = float(gtex_ref.abs().max())
    print("gtex: max |prb - render_bwd|", float((gtex - gtex_ref).abs().max()), "scale", ts)
    assert ts > 0 and float((gtex - gtex_ref).abs().max()) <= 1e-3 * ts
    # rows' colours (central differences are exact for the polynomial the image is in a colour up to h^2 f''' / 6 at depth 4); the floor's colour may be
    # its texture
    g, scale = gpu.rows_central_differences(ms, sd, app, rows, tex, spp, seed, gimg, depth, rr, skip=(0,) if bt is not None else ())
    # the bounces matter: the direct-light adjoint's rows differ
    _, app2 = _blocks(ms, sd, spp, seed, gimg, tex, 2, 5)
    assert np.abs(g - app2.rows.double().cpu().numpy()).max() > 1e-2 * scale
    # the spot's intensity
    gpu.spot_differences(ms, sd, app, None, tex, spp, seed, gimg, depth, rr)
    # a base-colour texture: directional derivatives
    if bt is not None:
        h = 1e-2
        t = ms._base_tex[0][1]
        gb = app.base_tex[0]
        assert float(app.rows[0].abs().max()) == 0 and float(gb.abs().sum()) > 0
        orig = t.clone()
        for s in range(2):
            v = torch.randn(t.shape, generator=torch.Generator().manual_seed(s)).to(DEV)
            ls = []
            for sign in (1, -1):
                t.copy_(orig + sign * h * v)
                ls.append(float((ms.geom.render_fwd(sd, None, tex, spp, seed, max_depth=depth, rr_depth=rr).double() * gimg.double()).sum()))
            t.copy_(orig)
            f = (ls[0] - ls[1]) / (2 * h)
            dd = float((gb.double() * v.double()).sum())
            print("base_tex dd", dd, f)
            assert abs(dd - f) <= 1e-3 * max(abs(f), float((gb.double().abs() * v.double().abs()).sum()) * 1e-2), (dd, f)
    # the eleven BSDF columns of the principled rows
    m = app.material.double().cpu().numpy()
    lam = rows[:, scenes.MAT_COLUMN["model"]] == 0 if rows.shape[1] > 3 else np.ones(rows.shape[0], bool)
    assert np.abs(m[lam]).max() == 0
    if lam.all():
        return
    m2 = app2.material.double().cpu().numpy()
    fdm, fdm2 = np.zeros_like(m), np.zeros_like(m)
    for i in np.flatnonzero(~lam):
        for j in range(11):
            fdm[i, j] = support.fd4(lambda r: gpu.loss(ms, sd, r, tex, spp, seed, gimg, depth, rr), rows, i, R0 + j, 1e-2)
            fdm2[i, j] = support.fd4(lambda r: gpu.loss(ms, sd, r, tex, spp, seed, gimg, 2, 5), rows, i, R0 + j, 1e-2)
    floor = np.abs(m2 - fdm2).max()  # (the existing adjoint against the same kind of difference, this run: the differences' noise floor)
    for j in range(11):
        sc_j = np.abs(fdm[:, j]).max()
        err, err2 = np.abs(m[:, j] - fdm[:, j]).max(), np.abs(m2[:, j] - fdm2[:, j]).max()
        print(f"{NAMES[j]:16s} err {err:.3e}  2e-3 scale {2e-3 * sc_j + 1e-9:.3e}  depth-2 err of the column {err2:.3e}  floor {floor:.3e}")
    for j in range(11):
        sc_j = np.abs(fdm[:, j]).max()
        assert np.abs(m[:, j] - fdm[:, j]).max() <= max(2e-3 * sc_j + 1e-9, 2 * floor), (NAMES[j], m[:, j], fdm[:, j], floor)
    assert (np.abs(m) > 0).sum() >= 8


@pytest.mark.parametrize("name,gaussian,depth,rr", [("lambert", False, 3, 1), ("defaults", True, 3, 1), ("every_lobe", False, 4, 2), ("defaults", False, 4, 4)])
def test_blocks_match_the_float64_restatement(name, gaussian, depth, rr):
    """against central differences of tests/ref_prb.py (roulette decisions and q frozen at the unperturbed rows).  float32 and float64 paths can part
    after a bounce, which test_path_render_matches_float64_restatement grants the texture gradient as 3 % of its L1 norm: every block is held to the
    same 3 %, and so is the texture gradient of the same call (the undisputed quantity)."""
    _, ms, sd, world, _ = _scene(name, gaussian, W=16, H=16)
    tex, gimg = gpu.rand_tex(sd, 1), gpu.rand_gimg(sd, 2)
    spp, seed = 8, 7
    gtex, app = _blocks(ms, sd, spp, seed, gimg, tex, depth, rr)
    rows = ms._albedo_host.astype(np.float64)
    tex_np, gimg_np = tex.cpu().numpy(), gimg.double().cpu().numpy()
    stddev = 0.5 if gaussian else None
    gt_ref = rp.render_bwd(*world, sd, rows, spp, seed, gimg_np, depth, rr, gaussian_stddev=stddev)
    e, s = np.abs(gtex.double().cpu().numpy() - gt_ref).sum(), np.abs(gt_ref).sum()
    print("gtex L1 err", e, "of", s)
    assert s > 0 and e <= 0.03 * s

    def f(r, sd_=sd):
        return float((ref_prb.render_fwd_frozen(*world, sd_, r, rows, tex_np, spp, seed, depth, rr, gaussian_stddev=stddev) * gimg_np).sum())

    g = app.rows.double().cpu().numpy()
    fd = np.zeros_like(g)
    for i in range(rows.shape[0]):
        for k in range(3):
            lo, hi = rows.copy(), rows.copy()
            lo[i, k] -= 1e-3
            hi[i, k] += 1e-3
            fd[i, k] = (f(hi) - f(lo)) / 2e-3
    print("rows L1 err", np.abs(g - fd).sum(), "of", np.abs(fd).sum())
    assert np.abs(fd).sum() > 0 and np.abs(g - fd).sum() <= 0.03 * np.abs(fd).sum(), (g, fd)
    gs, fs = app.spot.double().cpu().numpy(), np.zeros(3)
    for c in range(3):
        lo, hi = copy_desc(sd), copy_desc(sd)
        lo.spot.intensity[c] -= 0.5
        hi.spot.intensity[c] += 0.5
        fs[c] = f(rows, hi) - f(rows, lo)
    print("spot L1 err", np.abs(gs - fs).sum(), "of", np.abs(fs).sum())
    assert np.abs(fs).sum() > 0 and np.abs(gs - fs).sum() <= 0.03 * np.abs(fs).sum(), (gs, fs)
    lam = rows[:, scenes.MAT_COLUMN["model"]] == 0 if rows.shape[1] > 3 else np.ones(rows.shape[0], bool)
    if lam.all():
        return
    m = _blocks(ms, sd, spp, seed, gimg, tex, depth, rr)[1].material.double().cpu().numpy()
    fdm = np.zeros_like(m)
    for i in np.flatnonzero(~lam):
        for j in range(11):
            fdm[i, j] = support.fd(f, rows, i, R0 + j, 1e-4)
    print("material L1 err", np.abs(m - fdm).sum(), "of", np.abs(fdm).sum(), "\n", m, "\n", fdm)
    assert np.abs(fdm).sum() > 0 and np.abs(m - fdm).sum() <= 0.03 * np.abs(fdm).sum()


@pytest.mark.parametrize("gaussian", [False, True])
def test_the_relaying_surface_has_a_gradient_only_through_the_bounce(gaussian):
    """bounce_scene: the camera sees the wall, the emitters light the floor only.  The wall's base colour scales every pixel, and so does the floor's,
    which relays the light — at direct light both gradients are exactly 0, at depth 3 they are the central differences"""
    ms, sd, _ = gpu.load(cs.relay(True, True), gaussian, 1)
    tex, gimg = gpu.rand_tex(sd, 4), gpu.rand_gimg(sd, 5)
    spp, seed = 32, 5
    mats = ms.materials_arg(sd)
    _, app2 = ms.geom.render_bwd(sd, mats, spp, seed, gimg, appearance=True, tex=tex)
    assert float(app2.rows.abs().max()) == 0.0 and float(app2.spot.abs().max()) == 0.0
    gtex, app3 = ms.geom.render_bwd_prb(sd, mats, spp, seed, gimg, tex, 3)
    g = app3.rows.double().cpu().numpy()
    assert (g > 0).all() and float(app3.spot.min()) > 0
    rows = ms._albedo_host.copy() if sd.n_mat_h > 0 else ms.albedo.cpu().numpy().copy()
    h = 1e-2
    fd = np.zeros_like(g)

    def loss(r):
        s2 = copy_desc(sd)
        if sd.n_mat_h > 0:
            scene_desc.set_host_materials(s2, r)
            m2 = None
        else:
            m2 = torch.from_numpy(r).to(DEV)
        return float((ms.geom.render_fwd(s2, m2, tex, spp, seed, max_depth=3).double() * gimg.double()).sum())

    for i in range(2):
        for k in range(3):
            lo, hi = rows.copy(), rows.copy()
            lo[i, k] -= h
            hi[i, k] += h
            fd[i, k] = (loss(hi) - loss(lo)) / (2 * h)
    print(g, fd)
    assert np.abs(g - fd).max() <= 1e-3 * np.abs(fd).max(), (g, fd)
    assert float((gtex - ms.geom.render_bwd(sd, mats, spp, seed, gimg, max_depth=3)).abs().max()) <= 1e-3 * float(gtex.abs().max())


def test_mi_render_leaves_end_to_end(monkeypatch):
    sc = cs.corner(dict(cs.EVERY_LOBE, anisotropic=0.0, clearcoat=0.0), {"roughness": 0.6}, base_tex=cs.base_texture())
    ms, sd, _ = gpu.load(sc, False, 3)
    p = mi.traverse(ms)
    spp, seed = 16, 4
    it = mi.load_dict({"type": "prb", "max_depth": 3, "rr_depth": 2})
    tex, gimg = gpu.rand_tex(sd, 10), gpu.rand_gimg(sd, 11)
    p["tex.data"] = tex
    p.update()
    sd = ms.scene_desc(tex_channels=3)
    gtex_ref, app = ms.geom.render_bwd_prb(sd, None, spp, seed, gimg, tex, 3, 2, material=True)
    plain0 = mi.render(ms, spp=spp, seed=seed, integrator=it).torch().clone()
    F, Y = "mat-Floor.brdf_0.", "mat-WallY.brdf_0."
    keys = {F + "roughness.value": 0.4, F + "metallic.value": 0.3, F + "specular": 0.6, Y + "roughness.value": 0.6}
    leaves = {k: gpu.leaf(v) for k, v in keys.items()}
    yb = p[Y + "base_color.value"].t.clone()
    cb = p["mat-Cube.brdf_0.base_color.value"].t.clone()
    y_leaf, c_leaf = gpu.leaf(yb.tolist()), gpu.leaf(cb.tolist())
    s_leaf = gpu.leaf(p["emit-Spot.intensity.value"].t.tolist())
    bt_leaf = p[F + "base_color.data"].t.clone().requires_grad_(True) if hasattr(p[F + "base_color.data"], "t") else None
    t_leaf = tex.clone().requires_grad_(True)
    for k, v in leaves.items():
        p[k] = v
    p[Y + "base_color.value"] = y_leaf
    p["mat-Cube.brdf_0.base_color.value"] = c_leaf
    p["emit-Spot.intensity.value"] = s_leaf
    if bt_leaf is not None:
        p[F + "base_color.data"] = mi.TensorXf(bt_leaf)
    p["tex.data"] = t_leaf
    p.update()
    sd = ms.scene_desc(tex_channels=3)  # (the description points at the base texture the update installed)
    # `path` with leaves is refused, and says where to go
    with pytest.raises(ValueError, match="prb"):
        mi.render(ms, spp=spp, seed=seed, integrator=mi.load_dict({"type": "path", "max_depth": 3, "rr_depth": 2}))
    img = mi.render(ms, spp=spp, seed=seed, integrator=it).torch()
    assert torch.equal(img.detach(), plain0)
    (img * gimg).sum().backward()
    M = app.material
    for k, leaf in leaves.items():
        name = k.split("brdf_0.")[1].replace(".value", "")
        col = scenes.MAT_COLUMN["eta" if name == "specular" else name] - R0
        r = ms._material_meshes[k.split(".")[0]]
        want = M[r, col].sum() * (scenes.specular_to_eta_grad(0.6) if name == "specular" else 1.0)
        assert leaf.grad is not None and float(want.abs()) > 0, k
        assert torch.allclose(leaf.grad, want.reshape(leaf.shape), rtol=1e-4, atol=1e-6 * float(M.abs().max())), (k, leaf.grad, want)
    for leaf, mat in ((y_leaf, "mat-WallY"), (c_leaf, "mat-Cube")):
        want = app.rows[ms._material_meshes[mat]].sum(0)
        assert float(want.abs().max()) > 0 and torch.allclose(leaf.grad, want, rtol=1e-4, atol=1e-6)
    assert torch.allclose(s_leaf.grad, app.spot, rtol=1e-4, atol=1e-6)
    if bt_leaf is not None:
        assert float(app.base_tex[0].abs().max()) > 0
        assert torch.allclose(bt_leaf.grad, app.base_tex[0], rtol=1e-4, atol=1e-6 * float(app.base_tex[0].abs().max()))
    assert torch.allclose(t_leaf.grad, gtex_ref, rtol=1e-5, atol=1e-5 * float(gtex_ref.abs().max()))
    # prb at max_depth 2 takes the direct-light route
    for leaf in (y_leaf, c_leaf, s_leaf, t_leaf, *leaves.values()):
        leaf.grad = None
    (mi.render(ms, spp=spp, seed=seed, integrator=mi.load_dict({"type": "prb", "max_depth": 2})).torch() * gimg).sum().backward()
    _, app2 = ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex, material=True)
    assert torch.allclose(y_leaf.grad, app2.rows[ms._material_meshes["mat-WallY"]].sum(0), rtol=1e-4, atol=1e-6)
    # no deterministic adjoint
    monkeypatch.setenv("FFX_DETERMINISTIC", "1")
    with pytest.raises(ValueError):
        mi.render(ms, spp=spp, seed=seed, integrator=it)
    with pytest.raises(ValueError):
        ms.geom.render_bwd_prb(sd, None, spp, seed, gimg, tex, 3)
    monkeypatch.delenv("FFX_DETERMINISTIC")
    with pytest.raises(ValueError):
        ms.geom.render_bwd_prb(sd, None, spp, seed, gimg, tex, 3, deterministic=True)
    with pytest.raises(ValueError):
        ms.geom.render_bwd_prb(sd, None, spp, seed, gimg, tex, 9)
    # the direct-light doors stay shut at depth 3
    with pytest.raises(ValueError):
        ms.geom.render_bwd(sd, None, spp, seed, gimg, appearance=True, tex=tex, max_depth=3)
    # a pose update between the render and its backward raises
    img = mi.render(ms, spp=spp, seed=seed, integrator=it).torch()
    ms.geom.version += 1
    with pytest.raises(RuntimeError):
        (img * gimg).sum().backward()
    ms.geom.version -= 1


def test_inverse_rendering_at_depth_3():
    """the fits of tests/test_appearance_gpu.py (a base colour to 1e-2) and tests/test_material_grad_gpu.py (a roughness to 2e-2), with a bounce"""
    sc = cs.corner({"roughness": 0.35, "metallic": 0.2, "specular": 0.6}, {"roughness": 0.6})
    ms, sd, _ = gpu.load(sc, False, 1)
    it = mi.load_dict({"type": "prb", "max_depth": 3})
    p = mi.traverse(ms)
    p["tex.data"] = gpu.rand_tex(sd, 14)[..., 0].contiguous()
    p.update()
    spp, seed = 16, 5
    target = mi.render(ms, spp=spp, seed=seed, integrator=it).torch().clone()
    key = "mat-WallX.brdf_0.base_color.value"
    b_true = p[key].t.clone()
    b = gpu.fit(ms, key, (b_true + torch.tensor([0.15, -0.2, 0.1])).tolist(), target, spp, seed, 0.03, 300, it)
    assert float((b.cpu() - b_true.cpu()).abs().max()) < 1e-2, (b, b_true)
    p[key] = mi.Color3f(b_true)
    p.update()
    r = float(gpu.fit(ms, "mat-Floor.brdf_0.roughness.value", 0.55, target, spp, seed, 0.02, 300, it))
    assert abs(r - 0.35) < 2e-2, r


def test_full_size_vocalfold_at_depth_3():
    wl = workloads.vocalfold(device=DEV)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    ms = wl.mi_scene
    tex = workloads.build_texture(wl).detach()
    sd = ms.scene_desc(tex_channels=1)
    assert (sd.cam.width, sd.cam.height) == (512, 512)
    mats, t3, spp, seed, depth = ms.materials_arg(sd), tex.unsqueeze(-1).contiguous(), 64, 1, 3
    gimg = torch.full((512, 512, 3), 1.0 / (512 * 512), device=DEV)
    gtex, app = ms.geom.render_bwd_prb(sd, mats, spp, seed, gimg, t3, depth, depth, material=True)  # (roulette off: rr_depth = max_depth)
    g, m = app.rows.double().cpu().numpy(), app.material.double().cpu().numpy()
    assert all(np.isfinite(x).all() for x in (g, m, app.spot.cpu().numpy(), gtex.cpu().numpy())) and np.abs(g).max() > 0
    rows = ms._albedo_host.copy() if sd.n_mat_h > 0 else ms.albedo.cpu().numpy().copy()
    # one random direction over the rows' colours and the BSDF columns of the principled rows (inside their ranges)
    rng = np.random.default_rng(3)
    v = np.zeros_like(rows)
    v[:, :3] = rng.uniform(-1, 1, (rows.shape[0], 3))
    if rows.shape[1] > 3:
        pr = rows[:, scenes.MAT_COLUMN["model"]] != 0
        for j in range(11):
            col = rows[:, R0 + j]
            if R0 + j == scenes.MAT_COLUMN["eta"]:
                continue  # (at eta = 1 the column holds a limit, not the derivative: DESIGN.md 4.5.1)
            inside = pr & (col > 0.05) & (col < 0.95)
            v[inside, R0 + j] = rng.uniform(-1, 1, int(inside.sum()))
    h = 1e-2
    ls = []
    for sign in (1, -1):
        r = (rows + sign * h * v).astype(np.float32)
        s2 = copy_desc(sd)
        if sd.n_mat_h > 0:
            scene_desc.set_host_materials(s2, r)
            m2 = None
        else:
            m2 = torch.from_numpy(r).to(DEV)
        ls.append(float((ms.geom.render_fwd(s2, m2, t3, spp, seed, max_depth=depth, rr_depth=depth).double() * gimg.double()).sum()))
    fd = (ls[0] - ls[1]) / (2 * h)
    dd = float((g * v[:, :3]).sum() + ((m * v[:, R0:R0 + 11]).sum() if rows.shape[1] > 3 else 0.0))
    print("directional derivative", dd, "central difference", fd)
    assert abs(dd - fd) <= 1e-2 * abs(fd) + 1e-7, (dd, fd)
