"""Forward mode (FFX_RENDER_TANGENT) on the GPU: the primal is render_fwd's image bit for bit and the tangent image repeats bit for
bit; the linear special cases against the existing forward; the dot-product identity <J dtheta, g> = <dtheta, J^T g> against the existing adjoints
(render_bwd(appearance=True, material=True) at direct light, render_bwd_prb through the bounces), all blocks at once and one at a time, on rows
inside their ranges and on rows pinned at the bounds where the adjoint holds one-sided values; every pixel against the float64 tangent of
tests/ref_prb.py; mi.render_forward end to end; a full-size render.  Every compared figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fireflies_amd import mi, ops, scenes, workloads
from tests import corner_scenes as cs
from tests import gpu_support as gpu
from tests import ref_prb
from tests.corner_scenes import R0
from tests.gpu_support import DEV
from tests.support import copy_desc

pytestmark = pytest.mark.gpu
FILMS = [False, True]


def _scene(name, gaussian, **kw):
    """cs.scene(name) loaded with a 1-channel texture -> (scene, loaded scene, description, world arrays)"""
    sc = cs.scene(name, **kw)
    return (sc, *gpu.load(sc, gaussian, 1))


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("name", ["lambert", "every_lobe", "textured"])
def test_primal_is_render_fwd_bitwise_and_the_tangent_repeats_bitwise(name, gaussian):
    _, ms, sd, _ = _scene(name, gaussian)
    tex = gpu.rand_tex(sd, 1)
    dtex, tan = gpu.tangent(ms, sd, 7)
    for depth, rr in ((2, 5), (3, 5), (4, 1)):
        ref = ms.geom.render_fwd(sd, None if sd.n_mat_h > 0 else ms.albedo, tex, 16, 3, max_depth=depth, rr_depth=rr).clone()
        img, dimg = gpu.jvp(ms, sd, tex, 16, 3, dtex, tan, depth, rr)
        img, dimg = img.clone(), dimg.clone()
        img2, dimg2 = gpu.jvp(ms, sd, tex, 16, 3, dtex, tan, depth, rr)
        print(name, gaussian, depth, "max |img|", float(ref.abs().max()), "max |dimg|", float(dimg.abs().max()))
        assert float(ref.abs().max()) > 0 and torch.equal(img, ref) and torch.equal(img2, ref)
        assert torch.isfinite(dimg).all() and float(dimg.abs().max()) > 0 and torch.equal(dimg, dimg2)
        # a zero tangent gives a zero tangent image, exactly
        _, d0 = gpu.jvp(ms, sd, tex, 16, 3, None, None, depth, rr)
        assert float(d0.abs().max()) == 0.0


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth", [2, 3])
def test_linear_special_cases_against_the_forward(gaussian, depth):
    """identities of the model: the image is linear in the texture and in the spot's intensity, and (direct light, Lambert rows) in the base colours.
    1e-4 of the image scale per pixel: both sides are float32 sums of the same terms in another order"""
    _, ms, sd, _ = _scene("every_lobe", gaussian)
    tex = gpu.rand_tex(sd, 1)
    spp, seed, rr = 16, 5, depth
    mats = None if sd.n_mat_h > 0 else ms.albedo
    fwd = lambda s, t, m=mats: ms.geom.render_fwd(s, m, t, spp, seed, max_depth=depth, rr_depth=rr).clone()  # noqa: E731

    def check(what, dimg, want):
        scale, err = float(want.abs().max()), float((dimg - want).abs().max())
        print(f"{what} (depth {depth}, gaussian {gaussian}): max |dimg - forward| {err:.3e}  1e-4 scale {1e-4 * scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale

    dtex = gpu.rand(tuple(tex.shape), 3, 0.0, 1.0)
    _, dimg = gpu.jvp(ms, sd, tex, spp, seed, dtex, None, depth, rr)
    check("dtex", dimg, fwd(sd, dtex) - fwd(sd, torch.zeros_like(tex)))
    dspot = torch.tensor([0.5, 2.0, 1.25], device=DEV)
    _, dimg = gpu.jvp(ms, sd, tex, spp, seed, None, ops.AppearanceGrad(None, dspot, None, None), depth, rr)
    s2 = copy_desc(sd)
    for c in range(3):
        s2.spot.intensity[c] = float(dspot[c])
    check("dspot", dimg, fwd(s2, torch.zeros_like(tex)))
    if depth != 2:
        return
    _, ms, sd, _ = _scene("lambert", gaussian)
    tex = gpu.rand_tex(sd, 1)
    db = gpu.rand((sd.n_shapes, 3), 4, 0.1, 0.9)
    _, dimg = gpu.jvp(ms, sd, tex, spp, seed, None, ops.AppearanceGrad(db, None, None, None))
    s2 = copy_desc(sd)
    s2.n_mat_h = 0  # (the rows come from the table given)
    check("base colours of Lambert rows", dimg, ms.geom.render_fwd(s2, db.contiguous(), tex, spp, seed))


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth,rr", [(2, 5), (3, 3), (3, 1), (4, 4), (4, 2)])
@pytest.mark.parametrize("name", ["lambert", "every_lobe", "textured", "bounce"])
def test_dot_product_identity_against_the_adjoints(name, depth, rr, gaussian):
    """random gimg, a random tangent in every block and random dtex; then one block at a time, so that a wrong block cannot hide behind a large one.
    Roulette off (rr_depth = max_depth) and on"""
    _, ms, sd, _ = _scene(name, gaussian)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4) - 1.0  # (gimg in -0.5 .. 0.5)
    spp, seed = 16, 5
    dtex, tan = gpu.tangent(ms, sd, 11)
    what = f"{name} depth {depth} rr {rr} gaussian {gaussian}"
    if name == "bounce" and depth == 2:  # (the emitters light the floor only and the camera sees the wall: nothing arrives without a bounce)
        gtex, app = gpu.adjoint(ms, sd, spp, seed, gimg, tex, depth, rr)
        _, dimg = gpu.jvp(ms, sd, tex, spp, seed, dtex, tan, depth, rr)
        assert all(float(g.abs().max()) == 0.0 for _, _, g in gpu.pairs(dtex, tan, gtex, app)) and float(dimg.abs().max()) == 0.0
        return
    gpu.identity(ms, sd, tex, spp, seed, gimg, dtex, tan, depth, rr, what + " [all blocks]")
    gtex, app = gpu.adjoint(ms, sd, spp, seed, gimg, tex, depth, rr)
    live = 0
    for n, _, g in gpu.pairs(dtex, tan, gtex, app):
        if float(g.abs().max()) == 0.0:
            print(f"{what} [{n}]: the adjoint's block is zero; the tangent image must be too")
            _, dimg = gpu.jvp(ms, sd, tex, spp, seed, *gpu.one_block(dtex, tan, n), depth, rr)
            assert float((dimg.double() * gimg.double()).sum().abs()) <= 1e-12
            continue
        gpu.identity(ms, sd, tex, spp, seed, gimg, *gpu.one_block(dtex, tan, n), depth, rr, f"{what} [{n}]")
        live += 1
    assert live >= 3


# two corners of rows pinned at bounds.  0: both principled rows at eta = 1 (specular = 0), where the forward skips the main specular lobe — the wall
# (spec_trans = 1, no clearcoat, no sheen) then has A = B = 0 exactly and only one-sided tangents; 1: eta away from 1, so that anisotropic = 0 has a
# lobe to act on (at eta = 1 the adjoint's anisotropic column is 0: no lobe, no frame)
BOUNDS = (({"roughness": 0.4, "clearcoat": 0.0, "sheen": 0.0, "anisotropic": 0.0, "metallic": 1.0, "specular": 0.0, "flatness": 0.0, "spec_tint": 0.0},
           {"roughness": 0.3, "metallic": 0.0, "specular": 0.0, "spec_trans": 1.0, "clearcoat": 0.0, "sheen": 0.0, "spec_tint": 0.5}),
          ({"roughness": 0.4, "clearcoat": 0.0, "sheen": 0.0, "anisotropic": 0.0, "metallic": 1.0, "specular": 0.5, "flatness": 0.0, "spec_tint": 0.0},
           {"roughness": 0.3, "metallic": 0.0, "specular": 0.6, "anisotropic": 0.0, "clearcoat": 0.0, "sheen": 0.0, "flatness": 0.0, "spec_tint": 0.0}))
BOUNDS_COLUMNS = (("clearcoat", "sheen", "metallic", "eta"), ("clearcoat", "sheen", "metallic", "anisotropic", "flatness", "spec_tint"))


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth,rr", [(2, 5), (3, 3), (4, 2)])
@pytest.mark.parametrize("corner", [0, 1])
def test_one_sided_bounds_and_eta_1_follow_the_adjoint(corner, depth, rr, gaussian):
    """rows pinned at clearcoat = 0, sheen = 0, anisotropic = 0, flatness = 0, spec_tint = 0, metallic = 1 / 0, spec_trans = 1 and eta = 1
    (specular = 0): the tangent takes the adjoint's one-sided values (at eta = 1: its limit), by the identity on the material block, whole and
    column by column on columns where the adjoint is not zero"""
    _, ms, sd, _ = _scene(BOUNDS[corner], gaussian)
    rows = ms._albedo_host
    assert rows[0, scenes.MAT_COLUMN["metallic"]] == 1.0 and (rows[[0, 2], scenes.MAT_COLUMN["eta"]] == 1.0).all() == (corner == 0)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    dtex, tan = gpu.tangent(ms, sd, 21)
    what = f"bounds {corner} depth {depth} rr {rr} gaussian {gaussian}"
    gpu.identity(ms, sd, tex, 16, 5, gimg, *gpu.one_block(dtex, tan, "material"), depth, rr, what + " [material]")
    _, app = gpu.adjoint(ms, sd, 16, 5, gimg, tex, depth, rr)
    m = app.material.cpu().numpy()
    for col in BOUNDS_COLUMNS[corner]:
        j = scenes.MAT_COLUMN[col] - R0
        print(what, col, "adjoint column", m[:, j])
        assert np.abs(m[:, j]).max() > 0
        t = torch.zeros_like(tan.material)
        t[:, j] = tan.material[:, j]
        gpu.identity(ms, sd, tex, 16, 5, gimg, None, ops.AppearanceGrad(None, None, None, t), depth, rr, f"{what} [{col}]")


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth,rr", [(2, 5), (3, 1)])
def test_every_pixel_against_the_float64_tangent(depth, rr, gaussian):
    """tests/ref_prb.float64_tangent (differences converged to 1e-6, linear parts exact), roulette frozen at the unperturbed rows.  Per pixel
    1e-4 of max |dimg_ref|; at most 2e-4 of the pixels (one here) may hold a flipped sample — the forward's tolerance, which a derivative image of the
    same sums inherits (256 pixels: none may)"""
    W = H = 16
    sc = cs.small_corner(W, H, 8)
    ms, sd, world = gpu.load(sc, gaussian, 1)
    rows = ms._albedo_host.astype(np.float64)
    rng = np.random.default_rng(2)
    tex = gpu.rand_tex(sd, 1)
    drows = ref_prb.interior_material_tangent(rows, rng)
    drows[:, :3] = rng.uniform(0.5, 1.5, (rows.shape[0], 3))
    dtex = rng.uniform(-1, 1, (8, 8, 1)).astype(np.float32)
    dspot = np.array([0.5, 2.0, 1.25], np.float32)
    spp, seed = 8, 7
    ref = ref_prb.float64_tangent(world, sd, rows, tex.cpu().numpy(), spp, seed, depth, rr, 0.5 if gaussian else None, drows=drows, dtex=dtex, dspot=dspot)
    tan = ops.AppearanceGrad(torch.from_numpy(drows[:, :3].astype(np.float32)), torch.from_numpy(dspot), [],
                             torch.from_numpy(drows[:, R0:R0 + 11].astype(np.float32)))
    _, dimg = gpu.jvp(ms, sd, tex, spp, seed, torch.from_numpy(dtex), tan, depth, rr)
    err = np.abs(dimg.double().cpu().numpy() - ref).max(-1)
    scale = np.abs(ref).max()
    bad = int((err > 1e-4 * scale).sum())
    allowed = int(2e-4 * W * H)
    print(f"depth {depth} rr {rr} gaussian {gaussian}: max err {err.max():.3e}  1e-4 scale {1e-4 * scale:.3e}  pixels over {bad} (allowed {allowed})  "
          f"median err {np.median(err):.3e}")
    assert scale > 0 and bad <= allowed


def test_mi_render_forward_end_to_end():
    fb, wb, _ = cs.CASES["every_lobe"]
    sc = cs.corner(fb, wb, shared=True)  # (the floor and the wall x = 0 share mat-Floor)
    ms, sd, _ = gpu.load(sc, False, 1)
    tex = gpu.rand_tex(sd, 1)
    p = mi.traverse(ms)
    p["tex.data"] = tex[..., 0].clone()
    p.update()
    F, spot = "mat-Floor.brdf_0.", "emit-Spot.intensity.value"
    rows_f = ms._material_meshes["mat-Floor"]
    assert len(rows_f) == 2
    spec = float(fb["specular"])
    dt = gpu.rand((sd.proj.tex_h, sd.proj.tex_w), 9, -1.0, 1.0)
    tangents = {"tex.data": dt, F + "base_color.value": torch.tensor([0.3, -0.2, 0.5]), F + "roughness.value": torch.tensor(0.7), F + "specular": 0.4,
                F + "eta": 5.0, F + "clearcoat.value": -0.3, "mat-WallY.brdf_0.sheen.value": 1.0, spot: torch.tensor([1.0, 0.5, 2.0])}
    S = sd.n_shapes
    rows, mat = torch.zeros((S, 3)), torch.zeros((S, 11))
    rows[rows_f] = torch.tensor([0.3, -0.2, 0.5])
    mat[rows_f, scenes.MAT_COLUMN["roughness"] - R0] = 0.7
    mat[rows_f, scenes.MAT_COLUMN["clearcoat"] - R0] = -0.3
    chain = lambda s_: float(torch.tensor(0.4, device=DEV) * scenes.specular_to_eta_grad(s_))  # noqa: E731 (float32, as mi.render_forward forms it)
    mat[rows_f, scenes.MAT_COLUMN["eta"] - R0] = chain(spec)  # (`specular` drives eta: the `eta` tangent counts 0)
    mat[ms._material_meshes["mat-WallY"], scenes.MAT_COLUMN["sheen"] - R0] = 1.0
    want_tan = ops.AppearanceGrad(rows, torch.tensor([1.0, 0.5, 2.0]), [], mat)
    for it, depth, rr in ((None, 2, 5), (mi.load_dict({"type": "direct"}), 2, 5), (mi.load_dict({"type": "prb", "max_depth": 3, "rr_depth": 2}), 3, 2)):
        img, dimg = mi.render_forward(ms, p, tangents, spp=16, seed=3, integrator=it)
        sd_now = ms.scene_desc(tex_channels=1)
        want_img, want = gpu.jvp(ms, sd_now, tex, 16, 3, dt.unsqueeze(-1), want_tan, depth, rr)
        print("mi.render_forward", it, "max |dimg|", float(want.abs().max()), "max |difference|", float((dimg.torch() - want).abs().max()))
        assert float(want.abs().max()) > 0 and torch.equal(dimg.torch(), want) and torch.equal(img.torch(), want_img)
        assert torch.equal(img.torch(), mi.render(ms, spp=16, seed=3, integrator=it).torch())
        if it is not None:
            i2, d2 = it.render_forward(ms, p, tangents, seed=3, spp=16)
            assert torch.equal(i2.torch(), img.torch()) and torch.equal(d2.torch(), dimg.torch())
    # path with max_depth > 2: tex.data alone, and then it is prb's tangent
    path3, prb3 = mi.load_dict({"type": "path", "max_depth": 3}), mi.load_dict({"type": "prb", "max_depth": 3})
    a = mi.render_forward(ms, p, {"tex.data": dt}, spp=16, seed=3, integrator=path3)[1].torch()
    assert float(a.abs().max()) > 0 and torch.equal(a, mi.render_forward(ms, p, {"tex.data": dt}, spp=16, seed=3, integrator=prb3)[1].torch())
    with pytest.raises(ValueError, match="prb"):
        mi.render_forward(ms, p, tangents, spp=16, seed=3, integrator=path3)
    with pytest.raises(KeyError, match="tex.data"):
        mi.render_forward(ms, p, {"PerspectiveCamera.x_fov": 1.0})
    # once eta is assigned it drives the row: the `eta` tangent counts, `specular`'s does not
    p[F + "eta"] = 1.6
    p.update()
    sd_now = ms.scene_desc(tex_channels=1)
    only = {F + "specular": 0.4, F + "eta": 5.0}
    mat2 = torch.zeros((S, 11))
    mat2[rows_f, scenes.MAT_COLUMN["eta"] - R0] = 5.0
    got = mi.render_forward(ms, p, only, spp=16, seed=3)[1].torch()
    want = gpu.jvp(ms, sd_now, tex, 16, 3, None, ops.AppearanceGrad(None, None, [], mat2))[1]
    print("eta drives the row: max |dimg|", float(want.abs().max()))
    assert float(want.abs().max()) > 0 and torch.equal(got, want)
    # ... and back
    p[F + "specular"] = 0.0
    p.update()
    sd_now = ms.scene_desc(tex_channels=1)
    mat2[rows_f, scenes.MAT_COLUMN["eta"] - R0] = chain(0.0)  # (the finite limit at 0)
    got = mi.render_forward(ms, p, only, spp=16, seed=3)[1].torch()
    want = gpu.jvp(ms, sd_now, tex, 16, 3, None, ops.AppearanceGrad(None, None, [], mat2))[1]
    print("specular = 0 drives the row: max |dimg|", float(want.abs().max()))
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


def _full_size(gaussian):
    wl = workloads.vocalfold(device=DEV)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    ms = wl.mi_scene
    if gaussian:
        ms.rfilter = "gaussian"
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    sd = ms.scene_desc(tex_channels=1)
    assert (sd.cam.width, sd.cam.height) == (512, 512)
    gimg = gpu.rand((512, 512, 3), 1, -1.0, 1.0) / (512 * 512)
    dtex, tan = gpu.tangent(ms, sd, 31)
    for depth in (2, 3):
        ref = ms.geom.render_fwd(sd, ms.materials_arg(sd), tex, 64, 1, max_depth=depth, rr_depth=depth).clone()
        img, dimg = gpu.jvp(ms, sd, tex, 64, 1, dtex, tan, depth, depth)
        assert torch.equal(img, ref) and torch.isfinite(dimg).all() and float(dimg.abs().max()) > 0
        gpu.identity(ms, sd, tex, 64, 1, gimg, dtex, tan, depth, depth, f"vocal fold depth {depth} gaussian {gaussian}")


@pytest.mark.parametrize("gaussian", FILMS)
def test_full_size_vocalfold(gaussian):
    """512 x 512 x 64, direct light and depth 3 (roulette off): finite, the primal is render_fwd's, and the identity once per film and depth.  Runs
    in a child process under a time limit, so that a hang ends instead of holding the device.  The limit is sized to tools/pathbench.py's depth-3
    adjoint with the BSDF block (78.5 ms): the child's GPU work — two tangent renders, two adjoints, four forwards — is under half a second by
    that figure, and 60 s leave room for the interpreter's start, the imports, the device's initialisation and the scene's build on a busy machine"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_jvp_gpu", str(int(gaussian))], cwd=root, timeout=60, capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "vocal fold depth 3" in r.stdout


if __name__ == "__main__":
    _full_size(bool(int(sys.argv[1])))
