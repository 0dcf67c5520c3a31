"""The directional emitter on the GPU: k_lights_fwd<RF, DIR> against the float64 restatement (tests/ref_sun.py) on both films, film sizes and
row kinds, the closed forms on the quad that fills the film (with the roof that pins the shadow ray), the sun as the limit of a point light through the
kernel that exists, the bit identities, linearity, paths and the adjoint, a ragged second pass, and the public interface.  Independent evaluations are
held to the three conditions of tests/support.py's `independent`, the same computation by another kernel to rtol 1e-5."""
import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, scenes
from fireflies_amd import functional as Fn
from tests import gpu_support as gpu
from tests import light_scenes as ls
from tests import ref_path as rp
from tests import ref_sun as rs
from tests import sun_scenes as ss
from tests.gpu_support import DEV, table
from tests.support import copy_desc, independent

pytestmark = pytest.mark.gpu

SPP, SEED = 16, 7
LA = (0.2, 0.25, 0.3)


def case(film, principled, gaussian):
    return gpu.corner_case(ss.corner, film, principled, gaussian, SPP, SEED)


def sun_fwd(ms, sd, mats, tex, lights, spp=SPP, **kw):
    return ms.geom.render_fwd(sd, mats, tex, spp, SEED, lights=lights, lights_directional=True, **kw)


# ------------------------------------------------------------------ 1. against the float64 restatement
@pytest.mark.parametrize("film", sorted(ss.FILMS))
@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("principled", [False, True])
def test_direct_light_matches_the_float64_restatement(principled, gaussian, film):
    ms, sd, world, rows, tex, mats, unlit, main_ref = case(film, principled, gaussian)
    assert int(sd.mat_stride or 3) == (16 if principled else 3) and sd.shadows & 1
    for sun in (ss.SUN_A, ss.SUN_B):
        img = sun_fwd(ms, sd, mats, tex, table(sun))
        part = (img.double() - unlit.double()).cpu().numpy()
        ref = rs.render_sun(*world, sd, rows, ops.pack_lights([sun]).numpy(), SPP, SEED, gaussian_stddev=0.5 if gaussian else None)
        assert ref.mean() > 0.05 * (main_ref + ref).mean()
        independent(f"{film} principled={principled} gaussian={gaussian} {sun.name}", part, ref, float((main_ref + ref).max()), float(ref.sum()))


# ------------------------------------------------------------------ 2. closed forms on the device
@pytest.mark.parametrize("gaussian", [False, True])
def test_the_closed_form_and_the_roof(gaussian):
    """a Lambert quad that fills the film, no projector, no spot: every pixel is base E cos(theta) / pi.  Under a roof the camera does not see, every
    shadow ray — from the lifted point along wi over (0, 3e38) — hits: exactly 0; with bit 0 of `shadows` cleared the closed form is back.  A shadow ray
    cast the other way, or over an interval that ends short of 5.3, would leave the floor lit"""
    want = torch.tensor(ss.quad_closed_form(), dtype=torch.float64).expand(24, 24, 3)
    t = table(ss.SUN_Q)
    ms, sd, _ = gpu.load(ss.quad(), gaussian, 1)
    mats = ms.materials_arg(sd)
    assert sd.shadows & 1 and float(ms.geom.render_fwd(sd, mats, None, SPP, SEED).abs().max()) == 0.0
    img = sun_fwd(ms, sd, mats, None, t).double().cpu()
    print("quad: max relative error", float(((img - want) / want).abs().max()))
    torch.testing.assert_close(img, want, rtol=1e-5, atol=0.0)
    ms, sd, _ = gpu.load(ss.quad(roof=True), gaussian, 1)
    mats = ms.materials_arg(sd)
    dark = sun_fwd(ms, sd, mats, None, t)
    assert float(dark.abs().max()) == 0.0
    s2 = copy_desc(sd)
    s2.shadows &= ~1
    lit = sun_fwd(ms, s2, mats, None, t).double().cpu()
    print("quad under the roof, shadows off: max relative error", float(((lit - want) / want).abs().max()))
    torch.testing.assert_close(lit, want, rtol=1e-5, atol=0.0)
    # a frame whose +Z does not normalise lights nothing, and nothing is not a NaN
    for bad in (np.zeros((4, 4), np.float32), np.full((4, 4), np.nan, np.float32), np.full((4, 4), np.inf, np.float32)):
        out = sun_fwd(ms, s2, mats, None, table(scenes.LightData("bad", "directional", bad, (1.0, 1.0, 1.0))))
        assert float(out.abs().max()) == 0.0


# ------------------------------------------------------------------ 3. the sun as the limit of a point light, through the kernel that exists
@pytest.mark.parametrize("sun", [ss.SUN_A, ss.SUN_B], ids=["A", "B"])
@pytest.mark.parametrize("gaussian", [False, True])
def test_the_sun_is_the_limit_of_a_point_light(gaussian, sun):
    """shadows off, Lambert rows, D = 1e3 r, intensity E D^2: 4e-3 of the part's maximum — 3 r / D (the cosine moves by at most r / D, D^2 / d^2 by
    2 r / D) plus 1e-3 for float32 positions at that distance"""
    ms, sd, _, _, tex, mats, _, _ = case("21x19", False, gaussian)
    s2 = copy_desc(sd)
    s2.shadows &= ~1
    D = 1.0e3 * ss.RADIUS
    plain = ms.geom.render_fwd(s2, mats, tex, SPP, SEED).double()
    a = sun_fwd(ms, s2, mats, tex, table(sun)).double() - plain
    b = ms.geom.render_fwd(s2, mats, tex, SPP, SEED, lights=table(ss.far_point(sun, D))).double() - plain
    err = float((a - b).abs().max() / a.max())
    print(f"{sun.name} gaussian={gaussian}: max |sun - far point| / max {err:.3e} [4e-3], part's maximum {float(a.max()):.4g}")
    assert float(a.max()) > 0.05 and err <= 4e-3


# ------------------------------------------------------------------ 4. bit identities
@pytest.mark.parametrize("depth,gaussian,film", [(2, False, "21x19"), (2, True, "24x24"), (3, False, "24x24"), (3, True, "21x19"), (4, False, "21x19"), (4, True, "24x24")])
def test_bit_identities(depth, gaussian, film):
    ms, sd, _, _, tex, mats, _, _ = case(film, True, gaussian)
    t = table(ls.POINT, ss.SUN_A, ls.SPOT_B)
    plain = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth)
    a = sun_fwd(ms, sd, mats, tex, t, max_depth=depth)
    b = sun_fwd(ms, sd, mats, tex, t, max_depth=depth)
    assert torch.equal(a, b) and not torch.equal(a, plain)
    sun_only = sun_fwd(ms, sd, mats, tex, t[1:2], max_depth=depth)
    assert not torch.equal(sun_only, plain)
    dark = t[1:2].clone()
    dark[:, 16:19] = 0.0
    assert torch.equal(sun_fwd(ms, sd, mats, tex, dark, max_depth=depth), plain)  # (irradiance 0 adds +0.0)
    assert torch.equal(sun_fwd(ms, sd, mats, tex, t[:0], max_depth=depth), plain)  # (an empty table: the call as it was, the bit not set)
    img0, block0 = ms.geom.render_aov(sd, mats, tex, SPP, SEED, max_depth=depth)
    img1, block1 = ms.geom.render_aov(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t, lights_directional=True)
    assert torch.equal(img0, plain) and torch.equal(block1, block0) and torch.equal(img1, a)
    # a table without a sun: the same computation by the other kernel
    t2 = table(ls.POINT, ls.SPOT_B)
    with_bit = sun_fwd(ms, sd, mats, tex, t2, max_depth=depth)
    without = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t2)
    assert not torch.equal(without, plain)
    torch.testing.assert_close(with_bit, without, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ 5. linearity
@pytest.mark.parametrize("depth,gaussian", [(2, False), (3, True)])
def test_lamps_a_sun_and_a_world_are_the_sum_of_their_parts(depth, gaussian):
    ms, sd, _, _, tex, mats, _, _ = case("24x24", True, gaussian)
    kw = dict(max_depth=depth)
    plain = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, **kw)
    both = sun_fwd(ms, sd, mats, tex, table(ls.POINT, ls.SPOT_B, ss.SUN_A), ambient=LA, **kw)
    parts = [ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=table(ls.POINT), **kw), ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=table(ls.SPOT_B), **kw),
             sun_fwd(ms, sd, mats, tex, table(ss.SUN_A), **kw), ms.geom.render_fwd(sd, mats, tex, SPP, SEED, ambient=LA, **kw)]
    for p in parts:
        assert float((p - plain).max()) > 0
    total = sum(p.double() for p in parts) - 3.0 * plain.double()
    torch.testing.assert_close(both.double(), total, rtol=1e-5, atol=8e-7)


@pytest.mark.parametrize("gaussian", [False, True])
def test_eight_records_of_which_three_are_suns(gaussian):
    ms, sd, _, _, tex, mats, unlit, _ = case("24x24", True, gaussian)
    lights = ss.eight()
    assert len(lights) == _abi.RENDER_MAX_LIGHTS and sum(l.kind == "directional" for l in lights) == 3
    all8 = sun_fwd(ms, sd, mats, tex, table(*lights))
    total = -7.0 * unlit.double()
    for l in lights:
        one = sun_fwd(ms, sd, mats, tex, table(l))
        assert float((one - unlit).max()) > 0, l.name
        total += one.double()
    torch.testing.assert_close(all8.double(), total, rtol=1e-5, atol=8e-7)
    with pytest.raises(ValueError, match="at most 8"):
        sun_fwd(ms, sd, mats, tex, torch.zeros((9, 24), device=DEV))
    with pytest.raises(ValueError, match="fp32 film"):
        sun_fwd(ms, sd, mats, tex, table(ss.SUN_A), fp16=True)
    with pytest.raises(NotImplementedError, match="not differentiated"):
        ms.geom.render_bwd(sd, mats, SPP, SEED, gpu.rand_gimg(sd), appearance=True, tex=tex, lights=table(ss.SUN_A), lights_directional=True)


# ------------------------------------------------------------------ 6. paths and the adjoint
@pytest.mark.parametrize("depth,principled,gaussian", [(3, False, False), (4, True, True)])
def test_paths_match_the_float64_restatement_and_the_adjoint_ignores_the_sun(depth, principled, gaussian):
    ms, sd, world, rows, tex, mats, _, _ = case("24x24", principled, gaussian)
    t = table(ss.SUN_A)
    plain = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth)
    img = sun_fwd(ms, sd, mats, tex, t, max_depth=depth)
    part = (img.double() - plain.double()).cpu().numpy()
    stddev = 0.5 if gaussian else None
    ref = rs.render_sun(*world, sd, rows, t.cpu().numpy(), SPP, SEED, max_depth=depth, gaussian_stddev=stddev)
    ref2 = rs.render_sun(*world, sd, rows, t.cpu().numpy(), SPP, SEED, max_depth=2, gaussian_stddev=stddev)
    indirect = ref - ref2
    print("indirect / direct", indirect.mean() / ref2.mean())
    assert indirect.mean() > 0.05 * ref2.mean() > 0  # (the bounces carry the sun's light in this scene)
    main_ref = rp.render_fwd(*world, sd, rows, tex.cpu().numpy(), SPP, SEED, depth, gaussian_stddev=stddev)
    independent(f"depth {depth} principled={principled} gaussian={gaussian}", part, ref, float((main_ref + ref).max()), float(indirect.sum()))
    gimg = gpu.rand_gimg(sd, 3)
    g0 = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth)
    g1 = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth, lights=t, lights_directional=True)
    assert float(g0.abs().sum()) > 0
    torch.testing.assert_close(g1, g0, rtol=1e-5, atol=1e-8)
    # direct light: the adjoint of the packet kernels takes the bits too
    torch.testing.assert_close(ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, lights=t, lights_directional=True), ms.geom.render_bwd(sd, mats, SPP, SEED, gimg),
                               rtol=1e-5, atol=1e-8)
    # autograd of the texture through functional.render: the forward carries the sun, the gradient is that of the scene without it
    leaf = tex.clone().requires_grad_(True)
    out = Fn.render(leaf, ms.geom, sd, mats, SPP, SEED, max_depth=depth, lights=t, lights_directional=True)
    assert torch.equal(out.detach(), img)
    (out * gimg).sum().backward()
    torch.testing.assert_close(leaf.grad, g0, rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------ 7. a ragged second pass
def test_a_second_ragged_pass_of_samples():
    ms, sd, world, rows, tex, mats, _, _ = case("21x19", False, False)
    spp = 65
    plain = ms.geom.render_fwd(sd, mats, tex, spp, SEED)
    img = sun_fwd(ms, sd, mats, tex, table(ss.SUN_B), spp=spp)
    ref = rs.render_sun(*world, sd, rows, ops.pack_lights([ss.SUN_B]).numpy(), spp, SEED)
    main_ref = rp.render_fwd(*world, sd, rows, tex.cpu().numpy(), spp, SEED, 2)
    independent("65 samples per pixel", (img.double() - plain.double()).cpu().numpy(), ref, float((main_ref + ref).max()), float(ref.sum()))


# ------------------------------------------------------------------ 8. through the public interface
def _file_scene(tmp_path):
    scene = mi.load_file(ss.write_scene(tmp_path), device=DEV)
    params = mi.traverse(scene)
    params["tex.data"] = torch.zeros(32, 32, device=DEV)
    params["emit-Spot.intensity.value"] = mi.Color3f(torch.zeros(3))  # (projector and main spot dark: what is left is the extra emitters')
    params.update()
    return scene, params


def test_a_scene_file_with_a_sun_renders_and_follows_its_parameters(tmp_path):
    scene, params = _file_scene(tmp_path)
    assert [(l.name, l.kind) for l in scene.data.lights] == [("emit-Light", "point"), ("emit-Sun", "directional")] and scene.data.ambient is not None
    for k in ("emit-Light.position", "emit-Sun.irradiance.value", "emit-Sun.to_world", "emit-World.radiance.value"):
        assert k in params, k
    zero = torch.zeros(32, 32, 1, device=DEV)
    sd = scene.scene_desc(tex_channels=1)
    mats = scene.materials_arg(sd)
    t = scene.lights_table()
    assert t[1, 21] == 2.0 and scene.lights_directional()
    img = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    assert torch.equal(img, scene.geom.render_fwd(sd, mats, zero, SPP, SEED, lights=t, ambient=LA, lights_directional=True))
    deep = mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "prb", "max_depth": 3})).torch().clone()
    assert torch.equal(deep, scene.geom.render_fwd(sd, mats, zero, SPP, SEED, max_depth=3, lights=t, ambient=LA, lights_directional=True))
    assert float((deep - img).mean()) > 0.0
    # the sun's own image (everything else is dark or left out) ...
    sun_part = scene.geom.render_fwd(sd, mats, zero, SPP, SEED, lights=t[1:2], lights_directional=True)
    assert float(sun_part.mean()) > 0.05
    # ... is what three times the irradiance adds twice
    params["emit-Sun.irradiance.value"] = mi.Color3f(3.0 * torch.tensor(ss.FILE_SUN_IRRADIANCE))
    params.update()
    thrice = mi.render(scene, spp=SPP, seed=SEED).torch()
    torch.testing.assert_close(thrice - img, 2.0 * sun_part, rtol=1e-5, atol=1e-6)
    # a new pose turns the light
    params["emit-Sun.to_world"] = mi.Transform4f(ss.frame(ss.DIR_B))
    params.update()
    assert float((mi.render(scene, spp=SPP, seed=SEED).torch() - thrice).abs().max()) > 0.05
    # an aov integrator and the gaussian film
    block = mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": "direct"}})).torch()
    assert torch.equal(block[..., 1:], mi.render(scene, spp=SPP, seed=SEED).torch())
    scene.rfilter = "gaussian"
    soft = mi.render(scene, spp=SPP, seed=SEED).torch()
    sdg = scene.scene_desc(tex_channels=1)
    assert sdg.rfilter == _abi.RFILTER_GAUSSIAN and float(soft.mean()) > 0
    assert torch.equal(soft, scene.geom.render_fwd(sdg, scene.materials_arg(sdg), zero, SPP, SEED, lights=scene.lights_table(), ambient=LA, lights_directional=True))
    with pytest.raises(ValueError, match="fp16"):
        mi.render(scene, spp=SPP, seed=SEED, fp16=True)


def test_randomisation_reaches_the_render_key_by_key(tmp_path):
    import random

    import fireflies_amd as ff

    scene, params = _file_scene(tmp_path)
    ffs = ff.Scene(params, device=DEV)
    names = [l.name() for l in ffs.lights()]
    assert names[0] == "emit-Spot" and sorted(names[1:]) == ["emit-Light", "emit-Sun", "emit-World"], names  # (the main spot first)
    sun = ffs.light("emit-Sun")
    sun.add_vec3_key("irradiance.value", torch.tensor([3.0, 3.0, 3.0], device=DEV), torch.tensor([5.0, 4.5, 4.0], device=DEV))
    ffs.train()
    base = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    for k in range(3):
        torch.manual_seed(k)
        random.seed(k)
        ffs.randomize()
    img = mi.render(scene, spp=SPP, seed=SEED).torch()
    sd = scene.scene_desc(tex_channels=1)
    only = scene.geom.render_fwd(sd, scene.materials_arg(sd), torch.zeros(32, 32, 1, device=DEV), SPP, SEED,
                                 lights=table(scenes.LightData("emit-Sun", "directional", scene.data.lights[1].to_world, ss.FILE_SUN_IRRADIANCE)), lights_directional=True)
    drawn = params["emit-Sun.irradiance.value"].torch().reshape(3).to(DEV)
    file_e = torch.tensor(ss.FILE_SUN_IRRADIANCE, device=DEV)
    assert float((drawn - file_e).min()) >= 1.0  # (the draw came from [3, 4 .. 5])
    # the image is linear in the irradiance: the difference to the file's is the sun's own image, scaled per channel
    torch.testing.assert_close(img - base, only * ((drawn - file_e) / file_e), rtol=1e-5, atol=1e-6)
    print(scene.update_paths, scene.update_fallbacks)
    assert scene.update_paths["native"] == 0 and scene.update_fallbacks.get("extra emitters", 0) >= 1, (scene.update_paths, scene.update_fallbacks)


def test_gradients_and_refusals_through_mi_render(tmp_path):
    scene, params = _file_scene(tmp_path)
    sd = scene.scene_desc(tex_channels=1)
    tex = gpu.rand_tex(sd, 5)[..., 0].contiguous()
    gimg = gpu.rand_gimg(sd, 6)
    leaf = tex.clone().requires_grad_(True)
    params["tex.data"] = leaf
    params.update()
    img = mi.render(scene, spp=SPP, seed=SEED).torch()
    (img * gimg).sum().backward()
    want = scene.geom.render_bwd(sd, scene.materials_arg(sd), SPP, SEED, gimg)  # (the scene without the extra emitters: the texture does not see them)
    assert float(want.abs().sum()) > 0
    torch.testing.assert_close(leaf.grad, want[..., 0], rtol=1e-5, atol=1e-8)
    params["tex.data"] = tex
    params["mat-Floor.brdf_0.base_color.value"] = mi.Color3f(torch.tensor([0.5, 0.5, 0.5], requires_grad=True))
    params.update()
    with pytest.raises(NotImplementedError, match="extra emitters.*not differentiated"):
        mi.render(scene, spp=SPP, seed=SEED)
    with pytest.raises(NotImplementedError, match="extra emitters.*not differentiated"):
        mi.render_forward(scene, params, {"tex.data": torch.ones_like(tex)}, spp=SPP, seed=SEED)


def test_the_pattern_optimizer_on_a_scene_with_a_sun():
    from fireflies_amd import workloads
    from fireflies_amd.optim import PatternOptimizer

    wl = workloads.vocalfold(device=DEV, width=64, height=56, tex=96, grid=6, frames=5, n_fold=20, tube=(20, 24),
                             lights=[scenes.LightData("emit-Sun", "directional", ss.frame((0.1, -0.1, -1.0)), (0.5, 0.5, 0.5))])
    opt = PatternOptimizer(wl.mi_scene, wl.ff_scene, wl.laser, sigma=wl.sigma, tex_size=wl.tex_size, spp=8)
    with pytest.raises(NotImplementedError, match="extra emitters.*step_autograd"):
        opt.step()
    for _ in range(2):
        out = opt.step_autograd()
    assert torch.isfinite(wl.laser._rays).all()
    assert np.isfinite(float(out["loss"]))
