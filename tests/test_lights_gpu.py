"""Extra emitters on the GPU: k_lights_fwd against the float64 restatement (tests/ref_lights.py) on both films and row kinds, against the
packet kernels for the same spot, a point light against a spot that holds the whole scene, the bit identities, paths, the arms a small case misses.
Independent evaluations are held to the three conditions of tests/support.py's `independent`, the same computation by another route to
rtol 1e-5, atol 1e-7."""
import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, scenes
from fireflies_amd import functional as Fn
from tests import gpu_support as gpu
from tests import light_scenes as ls
from tests import ref_lights as rl
from tests import ref_path as rp
from tests.gpu_support import DEV, table
from tests.support import copy_desc, independent

pytestmark = pytest.mark.gpu

SPP, SEED = 16, 7


def case(film, principled, gaussian):
    return gpu.corner_case(ls.corner, film, principled, gaussian, SPP, SEED)


# ------------------------------------------------------------------ 1. against the float64 restatement
@pytest.mark.parametrize("film", sorted(ls.FILMS))
@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("principled", [False, True])
def test_direct_light_matches_the_float64_restatement(principled, gaussian, film):
    ms, sd, world, rows, tex, mats, unlit, main_ref = case(film, principled, gaussian)
    assert int(sd.mat_stride or 3) == (16 if principled else 3) and sd.shadows & 1
    for light in (ls.POINT, ls.SPOT_B):
        img = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=table(light))
        part = (img.double() - unlit.double()).cpu().numpy()
        ref = rl.render_lights(*world, sd, rows, ops.pack_lights([light]).numpy(), SPP, SEED, gaussian_stddev=0.5 if gaussian else None)
        assert ref.mean() > 0.05 * (main_ref + ref).mean()
        independent(f"{film} principled={principled} gaussian={gaussian} {light.name}", part, ref, float((main_ref + ref).max()), float(ref.sum()))


# ------------------------------------------------------------------ 2. the new pass against the packet kernels for the same spot
@pytest.mark.parametrize("gaussian", [False, True])
def test_superposition_through_the_kernels_that_exist(gaussian):
    ms, sd, world, rows, tex, mats, unlit, _ = case("24x24", False, gaussian)
    left = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=table(ls.SPOT_B))
    alone = ls.corner("24x24")
    alone.projector = None
    alone.spot = scenes.SpotData("emit-Spot", ls.SPOT_B.to_world, ls.SPOT_B.intensity, ls.SPOT_B.cutoff_angle, ls.SPOT_B.beam_width)
    ms2, sd2, _ = gpu.load(alone, gaussian, 1)
    b_img = ms2.geom.render_fwd(sd2, ms2.materials_arg(sd2), None, SPP, SEED)
    right = (unlit.double() + b_img.double()).cpu().numpy()
    assert float(b_img.mean()) > 0.05 * float(unlit.mean()) > 0
    independent(f"spot B by the lights' pass and as the main spot, gaussian={gaussian}", left.double().cpu().numpy(), right, float(right.max()), float(b_img.double().sum()))


# ------------------------------------------------------------------ 3. a point light and a spot whose beam holds the whole scene
@pytest.mark.parametrize("depth,gaussian", [(2, False), (3, True)])
def test_a_point_light_equals_a_wide_spot(depth, gaussian):
    ms, sd, _, _, tex, mats, unlit, _ = case("21x19", True, gaussian)
    a = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=table(ls.WIDE_POINT))
    b = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=table(ls.WIDE_SPOT))
    assert float((a - unlit).mean()) > 0.05 * float(unlit.mean())
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ 4. bit identities
@pytest.mark.parametrize("depth,gaussian", [(2, False), (2, True), (3, False), (4, True)])
def test_bit_identities(depth, gaussian):
    ms, sd, _, _, tex, mats, _, _ = case("21x19", True, gaussian)
    t = table(ls.POINT, ls.SPOT_B)
    plain = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth)
    a = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    b = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    assert torch.equal(a, b) and not torch.equal(a, plain)
    dark = t.clone()
    dark[:, 16:19] = 0.0
    assert torch.equal(ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=dark), plain)
    assert torch.equal(ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t[:0]), plain)
    img0, block0 = ms.geom.render_aov(sd, mats, tex, SPP, SEED, max_depth=depth)
    img1, block1 = ms.geom.render_aov(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    assert torch.equal(img0, plain) and torch.equal(block1, block0) and torch.equal(img1, a)
    # the rows on the device, in front of the lights, instead of inside the scene description: the lights' part by another route (two float32
    # images of size ~1 are subtracted on either side: 1e-6)
    assert sd.n_mat_h > 0
    s2 = copy_desc(sd)
    s2.n_mat_h = 0
    lit2, plain2 = (ms.geom.render_fwd(s2, ms.albedo, tex, SPP, SEED, max_depth=depth, lights=x) for x in (t, None))
    torch.testing.assert_close(lit2 - plain2, a - plain, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 5. paths
@pytest.mark.parametrize("depth,principled,gaussian", [(3, False, False), (4, True, True)])
def test_paths_match_the_float64_restatement_and_the_adjoint_ignores_the_lights(depth, principled, gaussian):
    ms, sd, world, rows, tex, mats, _, main_ref2 = case("24x24", principled, gaussian)
    t = table(ls.POINT)
    plain = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth)
    img = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    part = (img.double() - plain.double()).cpu().numpy()
    stddev = 0.5 if gaussian else None
    ref = rl.render_lights(*world, sd, rows, t.cpu().numpy(), SPP, SEED, max_depth=depth, gaussian_stddev=stddev)
    ref2 = rl.render_lights(*world, sd, rows, t.cpu().numpy(), SPP, SEED, max_depth=2, gaussian_stddev=stddev)
    indirect = ref - ref2
    assert indirect.mean() > 0.05 * ref2.mean() > 0  # (the bounces carry the light's radiance in this scene)
    main_ref = rp.render_fwd(*world, sd, rows, tex.cpu().numpy(), SPP, SEED, depth, gaussian_stddev=stddev)
    independent(f"depth {depth} principled={principled} gaussian={gaussian}", part, ref, float((main_ref + ref).max()), float(indirect.sum()))
    gimg = gpu.rand_gimg(sd, 3)
    g0 = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth)
    g1 = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth, lights=t)
    assert float(g0.abs().sum()) > 0
    torch.testing.assert_close(g1, g0, rtol=1e-5, atol=1e-8)
    # direct light: the adjoint of the packet kernels takes the bits too
    torch.testing.assert_close(ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, lights=t), ms.geom.render_bwd(sd, mats, SPP, SEED, gimg), rtol=1e-5, atol=1e-8)
    # autograd of the texture through functional.render: the forward carries the lights, the gradient is that of the scene without them
    leaf = tex.clone().requires_grad_(True)
    out = Fn.render(leaf, ms.geom, sd, mats, SPP, SEED, max_depth=depth, lights=t)
    assert torch.equal(out.detach(), img)
    (out * gimg).sum().backward()
    torch.testing.assert_close(leaf.grad, g0, rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------ 6. the arms a small case misses
def test_a_second_ragged_pass_of_samples():
    ms, sd, world, rows, tex, mats, _, _ = case("21x19", False, False)
    spp = 65
    plain = ms.geom.render_fwd(sd, mats, tex, spp, SEED)
    img = ms.geom.render_fwd(sd, mats, tex, spp, SEED, lights=table(ls.POINT))
    ref = rl.render_lights(*world, sd, rows, ops.pack_lights([ls.POINT]).numpy(), spp, SEED)
    main_ref = rp.render_fwd(*world, sd, rows, tex.cpu().numpy(), spp, SEED, 2)
    independent("65 samples per pixel", (img.double() - plain.double()).cpu().numpy(), ref, float((main_ref + ref).max()), float(ref.sum()))


@pytest.mark.parametrize("gaussian", [False, True])
def test_eight_lights_are_the_sum_of_eight_renders(gaussian):
    ms, sd, _, _, tex, mats, unlit, _ = case("24x24", True, gaussian)
    lights = ls.eight()
    assert len(lights) == _abi.RENDER_MAX_LIGHTS
    all8 = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=table(*lights))
    total = -7.0 * unlit.double()
    for l in lights:
        one = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=table(l))
        assert float((one - unlit).max()) > 0, l.name
        total += one.double()
    torch.testing.assert_close(all8.double(), total, rtol=1e-5, atol=8e-7)
    with pytest.raises(ValueError, match="at most 8"):
        ms.geom.render_fwd(sd, mats, tex, SPP, SEED, lights=torch.zeros((9, 24), device=DEV))
    with pytest.raises(ValueError, match="fp32 film"):
        ms.geom.render_fwd(sd, mats, tex, SPP, SEED, fp16=True, lights=table(ls.POINT))
    with pytest.raises(NotImplementedError, match="not differentiated"):
        ms.geom.render_bwd(sd, mats, SPP, SEED, gpu.rand_gimg(sd), appearance=True, tex=tex, lights=table(ls.POINT))


# ------------------------------------------------------------------ 7. through the public interface
def _file_scene(tmp_path):
    scene = mi.load_file(ls.write_scene(tmp_path), device=DEV)
    params = mi.traverse(scene)
    params["tex.data"] = torch.zeros(32, 32, device=DEV)
    params["emit-Spot.intensity.value"] = mi.Color3f(torch.zeros(3))  # (projector and main spot dark: what is left is the extra emitters')
    params.update()
    return scene, params


def test_a_scene_file_with_a_point_light_renders_and_follows_its_parameters(tmp_path):
    scene, params = _file_scene(tmp_path)
    assert [l.name for l in scene.data.lights] == ["emit-Light", "emit-PointLight", "emit-SecondSpot"]
    for k in ("emit-Light.position", "emit-Light.intensity.value", "emit-SecondSpot.to_world", "emit-SecondSpot.intensity.value", "emit-SecondSpot.cutoff_angle", "emit-SecondSpot.beam_width"):
        assert k in params, k
    for k in ("emit-PointLight.intensity.value", "emit-SecondSpot.intensity.value"):
        params[k] = mi.Color3f(torch.zeros(3))
    params.update()
    paths0 = dict(scene.render_paths)
    img = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    assert scene.render_paths["caller_stream"] == paths0["caller_stream"] + 1 and scene.render_paths["two_stream"] == paths0["two_stream"]
    assert float(img.max()) > 0.05 and float(img.min()) >= 0.0  # (only the point light reaches anything)
    sd = scene.scene_desc(tex_channels=1)
    assert torch.equal(img, scene.geom.render_fwd(sd, scene.materials_arg(sd), torch.zeros(32, 32, 1, device=DEV), SPP, SEED, lights=table(ls.POINT)))
    # twice the intensity: twice the lights' part (the rest of the image is dark here)
    params["emit-Light.intensity.value"] = mi.Color3f(2.0 * torch.tensor(ls.POINT.intensity))
    params.update()
    twice = mi.render(scene, spp=SPP, seed=SEED).torch()
    torch.testing.assert_close(twice, 2.0 * img, rtol=1e-5, atol=0.0)
    # a new position moves the light
    params["emit-Light.position"] = mi.Color3f(torch.tensor([1.5, 1.5, 2.5]))
    params.update()
    moved = mi.render(scene, spp=SPP, seed=SEED).torch()
    assert float((moved - twice).abs().max()) > 0.05
    # paths, the gaussian film and an aov integrator
    deep = mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "path", "max_depth": 3})).torch()
    assert float((deep - moved).min()) >= 0.0 and float((deep - moved).mean()) > 0.0
    block = mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": "direct"}})).torch()
    assert torch.equal(block[..., 1:], moved)
    scene.rfilter = "gaussian"
    soft = mi.render(scene, spp=SPP, seed=SEED).torch()
    sdg = scene.scene_desc(tex_channels=1)
    assert sdg.rfilter == _abi.RFILTER_GAUSSIAN and float(soft.mean()) > 0
    assert torch.equal(soft, scene.geom.render_fwd(sdg, scene.materials_arg(sdg), torch.zeros(32, 32, 1, device=DEV), SPP, SEED, lights=scene.lights_table()))
    with pytest.raises(ValueError, match="fp16"):
        mi.render(scene, spp=SPP, seed=SEED, fp16=True)


def test_randomisation_reaches_the_render_key_by_key(tmp_path):
    import random

    import fireflies_amd as ff

    scene, params = _file_scene(tmp_path)
    ffs = ff.Scene(params, device=DEV)
    names = [l.name() for l in ffs.lights()]
    assert names == ["emit-Spot", "emit-Light", "emit-PointLight", "emit-SecondSpot"], names  # (the main spot first)
    assert ffs.light("emit-Light") is not None and ffs.light_at(0).name() == "emit-Spot"
    light = ffs.light("emit-Light")
    light.add_vec3_key("intensity.value", torch.tensor([30.0, 30.0, 30.0], device=DEV), torch.tensor([50.0, 45.0, 40.0], device=DEV))
    ffs.train()
    base = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    for k in range(3):
        torch.manual_seed(k)
        random.seed(k)
        ffs.randomize()
    img = mi.render(scene, spp=SPP, seed=SEED).torch()
    only = scene.geom.render_fwd(scene.scene_desc(tex_channels=1), scene.materials_arg(scene.scene_desc(tex_channels=1)), torch.zeros(32, 32, 1, device=DEV), SPP, SEED,
                                 lights=table(ls.POINT))
    drawn = params["emit-Light.intensity.value"].torch().reshape(3).to(DEV)
    file_i = torch.tensor(ls.POINT.intensity, device=DEV)
    assert float((drawn - file_i).min()) >= 10.0  # (the draw came from [30, 40 .. 50])
    # the image is linear in the intensity: the difference to the file's is the point light's own image, scaled per channel
    torch.testing.assert_close(img - base, only * ((drawn - file_i) / file_i), rtol=1e-5, atol=1e-6)
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
    want = scene.geom.render_bwd(sd, scene.materials_arg(sd), SPP, SEED, gimg)  # (the scene without the extra lights: the texture does not see them)
    assert float(want.abs().sum()) > 0
    torch.testing.assert_close(leaf.grad, want[..., 0], rtol=1e-5, atol=1e-8)
    params["tex.data"] = tex
    params["mat-Floor.brdf_0.base_color.value"] = mi.Color3f(torch.tensor([0.5, 0.5, 0.5], requires_grad=True))
    params.update()
    with pytest.raises(NotImplementedError, match="not differentiated"):
        mi.render(scene, spp=SPP, seed=SEED)
    with pytest.raises(NotImplementedError, match="not differentiated"):
        mi.render_forward(scene, params, {"tex.data": torch.ones_like(tex)}, spp=SPP, seed=SEED)


def test_the_pattern_optimizer_on_a_scene_with_an_extra_light():
    from fireflies_amd import workloads
    from fireflies_amd.optim import PatternOptimizer

    tw = np.eye(4, dtype=np.float32)
    tw[:3, 3] = (0.1, -0.1, 1.6)
    wl = workloads.vocalfold(device=DEV, width=64, height=56, tex=96, grid=6, frames=5, n_fold=20, tube=(20, 24),
                             lights=[scenes.LightData("emit-Light", "point", tw, (3.0, 3.0, 3.0))])
    opt = PatternOptimizer(wl.mi_scene, wl.ff_scene, wl.laser, sigma=wl.sigma, tex_size=wl.tex_size, spp=8)
    with pytest.raises(NotImplementedError, match="step_autograd"):
        opt.step()
    for _ in range(2):
        out = opt.step_autograd()
    assert torch.isfinite(wl.laser._rays).all()
    assert np.isfinite(float(out["loss"]))
