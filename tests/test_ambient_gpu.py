"""The constant emitter on the GPU: k_lights_fwd<RF, DIR, AMB> in closed form, against the float64 restatement (tests/ref_ambient.py) on both
films, film sizes and row kinds at max_depth 2, 3 and 4, the identities, the arms a small case misses, the adjoint, and the public interface.
Independent evaluations are held to the three conditions of tests/support.py's `independent`, the same computation by another route to rtol 1e-5, atol 1e-7."""
import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops
from fireflies_amd import functional as Fn
from tests import ambient_scenes as am
from tests import gpu_support as gpu
from tests import light_scenes as ls
from tests import ref_ambient as ra
from tests import ref_path as rp
from tests.gpu_support import DEV
from tests.support import independent

pytestmark = pytest.mark.gpu

SPP, SEED = 16, 7
LA = am.RADIANCE
_RENDERED = {}


def case(film, principled, gaussian, dark=False):
    """gpu.corner_case without its direct-light images; in their place {(depth, rr, spp): the image without the bit} and {(depth, rr, spp): the float64
    restatement of that image}, filled by plain_of and main_ref_of"""
    c = gpu.corner_case(am.dark_corner if dark else am.corner, film, principled, gaussian, SPP, SEED, direct=False)
    return (*c[:6], *_RENDERED.setdefault((film, principled, gaussian, dark), ({}, {})))


def plain_of(c, depth, rr=5, spp=SPP):
    ms, sd, _, _, tex, mats, plain, _ = c
    if (depth, rr, spp) not in plain:
        plain[(depth, rr, spp)] = ms.geom.render_fwd(sd, mats, tex, spp, SEED, max_depth=depth, rr_depth=rr)
    return plain[(depth, rr, spp)]


def main_ref_of(c, depth, gaussian, rr=5, spp=SPP):
    _, sd, world, rows, tex, _, _, refs = c
    if (depth, rr, spp) not in refs:
        refs[(depth, rr, spp)] = rp.render_fwd(*world, sd, rows, tex.cpu().numpy(), spp, SEED, depth, rr, gaussian_stddev=0.5 if gaussian else None)
    return refs[(depth, rr, spp)]


# ------------------------------------------------------------------ 1. exact closed forms, no noise
@pytest.mark.parametrize("gaussian", [False, True])
def test_the_closed_forms(gaussian):
    """one Lambert quad that fills the film, no projector, no spot, max_depth 2: every closing ray escapes and f is the base colour — every pixel is
    base x L_a; the same camera turned to see no geometry: every pixel is L_a"""
    ms, sd, _ = gpu.load(am.quad(), gaussian, 1)
    mats = ms.materials_arg(sd)
    assert float(ms.geom.render_fwd(sd, mats, None, SPP, SEED).abs().max()) == 0.0
    img = ms.geom.render_fwd(sd, mats, None, SPP, SEED, ambient=LA)
    want = torch.tensor(am.QUAD_RGB, dtype=torch.float32).double() * torch.tensor(LA, dtype=torch.float32).double()
    print("quad: max relative error", float(((img.double().cpu() - want) / want).abs().max()))
    torch.testing.assert_close(img.double().cpu(), want.expand(24, 24, 3), rtol=1e-6, atol=0.0)
    ms, sd, _ = gpu.load(am.quad(away=True), gaussian, 1)
    img = ms.geom.render_fwd(sd, ms.materials_arg(sd), None, SPP, SEED, ambient=LA)
    torch.testing.assert_close(img.double().cpu(), torch.tensor(LA, dtype=torch.float32).double().expand(24, 24, 3), rtol=1e-6, atol=0.0)


# ------------------------------------------------------------------ 2. against the float64 restatement
@pytest.mark.parametrize("film", sorted(am.FILMS))
@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("principled", [False, True])
def test_the_ambient_part_matches_the_float64_restatement(principled, gaussian, film):
    c = case(film, principled, gaussian)
    ms, sd, world, rows, tex, mats, _, _ = c
    assert int(sd.mat_stride or 3) == (16 if principled else 3)
    for depth in (2, 3, 4):
        img = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=LA)
        part = (img.double() - plain_of(c, depth).double()).cpu().numpy()
        ref = ra.render_ambient(*world, sd, rows, LA, SPP, SEED, max_depth=depth, gaussian_stddev=0.5 if gaussian else None)
        main_ref = main_ref_of(c, depth, gaussian)
        assert ref.mean() > 0.05 * (main_ref + ref).mean()
        independent(f"{film} principled={principled} gaussian={gaussian} depth {depth}", part, ref, float((main_ref + ref).max()), float(ref.sum()))


# ------------------------------------------------------------------ 3. the same computation by another route
@pytest.mark.parametrize("depth,gaussian,principled", [(2, False, False), (2, True, True), (3, False, True), (4, True, False)])
def test_linearity_and_superposition(depth, gaussian, principled):
    """on the corner without projector and spot the image of the plain call is zero, so the ambient part is an image and not a difference"""
    ms, sd, _, _, tex, mats, _, _ = c = case("21x19", principled, gaussian, dark=True)
    plain = plain_of(c, depth)
    assert float(plain.abs().max()) == 0.0
    one = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=LA)
    two = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=tuple(2.0 * v for v in LA))
    assert float(one.mean()) > 0.1
    torch.testing.assert_close(two - plain, 2.0 * (one - plain), rtol=1e-5, atol=1e-7)
    t = ops.pack_lights([am.WEAK_POINT]).to(DEV)
    lit = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    both = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t, ambient=LA)
    assert 0.0 < float(lit.max()) < 0.1
    torch.testing.assert_close(both - lit, one - plain, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("depth,gaussian", [(2, False), (2, True), (3, False), (4, True)])
def test_bit_identities(depth, gaussian):
    ms, sd, _, _, tex, mats, _, _ = c = case("21x19", True, gaussian)
    plain = plain_of(c, depth)
    a = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=LA)
    b = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=torch.tensor(LA, device=DEV))
    assert torch.equal(a, b) and not torch.equal(a, plain)
    assert torch.equal(ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=(0.0, 0.0, 0.0)), plain)
    t = ops.pack_lights([ls.POINT, ls.SPOT_B]).to(DEV)
    lit = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    assert torch.equal(ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t, ambient=(0.0, 0.0, 0.0)), lit)
    img0, block0 = ms.geom.render_aov(sd, mats, tex, SPP, SEED, max_depth=depth)
    img1, block1 = ms.geom.render_aov(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=LA)
    assert torch.equal(img0, plain) and torch.equal(block1, block0) and torch.equal(img1, a)
    assert block0.shape[-1] == _abi.RENDER_AOV_FLOATS == 17


# ------------------------------------------------------------------ 4. the arms a small case misses
def test_a_second_ragged_pass_of_samples():
    ms, sd, world, rows, tex, mats, _, _ = c = case("21x19", False, False)
    spp = 70
    img = ms.geom.render_fwd(sd, mats, tex, spp, SEED, ambient=LA)
    ref = ra.render_ambient(*world, sd, rows, LA, spp, SEED)
    main_ref = main_ref_of(c, 2, False, spp=spp)
    independent("70 samples per pixel", (img.double() - plain_of(c, 2, spp=spp).double()).cpu().numpy(), ref, float((main_ref + ref).max()), float(ref.sum()))


@pytest.mark.parametrize("principled,gaussian", [(False, False), (True, True)])
def test_the_roulette_on_the_closing_ray(principled, gaussian):
    ms, sd, world, rows, tex, mats, _, _ = c = case("24x24", principled, gaussian)
    img = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=4, rr_depth=1, ambient=LA)
    parts = {}
    ref = ra.render_ambient(*world, sd, rows, LA, SPP, SEED, max_depth=4, rr_depth=1, gaussian_stddev=0.5 if gaussian else None, parts=parts)
    no_rr = ra.render_ambient(*world, sd, rows, LA, SPP, SEED, max_depth=4, rr_depth=99, gaussian_stddev=0.5 if gaussian else None)
    assert parts["closing"] > 0 and np.abs(ref - no_rr).max() > 0.05 * ref.max()  # (the roulette acts, on the closing ray too)
    main_ref = main_ref_of(c, 4, gaussian, rr=1)
    independent(f"rr_depth 1 at max_depth 4, principled={principled} gaussian={gaussian}", (img.double() - plain_of(c, 4, rr=1).double()).cpu().numpy(), ref,
                float((main_ref + ref).max()), float(ref.sum()))


@pytest.mark.parametrize("depth,gaussian", [(2, False), (3, True)])
def test_ambient_with_eight_lights_is_the_sum_of_the_parts(depth, gaussian):
    ms, sd, _, _, tex, mats, _, _ = c = case("24x24", True, gaussian)
    t = ops.pack_lights(ls.eight()).to(DEV)
    assert t.shape[0] == _abi.RENDER_MAX_LIGHTS
    plain = plain_of(c, depth)
    lit = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t)
    amb = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=LA)
    both = ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, lights=t, ambient=LA)
    assert float((lit - plain).mean()) > 0.05 and float((amb - plain).mean()) > 0.05
    torch.testing.assert_close(both.double(), lit.double() + amb.double() - plain.double(), rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ 5. the adjoint and the refusals
@pytest.mark.parametrize("depth,gaussian", [(2, False), (3, True)])
def test_the_adjoint_ignores_the_ambient_light(depth, gaussian):
    ms, sd, _, _, tex, mats, _, _ = case("24x24", False, gaussian)
    gimg = gpu.rand_gimg(sd, 3)
    g0 = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth)
    g1 = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth, ambient=LA)
    assert float(g0.abs().sum()) > 0
    torch.testing.assert_close(g1, g0, rtol=1e-5, atol=1e-8)
    leaf = tex.clone().requires_grad_(True)
    out = Fn.render(leaf, ms.geom, sd, mats, SPP, SEED, max_depth=depth, ambient=LA)
    assert torch.equal(out.detach(), ms.geom.render_fwd(sd, mats, tex, SPP, SEED, max_depth=depth, ambient=LA))
    (out * gimg).sum().backward()
    torch.testing.assert_close(leaf.grad, g0, rtol=1e-5, atol=1e-8)


def test_the_calls_refuse_what_is_not_served():
    ms, sd, _, _, tex, mats, _, _ = case("24x24", False, False)
    with pytest.raises(ValueError, match="constant emitter.*fp32 film"):
        ms.geom.render_fwd(sd, mats, tex, SPP, SEED, fp16=True, ambient=LA)
    with pytest.raises(ValueError, match="constant emitter.*adjoint cache"):
        ms.geom.render_fwd(sd, mats, tex, SPP, SEED, cache=torch.empty(ops.render_cache_bytes_sd(sd, SPP), dtype=torch.uint8, device=DEV), ambient=LA)
    with pytest.raises(NotImplementedError, match="constant emitter.*not differentiated"):
        ms.geom.render_bwd(sd, mats, SPP, SEED, gpu.rand_gimg(sd), appearance=True, tex=tex, ambient=LA)
    with pytest.raises(ValueError, match="constant emitter.*no fp16 film"):
        Fn.render(tex, ms.geom, sd, mats, SPP, SEED, fp16=True, ambient=LA)


# ------------------------------------------------------------------ 6. through the public interface
def _file_scene(tmp_path, xml=am.XML, name="ambient.xml", dark=True):
    scene = mi.load_file(am.write_scene(tmp_path, xml, name), device=DEV)
    params = mi.traverse(scene)
    params["tex.data"] = torch.zeros(32, 32, device=DEV)
    if dark:  # (projector and main spot dark: what is left is the constant emitter's)
        params["emit-Spot.intensity.value"] = mi.Color3f(torch.zeros(3))
    params.update()
    return scene, params


def test_a_scene_file_with_a_constant_emitter_renders_and_follows_its_parameter(tmp_path):
    scene, params = _file_scene(tmp_path)
    assert scene.data.ambient.name == "emit-World" and "emit-World.radiance.value" in params
    assert [float(v) for v in params["emit-World.radiance.value"].torch().reshape(-1)] == [float(np.float32(v)) for v in LA]
    paths0 = dict(scene.render_paths)
    img = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    assert scene.render_paths["caller_stream"] == paths0["caller_stream"] + 1 and scene.render_paths["two_stream"] == paths0["two_stream"]
    assert float(img.mean()) > 0.1 and float(img.min()) >= 0.0
    sd = scene.scene_desc(tex_channels=1)
    zero = torch.zeros(32, 32, 1, device=DEV)
    assert torch.equal(img, scene.geom.render_fwd(sd, scene.materials_arg(sd), zero, SPP, SEED, ambient=LA))
    # twice the radiance: twice the image (the rest of it is dark here); the device record is rebuilt on update()
    params["emit-World.radiance.value"] = mi.Color3f(2.0 * torch.tensor(LA))
    params.update()
    twice = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    torch.testing.assert_close(twice, 2.0 * img, rtol=1e-5, atol=0.0)
    # path and prb, an aov integrator, the gaussian film
    deep = mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "path", "max_depth": 3})).torch().clone()
    assert float((deep - twice).min()) >= 0.0 and float((deep - twice).mean()) > 0.0
    assert torch.equal(deep, scene.geom.render_fwd(sd, scene.materials_arg(sd), zero, SPP, SEED, max_depth=3, ambient=scene.ambient_record()))
    assert torch.equal(mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "prb", "max_depth": 3})).torch(), deep)
    block = mi.render(scene, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": "direct"}})).torch()
    assert torch.equal(block[..., 1:], twice)
    scene.rfilter = "gaussian"
    soft = mi.render(scene, spp=SPP, seed=SEED).torch()
    sdg = scene.scene_desc(tex_channels=1)
    assert sdg.rfilter == _abi.RFILTER_GAUSSIAN and float(soft.mean()) > 0
    assert torch.equal(soft, scene.geom.render_fwd(sdg, scene.materials_arg(sdg), zero, SPP, SEED, ambient=scene.ambient_record()))
    with pytest.raises(ValueError, match="constant emitter.*fp16"):
        mi.render(scene, spp=SPP, seed=SEED, fp16=True)


def test_a_scene_without_the_emitter_renders_what_it_rendered(tmp_path):
    scene, _ = _file_scene(tmp_path, am.XML.replace(am.WORLD, ""), "plain.xml", dark=False)
    assert scene.data.ambient is None and scene.ambient_record() is None and not [k for k in mi.traverse(scene).keys() if "radiance" in k]
    img = mi.render(scene, spp=SPP, seed=SEED).torch().clone()
    sd = scene.scene_desc(tex_channels=1)
    assert float(img.mean()) > 0 and torch.equal(img, scene.geom.render_fwd(sd, scene.materials_arg(sd), torch.zeros(32, 32, 1, device=DEV), SPP, SEED))


def test_randomisation_reaches_the_render_key_by_key(tmp_path):
    import random

    import fireflies_amd as ff

    scene, params = _file_scene(tmp_path)
    ffs = ff.Scene(params, device=DEV)
    names = [l.name() for l in ffs.lights()]
    assert names == ["emit-Spot", "emit-World"], names  # (listed with the lights, the main spot first)
    light = ffs.light("emit-World")
    lo, hi = torch.tensor([2.0, 3.0, 4.0], device=DEV), torch.tensor([2.5, 3.5, 4.5], device=DEV)
    light.add_vec3_key("radiance.value", lo, hi)
    ffs.train()
    for k in range(3):
        torch.manual_seed(k)
        random.seed(k)
        ffs.randomize()
    img = mi.render(scene, spp=SPP, seed=SEED).torch()
    drawn = params["emit-World.radiance.value"].torch().reshape(3).to(DEV)
    assert bool(((drawn >= lo) & (drawn <= hi)).all()), drawn
    sd = scene.scene_desc(tex_channels=1)
    assert torch.equal(img, scene.geom.render_fwd(sd, scene.materials_arg(sd), torch.zeros(32, 32, 1, device=DEV), SPP, SEED, ambient=drawn))
    print(scene.update_paths, scene.update_fallbacks)
    assert scene.update_paths["native"] == 0 and scene.update_fallbacks.get("constant emitter", 0) >= 1, (scene.update_paths, scene.update_fallbacks)


def test_gradients_and_refusals_through_mi_render(tmp_path):
    scene, params = _file_scene(tmp_path, dark=False)
    bare, bare_params = _file_scene(tmp_path, am.XML.replace(am.WORLD, ""), "plain.xml", dark=False)
    sd = scene.scene_desc(tex_channels=1)
    tex = gpu.rand_tex(sd, 5)[..., 0].contiguous()
    gimg = gpu.rand_gimg(sd, 6)
    grads = []
    for s, p in ((scene, params), (bare, bare_params)):
        leaf = tex.clone().requires_grad_(True)
        p["tex.data"] = leaf
        p.update()
        (mi.render(s, spp=SPP, seed=SEED).torch() * gimg).sum().backward()
        grads.append(leaf.grad.clone())
        p["tex.data"] = tex
        p.update()
    assert float(grads[1].abs().sum()) > 0
    torch.testing.assert_close(grads[0], grads[1], rtol=1e-5, atol=1e-8)
    assert float((mi.render(scene, spp=SPP, seed=SEED).torch() - mi.render(bare, spp=SPP, seed=SEED).torch()).mean()) > 0.1
    params["mat-Floor.brdf_0.base_color.value"] = mi.Color3f(torch.tensor([0.5, 0.5, 0.5], requires_grad=True))
    params.update()
    with pytest.raises(NotImplementedError, match="constant emitter.*not differentiated"):
        mi.render(scene, spp=SPP, seed=SEED)
    with pytest.raises(NotImplementedError, match="constant emitter.*not differentiated"):
        mi.render_forward(scene, params, {"tex.data": torch.ones_like(tex)}, spp=SPP, seed=SEED)


def test_the_pattern_optimizer_on_a_scene_with_ambient_light():
    from fireflies_amd import workloads
    from fireflies_amd.optim import PatternOptimizer

    wl = workloads.vocalfold(device=DEV, width=64, height=56, tex=96, grid=6, frames=5, n_fold=20, tube=(20, 24), ambient=(0.2, 0.2, 0.25))
    opt = PatternOptimizer(wl.mi_scene, wl.ff_scene, wl.laser, sigma=wl.sigma, tex_size=wl.tex_size, spp=8)
    with pytest.raises(NotImplementedError, match="constant emitter.*step_autograd"):
        opt.step()
    for _ in range(2):
        out = opt.step_autograd()
    assert torch.isfinite(wl.laser._rays).all()
    assert np.isfinite(float(out["loss"]))
