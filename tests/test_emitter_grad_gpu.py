"""The extra emitters' adjoint on the GPU: k_lights_bwd / k_lights_grad_reduce against the parent's forward (the dot-product identity),
against the float64 restatements (tests/ref_sun.py, tests/ref_ambient.py), exact linearity through mi.render, the bit identities, the sample
bookkeeping, and mi.render's autograd.  gpu.rand_gimg is positive: no term of an inner product cancels."""
import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, scenes
from tests import gpu_support as gpu
from tests import light_scenes as ls
from tests import ref_ambient as ra
from tests import ref_path as rp
from tests import ref_sun as rs
from tests import sun_scenes as ss
from tests.gpu_support import DEV, table

pytestmark = pytest.mark.gpu

SPP, SEED = 16, 7
LA = (0.2, 0.25, 0.3)
# the dot-product identity's bound: both sides are fp32 sums of the same non-negative per-sample terms in different orders, and the forward's side
# is the difference of two fp32 images.  4 x the worst relative deviation of the first run on the MI355X over the 48 tables of test 1 — 1.516e-7, 21x19,
# principled rows, box film, max_depth 4 (every case prints its figure) — and far below the cap of 1e-4.  Neither side uses an atomic: the
# figures are the same on every run
RTOL = 6e-7


def case(film, principled, gaussian):
    """gpu.corner_case on sun_scenes without its direct-light images; in their place the image gradient"""
    c = gpu.corner_case(ss.corner, film, principled, gaussian, SPP, SEED, direct=False)
    return (*c[:6], gpu.rand_gimg(c[1], 3))


def fwd(ms, sd, mats, tex, t=None, amb=None, depth=2, spp=SPP):
    return ms.geom.render_fwd(sd, mats, tex, spp, SEED, max_depth=depth, lights=t, ambient=amb, lights_directional=t is not None)


def bwd(ms, sd, mats, gimg, t=None, amb=None, depth=2, spp=SPP):
    return ms.geom.render_bwd(sd, mats, spp, SEED, gimg, max_depth=depth, lights=t, ambient=amb, lights_directional=t is not None, emitters=True)


def unit(t, k, ch):
    """record k alone at power e_ch"""
    one = t[k:k + 1].clone()
    one[:, 16:19] = 0.0
    one[0, 16 + ch] = 1.0
    return one


def forward_dots(ms, sd, mats, tex, gimg, t, amb, depth, spp=SPP):
    """[n + 1, 3] in float64 on the host: sum_p gimg[p, ch] (render_fwd(record k alone at power e_ch) - render_fwd(no table))[p, ch]; the last row: the
    constant emitter at radiance e_ch (zeros without one)"""
    g = gimg.double().cpu()
    plain = fwd(ms, sd, mats, tex, depth=depth, spp=spp).double().cpu()
    n = 0 if t is None else int(t.shape[0])
    out = torch.zeros(n + 1, 3, dtype=torch.float64)
    for k in range(n):
        for ch in range(3):
            img = fwd(ms, sd, mats, tex, unit(t, k, ch), depth=depth, spp=spp).double().cpu()
            out[k, ch] = ((img - plain) * g)[..., ch].sum()
    if amb is not None:
        for ch in range(3):
            e = [0.0, 0.0, 0.0]
            e[ch] = 1.0
            img = fwd(ms, sd, mats, tex, amb=e, depth=depth, spp=spp).double().cpu()
            out[n, ch] = ((img - plain) * g)[..., ch].sum()
    return out


def block_of(eg):
    """an EmitterGrad as [n + 1, 3] float64 on the host (the ambient row zero without one)"""
    amb = eg.ambient if eg.ambient is not None else torch.zeros(3, device=eg.lights.device)
    return torch.cat([eg.lights, amb[None]]).double().cpu()


def worst(got, want, what):
    """the worst relative deviation over the entries the forward lights; an entry it leaves dark must be an exact zero"""
    lit = want > 0
    assert torch.equal(got[~lit], torch.zeros_like(got[~lit])), (what, got, want)
    assert lit.any(), what
    rel = float(((got - want).abs()[lit] / want[lit]).max())
    print(f"{what}: worst relative deviation {rel:.3e} [{RTOL:.1e}] over {int(lit.sum())} entries")
    return rel


# ------------------------------------------------------------------ 1. against the parent's forward: the dot-product identity
@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("film", sorted(ss.FILMS))
@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("principled", [False, True])
def test_the_block_is_the_forwards_inner_product(principled, gaussian, film, depth):
    ms, sd, _, _, tex, mats, gimg = case(film, principled, gaussian)
    for name, t, amb in (("point + spot + sun", table(ls.POINT, ls.SPOT_B, ss.SUN_A), None), ("eight + ambient", table(*ss.eight()), LA)):
        _, eg = bwd(ms, sd, mats, gimg, t, amb, depth)
        assert eg.lights.shape == (t.shape[0], 3) and (eg.ambient is None) == (amb is None)
        want = forward_dots(ms, sd, mats, tex, gimg, t, amb, depth)
        assert bool((want[:t.shape[0]] > 0).all()), want  # (every record lights the corner in every channel)
        rel = worst(block_of(eg), want, f"{film} principled={principled} gaussian={gaussian} depth {depth}, {name}")
        assert rel <= RTOL


# ------------------------------------------------------------------ 2. against float64, every ray against every triangle
@pytest.mark.parametrize("depth,principled,gaussian,film", [(2, False, False, "21x19"), (2, True, True, "24x24"), (3, True, False, "24x24"), (3, False, True, "21x19")])
def test_the_block_matches_the_float64_restatement(depth, principled, gaussian, film):
    """the inner product is a weighted image sum: held to 1 % of the sum, the third of the conditions of tests/support.py's `independent`"""
    ms, sd, world, rows, tex, mats, gimg = case(film, principled, gaussian)
    lights = [ls.POINT, ls.SPOT_B, ss.SUN_A]
    t = table(*lights)
    _, eg = bwd(ms, sd, mats, gimg, t, LA, depth)
    got = block_of(eg).numpy()
    g = gimg.double().cpu().numpy()
    stddev = 0.5 if gaussian else None
    main_ref = rp.render_fwd(*world, sd, rows, tex.cpu().numpy(), SPP, SEED, depth, gaussian_stddev=stddev)
    host = ops.pack_lights(lights).numpy().astype(np.float64)
    parts = []
    for k in range(len(lights)):
        one = host[k:k + 1].copy()
        one[0, 16:19] = 1.0
        parts.append((rs.render_sun(*world, sd, rows, one, SPP, SEED, max_depth=depth, gaussian_stddev=stddev), np.asarray(lights[k].intensity)))
    parts.append((ra.render_ambient(*world, sd, rows, (1.0, 1.0, 1.0), SPP, SEED, max_depth=depth, gaussian_stddev=stddev), np.asarray(LA)))
    whole = main_ref + sum(u * c for u, c in parts)
    for k, (u, c) in enumerate(parts):
        share = (u * c).mean() / whole.mean()
        want = (u * g).sum((0, 1))
        print(f"depth {depth} principled={principled} gaussian={gaussian} {film} row {k}: share of the image {share:.3f} [> 0.05], got {got[k]}, float64 {want}, "
              f"relative {np.abs(got[k] - want) / want}")
        assert share > 0.05
        assert (want > 0).all() and (np.abs(got[k] - want) <= 0.01 * want).all()


# ------------------------------------------------------------------ 3. exact linearity through the public interface
def _mi_scene(film="24x24", principled=True, gaussian=False, lights=(ls.POINT, ls.SPOT_B, ss.SUN_A), ambient=LA):
    sc = ss.corner(film, principled)
    sc.lights = list(lights)
    sc.ambient = scenes.AmbientData("emit-World", tuple(ambient)) if ambient is not None else None
    ms = mi.load_scene_data(sc, device=DEV, shadows=True)
    if gaussian:
        ms.rfilter = "gaussian"
    sd = ms.scene_desc(tex_channels=1)
    p = mi.traverse(ms)
    p["tex.data"] = gpu.rand_tex(sd, 5)[..., 0].contiguous()
    p.update()
    return ms, p, gpu.rand_gimg(sd, 6)


_KEYS = {"emit-Light.intensity.value": ls.POINT.intensity, "emit-SunA.irradiance.value": ss.SUN_A.intensity, "emit-World.radiance.value": LA}


@pytest.mark.parametrize("integrator", ["path", "prb"])
@pytest.mark.parametrize("gaussian", [False, True])
def test_the_loss_is_exactly_linear_through_mi_render(gaussian, integrator):
    """L(c) = <gimg, mi.render>: L(c + d) - L(c) = <grad, d> for a d of the size of c, within test 1's bound (the left side is test 1's difference of two
    fp32 images)"""
    ms, p, gimg = _mi_scene("21x19" if gaussian else "24x24", True, gaussian)
    it = mi.load_dict({"type": integrator, "max_depth": 3})

    def L():
        return (mi.render(ms, spp=SPP, seed=SEED, integrator=it).torch().double() * gimg.double()).sum()

    for key, c in _KEYS.items():
        leaf = gpu.leaf(list(c))
        p[key] = leaf
        p.update()
        l0 = L()
        l0.backward()
        delta = torch.tensor(c, dtype=torch.float64) * torch.tensor([0.7, 1.1, 0.9], dtype=torch.float64)
        p[key] = mi.Color3f((torch.tensor(c, dtype=torch.float64) + delta).float())
        p.update()
        assert not p._emitter_leaves
        with torch.no_grad():
            l1 = L()
        lhs, rhs = float(l1 - l0.detach()), float((leaf.grad.double().cpu() * delta).sum())
        print(f"{integrator} gaussian={gaussian} {key}: L(c + d) - L(c) = {lhs:.9g}, <grad, d> = {rhs:.9g}, relative {abs(lhs - rhs) / rhs:.3e} [{RTOL:.1e}]")
        assert rhs > 0 and abs(lhs - rhs) <= RTOL * rhs
        p[key] = mi.Color3f(torch.tensor(c))
        p.update()


# ------------------------------------------------------------------ 4. bit identities
DARK_SUN = scenes.LightData("emit-NoSun", "directional", np.zeros((4, 4), np.float32), (1.0, 1.0, 1.0))
AWAY_SPOT = scenes.LightData("emit-Away", "spot", scenes.look_at((2.7, 0.6, 2.2), (6.0, 3.0, 6.0), up=(0, 0, 1)), (6.0, 9.0, 12.0), 35.0, 22.0)


@pytest.mark.parametrize("depth,gaussian,film", [(2, False, "21x19"), (2, True, "24x24"), (3, False, "24x24"), (3, True, "21x19")])
def test_bit_identities(depth, gaussian, film):
    ms, sd, _, _, tex, mats, gimg = case(film, True, gaussian)
    t = table(ls.POINT, DARK_SUN, ss.SUN_A, AWAY_SPOT, ls.SPOT_B)
    g0, a = bwd(ms, sd, mats, gimg, t, LA, depth)
    g1, b = bwd(ms, sd, mats, gimg, t, LA, depth)
    assert torch.equal(a.lights, b.lights) and torch.equal(a.ambient, b.ambient)  # (no atomics: two calls, the same bits)
    assert float(a.lights[[0, 2, 4]].min()) > 0 and float(a.ambient.min()) > 0
    # a record that lights nothing: an exact zero row
    assert torch.equal(a.lights[[1, 3]], torch.zeros(2, 3, device=DEV))
    assert float(fwd(ms, sd, mats, tex, t[[1, 3]], depth=depth).sub(fwd(ms, sd, mats, tex, depth=depth)).abs().max()) == 0.0
    # gtex is that of the call without the bit
    plain = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth)
    assert float(plain.abs().sum()) > 0
    torch.testing.assert_close(g0, plain, rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(g1, plain, rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=depth, lights=t, ambient=LA, lights_directional=True), plain, rtol=1e-5, atol=1e-8)
    # the whole block, through a buffer of the caller's: rows >= n and the ambient row without the bit are exact zeros whatever the buffer held
    n_tex = sd.proj.tex_h * sd.proj.tex_w * sd.proj.tex_channels
    buf = torch.full((n_tex + _abi.emitter_grad_floats(sd.cam.width, sd.cam.height),), float("nan"), device=DEV)
    ms.geom._render_bwd_emitters(sd, mats, SPP, SEED, gimg, None, depth, 5, t[:2], None, True, out=buf)
    block = buf[n_tex:n_tex + 27].view(9, 3)
    assert torch.equal(block[0], a.lights[0]) and torch.equal(block[1:], torch.zeros(8, 3, device=DEV))
    ms.geom._render_bwd_emitters(sd, mats, SPP, SEED, gimg, None, depth, 5, None, LA, False, out=buf)
    block = buf[n_tex:n_tex + 27].view(9, 3)
    assert torch.equal(block[8], a.ambient) and torch.equal(block[:8], torch.zeros(8, 3, device=DEV))


# ------------------------------------------------------------------ 5. sample bookkeeping
@pytest.mark.parametrize("spp,gaussian", [(65, False), (130, True), (1, False), (1, True)])
def test_ragged_passes_and_one_sample(spp, gaussian):
    ms, sd, _, _, tex, mats, gimg = case("21x19", False, gaussian)
    t = table(ls.POINT, ss.SUN_B)
    _, eg = bwd(ms, sd, mats, gimg, t, LA, 3, spp=spp)
    want = forward_dots(ms, sd, mats, tex, gimg, t, LA, 3, spp=spp)
    assert worst(block_of(eg), want, f"{spp} samples per pixel, gaussian={gaussian}") <= RTOL


@pytest.mark.parametrize("gaussian", [False, True])
def test_skipped_pixels_write_zeros_and_a_stale_workspace_does_not_leak(gaussian):
    """gimg zero on the upper half of the film: pixel_adjoint skips those pixels (the gaussian film: those whose whole window is dark).  The first call
    finds NaN in the buffer, the second the first call's slots: neither may show"""
    ms, sd, _, _, tex, mats, gimg = case("21x19", True, gaussian)
    t = table(ls.POINT, ls.SPOT_B, ss.SUN_A)
    H, W = sd.cam.height, sd.cam.width
    half = gimg.clone()
    half[:H // 2] = 0.0
    n_tex = sd.proj.tex_h * sd.proj.tex_w * sd.proj.tex_channels
    buf = torch.full((n_tex + _abi.emitter_grad_floats(W, H),), float("nan"), device=DEV)

    def call(g):
        ms.geom._render_bwd_emitters(sd, mats, SPP, SEED, g, None, 3, 5, t, LA, True, out=buf)
        assert bool(torch.isfinite(buf).all())  # (gtex, the block and every slot of the workspace were written)
        return buf[n_tex:n_tex + 27].view(9, 3).clone(), buf[n_tex + 27:].view(27, H * W).clone()

    full, _ = call(gimg)
    got, slots = call(half)
    fresh = bwd(ms, sd, mats, half, t, LA, 3)[1]
    assert torch.equal(got[:3], fresh.lights) and torch.equal(got[8], fresh.ambient)
    dark_rows = H // 2 - (2 if gaussian else 0)  # (the gaussian film's window reaches two rows up)
    assert dark_rows > 0 and torch.equal(slots[:, :dark_rows * W], torch.zeros(27, dark_rows * W, device=DEV))
    assert float(slots[:, (H // 2) * W:].abs().sum()) > 0 and float((full[:3] - got[:3]).min()) > 0
    want = forward_dots(ms, sd, mats, tex, half, t, LA, 3)
    assert worst(torch.cat([got[:3], got[8:]]).double().cpu(), want, f"half the film dark, gaussian={gaussian}") <= RTOL


# ------------------------------------------------------------------ 6. mi.render's autograd
@pytest.mark.parametrize("gaussian", [False, True])
def test_backward_fills_every_kind_of_leaf_and_the_texture_in_one_pass(gaussian):
    ms, p, gimg = _mi_scene("24x24", True, gaussian)
    sd = ms.scene_desc(tex_channels=1)
    tex = gpu.rand_tex(sd, 5)[..., 0].contiguous().requires_grad_(True)
    lamp, sun, world = gpu.leaf(list(ls.POINT.intensity)), gpu.leaf(3.0), gpu.leaf(list(LA))
    old = gpu.leaf(list(ls.SPOT_B.intensity))
    p["tex.data"] = tex
    p["emit-Light.intensity.value"] = lamp
    p["emit-SunA.irradiance.value"] = sun  # (a scalar: broadcast to the three channels)
    p["emit-World.radiance.value"] = mi.Color3f(world)
    p["emit-SecondSpot.intensity.value"] = old
    p["emit-SecondSpot.intensity.value"] = mi.Color3f(torch.tensor(ls.SPOT_B.intensity))  # (overwritten by a plain value: no leaf)
    p.update()
    assert sorted(p._emitter_leaves) == ["emit-Light.intensity.value", "emit-SunA.irradiance.value", "emit-World.radiance.value"]
    it = mi.load_dict({"type": "path", "max_depth": 3})
    img = mi.render(ms, spp=SPP, seed=SEED, integrator=it).torch()
    t = ms.lights_table()
    assert t[2, 16:19].tolist() == [3.0, 3.0, 3.0]
    mats = ms.materials_arg(sd)
    assert torch.equal(img.detach(), ms.geom.render_fwd(sd, mats, tex.detach()[..., None].contiguous(), SPP, SEED, max_depth=3, lights=t, ambient=LA, lights_directional=True))
    (img * gimg).sum().backward()
    gtex, eg = ms.geom.render_bwd(sd, mats, SPP, SEED, gimg, max_depth=3, lights=t, ambient=LA, lights_directional=True, emitters=True)
    assert torch.equal(lamp.grad, eg.lights[0]) and torch.equal(world.grad, eg.ambient) and old.grad is None
    assert sun.grad.shape == () and torch.equal(sun.grad, eg.lights[2].sum())
    assert float(lamp.grad.min()) > 0 and float(sun.grad) > 0 and float(world.grad.min()) > 0 and float(gtex.abs().sum()) > 0
    torch.testing.assert_close(tex.grad, gtex[..., 0], rtol=1e-5, atol=1e-8)
    # an aov integrator serves the RGB channels
    lamp.grad = None
    aov = mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": "path", "max_depth": 3}})
    block = mi.render(ms, spp=SPP, seed=SEED, integrator=aov).torch()
    assert torch.equal(block[..., 1:].detach(), img.detach())
    (block[..., 1:] * gimg).sum().backward()
    assert torch.equal(lamp.grad, eg.lights[0])


def test_the_pose_guard_and_the_mixed_scene():
    ms, p, gimg = _mi_scene()
    p["emit-Light.intensity.value"] = gpu.leaf(list(ls.POINT.intensity))
    p.update()
    img = mi.render(ms, spp=SPP, seed=SEED).torch()
    ms.geom.version += 1  # (what a pose update does)
    with pytest.raises(RuntimeError, match="the scene was updated between the render and its backward"):
        (img * gimg).sum().backward()
    key = sorted(k for k in p._leaf_keys if k.endswith(".brdf_0.base_color.value"))[0]
    p[key] = mi.Color3f(torch.tensor([0.5, 0.5, 0.5], requires_grad=True))
    p.update()
    with pytest.raises(NotImplementedError, match="extra emitters.*not differentiated"):
        mi.render(ms, spp=SPP, seed=SEED)
    with pytest.raises(ValueError, match="fp16"):
        mi.render(ms, spp=SPP, seed=SEED, fp16=True)


def test_adam_recovers_a_lamp_and_the_world_from_a_photograph():
    """24 x 24, 16 spp, fixed seed: the image is linear in the two leaves and the loss quadratic; 200 steps of Adam bring each within 1 %"""
    ms, p, _ = _mi_scene("24x24", False, False, lights=(ls.POINT,), ambient=LA)
    with torch.no_grad():
        target = mi.render(ms, spp=SPP, seed=SEED).torch().clone()
    want_lamp, want_world = torch.tensor(ls.POINT.intensity, device=DEV), torch.tensor(LA, device=DEV)
    lamp, world = gpu.leaf([8.0, 30.0, 9.0]), gpu.leaf([0.5, 0.1, 0.45])
    opt = torch.optim.Adam([{"params": [lamp], "lr": 1.5}, {"params": [world], "lr": 0.03}])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.975)
    for _ in range(200):
        p["emit-Light.intensity.value"] = lamp
        p["emit-World.radiance.value"] = world
        p.update()
        err = ((mi.render(ms, spp=SPP, seed=SEED).torch() - target) ** 2).mean()
        opt.zero_grad()
        err.backward()
        opt.step()
        sched.step()
    print("lamp", lamp.detach().tolist(), "world", world.detach().tolist(), "loss", float(err))
    assert float(((lamp.detach() - want_lamp).abs() / want_lamp).max()) <= 0.01
    assert float(((world.detach() - want_world).abs() / want_world).max()) <= 0.01
