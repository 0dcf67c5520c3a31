"""Perlin base-colour textures on the device: ffx_perlin_texture against the float64 restatement tests/ref_perlin.py on every case of
the suite in both layouts — bounded per case by four times the float32 torch CPU path's own deviation from that restatement —, the extremes, the
degenerate plane, determinism, the sampler's device engine under the golden g13's seeds, and the texture's way into the renderer without a copy."""
import random

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops
from fireflies_amd.sampling import NoiseTextureLerpSampler
from fireflies_amd.sampling import noise_texture_lerp as ntl
from tests import corner_scenes as cs
from tests import perlin_support as ps
from tests import ref_perlin
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYOUTS = ("hwc", "chw")
BLACK_WHITE = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def device_texture(name, seed=0, layout="hwc", colors=(ps.COLOR_A, ps.COLOR_B), **kw):
    """ops.perlin_texture on the case's inputs -> [3, h, w] on the device, whatever the layout"""
    i = ps.inputs(name, seed)
    out = ops.perlin_texture(i.packed_angles.to(DEV), i.packed_pos.to(DEV), i.octaves, i.res, i.persistence, i.shape, torch.tensor(colors[0], device=DEV),
                             torch.tensor(colors[1], device=DEV), layout=layout, **kw)
    assert out.shape == (i.shape + (3,) if layout == "hwc" else (3,) + i.shape) and out.is_contiguous() and out.dtype == torch.float32
    return out.permute(2, 0, 1) if layout == "hwc" else out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(ref_perlin.CASES))
def test_the_texture_is_the_float64_restatement(name, layout):
    """the bound is the reference's: four times what the float32 torch path on the CPU deviates from float64 on the same case (the margin of
    tests/test_refit_gpu.py for a device against its oracle)"""
    got = device_texture(name, layout=layout).cpu().numpy().astype(np.float64)
    yardstick = ps.torch_deviation(name)
    dev = float(np.abs(got - ps.reference(name)).max())
    print(f"{name} {layout}: device against float64 {dev:.3e}, float32 torch CPU path against float64 {yardstick:.3e}, bound {4 * yardstick:.3e}")
    assert np.isfinite(got).all() and yardstick > 0
    assert dev <= 4 * yardstick


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(ref_perlin.CASES))
def test_the_extremes_are_exact(name, layout):
    got = device_texture(name, layout=layout, colors=BLACK_WHITE)
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert bool(((got >= 0.0) & (got <= 1.0)).all())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


@pytest.mark.parametrize("seed", range(8))
def test_the_extreme_texels_are_the_references(seed):
    i = ps.inputs("G", seed)
    got = device_texture("G", seed, colors=BLACK_WHITE)[0].cpu().numpy()
    plane = ref_perlin.noise(i.angles, i.pos, i.shape, i.res, i.octaves, i.persistence)
    assert got.argmin() == plane.argmin() and got.argmax() == plane.argmax()
    assert got.reshape(-1)[plane.argmin()] == 0.0 and got.reshape(-1)[plane.argmax()] == 1.0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_plane_of_one_texel_cells_is_nan_as_the_torch_engine_gives_it(layout):
    got = device_texture("F'", layout=layout)
    assert bool(torch.isnan(got).all())
    i = ps.inputs("F'")
    plane = ntl.perlin_2d_octaves(i.shape, i.res, i.octaves, i.persistence, device=DEV, angles=[torch.from_numpy(a) for a in i.angles])
    same = ntl.blend(plane, torch.tensor(ps.COLOR_A), torch.tensor(ps.COLOR_B), DEV)
    assert same.shape == got.shape and bool(torch.isnan(same).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_give_the_same_bits(layout):
    i = ps.inputs("G")
    first = device_texture("G", layout=layout)
    ws = torch.full((_abi.perlin_workspace_bytes(*i.shape) + 64,), 0xFF, dtype=torch.uint8, device=DEV)  # (whatever the workspace held: NaN patterns here)
    second = device_texture("G", layout=layout, workspace=ws)
    assert first.data_ptr() != second.data_ptr()  # a fresh tensor per call
    assert torch.equal(first.contiguous().view(torch.int32), second.contiguous().view(torch.int32))
    with pytest.raises(ValueError, match="workspace"):
        device_texture("G", layout=layout, workspace=ws[:16])


@pytest.mark.parametrize("tag", ps.G13_TAGS)
def test_the_device_engine_under_the_golden_seeds(tag):
    """the seeds and draws of tests/test_api_cpu.py::test_noise_texture_sampler_matches_the_reference: the fixture at its tolerances, the torch engine on
    the same device at the rule of test_the_texture_is_the_float64_restatement, and both generators where the torch engine leaves them"""
    g = load_golden("g13_noise_texture.npz")
    seed, shape = int(g[f"{tag}_seed"]), tuple(int(v) for v in g[f"{tag}_shape"])
    # the yardstick: the float32 torch path on the CPU against float64 on the same draws
    draws = ps.g13_replay(g, tag, lambda a, b, s: NoiseTextureLerpSampler(color_a=a, color_b=b, texture_shape=s, device=torch.device("cpu")))
    textures, states = {}, {}
    for engine in ("cpu", "torch", "device"):
        torch.manual_seed(seed)
        random.seed(seed)
        ca, cb = torch.rand(3), torch.rand(3)
        smp = NoiseTextureLerpSampler(color_a=ca, color_b=cb, texture_shape=shape, device=torch.device("cpu" if engine == "cpu" else DEV),
                                      engine="torch" if engine == "cpu" else engine)
        textures[engine] = [smp.sample() for _ in range(2)]
        states[engine] = (random.getstate(), torch.get_rng_state())
    for k in range(2):
        t = textures["device"][k]
        assert t.shape == (3,) + shape and t.moveaxis(0, -1).is_contiguous()
        t = t.cpu().numpy()
        np.testing.assert_allclose(t[:, ::8, ::8], g[f"{tag}_tex{k}_sub"], rtol=0, atol=1e-6)
        assert float(t.astype(np.float64).mean()) == pytest.approx(float(g[f"{tag}_tex{k}_mean"]), abs=1e-7)
        assert float((t.astype(np.float64) ** 2).sum()) == pytest.approx(float(g[f"{tag}_tex{k}_sq"]), rel=1e-6)
        args, colors = draws[k]
        yardstick = float(np.abs(textures["cpu"][k].numpy().astype(np.float64) - ref_perlin.texture(*args, *colors)).max())
        apart = float(np.abs(t.astype(np.float64) - textures["torch"][k].cpu().numpy().astype(np.float64)).max())
        print(f"g13 {tag} texture {k}: device engine against the torch engine on the device {apart:.3e}, float32 torch CPU path against float64 "
              f"{yardstick:.3e}, bound {4 * yardstick:.3e}")
        assert yardstick > 0 and apart <= 4 * yardstick
    for engine in ("torch", "device"):
        assert states[engine][0] == states["cpu"][0] and torch.equal(states[engine][1], states["cpu"][1])


def test_the_texture_reaches_the_renderer_without_a_copy():
    """sample() hands out the [3, H, W] view of [H, W, 3] storage: moved back, it is the tensor the scene description points the kernels at, and the render
    is the one of the same values assigned through numpy (main.py:153)"""
    ms = mi.load_scene_data(cs.corner(cs.PRINCIPLED, {"roughness": 0.6}, base_tex=cs.base_texture()), device=DEV, shadows=True)
    params = mi.traverse(ms)
    params["tex.data"] = torch.rand(32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.manual_seed(7)
    random.seed(7)  # (an 8 x 8 lattice in two octaves, then a 2 x 2 lattice: both fit the texture)
    smp = NoiseTextureLerpSampler(color_a=torch.rand(3, device=DEV), color_b=torch.rand(3, device=DEV), texture_shape=(64, 128), device=DEV, engine="device")
    t = smp.sample()
    assert t.shape == (3, 64, 128) and t.moveaxis(0, -1).is_contiguous() and t.moveaxis(0, -1).data_ptr() == t.data_ptr()
    key = "mat-Floor.brdf_0.base_color.data"
    params[key] = mi.TensorXf(t.moveaxis(0, -1))
    params.update()
    sd = ms.scene_desc(tex_channels=1)
    assert sd.n_base_tex == 1 and sd.base_tex[0] == t.data_ptr() and (sd.base_tex_h[0], sd.base_tex_w[0]) == (64, 128)
    direct = mi.render(ms, spp=8, seed=4).torch().clone()
    params[key] = mi.TensorXf(t.moveaxis(0, -1).cpu().numpy())
    params.update()
    assert ms.scene_desc(tex_channels=1).base_tex[0] != t.data_ptr()
    through_numpy = mi.render(ms, spp=8, seed=4).torch()
    assert torch.equal(direct, through_numpy) and float(direct.max()) > 0
    other = smp.sample()  # the next texture is new storage: a render still reading the previous one is not disturbed
    assert other.data_ptr() != t.data_ptr() and not torch.equal(other, t)
