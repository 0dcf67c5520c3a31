"""Perlin base-colour textures without a device: the float64 restatement tests/ref_perlin.py against the sampler's float32 torch path on
every case of the suite and against the golden g13 under its seeds and draws, the workspace macro of include/ffx_labels.h against its Python mirror,
the refusals of ffx_perlin_texture (each before any launch), what the ops wrapper turns away, and the sampler's engines: the shared draws leave
both generators where the torch engine leaves them."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, _lib, ops
from fireflies_amd.sampling import NoiseTextureLerpSampler
from fireflies_amd.sampling import noise_texture_lerp as ntl
from tests import perlin_support as ps
from tests import ref_perlin
from tests.conftest import load_golden
from tests.support import FFX_ERR_ARG, ROOT, c_compiler

# float32 against float64 on one texel, to first order: the value passes through about sixteen dependent float32 roundings per octave (a difference, two
# products and their sum per corner, three lerps of three operations, the two scalings, the accumulation, then the normalisation and the blend), each
# within 2^-24 of an intermediate, and no intermediate exceeds 2 sqrt(2) sum a_o; the normalisation divides by the plane's max - min, the colours lie
# within 0..1: sixteen units of 2^-24 times perlin_support.magnitude, the quotient of those two (from the float64 plane, at least one)
ROUNDINGS = 16 * 2.0**-24


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(ref_perlin.CASES))
def test_the_float64_restatement_is_the_torch_path(name, seed):
    got, want = ps.torch_path(name, seed), ps.reference(name, seed)
    assert got.shape == want.shape == (3,) + ref_perlin.CASES[name][0]
    dev, bound = ps.torch_deviation(name, seed), ROUNDINGS * ps.magnitude(name, seed)
    print(f"{name} seed {seed}: float32 torch path against float64, largest deviation {dev:.3e} [{bound:.3e}: magnitude {ps.magnitude(name, seed):.2f}]")
    assert np.isfinite(want).all() and dev <= bound
    lo, hi = np.minimum(ps.COLOR_A, ps.COLOR_B), np.maximum(ps.COLOR_A, ps.COLOR_B)
    for c in range(3):  # both extremes are reached in every channel
        assert want[c].min() == pytest.approx(lo[c], abs=1e-7) and want[c].max() == pytest.approx(hi[c], abs=1e-7)


def test_one_texel_cells_add_exact_zeros_and_a_plane_of_them_is_nan():
    i = ps.inputs("F")
    both = ref_perlin.noise(i.angles, i.pos, i.shape, i.res, 2, i.persistence)
    first = ref_perlin.noise(i.angles[:1], i.pos[:1], i.shape, i.res, 1, i.persistence)
    assert np.array_equal(both, first) and not i.pos[1][0].any() and not i.pos[1][1].any()
    assert np.isnan(ps.reference("F'")).all() and np.isnan(ps.torch_path("F'")).all()


@pytest.mark.parametrize("tag", ps.G13_TAGS)
def test_the_float64_restatement_reproduces_the_golden_textures(tag):
    """the seeds and draws of tests/test_api_cpu.py::test_noise_texture_sampler_matches_the_reference, at its tolerances"""
    g = load_golden("g13_noise_texture.npz")
    draws = ps.g13_replay(g, tag, lambda a, b, shape: NoiseTextureLerpSampler(color_a=a, color_b=b, texture_shape=shape, device=torch.device("cpu")))
    for k, (args, colors) in enumerate(draws):
        t = ref_perlin.texture(*args, *colors)
        np.testing.assert_allclose(t[:, ::8, ::8], g[f"{tag}_tex{k}_sub"], rtol=0, atol=1e-6)
        assert float(t.mean()) == pytest.approx(float(g[f"{tag}_tex{k}_mean"]), abs=1e-7)
        assert float((t**2).sum()) == pytest.approx(float(g[f"{tag}_tex{k}_sq"]), rel=1e-6)


def test_the_workspace_macro_and_its_python_mirror_agree(tmp_path):
    cc = c_compiler()
    assert cc is not None, "a C compiler is needed to evaluate the header's macro"
    cases = [(1, 1), (16, 64), (17, 64), (16, 65), (2, 2), (257, 130), (1024, 1024), (1000, 24), (32768, 32768)]
    src = ['#include <stdio.h>', '#include "ffx_labels.h"', "int main(void) {"]
    src += [f'  printf("%zu\\n", FFX_PERLIN_WORKSPACE_BYTES({h}, {w}));' for h, w in cases]
    src += ["  return 0;", "}"]
    (tmp_path / "ws.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "ws.c"), "-o", str(tmp_path / "ws")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ws")]).split()]
    assert got == [_abi.perlin_workspace_bytes(*c) for c in cases]
    assert _abi.perlin_workspace_bytes(1024, 1024) == 16 + 8 * 1024


# every refusal of DESIGN.md 4.12: (what changes against a valid call, the words its message must hold)
REFUSALS = {
    "angles NULL": (dict(angles=None), "angles is NULL"),
    "pos NULL": (dict(pos=None), "pos is NULL"),
    "color_a NULL": (dict(color_a=None), "color_a is NULL"),
    "color_b NULL": (dict(color_b=None), "color_b is NULL"),
    "out NULL": (dict(out=None), "out is NULL"),
    "workspace NULL": (dict(workspace=None), "workspace is NULL"),
    "workspace misaligned": (dict(workspace="misaligned"), "workspace must be 8-byte aligned"),
    "octaves 0": (dict(octaves=0), "octaves 0"),
    "octaves 9": (dict(octaves=9, h=32768, w=32768), "octaves 9"),
    "h 0": (dict(h=0), "h 0"),
    "w 0": (dict(w=0), "w 0"),
    "h 32769": (dict(h=32769), "h 32769"),
    "w 32769": (dict(w=32769), "w 32769"),
    "r0 0": (dict(r0=0), "r0 0"),
    "r1 0": (dict(r1=0), "r1 0"),
    "rows below a cell at octave 0": (dict(r0=9), "octave 0"),
    "columns below a cell at octave 2": (dict(r1=3), "octave 2"),
    "layout 2": (dict(layout=2), "layout 2"),
    "layout -1": (dict(layout=-1), "layout -1"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_perlin_texture_refuses_before_any_launch(case):
    """dummy host pointers: a launch would fault on them — the call returns FFX_ERR_ARG first and names the parameter"""
    changes, words = REFUSALS[case]
    lib = _lib.api().lib
    buf = np.zeros(64, np.float32)
    addr = (buf.ctypes.data + 15) & ~15
    args = dict(angles=addr, pos=addr, octaves=3, r0=2, r1=2, persistence=0.5, h=8, w=8, color_a=addr, color_b=addr, layout=1, out=addr, workspace=addr,
                stream=None)
    assert not set(changes) - set(args)
    args.update({k: addr + 4 if v == "misaligned" else v for k, v in changes.items()})
    rc = lib.ffx_perlin_texture(*args.values())
    msg = (lib.ffx_last_error() or b"").decode()
    assert rc == FFX_ERR_ARG, (case, rc, msg)
    assert msg.startswith("perlin_texture: ") and words in msg, (case, msg)


def test_the_wrapper_turns_away_what_it_cannot_draw():
    i = ps.inputs("A-0.5")
    ca, cb = torch.tensor(ps.COLOR_A), torch.tensor(ps.COLOR_B)
    good = dict(angles=i.packed_angles, pos=i.packed_pos, octaves=i.octaves, res=i.res, persistence=i.persistence, shape=i.shape, color_a=ca, color_b=cb)

    def call(**changes):
        return ops.perlin_texture(**dict(good, **changes))

    assert i.packed_angles.numel() == ops.perlin_angle_count(i.res, i.octaves) == 9 + 25 + 81 + 289
    with pytest.raises(RuntimeError, match="HIP device"):
        call()
    with pytest.raises(TypeError, match="angles: expected a torch.Tensor"):
        call(angles=i.packed_angles.numpy())
    with pytest.raises(TypeError, match="pos: expected float32"):
        call(pos=i.packed_pos.double())
    with pytest.raises(ValueError, match="layout"):
        call(layout="whc")
    with pytest.raises(ValueError, match="octaves"):
        call(octaves=9)
    with pytest.raises(ValueError, match="angles: expected 115"):
        call(octaves=3)
    with pytest.raises(ValueError, match="pos: expected"):
        call(pos=i.packed_pos[:-1])
    with pytest.raises(ValueError, match="needs at least as many texels"):
        call(shape=(8, 32))
    with pytest.raises(ValueError, match=r"color_b: expected \[3\]"):
        call(color_b=torch.zeros(4))


DRAW_SEEDS = (0, 3, 17, 24)  # (17 and 24 draw a lattice finer than the texture at the fourth octave)


def _states():
    return random.getstate(), torch.get_rng_state()


@pytest.mark.parametrize("seed", DRAW_SEEDS)
def test_the_shared_draws_leave_the_generators_where_the_existing_path_leaves_them(seed):
    """the existing path: the module's perlin_2d_octaves drawing its own angles behind the three `random` draws, as sample_train did before the draws were
    factored out"""
    shape = (256, 128)
    smp = NoiseTextureLerpSampler(color_a=torch.zeros(3), color_b=torch.ones(3), texture_shape=shape, device=torch.device("cpu"))
    outcomes = []
    for how in ("existing", "sampler", "draws"):
        torch.manual_seed(seed)
        random.seed(seed)
        try:
            if how == "existing":
                lattice, octaves, persistence = 2 ** random.randint(1, 6), random.randint(1, 4), random.uniform(0.1, 2.0)
                tex = ntl.blend(ntl.perlin_2d_octaves(shape, (lattice, lattice), octaves, persistence), smp._color_a, smp._color_b, "cpu")
            elif how == "sampler":
                tex = smp.sample()
            else:
                tex = smp._draw()[3]
        except ValueError as e:  # (a lattice finer than the texture: refused at the same octave, behind the same draws)
            tex = str(e)
        outcomes.append((tex, _states()))
    (t0, s0), (t1, s1), (_, s2) = outcomes
    assert isinstance(t0, str) == isinstance(t1, str) and (t0 == t1 if isinstance(t0, str) else torch.equal(t0, t1))
    for s in (s1, s2):
        assert s[0] == s0[0] and torch.equal(s[1], s0[1])


def test_the_seeds_of_the_draw_test_cover_a_refused_lattice_and_an_accepted_one():
    kinds = set()
    for seed in DRAW_SEEDS:
        random.seed(seed)
        lattice, octaves = 2 ** random.randint(1, 6), random.randint(1, 4)
        kinds.add((lattice << (octaves - 1)) > 128)
    assert kinds == {False, True}


def test_the_engines_the_sampler_takes():
    with pytest.raises(ValueError, match="HIP device"):
        NoiseTextureLerpSampler(color_a=torch.zeros(3), color_b=torch.ones(3), texture_shape=(64, 64), device=torch.device("cpu"), engine="device")
    with pytest.raises(ValueError, match="engine must be"):
        NoiseTextureLerpSampler(color_a=torch.zeros(3), color_b=torch.ones(3), texture_shape=(64, 64), device=torch.device("cpu"), engine="hip")
    smp = NoiseTextureLerpSampler(color_a=torch.zeros(3), color_b=torch.ones(3), texture_shape=(64, 64), device=torch.device("cpu"))
    assert smp._engine == "torch"
