"""What the Perlin-texture suites with and without a GPU share: the inputs of a case of tests/ref_perlin.py (seeded lattice angles as the sampler draws
them, the position tables as torch's CPU arange rounds them), the float64 reference on them, and the repository's float32 torch path on the CPU with
its deviation from that reference — each computed once per (case, seed).  torch on the CPU, numpy and the package's host-side modules only."""
import functools
import math
import random
from collections import namedtuple

import numpy as np
import torch

from fireflies_amd.sampling import noise_texture_lerp as ntl
from tests import ref_perlin

COLOR_A, COLOR_B = (0.125, 0.75, 0.3), (0.9, 0.2, 0.65)
Inputs = namedtuple("Inputs", "shape res octaves persistence angles pos packed_angles packed_pos")
G13_TAGS = "abc"


def case_args(name):
    return ref_perlin.DEGENERATE if name == "F'" else ref_perlin.CASES[name]


@functools.lru_cache(maxsize=None)
def inputs(name, seed=0):
    """angles: one [R0 + 1, R1 + 1] float32 array per octave (2 pi torch.rand from a generator of that seed); pos: (fy, fx) per octave; packed_*: the
    flat host tensors that ops.perlin_texture takes"""
    shape, res, octaves, persistence = case_args(name)
    g = torch.Generator().manual_seed(seed)
    angles = [2 * math.pi * torch.rand(r0 + 1, r1 + 1, generator=g) for r0, r1 in ref_perlin.lattices(res, octaves)]
    packed_pos = ntl.position_tables(shape, res, octaves)
    h, w = shape
    pos = [(packed_pos[o * (h + w): o * (h + w) + h].numpy(), packed_pos[o * (h + w) + h: (o + 1) * (h + w)].numpy()) for o in range(octaves)]
    return Inputs(shape, res, octaves, persistence, [a.numpy() for a in angles], pos, torch.cat([a.reshape(-1) for a in angles]), packed_pos)


@functools.lru_cache(maxsize=None)
def reference(name, seed=0, colors=(COLOR_A, COLOR_B)):
    """[3, h, w] float64 (read-only)"""
    i = inputs(name, seed)
    out = ref_perlin.texture(i.angles, i.pos, i.shape, i.res, i.octaves, i.persistence, *colors)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def magnitude(name, seed=0):
    """how far a texel's float32 intermediates can exceed what the normalisation divides by: 2 sqrt(2) sum a_o (a corner value is within |py| + |px| <= 2,
    an octave within sqrt(2) times that) over the float64 plane's max - min, at least one"""
    i = inputs(name, seed)
    plane = ref_perlin.noise(i.angles, i.pos, i.shape, i.res, i.octaves, i.persistence)
    amplitudes = sum(float(np.float32(i.persistence**o)) for o in range(i.octaves))
    return max(1.0, 2.0 * math.sqrt(2.0) * amplitudes / float(plane.max() - plane.min()))


@functools.lru_cache(maxsize=None)
def torch_path(name, seed=0, colors=(COLOR_A, COLOR_B)):
    """[3, h, w] float32: the sampler's torch engine on the CPU under the case's angles (read-only)"""
    i = inputs(name, seed)
    plane = ntl.perlin_2d_octaves(i.shape, i.res, i.octaves, i.persistence, device="cpu", angles=[torch.from_numpy(a) for a in i.angles])
    out = ntl.blend(plane, torch.tensor(colors[0]), torch.tensor(colors[1]), "cpu").numpy().copy()
    out.setflags(write=False)
    return out


def torch_deviation(name, seed=0, colors=(COLOR_A, COLOR_B)):
    """the float32 torch CPU path's largest deviation from the float64 reference on the case: the yardstick of the device's bound"""
    return float(np.abs(torch_path(name, seed, colors).astype(np.float64) - reference(name, seed, colors)).max())


def g13_replay(g, tag, make_sampler):
    """the draws of the golden g13's part `tag` (seeds, two colours, two textures) -> per texture (the sampler's draws as ref_perlin takes them, the
    colours); make_sampler(color_a, color_b, shape) builds the sampler whose _draw() is replayed"""
    seed, shape = int(g[f"{tag}_seed"]), tuple(int(v) for v in g[f"{tag}_shape"])
    torch.manual_seed(seed)
    random.seed(seed)
    ca, cb = torch.rand(3), torch.rand(3)
    smp = make_sampler(ca, cb, shape)
    out = []
    for _ in range(2):
        lattice, octaves, persistence, _, views = smp._draw()
        packed_pos = ntl.position_tables(shape, (lattice, lattice), octaves)
        h, w = shape
        pos = [(packed_pos[o * (h + w): o * (h + w) + h].numpy(), packed_pos[o * (h + w) + h: (o + 1) * (h + w)].numpy()) for o in range(octaves)]
        out.append(((([v.numpy().copy() for v in views]), pos, shape, (lattice, lattice), octaves, persistence), (ca.numpy(), cb.numpy())))
    return out
