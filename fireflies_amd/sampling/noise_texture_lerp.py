"""Perlin-noise base-colour textures — behaviour of fireflies/sampling/noise_texture_lerp.py.

The reference's dataset loop draws one of these per iteration and assigns it to the mucosa's texture-valued base colour
(`mat-Mucosa.brdf_0.base_color.data`, main.py:138-153).  Same draws from the same generators in the same order, so a seeded
script sees the same textures (pinned by tests/golden/g13, captured from the reference): per sample
`random.randint(1, 6)` (lattice 2^i), `random.randint(1, 4)` (octaves), `random.uniform(0.1, 2)` (persistence), then one
`torch.rand(r + 1, r + 1)` of lattice angles per octave from torch's CPU generator.  The lattice (a few hundred KB at most)
is drawn on the host as in the reference; the per-texel arithmetic runs on the sampler's device: as torch expressions
(engine="torch", the default) or in one call into the native library (engine="device": ops.perlin_texture).
"""
import math
import random

import torch

from . import base


def _fade(t):
    return 6 * t**5 - 15 * t**4 + 10 * t**3


def _cell(h, w, r0, r1):
    cell = (h // r0, w // r1)
    if cell[0] < 1 or cell[1] < 1:
        raise ValueError(f"a {r0} x {r1} lattice needs at least as many texels per axis (got {h} x {w})")
    return cell


def cell_positions(n, r):
    """the position of each of n texels inside its cell of an r-cell lattice axis, as torch's CPU float arange rounds it (an input of
    the device engine, not recomputed there)"""
    return (torch.arange(0, r, r / n) % 1)[:n]


def perlin_2d(shape, res, device="cpu", angles=None):
    """one octave of 2-D gradient noise, [shape0, shape1], lattice res0 x res1 cells (rand_perlin_2d, :8-47); angles: the [res0 + 1, res1 + 1] lattice
    angles on the host, where the caller has drawn them already"""
    h, w = int(shape[0]), int(shape[1])
    r0, r1 = int(res[0]), int(res[1])
    cell = _cell(h, w, r0, r1)
    if angles is None:
        angles = 2 * math.pi * torch.rand(r0 + 1, r1 + 1)  # torch's CPU generator, as in the reference
    grad = torch.stack((torch.cos(angles), torch.sin(angles)), dim=-1).to(device)
    # position of every texel inside its lattice cell, and the cell it is in
    fy = cell_positions(h, r0).to(device)
    fx = cell_positions(w, r1).to(device)
    cy = (torch.arange(h, device=device) // cell[0]).clamp_(max=r0 - 1)
    cx = (torch.arange(w, device=device) // cell[1]).clamp_(max=r1 - 1)
    py, px = fy[:, None].expand(h, w), fx[None, :].expand(h, w)

    def corner(dy, dx):  # gradient of the cell's corner (dy, dx) dotted with the offset from that corner
        g = grad[(cy + dy)[:, None], (cx + dx)[None, :]]
        return torch.stack(((py - dy) * g[..., 0], (px - dx) * g[..., 1]), dim=-1).sum(dim=-1)

    ty, tx = _fade(py), _fade(px)
    top = torch.lerp(corner(0, 0), corner(1, 0), ty)
    bottom = torch.lerp(corner(0, 1), corner(1, 1), ty)
    return math.sqrt(2) * torch.lerp(top, bottom, tx)


def perlin_2d_octaves(shape, res, octaves=1, persistence=0.5, device="cpu", angles=None):
    """angles: one host tensor of lattice angles per octave, where the caller has drawn them already"""
    noise = torch.zeros(tuple(int(v) for v in shape), device=device)
    frequency, amplitude = 1, 1
    for o in range(octaves):
        noise += amplitude * perlin_2d(shape, (frequency * res[0], frequency * res[1]), device=device, angles=None if angles is None else angles[o])
        frequency *= 2
        amplitude *= persistence
    return noise


def position_tables(shape, res, octaves):
    """per octave the shape0 row positions then the shape1 column positions (cell_positions), packed in one host tensor: the `pos` argument of
    ops.perlin_texture"""
    h, w = int(shape[0]), int(shape[1])
    return torch.cat([t for o in range(int(octaves)) for t in (cell_positions(h, int(res[0]) << o), cell_positions(w, int(res[1]) << o))])


def blend(noise, color_a, color_b, device):
    """[3, H, W]: color_a .. color_b blended by the noise plane normalised to 0..1 (:86-98)"""
    t = (noise - noise.min()) / (noise.max() - noise.min())
    a = color_a.to(device).reshape(3, 1, 1).expand(3, *t.shape)
    b = color_b.to(device).reshape(3, 1, 1).expand(3, *t.shape)
    return torch.lerp(a, b, t.unsqueeze(0).expand(3, *t.shape))


class NoiseTextureLerpSampler(base.Sampler):
    """sample() -> [3, H, W]: colour_a .. colour_b blended by normalised multi-octave Perlin noise (:63-102).  engine="torch" (default) builds the
    texture out of torch expressions on the sampler's device; engine="device" draws the same lattices from the same generators and builds it in one
    call into the native library (ops.perlin_texture) on a HIP device: [H, W, 3] storage — the renderer's layout — handed out as its [3, H, W] view,
    so `sample().moveaxis(0, -1)` is contiguous and reaches a texture parameter without a copy."""

    def __init__(self, color_a, color_b, texture_shape, eval_step_size: float = 0.01, device=torch.device("cuda"), engine: str = "torch") -> None:
        super().__init__(torch.tensor([0.0], device=device), torch.tensor([1.0], device=device), eval_step_size, device)
        if engine not in ("torch", "device"):
            raise ValueError("engine must be 'torch' or 'device'")
        if engine == "device" and torch.device(device).type != "cuda":
            raise ValueError(f"engine='device' needs a HIP device (got {device})")
        self._color_a, self._color_b = color_a, color_b
        self._texture_shape = texture_shape
        self._engine = engine
        self._positions = {}  # (h, w, lattice, octaves) -> the packed position tables on the device (they do not depend on the draws)

    def _draw(self, pinned=False):
        """the draws of one texture, in the reference's order -> (lattice, octaves, persistence, the octaves' angles packed in one host tensor, its
        per-octave [R + 1, R + 1] views)"""
        lattice = 2 ** random.randint(1, 6)
        octaves = random.randint(1, 4)
        persistence = random.uniform(0.1, 2.0)
        h, w = int(self._texture_shape[0]), int(self._texture_shape[1])
        sides = [(lattice << o) + 1 for o in range(octaves)]
        packed = torch.empty(sum(n * n for n in sides), pin_memory=pinned)
        views, at = [], 0
        for n in sides:
            _cell(h, w, n - 1, n - 1)  # (refused before the octave's draw, as perlin_2d refuses it)
            v = packed[at:at + n * n].view(n, n)
            torch.rand(n, n, out=v)  # torch's CPU generator, as in the reference
            v.mul_(2 * math.pi)
            views.append(v)
            at += n * n
        return lattice, octaves, persistence, packed, views

    def _position_tables(self, h, w, lattice, octaves):
        key = (h, w, lattice, octaves)
        if key not in self._positions:
            self._positions[key] = position_tables((h, w), (lattice, lattice), octaves).to(self._device)
        return self._positions[key]

    def sample_train(self):
        if self._engine == "device":
            from .. import ops

            lattice, octaves, persistence, packed, _ = self._draw(pinned=True)
            h, w = int(self._texture_shape[0]), int(self._texture_shape[1])
            color = [c.to(self._device, torch.float32).reshape(3).contiguous() for c in (self._color_a, self._color_b)]
            tex = ops.perlin_texture(packed.to(self._device, non_blocking=True), self._position_tables(h, w, lattice, octaves), octaves, (lattice, lattice),
                                     persistence, (h, w), color[0], color[1], layout="hwc")
            return tex.permute(2, 0, 1)
        lattice, octaves, persistence, _, angles = self._draw()
        t = perlin_2d_octaves(self._texture_shape, (lattice, lattice), octaves, persistence, device=self._device, angles=angles)
        return blend(t, self._color_a, self._color_b, self._device)

    def sample_eval(self):  # (the reference draws a random texture in eval mode too, :100-102)
        return self.sample_train()

    def sample(self):
        return self.sample_train()
