"""Pattern optimisation through geometry instead of radiance (the reference ships 10_pattern_creation.py EMPTY; its second route to a
pattern gradient, SURVEY 3.5 `depth.from_laser`): the laser's rays are intersected with the scene, the hits are projected into the
camera and splatted as a sparse depth pyramid, and an L1 loss against the pyramid of a target pattern is driven down by Adam on
`laser._rays` — every step on the device, nothing rendered.

    python examples/10_sparse_depth_pattern.py [steps] [grid]

The start pattern is the target with every ray displaced by the same small offset; the loop walks it back (on the vocal-fold scene the
loss falls by a factor of 20 in 100 steps and the median ray ends 2e-5 from its target).  A ray whose hit sits at the film's border or at a
depth step has no edge term to pull it back (out of scope) and may drift: the median tells the fit, the largest offset those rays."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fireflies_amd import workloads  # noqa: E402
from fireflies_amd.graphics import depth, rasterization  # noqa: E402
from fireflies_amd.utils import math as ffmath  # noqa: E402

LEVELS, SIGMA = 3, 6.0


def emitted_rays(laser):
    """origins and world directions of the pattern as the projector emits it.  The pattern lives in the projector's frame looking down -z
    (Laser.generate_uniform_rays) and its texture position is K FLIP_Y ray: both signs of a ray land on the same texel, and the light leaves
    along the one in front of the projector, -FLIP_Y ray."""
    local = laser._rays * torch.tensor([-1.0, 1.0, -1.0], device=laser._rays.device)
    return laser.originPerRay(), ffmath.transform_directions(local, laser.origin().to(local.device))


def pyramid(scene, laser, sensor_size):
    """the sparse depth pyramid of the laser's hits as the camera sees them, invalid points (misses, hits beside the film) left out"""
    origin, direction = emitted_rays(laser)
    pts, valid = depth.laser_points_in_camera(scene, origin=origin, direction=direction)
    return rasterization.subsampled_point_raster(pts[valid], LEVELS, SIGMA, sensor_size), int(valid.sum())


if __name__ == "__main__":
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    grid = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    wl = workloads.vocalfold(grid=grid)
    scene, laser = wl.mi_scene, wl.laser
    torch.manual_seed(0)
    wl.ff_scene.randomize()  # one pose of the scene; it stays for the whole fit
    w, h = scene.sensors()[0].film().crop_size()
    size = torch.tensor([w, h])
    with torch.no_grad():
        target_rays = laser._rays.clone()
        target, n_valid = pyramid(scene, laser, size)
        laser._rays[:] = target_rays + torch.tensor([0.004, -0.0025, 0.0], device=target_rays.device)
        laser.normalize_rays()
    print(f"{laser._rays.shape[0]} rays, {n_valid} of them seen by the {w} x {h} camera; {LEVELS} levels, sigma {SIGMA}")
    laser._rays.requires_grad_(True)
    opt = torch.optim.Adam([laser._rays], lr=2e-4)
    for i in range(steps):
        opt.zero_grad()
        levels, _ = pyramid(scene, laser, size)
        loss = sum(torch.nn.functional.l1_loss(a, b) for a, b in zip(levels, target))
        loss.backward()
        opt.step()
        laser.clamp_to_fov()
        laser.normalize_rays()
        if i % 10 == 0 or i == steps - 1:
            off = (laser._rays.detach() - target_rays).norm(dim=1)
            print(f"step {i:4d}  loss {float(loss.detach()):.6f}  ray offset from the target: median {float(off.median()):.5f}, largest {float(off.max()):.5f}")
