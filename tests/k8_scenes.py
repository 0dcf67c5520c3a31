"""The small plain scene of the packet render kernel's tests and what they do to its camera and projector texture: the vocal fold of
tests/test_k8_plain_gpu.py (two shapes, 8 x 8 fold lips in an 8 x 16 tube, a 4 x 4 laser) on a film of any size, and copies of its scene
description with another field of view, another sample-to-camera matrix or another texture size."""
import ctypes as C
import random

import numpy as np
import torch

DEV = "cuda"


def workload(width=64, height=48, tex=64):
    from fireflies_amd import workloads

    wl = workloads.vocalfold(device=DEV, width=width, height=height, tex=tex, grid=4, frames=4, n_fold=8, tube=(8, 16), entity_device="cpu")
    t = workloads.build_texture(wl).detach().contiguous()
    wl.params["tex.data"] = t
    return wl, t


def pose(wl, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    wl.ff_scene.randomize()


def sd_copy(sd):
    """an unfrozen copy of a scene description (the render calls derive its pre-pass key from its bytes)"""
    from fireflies_amd import _abi

    out = _abi.SceneDesc()
    C.memmove(C.addressof(out), C.addressof(sd), C.sizeof(sd))
    return out


def camera_to_sample(sd, fov_deg):
    """the perspective camera-to-sample matrix of the description's film at another horizontal field of view (float64 4 x 4)"""
    from fireflies_amd import mi

    w, h = sd.cam.width, sd.cam.height
    return mi.perspective_projection((w, h), (w, h), (0, 0), fov_deg, sd.cam.near_clip, sd.cam.far_clip).numpy().astype(np.float64)


def with_camera(sd, K):
    """a copy of `sd` whose camera_to_sample is K"""
    from fireflies_amd import scene_desc

    out = sd_copy(sd)
    out.cam.camera_to_sample = scene_desc._m16(np.asarray(K, np.float32))
    return out


def scaled_s2c(K, log2_scale):
    """K such that rows 0..2 of its inverse (sample -> camera: what the kernels' q = s2c (sx, sy, 0, 1) reads) are those of K's inverse times
    2^log2_scale, row 3 (the homogeneous w) unchanged: the near-plane point np = q / w grows by that factor, the ray direction stays"""
    return np.asarray(K, np.float64) @ np.diag([2.0 ** -log2_scale] * 3 + [1.0])


def nonuniform_w(K, a=0.05):
    """K whose inverse has a homogeneous w that varies over the film (s2c[12] != 0): not a perspective sensor's matrix"""
    K2 = np.array(K, np.float64)
    K2[3, 0] += a
    assert np.linalg.inv(K2)[3, 0] != 0.0
    return K2


def with_texture(sd, tw, th):
    """a copy of `sd` whose one-channel projector texture is tw x th, and such a texture [th, tw, 1]: bright everywhere (every probe and gather
    reads non-zero texels, the border's among them), values that differ from texel to texel"""
    out = sd_copy(sd)
    out.proj.tex_w, out.proj.tex_h = int(tw), int(th)
    g = torch.Generator().manual_seed(tw * 1000 + th)
    tex = (0.25 + 0.75 * torch.rand((th, tw, 1), generator=g)).to(DEV).contiguous()
    return out, tex
