"""The path integrator without a GPU: its float64 restatement (tests/ref_path.py) against a quadrature of the one-bounce
radiance, and the argument checks of the Python layers and the ABI."""
import re

import numpy as np
import pytest

from fireflies_amd import _abi, ops, scene_desc
from tests import ref_bruteforce as bf
from tests import ref_path as rp
from tests.corner_scenes import relay
from tests.support import define, header, world_arrays



def test_path_estimator_matches_a_quadrature_of_the_one_bounce_radiance():
    sc = relay(False, True, 8, 8, projector_scale=1.0)  # (the spot alone)
    verts, gidx, shape, alb = world_arrays(sc)
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    spp, seed = 1024, 3
    # direct light only: the wall is dark
    assert np.abs(rp.sample_radiance(verts, gidx, shape, sd, alb, None, 4, seed, 2)).max() == 0.0
    L = rp.sample_radiance(verts, gidx, shape, sd, alb, None, spp, seed, 3)[:, 0]
    mc, sigma = L.mean(), L.std() / np.sqrt(len(L))
    assert sigma < 0.03 * mc
    # the same samples' hit points on the wall; L_wall(x) = rho_w / pi * int_floor L_floor(y) cos_x cos_y / r^2 dA,
    # L_floor(y) = rho_f / pi * I * falloff * cos_s / d^2 (midpoint rule over the floor around the spot's cone)
    o, d, nt, ft = bf.camera_rays(sd.cam, spp, True, seed)
    sub = np.random.default_rng(0).choice(len(d), 1024, replace=False)
    t, prim = bf.intersect(o[sub], d[sub], bf.world_triangles(verts, gidx), nt[sub], ft[sub])
    assert (shape[prim] == 0).all()
    X = o[sub] + t[:, None] * d[sub]
    n_g = 200
    g = (np.arange(n_g) + 0.5) / n_g * 1.2 - 0.6
    Y = np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(-1, 2)
    Y = np.concatenate([Y, np.zeros((len(Y), 1))], 1)
    dA = (1.2 / n_g) ** 2
    spos = np.array([0.0, 0.0, 1.5])
    ws = spos - Y
    d2 = (ws * ws).sum(1)
    ang = np.arccos(np.clip(ws[:, 2] / np.sqrt(d2), -1, 1))
    cut, beam = np.deg2rad(20.0), np.deg2rad(15.0)
    fall = np.where(ang <= beam, 1.0, np.where(ang < cut, (cut - ang) / (cut - beam), 0.0))
    L_floor = 0.5 / np.pi * 10.0 * fall * (ws[:, 2] / np.sqrt(d2)) / d2
    r = Y[None] - X[:, None]
    r2 = (r * r).sum(-1)
    cos_x, cos_y = r[..., 0] / np.sqrt(r2), -r[..., 2] / np.sqrt(r2)
    L_wall = 0.8 / np.pi * (L_floor[None] * cos_x * cos_y / r2).sum(1) * dA
    quad = L_wall.mean()
    assert abs(mc - quad) <= 4.0 * sigma + 5e-3 * quad, (mc, quad, sigma)
    # the estimator's arithmetic, not luck: a missing pi or cosine is many sigma away
    assert abs(mc / np.pi - quad) > 8.0 * sigma and abs(mc * np.pi - quad) > 8.0 * sigma


def test_random_numbers_are_independent_of_the_jitter_stream():
    idx = np.arange(1 << 14, dtype=np.uint64)
    jx, jy = bf.jitter(7, idx)
    u0, u1 = rp.path_u(rp.path_key(7), idx, 1, 0), rp.path_u(rp.path_key(7), idx, 1, 1)
    for a in (jx, jy):
        for b in (u0, u1):
            assert abs(np.corrcoef(a, b)[0, 1]) < 0.05
    assert 0.0 <= u0.min() and u0.max() < 1.0 and abs(u0.mean() - 0.5) < 0.01
    assert not np.array_equal(u0, rp.path_u(rp.path_key(7), idx, 2, 0))


def test_depth_arguments_are_checked():
    assert ops.path_flags(2) == 0
    assert ops.path_flags(3, 5) == (3 << 8) | (5 << 12)
    assert ops.path_flags(8, 100) == (8 << 8) | (15 << 12)
    for bad in (-1, 0, 1, 9, 2.5, True):
        with pytest.raises(ValueError):
            ops.path_flags(bad)
    with pytest.raises(ValueError):
        ops.path_flags(3, 0)


def test_load_dict_returns_integrators():
    from fireflies_amd import mi

    it = mi.load_dict({"type": "path", "max_depth": 4, "rr_depth": 3})
    assert (it.type, it.max_depth, it.rr_depth) == ("path", 4, 3)
    assert mi.load_dict({"type": "path", "max_depth": 3}).rr_depth == 5
    assert mi.load_dict({"type": "direct"}).max_depth == 2
    for bad in ({"type": "path"}, {"type": "path", "max_depth": -1}, {"type": "path", "max_depth": 9}, {"type": "path", "max_depth": 3, "hide_emitters": True}):
        with pytest.raises(ValueError):
            mi.load_dict(bad)
    with pytest.raises(NotImplementedError):
        mi.load_dict({"type": "volpath", "max_depth": 3})


def test_path_macros_in_header_and_abi():
    hdr = header()
    assert define("FFX_ABI_VERSION") == _abi.FFX_ABI_VERSION == 11
    for name, val in (("MAX_DEPTH_SHIFT", _abi.RENDER_MAX_DEPTH_SHIFT), ("RR_DEPTH_SHIFT", _abi.RENDER_RR_DEPTH_SHIFT), ("MAX_DEPTH_LIMIT", _abi.RENDER_MAX_DEPTH_LIMIT)):
        assert int(re.search(rf"#define FFX_RENDER_{name} (\d+)", hdr).group(1)) == val
    assert int(re.search(r"#define FFX_RENDER_PATH_MASK (0x[0-9a-fA-F]+)", hdr).group(1), 16) == _abi.RENDER_PATH_MASK
    assert "#define FFX_RENDER_PATH(max_depth, rr_depth)" in hdr
    # the path bits stay clear of the other flags of the render calls
    assert _abi.RENDER_PATH_MASK & (_abi.RENDER_FP16 | _abi.RENDER_SPARSE_ADJOINT | _abi.RENDER_APEX_READY | _abi.RENDER_CACHE_ZEROED | _abi.RENDER_CACHE_KEEP_DROPPED) == 0
