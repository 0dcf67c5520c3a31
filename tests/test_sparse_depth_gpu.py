"""The sparse-depth route on the device: the fused forward against the host product of the dense layers (bit for bit) and
the goldens, the dense and fused adjoints against the reference's float64 autograd (golden g15) and tests/ref_sparse_depth.py, the ray
adjoint against the plane formula and central differences of the forward, and the chain laser rays -> hits -> camera -> pyramid -> L1.
Every test prints its figures before it asserts.  Run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import fireflies_amd as ff
from fireflies_amd import _lib, mi, ops
from fireflies_amd import functional as Fn
from fireflies_amd.graphics import depth as gdepth
from fireflies_amd.graphics import rasterization as R
from tests import ref_sparse_depth as ref
from tests import sparse_depth_cases as sc
from tests.conftest import load_golden
from tests.gpu_support import dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0**-24
SIGMA = sc.SIGMA
# What the kernels' binary32 terms may miss the float64 reference by, relative to the sum of the ABSOLUTE values of the terms of each output
# (ref_sparse_depth's `magnitudes`): a term is a product of about eight rounded operations and an expf (2 ulp) whose argument carries two
# roundings amplified by q^2 e <= 1 / e; a factor of the fused product adds three roundings per neighbour (at most three neighbours where this
# bound is used).  64 roundings cover them; the sums themselves are binary64.
TERM_TOL = 64 * EPS32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host_softor(layers):
    """1 - prod (1 - layer) in ascending order, every operation rounded to binary32"""
    acc = np.ones(layers.shape[1:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(layers.shape[0]):
            acc = acc * (np.float32(1.0) - layers[k])
        return np.float32(1.0) - acc


def _rand_pts(n, seed, lo=-0.05, hi=1.05):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 2)) * (hi - lo) + lo).astype(np.float32), rng.random(n).astype(np.float32)


# ------------------------------------------------------------------------------------------ forwards
@pytest.mark.parametrize("n,s0,s1", [(0, 8, 16), (1, 8, 16), (64, 8, 16), (64, 33, 47), (5, 1, 1), (1, 1, 1), (64, 64, 48), (513, 16, 16)])
def test_the_fused_forward_is_the_host_product_of_the_dense_layers_bit_for_bit(n, s0, s1):
    pts, z = _rand_pts(n, 100 + n + s0)
    got = host(ops.splat_depth_softor_fwd(dev(pts).reshape(n, 2), dev(z), SIGMA, s0, s1))
    assert got.shape == (s1, s0)
    if n == 0:
        assert not got.any()
        return
    layers = host(ops.splat_depth_fwd(dev(pts), dev(z), SIGMA, s0, s1))
    want = _host_softor(layers)
    print(f"n {n} {s0}x{s1}: max |fused - host product| {np.abs(got - want).max():.3e}, plane max {want.max():.4f}")
    assert np.isfinite(want).all() and np.array_equal(_bits(got), _bits(want))
    np.testing.assert_allclose(got, ref.fused_forward(pts, z, SIGMA, s0, s1), rtol=1e-5, atol=2e-6)


def test_a_point_whose_layer_maximum_underflows_makes_the_plane_nan_where_the_layers_do():
    pts, z = _rand_pts(12, 5)
    pts[7] = (-3.0, 0.4)  # 48 texels left of a 16-texel texture: e underflows at the nearest texel, m = 0
    layers = host(ops.splat_depth_fwd(dev(pts), dev(z), SIGMA, 16, 16))
    assert np.isnan(layers[7]).all() and np.isfinite(np.delete(layers, 7, axis=0)).all()
    want = _host_softor(layers)
    got = host(ops.splat_depth_softor_fwd(dev(pts), dev(z), SIGMA, 16, 16))
    assert np.isnan(want).all() and np.array_equal(np.isnan(got), np.isnan(want))


def test_the_fused_forward_meets_the_goldens():
    g5 = load_golden("g5_depth_lines.npz")
    p3 = g5["depth_pts"].astype(np.float32)
    for i in range(3):
        got = host(ops.splat_depth_softor_fwd(dev(p3[:, 0:2]), dev(p3[:, 2]), 6.0, 32 // 2**i, 32 // 2**i))
        np.testing.assert_allclose(got[None], g5[f"subsampled_{i}"], rtol=1e-5, atol=2e-6)
    g, blocks = sc.g15_blocks()
    worst = 0.0
    for case, lv, pts, z, l0, l1 in blocks:
        got = host(ops.splat_depth_softor_fwd(dev(pts), dev(z), float(g["sigma"]), l0, l1))
        want = g[f"{case}_l{lv}_fused"]
        worst = max(worst, float(np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
    print(f"fused forward against g15's float64 planes: worst |difference| {worst:.3e}")


def test_rasterize_depth_under_autograd_is_the_no_grad_kernel_and_the_pyramid_keeps_its_shapes():
    g5 = load_golden("g5_depth_lines.npz")
    p3 = dev(g5["depth_pts"]).requires_grad_(True)
    size = torch.tensor(g5["depth_size"])
    out = R.rasterize_depth(p3[:, 0:2], p3[:, 2:3], 6.0, size)
    with torch.no_grad():
        out2 = R.rasterize_depth(p3[:, 0:2], p3[:, 2:3], 6.0, size)
    assert out.requires_grad and torch.equal(out, out2)
    sub = R.subsampled_point_raster(p3, 3, 6.0, torch.tensor([33, 47]))
    assert [tuple(s.shape) for s in sub] == [(1, 47, 33), (1, 23, 16), (1, 11, 8)] and all(s.requires_grad for s in sub)
    with pytest.raises(ValueError, match="level 2"):
        R.subsampled_point_raster(p3, 3, 6.0, torch.tensor([33, 3]))


# ------------------------------------------------------------------------------------------ adjoints against the reference's autograd
def test_the_adjoints_meet_the_float64_autograd_of_g15_within_four_times_its_float32_deviation():
    """Bound per block (case, level, path, gpts / gdepth): 4 x the deviation of the reference's float32 autograd from its float64 autograd on
    that block, relative to the block's largest magnitude; both stored in golden g15."""
    g, blocks = sc.g15_blocks()
    sigma = float(g["sigma"])
    figures = []
    for case, lv, pts, z, l0, l1 in blocks:
        k = f"{case}_l{lv}_"
        p, d = dev(pts), dev(z)
        dense = ops.splat_depth_bwd(p, d, sigma, l0, l1, dev(g[k + "w8_dense"].astype(np.float32) / 8.0))
        fused = ops.splat_depth_softor_bwd(p, d, sigma, l0, l1, dev(g[k + "w8_fused"].astype(np.float32) / 8.0))
        for path, got in (("dense", dense), ("fused", fused)):
            for what, a in zip(("gpts", "gz"), got):
                key = k + f"{path}_{what}"
                bound, scale = sc.g15_bound(g, key)
                err = float(np.abs(host(a).astype(np.float64) - g[key + "_f64"]).max())
                figures.append((err / bound if bound > 0 else np.inf, err / scale, bound / scale, key))
    figures.sort(reverse=True)
    for ratio, err, bound, key in figures[:12]:
        print(f"{key}: error {err:.3e} of the block's largest magnitude, bound {bound:.3e} ({ratio:.2f} of it)")
    print(f"worst error of a block relative to its largest magnitude: {max(f[1] for f in figures):.3e}; blocks over their bound: "
          f"{sum(f[0] > 1 for f in figures)} of {len(figures)}")
    assert all(f[0] <= 1.0 for f in figures), figures[0]


def test_the_dense_adjoint_meets_g5_through_rasterize_depth():
    g5 = load_golden("g5_depth_lines.npz")
    p3 = dev(g5["depth_pts"]).requires_grad_(True)
    out = R.rasterize_depth(p3[:, 0:2], p3[:, 2:3], 6.0, torch.tensor(g5["depth_size"]))
    (out * dev(g5["depth_w"])).sum().backward()
    want = g5["depth_gpts"]
    print(f"g5 depth_gpts: max |difference| {np.abs(host(p3.grad) - want).max():.3e} of {np.abs(want).max():.3e}")
    np.testing.assert_allclose(host(p3.grad), want, rtol=2e-3, atol=1e-4 * np.abs(want).max())


# ------------------------------------------------------------------------------------------ adjoints against ref_sparse_depth
def _edge_cases():
    s0, s1 = 16, 12
    c = lambda j, i: (j / s0, i / s1)  # noqa: E731  (a texel centre)
    return {
        "z_one_on_a_centre_under_a_second_point": ([c(5, 7), ((5 + 1.3) / s0, (7 + 0.4) / s1)], [1.0, 0.5]),
        "z_zero": ([c(4, 4.3), (0.55, 0.5), (0.6, 0.62)], [0.0, 0.7, 0.3]),
        "two_coincident_points": ([(0.41, 0.37), (0.41, 0.37), (0.7, 0.6)], [0.6, 0.6, 0.2]),
        "a_point_outside_the_texture": ([(-0.2, 0.5), (1.12, 1.07), (0.1, 0.45)], [0.8, 0.9, 0.4]),
    }


@pytest.mark.parametrize("name", sorted(_edge_cases()))
def test_the_adjoints_meet_the_float64_reference_on_edge_cases(name):
    s0, s1 = 16, 12
    pts, z = (np.asarray(a, np.float32) for a in _edge_cases()[name])
    n = len(z)
    rng = np.random.default_rng(3)
    gd, gf = rng.standard_normal((n, s1, s0)).astype(np.float32), rng.standard_normal((s1, s0)).astype(np.float32)
    if name.startswith("z_one"):
        gf[7, 5] = 2.0  # weight on the texel where 1 - layer_0 is exactly 0
        assert host(ops.splat_depth_fwd(dev(pts), dev(z), SIGMA, s0, s1))[0, 7, 5] == 1.0
    for path, got, want, mag in (
            ("dense", ops.splat_depth_bwd(dev(pts), dev(z), SIGMA, s0, s1, dev(gd)), ref.dense_adjoint(pts, z, SIGMA, s0, s1, gd),
             ref.dense_adjoint(pts, z, SIGMA, s0, s1, gd, magnitudes=True)),
            ("fused", ops.splat_depth_softor_bwd(dev(pts), dev(z), SIGMA, s0, s1, dev(gf)), ref.fused_adjoint(pts, z, SIGMA, s0, s1, gf),
             ref.fused_adjoint(pts, z, SIGMA, s0, s1, gf, magnitudes=True))):
        for what, a, w, m in zip(("gpts", "gdepth"), got, want, mag):
            a = host(a).astype(np.float64)
            err = np.abs(a - w)
            print(f"{name} {path} {what}: worst error / bound {np.max(err / (TERM_TOL * m + 1e-30)):.3f}, largest |value| {np.abs(w).max():.3e}")
            assert np.isfinite(a).all() and (err <= TERM_TOL * m + 1e-30).all(), (path, what, a, w)
    if name == "two_coincident_points":
        for path_out in (ops.splat_depth_bwd(dev(pts), dev(z), SIGMA, s0, s1, dev(np.stack([gd[0], gd[0], gd[2]]))),):
            assert torch.equal(path_out[0][0], path_out[0][1]) and torch.equal(path_out[1][0], path_out[1][1])


def _raw(name, *args):
    _lib.api().call(name, *[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args], None)
    torch.cuda.synchronize()


def test_zero_gradients_give_zeros_outputs_are_overwritten_and_two_calls_give_the_same_bits():
    pts, z = _rand_pts(40, 11)
    s0, s1 = 33, 47
    p, d = dev(pts), dev(z)
    rng = np.random.default_rng(0)
    for entry, gout in (("ffx_splat_depth_bwd", rng.standard_normal((40, s1, s0))), ("ffx_splat_depth_softor_bwd", rng.standard_normal((s1, s0)))):
        outs = []
        for g in (dev(gout), dev(gout), dev(0 * gout)):
            gp = torch.full((40, 2), float("nan"), device=DEV)
            gz = torch.full((40,), float("nan"), device=DEV)
            _raw(entry, p, d, 40, C.c_float(SIGMA), s0, s1, g, gp, gz)
            outs.append((host(gp), host(gz)))
        assert np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all() and np.abs(outs[0][0]).max() > 0, entry
        assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1])), entry
        assert not outs[2][0].any() and not outs[2][1].any(), entry
    out = torch.full((s1, s0), float("nan"), device=DEV)
    _raw("ffx_splat_depth_softor_fwd", p, d, 40, C.c_float(SIGMA), s0, s1, out)
    assert torch.isfinite(out).all() and torch.equal(out, ops.splat_depth_softor_fwd(p, d, SIGMA, s0, s1))


def test_one_point_more_than_the_neighbour_list_holds_takes_the_plain_loop_to_the_same_result():
    """2049 points on 16 x 16: the adjoint's neighbour list holds 2048, so every workgroup loops over all points instead.  The last point has
    depth 0 — its layer is exactly 0 and its factor exactly 1 —, so the first 2048 gradients must be the list path's on those 2048 points bit for
    bit; its own gradient (gdepth is not 0) is held to the float64 reference."""
    rng = np.random.default_rng(21)
    pts = rng.random((2049, 2)).astype(np.float32)
    z = (rng.random(2049) * 2e-3).astype(np.float32)  # (small depths: the product over 2048 factors stays of order 1)
    z[2048] = 0.0
    gout = rng.standard_normal((16, 16)).astype(np.float32)
    gp_all, gz_all = (host(a) for a in ops.splat_depth_softor_bwd(dev(pts), dev(z), SIGMA, 16, 16, dev(gout)))
    gp_list, gz_list = (host(a) for a in ops.splat_depth_softor_bwd(dev(pts[:2048]), dev(z[:2048]), SIGMA, 16, 16, dev(gout)))
    assert np.abs(gz_list).max() > 0 and np.isfinite(gp_all).all() and np.isfinite(gz_all).all()
    assert np.array_equal(_bits(gp_all[:2048]), _bits(gp_list)) and np.array_equal(_bits(gz_all[:2048]), _bits(gz_list))
    wp, wz = ref.fused_adjoint(pts, z, SIGMA, 16, 16, gout)
    mp, mz = ref.fused_adjoint(pts, z, SIGMA, 16, 16, gout, magnitudes=True)
    # (2048 factors of three roundings each in the product of the last point's weights)
    tol = (64 + 3 * 2048) * EPS32
    print(f"point 2048: gdepth {gz_all[2048]:.6e} (float64 {wz[2048]:.6e}), error / bound {abs(gz_all[2048] - wz[2048]) / (tol * mz[2048]):.3f}")
    assert not gp_all[2048].any() and abs(gz_all[2048] - wz[2048]) <= tol * mz[2048] and abs(wz[2048]) > 0
    assert (np.abs(gz_all - wz) <= tol * mz).all() and (np.abs(gp_all - wp) <= tol * mp).all()
    fwd = host(ops.splat_depth_softor_fwd(dev(pts), dev(z), SIGMA, 16, 16))
    np.testing.assert_allclose(fwd, ref.fused_forward(pts, z, SIGMA, 16, 16), rtol=1e-5, atol=2e-6)


# ------------------------------------------------------------------------------------------ rays
def _geometry(verts, tris):
    gd = ops.DeviceGeometry(verts, tris, np.zeros(len(tris), np.int32), np.zeros(1, np.int32))
    gd.update(np.eye(4, dtype=np.float32)[None], np.zeros(1, np.int32))
    return gd


def _plane_formula_f32(o, d, verts, tris, prim):
    """ref.plane_hit's formula with every operation rounded to binary32 (the inputs are binary32 already) -> (dt_do, dt_dd)"""
    k = np.where(prim >= 0, prim, 0)
    v0, v1, v2 = (verts[tris[k, c]].astype(np.float32) for c in range(3))
    e1, e2 = v1 - v0, v2 - v0
    N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # noqa: E731
    nd = dot(N, d)
    t = dot(N, v0 - o) / nd
    dt_do = -N / nd[:, None]
    hit = (prim >= 0)[:, None]
    return np.where(hit, dt_do, 0).astype(np.float64), np.where(hit, dt_do * t[:, None], 0).astype(np.float64)


@pytest.mark.parametrize("name", ["plane", "tilted", "sphere"])
def test_the_ray_adjoint_is_the_plane_formula_on_the_forwards_hits(name):
    """Bound: 4 x what the plane formula evaluated in binary32 on the same binary32 inputs misses its float64 value by, per block (gorig, gdir),
    relative to the block's largest magnitude."""
    verts, tris = sc.ray_meshes()[name]
    o, d = sc.seeded_rays(name)
    gd = _geometry(verts, tris)
    t, _, prim = gd.trace_rays(dev(o), dev(d))
    prim_h = host(prim).astype(np.int64)
    t_ref, prim_ref = ref.trace(o, d, verts, tris)
    assert (prim_h == prim_ref).mean() >= 0.97 and (prim_h >= 0).sum() >= 60 and (prim_h < 0).sum() >= 4
    gt = np.random.default_rng(1).standard_normal(len(o)).astype(np.float32)
    go, gdir = (host(a).astype(np.float64) for a in gd.trace_rays_bwd(dev(o), dev(d), t, prim, dev(gt)))
    _, dt_do, dt_dd = ref.plane_hit(o, d, verts, tris, prim_h)
    f_do, f_dd = _plane_formula_f32(o, d, verts, tris, prim_h)
    miss = prim_h < 0
    assert not go[miss].any() and not gdir[miss].any()
    for what, got, want, f32 in (("gorig", go, gt[:, None] * dt_do, gt[:, None] * f_do), ("gdir", gdir, gt[:, None] * dt_dd, gt[:, None] * f_dd)):
        scale = np.abs(want).max()
        bound, err = 4.0 * np.abs(f32 - want).max(), np.abs(got - want).max()
        print(f"{name} {what}: error {err / scale:.3e} of the largest magnitude, bound {bound / scale:.3e}")
        assert err <= bound, (name, what)
    e0, e1 = gd.trace_rays_bwd(dev(o[:0]), dev(d[:0]), t[:0], prim[:0], dev(gt[:0]))
    assert tuple(e0.shape) == (0, 3) and tuple(e1.shape) == (0, 3)


def test_a_pose_update_between_forward_and_backward_raises():
    verts, tris = sc.ray_meshes()["tilted"]
    o, d = sc.seeded_rays("tilted", n=32)
    gd = _geometry(verts, tris)
    dd = dev(d).requires_grad_(True)
    t, shape, prim = Fn.trace_rays(gd, dev(o), dd)
    assert t.requires_grad and not shape.requires_grad and not prim.requires_grad
    t.sum().backward(retain_graph=True)
    assert torch.isfinite(dd.grad).all() and float(dd.grad.abs().sum()) > 0
    gd.update(np.eye(4, dtype=np.float32)[None], np.zeros(1, np.int32))
    with pytest.raises(RuntimeError, match="re-fitted"):
        t.sum().backward()


def test_the_ray_adjoint_agrees_with_central_differences_of_the_forward_on_the_sphere():
    verts, tris = sc.ray_meshes()["sphere"]
    o, d = sc.seeded_rays(**sc.CD_RAYS)
    n = len(o)
    gd = _geometry(verts, tris)
    t, _, prim = gd.trace_rays(dev(o), dev(d))
    oo, dd = sc.cd_neighbours(o, d)
    t12, _, p12 = gd.trace_rays(dev(oo.reshape(-1, 3)), dev(dd.reshape(-1, 3)))
    prim_h = host(prim).astype(np.int64)
    cdo, cdd, usable = sc.cd_from_t(o, d, oo, dd, host(t12).reshape(12, n), host(p12).reshape(12, n).astype(np.int64), prim_h)
    go, gdir = (host(a).astype(np.float64) for a in gd.trace_rays_bwd(dev(o), dev(d), t, prim, dev(np.ones(n, np.float32))))
    bo, bd = sc.cd_bound(o, d, verts, tris, prim_h, host(t).astype(np.float64))
    eo, ed = np.abs(go - cdo)[usable], np.abs(gdir - cdd)[usable]
    print(f"central differences: {usable.sum()} of {n} rays usable; worst error / bound: origins {np.max(eo / bo[usable]):.3f}, directions "
          f"{np.max(ed / bd[usable]):.3f}; largest derivative {np.abs(gdir).max():.3f}")
    assert usable.mean() >= 0.95
    assert (eo <= bo[usable]).all() and (ed <= bd[usable]).all()


# ------------------------------------------------------------------------------------------ end to end
def _e2e():
    data = sc.two_planes()
    ms = mi.load_scene_data(data)
    ms.geom.update(ms._xforms, ms._offs)
    verts, tris = sc.world_mesh(data)
    M = sc.world_to_sample(data.camera)
    targets = sc.e2e_targets(verts, tris, M)
    tr = ff.entity.Transformable("laser", DEV)
    laser = ff.projection.Laser(tr, dev(sc.pattern(sc.E2E_OFFSET)), torch.from_numpy(sc.laser_K()), sc.LASER_FOV, sc.LASER_NEAR, sc.LASER_FAR, device=DEV)
    return ms, laser, verts, tris, M, targets


def _pyramid_loss(ms, laser, targets, detach_t=False):
    if detach_t:  # the hit as the parent formed it: o + t d with t a constant
        o, d = laser.originPerRay().contiguous().float(), laser.rays().contiguous().float()
        t, _, _ = ms.geom.trace_rays(o.detach(), d.detach())
        pts = Fn.project_rays(o + t.unsqueeze(-1) * d, gdepth._world_to_sample(ms))
    else:
        pts, valid = gdepth.laser_points_in_camera(ms, laser=laser)
        assert bool(valid.all())
    levels = R.subsampled_point_raster(pts, sc.E2E_LEVELS, SIGMA, torch.tensor([sc.E2E_SENSOR, sc.E2E_SENSOR]))
    return sum(torch.nn.functional.l1_loss(lv[0], dev(tg)) for lv, tg in zip(levels, targets)), pts


# The chain's gradient against its float64 restatement, relative to the gradient's largest magnitude: binary32 roundings (6e-8) amplified by the
# cancellation of the pyramid's sums (sum of |terms| over |sum|: below 100 here) and by 1 / cos at the hits (below 2) stay under 2e-5; the
# L1 loss adds the texels whose difference changes sign within the forward's rounding (each moves the gradient by 2 / texels of its weight).
# 1e-3 leaves room for a handful of them and is still a hundredth of the term the parent's gradient lacks.
E2E_TOL = 1e-3


def test_the_pyramid_loss_gradient_reaches_the_laser_rays_complete():
    ms, laser, verts, tris, M, targets = _e2e()
    rays = host(laser._rays)
    loss_ref, g_ref, pts_ref, _ = sc.e2e_loss_grad(rays, targets, verts, tris, M)
    _, g_const, _, _ = sc.e2e_loss_grad(rays, targets, verts, tris, M, plane_term=False)
    laser._rays.requires_grad_(True)
    loss, pts = _pyramid_loss(ms, laser, targets)
    loss.backward()
    g = host(laser._rays.grad).astype(np.float64)
    scale = np.abs(g_ref).max()
    print(f"loss {float(loss.detach()):.6f} (float64 {loss_ref:.6f}); gradient error {np.abs(g - g_ref).max() / scale:.3e} of its largest magnitude (bound {E2E_TOL:.0e}); "
          f"the t term is {np.abs(g_const - g_ref).max() / scale:.3e} of it")
    np.testing.assert_allclose(host(pts), pts_ref, rtol=0, atol=2e-5)
    assert abs(float(loss.detach()) - loss_ref) <= 1e-5 * loss_ref
    assert np.abs(g - g_ref).max() <= E2E_TOL * scale
    # the parent's cast_laser (t a constant) gives the gradient WITHOUT the closed-form t term, and misses the bound by it
    laser._rays.grad = None
    loss_p, _ = _pyramid_loss(ms, laser, targets, detach_t=True)
    loss_p.backward()
    gp = host(laser._rays.grad).astype(np.float64)
    assert np.abs(gp - g_const).max() <= E2E_TOL * scale
    assert np.abs(gp - g_ref).max() > 20 * E2E_TOL * scale
    # a ray that hits nothing is invalid, and so is a hit outside the film
    o = dev(np.zeros((2, 3), np.float32))
    d = dev(np.array([[0.0, 0.0, -1.0], [-0.64, 0.0, 0.768]], np.float32))  # away from the planes; onto the left plane at x = -2.5, beside the film
    _, valid = gdepth.laser_points_in_camera(ms, origin=o, direction=d)
    assert valid.tolist() == [False, False]


FIT_STEPS, FIT_RATIO = 40, 0.04  # tests/test_sparse_depth_cpu.py: the float64 loop is under 4 % of its first loss within 40 steps


def test_the_examples_fit_recovers_the_displaced_pattern():
    """Adam on laser._rays through laser_points_in_camera -> subsampled_point_raster -> L1, clamp_to_fov and normalize_rays after each step: within
    twice the float64 loop's 40 steps the loss falls under the 4 % of its start that loop reaches."""
    ms, laser, verts, tris, M, targets = _e2e()
    laser._rays.requires_grad_(True)
    opt = torch.optim.Adam([laser._rays], lr=sc.E2E_LR)
    losses = []
    for _ in range(2 * FIT_STEPS):
        opt.zero_grad()
        loss, _ = _pyramid_loss(ms, laser, targets)
        loss.backward()
        losses.append(loss.detach())
        opt.step()
        laser.clamp_to_fov()
        laser.normalize_rays()
    with torch.no_grad():
        losses.append(_pyramid_loss(ms, laser, targets)[0])
    losses = torch.stack(losses).cpu().numpy()
    print(f"fit: loss {losses[0]:.5f} -> {losses[FIT_STEPS]:.5f} after {FIT_STEPS} steps, best {losses.min():.5f} ({losses.min() / losses[0]:.4f} of the start)")
    assert losses.min() <= FIT_RATIO * losses[0]
    err = np.abs(host(laser._rays) - sc.pattern()).max()
    assert err < 0.5 * np.abs(sc.pattern(sc.E2E_OFFSET) - sc.pattern()).max(), err
