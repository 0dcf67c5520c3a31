"""The sparse-depth route without a device: the four entry points' prototypes and refusals, the float64 reference
(tests/ref_sparse_depth.py) against the reference's own autograd (golden g15) and against closed forms, the ops wrappers' refusal of host
tensors, and the seeded cases of the GPU suite (rays that central differences can use, the fit the example's loop must repeat).
Run with `-m "not gpu"`."""
import ctypes as C

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, _lib, ops
from tests import ref_sparse_depth as ref
from tests import sparse_depth_cases as sc
from tests.support import enum_value

ERR_ARG = enum_value("FFX_ERR_ARG")

ENTRIES = ("ffx_splat_depth_bwd", "ffx_splat_depth_softor_fwd", "ffx_splat_depth_softor_bwd", "ffx_trace_rays_bwd")
# the parameters of the four entry points in the order and under the names of include/ffx_labels.h
PARAMS = {
    "ffx_splat_depth_bwd": "pts depth n sigma size0 size1 gout gpts gdepth stream",
    "ffx_splat_depth_softor_fwd": "pts depth n sigma size0 size1 out stream",
    "ffx_splat_depth_softor_bwd": "pts depth n sigma size0 size1 gout gpts gdepth stream",
    "ffx_trace_rays_bwd": "bvh info origins dirs n t prim gt gorig gdir stream",
}


def test_the_python_table_binds_the_four_entries_as_declared():
    api = _lib.api()
    for name in ENTRIES:
        res, args = _abi.PROTOTYPES_NO_ORACLE[name]
        fn = getattr(api.lib, name)
        assert fn.restype == res and fn.argtypes == args and len(args) == len(PARAMS[name].split()), name


def _call(name, **changes):
    """`name` with every pointer at a dummy host buffer the library never dereferences (a refusal comes before any launch) -> (rc, message)"""
    lib = _lib.api().lib
    buf = np.zeros(64, np.float32)
    addr = (buf.ctypes.data + 15) & ~15
    info = _abi.BvhInfo(n_tris=1, n_nodes=1, max_depth=1, off_tq=64)
    args = {p: addr for p in PARAMS[name].split()}
    args.update(n=4, sigma=6.0, size0=8, size1=8, stream=None, info=C.byref(info))
    assert not set(changes) - set(args), (name, changes)
    if changes.get("info", 1) is None:
        changes["info"] = None
    args.update(changes)
    rc = getattr(lib, name)(*[args[p] for p in PARAMS[name].split()])
    return rc, (lib.ffx_last_error() or b"").decode()


def _refusals():
    cases = []
    for name in ENTRIES[:3]:
        ptrs = [p for p in PARAMS[name].split() if p not in ("n", "sigma", "size0", "size1", "stream")]
        cases += [(name, {p: None}, p) for p in ptrs]
        cases += [(name, {"n": -1}, "n"), (name, {"size0": 0}, "size0"), (name, {"size1": 0}, "size1"), (name, {"size0": -3}, "size0"),
                  (name, {"sigma": 0.0}, "sigma"), (name, {"sigma": -1.0}, "sigma"), (name, {"sigma": float("nan")}, "sigma")]
    name = ENTRIES[3]
    cases += [(name, {p: None}, p) for p in PARAMS[name].split() if p not in ("n", "stream")]
    cases += [(name, {"n": -1}, "n")]
    return cases


@pytest.mark.parametrize("name,changes,named", _refusals(), ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_refusals_come_before_any_launch_and_name_the_parameter(name, changes, named):
    rc, msg = _call(name, **changes)
    assert rc == ERR_ARG and named in msg and name[4:] in msg, (rc, msg)


def test_a_bvh_info_that_trace_rays_refuses_is_refused():
    lib = _lib.api().lib
    buf = np.zeros(64, np.float32)
    bad = _abi.BvhInfo(n_tris=0, n_nodes=1, max_depth=1)
    a = buf.ctypes.data
    assert lib.ffx_trace_rays_bwd(a, C.byref(bad), a, a, 4, a, a, a, a, a, None) == ERR_ARG
    assert "trace_rays_bwd" in lib.ffx_last_error().decode()


def test_the_ops_wrappers_refuse_host_tensors():
    pts, z = torch.rand(4, 2), torch.rand(4)
    for call in (lambda: ops.splat_depth_bwd(pts, z, 6.0, 8, 8, torch.zeros(4, 8, 8)), lambda: ops.splat_depth_softor_fwd(pts, z, 6.0, 8, 8),
                 lambda: ops.splat_depth_softor_bwd(pts, z, 6.0, 8, 8, torch.zeros(8, 8))):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(ValueError, match="one value per point"):
        ops.splat_depth_softor_fwd(pts, torch.rand(3), 6.0, 8, 8)
    with pytest.raises(ValueError, match=r"\[N,2\]"):
        ops.splat_depth_softor_fwd(torch.rand(4, 3), z, 6.0, 8, 8)


# ------------------------------------------------------------------------------------------ the float64 reference
def test_the_reference_restates_the_reference_autograd_of_g15():
    g, blocks = sc.g15_blocks()
    assert len(blocks) == 24 and sorted({c for c, *_ in blocks}) == sorted(str(c) for c in g["cases"])
    sigma = float(g["sigma"])
    for case, lv, pts, z, l0, l1 in blocks:
        assert ref.tie_distance(pts, l0, l1) >= 2.0**-8
        k = f"{case}_l{lv}_"
        np.testing.assert_allclose(ref.fused_forward(pts, z, sigma, l0, l1), g[k + "fused"], rtol=0, atol=1e-14)
        wd, wf = g[k + "w8_dense"] / 8.0, g[k + "w8_fused"] / 8.0
        np.testing.assert_allclose((ref.layers(pts, z, sigma, l0, l1) * wd).sum(), g[k + "dense_loss"], rtol=1e-12, atol=1e-12)
        for path, got in (("dense", ref.dense_adjoint(pts, z, sigma, l0, l1, wd)), ("fused", ref.fused_adjoint(pts, z, sigma, l0, l1, wf))):
            for what, a in zip(("gpts", "gz"), got):
                want = g[k + f"{path}_{what}_f64"]
                assert np.abs(a - want).max() <= 1e-12 * np.abs(want).max(), (k, path, what)
    k = "c5_24x20_l0_"
    np.testing.assert_allclose(ref.layers(g["c5_24x20_pts"], g["c5_24x20_depth"], sigma, 24, 20), g[k + "dense"], rtol=0, atol=1e-14)


def test_one_point_on_a_texel_centre_in_closed_form():
    s0, s1, sigma, z = 16, 12, 6.0, 0.75
    j0, i0 = 5, 7
    pts = np.array([[j0 / s0, i0 / s1]])
    lay = ref.layers(pts, [z], sigma, s0, s1)[0]
    assert lay[i0, j0] == z  # m = 1: the peak is the depth itself
    dj, di = 2, -1
    e = np.exp(-(((dj * dj + di * di) / sigma) ** 2))
    np.testing.assert_allclose(lay[i0 + di, j0 + dj], z * e, rtol=1e-15)
    # a unit gradient on that one texel: d layer / d p = z e 4 d (x - p) / sigma^2 (the peak's own derivative vanishes on a centre), times the size
    G = np.zeros((1, s1, s0))
    G[0, i0 + di, j0 + dj] = 1.0
    gp, gz = ref.dense_adjoint(pts, [z], sigma, s0, s1, G)
    c = z * e * 4.0 * (dj * dj + di * di) / sigma**2
    np.testing.assert_allclose(gp[0], [c * dj * s0, c * di * s1], rtol=1e-14)
    np.testing.assert_allclose(gz[0], e, rtol=1e-15)
    # with one point the fused plane is its layer and the fused adjoint the dense one
    np.testing.assert_allclose(ref.fused_forward(pts, [z], sigma, s0, s1), lay, rtol=0, atol=1e-16)
    fp, fz = ref.fused_adjoint(pts, [z], sigma, s0, s1, G[0])
    np.testing.assert_allclose(fp, gp, rtol=1e-14)
    np.testing.assert_allclose(fz, gz, rtol=1e-14)
    # z = 1 on a centre under a second point: the other point's weight there is exactly 0, nothing is divided by it
    two = np.array([[j0 / s0, i0 / s1], [(j0 + 1.3) / s0, (i0 + 0.4) / s1]])
    fp2, fz2 = ref.fused_adjoint(two, [1.0, 0.5], sigma, s0, s1, G[0] + np.eye(s1, s0))
    assert np.isfinite(fp2).all() and np.isfinite(fz2).all()


def test_a_ray_on_the_plane_z_equals_c_in_closed_form():
    verts, tris = sc.ray_meshes()["plane"]  # z = 2
    o = np.array([[0.3, -0.2, -1.0], [0.0, 0.5, 0.5]])
    d = np.array([[0.2, 0.1, 1.5], [-0.3, 0.2, 0.6]])
    t, prim = ref.trace(o, d, verts, tris)
    assert (prim >= 0).all()
    np.testing.assert_allclose(t, (2.0 - o[:, 2]) / d[:, 2], rtol=1e-15)
    tp, dt_do, dt_dd = ref.plane_hit(o, d, verts, tris, prim)
    np.testing.assert_allclose(tp, t, rtol=1e-15)
    np.testing.assert_allclose(dt_do, np.stack([0 * t, 0 * t, -1.0 / d[:, 2]], -1), rtol=1e-15, atol=1e-300)
    np.testing.assert_allclose(dt_dd, np.stack([0 * t, 0 * t, -t / d[:, 2]], -1), rtol=1e-15, atol=1e-300)
    _, prim_miss = ref.trace([[0, 0, 5.0]], [[0, 0, 1.0]], verts, tris)
    assert prim_miss[0] == -1 and not ref.plane_hit([[0, 0, 5.0]], [[0, 0, 1.0]], verts, tris, prim_miss)[1].any()
    # the hit stays on the plane: d hit_z / d ray = 0 through hits_vjp, whatever moves
    go, gd = ref.hits_vjp(o, d, tp, dt_do, dt_dd, np.tile([0.0, 0.0, 1.0], (2, 1)))
    assert np.abs(go).max() < 1e-15 and np.abs(gd).max() < 1e-15


def test_projection_and_pyramid_adjoints_agree_with_differences_of_the_reference():
    rng = np.random.default_rng(0)
    M = sc.world_to_sample(sc.two_planes().camera)
    p = rng.random((6, 3)) * [1.0, 1.0, 0.5] + [-0.5, -0.5, 3.0]
    g = rng.standard_normal((6, 3))
    vjp = ref.project_vjp(p, M, g)
    h = 1e-6
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = ((ref.project(p + e, M) - ref.project(p - e, M)) * g).sum(axis=1) / (2 * h)
        np.testing.assert_allclose(vjp[:, a], fd, rtol=1e-6, atol=1e-9)
    pts = rng.random((5, 3)) * [0.8, 0.8, 1.0] + [0.1, 0.1, 0.0]
    targets = [rng.random((l1, l0)) for l0, l1 in ref.level_sizes(20, 24, 3)]
    assert [t.shape for t in ref.pyramid(pts, 3, 6.0, 20, 24)] == [(24, 20), (12, 10), (6, 5)]
    loss, gp = ref.pyramid_l1(pts, targets, 6.0, 20, 24)
    for k, a in ((0, 0), (3, 1), (4, 2)):
        e = np.zeros_like(pts)
        e[k, a] = 1e-6
        fd = (ref.pyramid_l1(pts + e, targets, 6.0, 20, 24)[0] - ref.pyramid_l1(pts - e, targets, 6.0, 20, 24)[0]) / 2e-6
        np.testing.assert_allclose(gp[k, a], fd, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------ the seeded cases of the GPU suite
def test_central_differences_can_use_at_least_95_percent_of_the_seeded_rays():
    verts, tris = sc.ray_meshes()["sphere"]
    assert tris.shape == (48, 3)  # 8 x 4: two fans of 8 and two bands of 16
    o, d = sc.seeded_rays(**sc.CD_RAYS)
    t, prim = ref.trace(o, d, verts, tris)
    assert (prim >= 0).all()
    oo, dd = sc.cd_neighbours(o, d)
    t12, p12 = zip(*(ref.trace(oo[r], dd[r], verts, tris) for r in range(12)))
    cdo, cdd, usable = sc.cd_from_t(o, d, oo, dd, np.stack(t12), np.stack(p12), prim)
    assert usable.mean() >= 0.95
    _, dt_do, dt_dd = ref.plane_hit(o, d, verts, tris, prim)
    bo, bd = sc.cd_bound(o, d, verts, tris, prim, t)
    assert (np.abs(cdo - dt_do)[usable] <= bo[usable]).all() and (np.abs(cdd - dt_dd)[usable] <= bd[usable]).all()
    assert bd[usable].max() < 0.05 * np.abs(dt_dd[usable]).max()  # the bound still tells a wrong derivative from a right one


def test_the_ray_cases_have_hits_misses_and_steep_enough_angles():
    for name, (verts, tris) in sc.ray_meshes().items():
        o, d = sc.seeded_rays(name)
        _, prim = ref.trace(o, d, verts, tris)
        n_len = np.linalg.norm(d.astype(np.float64), axis=1)
        assert (prim >= 0).sum() >= 64 and (prim < 0).sum() >= 4 and np.abs(n_len - 1).min() > 1e-3, name
        if name != "plane":
            assert len(np.unique(prim[prim >= 0])) >= 2, name


FIT_STEPS, FIT_RATIO = 40, 0.04  # the float64 loop brings the loss under 4 % of its start within 40 steps (it reaches 3.2 %)


def test_the_float64_fit_recovers_the_displaced_pattern():
    losses = sc.reference_fit(FIT_STEPS)
    assert losses[-1] <= FIT_RATIO * losses[0] and losses[0] > 0.1, losses[[0, -1]]
    # the end-to-end case: all 16 rays hit, both planes are hit, every hit lands on the film, and the plane term matters
    data = sc.two_planes()
    verts, tris = sc.world_mesh(data)
    M = sc.world_to_sample(data.camera)
    targets = sc.e2e_targets(verts, tris, M)
    rays = sc.pattern(sc.E2E_OFFSET)
    loss, g, pts, prim = sc.e2e_loss_grad(rays, targets, verts, tris, M)
    _, g0, _, _ = sc.e2e_loss_grad(rays, targets, verts, tris, M, plane_term=False)
    assert set(prim // 2) == {0, 1} and (pts > 0).all() and (pts < 1).all()
    assert np.abs(g - g0).max() > 0.05 * np.abs(g).max()
