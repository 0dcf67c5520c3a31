"""Forward mode (FFX_RENDER_TANGENT) without a GPU: the bit in the header and in _abi, the refusals that come before any launch
(tests/refusals.py's set-up), the packing of the tangent blocks behind the texture, mi.render_forward's key and integrator rules (on a
stand-in for the scene: they are decided before the geometry is touched) and the float64 tangent that tests/test_jvp_gpu.py compares to — central
differences of tests/ref_prb.render_fwd_frozen along the tangent, with the linear parts (texture, spot intensity) taken exactly."""
import re
import types

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, scene_desc, scenes
from tests import ref_prb, refusals
from tests.corner_scenes import small_corner
from tests.support import FFX_ERR_ARG, FFX_ERR_UNSUPPORTED, copy_desc, define, header, world_arrays

TAN = 0x80000
GAUSS = refusals.GAUSS
R0 = scenes.MAT_COLUMN["roughness"]


def test_bit_in_header_and_abi_agree_and_the_abi_is_frozen():
    h = header()
    assert define("FFX_RENDER_TANGENT") == _abi.RENDER_TANGENT == TAN
    assert define("FFX_ABI_VERSION") == _abi.FFX_ABI_VERSION == 11
    for name, val in re.findall(r"^#define\s+(FFX_RENDER_[A-Z_0-9]+)\s+(0x[0-9a-fA-F]+|\d+)\s", h, re.M):
        if name in ("FFX_RENDER_TANGENT", "FFX_RENDER_MAX_DEPTH_SHIFT", "FFX_RENDER_RR_DEPTH_SHIFT", "FFX_RENDER_MAX_DEPTH_LIMIT", "FFX_RENDER_MATERIAL_COLS"):
            continue
        assert TAN & int(val, 0) == 0, name
    assert "render_jvp" not in h and "ffx_render_forward" not in h  # (no new entry point: the bit rides on ffx_render_fwd[_filtered])


_OTHERS = ("ffx_render_fwd_cache", "ffx_render_fwd_adjoint", "ffx_render_fwd_adjoint_filtered", "ffx_render_fwd_cache_filtered", "ffx_render_bwd",
           "ffx_render_bwd_filtered", "ffx_render_bwd_det", "ffx_render_bwd_det_part", "ffx_render_bwd_cached")
_P3 = _abi.render_path(3, 5)
# (entry point, scene / bvh info changes, argument changes, return code, message)
_CASES = [
    ("ffx_render_fwd", {}, {"flags": TAN | _abi.RENDER_FP16}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_TANGENT has no fp16 film"),
    ("ffx_render_fwd", {}, {"flags": TAN | _abi.RENDER_FP16 | _P3}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_TANGENT has no fp16 film"),
    ("ffx_render_fwd_filtered", GAUSS, {"flags": TAN | _abi.RENDER_FP16}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: FFX_RENDER_TANGENT has no fp16 film"),
    ("ffx_render_fwd", {}, {"flags": TAN, "mats": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_TANGENT needs the device material table"),
    ("ffx_render_fwd", {"n_mat_h": 3}, {"flags": TAN | _P3, "mats": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_TANGENT needs the device material table"),
    ("ffx_render_fwd_filtered", GAUSS, {"flags": TAN, "mats": None}, FFX_ERR_ARG, "render_fwd_filtered: FFX_RENDER_TANGENT needs the device material table"),
    *[(f, GAUSS if "filtered" in f else {}, {"flags": TAN}, FFX_ERR_UNSUPPORTED, f"{f[4:]}: FFX_RENDER_TANGENT is served by ffx_render_fwd[_filtered] only")
      for f in _OTHERS],
    ("ffx_render_bwd", {}, {"flags": TAN | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_PRB | _P3}, FFX_ERR_UNSUPPORTED,
     "render_bwd: FFX_RENDER_TANGENT is served by ffx_render_fwd[_filtered] only"),
    # the other refusals of the served route still come first or in their order (nothing launches: the bvh info is refused)
    ("ffx_render_fwd", {}, {"flags": TAN | _abi.RENDER_GRAD_APPEARANCE}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_GRAD_APPEARANCE is served by"),
    ("ffx_render_fwd", {}, {"flags": TAN, "tex": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_TANGENT but tex (the tangent blocks) is NULL"),
    ("ffx_render_fwd", {"proj.enabled": 0}, {"flags": TAN, "tex": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_TANGENT but tex (the tangent blocks) is NULL"),
    ("ffx_render_fwd", {}, {"flags": TAN, "img": None}, FFX_ERR_ARG, "render_fwd: bad argument"),
    ("ffx_render_fwd", {"info.n_tris": 0}, {"flags": TAN}, FFX_ERR_ARG, "render_fwd: bad bvh info"),
    ("ffx_render_fwd", {"info.n_tris": 0}, {"flags": TAN | _P3}, FFX_ERR_ARG, "render_fwd: bad bvh info"),
    ("ffx_render_fwd_filtered", {"info.n_tris": 0, **GAUSS}, {"flags": TAN | _P3}, FFX_ERR_ARG, "render_fwd: bad bvh info"),
    ("ffx_render_fwd", GAUSS, {"flags": TAN}, FFX_ERR_UNSUPPORTED, "render_fwd: the scene's reconstruction filter is not the box"),
    ("ffx_render_fwd_filtered", {}, {"flags": TAN}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: rfilter must be FFX_RFILTER_GAUSSIAN"),
    ("ffx_render_fwd", {}, {"flags": TAN | _abi.render_path(9, 5)}, FFX_ERR_ARG, "render_fwd: max_depth must be 2 .. 8"),
    ("ffx_render_fwd", {"n_shapes": 0}, {"flags": TAN}, FFX_ERR_ARG, "render_fwd: n_shapes < 1"),
    ("ffx_render_fwd", {"cam.width": 65536, "cam.height": 32768}, {"flags": TAN, "spp": 1}, FFX_ERR_UNSUPPORTED, "render_fwd: more than 2^31 pixels"),
    # the last refusal in front of the primal's launches, as without the bit
    ("ffx_render_fwd", {}, {"flags": TAN}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
]


@pytest.mark.parametrize("case", _CASES, ids=lambda c: f"{c[0][4:]}-{c[3]}-{c[4][:48]}")
def test_refusals_before_any_launch(case, monkeypatch):
    name, changes, arg_changes, rc, msg = case
    got, err = refusals.call(name, changes, arg_changes, monkeypatch=monkeypatch)
    assert got == rc, (got, err)
    assert msg in err, err


def _sd(S, stride, proj, bt=()):
    sd = _abi.SceneDesc()
    sd.n_shapes, sd.mat_stride = S, stride
    sd.proj.enabled, sd.proj.tex_w, sd.proj.tex_h, sd.proj.tex_channels = int(proj), 5, 4, 1
    sd.n_base_tex = len(bt)
    for k, (h, w) in enumerate(bt):
        sd.base_tex_h[k], sd.base_tex_w[k] = h, w
    return sd


def test_packing_of_the_tangent_blocks():
    """[texture, tangent texture] (with a projector), then _abi.appearance_floats in the gradient block's layout, then the material block iff the
    table has material columns"""
    S, bt = 3, [(2, 3), (1, 2)]
    sd = _sd(S, _abi.MAT_STRIDE, True, bt)
    n_tex, n_app, n_mat = 20, _abi.appearance_floats(S, bt), _abi.material_floats(S)
    assert n_app == 3 * S + 3 + 3 * (6 + 2) and n_mat == 11 * S
    tex, dtex = torch.arange(20.0).reshape(4, 5, 1), 100 + torch.arange(20.0).reshape(4, 5, 1)
    rows, spot = 200 + torch.arange(9.0).reshape(3, 3), torch.tensor([301.0, 302.0, 303.0])
    b0, b1 = 400 + torch.arange(18.0).reshape(2, 3, 3), 500 + torch.arange(6.0).reshape(1, 2, 3)
    mat = 600 + torch.arange(33.0).reshape(3, 11)
    buf = ops.DeviceGeometry.pack_tangent(sd, tex, dtex, ops.AppearanceGrad(rows, spot, [b0, b1], mat))
    assert buf.dtype == torch.float32 and buf.numel() == 2 * n_tex + n_app + n_mat
    want = torch.cat([x.reshape(-1) for x in (tex, dtex, rows, spot, b0, b1, mat)])
    assert torch.equal(buf, want)
    # None is a zero tangent, field by field
    buf = ops.DeviceGeometry.pack_tangent(sd, tex, None, ops.AppearanceGrad(None, spot, [None, b1], None))
    want = torch.cat([tex.reshape(-1), torch.zeros(20 + 9), spot, torch.zeros(18), b1.reshape(-1), torch.zeros(33)])
    assert torch.equal(buf, want)
    assert torch.equal(ops.DeviceGeometry.pack_tangent(sd, tex, None, None)[n_tex:], torch.zeros(n_tex + n_app + n_mat))
    # no projector: neither texture; a table of stride 3: no material block
    sd = _sd(2, 3, False)
    buf = ops.DeviceGeometry.pack_tangent(sd, None, None, ops.AppearanceGrad(torch.ones(2, 3), None, [], None))
    assert buf.numel() == _abi.appearance_floats(2) == 9 and torch.equal(buf, torch.tensor([1.0] * 6 + [0.0] * 3))
    with pytest.raises(ValueError):
        ops.DeviceGeometry.pack_tangent(sd, None, None, ops.AppearanceGrad(None, None, [], torch.ones(2, 11)))
    with pytest.raises(ValueError):
        ops.DeviceGeometry.pack_tangent(_sd(2, 3, True), None, None, None)  # (the projector's texture is needed)
    with pytest.raises(ValueError):
        ops.DeviceGeometry.pack_tangent(_sd(2, 3, False), None, None, ops.AppearanceGrad(torch.ones(3, 3), None, [], None))


@pytest.mark.parametrize("material", [False, True])
@pytest.mark.parametrize("bt", [[], [(2, 3), (1, 4)]])
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("S", [2, 3])
def test_one_layout_of_the_gradient_and_tangent_blocks(S, proj, bt, material):
    """ops.appearance_blocks is the one place that knows the blocks' order and offsets: its views tile the buffer behind the start offset — rows, spot,
    the base textures in index order, the material block — without a gap or an overlap, they cover what _abi's totals say, and what pack_tangent
    writes is what they read (behind the texture and its tangent)"""
    sd = _sd(S, _abi.MAT_STRIDE if material else 3, proj, bt)
    total = _abi.appearance_floats(S, bt) + (_abi.material_floats(S) if material else 0)
    start = 7
    buf = torch.arange(float(start + total))
    blocks, n = ops.appearance_blocks(sd, material, buf, start)
    assert n == total
    assert tuple(blocks.rows.shape) == (S, 3) and tuple(blocks.spot.shape) == (3,) and [tuple(b.shape) for b in blocks.base_tex] == [(h, w, 3) for h, w in bt]
    assert (blocks.material is None) == (not material) and (not material or tuple(blocks.material.shape) == (S, 11))
    parts = [blocks.rows, blocks.spot, *blocks.base_tex] + ([blocks.material] if material else [])
    assert torch.equal(torch.cat([x.reshape(-1) for x in parts]), buf[start:])  # every float behind `start` once, in this order
    assert all(x.data_ptr() == buf.data_ptr() + 4 * int(x.reshape(-1)[0]) for x in parts)  # ... as views, not copies
    # distinct inputs through pack_tangent, read back through the same views
    n_tex = 20 if proj else 0
    g = torch.Generator().manual_seed(S + 10 * len(bt))
    tex, dtex = (torch.rand(4, 5, 1, generator=g), torch.rand(4, 5, 1, generator=g)) if proj else (None, None)
    tan = ops.AppearanceGrad(torch.rand(S, 3, generator=g), torch.rand(3, generator=g), [torch.rand(h, w, 3, generator=g) for h, w in bt],
                             torch.rand(S, 11, generator=g) if material else None)
    packed = ops.DeviceGeometry.pack_tangent(sd, tex, dtex, tan)
    assert packed.numel() == 2 * n_tex + total
    back, _ = ops.appearance_blocks(sd, material, packed, 2 * n_tex)
    assert torch.equal(back.rows, tan.rows) and torch.equal(back.spot, tan.spot) and len(back.base_tex) == len(bt)
    assert all(torch.equal(a, b) for a, b in zip(back.base_tex, tan.base_tex))
    assert back.material is None if not material else torch.equal(back.material, tan.material)
    if proj:
        assert torch.equal(packed[:2 * n_tex], torch.cat([tex.reshape(-1), dtex.reshape(-1)]))


class _NoGeometry:
    def __getattr__(self, name):
        raise AssertionError(f"the rule must be decided before the geometry is touched (geom.{name})")


class _Served(Exception):
    """the rules let the call through: it went on to read the scene's parameters"""


class _Params:
    _leaf_keys = frozenset(["mat-A.brdf_0.base_color.value", "mat-A.brdf_0.roughness.value", "mat-A.brdf_0.specular", "emit-Spot.intensity.value"])

    def __getitem__(self, k):
        raise _Served(k)


def _stand_in(projector=True):
    return types.SimpleNamespace(_params=_Params(), data=types.SimpleNamespace(projector=object() if projector else None), geom=_NoGeometry())


def test_render_forward_refuses_unknown_keys_and_path_with_appearance_tangents():
    sc = _stand_in()
    with pytest.raises(KeyError) as e:
        mi.render_forward(sc, None, {"mat-A.brdf_0.base_color.value": torch.ones(3), "PerspectiveCamera.to_world": torch.eye(4)})
    msg = str(e.value)
    assert "PerspectiveCamera.to_world" in msg and all(k in msg for k in sorted(sc._params._leaf_keys) + ["tex.data"])
    with pytest.raises(KeyError) as e:
        mi.render_forward(_stand_in(projector=False), None, {"tex.data": torch.ones(2, 2)})
    assert "tex.data" in str(e.value)
    path3 = mi.load_dict({"type": "path", "max_depth": 3})
    with pytest.raises(ValueError, match="prb") as e:
        mi.render_forward(sc, None, {"tex.data": torch.ones(2, 2), "mat-A.brdf_0.roughness.value": 1.0}, integrator=path3)
    assert "mat-A.brdf_0.roughness.value" in str(e.value)
    with pytest.raises(ValueError, match="prb"):
        path3.render_forward(sc, None, {"emit-Spot.intensity.value": torch.ones(3)})
    with pytest.raises(TypeError):
        mi.render_forward(sc, None, {"tex.data": torch.ones(2, 2)}, integrator="prb")
    with pytest.raises(TypeError):
        mi.render_forward(sc, None, ["tex.data"])
    with pytest.raises(NotImplementedError):
        mi.render_forward(sc, None, {}, sensor=1)
    # what is served goes on to the geometry: path + tex.data alone, prb, direct, max_depth 2
    for it, tan in ((path3, {"tex.data": 0}), (mi.load_dict({"type": "prb", "max_depth": 3}), {"mat-A.brdf_0.specular": 0}),
                    (mi.load_dict({"type": "direct"}), {"mat-A.brdf_0.specular": 0}), (mi.load_dict({"type": "path", "max_depth": 2}), {"mat-A.brdf_0.specular": 0})):
        with pytest.raises(_Served):
            mi.render_forward(sc, None, tan, integrator=it)


# ---------------------------------------------------------------------------------------------- the float64 tangent (tests/ref_prb.py)
@pytest.mark.parametrize("depth,rr,stddev", [(2, 5, None), (3, 1, None), (3, 1, 0.5)])
def test_float64_tangent_is_converged_in_h(depth, rr, stddev):
    """halving h changes the reference by less than 1e-6 of its scale (the stencil's h^4 term and the differences' rounding are both below it), and the
    exact linear parts are what differences of the texture and the intensity give"""
    sc = small_corner()
    world = world_arrays(sc)[:3]
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    if stddev is not None:
        sd.rfilter = _abi.RFILTER_GAUSSIAN
    rows = scenes.material_rows(sc).astype(np.float64)
    rng = np.random.default_rng(1)
    tex = rng.uniform(0, 1, (8, 8, 1))
    drows = ref_prb.interior_material_tangent(rows, rng)
    drows[:, :3] = rng.uniform(0.5, 1.5, (rows.shape[0], 3))
    assert (drows[:, R0:R0 + 11] != 0).sum() >= 12
    spp, seed = 4, 3
    a = ref_prb.float64_tangent(world, sd, rows, tex, spp, seed, depth, rr, stddev, drows=drows, h=5e-4)
    b = ref_prb.float64_tangent(world, sd, rows, tex, spp, seed, depth, rr, stddev, drows=drows, h=2.5e-4)
    scale = np.abs(a).max()
    print("depth", depth, "rr", rr, "stddev", stddev, ": max |T(h) - T(h/2)|", np.abs(a - b).max(), "scale", scale)
    assert scale > 0 and np.abs(a - b).max() <= 1e-6 * scale
    dtex = rng.uniform(-1, 1, (8, 8, 1))
    dspot = np.array([0.5, 2.0, 1.25], np.float32)
    lin = ref_prb.float64_tangent(world, sd, rows, tex, spp, seed, depth, rr, stddev, dtex=dtex, dspot=dspot)
    hi = copy_desc(sd)
    for c in range(3):
        hi.spot.intensity[c] = float(sd.spot.intensity[c]) + float(dspot[c])
    fd = (ref_prb.render_fwd_frozen(*world, hi, rows, rows, tex + dtex, spp, seed, depth, rr, gaussian_stddev=stddev)
          - ref_prb.render_fwd_frozen(*world, sd, rows, rows, tex, spp, seed, depth, rr, gaussian_stddev=stddev))
    print("linear parts: max |exact - difference|", np.abs(lin - fd).max(), "scale", np.abs(fd).max())
    assert np.abs(fd).max() > 0 and np.abs(lin - fd).max() <= 1e-9 * np.abs(fd).max()
