"""The `aov` integrator without a GPU: mi.load_dict's parsing, names and refusals, the ABI constants against the header, the refusals
of FFX_RENDER_AOV that come before any launch, and tests/ref_aov.py on a plane in closed form."""
import re

import numpy as np
import pytest

from fireflies_amd import _abi, mi, ops, scene_desc, scenes
from fireflies_amd import functional as Fn
from fireflies_amd.optim import PatternOptimizer
from tests import ref_aov, refusals
from tests.support import FFX_ERR_ARG, FFX_ERR_UNSUPPORTED, define, header

SERVED = ["albedo", "depth", "geo_normal", "position", "prim_index", "sh_normal", "shape_index", "uv"]


def test_load_dict_keeps_the_order_of_aovs_and_names_the_channels():
    it = mi.load_dict({"type": "aov", "aovs": "dd.y:depth, nn:sh_normal,pos:position,tc:uv,alb:albedo,gn:geo_normal,sid:shape_index,pid:prim_index",
                       "my_image": {"type": "path", "max_depth": 3}})
    assert isinstance(it, mi.Integrator) and it.type == "aov"
    assert it.aovs == [("dd.y", "depth"), ("nn", "sh_normal"), ("pos", "position"), ("tc", "uv"), ("alb", "albedo"), ("gn", "geo_normal"),
                       ("sid", "shape_index"), ("pid", "prim_index")]
    assert it.aov_names() == ["dd.y", "nn.X", "nn.Y", "nn.Z", "pos.X", "pos.Y", "pos.Z", "tc.U", "tc.V", "alb.R", "alb.G", "alb.B", "gn.X", "gn.Y", "gn.Z",
                              "sid", "pid", "my_image.R", "my_image.G", "my_image.B"]
    key, inner = it.nested
    assert key == "my_image" and inner.type == "path" and inner.max_depth == 3 and (it.max_depth, it.rr_depth) == (3, 5)
    alone = mi.load_dict({"type": "aov", "aovs": "d:depth"})
    assert alone.nested is None and alone.aov_names() == ["d"] and alone.max_depth == 2
    for t in ("prb", "direct"):
        assert mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": t, **({"max_depth": 4} if t == "prb" else {})}}).nested[1].type == t


@pytest.mark.parametrize("type_", ["dp_du", "dp_dv", "duv_dx", "duv_dy", "normals"])
def test_load_dict_refuses_types_that_are_not_served(type_):
    with pytest.raises(ValueError) as e:
        mi.load_dict({"type": "aov", "aovs": f"d:depth,x:{type_}"})
    assert type_ in str(e.value) and all(s in str(e.value) for s in SERVED)


def test_load_dict_refuses_malformed_and_nested_aov_integrators():
    with pytest.raises(ValueError, match="at most one nested integrator"):
        mi.load_dict({"type": "aov", "aovs": "d:depth", "a": {"type": "path", "max_depth": 3}, "b": {"type": "direct"}})
    with pytest.raises(ValueError, match="cannot be nested"):
        mi.load_dict({"type": "aov", "aovs": "d:depth", "a": {"type": "aov", "aovs": "d:depth"}})
    with pytest.raises(ValueError, match="needs 'aovs'"):
        mi.load_dict({"type": "aov"})
    with pytest.raises(ValueError, match="<name>:<type>"):
        mi.load_dict({"type": "aov", "aovs": "depth"})
    with pytest.raises(ValueError, match="not served"):
        mi.load_dict({"type": "aov", "aovs": "d:depth", "max_depth": 3})


def test_everything_but_mi_render_refuses_an_aov_integrator():
    it = mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": "direct"}})
    with pytest.raises(ValueError, match="aov"):
        mi.render_forward(None, None, {}, integrator=it)
    with pytest.raises(ValueError, match="aov"):
        Fn.render(None, None, None, None, 1, integrator=it)
    with pytest.raises(ValueError, match="aov"):
        PatternOptimizer(None, None, None, integrator=it)
    with pytest.raises(ValueError, match="fp16"):
        mi.render(None, spp=1, fp16=True, integrator=it)


def test_abi_constants_agree_with_the_header():
    text = header()
    assert int(re.search(r"#define FFX_RENDER_AOV (0x[0-9a-fA-F]+)", text).group(1), 16) == _abi.RENDER_AOV == 0x100000
    assert int(re.search(r"#define FFX_RENDER_AOV_FLOATS (\d+)", text).group(1)) == _abi.RENDER_AOV_FLOATS == 17 == ref_aov.FLOATS
    assert define("FFX_ABI_VERSION") == 11
    assert ops.AOV_CHANNELS == ref_aov.CHANNELS
    taken = (_abi.RENDER_FP16 | _abi.RENDER_SPARSE_ADJOINT | _abi.RENDER_APEX_READY | _abi.RENDER_CACHE_ZEROED | _abi.RENDER_CACHE_KEEP_DROPPED
             | _abi.RENDER_PATH_MASK | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL | _abi.RENDER_GRAD_PRB | _abi.RENDER_TANGENT)
    assert _abi.RENDER_AOV & taken == 0


_AOV = _abi.RENDER_AOV
_REFUSALS = [
    ("ffx_render_fwd", _AOV | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_AOV has no fp16 film"),
    ("ffx_render_fwd_filtered", _AOV | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: FFX_RENDER_AOV has no fp16 film"),
    ("ffx_render_fwd", _AOV | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "FFX_RENDER_AOV is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd_filtered", _AOV | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "FFX_RENDER_AOV is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd", _AOV | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "FFX_RENDER_GRAD_APPEARANCE is served by ffx_render_bwd[_filtered] only"),
    ("ffx_render_fwd_filtered", _AOV | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED, "is served by ffx_render_bwd[_filtered] only"),
    ("ffx_render_fwd", _AOV | _abi.RENDER_GRAD_PRB, {}, FFX_ERR_UNSUPPORTED, "FFX_RENDER_GRAD_PRB is served by ffx_render_bwd[_filtered] only"),
    ("ffx_render_bwd", _AOV, {}, FFX_ERR_UNSUPPORTED, "render_bwd: FFX_RENDER_AOV is served by ffx_render_fwd[_filtered] only"),
    ("ffx_render_fwd_cache", _AOV, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache: FFX_RENDER_AOV is served by ffx_render_fwd[_filtered] only"),
    ("ffx_render_fwd", _AOV, {"mats": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_AOV needs a material table"),
    ("ffx_render_fwd", _AOV, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),  # (the last refusal in front of the launches)
]


@pytest.mark.parametrize("case", _REFUSALS, ids=lambda c: f"{c[0][4:]}-{c[1]:#x}-{'nomats' if c[2] else 'mats'}")
def test_the_bit_is_refused_before_any_launch(case, monkeypatch):
    """tests/refusals.py's set-up: nothing can launch"""
    name, flags, arg_changes, rc, msg = case
    got, err = refusals.call(name, refusals.GAUSS if "filtered" in name else {}, {"flags": flags, **arg_changes}, monkeypatch=monkeypatch)
    assert got == rc, (got, err)
    assert msg in err, err


def test_ref_aov_on_a_plane_in_closed_form():
    """a camera at (0.3, -0.2, 4) looking down at the plane z = 0.5 (two triangles, wound so that e1 x e2 = -z for the second mesh): depth is the distance
    along the ray from the near plane, the position lies on the plane, the normals are (0, 0, +-1) unfaced, uv is affine in the position"""
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    corners = np.array([[-4, -4, 0.5], [4, -4, 0.5], [4, 4, 0.5], [-4, 4, 0.5]], np.float64)
    W, H, spp, seed, near = 9, 7, 3, 5, 0.05
    sensor = scenes.SensorData("cam", scenes.look_at((0.3, -0.2, 4.0), (0.3, -0.2, 0.0), up=(0, 1, 0)), 40.0, near, 100.0, W, H)
    cam = scene_desc.camera_from_sensor(sensor)
    uv = (corners[:, :2] + 4.0) / 8.0 * np.array([3.0, 2.0]) + np.array([-0.5, 0.25])  # affine, beyond [0, 1]: not wrapped
    mats = np.array([[0.2, 0.4, 0.6]])
    for flip, nz in ((False, 1.0), (True, -1.0)):
        tri = quad[:, ::-1] if flip else quad
        a = ref_aov.aov_samples(corners, tri, np.zeros(2, np.int64), cam, spp, seed, mats, smooth=[True], vert_uv=uv)
        assert a.shape == (W * H * spp, 17) and (a[:, 15] == 0).all() and set(a[:, 16]) <= {0.0, 1.0}
        o, d, nt, _ = ref_aov.rb.camera_rays(cam, spp, True, seed)
        t = (0.5 - o[:, 2]) / d[:, 2]
        print("plane: max |depth - closed form|", np.abs(a[:, 0] - (t - nt)).max())
        np.testing.assert_allclose(a[:, 0], t - nt, rtol=0, atol=1e-12)
        np.testing.assert_allclose(nt, cam.near_clip / (-d[:, 2]), rtol=1e-12)  # (the camera looks along -z; the struct holds the clip as a float32)
        np.testing.assert_allclose(a[:, 1:4], o + t[:, None] * d, rtol=0, atol=1e-12)
        np.testing.assert_allclose(a[:, 3], 0.5, rtol=0, atol=1e-12)
        np.testing.assert_allclose(a[:, 4:7], np.broadcast_to([0, 0, nz], (len(a), 3)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(a[:, 7:10], np.broadcast_to([0, 0, nz], (len(a), 3)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(a[:, 10:12], (a[:, 1:3] + 4.0) / 8.0 * np.array([3.0, 2.0]) + np.array([-0.5, 0.25]), rtol=0, atol=1e-12)
        assert a[:, 10].max() > 1.0  # (not wrapped)
        np.testing.assert_allclose(a[:, 12:15], np.broadcast_to(mats[0], (len(a), 3)))
        box = ref_aov.aov_block(corners, tri, np.zeros(2, np.int64), cam, spp, seed, mats, smooth=[True], vert_uv=uv)
        np.testing.assert_allclose(box, a.reshape(H, W, spp, 17).mean(2))
        gau = ref_aov.aov_block(corners, tri, np.zeros(2, np.int64), cam, spp, seed, mats, smooth=[True], vert_uv=uv, gaussian_stddev=0.5)
        np.testing.assert_allclose(gau[..., 3], 0.5, atol=1e-12)  # (a constant channel survives any normalised film)
        np.testing.assert_allclose(gau[..., 6], nz, atol=1e-12)
    # a miss is all zeros
    far = ref_aov.aov_samples(corners + np.array([100.0, 0, 0]), quad, np.zeros(2, np.int64), cam, 1, seed, mats)
    assert not far.any()
