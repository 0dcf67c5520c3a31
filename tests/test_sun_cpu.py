"""The directional emitter without a GPU: the header's macros against _abi, ops.pack_lights' record and the bit _with_lights sets, the
refusals of FFX_RENDER_LIGHTS_DIRECTIONAL that come before any launch, the loader, mi.Scene's parameter map (over a stand-in for the device geometry),
tests/ref_sun.py's own identities in float64 and — on ref_sun alone — the preconditions of the comparisons tests/test_sun_gpu.py makes."""
import re
import types

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, loaders, mi, ops, scenes
from tests import light_scenes as ls
from tests import ref_lights as rl
from tests import ref_path as rp
from tests import ref_sun as rs
from tests import refusals
from tests import sun_scenes as ss
from tests.support import FFX_ERR_ARG, FFX_ERR_UNSUPPORTED, arrays, define, header, host_tex, load_xml


# ------------------------------------------------------------------ 1. header and ABI
def test_the_headers_macros_equal_abis_and_the_abi_version_stays():
    assert define("FFX_ABI_VERSION") == 11
    assert define("FFX_LIGHT_DIRECTIONAL") == _abi.LIGHT_DIRECTIONAL == 2
    assert define("FFX_RENDER_LIGHTS_DIRECTIONAL") == _abi.RENDER_LIGHTS_DIRECTIONAL == 0x4000000 == 1 << 26
    assert (define("FFX_LIGHT_POINT"), define("FFX_LIGHT_SPOT"), define("FFX_LIGHT_FLOATS"), define("FFX_RENDER_MAX_LIGHTS")) == (0, 1, 24, 8)
    taken = (_abi.RENDER_FP16 | _abi.RENDER_SPARSE_ADJOINT | _abi.RENDER_APEX_READY | _abi.RENDER_CACHE_ZEROED | _abi.RENDER_CACHE_KEEP_DROPPED | _abi.RENDER_PATH_MASK
             | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL | _abi.RENDER_GRAD_PRB | _abi.RENDER_TANGENT | _abi.RENDER_AOV | _abi.RENDER_LIGHTS_MASK
             | _abi.RENDER_AMBIENT)
    assert _abi.RENDER_LIGHTS_DIRECTIONAL & taken == 0 and taken < 1 << 26
    # no other flag word of the header's render calls uses bit 26
    words = {n: int(v, 16) for n, v in re.findall(r"#define (FFX_RENDER_\w+) (0x[0-9a-fA-F]+)\b", header())}
    assert len(words) >= 7 and words.pop("FFX_RENDER_LIGHTS_DIRECTIONAL") == 1 << 26
    assert not [n for n, v in words.items() if v & (1 << 26)], words


# ------------------------------------------------------------------ 2. packing and LightData
def test_pack_lights_writes_the_directional_record_word_for_word():
    t = ops.pack_lights([ls.POINT, ss.SUN_A, ls.SPOT_B]).numpy()
    assert t.shape == (3, 24) and t.dtype == np.float32
    row = t[1]
    np.testing.assert_array_equal(row[:16], np.asarray(ss.SUN_A.to_world, np.float32).reshape(16))
    np.testing.assert_array_equal(row[16:19], np.asarray(ss.SUN_A.intensity, np.float32))
    assert (row[19], row[20], row[21], row[22], row[23]) == (0.0, 0.0, 2.0, 0.0, 0.0)
    np.testing.assert_array_equal(rs.table_row(ss.SUN_A.to_world, ss.SUN_A.intensity).astype(np.float32), row)
    # the other two records are what they were
    np.testing.assert_array_equal(t[[0, 2]], ops.pack_lights([ls.POINT, ls.SPOT_B]).numpy())
    assert ops.lights_directional([ls.POINT, ss.SUN_A]) is True and ops.lights_directional([ls.POINT, ls.SPOT_B]) is False and ops.lights_directional([]) is False
    with pytest.raises(ValueError, match="at most 8"):
        ops.pack_lights([ss.SUN_A] * 9)


def test_light_data_accepts_the_kind_and_still_refuses_others():
    sun = scenes.LightData("s", "directional", np.eye(4), (1.0, 2.0, 3.0))
    assert sun.kind == "directional" and sun.intensity == (1.0, 2.0, 3.0)
    for kind in ("area", "sun", "envmap"):
        with pytest.raises(ValueError, match="kind"):
            scenes.LightData("x", kind, np.eye(4))


def test_with_lights_ors_the_bit_and_defaults_to_todays_bits():
    geom = types.SimpleNamespace(device=torch.device("cpu"))
    sd = _abi.SceneDesc()
    sd.n_shapes, sd.mat_stride = 2, 0
    rows = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    lights = ops.pack_lights([ls.POINT, ss.SUN_A])
    orig = ops._dev
    try:
        ops._dev = lambda t, *a, **k: t
        today = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights, "test")
        assert len(today) == 3 and today[1] == _abi.render_lights(2)
        arg, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights, "test", lights_directional=True)
        assert bits == _abi.render_lights(2) | _abi.RENDER_LIGHTS_DIRECTIONAL and torch.equal(buf, today[2]) and arg is buf
        _, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights, "test", (0.25, 0.5, 2.0), lights_directional=True)
        assert bits == _abi.render_lights(2) | _abi.RENDER_AMBIENT | _abi.RENDER_LIGHTS_DIRECTIONAL and buf.tolist()[-4:] == [0.25, 0.5, 2.0, 0.0]
        _, bits, _ = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights, "test", None, False)  # (the keyword goes last)
        assert bits == _abi.render_lights(2)
        # without a table there is nothing the bit could speak of: it is not set (the library would refuse it)
        assert ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", None, "test", lights_directional=True) == ("mats", 0, None)
        _, bits, _ = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights[:0], "test", (1.0, 1.0, 1.0), lights_directional=True)
        assert bits == _abi.RENDER_AMBIENT
    finally:
        ops._dev = orig


# ------------------------------------------------------------------ 3. refusals before any launch (tests/refusals.py's set-up)
_D, _L1, _A = _abi.RENDER_LIGHTS_DIRECTIONAL, _abi.render_lights(1), _abi.RENDER_AMBIENT
_DL = _D | _L1
_ONLY = "FFX_RENDER_LIGHTS is served by ffx_render_fwd[_filtered] only"  # (the count's refusal comes first: its wording stays)
_ONLY_D = "FFX_RENDER_LIGHTS_DIRECTIONAL is served by ffx_render_fwd[_filtered] only"
_GRAD = "is not served together with a FFX_RENDER_GRAD_* bit"
_REFUSALS = [
    # the bit without a count: the message names both
    ("ffx_render_fwd", _D, {}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_LIGHTS_DIRECTIONAL needs FFX_RENDER_LIGHTS(n >= 1)"),
    ("ffx_render_fwd_filtered", _D | _A, {}, FFX_ERR_ARG, "render_fwd_filtered: FFX_RENDER_LIGHTS_DIRECTIONAL needs FFX_RENDER_LIGHTS(n >= 1)"),
    ("ffx_render_fwd", _D | _abi.render_path(3, 5), {}, FFX_ERR_ARG, "FFX_RENDER_LIGHTS_DIRECTIONAL needs FFX_RENDER_LIGHTS(n >= 1)"),
    # refused where FFX_RENDER_LIGHTS is
    ("ffx_render_fwd", _DL | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "no fp16 film"),
    ("ffx_render_fwd_filtered", _DL | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "no fp16 film"),
    ("ffx_render_fwd", _DL | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd_filtered", _DL | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd", _DL | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, _GRAD),
    ("ffx_render_fwd_filtered", _DL | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED, _GRAD),
    ("ffx_render_fwd", _DL | _abi.RENDER_GRAD_PRB, {}, FFX_ERR_UNSUPPORTED, _GRAD),
    ("ffx_render_bwd", _DL | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_bwd: FFX_RENDER_LIGHTS " + _GRAD),
    ("ffx_render_bwd", _D | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_bwd: FFX_RENDER_LIGHTS_DIRECTIONAL " + _GRAD),
    ("ffx_render_bwd_filtered", _DL | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_PRB | _abi.render_path(3, 5), {}, FFX_ERR_UNSUPPORTED,
     "render_bwd_filtered: FFX_RENDER_LIGHTS " + _GRAD),
    ("ffx_render_bwd_filtered", _D | _abi.RENDER_GRAD_MATERIAL | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED,
     "render_bwd_filtered: FFX_RENDER_LIGHTS_DIRECTIONAL " + _GRAD),
    ("ffx_render_fwd_cache", _DL, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache: " + _ONLY),
    ("ffx_render_fwd_cache", _D, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache: " + _ONLY_D),
    ("ffx_render_fwd_cache_filtered", _D, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: " + _ONLY_D),
    ("ffx_render_fwd_adjoint", _D, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint: " + _ONLY_D),
    ("ffx_render_fwd_adjoint_filtered", _D, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint_filtered: " + _ONLY_D),
    ("ffx_render_bwd_det", _D, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det: " + _ONLY_D),
    ("ffx_render_bwd_det_part", _D, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det_part: " + _ONLY_D),
    ("ffx_render_fwd", _D | _abi.render_lights(9), {}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_LIGHTS(9): at most 8 extra emitters"),
    ("ffx_render_fwd", _DL, {"mats": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_LIGHTS needs the device buffer [material table | lights] (shape_albedo is NULL)"),
    # served — with paths, an AOV block and the constant emitter — and accepted and ignored by the adjoint without a FFX_RENDER_GRAD_* bit: the calls get
    # as far as the last refusal in front of the launches
    ("ffx_render_fwd", _DL, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_fwd", _D | _abi.render_lights(8) | _A, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_fwd", _DL | _abi.RENDER_AOV, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_bwd", _DL, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
    ("ffx_render_bwd", _D, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
    ("ffx_render_bwd_filtered", _DL | _A, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
]


@pytest.mark.parametrize("case", _REFUSALS, ids=lambda c: f"{c[0][4:]}-{c[1]:#x}-{'nomats' if c[2] else 'mats'}")
def test_the_bit_is_refused_before_any_launch(case, monkeypatch):
    """tests/refusals.py's set-up (nothing can launch), with this suite's own default: no dot_out / loss_slots buffer"""
    name, flags, arg_changes, rc, msg = case
    got, err = refusals.call(name, refusals.GAUSS if "filtered" in name else {}, {"flags": flags, "dot": None, **arg_changes}, monkeypatch=monkeypatch)
    assert got == rc, (got, err)
    assert msg in err, err


# ------------------------------------------------------------------ 4. the loader
def _sun_dir(light):
    z = np.asarray(light.to_world, np.float64)[:3, 2]
    return z / np.linalg.norm(z)


def test_the_loader_reads_the_directional_emitter(tmp_path):
    sc, reports = load_xml(ss.write_scene(tmp_path))
    print(reports)
    assert [(l.name, l.kind) for l in sc.lights] == [("emit-Light", "point"), ("emit-Sun", "directional")]  # (file order)
    sun = sc.lights[1]
    assert sun.intensity == ss.FILE_SUN_IRRADIANCE
    tw = np.asarray(sun.to_world, np.float64)
    np.testing.assert_allclose(_sun_dir(sun), ss.FILE_SUN_DIR, atol=1e-6)
    np.testing.assert_allclose(tw[:3, :3].T @ tw[:3, :3], np.eye(3), atol=1e-6)  # (a frame about the direction)
    assert np.linalg.det(tw[:3, :3]) > 0
    assert sc.spot is not None and sc.projector is not None and sc.ambient is not None and sc.ambient.radiance == ss.WORLD_RADIANCE
    assert not any("directional" in r for r in reports), reports
    # the other spelling of the vector, a single float, a spectrum
    sc1, r1 = load_xml(ss.write_scene(tmp_path, ss.with_sun('<emitter type="directional" id="sun"><float name="irradiance" value="0.25"/>'
                                                         '<vector name="direction" x="0" y="3" z="-4"/></emitter>'), "f.xml"))
    assert sc1.lights[1].name == "sun" and sc1.lights[1].intensity == (0.25, 0.25, 0.25) and not any("directional" in r for r in r1)
    np.testing.assert_allclose(_sun_dir(sc1.lights[1]), (0.0, 0.6, -0.8), atol=1e-6)
    sc2, _ = load_xml(ss.write_scene(tmp_path, ss.with_sun('<emitter type="directional" id="sun"><spectrum name="irradiance" value="3"/></emitter>'), "s.xml"))
    assert sc2.lights[1].intensity == (3.0, 3.0, 3.0)
    # no id, no irradiance, no pose: Mitsuba's defaults — irradiance 1 along the local +Z of the identity
    sc3, _ = load_xml(ss.write_scene(tmp_path, ss.with_sun('<emitter type="directional"/>'), "d.xml"))
    assert sc3.lights[1].kind == "directional" and sc3.lights[1].intensity == (1.0, 1.0, 1.0)
    np.testing.assert_array_equal(np.asarray(sc3.lights[1].to_world), np.eye(4, dtype=np.float32))
    # to_world: the whole transform is kept, its +Z is the direction
    look = '<transform name="to_world"><lookat origin="4,3,5" target="1,1,0" up="0,0,1"/></transform>'
    sc4, _ = load_xml(ss.write_scene(tmp_path, ss.with_sun(f'<emitter type="directional" id="sun"><rgb name="irradiance" value="1,2,3"/>{look}</emitter>'), "t.xml"))
    np.testing.assert_allclose(np.asarray(sc4.lights[1].to_world), scenes.look_at((4, 3, 5), (1, 1, 0), up=(0, 0, 1)), atol=1e-6)
    np.testing.assert_allclose(_sun_dir(sc4.lights[1]), ss.unit((-3, -2, -5)), atol=1e-6)
    assert sc4.lights[1].intensity == (1.0, 2.0, 3.0)


def test_both_poses_and_a_zero_direction_raise(tmp_path):
    look = '<transform name="to_world"><lookat origin="4,3,5" target="1,1,0" up="0,0,1"/></transform>'
    both = f'<emitter type="directional" id="sun"><vector name="direction" value="0,0,-1"/>{look}</emitter>'
    with pytest.raises(ValueError, match=r"'direction'.*'to_world'"):
        loaders.load_mitsuba_xml(ss.write_scene(tmp_path, ss.with_sun(both), "both.xml"))
    for k, zero in enumerate(('<vector name="direction" value="0,0,0"/>', '<vector name="direction" x="0" y="0" z="0"/>')):
        with pytest.raises(ValueError, match="direction"):
            loaders.load_mitsuba_xml(ss.write_scene(tmp_path, ss.with_sun(f'<emitter type="directional" id="sun">{zero}</emitter>'), f"zero{k}.xml"))


def test_the_slots_are_eight_in_file_order_and_unknown_properties_are_reported_once(tmp_path):
    sc, reports = load_xml(ss.write_scene(tmp_path, ss.with_extra_suns(8), "ten.xml"))  # 2 + 8 = 10 extra emitters
    assert len(sc.lights) == 8 and [l.name for l in sc.lights] == ["emit-Light", "emit-Sun"] + [f"emit-More{k}" for k in range(6)]
    assert all(l.kind == "directional" for l in sc.lights[1:])
    told = [r for r in reports if "dropped" in r and "emitters" in r]
    assert len(told) == 1 and "emit-More6" in told[0], reports
    extra = '<float name="scale" value="2"/>'
    xml = ss.with_sun(f'<emitter type="directional" id="a">{extra}</emitter><emitter type="directional" id="b">{extra}</emitter>')
    sc, reports = load_xml(ss.write_scene(tmp_path, xml, "p.xml"))
    assert [l.name for l in sc.lights] == ["emit-Light", "a", "b"]
    assert [r for r in reports if "directional emitter property 'scale' is ignored" in r] and len([r for r in reports if "'scale'" in r]) == 1, reports


def test_a_file_without_the_emitter_loads_as_before_and_the_pinned_reports_keep_their_wording(tmp_path):
    plain, r0 = load_xml(ss.write_scene(tmp_path, ss.with_sun(""), "plain.xml"))
    with_s, r1 = load_xml(ss.write_scene(tmp_path))
    assert [l.name for l in plain.lights] == ["emit-Light"] and r0 == [r.replace("sun.xml", "plain.xml") for r in r1]
    assert np.array_equal(plain.spot.to_world, with_s.spot.to_world) and plain.spot.intensity == with_s.spot.intensity and plain.ambient == with_s.ambient
    assert np.array_equal(plain.lights[0].to_world, with_s.lights[0].to_world) and plain.lights[0].intensity == with_s.lights[0].intensity
    xml = ss.with_sun('<emitter type="envmap" id="sky"><string name="filename" value="e.exr"/></emitter>')
    xml = xml.replace('</bsdf></shape>', '</bsdf><emitter type="area"><rgb name="radiance" value="1"/></emitter></shape>', 1)
    _, reports = load_xml(ss.write_scene(tmp_path, xml, "env.xml"))
    assert any("emitter type 'envmap' ignored: only `projector` and `spot` emitters illuminate the scene" in r for r in reports), reports
    assert any("area emitter on a shape ignored" in r for r in reports), reports
    # light_scenes' file (no sun): what it loaded before
    sc, reports = load_xml(ls.write_scene(tmp_path))
    assert [(l.name, l.kind) for l in sc.lights] == [("emit-Light", "point"), ("emit-PointLight", "point"), ("emit-SecondSpot", "spot")]
    assert not any("directional" in r for r in reports)


# ------------------------------------------------------------------ 5. mi.Scene's parameter map (a stand-in for the device geometry: no key here moves it)
class _NoGeometry:
    def __init__(self, *a, device=None, **k):
        self.device, self.version, self._async, self.n_shapes = device, 0, False, 4

    def update(self, *a, **k):
        raise AssertionError("an emitter's key pushed the geometry")


def test_the_parameter_map_holds_the_sun_and_the_table_follows_it(monkeypatch):
    import fireflies_amd as ff

    monkeypatch.setattr(ops, "DeviceGeometry", _NoGeometry)
    sc = ss.corner()
    sc.lights = [ls.POINT, ss.SUN_A]
    scene = mi.load_scene_data(sc, device="cpu", shadows=True)
    params = mi.traverse(scene)
    assert "emit-SunA.irradiance.value" in params and "emit-SunA.to_world" in params
    assert not [k for k in params.keys() if k.startswith("emit-SunA.") and k.split(".", 1)[1] not in ("irradiance.value", "to_world")]
    assert scene.lights_directional() is True and mi._has_lights(scene)
    t0 = scene.lights_table()
    assert torch.equal(t0, ops.pack_lights([ls.POINT, ss.SUN_A])) and scene.lights_table() is t0  # (kept until an update touches a key)
    params["emit-SunA.irradiance.value"] = mi.Color3f(torch.tensor([4.0, 5.0, 6.0]))
    params.update()
    t1 = scene.lights_table()
    assert t1 is not t0 and t1[1, 16:19].tolist() == [4.0, 5.0, 6.0] and torch.equal(t1[1, :16], t0[1, :16]) and torch.equal(t1[0], t0[0])
    params["emit-SunA.to_world"] = mi.Transform4f(ss.frame((0.0, 0.6, -0.8)))
    params.update()
    t2 = scene.lights_table()
    np.testing.assert_allclose(t2[1, :16].reshape(4, 4)[:3, 2].numpy(), (0.0, 0.6, -0.8), atol=1e-6)
    assert t2[1, 16:24].tolist() == [4.0, 5.0, 6.0, 0.0, 0.0, 2.0, 0.0, 0.0]
    assert [(l.name, l.kind) for l in scene.current_lights()] == [("emit-Light", "point"), ("emit-SunA", "directional")]
    # ff.Scene lists it among the lights whatever its id says ("emit-SunA" holds neither "light" nor "spot"), behind the main spot
    names = [l.name() for l in ff.Scene(params, device="cpu").lights()]
    assert names == ["emit-Spot", "emit-Light", "emit-SunA"], names
    # a scene without a sun says so
    sc2 = ss.corner()
    sc2.lights = [ls.POINT]
    assert mi.load_scene_data(sc2, device="cpu", shadows=True).lights_directional() is False


# ------------------------------------------------------------------ 6. ref_sun's own identities in float64
def _row(sun):
    return rs.table_row(sun.to_world, sun.intensity)


@pytest.mark.parametrize("gaussian", [False, True])
def test_the_closed_form_on_the_quad_that_fills_the_film(gaussian):
    want = ss.quad_closed_form()
    stddev = 0.5 if gaussian else None
    sd, world, alb = arrays(ss.quad())
    img = rs.render_sun(*world, sd, alb, [_row(ss.SUN_Q)], 4, 3, gaussian_stddev=stddev)
    rel = np.abs(img - want) / want
    print("quad, gaussian", gaussian, ": max relative error", rel.max())
    assert img.shape == (24, 24, 3) and rel.max() <= 1e-6
    # under a roof the camera does not see: every shadow ray hits it; with bit 0 of `shadows` cleared the closed form is back
    sd, world, alb = arrays(ss.quad(roof=True))
    st = {}
    dark = rs.render_sun(*world, sd, alb, [_row(ss.SUN_Q)], 4, 3, gaussian_stddev=stddev, stats=st)
    assert (dark == 0.0).all() and st[0]["occluded"] == st[0]["faces"] == 24 * 24 * 4
    sd.shadows &= ~1
    lit = rs.render_sun(*world, sd, alb, [_row(ss.SUN_Q)], 4, 3, gaussian_stddev=stddev)
    assert (np.abs(lit - want) / want).max() <= 1e-6
    # a frame without a +Z, and one that is not finite, light nothing; the translation is not read
    for bad in (np.zeros((4, 4)), np.diag([1.0, 1.0, 0.0, 1.0]), np.full((4, 4), np.nan)):
        assert (rs.render_sun(*world, sd, alb, [rs.table_row(bad, (1.0, 1.0, 1.0))], 1, 3) == 0.0).all()
    moved = np.asarray(ss.SUN_Q.to_world, np.float64).copy()
    moved[:3, 3] = (50.0, -70.0, 2.0)
    moved[:3, :3] *= 7.0  # (nor does the frame's scale count: the direction is normalised)
    np.testing.assert_allclose(rs.render_sun(*world, sd, alb, [rs.table_row(moved, ss.SUN_Q.intensity)], 4, 3, gaussian_stddev=stddev), lit, rtol=1e-12)


@pytest.mark.parametrize("sun", [ss.SUN_A, ss.SUN_B], ids=["A", "B"])
def test_the_sun_is_the_limit_of_a_point_light(sun):
    """shadows off, D = 1e6 r: the point light of intensity E D^2 at c - D dir against the sun, to 4 r / D of the part's maximum — the direction and the
    cosine each move by at most r / D, and D^2 / d^2 by 2 r / D (|d - D| <= r).  Lambert rows: the derivation takes the radiance to depend on the
    direction through the cosine alone (a specular lobe's slope in the direction is a multiple of its value)"""
    sd, world, mats = arrays(ss.corner("21x19"))
    sd.shadows &= ~1
    D = 1.0e6 * ss.RADIUS
    tw = np.eye(4)
    tw[:3, 3] = ss.CENTRE - D * rs.direction(_row(sun))  # (in float64: a float32 position at this distance is good to 0.1)
    a = rs.render_sun(*world, sd, mats, [_row(sun)], 4, 7, max_depth=3)
    b = rl.render_lights(*world, sd, mats, [rl.table_row("point", tw, np.asarray(sun.intensity, np.float64) * D * D)], 4, 7, max_depth=3)
    err = np.abs(a - b).max() / a.max()
    print(sun.name, ": max |sun - far point| / max", err, "bound", 4 * ss.RADIUS / D)
    assert a.max() > 0 and err <= 4 * ss.RADIUS / D


def test_linearity_in_float64():
    sd, world, alb = arrays(ss.corner("21x19"))
    t = ops.pack_lights([ls.POINT, ls.SPOT_B, ss.SUN_A]).numpy().astype(np.float64)
    all3 = rs.render_sun(*world, sd, alb, t, 4, 3, max_depth=3)
    parts = [rs.render_sun(*world, sd, alb, t[k:k + 1], 4, 3, max_depth=3) for k in range(3)]
    assert all(p.mean() > 0 for p in parts)
    np.testing.assert_allclose(all3, sum(parts), rtol=1e-12, atol=1e-12 * all3.max())
    np.testing.assert_allclose(parts[0] + parts[1], rl.render_lights(*world, sd, alb, t[:2], 4, 3, max_depth=3), rtol=1e-12, atol=1e-12 * all3.max())
    dark = t[2:3].copy()
    dark[:, 16:19] = 0.0
    assert (rs.render_sun(*world, sd, alb, dark, 4, 3, max_depth=3) == 0.0).all()


# ------------------------------------------------------------------ the preconditions of tests/test_sun_gpu.py's comparisons
@pytest.mark.parametrize("film", sorted(ss.FILMS))
@pytest.mark.parametrize("principled", [False, True])
def test_the_suns_matter_in_the_scenes_of_the_gpu_tests(film, principled):
    sc = ss.corner(film, principled)
    sd, world, mats = arrays(sc, principled)
    spp, seed = 16, 7
    main = rp.render_fwd(*world, sd, mats, host_tex(sc), spp, seed, 2)
    for sun in (ss.SUN_A, ss.SUN_B):
        st = {}
        part = rs.render_sun(*world, sd, mats, [_row(sun)], spp, seed, stats=st)
        share = part.mean() / (main + part).mean()
        occ = st[0]["occluded"] / st[0]["faces"]
        print(film, principled, sun.name, "share of the image's mean", share, "occluded share of the samples that face it", occ)
        assert share > 0.05
        if sun is ss.SUN_B:  # (SUN_A's only shadow at the primary hit, the cube's, lies behind the cube as the camera sees it)
            assert 0.05 < occ < 0.95


def test_sun_b_leaves_the_walls_dark_and_its_shadow_strip_holds_lit_and_unlit_floor():
    sc = ss.corner("24x24")
    sd, world, alb = arrays(sc)
    verts, tri_idx, tri_shape = world
    L = rs.sample_radiance(*world, sd, alb, [_row(ss.SUN_B)], 1, 7, use_jitter=False)
    from tests import ref_bruteforce as bf

    o, d, nt, ft = bf.camera_rays(sd.cam, 1, False, 7)
    t, prim = bf.intersect(o, d, bf.world_triangles(verts, tri_idx), nt, ft)
    shape = np.where(prim >= 0, np.asarray(tri_shape)[np.maximum(prim, 0)], -1)
    P = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d
    lit = L.sum(1) > 0
    names = [m.name for m in sc.meshes]
    floor, wall_x, wall_y = (shape == names.index(n) for n in ("mesh-Floor", "mesh-WallX", "mesh-WallY"))
    assert wall_x.sum() > 20 and wall_y.sum() > 20 and not lit[wall_x].any() and not lit[wall_y].any()  # (it faces neither wall)
    # the top edge of wall y = 0 shadows the floor up to y = 1.5 (where the ray towards the sun still meets the wall: x - 0.2 y / 0.75 >= 0)
    strip = floor & (P[:, 1] < 1.45) & (P[:, 0] - 0.2 * P[:, 1] / 0.75 > 0.05)
    beyond = floor & (P[:, 1] > 1.55)
    print("floor samples: in the strip", int(strip.sum()), "lit", int(lit[strip].sum()), "; beyond it", int(beyond.sum()), "lit", int(lit[beyond].sum()))
    assert strip.sum() >= 10 and not lit[strip].any()
    assert beyond.sum() >= 10 and lit[beyond].sum() >= 0.5 * beyond.sum()  # (the cube shadows some)


def test_bounces_carry_the_suns_light():
    sd, world, alb = arrays(ss.corner("24x24"))
    st = {}
    L = rs.sample_radiance(*world, sd, alb, [_row(ss.SUN_A)], 16, 7, max_depth=3, stats=st)
    direct = st["direct"].sum()
    print("indirect / direct of SUN_A at max_depth 3:", (L.sum() - direct) / direct, st[0])
    assert L.sum() - direct > 0.05 * direct > 0
    assert st[0]["occluded"] > 0  # (some bounce vertices meet the cube's shadow, which the camera does not see)
