"""The constant emitter without a GPU: the header's macros against _abi, the [table | lights | ambient] buffer, the refusals of
FFX_RENDER_AMBIENT that come before any launch, the loader, the record mi.Scene forms from its parameter map, tests/ref_ambient.py's own identities, and
— on ref_ambient alone — the preconditions of the comparisons tests/test_ambient_gpu.py makes."""
import types

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, scenes
from tests import ambient_scenes as am
from tests import ref_ambient as ra
from tests import ref_path as rp
from tests import refusals
from tests.support import FFX_ERR_ARG, FFX_ERR_UNSUPPORTED, arrays, define, header, host_tex, independent, load_xml


# ------------------------------------------------------------------ header and ABI
def test_the_headers_macros_equal_abis_and_the_abi_version_stays():
    assert define("FFX_ABI_VERSION") == 11
    assert define("FFX_RENDER_AMBIENT") == _abi.RENDER_AMBIENT == 0x2000000 == 1 << 25
    assert define("FFX_AMBIENT_FLOATS") == _abi.AMBIENT_FLOATS == 4
    taken = (_abi.RENDER_FP16 | _abi.RENDER_SPARSE_ADJOINT | _abi.RENDER_APEX_READY | _abi.RENDER_CACHE_ZEROED | _abi.RENDER_CACHE_KEEP_DROPPED | _abi.RENDER_PATH_MASK
             | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL | _abi.RENDER_GRAD_PRB | _abi.RENDER_TANGENT | _abi.RENDER_AOV | _abi.RENDER_LIGHTS_MASK)
    assert _abi.RENDER_AMBIENT & taken == 0
    # no other flag word of the header's render calls uses bit 25
    import re

    words = {n: int(v, 16) for n, v in re.findall(r"#define (FFX_RENDER_\w+) (0x[0-9a-fA-F]+)\b", header())}
    assert len(words) >= 6 and words.pop("FFX_RENDER_AMBIENT") == 1 << 25
    assert not [n for n, v in words.items() if v & (1 << 25)], words


# ------------------------------------------------------------------ packing
def test_pack_ambient_and_the_buffer_behind_the_lights():
    rec = ops.pack_ambient((0.25, 0.5, 2.0))
    assert rec.dtype == torch.float32 and rec.tolist() == [0.25, 0.5, 2.0, 0.0]
    assert ops.pack_ambient(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)).tolist() == [1.0, 2.0, 3.0, 0.0]
    assert ops.pack_ambient(scenes.AmbientData("w", (3.0, 2.0, 1.0))).tolist() == [3.0, 2.0, 1.0, 0.0]
    assert ops.pack_ambient(None) is None
    with pytest.raises(ValueError, match="three floats"):
        ops.pack_ambient((1.0, 2.0))
    # DeviceGeometry._with_lights on a stand-in that has what it reads (the device): [table | lights | ambient], the bits, with and without lights
    geom = types.SimpleNamespace(device=torch.device("cpu"))
    sd = _abi.SceneDesc()
    sd.n_shapes, sd.mat_stride = 2, 0
    rows = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    lights = torch.arange(48, dtype=torch.float32).reshape(2, 24) + 100.0
    seen = {}
    orig = ops._dev
    try:
        ops._dev = lambda t, *a, **k: seen.setdefault("buf", t)
        _, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights, "test", (0.25, 0.5, 2.0))
        assert bits == _abi.render_lights(2) | _abi.RENDER_AMBIENT
        assert buf.tolist() == rows.reshape(-1).tolist() + lights.reshape(-1).tolist() + [0.25, 0.5, 2.0, 0.0]
        _, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", None, "test", (0.25, 0.5, 2.0))
        assert bits == _abi.RENDER_AMBIENT and buf.tolist() == rows.reshape(-1).tolist() + [0.25, 0.5, 2.0, 0.0]
        _, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, None, "mats", lights[:0], "test", torch.tensor([1.0, 1.0, 1.0]))  # (rows in the description)
        assert bits == _abi.RENDER_AMBIENT and buf.tolist() == [0.0] * 6 + [1.0, 1.0, 1.0, 0.0]
        arg, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", None, "test", None)  # (neither: the call as it was)
        assert (arg, bits, buf) == ("mats", 0, None)
        _, bits, buf = ops.DeviceGeometry._with_lights(geom, sd, rows, "mats", lights, "test")
        assert bits == _abi.render_lights(2) and buf.numel() == 6 + 48
    finally:
        ops._dev = orig


# ------------------------------------------------------------------ refusals (tests/refusals.py's set-up)
_A, _L1 = _abi.RENDER_AMBIENT, _abi.render_lights(1)
_ONLY = "FFX_RENDER_AMBIENT is served by ffx_render_fwd[_filtered] only"
_GRAD = "FFX_RENDER_AMBIENT is not served together with a FFX_RENDER_GRAD_* bit"
_REFUSALS = [
    ("ffx_render_fwd", _A | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_AMBIENT has no fp16 film"),
    ("ffx_render_fwd_filtered", _A | _L1 | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: FFX_RENDER_AMBIENT has no fp16 film"),
    ("ffx_render_fwd", _A | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_AMBIENT is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd_filtered", _A | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "FFX_RENDER_AMBIENT is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd", _A | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_fwd: " + _GRAD),
    ("ffx_render_fwd_filtered", _A | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: " + _GRAD),
    ("ffx_render_fwd", _A | _abi.RENDER_GRAD_PRB, {}, FFX_ERR_UNSUPPORTED, _GRAD),
    ("ffx_render_bwd", _A | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_bwd: " + _GRAD),
    ("ffx_render_bwd", _A | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED, "render_bwd: " + _GRAD),
    ("ffx_render_bwd_filtered", _A | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_PRB | _abi.render_path(3, 5), {}, FFX_ERR_UNSUPPORTED, "render_bwd_filtered: " + _GRAD),
    ("ffx_render_fwd_cache", _A, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache: " + _ONLY),
    ("ffx_render_fwd_cache_filtered", _A, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: " + _ONLY),
    ("ffx_render_fwd_adjoint", _A, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint: " + _ONLY),
    ("ffx_render_fwd_adjoint_filtered", _A, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint_filtered: " + _ONLY),
    ("ffx_render_bwd_det", _A, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det: " + _ONLY),
    ("ffx_render_bwd_det_part", _A, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det_part: " + _ONLY),
    ("ffx_render_fwd", _A, {"mats": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_AMBIENT needs the device buffer [material table | lights | ambient] (shape_albedo is NULL)"),
    ("ffx_render_fwd_filtered", _A | _abi.RENDER_AOV, {"mats": None}, FFX_ERR_ARG, "FFX_RENDER_AMBIENT needs the device buffer"),
    # served — with lights and an AOV block — and accepted by the adjoint without a FFX_RENDER_GRAD_* bit: the calls get as far as the last
    # refusal in front of the launches
    ("ffx_render_fwd", _A, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_fwd", _A | _abi.render_lights(8), {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_fwd", _A | _abi.RENDER_AOV, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_bwd", _A, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
    ("ffx_render_bwd_filtered", _A | _L1, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
]


@pytest.mark.parametrize("case", _REFUSALS, ids=lambda c: f"{c[0][4:]}-{c[1]:#x}-{'nomats' if c[2] else 'mats'}")
def test_the_bit_is_refused_before_any_launch(case, monkeypatch):
    """tests/refusals.py's set-up (nothing can launch), with this suite's own default: no dot_out / loss_slots buffer"""
    name, flags, arg_changes, rc, msg = case
    got, err = refusals.call(name, refusals.GAUSS if "filtered" in name else {}, {"flags": flags, "dot": None, **arg_changes}, monkeypatch=monkeypatch)
    assert got == rc, (got, err)
    assert msg in err, err


def test_the_python_layers_refuse_what_the_library_would():
    geom = types.SimpleNamespace(device=torch.device("cpu"))
    sd = _abi.SceneDesc()
    with pytest.raises(ValueError, match="constant emitter.*fp32 film"):
        ops.DeviceGeometry.render_fwd(geom, sd, None, None, 4, fp16=True, ambient=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="constant emitter.*without an adjoint cache"):
        ops.DeviceGeometry.render_fwd(geom, sd, None, None, 4, cache=torch.zeros(8, dtype=torch.uint8), ambient=(1.0, 1.0, 1.0))
    with pytest.raises(NotImplementedError, match="constant emitter.*not differentiated"):
        ops.DeviceGeometry.render_bwd(geom, sd, None, 4, 0, None, appearance=True, ambient=(1.0, 1.0, 1.0))
    from fireflies_amd import functional as Fn

    with pytest.raises(ValueError, match="constant emitter.*no fp16 film"):
        Fn.render(torch.zeros(2, 2), geom, sd, None, 4, fp16=True, ambient=(1.0, 1.0, 1.0))


# ------------------------------------------------------------------ the loader
def test_the_loader_reads_the_constant_emitter(tmp_path):
    sc, reports = load_xml(am.write_scene(tmp_path))
    print(reports)
    assert isinstance(sc.ambient, scenes.AmbientData) and sc.ambient.name == "emit-World" and sc.ambient.radiance == (0.8, 1.0, 1.3)
    assert sc.spot is not None and sc.projector is not None and sc.lights == []
    assert not any("constant" in r for r in reports), reports
    # a single float; an emitter without id or radiance: Mitsuba's default radiance 1
    sc1, r1 = load_xml(am.write_scene(tmp_path, am.XML.replace(am.WORLD, '<emitter type="constant" id="sky"><float name="radiance" value="0.25"/></emitter>'), "f.xml"))
    assert sc1.ambient.name == "sky" and sc1.ambient.radiance == (0.25, 0.25, 0.25) and not any("constant" in r for r in r1)
    sc2, _ = load_xml(am.write_scene(tmp_path, am.XML.replace(am.WORLD, '<emitter type="constant"/>'), "d.xml"))
    assert sc2.ambient.name == "emit-Constant" and sc2.ambient.radiance == (1.0, 1.0, 1.0)
    # an unknown property is reported as for the other emitters
    _, r3 = load_xml(am.write_scene(tmp_path, am.XML.replace(am.WORLD, '<emitter type="constant" id="w"><rgb name="radiance" value="1"/><float name="scale" value="2"/></emitter>'),
                                 "p.xml"))
    assert any("constant emitter property 'scale' is ignored" in r for r in r3), r3


def test_a_second_constant_emitter_is_reported_once_and_ignored(tmp_path):
    more = "".join(f'<emitter type="constant" id="second-{k}"><rgb name="radiance" value="9"/></emitter>' for k in range(2))
    sc, reports = load_xml(am.write_scene(tmp_path, am.XML.replace("</scene>", more + "</scene>"), "two.xml"))
    assert sc.ambient.name == "emit-World" and sc.ambient.radiance == (0.8, 1.0, 1.3)
    told = [r for r in reports if "second constant emitter" in r]
    assert len(told) == 1 and "second-0" in told[0], reports


def test_envmap_and_area_emitters_stay_reported_and_a_file_without_the_emitter_is_unchanged(tmp_path):
    xml = am.XML.replace(am.WORLD, '<emitter type="envmap" id="sky"><string name="filename" value="e.exr"/></emitter>')
    xml = xml.replace('</bsdf></shape>', '</bsdf><emitter type="area"><rgb name="radiance" value="1"/></emitter></shape>', 1)
    sc, reports = load_xml(am.write_scene(tmp_path, xml, "env.xml"))
    assert sc.ambient is None
    assert any("emitter type 'envmap' ignored" in r for r in reports), reports
    assert any("area emitter on a shape ignored" in r for r in reports), reports
    plain, r0 = load_xml(am.write_scene(tmp_path, am.XML.replace(am.WORLD, ""), "plain.xml"))
    with_w, r1 = load_xml(am.write_scene(tmp_path))
    assert plain.ambient is None and with_w.ambient is not None and r0 == [r.replace("ambient.xml", "plain.xml") for r in r1]
    assert np.array_equal(plain.spot.to_world, with_w.spot.to_world) and plain.spot.intensity == with_w.spot.intensity
    assert (plain.projector_scale, plain.lights, len(plain.meshes)) == (with_w.projector_scale, with_w.lights, len(with_w.meshes))
    assert list(scenes.SceneData.__dataclass_fields__)[-1] == "ambient"  # (last: constructors pass by position)


# ------------------------------------------------------------------ mi.Scene's record (a Scene itself needs a device: tests/test_ambient_gpu.py has the map)
def test_the_ambient_record_follows_the_parameter_map():
    params = {"emit-World.radiance.value": mi.Color3f(torch.tensor([0.8, 1.0, 1.3]))}
    stub = types.SimpleNamespace(_ambient_name="emit-World", _ambient_dev=None, _params=params, device=torch.device("cpu"))
    rec = mi.Scene.ambient_record(stub)
    assert rec.dtype == torch.float32 and rec.tolist() == torch.tensor([0.8, 1.0, 1.3]).tolist()
    assert mi.Scene.ambient_record(stub) is rec  # (kept until an update touches the key)
    params["emit-World.radiance.value"] = mi.Color3f(torch.tensor([2.0, 2.0, 2.0]))
    stub._ambient_dev = None  # (what _apply does for a dirty key of the emitter)
    assert mi.Scene.ambient_record(stub).tolist() == [2.0, 2.0, 2.0]
    params["emit-World.radiance.value"] = 0.5  # (a plain float: a grey world)
    stub._ambient_dev = None
    assert mi.Scene.ambient_record(stub).tolist() == [0.5, 0.5, 0.5]
    assert mi.Scene.ambient_record(types.SimpleNamespace(_ambient_name=None)) is None


# ------------------------------------------------------------------ ref_ambient's own identities
@pytest.mark.parametrize("gaussian", [False, True])
def test_the_closed_forms(gaussian):
    """one Lambert quad that fills the film at max_depth 2: every closing ray escapes and f is the base colour — every pixel base x L_a; the camera turned
    away: every pixel L_a"""
    La, std = np.array([0.8, 1.0, 1.3]), 0.5 if gaussian else None
    sd, world, alb = arrays(am.quad())
    parts = {}
    img = ra.render_ambient(*world, sd, alb, La, 4, 3, gaussian_stddev=std, parts=parts)
    np.testing.assert_allclose(img, np.broadcast_to(np.asarray(am.QUAD_RGB, np.float32).astype(np.float64) * La, img.shape), rtol=1e-12)
    assert parts["closing"] == parts["escaped"] == 24 * 24 * 4 and parts[0].sum() == 0.0
    sd, world, alb = arrays(am.quad(away=True))
    parts = {}
    img = ra.render_ambient(*world, sd, alb, La, 4, 3, gaussian_stddev=std, parts=parts)
    np.testing.assert_allclose(img, np.broadcast_to(La, img.shape), rtol=1e-12)
    assert parts["closing"] == 0 and parts["escaped"] == 24 * 24 * 4


def test_the_term_of_a_vertex_does_not_depend_on_max_depth_and_the_part_is_linear():
    sd, world, alb = arrays(am.corner("21x19"))
    p2, p3, p4 = {}, {}, {}
    L2 = ra.sample_radiance(*world, sd, alb, am.RADIANCE, 4, 3, max_depth=2, rr_depth=99, parts=p2)
    L3 = ra.sample_radiance(*world, sd, alb, am.RADIANCE, 4, 3, max_depth=3, rr_depth=99, parts=p3)
    ra.sample_radiance(*world, sd, alb, am.RADIANCE, 4, 3, max_depth=4, rr_depth=99, parts=p4)
    assert p2[1].sum() > 0 and p3[2].sum() > 0 and p2[0].sum() > 0
    # the closing ray at the primary hit (max_depth 2) is the walk's own bounce ray at max_depth 3, seen escaping
    np.testing.assert_array_equal(p2[0], p3[0])
    np.testing.assert_allclose(p2[1], p3[1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(p3[2], p4[2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(L3 - L2, p3[2], rtol=1e-12, atol=1e-15)
    twice = ra.sample_radiance(*world, sd, alb, 2.0 * np.asarray(am.RADIANCE), 4, 3, max_depth=3)
    np.testing.assert_allclose(twice, 2.0 * ra.sample_radiance(*world, sd, alb, am.RADIANCE, 4, 3, max_depth=3), rtol=1e-12)


def test_the_roulette_on_the_closing_ray_keeps_the_mean():
    """rr_depth 1: every bounce — the closing one too — survives with q = min(max beta f, 0.95) and is divided by q; over many samples the part's sum
    is that without roulette (an unbiased estimator: 3 % at 21 x 19 x 64 samples), and the kept samples are fewer"""
    sd, world, alb = arrays(am.corner("21x19"))
    on, off = {}, {}
    a = ra.sample_radiance(*world, sd, alb, am.RADIANCE, 64, 5, max_depth=2, rr_depth=1, parts=on)
    b = ra.sample_radiance(*world, sd, alb, am.RADIANCE, 64, 5, max_depth=2, rr_depth=99, parts=off)
    print("closing rays with / without roulette", on["closing"], off["closing"], "sums", a.sum(), b.sum())
    assert on["closing"] < 0.9 * off["closing"]
    assert abs(a.sum() - b.sum()) <= 0.03 * b.sum()


# ------------------------------------------------------------------ the preconditions of tests/test_ambient_gpu.py's comparisons
@pytest.mark.parametrize("film", sorted(am.FILMS))
@pytest.mark.parametrize("principled", [False, True])
def test_the_ambient_part_matters_and_single_precision_stays_inside_the_caps(film, principled):
    """the part under test is well above zero in the scenes of the GPU tests, at every depth they use, on both films; and the same statement with every
    ray, point and weight rounded to float32 stays inside the three caps the GPU comparison is held to"""
    sc = am.corner(film, principled)
    sd, world, mats = arrays(sc, principled)
    spp, seed = 16, 7
    for depth, rr in ((2, 5), (3, 5), (4, 5), (4, 1)):
        main = rp.render_fwd(*world, sd, mats, host_tex(sc), spp, seed, depth, rr)
        for std in (None, 0.5):
            parts = {}
            part = ra.render_ambient(*world, sd, mats, am.RADIANCE, spp, seed, depth, rr, gaussian_stddev=std, parts=parts)
            share = part.mean() / (main.mean() + part.mean())
            print(film, principled, depth, rr, std, "share of the image's mean", share, "closing", parts["closing"], "escaped", parts["escaped"])
            assert share > 0.05 and 0 < parts["escaped"] and parts["closing"] > 0
            single = ra.render_ambient(*world, sd, mats, am.RADIANCE, spp, seed, depth, rr, gaussian_stddev=std, round32=True)
            independent(f"{film} principled={principled} depth {depth} rr {rr} gaussian={std is not None}: float32-rounded against float64", single, part,
                        float((main + part).max()), float(part.sum()))
