"""Extra emitters without a GPU: the header's macros against _abi, the loader's point lights and further spots, ops.pack_lights' layout,
the refusals of FFX_RENDER_LIGHTS that come before any launch, tests/ref_lights.py against closed forms, and — on ref_lights alone — the preconditions of
the comparisons tests/test_lights_gpu.py makes."""
import re

import numpy as np
import pytest

from fireflies_amd import _abi, ops, scene_desc, scenes
from tests import light_scenes as ls
from tests import ref_lights as rl
from tests import ref_path as rp
from tests import refusals
from tests.support import FFX_ERR_ARG, FFX_ERR_UNSUPPORTED, define, header, host_tex, load_xml, world_arrays


# ------------------------------------------------------------------ header and ABI
def test_the_headers_macros_equal_abis_and_the_abi_version_stays():
    assert define("FFX_ABI_VERSION") == 11
    assert define("FFX_RENDER_MAX_LIGHTS") == _abi.RENDER_MAX_LIGHTS == 8 == scenes.MAX_EXTRA_LIGHTS
    assert define("FFX_RENDER_LIGHTS_SHIFT") == _abi.RENDER_LIGHTS_SHIFT == 21
    assert define("FFX_RENDER_LIGHTS_MASK") == _abi.RENDER_LIGHTS_MASK == 0x1E00000 == 15 << 21
    assert define("FFX_LIGHT_FLOATS") == _abi.LIGHT_FLOATS == 24
    assert (define("FFX_LIGHT_POINT"), define("FFX_LIGHT_SPOT")) == (_abi.LIGHT_POINT, _abi.LIGHT_SPOT) == (0, 1)
    assert re.search(r"#define FFX_RENDER_LIGHTS\(n\) \(\(\(n\) & 15\) << FFX_RENDER_LIGHTS_SHIFT\)", header())
    assert [_abi.render_lights(n) for n in (0, 1, 8)] == [0, 1 << 21, 8 << 21]
    taken = (_abi.RENDER_FP16 | _abi.RENDER_SPARSE_ADJOINT | _abi.RENDER_APEX_READY | _abi.RENDER_CACHE_ZEROED | _abi.RENDER_CACHE_KEEP_DROPPED | _abi.RENDER_PATH_MASK
             | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL | _abi.RENDER_GRAD_PRB | _abi.RENDER_TANGENT | _abi.RENDER_AOV)
    assert _abi.RENDER_LIGHTS_MASK & taken == 0


def test_the_header_declares_no_function_that_the_prototypes_lack():
    declared = set(re.findall(r"^\s*(?:[A-Za-z_][\w \*]*?)\b(ffx_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header(), flags=re.S), re.M))
    declared = {d for d in declared if not re.search(r"typedef[^;]*\b" + d + r"\b", header())}
    assert len(declared) > 40
    assert declared <= set(_abi.PROTOTYPES), sorted(declared - set(_abi.PROTOTYPES))


# ------------------------------------------------------------------ the loader
def test_point_lights_and_further_spots_are_kept_in_file_order(tmp_path):
    sc, reports = load_xml(ls.write_scene(tmp_path))
    assert sc.spot is not None and sc.spot.name == "emit-Spot" and sc.spot.intensity == (8.0, 8.0, 8.0) and sc.spot.cutoff_angle == 30.0
    assert [(l.name, l.kind) for l in sc.lights] == [("emit-Light", "point"), ("emit-PointLight", "point"), ("emit-SecondSpot", "spot")]
    a, b, s2 = sc.lights
    np.testing.assert_allclose(np.asarray(a.to_world)[:3, 3], (1.0, -0.5, 3.5))  # (a <point name="position">)
    np.testing.assert_allclose(np.asarray(b.to_world)[:3, 3], (0.5, 1.5, 1.0))  # (the translation of to_world)
    assert a.intensity == (20.0, 18.0, 15.0) and b.intensity == (2.0, 2.0, 2.0)
    np.testing.assert_allclose(np.asarray(s2.to_world), np.asarray(ls.SPOT_B.to_world), rtol=1e-6, atol=1e-6)
    assert (s2.intensity, s2.cutoff_angle, s2.beam_width) == ((6.0, 9.0, 12.0), 35.0, 22.0)
    print(reports)
    assert not any("point" in r for r in reports), reports
    # the default intensity of a point light is 1
    sc1, _ = load_xml(ls.write_scene(tmp_path, ls.with_extra_points(1), "one.xml"))
    assert sc1.lights[-1].intensity == (1.0, 1.0, 1.0) and np.allclose(np.asarray(sc1.lights[-1].to_world)[:3, 3], (0.0, 1.0, 2.0))


def test_beyond_eight_extra_lights_the_rest_are_reported_once_and_dropped(tmp_path):
    sc, reports = load_xml(ls.write_scene(tmp_path, ls.with_extra_points(7), "ten.xml"))  # 3 + 7 = 10 extra emitters
    assert len(sc.lights) == 8 and [l.name for l in sc.lights[:3]] == ["emit-Light", "emit-PointLight", "emit-SecondSpot"] and sc.lights[-1].name == "emit-More4"
    told = [r for r in reports if "dropped" in r and "emitters" in r]
    assert len(told) == 1, reports


def test_the_pinned_reports_keep_their_wording(tmp_path):
    xml = ls.XML.replace("</scene>", '<emitter type="envmap" id="env"/></scene>')
    _, reports = load_xml(ls.write_scene(tmp_path, xml, "env.xml"))
    assert any("emitter type 'envmap' ignored" in r for r in reports), reports


# ------------------------------------------------------------------ packing
def test_pack_lights_matches_the_layout_word_for_word():
    t = ops.pack_lights([ls.POINT, ls.SPOT_B]).numpy()
    assert t.shape == (2, 24) and t.dtype == np.float32
    for row, l in zip(t, (ls.POINT, ls.SPOT_B)):
        np.testing.assert_array_equal(row[:16], np.asarray(l.to_world, np.float32).reshape(16))
        np.testing.assert_array_equal(row[16:19], np.asarray(l.intensity, np.float32))
        assert (row[19], row[20]) == (np.float32(l.cutoff_angle), np.float32(l.beam_width))
        assert row[21] == (1.0 if l.kind == "spot" else 0.0) and (row[22], row[23]) == (0.0, 0.0)
    assert tuple(ops.pack_lights([]).shape) == (0, 24)
    with pytest.raises(ValueError, match="at most 8"):
        ops.pack_lights([ls.POINT] * 9)
    with pytest.raises(ValueError, match="kind"):
        scenes.LightData("x", "area", np.eye(4))
    np.testing.assert_array_equal(rl.table_row("spot", ls.SPOT_B.to_world, ls.SPOT_B.intensity, 35.0, 22.0).astype(np.float32), t[1])


# ------------------------------------------------------------------ refusals (tests/refusals.py's set-up)
_L1, _L8, _L9 = _abi.render_lights(1), _abi.render_lights(8), _abi.render_lights(9)
_ONLY = "FFX_RENDER_LIGHTS is served by ffx_render_fwd[_filtered] only"
_GRAD = "FFX_RENDER_LIGHTS is not served together with a FFX_RENDER_GRAD_* bit"
_REFUSALS = [
    ("ffx_render_fwd", _L1 | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_LIGHTS has no fp16 film"),
    ("ffx_render_fwd_filtered", _L8 | _abi.RENDER_FP16, {}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: FFX_RENDER_LIGHTS has no fp16 film"),
    ("ffx_render_fwd", _L1 | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "render_fwd: FFX_RENDER_LIGHTS is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd_filtered", _L1 | _abi.RENDER_TANGENT, {}, FFX_ERR_UNSUPPORTED, "FFX_RENDER_LIGHTS is not served together with FFX_RENDER_TANGENT"),
    ("ffx_render_fwd", _L1 | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_fwd: " + _GRAD),
    ("ffx_render_fwd_filtered", _L1 | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: " + _GRAD),
    ("ffx_render_fwd", _L1 | _abi.RENDER_GRAD_PRB, {}, FFX_ERR_UNSUPPORTED, _GRAD),
    ("ffx_render_bwd", _L1 | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_bwd: " + _GRAD),
    ("ffx_render_bwd", _L1 | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED, "render_bwd: " + _GRAD),
    ("ffx_render_bwd_filtered", _L1 | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_PRB | _abi.render_path(3, 5), {}, FFX_ERR_UNSUPPORTED, "render_bwd_filtered: " + _GRAD),
    ("ffx_render_fwd_cache", _L1, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache: " + _ONLY),
    ("ffx_render_fwd_cache_filtered", _L1, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: " + _ONLY),
    ("ffx_render_fwd_adjoint", _L1, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint: " + _ONLY),
    ("ffx_render_fwd_adjoint_filtered", _L1, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint_filtered: " + _ONLY),
    ("ffx_render_bwd_det", _L1, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det: " + _ONLY),
    ("ffx_render_bwd_det_part", _L1, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det_part: " + _ONLY),
    ("ffx_render_fwd", _L9, {}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_LIGHTS(9): at most 8 extra emitters"),
    ("ffx_render_fwd_filtered", _abi.render_lights(15), {}, FFX_ERR_ARG, "render_fwd_filtered: FFX_RENDER_LIGHTS(15): at most 8 extra emitters"),
    ("ffx_render_fwd", _L1, {"mats": None}, FFX_ERR_ARG, "render_fwd: FFX_RENDER_LIGHTS needs the device buffer [material table | lights] (shape_albedo is NULL)"),
    ("ffx_render_fwd", _L1 | _abi.RENDER_AOV, {"mats": None}, FFX_ERR_ARG, "FFX_RENDER_LIGHTS needs the device buffer"),
    # served, and accepted by the adjoint without a FFX_RENDER_GRAD_* bit: the calls get as far as the last refusal in front of the launches
    ("ffx_render_fwd", _L8, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_fwd", _L1 | _abi.RENDER_AOV, {}, FFX_ERR_ARG, "render_fwd: blob without per-slot normals"),
    ("ffx_render_bwd", _L8, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
    ("ffx_render_bwd_filtered", _L1, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
]


@pytest.mark.parametrize("case", _REFUSALS, ids=lambda c: f"{c[0][4:]}-{c[1]:#x}-{'nomats' if c[2] else 'mats'}")
def test_the_bits_are_refused_before_any_launch(case, monkeypatch):
    """tests/refusals.py's set-up (nothing can launch), with this suite's own default: no dot_out / loss_slots buffer"""
    name, flags, arg_changes, rc, msg = case
    got, err = refusals.call(name, refusals.GAUSS if "filtered" in name else {}, {"flags": flags, "dot": None, **arg_changes}, monkeypatch=monkeypatch)
    assert got == rc, (got, err)
    assert msg in err, err


# ------------------------------------------------------------------ ref_lights against closed forms
QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _plane_scene(occluder):
    plane = np.array([[-4, -4, 0], [4, -4, 0], [4, 4, 0], [-4, 4, 0]], np.float32)[None]
    meshes = [scenes.MeshData("mesh-Plane", plane, QUAD, (0.75, 0.5, 0.25))]  # (albedos that a float32 table holds exactly)
    if occluder:
        q = np.array([[-0.3, -0.3, 1.5], [0.3, -0.3, 1.5], [0.3, 0.3, 1.5], [-0.3, 0.3, 1.5]], np.float32)[None]
        meshes.append(scenes.MeshData("mesh-Occluder", q, QUAD, (0.25, 0.875, 0.5)))
    cam = scenes.SensorData("cam", scenes.look_at((0.2, -0.1, 4.0), (0.2, -0.1, 0.0), up=(0, 1, 0)), 50.0, 0.05, 100.0, 13, 11)
    return scenes.SceneData(meshes, cam)


def _plane_closed_form(sc, light_pos, inten, occluder):
    """per sample (un-jittered, 1 spp): albedo / pi I cos / d^2 at the ray's point on the occluder quad (z = 1.5, |x|, |y| <= 0.3) or the plane z = 0;
    -> (values [N,3], the plane samples whose segment to the light crosses the quad's interior)"""
    sd = scene_desc.scene_desc(sc, shadows=True)
    from tests import ref_bruteforce as bf

    o, d, _, _ = bf.camera_rays(sd.cam, 1, False, 0)
    L, inten = np.asarray(light_pos, np.float64), np.asarray(inten, np.float64)
    P0 = o + ((0.0 - o[:, 2]) / d[:, 2])[:, None] * d
    P1 = o + ((1.5 - o[:, 2]) / d[:, 2])[:, None] * d
    on_quad = occluder & (np.abs(P1[:, 0]) <= 0.3) & (np.abs(P1[:, 1]) <= 0.3)
    P = np.where(on_quad[:, None], P1, P0)
    alb = np.where(on_quad[:, None], np.array([0.25, 0.875, 0.5]), np.array([0.75, 0.5, 0.25]))
    w = L - P
    d2 = (w * w).sum(1)
    cos = w[:, 2] / np.sqrt(d2)  # (both normals are +z, faced to the camera above)
    val = alb / np.pi * inten[None] * (cos / d2)[:, None]
    s = (1.5 - L[2]) / (P0[:, 2] - L[2])  # where the segment light -> plane point crosses z = 1.5
    X = L[None] + s[:, None] * (P0 - L[None])
    shadowed = occluder & ~on_quad & (np.abs(X[:, 0]) < 0.299) & (np.abs(X[:, 1]) < 0.299)
    edge = occluder & ~on_quad & ~shadowed & (np.abs(X[:, 0]) < 0.301) & (np.abs(X[:, 1]) < 0.301)
    return sd, val, shadowed, edge


def test_a_point_light_above_a_lambert_plane_in_closed_form():
    light, inten = (0.5, 0.3, 3.0), (5.0, 7.0, 11.0)
    row = rl.table_row("point", np.array([[1, 0, 0, light[0]], [0, 1, 0, light[1]], [0, 0, 1, light[2]], [0, 0, 0, 1.0]]), inten)
    for occluder in (False, True):
        sc = _plane_scene(occluder)
        sd, want, shadowed, edge = _plane_closed_form(sc, light, inten, occluder)
        verts, tri_idx, tri_shape, alb = world_arrays(sc)
        got = rl.sample_radiance(verts, tri_idx, tri_shape, sd, alb, [row], 1, 0, use_jitter=False)
        assert got.shape == want.shape and (want > 0).all()
        lit = ~shadowed & ~edge
        rel = np.abs(got[lit] - want[lit]) / want[lit]
        print("plane, occluder", occluder, ": max relative error", rel.max(), "shadowed samples", int(shadowed.sum()), "of", len(want))
        assert rel.max() <= 1e-12
        if occluder:
            assert shadowed.sum() >= 3 and (got[shadowed] == 0.0).all()
        else:
            assert not shadowed.any()


def test_superposition_of_two_lights():
    sc = ls.corner("21x19")
    sd = scene_desc.scene_desc(sc, shadows=True)
    verts, tri_idx, tri_shape, alb = world_arrays(sc)
    t = ops.pack_lights([ls.POINT, ls.SPOT_B]).numpy().astype(np.float64)
    both = rl.render_lights(verts, tri_idx, tri_shape, sd, alb, t, 4, 3, max_depth=3)
    one = [rl.render_lights(verts, tri_idx, tri_shape, sd, alb, t[k:k + 1], 4, 3, max_depth=3) for k in range(2)]
    assert one[0].mean() > 0 and one[1].mean() > 0
    np.testing.assert_allclose(both, one[0] + one[1], rtol=1e-12, atol=1e-12 * both.max())


# ------------------------------------------------------------------ the preconditions of tests/test_lights_gpu.py's comparisons
@pytest.mark.parametrize("film", sorted(ls.FILMS))
@pytest.mark.parametrize("principled", [False, True])
def test_the_extra_lights_matter_in_the_scenes_of_the_gpu_tests(film, principled):
    sc = ls.corner(film, principled)
    sd = scene_desc.scene_desc(sc, shadows=True, mat_stride=16 if principled else 0)
    verts, tri_idx, tri_shape, alb = world_arrays(sc)
    mats = scenes.material_rows(sc) if principled else alb
    spp, seed = 16, 7
    main = rp.render_fwd(verts, tri_idx, tri_shape, sd, mats, host_tex(sc), spp, seed, 2)
    for light in (ls.POINT, ls.SPOT_B):
        st = {}
        part = rl.render_lights(verts, tri_idx, tri_shape, sd, mats, ops.pack_lights([light]).numpy(), spp, seed, stats=st)
        share = part.mean() / (main + part).mean()
        print(film, principled, light.name, "share of the image's mean", share, st[0])
        assert share > 0.05
    st = {}
    rl.render_lights(verts, tri_idx, tri_shape, sd, mats, ops.pack_lights([ls.POINT]).numpy(), spp, seed, stats=st)
    occ = st[0]["occluded"] / st[0]["lit"]
    print(film, principled, "occluded share of the samples that face the point light", occ)
    assert 0.05 < occ < 0.95


def test_bounces_matter_and_the_wide_spot_holds_every_vertex():
    sc = ls.corner("24x24")
    sd = scene_desc.scene_desc(sc, shadows=True)
    verts, tri_idx, tri_shape, alb = world_arrays(sc)
    st = {}
    L = rl.sample_radiance(verts, tri_idx, tri_shape, sd, alb, ops.pack_lights([ls.POINT]).numpy(), 16, 7, max_depth=3, stats=st)
    direct = st["direct"].sum()
    print("indirect / direct of the point light at max_depth 3:", (L.sum() - direct) / direct)
    assert L.sum() - direct > 0.05 * direct > 0
    for depth in (2, 3):
        st = {}
        rl.sample_radiance(verts, tri_idx, tri_shape, sd, alb, ops.pack_lights([ls.WIDE_SPOT]).numpy(), 16, 7, max_depth=depth, stats=st)
        assert st[0]["faces"] > 0 and st[0]["min_fall"] == 1.0, st[0]
