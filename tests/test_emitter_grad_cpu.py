"""The extra emitters' adjoint without a GPU: the bit in the header and the ABI module, its refusals before any launch
(tests/refusals.py's set-up: nothing can launch), ops.render_bwd's argument checks, and mi.Scene's two leaf registries."""
import re
import types

import pytest
import torch

from fireflies_amd import _abi, mi, ops, scenes
from tests import light_scenes as ls
from tests import refusals
from tests import sun_scenes as ss
from tests.support import FFX_ERR_ARG, FFX_ERR_UNSUPPORTED, define, header


# ------------------------------------------------------------------ 1. header and ABI
def test_the_headers_bit_equals_abis_and_overlaps_no_other_flag():
    assert define("FFX_ABI_VERSION") == 11
    assert define("FFX_RENDER_EMITTER_GRAD") == _abi.RENDER_EMITTER_GRAD == 0x8000000 == 1 << 27
    assert _abi.RENDER_EMITTER_GRAD_BLOCK_FLOATS == 3 * (define("FFX_RENDER_MAX_LIGHTS") + 1) == 27
    assert _abi.emitter_grad_floats(21, 19) == 27 * (21 * 19 + 1)
    taken = (_abi.RENDER_FP16 | _abi.RENDER_SPARSE_ADJOINT | _abi.RENDER_APEX_READY | _abi.RENDER_CACHE_ZEROED | _abi.RENDER_CACHE_KEEP_DROPPED | _abi.RENDER_PATH_MASK
             | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL | _abi.RENDER_GRAD_PRB | _abi.RENDER_TANGENT | _abi.RENDER_AOV | _abi.RENDER_LIGHTS_MASK
             | _abi.RENDER_AMBIENT | _abi.RENDER_LIGHTS_DIRECTIONAL)
    assert _abi.RENDER_EMITTER_GRAD & taken == 0 and taken < 1 << 27
    words = {n: int(v, 16) for n, v in re.findall(r"#define (FFX_RENDER_\w+) (0x[0-9a-fA-F]+)\b", header())}
    assert len(words) >= 8 and words.pop("FFX_RENDER_EMITTER_GRAD") == 1 << 27
    assert not [n for n, v in words.items() if v & (1 << 27)], words
    # the name keeps clear of the refusals' wildcard, and the header spells the wildcard out
    assert not [n for n in re.findall(r"#define (FFX_RENDER_GRAD_\w+)", header()) if "EMITTER" in n]
    assert "FFX_RENDER_GRAD_*" not in header()


# ------------------------------------------------------------------ 2. refusals before any launch
_E, _D, _L1, _A = _abi.RENDER_EMITTER_GRAD, _abi.RENDER_LIGHTS_DIRECTIONAL, _abi.render_lights(1), _abi.RENDER_AMBIENT
_GRAD = "is not served together with a FFX_RENDER_GRAD_* bit"
_ONLY = "FFX_RENDER_EMITTER_GRAD is served by ffx_render_bwd[_filtered] only"
_NEEDS = "FFX_RENDER_EMITTER_GRAD needs FFX_RENDER_LIGHTS(n >= 1) or FFX_RENDER_AMBIENT"
_REFUSALS = [
    # the bit alone, with path bits, and with the table's bit but no table
    ("ffx_render_bwd", _E, {}, FFX_ERR_ARG, "render_bwd: " + _NEEDS),
    ("ffx_render_bwd_filtered", _E, {}, FFX_ERR_ARG, "render_bwd_filtered: " + _NEEDS),
    ("ffx_render_bwd", _E | _abi.render_path(3, 5), {}, FFX_ERR_ARG, "render_bwd: " + _NEEDS),
    ("ffx_render_bwd", _E | _D, {}, FFX_ERR_ARG, "render_bwd: " + _NEEDS),
    ("ffx_render_bwd", _E | _D | _A, {}, FFX_ERR_ARG, "render_bwd: FFX_RENDER_LIGHTS_DIRECTIONAL needs FFX_RENDER_LIGHTS(n >= 1)"),
    ("ffx_render_bwd", _E | _abi.render_lights(9), {}, FFX_ERR_ARG, "render_bwd: FFX_RENDER_LIGHTS(9): at most 8 extra emitters"),
    ("ffx_render_bwd", _E | _L1, {"mats": None}, FFX_ERR_ARG, "render_bwd: FFX_RENDER_EMITTER_GRAD needs the device buffer"),
    # with each of the three GRAD bits the existing refusal of the lights' bits fires first, in its own words
    ("ffx_render_bwd", _E | _L1 | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_bwd: FFX_RENDER_LIGHTS " + _GRAD + " (the extra emitters are not differentiated)"),
    ("ffx_render_bwd", _E | _L1 | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED,
     "render_bwd: FFX_RENDER_LIGHTS " + _GRAD + " (the extra emitters are not differentiated)"),
    ("ffx_render_bwd_filtered", _E | _L1 | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_PRB | _abi.render_path(3, 5), {}, FFX_ERR_UNSUPPORTED,
     "render_bwd_filtered: FFX_RENDER_LIGHTS " + _GRAD + " (the extra emitters are not differentiated)"),
    ("ffx_render_bwd", _E | _A | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED, "render_bwd: FFX_RENDER_AMBIENT " + _GRAD + " (the constant emitter is not differentiated)"),
    ("ffx_render_bwd_filtered", _E | _A | _abi.RENDER_GRAD_APPEARANCE | _abi.RENDER_GRAD_MATERIAL, {}, FFX_ERR_UNSUPPORTED,
     "render_bwd_filtered: FFX_RENDER_AMBIENT " + _GRAD + " (the constant emitter is not differentiated)"),
    # a GRAD bit beside the bit alone: refused under the bit's own name, the three spelled out
    ("ffx_render_bwd", _E | _abi.RENDER_GRAD_APPEARANCE, {}, FFX_ERR_UNSUPPORTED,
     "render_bwd: FFX_RENDER_EMITTER_GRAD is not served together with FFX_RENDER_GRAD_APPEARANCE, FFX_RENDER_GRAD_MATERIAL or FFX_RENDER_GRAD_PRB"),
    # every other entry point
    ("ffx_render_fwd", _E | _L1, {}, FFX_ERR_UNSUPPORTED, "render_fwd: " + _ONLY),
    ("ffx_render_fwd", _E, {}, FFX_ERR_UNSUPPORTED, "render_fwd: " + _ONLY),
    ("ffx_render_fwd_filtered", _E | _A, {}, FFX_ERR_UNSUPPORTED, "render_fwd_filtered: " + _ONLY),
    ("ffx_render_fwd_cache", _E, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache: " + _ONLY),
    ("ffx_render_fwd_cache_filtered", _E, {}, FFX_ERR_UNSUPPORTED, "render_fwd_cache_filtered: " + _ONLY),
    ("ffx_render_fwd_adjoint", _E, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint: " + _ONLY),
    ("ffx_render_fwd_adjoint_filtered", _E, {}, FFX_ERR_UNSUPPORTED, "render_fwd_adjoint_filtered: " + _ONLY),
    ("ffx_render_bwd_det", _E, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det: " + _ONLY),
    ("ffx_render_bwd_det_part", _E, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det_part: " + _ONLY),
    ("ffx_render_bwd_cached", _E, {}, FFX_ERR_UNSUPPORTED, "render_bwd_cached: " + _ONLY),
    # the lights' bits in front of the bit keep their own refusal there
    ("ffx_render_bwd_det", _E | _L1, {}, FFX_ERR_UNSUPPORTED, "render_bwd_det: FFX_RENDER_LIGHTS is served by ffx_render_fwd[_filtered] only"),
    # served: the calls get as far as the last refusal in front of the launches
    ("ffx_render_bwd", _E | _L1, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
    ("ffx_render_bwd", _E | _A, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
    ("ffx_render_bwd_filtered", _E | _D | _abi.render_lights(8) | _A, {}, FFX_ERR_ARG, "render_bwd: blob without per-slot normals"),
]


@pytest.mark.parametrize("case", _REFUSALS, ids=lambda c: f"{c[0][4:]}-{c[1]:#x}-{'nomats' if c[2] else 'mats'}")
def test_the_bit_is_refused_before_any_launch(case, monkeypatch):
    """tests/refusals.py's set-up (nothing can launch), with this suite's own default: no dot_out / loss_slots buffer"""
    name, flags, arg_changes, rc, msg = case
    got, err = refusals.call(name, refusals.GAUSS if "filtered" in name else {}, {"flags": flags, "dot": None, **arg_changes}, monkeypatch=monkeypatch)
    assert got == rc, (got, err)
    assert msg in err, err


# ------------------------------------------------------------------ 3. ops.render_bwd's argument checks
def test_render_bwd_checks_its_arguments_before_it_touches_the_device(monkeypatch):
    geom = types.SimpleNamespace(device=torch.device("cpu"))
    geom._render_bwd_emitters = types.MethodType(ops.DeviceGeometry._render_bwd_emitters, geom)
    geom._with_lights = types.MethodType(ops.DeviceGeometry._with_lights, geom)
    sd = _abi.SceneDesc()
    sd.cam.width, sd.cam.height, sd.n_shapes = 4, 4, 1
    rows = torch.zeros(1, 3)
    gimg = torch.zeros(4, 4, 3)
    lights = ops.pack_lights([ls.POINT, ss.SUN_A])
    call = ops.DeviceGeometry.render_bwd
    for k in ("FFX_DETERMINISTIC",):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(ValueError, match=r"emitters=True\) needs lights= and / or ambient="):
        call(geom, sd, rows, 4, 1, gimg, emitters=True)
    with pytest.raises(ValueError, match=r"emitters=True\) needs lights= and / or ambient="):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=lights[:0])
    # appearance=True: the existing raises fire first, in their words; without emitters to speak of, the keyword's own
    with pytest.raises(NotImplementedError, match=r"extra emitters \(lights=\) are not differentiated"):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=lights, appearance=True)
    with pytest.raises(NotImplementedError, match=r"the constant emitter \(ambient=\) is not differentiated"):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, ambient=(1.0, 1.0, 1.0), appearance=True)
    with pytest.raises(NotImplementedError, match=r"emitters=True\): not served together with appearance=True"):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, appearance=True)
    with pytest.raises(ValueError, match="max_depth must be an integer in 2 .. 8"):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=lights, max_depth=9)
    with pytest.raises(ValueError, match="no deterministic adjoint"):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=lights, deterministic=True)
    monkeypatch.setenv("FFX_DETERMINISTIC", "1")
    with pytest.raises(ValueError, match="no deterministic adjoint"):
        call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=lights)
    monkeypatch.delenv("FFX_DETERMINISTIC")
    with pytest.raises(ValueError, match=r"gimg must hold \[H, W, 3\] floats"):
        call(geom, sd, rows, 4, 1, gimg[:2], emitters=True, lights=lights)
    orig = ops._dev
    try:
        ops._dev = lambda t, *a, **k: t
        with pytest.raises(ValueError, match="at most 8 extra emitters"):
            call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=torch.zeros(9, 24))
        with pytest.raises(ValueError, match=r"lights must be a \[n, 24\] float32 tensor"):
            call(geom, sd, rows, 4, 1, gimg, emitters=True, lights=torch.zeros(2, 23))
        with pytest.raises(ValueError, match="three floats"):
            call(geom, sd, rows, 4, 1, gimg, emitters=True, ambient=(1.0, 2.0))
    finally:
        ops._dev = orig
    # the keyword is the last one, and the result type names its two blocks
    import inspect

    assert list(inspect.signature(call).parameters)[-1] == "emitters" and inspect.signature(call).parameters["emitters"].default is False
    assert ops.EmitterGrad._fields == ("lights", "ambient")


# ------------------------------------------------------------------ 4. the two registries (a stand-in for the device geometry: no key here moves it)
class _NoGeometry:
    def __init__(self, *a, device=None, **k):
        self.device, self.version, self._async, self.n_shapes = device, 0, False, 4

    def update(self, *a, **k):
        raise AssertionError("an emitter's key pushed the geometry")


def _scene():
    sc = ss.corner("24x24", True)
    sc.lights = [ls.POINT, ls.SPOT_B, ss.SUN_A]
    sc.ambient = scenes.AmbientData("emit-World", (0.2, 0.25, 0.3))
    return sc


_KEYS = ("emit-Light.intensity.value", "emit-SecondSpot.intensity.value", "emit-SunA.irradiance.value", "emit-World.radiance.value")


def test_the_emitter_leaves_have_a_registry_of_their_own(monkeypatch):
    monkeypatch.setattr(ops, "DeviceGeometry", _NoGeometry)
    plain = mi.load_scene_data(ss.corner("24x24", True), device="cpu")
    ms = mi.load_scene_data(_scene(), device="cpu")
    p = mi.traverse(ms)
    assert p._emitter_leaf_keys == frozenset(_KEYS)
    assert mi.traverse(plain)._emitter_leaf_keys == frozenset() and mi.traverse(plain)._emitter_leaves == {}
    # what keys off the appearance registry is what it was: the same keys as the scene without extra emitters, the first spot's intensity among them
    assert p._leaf_keys == mi.traverse(plain)._leaf_keys and not p._leaf_keys & p._emitter_leaf_keys
    assert ms.data.spot.name + ".intensity.value" in p._leaf_keys
    assert mi._forward_keys(ms) == mi._forward_keys(plain)
    for k in _KEYS:  # each of the three kinds of key: a grad tensor registers, a plain value drops
        t = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
        p[k] = t
        assert p._emitter_leaves == {k: t} and p._leaves == {}
        p[k] = mi.Color3f(torch.tensor([1.0, 2.0, 3.0]))
        assert p._emitter_leaves == {}
        w = mi.Color3f(torch.tensor([1.0, 2.0, 3.0], requires_grad=True))
        p[k] = w
        assert list(p._emitter_leaves) == [k] and p._emitter_leaves[k] is w.t
        p[k] = torch.tensor([1.0, 2.0, 3.0])
        assert p._emitter_leaves == {}
    # keys of the emitters that are no power: not leaves
    p["emit-Light.position"] = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    p["emit-SecondSpot.cutoff_angle"] = torch.tensor(30.0, requires_grad=True)
    assert p._emitter_leaves == {} and p._leaves == {}
    # the first spot's intensity stays an appearance leaf
    k0 = ms.data.spot.name + ".intensity.value"
    p[k0] = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    assert list(p._leaves) == [k0] and p._emitter_leaves == {}


def test_a_mixed_scene_and_the_deterministic_mode_are_refused_before_any_render(monkeypatch):
    monkeypatch.setattr(ops, "DeviceGeometry", _NoGeometry)
    ms = mi.load_scene_data(_scene(), device="cpu")
    p = mi.traverse(ms)
    p[_KEYS[0]] = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    monkeypatch.setattr(ms, "lights_table", lambda: torch.zeros(3, 24))
    monkeypatch.setattr(ms, "ambient_record", lambda: torch.zeros(3))
    monkeypatch.setenv("FFX_DETERMINISTIC", "1")
    with pytest.raises(ValueError, match="extra emitters' powers have no deterministic adjoint"):
        mi.render(ms, spp=4)
    monkeypatch.delenv("FFX_DETERMINISTIC")
    with pytest.raises(ValueError, match="no fp16 film"):
        mi.render(ms, spp=4, fp16=True)
    p[sorted(k for k in p._leaf_keys if k.endswith(".brdf_0.base_color.value"))[0]] = torch.tensor([0.5, 0.5, 0.5], requires_grad=True)
    with pytest.raises(NotImplementedError, match="extra emitters.*not differentiated"):
        mi.render(ms, spp=4)
