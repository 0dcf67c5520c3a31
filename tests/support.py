"""Helpers that tests with and without a GPU share: a scene's world arrays, copies of a scene description, a loaded scene file, finite-difference stencils, the outlier rule and the
three conditions of an independent evaluation,
what include/ffx.h says, a C compiler, the oracle's geometry of a scene.  numpy, ctypes and the standard library beside the package's host-side
modules: nothing here needs a device (tests/gpu_support.py holds what does)."""
import ctypes as C
import os
import re
import shutil
import warnings

import numpy as np

from fireflies_amd import _abi, loaders, scene_desc, scenes
from tests import tie_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ include/ffx.h
def header():
    with open(os.path.join(ROOT, "include", "ffx.h")) as f:
        return f.read()


def define(name):
    m = re.search(r"^#define\s+" + name + r"\s+(\S+)", header(), re.M)
    assert m, name
    return int(m.group(1), 0)


def enum_value(name):
    m = re.search(r"^\s*" + name + r"\s*=\s*(-?\d+)", header(), re.M)
    assert m, name
    return int(m.group(1))


FFX_ERR_ARG, FFX_ERR_UNSUPPORTED = enum_value("FFX_ERR_ARG"), enum_value("FFX_ERR_UNSUPPORTED")


def c_compiler():
    for c in (os.environ.get("CC"), "cc", "gcc", "clang"):
        if c and shutil.which(c):
            return c
    return None


# ------------------------------------------------------------------ scenes and their descriptions
def world_arrays(sc):
    """-> (vertex pool in float64, triangles in pool indices, shape of every triangle, albedo rows): what the float64 restatements take"""
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    return pool.astype(np.float64), tris + off[shape][:, None], shape, alb


def arrays(sc, principled=False):
    """-> (the description with shadows, (vertex pool, triangles, shape of every triangle), the material rows or the albedos): what the float64
    restatements of the emitter suites take"""
    sd = scene_desc.scene_desc(sc, shadows=True, mat_stride=16 if principled else 0)
    verts, tri_idx, tri_shape, alb = world_arrays(sc)
    return sd, (verts, tri_idx, tri_shape), scenes.material_rows(sc) if principled else alb


def load_xml(path):
    """-> (the scene of a Mitsuba-XML file, the loader's reports as strings)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sc = loaders.load_mitsuba_xml(path)
    return sc, [str(x.message) for x in w]


def copy_desc(sd):
    out = _abi.SceneDesc()
    C.memmove(C.addressof(out), C.addressof(sd), C.sizeof(out))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_geom(oracle, sc, frame=0):
    """-> (the oracle's geometry of `sc` at `frame`, albedo rows); a scene marked by tie_scenes.sheets_far_unpadded is re-fitted with leaf_pad = 0"""
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    g = oracle.Geometry(pool, tris, shape, off)
    g.update(np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)), (off + np.minimum(frame, nfr - 1) * stride).astype(np.int32))
    tie_scenes.refit_with_marked_pad(sc, [g], np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)))
    return g, alb


def host_tex(sc, ch=1):
    if sc.projector is None:
        return np.zeros((1, 1), np.float32)
    rng = np.random.default_rng(0)
    return rng.random((sc.projector.height, sc.projector.width) + ((ch,) if ch > 1 else ()), dtype=np.float32)


def material_rows(S, seed, model=1.0, **fixed):
    """random principled material rows [S,16] over the ranges the reference randomises (main.py:97-107)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((S, _abi.MAT_STRIDE), np.float32)
    m[:, 0:3] = rng.uniform(0.1, 0.9, (S, 3))
    m[:, _abi.MAT_MODEL] = model
    m[:, _abi.MAT_ROUGHNESS] = rng.uniform(0.05, 1.0, S)
    m[:, _abi.MAT_ANISOTROPIC] = rng.uniform(0.0, 1.0, S)
    m[:, _abi.MAT_METALLIC] = rng.uniform(0.0, 0.5, S)
    m[:, _abi.MAT_SPEC_TRANS] = rng.uniform(0.0, 0.4, S)
    specular = rng.uniform(0.05, 1.0, S)
    m[:, _abi.MAT_ETA] = 2.0 / (1.0 - np.sqrt(0.08 * specular)) - 1.0
    m[:, _abi.MAT_SPEC_TINT] = rng.uniform(0.0, 1.0, S)
    m[:, _abi.MAT_SHEEN] = rng.uniform(0.0, 0.5, S)
    m[:, _abi.MAT_SHEEN_TINT] = rng.uniform(0.0, 1.0, S)
    m[:, _abi.MAT_FLATNESS] = rng.uniform(0.0, 1.0, S)
    m[:, _abi.MAT_CLEARCOAT] = rng.uniform(0.0, 1.0, S)
    m[:, _abi.MAT_CLEARCOAT_GLOSS] = rng.uniform(0.0, 1.0, S)
    for k, v in fixed.items():
        m[:, getattr(_abi, "MAT_" + k.upper())] = v
    return m


# ------------------------------------------------------------------ a scene file of the Mitsuba-XML subset (tests/test_loaders_cpu.py writes its meshes)
SCENE_XML = """<scene version="3.0.0">
  <default name="spp" value="64"/>
  <default name="res" value="96"/>
  <bsdf type="twosided" id="mat-Mucosa"><bsdf type="principled"><rgb name="base_color" value="0.8, 0.3, 0.35"/><float name="roughness" value="0.35"/><float name="specular" value="0.6"/><float name="clearcoat" value="0.25"/></bsdf></bsdf>
  <sensor type="perspective" id="PerspectiveCamera">
    <float name="fov" value="60"/><float name="near_clip" value="0.01"/><float name="far_clip" value="100"/>
    <transform name="to_world"><lookat origin="0,0,1.5" target="0,0,5" up="0,1,0"/></transform>
    <film type="hdrfilm"><integer name="width" value="$res"/><integer name="height" value="$res"/></film>
  </sensor>
  <sensor type="perspective" id="PerspectiveCamera_1">
    <float name="fov" value="30"/>
    <transform name="to_world"><lookat origin="0.25,0,1.5" target="0,0,5" up="0,1,0"/></transform>
    <film type="hdrfilm"><integer name="width" value="128"/><integer name="height" value="128"/></film>
  </sensor>
  <shape type="obj" id="mesh-Wall">
    <string name="filename" value="wall.obj"/>
    <transform name="to_world"><scale value="2"/><translate z="6"/></transform>
    <ref id="mat-Mucosa"/>
  </shape>
  <shape type="obj" id="mesh-Quad"><string name="filename" value="quad.obj"/>
    <bsdf type="diffuse"><rgb name="reflectance" value="0.2"/></bsdf></shape>
  <emitter type="spot" id="emit-Spot"><rgb name="intensity" value="8"/><float name="cutoff_angle" value="40"/>
    <transform name="to_world"><lookat origin="0,0.1,1.5" target="0,0,5" up="0,1,0"/></transform></emitter>
  <emitter type="projector" id="Projector"><float name="scale" value="20"/>
    <transform name="to_world"><lookat origin="0.25,0,1.5" target="0,0,5" up="0,1,0"/></transform></emitter>
</scene>"""


# ------------------------------------------------------------------ finite differences of a material table
def fd(f, rows, i, col, h, lo=0.0, hi=1.0):
    """d f / d rows[i, col]: central, or second-order one-sided into [lo, hi] at a bound (the forward skips a lobe whose parameter sits there)"""
    x = float(rows[i, col])

    def at(v):
        r = rows.copy()
        r[i, col] = v
        return f(r)

    if col != scenes.MAT_COLUMN["eta"] and x - h < lo:
        return (-3 * at(x) + 4 * at(x + h) - at(x + 2 * h)) / (2 * h)
    if col != scenes.MAT_COLUMN["eta"] and x + h > hi:
        return (3 * at(x) - 4 * at(x - h) + at(x - 2 * h)) / (2 * h)
    return (at(x + h) - at(x - h)) / (2 * h)


def fd4(f, rows, i, col, h):
    """d f / d rows[i, col] by the five-point central stencil (error h^4 f^(5) / 30) where x -+ 2h stays inside the parameter's range, else fd's
    second-order one-sided form.  The three-point stencil is not enough for roughness once a bounce samples the GGX peak, where D ~ roughness^-4:
    at h = 1e-2 its h^2 f(3) / 6 was 1 % of the floor's roughness gradient on the textured corner and fell by 4 with every halving of h (6.1e-2,
    1.5e-2, 3.7e-3, 7.8e-4 at h = 2e-2 .. 2.5e-3), while this stencil agreed with the adjoint to 8e-6."""
    x = float(rows[i, col])
    if col != scenes.MAT_COLUMN["eta"] and (x - 2 * h < 0.0 or x + 2 * h > 1.0):
        return fd(f, rows, i, col, h)

    def at(v):
        r = rows.copy()
        r[i, col] = v
        return f(r)

    return (-at(x + 2 * h) + 8 * at(x + h) - 8 * at(x - h) + at(x - 2 * h)) / (12 * h)


# ------------------------------------------------------------------ comparisons
def _independent(got, ref, scale, part_sum):
    """-> (the three figures, their bounds): the share of the pixels off by more than 2e-3 of the scale [0.04], the median error [1e-4 of the scale], the
    sums' difference [1 % of the part under test]"""
    err = np.abs(got - ref)
    return (float((err > 2e-3 * scale).mean()), np.median(err), abs(got.sum() - ref.sum())), (0.04, 1e-4 * scale, 0.01 * part_sum)


def _fractions(figures, bounds):
    return tuple(float(v) / b for v, b in zip(figures, bounds))


def independent_figures(got, ref, scale, part_sum):
    """the figures of `independent`, each as a fraction of its bound"""
    return _fractions(*_independent(got, ref, scale, part_sum))


def independent(what, got, ref, scale, part_sum):
    """the three conditions that an evaluation independent of its reference is held to: at most 0.04 of the pixels off by more than 2e-3 of the image's
    scale, the median error within 1e-4 of it, the sums within 1 % of the part under test — the figures themselves against their bounds, no quotient
    in between; they are printed before they are asserted -> the figures as fractions of the bounds"""
    (off, median, dsum), bounds = _independent(got, ref, scale, part_sum)
    f = _fractions((off, median, dsum), bounds)
    print(f"{what}: scale {scale:.4g}, off by > 2e-3 scale {off:.4f} [0.04], median {median / scale:.2e} [1e-4], |sum - ref sum| {dsum:.4g} "
          f"[{bounds[2]:.4g}]; as fractions of the bounds: pixels off by > 2e-3 scale {f[0]:.2e}, median {f[1]:.2e}, sums {f[2]:.2e}")
    assert np.isfinite(got).all() and part_sum > 0
    assert off <= bounds[0], what
    assert median <= bounds[1], what
    assert dsum <= bounds[2], what
    return f


def outlier_rule(what, got, want, scale, spp):
    """the project's rule: per pixel within 1e-4 of the scale; at most 2e-4 of the pixels (at least one) beyond, none by more than 1.5 scale / spp — one
    sample on the other side of a triangle edge"""
    err = np.abs(got - want)
    err = err.reshape(err.shape[0] * err.shape[1], -1).max(1)
    out = err > 1e-4 * scale
    allowed = max(1, int(2e-4 * err.size))
    print(f"{what}: scale {scale:.4g}, max err {err.max():.3e}, median {np.median(err):.3e}, outliers {int(out.sum())} / {err.size} (allowed {allowed}), "
          f"cap {1.5 * scale / spp:.3e}")
    assert out.sum() <= allowed, what
    assert err.max() <= 1.5 * scale / spp, what
