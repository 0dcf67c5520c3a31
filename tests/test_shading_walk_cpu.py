"""The float64 walk on shading normals and base-colour textures (tests/ref_path.py `walk`) without a GPU: what the restatements
gave on flat scenes before they shared it is what they give now, bit for bit; vertex 1 of the walk is tests/ref_bruteforce.py's; the scene of
tests/test_shading_walk_gpu.py (corner_scenes.smooth_corner at tests/smooth_cases.py's films and seeds) puts enough vertices where the two normals
differ; and every rule of the walk, swapped for the mistake a kernel could make, misses a bound of that file on that scene."""
import os

import numpy as np
import pytest

from fireflies_amd import scene_desc
from tests import ambient_scenes as am
from tests import corner_scenes as cs
from tests import light_scenes as ls
from tests import ref_ambient as ra
from tests import ref_bruteforce as bf
from tests import ref_lights as rl
from tests import ref_path as rp
from tests import ref_prb
from tests import ref_sun as rs
from tests import smooth_cases as sm
from tests import sun_scenes as ss
from tests.support import ROOT, independent_figures, world_arrays

GOLDEN = os.path.join(ROOT, "tests", "golden", "shading_walk_parent.npz")


def _host(sc, shadows=True):
    return world_arrays(sc)[:3], scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows), sm.host_rows(sc)


# ------------------------------------------------------------------ a. nothing moved
def _cat(out, name, vertices):
    vertices = list(vertices)
    out[name + "/count"] = np.asarray([len(v[0]) for v in vertices])
    for k in range(len(vertices[0])):
        out[f"{name}/{k}"] = np.concatenate([np.asarray(v[k], np.float64).reshape(len(v[0]), -1) for v in vertices])


def _emitters(lst):
    return [(idx, beta, e["pfac"], e["spot"], np.stack(e["taps"], 1), np.stack(e["w"], 1)) for idx, beta, e in lst]


def walk_values():
    """every array the restatements hand out on five flat, untextured cases.  tests/golden/shading_walk_parent.npz holds what this function returned
    (np.savez_compressed) at the commit before the restatements shared one walk, when ref_lights.vertices yielded one normal n where it now yields
    n_g and n_s: the file's lights/4 is that n, and both normals must equal it"""
    out = {}
    world, sd, rows = _host(cs.path_corner(True, W=8, H=8, tex=8))
    _cat(out, "path_corner", _emitters(rp.path_vertices(*world, sd, rows, 4, 7, 4, 2)))
    dimmer = rows.copy()
    dimmer[:, :3] *= 0.9
    _cat(out, "path_corner_frozen", _emitters(ref_prb.path_vertices_frozen(*world, sd, dimmer, rows, 4, 7, 4, 2)))
    world, sd, rows = _host(cs.relay(True, True, W=8, H=8, tex=8))
    _cat(out, "relay", _emitters(rp.path_vertices(*world, sd, rows, 4, 7, 3)))
    world, sd, rows = _host(ls.corner("21x19", True))
    seen = list(rl.vertices(*world, sd, rows, 2, 7, 4, 2))
    _cat(out, "lights", [(idx, [v] * len(idx), beta, P, ng, Po, d, r) for v, idx, beta, P, ng, ns, Po, d, r in seen])
    _cat(out, "lights_ns", [(idx, ns) for v, idx, beta, P, ng, ns, Po, d, r in seen])
    out["lights/image"] = rl.render_lights(*world, sd, rows, sm.host_table(ls.POINT, ls.SPOT_B), 2, 7, 4, 2, gaussian_stddev=0.5)
    world, sd, rows = _host(am.corner("21x19", False))
    out["ambient/image"] = ra.render_ambient(*world, sd, rows, am.RADIANCE, 2, 7, 3, 1)
    out["ambient/image32"] = ra.render_ambient(*world, sd, rows, am.RADIANCE, 2, 7, 3, 1, round32=True)
    world, sd, rows = _host(ss.corner("21x19", True))
    out["sun/image"] = rs.render_sun(*world, sd, rows, sm.host_table(ss.SUN_A, ls.POINT), 2, 7, 3, 1, gaussian_stddev=0.5)
    return out


def test_the_shared_walk_moved_no_value_of_the_flat_restatements():
    got = walk_values()
    want = np.load(GOLDEN)
    assert np.array_equal(got.pop("lights_ns/1"), want["lights/4"]) and np.array_equal(got.pop("lights_ns/0"), want["lights/0"])
    del got["lights_ns/count"]
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert want["path_corner/count"].sum() > 250 and np.abs(want["sun/image"]).max() > 0  # (the file holds something)


def test_flat_flags_and_absent_textures_are_the_walk_without_them():
    world, sd, rows = _host(cs.path_corner(True, W=8, H=8, tex=8))
    tex = np.random.default_rng(1).random((8, 8, 1))
    a = rp.render_fwd(*world, sd, rows, tex, 4, 7, 4, 2)
    b = rp.render_fwd(*world, sd, rows, tex, 4, 7, 4, 2, smooth=[False] * 4, vert_uv=None, base_tex=None)
    assert a.max() > 0 and np.array_equal(a, b)


# ------------------------------------------------------------------ b. vertex 1 is ref_bruteforce's
@pytest.mark.parametrize("stddev", [None, 0.5], ids=["box", "gaussian"])
@pytest.mark.parametrize("kw", [{}, {"lambert_only": True}, {"every_lobe": True}], ids=["rows", "stride3", "every_lobe"])
def test_vertex_1_is_the_brute_force_restatement(kw, stddev):
    sc, bt, uv = sm.scene("13x11", **kw)
    world, sd, rows = _host(sc)
    sh = sm.shading(sc, bt, uv)
    assert any(sh["smooth"]) and rows.shape[1] == (3 if kw.get("lambert_only") else 16)
    tex = np.random.default_rng(1).random((32, 32, 1))
    gimg = np.random.default_rng(2).uniform(0.5, 1.5, (11, 13, 3))
    a = rp.render_fwd(*world, sd, rows, tex, sm.SPP, sm.SEED, 2, gaussian_stddev=stddev, **sh)
    b = bf.render_fwd(*world, sd, rows, tex, sm.SPP, sm.SEED, gaussian_stddev=stddev, **sh)
    flat = bf.render_fwd(*world, sd, rows, tex, sm.SPP, sm.SEED, gaussian_stddev=stddev)
    print("forward: max |difference|", np.abs(a - b).max(), "scale", b.max(), "smooth and textured vs flat", np.abs(b - flat).max())
    assert b.max() > 0 and np.abs(a - b).max() <= 1e-12 * b.max()
    assert np.abs(b - flat).max() > 0.05 * b.max()  # (the arguments matter)
    ga = rp.render_bwd(*world, sd, rows, sm.SPP, sm.SEED, gimg, 2, gaussian_stddev=stddev, **sh)[..., 0]
    gb = bf.render_bwd(*world, sd, rows, sm.SPP, sm.SEED, gimg, gaussian_stddev=stddev, **sh)
    print("adjoint: max |difference|", np.abs(ga - gb).max(), "scale", np.abs(gb).max())
    assert np.abs(gb).max() > 0 and np.abs(ga - gb).max() <= 1e-12 * np.abs(gb).max()


# ------------------------------------------------------------------ c. the scene does its job
BALL, FLOOR = 3, 0
CASES_C = [(film, sm.SPP, sm.SEED) for film in sm.FILMS] + [(sm.DIFF_FILM, sm.DIFF_SPP, sm.DIFF_SEED)]


def census(film, spp, seed, depth=4, **kw):
    """what the reference's own walk meets on smooth_corner: per vertex the shares of vertices on the ball and on the floor; the angles between n_s
    and n_g on the ball; the bounces that n_g . wo <= 0 ends, the vertices with n_s . n_g < 0, and the samples an fp32 walk could decide the other
    way (|n_g . wo| or |n_s . d| below 1e-5)"""
    sc, bt, uv = sm.scene(film, **kw)
    world, sd, rows = _host(sc)
    key = rp.path_key(seed)
    out = {"ball": [], "floor": [], "angles": [], "ended": 0, "flipped": 0, "near": 0, "samples": sd.cam.width * sd.cam.height * spp}
    for x in rp.walk(*world, sd, rows, spp, seed, depth, **sm.shading(sc, bt, uv)):
        on = x.shape == BALL
        wo = rp.cosine_dir(x.ns, rp.path_u(key, x.idx, x.v, 0), rp.path_u(key, x.idx, x.v, 1))
        gw, sg = (x.ng * wo).sum(1), (x.ns * x.ng).sum(1)
        out["ball"].append(float(on.mean()))
        out["floor"].append(float((x.shape == FLOOR).mean()))
        out["angles"].append(np.degrees(np.arccos(np.clip(np.abs(sg[on]), 0.0, 1.0))))
        out["ended"] += int((gw <= 0).sum())
        out["flipped"] += int((sg < 0).sum())
        out["near"] += int((np.abs(gw) < 1e-5).sum() + (np.abs((x.ns * x.d).sum(1)) < 1e-5).sum())
        assert np.allclose(sg[~on], 1.0, rtol=0, atol=1e-15)  # (flat shapes: one normal)
    return out


@pytest.mark.parametrize("film,spp,seed", CASES_C, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_the_scene_puts_the_walk_where_the_normals_differ(film, spp, seed):
    """conditions, not measurements.  The two counts are stated for the 2304-sample film (12 x 12 x 16); a film of n samples is held to the same rate,
    10 n / 2304 rounded down — 9 on the ragged 13 x 11 (2288 samples), 2 on the 8 x 8 x 8 film of the difference tests, where no seed of 1 .. 15
    reaches 10 with 512 samples (1 .. 9 bounces end, 1 .. 6 normals face away)"""
    c = census(film, spp, seed)
    need = max(1, 10 * c["samples"] // 2304)
    med = float(np.median(np.concatenate(c["angles"])))
    print(f"{film} x {spp} spp, seed {seed}: on the ball {np.round(c['ball'], 3)}, on the floor {np.round(c['floor'], 3)}, median angle {med:.1f} deg, "
          f"ended by n_g.wo <= 0: {c['ended']} (>= {need}), n_s.n_g < 0: {c['flipped']} (>= {need}), within 1e-5 of a decision: {c['near']}")
    assert c["ball"][0] >= 0.10 and c["ball"][1] >= 0.30
    assert med >= 10.0
    assert c["ended"] >= need and c["flipped"] >= need
    assert c["floor"][1] >= 0.15
    assert c["near"] == 0


# ------------------------------------------------------------------ d. each rule is visible at the GPU tests' bound
_TRUE = {}


def parts(film, depth, stddev, shadows, swap):
    """the five parts tests/test_shading_walk_gpu.py compares — the main emitters' image and what a point light, a spot, a sun and the constant
    emitter add — of the walk with one rule swapped (None: the true walk), and the scale and the part's sum each is judged by"""
    key = (film, depth, stddev, shadows, swap)
    if swap is None and key in _TRUE:
        return _TRUE[key]
    sc, bt, uv = sm.scene(film)
    world, sd, rows = _host(sc, shadows)
    k = dict(sm.shading(sc, bt, uv), swap=swap)
    tex = np.random.default_rng(1).random((32, 32, 1))
    a = (*world, sd, rows)
    b = (sm.SPP, sm.SEED, depth)
    p = {"main": rp.render_fwd(*a, tex, *b, gaussian_stddev=stddev, **k),
         "point": rl.render_lights(*a, sm.host_table(sm.POINT), *b, gaussian_stddev=stddev, **k),
         "spot": rl.render_lights(*a, sm.host_table(sm.SPOT), *b, gaussian_stddev=stddev, **k),
         "sun": rs.render_sun(*a, sm.host_table(sm.SUN), *b, gaussian_stddev=stddev, **k),
         "ambient": ra.render_ambient(*a, sm.RADIANCE, *b, gaussian_stddev=stddev, **k)}
    if swap is None:
        direct = rp.render_fwd(*a, tex, sm.SPP, sm.SEED, 2, gaussian_stddev=stddev, **k)
        p["indirect"] = p["main"] - direct
        _TRUE[key] = p
    return p


def judged_by(name, true, direct):
    """the scale and the sum tests/test_shading_walk_gpu.py judges a part by at max_depth > 2: the whole image's scale; the main image's and the
    lights' and the sun's indirect share, the constant emitter's whole part"""
    scale = float(true["main"].max()) if name == "main" else float((true["main"] + true[name]).max())
    return scale, float(true[name].sum() if name == "ambient" else (true[name] - direct[name]).sum())


# (the rule, the parts it acts on: the constant emitter has no cosine and no side of its own)
RULES = [(s, ("main", "point", "spot", "sun") + (() if s in ("emitter_cosine_from_ng", "no_geometric_side") else ("ambient",))) for s in rp.SWAPS]


@pytest.mark.parametrize("swap,names", RULES, ids=[r[0] for r in RULES])
def test_a_walk_with_one_rule_swapped_misses_a_bound_of_the_gpu_tests(swap, names):
    """at max_depth 4 on the 12 x 12 box film, for every part the rule acts on: the swapped walk against the true one fails at least one of the three
    conditions the GPU file holds the kernels to — so a kernel that made this mistake could not pass there.  The emitter's geometric side is the one
    rule a shadow ray hides: a light behind the facet (n_g . wi <= 0) that the shading normal sees (n_s . wi > 0) is occluded by that very facet on
    its way to the lifted point, so with shadows the swapped walk differs by 0 .. 0.17 of a bound; it is judged, as the GPU file judges it, on the
    scene loaded without shadows"""
    shadows = swap != "no_geometric_side"
    true, direct = parts("12x12", 4, None, shadows, None), parts("12x12", 2, None, shadows, None)
    got = parts("12x12", 4, None, shadows, swap)
    assert true["indirect"].mean() > 0.05 * true["main"].mean()
    for name in names:
        f = independent_figures(got[name], true[name], *judged_by(name, true, direct))
        print(f"{swap}, {name}: as fractions of the bounds: pixels off {f[0]:.2f}, median {f[1]:.2f}, sums {f[2]:.2f}")
        assert max(f) > 1.0, (swap, name, f)


def test_the_emitters_side_is_hidden_by_the_shadow_ray():
    """the reason the unshadowed load exists: with shadows the walk without the geometric-side test stays far inside every bound"""
    true, direct, got = parts("12x12", 4, None, True, None), parts("12x12", 2, None, True, None), parts("12x12", 4, None, True, "no_geometric_side")
    for name in ("main", "point", "spot", "sun"):
        f = independent_figures(got[name], true[name], *judged_by(name, true, direct))
        print(f"{name}: as fractions of the bounds {np.round(f, 3)}")
        assert max(f) < 0.5, (name, f)
