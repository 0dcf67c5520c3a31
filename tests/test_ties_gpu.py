"""Every closest-hit walk of libffx_hip.so held to the tie-break rule (closest hit; at equal t the smaller primitive id,
whatever the tree and the traversal order) on the fixtures of tests/tie_scenes.py, which tests/test_ties_cpu.py proves to tie on the oracle.
NO ray is left out anywhere in this file: a difference is a finding to explain.  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

from fireflies_amd import ops, scenes, scene_desc
from tests import tie_scenes as ts
from tests.conftest import assert_image_close
from tests.gpu_support import WALK_KNOBS, Env, dev, host, splat_tex
from tests.gpu_support import pair as _pair_as_built
from tests.support import bits

pytestmark = pytest.mark.gpu

# the walks of K7 (include/ffx.h): the camera's tile bins; the 64-wide tree walk; the binary octant walk; the per-lane walk; the branch a
# grid whose lists overflowed takes
K7_WALKS = {"bins": {}, "wide": {"FFX_BINS": "0"}, "binary": {"FFX_BINS": "0", "FFX_WIDE": "0"}, "lane": {"FFX_TRAVERSAL": "lane"}, "bin_cap_0": {"FFX_BIN_CAP": "0"}}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need a HIP device"


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in WALK_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _pair(oracle, sc):
    """the oracle's and the device's geometry of `sc`; a scene marked by tie_scenes.sheets_far_unpadded is re-fitted with leaf_pad = 0 on both"""
    go, gd, alb = _pair_as_built(oracle, sc)
    ts.refit_with_marked_pad(sc, [go, gd], np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)))
    return go, gd, alb


# ------------------------------------------------------------------ the fixtures and what the rule says about each
def _in01(sc):
    return lambda t, s, p: None if set(np.unique(p[p >= 0])) <= {0, 1} else f"primitives {sorted(set(np.unique(p)) - {-1, 0, 1})[:8]} of the stack answer"


def _shape0(sc):
    return lambda t, s, p: None if (s == 0).all() else f"{int((s != 0).sum())} rays do not return shape 0"


def _no_copy(f_single):
    return lambda sc: (lambda t, s, p: None if (p < f_single).all() else f"{int((p >= f_single).sum())} rays return a copy's primitive")


def _nothing(sc):
    return lambda t, s, p: None


def _dup(name):
    sc = ts.dup_cases()[name]()
    return ts.duplicated(sc), _no_copy(sc.n_tris)


K7_FIXTURES = {
    "sheets": lambda: (ts.sheets(False), _shape0),
    "sheets_fine_first": lambda: (ts.sheets(True), _shape0),
    "sheets_far": lambda: (ts.sheets_far_from_their_plane(False), _shape0),
    "sheets_far_fine_first": lambda: (ts.sheets_far_from_their_plane(True), _shape0),
    "sheets_far_unpadded": lambda: (ts.sheets_far_unpadded(False), _shape0),
    "sheets_far_unpadded_fine_first": lambda: (ts.sheets_far_unpadded(True), _shape0),
    "dup_colon": lambda: _dup("colon"),
    "dup_vocalfold": lambda: _dup("vocalfold"),
    "dup_hello": lambda: _dup("hello"),
    "budget": lambda: (ts.budget(), _in01),
}
for _n, _f in ts.seam_cases().items():
    K7_FIXTURES[f"seam_{_n}"] = lambda f=_f: (f(), _nothing)
    K7_FIXTURES[f"seam_{_n}_relabelled"] = lambda f=_f: (ts.reversed_tris(f()), _nothing)
_BUILT = {}  # name -> (scene, oracle geometry, device geometry, closed-form check): built once, shared, never modified
_WANT = {}   # (name, spp, jitter) -> the oracle's hits


def _built(oracle, name):
    if name not in _BUILT:
        sc, expect = K7_FIXTURES[name]()
        go, gd, _ = _pair(oracle, sc)
        _BUILT[name] = (sc, go, gd, expect(sc))
    return _BUILT[name]


def _want(oracle, name, spp, jitter):
    key = (name, spp, jitter)
    if key not in _WANT:
        sc, go, _, _ = _built(oracle, name)
        _WANT[key] = go.trace_primary(scene_desc.camera_from_sensor(sc.camera), spp, jitter, seed=5)
    return _WANT[key]


def _k7_problems(oracle, monkeypatch, name, gd, spp, jitter, walks):
    """-> the list of what is wrong, over ALL the walks (one failing walk does not hide another)"""
    sc, _, _, expect = _built(oracle, name)
    cam = scene_desc.camera_from_sensor(sc.camera)
    t_o, s_o, p_o = _want(oracle, name, spp, jitter)
    n = cam.width * cam.height * spp
    bad, first = [], None
    for walk, env in walks.items():
        with Env(monkeypatch, env):
            t, s, p = (host(a) for a in gd.trace_primary(cam, spp, jitter, seed=5))
        assert t.shape == (n,) and s.shape == (n,) and p.shape == (n,)
        msg = expect(t, s, p)
        if msg:
            bad.append(f"{walk}: {msg}")
        dp = np.nonzero(p != p_o)[0]
        if dp.size:
            r = int(dp[0])
            bad.append(f"{walk}: {dp.size} of {n} rays return another primitive than the oracle; first: ray {r} (pixel {r // spp % cam.width}, {r // spp // cam.width}) "
                       f"prim {p[r]} t {t[r]!r}, oracle prim {p_o[r]} t {t_o[r]!r}")
        if (s != s_o).any():
            bad.append(f"{walk}: {int((s != s_o).sum())} rays return another shape than the oracle")
        if first is None:
            first = (walk, t, s, p)
        else:
            for what, a, b in (("t bits", bits(t), bits(first[1])), ("shapes", s, first[2]), ("prims", p, first[3])):
                if not np.array_equal(a, b):
                    bad.append(f"{walk}: {what} differ from the {first[0]} walk's on {int((a != b).sum())} rays")
    return bad, first


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("spp", [1, 3, 64])  # the 8x8-pixel, the odd and the 1-pixel packet layouts
@pytest.mark.parametrize("name", list(K7_FIXTURES))
def test_k7_every_walk_breaks_ties_by_the_smaller_primitive_id(oracle, monkeypatch, name, spp, jitter):
    """K7 trace_primary on every fixture through the tile bins, the wide walk, the binary octant walk, the per-lane walk and the bins' fallback
    branch: the closed-form expectation of the fixture (shape 0 / no copy's primitive / primitive 0 or 1), the oracle's primitive and shape on
    EVERY ray, and t bits, primitives and shapes identical across the walks."""
    _, _, gd, _ = _built(oracle, name)
    bad, _ = _k7_problems(oracle, monkeypatch, name, gd, spp, jitter, K7_WALKS)
    assert not bad, f"{name} spp={spp} jitter={jitter}:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("name", list(ts.seam_cases()))
def test_k7_relabelled_seams_give_the_oracles_pick_on_the_tied_rays(oracle, monkeypatch, name):
    """the un-jittered stock scenes, relabelled (triangle order reversed inside every mesh): on the rays whose pick the id order decides — found on the
    oracle — every walk returns, mapped back, the triangle the oracle returns for the relabelled scene: another one than before the relabelling."""
    sc = _built(oracle, f"seam_{name}")[0]
    p_o = _want(oracle, f"seam_{name}", 1, 0)[2]
    back_o = ts.map_back(_want(oracle, f"seam_{name}_relabelled", 1, 0)[2], sc)
    tied = back_o != p_o
    assert tied.sum() >= 5
    gd = _built(oracle, f"seam_{name}_relabelled")[2]
    cam = scene_desc.camera_from_sensor(sc.camera)
    bad = []
    for walk, env in K7_WALKS.items():
        with Env(monkeypatch, env):
            p = host(gd.trace_primary(cam, 1, 0, seed=5)[2])
        back = ts.map_back(p, sc)
        if not np.array_equal(back[tied], back_o[tied]):
            k = np.nonzero(tied & (back != back_o))[0]
            bad.append(f"{walk}: {k.size} of {int(tied.sum())} tied rays; first: ray {int(k[0])} prim {back[k[0]]} (oracle {back_o[k[0]]}, before the relabelling {p_o[k[0]]})")
    assert not bad, f"{name}:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", ["sheets", "dup_vocalfold"])
def test_k7_ties_under_every_wide_overlay_builder(oracle, monkeypatch, name, spp, jitter):
    """the three host builders of the 64-wide overlay (FFX_WIDE_BUILD, read by ffx_bvh_build_host) put the tied triangles into different clusters:
    the wide walk's hits — and the bins' — stay the oracle's, bit for bit the same under all three"""
    sc = _built(oracle, name)[0]
    seen, res = [], []
    for mode in ("area", "count", "layers"):
        monkeypatch.setenv("FFX_WIDE_BUILD", mode)
        _, gd, _ = _pair(oracle, sc)
        monkeypatch.delenv("FFX_WIDE_BUILD")
        seen.append((gd.info.n_wide, gd.info.wide_depth))
        bad, first = _k7_problems(oracle, monkeypatch, name, gd, spp, jitter, {"wide": {"FFX_BINS": "0"}, "bins": {}})
        assert not bad, f"{name} FFX_WIDE_BUILD={mode} spp={spp} jitter={jitter}:\n  " + "\n  ".join(bad)
        res.append(first)
    for k in (1, 2):
        assert np.array_equal(bits(res[0][1]), bits(res[k][1])) and np.array_equal(res[0][3], res[k][3])
    assert name != "dup_vocalfold" or len(set(seen)) > 1, seen  # (they really are different overlays)


def test_trace_rays_on_lattice_rays_equals_the_all_pairs_reference():
    """K7 trace_rays (the non-apex triangle test, per-lane walk): integer rays through the grid vertices (6 triangles tie) and edge midpoints (2 tie)
    of a dyadic sheet — ids and t bits equal the float32 all-pairs reference on every ray"""
    mesh, o, d, ties = ts.lattice()
    t_ref, p_ref, n_tied = ts.tri_hit_all_pairs(mesh.frames[0], mesh.tris, o, d)
    assert np.array_equal(n_tied, ties) and (p_ref >= 0).all()
    pool, tris, shape, off, *_ = scenes.flatten(scenes.SceneData([mesh], None))
    gd = ops.DeviceGeometry(pool, tris, shape, off)
    gd.update(np.eye(4, dtype=np.float32)[None])
    t, s, p = (host(a) for a in gd.trace_rays(dev(o), dev(d)))
    k = np.nonzero((p != p_ref) | (bits(t) != bits(t_ref)))[0]
    assert k.size == 0, f"{k.size} of {p.size} rays; first: direction {d[k[0]]} ({ties[k[0]]} triangles tie) prim {p[k[0]]} t {t[k[0]]!r}, reference prim {p_ref[k[0]]} t {t_ref[k[0]]!r}"
    assert (s == 0).all()


# ------------------------------------------------------------------ the render kernels: "appending an exact copy of every mesh changes nothing"
RENDER_WALKS = {"default": {}, "FFX_BINS=0": {"FFX_BINS": "0"}, "FFX_WIDE=0": {"FFX_WIDE": "0"}, "FFX_TRAVERSAL=lane": {"FFX_TRAVERSAL": "lane"}, "FFX_ENVELOPE=0": {"FFX_ENVELOPE": "0"}}
_RENDER = {}


def _render_pair(oracle, name):
    """-> (single scene, duplicated scene, their device geometries and albedo tables, the duplicate's oracle geometry, texture): built once per scene"""
    if name not in _RENDER:
        sc = ts.dup_cases()[name]()
        dup = ts.duplicated(sc)
        _, g1, a1 = _pair(oracle, sc)
        go2, g2, a2 = _pair(oracle, dup)
        _RENDER[name] = (sc, dup, g1, dev(a1), g2, dev(a2), go2, a2, splat_tex(sc) if sc.projector is not None else None)
    return _RENDER[name]


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("walk", list(RENDER_WALKS))
@pytest.mark.parametrize("name", ["colon", "vocalfold", "hello"])
def test_render_fwd_does_not_see_an_exact_copy_of_every_mesh(oracle, monkeypatch, name, walk, shadows):
    """K8 at 5 spp (several pixels per wave: bins_block) and 70 (a pixel per wave, R > 1 walks): primary and shadow walks.  GPU against GPU, bit for
    bit; the duplicate's image is also the oracle's within the radiance bounds."""
    sc, dup, g1, a1, g2, a2, go2, alb2, tex = _render_pair(oracle, name)
    sd1, sd2 = scene_desc.scene_desc(sc, shadows=shadows), scene_desc.scene_desc(dup, shadows=shadows)
    for spp in (5, 70):
        with Env(monkeypatch, RENDER_WALKS[walk]):
            one = g1.render_fwd(sd1, a1, tex, spp, seed=3)
            two = g2.render_fwd(sd2, a2, tex, spp, seed=3)
        assert float(one.max()) > 0.01
        assert torch.equal(one, two), f"{name} {walk} shadows={shadows} spp={spp}: {int((one != two).any(-1).sum())} pixels differ"
        if walk == "default":
            want = go2.render_fwd(sd2, alb2, host(tex) if tex is not None else np.zeros((1, 1), np.float32), spp, seed=3)
            assert_image_close(host(two), want, spp, what=f"{name} duplicated, shadows={shadows}, {spp} spp")


@pytest.mark.parametrize("walk", list(RENDER_WALKS))
@pytest.mark.parametrize("make", [ts.sheets, ts.sheets_far_from_their_plane, ts.sheets_far_unpadded])
def test_renders_do_not_see_a_coplanar_second_sheet(oracle, monkeypatch, make, walk):
    """the stacked sheets under a spot light, in both orders: render_fwd at 5 and 70 spp, render_aov and a max_depth = 3 path render (primary rays on
    the per-lane walk) give, bit for bit, the image of the first sheet alone; the ids are the first sheet's"""
    for fine_first in (False, True):
        sc = make(fine_first)
        one = ts.first_sheet_only(sc)
        _, g1, a1 = _pair(oracle, one)
        _, g2, a2 = _pair(oracle, sc)
        sd1, sd2 = scene_desc.scene_desc(one, shadows=True), scene_desc.scene_desc(sc, shadows=True)
        with Env(monkeypatch, RENDER_WALKS[walk]):
            for spp in (5, 70):
                i1, i2 = g1.render_fwd(sd1, dev(a1), None, spp, seed=3), g2.render_fwd(sd2, dev(a2), None, spp, seed=3)
                assert float(i1.min()) > 0.01
                assert torch.equal(i1, i2), f"fine_first={fine_first} {spp} spp: {int((i1 != i2).any(-1).sum())} pixels differ"
            (m1, v1), (m2, v2) = g1.render_aov(sd1, dev(a1), None, 5, seed=3), g2.render_aov(sd2, dev(a2), None, 5, seed=3)
            assert torch.equal(m1, m2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32)), f"fine_first={fine_first}: render_aov"
            lo = ops.AOV_CHANNELS["shape_index"][0]
            assert float(v2[..., lo].max()) == float(v1[..., lo].max())
            p1, p2 = g1.render_fwd(sd1, dev(a1), None, 5, seed=3, max_depth=3), g2.render_fwd(sd2, dev(a2), None, 5, seed=3, max_depth=3)
            assert torch.equal(p1, p2), f"fine_first={fine_first} max_depth=3: {int((p1 != p2).any(-1).sum())} pixels differ"


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("name", ["colon", "vocalfold", "hello"])
def test_other_render_entry_points_do_not_see_the_copy(oracle, name, shadows):
    """the gaussian film forward, the cache-writing forward, render_aov (every channel, the shape and triangle ids included) and a max_depth = 3 path
    render, whose bounce rays are lane walks from arbitrary origins: bit for bit the single scene's"""
    sc, dup, g1, a1, g2, a2, _, _, tex = _render_pair(oracle, name)
    spp = 5
    sd1, sd2 = scene_desc.scene_desc(sc, shadows=shadows), scene_desc.scene_desc(dup, shadows=shadows)
    f1, f2 = (scene_desc.scene_desc(s, shadows=shadows, rfilter="gaussian") for s in (sc, dup))
    assert torch.equal(g1.render_fwd(f1, a1, tex, spp, seed=3), g2.render_fwd(f2, a2, tex, spp, seed=3)), "gaussian film"
    c1, c2 = (torch.zeros(ops.render_cache_bytes_sd(sd, spp), dtype=torch.uint8, device="cuda") for sd in (sd1, sd2))
    i1, i2 = g1.render_fwd(sd1, a1, tex, spp, seed=3, cache=c1), g2.render_fwd(sd2, a2, tex, spp, seed=3, cache=c2)
    assert torch.equal(i1, i2) and torch.equal(i1, g1.render_fwd(sd1, a1, tex, spp, seed=3)), "cache-writing forward"
    (m1, v1), (m2, v2) = g1.render_aov(sd1, a1, tex, spp, seed=3), g2.render_aov(sd2, a2, tex, spp, seed=3)
    assert torch.equal(m1, m2) and torch.equal(m1, i1), "render_aov: image"
    for ch, (lo, n) in ops.AOV_CHANNELS.items():
        a, b = v1[..., lo:lo + n], v2[..., lo:lo + n]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"render_aov: {ch} differs on {int((a != b).any(-1).sum())} pixels"
    assert float(v1[..., ops.AOV_CHANNELS["prim_index"][0]].max()) < sc.n_tris + 1
    p1, p2 = g1.render_fwd(sd1, a1, tex, spp, seed=3, max_depth=3), g2.render_fwd(sd2, a2, tex, spp, seed=3, max_depth=3)
    assert torch.equal(p1, p2), f"max_depth=3: {int((p1 != p2).any(-1).sum())} pixels differ"
    assert not torch.equal(p1, i1)  # (the bounce adds light)


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("name", ["colon", "vocalfold"])
def test_texture_gradient_does_not_see_the_copy(oracle, name, shadows):
    """the projector texture's gradient (the scenes with a projector): bit-equal through the deterministic adjoint; the float-atomic adjoints —
    re-tracing and cached — within 1e-3 of the gradient's scale (their sums depend on the arrival order)"""
    sc, dup, g1, a1, g2, a2, _, _, tex = _render_pair(oracle, name)
    spp = 5
    sd1, sd2 = scene_desc.scene_desc(sc, shadows=shadows), scene_desc.scene_desc(dup, shadows=shadows)
    rng = np.random.default_rng(1)
    gimg = dev(rng.standard_normal((sc.camera.height, sc.camera.width, 3)).astype(np.float32))
    d1, d2 = g1.render_bwd(sd1, a1, spp, 3, gimg, deterministic=True), g2.render_bwd(sd2, a2, spp, 3, gimg, deterministic=True)
    scale = float(d1.abs().max())
    assert scale > 0
    assert torch.equal(d1, d2), f"render_bwd_det: {int((d1 != d2).sum())} texels differ"
    c1, c2 = (torch.zeros(ops.render_cache_bytes_sd(sd, spp), dtype=torch.uint8, device="cuda") for sd in (sd1, sd2))
    g1.render_fwd(sd1, a1, tex, spp, seed=3, cache=c1)
    g2.render_fwd(sd2, a2, tex, spp, seed=3, cache=c2)
    for what, x, y in (("render_bwd", g1.render_bwd(sd1, a1, spp, 3, gimg, deterministic=False), g2.render_bwd(sd2, a2, spp, 3, gimg, deterministic=False)),
                       ("render_bwd_cached", g1.render_bwd_cached(sd1, a1, c1, spp, gimg), g2.render_bwd_cached(sd2, a2, c2, spp, gimg))):
        for who, g in (("single", x), ("duplicated", y)):
            err = (g - d1).abs()
            assert float((err > 1e-3 * scale).float().mean()) <= 2e-4 and float(err.max()) <= 0.1 * scale, (what, who, float(err.max()) / scale)
