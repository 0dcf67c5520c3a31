"""The seam fixtures of tests/seam_scenes.py, proved on the CPU oracle, and the oracle's tree held to its own tree-free mode.

DESIGN.md 4.1: boxes can only be hit more often than in exact arithmetic; the triangle test alone decides.  `oracle.tree_free()` is that
sentence as a mode — every box test skipped, every leaf visited — and is itself pinned here against tie_scenes.tri_hit_all_pairs, an
independent numpy statement of the triangle test.  Then, on EVERY ray of every fixture: the oracle with its tree == the oracle without.

With the leaf pad of 4e-7 of a box's own coordinates and no absolute term (the pad before ffx_bvh_info.leaf_pad) the second comparison
fails, measured on these fixtures (rays whose primitive / whose t bits differ):
    trace_rays    ridge+0.25 105 / 2     ridge-0.25 136 / 0     flat 30 / 0     wobbled_edge_of_range 6 / 2      (of 40 000 each)
    trace_primary wobbled_far 105 / 0, wobbled_far_narrow 23 / 0 of 196 608; wobbled_near, axis_parallel_*, wobbled_edge_of_range 0
    stock scenes  trace_primary: vocalfold 242 / 101 on 8 of the 48 cameras (|k| <= 1.25), colon 147 / 60 on 4 (k = -1 .. -1/4), of 4 096 each
The tree never returned a miss where the tree-free walk hit; it returned the neighbour across the seam.  CPU only."""
import numpy as np
import pytest

from fireflies_amd import scenes, scene_desc
from tests import seam_scenes as ss
from tests.support import bits, host_tex, oracle_geom

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _differences(what, got, want):
    """-> [] or the list of what differs between two (t, shape, prim) answers, over all rays"""
    (t, s, p), (tw, sw, pw) = got, want
    bad = []
    dp = np.nonzero(p != pw)[0]
    if dp.size:
        r = int(dp[0])
        lost = int(((p < 0) & (pw >= 0)).sum())
        bad.append(f"{what}: prim differs on {dp.size} of {p.size} rays ({lost} of them a miss where the tree-free walk hits); first: ray {r} prim {p[r]} t {t[r]!r}, "
                   f"tree-free prim {pw[r]} t {tw[r]!r}")
    if (bits(t) != bits(tw)).any():
        bad.append(f"{what}: t bits differ on {int((bits(t) != bits(tw)).sum())} rays")
    if (s != sw).any():
        bad.append(f"{what}: shape differs on {int((s != sw).sum())} rays")
    return bad


# ------------------------------------------------------------------ trace_rays: the non-apex test
def _ray_case(oracle, name):
    def make():
        mesh, eye = ss.RAY_FIXTURES[name]()
        g, _ = oracle_geom(oracle, scenes.SceneData([mesh], None))
        o, d, k = ss.grazing_rays(eye)
        with oracle.tree_free():
            free = g.trace_rays(o, d)
        return mesh, g, o, d, k, free
    return _once(("rays", name), make)


@pytest.mark.parametrize("name", list(ss.RAY_FIXTURES))
def test_tree_free_oracle_equals_the_all_pairs_reference_on_grazing_rays(oracle, name):
    """pins the new mode against an independent statement: t bits and prim of every ray"""
    mesh, g, o, d, k, (t, s, p) = _ray_case(oracle, name)
    t_ref, p_ref = ss.all_pairs(mesh, o, d)
    np.testing.assert_array_equal(p, p_ref)
    np.testing.assert_array_equal(bits(t), bits(t_ref))
    assert ((s == 0) == (p >= 0)).all()


@pytest.mark.parametrize("name", list(ss.RAY_FIXTURES))
def test_grazing_rays_land_beside_the_seam_on_the_side_they_aim_at(oracle, name):
    """meaningfulness: the rays hit (the test is not watertight ON an edge: under 1 % fall through the seam, in both walks alike), the hit is
    within a few ulp of the seam, and for each sign of k at least 95 % of the rays land on that side"""
    mesh, g, o, d, k, (t, s, p) = _ray_case(oracle, name)
    assert (p >= 0).mean() > 0.99
    side = ss.side_of_prim(mesh)
    y = o[:, 1] + t.astype(np.float64) * d[:, 1]
    assert np.abs(y[p >= 0]).max() < 1e-4
    for sg in (-1, 1):
        m = (np.sign(k) == sg) & (p >= 0)
        assert m.sum() > 15000 and (side[p[m]] == sg).mean() >= 0.95, (name, sg, float((side[p[m]] == sg).mean()))


@pytest.mark.parametrize("name", list(ss.RAY_FIXTURES))
def test_trace_rays_with_the_tree_equals_tree_free_on_every_grazing_ray(oracle, name):
    mesh, g, o, d, k, free = _ray_case(oracle, name)
    bad = _differences(name, g.trace_rays(o, d), free)
    assert not bad, "\n  ".join(bad)


# ------------------------------------------------------------------ trace_primary: the apex test
def _cam_case(oracle, name):
    def make():
        mesh, eye, fov = ss.CAM_FIXTURES[name]()
        g, _ = oracle_geom(oracle, scenes.SceneData([mesh], None))
        cams = ss.pitched_cameras(eye, fov=fov)
        with oracle.tree_free():
            free = [g.trace_primary(scene_desc.camera_from_sensor(c), 1, 0, 0) for c in cams]
        return mesh, g, cams, free
    return _once(("cams", name), make)


@pytest.mark.parametrize("name", list(ss.CAM_FIXTURES))
def test_pitched_cameras_hit_on_the_centre_row_and_land_on_the_side_of_their_pitch(oracle, name):
    """meaningfulness: every ray of the centre row that is aimed at the sheet hits (from 9.1 away the 50-degree film is wider than the
    sheet — 9.1 tan 25 = 4.24 > 4 — so its outermost columns must miss) once the pitch is a whole 2^-23 or more; below that the rays run
    within an ulp of the seam itself, where the test is not watertight (up to 104 of 2048 fall through the wobbled seam at
    k = -1/4, with and without the tree alike), and 90 % must hit.  For each sign of k at least 95 % of the centre row's hits are on that side."""
    mesh, g, cams, free = _cam_case(oracle, name)
    side = ss.side_of_prim(mesh)
    on = {-1: [], 1: []}
    for k, cam, (t, s, p) in zip(ss.KS, cams, free):
        row = p[ss.FILM_W:]
        aimed = ss.aimed_at_sheet(cam)
        assert aimed.all() if name not in ("wobbled_far", "axis_parallel_far") else aimed.mean() > 0.9, (name, k)  # (every other film lies on the sheet: exact)
        assert (row[aimed] >= 0).mean() >= (1.0 if abs(k) >= 1 else 0.9), (name, k, int((row[aimed] < 0).sum()))
        on[int(np.sign(k))].append(side[row[row >= 0]] == int(np.sign(k)))
    for sg in (-1, 1):
        frac = float(np.concatenate(on[sg]).mean())
        assert frac >= 0.95, (name, sg, frac)


@pytest.mark.parametrize("name", list(ss.CAM_FIXTURES))
def test_trace_primary_with_the_tree_equals_tree_free_on_every_ray(oracle, name):
    mesh, g, cams, free = _cam_case(oracle, name)
    bad = []
    for k, cam, want in zip(ss.KS, cams, free):
        bad += _differences(f"{name} k={k:+.2f}", g.trace_primary(scene_desc.camera_from_sensor(cam), 1, 0, 0), want)
    assert not bad, f"{len(bad)} findings:\n  " + "\n  ".join(bad[:12])


# ------------------------------------------------------------------ the small stock scenes: primary and shadow rays
@pytest.mark.parametrize("name", ["vocalfold", "colon"])
def test_stock_scenes_trace_and_render_the_same_with_the_tree_and_tree_free(oracle, name):
    """the pitched cameras in the scenes' plane of symmetry, the spot in it too: trace_primary on every ray, and render_fwd with shadows on
    (jittered: primary, projector-shadow and spot-shadow walks) bit for bit — the oracle's sample order does not depend on the walk.  The
    cameras of k a multiple of 1/2 render at 1 spp and those of ss.RENDER_KS, which tests/test_seams_gpu.py renders, at its 8 spp (a tree-free
    render tests every sample against every triangle: 8 spp on all 48 cameras would take minutes).  Only the trace_primary half is shown to
    detect the defect: with the leaf pad's absolute term zeroed it fails with the counts above, and no render comparison of these cameras does."""
    sc, eye, target = ss.stock(name)
    g, alb = oracle_geom(oracle, sc)
    tex = host_tex(sc)
    bad, lit = [], 0.0
    for k, cam in zip(ss.KS, ss.pitched_cameras(eye, target=target)):
        sck = ss.with_camera(sc, cam)
        c = scene_desc.camera_from_sensor(cam)
        sd = scene_desc.scene_desc(sck, shadows=True)
        with oracle.tree_free():
            want = g.trace_primary(c, 1, 0, 0)
        assert (want[2][ss.FILM_W:] >= 0).mean() > 0.5, (name, k)  # (the tubes are open at the far end: the middle of the row looks out)
        bad += _differences(f"{name} k={k:+.2f}", g.trace_primary(c, 1, 0, 0), want)
        for spp in ((8,) if k in ss.RENDER_KS else ()) + ((1,) if 2 * k == int(2 * k) else ()):
            with oracle.tree_free():
                img_free = g.render_fwd(sd, alb, tex, spp, seed=3)
            img = g.render_fwd(sd, alb, tex, spp, seed=3)
            lit = max(lit, float(img_free.max()))
            if not np.array_equal(img.view(np.uint32), img_free.view(np.uint32)):
                bad.append(f"{name} k={k:+.2f} {spp} spp: render_fwd differs on {int((img != img_free).any(-1).sum())} pixels")
    assert lit > 0.01
    assert not bad, f"{len(bad)} findings:\n  " + "\n  ".join(bad[:12])
