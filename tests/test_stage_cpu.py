"""tests/stage_scenes.py on the CPU: (i) the oracle against the independent float64 restatement (tests/ref_bruteforce.py) on every scene and
variant that tests/test_stage_gpu.py renders — until now the two references had only met on scenes whose emitters stand beside the camera;
(ii) each scene does what it is for, as geometric facts stated in numpy from the scene itself (no restatement of the pre-pass classifier)."""
import numpy as np
import pytest

from fireflies_amd import scene_desc, scenes
from tests import ref_bruteforce as bf
from tests import stage_scenes as ss

W, H, SPP = 48, 40, 4


def _geometry(oracle, sc):
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    go = oracle.Geometry(pool, tris, shape, off)
    go.update(np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)))
    return go, alb, pool.astype(np.float64), tris + off[shape][:, None], shape


def _desc(sc, frame, shadows, **kw):
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows, **kw)
    return sd if frame is None else ss.set_spot_frame(sd, frame)


# ----------------------------------------------------------------------------- (i) oracle against the float64 restatement
@pytest.mark.parametrize("base", ["side_lit", "facing"])
def test_primary_hits_agree_with_the_bruteforce_restatement(oracle, base):
    """K7 on the two stages, jittered (un-jittered, the centre row and column of `facing` lie exactly in the tube's planes of symmetry, where
    its seams are: exact ties, which tests/test_seams_*.py are about), in the form of tests/test_bruteforce_cpu.py: the same primitive on
    99.8 % of the rays, t to 2e-5.  Observed: every ray of both scenes hits the same primitive (share of different hits 0)."""
    sc = {"side_lit": ss.side_lit, "facing": ss.facing}[base](W, H)
    go, alb, verts, gidx, shape = _geometry(oracle, sc)
    cam = scene_desc.camera_from_sensor(sc.camera)
    for seed in (5, 6):
        t_o, s_o, p_o = go.trace_primary(cam, SPP, 1, seed=seed)
        t_b, s_b, p_b = bf.trace_primary(verts, gidx, shape, cam, SPP, True, seed)
        same = (p_o == p_b) & (s_o == s_b)
        print(f"{base} seed={seed}: {1 - same.mean():.2e} of the rays hit a different primitive")
        assert same.mean() >= 0.998
        assert (p_o >= 0).mean() > 0.3
        np.testing.assert_allclose(t_o[same], t_b[same], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("case", sorted(ss.CASES))
def test_oracle_agrees_with_the_bruteforce_restatement_on_the_stages(oracle, case):
    """render_fwd with shadows on and off and render_bwd (texture gradient) at 48 x 40 x 4 spp, jittered, with the bounds of
    tests/test_bruteforce_cpu.py::test_oracle_agrees_with_an_independent_bruteforce_restatement: 2e-4 of the scale on all but 1 % of the pixel
    channels, no channel off by more than 1.5 scale / spp, means within 2e-3; gradient: 1e-3 of its scale on all but 1 % of the texels, none
    off by more than half of it.  The scenes whose emitters see nothing must be exactly black in both.

    Observed on every case: NO pixel channel beyond 2e-4 of the scale (worst 1.7e-5 of the scale, facing at 3 degrees) and no texel beyond 1e-3 of
    the gradient's scale (worst 2.3e-5): float32 against float64 rounding only, not one flipped sample."""
    sc, frame = ss.build(case, W, H)
    go, alb, verts, gidx, shape = _geometry(oracle, sc)
    rng = np.random.default_rng(1)
    tex = rng.random((sc.projector.height, sc.projector.width)).astype(np.float32)
    gimg = rng.standard_normal((H, W, 3)).astype(np.float32)
    dark = case.startswith("away_")
    scale = None
    for shadows in (True, False):
        sd = _desc(sc, frame, shadows)
        img_o = go.render_fwd(sd, alb, tex, SPP, seed=9)
        img_b = bf.render_fwd(verts, gidx, shape, sd, alb, tex, SPP, 9)
        if dark:
            assert np.all(img_o == 0) and np.all(img_b == 0)
            continue
        if scale is None:
            scale = float(img_b.max())
        assert scale > 0.01
        err = np.abs(img_o - img_b)
        print(f"{case} shadows={shadows}: {(err > 2e-4 * scale).mean():.2e} of the pixel channels differ, worst {err.max() / scale:.2e} of the scale")
        assert (err > 2e-4 * scale).mean() <= 1e-2
        assert err.max() <= 1.5 * scale / SPP
        assert abs(float(img_o.mean()) - float(img_b.mean())) <= 2e-3 * float(img_b.mean())
    sd = _desc(sc, frame, True)
    gt_o = go.render_bwd(sd, alb, SPP, 9, gimg)[..., 0]
    gt_b = bf.render_bwd(verts, gidx, shape, sd, alb, SPP, 9, gimg)
    if dark or case.endswith("_projector_away"):
        assert np.all(gt_o == 0) and np.all(gt_b == 0)
        return
    gs = float(np.abs(gt_b).max())
    assert gs > 0
    gerr = np.abs(gt_o - gt_b)
    print(f"{case} gradient: {(gerr > 1e-3 * gs).mean():.2e} of the texels differ, worst {gerr.max() / gs:.2e} of the scale")
    assert (gerr > 1e-3 * gs).mean() <= 1e-2 and gerr.max() <= 0.5 * gs


# ----------------------------------------------------------------------------- (ii) the scenes do what they are for
@pytest.mark.parametrize("emitter", ["projector", "spot"])
def test_side_lit_casts_shadows_the_camera_sees(oracle, emitter):
    """under each emitter alone, at least 15 % of the lit pixel channels change when the shadows are switched off (observed: projector 57 %,
    spot 28 %; scenes.vocalfold: under 1 %)"""
    sc = ss.side_lit(W, H)
    go, alb, *_ = _geometry(oracle, sc)
    tex = np.random.default_rng(1).random((sc.projector.height, sc.projector.width)).astype(np.float32) + 0.05
    img = {}
    for shadows in (True, False):
        sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows)
        if emitter == "projector":
            sd.spot.enabled = 0
        else:
            sd.proj.enabled = 0
        img[shadows] = go.render_fwd(sd, alb, tex, SPP, seed=9)
    lit = img[False] > 0
    share = float((img[True] != img[False])[lit].mean())
    print(f"side_lit, {emitter} alone: {lit.mean():.2f} of the pixel channels lit, {share:.2f} of them change without shadows")
    assert lit.mean() > 0.1 and share >= 0.15
    assert np.all(img[True] <= img[False])  # (a shadow only ever removes light)


def test_side_lit_floor_spans_more_than_sixteen_tiles_of_every_grid():
    """each of the floor's two triangles, cut at the apex plane and projected, contains the CENTRES of more than sixteen tiles of the camera's
    grid (12 x 10 and 8 x 6 tiles), the spot's (70 x 70) and — with the 104 x 88 texture — the projector's (7 x 6).  The default 40 x 24 texture
    has 3 x 2 tiles in all: there the grid is the part-filled one, and no triangle can span more than six."""
    for sc in (ss.side_lit(96, 80, 104, 88), ss.side_lit(64, 48, 104, 88)):
        floor = ss.world_tris(sc)[:2]
        for name, to_world, to_tiles, nx, ny in ss.tile_grids(sc):
            n = [ss.tiles_covered(to_tiles(ss.clip_front(ss.local(to_world, t))), nx, ny) for t in floor]
            print(f"{sc.camera.width}x{sc.camera.height} {name}: {nx} x {ny} tiles, the floor's triangles hold {n} tile centres")
            assert max(n) > 16, (name, n)
    sc = ss.side_lit()
    _, _, _, nx, ny = ss.tile_grids(sc)[1]
    assert (nx, ny) == (3, 2) and sc.projector.width % 16 and sc.projector.height % 16
    assert ss.tile_grids(ss.facing())[1][3:] == (2, 3)


def _emitters(sc):
    return (("projector", sc.projector.to_world, lambda pl: ss.in_frustum(sc.projector, pl)),
            ("spot", sc.spot.to_world, lambda pl: ss.in_cone(sc.spot.cutoff_angle, pl)))


def test_facing_has_geometry_behind_and_beside_both_apexes():
    """projector and 74-degree spot: at least 8 triangles wholly behind the apex plane (local z <= 0 at all three vertices) and at least 8 that
    straddle it and still have a vertex inside the frustum / cone.  Observed: projector 127 behind, 58 straddle, 8 of them with a lit vertex;
    spot 478 / 104 / 8 — the eight are the fin's long triangles; the tube's own straddlers lie 80 degrees and more off either axis."""
    sc = ss.facing(cutoff=74.0)
    tris = ss.world_tris(sc)
    for name, to_world, inside in _emitters(sc):
        pl = ss.local(to_world, tris)
        z = pl[..., 2]
        behind = (z <= 0).all(1)
        straddle = (z <= 0).any(1) & (z > 0).any(1)
        reached = straddle & inside(pl).any(1)
        print(f"facing, {name}: {behind.sum()} triangles behind the apex plane, {straddle.sum()} straddle it, {reached.sum()} of those have a vertex inside")
        assert behind.sum() >= 8 and reached.sum() >= 8
        assert inside(pl).any(1).sum() > 100  # (and it lights something)


@pytest.mark.parametrize("base", ["side_lit", "facing"])
def test_away_leaves_nothing_in_front_of_either_emitter(base):
    sc = ss.away({"side_lit": ss.side_lit, "facing": ss.facing}[base]())
    tris = ss.world_tris(sc)
    for name, to_world, inside in _emitters(sc):
        assert not inside(ss.local(to_world, tris)).any(), name
    for which, other in (("projector", 1), ("spot", 0)):  # one at a time: the other emitter still lights the scene
        one = ss.away({"side_lit": ss.side_lit, "facing": ss.facing}[base](), (which,))
        name, to_world, inside = _emitters(one)[other]
        assert inside(ss.local(to_world, ss.world_tris(one))).any(), name


def test_spot_frames_lie_on_the_intended_side_of_the_hosts_threshold():
    """the host's measure (max |W W^T - 1| over the 3x3 part of to_world^-1, here in float64 from the float32 matrix the ABI carries) against
    its threshold 2e-6.  Observed: rigid 4e-8, nearly_rigid 1.08e-6, just_not 4.04e-6, scaled 0.75, squeezed 1.78 — and mirrored 4e-8: a
    reflection IS orthonormal, |l| = |w| holds and l.z is one row of the matrix, so the rotation shortcut is exact for it and the host rightly
    takes it (only a determinant would tell it from a rotation, and the cone does not depend on it)."""
    m = {}
    for name, frame in ss.spot_frames().items():
        m[name] = ss.spot_rigid_measure(ss.set_spot_frame(scene_desc.scene_desc(ss.side_lit(), tex_channels=1), frame))
    print(m)
    for name in ("rigid", "nearly_rigid", "mirrored"):
        assert m[name] < ss.SPOT_RIGID_TOL, (name, m[name])
    for name in ("scaled", "squeezed", "just_not"):
        assert m[name] > ss.SPOT_RIGID_TOL, (name, m[name])
    assert m["nearly_rigid"] > 0.5 * ss.SPOT_RIGID_TOL and m["just_not"] < 4 * ss.SPOT_RIGID_TOL  # (the pair brackets the threshold closely)
