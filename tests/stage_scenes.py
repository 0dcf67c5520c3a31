"""Scenes whose emitters stand APART from the camera — TEST INFRASTRUCTURE (numpy only).

In scenes.vocalfold and scenes.colon the camera, the projector and the spot stand within 0.25 units of each other and look at the same target:
almost nothing the camera sees lies in an emitter's shadow, every emitter grid sees the geometry the way the camera's does, the projector
texture is square and the spot's frame is a rotation.  What K8 does for speed depends on exactly that arrangement — the envelopes
(k_bin_env / bins_shadow: a proof that a shadow packet may skip its any-hit stage; a wrong proof is a light leak, visible only where an
occluder stands between an emitter and a surface the camera sees), the pre-pass classes of k_bin (behind the apex plane / few tiles / many
tiles / projection not trusted), the spot's rotation shortcut (ShadeK.s_rigid) and the spot grid's cone limits.  The builders here move
the emitters; tests/test_stage_cpu.py proves on the oracle and the float64 restatement that each scene does what it is for, and
tests/test_stage_gpu.py holds the HIP kernels to the oracle on them.

  side_lit()        a floor of TWO triangles, a cube, a sphere and a leaning slab; the projector grazes the floor from the side, the spot
                    shines from behind: long cast shadows under both, a non-square texture whose last tiles are part-filled
  facing(cutoff)    the larynx tube, a sphere and two fins; the projector looks BACK at the camera from the far end (half the tube behind it,
                    rings of the tube beside its apex), the spot stands inside and is aimed sideways at the wall; its cone is a parameter
  away(sc, which)   the same scene with the projector and / or the spot re-aimed at nothing
  swapped(sc)       the projector in the spot's pose and the spot in the projector's
  spot_frames()     3x3 matrices to right-multiply into the spot's to_world: rotation, scale, shear, mirror, and the two sides of the
                    host's orthonormality threshold;  set_spot_frame(sd, F) writes one into a finished ffx_scene_desc
  CASES             name -> builder of every scene variant the two test modules render
"""
import ctypes as C
from dataclasses import replace

import numpy as np

from fireflies_amd import scenes

F32 = np.float32
SPOT_RIGID_TOL = 2e-6  # ffx_trace.hip shade_prepare: rows of the spot's world-to-local orthonormal to this -> ShadeK.s_rigid


def _mesh(name, v, t, albedo, principled):
    return scenes.MeshData("mesh-" + name, np.ascontiguousarray(v, F32)[None], np.ascontiguousarray(t, np.int32), albedo, "mat-" + name,
                           {} if principled else None)


# ----------------------------------------------------------------------------- side_lit
def side_lit(width=96, height=80, tex_w=40, tex_h=24, principled=False):
    """floor in y = 0 (half-width 4, two triangles), cube, 16x8 uv-sphere, a thin slab leaning over the floor between the projector and the
    middle of the stage.  Camera (0.5, 3, 4.5) -> (0, 0.3, 0), fov 50.  Projector (5, 1.2, 0.5) -> (0, 0.3, 0), fov 50: 13 degrees above the
    floor, every object throws a shadow several times its height.  Spot (-3, 4, -2.5) -> origin, cutoff 35, beam 25: behind the objects as
    the camera sees them, their shadows fall towards the camera.  Texture 40 x 24: 3 x 2 tiles of 16 texels, the last column and row
    part-filled (104 x 88: 7 x 6 tiles, also part-filled, in which the floor spans more than sixteen)."""
    gv, gt = scenes.make_plane(0.0, 4.0, 1, 1)
    gv = gv[:, [0, 2, 1]].copy()
    cv, ct = scenes.make_cube((-0.8, 0.5, 0.2), 0.5)
    sv, st = scenes.make_uv_sphere((0.9, 0.6, -0.3), 0.6, 16, 8)
    # the slab: 1.4 x 0.04 x 0.9, turned 55 degrees about z so that it leans towards the projector, its lower edge 0.02 above the floor
    bv, bt = scenes.make_cube((0.0, 0.0, 0.0), 1.0)
    bv = bv.astype(np.float64) * (0.7, 0.02, 0.45)
    a = np.deg2rad(55.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    bv = bv @ R.T
    bv += (2.3, 0.02 - bv[:, 1].min(), 1.3)
    cam = scenes.SensorData("PerspectiveCamera", scenes.look_at((0.5, 3.0, 4.5), (0.0, 0.3, 0.0)), 50.0, 0.01, 100.0, width, height)
    proj = scenes.SensorData("PerspectiveCamera_1", scenes.look_at((5.0, 1.2, 0.5), (0.0, 0.3, 0.0)), 50.0, 0.01, 100.0, tex_w, tex_h)
    spot = scenes.SpotData("emit-Spot", scenes.look_at((-3.0, 4.0, -2.5), (0.0, 0.0, 0.0)), (40.0, 40.0, 40.0), 35.0, 25.0)
    return scenes.SceneData(
        [_mesh("Floor", gv, gt, (0.6, 0.6, 0.6), principled), _mesh("Cube", cv, ct, (0.8, 0.3, 0.2), principled),
         _mesh("Ball", sv, st, (0.3, 0.5, 0.8), principled), _mesh("Slab", bv, bt, (0.7, 0.7, 0.3), principled)],
        cam, proj, spot, projector_scale=20.0, notes={"config": "side_lit"})


# ----------------------------------------------------------------------------- facing
def facing(width=96, height=80, tex_w=24, tex_h=40, cutoff=74.0, principled=False):
    """the larynx tube (24 x 32 quads, z 0..6, radius 1.25 plus scenes.vocalfold's ripple), a uv-sphere and two fins inside it.  Camera (0, 0, 0.6)
    looking down +z, fov 70.  Projector (0.2, 0.1, 5.4) looking back at the origin, fov 60: what the camera sees is lit from the front, the
    sphere's shadow falls towards the camera, and the tube's last rings lie beside and behind the projector's apex.  Spot (0, 0.2, 2.0) aimed
    sideways at the wall at (1.25, 0.3, 3.0), cutoff `cutoff`, beam 0.75 cutoff: at 74 degrees most of the tube is inside the cone and a
    third of it behind the apex plane."""
    tv, tt = scenes._tube(24, 32, 0.0, 6.0, lambda t, z: 1.25 + 0.08 * np.sin(3 * t) * np.sin(1.3 * z) + 0.05 * np.cos(2.1 * z))
    sv, st = scenes.make_uv_sphere((0.3, -0.2, 3.2), 0.45, 16, 8)
    # two fins, 1 x 4 quads each, that pass BESIDE an emitter's apex and reach into its frustum / cone: every one of their long triangles has a
    # vertex behind the apex plane and a vertex the emitter lights (the tube's own triangles are too small for that: the ones that straddle an
    # apex plane lie 80 degrees and more off the axis).  One under the projector, along the tube; one under the spot, across it.
    pv, pt = scenes.make_plane(0.0, 1.0, 4, 1)
    pv = pv.astype(np.float64)
    fin_p = np.stack([0.2 + 0.5 * pv[:, 0], np.full(len(pv), -0.45), 5.1 + 0.8 * pv[:, 1]], -1)  # x -0.3 .. 0.7, y -0.45, z 4.3 .. 5.9
    fin_s = np.stack([0.1 + 0.8 * pv[:, 1], np.full(len(pv), -0.3), 2.3 + 0.6 * pv[:, 0]], -1)  # x -0.7 .. 0.9, y -0.3, z 1.7 .. 2.9
    fv, ft = np.concatenate([fin_p, fin_s]), np.concatenate([pt, pt + len(pv)])
    cam = scenes.SensorData("PerspectiveCamera", scenes.look_at((0.0, 0.0, 0.6), (0.0, 0.0, 5.0)), 70.0, 0.01, 100.0, width, height)
    proj = scenes.SensorData("PerspectiveCamera_1", scenes.look_at((0.2, 0.1, 5.4), (0.0, 0.0, 0.0)), 60.0, 0.01, 100.0, tex_w, tex_h)
    spot = scenes.SpotData("emit-Spot", scenes.look_at((0.0, 0.2, 2.0), (1.25, 0.3, 3.0)), (8.0, 8.0, 8.0), float(cutoff), 0.75 * float(cutoff))
    return scenes.SceneData([_mesh("Larynx", tv, tt, (0.80, 0.32, 0.34), principled), _mesh("Ball", sv, st, (0.3, 0.5, 0.8), principled),
                             _mesh("Fins", fv, ft, (0.7, 0.7, 0.3), principled)],
                            cam, proj, spot, projector_scale=6.0, notes={"config": "facing"})


# ----------------------------------------------------------------------------- re-aimed emitters
def away(sc, which=("projector", "spot")):
    """`sc` with the named emitters re-aimed so that no geometry lies in front of them (the positions stay).  side_lit: the projector stands
    outside the floor's edge and turns its back on the stage, the spot looks straight up.  facing: the projector looks out of the tube's
    far end, the spot out of its near end — from inside a tube no direction is free under a 74-degree cone, so the spot's cone is narrowed
    to 20 / 15 degrees as well (the near opening is 29 degrees wide from where it stands)."""
    proj, spot = sc.projector, sc.spot
    side = sc.notes["config"] == "side_lit"
    if "projector" in which:
        p = proj.to_world[:3, 3].astype(np.float64)
        proj = replace(proj, to_world=scenes.look_at(p, p + ((5.0, 1.8, 0.0) if side else (0.0, 0.0, 5.0))))
    if "spot" in which:
        p = spot.to_world[:3, 3].astype(np.float64)
        if side:
            spot = replace(spot, to_world=scenes.look_at(p, p + (0.0, 5.0, 0.0), up=(0.0, 0.0, 1.0)))
        else:
            spot = replace(spot, to_world=scenes.look_at(p, p + (0.0, 0.0, -5.0)), cutoff_angle=20.0, beam_width=15.0)
    return replace(sc, projector=proj, spot=spot)


def swapped(sc):
    """`sc` with the projector in the spot's pose and the spot in the projector's"""
    return replace(sc, projector=replace(sc.projector, to_world=sc.spot.to_world.copy()), spot=replace(sc.spot, to_world=sc.projector.to_world.copy()))


# ----------------------------------------------------------------------------- spot frames
def spot_frames():
    """name -> 3x3 float64, right-multiplied into the rotation part of the spot's to_world (the local axes are scaled / sheared / mirrored, the
    position stays).  The cone is cos_t = l.z / |l| of the LOCAL direction l = to_world^-1 w: `scaled` and `mirrored` describe the same cone as
    `rigid` (a uniform scale cancels, the cone is symmetric about its axis), `squeezed` an elliptic one.  `nearly_rigid` and `just_not` sit on
    the two sides of SPOT_RIGID_TOL: a scale of 1 + e moves the measure by 2 e.  `mirrored` is orthonormal — a reflection — and so lies on
    the rigid side of the host's measure, rightly: |l| = |w| and l.z is one row of the matrix (tests/test_stage_cpu.py)."""
    return {
        "rigid": np.eye(3),
        "scaled": 2.0 * np.eye(3),
        "squeezed": np.array([[1.0, 0.3, 0.0], [0.0, 0.6, 0.0], [0.0, 0.0, 1.0]]),
        "mirrored": np.diag([-1.0, 1.0, 1.0]),
        "nearly_rigid": (1.0 + 5e-7) * np.eye(3),
        "just_not": (1.0 + 2e-6) * np.eye(3),
    }


def set_spot_frame(sd, frame):
    """sd.spot.to_world[:3, :3] <- sd.spot.to_world[:3, :3] @ frame (formed in float64, stored as the float32 the ABI carries) -> sd"""
    m = np.array(list(sd.spot.to_world), np.float64).reshape(4, 4)
    m[:3, :3] = m[:3, :3] @ np.asarray(frame, np.float64)
    sd.spot.to_world = (C.c_float * 16)(*m.astype(F32).reshape(-1).tolist())
    return sd


def spot_rigid_measure(sd):
    """the host's orthonormality measure of the spot's frame, restated in float64: max |W W^T - 1| over the 3x3 part W of to_world^-1"""
    w = np.linalg.inv(np.array(list(sd.spot.to_world), np.float64).reshape(4, 4))[:3, :3]
    return float(np.abs(w @ w.T - np.eye(3)).max())


# ----------------------------------------------------------------------------- the variants both test modules render
# name -> (builder(width, height) -> SceneData, spot frame or None)
CUTOFFS = (3.0, 74.0, 75.0, 75.5)
CASES = {"side_lit": (lambda w, h: side_lit(w, h), None), "side_lit_104x88": (lambda w, h: side_lit(w, h, 104, 88), None)}
for _c in CUTOFFS:
    CASES[f"facing_{_c:g}"] = (lambda w, h, c=_c: facing(w, h, cutoff=c), None)
for _n in spot_frames():
    if _n != "rigid":
        CASES["side_lit_spot_" + _n] = (lambda w, h: side_lit(w, h), _n)
for _b, _mk in (("side_lit", side_lit), ("facing", facing)):
    CASES[f"away_{_b}"] = (lambda w, h, mk=_mk: away(mk(w, h)), None)
    CASES[f"{_b}_projector_away"] = (lambda w, h, mk=_mk: away(mk(w, h), ("projector",)), None)
    CASES[f"{_b}_spot_away"] = (lambda w, h, mk=_mk: away(mk(w, h), ("spot",)), None)
CASES["side_lit_swapped"] = (lambda w, h: swapped(side_lit(w, h)), None)


def build(name, width, height):
    """-> (SceneData, spot frame [3,3] or None) of CASES[name]"""
    mk, frame = CASES[name]
    return mk(width, height), (None if frame is None else spot_frames()[frame])


# ----------------------------------------------------------------------------- geometry as an emitter sees it
def world_tris(sc):
    """[F,3,3] float64: the triangles' vertices (first frame, no transforms)"""
    return np.concatenate([m.frames[0].astype(np.float64)[m.tris] for m in sc.meshes])


def local(to_world, p):
    """points p [...,3] in the frame of to_world (float64)"""
    w = np.linalg.inv(np.asarray(to_world, np.float64).reshape(4, 4))
    return p @ w[:3, :3].T + w[:3, 3]


def in_frustum(sensor, pl):
    """local points inside the sensor's frustum: in front of the apex plane and sample coordinates in [0, 1]^2"""
    K = sensor.K.astype(np.float64)
    q = pl @ K[:3, :3].T + K[:3, 3]
    w = pl @ K[3, :3] + K[3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = q[..., 0] / w, q[..., 1] / w
    return (pl[..., 2] > 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)


def in_cone(cutoff_deg, pl):
    """local points inside the cone of half angle cutoff_deg about +z"""
    n = np.linalg.norm(pl, axis=-1)
    return (pl[..., 2] > 0) & (pl[..., 2] >= np.cos(np.deg2rad(cutoff_deg)) * n)


def spot_grid_n(cutoff_deg):
    """tiles per side of the spot's grid (about one degree per tile, 8 .. 128; none beyond 75 degrees)"""
    return min(128, max(8, int(2.0 * cutoff_deg + 0.999))) if 0.0 < cutoff_deg <= 75.0 else 0


def tile_grids(sc):
    """[(name, to_world, f(local points [n,3]) -> tile coordinates [n,2], nx, ny)] of the camera's, the projector's and the spot's tile grid:
    8-pixel tiles of the film, 16-texel tiles of the texture, and a square perspective grid of half angle cutoff + 1 degree about the cone's axis"""
    def sensor(s, tile):
        K = s.K.astype(np.float64)

        def f(pl):
            q = pl @ K[:3, :3].T + K[:3, 3]
            w = pl @ K[3, :3] + K[3, 3]
            return np.stack([q[:, 0] / w * s.width / tile, q[:, 1] / w * s.height / tile], -1)

        return f, -(-s.width // tile), -(-s.height // tile)

    n = spot_grid_n(sc.spot.cutoff_angle)
    tanc = np.tan(np.deg2rad(sc.spot.cutoff_angle + 1.0))
    return [("camera", sc.camera.to_world, *sensor(sc.camera, 8)), ("projector", sc.projector.to_world, *sensor(sc.projector, 16)),
            ("spot", sc.spot.to_world, lambda pl: 0.5 * n * (pl[:, :2] / (pl[:, 2:3] * tanc) + 1.0), n, n)]


def clip_front(tri, eps=1e-6):
    """the part of a local-space triangle [3,3] with z >= eps, as a polygon [n,3] (Sutherland-Hodgman against one plane; n = 0: nothing)"""
    out = []
    for i in range(3):
        a, b = tri[i], tri[(i + 1) % 3]
        ia, ib = a[2] >= eps, b[2] >= eps
        if ia:
            out.append(a)
        if ia != ib:
            out.append(a + (b - a) * (eps - a[2]) / (b[2] - a[2]))
    return np.asarray(out).reshape(-1, 3)


def tiles_covered(poly_xy, nx, ny):
    """how many tiles of an nx x ny grid have their CENTRE inside the convex polygon poly_xy [n,2] (tile units): a lower bound of the tiles it spans"""
    if len(poly_xy) < 3:
        return 0
    cx, cy = np.meshgrid(np.arange(nx) + 0.5, np.arange(ny) + 0.5)
    s = []
    for i in range(len(poly_xy)):
        a, b = poly_xy[i], poly_xy[(i + 1) % len(poly_xy)]
        s.append((b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0]))
    s = np.asarray(s)
    return int(((s >= 0).all(0) | (s <= 0).all(0)).sum())
