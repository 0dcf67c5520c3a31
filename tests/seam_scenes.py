"""Seams in a coordinate plane and rays that travel almost inside that plane — TEST INFRASTRUCTURE (numpy only).

The rule under test: boxes may only make a walk cheaper, "the triangle test alone decides".  The exact test accepts a
ray that passes an edge on the OUTSIDE by a few ulp of its distance from the apex; a leaf box that ends exactly on a seam in the plane
y = 0 and is padded only relative to its own coordinates is then never entered, and a tree walk returns the neighbour across the seam
where a walk without a tree returns the triangle the rule names.  tests/test_seams_cpu.py proves on the oracle that every fixture here
produces such rays (it fails on a leaf pad without an absolute term) and holds the oracle's tree to its tree-free mode;
tests/test_seams_gpu.py then holds every walk of the HIP library to the tree-free oracle.

  ridge(slope, wobble_z)   a 16x16-quad sheet of half-extent 4 folded along y = 0 (z += slope |y|); with wobble_z the seam's vertices get a
                           seeded z in +-0.1: the seam stays in y = 0, its edges leave the x axis
  grazing_rays(eye, n, seed)   rays from `eye` through points k ulp(D) u beside the seam (trace_rays, the non-apex test)
  pitched_cameras(eye, ks)     2048x2 cameras in the plane y = 0 pitched out of it by k 2^-23 (trace_primary and the renders, the apex test)
  stock(name)              small_vocalfold / small_colon with their spot moved into the plane of symmetry y = 0
  all_pairs                tie_scenes.tri_hit_all_pairs in chunks of rays
"""
from dataclasses import replace

import numpy as np

from fireflies_amd import scenes
from tests import tie_scenes as ts

F32 = np.float32
EXTENT = 4.0          # half-extent of the ridge: its largest coordinate, the builders' scene scale
EYE_NEAR = (0.3, 0.0, -2.3)
EYE_FAR = (0.3, 0.0, -9.1)
EYE_EDGE = (0.3, 0.0, -15.7)  # |eye| = 15.703 of the 4 x EXTENT = 16 the leaf pad is derived for: the edge of the range
KS = tuple(k / 4.0 for k in range(-24, 25) if k != 0)  # pitch in units of 2^-23: -6 .. 6 in steps of 1/4, without 0
RENDER_KS = (-1.0, 0.25)  # the pitches whose cameras the stock scenes are RENDERED from against a tree-free oracle render (minutes on all 48)
FILM_W, FILM_H = 2048, 2


# ----------------------------------------------------------------------------- the ridge
def ridge(slope, wobble_z=False, seed=7):
    """-> MeshData.  scenes.make_plane(0, 4, 16, 16) with z += slope |y|: two flanks that meet in a seam along y = 0, whose leaf boxes
    end exactly on y = 0.  wobble_z: every seam vertex gets a seeded z offset from +-0.1, so the seam's edges are no longer axis-parallel
    (the apex form decides an exactly axis-parallel edge exactly)."""
    v, t = scenes.make_plane(0.0, EXTENT, 16, 16)
    v = v.copy()
    v[:, 2] += F32(slope) * np.abs(v[:, 1])
    if wobble_z:
        seam = v[:, 1] == 0
        assert seam.sum() == 17
        v[seam, 2] += np.random.default_rng(seed).uniform(-0.1, 0.1, int(seam.sum())).astype(F32)
    return scenes.MeshData("mesh-Ridge", np.ascontiguousarray(v, F32)[None], t)


def side_of_prim(mesh_or_scene):
    """[F] sign of y of every triangle's centroid: which side of the plane y = 0 a primitive lies on (first frame)"""
    meshes = mesh_or_scene.meshes if hasattr(mesh_or_scene, "meshes") else [mesh_or_scene]
    return np.concatenate([np.sign(m.frames[0][m.tris][:, :, 1].astype(np.float64).mean(1)) for m in meshes]).astype(np.int32)


# ----------------------------------------------------------------------------- rays for trace_rays
def grazing_rays(eye, n=40000, seed=3):
    """-> (origins [n,3], dirs [n,3] float32, k [n]): from `eye` (in the plane y = 0) through (x, k ulp(D) u, 0) with x from +-3.9, integer k
    from [-6, 6], u from [0.2, 1.5], D = |eye| and ulp(D) the spacing of float32 at D: the rays cross the plane z = 0 a few ulp of their length
    beside the seam.  Normalised in float64, then rounded to float32."""
    rng = np.random.default_rng(seed)
    eye = np.asarray(eye, np.float64)
    D = float(np.linalg.norm(eye))
    x = rng.uniform(-3.9, 3.9, n)
    k = rng.integers(-6, 7, n)
    u = rng.uniform(0.2, 1.5, n)
    target = np.stack([x, k * float(np.spacing(F32(D))) * u, np.zeros(n)], -1)
    d = target - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.broadcast_to(eye.astype(F32), (n, 3))), np.ascontiguousarray(d, F32), k.astype(np.int32)


# name -> (mesh, eye)
RAY_FIXTURES = {
    "ridge+0.25": lambda: (ridge(0.25), EYE_NEAR),
    "ridge-0.25": lambda: (ridge(-0.25), EYE_NEAR),
    "flat": lambda: (ridge(0.0), EYE_NEAR),
    "wobbled_edge_of_range": lambda: (ridge(0.25, True), EYE_EDGE),
}


def all_pairs(mesh, origins, dirs, chunk=2000):
    """tie_scenes.tri_hit_all_pairs (every ray against every triangle, no tree) over chunks of rays -> (t, prim)"""
    out = [ts.tri_hit_all_pairs(mesh.frames[0], mesh.tris, origins[i:i + chunk], dirs[i:i + chunk])[:2] for i in range(0, origins.shape[0], chunk)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


# ----------------------------------------------------------------------------- cameras for trace_primary and the renders
def pitched_cameras(eye, ks=KS, target=None, fov=50.0):
    """-> [SensorData]: look_at(eye, target or eye + z) times the pitch R[1,2] = e, R[2,1] = -e with e = k 2^-23, film 2048x2, fov 50, clips
    0.05 / 100.  Un-jittered at 1 spp, row 1 of the film has d_l.y = 0: with the eye and the target in the plane y = 0 every ray of that row
    leaves the plane by e alone."""
    eye = np.asarray(eye, np.float64)
    base = scenes.look_at(eye, eye + (0.0, 0.0, 1.0) if target is None else target).astype(np.float64)
    cams = []
    for k in ks:
        R = np.eye(4)
        R[1, 2], R[2, 1] = k * 2.0 ** -23, -k * 2.0 ** -23
        cams.append(scenes.SensorData(f"cam{k:+.2f}", (base @ R).astype(F32), fov, 0.05, 100.0, FILM_W, FILM_H))
    return cams


# name -> (mesh, eye, fov).  The apex form needs seam edges that leave the axis, and distance: the wobbled ridge from EYE_FAR is the fixture
# that differs at a relative pad; the others hold the rule where it already held (and guard against a fix that breaks them).
CAM_FIXTURES = {
    "wobbled_far": lambda: (ridge(0.25, True), EYE_FAR, 50.0),  # (9.1 tan 25 = 4.24 > 4: this film is wider than the sheet)
    "wobbled_far_narrow": lambda: (ridge(0.25, True), EYE_FAR, 25.0),  # (the same eye, the whole film on the sheet)
    "wobbled_near": lambda: (ridge(0.25, True), EYE_NEAR, 50.0),
    "axis_parallel_far": lambda: (ridge(0.25), EYE_FAR, 50.0),
    "axis_parallel_near": lambda: (ridge(0.25), EYE_NEAR, 50.0),
    "wobbled_edge_of_range": lambda: (ridge(0.25, True), EYE_EDGE, 25.0),  # (fov 25: the film still lies on the sheet from that far)
}


def aimed_at_sheet(cam, margin=0.1):
    """[2048] whether the centre row's ray of each pixel column crosses the plane z = 0 at |x| < EXTENT - margin: the far eye's 50-degree film
    is wider than the sheet (9.1 tan 25 = 4.24 > 4), and those columns must miss; every other column must hit"""
    K_inv = np.linalg.inv(cam.K.astype(np.float64))
    sx = np.arange(FILM_W) / FILM_W
    p = K_inv @ np.stack([sx, np.full(FILM_W, 0.5), np.zeros(FILM_W), np.ones(FILM_W)])
    d = cam.to_world[:3, :3].astype(np.float64) @ (p[:3] / p[3])
    x = cam.to_world[0, 3] + d[0] / d[2] * (0.0 - cam.to_world[2, 3])
    return np.abs(x) < EXTENT - margin


# ----------------------------------------------------------------------------- the small stock scenes
def stock(name):
    """-> (scene, eye, target): tie_scenes.small_vocalfold / small_colon — both symmetric about y = 0, where the tubes' seams and the lips'
    edges lie, with eye and target in that plane — and the spot moved into the plane too, so that its shadow rays graze the seams as the
    primary rays of a pitched camera do"""
    sc = {"vocalfold": ts.small_vocalfold, "colon": ts.small_colon}[name]()
    eye = sc.camera.to_world[:3, 3].astype(np.float64)
    target = {"vocalfold": (0.0, 0.0, 5.0), "colon": (0.35, 0.0, 3.0)}[name]
    assert eye[1] == 0.0
    spot_eye = eye + (0.1, 0.0, 0.0)
    spot = replace(sc.spot, to_world=scenes.look_at(spot_eye, target))
    return replace(sc, spot=spot), eye, target


def with_camera(sc, cam):
    return replace(sc, camera=cam)
