"""Scenes in which rays meet several triangles at EXACTLY the same distance — TEST INFRASTRUCTURE (numpy only).

The rule under test: closest hit, and at equal t the smaller primitive id wins, whatever the tree and the
traversal order.  tests/test_ties_cpu.py proves on the oracle that every fixture here really produces the ties it is meant
to; tests/test_ties_gpu.py then holds every walk of the HIP library to the rule on them.

  sheets()        two coplanar planes at z = 2 (4x4 and 16x16 quads, two shapes): every ray ties between the shapes
  sheets_far_from_their_plane()   the same in the plane z = 0 seen from z = -2.3: flat boxes, 2^-16 of the scene scale behind the hit
  sheets_far_unpadded()           ... re-fitted with leaf_pad = 0: the boxes end exactly ON the hit (guards the cull's widening)
  duplicated(sc)  every mesh of `sc` appended once more as an extra shape: every hit ties with its copy
  reversed_tris / map_back   relabel a scene (triangle order reversed inside every mesh): a ray whose geometric pick
                  changes under the relabelling is one the id order decided — a natural tie of the stock scenes' seams
  budget()        one quad's two triangles 64 times over: 128 coincident triangles, more exact tests than one wide walk may spend
  lattice()       a dyadic sheet and integer rays through its grid vertices (6 triangles tie) and edge midpoints (2 tie)
  tri_hit_all_pairs   float32 numpy restatement of the non-apex triangle test, every ray against every triangle, min t then min id
"""
from dataclasses import replace

import numpy as np

from fireflies_amd import scenes

F32 = np.float32


# ----------------------------------------------------------------------------- stacked sheets
def sheets(fine_first=False, width=40, height=24, z=2.0, eye_z=0.0):
    """two coplanar planes at `z`, half-extent 2: 4x4 quads (spacing 1) and 16x16 quads (spacing 1/4), two shapes; camera at
    (0.1, -0.07, eye_z) looking along +z.  The sheets' coordinates are dyadic and the doubled areas are powers of two (2 and
    1/8), so the apex form's t = T/det = (z - eye_z) s^2 / (d_z s^2) rounds identically for both sheets: every ray ties.  The
    tied triangles have very different boxes: they sit in different leaves, clusters and tile-bin entries."""
    cv, ct = scenes.make_plane(z, 2.0, 4, 4)
    fv, ft = scenes.make_plane(z, 2.0, 16, 16)
    coarse = scenes.MeshData("mesh-Coarse", cv[None], ct, (0.7, 0.5, 0.3))
    fine = scenes.MeshData("mesh-Fine", fv[None], ft, (0.3, 0.5, 0.7))
    eye = (0.1, -0.07, eye_z)
    cam = scenes.SensorData("cam", scenes.look_at(eye, (eye[0], eye[1], eye_z + 1.0)), 50.0, 0.05, 100.0, width, height)
    # (a spot next to the eye, for the render kernels: the sheets carry different albedos, so the image shows which one answered)
    spot = scenes.SpotData("spot", scenes.look_at((0.3, 0.2, eye_z), (0.0, 0.0, z)), (20.0, 20.0, 20.0), 40.0, 30.0)
    return scenes.SceneData([fine, coarse] if fine_first else [coarse, fine], cam, None, spot)


def first_sheet_only(sc):
    """the scene without its second sheet: what every ray and every render of the stacked sheets must see"""
    return replace(sc, meshes=sc.meshes[:1])


def sheets_far_from_their_plane(fine_first=False):
    """the stacked sheets in the plane z = 0 seen from z = -2.3, with the builders' pad of today (4e-7 of a box's own
    coordinates plus 2^-16 of the scene scale): every box of the scene is flat in z and ends 2^-16 x 2 BEHIND the hit.  This variant holds
    the tie-break on boxes as every scene gets them; it no longer fails when a walk culls boxes against the bare hit distance —
    sheets_far_unpadded does."""
    return sheets(fine_first, z=0.0, eye_z=-2.3)


def sheets_far_unpadded(fine_first=False):
    """the same scene, marked (notes["leaf_pad"] = 0) for the tests to re-fit with ffx_bvh_info.leaf_pad set to 0 after the build — the
    info of an older blob (include/ffx.h), and what a pose far larger than the build vertices comes to.  Then every box of the scene ends
    exactly ON the hit: the relative pad is nothing at z = 0, and the eye's depth is no dyadic number, so
    the entry distance a box test computes, (0 - eye_z) * (1 / d_z), is rounded twice where the hit distance (0 - eye_z) / d_z is
    rounded once: on one ray in five it comes out one ulp BEHIND the hit.  A walk that culls boxes against the bare hit distance
    then never looks at the other sheet.  This is the variant that guards the cull's widening (FFX_TIE_WIDEN, the octant and wide
    walks' `sw`, the oracle's 1.0000004): with the widening removed it fails, the padded variant does not."""
    sc = sheets_far_from_their_plane(fine_first)
    return replace(sc, notes=dict(sc.notes, leaf_pad=0.0))


def refit_with_marked_pad(sc, geometries, xforms):
    """if `sc` is marked (notes["leaf_pad"]): set that value in the info of every geometry — the oracle's and the device's alike — and
    re-fit, so that all boxes are rebuilt with it"""
    pad = sc.notes.get("leaf_pad")
    if pad is not None:
        for g in geometries:
            g.info.leaf_pad = float(pad)
            g.update(xforms)


# ----------------------------------------------------------------------------- exact duplicates
def duplicated(sc):
    """`sc` with every mesh appended once more as an extra shape with the same vertices, triangles and material: shape S + i is
    shape i again, primitive F + k is primitive k again.  The rule says the copy is never seen."""
    return replace(sc, meshes=list(sc.meshes) + [replace(m, name=m.name + "-Copy") for m in sc.meshes])


def dup_cases():
    """name -> the small stock scenes of the duplicate tests (all diffuse)"""
    return {"colon": lambda: small_colon(52, 45), "vocalfold": lambda: small_vocalfold(45, 37), "hello": lambda: scenes.hello_world(48, 40)}


def small_colon(width=64, height=64):
    return scenes.colon(width=width, height=height, tex=64, n_around=32, n_along=96, principled=False)


def small_vocalfold(width=64, height=64):
    return scenes.vocalfold(width=width, height=height, tex=64, frames=2, n_fold=16, tube=(24, 24), principled=False)


def seam_cases():
    """name -> the same scenes on an even film: un-jittered, the rays of the centre row and column lie in the meshes' planes of symmetry,
    where the tubes' seams and the lips' edges are — natural exact ties.  On the 64x64 film the centre row starts an 8x8-pixel packet; on
    the 60x52 film it lies inside one, whose rays then disagree on a direction sign (the generic packet walk)."""
    return {"colon": small_colon, "vocalfold": small_vocalfold, "colon_60x52": lambda: small_colon(60, 52), "vocalfold_60x52": lambda: small_vocalfold(60, 52)}


# ----------------------------------------------------------------------------- relabelling
def reversed_tris(sc):
    """the same geometry with the triangle order reversed inside every mesh"""
    return replace(sc, meshes=[replace(m, tris=np.ascontiguousarray(m.tris[::-1])) for m in sc.meshes])


def map_back(prim, sc):
    """primitive ids of reversed_tris(sc) -> the ids the same triangles have in `sc` (misses stay -1)"""
    prim = np.asarray(prim, np.int64)
    counts = np.array([m.tris.shape[0] for m in sc.meshes], np.int64)
    base = np.concatenate([[0], np.cumsum(counts)])
    mesh = np.clip(np.searchsorted(base, prim, side="right") - 1, 0, len(counts) - 1)
    back = base[mesh] + (counts[mesh] - 1 - (prim - base[mesh]))
    return np.where(prim >= 0, back, -1).astype(np.int32)


# ----------------------------------------------------------------------------- work budget
BUDGET_COPIES = 64


def budget(width=24, height=16):
    """one mesh whose triangle list repeats the two triangles of one quad (z = 2, half-extent 0.5) BUDGET_COPIES times: 128
    coincident triangles — more exact tests than a 64-wide walk may spend, so the packet is handed to the binary walk.
    Every hit must be primitive 0 or 1.  The film is wider than the quad: some rays miss."""
    v, t = scenes.make_plane(2.0, 0.5, 1, 1)
    tris = np.ascontiguousarray(np.tile(t, (BUDGET_COPIES, 1)), np.int32)
    cam = scenes.SensorData("cam", scenes.look_at((0.03, 0.02, 0.0), (0.03, 0.02, 1.0)), 50.0, 0.05, 100.0, width, height)
    return scenes.SceneData([scenes.MeshData("mesh-Stack", v[None], tris)], cam)


# ----------------------------------------------------------------------------- lattice rays
LATTICE_N = 8  # quads per side; spacing 1, z = 4


def lattice():
    """-> (mesh, origins [n,3], dirs [n,3], ties [n]): a sheet of 8x8 unit quads at z = 4 around the integer origin (0, 0, 0) and
    un-normalised integer directions through every grid vertex (t = 1; 6 triangles tie at an interior vertex) and through the
    midpoint of every edge, the quads' diagonals included (t = 1/2; 2 triangles tie on an interior edge).  Every intermediate
    of the triangle test is a small integer and t is 1 or 1/2: exactly representable, whatever the operation order."""
    n, h = LATTICE_N, LATTICE_N // 2
    v, t = scenes.make_plane(4.0, float(h), n, n)
    mesh = scenes.MeshData("mesh-Lattice", v[None], t)
    d, ties = [], []
    for j in range(-h, h + 1):
        for i in range(-h, h + 1):
            d.append((i, j, 4))  # a vertex
            on_x, on_y = abs(i) == h, abs(j) == h
            # corner: 1 or 2 (the diagonal runs from the low to the high corner of a quad); border: 3; interior: 6
            ties.append(6 if not (on_x or on_y) else (3 if on_x != on_y else (2 if i * j > 0 else 1)))
            if i < h:
                d.append((2 * i + 1, 2 * j, 8))  # midpoint of an edge along x
                ties.append(1 if on_y else 2)
            if j < h:
                d.append((2 * i, 2 * j + 1, 8))  # ... along y
                ties.append(1 if on_x else 2)
            if i < h and j < h:
                d.append((2 * i + 1, 2 * j + 1, 8))  # ... of the quad's diagonal
                ties.append(2)
    dirs = np.asarray(d, F32)
    return mesh, np.zeros_like(dirs), dirs, np.asarray(ties, np.int32)


def _cross(a, b):
    """cross(a,b).x = fma(a.y, b.z, -(a.z * b.y)) etc. (include/ffx.h); the fma's single rounding is reproduced in float64, where the
    product of two float32 is exact and the sum of two such products rounds once to double before the final rounding to float —
    exact whenever the result is representable, as it is for the lattice's small integers"""
    def one(ay, bz, az, by):
        return (ay.astype(np.float64) * bz - (az * by).astype(np.float64)).astype(F32)
    return np.stack([one(a[..., 1], b[..., 2], a[..., 2], b[..., 1]), one(a[..., 2], b[..., 0], a[..., 0], b[..., 2]),
                     one(a[..., 0], b[..., 1], a[..., 1], b[..., 0])], -1)


def _dot(a, b):
    """dot = fma(x, x', fma(y, y', z * z'))"""
    zz = (a[..., 2] * b[..., 2]).astype(F32)
    inner = (a[..., 1].astype(np.float64) * b[..., 1] + zz).astype(F32)
    return (a[..., 0].astype(np.float64) * b[..., 0] + inner).astype(F32)


def tri_hit_all_pairs(verts, tris, origins, dirs, tmin=0.0, tmax=3.0e38):
    """every ray against every triangle in float32, in the operation order of the library's non-apex test (include/ffx.h, K7):
    pv = cross(d, e2); det = dot(e1, pv); tv = o - v0; qv = cross(tv, e1); U = dot(tv, pv); V = dot(d, qv); T = dot(e2, qv);
    det < 0: negate all four; hit iff det > 0, U >= 0, V >= 0, U + V <= det, t = T / det, tmin < t <= tmax.
    Reduced by min t, then min id.  -> (t [n] float32, 0 on a miss; prim [n] int32, -1 on a miss; the number of triangles at that t [n])"""
    p = np.asarray(verts, F32)[np.asarray(tris)]
    v0, e1, e2 = p[None, :, 0], (p[:, 1] - p[:, 0])[None], (p[:, 2] - p[:, 0])[None]
    o, d = np.asarray(origins, F32)[:, None, :], np.asarray(dirs, F32)[:, None, :]
    pv = _cross(np.broadcast_to(d, (d.shape[0], p.shape[0], 3)), np.broadcast_to(e2, (d.shape[0], p.shape[0], 3)))
    det = _dot(np.broadcast_to(e1, pv.shape), pv)
    tv = (o - v0).astype(F32)
    qv = _cross(tv, np.broadcast_to(e1, tv.shape))
    U, V, T = _dot(tv, pv), _dot(np.broadcast_to(d, qv.shape), qv), _dot(np.broadcast_to(e2, qv.shape), qv)
    neg = det < 0
    det, U, V, T = np.where(neg, -det, det), np.where(neg, -U, U), np.where(neg, -V, V), np.where(neg, -T, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (T / det).astype(F32)
    ok = (det > 0) & (U >= 0) & (V >= 0) & ((U + V).astype(F32) <= det) & (t > F32(tmin)) & (t <= F32(tmax))
    tt = np.where(ok, t, np.inf).astype(F32)
    best = tt.min(1)
    prim = np.argmax(tt == best[:, None], axis=1)  # the first = smallest id among equal distances
    hit = np.isfinite(best)
    return np.where(hit, best, 0).astype(F32), np.where(hit, prim, -1).astype(np.int32), (ok & (tt == best[:, None])).sum(1)
