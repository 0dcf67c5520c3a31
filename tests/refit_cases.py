"""The scenes and poses whose geometry update tests/test_refit_cpu.py and tests/test_refit_gpu.py hold to tests/ref_refit.py — TEST INFRASTRUCTURE (numpy;
the host builder through fireflies_amd._lib).  The smallest sizes at which the paths of ffx_scene_update / ffx_bvh_build_host still differ:

  one            1 triangle, 1 flat shape                   a single leaf, no wide node, a treelet without nodes
  leaf4          4 triangles of a 2 x 1 grid, smooth        a root with one full leaf and an empty child
  cluster65      the first 65 triangles of a 6 x 6 grid, smooth     the first scene with a wide node
  two_shapes     a 6 x 6 plane (shape 0, flat) and a 24 x 12 uv-sphere between the colatitudes 0.25 and pi - 0.25 (shape 1, smooth, two animation
                 frames), 648 triangles.  The pool holds the sphere's frames FIRST, so vert_off[1] (0, or 312 at frame 1) never equals vbase[1] (49)
  forty_shapes   40 flat patches of 8 triangles, each with a placement of its own: the device-table entry point (a host table above 32 shapes takes it)
  degenerate     two_shapes with extras on the smooth shape: a triangle with a repeated index (a, a, b), a collinear triangle on three vertices of
                 its own (so those vertices are touched by degenerate faces only)

Every shape but the sphere is a patch in its local xy-plane, so a pose can collapse it exactly.  POSES, applied in this order to ONE blob (a box has
to grow and to shrink back):
  identity . rot_aniso (rotation, scale 1.5 / 0.7 / 1.2) . mirror (negative determinant) . tiny (scale 1e-3: leaf_pad dominates the boxes' pad) .
  far (translation 200 / -200 / 150: the relative term dominates) . collapse (the LAST shape's local x scaled to 0 by an axis-aligned matrix: its posed
  x and z are constants, every edge is (0, dy, 0) and every float32 cross product exactly zero) . back (a regular pose again) . frame1 (the next
  animation frame of every shape that has one, through vert_off)

Matrices are rounded to ten significant bits of their largest entry (translations to the same grid).  The collinear triangle's vertices are small
dyadic numbers, so its posed corners are EXACT in float32 in every pose, e2 = 2 e1 holds exactly and so does cross(e1, e2) = 0 under the device's
fma(a, b, -(c d)) (the products have at most 22 bits); a triangle (a, a, b) has e1 = 0.  Degeneracy of the listed triangles is therefore a fact of
the float32 arithmetic, not a tolerance — and no other triangle is anywhere near it (test_refit_cpu.py: |cross| > 1e-3 |e1| |e2|).

VN_MEASURED: per case and pose the largest deviation of the ORACLE's float32 vertex normals (oracle/ffx_oracle.c vertex_normals, on this CPU) from the
float64 reference tests/ref_bruteforce.vertex_normals, any component of any row a smooth slot reads, rounded up to two digits.  The device gets
VN_MARGIN = 4 times that: it differs from the oracle only in the last bit of asinf, sqrtf and division, while a wrong weight, row or face set is off
by 1e-2 and more.  tests/test_refit_cpu.py re-measures the oracle against this table; nothing in it was taken from the device.  The deviation grows
with the translation (the float32 posed vertices carry 2^-24 of 200 against edges of 0.1 - 0.3) and is zero where every face is degenerate.
"""
import ctypes as C
import functools

import numpy as np

from fireflies_amd import _abi, _lib, scenes

POSE_NAMES = ("identity", "rot_aniso", "mirror", "tiny", "far", "collapse", "back", "frame1")
VN_MARGIN = 4.0
VN_MEASURED = {
    "leaf4": {"identity": 2.0e-8, "rot_aniso": 5.1e-8, "mirror": 5.0e-8, "tiny": 4.6e-8, "far": 7.1e-8, "collapse": 0.0, "back": 4.5e-8, "frame1": 4.0e-8},
    "cluster65": {"identity": 1.4e-7, "rot_aniso": 5.0e-7, "mirror": 2.6e-7, "tiny": 1.1e-7, "far": 1.3e-5, "collapse": 0.0, "back": 1.5e-7, "frame1": 3.6e-7},
    "two_shapes": {"identity": 6.1e-7, "rot_aniso": 8.3e-7, "mirror": 9.2e-7, "tiny": 4.0e-7, "far": 1.1e-4, "collapse": 4.6e-7, "back": 7.3e-7, "frame1": 5.4e-7},
    "degenerate": {"identity": 6.1e-7, "rot_aniso": 8.3e-7, "mirror": 9.2e-7, "tiny": 4.0e-7, "far": 1.1e-4, "collapse": 4.6e-7, "back": 7.3e-7, "frame1": 5.4e-7},
}


class Case:
    """pool [P,3] float32; tris [F,3] shape-local; tri_shape [F]; off / stride / nfr [S]: frame f of shape s starts at off[s] + f stride[s]; smooth [S];
    base [S,4,4]: each shape's placement; listed [F] bool: the triangles the case lists as degenerate in EVERY pose"""

    def __init__(self, name, pool, tris, tri_shape, off, stride, nfr, smooth, base, listed=()):
        self.name = name
        self.pool = np.ascontiguousarray(pool, np.float32)
        self.tris = np.ascontiguousarray(tris, np.int32)
        self.tri_shape = np.ascontiguousarray(tri_shape, np.int32)
        self.off, self.stride, self.nfr = (np.asarray(v, np.int32) for v in (off, stride, nfr))
        self.smooth = [bool(s) for s in smooth]
        self.base = np.asarray(base, np.float64)
        self.n_shapes, self.n_tris = len(self.smooth), self.tris.shape[0]
        self.listed = np.zeros(self.n_tris, bool)
        self.listed[list(listed)] = True
        self.collapsed = self.n_shapes - 1  # the shape the `collapse` pose flattens

    def vn_bound(self, pose):
        """what a vertex-normal component of this case in this pose may be off by (module docstring); None: the case has no smooth shape"""
        return VN_MARGIN * VN_MEASURED[self.name][pose.name] if self.name in VN_MEASURED else None


class Pose:
    """xforms [S,4,4] float32, vert_off [S] int32, listed [F] bool: the case's degenerate triangles in THIS pose"""

    def __init__(self, name, xforms, vert_off, listed):
        self.name, self.xforms, self.vert_off, self.listed = name, xforms, vert_off, listed


# ----------------------------------------------------------------------------- matrices
def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(4)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _tr(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def _sc(x, y, z):
    return np.diag([x, y, z, 1.0])


def dyadic(m):
    """the affine rows rounded to ten significant bits of the largest entry of the 3 x 3 (module docstring) -> float32"""
    m = np.array(m, np.float64)
    g = 2.0 ** (np.floor(np.log2(np.abs(m[:3, :3]).max())) - 9)
    m[:3] = np.round(m[:3] / g) * g
    return m.astype(np.float32)


_GLOBAL = {
    "identity": np.eye(4),
    "rot_aniso": _tr(0.3, -0.2, 0.5) @ _rot(2, 0.7) @ _rot(0, -0.4) @ _sc(1.5, 0.7, 1.2),
    "mirror": _tr(-0.4, 0.1, 0.2) @ _rot(1, 0.5) @ _sc(-1.0, 1.1, 0.9),
    "tiny": _tr(2e-4, 1e-4, -3e-4) @ _rot(0, 0.3) @ _sc(1e-3, 1e-3, 1e-3),
    "far": _tr(200.0, -200.0, 150.0) @ _rot(2, -0.3),
    "collapse": _rot(2, 0.2) @ _tr(0.1, 0.0, 0.0),
    "back": _tr(0.2, 0.3, -0.1) @ _rot(1, -0.6) @ _sc(0.9, 1.2, 1.0),
    "frame1": _tr(-0.1, 0.2, 0.1) @ _rot(0, 0.25),
}
_COLLAPSED = _tr(0.5, -0.25, 0.125) @ _sc(0.0, 1.25, 0.75)  # axis-aligned: posed x and z of a patch in its local xy-plane are constants


def poses(case):
    """the sequence of POSE_NAMES for a case"""
    out = []
    for name in POSE_NAMES:
        xf = np.stack([dyadic(_GLOBAL[name] @ case.base[s]) for s in range(case.n_shapes)])
        listed = case.listed.copy()
        if name == "collapse":
            xf[case.collapsed] = _COLLAPSED.astype(np.float32)
            listed |= case.tri_shape == case.collapsed
        frame = np.minimum(1 if name == "frame1" else 0, case.nfr - 1)
        out.append(Pose(name, xf, (case.off + frame * case.stride).astype(np.int32), listed))
    return out


# ----------------------------------------------------------------------------- scenes
def _patch(nu, nv, half=0.5, z=0.25):
    return scenes.make_plane(z, half, nu, nv)


def _single(name, verts, tris, smooth):
    return Case(name, verts, tris, np.zeros(len(tris), np.int32), [0], [len(verts)], [1], [smooth], [_tr(0.1, -0.05, 0.2) @ _rot(1, 0.35)])


def _sphere(frame):
    """24 x 12 quads between the colatitudes 0.25 and pi - 0.25 (no pole: no degenerate triangle); frame 1 bulges"""
    nu, nv = 24, 12
    th = np.linspace(0.25, np.pi - 0.25, nv + 1)
    ph = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    pp, tt = np.meshgrid(ph, th, indexing="xy")
    r = 1.0 + 0.15 * frame * np.sin(2 * tt) * np.cos(3 * pp)
    v = np.stack([r * np.sin(tt) * np.cos(pp), r * np.sin(tt) * np.sin(pp), r * np.cos(tt)], -1).reshape(-1, 3)
    return v.astype(np.float32), scenes.grid_tris(nu, nv, wrap_u=True)


def _two_shapes(name, extras):
    pv, pt = _patch(6, 6, half=1.5, z=-1.25)
    s0, st = _sphere(0)
    s1, _ = _sphere(1)
    listed = []
    if extras:
        V = s0.shape[0]
        line = np.array([[0.25, 0.5, 1.0], [0.75, 0.5, 1.0], [1.25, 0.5, 1.0]], np.float32)  # v2 - v0 = 2 (v1 - v0), along the local x axis
        s0, s1 = np.concatenate([s0, line]), np.concatenate([s1, line + np.float32([0.0, 0.0, 0.25])])
        st = np.concatenate([st, np.array([[5, 5, 30], [V, V + 1, V + 2]], np.int32)])
        listed = [len(pt) + len(st) - 2, len(pt) + len(st) - 1]
    V = s0.shape[0]
    pool = np.concatenate([s0, s1, pv])
    tris = np.concatenate([pt, st])
    shape = np.concatenate([np.zeros(len(pt), np.int32), np.ones(len(st), np.int32)])
    base = [_tr(0.0, 0.0, 0.0), _tr(0.2, 0.1, 0.3) @ _rot(0, 0.2)]
    c = Case(name, pool, tris, shape, [2 * V, 0], [len(pv), V], [1, 2], [False, True], base, listed)
    c.collapsed = 0  # the plane
    return c


def _forty_shapes():
    pv, pt = _patch(2, 2, half=0.25, z=0.0)
    S = 40
    pool = np.concatenate([pv * np.float32(1.0 + 0.02 * s) for s in range(S)])
    base = [_tr(0.6 * (s % 8), 0.6 * (s // 8), 0.1 * s) @ _rot(2, 0.1 * s) @ _rot(0, 0.05 * s) for s in range(S)]
    return Case("forty_shapes", pool, np.tile(pt, (S, 1)), np.repeat(np.arange(S, dtype=np.int32), len(pt)), np.arange(S) * len(pv), [len(pv)] * S, [1] * S,
                [False] * S, base)


def _cluster65():
    v, t = _patch(6, 6)
    return _single("cluster65", v, t[:65], True)


_MAKERS = {
    "one": lambda: _single("one", np.array([[0, 0, 0.25], [1, 0, 0.25], [0, 1, 0.25]], np.float32), np.array([[0, 1, 2]], np.int32), False),
    "leaf4": lambda: _single("leaf4", *_patch(2, 1), True),
    "cluster65": _cluster65,
    "two_shapes": lambda: _two_shapes("two_shapes", False),
    "forty_shapes": _forty_shapes,
    "degenerate": lambda: _two_shapes("degenerate", True),
}
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _MAKERS[name]()


def host_build(c):
    """(blob bytes up to off_bins, info): ffx_bvh_build_host on the pool and the frame-0 triangles, exactly as ops.DeviceGeometry(pool, tris, shape,
    off) calls it (the builder reads FFX_TREELET_TRIS and FFX_WIDE_BUILD)"""
    a = _lib.api()
    glob = np.ascontiguousarray(c.tris + c.off[c.tri_shape][:, None], np.int32)
    n = a.lib.ffx_bvh_blob_bytes(c.n_tris)
    blob = np.zeros(n, np.uint8)
    info = _abi.BvhInfo()
    a.call("ffx_bvh_build_host", c.pool.ctypes.data, c.pool.shape[0], glob.ctypes.data, c.n_tris, blob.ctypes.data, n, C.byref(info))
    return blob[: int(info.off_bins)].copy(), info
