"""The tile bins and the emitters' envelopes restated in float64 — TEST INFRASTRUCTURE (numpy only, no torch, no tree).

The pre-pass of a packet render (fireflies_amd/csrc/ffx_bins.hip) lists, per tile of three perspective grids, the triangles a ray through that tile can
hit, and gives every cell of an emitter's grid one plane that lies in front of everything listed there.  This module states what those structures must
hold, from the comments of ffx_common.h and DESIGN.md 4.3 / 5.1 — geometry in float64, not the kernels' control flow:

  grids_of(sd, ...)       the three grids of a scene description: tile coordinates of a world point p seen from o are (M (p - o)).xy / (M (p - o)).z
  must_list(grid, tris)   the (slot, tile) pairs whose triangle really meets the tile's pyramid (Sutherland-Hodgman in 3-D, the closed unpadded tile)
  may_list(grid, tris)    the pairs the kernel is allowed to list: the same test with the tile grown by 2 PAD — the kernel lists with 1 PAD
  klass(grid, tris)       behind / at most sixteen tiles / more / projection not trusted — to report, and to require that every class is exercised
  check_lists / check_entries / check_reader / check_envelope     a grid's lists, 64-byte entries and envelope cells against the above; every one returns
                          figures and a list of complaints, empty when the structure is right (tests/test_bins_cpu.py feeds them right and wrong ones)
  build_lists / build_envelope    a right structure from float64, as ffx_common.h describes it: what the checks must accept, and what the CPU tests spoil

Only two margins are used.  PAD (1 / 256 tile, FFX_BIN_PAD) is the kernel's own: it pads by one, so it holds `must` (no pad) and stays inside `may`
(two).  TOL bounds the float32 rounding of a projected vertex, from the number format: a coordinate formed as M (v - o) in float32 is off by at most
1e-6 |M row| (|v| + |o|) (three subtractions and three multiply-adds at 6e-8 each, with room).  It only ever WIDENS `may` (which triangles are
certainly trusted, certainly in front); `must` and the envelope inequality are pure float64 geometry.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fireflies_amd", "csrc")


def _define(fname, name):
    with open(os.path.join(CSRC, fname)) as f:
        m = re.search(r"^#define\s+" + name + r"\s+(.+?)\s*(//.*)?$", f.read(), re.M)
    assert m, name
    return m.group(1)


def _number(text):
    return float(np.float32(float(text.rstrip("f")))) if text.endswith("f") else float(text)


PAD = _number(_define("ffx_common.h", "FFX_BIN_PAD"))  # 1 / 256 tile
FAR = _number(_define("ffx_common.h", "FFX_BIN_FAR"))  # 512 tiles
ENV_SUB = int(_define("ffx_common.h", "FFX_ENV_SUB"))  # 7 x 7 cells per tile
MAX_TILES = int(_define("ffx_common.h", "FFX_BIN_MAX_TILES"))
RAY_EPS = _number(_define("ffx_trace.hip", "RAY_EPS"))
_m = re.fullmatch(r"\((\S+)\s*\*\s*RAY_EPS\)", _define("ffx_trace.hip", "SHADOW_EPS"))
assert _m, "SHADOW_EPS is no longer a multiple of RAY_EPS"
SHADOW_EPS = float(np.float32(_number(_m.group(1))) * np.float32(RAY_EPS))  # "10 eps": the ignored tail of a shadow ray
CELL_PE = 1.0 / 4096.0  # k_bin_env: a cell's vertex collects the entries within one cell + this of it
SLIVER = 1e-5  # bin_make_entry: |area2| <= this * (|a.x| + |a.y|) (|c.x| + |c.y|) keeps its box only
BEHIND, FEW, MANY, UNTRUSTED = 0, 1, 2, 3
CLASS_NAMES = ("behind", "<=16 tiles", ">16 tiles", "not trusted")
ENTRY = np.dtype([("bb", "<f4", 4), ("e", "<f4", 9), ("slot", "<i4"), ("pad", "<u4", 2)])
assert ENTRY.itemsize == 64


# ----------------------------------------------------------------------------- grids
class Grid:
    """tile coordinates of a world point p: (X, Y) / Z with (X, Y, Z) = M (p - o), Z > 0; nx x ny tiles"""

    def __init__(self, name, M, o, nx, ny):
        self.name, self.nx, self.ny = name, int(nx), int(ny)
        self.M = np.asarray(M, np.float32).astype(np.float64).reshape(3, 3)  # (the kernels hold float32)
        self.o = np.asarray(o, np.float64).reshape(3)
        self.Minv = np.linalg.inv(self.M)

    def homog(self, p):
        """world points [..., 3] -> (X, Y, Z) [..., 3]"""
        return (np.asarray(p, np.float64) - self.o) @ self.M.T

    def tol(self, p):
        """[..., 3]: what float32 can be off by in each of X, Y, Z of a point (module docstring)"""
        p = np.asarray(p, np.float64)
        return 1e-6 * np.linalg.norm(self.M, axis=1) * (np.linalg.norm(p, axis=-1) + np.linalg.norm(self.o))[..., None]

    def graz(self):
        """EnvBuild.graz: the largest |Minv (x, y, 1)| over the grid's corners, divided by 40"""
        c = np.array([[x, y, 1.0] for x in (0.0, self.nx) for y in (0.0, self.ny)])
        return float(np.linalg.norm(c @ self.Minv.T, axis=1).max()) / 40.0


def _m4(a):
    return np.array(list(a), np.float64).reshape(4, 4)


def sensor_grid(name, to_world, camera_to_sample, width, height, tile):
    """tiles of `tile` film pixels (texels); the tile doubles until neither side has more than 128"""
    tw, c2s = _m4(to_world), _m4(camera_to_sample)
    while -(-width // tile) > 128 or -(-height // tile) > 128:
        tile *= 2
    rows = np.stack([c2s[0, :3] * width / tile, c2s[1, :3] * height / tile, c2s[3, :3]])
    return Grid(name, rows @ np.linalg.inv(tw)[:3, :3], tw[:3, 3], -(-width // tile), -(-height // tile)), tile


def spot_grid_n(cutoff_deg, plain=False):
    """tiles per side: about a degree per tile — ceil(2 cutoff), ceil(1.2 cutoff) under the short-render hint —, 8 .. 128"""
    n = int(np.float32(np.float32(1.2 if plain else 2.0) * np.float32(cutoff_deg)) + np.float32(0.999))
    return min(128, max(8, n))


def spot_grid(to_world, cutoff_deg, n):
    """a square grid about the cone's axis, half angle cutoff + 1 degree"""
    tw = _m4(to_world)
    w = np.linalg.inv(tw)[:3, :3]
    tanc = np.tan(np.deg2rad(float(cutoff_deg) + 1.0))
    return Grid("spot", np.stack([0.5 * n * (w[0] / tanc + w[2]), 0.5 * n * (w[1] / tanc + w[2]), w[2]]), tw[:3, 3], n, n)


def grids_of(sd, tile=8, tile_proj=None, spot_n=None):
    """[camera, projector, spot] of a scene description (fireflies_amd._abi.SceneDesc); None for a grid that is off.  tile / tile_proj / spot_n: what
    FFX_BIN_TILE, FFX_BIN_TILE_PROJ and FFX_BIN_SPOT_N say (default: 8 pixels, twice the camera's tile, by the cone)"""
    out = [sensor_grid("camera", sd.cam.to_world, sd.cam.camera_to_sample, sd.cam.width, sd.cam.height, tile)[0], None, None]
    if sd.proj.enabled:
        out[1] = sensor_grid("projector", sd.proj.to_world, sd.proj.camera_to_sample, sd.proj.tex_w, sd.proj.tex_h, tile_proj or 2 * tile)[0]
    if sd.spot.enabled and 0.0 < sd.spot.cutoff_deg <= 75.0:
        out[2] = spot_grid(sd.spot.to_world, sd.spot.cutoff_deg, spot_n or spot_grid_n(sd.spot.cutoff_deg, bool(int(sd.shadows) & 2)))
    return out


# ----------------------------------------------------------------------------- polygons, many at once
def _clip(poly, cnt, nrm):
    """one Sutherland-Hodgman step for N convex polygons: the part with nrm . p >= 0.  poly [N,K,3] (vertices beyond cnt unused), cnt [N], nrm [N,3]"""
    N, K, _ = poly.shape
    if N == 0:
        return poly, cnt
    d = np.einsum("nkc,nc->nk", poly, nrm)
    idx = np.arange(K)[None, :]
    valid = idx < cnt[:, None]
    nxt = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    pn = np.take_along_axis(poly, nxt[:, :, None], 1)
    dn = np.take_along_axis(d, nxt, 1)
    ina, inb = d >= 0, dn >= 0
    keep, cross = valid & ina, valid & (ina != inb)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(cross, d / (d - dn), 0.0)
    cand = np.stack([poly, poly + t[:, :, None] * (pn - poly)], 2).reshape(N, 2 * K, 3)
    flag = np.stack([keep, cross], 2).reshape(N, 2 * K)
    out_cnt = flag.sum(1)
    out = np.zeros((N, max(int(out_cnt.max()), 1), 3))
    r, c = np.nonzero(flag)
    out[r, (np.cumsum(flag, 1) - 1)[r, c]] = cand[r, c]
    return out, out_cnt


def _area(poly, cnt):
    """[N]: area of the polygons (fan about vertex 0)"""
    if poly.shape[1] < 3:
        return np.zeros(poly.shape[0])
    a = poly[:, 1:-1] - poly[:, :1]
    b = poly[:, 2:] - poly[:, :1]
    use = (np.arange(2, poly.shape[1])[None, :] < cnt[:, None])[:, :, None]
    return 0.5 * np.linalg.norm((np.cross(a, b) * use).sum(1), axis=1)


def clip_to_boxes(P, x0, y0, x1, y1, chunk=200000):
    """triangles P [N,3,3] in (X, Y, Z), each cut to its own pyramid x0 <= X / Z <= x1, y0 <= Y / Z <= y1, Z >= 0 (closed) -> (polygons [N,K,3], counts)"""
    polys, cnts = [], []
    for s in range(0, len(P), chunk):
        e = slice(s, s + chunk)
        n = len(P[e])
        poly, cnt = P[e], np.full(n, 3)
        z, o = np.zeros(n), np.ones(n)
        for nrm in (np.stack([z, z, o], 1), np.stack([o, z, -x0[e]], 1), np.stack([-o, z, x1[e]], 1), np.stack([z, o, -y0[e]], 1), np.stack([z, -o, y1[e]], 1)):
            poly, cnt = _clip(poly, cnt, nrm)
        polys.append(poly)
        cnts.append(cnt)
    if not polys:
        return np.zeros((0, 3, 3)), np.zeros(0, int)
    K = max(p.shape[1] for p in polys)
    return np.concatenate([np.pad(p, ((0, 0), (0, K - p.shape[1]), (0, 0))) for p in polys]), np.concatenate(cnts)


AREA_REL = 1e-12  # "positive area": above this share of the triangle's own (the clip points' float64 rounding is 1e-16 of the coordinates)


def _tri_area(P):
    return 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)


def _overlap(poly, cnt, P):
    """[N] bool: the clipped polygons that are an overlap — three vertices or more and positive area; a triangle without area of its own (two vertices in
    one place, three on a line: below AREA_REL of its longest edge squared) overlaps nothing"""
    e = np.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 1], P[:, 0] - P[:, 2]], 1)
    ta = _tri_area(P)
    return (cnt >= 3) & (ta > AREA_REL * (e * e).sum(2).max(1)) & (_area(poly, cnt) > AREA_REL * ta)


# ----------------------------------------------------------------------------- which tiles
def _wedges(P, n, axis, pad, slack=None):
    """[F, n] bool: column (axis 0) / row (axis 1) c of the grid is NOT missed by the triangle in the sense of the plane rule — a column is the wedge
    between two planes through the apex, and the triangle misses it iff all three vertices lie beyond the same one of the two (any vertex position,
    also behind the apex).  pad: how far the wedge is grown on both sides (tile units); slack [F,3]: added to every plane value"""
    c = np.arange(n, dtype=np.float64)[None, None, :]
    X, Z = P[:, :, axis, None], P[:, :, 2, None]
    s = 0.0 if slack is None else slack[:, :, None]
    return ~((X - (c - pad) * Z + s < 0).all(1)) & ~(((c + 1.0 + pad) * Z - X + s < 0).all(1))


def _pairs(grid, P, pad, front, slack=None):
    """(slot [N], tx [N], ty [N]) of the product of wedge columns and wedge rows of every triangle with front[slot]"""
    cols, rows = _wedges(P, grid.nx, 0, pad, slack), _wedges(P, grid.ny, 1, pad, slack) & front[:, None]
    step = max(1, (1 << 25) // (grid.nx * grid.ny))  # (triangles per trip: the product is formed as a [step, ny, nx] mask)
    out = [np.nonzero(rows[s: s + step, :, None] & cols[s: s + step, None, :]) for s in range(0, len(P), step)]
    f = np.concatenate([o[0] + s for o, s in zip(out, range(0, len(P), step))]) if out else np.zeros(0, np.int64)
    return f, np.concatenate([o[2] for o in out]) if out else f, np.concatenate([o[1] for o in out]) if out else f


def _as_set(grid, f, tx, ty):
    return set((f.astype(np.int64) * (grid.nx * grid.ny) + ty * grid.nx + tx).tolist())


def pair_key(grid, slot, tile):
    return int(slot) * (grid.nx * grid.ny) + int(tile)


def must_list(grid, tris):
    """the set of slot * (nx ny) + tile for which triangle `slot` (tris [F,3,3], world) meets the pyramid of the closed, unpadded tile in a polygon of at
    least three vertices and positive area"""
    P = grid.homog(tris)
    f, tx, ty = _pairs(grid, P, 0.0, (P[:, :, 2] > 0).any(1))
    poly, cnt = clip_to_boxes(P[f], tx.astype(float), ty.astype(float), tx + 1.0, ty + 1.0)
    ok = _overlap(poly, cnt, P[f])
    return _as_set(grid, f[ok], tx[ok], ty[ok])


def projection(grid, tris):
    """-> (xy [F,3,2] tile coordinates (NaN where Z <= 0), area2 [F] signed doubled area of the projection, sliver [F]: bin_make_entry's test in float64)"""
    P = grid.homog(tris)
    with np.errstate(divide="ignore", invalid="ignore"):
        xy = np.where(P[:, :, 2:3] > 0, P[:, :, :2] / P[:, :, 2:3], np.nan)
    a, c = xy[:, 1] - xy[:, 0], xy[:, 0] - xy[:, 2]
    area2 = a[:, 0] * (xy[:, 2, 1] - xy[:, 0, 1]) - a[:, 1] * (xy[:, 2, 0] - xy[:, 0, 0])
    scale = np.abs(a).sum(1) * np.abs(c).sum(1)
    return xy, area2, scale


def trust(grid, tris):
    """-> (trusted, surely, surely_not) [F] bool: every vertex in front with |X|, |Y| <= FAR Z — in float64; whatever float32 makes of it; not even in float32"""
    P, t = grid.homog(tris), grid.tol(tris)
    X, Y, Z = np.abs(P[..., 0]), np.abs(P[..., 1]), P[..., 2]
    trusted = ((Z > 0) & (X <= FAR * Z) & (Y <= FAR * Z)).all(1)
    zl = Z - t[..., 2]
    surely = ((zl > 0) & (X + t[..., 0] <= FAR * zl * (1 - 1e-6)) & (Y + t[..., 1] <= FAR * zl * (1 - 1e-6))).all(1)
    zh = Z + t[..., 2]
    surely_not = ((zh <= 0) | (X - t[..., 0] > FAR * zh * (1 + 1e-6)) | (Y - t[..., 1] > FAR * zh * (1 + 1e-6))).any(1)
    return trusted, surely, surely_not


def projection_error(grid, tris):
    """[F]: how far float32 can put a projected vertex from its float64 place (tile units; inf where a vertex is not surely in front)"""
    P, t = grid.homog(tris), grid.tol(tris)
    zl = P[..., 2] - t[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = (np.maximum(t[..., 0], t[..., 1]) + np.abs(P[..., :2]).max(-1) / np.maximum(P[..., 2], 1e-300) * t[..., 2]) / zl + 2e-7 * FAR
    return np.where(zl > 0, e, np.inf).max(1)


def may_list(grid, tris):
    """the pairs the kernel may list.  A triangle that is certainly trusted (every vertex in front and within FAR tiles whatever float32 rounds), whose
    projection is certainly not a sliver (twice bin_make_entry's threshold) and lands within PAD / 2 of its float64 place: the polygon test of must_list
    with the tile grown by 2 PAD, any contact.  Every other triangle with a vertex in front: the product of the columns and the rows it does not miss by
    the plane rule (_wedges), the planes moved out by 2 PAD — for a triangle in front that IS the product of the bounding columns and rows of its
    projection; for one that crosses the apex plane it also holds the columns only its part behind the apex plane points at, which is what the kernel's
    class-3 rule ('all three vertices beyond the same plane, any vertex position, also behind the apex') lists and the issue's clipped projection does not"""
    P, t = grid.homog(tris), grid.tol(tris)
    front = (P[:, :, 2] + t[:, :, 2] > 0).any(1)
    _, surely, _ = trust(grid, tris)
    _, area2, scale = projection(grid, tris)
    with np.errstate(invalid="ignore"):
        exact = surely & (np.abs(area2) > 2 * SLIVER * scale) & (projection_error(grid, tris) <= 0.5 * PAD)
    f, tx, ty = _pairs(grid, P, 2 * PAD, front, slack=np.maximum(t[:, :, 0], t[:, :, 1]) + (max(grid.nx, grid.ny) + 1) * t[:, :, 2])
    keep = ~exact[f]
    poly, cnt = clip_to_boxes(P[f[~keep]], tx[~keep] - 2 * PAD, ty[~keep] - 2 * PAD, tx[~keep] + 1 + 2 * PAD, ty[~keep] + 1 + 2 * PAD)
    keep[~keep] = cnt >= 1
    return _as_set(grid, f[keep], tx[keep], ty[keep])


def klass(grid, tris):
    """[F] of BEHIND (no ray of the grid reaches it: behind the apex plane, or wholly beyond one of the grid's four side planes), FEW, MANY (its padded
    box spans at most / more than sixteen tiles), UNTRUSTED (a vertex behind or beside the apex, or beyond FAR tiles) — float64"""
    P = grid.homog(tris)
    trusted, _, _ = trust(grid, tris)
    xy, _, _ = projection(grid, tris)
    out = np.zeros(len(P), int)
    with np.errstate(invalid="ignore"):
        lo, hi = xy.min(1) - PAD, xy.max(1) + PAD
        on = trusted & (hi[:, 0] >= 0) & (hi[:, 1] >= 0) & (lo[:, 0] < grid.nx) & (lo[:, 1] < grid.ny)
        span = (np.minimum(grid.nx - 1, np.floor(hi[:, 0])) - np.maximum(0, np.floor(lo[:, 0])) + 1) * (np.minimum(grid.ny - 1, np.floor(hi[:, 1])) - np.maximum(0, np.floor(lo[:, 1])) + 1)
    out[on] = np.where(span[on] <= 16, FEW, MANY)
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    beyond = (X + PAD * Z < 0).all(1) | ((grid.nx + PAD) * Z - X < 0).all(1) | (Y + PAD * Z < 0).all(1) | ((grid.ny + PAD) * Z - Y < 0).all(1)
    out[~trusted & (Z > 0).any(1) & ~beyond] = UNTRUSTED
    return out


# ----------------------------------------------------------------------------- a grid's lists against the reference
def entry_tiles(starts, n, nt):
    """[n]: the tile whose list entry i stands in (the last tile that starts at or before i)"""
    return np.clip(np.searchsorted(starts[1: nt + 1].astype(np.int64), np.arange(n), side="right"), 0, nt - 1)


def check_lists(grid, tris, hdr, starts, cursors, entries, cap):
    """the integers, exactly, and must <= listed <= may -> (figures, complaints, per-tile sets)"""
    F, nt = len(tris), grid.nx * grid.ny
    bad = []
    if int(hdr[0]) != 1 or int(hdr[2]) != cap:
        bad.append(f"header ok {hdr[0]} cap {hdr[2]} (want 1, {cap})")
    if starts[0] != 0 or (np.diff(starts.astype(np.int64)) < 0).any() or int(starts[nt]) != int(hdr[1]) or len(entries) != int(hdr[1]):
        bad.append(f"starts: first {starts[0]}, last {starts[nt]}, header total {hdr[1]}, {len(entries)} entries read")
    if cursors.any():
        bad.append(f"{int((cursors != 0).sum())} cursors are not back at zero (first at tile {int(np.nonzero(cursors)[0][0])})")
    slot = entries["slot"].astype(np.int64)
    if len(slot) and (slot.min() < 0 or slot.max() >= F):
        bad.append(f"slots {slot.min()} .. {slot.max()} outside [0, {F})")
    if entries["pad"].any():
        bad.append("pad words not zero")
    keys = slot * nt + entry_tiles(starts, len(slot), nt)
    listed = set(keys.tolist())
    if len(listed) != len(keys):
        u, c = np.unique(keys, return_counts=True)
        bad.append(f"{int((c > 1).sum())} (slot, tile) pairs listed more than once, e.g. slot {int(u[c > 1][0] // nt)} in tile {int(u[c > 1][0] % nt)}")
    must, may = must_list(grid, tris), may_list(grid, tris)
    if not must <= may:
        bad.append("REFERENCE: must is not inside may")
    holes, extra = sorted(must - listed), sorted(listed - may)
    if holes:
        bad.append(f"{len(holes)} pairs the rays need are not listed, e.g. (slot, tile) {[(k // nt, k % nt) for k in holes[:4]]}")
    if extra:
        bad.append(f"{len(extra)} pairs listed beyond the padded test, e.g. (slot, tile) {[(k // nt, k % nt) for k in extra[:4]]}")
    hist = np.bincount(klass(grid, tris), minlength=4)
    fig = {"must": len(must), "listed": len(listed), "may": len(may), "classes": [int(v) for v in hist]}
    return fig, bad, keys


def check_entries(grid, tris, entries):
    """every entry against the float64 projection of its triangle -> (figures, complaints)"""
    bad = []
    entries = entries[(entries["slot"] >= 0) & (entries["slot"] < len(tris))]  # (check_lists names the others)
    slot = entries["slot"].astype(np.int64)
    bb, e = entries["bb"].astype(np.float64), entries["e"].astype(np.float64).reshape(-1, 3, 3)
    xy, area2, scale = projection(grid, tris)
    _, surely, surely_not = trust(grid, tris)
    untrusted = np.isinf(bb).any(1)
    flat = (e == np.array([0.0, 0.0, 1.0])).all((1, 2))
    degenerate, normal = ~untrusted & flat, ~untrusted & ~flat
    w = untrusted & ~((bb == np.array([-np.inf, -np.inf, np.inf, np.inf])).all(1) & flat)
    if w.any():
        bad.append(f"{int(w.sum())} entries with an infinite box are not exactly (-inf, -inf, inf, inf), (0, 0, 1) x 3")
    if (~np.isfinite(bb[~untrusted])).any() or (~np.isfinite(e)).any():
        bad.append("non-finite numbers in a trusted entry")
    w = untrusted & surely[slot]
    if w.any():
        bad.append(f"{int(w.sum())} always-pass entries for triangles that are in front and within FAR tiles, e.g. slot {int(slot[w][0])}")
    w = ~untrusted & surely_not[slot]
    if w.any():
        bad.append(f"{int(w.sum())} projected entries for triangles with a vertex behind / beside the apex, e.g. slot {int(slot[w][0])}")
    with np.errstate(invalid="ignore"):
        sure_area = np.abs(area2) > 2 * SLIVER * scale
        sure_sliver = np.abs(area2) < 0.5 * SLIVER * scale
    w = degenerate & surely[slot] & sure_area[slot] & (projection_error(grid, tris)[slot] <= 0.5 * PAD)
    if w.any():
        bad.append(f"{int(w.sum())} box-only entries for projections that are no slivers, e.g. slot {int(slot[w][0])}")
    w = normal & sure_sliver[slot]
    if w.any():
        bad.append(f"{int(w.sum())} entries trust the orientation of a sliver, e.g. slot {int(slot[w][0])}")
    # ---- the box and the edge functions of entries whose triangle float64 also projects
    t = ~untrusted & np.isfinite(xy[slot]).all((1, 2))
    v = xy[slot[t]]
    lo, hi = v.min(1), v.max(1)
    b = bb[t]
    inside = (b[:, :2] <= lo) & (b[:, 2:] >= hi)
    tight = (b[:, :2] >= lo - 2 * PAD) & (b[:, 2:] <= hi + 2 * PAD)
    if not inside.all() or not tight.all():
        bad.append(f"boxes: {int((~inside.all(1)).sum())} do not hold the projection, {int((~tight.all(1)).sum())} exceed it by more than 2 PAD, e.g. slot {int(slot[t][~(inside & tight).all(1)][0])}")
    n = normal[t]
    en, vn, sn = e[t][n], v[n], slot[t][n]
    cen = vn.mean(1)
    pts = np.concatenate([vn, cen[:, None]], 1)  # [N,4,2]
    val = np.einsum("nkc,npc->nkp", en[:, :, :2], pts) + en[:, :, 2:3]
    if (val < 0).any():
        w = (val < 0).any((1, 2))
        bad.append(f"{int(w.sum())} entries have an edge function below zero at a vertex or the centroid of their own triangle, e.g. slot {int(sn[w][0])}")
    # the centroid mirrored across edge k (through vertices k and k + 1) and pushed 4 PAD further out lies outside that edge
    p, q = vn, np.roll(vn, -1, 1)
    d = q - p
    L = np.linalg.norm(d, axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.stack([-d[..., 1], d[..., 0]], -1) / L
    dist = ((cen[:, None] - p) * nrm).sum(2, keepdims=True)  # signed distance of the centroid from the edge's line
    out_pt = cen[:, None] - (2 * dist + np.sign(dist) * 4 * PAD) * nrm
    val = (en[:, :, :2] * out_pt).sum(2) + en[:, :, 2]
    use = np.isfinite(val)
    if (val[use] >= 0).any():
        w = ((val >= 0) & use).any(1)
        bad.append(f"{int(w.sum())} entries have an edge function that does not turn negative beyond its edge, e.g. slot {int(sn[w][0])}")
    orient = np.sign(area2[sn])
    fig = {"normal": int(normal.sum()), "degenerate": int(degenerate.sum()), "untrusted": int(untrusted.sum()), "ccw": int((orient > 0).sum()), "cw": int((orient < 0).sum())}
    return fig, bad


def reader_points(grid, tris):
    """(slot [N], xy [N,2]) of every triangle wholly in front: its projected vertices and edge midpoints pulled 1e-3 tile towards the centroid (half the
    way, if that is less) and the centroid — those that fall inside the grid"""
    xy, _, _ = projection(grid, tris)
    f = np.nonzero(np.isfinite(xy).all((1, 2)))[0]
    v = xy[f]
    cen = v.mean(1, keepdims=True)
    raw = np.concatenate([v, 0.5 * (v + np.roll(v, -1, 1))], 1)
    d = cen - raw
    L = np.linalg.norm(d, axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        pts = np.concatenate([raw + np.where(L > 0, d / L, 0.0) * np.minimum(1e-3, 0.5 * L), cen], 1)
    slot = np.repeat(f, pts.shape[1])
    pts = pts.reshape(-1, 2)
    ok = (pts[:, 0] >= 0) & (pts[:, 0] < grid.nx) & (pts[:, 1] >= 0) & (pts[:, 1] < grid.ny)
    return slot[ok], pts[ok]


def check_reader(grid, tris, starts, entries):
    """a reader at a point of a triangle finds the triangle in the list of the point's tile, and its entry passes traverse_bins' test (box, then the three
    edge functions) for a rectangle of zero half extents there -> (figures, complaints)"""
    nt = grid.nx * grid.ny
    slot, pts = reader_points(grid, tris)
    tile = np.floor(pts[:, 1]).astype(np.int64) * grid.nx + np.floor(pts[:, 0]).astype(np.int64)
    keys = entries["slot"].astype(np.int64) * nt + entry_tiles(starts, len(entries), nt)
    order = np.argsort(keys, kind="stable")
    want = slot * nt + tile
    at = np.searchsorted(keys[order], want)
    found = (at < len(keys)) & (keys[order][np.minimum(at, max(len(keys) - 1, 0))] == want) if len(keys) else np.zeros(len(want), bool)
    bad = []
    if not found.all():
        bad.append(f"{int((~found).sum())} points of a triangle whose tile does not list it, e.g. slot {int(slot[~found][0])} at {pts[~found][0]}")
    en = entries[order[at[found]]]
    p = pts[found].astype(np.float32).astype(np.float64)
    bb, e = en["bb"].astype(np.float64), en["e"].astype(np.float64).reshape(-1, 3, 3)
    ok = (bb[:, 0] <= p[:, 0]) & (bb[:, 2] >= p[:, 0]) & (bb[:, 1] <= p[:, 1]) & (bb[:, 3] >= p[:, 1])
    ok &= ((e[:, :, 0] * p[:, None, 0] + e[:, :, 1] * p[:, None, 1] + e[:, :, 2]) >= 0).all(1)
    if not ok.all():
        bad.append(f"{int((~ok).sum())} points of a triangle that its own entry rejects, e.g. slot {int(slot[found][~ok][0])} at {pts[found][~ok][0]}")
    return {"points": int(len(want))}, bad


# ----------------------------------------------------------------------------- envelopes
def _cell_pairs(grid, P, front):
    """(slot, cx, cy) of every (triangle, cell) whose cell lies in the product of the triangle's wedge columns and rows of the FINE grid"""
    fine = Grid(grid.name, np.eye(3), np.zeros(3), grid.nx * ENV_SUB, grid.ny * ENV_SUB)
    Q = P * np.array([ENV_SUB, ENV_SUB, 1.0])
    return _pairs(fine, Q, 0.0, front)


def _lone_cells(f, cx, cy, ny, nx, reach=2):
    """[ny, nx] bool: cells in whose (2 reach + 1)^2 neighbourhood the bounding boxes of exactly one and the same triangle lie; not the grid's rim"""
    cnt, who = np.zeros((ny, nx), np.int64), np.zeros((ny, nx), np.int64)
    np.add.at(cnt, (cy, cx), 1)
    np.add.at(who, (cy, cx), f)
    lone = np.zeros((ny, nx), bool)
    r = reach
    if ny <= 2 * r or nx <= 2 * r:
        return lone
    lone[r: ny - r, r: nx - r] = True
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sl = (slice(r + dy, ny - r + dy), slice(r + dx, nx - r + dx))
            lone[r: ny - r, r: nx - r] &= (cnt[sl] == 1) & (who[sl] == who[r: ny - r, r: nx - r])
    return lone


def check_envelope(grid, tris, cells, starts=None, entries=None, apex=None):
    """cells [ny SUB, nx SUB, 4] of an emitter's grid against every triangle of the scene.  A FINITE cell's plane N . (X - o) = 1 lies in front of the
    counted part of every shadow ray through the cell: over the part of a triangle inside the cell's pyramid both 1 / s_j (the triangle's plane along the
    ray d) and N . d are affine in the image point, so the vertices of the clipped polygon decide —  N . d > 0 and s_j >= (1 - SHADOW_EPS) / (N . d)
    there, with 1e-9 for this float64.  A ZERO cell overlaps no triangle.  A NaN cell (no proof offered) needs a reason (starts, entries and the apex
    records (A [F,3], T [F]) given): an entry of its tile whose box reaches the neighbourhood of one of the cell's four vertices and whose plane value
    there is below 1.01 |n_j| graz, not positive, or whose T is zero.  And a cell that one triangle alone decides has its plane no further in front
    than the kernel's stated margins put it (below) -> (figures — `worst`: the largest s_env / s_j over real overlaps —, complaints)"""
    ny, nx = grid.ny * ENV_SUB, grid.nx * ENV_SUB
    N3 = cells[..., :3].astype(np.float64)
    bad = []
    if cells.shape != (ny, nx, 4) or (cells[..., 3] != 0).any():
        bad.append(f"cells {cells.shape}, fourth words not zero: {int((cells[..., 3] != 0).sum())}")
    nan = np.isnan(N3).any(2)
    zero = ~nan & (N3 == 0).all(2)
    finite = ~nan & ~zero
    if (~np.isfinite(N3[finite])).any():
        bad.append("infinite plane in a cell")
    P = grid.homog(tris)
    f, cx, cy = _cell_pairs(grid, P, (P[:, :, 2] > 0).any(1))
    f_all, cx_all, cy_all = f, cx, cy
    f, cx, cy = (v[~nan[cy, cx]] for v in (f, cx, cy))
    h = 1.0 / ENV_SUB
    lim = (1.0 - SHADOW_EPS) * (1.0 - 1e-9)
    # ---- most pairs are settled without a polygon: in the image plane the triangle's plane is 1 / s_j = m_j . (x, y, 1) and the cell's is N . d =
    # Nh . (x, y, 1), both affine — N . d > 0 and N . d >= (1 - SHADOW_EPS) m_j at the cell's four corners hold over the whole cell, and so over the
    # part of the triangle inside it (whether there is one or not).  The pairs this does not settle, and every pair of a zero cell, are clipped
    nP = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    kP = (nP * P[:, 0]).sum(1)
    Nh = N3[cy, cx] @ grid.Minv
    corner = np.stack([np.stack([(cx + i) * h, (cy + j) * h, np.ones(len(cx))], 1) for i in (0, 1) for j in (0, 1)], 1)  # [n,4,3]
    with np.errstate(invalid="ignore", divide="ignore"):
        mj = (corner * nP[f][:, None]).sum(2) / kP[f][:, None]
        Ndc = (corner * Nh[:, None]).sum(2)
        settled = finite[cy, cx] & np.isfinite(mj).all(1) & (Ndc > 0).all(1) & (Ndc >= lim * mj).all(1)
        bound = np.where(settled, np.where(mj > 0, mj / Ndc, 0.0).max(1), 0.0)  # of s_env / s_j over the cell, whatever part of it the triangle covers
    n_pairs = len(f)
    # ---- and not needlessly far in front.  A cell that lies wholly inside ONE triangle's projection, with no other triangle's box within two cells
    # of it, gets its four vertex values from that triangle's plane alone: the bilinear patch IS the plane, and k_bin_env adds 2e-6 (|c0| + the
    # slopes across the cell) and a few float32 roundings (1e-5 here) before kap = (1 - SHADOW_EPS)(1 + 6e-5) (ffx_common.h): somewhere on the cell
    # s_env / s_j reaches 1 / (kap (1 + delta)) — the envelope does spend the ignored tail of the shadow ray
    lone = _lone_cells(f_all, cx_all, cy_all, ny, nx)[cy, cx] & finite[cy, cx]
    nE = np.cross(P, np.roll(P, -1, 1))[f[lone]]  # [n,3 edges,3]: the planes through the apex and each edge
    side = np.einsum("nkc,nec->nke", corner[lone], nE)
    lone[lone] = (P[f[lone], :, 2] > 0).all(1) & ((side >= 0).all(2) | (side <= 0).all(2)).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx, mn = mj[lone].max(1), mj[lone].min(1)
        delta = 2e-6 * (3 * mx - 2 * mn) / mn + 1e-5
        slack = lone.copy()
        slack[lone] = (mn > 0) & ~((mj[lone] / Ndc[lone]).max(1) >= 1.0 / ((1.0 - SHADOW_EPS) * (1.0 + 6e-5) * (1.0 + delta)))
    if slack.any():
        k = np.nonzero(slack)[0][0]
        bad.append(f"{int(slack.sum())} of {int(lone.sum())} cells inside one triangle alone have their plane further in front than the kernel's margins explain: s_env / s_j "
                   f"{float((mj[k] / Ndc[k]).max()):.9f}, e.g. slot {int(f[k])} in cell ({int(cx[k])}, {int(cy[k])})")
    n_lone = int(lone.sum())
    fs, cxs, cys, bound = (v[settled] for v in (f, cx, cy, bound))
    f, cx, cy = (v[~settled] for v in (f, cx, cy))
    poly, cnt = clip_to_boxes(P[f], cx * h, cy * h, (cx + 1) * h, (cy + 1) * h)
    ok = _overlap(poly, cnt, P[f])
    f, cx, cy, poly, cnt = f[ok], cx[ok], cy[ok], poly[ok], cnt[ok]
    w = zero[cy, cx]
    if w.any():
        bad.append(f"{int(w.sum())} (triangle, cell) overlaps in cells that claim to be empty, e.g. slot {int(f[w][0])} in cell ({int(cx[w][0])}, {int(cy[w][0])})")
    fin = finite[cy, cx]
    D = poly[fin] @ grid.Minv.T  # the polygon's vertices as world offsets from the apex: directions d of the rays through them
    use = np.arange(poly.shape[1])[None, :] < cnt[fin][:, None]
    tw = np.asarray(tris, np.float64)[f[fin]]
    nj = np.cross(tw[:, 1] - tw[:, 0], tw[:, 2] - tw[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        s_j = ((tw[:, 0] - grid.o) * nj).sum(1)[:, None] / (D * nj[:, None]).sum(2)  # the ray / plane intersection, two-sided (1 up to rounding: d ends on the triangle)
        Nd = (D * N3[cy[fin], cx[fin]][:, None]).sum(2)
        ratio = np.where(use & (Nd > 0), 1.0 / (Nd * s_j), 0.0)  # s_env / s_j
        leak = use & (Nd > 0) & ~(s_j >= lim / Nd)
    neg = use & ~(Nd > 0)
    if neg.any():
        bad.append(f"{int(neg.any(1).sum())} (triangle, cell) overlaps where the cell's plane lies behind the emitter (N . d <= 0)")
    worst = float(ratio.max()) if ratio.size else 0.0
    # the worst ratio over REAL overlaps: a settled pair counts with what its clipped polygon gives, and only pairs whose bound over the cell exceeds
    # the worst found so far can raise it — those are clipped, largest bound first
    order = np.argsort(-bound)
    for s0 in range(0, len(order), 20000):
        i = order[s0: s0 + 20000]
        if not (bound[i[0]] > worst):
            break
        pl, cn = clip_to_boxes(P[fs[i]], cxs[i] * h, cys[i] * h, (cxs[i] + 1) * h, (cys[i] + 1) * h)
        o = _overlap(pl, cn, P[fs[i]])
        with np.errstate(invalid="ignore", divide="ignore"):
            r = ((pl[o] @ grid.Minv.T) * N3[cys[i][o], cxs[i][o]][:, None]).sum(2)  # N . D: the vertex as a world offset D ends ON the triangle, s_j = 1 along it
            r = np.where((np.arange(pl.shape[1])[None, :] < cn[o][:, None]) & (r > 0), 1.0 / r, 0.0)
        if r.size:
            worst = max(worst, float(r.max()))
    if leak.any():
        k = np.nonzero(leak.any(1))[0][0]
        bad.append(f"{int(leak.any(1).sum())} (triangle, cell) overlaps where the plane lies behind the triangle: worst s_env / s_j {float(ratio.max()):.9f} against {1.0 / (1.0 - SHADOW_EPS):.9f}, "
                   f"e.g. slot {int(f[fin][k])} in cell ({int(cx[fin][k])}, {int(cy[fin][k])})")
    n_unjust = 0
    if nan.any() and entries is not None:
        n_unjust = _unjustified(grid, nan, starts, entries, apex)
        if n_unjust:
            bad.append(f"{n_unjust} NaN cells without a listed triangle seen edge-on, from behind or with T = 0 near one of their vertices")
    fig = {"zero": float(zero.mean()), "finite": float(finite.mean()), "nan": float(nan.mean()), "n_nan": int(nan.sum()), "unjustified": n_unjust, "worst": worst,
           "limit": 1.0 / (1.0 - SHADOW_EPS), "pairs": n_pairs, "clipped": int(len(ok)), "lone": n_lone}
    return fig, bad


def _unjustified(grid, nan, starts, entries, apex):
    A, T = np.asarray(apex[0], np.float64), np.asarray(apex[1], np.float64)
    graz, h = grid.graz(), 1.0 / ENV_SUB
    n = 0
    for cy, cx in zip(*np.nonzero(nan)):
        tile = (cy // ENV_SUB) * grid.nx + cx // ENV_SUB
        en = entries[int(starts[tile]): int(starts[tile + 1])]
        bb, slot = en["bb"].astype(np.float64), en["slot"].astype(np.int64)
        why = False
        for vx, vy in ((cx, cy), (cx + 1, cy), (cx, cy + 1), (cx + 1, cy + 1)):
            x, y = vx * h, vy * h
            near = (bb[:, 0] <= x + h + CELL_PE) & (bb[:, 2] >= x - h - CELL_PE) & (bb[:, 1] <= y + h + CELL_PE) & (bb[:, 3] >= y - h - CELL_PE)
            s = slot[near]
            with np.errstate(invalid="ignore", divide="ignore"):
                nj = A[s] / T[s][:, None]
                pv = nj @ (grid.Minv @ np.array([x, y, 1.0]))
                why |= bool(((T[s] == 0) | ~np.isfinite(pv) | (pv <= 0) | (pv < 1.01 * np.linalg.norm(nj, axis=1) * graz)).any())
        n += not why
    return n


def build_envelope(grid, tris, factor=(1.0 - SHADOW_EPS) * (1.0 + 6e-5)):
    """a right envelope from float64: every cell a plane of constant depth along the grid's axis, at the nearest point of what overlaps it (N = factor
    max (1 / Z) M[2]: N . d = factor max (1 / Z) for every d = Minv (x, y, 1)); zero where nothing does -> cells [ny SUB, nx SUB, 4] float32"""
    P = grid.homog(tris)
    f, cx, cy = _cell_pairs(grid, P, (P[:, :, 2] > 0).any(1))
    h = 1.0 / ENV_SUB
    poly, cnt = clip_to_boxes(P[f], cx * h, cy * h, (cx + 1) * h, (cy + 1) * h)
    ok = _overlap(poly, cnt, P[f])
    with np.errstate(divide="ignore"):
        inv = np.where(np.arange(poly.shape[1])[None, :] < cnt[:, None], 1.0 / poly[:, :, 2], 0.0).max(1)
    c0 = np.zeros((grid.ny * ENV_SUB, grid.nx * ENV_SUB))
    np.maximum.at(c0, (cy[ok], cx[ok]), inv[ok])
    cells = np.zeros(c0.shape + (4,), np.float32)
    cells[..., :3] = (factor * c0[..., None] * grid.M[2]).astype(np.float32)
    return cells


# ----------------------------------------------------------------------------- a right structure, built from the reference (tests/test_bins_cpu.py)
def build_lists(grid, tris):
    """lists and entries as the header comment of ffx_common.h describes them, from float64: every pair whose triangle touches the tile grown by PAD, the
    entry's box and edge offsets padded by PAD -> (hdr, starts, cursors, entries).  What the checks above must accept."""
    F, nt = len(tris), grid.nx * grid.ny
    P = grid.homog(tris)
    trusted, _, _ = trust(grid, tris)
    xy, area2, scale = projection(grid, tris)
    f, tx, ty = _pairs(grid, P, PAD, (P[:, :, 2] > 0).any(1))
    keep = ~trusted[f]
    poly, cnt = clip_to_boxes(P[f[~keep]], tx[~keep] - PAD, ty[~keep] - PAD, tx[~keep] + 1 + PAD, ty[~keep] + 1 + PAD)
    keep[~keep] = cnt >= 1
    f, tile = f[keep], (ty * grid.nx + tx)[keep]
    order = np.lexsort((f, tile))
    f, tile = f[order], tile[order]
    en = np.zeros(len(f), ENTRY)
    en["slot"] = f
    en["e"] = np.tile(np.array([0, 0, 1], np.float32), 3)
    en["bb"] = np.array([-np.inf, -np.inf, np.inf, np.inf], np.float32)
    t = trusted[f]
    v = xy[f[t]]
    en["bb"][t] = np.concatenate([v.min(1) - PAD, v.max(1) + PAD], 1)
    with np.errstate(invalid="ignore"):
        good = np.abs(area2[f[t]]) > SLIVER * scale[f[t]]
    s = np.where(area2[f[t]] >= 0, 1.0, -1.0)[:, None]
    d = np.roll(v, -1, 1) - v
    nx_, ny_ = -s * d[..., 1], s * d[..., 0]
    c = -(nx_ * v[..., 0] + ny_ * v[..., 1]) + PAD * (np.abs(nx_) + np.abs(ny_))
    e = np.stack([nx_, ny_, c], 2).reshape(-1, 9)
    idx = np.nonzero(t)[0][good]
    en["e"][idx] = e[good]
    starts = np.zeros(nt + 1, np.uint32)
    starts[1:] = np.cumsum(np.bincount(tile, minlength=nt))
    hdr = np.zeros(16, np.uint32)
    hdr[:3] = (1, len(f), 2 * F + MAX_TILES)
    return hdr, starts, np.zeros(nt, np.uint32), en
