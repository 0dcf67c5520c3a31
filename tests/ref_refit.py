"""What ffx_scene_update must leave in the BVH blob for a pose, restated in float64 — TEST INFRASTRUCTURE (numpy only: no torch, no library call, and
nothing read from any kernel but the blob under test).

The update (fireflies_amd/csrc/ffx_scene.hip) writes six things every render, trace, pre-pass and adjoint starts from: the 48-byte triangle records, the
per-slot geometric normals with their tag word (off_gn), the per-slot vertex normals (off_nrec), the per-triangle boxes (off_tq), the binary nodes'
child boxes and the 64-wide overlay's child boxes.  This module states them from include/ffx.h and ffx_common.h:

  posed(case, pose)     the world corners [F,3,3] in float64 from the float32 pool, vert_off, the shape-local triangles, tri_shape and each shape's
                        float32 4x4 — and B, the rounding bound of the device's fma chain per component
  check_blob(...)       a host copy of a blob against the pose (tier A) and against itself and the builder's output (tier B); returns a list of named
                        findings, empty when the blob is right (tests/test_refit_cpu.py feeds it right and wrong blobs)
  check_oracle_blob     tier A's records, flags and vertex-normal rows on the oracle's blob, which shares those layouts (its nodes are its own)
  write_expected(...)   a numpy restatement of the refit in emulated float32 (every fma as float32(float64(a) * b + c)) on a copy of the builder's
                        blob: what check_blob must accept, and what the CPU tests spoil

Bounds, all derived (none was measured on the code under test):
  B = 4 * 2^-24 (|M| |v| + |t|)    a posed coordinate is fma(m0, x, fma(m1, y, fma(m2, z, t))): three fused steps, each rounded once, each at most
                                   half an ulp (2^-24 relative) of a partial sum no larger than |M| |v| + |t|; 4 instead of 3 leaves room
  |v0 - p0| <= B;  |e1 - (p1 - p0)| <= B(p0) + B(p1) + 2^-24 |e1|    (one rounded subtraction more)
  geometric normal: atol 3e-6 against normalize(cross(e1, e2)) of the RECORD in float64 (the project's figure for this quantity)
  triangle box: with mn, mx the float64 extent of v0, v0 + e1, v0 + e2 on an axis and m = max(|mn|, |mx|):
      mn - (6e-7 m + 1.01 leaf_pad) <= lo <= mn - (2e-7 m + 0.99 leaf_pad), mirrored for hi
    — the device pads by fmaf(4e-7, m, leaf_pad) after re-rounding one corner and rounds the subtraction, each at most 6e-8 m.  The lower bound is
    enclosure with a real margin, the upper bound tightness (a box that is too large renders the same bits, only slower)
  every box above the triangles is a pure min / max of boxes below it: bit for bit
  vertex normals: the case's own bound (tests/refit_cases.py: four times the oracle's measured deviation from float64)
"""
import numpy as np

from tests import ref_bruteforce as rbf

EMPTY = -(2**31)
U = 2.0**-24
GN_ATOL = 3e-6
f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------- the blob's areas
class Areas:
    """numpy views into a host copy of a blob (include/ffx.h ffx_bvh_info, ffx_common.h BvhNode / TriRec / WideChild)"""

    def __init__(self, blob, info):
        blob = np.asarray(blob).view(np.uint8).reshape(-1)
        F, N, nw = int(info.n_tris), int(info.n_nodes), int(info.n_wide)

        def words(off, n):
            return blob[int(off): int(off) + 4 * n].view(np.uint32)

        self.F, self.N, self.nw = F, N, nw
        self.nodes = words(info.off_nodes, 16 * N).reshape(N, 16)  # lo0 hi0 lo1 hi1 (12 floats), c0, c1, pad0, pad1
        self.order = words(info.off_order, F).view(np.int32)
        self.refit = words(info.off_refit, N).view(np.int32)
        self.recs = words(info.off_recs, 12 * F).reshape(F, 12)  # v0, e1, e2, prim, shape, flag
        self.wn = words(info.off_wnodes, 8 * 64 * nw).reshape(64 * nw, 8)  # lo, hi, ref, pad
        self.tq = words(info.off_tq, 8 * F).reshape(F, 8)
        self.wsrc = words(info.off_wsrc, 64 * nw).view(np.int32)
        self.plan = words(info.off_plan, int(info.plan_ints)).view(np.int32)
        self.nrec = words(info.off_nrec, 12 * F).reshape(F, 3, 4)
        self.gn = words(info.off_gn, 4 * F).reshape(F, 4)


def _f(a):
    return a.view(np.float32)


# ----------------------------------------------------------------------------- the pose
def posed(case, pose):
    """-> (P [F,3,3] float64 world corners in scene order, B [F,3,3] the device's rounding bound per component)"""
    v = case.pool[case.tris + pose.vert_off[case.tri_shape][:, None]].astype(f64)  # [F,3,3]
    m = pose.xforms.astype(f64)[case.tri_shape]  # [F,4,4]
    P = np.einsum("fij,fkj->fki", m[:, :3, :3], v) + m[:, None, :3, 3]
    B = 4.0 * U * (np.einsum("fij,fkj->fki", np.abs(m[:, :3, :3]), np.abs(v)) + np.abs(m[:, None, :3, 3]))
    return P, B


def reference_normals(case, pose):
    """{smooth shape: [n_local, 3] float64}: tests/ref_bruteforce.vertex_normals on the float64 posed vertices of the shape's current frame, over the
    shape's faces only, the pose's listed triangles left out"""
    out = {}
    for s in range(case.n_shapes):
        if not case.smooth[s]:
            continue
        sel = case.tri_shape == s
        tr = case.tris[sel]
        n_local = int(tr.max()) + 1
        m = pose.xforms[s].astype(f64)
        v = case.pool[int(pose.vert_off[s]): int(pose.vert_off[s]) + n_local].astype(f64)
        out[s] = rbf.vertex_normals(v @ m[:3, :3].T + m[:3, 3], tr, use=~pose.listed[sel])
    return out


def vbase_of(case):
    """ffx_smooth.shape_vbase: the first vertex-normal row of each shape (one frame each, in shape order)"""
    n_local = np.zeros(case.n_shapes, np.int64)
    np.maximum.at(n_local, case.tri_shape, case.tris.max(axis=1) + 1)
    return np.concatenate([[0], np.cumsum(n_local)[:-1]]).astype(np.int64), int(n_local.sum())


# ----------------------------------------------------------------------------- tier A
def _tier_a(out, stats, recs, order, nrec, case, pose, smooth):
    F = case.n_tris
    if sorted(order.tolist()) != list(range(F)):
        out.append("rec.order: the slots do not hold a permutation of the triangles")
        return
    P, B = posed(case, pose)
    P, B = P[order], B[order]
    sh = case.tri_shape[order]
    r = _f(recs[:, :9]).astype(f64).reshape(F, 3, 3)
    prim, shape, flag = recs[:, 9].view(np.int32), recs[:, 10].view(np.int32), recs[:, 11]
    for k in np.nonzero(prim != order)[0][:3]:
        out.append(f"rec.prim: slot {k} holds prim {prim[k]}, order says {order[k]}")
    for k in np.nonzero(shape != sh)[0][:3]:
        out.append(f"rec.shape: slot {k} holds shape {shape[k]}, the scene says {sh[k]}")
    on = np.array([bool(smooth is not None and any(smooth) and smooth[s]) for s in range(case.n_shapes)])[sh]
    want = np.where(on, f32(1.0).view(np.uint32), np.uint32(0))
    for k in np.nonzero(flag != want)[0][:3]:
        out.append(f"rec.flag: slot {k} (shape {sh[k]}) holds the bits {int(flag[k]):#x}, want {int(want[k]):#x}")
    d0 = np.abs(r[:, 0] - P[:, 0])
    stats["rec_v0_over_B"] = max(stats.get("rec_v0_over_B", 0.0), float((d0 / np.where(B[:, 0] > 0, B[:, 0], 1.0)).max()))
    for k in np.nonzero((d0 > B[:, 0]).any(1))[0][:3]:
        out.append(f"rec.v0: slot {k} (prim {order[k]}) off by {d0[k].max():.3e}, bound {B[k, 0].max():.3e}")
    for c, name in ((1, "e1"), (2, "e2")):
        d = np.abs(r[:, c] - (P[:, c] - P[:, 0]))
        bound = B[:, 0] + B[:, c] + U * np.abs(r[:, c])
        stats["rec_e_over_bound"] = max(stats.get("rec_e_over_bound", 0.0), float((d / np.where(bound > 0, bound, 1.0)).max()))
        for k in np.nonzero((d > bound).any(1))[0][:3]:
            out.append(f"rec.{name}: slot {k} (prim {order[k]}) off by {d[k].max():.3e}, bound {bound[k].max():.3e}")
    # ---- vertex normals of the flagged slots
    if not on.any():
        return
    tol = case.vn_bound(pose)
    ref = reference_normals(case, pose)
    got = _f(nrec)  # [F,3,4]
    worst = 0.0
    n_bad = 0
    for k in np.nonzero(on)[0]:
        want_rows = ref[int(sh[k])][case.tris[order[k]]]  # [3,3]: the rows vbase[shape] + local index hold
        if (nrec[k, :, 3] != 0).any():
            out.append(f"vn.w: slot {k} holds a fourth component other than 0")
        dev = np.abs(got[k, :, :3].astype(f64) - want_rows)
        zero = ~want_rows.any(1)
        if (got[k, zero, :3] != 0).any():
            out.append(f"vn.zero: slot {k}: a vertex all of whose faces are degenerate does not hold exactly (0, 0, 0)")
        worst = max(worst, float(dev.max()))
        if dev.max() > tol and n_bad < 3:
            n_bad += 1
            out.append(f"vn.row: slot {k} (prim {order[k]}, shape {sh[k]}) off by {dev.max():.3e}, bound {tol:.3e}")
    stats["vn_dev"] = max(stats.get("vn_dev", 0.0), worst)


def check_oracle_blob(blob, info, case, pose, smooth, stats=None):
    """tier A on the oracle's blob: its records, their flags and its off_nrec rows share the product's layout"""
    out, stats = [], {} if stats is None else stats
    blob = np.asarray(blob).view(np.uint8).reshape(-1)
    F = case.n_tris
    order = blob[int(info.off_order): int(info.off_order) + 4 * F].view(np.int32)
    recs = blob[int(info.off_recs): int(info.off_recs) + 48 * F].view(np.uint32).reshape(F, 12)
    nrec = blob[int(info.off_nrec): int(info.off_nrec) + 48 * F].view(np.uint32).reshape(F, 3, 4)
    _tier_a(out, stats, recs, order, nrec, case, pose, smooth)
    return out


# ----------------------------------------------------------------------------- tier B
def f32_cross_is_zero(e1, e2):
    """[F] bool: the float32 cross product of the record's edges as ffx_common.h forms it, fma(a, b, -(c d)) per component, is exactly zero (a float64
    product of two float32 is exact, and a difference of two unequal numbers never rounds to zero)"""
    a, b = e1.astype(f32), e2.astype(f32)

    def dp(p, q, r, s):
        return p.astype(f64) * q.astype(f64) - (r * s).astype(f64)  # (r * s: a float32 product, rounded once)

    n = np.stack([dp(a[:, 1], b[:, 2], a[:, 2], b[:, 1]), dp(a[:, 2], b[:, 0], a[:, 0], b[:, 2]), dp(a[:, 0], b[:, 1], a[:, 1], b[:, 0])], 1)
    return ~n.astype(f32).any(1)


def walk_wide(info, A):
    """the (wide element, binary box source) of every used child of the overlay, from wide_root down as tests/test_abi_cpu.py walks it"""
    used = []
    stack = [int(info.wide_root) & 0xFFFFFFFF]
    while stack:
        ref = stack.pop()
        if ref >> 31:
            continue  # a cluster of triangle boxes
        elem, cnt = (ref >> 6) & 0x1FFFFFF, (ref & 63) + 1
        for j in range(cnt):
            used.append((elem + j, int(A.wsrc[elem + j])))
            stack.append(int(A.wn[elem + j, 6]))
    return used


def _tier_b(out, stats, A, B0, info, smooth, listed_slots):
    F, N = A.F, A.N
    r = _f(A.recs[:, :9]).astype(f64).reshape(F, 3, 3)
    shape, flag = A.recs[:, 10].view(np.int32).astype(np.int64), A.recs[:, 11]
    one = f32(1.0).view(np.uint32)
    for k in np.nonzero((flag != 0) & (flag != one))[0][:3]:
        out.append(f"rec.flag: slot {k} holds the bits {int(flag[k]):#x}, neither 0.0f nor 1.0f")
    if smooth is not None:
        on = np.array([bool(any(smooth) and s) for s in smooth])[np.clip(shape, 0, len(smooth) - 1)]
        for k in np.nonzero((flag == one) != on)[0][:3]:
            out.append(f"rec.flag: slot {k} (shape {shape[k]}) holds the bits {int(flag[k]):#x}")
    # ---- geometric normals and their tag word
    if int(info.off_gn):
        zero = f32_cross_is_zero(r[:, 1], r[:, 2])
        n = np.cross(r[:, 1], r[:, 2])
        nl = np.linalg.norm(n, axis=1)
        sin = nl / np.maximum(np.linalg.norm(r[:, 1], axis=1) * np.linalg.norm(r[:, 2], axis=1), 1e-300)
        got = _f(A.gn[:, :3]).astype(f64)
        tag = (shape + 1) | np.where(flag == one, 1 << 30, 0)
        for k in np.nonzero(zero & A.gn.any(1))[0][:3]:
            out.append(f"gn.zero: slot {k}: a triangle whose float32 cross product is zero holds {[hex(int(w)) for w in A.gn[k]]}, not sixteen zero bytes")
        live = ~zero
        for k in np.nonzero(live & (A.gn[:, 3].astype(np.int64) != tag))[0][:3]:
            out.append(f"gn.tag: slot {k} (shape {shape[k]}, flag bits {int(flag[k]):#x}) holds the tag {int(A.gn[k, 3]):#x}, want {int(tag[k]):#x}")
        # the direction is held to 3e-6 wherever the record itself defines it: every triangle but the listed ones (of a blob without a case: those whose
        # edges are within 1e-3 of parallel, where the float32 cross product has lost its digits)
        firm = live & (~listed_slots if listed_slots is not None else sin > 1e-3)
        dev = np.abs(got - n / np.maximum(nl, 1e-300)[:, None]).max(1)
        stats["gn_dev"] = max(stats.get("gn_dev", 0.0), float(dev[firm].max()) if firm.any() else 0.0)
        stats["gn_not_firm"] = stats.get("gn_not_firm", 0) + int((live & ~firm).sum())
        for k in np.nonzero(firm & ~(dev <= GN_ATOL))[0][:3]:
            out.append(f"gn.normal: slot {k} off by {dev[k]:.3e} from the record's own cross product (atol {GN_ATOL:g})")
        ln = np.abs(np.linalg.norm(got, axis=1) - 1.0)
        for k in np.nonzero(live & ~firm & ~(ln <= GN_ATOL))[0][:3]:
            out.append(f"gn.normal: slot {k} holds a vector of length 1 {ln[k]:+.3e}")
    # ---- per-triangle boxes
    lp = float(f32(info.leaf_pad))
    corners = np.stack([r[:, 0], r[:, 0] + r[:, 1], r[:, 0] + r[:, 2]], 1)
    mn, mx = corners.min(1), corners.max(1)
    m = np.maximum(np.abs(mn), np.abs(mx))
    lo, hi = _f(A.tq[:, 0:3]).astype(f64), _f(A.tq[:, 3:6]).astype(f64)
    wide, tight = 6e-7 * m + 1.01 * lp, 2e-7 * m + 0.99 * lp
    with np.errstate(invalid="ignore"):
        encl = ~((lo <= mn - tight) & (hi >= mx + tight))
        loose = ~((lo >= mn - wide) & (hi <= mx + wide))
    for k in np.nonzero(encl.any(1))[0][:3]:
        out.append(f"tq.enclose: slot {k}: box [{lo[k]}, {hi[k]}] around [{mn[k]}, {mx[k]}] lacks its margin (leaf_pad {lp:.3e})")
    for k in np.nonzero(loose.any(1))[0][:3]:
        out.append(f"tq.tight: slot {k}: box [{lo[k]}, {hi[k]}] around [{mn[k]}, {mx[k]}] is wider than the pad allows (leaf_pad {lp:.3e})")
    for k in np.nonzero(A.tq[:, 6:8].any(1))[0][:3]:
        out.append(f"tq.ref: slot {k}: the ref / pad words are {A.tq[k, 6:8]}")
    # ---- every box above: a bit-exact union
    tlo, thi = _f(A.tq[:, 0:3]), _f(A.tq[:, 3:6])
    inf = f32(np.inf)
    n_bad = {"node.leaf": 0, "node.inner": 0, "node.empty": 0}
    for i in range(N):
        for side in (0, 1):
            c = int(A.nodes[i, 12 + side].view(np.int32))
            have = A.nodes[i, 6 * side: 6 * side + 6]
            if c == EMPTY:
                what, want = "node.empty", np.array([inf, inf, inf, -inf, -inf, -inf], f32)
            elif c < 0:
                lc = (~c) & 0xFFFFFFFF
                first, cnt = lc >> 3, (lc & 7) + 1
                what, want = "node.leaf", np.concatenate([tlo[first: first + cnt].min(0), thi[first: first + cnt].max(0)])
            else:
                ch = _f(A.nodes[c, :12])
                what, want = "node.inner", np.concatenate([np.minimum(ch[0:3], ch[6:9]), np.maximum(ch[3:6], ch[9:12])])
            if (have != want.view(np.uint32)).any():
                n_bad[what] += 1
                if n_bad[what] <= 3:
                    out.append(f"{what}: node {i} side {side} (child {c}) holds {_f(have)}, the union below it is {want}")
    used = walk_wide(info, A)
    stats["wide_children"] = len(used)
    n_w = 0
    for k, src in used:
        if not 0 <= src < 2 * N:
            out.append(f"own.wsrc: wide child {k} names the source {src}")
            continue
        want = A.nodes[src >> 1, 6 * (src & 1): 6 * (src & 1) + 6]
        if (A.wn[k, :6] != want).any():
            n_w += 1
            if n_w <= 3:
                out.append(f"wide.box: wide child {k} holds {_f(A.wn[k, :6])}, binary node {src >> 1} side {src & 1} holds {_f(want)}")
    # ---- the update writes only what it owns
    for name, a, b in (("own.order", A.order, B0.order), ("own.refit", A.refit, B0.refit), ("own.child", A.nodes[:, 12:], B0.nodes[:, 12:]),
                       ("own.wsrc", A.wsrc, B0.wsrc), ("own.wref", A.wn[:, 6:], B0.wn[:, 6:]), ("own.plan", A.plan[:-1], B0.plan[:-1])):
        if a.shape != b.shape or (a != b).any():
            out.append(f"{name}: differs from the builder's output in {int((a != b).sum()) if a.shape == b.shape else 'shape'} words")
    if int(A.plan[-1]) != 0:
        out.append(f"own.counter: the arrival counter of the plan is {int(A.plan[-1])}")


def check_blob(blob_bytes, info, builder_blob_bytes, case=None, pose=None, smooth=None, stats=None):
    """A host copy of an updated blob (at least its first off_bins bytes) against the pose (tier A: needs `case` and `pose`) and against itself and the
    builder's blob of the same topology (tier B: needs neither, so it also serves a blob whose pose the test did not choose).  smooth: the flags the
    geometry was made with.  -> a list of findings "name: what"; `stats` (a dict) receives the figures: the largest deviations and counts"""
    out, stats = [], {} if stats is None else stats
    A, B0 = Areas(blob_bytes, info), Areas(builder_blob_bytes, info)
    listed_slots = None
    if case is not None:
        _tier_a(out, stats, A.recs, A.order, A.nrec, case, pose, smooth)
        if sorted(A.order.tolist()) == list(range(A.F)):
            listed_slots = pose.listed[A.order]
    _tier_b(out, stats, A, B0, info, smooth, listed_slots)
    return out


def names(findings):
    return sorted({f.split(":", 1)[0] for f in findings})


# ----------------------------------------------------------------------------- the refit restated in emulated float32
def _fma(a, b, c):
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def _xf32(m, v):
    """xf_point: fma(m0, x, fma(m1, y, fma(m2, z, m3))) per row; m [..., 4, 4], v [..., 3] float32"""
    return np.stack([_fma(m[..., i, 0], v[..., 0], _fma(m[..., i, 1], v[..., 1], _fma(m[..., i, 2], v[..., 2], m[..., i, 3]))) for i in range(3)], -1)


def _cross32(a, b):
    def dp(p, q, r, s):
        return _fma(p, q, -(r * s))

    return np.stack([dp(a[..., 1], b[..., 2], a[..., 2], b[..., 1]), dp(a[..., 2], b[..., 0], a[..., 0], b[..., 2]), dp(a[..., 0], b[..., 1], a[..., 1], b[..., 0])], -1)


def _dot32(a, b):
    return _fma(a[..., 0], b[..., 0], _fma(a[..., 1], b[..., 1], a[..., 2] * b[..., 2]))


def _angle32(a, b):
    """Mitsuba's unit_angle as the update writes it"""
    if _dot32(a, b) >= 0:
        d = b - a
        return f32(2.0) * np.arcsin(min(f32(0.5) * np.sqrt(_dot32(d, d)), f32(1.0)))
    s = a + b
    return f32(np.pi) - f32(2.0) * np.arcsin(min(f32(0.5) * np.sqrt(_dot32(s, s)), f32(1.0)))


def vertex_normals32(case, pose, smooth, row_base=None):
    """[n_vn, 3] float32: angle-weighted vertex normals as k_vertex_normals forms them — faces in ascending order, each non-degenerate face adding
    n_face * angle to its three rows vbase[shape] + index by one fma per component"""
    vbase, n_vn = vbase_of(case)
    acc = np.zeros((n_vn, 3), f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(case.n_tris):
            s = int(case.tri_shape[t])
            if not smooth[s]:
                continue
            p = _xf32(pose.xforms[s][None], case.pool[case.tris[t] + pose.vert_off[s]])
            n = _cross32(p[1] - p[0], p[2] - p[0])
            nl = np.sqrt(_dot32(n, n))
            if not nl > 0:
                continue
            n = n / nl
            for c in range(3):
                d0, d1 = p[(c + 1) % 3] - p[c], p[(c + 2) % 3] - p[c]
                l0, l1 = np.sqrt(_dot32(d0, d0)), np.sqrt(_dot32(d1, d1))
                if not l0 > 0 or not l1 > 0:
                    continue
                row = int(vbase[s]) + int(case.tris[t, c])
                acc[row] = _fma(n, _angle32(d0 / l0, d1 / l1), acc[row])
    l = np.sqrt(_fma(acc[:, 0], acc[:, 0], _fma(acc[:, 1], acc[:, 1], acc[:, 2] * acc[:, 2])))
    return np.where(l[:, None] > 0, acc / np.where(l > 0, l, f32(1.0))[:, None], acc).astype(f32)


def write_expected(builder_blob, info, case, pose, smooth, vn=None):
    """a copy of the host-built blob filled as ffx_scene_update fills it for `pose` (module docstring); vn: vertex_normals32 of the pose, if at hand"""
    blob = np.array(builder_blob, np.uint8, copy=True)
    A = Areas(blob, info)
    F, N = A.F, A.N
    order = A.order
    sh = case.tri_shape[order]
    m = pose.xforms[sh]  # [F,4,4]
    v = case.pool[case.tris[order] + pose.vert_off[sh][:, None]]  # [F,3,3]
    p = np.stack([_xf32(m, v[:, c]) for c in range(3)], 1)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    any_smooth = smooth is not None and any(smooth)
    on = np.array([bool(any_smooth and s) for s in (smooth if smooth is not None else [False] * case.n_shapes)])[sh]
    A.recs[:, 0:3], A.recs[:, 3:6], A.recs[:, 6:9] = p[:, 0].view(np.uint32), e1.view(np.uint32), e2.view(np.uint32)
    A.recs[:, 9], A.recs[:, 10] = order.view(np.uint32), sh.view(np.uint32)
    A.recs[:, 11] = np.where(on, f32(1.0).view(np.uint32), np.uint32(0))
    if any_smooth:
        vbase, _ = vbase_of(case)
        vn = vertex_normals32(case, pose, smooth) if vn is None else vn
        rows = vbase[sh][:, None] + case.tris[order]  # [F,3]
        A.nrec[on, :, :3] = vn[rows[on]].view(np.uint32)
        A.nrec[on, :, 3] = 0
    if int(info.off_gn):
        n = _cross32(e1, e2)
        with np.errstate(invalid="ignore", divide="ignore"):
            nl = np.sqrt(_dot32(n, n))
            live = nl > 0
            unit = (n * (f32(1.0) / nl)[:, None]).astype(f32)
        A.gn[:, :3] = np.where(live[:, None], unit.view(np.uint32), np.uint32(0))
        A.gn[:, 3] = np.where(live, ((sh.astype(np.int64) + 1) | np.where(on, 1 << 30, 0)).astype(np.uint32), np.uint32(0))
    # per-triangle boxes: the record's corners re-rounded, the pad by one fma
    q = np.stack([p[:, 0], p[:, 0] + e1, p[:, 0] + e2], 1)
    mn, mx = q.min(1), q.max(1)
    pad = _fma(f32(4e-7), np.maximum(np.abs(mn), np.abs(mx)), f32(info.leaf_pad))
    A.tq[:, 0:3], A.tq[:, 3:6], A.tq[:, 6:8] = (mn - pad).view(np.uint32), (mx + pad).view(np.uint32), 0
    tlo, thi = _f(A.tq[:, 0:3]), _f(A.tq[:, 3:6])
    inf = f32(np.inf)
    for l in range(int(info.n_levels)):
        for i in A.refit[int(info.level_start[l]): int(info.level_start[l + 1])]:
            for side in (0, 1):
                c = int(A.nodes[i, 12 + side].view(np.int32))
                if c == EMPTY:
                    box = np.array([inf, inf, inf, -inf, -inf, -inf], f32)
                elif c < 0:
                    lc = (~c) & 0xFFFFFFFF
                    first, cnt = lc >> 3, (lc & 7) + 1
                    box = np.concatenate([tlo[first: first + cnt].min(0), thi[first: first + cnt].max(0)])
                else:
                    ch = _f(A.nodes[c, :12])
                    box = np.concatenate([np.minimum(ch[0:3], ch[6:9]), np.maximum(ch[3:6], ch[9:12])])
                A.nodes[i, 6 * side: 6 * side + 6] = box.view(np.uint32)
    for k in np.nonzero(A.wsrc >= 0)[0]:
        src = int(A.wsrc[k])
        A.wn[k, :6] = A.nodes[src >> 1, 6 * (src & 1): 6 * (src & 1) + 6]
    return blob
