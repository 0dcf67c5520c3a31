"""tests/ref_refit.py on the CPU: (i) the cases of tests/refit_cases.py are what they claim — the topologies the builder's paths need, no triangle near
degenerate but the listed ones, the listed ones degenerate in float32 itself; (ii) check_blob accepts the refit restated in emulated float32
(write_expected) on the host builder's topology, for every case, pose and treelet size, and NAMES every wrong blob it is given; (iii) the oracle's blob,
where it shares a layout (records, flags, vertex-normal rows), passes the same checks at the same tolerances, and its vertex normals' deviation from
float64 is what the case table says — the figure the device's tolerance is derived from."""
import functools

import numpy as np
import pytest

from tests import ref_refit as rr
from tests import refit_cases as rc

TREELETS = (None, "4", "32")
ONE = np.float32(1.0).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _vn(name, pose_name):
    c = rc.case(name)
    return rr.vertex_normals32(c, _pose(name, pose_name), c.smooth) if any(c.smooth) else None


@functools.lru_cache(maxsize=None)
def _poses(name):
    return {p.name: p for p in rc.poses(rc.case(name))}


def _pose(name, pose_name):
    return _poses(name)[pose_name]


def _built(name, treelet, monkeypatch):
    monkeypatch.delenv("FFX_WIDE_BUILD", raising=False)
    if treelet is None:
        monkeypatch.delenv("FFX_TREELET_TRIS", raising=False)
    else:
        monkeypatch.setenv("FFX_TREELET_TRIS", treelet)
    return rc.host_build(rc.case(name))


def _expected(name, pose_name, built):
    c = rc.case(name)
    return rr.write_expected(built[0], built[1], c, _pose(name, pose_name), c.smooth, vn=_vn(name, pose_name))


def _check(blob, built, name, pose_name, stats=None):
    c = rc.case(name)
    return rr.check_blob(blob, built[1], built[0], c, _pose(name, pose_name), c.smooth, stats=stats)


# ----------------------------------------------------------------------------- (i) the cases
@pytest.mark.parametrize("name", rc.NAMES)
def test_only_the_listed_triangles_are_degenerate_and_those_exactly(name):
    """every triangle a pose does not list has |cross| > 1e-3 |e1| |e2| in float64 — so the reference needs no exclusion beyond the list — and every listed
    one has a float32 cross product of exactly zero under the device's own formula; the collapse pose lists the whole collapsed shape"""
    c = rc.case(name)
    assert [p.name for p in rc.poses(c)] == list(rc.POSE_NAMES)
    for p in rc.poses(c):
        P, B = rr.posed(c, p)
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        sin = np.linalg.norm(np.cross(e1, e2), axis=1) / np.maximum(np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1), 1e-300)
        assert (sin[~p.listed] > 1e-3).all(), (name, p.name, float(sin[~p.listed].min()))
        assert (sin[p.listed] == 0).all(), (name, p.name)
        assert rr.f32_cross_is_zero(e1.astype(np.float32), e2.astype(np.float32))[p.listed].all()
        assert (p.listed == (c.listed | (c.tri_shape == c.collapsed))).all() if p.name == "collapse" else (p.listed == c.listed).all()
        assert np.linalg.det(p.xforms[0][:3, :3].astype(np.float64)) < 0 if p.name == "mirror" else True
    vbase, n_vn = rr.vbase_of(c)
    if name in ("two_shapes", "degenerate"):
        assert c.n_tris == (648 if name == "two_shapes" else 650) and c.smooth == [False, True] and c.nfr.tolist() == [1, 2]
        for p in rc.poses(c):
            assert int(p.vert_off[1]) != int(vbase[1])  # a normal row taken at vert_off is never the right one
        assert int(_pose(name, "frame1").vert_off[1]) == int(c.stride[1]) != 0
    if name == "degenerate":
        # the three vertices of the collinear triangle are touched by listed faces only
        own = c.tris[c.n_tris - 1]
        assert c.listed[-2:].all() and c.listed.sum() == 2 and not np.isin(c.tris[~c.listed & (c.tri_shape == 1)], own).any()
        assert c.tris[c.n_tris - 2, 0] == c.tris[c.n_tris - 2, 1]
    if name == "forty_shapes":
        assert c.n_shapes == 40 and c.n_tris == 320 and not any(c.smooth)


def test_the_posing_bound_holds_for_the_emulated_float32_chain_with_room():
    """B = 4 * 2^-24 (|M| |v| + |t|) against the float32 fma chain itself: every case and pose, mirror, anisotropic scale and translation 200 included,
    sits below half of it"""
    worst = 0.0
    for name in rc.NAMES:
        c = rc.case(name)
        for p in rc.poses(c):
            P, B = rr.posed(c, p)
            got = np.stack([rr._xf32(p.xforms[c.tri_shape], c.pool[c.tris[:, k] + p.vert_off[c.tri_shape]]) for k in range(3)], 1).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(B > 0, np.abs(got - P) / B, 0.0)
            assert (np.abs(got - P) <= B).all()
            worst = max(worst, float(q.max()))
    print("posed float32 chain / B: worst", worst)
    assert 0.05 < worst < 0.5


@pytest.mark.parametrize("treelet", TREELETS)
def test_the_builder_gives_the_topologies_the_cases_are_there_for(treelet, monkeypatch):
    infos = {n: _built(n, treelet, monkeypatch) for n in rc.NAMES}
    one, leaf4, c65 = infos["one"][1], infos["leaf4"][1], infos["cluster65"][1]
    assert one.n_nodes == 1 and one.n_wide == 0 and one.n_treelets == 1
    A = rr.Areas(infos["leaf4"][0], leaf4)
    assert leaf4.n_nodes == 1 and int(A.nodes[0, 13].view(np.int32)) == rr.EMPTY and (~int(A.nodes[0, 12].view(np.int32)) & 7) + 1 == 4
    assert c65.n_wide >= 1 and infos["two_shapes"][1].n_wide >= 1
    if treelet is None:
        assert infos["two_shapes"][1].n_treelets > 1
    if treelet == "4":  # some treelet is a bare leaf hanging off the top: it owns slots but no node
        for n in ("cluster65", "two_shapes", "forty_shapes", "degenerate"):
            blob, info = infos[n]
            hdr = rr.Areas(blob, info).plan[: 8 * info.n_treelets].reshape(-1, 8)
            assert ((hdr[:, 1] > 0) & (hdr[:, 3] == 0)).any(), n
            assert int(rr.Areas(blob, info).plan[8 * info.n_treelets + 3]) >= 1  # ... and the top has levels of its own


# ----------------------------------------------------------------------------- (ii) the reference accepts its own blob, and names every wrong one
@pytest.mark.parametrize("treelet", TREELETS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_check_blob_accepts_the_restated_refit(name, treelet, monkeypatch):
    built = _built(name, treelet, monkeypatch)
    for pose_name in rc.POSE_NAMES:
        stats = {}
        found = _check(_expected(name, pose_name, built), built, name, pose_name, stats)
        assert found == [], (name, pose_name, found[:5])
        assert stats.get("gn_not_firm", 0) == 0  # no geometric normal escaped the 3e-6 comparison but the exact zeros
        if pose_name == "far" and treelet is None:
            print(name, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in stats.items()})


def test_check_blob_needs_no_pose_for_tier_b(monkeypatch):
    built = _built("two_shapes", None, monkeypatch)
    blob = _expected("two_shapes", "mirror", built)
    assert rr.check_blob(blob, built[1], built[0]) == []
    rr.Areas(blob, built[1]).tq[7, 1] ^= 0x00400000
    assert "tq.enclose" in rr.names(rr.check_blob(blob, built[1], built[0])) or "tq.tight" in rr.names(rr.check_blob(blob, built[1], built[0]))


def _ulp(word, outward_sign):
    """the float32 bits one ulp further in the direction of `outward_sign` (+1: towards +inf)"""
    v = np.array([word], np.uint32).view(np.float32)
    return np.nextafter(v, np.float32(np.inf * outward_sign)).view(np.uint32)[0]


def _inner_child(A):
    for i in range(A.N):
        for side in (0, 1):
            if int(A.nodes[i, 12 + side].view(np.int32)) >= 0:
                return i, side
    raise AssertionError("no inner child")


def _mutations():
    """name -> (case, pose, spoil(A, case, pose, built) — edits the areas of an expected blob in place —, the finding that must name it)"""
    def tq_in(A, c, p, built):
        # lo.x of the slot that bounds its leaf on that side, one ulp inward: still inside the pad's window (an ulp is 6e-8 of the magnitude, the window
        # 2e-7 either way), but no longer what the leaf above it unites.  (A bound that is not its leaf's extreme is out of the unions' sight.)
        for i in A.refit:
            c0 = int(A.nodes[i, 12].view(np.int32))
            if c0 >= 0 or c0 == rr.EMPTY:
                continue
            first, cnt = (~c0 & 0xFFFFFFFF) >> 3, (~c0 & 7) + 1
            v = np.sort(A.tq[first: first + cnt, 0].view(np.float32))
            if cnt == 1 or v[0] < v[1]:  # (triangles of one patch share corners: take a leaf whose extreme belongs to one slot)
                k = first + int(np.argmin(A.tq[first: first + cnt, 0].view(np.float32)))
                A.tq[k, 0] = _ulp(A.tq[k, 0], +1)
                return
        raise AssertionError("no leaf with a unique extreme")

    def tq_out(A, c, p, built):
        v = A.tq[5, 3:4].view(np.float32)  # hi.x outward by 1e-5 of its magnitude (pose `far`: 200)
        v[0] = np.float32(v[0] + 1e-5 * abs(v[0]))

    def stale_inner(A, c, p, built):
        big = rr.Areas(_expected("two_shapes", "rot_aniso", built), built[1])
        i, side = _inner_child(A)
        A.nodes[i, 6 * side: 6 * side + 6] = big.nodes[i, 6 * side: 6 * side + 6]

    def stale_wide(A, c, p, built):
        big = rr.Areas(_expected("cluster65", "rot_aniso", built), built[1])
        k = rr.walk_wide(built[1], A)[1][0]
        A.wn[k, :6] = big.wn[k, :6]

    def swap(A, c, p, built):
        A.recs[9, 3:6], A.recs[9, 6:9] = A.recs[9, 6:9].copy(), A.recs[9, 3:6].copy()

    def row_at_vert_off(A, c, p, built):
        vn = _vn(c.name, p.name)
        k = int(np.nonzero(c.tri_shape[A.order] == 1)[0][0])
        A.nrec[k, :, :3] = vn[c.tris[A.order[k]] + p.vert_off[1]].view(np.uint32)

    def smooth_slot(A, c):
        return int(np.nonzero((A.recs[:, 11] == ONE) & (A.gn[:, 3] != 0))[0][0])

    def tag_no_smooth(A, c, p, built):
        A.gn[smooth_slot(A, c), 3] &= ~np.uint32(1 << 30)

    def tag_shape(A, c, p, built):
        A.gn[smooth_slot(A, c), 3] -= 1

    def tag_on_degenerate(A, c, p, built):
        k = int(np.nonzero(p.listed[A.order])[0][0])
        A.gn[k, 3] = np.uint32(2 | (1 << 30))

    def c0(A, c, p, built):
        A.nodes[0, 12] ^= 8

    def counter(A, c, p, built):
        A.plan[-1] = 1

    return {
        "a tq bound moved inward by one ulp": ("two_shapes", "back", tq_in, "node.leaf"),
        "a tq bound moved outward by 1e-5 of its magnitude": ("two_shapes", "far", tq_out, "tq.tight"),
        "an inner box left at the previous, larger pose": ("two_shapes", "tiny", stale_inner, "node.inner"),
        "a wide child not refreshed": ("cluster65", "tiny", stale_wide, "wide.box"),
        "a record's e1 and e2 swapped": ("two_shapes", "mirror", swap, "rec.e1"),
        "a normal row taken at vert_off instead of vbase": ("two_shapes", "back", row_at_vert_off, "vn.row"),
        "the tag word without the smooth bit": ("two_shapes", "back", tag_no_smooth, "gn.tag"),
        "the tag word with shape instead of shape + 1": ("two_shapes", "back", tag_shape, "gn.tag"),
        "a non-zero tag on a degenerate slot": ("degenerate", "rot_aniso", tag_on_degenerate, "gn.zero"),
        "a c0 word overwritten": ("two_shapes", "identity", c0, "own.child"),
        "the plan counter left at 1": ("two_shapes", "identity", counter, "own.counter"),
    }


MUTATIONS = _mutations()


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_check_blob_names_the_mutation(what, monkeypatch):
    name, pose_name, spoil, finding = MUTATIONS[what]
    built = _built(name, None, monkeypatch)
    blob = _expected(name, pose_name, built)
    assert _check(blob, built, name, pose_name) == []
    spoil(rr.Areas(blob, built[1]), rc.case(name), _pose(name, pose_name), built)
    found = _check(blob, built, name, pose_name)
    print(what, "->", found[:4])
    assert finding in rr.names(found), (what, found)


# ----------------------------------------------------------------------------- (iii) the oracle
@pytest.mark.parametrize("name", rc.NAMES)
def test_the_oracles_records_flags_and_normal_rows_pass_and_its_normals_deviate_as_tabulated(name, oracle):
    """the oracle's update over the same sequence of poses on one blob: tier A at the device's tolerances, and — the figure those tolerances are four times
    of — the largest deviation of its float32 vertex normals from float64 per pose: at most what tests/refit_cases.py records, and no less than half of
    it (the table is a measurement, not a guess)"""
    c = rc.case(name)
    go = oracle.Geometry(c.pool, c.tris, c.tri_shape, c.off, smooth=c.smooth)
    for p in rc.poses(c):
        go.update(p.xforms, p.vert_off)
        stats = {}
        found = rr.check_oracle_blob(go.blob, go.info, c, p, c.smooth, stats)
        print(f"{name:13s} {p.name:10s} oracle: v0 {stats['rec_v0_over_B']:.2f} B, e {stats['rec_e_over_bound']:.2f} of its bound, "
              f"vertex normals {stats.get('vn_dev', float('nan')):.3e}")
        assert found == [], (name, p.name, found[:5])
        assert stats["rec_v0_over_B"] <= 0.5
        if any(c.smooth):
            rec = rc.VN_MEASURED[name][p.name]
            assert 0.5 * rec <= stats["vn_dev"] <= rec, (name, p.name, stats["vn_dev"], rec)
