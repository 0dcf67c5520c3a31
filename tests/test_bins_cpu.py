"""tests/ref_bins.py on the CPU: (i) the float64 reference of the tile bins on hand-built triangles whose tiles are known, (ii) must <= may on every
stage scene, and the poses of tests/test_bins_gpu.py populate every class, both orientations and every kind of entry, (iii) the checks that module
applies to the device's lists, entries and envelopes accept a right structure built from the reference and name every wrong one."""
import numpy as np
import pytest

from fireflies_amd import scene_desc
from tests import bin_cases as bc
from tests import ref_bins as rb
from tests import stage_scenes as ss

# one grid of 8 x 8 tiles about +z, 90 degrees wide: tile coordinates (4 + 4 X / Z, 4 + 4 Y / Z)
G = rb.Grid("hand", [[4, 0, 4], [0, 4, 4], [0, 0, 1]], (0, 0, 0), 8, 8)


def at(x, y, z=2.0):
    """the world point of tile coordinates (x, y) at depth z"""
    return ((x - 4.0) / 4.0 * z, (y - 4.0) / 4.0 * z, z)


def tiles(keys, grid=G):
    return sorted((int(k) % (grid.nx * grid.ny) % grid.nx, int(k) % (grid.nx * grid.ny) // grid.nx) for k in keys)


def lists(tri, grid=G):
    t = np.asarray([tri], np.float64)
    return tiles(rb.must_list(grid, t)), tiles(rb.may_list(grid, t)), int(rb.klass(grid, t)[0])


# ----------------------------------------------------------------------------- (i) known answers
def test_a_triangle_inside_one_tile():
    must, may, k = lists([at(2.2, 3.2), at(2.8, 3.3), at(2.5, 3.8, 3.0)])
    assert must == [(2, 3)] and may == [(2, 3)] and k == rb.FEW


def test_a_triangle_within_two_pads_of_a_tile_may_be_listed_there_but_need_not():
    """its right-most vertex 1.5 PAD short of tile 3: must holds tile 2 alone, may both; 2.5 PAD short: both hold tile 2 alone"""
    for gap, want in ((1.5, [(2, 3), (3, 3)]), (2.5, [(2, 3)])):
        must, may, _ = lists([at(2.2, 3.2), at(3.0 - gap * rb.PAD, 3.3), at(2.5, 3.8)])
        assert must == [(2, 3)] and may == want, (gap, must, may)


def test_a_triangle_about_a_tile_corner_lies_in_four_tiles():
    must, may, k = lists([at(2.8, 2.8), at(3.3, 2.9), at(2.9, 3.3)])
    assert must == [(2, 2), (2, 3), (3, 2), (3, 3)] and may == must and k == rb.FEW


def test_a_sliver_of_overlap_counts():
    """a corner of the triangle reaches 1e-6 tile past the corner (3, 3) of tile (2, 2), one edge along the diagonal, the other at slope 1 / 2: beside
    tile (3, 3) it crosses y = 3 at x = 3 - 1e-6 and so holds 1e-6 x 5e-7 of tile (2, 3) as well — and nothing of tile (3, 2), which the diagonal edge
    only touches"""
    must, _, _ = lists([at(2.2, 2.2), at(3.0 + 1e-6, 3.0 + 1e-6), at(2.2, 2.6)])
    assert must == [(2, 2), (2, 3), (3, 3)]


def test_a_triangle_over_the_whole_grid_lies_in_all_64_tiles():
    must, may, k = lists([at(-10, -10), at(30, -10), at(-10, 30)])
    assert len(must) == 64 and may == must and k == rb.MANY


def test_a_triangle_behind_the_apex_lies_in_no_tile():
    must, may, k = lists([at(2.2, 3.2, -1.0), at(2.8, 3.3, -1.0), at(2.5, 3.8, -2.0)])
    assert must == [] and may == [] and k == rb.BEHIND


def test_a_triangle_across_the_apex_plane():
    """(-0.2, 0.1, 1), (0.2, 0.1, 1), (0, 0.1, -1).  Cut at the apex plane it is a quad whose two long edges run off to infinity: along the first, with
    u = 1 / Z >= 1, the image point is (3.6 - 0.4 u, 4 + 0.4 u), i.e. x = 7.6 - y, and by symmetry about x = 4 the other is x = 0.4 + y; the short edge
    is y = 4.4.  Row ty >= 4 is widest at its far side y = ty + 1: x from 6.6 - ty to 1.4 + ty, so rows 4 .. 7 hold tiles 2 .. 5, 1 .. 6, 0 .. 7, 0 .. 7: 26.
    may is the plane rule's product: the vertex behind the apex has the formal image point (4, 3.6) and stands on the OTHER side of every plane, so no
    column is missed, and the only row that all three vertices lie beyond the same plane of is row 3 (y = 4.4 twice beyond its far plane, 3.6 beyond
    it from behind): 7 rows x 8 columns."""
    must, may, k = lists([(-0.2, 0.1, 1.0), (0.2, 0.1, 1.0), (0.0, 0.1, -1.0)])
    want = [(tx, ty) for ty in range(4, 8) for tx in range(max(0, int(np.floor(6.6 - ty))), min(7, int(np.floor(1.4 + ty))) + 1)]
    assert len(want) == 26 and must == sorted(want)
    assert may == sorted((tx, ty) for ty in (0, 1, 2, 4, 5, 6, 7) for tx in range(8)) and set(must) <= set(may) and k == rb.UNTRUSTED


def test_a_triangle_seen_edge_on_is_a_line_of_tiles():
    """in the plane Y = 0.1 Z through the apex: image points (2.2, 4.4), (5.8, 4.4), (4, 4.4)"""
    must, may, k = lists([(-0.45, 0.1, 1.0), (0.45, 0.1, 1.0), (0.0, 0.2, 2.0)])
    assert must == [(2, 4), (3, 4), (4, 4), (5, 4)] and set(must) <= set(may) and k == rb.FEW
    # ... and one whose plane misses the apex by a hair is the same line
    must2, may2, _ = lists([(-0.45, 0.1, 1.0), (0.45, 0.1, 1.0), (0.0, 0.2 + 1e-9, 2.0)])
    assert must2 == must and set(must2) <= set(may2)


def test_a_triangle_beyond_a_side_plane_lies_in_no_tile():
    must, may, k = lists([at(9, 3), at(10, 4), at(9.5, 5)])
    assert must == [] and may == [] and k == rb.BEHIND
    # ... also when the projection is not trusted: two vertices beside the apex (Z small against X), all three beyond the right plane
    must, may, k = lists([(1.0, 0.0, 0.001), (1.0, 0.1, 0.001), (2.0, 0.0, 0.5)])
    assert must == [] and may == [] and k == rb.BEHIND


def test_a_degenerate_triangle_lies_in_no_tile_it_must():
    t = [at(2.2, 3.2), at(2.2, 3.2), at(2.8, 3.3)]
    assert lists(t)[0] == []


def test_the_grids_are_the_ones_the_stage_scenes_state():
    """grids_of (from the scene description's matrices, as the library derives them) against stage_scenes.tile_grids (from the scene's own sensors):
    the tile coordinates of points in front of each apex agree to 1e-4 tile, and so do the tile counts"""
    for sc in (ss.side_lit(), ss.facing(cutoff=20.0)):
        sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
        for g, (name, to_world, to_tiles, nx, ny) in zip(rb.grids_of(sd), ss.tile_grids(sc)):
            assert (g.name, g.nx, g.ny) == (name, nx, ny)
            pl = np.random.default_rng(0).uniform(-1, 1, (50, 3)) * (1.0, 1.0, 0.0) + (0.0, 0.0, 3.0)
            tw = np.asarray(to_world, np.float64).reshape(4, 4)
            P = g.homog(pl @ tw[:3, :3].T + tw[:3, 3])
            np.testing.assert_allclose(P[:, :2] / P[:, 2:], to_tiles(pl), atol=1e-4)
    sd = scene_desc.scene_desc(ss.side_lit(), tex_channels=1, shadows=bc.SHADOWS_PLAIN)
    assert rb.grids_of(sd)[2].nx == 42 and rb.grids_of(sd, tile=4)[0].nx == 24 and rb.grids_of(sd, tile_proj=4)[1].ny == 6
    assert rb.spot_grid_n(3.0) == 8 and rb.spot_grid_n(74.0) == 128 and rb.SHADOW_EPS == pytest.approx(8.94e-4, rel=1e-3) and rb.PAD == 1 / 256


# ----------------------------------------------------------------------------- (ii) the scenes
def _case(name):
    mk, env, spp, shadows, (seed, frame) = bc.CASES[name]
    sc = mk()
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows)
    return sc, sd, rb.grids_of(sd, **bc.knobs(env)), bc.posed_tris(sc, seed, frame)


@pytest.mark.parametrize("case", sorted(ss.CASES))
def test_must_lies_inside_may_on_every_stage_scene(case):
    sc, _ = ss.build(case, 64, 48)
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    tris = ss.world_tris(sc)
    for g in rb.grids_of(sd):
        if g is not None:
            must, may = rb.must_list(g, tris), rb.may_list(g, tris)
            print(f"{case} {g.name} {g.nx} x {g.ny}: must {len(must)} may {len(may)}")
            assert must <= may, (case, g.name, len(must - may))


def test_the_gpu_cases_populate_every_class_orientation_and_entry_kind():
    """over the (case, apex) pairs of tests/test_bins_gpu.py: each of the four classes on at least one of them (in fact all four together on the spot
    grid of facing_74_n32), and within every case trusted projections of both orientations; slivers (box-only entries: the two-vertex triangles at a sphere's poles) and untrusted triangles
    (always-pass entries) that reach a grid on at least one; must <= may on all; and the lists fit the capacity 2 F + 16 384 with room for the float32
    kernel's own choices (may is an upper bound of what it lists)"""
    seen = np.zeros(4, int)
    kinds = {"sliver": 0, "untrusted": 0}
    for name in bc.CASES:
        sc, sd, grids, tris = _case(name)
        cw = ccw = 0
        for g in grids:
            if g is None:
                continue
            k = rb.klass(g, tris)
            hist = np.bincount(k, minlength=4)
            seen += hist > 0
            must, may = rb.must_list(g, tris), rb.may_list(g, tris)
            assert must <= may and len(may) <= 2 * len(tris) + rb.MAX_TILES, (name, g.name, len(must), len(may))
            _, area2, scale = rb.projection(g, tris)
            reach, listable = np.zeros(len(tris), bool), np.zeros(len(tris), bool)
            reach[np.unique(np.fromiter(must, np.int64, len(must)) // (g.nx * g.ny))] = True
            listable[np.unique(np.fromiter(may, np.int64, len(may)) // (g.nx * g.ny))] = True
            with np.errstate(invalid="ignore"):
                ccw += int((reach & (area2 > 2 * rb.SLIVER * scale)).sum())
                cw += int((reach & (area2 < -2 * rb.SLIVER * scale)).sum())
                kinds["sliver"] += int((listable & (k != rb.UNTRUSTED) & (np.abs(area2) < 0.5 * rb.SLIVER * scale)).sum())
            kinds["untrusted"] += int((reach & (k == rb.UNTRUSTED)).sum())
            print(f"{name} {g.name} {g.nx} x {g.ny}: classes {dict(zip(rb.CLASS_NAMES, hist.tolist()))} must {len(must)} may {len(may)}")
        assert cw > 0 and ccw > 0, (name, cw, ccw)
    assert (seen > 0).all(), dict(zip(rb.CLASS_NAMES, seen.tolist()))
    assert kinds["sliver"] > 0 and kinds["untrusted"] > 0, kinds
    sc, sd, grids, tris = _case("facing_74_n32")
    assert (np.bincount(rb.klass(grids[2], tris), minlength=4) > 0).all()


# ----------------------------------------------------------------------------- (iii) the checks on right and wrong structures
@pytest.fixture(scope="module")
def right():
    """facing_74_n32's spot grid (all four classes) with lists, entries and an envelope built from the reference"""
    sc, sd, grids, tris = _case("facing_74_n32")
    g = grids[2]
    return g, tris, rb.build_lists(g, tris), rb.build_envelope(g, tris)


def _all_checks(g, tris, hdr, starts, cursors, en):
    fig, bad, _ = rb.check_lists(g, tris, hdr, starts, cursors, en, 2 * len(tris) + rb.MAX_TILES)
    return bad + rb.check_entries(g, tris, en)[1] + rb.check_reader(g, tris, starts, en)[1]


def test_the_checks_accept_lists_built_from_the_reference(right):
    g, tris, (hdr, starts, cursors, en), _ = right
    assert _all_checks(g, tris, hdr, starts, cursors, en) == []
    fig, bad = rb.check_entries(g, tris, en)
    assert min(fig.values()) > 0, fig  # (every kind of entry, both orientations)


def _mutations():
    def hole(h, s, c, e, tris, g):  # an entry of a pair the rays need becomes a second copy of its neighbour
        nt = g.nx * g.ny
        tile = np.repeat(np.arange(nt), np.diff(s.astype(np.int64)))
        must = rb.must_list(g, tris)
        i = next(i for i in range(1, len(e)) if tile[i] == tile[i - 1] and rb.pair_key(g, e["slot"][i], tile[i]) in must)
        e[i] = e[i - 1]

    def shifted(h, s, c, e, tris, g):  # a cursor left at one: the next fill lands one entry further, in the neighbouring tile's list
        t = int(np.nonzero(np.diff(s.astype(np.int64)) > 0)[0][3])
        c[t] = 1

    def sign(h, s, c, e, tris, g):  # the orientation taken as +1 for every triangle
        _, area2, _ = rb.projection(g, tris)
        n = e["e"].reshape(-1, 3, 3).copy()
        w = (area2[e["slot"]] < 0) & np.isfinite(e["bb"]).all(1) & (n[:, 0, :2] != 0).any(1)
        padded = rb.PAD * (np.abs(n[w, :, 0]) + np.abs(n[w, :, 1]))
        n[w, :, :2] *= -1
        n[w, :, 2] = -(n[w, :, 2] - padded) + padded
        e["e"] = n.reshape(-1, 9)
        assert w.any()

    def no_pad(h, s, c, e, tris, g):  # edge offsets without their pad
        n = e["e"].reshape(-1, 3, 3)
        w = np.isfinite(e["bb"]).all(1) & (n[:, 0, 0] != 0)
        n[w, :, 2] -= rb.PAD * (np.abs(n[w, :, 0]) + np.abs(n[w, :, 1]))
        e["e"] = n.reshape(-1, 9)

    def short_row(h, s, c, e, tris, g):  # the last tile row of one many-tile triangle is not listed (slots renamed to a triangle listed there anyway)
        nt = g.nx * g.ny
        tile = np.repeat(np.arange(nt), np.diff(s.astype(np.int64)))
        many = np.nonzero(rb.klass(g, tris) == rb.MANY)[0]
        must = rb.must_list(g, tris)
        for m in many:
            rows = tile[e["slot"] == m] // g.nx
            last = (e["slot"] == m) & (tile // g.nx == rows.max())
            if any(rb.pair_key(g, m, t) in must for t in tile[last]):
                e["slot"][last] = -1
                return
        raise AssertionError("no many-tile triangle")

    def total(h, s, c, e, tris, g):  # a scan that loses a row's carry: the last start is not the total
        s[-1] -= 1

    # the scan of a row of 64 tiles without the step that carries lanes 0 .. 31 into lanes 32 .. 63 (row_bcast:31).  Pinned here and not on the device: starts that
    # decrease make k_bin_env form a list length by unsigned wrap-around, so a library built that way reads far outside the entries
    def scan_carry(h, s, c, e, tris, g):
        n = np.diff(s.astype(np.int64))
        run, out = 0, []
        for r in range(0, len(n), 64):
            row = n[r: r + 64]
            incl = np.cumsum(row)
            incl[32:] -= incl[31]
            out.extend((run + incl - row).tolist())
            run += int(incl[-1])
        s[:-1], s[-1], h[1] = np.asarray(out, np.uint32), run, run

    def untrusted_as_box(h, s, c, e, tris, g):  # an always-pass entry written with a finite box
        w = np.nonzero(np.isinf(e["bb"]).any(1))[0][0]
        e["bb"][w] = (0, 0, 1, 1)

    return {"hole + duplicate": hole, "cursor left at one": shifted, "orientation fixed": sign, "no pad on the edges": no_pad, "a tile row short": short_row,
            "total": total, "scan without a carry": scan_carry, "always-pass entry with a box": untrusted_as_box}


@pytest.mark.parametrize("what", sorted(_mutations()))
def test_the_checks_name_a_wrong_list(right, what):
    g, tris, (hdr, starts, cursors, en), _ = right
    hdr, starts, cursors, en = hdr.copy(), starts.copy(), cursors.copy(), en.copy()
    _mutations()[what](hdr, starts, cursors, en, tris, g)
    bad = _all_checks(g, tris, hdr, starts, cursors, en)
    print(what, bad)
    assert bad, what


def test_the_envelope_check_on_one_cell():
    """one triangle across cell (3, 3) .. of tile (4, 4), facing the apex at depth 2: the plane of constant depth 2 (1 - SHADOW_EPS) passes when it is
    pulled forward by 1e-6 and fails when it is pushed back by 1e-6; a zero cell under the triangle fails; a cell beside it must be zero or in front"""
    tris = np.asarray([[at(4.30, 4.30), at(4.60, 4.32), at(4.40, 4.62)]], np.float64)
    cx, cy = int(4.43 * rb.ENV_SUB), int(4.41 * rb.ENV_SUB)  # a cell the triangle covers
    front = rb.build_envelope(G, tris, factor=(1.0 - rb.SHADOW_EPS) * (1.0 + 1e-6))
    fig, bad = rb.check_envelope(G, tris, front)
    assert bad == [] and fig["worst"] == pytest.approx(1.0 / ((1.0 - rb.SHADOW_EPS) * (1.0 + 1e-6)), rel=1e-6) and front[cy, cx, 2] > 0, (fig, bad)
    assert 0 < fig["finite"] < 0.01 and fig["nan"] == 0
    behind = rb.build_envelope(G, tris, factor=(1.0 - rb.SHADOW_EPS) * (1.0 - 1e-6))
    fig, bad = rb.check_envelope(G, tris, behind)
    assert len(bad) == 1 and "behind the triangle" in bad[0], bad
    one = front.copy()
    one[cy, cx, :3] = behind[cy, cx, :3]  # a single cell a hair too far back
    assert len(rb.check_envelope(G, tris, one)[1]) == 1
    one[cy, cx, :3] = 0.0
    assert "claim to be empty" in rb.check_envelope(G, tris, one)[1][0]
    one[cy, cx, :3] = -front[cy, cx, :3]
    assert "behind the emitter" in rb.check_envelope(G, tris, one)[1][0]
    # a plane tilted about the cell's middle column: (M[0] - xc M[2]) . d = x - xc for the ray d through (x, y), so this one falls back where x > xc
    xc = (cx + 0.5) / rb.ENV_SUB
    tilt = front.copy()
    tilt[cy, cx, :3] -= (1e-3 * float(np.abs(front[cy, cx, :3]).max()) * (G.M[0] - xc * G.M[2])).astype(np.float32)
    bad = rb.check_envelope(G, tris, tilt)[1]
    assert len(bad) == 1 and "behind the triangle" in bad[0], bad


def test_the_envelope_check_accepts_the_reference_and_wants_a_reason_for_nan(right):
    g, tris, (hdr, starts, cursors, en), cells = right
    fig, bad = rb.check_envelope(g, tris, cells)
    print(fig)
    assert bad == [] and fig["zero"] > 0 and fig["finite"] > 0.9
    # NaN needs a reason: none of the entries near this (well-lit, finite) cell is seen edge-on
    A = np.cross(tris[:, 2] - tris[:, 0], tris[:, 1] - tris[:, 0])
    T = ((tris[:, 2] - tris[:, 0]) * np.cross(g.o - tris[:, 0], tris[:, 1] - tris[:, 0])).sum(1)
    finite = np.argwhere((cells[..., :3] != 0).any(2))[::61]
    some = cells.copy()
    some[finite[:, 0], finite[:, 1], :3] = np.nan
    fig, bad = rb.check_envelope(g, tris, some, starts, en, (A, T))
    print(len(finite), fig)
    assert fig["n_nan"] == len(finite) and 0 < fig["unjustified"] < len(finite) and len(bad) == 1  # (cells beside a grazing triangle have a reason, the others are named)


def test_the_envelope_check_wants_the_ignored_tail_spent():
    """side_lit's spot sees the floor's two triangles across thousands of cells that nothing else comes near: there the kernel's plane is the
    triangle's own, moved by its stated margins, and s_env / s_j must reach 1 / ((1 - SHADOW_EPS)(1 + 6e-5)(1 + delta)).  A right envelope built with
    that factor passes; one built without the (1 - SHADOW_EPS) — safe, but every shadow packet near the floor would run its any-hit stage — is named"""
    sc, sd, grids, tris = _case("side_lit")
    g = grids[2]
    fig, bad = rb.check_envelope(g, tris, rb.build_envelope(g, tris))
    assert bad == [] and fig["lone"] > 1000, (fig, bad)
    fig, bad = rb.check_envelope(g, tris, rb.build_envelope(g, tris, factor=1.0 + 6e-5))
    assert len(bad) == 1 and "further in front" in bad[0] and fig["worst"] < 1.0, (fig, bad)
