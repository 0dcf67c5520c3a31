"""The tile-bin pre-pass read back from the blob and held to the float64 reference of tests/ref_bins.py (the reference on known answers, and the proof
that these poses populate every class: tests/test_bins_cpu.py).  k_bin<false>, k_bin_scan, k_bin<true> and k_bin_env (ffx_bins.hip) decide which triangles
a packet render looks at at all and which shadow packets skip their any-hit stage; the rest of the suite sees them through images, hits and headers,
which sample a tile at a few points per pixel.  Here, per pose and apex: the integers exactly, must <= listed <= may as sets of (slot, tile) pairs with
no exception on either side, every 64-byte entry against the float64 projection of its triangle, what a reader finds at points of every triangle, every
cell of both envelopes against every triangle of the scene, and what one blob holds after other poses and after a pose whose lists do not fit.
Run with `-m gpu`; every test prints its figures before it asserts (`-s`).

Observed on an MI355X — (slot, tile) pairs must / listed / may, triangles per class (behind, <= 16 tiles, > 16 tiles, not trusted):
  side_lit        camera 648 / 708 / 714 (2, 278, 2, 0)            projector 286 / 321 / 327 (2, 280, 0, 0)          spot 5 405 / 5 555 / 5 573 (0, 258, 24, 0)
  facing_20       camera 1 928 / 2 284 / 2 307 (598, 1 210, 0, 0)  projector 1 593 / 1 654 / 1 677 (452, 1 348, 0, 8)  spot 2 867 / 2 878 / 2 892 (1 698, 29, 81, 0)
  facing_74_n32   camera and projector as facing_20                                                                 spot 5 625 / 10 337 / 10 794 (644, 1 042, 114, 8)
  away            camera as facing_20                               projector 8 / 11 / 11 (1 801, 0, 0, 7)            spot 0 / 0 / 0 (1 805, 3, 0, 0)
  vocalfold_a     camera 4 808 / 4 869 / 4 945 (611, 3 229, 0, 0)  projector 2 269 / 2 294 / 2 307 (1 712, 2 128, 0, 0)  spot 22 574 / 22 710 / 22 869 (466, 2 869, 505, 0)
  vocalfold_b     camera 4 850 / 4 910 / 4 984 (606, 3 234, 0, 0)  projector 2 548 / 2 577 / 2 604 (1 452, 2 388, 0, 0)  spot 22 685 / 22 859 / 23 039 (458, 2 885, 497, 0)
  hello_world     camera 46 / 51 / 51 (0, 12, 0, 2)                                                                  spot 5 077 / 5 089 / 5 090 (0, 0, 14, 0)
  tile_4          camera 1 308 / 1 398 / 1 406 (2, 269, 11, 0)     projector 396 / 429 / 435 (2, 280, 0, 0)          spot as side_lit
  proj_tile_4     camera as side_lit                                projector 602 / 644 / 647 (2, 278, 2, 0)          spot as side_lit
  plain_16spp     camera and projector as side_lit                                                                  spot 2 379 / 2 473 / 2 487 (0, 260, 22, 0)
No exception on either side anywhere; 106 857 projected, 1 108 box-only and 5 155 always-pass entries.  Envelopes, shares of zero / finite / NaN cells and
the worst s_env / s_j over real overlaps (limit 1 / (1 - SHADOW_EPS) = 1.000 894 87; 1 / kap = 1.000 832 8 is what an exact plane would give):
  side_lit projector 0.16 / 0.67 / 0.17, 1.000 832 9; spot 0.30 / 0.70 / 0.004, 1.000 846 9      facing_20 projector 0 / 0.80 / 0.20, 1.000 832 8; spot 0 / 0.999 / 0.000 6, 1.000 835 5
  facing_74_n32 spot 0.018 / 0.56 / 0.42, 1.000 886 6 (the closest: 5.2e-5 of the kernel's 6e-5 spent)      away projector 0.67 / 0.33 / 0, 1.000 833 0; spot all zero
  vocalfold_a projector 0 / 0.98 / 0.02, 1.000 832 8; spot 0.007 / 0.992 / 0.001, 1.000 834 1      vocalfold_b projector 0.06 / 0.52 / 0.42, 0.998 3; spot 0.012 / 0.980 / 0.008, 1.000 835 9
  hello_world spot 0.12 / 0.88 / 0, 1.000 846 7      tile_4 projector 0.22 / 0.62 / 0.16, 1.000 832 9      proj_tile_4 projector 0.25 / 0.68 / 0.07, 1.000 833 1
Every NaN cell had its reason.  The module takes 12 s, its slowest test (vocalfold_b's spot envelope: 1.08 M candidate pairs) 2.5 s.
"""
import functools
import time

import numpy as np
import pytest
import torch

from fireflies_amd import ops, scene_desc, scenes
from tests import bin_cases as bc
from tests import ref_bins as rb
from tests.gpu_support import apex_records, bin_lists, dev, envelope, tri_records

pytestmark = pytest.mark.gpu

KNOBS = ("FFX_ENVELOPE", "FFX_BINS", "FFX_WIDE", "FFX_TRAVERSAL", "FFX_BIN_CAP", "FFX_BIN_TILE", "FFX_BIN_TILE_PROJ", "FFX_BIN_SPOT_N", "FFX_K8_PLAIN",
         "FFX_PIXELS_PER_WAVE", "FFX_ASYNC_UPDATE", "FFX_RENDER_BLOCKS")
APEX = ("camera", "projector", "spot")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _geometry(sc):
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    return ops.DeviceGeometry(pool, tris, shape, off), alb


def _texture(sc):
    if sc.projector is None:
        return None
    return dev(np.random.default_rng(3).random((sc.projector.height, sc.projector.width)).astype(np.float32))


def _prepass(gd, sd, alb, tex, spp, xf, offs):
    """a fresh pose and one render at the needed samples per pixel: the blob the next render reads then holds this pose's pre-pass"""
    gd.update(xf, offs)
    img = gd.render_fwd(sd, dev(alb), tex, spp, seed=3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(img).all())


def _read(gd, grids, with_envelopes=True):
    """-> {apex: (hdr, starts, cursors, entries)}, {emitter: (flag, cells)} as numpy copies"""
    lists, envs = {}, {}
    for a, g in enumerate(grids):
        if g is None:
            continue
        lists[a] = tuple(np.array(v) for v in bin_lists(gd, a, g.nx, g.ny))
        if a >= 1 and with_envelopes:
            flag, cells, _ = envelope(gd, a, g.nx * rb.ENV_SUB, g.ny * rb.ENV_SUB)
            envs[a] = (flag, np.array(cells))
    return lists, envs


@functools.lru_cache(maxsize=None)
def _state(case):
    """one case rendered once: (grids, triangles of the blob's own records, the three lists, both envelopes, the emitters' apex records)"""
    mk, env, spp, shadows, (seed, frame) = bc.CASES[case]
    sc = mk()
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        gd, alb = _geometry(sc)
        sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows)
        _prepass(gd, sd, alb, _texture(sc), spp, *bc.pose(sc, seed, frame))
        grids = rb.grids_of(sd, **bc.knobs(env))
        lists, envs = _read(gd, grids)
        apex = {a: np.array(apex_records(gd, a)) for a in envs}
        return grids, tri_records(gd), lists, envs, apex, int(gd.info.n_tris)


PAIRS = [(c, a) for c in bc.CASES for a in range(3) if not (c == "hello_world" and a == 1)]
ENVELOPES = [(c, a) for c, a in PAIRS if a >= 1]


def _say(what, fig, t0):
    print(f"BINS {what}: " + ", ".join(f"{k} {v:.9g}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()) + f"  [{time.time() - t0:.2f} s of reference]")


# ------------------------------------------------------------------ a. the lists, the entries and a reader's view
@pytest.mark.parametrize("case,a", PAIRS, ids=[f"{c}-{APEX[a]}" for c, a in PAIRS])
def test_lists_and_entries_meet_the_float64_reference(case, a):
    """per pose and apex — integers, exactly: ok = 1, cap = 2 F + 16 384, starts from 0, non-decreasing, ending in the header's total; every cursor back
    at zero; slots in [0, F), none twice in a tile, pad words zero.  Lists: must <= listed <= may, zero exceptions.  Entries: a trusted entry's box holds
    the float64 projection and exceeds it by at most 2 PAD a side, its edge functions are >= 0 at the triangle's projected vertices and centroid and < 0 at
    the centroid mirrored across each edge and pushed 4 PAD further; box-only and always-pass entries are exactly what ffx_common.h says.  A reader at the
    vertices and edge midpoints (1e-3 tile inwards) and the centroid of every triangle finds it in that tile's list and its entry passes traverse_bins' test."""
    grids, tris, lists, envs, apex, F = _state(case)
    g = grids[a]
    hdr, starts, cursors, entries = lists[a]
    t0 = time.time()
    fig, bad, _ = rb.check_lists(g, tris, hdr, starts, cursors, entries, 2 * F + rb.MAX_TILES)
    fig["classes"] = dict(zip(rb.CLASS_NAMES, fig["classes"]))
    fe, bad_e = rb.check_entries(g, tris, entries)
    fr, bad_r = rb.check_reader(g, tris, starts, entries)
    _say(f"{case} {APEX[a]} {g.nx} x {g.ny} F {F}", {**fig, **fe, **fr}, t0)
    assert not (bad + bad_e + bad_r), (case, APEX[a], bad + bad_e + bad_r)
    if bc.CASES[case][3] == bc.SHADOWS_PLAIN and a == 2:
        assert g.nx == rb.spot_grid_n(35.0, plain=True) < rb.spot_grid_n(35.0) and int(hdr[4]) == 0  # (the coarser grid, no envelope)


def test_every_case_lists_both_orientations_and_the_module_every_kind_of_entry():
    """what tests/test_bins_cpu.py proves of the reference, of the device's entries: in every case entries of both orientations as seen from an apex;
    over the module box-only and always-pass entries, and triangles of all four classes"""
    kinds, classes = np.zeros(3, int), np.zeros(4, int)
    for case in bc.CASES:
        grids, tris, lists, _, _, _ = _state(case)
        ccw = cw = 0
        for a, (hdr, starts, cursors, entries) in lists.items():
            fe, _ = rb.check_entries(grids[a], tris, entries)
            ccw, cw = ccw + fe["ccw"], cw + fe["cw"]
            kinds += (fe["normal"], fe["degenerate"], fe["untrusted"])
            classes += np.bincount(rb.klass(grids[a], tris), minlength=4)
        assert ccw > 0 and cw > 0, (case, ccw, cw)
    print("BINS entries (projected, box-only, always-pass)", kinds.tolist(), "classes", dict(zip(rb.CLASS_NAMES, classes.tolist())))
    assert (kinds > 0).all() and (classes > 0).all()


# ------------------------------------------------------------------ b. the envelopes
@pytest.mark.parametrize("case,a", ENVELOPES, ids=[f"{c}-{APEX[a]}" for c, a in ENVELOPES])
def test_envelopes_lie_in_front_of_every_triangle(case, a):
    """every cell of the emitter's envelope against every triangle of the scene (ref_bins.check_envelope): a finite cell's plane has N . d > 0 and
    s_j >= (1 - SHADOW_EPS) s_env over the whole part of every triangle inside the cell's pyramid — no exception, 1e-9 for the reference's own float64;
    a zero cell overlaps no triangle; a NaN cell has a listed triangle seen edge-on, from behind or with T = 0 at one of its vertices; and a cell that
    one triangle alone decides has its plane no further in front than kap (1 - SHADOW_EPS)(1 + 6e-5) and the kernel's rounding allowance put it.  Under the
    short-render hint the header says that no envelope was built."""
    grids, tris, lists, envs, apex, F = _state(case)
    g = grids[a]
    flag, cells = envs[a]
    hdr, starts, cursors, entries = lists[a]
    if bc.CASES[case][3] == bc.SHADOWS_PLAIN:
        assert flag == 0 and int(hdr[0]) == 1
        return
    assert flag == 1 and int(hdr[0]) == 1, (case, APEX[a], hdr[:5])
    t0 = time.time()
    fig, bad = rb.check_envelope(g, tris, cells, starts, entries, (apex[a]["A"], apex[a]["T"]))
    _say(f"{case} {APEX[a]} envelope {g.nx * rb.ENV_SUB} x {g.ny * rb.ENV_SUB} cells", fig, t0)
    assert not bad, (case, APEX[a], bad)
    if case == "side_lit":
        assert fig["lone"] > 0  # (the floor: cells that one triangle alone decides, where the plane must not lie further in front than the stated margins)


# ------------------------------------------------------------------ c. what a blob holds after other poses
def _snapshot(gd, grids):
    """per apex the lists as per-tile sets of slots (one sorted array of slot * tiles + tile) and the integers; per emitter the envelope's bits"""
    lists, envs = _read(gd, grids)
    out = {}
    for a, (hdr, starts, cursors, entries) in lists.items():
        nt = grids[a].nx * grids[a].ny
        keys = np.sort(entries["slot"].astype(np.int64) * nt + rb.entry_tiles(starts, len(entries), nt))
        assert int(hdr[0]) == 1 and not cursors.any() and len(np.unique(keys)) == len(keys), (APEX[a], hdr[:5], int(cursors.any()))
        out[a] = (keys, starts.copy(), hdr[:5].copy(), None if a == 0 else envs[a][1].view(np.uint32))
    return out


def _same(s0, s1, what):
    for a in s0:
        assert np.array_equal(s0[a][0], s1[a][0]) and np.array_equal(s0[a][1], s1[a][1]) and np.array_equal(s0[a][2], s1[a][2]), f"{what}: the {APEX[a]}'s lists differ"
        if a >= 1:
            assert int(s1[a][2][4]) == 1 and np.array_equal(s0[a][3], s1[a][3]), f"{what}: {int((s0[a][3] != s1[a][3]).sum())} words of the {APEX[a]}'s envelope differ"


def _two_poses():
    sc = bc.CASES["vocalfold_a"][0]()
    sd = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    return sc, sd, rb.grids_of(sd), bc.pose(sc, 7, 0), bc.pose(sc, 8, 1)


def test_one_blob_holds_the_same_lists_after_other_poses_and_after_an_overflow(monkeypatch):
    """ONE blob (FFX_ASYNC_UPDATE=0): pose A, pose B, pose A — A's lists as per-tile sets, its list starts and its envelope cells bit for bit are what they
    were the first time (the fill pass counts every cursor back down to zero; no launch clears them).  Then B with FFX_BIN_CAP=0: ok = 0, total > cap,
    every cursor zero (the scan clears them: no fill pass runs), the entries area still holds A's bytes; and A again: the same sets."""
    monkeypatch.setenv("FFX_ASYNC_UPDATE", "0")
    sc, sd, grids, A, B = _two_poses()
    gd, alb = _geometry(sc)
    assert len(gd._blobs) == 1
    tex = _texture(sc)
    _prepass(gd, sd, alb, tex, 64, *A)
    first = _snapshot(gd, grids)
    _prepass(gd, sd, alb, tex, 64, *B)
    other = _snapshot(gd, grids)
    assert any(not np.array_equal(first[a][0], other[a][0]) for a in first)  # (B is another pose)
    _prepass(gd, sd, alb, tex, 64, *A)
    _same(first, _snapshot(gd, grids), "A behind B")
    held = {a: np.array(bin_lists(gd, a, g.nx, g.ny)[3]) for a, g in enumerate(grids)}
    monkeypatch.setenv("FFX_BIN_CAP", "0")
    _prepass(gd, sd, alb, tex, 64, *B)
    for a, g in enumerate(grids):
        hdr, starts, cursors, entries = bin_lists(gd, a, g.nx, g.ny, n_entries=len(held[a]))
        print(f"BINS overflow {APEX[a]}: header {hdr[:5].tolist()}")
        assert int(hdr[0]) == 0 and int(hdr[1]) == int(other[a][2][1]) > int(hdr[2]) == 0 and int(hdr[4]) == 0, (APEX[a], hdr[:5])
        assert int(starts[g.nx * g.ny]) == int(hdr[1]) and not cursors.any(), (APEX[a], int((cursors != 0).sum()))
        assert np.array_equal(entries.view(np.uint8), held[a].view(np.uint8)), f"the {APEX[a]}'s entries area was written by a pose whose lists do not fit"
    monkeypatch.delenv("FFX_BIN_CAP")
    _prepass(gd, sd, alb, tex, 64, *A)
    _same(first, _snapshot(gd, grids), "A behind an overflowing B")


def test_alternating_blobs_hold_the_same_lists_for_the_same_pose():
    """the default double buffer: update() alternates between two blobs at 64 samples per pixel (four below 33).  A, B, A, A puts A into one blob
    twice and then into the blob that last held B; at 16 samples per pixel four more poses walk the ring of four.  Every A is the first A."""
    sc, sd, grids, A, B = _two_poses()
    gd, alb = _geometry(sc)
    assert len(gd._blobs) == 4
    tex = _texture(sc)
    _prepass(gd, sd, alb, tex, 64, *A)
    first, blob_a = _snapshot(gd, grids), gd._cur
    _prepass(gd, sd, alb, tex, 64, *B)
    assert gd._cur != blob_a
    _snapshot(gd, grids)
    _prepass(gd, sd, alb, tex, 64, *A)
    assert gd._cur == blob_a
    _same(first, _snapshot(gd, grids), "A, B, A")
    _prepass(gd, sd, alb, tex, 64, *A)
    assert gd._cur != blob_a
    _same(first, _snapshot(gd, grids), "A in the blob that held B")
    sd16 = scene_desc.scene_desc(sc, tex_channels=1, shadows=True)
    seen = set()
    for pose in (B, A, B, A, A):
        _prepass(gd, sd16, alb, tex, 16, *pose)
        seen.add(gd._cur)
        snap = _snapshot(gd, grids)
        if pose is A:
            _same(first, snap, f"A at 16 samples per pixel in blob {gd._cur}")
    assert len(seen) == 4
