"""What ffx_scene_update / ffx_scene_update_h / ffx_scene_refit_top (fireflies_amd/csrc/ffx_scene.hip) leave in the BVH blob, read back and held to the
float64 statement of the pose in tests/ref_refit.py: the records, the per-slot geometric normals and their tag word, the per-slot vertex normals, the
per-triangle boxes, the binary nodes' and the wide overlay's child boxes — and that nothing else of the blob changes.  The reference on its own blob
and on every wrong one: tests/test_refit_cpu.py; the cases, the poses and the vertex normals' tolerance (from the oracle, not from here):
tests/refit_cases.py.  Every pose of a case goes into the SAME geometry in sequence, so a box has to grow and to shrink back.
Run with `-m gpu`; the figures are printed before they are asserted (`-s`).

Observed on an MI355X (the same under host and device tables, every FFX_REFIT form, every treelet size, one blob or four): no finding anywhere.
Records: v0 at most 0.44 B, edges at most 0.37 of their bound (two_shapes, `far`).  Geometric normals at most 1.4e-7 from the record's own cross
product (atol 3e-6), the vocal fold behind the native step included.  Vertex normals, largest deviation from float64 per pose in the order of
refit_cases.POSE_NAMES, device / oracle (the bound is four times the oracle's figure as tabulated):
  leaf4        5.1e-8 / 2.0e-8   5.0e-8 / 5.0e-8   5.0e-8 / 5.0e-8   3.2e-8 / 4.6e-8   4.9e-8 / 7.0e-8   0 / 0   4.4e-8 / 4.4e-8   3.9e-8 / 3.9e-8
  cluster65    1.4e-7 / 1.4e-7   4.9e-7 / 4.9e-7   2.4e-7 / 2.5e-7   1.0e-7 / 1.1e-7   1.2e-5 / 1.2e-5   0 / 0   1.5e-7 / 1.5e-7   3.3e-7 / 3.6e-7
  two_shapes   6.0e-7 / 6.0e-7   8.3e-7 / 8.3e-7   9.1e-7 / 9.1e-7   3.9e-7 / 3.9e-7   1.0e-4 / 1.0e-4   4.5e-7 / 4.5e-7   7.2e-7 / 7.2e-7   5.5e-7 / 5.4e-7
  degenerate   as two_shapes (its extra faces add nothing, and the three vertices only they touch hold exact zeros)
The closest to its bound is leaf4 at identity (0.64 of it): the oracle's normal of that flat patch happens to be rounded correctly, the device's is
one ulp of a component off.  A build with the triangle boxes' pad doubled, two normal rows of a slot swapped and one axis of the inner union dropped
fails all 28 tests of this module (the first findings of each: tq.tight and vn.row).  The module takes 4 s.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, mi, ops, workloads
from tests import ref_refit as rr
from tests import refit_cases as rc
from tests.gpu_support import DEV, blob_host

pytestmark = pytest.mark.gpu

KNOBS = ("FFX_REFIT", "FFX_TREELET_TRIS", "FFX_ASYNC_UPDATE", "FFX_DEFER_TOP", "FFX_WIDE_BUILD", "FFX_NATIVE_UPDATE", "FFX_NATIVE_RANDOMIZE")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def entry_points(monkeypatch):
    """the names of the library calls made through the bindings, in order"""
    names, real = [], _abi.Api.call

    def recording(self, name, *a):
        names.append(name)
        return real(self, name, *a)

    monkeypatch.setattr(_abi.Api, "call", recording)
    return names


def _run(name, tables="host", check=True):
    """the case's poses in sequence through one DeviceGeometry under the environment of the caller -> the host copies of the blob after each pose.
    tables: "host" (numpy transforms: ffx_scene_update_h up to 32 shapes) or "device" (a CUDA tensor: ffx_scene_update)"""
    c = rc.case(name)
    built = rc.host_build(c)  # (the same builder, inputs and environment as the constructor below: the update may change none of its topology)
    gd = ops.DeviceGeometry(c.pool, c.tris, c.tri_shape, c.off, smooth=c.smooth)
    gd._last_spp = 8  # (the ring of an asynchronous geometry then takes in all four copies)
    assert bytes(built[1]) == bytes(gd.info)
    blobs, used = [], set()
    for p in rc.poses(c):
        gd.update(torch.from_numpy(p.xforms).to(DEV) if tables == "device" else p.xforms, p.vert_off)
        used.add(gd._cur)
        blob = blob_host(gd)
        blobs.append(blob)
        if check:
            stats = {}
            found = rr.check_blob(blob, gd.info, built[0], c, p, c.smooth, stats)
            print(f"{name:13s} {p.name:10s} {tables:6s} copy {gd._cur}: v0 {stats['rec_v0_over_B']:.2f} B, e {stats['rec_e_over_bound']:.2f} of its bound, geometric normals "
                  f"{stats.get('gn_dev', 0.0):.2e} [{rr.GN_ATOL:g}], vertex normals {stats.get('vn_dev', float('nan')):.3e} [{c.vn_bound(p) if any(c.smooth) else float('nan'):.3e}], "
                  f"{stats['wide_children']} wide children; {len(found)} findings")
            assert found == [], (name, p.name, tables, found[:6])
            assert stats.get("gn_not_firm", 0) == 0
    assert used == (set(range(4)) if gd._async else {0})  # every copy has been the target, and was checked when it was
    return blobs, gd.info


@pytest.mark.parametrize("ring", ["ring", "single"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_the_blob_holds_the_pose_under_host_and_device_tables(name, ring, monkeypatch, entry_points):
    """every case and pose through the host-table and the device-table entry point, on the default ring of four blob copies and on a single blob
    (FFX_ASYNC_UPDATE=0); the two entry points leave the same bits in everything the update writes"""
    if ring == "single":
        monkeypatch.setenv("FFX_ASYNC_UPDATE", "0")
    h, info = _run(name, "host")
    n_poses = len(rc.POSE_NAMES)
    # host tables travel as kernel arguments up to 32 shapes; above, the device-table entry point serves them
    assert entry_points.count("ffx_scene_update" if rc.case(name).n_shapes > 32 else "ffx_scene_update_h") == n_poses + 1  # (+ the constructor's pose)
    del entry_points[:]
    d, _ = _run(name, "device")
    assert entry_points.count("ffx_scene_update") == n_poses + (rc.case(name).n_shapes > 32)
    for p, a, b in zip(rc.POSE_NAMES, h, d):
        assert np.array_equal(a, b), (name, p, np.nonzero(a != b)[0][:8], {f: int(getattr(info, f)) for f in ("off_recs", "off_wnodes", "off_tq", "off_plan", "off_nrec", "off_gn")})


@pytest.mark.parametrize("name", ["two_shapes", "degenerate", "cluster65"])
def test_the_three_refits_write_the_same_right_blob_with_a_smooth_shape(name, monkeypatch):
    """FFX_REFIT unset (treelets, then the top), `fused` (one launch) and `levels` (records, level by level, tail, wide boxes) with a shape that
    interpolates its normals: each is right, and the three agree bit for bit in all the update writes, off_nrec and off_gn included (but for the 64
    bytes of the overlay's header, which only the level launches write and nothing reads)"""
    assert any(rc.case(name).smooth)
    monkeypatch.setenv("FFX_ASYNC_UPDATE", "0")
    runs = {}
    for mode in (None, "fused", "levels"):
        if mode is None:
            monkeypatch.delenv("FFX_REFIT", raising=False)
        else:
            monkeypatch.setenv("FFX_REFIT", mode)
        runs[mode], info = _run(name)
    w0, w1 = int(info.off_whdr), int(info.off_whdr) + 64
    assert w1 <= int(info.off_plan)
    for mode in ("fused", "levels"):
        for p, a, b in zip(rc.POSE_NAMES, runs[None], runs[mode]):
            same = np.array_equal(a[:w0], b[:w0]) and np.array_equal(a[w1:], b[w1:])
            assert same, (name, mode, p, np.nonzero(a != b)[0][:8])


@pytest.mark.parametrize("treelet", ["4", "32"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_the_blob_holds_the_pose_under_small_treelets(name, treelet, monkeypatch):
    """FFX_TREELET_TRIS=4: treelets that are a bare leaf hanging off the top (slots, no node), and a top that holds most of the tree; 32: several levels
    on both sides of the cut"""
    monkeypatch.setenv("FFX_TREELET_TRIS", treelet)
    _, info = _run(name)
    if rc.case(name).n_tris > 64:
        assert info.n_treelets > (8 if treelet == "4" else 2)


def test_a_deferred_top_is_in_place_once_a_render_has_taken_the_blob(monkeypatch):
    """the native step (ffx_scene_step_h) behind 4-spp renders leaves the top of the tree to the first reader (FFX_DEFER_TOP=8): after a render has
    acquired the blob, everything tier B can say about it without knowing the pose holds — the top's boxes are the unions of what lies below them, the
    wide children mirror them, the triangle boxes enclose the records tightly, the tags follow the records, the topology is the builder's"""
    monkeypatch.setenv("FFX_DEFER_TOP", "8")
    built, tops = [], []
    real = _abi.Api.call

    def recording(self, name, *a):
        real(self, name, *a)
        if name == "ffx_bvh_build_host" and self.backend != "cpu-oracle":
            info = a[6]._obj
            built.append((np.frombuffer(C.string_at(a[4], int(info.off_bins)), np.uint8).copy(), info))
        if name == "ffx_scene_refit_top":
            tops.append(name)

    monkeypatch.setattr(_abi.Api, "call", recording)
    wl = workloads.vocalfold(device=DEV, width=64, height=56, tex=96, grid=6, frames=5, n_fold=20, tube=(20, 24))
    geom = wl.mi_scene.geom
    builder_blob = next(b for b, info in built if info is geom.info)
    torch.manual_seed(3)
    random.seed(3)
    for k in range(5):
        wl.ff_scene.randomize()
        img = mi.render(wl.mi_scene, spp=4, seed=100 + k).torch()
        blob = blob_host(geom)
        assert bool(torch.isfinite(img).all())
        stats = {}
        found = rr.check_blob(blob, geom.info, builder_blob, smooth=geom.smooth, stats=stats)
        print(f"step {k}: copy {geom._cur}, {len(tops)} deferred tops so far, geometric normals {stats['gn_dev']:.2e} [{rr.GN_ATOL:g}] "
              f"({stats['gn_not_firm']} slots with edges within 1e-3 of parallel), {stats['wide_children']} wide children; {len(found)} findings")
        assert found == [], found[:6]
        assert stats["gn_not_firm"] == 0  # (the vocal fold has no sliver: every geometric normal was held to 3e-6)
    assert wl.mi_scene.update_paths["native"] >= 4 and len(tops) >= 3, (dict(wl.mi_scene.update_paths), len(tops))
