"""ffx_connected_components on the device against tests/ref_components.py: every comparison is exact — torch.equal on n_labels, labels
and stats, the centroids bit for bit against sx / area in numpy float64 (NaN where the reference has NaN)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import fireflies_amd as ff
from fireflies_amd import _abi, _lib, ops, workloads
from fireflies_amd.graphics import components as gc
from tests import ref_components as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))  # (a copy: the shared masks are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def same(got, want, what, rows=None):
    """a Components against the reference's four outputs; `rows`: compare that many statistics rows only"""
    n, lab, st, cen = want
    assert int(got.n_labels) == n, (what, int(got.n_labels), n)
    assert got.n_labels.dtype == torch.int32 and got.n_labels.dim() == 0
    if got.labels is not None:
        assert got.labels.dtype == torch.int32 and torch.equal(got.labels.cpu(), torch.from_numpy(np.array(lab))), what
    if got.stats is not None:
        rows = len(st) if rows is None else rows
        assert got.stats.dtype == torch.int32 and torch.equal(got.stats.cpu()[:rows], torch.from_numpy(np.array(st[:rows]))), what
        g, c = got.centroids.cpu().numpy()[:rows], np.asarray(cen[:rows])
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(c)), what
        assert np.array_equal(g[~np.isnan(c)].view(np.int64), c[~np.isnan(c)].view(np.int64)), what


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(rc.MASKS))
def test_every_mask_against_the_reference(name, connectivity):
    same(ops.connected_components(dev(rc.mask(name)), connectivity), rc.expected(name, connectivity), name)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw(img, connectivity, background, max_labels, labels, n_labels, stats, centroids, workspace):
    """the C entry point on the caller's buffers, on the current stream"""
    _lib.api().call("ffx_connected_components", _ptr(img), img.element_size(), img.shape[0], img.shape[1], background, connectivity, _ptr(labels), _ptr(n_labels),
                    _ptr(stats), _ptr(centroids), max_labels, _ptr(workspace), ops._stream())


def buffers(h, w, max_labels, guard=0, fill=0x7F):
    """outputs filled with a byte pattern (the centroids with NaN), `guard` extra rows behind stats and centroids, and a workspace of garbage"""
    lab = torch.full((h, w), fill * 0x01010101, dtype=torch.int32, device=DEV)
    n = torch.full((1,), fill * 0x01010101, dtype=torch.int32, device=DEV)
    st = torch.full((max_labels + guard, 5), fill * 0x01010101, dtype=torch.int32, device=DEV)
    cen = torch.full((max_labels + guard, 2), float("nan"), dtype=torch.float64, device=DEV)
    if guard:
        cen[max_labels:] = 12345.678
    g = torch.Generator(device=DEV).manual_seed(h * 131 + w)
    ws = torch.randint(0, 256, (_abi.components_workspace_bytes(h, w, max_labels),), dtype=torch.uint8, device=DEV, generator=g)
    return lab, n, st, cen, ws


def test_more_components_than_rows_loses_only_the_rows_that_do_not_fit():
    """the 64 x 64 checkerboard at 4-connectivity: 2 048 components for 256 rows; guard rows behind both tables keep their pattern"""
    m = dev(rc.mask("checkerboard-64"))
    want = rc.expected("checkerboard-64", 4)
    assert want[0] == 2049
    lab, n, st, cen, ws = buffers(64, 64, 256, guard=64)
    raw(m, 4, 0, 256, lab, n, st, cen, ws)
    same(ops.Components(n[0], lab, st[:256], cen[:256]), want, "checkerboard")
    assert bool((st[256:] == 0x7F7F7F7F).all()) and bool((cen[256:] == 12345.678).all())
    same(ops.connected_components(m, 4, max_labels=3000), rc.expected("checkerboard-64", 4, 3000), "checkerboard, every row")
    same(ops.connected_components(m, 4, max_labels=1), rc.expected("checkerboard-64", 4, 1), "checkerboard, one row")


@pytest.mark.parametrize("name", ["random-33x65-0.593-seed2", "rings", "full-1x1", "empty-130x67"])
def test_prefilled_outputs_and_a_garbage_workspace(name):
    """every output word is written, the rows behind n_labels included; what the workspace held does not matter, the state of a call on a larger image
    included; two calls give the same bytes"""
    m = dev(rc.mask(name))
    h, w = m.shape
    want = rc.expected(name, 8)
    outs = []
    for fill in (0x7F, 0x00):
        lab, n, st, cen, ws = buffers(h, w, 256, fill=fill)
        raw(m, 8, 0, 256, lab, n, st, cen, ws)
        same(ops.Components(n[0], lab, st, cen), want, name)
        outs.append((lab, n, st, cen))
    big = dev(rc.mask("random-96x80-0.5-seed1"))
    ws = torch.empty(_abi.components_workspace_bytes(130, 130, 256), dtype=torch.uint8, device=DEV)
    same(ops.connected_components(big, 8, workspace=ws), rc.expected("random-96x80-0.5-seed1", 8), "the larger image")
    again = ops.connected_components(m, 8, workspace=ws)
    same(again, want, name + " behind a larger image")
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(again.centroids.view(torch.uint8), outs[0][3].view(torch.uint8))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_element_sizes_and_backgrounds_give_one_answer(connectivity):
    name = "random-96x80-0.593-seed0"
    m, want = rc.mask(name), rc.expected(name, connectivity)
    for what, img, bg in (("bool", dev(m), 0), ("uint8", dev(m, torch.uint8), 0), ("int32", dev(m, torch.int32), 0), ("int64", dev(m, torch.int64), 0),
                          ("uint8 on 2", dev(np.where(m, 200, 2), torch.uint8), 2), ("int32 on 2", dev(np.where(m, -1, 2), torch.int32), 2),
                          ("int64 on -3", dev(np.where(m, 1 << 40, -3), torch.int64), -3), ("int32 on -3", dev(np.where(m, 0, -3), torch.int32), -3),
                          ("int64 on 2^40", dev(np.where(m, 0, 1 << 40), torch.int64), 1 << 40)):
        same(ops.connected_components(img, connectivity, background=bg), want, what)
    # a 1-byte pixel is zero-extended: no pixel equals a background outside 0..255
    full = rc.components(np.ones_like(m), connectivity)
    for bg in (-1, 256, 1 << 40):
        same(ops.connected_components(dev(m, torch.uint8), connectivity, background=bg), full, f"uint8 on {bg}")


@pytest.mark.parametrize("name", ["random-96x80-0.3-seed0", "serpentine-130x67"])
def test_outputs_that_are_not_asked_for(name):
    m, want = dev(rc.mask(name)), rc.expected(name, 4)
    for labels in (True, False):
        for stats in (True, False):
            got = ops.connected_components(m, 4, labels=labels, stats=stats)
            assert (got.labels is not None) == labels and (got.stats is not None) == stats and (got.centroids is not None) == stats
            same(got, want, (name, labels, stats))
    n, lab = gc.connected_components(m, 4)
    same(ops.Components(n, lab), want, name)
    same(ops.Components(*gc.connected_components_with_stats(m, 4)), want, name)


def test_a_dependent_op_on_a_side_stream_sees_the_result():
    name = "random-96x80-0.5-seed2"
    m, want = dev(rc.mask(name)), rc.expected(name, 8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.connected_components(m, 8)
        total = got.labels.to(torch.int64).sum() + got.stats[:, 4].to(torch.int64).sum() * 1000 + got.n_labels  # no synchronise in between
    side.synchronize()
    assert int(total) == int(want[1].astype(np.int64).sum()) + int(want[2][:, 4].astype(np.int64).sum()) * 1000 + want[0]
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("case", sorted(rc.seg_cases()))
def test_accept_segmentation_in_closed_form(case):
    seg, n_labels, kept = rc.seg_cases()[case]
    flag = gc.accept_segmentation(dev(seg))
    assert flag.dtype == torch.bool and flag.dim() == 0 and flag.is_cuda and bool(flag) is kept
    assert int(ops.connected_components(dev(seg), 8, background=2, labels=False, stats=False).n_labels) == n_labels
    assert bool(ff.graphics.accept_segmentation(dev(seg, torch.int32))) is kept


def _pose(wl, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    wl.ff_scene.randomize()
    return ff.graphics.depth.get_segmentation_from_camera(wl.mi_scene)


def test_accept_segmentation_on_the_reduced_vocal_fold():
    wl = workloads.vocalfold(device=DEV, width=64, height=64, tex=96, grid=6, frames=5, n_fold=20, tube=(20, 24))
    for seed in range(8):
        seg = _pose(wl, seed)
        flag = gc.accept_segmentation(seg)
        host = seg.cpu().numpy()
        print(f"seed {seed}: labels {np.unique(host).tolist()}, n_labels {rc.components(host, 8, background=2)[0]}, kept {bool(flag)}")
        assert bool(flag) is rc.accept(host), seed


def test_the_full_size_vocal_fold_segmentation():
    wl = workloads.vocalfold(device=DEV)
    seg = _pose(wl, 3)
    assert tuple(seg.shape) == (512, 512)
    host = seg.cpu().numpy()
    got = ops.Components(*gc.connected_components_with_stats(seg != 2))
    try:
        from scipy import ndimage as ndi
    except ImportError:
        want = rc.components(host != 2, 8)
    else:
        lab, c = ndi.label(host != 2, structure=np.ones((3, 3), int))
        want = (c + 1, lab.astype(np.int32)) + rc.stats(lab.astype(np.int32), c + 1, 256)
    print(f"512 x 512 vocal fold: n_labels {want[0]}, areas {want[2][:want[0], 4].tolist()}")
    same(got, want, "512 x 512")
    assert bool(gc.accept_segmentation(seg)) is rc.accept(host)
