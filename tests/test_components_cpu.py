"""Connected components without a device: include/ffx_labels.h against the Python ABI and the library's exports, the refusals of ffx_connected_components
(each before any launch), the numpy restatement tests/ref_components.py against scipy.ndimage on every mask of the suite, the dataset loop's acceptance
rule in closed form, and what the ops wrapper turns away."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fireflies_amd import _abi, _lib, ops
from tests import ref_components as rc
from tests.support import FFX_ERR_ARG, ROOT, c_compiler, header

LABELS_H = os.path.join(ROOT, "include", "ffx_labels.h")


def _symbols(text):
    return sorted(set(re.findall(r"\b(ffx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def test_the_second_header_the_python_table_and_the_library_agree():
    with open(LABELS_H) as f:
        mine = _symbols(f.read())
    assert mine == sorted(_abi.PROTOTYPES_NO_ORACLE) and mine
    assert not set(mine) & set(_symbols(header())) and not set(mine) & set(_abi.PROTOTYPES)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in mine:
        assert hasattr(lib, name), name
    api = _lib.api()  # Api.__init__ binds both tables
    assert api.lib.ffx_connected_components.argtypes == _abi.PROTOTYPES_NO_ORACLE["ffx_connected_components"][1]


def test_the_workspace_macro_and_its_python_mirror_agree(tmp_path):
    cc = c_compiler()
    assert cc is not None, "a C compiler is needed to evaluate the header's macro"
    cases = [(1, 1, 0), (1, 1, 1), (64, 64, 256), (512, 512, 3), (33, 65, 7), (4097, 1, 2), (32768, 32768, 1 << 20)]
    src = ['#include <stdio.h>', '#include "ffx_labels.h"', "int main(void) {"]
    src += [f'  printf("%zu\\n", FFX_COMPONENTS_WORKSPACE_BYTES({h}, {w}, {m}));' for h, w, m in cases]
    src += ["  return 0;", "}"]
    (tmp_path / "ws.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "ws.c"), "-o", str(tmp_path / "ws")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ws")]).split()]
    assert got == [_abi.components_workspace_bytes(*c) for c in cases]


# every refusal of DESIGN.md 4.11: (what changes against a valid call, the word its message must hold)
REFUSALS = {
    "img NULL": (dict(img=None), "img"),
    "n_labels NULL": (dict(n_labels=None), "n_labels"),
    "workspace NULL": (dict(workspace=None), "workspace"),
    "workspace misaligned": (dict(workspace="misaligned"), "workspace"),
    "elem_size 2": (dict(elem_size=2), "elem_size"),
    "elem_size 0": (dict(elem_size=0), "elem_size"),
    "h 0": (dict(h=0), "h "),
    "w 0": (dict(w=0), "w "),
    "h 32769": (dict(h=32769, w=1), "h "),
    "w 32769": (dict(h=1, w=32769), "w "),
    "h * w = 2^30 + 1": (dict(h=1, w=(1 << 30) + 1), "h * w"),
    "h * w = 2^30 + 2^15": (dict(h=32768, w=32769), "h * w"),
    "connectivity 6": (dict(connectivity=6), "connectivity"),
    "connectivity 0": (dict(connectivity=0), "connectivity"),
    "centroids without stats": (dict(stats=None), "centroids without stats"),
    "max_labels 0 with stats": (dict(max_labels=0), "max_labels"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_connected_components_refuses_before_any_launch(case):
    """dummy host pointers: a launch would fault on them — the call returns FFX_ERR_ARG first and names the parameter"""
    changes, word = REFUSALS[case]
    lib = _lib.api().lib
    buf = np.zeros(64, np.float32)
    addr = (buf.ctypes.data + 15) & ~15
    args = dict(img=addr, elem_size=1, h=4, w=4, background=0, connectivity=8, labels=addr, n_labels=addr, stats=addr, centroids=addr, max_labels=2,
                workspace=addr, stream=None)
    assert not set(changes) - set(args)
    args.update({k: addr + 4 if v == "misaligned" else v for k, v in changes.items()})
    rc_ = lib.ffx_connected_components(*args.values())
    msg = (lib.ffx_last_error() or b"").decode()
    assert rc_ == FFX_ERR_ARG, (case, rc_, msg)
    assert msg.startswith("connected_components: ") and word in msg, (case, msg)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(rc.MASKS))
def test_the_numpy_restatement_is_scipys_labelling(name, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    m = rc.mask(name)
    n, lab, st, cen = rc.expected(name, connectivity)
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    want, c = ndi.label(m, structure=structure)
    assert n == c + 1 and np.array_equal(lab, want)
    rows = min(n, 256)
    for k, sl in enumerate(ndi.find_objects(want)[: rows - 1], start=1):
        assert tuple(st[k]) == (sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start, int((want == k).sum())), (name, k)
    if rows > 1:
        com = np.asarray(ndi.center_of_mass(m, want, list(range(1, rows))))
        assert np.abs(cen[1:rows] - com[:, ::-1]).max() <= 1e-12
    # the background's row, and the rows behind the last component
    bg = ~m
    if bg.any():
        ys, xs = np.nonzero(bg)
        assert tuple(st[0]) == (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1, bg.sum())
        assert np.abs(cen[0] - (xs.mean(), ys.mean())).max() <= 1e-12
    else:
        assert not st[0].any() and np.isnan(cen[0]).all()
    assert not st[rows:].any() and np.isnan(cen[rows:]).all()


def test_the_counts_the_suite_relies_on():
    assert rc.expected("checkerboard-64", 8)[0] == 2 and rc.expected("checkerboard-64", 4)[0] == 2049
    # sparse masks at 4-connectivity hold more components than the 256 statistics rows, dense ones at 8-connectivity a single one
    assert rc.expected("random-96x80-0.3-seed0", 4)[0] == 1057 and rc.expected("random-33x65-0.3-seed0", 4)[0] == 293
    assert rc.expected("random-96x80-0.8-seed1", 8)[0] == 2 and rc.expected("random-33x65-0.8-seed3", 8)[0] == 2
    assert rc.expected("serpentine-130x67", 4)[0] == 2 and rc.expected("serpentine-130x67", 8)[0] == 2
    assert rc.expected("comb-96x80", 4)[0] == 2
    for name in ("diagonal", "anti-diagonal"):
        assert rc.expected(name, 8)[0] == 2 and rc.expected(name, 4)[0] == 81
    pairs = 11 * 9
    for name in ("corner-pairs", "corner-pairs-anti"):
        assert rc.expected(name, 8)[0] == pairs + 1 and rc.expected(name, 4)[0] == 2 * pairs + 1
    assert rc.expected("rings", 8)[0] == 4 and rc.expected("rings", 4)[0] == 4


@pytest.mark.parametrize("case", sorted(rc.seg_cases()))
def test_the_acceptance_rule_in_closed_form(case):
    seg, n_labels, kept = rc.seg_cases()[case]
    assert rc.components(seg, 8, background=2)[0] == n_labels
    assert rc.accept(seg) is kept
    assert kept == (seg.max() != 0 and n_labels <= 3)


def test_the_wrapper_turns_away_what_it_cannot_label():
    good = torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.connected_components(good)
    with pytest.raises(TypeError, match="float32"):
        ops.connected_components(good.float())
    with pytest.raises(ValueError, match="2-D"):
        ops.connected_components(good.reshape(2, 4, 8))
    with pytest.raises(ValueError, match="contiguous"):
        ops.connected_components(torch.zeros((8, 16), dtype=torch.uint8)[:, ::2])
    with pytest.raises(ValueError, match="max_labels"):
        ops.connected_components(good, max_labels=0)
