"""The appearance adjoint's ABI (include/ffx.h FFX_RENDER_GRAD_APPEARANCE) without a GPU: the bit in the header and in _abi, its place
among the flags, and the size of the appearance block from the header's macro against _abi.appearance_floats."""
import os
import subprocess

import pytest

from fireflies_amd import _abi
from tests.support import ROOT, c_compiler, define, header



def test_bit_in_header_and_abi_agree():
    assert define("FFX_RENDER_GRAD_APPEARANCE") == _abi.RENDER_GRAD_APPEARANCE == 0x10000
    assert "FFX_RENDER_APPEARANCE_FLOATS(sd)" in header()


def test_bit_is_clear_of_the_other_flags():
    a = _abi.RENDER_GRAD_APPEARANCE
    assert a & (a - 1) == 0
    assert a & _abi.RENDER_PATH_MASK == 0 and a & define("FFX_RENDER_PATH_MASK") == 0
    others = [_abi.RENDER_FP16, _abi.RENDER_SPARSE_ADJOINT, _abi.RENDER_APEX_READY, _abi.RENDER_CACHE_ZEROED, _abi.RENDER_CACHE_KEEP_DROPPED]
    for name in ("FFX_RENDER_FP16", "FFX_RENDER_SPARSE_ADJOINT", "FFX_RENDER_APEX_READY", "FFX_RENDER_CACHE_ZEROED", "FFX_RENDER_CACHE_KEEP_DROPPED"):
        others.append(define(name))
    for f in others:
        assert a & f == 0, f
    # every depth the path integrator can carry stays clear of the bit
    for md in range(2, _abi.RENDER_MAX_DEPTH_LIMIT + 1):
        for rr in range(1, 16):
            assert _abi.render_path(md, rr) & a == 0


CASES = [(1, []), (4, [(8, 8)]), (7, [(16, 4), (3, 5)]), (2, [(1, 1), (2, 3), (4, 5)]), (12, [(64, 32), (7, 9), (1, 13), (128, 2)])]


def test_block_size_macro_matches_the_helper(tmp_path):
    cc = c_compiler()
    assert cc is not None, "a C compiler is needed (the CPU oracle is built with one)"
    lines = ['#include "ffx.h"', "#include <stdio.h>", "#include <string.h>", "int main(void) {", "  ffx_scene_desc sd;"]
    for n_shapes, bt in CASES:
        lines.append("  memset(&sd, 0, sizeof sd);")
        lines.append(f"  sd.n_shapes = {n_shapes}; sd.n_base_tex = {len(bt)};")
        for k, (h, w) in enumerate(bt):
            lines.append(f"  sd.base_tex_h[{k}] = {h}; sd.base_tex_w[{k}] = {w};")
        # (texture sizes beyond n_base_tex are not counted)
        for k in range(len(bt), 4):
            lines.append(f"  sd.base_tex_h[{k}] = 99; sd.base_tex_w[{k}] = 99;")
        lines.append('  printf("%zu\\n", (size_t)FFX_RENDER_APPEARANCE_FLOATS(&sd));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "app.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "app"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    want = [_abi.appearance_floats(n, bt) for n, bt in CASES]
    assert got == want


@pytest.mark.parametrize("n_tex", [0, 1, 2, 3, 4])
def test_block_layout_for_0_to_4_base_textures(n_tex):
    sizes = [(5, 7), (2, 3), (11, 1), (4, 4)][:n_tex]
    n = _abi.appearance_floats(9, sizes)
    assert n == 9 * 3 + 3 + 3 * sum(h * w for h, w in sizes)
    assert n_tex <= _abi.MAX_BASE_TEX
