"""The BSDF adjoint's ABI (include/ffx.h FFX_RENDER_GRAD_MATERIAL) without a GPU: the bit in the header and in _abi, its place among the
flags, the block size from the header's macro against _abi.material_floats, the column order, and the specular -> eta chain factor."""
import os
import subprocess

import numpy as np

from fireflies_amd import _abi, scenes
from tests.support import ROOT, c_compiler, define, header



def test_bit_in_header_and_abi_agree():
    assert define("FFX_RENDER_GRAD_MATERIAL") == _abi.RENDER_GRAD_MATERIAL == 0x20000
    assert define("FFX_RENDER_MATERIAL_COLS") == _abi.RENDER_MATERIAL_COLS == 11
    assert "FFX_RENDER_MATERIAL_FLOATS(sd)" in header()
    assert define("FFX_ABI_VERSION") == 11


def test_bit_is_clear_of_the_other_flags():
    m = _abi.RENDER_GRAD_MATERIAL
    assert m & (m - 1) == 0
    assert m & _abi.RENDER_GRAD_APPEARANCE == 0 and m & define("FFX_RENDER_GRAD_APPEARANCE") == 0
    assert m & _abi.RENDER_PATH_MASK == 0 and m & define("FFX_RENDER_PATH_MASK") == 0
    for name in ("FFX_RENDER_FP16", "FFX_RENDER_SPARSE_ADJOINT", "FFX_RENDER_APEX_READY", "FFX_RENDER_CACHE_ZEROED", "FFX_RENDER_CACHE_KEEP_DROPPED"):
        assert m & define(name) == 0, name
    for f in (_abi.RENDER_FP16, _abi.RENDER_SPARSE_ADJOINT, _abi.RENDER_APEX_READY, _abi.RENDER_CACHE_ZEROED, _abi.RENDER_CACHE_KEEP_DROPPED):
        assert m & f == 0, f
    for md in range(2, _abi.RENDER_MAX_DEPTH_LIMIT + 1):
        for rr in range(1, 16):
            assert _abi.render_path(md, rr) & m == 0


def test_block_size_macro_matches_the_helper(tmp_path):
    cc = c_compiler()
    assert cc is not None, "a C compiler is needed (the CPU oracle is built with one)"
    cases = [1, 2, 7, 64, 65, 255, 1000]
    lines = ['#include "ffx.h"', "#include <stdio.h>", "#include <string.h>", "int main(void) {", "  ffx_scene_desc sd;"]
    for n in cases:
        lines += ["  memset(&sd, 0, sizeof sd);", f"  sd.n_shapes = {n}; sd.n_base_tex = 2; sd.base_tex_h[0] = 3; sd.base_tex_w[0] = 5;",
                  '  printf("%zu\\n", (size_t)FFX_RENDER_MATERIAL_FLOATS(&sd));']
    lines += ["  return 0;", "}"]
    src = tmp_path / "mat.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "mat"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [_abi.material_floats(n) for n in cases] == [11 * n for n in cases]


def test_columns_follow_the_material_row():
    names = ["roughness", "anisotropic", "metallic", "spec_trans", "eta", "spec_tint", "sheen", "sheen_tint", "flatness", "clearcoat", "clearcoat_gloss"]
    assert [scenes.MAT_COLUMN[n] for n in names] == list(range(define("FFX_MAT_ROUGHNESS"), define("FFX_MAT_CLEARCOAT_GLOSS") + 1))
    for n in names:
        assert scenes.MAT_COLUMN[n] == define("FFX_MAT_" + n.upper())
    assert define("FFX_MAT_CLEARCOAT_GLOSS") - define("FFX_MAT_ROUGHNESS") + 1 == _abi.RENDER_MATERIAL_COLS


def _eta64(s):
    return 2.0 / (1.0 - np.sqrt(0.08 * s)) - 1.0


def test_specular_chain_matches_central_differences():
    for s in [1e-4, 1e-3, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0]:
        h = 1e-6 * s
        fd = (_eta64(s + h) - _eta64(s - h)) / (2 * h)
        assert abs(scenes.specular_to_eta_grad(s) - fd) <= 1e-6 * abs(fd), (s, scenes.specular_to_eta_grad(s), fd)


def test_specular_chain_at_zero_is_the_finite_limit():
    g0 = scenes.specular_to_eta_grad(0.0)
    assert np.isfinite(g0)
    # the limit of (eta - 1) d eta / d specular as specular -> 0
    for s in (1e-8, 1e-10, 1e-12):
        assert abs((_eta64(s) - 1.0) * scenes.specular_to_eta_grad(s) - g0) <= 1e-4 * g0
    assert scenes.specular_to_eta(0.0) == 1.0
