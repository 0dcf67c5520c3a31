"""The pixel rectangles of the camera's tile bins as tables (fireflies_amd/csrc/ffx_rect.h): the plain-scene instance of the packet render kernel
reads a pixel's centre, box bounds and tile from them instead of forming them per pixel, so every entry must hold the bits the generic instance's
bins_primary / traverse_bins compute:  x0 = (float)px * its,  h = 0.5f * its - 0.25f * FFX_BIN_PAD,  c = x0 + h,  r0 = c - h,  r1 = c + h,  t = (int)x0.

The header is host code without HIP: a small program around it is compiled here with g++ (-ffp-contract=off, as the library) and prints the tables
as hexadecimal words; a float32 numpy restatement of the six expressions, one rounding per operation, must give the same words."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
FILMS = [(1, 1), (8, 8), (37, 29), (64, 48), (512, 512), (4096, 3)]
SIDES = [4, 8, 16]
PAD = np.float32(0.00390625)  # FFX_BIN_PAD

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "ffx_rect.h"
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]), side = atoi(argv[3]);
  const float its = 1.0f / (float)side;
  std::vector<FfxRectEntry> tab;
  float hx = -1.f, hy = -1.f;
  if (!ffx_rect_fill(W, H, its, its, tab, hx, hy)) { printf("refused\n"); return 0; }
  uint32_t w[2];
  memcpy(&w[0], &hx, 4); memcpy(&w[1], &hy, 4);
  printf("%zu %08x %08x\n", tab.size(), w[0], w[1]);
  for (const FfxRectEntry &e : tab) {
    uint32_t q[4];
    memcpy(q, &e, 16);
    printf("%08x %08x %08x %08x\n", q[0], q[1], q[2], q[3]);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program around ffx_rect.h"
    d = tmp_path_factory.mktemp("rect")
    (d / "rect_driver.cpp").write_text(DRIVER)
    exe = d / "rect_driver"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", str(REPO / "fireflies_amd" / "csrc"), str(d / "rect_driver.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def _tables(driver, W, H, side):
    out = subprocess.run([driver, str(W), str(H), str(side)], capture_output=True, text=True, check=True).stdout.split("\n")
    if out[0] == "refused":
        return None
    n, hx, hy = out[0].split()
    words = np.array([[int(x, 16) for x in l.split()] for l in out[1:1 + int(n)]], dtype=np.uint32)
    assert words.shape == (W + H, 4)
    return words, np.uint32(int(hx, 16)), np.uint32(int(hy, 16))


def _restated(n, side):
    """the six expressions for p = 0 .. n - 1 in float32, every operation rounded once (numpy float32 arithmetic) -> ([n, 4] words, h's word)"""
    its = np.float32(1.0) / np.float32(side)
    p = np.arange(n, dtype=np.int32).astype(np.float32)
    x0 = p * its
    h = np.float32(0.5) * its - np.float32(0.25) * PAD
    assert h.dtype == np.float32 and x0.dtype == np.float32
    c = x0 + h
    r0, r1 = c - h, c + h
    t = x0.astype(np.int32)  # (non-negative: truncation)
    words = np.stack([c.view(np.uint32), r0.view(np.uint32), r1.view(np.uint32), t.view(np.uint32)], axis=1)
    return words, np.float32(h).reshape(1).view(np.uint32)[0]


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_tables_hold_the_kernels_bits(driver, film, side):
    W, H = film
    words, hx, hy = _tables(driver, W, H, side)
    ref_x, h = _restated(W, side)
    ref_y, _ = _restated(H, side)
    assert hx == h and hy == h
    assert np.array_equal(words[:W], ref_x), "columns"
    assert np.array_equal(words[W:], ref_y), "rows"
    log2 = side.bit_length() - 1
    for n, part in ((W, words[:W]), (H, words[W:])):
        p = np.arange(n)
        t = part[:, 3].view(np.int32)
        assert np.array_equal(t, p >> log2), "the tile of a column / row is its index shifted by the tile side"
        c, r0, r1 = (part[:, k].view(np.float32).astype(np.float64) for k in range(3))
        hh = float(np.array([h], np.uint32).view(np.float32)[0])
        # the half-pad rule: the rectangle starts within a rounding of the pixel's near edge and ends a half pad short of its far edge — inside the
        # pixel's own tile even for the last column of a tile and for the film's last column, beyond every sample position short of p + 1 by less than
        # the entries' padding (half a pad: 1/512 tile)
        near, far = p / side, (p + 1) / side
        assert np.all(np.abs(r0 - near) <= 2.0 ** -20 * np.maximum(1.0, near)) and np.all(r1 < far) and np.all(far - r1 <= 0.5 * float(PAD) + 2.0 ** -20 * far)
        assert np.all(np.floor(r1) == t), "the far bound inside the pixel's own tile"
        assert np.all(np.abs(c - (near + hh)) <= 2.0 ** -20 * np.maximum(1.0, near))
        for q in sorted({side - 1, n - 1} & set(range(n))):  # the last column of the first tile, and the film's last column
            assert t[q] == q >> log2 and r1[q] < (q + 1) / side and np.floor(r1[q]) == q >> log2
        last_of_tiles = p[(p % side) == side - 1]
        assert np.all(r1[last_of_tiles] < (last_of_tiles + 1) / side), "the last column of every tile stays out of the next tile"


def test_films_without_a_table(driver):
    """no table beyond FFX_RECT_MAX_SIDE (4096) pixels a side, for an empty film or for a tile side that is no reciprocal in (0, 1]"""
    assert _tables(driver, 4097, 3, 8) is None and _tables(driver, 3, 4097, 8) is None
    assert _tables(driver, 0, 3, 8) is None and _tables(driver, 3, 0, 8) is None
    assert _tables(driver, 4096, 4096, 8) is not None
