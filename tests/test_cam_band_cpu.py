"""The camera's operand band (fireflies_amd/csrc/ffx_band.h): the host-side proof that lets the plain-scene instance of the packet render kernel
take cam_ray's root and reciprocals without the IEEE expansions' range fix-ups.

  * soundness — whenever the helper says "in band", a dense float64 scan of the film finds |np|^2, |np| and |dl.z| inside the band
    (|np|^2, |dl.z| in [2^-40, 2^40], so |np| in [2^-20, 2^20]) and inside the helper's own bounds;
  * rejection — cameras with sample-to-camera rows scaled by 2^+-50, with a homogeneous w that varies over the film, or whose qz changes sign on
    the film are "out";
  * exactness — the in-band chains (seed, the expansion's fma sequence, for the root the +-1-ulp residual correction) return exactly 1.0f / x and
    sqrtf(x) for every seed within an ulp of the correctly rounded one, for 10^6 random in-band operands and the band's edges.  (Found while
    writing it: at operands with an all-ones mantissa the reciprocal chain is exact from the correctly rounded seed only — see the test.)

The helper is a header without HIP: a small host program around it is compiled here with g++."""
import math
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent

LO, HI = 2.0 ** -40, 2.0 ** 40

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <random>
#include "ffx_band.h"
// cams: stdin holds cameras, one per line: 16 floats of s2c (as hex bit patterns), w_uniform, iw_u's bits -> "in np2_lo np2_hi dz_lo dz_hi" per camera
// exact N: the chains against 1.0f / x and sqrtf(x) -> "rcp <tested> <differing>" and "sqrt <tested> <differing>"
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "cams")) {
    for (;;) {
      float m[16];
      unsigned u, wu;
      int ok = 1;
      for (int i = 0; i < 16; ++i) { if (scanf("%x", &u) != 1) { ok = 0; break; } m[i] = from_bits(u); }
      if (!ok || scanf("%u %x", &wu, &u) != 2) break;
      FfxCamBand b;
      const bool in = ffx_cam_in_band(m, (int)wu, from_bits(u), &b);
      printf("%d %.17g %.17g %.17g %.17g\n", in ? 1 : 0, b.np2_lo, b.np2_hi, b.dz_lo, b.dz_hi);
    }
    return 0;
  }
  const long n = argc > 2 ? atol(argv[2]) : 1000000;
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> ex(-40.0, 40.0);
  long n_rcp = 0, bad_rcp = 0, n_sqrt = 0, bad_sqrt = 0, n_ones = 0, bad_ones_exact = 0, bad_ones_off = 0;
  // ones: x's mantissa is all ones (x = 2^(e+1) - 1 ulp), Markstein's hard operand of a reciprocal — the quotient lies a hair above a rounding
  // midpoint and the chain reaches it from the correctly rounded seed only; counted apart (see the test)
  auto one = [&](float x, bool ones) {
    for (int sg = 0; sg < 2; ++sg) { // the reciprocal's operand dl.z takes either sign
      const float d = sg ? -x : x, want = 1.0f / d;
      const float seeds[3] = {std::nextafterf(want, 0.0f), want, std::nextafterf(want, sg ? -INFINITY : INFINITY)};
      for (int k = 0; k < 3; ++k) {
        const float s = seeds[k], got = ffx_band_rcp_chain(d, s);
        const bool bad = memcmp(&got, &want, 4) != 0;
        if (ones) { ++n_ones; if (bad) ++(k == 1 ? bad_ones_exact : bad_ones_off); continue; }
        ++n_rcp;
        if (bad && bad_rcp++ < 5) fprintf(stderr, "rcp %a seed %a: %a, want %a\n", d, s, got, want);
      }
    }
    const float want = sqrtf(x);
    const float seeds[3] = {std::nextafterf(want, 0.0f), want, std::nextafterf(want, INFINITY)};
    for (float s : seeds) { ++n_sqrt; const float got = ffx_band_sqrt_chain(x, s); if (memcmp(&got, &want, 4)) { if (bad_sqrt++ < 5) fprintf(stderr, "sqrt %a seed %a: %a, want %a\n", x, s, got, want); } }
  };
  for (long i = 0; i < n; ++i) one((float)std::exp2(ex(rng)), false);
  const float lo = (float)FFX_BAND_LO, hi = (float)FFX_BAND_HI, rlo = 0x1p-20f, rhi = 0x1p20f; // the band's edges, and those of |np| = sqrt(|np|^2)
  const float edges[] = {lo, std::nextafterf(lo, 1.0f), hi, rlo, std::nextafterf(rlo, 1.0f), rhi, 1.0f, std::nextafterf(1.0f, 2.0f)};
  for (float e : edges) one(e, false);
  const float ones[] = {std::nextafterf(hi, 1.0f), std::nextafterf(rhi, 1.0f), std::nextafterf(1.0f, 0.0f)}; // the last floats inside the upper edges
  for (float e : ones) one(e, true);
  printf("rcp %ld %ld\nsqrt %ld %ld\nones %ld %ld %ld\n", n_rcp, bad_rcp, n_sqrt, bad_sqrt, n_ones, bad_ones_exact, bad_ones_off);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program around ffx_band.h"
    d = tmp_path_factory.mktemp("band")
    (d / "band_driver.cpp").write_text(DRIVER)
    exe = d / "band_driver"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", str(REPO / "fireflies_amd" / "csrc"), str(d / "band_driver.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def _perspective_s2c(fov_deg, near, far, w, h):
    """sample -> camera of a perspective sensor (fireflies_amd.mi.perspective_projection's matrix, inverted in float64 like the library's ffx_inv4)"""
    aspect = w / h
    c = 1.0 / math.tan(math.radians(fov_deg) * 0.5)
    P = np.array([[c, 0, 0, 0], [0, c, 0, 0], [0, 0, far / (far - near), -near * far / (far - near)], [0, 0, 1, 0]], np.float64)
    T1 = np.eye(4)
    T1[0, 3], T1[1, 3] = -1.0, -1.0 / aspect
    S1 = np.diag([-0.5, -0.5 * aspect, 1.0, 1.0])
    K = (S1 @ T1 @ P).astype(np.float32).astype(np.float64)
    return np.linalg.inv(K).astype(np.float32)


def _cam(s2c):
    """what cam_prepare derives: (s2c float32 [4, 4], w_uniform, iw_u)"""
    s2c = np.asarray(s2c, np.float32).reshape(4, 4)
    wu = int(s2c[3, 0] == 0 and s2c[3, 1] == 0 and s2c[3, 3] != 0)
    with np.errstate(all="ignore"):
        iw = np.float32(1.0) / s2c[3, 3] if wu else np.float32(0.0)
    return s2c, wu, np.float32(iw)


def _ask(driver, cams):
    lines = []
    for s2c, wu, iw in cams:
        lines.append(" ".join(f"{int(v):x}" for v in s2c.reshape(-1).view(np.uint32)) + f" {wu} {int(np.float32(iw).view(np.uint32)):x}")
    out = subprocess.run([driver, "cams"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    res = [l.split() for l in out if l.strip()]
    assert len(res) == len(cams)
    return [(r[0] == "1", tuple(float(v) for v in r[1:])) for r in res]


def _scan(s2c, wu, iw, n=65):
    """float64 over an n x n lattice of the film, corners included -> (min, max) of |np|^2 and of |dl.z|, and whether qz keeps one sign"""
    m = s2c.astype(np.float64)
    s = np.linspace(0.0, 1.0, n)
    sx, sy = np.meshgrid(s, s)
    with np.errstate(all="ignore"):
        q = [m[k, 0] * sx + m[k, 1] * sy + m[k, 3] for k in range(3)]
        w = float(iw) if wu else 1.0 / (m[3, 0] * sx + m[3, 1] * sy + m[3, 3])
        npv = [qk * w for qk in q]
        n2 = npv[0] ** 2 + npv[1] ** 2 + npv[2] ** 2
        dz = np.abs(npv[2]) / np.sqrt(n2)
    return (n2.min(), n2.max()), (dz.min(), dz.max()), bool((q[2] > 0).all() or (q[2] < 0).all())


def _scaled(s2c, log2_scale):
    out = np.array(s2c, np.float32)
    out[:3] *= np.float32(2.0 ** log2_scale)
    return out


def _cameras():
    rng = np.random.default_rng(7)
    cams, expect = [], []  # expect: True in band, False out, None whatever the helper can prove
    for _ in range(300):  # random sensors over the whole range of fields of view and near planes
        fov = float(rng.uniform(1.0, 179.0))
        near = float(10.0 ** rng.uniform(-6.0, 3.0))
        far = near * float(10.0 ** rng.uniform(0.5, 6.0))
        w, h = int(rng.integers(1, 2049)), int(rng.integers(1, 2049))
        cams.append(_cam(_perspective_s2c(fov, near, far, w, h)))
        expect.append(None)
    for fov in (1.0, 20.0, 90.0, 170.0, 179.0):  # the extremes by hand, on square and very oblong films
        for near in (1e-6, 1e-2, 1.0, 1e3):
            for w, h in ((512, 512), (2048, 16), (16, 2048)):
                cams.append(_cam(_perspective_s2c(fov, near, near * 1e3, w, h)))
                expect.append(True if (w == h and near <= 1.0) else None)
    base = _perspective_s2c(60.0, 0.01, 100.0, 512, 512)
    for sc in (50, -50):  # rows 0..2 times 2^+-50: |np|^2 = 2^+-100 times the sensor's
        cams.append(_cam(_scaled(base, sc)))
        expect.append(False)
    nu = np.array(base)  # a homogeneous w that varies over the film
    nu[3, 0] = 0.05
    cams.append(_cam(nu))
    expect.append(False)
    for col in (0, 1):  # qz changes sign across the film
        sg = np.array(base)
        sg[2, col] = -2.0 * sg[2, 3]
        cams.append(_cam(sg))
        expect.append(False)
    z0 = np.array(base)  # qz reaches zero at a corner
    z0[2, 0] = -z0[2, 3]
    cams.append(_cam(z0))
    expect.append(False)
    for bad in (np.inf, np.nan):
        b = np.array(base)
        b[0, 3] = bad
        cams.append(_cam(b))
        expect.append(False)
    return cams, expect


def test_helper_is_sound_and_rejects_what_it_must(driver):
    cams, expect = _cameras()
    res = _ask(driver, cams)
    n_in = 0
    for i, ((s2c, wu, iw), (inb, (n2lo, n2hi, dzlo, dzhi)), exp) in enumerate(zip(cams, res, expect)):
        if exp is not None:
            assert inb == exp, f"camera {i}: helper says {'in' if inb else 'out'}\n{s2c}"
        if not inb:
            continue
        n_in += 1
        assert wu == 1
        (a, b), (c, d), one_sign = _scan(s2c, wu, iw)
        assert one_sign, f"camera {i}: qz changes sign"
        assert LO <= a and b <= HI and LO <= c and d <= HI, f"camera {i}: scan finds |np|^2 in [{a}, {b}], |dl.z| in [{c}, {d}]"
        assert math.sqrt(LO) <= math.sqrt(a) and math.sqrt(b) <= math.sqrt(HI)  # |np|
        assert n2lo <= a and b <= n2hi and dzlo <= c and d <= dzhi, f"camera {i}: outside the helper's own bounds"
    # the band is generous: every perspective sensor drawn above is inside it (1 to 179 degrees, near planes from 1e-6 to 1e3)
    print(f"{n_in} of {len(cams)} cameras in band")
    assert n_in >= 300


def test_chains_are_exact_for_every_seed_within_an_ulp(driver):
    out = subprocess.run([driver, "exact", "1000000"], capture_output=True, text=True, check=True)
    got = {l.split()[0]: tuple(int(v) for v in l.split()[1:]) for l in out.stdout.strip().split("\n")}
    print(out.stdout, out.stderr[-600:])
    assert got["rcp"][0] >= 6 * 1000000 and got["sqrt"][0] >= 3 * 1000000
    assert got["rcp"][1] == 0, f"reciprocal chain: {got['rcp'][1]} of {got['rcp'][0]} results differ from 1.0f / x\n{out.stderr[-600:]}"
    assert got["sqrt"][1] == 0, f"root chain: {got['sqrt'][1]} of {got['sqrt'][0]} results differ from sqrtf(x)\n{out.stderr[-600:]}"
    # Operands whose mantissa is all ones (the last float inside each upper edge): 1 / x lies 2^-49 (relative) above a rounding midpoint, and the fma
    # chain — the compiler's own, with or without its scaling steps — lands on the correctly rounded quotient from the correctly rounded seed only:
    # measured here, from a seed one ulp off it returns the neighbour (12 of 12 such cases).  That is a property of the IEEE expansion itself, whose
    # result at these operands rests on the hardware's seed; cam_ray<BAND> performs the same operations on the same seed, so the two forms agree there
    # whatever the seed is (tools/ubench/band_exact.hip compares them on the device at these operands too).  Asserted: exact from the exact seed.
    n_ones, bad_exact, bad_off = got["ones"]
    print(f"all-ones mantissas: {n_ones} results, {bad_exact} differ from the exact seed, {bad_off} from a seed one ulp off")
    assert n_ones == 18 and bad_exact == 0
