"""DESIGN.md 4.12 in float64: the multi-octave Perlin base-colour texture that ffx_perlin_texture and the sampler's torch path are held to, from the
same binary32 tables (lattice angles, positions inside the cells) that they take.  numpy only; the cases of the suites stand here once."""
import numpy as np

# name -> (shape, base lattice, octaves, persistence): the issue's list.  A twice, for a persistence below and above one; E and F at 0.5
CASES = {
    "A-0.5": ((32, 32), (2, 2), 4, 0.5),
    "A-2.0": ((32, 32), (2, 2), 4, 2.0),
    "B": ((40, 24), (2, 2), 3, 1.3),      # non-divisible, clamped cells, w below a tile's width
    "C": ((33, 47), (4, 4), 2, 0.1),
    "D": ((96, 64), (2, 4), 3, 0.7),      # anisotropic lattice
    "E": ((2, 2), (1, 1), 1, 0.5),        # smallest
    "F": ((64, 64), (32, 32), 2, 0.5),    # the second octave has one-texel cells and adds exact zeros
    "G": ((257, 130), (1, 2), 4, 1.3),    # ragged in both axes, several workgroups, extremes far apart
}
DEGENERATE = ((64, 64), (64, 64), 1, 0.5)  # F': every cell is one texel, every position 0: max == min, a NaN texture


def lattices(res, octaves):
    """[(R0, R1)] per octave"""
    return [(int(res[0]) << o, int(res[1]) << o) for o in range(int(octaves))]


def fade(t):
    return 6 * t**5 - 15 * t**4 + 10 * t**3


def lerp(a, b, t):
    return a + t * (b - a)


def noise(angles, pos, shape, res, octaves, persistence):
    """the noise plane [h, w] in float64.  angles: per octave the [R0 + 1, R1 + 1] binary32 lattice angles; pos: per octave (fy [h], fx [w]), the
    binary32 positions inside the cells"""
    h, w = int(shape[0]), int(shape[1])
    out = np.zeros((h, w), np.float64)
    amplitude = 1.0
    for (R0, R1), ang, (fy, fx) in zip(lattices(res, octaves), angles, pos):
        c0, c1 = h // R0, w // R1
        assert c0 >= 1 and c1 >= 1 and ang.shape == (R0 + 1, R1 + 1) and ang.dtype == np.float32 and fy.dtype == np.float32 and fx.dtype == np.float32
        assert fy.shape == (h,) and fx.shape == (w,)
        a = ang.astype(np.float64)
        gc, gs = np.cos(a), np.sin(a)
        cy = np.minimum(np.arange(h) // c0, R0 - 1)[:, None]
        cx = np.minimum(np.arange(w) // c1, R1 - 1)[None, :]
        py, px = fy.astype(np.float64)[:, None], fx.astype(np.float64)[None, :]

        def n(dy, dx):
            return (py - dy) * gc[cy + dy, cx + dx] + (px - dx) * gs[cy + dy, cx + dx]

        ty, tx = fade(py), fade(px)
        octave = np.sqrt(2.0) * lerp(lerp(n(0, 0), n(1, 0), ty), lerp(n(0, 1), n(1, 1), ty), tx)
        out += float(np.float32(amplitude)) * octave  # a_o: the binary32 value of persistence^o
        amplitude *= float(persistence)
    return out


def normalised(plane):
    """t = (noise - min) / (max - min); max == min is the same division: NaN"""
    lo, hi = plane.min(), plane.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return (plane - lo) / (hi - lo)


def texture(angles, pos, shape, res, octaves, persistence, color_a, color_b):
    """[3, h, w] in float64: color_a .. color_b (binary32 values) blended by the normalised noise"""
    t = normalised(noise(angles, pos, shape, res, octaves, persistence))[None]
    a = np.asarray(color_a, np.float32).astype(np.float64).reshape(3, 1, 1)
    b = np.asarray(color_b, np.float32).astype(np.float64).reshape(3, 1, 1)
    return lerp(a, b, t)
