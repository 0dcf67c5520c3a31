"""A numpy restatement of DESIGN.md 4.11 (connected components with statistics, include/ffx_labels.h) and the masks its tests share.  numpy only: no
torch, no device.
  labels       every foreground pixel takes the smallest linear index it can reach: the minimum over its 4 / 8 neighbours, repeated until nothing
               changes (with a pointer jump per round, which only shortens the way); the pixels that kept their own index are the roots, a root's rank
               in linear order + 1 is its component's number
  stats        from the labels in int64; centroids: exact int64 sums, converted to float64, one division
  accept       the reference's literal chain of main.py:168-180 over these labels
"""
import functools

import numpy as np

SIZES = ((1, 1), (1, 70), (70, 1), (33, 65), (96, 80), (130, 67))  # (h, w): they straddle any tile side up to 64


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside"""
    h, w = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def label(fg, connectivity=8):
    """-> (n_labels, labels int32 [h, w]) of the boolean mask `fg`"""
    assert connectivity in (4, 8)
    fg = np.asarray(fg, bool)
    h, w = fg.shape
    n = h * w
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    low = np.where(fg, idx, n)  # n: the background's sentinel, larger than every index
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    while True:
        new = low.copy()
        for dy, dx in steps:
            new = np.minimum(new, _shift(low, dy, dx, n))
        new = np.where(fg, new, n)
        new = np.append(new.ravel(), n)[new]  # the pixel my minimum points at may know a smaller one
        if np.array_equal(new, low):
            break
        low = new
    roots = fg & (low == idx)
    number = np.cumsum(roots.ravel())  # number[r] of a root r: its rank + 1
    labels = np.where(fg, np.append(number, 0)[low], 0).astype(np.int32)
    return int(roots.sum()) + 1, labels


def stats(labels, n_labels, max_labels):
    """-> (stats int32 [max_labels, 5]: left, top, width, height, area; centroids float64 [max_labels, 2]) of a label image"""
    h, w = labels.shape
    rows = min(n_labels, max_labels)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    keep = labels.ravel() < rows
    lab, x, y = labels.ravel()[keep].astype(np.int64), xs.ravel()[keep], ys.ravel()[keep]
    area, sx, sy = (np.zeros(max_labels, np.int64) for _ in range(3))
    np.add.at(area, lab, 1)
    np.add.at(sx, lab, x)
    np.add.at(sy, lab, y)
    x0, y0 = np.full(max_labels, w, np.int64), np.full(max_labels, h, np.int64)
    x1, y1 = np.full(max_labels, -1, np.int64), np.full(max_labels, -1, np.int64)
    np.minimum.at(x0, lab, x)
    np.minimum.at(y0, lab, y)
    np.maximum.at(x1, lab, x)
    np.maximum.at(y1, lab, y)
    on = area > 0
    st = np.where(on[:, None], np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1, area], 1), 0).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        cen = np.stack([sx.astype(np.float64) / area.astype(np.float64), sy.astype(np.float64) / area.astype(np.float64)], 1)
    return st, cen


def components(img, connectivity=8, background=0, max_labels=256):
    """the four outputs of ffx_connected_components for the integer image `img`"""
    n, lab = label(np.asarray(img).astype(np.int64) != int(background), connectivity)
    st, cen = stats(lab, n, max_labels)
    return n, lab, st, cen


def accept(seg):
    """main.py:161-180, literally, on the label image `seg`: whether the dataset loop keeps the sample"""
    segmentation = np.asarray(seg).astype(np.float32)
    if segmentation.max() == 0:
        return False
    seg_test = segmentation.copy()
    seg_test[seg_test == 1] = 0
    seg_test[seg_test == 2] = 1
    seg_test = 1 - seg_test
    with np.errstate(invalid="ignore"):
        mask = seg_test.astype(np.int64).astype(np.uint8)  # (through int64: a negative float to uint8 directly is left to the C compiler; this is the wrap)
    n_labels, _ = label(mask != 0, 8)  # cv2.connectedComponentsWithStats' default connectivity
    return not n_labels > 3


# ------------------------------------------------------------------ the masks
def full(h, w, value=True):
    return np.full((h, w), value, bool)


def checkerboard(h=64, w=64):
    y, x = np.mgrid[0:h, 0:w]
    return (x + y) % 2 == 0


def random_mask(h, w, density, seed):
    return np.random.default_rng(seed).random((h, w)) < density


def serpentine(h=130, w=67):
    """a one-pixel path through the whole image: every other row, joined at alternating ends"""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def comb(h=96, w=80):
    """vertical teeth one pixel apart, joined by the last row only"""
    m = np.zeros((h, w), bool)
    m[:, 0::2] = True
    m[h - 1] = True
    return m


def diagonal(h=96, w=80, anti=False):
    m = np.zeros((h, w), bool)
    k = np.arange(min(h, w))
    m[k, (w - 1 - k) if anti else k] = True
    return m


def corner_pairs(h=96, w=80, anti=False, step=8):
    """a two-pixel pair across every interior grid corner at the multiples of `step` (so of 16, 32 and 64 too): the pixels (cy - 1, cx - 1), (cy, cx), or
    with `anti` (cy - 1, cx), (cy, cx - 1) — joined at 8-connectivity only, and only across the corner"""
    m = np.zeros((h, w), bool)
    for cy in range(step, h, step):
        for cx in range(step, w, step):
            m[cy - 1, cx if anti else cx - 1] = True
            m[cy, cx - 1 if anti else cx] = True
    return m


def rings(h=96, w=80, n=3, value=True, dtype=bool, gap=6, at=(4, 4), into=None):
    """n nested one-pixel square rings, the outermost with its corner at `at`"""
    m = np.zeros((h, w), dtype) if into is None else into
    y0, x0 = at
    side = min(h - y0, w - x0) - 4 if into is None else gap * 2 * n + 2
    for k in range(n):
        a, b = k * gap, side - 1 - k * gap
        if b - a < 2:
            break
        m[y0 + a, x0 + a:x0 + b + 1] = value
        m[y0 + b, x0 + a:x0 + b + 1] = value
        m[y0 + a:y0 + b + 1, x0 + a] = value
        m[y0 + a:y0 + b + 1, x0 + b] = value
    return m


RANDOM = [(h, w, d, s) for (h, w) in ((96, 80), (33, 65)) for d in (0.3, 0.5, 0.593, 0.8) for s in range(4)]  # 32 masks
MASKS = {
    **{f"full-{h}x{w}": functools.partial(full, h, w) for h, w in SIZES},
    **{f"empty-{h}x{w}": functools.partial(full, h, w, False) for h, w in SIZES},
    "checkerboard-64": checkerboard,
    **{f"random-{h}x{w}-{d}-seed{s}": functools.partial(random_mask, h, w, d, s) for h, w, d, s in RANDOM},
    "serpentine-130x67": serpentine,
    "comb-96x80": comb,
    "comb-130x67": functools.partial(comb, 130, 67),
    "diagonal": diagonal,
    "anti-diagonal": functools.partial(diagonal, anti=True),
    "corner-pairs": corner_pairs,
    "corner-pairs-anti": functools.partial(corner_pairs, anti=True),
    "rings": rings,
}


@functools.lru_cache(maxsize=None)
def mask(name):
    m = MASKS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(name, connectivity, max_labels=256):
    """components() of a mask, computed once and handed out read-only"""
    out = components(mask(name), connectivity, 0, max_labels)
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ label images with a known verdict: name -> (seg, n_labels of seg != 2, kept)
def _seg_base(h=64, w=64):
    seg = np.zeros((h, w), np.int64)
    seg[:, w // 2:] = 1  # labels 0 and 1 side by side: one piece of foreground
    return seg


def seg_cases():
    out = {"all-zero": (np.zeros((64, 64), np.int64), 2, False)}
    blob = _seg_base()
    blob[20:30, 25:40] = 2
    out["blob"] = (blob, 2, True)
    ring = rings(n=1, value=2, at=(10, 12), into=_seg_base())
    out["ring"] = (ring, 3, True)
    two = rings(n=1, value=2, at=(40, 30), into=ring.copy())
    out["two-rings"] = (two, 4, False)
    # the glottis against the image's border, its inside of label 3: were label 3 background, like 2, one piece would remain
    three = _seg_base()
    three[0:12, 0:12] = 2
    three[0:11, 0:11] = 3
    out["label-3-is-foreground"] = (three, 3, True)
    three_b = rings(n=1, value=2, at=(40, 30), into=rings(n=1, value=2, at=(10, 12), into=three.copy()))
    out["label-3-and-two-rings"] = (three_b, 5, False)
    # ... and here the verdict hangs on it: the pocket of label 3, the inside of one ring and the rest are three pieces (dropped); with label 3 taken for
    # background there would be two (kept)
    flips = rings(n=1, value=2, at=(40, 30), into=three.copy())
    assert label((flips == 0) | (flips == 1), 8)[0] == 3
    out["label-3-flips-the-verdict"] = (flips, 4, False)
    return out
