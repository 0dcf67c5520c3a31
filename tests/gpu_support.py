"""Helpers of the tests that need the device (tests/*_gpu.py and tests/test_hip_parity.py only): arrays to and from it, the oracle's and the device's
geometry of one scene, what a blob's bin and envelope headers say, its tile lists, apex records and triangle records, a host copy of all the update writes, a loaded scene with its world
arrays, seeded textures and gradient images, the lights' table and the emitter suites' corner cases, the loss of a material table, leaves and fits, the rows' and the spot's central differences of the GPU forward, forward mode against the adjoints."""
import numpy as np
import torch

from fireflies_amd import mi, ops, scene_desc, scenes
from tests import ref_path
from tests.support import copy_desc, world_arrays

DEV = "cuda"
# the knobs that choose a walk or a kernel variant: tests/test_ties_gpu.py and tests/test_seams_gpu.py clear them before every test
WALK_KNOBS = ("FFX_BINS", "FFX_WIDE", "FFX_TRAVERSAL", "FFX_BIN_CAP", "FFX_WIDE_BUILD", "FFX_ENVELOPE", "FFX_RENDER_BLOCKS", "FFX_DETERMINISTIC", "FFX_BIN_TILE",
              "FFX_TREELET_TRIS", "FFX_PIXELS_PER_WAVE", "FFX_XCD_REMAP", "FFX_TILE_BLOCK")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def host(t):
    return t.detach().cpu().numpy()


class Env:
    """with Env(monkeypatch, {...}): the variables are set inside the block and unset behind it"""

    def __init__(self, monkeypatch, env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k, raising=False)


# ------------------------------------------------------------------ the oracle and the device on one scene
def pair(oracle, sc, frame=0, xforms=None):
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    S = len(sc.meshes)
    if xforms is None:
        xforms = np.tile(np.eye(4, dtype=np.float32), (S, 1, 1))
    offs = (off + np.minimum(frame, nfr - 1) * stride).astype(np.int32)
    go = oracle.Geometry(pool, tris, shape, off)
    go.update(xforms, offs)
    gd = ops.DeviceGeometry(pool, tris, shape, off)
    gd.update(xforms, offs)
    return go, gd, alb


def splat_tex(sc, ch=1, seed=0):
    """a projector texture of 64 blurred splats (rand_tex: uniform noise of a description's size)"""
    rng = np.random.default_rng(seed)
    n = 64
    pts = (rng.random((n, 2)) * 0.8 + 0.1).astype(np.float32)
    t = ops.blur_fwd(ops.splat_fwd(dev(pts), 10.0, "sum", -1, sc.projector.width, sc.projector.height))
    if ch == 3:
        t = torch.stack([0.2 * t, t, 0.1 * t], -1).contiguous()
    return t


def bin_headers(gd):
    """{ok, total, cap} of the three tile-bin grids (camera, projector, spot) of the blob the next render reads (ffx_common.h BinHdr)"""
    torch.cuda.synchronize()
    blob, info = gd.blob, gd.info
    out = []
    for a in range(3):
        o = int(info.off_bins) + a * int(info.bins_stride)
        out.append(tuple(int(v) for v in blob[o: o + 12].cpu().numpy().view(np.uint32)))
    return out


def envelope(gd, a, n_cells_x, n_cells_y):
    """(header flag, [ny, nx, 4] cells) of emitter a's envelope in the blob the next render reads (ffx_common.h FFX_ENV_SUB, ffx_bin_off_env)"""
    torch.cuda.synchronize()
    info, blob = gd.info, gd.blob
    F, NT = int(info.n_tris), 16384
    off_entries = ((64 + 4 * (NT + 16) + 4 * NT + 63) // 64) * 64
    off_env = ((off_entries + 64 * (2 * F + NT + 64) + 63) // 64) * 64
    base = int(info.off_bins) + a * int(info.bins_stride)
    hdr = blob[base: base + 64].cpu().numpy().view(np.uint32)
    cells = blob[base + off_env: base + off_env + 16 * n_cells_x * n_cells_y].cpu().numpy().view(np.float32).reshape(n_cells_y, n_cells_x, 4)
    return int(hdr[4]), cells, int(hdr[0])


BIN_MAX_TILES, LEAF_MAX = 16384, 4  # ffx_common.h FFX_BIN_MAX_TILES, FFX_LEAF_MAX
BIN_ENTRY = np.dtype([("bb", "<f4", 4), ("e", "<f4", 9), ("slot", "<i4"), ("pad", "<u4", 2)])  # ffx_common.h BinEntry
TRI_APEX = np.dtype([("A", "<f4", 3), ("B", "<f4", 3), ("C", "<f4", 3), ("T", "<f4"), ("prim", "<i4"), ("shape", "<i4")])  # ffx_common.h TriApex


def _bytes(blob, off, n):
    return blob[off: off + n].cpu().numpy()


def bin_lists(gd, a, nx, ny, n_entries=None):
    """(hdr [16] uint32, starts [nt + 1], cursors [nt], entries [total] as BIN_ENTRY) of grid a (0 camera, 1 projector, 2 spot) of nx x ny tiles in the
    blob the next render reads (ffx_common.h BinHdr, ffx_bin_off_starts / _cursors / _entries).  n_entries: read that many entries whatever the header
    says (lists that did not fit: what the entries area holds)"""
    torch.cuda.synchronize()
    blob, nt = gd.blob, nx * ny
    base = int(gd.info.off_bins) + a * int(gd.info.bins_stride)
    off_cursors = 64 + 4 * (BIN_MAX_TILES + 16)
    off_entries = (off_cursors + 4 * BIN_MAX_TILES + 63) // 64 * 64
    hdr = _bytes(blob, base, 64).view(np.uint32)
    starts = _bytes(blob, base + 64, 4 * (nt + 1)).view(np.uint32)
    cursors = _bytes(blob, base + off_cursors, 4 * nt).view(np.uint32)
    n = int(hdr[1]) if n_entries is None else int(n_entries)
    assert 0 <= n <= 2 * int(gd.info.n_tris) + BIN_MAX_TILES + 64, (n, hdr[:5])  # (the entries area: cap + 64)
    return hdr, starts, cursors, _bytes(blob, base + off_entries, 64 * n).view(BIN_ENTRY)


def apex_records(gd, a):
    """[F] TRI_APEX: the triangles as apex a sees them (A = e2 x e1, T = e2 . ((o - v0) x e1)), in leaf-slot order, from the blob the next render reads"""
    torch.cuda.synchronize()
    F = int(gd.info.n_tris)
    stride = ((F + LEAF_MAX) * 48 + 63) // 64 * 64
    return _bytes(gd.blob, int(gd.info.total_bytes) - (3 - a) * stride, 48 * F).view(TRI_APEX)


def tri_records(gd):
    """[F, 3, 3] float64: the posed triangles in leaf-slot order as the blob's own records hold them (float32 v0, v0 + e1, v0 + e2, widened)"""
    torch.cuda.synchronize()
    r = _bytes(gd.blob, int(gd.info.off_recs), 48 * int(gd.info.n_tris)).view(np.float32).reshape(-1, 12).astype(np.float64)
    return np.stack([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9]], 1)


def blob_host(gd, copy=None):
    """the first off_bins bytes — everything the builder and the geometry update write — of the blob the next render reads (or of blob copy `copy`),
    on the host.  Taking the blob orders the caller's stream behind its re-fit (and launches a deferred top): what a render would find"""
    b = gd.blob if copy is None else gd._blobs[copy]
    torch.cuda.synchronize()
    return _bytes(b, 0, int(gd.info.off_bins)).copy()


def grad_close(got, want, what, frac):
    """a texture gradient against the oracle's: 1e-3 of its scale per texel on all but `frac` of them, none off by more than 0.1 of it; the figures are
    printed before they are asserted"""
    got, want = np.asarray(got), np.asarray(want)
    gs = float(np.abs(want).max())
    assert gs > 0, what
    err = np.abs(got - want.reshape(got.shape))
    print(f"GRAD {what}: {float((err > 1e-3 * gs).mean()):.2e} of the texels off by more than 1e-3 of the scale [{frac:g}], worst {err.max() / gs:.2e} [0.1]")
    assert np.isfinite(got).all() and (err > 1e-3 * gs).mean() <= frac and err.max() <= 0.1 * gs, what


# ------------------------------------------------------------------ a loaded scene and what the adjoint tests feed it
def load(sc, gaussian, tc):
    """-> (the loaded scene, its description with tc texture channels, (vertex pool in float64, triangles in pool indices, shape of every triangle))"""
    ms = mi.load_scene_data(sc, device=DEV, shadows=True)
    if gaussian:
        ms.rfilter = "gaussian"
    return ms, ms.scene_desc(tex_channels=tc), world_arrays(sc)[:3]


def rand_tex(sd, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels), generator=g).to(DEV)


def rand_gimg(sd, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + torch.rand((sd.cam.height, sd.cam.width, 3), generator=g)).to(DEV)


def table(*lights):
    """the lights' [n, 24] table of ops.pack_lights on the device"""
    return ops.pack_lights(lights).to(DEV)


_CORNERS = {}


def corner_case(corner, film, principled, gaussian, spp, seed, direct=True):
    """the scene `corner(film, principled)` of one of the emitter suites' builders, loaded once per builder and arguments: (scene, description, world
    arrays, rows in float64, texture — None without a projector —, materials argument, the image without extra emitters at direct light and its float64
    restatement — None, None unless `direct`)"""
    key = (corner, film, principled, gaussian, spp, seed, direct)
    if key not in _CORNERS:
        ms, sd, world = load(corner(film, principled), gaussian, 1)
        rows = ms.albedo.cpu().numpy().astype(np.float64)
        tex = rand_tex(sd, 1) if sd.proj.enabled else None
        mats = ms.materials_arg(sd)
        unlit = main_ref = None
        if direct:
            unlit = ms.geom.render_fwd(sd, mats, tex, spp, seed)
            main_ref = ref_path.render_fwd(*world, sd, rows, tex.cpu().numpy(), spp, seed, 2, gaussian_stddev=0.5 if gaussian else None)
        _CORNERS[key] = (ms, sd, world, rows, tex, mats, unlit, main_ref)
    return _CORNERS[key]


def loss(ms, sd, rows, tex, spp, seed, gimg, max_depth=2, rr_depth=5):
    """<render_fwd under the material table `rows`, gimg> in float64"""
    s2 = copy_desc(sd)
    assert scene_desc.set_host_materials(s2, np.asarray(rows, np.float32)) is not False
    img = ms.geom.render_fwd(s2, None, tex, spp, seed, max_depth=max_depth, rr_depth=rr_depth)
    return float((img.double() * gimg.double()).sum())


def rows_central_differences(ms, sd, app, rows, tex, spp, seed, gimg, depth, rr, skip=(), h=1e-2):
    """the rows block of `app` against central differences of render_fwd over every base colour (rows in `skip` excepted: their colour is a texture),
    roulette off by the caller's rr: 1e-3 of the largest difference -> (the block, the differences' scale)"""
    g = app.rows.double().cpu().numpy()
    fd = np.zeros_like(g)
    for i in range(rows.shape[0]):
        if i in skip:
            continue
        for k in range(3):
            lo, hi = rows.copy(), rows.copy()
            lo[i, k] -= h
            hi[i, k] += h
            fd[i, k] = (loss(ms, sd, hi, tex, spp, seed, gimg, depth, rr) - loss(ms, sd, lo, tex, spp, seed, gimg, depth, rr)) / (2 * h)
    scale = np.abs(fd).max()
    print("rows: max |g - fd|", np.abs(g - fd).max(), "scale", scale)
    assert scale > 0 and np.abs(g - fd).max() <= 1e-3 * scale, (g, fd)
    return g, scale


def spot_differences(ms, sd, app, mats, tex, spp, seed, gimg, depth, rr):
    """the spot block of `app` against differences of render_fwd over the intensity (the image is linear in it): 1e-3 of each"""
    for c in range(3):
        lo, hi = copy_desc(sd), copy_desc(sd)
        lo.spot.intensity[c] -= 0.5
        hi.spot.intensity[c] += 0.5
        ls = [float((ms.geom.render_fwd(s, mats, tex, spp, seed, max_depth=depth, rr_depth=rr).double() * gimg.double()).sum()) for s in (hi, lo)]
        f = ls[0] - ls[1]
        print("spot", c, float(app.spot[c]), f)
        assert f > 0 and abs(float(app.spot[c]) - f) <= 1e-3 * f


def leaf(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV, requires_grad=True)


def fit(ms, key, start, target_img, spp, seed, lr, iters, integrator=None):
    """Adam on the parameter `key` from `start` towards the image `target_img` -> the fitted value"""
    p = mi.traverse(ms)
    x = leaf(start)
    opt = torch.optim.Adam([x], lr=lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.98)
    for _ in range(iters):
        p[key] = x
        p.update()
        err = ((mi.render(ms, spp=spp, seed=seed, integrator=integrator).torch() - target_img) ** 2).mean()
        opt.zero_grad()
        err.backward()
        opt.step()
        sched.step()
    return x.detach()


# ------------------------------------------------------------------ forward mode against the adjoints: the dot-product identity
def rand(shape, seed, lo=0.5, hi=1.5):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g)).to(DEV)


def tangent(ms, sd, seed):
    """a random tangent in every block: (dtex, AppearanceGrad)"""
    S = sd.n_shapes
    dtex = rand((sd.proj.tex_h, sd.proj.tex_w, sd.proj.tex_channels), seed, -1.0, 1.0) if sd.proj.enabled else None
    bts = [rand(tuple(t.shape), seed + 10 + k, -1.0, 1.0) for k, (_, t) in enumerate(ms._base_tex)]
    mat = rand((S, 11), seed + 3, -1.0, 1.0) if int(sd.mat_stride) == scenes.MAT_STRIDE else None
    return dtex, ops.AppearanceGrad(rand((S, 3), seed + 1, -1.0, 1.0), rand((3,), seed + 2, -1.0, 1.0), bts, mat)


def jvp(ms, sd, tex, spp, seed, dtex, tan, depth=2, rr=5):
    return ms.geom.render_jvp(sd, ms.albedo, tex, spp, seed, dtex=dtex, tangent=tan, max_depth=depth, rr_depth=rr)


def adjoint(ms, sd, spp, seed, gimg, tex, depth, rr):
    material = int(sd.mat_stride) == scenes.MAT_STRIDE
    if depth == 2:
        return ms.geom.render_bwd(sd, None if sd.n_mat_h > 0 else ms.albedo, spp, seed, gimg, appearance=True, tex=tex, material=material)
    return ms.geom.render_bwd_prb(sd, None if sd.n_mat_h > 0 else ms.albedo, spp, seed, gimg, tex, depth, rr, material=material)


def pairs(dtex, tan, gtex, app):
    """(name, tangent block, gradient block) for every block both sides hold"""
    out = [("tex", dtex, gtex), ("rows", tan.rows, app.rows), ("spot", tan.spot, app.spot)]
    out += [(f"base_tex[{k}]", t, g) for k, (t, g) in enumerate(zip(tan.base_tex or [], app.base_tex))]
    if tan.material is not None:
        out.append(("material", tan.material, app.material))
    return [(n, t, g) for n, t, g in out if t is not None]


def identity(ms, sd, tex, spp, seed, gimg, dtex, tan, depth, rr, what):
    """|<dimg, gimg> - <tangent, gradient>| <= 1e-3 sum |terms|, the terms being the products the right side sums: the adjoint's entries are sums of
    float atomics, each good to 1e-3 of its own size, and the inner product weighs entry i by the tangent's entry i.  float64 on the host"""
    _, dimg = jvp(ms, sd, tex, spp, seed, dtex, tan, depth, rr)
    gtex, app = adjoint(ms, sd, spp, seed, gimg, tex, depth, rr)
    lhs = float((dimg.double() * gimg.double()).sum())
    rhs = terms = 0.0
    for _, t, g in pairs(dtex, tan, gtex, app):
        p = t.double().reshape(-1) * g.double().reshape(-1)
        rhs += float(p.sum())
        terms += float(p.abs().sum())
    print(f"{what}: <dimg, gimg> {lhs:.9e}  <tangent, gradient> {rhs:.9e}  |difference| {abs(lhs - rhs):.3e}  1e-3 sum |terms| {1e-3 * terms:.3e}")
    assert np.isfinite(lhs) and terms > 0 and abs(lhs - rhs) <= 1e-3 * terms, (what, lhs, rhs, terms)
    return lhs


def one_block(dtex, tan, name):
    """the tangent with every block but `name` zeroed"""
    z = lambda t: None if t is None else torch.zeros_like(t)  # noqa: E731
    bts = [t if name == f"base_tex[{k}]" else z(t) for k, t in enumerate(tan.base_tex or [])]
    return (dtex if name == "tex" else z(dtex),
            ops.AppearanceGrad(tan.rows if name == "rows" else z(tan.rows), tan.spot if name == "spot" else z(tan.spot), bts,
                               tan.material if name == "material" else z(tan.material)))
