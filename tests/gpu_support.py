"""Helpers of the tests that need the device (tests/*_gpu.py and tests/test_hip_parity.py only): arrays to and from it, the oracle's and the device's
geometry of one scene, what a blob's bin and envelope headers say, a loaded scene with its world arrays, seeded textures and gradient images, the loss
of a material table, leaves and fits."""
import numpy as np
import torch

from fireflies_amd import mi, ops, scene_desc, scenes
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


def loss(ms, sd, rows, tex, spp, seed, gimg, max_depth=2, rr_depth=5):
    """<render_fwd under the material table `rows`, gimg> in float64"""
    s2 = copy_desc(sd)
    assert scene_desc.set_host_materials(s2, np.asarray(rows, np.float32)) is not False
    img = ms.geom.render_fwd(s2, None, tex, spp, seed, max_depth=max_depth, rr_depth=rr_depth)
    return float((img.double() * gimg.double()).sum())


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
