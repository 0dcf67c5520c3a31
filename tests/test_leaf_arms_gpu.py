"""The arms of the per-lane differentiated renders that tests/corner_scenes.py's four-shape scenes never reach: row sums that bypass LDS
(more than 64 / 255 shapes), several base-colour textures, max_depth 5 .. 8 with the default roulette, more than one pass of 64 samples, prb's two-wave
workgroup.  The references are the same computation through the arm the existing tests hold (corner_scenes.mosaic with and without a shape no ray
reaches), the dot-product identity against forward mode — which has no row sums, no LDS records and no atomics —, central differences of the GPU
forward, and, where they apply, the float64 restatements.  Every compared figure is printed before it is asserted.  tests/test_leaf_arms_cpu.py
holds the scenes' layouts and shows that their high rows receive samples on the film used here."""
import numpy as np
import pytest
import torch

from fireflies_amd import mi, ops, scenes
from tests import corner_scenes as cs
from tests import gpu_support as gpu
from tests import ref_path as rp
from tests import ref_prb
from tests import support
from tests.corner_scenes import R0
from tests.support import copy_desc

pytestmark = pytest.mark.gpu
FILMS = [False, True]
FILM, SPP, TEX = cs.MOSAIC_FILM, cs.MOSAIC_SPP, cs.MOSAIC_TEX
SEED = 5


def _mosaic(gaussian, S, **kw):
    sc = cs.mosaic(S, W=FILM[0], H=FILM[1], tex=TEX, **kw)
    ms, sd, _ = gpu.load(sc, gaussian, 1)
    assert sd.n_mat_h == 0 and sd.n_shapes == len(sc.meshes)  # (a device table)
    return ms, sd


def _corner(name, gaussian, **kw):
    return gpu.load(cs.scene(name, **kw), gaussian, 1)


def _fwd(ms, sd, tex, spp, seed, depth, rr, mats=None):
    return ms.geom.render_fwd(sd, ms.materials_arg(sd) if mats is None else mats, tex, spp, seed, max_depth=depth, rr_depth=rr).clone()


def _loss(ms, sd, rows, tex, spp, seed, gimg, depth, rr):
    """<render_fwd under the material table `rows`, gimg> in float64, the table inside the scene description or on the device as the scene has it"""
    if sd.n_mat_h > 0:
        return gpu.loss(ms, sd, rows, tex, spp, seed, gimg, depth, rr)
    return float((_fwd(ms, sd, tex, spp, seed, depth, rr, gpu.dev(rows)).double() * gimg.double()).sum())


def _directional(what, dd, fd, floor):
    """a directional derivative against a central difference, test_base_texture_directional_derivative's bound"""
    print(f"{what}: <g, v> {dd:.9e}  central difference {fd:.9e}  |difference| {abs(dd - fd):.3e}  bound {1e-3 * max(abs(fd), 1e-2 * floor):.3e}")
    assert np.isfinite(dd) and floor > 0 and abs(dd - fd) <= 1e-3 * max(abs(fd), 1e-2 * floor), (what, dd, fd)


def _rows_directions(what, ms, sd, app, tex, spp, seed, gimg, depth, lows=(0, 0, 0, 0), h=1e-2):
    """central differences of render_fwd (roulette off) with the table perturbed along seeded random directions of the rows block, one per entry of
    `lows`: the direction is zero on the rows below that index"""
    rows = ms._albedo_host.astype(np.float64)
    g = app.rows.double().cpu().numpy()
    for k, lo in enumerate(lows):
        v = np.random.default_rng(100 + k).uniform(-1.0, 1.0, g.shape)
        v[:lo] = 0.0
        d = np.zeros_like(rows)
        d[:, :3] = v
        fd = (_loss(ms, sd, rows + h * d, tex, spp, seed, gimg, depth, depth) - _loss(ms, sd, rows - h * d, tex, spp, seed, gimg, depth, depth)) / (2 * h)
        _directional(f"{what} [rows >= {lo}, direction {k}]", float((g * v).sum()), fd, float((np.abs(g) * np.abs(v)).sum()))


def _block_by_block(what, ms, sd, tex, spp, seed, gimg, dtex, tan, depth, rr, min_live=3):
    """the identity over all blocks, then one block at a time as test_dot_product_identity_against_the_adjoints does -> the adjoint's (gtex, blocks)"""
    gpu.identity(ms, sd, tex, spp, seed, gimg, dtex, tan, depth, rr, what + " [all blocks]")
    gtex, app = gpu.adjoint(ms, sd, spp, seed, gimg, tex, depth, rr)
    live = 0
    for n, _, g in gpu.pairs(dtex, tan, gtex, app):
        if float(g.abs().max()) == 0.0:
            print(f"{what} [{n}]: the adjoint's block is zero; the tangent image must be too")
            _, dimg = gpu.jvp(ms, sd, tex, spp, seed, *gpu.one_block(dtex, tan, n), depth, rr)
            assert float((dimg.double() * gimg.double()).sum().abs()) <= 1e-12
            continue
        gpu.identity(ms, sd, tex, spp, seed, gimg, *gpu.one_block(dtex, tan, n), depth, rr, f"{what} [{n}]")
        live += 1
    assert live >= min_live
    return gtex, app


def _rows_from(tan, lo):
    """the tangent restricted to the rows of index >= lo of the rows and the material block"""
    def keep(t):
        if t is None:
            return None
        t = t.clone()
        t[:lo] = 0.0
        return t

    return ops.AppearanceGrad(keep(tan.rows), None, None, keep(tan.material))


def _nonzero_rows(block, lo):
    return int((block[lo:].abs().amax(1) > 0).sum())


# ------------------------------------------------------------------ 1, 2: the global-atomic arms and several base-colour textures
@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("S", [64, 255])
def test_one_arm_against_the_other(S, depth, gaussian):
    """mosaic(S) keeps the BSDF sums (S = 64) or the base-colour sums (S = 255) in LDS; one more shape, which no ray reaches, sends every sample of them
    to global atomics.  Closest hits and shadow tests do not depend on the tree, so the forward images are equal bit for bit, and the
    blocks are the same sums in another order: 1e-3 of each block's largest magnitude (float atomics); the hidden shape's rows are 0"""
    out = []
    for hidden in (False, True):
        ms, sd = _mosaic(gaussian, S, base_tex=2, hidden=hidden)
        tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4) - 1.0
        img = _fwd(ms, sd, tex, SPP, SEED, depth, 5)
        gtex, app = gpu.adjoint(ms, sd, SPP, SEED, gimg, tex, depth, 5)
        assert app.material is not None and len(app.base_tex) == 2
        out.append((img, gtex, app))
    (img, gtex, app), (img_h, gtex_h, app_h) = out
    what = f"mosaic({S}) against mosaic({S}, hidden) depth {depth} gaussian {gaussian}"
    scale, err = float(img.abs().max()), float((img - img_h).abs().max())
    print(f"{what}: forward images bitwise equal {torch.equal(img, img_h)}, max |difference| {err:.3e}, scale {scale:.4g}")
    assert scale > 0 and torch.equal(img, img_h)
    blocks = [("tex", gtex, gtex_h), ("rows", app.rows, app_h.rows[:S]), ("spot", app.spot, app_h.spot), ("material", app.material, app_h.material[:S])]
    blocks += [(f"base_tex[{k}]", a, b) for k, (a, b) in enumerate(zip(app.base_tex, app_h.base_tex))]
    for n, a, b in blocks:
        s, e = float(a.abs().max()), float((a - b).abs().max())
        print(f"{what} [{n}]: max |difference| {e:.3e}  1e-3 of the block's largest {1e-3 * s:.3e}")
        assert s > 0 and torch.isfinite(b).all() and e <= 1e-3 * s, n
    assert float(app_h.rows[S:].abs().max()) == 0.0 and float(app_h.material[S:].abs().max()) == 0.0
    # not vacuous: rows far above the four the other tests reach — above 64 where the scene has them — carry sums in both blocks (every third is principled
    # with extra lobes, wall x = 0 and the cube are Lambert rows)
    lo = 64 if S > 72 else 4
    for a in (app, app_h):
        print(f"{what}: non-zero rows of index >= {lo}: rows block {_nonzero_rows(a.rows[:S], lo)}, material block {_nonzero_rows(a.material[:S], lo)}")
        assert _nonzero_rows(a.rows[:S], lo) >= 8 and _nonzero_rows(a.material[:S], lo) >= 8


IDENTITY_CASES = [((70, 0, False), 2, 5), ((70, 0, False), 3, 1), ((300, 0, False), 2, 5), ((300, 0, False), 3, 3), ((300, 0, True), 2, 5), ((300, 0, True), 3, 3),
                  ((70, 4, False), 2, 5), ((70, 4, False), 4, 2)]


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("scene,depth,rr", IDENTITY_CASES)
def test_dot_product_identity_on_the_global_arms(scene, depth, rr, gaussian):
    """mosaic(70): base colours in LDS, BSDF columns global; mosaic(300): both global; lambert: the stride-3 table, no material block; base_tex = 4:
    every slot of the texture gradients.  All blocks at once, one at a time, and the rows and material blocks restricted to rows >= 64 (and >= 255)"""
    S, base_tex, lambert = scene
    ms, sd = _mosaic(gaussian, S, base_tex=base_tex, lambert=lambert)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4) - 1.0
    dtex, tan = gpu.tangent(ms, sd, 11)
    assert (tan.material is None) == lambert and len(tan.base_tex) == base_tex
    what = f"mosaic({S}, base_tex={base_tex}, lambert={lambert}) depth {depth} rr {rr} gaussian {gaussian}"
    gtex, app = _block_by_block(what, ms, sd, tex, SPP, SEED, gimg, dtex, tan, depth, rr, min_live=(3 if lambert else 4) + base_tex)
    for lo in (64, 255):
        if S <= lo:
            continue
        n_rows, n_mat = _nonzero_rows(app.rows, lo), (0 if lambert else _nonzero_rows(app.material, lo))
        print(f"{what}: non-zero rows of index >= {lo}: rows block {n_rows}, material block {n_mat}")
        need = min(8, S - lo - 2)  # (mosaic(70) has six rows from 64 on, two of them Lambert)
        assert n_rows >= need and (lambert or n_mat >= max(need - 2, 2))
        gpu.identity(ms, sd, tex, SPP, SEED, gimg, None, _rows_from(tan, lo), depth, rr, f"{what} [rows and material, index >= {lo}]")


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth", [2, 3])
def test_rows_follow_central_differences_on_the_global_arm(depth, gaussian):
    """mosaic(300), roulette off: the device table perturbed along four random directions of the whole rows block and one each confined to the rows
    >= 64 and >= 255.  (The material block is not differenced here: test_one_arm_against_the_other ties its global arm to the LDS arm, which the
    existing tests hold to differences, and the identity ties both to forward mode)"""
    ms, sd = _mosaic(gaussian, 300)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    _, app = gpu.adjoint(ms, sd, SPP, SEED, gimg, tex, depth, depth)
    assert _nonzero_rows(app.rows, 255) >= 8
    _rows_directions(f"mosaic(300) depth {depth} gaussian {gaussian}", ms, sd, app, tex, SPP, SEED, gimg, depth, lows=(0, 0, 0, 0, 64, 255))


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth", [2, 3])
def test_each_of_four_base_textures_follows_central_differences(depth, gaussian):
    ms, sd = _mosaic(gaussian, 70, base_tex=4)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    _, app = gpu.adjoint(ms, sd, SPP, SEED, gimg, tex, depth, depth)
    assert sd.n_base_tex == 4 and float(app.rows[:4].abs().max()) == 0.0
    h = 1e-2
    for k, (_, t) in enumerate(ms._base_tex):
        gb = app.base_tex[k]
        assert tuple(gb.shape) == tuple(t.shape) == (*cs.MOSAIC_TEX_SIZES[k], 3) and float(gb.abs().sum()) > 0
        orig = t.clone()
        try:
            for s in range(2):
                v = torch.randn(t.shape, generator=torch.Generator().manual_seed(10 * k + s)).to(gpu.DEV)
                ls = []
                for sign in (1, -1):
                    t.copy_(orig + sign * h * v)
                    ls.append(float((_fwd(ms, sd, tex, SPP, SEED, depth, depth).double() * gimg.double()).sum()))
                _directional(f"mosaic(70, base_tex=4) depth {depth} gaussian {gaussian} [base_tex[{k}], direction {s}]", float((gb.double() * v.double()).sum()),
                             (ls[0] - ls[1]) / (2 * h), float((gb.double().abs() * v.double().abs()).sum()))
        finally:
            t.copy_(orig)


# ------------------------------------------------------------------ 3: paths deeper than 4
@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth,rr", [(5, 5), (6, 3), (8, 8), (8, 5)])
@pytest.mark.parametrize("name", ["every_lobe", "textured"])
def test_deep_paths_dot_product_identity(name, depth, rr, gaussian):
    """(8, 5) is the default roulette, which first acts at the bounce of vertex 5"""
    ms, sd, _ = _corner(name, gaussian)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4) - 1.0
    dtex, tan = gpu.tangent(ms, sd, 11)
    _block_by_block(f"{name} depth {depth} rr {rr} gaussian {gaussian}", ms, sd, tex, 16, SEED, gimg, dtex, tan, depth, rr, min_live=4)


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth", [6, 8])
@pytest.mark.parametrize("name", ["every_lobe", "textured"])
def test_deep_paths_rows_and_spot_match_central_differences(name, depth, gaussian):
    """test_blocks_match_central_differences_of_the_gpu_forward's rows and spot parts (tests/gpu_support.py), roulette off"""
    sc = cs.scene(name)
    ms, sd, _ = gpu.load(sc, gaussian, 1)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4)
    _, app = ms.geom.render_bwd_prb(sd, None, 16, SEED, gimg, tex, depth, depth, material=True)
    rows = ms._albedo_host.astype(np.float64)
    gpu.rows_central_differences(ms, sd, app, rows, tex, 16, SEED, gimg, depth, depth, skip=(0,) if sc.meshes[0].base_tex is not None else ())
    gpu.spot_differences(ms, sd, app, None, tex, 16, SEED, gimg, depth, depth)


@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("name", ["every_lobe", "textured"])
def test_depth_8_repeats_bitwise_and_prb_renders_the_path_image(name, gaussian):
    ms, sd, _ = _corner(name, gaussian)
    tex = gpu.rand_tex(sd, 1)
    dtex, tan = gpu.tangent(ms, sd, 7)
    ms._params["tex.data"] = tex[..., 0].clone()
    for rr in (5, 8):
        a, b = _fwd(ms, sd, tex, 16, 3, 8, rr), _fwd(ms, sd, tex, 16, 3, 8, rr)
        img, dimg = (t.clone() for t in gpu.jvp(ms, sd, tex, 16, 3, dtex, tan, 8, rr))
        img2, dimg2 = gpu.jvp(ms, sd, tex, 16, 3, dtex, tan, 8, rr)
        print(name, gaussian, rr, "max |img|", float(a.abs().max()), "max |dimg|", float(dimg.abs().max()))
        assert float(a.abs().max()) > 0 and torch.equal(a, b) and torch.equal(img, a) and torch.equal(img2, a)
        assert torch.isfinite(dimg).all() and float(dimg.abs().max()) > 0 and torch.equal(dimg, dimg2)
        assert not torch.equal(a, _fwd(ms, sd, tex, 16, 3, 4, rr))  # (the deeper vertices carry light)
        p = mi.render(ms, spp=16, seed=3, integrator=mi.load_dict({"type": "path", "max_depth": 8, "rr_depth": rr})).torch().clone()
        q = mi.render(ms, spp=16, seed=3, integrator=mi.load_dict({"type": "prb", "max_depth": 8, "rr_depth": rr})).torch()
        assert torch.equal(p, a) and torch.equal(q, a)
    assert not torch.equal(_fwd(ms, sd, tex, 16, 3, 8, 5), _fwd(ms, sd, tex, 16, 3, 8, 8))  # (the default roulette acts at max_depth 8)


# the bounds of test_path_render_matches_float64_restatement (set at depths 3 and 4): the fraction of entries off by more than 2e-3 of the scale, the
# median error over the scale, |sum difference| over the indirect sum, the texture gradient's L1 error over its L1 norm
PATH_BOUNDS = (0.04, 1e-4, 0.01, 0.03)
PATH_BOUNDS_AT = {}  # depth -> bounds where a deeper case needed its own (twice the measured value, at most twice PATH_BOUNDS): none did


@pytest.mark.parametrize("principled,tc,gaussian", [(False, 1, False), (True, 3, True), (True, 1, True), (False, 3, False)])
def test_deep_path_render_matches_float64_restatement(principled, tc, gaussian):
    """test_path_render_matches_float64_restatement's four criteria at max_depth 6 and 8 (default roulette), with depths 3 and 4 in the same run for
    comparison: float32 and float64 paths can part at every further vertex, so the deeper values are measured, not assumed.  Measured (MI355X), as
    (fraction over 2e-3 scale [0.04], median / scale [1e-4], |sum difference| / indirect sum [0.01], gradient L1 / norm [0.03]), the largest of
    the four cases per depth: 3: (0, 3.3e-8, 1.1e-6, 2.4e-6); 4: (0, 3.8e-8, 9.2e-7, 2.8e-6); 6: (0, 3.9e-8, 8.6e-7, 2.9e-6);
    8: (0, 3.8e-8, 8.7e-7, 3.0e-6).  No path parted on this film, so every depth keeps the existing bounds"""
    ms, sd, world = gpu.load(cs.path_corner(principled), gaussian, tc)
    alb = ms.albedo.cpu().numpy().astype(np.float64)
    tex = gpu.rand_tex(sd, 1)
    spp, seed = 16, 7
    mats = ms.materials_arg(sd)
    tex_np = tex.cpu().numpy()
    stddev = 0.5 if gaussian else None
    ref2 = rp.render_fwd(*world, sd, alb, tex_np, spp, seed, 2, gaussian_stddev=stddev)
    values = {}
    for depth in (3, 4, 6, 8):
        img = ms.geom.render_fwd(sd, mats, tex, spp, seed, max_depth=depth).cpu().numpy().astype(np.float64)
        ref = rp.render_fwd(*world, sd, alb, tex_np, spp, seed, depth, gaussian_stddev=stddev)
        indirect = ref - ref2
        scale = float(ref.max())
        assert indirect.mean() > 0.05 * ref.mean() > 0
        err = np.abs(img - ref)
        gimg = np.where(np.random.default_rng(2).random(img.shape) < 0.5, -1.0, 1.0).astype(np.float32) / img.size
        gt = ms.geom.render_bwd(sd, mats, spp, seed, torch.from_numpy(gimg).to(gpu.DEV), max_depth=depth).cpu().numpy().astype(np.float64)
        gt_ref = rp.render_bwd(*world, sd, alb, spp, seed, gimg, depth, gaussian_stddev=stddev)
        gs = np.abs(gt_ref).sum()
        assert gs > 0
        values[depth] = (float((err > 2e-3 * scale).mean()), float(np.median(err) / scale), float(abs(img.sum() - ref.sum()) / indirect.sum()),
                         float(np.abs(gt - gt_ref).sum() / gs))
        print(f"principled {principled} tc {tc} gaussian {gaussian} depth {depth}: " + "  ".join(f"{v:.3e}" for v in values[depth]))
    for depth, v in values.items():
        bounds = PATH_BOUNDS_AT.get(depth, PATH_BOUNDS)
        assert all(b <= 2 * e for b, e in zip(bounds, PATH_BOUNDS)) and all(x <= b for x, b in zip(v, bounds)), (depth, v, bounds)


PRB_BOUND = 0.03  # test_blocks_match_the_float64_restatement's: every block's L1 error over its L1 norm
PRB_BOUND_AT = {}  # (depth, rr) -> the bound where a deeper case needed its own (twice the measured value, at most 2 PRB_BOUND): none did


@pytest.mark.parametrize("depth,rr", [(3, 1), (4, 2), (6, 6), (8, 5)])
@pytest.mark.parametrize("name,gaussian", [("every_lobe", False), ("defaults", True)])
def test_deep_blocks_match_the_float64_restatement(name, gaussian, depth, rr):
    """test_blocks_match_the_float64_restatement (central differences of tests/ref_prb.py, roulette frozen) on its 16 x 16 film with 8 samples at
    (6, 6) and (8, 5), with (3, 1) and (4, 2) beside them for comparison.  Measured (MI355X), L1 error over L1 norm of (gtex, rows, spot, material),
    every_lobe on the box film / defaults on the gaussian: (3, 1): (3.5e-6, 1.4e-7, 2.4e-7, 5.5e-7) / (2.6e-6, 2.4e-7, 3.8e-7, 2.3e-7);
    (4, 2): (3.9e-6, 2.6e-7, 1.9e-7, 7.0e-7) / (2.8e-6, 2.5e-7, 3.0e-7, 2.6e-7); (6, 6): (4.1e-6, 2.2e-7, 1.4e-7, 4.9e-7) / (2.9e-6, 2.3e-7,
    2.2e-7, 3.0e-7); (8, 5): (4.1e-6, 1.8e-7, 2.7e-7, 5.0e-7) / (3.1e-6, 2.3e-7, 2.8e-7, 2.8e-7): the deeper cases keep the 3 %"""
    ms, sd, world = _corner(name, gaussian, W=16, H=16)
    tex, gimg = gpu.rand_tex(sd, 1), gpu.rand_gimg(sd, 2)
    spp, seed = 8, 7
    gtex, app = ms.geom.render_bwd_prb(sd, None, spp, seed, gimg, tex, depth, rr, material=True)
    rows = ms._albedo_host.astype(np.float64)
    tex_np, gimg_np = tex.cpu().numpy(), gimg.double().cpu().numpy()
    stddev = 0.5 if gaussian else None

    def f(r, sd_=sd):
        return float((ref_prb.render_fwd_frozen(*world, sd_, r, rows, tex_np, spp, seed, depth, rr, gaussian_stddev=stddev) * gimg_np).sum())

    gt_ref = rp.render_bwd(*world, sd, rows, spp, seed, gimg_np, depth, rr, gaussian_stddev=stddev)
    fd = np.zeros((rows.shape[0], 3))
    for i in range(rows.shape[0]):
        for k in range(3):
            lo, hi = rows.copy(), rows.copy()
            lo[i, k] -= 1e-3
            hi[i, k] += 1e-3
            fd[i, k] = (f(hi) - f(lo)) / 2e-3
    fs = np.zeros(3)
    for c in range(3):
        lo, hi = copy_desc(sd), copy_desc(sd)
        lo.spot.intensity[c] -= 0.5
        hi.spot.intensity[c] += 0.5
        fs[c] = f(rows, hi) - f(rows, lo)
    m = app.material.double().cpu().numpy()
    fdm = np.zeros_like(m)
    for i in np.flatnonzero(rows[:, scenes.MAT_COLUMN["model"]] != 0):
        for j in range(11):
            fdm[i, j] = support.fd(f, rows, i, R0 + j, 1e-4)
    pairs = (("gtex", gtex.double().cpu().numpy(), gt_ref), ("rows", app.rows.double().cpu().numpy(), fd), ("spot", app.spot.double().cpu().numpy(), fs),
             ("material", m, fdm))
    values = {}
    for n, got, want in pairs:
        assert np.abs(want).sum() > 0 and np.isfinite(got).all(), n
        values[n] = float(np.abs(got - want.reshape(got.shape)).sum() / np.abs(want).sum())
    bound = PRB_BOUND_AT.get((depth, rr), PRB_BOUND)
    print(f"{name} gaussian {gaussian} depth {depth} rr {rr}: L1 error over L1 norm " + "  ".join(f"{n} {v:.3e}" for n, v in values.items()) + f"  [{bound:g}]")
    assert bound <= 2 * PRB_BOUND and all(v <= bound for v in values.values()), values


# ------------------------------------------------------------------ 4: more than one pass of 64 samples
@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("spp", [65, 130])
def test_more_than_one_pass_of_64_samples(spp, depth, gaussian):
    """an 8 x 8 film with a second and a ragged last pass (one lane of 64, two of 64 in the third) through the forward, the path adjoint, the leaves /
    prb and forward mode.  The float64 criteria are test_path_render_matches_float64_restatement's; at max_depth 2 there is no indirect light for the
    sum's criterion to be a percent of, so the sum is held to 1 % of the light there is, the direct sum"""
    ms, sd, world = _corner("every_lobe", gaussian, W=8, H=8)
    rows = ms._albedo_host.astype(np.float64)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4) - 1.0
    what = f"every_lobe 8 x 8 spp {spp} depth {depth} gaussian {gaussian}"
    stddev = 0.5 if gaussian else None
    img_t = _fwd(ms, sd, tex, spp, SEED, depth, 5)
    img, tex_np = img_t.double().cpu().numpy(), tex.cpu().numpy()
    ref = rp.render_fwd(*world, sd, rows, tex_np, spp, SEED, depth, gaussian_stddev=stddev)
    part = (ref - rp.render_fwd(*world, sd, rows, tex_np, spp, SEED, 2, gaussian_stddev=stddev)) if depth > 2 else ref
    err, scale = np.abs(img - ref), float(ref.max())
    gnp = gimg.cpu().numpy()
    gt = ms.geom.render_bwd(sd, None, spp, SEED, gimg, max_depth=depth).double().cpu().numpy()
    gt_ref = rp.render_bwd(*world, sd, rows, spp, SEED, gnp, depth, gaussian_stddev=stddev)
    gs = np.abs(gt_ref).sum()
    print(f"{what}: over 2e-3 scale {float((err > 2e-3 * scale).mean()):.3e} [0.04]  median / scale {np.median(err) / scale:.3e} [1e-4]  "
          f"|sum difference| {abs(img.sum() - ref.sum()):.3e} [{0.01 * part.sum():.3e}]  gradient L1 {np.abs(gt - gt_ref).sum() / gs:.3e} [0.03]")
    assert part.mean() > 0.05 * ref.mean() > 0 and gs > 0
    assert (err > 2e-3 * scale).mean() <= 0.04 and np.median(err) <= 1e-4 * scale and abs(img.sum() - ref.sum()) <= 0.01 * part.sum()
    assert np.abs(gt - gt_ref).sum() <= 0.03 * gs
    # the samples of the later passes count: half of them give another image
    assert not torch.equal(img_t, _fwd(ms, sd, tex, 64, SEED, depth, 5))
    dtex, tan = gpu.tangent(ms, sd, 11)
    gpu.identity(ms, sd, tex, spp, SEED, gimg, dtex, tan, depth, 5, what + " [all blocks]")
    _, app = gpu.adjoint(ms, sd, spp, SEED, gimg, tex, depth, depth)
    _rows_directions(what, ms, sd, app, tex, spp, SEED, gimg, depth)
    a, da = (t.clone() for t in gpu.jvp(ms, sd, tex, spp, SEED, dtex, tan, depth, 5))
    b, db = gpu.jvp(ms, sd, tex, spp, SEED, dtex, tan, depth, 5)
    assert torch.equal(a, img_t) and torch.equal(b, img_t) and torch.equal(da, db) and float(da.abs().max()) > 0
    assert torch.equal(_fwd(ms, sd, tex, spp, SEED, depth, 5), img_t)
    ms._params["tex.data"] = tex[..., 0].clone()
    for t in ("path", "prb"):
        assert torch.equal(mi.render(ms, spp=spp, seed=SEED, integrator=mi.load_dict({"type": t, "max_depth": depth})).torch(), img_t), t


# ------------------------------------------------------------------ 5: prb's two-wave workgroup
@pytest.mark.parametrize("gaussian", FILMS)
@pytest.mark.parametrize("rr", [5, 8])
def test_prb_blocks_do_not_depend_on_the_workgroup_the_host_picks(rr, gaussian):
    """render_bwd_prb halves its workgroup while 4 waves' traversal stacks and path records do not fit 64 KB of LDS beside the row sums: at max_depth 8
    from a tree depth of 17 on.  ffx_bvh_info.max_depth only sizes the traversal stack — a larger value describes a deeper tree than the real one,
    and the ABI accepts up to 48 — so raising it is the one input that reaches the two-wave launch without a scene built to defeat the SAH builder:
    16 is the fullest four-wave launch (65 268 bytes), 17 and 48 launch two waves.  The blocks are the same sums in another order (1e-3 of each
    block's largest magnitude), and the forward, whose stack the field sizes too, renders the same bits"""
    ms, sd, _ = _corner("every_lobe", gaussian)
    tex, gimg = gpu.rand_tex(sd, 3), gpu.rand_gimg(sd, 4) - 1.0
    info = ms.geom.info
    own = int(info.max_depth)
    assert own < 16

    def run():
        gtex, app = ms.geom.render_bwd_prb(sd, None, 16, SEED, gimg, tex, 8, rr, material=True)
        torch.cuda.synchronize()
        return [("tex", gtex), ("rows", app.rows), ("spot", app.spot), ("material", app.material)]

    first, img = run(), _fwd(ms, sd, tex, 16, SEED, 8, rr)
    try:
        for d in (16, 17, 48):
            info.max_depth = d
            for (n, a), (_, b) in zip(first, run()):
                s, e = float(a.abs().max()), float((a - b).abs().max())
                print(f"every_lobe depth 8 rr {rr} gaussian {gaussian}, tree depth {own} given as {d} [{n}]: max |difference| {e:.3e}  1e-3 of the block's largest {1e-3 * s:.3e}")
                assert s > 0 and torch.isfinite(b).all() and e <= 1e-3 * s, (d, n)
            assert torch.equal(_fwd(ms, sd, tex, 16, SEED, 8, rr), img)
    finally:
        info.max_depth = own
