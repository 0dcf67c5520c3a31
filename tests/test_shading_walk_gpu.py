"""Every per-lane walk on shading normals and base-colour textures against the float64 walk of tests/ref_path.py, on
corner_scenes.smooth_corner: k_path_fwd / k_path_bwd, the kernel of the extra emitters in its instances, prb's blocks, forward mode and the direct-light lane
adjoints, and the bit rules that must survive.  tests/test_shading_walk_cpu.py shows that on these films and seeds the walk meets the places where
n_s differs from n_g and that each rule of the walk, swapped, misses a bound held here.  The bounds are those of the flat-scene test of the same
kernel, named at each test; every figure is printed, as a fraction of its bound, before it is asserted.  46 cases in 10 .. 14 s on an MI355X, the
slowest (the first load) 1.4 s; measured there, no figure exceeds 5 % of its bound and no pixel of any image is off by 2e-3 of its scale."""
import types

import numpy as np
import pytest
import torch

from fireflies_amd import mi, ops, scenes
from fireflies_amd import functional as Fn
from tests import corner_scenes as cs
from tests import gpu_support as gpu
from tests import ref_ambient as ra
from tests import ref_bruteforce as rb
from tests import ref_lights as rl
from tests import ref_path as rp
from tests import ref_prb
from tests import ref_sun as rs
from tests import smooth_cases as sm
from tests import support
from tests.corner_scenes import NAMES, R0
from tests.gpu_support import DEV
from tests.support import copy_desc, independent, world_arrays

pytestmark = pytest.mark.gpu
SPP, SEED = sm.SPP, sm.SEED
DSPP, DSEED = sm.DIFF_SPP, sm.DIFF_SEED
FLOOR = 0

_CASES = {}


def case(film, gaussian=False, tc=1, shadows=True, **kw):
    """smooth_corner, loaded once per (film, filter, texture channels, shadows, options), with the float64 restatements' inputs taken as
    tests/test_aov_gpu.py takes them and the images both sides have rendered so far"""
    key = (film, gaussian, tc, shadows, tuple(sorted(kw.items())))
    if key not in _CASES:
        sc, bt, uv = sm.scene(film, **kw)
        if shadows:
            ms, sd, world = gpu.load(sc, gaussian, tc)
        else:  # (gpu.load's steps without shadow rays: the emitters' geometric side shows only there)
            ms = mi.load_scene_data(sc, device=DEV, shadows=False)
            if gaussian:
                ms.rfilter = "gaussian"
            sd, world = ms.scene_desc(tex_channels=tc), world_arrays(sc)[:3]
        assert bool(sd.shadows & 1) == shadows
        tex = gpu.rand_tex(sd, 1)
        _CASES[key] = types.SimpleNamespace(sc=sc, ms=ms, sd=sd, world=world, rows=ms._albedo_host.astype(np.float64), sh=sm.shading(sc, bt, uv), tex=tex,
                                            tex_np=tex.cpu().numpy(), mats=ms.materials_arg(sd), std=0.5 if gaussian else None, refs={}, imgs={},
                                            what=f"{film} {'gaussian' if gaussian else 'box'} tc {tc} shadows {shadows} {kw}")
    return _CASES[key]


EXTRA = {"point": dict(lights=(sm.POINT,)), "spot": dict(lights=(sm.SPOT,)), "sun": dict(lights=(sm.SUN,)), "ambient": dict(ambient=sm.RADIANCE),
         "all": dict(lights=(sm.POINT, sm.SUN, sm.SPOT), ambient=sm.RADIANCE)}


def gpu_image(c, part, depth):
    """the render with the emitters of `part` ("main": none beyond projector and spot), float64 on the host"""
    if (part, depth) not in c.imgs:
        kw = {}
        if part != "main":
            e = EXTRA[part]
            if "lights" in e:
                kw["lights"] = ops.pack_lights(list(e["lights"])).to(DEV)
                if any(l is sm.SUN for l in e["lights"]):
                    kw["lights_directional"] = True
            if "ambient" in e:
                kw["ambient"] = e["ambient"]
        c.imgs[(part, depth)] = c.ms.geom.render_fwd(c.sd, c.mats, c.tex, SPP, SEED, max_depth=depth, **kw).double().cpu().numpy()
    return c.imgs[(part, depth)]


def ref_image(c, part, depth):
    """the float64 restatement of the main emitters' image, or of what the emitters of `part` add to it"""
    if (part, depth) not in c.refs:
        a, b = (*c.world, c.sd, c.rows), (SPP, SEED, depth)
        if part == "main":
            r = rp.render_fwd(*a, c.tex_np, *b, gaussian_stddev=c.std, **c.sh)
        elif part in ("point", "spot"):
            r = rl.render_lights(*a, sm.host_table(*EXTRA[part]["lights"]), *b, gaussian_stddev=c.std, **c.sh)
        elif part == "sun":
            r = rs.render_sun(*a, sm.host_table(sm.SUN), *b, gaussian_stddev=c.std, **c.sh)
        elif part == "ambient":
            r = ra.render_ambient(*a, sm.RADIANCE, *b, gaussian_stddev=c.std, **c.sh)
        else:  # (the render is linear in the emitters)
            r = sum(ref_image(c, p, depth) for p in ("point", "spot", "sun", "ambient"))
        c.refs[(part, depth)] = r
    return c.refs[(part, depth)]


# ------------------------------------------------------------------ 1. the path forward and its texture adjoint
PATH_CASES = [(3, 1, False, "12x12", True, {}), (4, 3, True, "12x12", True, {}), (3, 3, True, "13x11", True, {}), (4, 1, False, "13x11", True, {}),
              (4, 1, False, "12x12", False, {}), (4, 1, True, "13x11", True, {"lambert_only": True}), (3, 1, True, "12x12", True, {"every_lobe": True}),
              (4, 1, False, "12x12", True, {"smooth": False})]


@pytest.mark.parametrize("depth,tc,gaussian,film,shadows,kw", PATH_CASES,
                         ids=[f"depth{d}-tc{t}-{'gaussian' if g else 'box'}-{f}{'' if s else '-unshadowed'}{''.join('-' + k for k in kw)}" for d, t, g, f, s, kw in PATH_CASES])
def test_path_render_and_its_texture_adjoint_match_the_float64_walk(depth, tc, gaussian, film, shadows, kw):
    """tests/test_path_gpu.py test_path_render_matches_float64_restatement's bounds: at most 0.04 of the pixels off by more than 2e-3 of the scale, the
    median within 1e-4 of it, the sum within 1 % of the indirect part, the adjoint's L1 error within 0.03.  The last case is the flat twin: the same
    geometry without shading normals"""
    c = case(film, gaussian, tc, shadows, **kw)
    assert int(c.sd.mat_stride or 3) == (3 if kw.get("lambert_only") else 16) and any(c.sh["smooth"]) == kw.get("smooth", True)
    img, ref = gpu_image(c, "main", depth), ref_image(c, "main", depth)
    indirect = ref - ref_image(c, "main", 2)
    assert indirect.mean() > 0.05 * ref.mean() > 0  # (the bounces matter in this scene)
    independent(f"path {c.what} depth {depth}", img, ref, float(ref.max()), float(indirect.sum()))
    gimg = np.where(np.random.default_rng(2).random(img.shape) < 0.5, -1.0, 1.0).astype(np.float32) / img.size
    gt = c.ms.geom.render_bwd(c.sd, c.mats, SPP, SEED, torch.from_numpy(gimg).to(DEV), max_depth=depth).double().cpu().numpy()
    gt_ref = rp.render_bwd(*c.world, c.sd, c.rows, SPP, SEED, gimg, depth, gaussian_stddev=c.std, **c.sh)
    e, s = np.abs(gt - gt_ref).sum(), np.abs(gt_ref).sum()
    print(f"texture adjoint: L1 error {e / s / 0.03:.2e} of its bound (0.03 of {s:.4g})")
    assert s > 0 and e <= 0.03 * s


# ------------------------------------------------------------------ 2. point light, spot, sun and the constant emitter, each and all at once
@pytest.mark.parametrize("depth", sm.DEPTHS)
@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
@pytest.mark.parametrize("film,shadows", [("12x12", True), ("13x11", True), ("12x12", False)], ids=["12x12", "13x11", "12x12-unshadowed"])
def test_what_every_extra_emitter_adds_matches_the_float64_walk(film, shadows, gaussian, depth):
    """k_lights_fwd's instances — plain (point, spot), DIR (sun), AMB (the constant emitter, closing ray included) and DIR with AMB (all at
    once): image minus unlit image against the restatement of that part, under the three conditions of tests/support.py's `independent` with the sums the flat tests of each kernel use — the part itself at direct light and for the constant emitter, the part's indirect share
    through the bounces of the lights and the sun"""
    c = case(film, gaussian, 1, shadows)
    plain, main_ref = gpu_image(c, "main", depth), ref_image(c, "main", depth)
    for part in ("point", "spot", "sun", "ambient", "all"):
        got, ref = gpu_image(c, part, depth) - plain, ref_image(c, part, depth)
        assert ref.mean() > 0.05 * (main_ref + ref).mean()
        part_sum = ref.sum()
        if depth > 2 and part != "ambient":
            part_sum = (ref - ref_image(c, part, 2)).sum()
            assert part_sum / ref.size > 0.05 * ref_image(c, part, 2).mean() > 0  # (the bounces carry this emitter's light)
        independent(f"{part} {c.what} depth {depth}", got, ref, float((main_ref + ref).max()), float(part_sum))


# ------------------------------------------------------------------ 3. prb's blocks against frozen float64 differences
def _prb_case(depth, rr, gaussian, **kw):
    c = case(sm.DIFF_FILM, gaussian, 1, True, **kw)
    gimg = gpu.rand_gimg(c.sd, 2)
    gimg_np = gimg.double().cpu().numpy()
    gtex, app = c.ms.geom.render_bwd_prb(c.sd, None, DSPP, DSEED, gimg, c.tex, depth, rr, material=True)
    sh = {k: v for k, v in c.sh.items() if k != "base_tex"}

    def channels(r, sd_=c.sd, bt=None):
        """<frozen float64 image, gimg> per colour channel: rows r, the roulette of the unperturbed rows and textures"""
        img = ref_prb.render_fwd_frozen(*c.world, sd_, r, c.rows, c.tex_np, DSPP, DSEED, depth, rr, gaussian_stddev=c.std, base_tex=bt or c.sh["base_tex"],
                                        base_tex0=c.sh["base_tex"], **sh)
        return (img * gimg_np).sum((0, 1))

    return c, gimg_np, gtex, app, channels


def _l1(what, got, want):
    e, s = np.abs(got - want).sum(), np.abs(want).sum()
    print(f"{what}: L1 error {e / s / 0.03:.2e} of its bound (0.03 of {s:.4g})")
    assert s > 0 and e <= 0.03 * s, (what, got, want)


@pytest.mark.parametrize("depth,rr,gaussian,kw", [(3, 1, True, {}), (4, 2, False, {"every_lobe": True})], ids=["depth3-rr1-gaussian", "depth4-rr2-box-every_lobe"])
def test_prb_rows_spot_and_material_match_frozen_float64_differences(depth, rr, gaussian, kw):
    """tests/test_prb_gpu.py test_blocks_match_the_float64_restatement's bound — every block, and the texture gradient of the same call, within 3 % of
    its L1 norm — against differences of tests/ref_prb.py's frozen render: rows by central differences at h = 1e-3, the spot by +- 0.5 (the image is
    linear in it), the material columns by support.fd4 at h = 1e-3"""
    c, gimg_np, gtex, app, channels = _prb_case(depth, rr, gaussian, **kw)
    with ref_prb.SameRays():
        _l1("gtex", gtex.double().cpu().numpy(), rp.render_bwd(*c.world, c.sd, c.rows, DSPP, DSEED, gimg_np, depth, rr, gaussian_stddev=c.std, **c.sh))
        f = lambda r, sd_=c.sd: float(channels(r, sd_).sum())  # noqa: E731
        g = app.rows.double().cpu().numpy()
        assert float(np.abs(g[FLOOR]).max()) == 0  # (the floor's colour is its texture)
        fd = np.zeros_like(g)
        for i in range(1, c.rows.shape[0]):
            for k in range(3):
                lo, hi = c.rows.copy(), c.rows.copy()
                lo[i, k] -= 1e-3
                hi[i, k] += 1e-3
                fd[i, k] = (f(hi) - f(lo)) / 2e-3
        _l1("rows", g, fd)
        fs = np.zeros(3)
        for ch in range(3):
            lo, hi = copy_desc(c.sd), copy_desc(c.sd)
            lo.spot.intensity[ch] -= 0.5
            hi.spot.intensity[ch] += 0.5
            fs[ch] = f(c.rows, hi) - f(c.rows, lo)
        _l1("spot", app.spot.double().cpu().numpy(), fs)
        m = app.material.double().cpu().numpy()
        lam = c.rows[:, scenes.MAT_COLUMN["model"]] == 0
        assert lam.sum() == (1 if kw else 2) and np.abs(m[lam]).max() == 0
        fdm = np.zeros_like(m)
        for i in np.flatnonzero(~lam):
            for j in range(11):
                fdm[i, j] = support.fd4(f, c.rows, i, R0 + j, 1e-3)
        _l1("material", m, fdm)


@pytest.mark.parametrize("depth,rr,gaussian", [(3, 1, False), (4, 2, True)], ids=["depth3-rr1-box", "depth4-rr2-gaussian"])
def test_prb_base_texture_matches_frozen_float64_differences(depth, rr, gaussian):
    """the same bound for base_tex[0], texel by texel.  The floor's row has no tint term (spec_tint, sheen and metallic are 0), so channel c of the
    image depends on channel c of the texture alone — checked here on one texel — and one central difference of a texel's three channels at once
    gives its three derivatives, each from its own channel of the loss.  Central differences are exact: the floor is flat, so a path meets it at
    most at every other vertex and the image is at most quadratic in a texel"""
    c, gimg_np, _, app, channels = _prb_case(depth, rr, gaussian)
    row = c.rows[FLOOR]
    assert row[15] == 1 and all(row[scenes.MAT_COLUMN[k]] == 0 for k in ("spec_tint", "sheen", "metallic"))
    bt0 = c.sh["base_tex"][0]
    g = app.base_tex[0].double().cpu().numpy()
    assert g.shape == bt0.shape
    h = 1e-3
    with ref_prb.SameRays():
        base = channels(c.rows)
        one = bt0.copy()
        one[3, 4, 0] += 0.1
        moved = channels(c.rows, bt=[one])
        assert moved[0] != base[0] and moved[1] == base[1] and moved[2] == base[2]
        fd = np.zeros_like(g)
        for y in range(bt0.shape[0]):
            for x in range(bt0.shape[1]):
                lo, hi = bt0.copy(), bt0.copy()
                lo[y, x] -= h
                hi[y, x] += h
                fd[y, x] = (channels(c.rows, bt=[hi]) - channels(c.rows, bt=[lo])) / (2 * h)
    assert (np.abs(fd) > 0).mean() > 0.9  # (the uv run beyond [0, 1]: the floor wraps the whole texture)
    _l1("base_tex[0]", g, fd)


# ------------------------------------------------------------------ 4. forward mode
@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
@pytest.mark.parametrize("depth,rr", [(2, 5), (3, 1)])
def test_every_pixel_against_the_float64_tangent(depth, rr, gaussian):
    """tests/test_jvp_gpu.py test_every_pixel_against_the_float64_tangent's rule: per pixel 1e-4 of max |dimg_ref|, at most 2e-4 of the pixels beyond
    (64 pixels: none) — with tangents in the rows, the BSDF columns, the projector texture, the spot and the floor's base-colour texture"""
    c = case(sm.DIFF_FILM, gaussian, 1, True, every_lobe=True)
    W, H = sm.DIFF_FILM
    rng = np.random.default_rng(2)
    drows = ref_prb.interior_material_tangent(c.rows, rng)
    drows[:, :3] = rng.uniform(0.5, 1.5, (c.rows.shape[0], 3))
    drows[FLOOR, :3] = 0.0  # (the floor's colour is its texture: the row's has no say)
    dtex = rng.uniform(-1, 1, c.tex_np.shape).astype(np.float32)
    dspot = np.array([0.5, 2.0, 1.25], np.float32)
    dbt = rng.uniform(-1, 1, c.sh["base_tex"][0].shape).astype(np.float32)
    with ref_prb.SameRays():
        ref = ref_prb.float64_tangent(c.world, c.sd, c.rows, c.tex_np, DSPP, DSEED, depth, rr, c.std, drows=drows, dtex=dtex, dspot=dspot, dbase_tex=[dbt], **c.sh)
        only_bt = ref_prb.float64_tangent(c.world, c.sd, c.rows, c.tex_np, DSPP, DSEED, depth, rr, c.std, dbase_tex=[dbt], **c.sh)
    assert np.abs(only_bt).max() > 0.05 * np.abs(ref).max()  # (the texture's tangent is a visible part of the whole)
    tan = ops.AppearanceGrad(gpu.dev(drows[:, :3]), gpu.dev(dspot), [gpu.dev(dbt)], gpu.dev(drows[:, R0:R0 + 11]))
    _, dimg = gpu.jvp(c.ms, c.sd, c.tex, DSPP, DSEED, gpu.dev(dtex), tan, depth, rr)
    err = np.abs(dimg.double().cpu().numpy() - ref).max(-1)
    scale = np.abs(ref).max()
    bad, allowed = int((err > 1e-4 * scale).sum()), int(2e-4 * W * H)
    print(f"depth {depth} rr {rr} gaussian {gaussian}: max err {err.max() / (1e-4 * scale):.2e} of its bound (1e-4 of {scale:.4g}), pixels over {bad} (allowed {allowed}), "
          f"median err {np.median(err):.3e}")
    assert scale > 0 and bad <= allowed


@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
@pytest.mark.parametrize("depth,rr", [(2, 5), (3, 1), (4, 2)])
def test_dot_product_identity_on_shading_normals_and_textures(depth, rr, gaussian):
    """gpu_support.identity: forward mode against render_bwd(appearance, material) at direct light and render_bwd_prb through the bounces"""
    c = case("13x11", gaussian, 1, True, every_lobe=True)
    tex, gimg = gpu.rand_tex(c.sd, 3), gpu.rand_gimg(c.sd, 4) - 1.0
    dtex, tan = gpu.tangent(c.ms, c.sd, 11)
    assert len(tan.base_tex) == 1 and tan.material is not None
    gpu.identity(c.ms, c.sd, tex, SPP, SEED, gimg, dtex, tan, depth, rr, f"{c.what} depth {depth} rr {rr} [all blocks]")
    gpu.identity(c.ms, c.sd, tex, SPP, SEED, gimg, *gpu.one_block(dtex, tan, "base_tex[0]"), depth, rr, f"{c.what} depth {depth} rr {rr} [base_tex[0]]")


# ------------------------------------------------------------------ 5. the direct-light lane adjoints on a smooth shape
@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
def test_direct_light_lane_adjoints_match_float64_differences(gaussian):
    """k_render_bwd_appearance / k_render_bwd_material: tests/test_material_grad_gpu.py test_every_parameter_matches_the_float64_restatement's bound,
    2e-3 of a column's largest difference + 1e-9, for the BSDF columns (support.fd at h = 1e-4 of ref_bruteforce.render_fwd with shading normals and
    the texture) and, a column being a colour channel there, for the rows' colours"""
    c = case(sm.DIFF_FILM, gaussian, 1, True, every_lobe=True)
    gimg = gpu.rand_gimg(c.sd, 2)
    gimg_np = gimg.double().cpu().numpy()
    _, app = c.ms.geom.render_bwd(c.sd, None, DSPP, DSEED, gimg, appearance=True, tex=c.tex, material=True)

    def f(r):
        return float((rb.render_fwd(*c.world, c.sd, r, c.tex_np, DSPP, DSEED, gaussian_stddev=c.std, **c.sh) * gimg_np).sum())

    g, m = app.rows.double().cpu().numpy(), app.material.double().cpu().numpy()
    lam = c.rows[:, scenes.MAT_COLUMN["model"]] == 0
    assert lam.sum() == 1 and np.abs(m[lam]).max() == 0 and np.abs(g[FLOOR]).max() == 0
    fd, fdm = np.zeros_like(g), np.zeros_like(m)
    for i in range(1, c.rows.shape[0]):
        for k in range(3):
            fd[i, k] = support.fd(f, c.rows, i, k, 1e-4)
    for i in np.flatnonzero(~lam):
        for j in range(11):
            fdm[i, j] = support.fd(f, c.rows, i, R0 + j, 1e-4)
    for name, got, want in [(f"colour {k}", g[:, k], fd[:, k]) for k in range(3)] + [(NAMES[j], m[:, j], fdm[:, j]) for j in range(11)]:
        bound = 2e-3 * np.abs(want).max() + 1e-9
        print(f"{name:16s} max |g - fd| {np.abs(got - want).max() / bound:.2e} of its bound ({bound:.3e})")
    for name, got, want in [(f"colour {k}", g[:, k], fd[:, k]) for k in range(3)] + [(NAMES[j], m[:, j], fdm[:, j]) for j in range(11)]:
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 1e-9, (name, got, want)
    assert (np.abs(m) > 0).sum() >= 16 and np.abs(m[3]).max() > 0  # (the ball's row among them)


# ------------------------------------------------------------------ 6. bit rules that must survive
@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
def test_bit_rules(gaussian):
    c = case("13x11", gaussian, 1, True)
    t = ops.pack_lights([sm.POINT, sm.SUN, sm.SPOT]).to(DEV)
    c.ms._params["tex.data"] = c.tex[..., 0].clone()
    for depth, rr in ((3, 5), (4, 1)):
        a = c.ms.geom.render_fwd(c.sd, c.mats, c.tex, SPP, SEED, max_depth=depth, rr_depth=rr, lights=t, lights_directional=True, ambient=sm.RADIANCE).clone()
        b = c.ms.geom.render_fwd(c.sd, c.mats, c.tex, SPP, SEED, max_depth=depth, rr_depth=rr, lights=t, lights_directional=True, ambient=sm.RADIANCE)
        assert float(a.abs().max()) > 0 and torch.equal(a, b)  # (two runs are equal)
        path = mi.render(c.ms, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "path", "max_depth": depth, "rr_depth": rr})).torch().clone()
        prb = mi.render(c.ms, spp=SPP, seed=SEED, integrator=mi.load_dict({"type": "prb", "max_depth": depth, "rr_depth": rr})).torch()
        assert float(path.abs().max()) > 0 and torch.equal(path, prb)  # (the prb forward is the path forward)
        assert torch.equal(c.ms.geom.render_fwd(c.sd, None, c.tex, SPP, SEED, max_depth=depth, rr_depth=rr), path)
        assert torch.equal(Fn.render(c.tex, c.ms.geom, c.sd, None, SPP, SEED, max_depth=depth, rr_depth=rr), path)


@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
def test_flat_shapes_beside_a_smooth_one_render_the_image_of_the_flat_load(gaussian):
    """with every smooth flag false a load carries no normal table at all; the rule that can break is the flat shape in a scene that has one.  The
    same flat geometry, once with a small smooth quad under the floor that no ray reaches and once with that quad flat: the same image, bit for bit,
    and it is not the smooth ball's"""
    flat, _, _ = sm.scene("13x11", smooth=False)
    hidden = cs._quad([[0.99, 0.99, -0.05], [1.01, 0.99, -0.05], [1.01, 1.01, -0.05], [0.99, 1.01, -0.05]])
    imgs = []
    for smooth in (True, False):
        sc = scenes.SceneData(flat.meshes + [scenes.MeshData("mesh-Hidden", hidden, cs.QUAD, (0.5, 0.5, 0.5), material="mat-Hidden", smooth=smooth)],
                              flat.camera, flat.projector, flat.spot, 1.0)
        ms, sd, _ = gpu.load(sc, gaussian, 1)
        assert (ms.geom._smooth is not None) == smooth
        tex = gpu.rand_tex(sd, 1)
        imgs.append([ms.geom.render_fwd(sd, ms.materials_arg(sd), tex, SPP, SEED, max_depth=d).clone() for d in (2, 4)])
    for a, b in zip(*imgs):
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
    c = case("13x11", gaussian, 1, True)
    assert not np.array_equal(gpu_image(c, "main", 4), imgs[0][1].double().cpu().numpy())
