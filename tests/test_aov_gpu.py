"""FFX_RENDER_AOV on the GPU: the block against K7 (ids exact), against the float64 restatement tests/ref_aov.py on both films, against
the image it was rendered beside, bit-for-bit repeatability, mi.render end to end and one full-size render."""
import numpy as np
import pytest
import torch

from fireflies_amd import mi, ops, scenes, workloads
from tests import ref_aov
from tests import ref_bruteforce as rb
from tests.corner_scenes import aov_corner
from tests.gpu_support import DEV
from tests.support import outlier_rule, world_arrays

pytestmark = pytest.mark.gpu
CH = ops.AOV_CHANNELS
FILMS = [(37, 29), (64, 64)]
SPPS = [1, 4, 32, 33, 100]


_CACHE = {}


def _case(film, lambert_only=False, gaussian=False):
    """one scene per (film, table): the loaded scene, its description, the world triangles and the float64 reference's inputs, shared by the tests"""
    key = (film, lambert_only, gaussian)
    if key not in _CACHE:
        sc, base_tex, uv = aov_corner(*film, lambert_only=lambert_only)
        ms = mi.load_scene_data(sc, device=DEV, shadows=True)
        if gaussian:
            ms.rfilter = "gaussian"
        sd = ms.scene_desc(tex_channels=1)
        world = world_arrays(sc)[:3]
        vuv = None
        if uv is not None:
            vuv = np.zeros((world[0].shape[0], 2))
            vuv[:4] = uv
        ref = dict(mats=ms._albedo_host.astype(np.float64), smooth=[m.smooth for m in sc.meshes], vert_uv=vuv,
                   base_tex=None if base_tex is None else [base_tex.astype(np.float64)])
        g = torch.Generator().manual_seed(3)
        tex = torch.rand((sd.proj.tex_h, sd.proj.tex_w, 1), generator=g).to(DEV)
        _CACHE[key] = (sc, ms, sd, world, ref, tex)
    return _CACHE[key]


_TRACED, _SAMPLES = {}, {}


def _ref_block(film, lambert_only, gaussian, spp, seed):
    """the float64 block; the rays' hits are computed once per (film, spp, seed) — both tables share geometry and camera — and the per-sample values
    once per table, for both films"""
    _, _, sd, world, ref, _ = _case(film, lambert_only, gaussian)
    tk = (film, spp, seed)
    if tk not in _TRACED:
        _TRACED[tk] = ref_aov.trace(world[0], world[1], sd.cam, spp, seed)
    sk = (film, lambert_only, spp, seed)
    if sk not in _SAMPLES:
        _SAMPLES[sk] = ref_aov.aov_samples(*world, sd.cam, spp, seed, ref["mats"], ref["smooth"], ref["vert_uv"], ref["base_tex"], traced=_TRACED[tk])
    return ref_aov.film(_SAMPLES[sk], sd.cam, spp, seed, 0.5 if gaussian else None)


def _aov(ms, sd, tex, spp, seed, **kw):
    return ms.geom.render_aov(sd, ms.materials_arg(sd), tex, spp, seed, **kw)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("spp", SPPS)
def test_depth_and_ids_against_k7(film, spp):
    _, ms, sd, _, _, tex = _case(film)
    seed = 11
    _, a = _aov(ms, sd, tex, spp, seed)
    t, shape, prim = ms.geom.trace_primary(sd.cam, spp=spp, jitter=1, seed=seed)
    H, W = sd.cam.height, sd.cam.width
    t = t.view(H, W, spp)
    if spp == 1:
        # (a sample that misses is 0 in every channel of the block; K7 writes -1 ids there)
        shape_f, prim_f = shape.view(H, W).clamp_min(0).float(), prim.view(H, W).clamp_min(0).float()
        print("1 spp: depth / shape / prim differences:", int((a[..., 0] != t[..., 0]).sum()), int((a[..., 15] != shape_f).sum()), int((a[..., 16] != prim_f).sum()))
        assert torch.equal(a[..., 0], t[..., 0])
        assert torch.equal(a[..., 15], shape_f)
        assert torch.equal(a[..., 16], prim_f)
        assert torch.equal(a[..., 0] == 0, shape.view(H, W) < 0)
        assert (shape >= 0).any() and (shape < 0).any()  # (hits and misses both)
    else:
        want = t.double().mean(-1)
        rel = ((a[..., 0].double() - want).abs() / want.abs().clamp_min(1e-30))[want > 0]
        print(f"{spp} spp: depth vs mean of K7's t: max rel {float(rel.max()):.3e}")
        assert float(rel.max()) <= 1e-6
        assert torch.equal(a[..., 0] == 0, want == 0)


@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
@pytest.mark.parametrize("lambert_only", [False, True], ids=["rows", "stride3"])
@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("spp", SPPS)
def test_every_channel_against_the_float64_restatement(film, spp, lambert_only, gaussian):
    _, ms, sd, _, _, tex = _case(film, lambert_only, gaussian)
    assert int(sd.mat_stride or 3) == (3 if lambert_only else 16)
    seed = 7
    _, a = _aov(ms, sd, tex, spp, seed)
    got, want = a.double().cpu().numpy(), _ref_block(film, lambert_only, gaussian, spp, seed)
    assert np.isfinite(got).all()
    for name, (first, n) in CH.items():
        w = want[..., first:first + n]
        scale = float(w.max() - w.min())
        if name == "uv" and lambert_only:
            assert scale == 0 and not got[..., first:first + n].any()  # (no slot_uv: zeros)
            continue
        assert scale > 0, name
        outlier_rule(f"{name} ({'gaussian' if gaussian else 'box'}, {spp} spp)", got[..., first:first + n], w, scale, spp)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_the_block_describes_the_samples_of_the_image(film):
    """spot only, Lambert rows, no shadows, 1 spp, box film: the image recomputed in float64 from position, sh_normal and albedo with DESIGN 4.3's spot
    formula (the normal faced to the viewer here) is render_fwd's image"""
    sc, _, _ = aov_corner(*film, lambert_only=True)
    sc = scenes.SceneData(sc.meshes, sc.camera, None, sc.spot, 1.0)
    ms = mi.load_scene_data(sc, device=DEV, shadows=False)
    sd = ms.scene_desc(tex_channels=1)
    assert not sd.proj.enabled and not (sd.shadows & 1)
    seed = 5
    img, a = _aov(ms, sd, None, 1, seed)
    a = a.double().cpu().numpy()
    P, ns, alb, hit = a[..., 1:4], a[..., 7:10], a[..., 12:15], a[..., 0:1] > 0
    tw = rb._m(sd.cam.to_world, 4)
    wv = tw[:3, 3] - P
    wv /= np.maximum(np.linalg.norm(wv, axis=-1, keepdims=True), 1e-300)
    ns = np.where((ns * wv).sum(-1, keepdims=True) < 0, -ns, ns)
    sw = rb._m(sd.spot.to_world, 4)
    spos, axis = sw[:3, 3], sw[:3, 2]
    wi = spos - P
    d2 = (wi * wi).sum(-1, keepdims=True)
    wi = wi / np.sqrt(np.maximum(d2, 1e-300))
    cos_s = (ns * wi).sum(-1, keepdims=True)
    cos_l = -(wi * axis).sum(-1, keepdims=True)
    cut, beam = np.deg2rad(sd.spot.cutoff_deg), np.deg2rad(sd.spot.beam_width_deg)
    ang = np.arccos(np.clip(cos_l, -1, 1))
    fall = np.where(ang <= beam, 1.0, np.where(ang < cut, (cut - ang) / (cut - beam), 0.0))
    inten = np.asarray(list(sd.spot.intensity), np.float64)
    rad = alb / np.pi * inten * fall * np.maximum(cos_s, 0.0) / np.maximum(d2, 1e-300)
    want = np.where(hit & (cos_s > 0), rad, 0.0)
    got = img.double().cpu().numpy()
    # the geometric side test of DESIGN 4.3 (the emitter on the viewer's geometric side) needs the geometric normal: from its channel
    ng = a[..., 4:7]
    ng = np.where((ng * wv).sum(-1, keepdims=True) < 0, -ng, ng)
    want = np.where((ng * wi).sum(-1, keepdims=True) > 0, want, 0.0)
    scale = float(got.max())
    assert scale > 0
    outlier_rule("image from the block", got, want, scale, 1)


@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
def test_nothing_else_moves_and_it_repeats(gaussian, monkeypatch):
    _, ms, sd, _, _, tex = _case((37, 29), False, gaussian)
    mats = ms.materials_arg(sd)
    for spp in (4, 33):
        for md in (2, 3):
            img, a = _aov(ms, sd, tex, spp, 9, max_depth=md)
            plain = ms.geom.render_fwd(sd, mats, tex, spp, 9, max_depth=md)
            print(f"{spp} spp, max_depth {md}: image bits differ at {int((img != plain).sum())} floats")
            assert torch.equal(img, plain)
            img2, a2 = _aov(ms, sd, tex, spp, 9, max_depth=md)
            assert torch.equal(img2, img) and torch.equal(a2, a)
            if md == 2:
                first = a.clone()
            else:
                assert torch.equal(a, first)  # (the path bits choose the image only)
        monkeypatch.setenv("FFX_BINS", "0")
        _, a3 = _aov(ms, sd, tex, spp, 9)
        monkeypatch.delenv("FFX_BINS")
        print(f"{spp} spp: tree walk vs bins: block bits differ at {int((a3 != first).sum())} floats")
        assert torch.equal(a3, first)


def test_mi_render_end_to_end():
    sc, ms, sd, _, _, tex = _case((37, 29))
    ms._params["tex.data"] = tex[..., 0].clone()
    inner = mi.load_dict({"type": "path", "max_depth": 3})
    it = mi.load_dict({"type": "aov", "aovs": "nn:sh_normal,dd.y:depth,id:shape_index,alb:albedo", "img": {"type": "path", "max_depth": 3}})
    out = mi.render(ms, spp=4, seed=3, integrator=it).torch()
    assert tuple(out.shape) == (29, 37, 3 + 1 + 1 + 3 + 3) and len(it.aov_names()) == out.shape[-1]
    _, block = _aov(ms, ms.scene_desc(tex_channels=1), tex, 4, 3)
    assert torch.equal(out[..., 0:3], block[..., 7:10]) and torch.equal(out[..., 3], block[..., 0]) and torch.equal(out[..., 4], block[..., 15])
    assert torch.equal(out[..., 5:8], block[..., 12:15])
    rgb = mi.render(ms, spp=4, seed=3, integrator=inner).torch()
    assert torch.equal(out[..., 8:], rgb)
    # with a texture that requires grad: the same image, the same gradient through the RGB tail, none through the block
    t1 = tex[..., 0].clone().requires_grad_(True)
    ms._params["tex.data"] = t1
    out_g = mi.render(ms, spp=4, seed=3, integrator=it).torch()
    assert out_g.requires_grad and torch.equal(out_g.detach()[..., 8:], rgb) and torch.equal(out_g.detach()[..., :8], out[..., :8])
    g = torch.Generator().manual_seed(1)
    w = torch.rand(out_g.shape, generator=g).to(DEV)
    (out_g * w).sum().backward()
    t2 = tex[..., 0].clone().requires_grad_(True)
    ms._params["tex.data"] = t2
    (mi.render(ms, spp=4, seed=3, integrator=inner).torch() * w[..., 8:]).sum().backward()
    print("d/d tex through the aov wrapper vs without: max |diff|", float((t1.grad - t2.grad).abs().max()), "scale", float(t2.grad.abs().max()))
    assert float(t2.grad.abs().max()) > 0 and torch.allclose(t1.grad, t2.grad, rtol=1e-5, atol=1e-6 * float(t2.grad.abs().max()))
    only = mi.render(ms, spp=4, seed=3, integrator=mi.load_dict({"type": "aov", "aovs": "d:depth"})).torch()
    assert not only.requires_grad and tuple(only.shape) == (29, 37, 1)
    with pytest.raises(ValueError, match="fp16"):
        mi.render(ms, spp=4, fp16=True, integrator=it)
    # a loaded scene under the gaussian film
    _, mg, sdg, _, _, texg = _case((37, 29), False, True)
    mg._params["tex.data"] = texg[..., 0].clone()
    og = mi.render(mg, spp=4, seed=3, integrator=mi.load_dict({"type": "aov", "aovs": "p:position", "img": {"type": "direct"}})).torch()
    want = _ref_block((37, 29), False, True, 4, 3)[..., 1:4]
    outlier_rule("mi.render position (gaussian)", og[..., :3].double().cpu().numpy(), want, float(want.max() - want.min()), 4)
    assert torch.equal(og[..., 3:], mi.render(mg, spp=4, seed=3).torch())


@pytest.mark.parametrize("gaussian", [False, True], ids=["box", "gaussian"])
def test_full_size_once(gaussian):
    wl = workloads.vocalfold(device=DEV, width=512, height=512)
    ms = wl.mi_scene
    if gaussian:
        ms.rfilter = "gaussian"
    tex = workloads.build_texture(wl).detach()
    sd = ms.scene_desc(tex_channels=1)
    tex3 = tex.unsqueeze(-1).contiguous()
    img, a = _aov(ms, sd, tex3, 64, 1)
    assert torch.isfinite(a).all() and torch.isfinite(img).all()
    t, shape, _ = ms.geom.trace_primary(sd.cam, spp=64, jitter=1, seed=1)
    if not gaussian:
        want = t.view(512, 512, 64).double().mean(-1)
        rel = ((a[..., 0].double() - want).abs() / want.clamp_min(1e-30))[want > 0]
        print("512^2 x 64: depth vs mean of K7's t: max rel", float(rel.max()))
        assert float(rel.max()) <= 1e-6
    else:  # K7's t through the gaussian film of the float64 restatement: sum(w t) / sum(w) over the same samples
        # (a band of the film: every pixel of rows 200 .. 263 receives from rows 198 .. 265 only; the whole film's splat takes a minute on the host)
        y0, y1 = 198, 266
        x, y, fx, fy = rb._film_positions(512, 512, 64, 1)
        rows = (y >= y0) & (y < y1)
        tt = t.double().cpu().numpy()[rows]
        num, den = np.zeros((y1 - y0, 512)), np.zeros((y1 - y0, 512))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                tx, ty = x[rows] + dx, y[rows] + dy - y0
                ok = (tx >= 0) & (tx < 512) & (ty >= 0) & (ty < y1 - y0)
                w = np.where(ok, rb._gaussian((tx + 0.5) - fx[rows], 0.5) * rb._gaussian((ty + y0 + 0.5) - fy[rows], 0.5), 0.0)
                np.add.at(num, (np.clip(ty, 0, y1 - y0 - 1), np.clip(tx, 0, 511)), w * tt)
                np.add.at(den, (np.clip(ty, 0, y1 - y0 - 1), np.clip(tx, 0, 511)), w)
        want = (num / den)[2:-2]
        got = a[200:264, :, 0].double().cpu().numpy()
        rel = np.abs(got - want)[want > 0] / want[want > 0]
        print("512^2 x 64 gaussian: depth vs K7's t through the film (rows 200 .. 263): max rel", float(rel.max()))
        # (the kernels' weights are rf_weights' two-exponential form, 1e-6 of a weight off the five expf of the restatement: DESIGN 4.2)
        assert float(rel.max()) <= 1e-5
    _, a1 = _aov(ms, sd, tex3, 1, 1)
    _, s1, _ = ms.geom.trace_primary(sd.cam, spp=1, jitter=1, seed=1)
    if not gaussian:
        assert torch.equal(a1[..., 15], s1.view(512, 512).clamp_min(0).float())
