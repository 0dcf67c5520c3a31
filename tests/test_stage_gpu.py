"""The direct-light render kernels under emitters that stand apart from the camera (tests/stage_scenes.py; the scenes' own facts and the
oracle's agreement with the float64 restatement on them: tests/test_stage_cpu.py).  Every render test with a projector used to build its
scene from scenes.vocalfold / scenes.colon, whose emitters stand beside the camera: no cast shadow under the projector's envelope, no
geometry behind or beside an emitter's apex, a square texture, a rigid spot.  Here: images against the oracle (conftest.assert_image_close,
hard bound 1.5 scale / spp), gradients against the oracle's ((err > 1e-3 gs) on at most 1e-3 of the texels, none above 0.1 gs), and the
project's bit-for-bit invariants (envelopes, bins, walks, the plain-scene instance change nothing).  Run with `-m gpu`.

Sizes: 96 x 80 for the two base scenes (12 x 10 camera tiles), 64 x 48 for the parametrised variants; 64 samples per pixel (one wave per
pixel: the packet kernel) and 16 (the pixel-block kernel).

Observed on an MI355X (every comparison prints its share and its worst channel): in all 112 comparisons of this module — 52 images, 60
gradients — NOT ONE pixel channel is off by more than `rel` of the scale and not one texel by more than 1e-3 of the gradient's: share 0 against
the bounds 1e-3 (box film), 0.02 (gaussian film) and 1e-3 (gradients), which therefore stay where the suite had them.  Worst image channel
1.9e-5 of the scale (facing, the 3-degree cone, whose transition band is 0.75 degrees wide), 4.8e-6 elsewhere; worst texel 2.7e-6 of the
gradient's scale.  No sample flipped on any shadow or silhouette edge of these scenes; every torch.equal of the module held.
"""
import os

import numpy as np
import pytest
import torch

from fireflies_amd import ops, scene_desc, scenes
from tests import stage_scenes as ss
from tests.conftest import assert_image_close
from tests.gpu_support import bin_headers, dev, envelope, grad_close, host, pair
from tests.support import material_rows

pytestmark = pytest.mark.gpu

FRAC_BOX, FRAC_GAUSS = 1e-3, 0.02  # the widest shares the suite allows a scene with a cast shadow (box) / the small gaussian films
FRAC_GRAD = 1e-3  # ... and a texture gradient
KNOBS = ("FFX_ENVELOPE", "FFX_BINS", "FFX_WIDE", "FFX_TRAVERSAL", "FFX_BIN_CAP", "FFX_BIN_TILE", "FFX_BIN_TILE_PROJ", "FFX_BIN_SPOT_N", "FFX_K8_PLAIN",
         "FFX_PIXELS_PER_WAVE", "FFX_HOST_MATERIALS")
SPOT_GRID_N = "32"  # FFX_BIN_SPOT_N for `facing` where the test is about the spot's grid: the default 128 x 128 tiles overflow there (see test a)


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _texture(sc, ch, seed=3):
    """uniform noise with one dark quarter (footprints that are exactly zero: the forward skips their projector walk)"""
    t = np.random.default_rng(seed).random((sc.projector.height, sc.projector.width, ch)).astype(np.float32)
    t[: t.shape[0] // 2, : t.shape[1] // 2] = 0.0
    return dev(t if ch == 3 else t[..., 0])


def _rows(sc, kind):
    """-> (material table, mat_stride, rel): Lambert albedos / random principled rows with one Lambert shape among them (optional lobes: 2e-4)"""
    if kind == "albedo":
        return scenes.flatten(sc)[6], 0, 1e-4
    mats = material_rows(len(sc.meshes), 23)
    mats[0, 3] = 0.0
    return mats, 16, 2e-4


def _desc(sc, frame=None, **kw):
    sd = scene_desc.scene_desc(sc, shadows=kw.pop("shadows", True), **kw)
    return sd if frame is None else ss.set_spot_frame(sd, frame)


def _close(img_d, img_o, spp, frac, rel, what):
    img_d, img_o = np.asarray(img_d, np.float32), np.asarray(img_o, np.float32)
    scale = float(img_o.max())
    err = np.abs(img_d.astype(np.float64) - img_o)
    print(f"SHARE {what}: {float((err > rel * scale).mean()):.2e} of the pixel channels off by more than {rel:g} of the scale [{frac:g}], "
          f"worst {err.max() / scale:.2e} [{1.5 / spp:.2e}]")
    assert np.isfinite(img_d).all(), what
    return assert_image_close(img_d, img_o, spp, frac=frac, rel=rel, what=what)


def _grids_and_envelopes(gd, sd, what):
    """all three grids built with their lists within the capacity, and both emitters' envelopes written by this pose's pre-pass"""
    hdrs = bin_headers(gd)
    assert all(h[0] == 1 and 0 < h[1] <= h[2] for h in hdrs), (what, hdrs)
    n = int(os.environ.get("FFX_BIN_SPOT_N", ss.spot_grid_n(sd.spot.cutoff_deg)))
    assert envelope(gd, 1, 7 * ((sd.proj.tex_w + 15) // 16), 7 * ((sd.proj.tex_h + 15) // 16))[0] == 1, what
    assert envelope(gd, 2, 7 * n, 7 * n)[0] == 1, what
    return hdrs


# ------------------------------------------------------------------ a. every direct-light entry point
@pytest.mark.parametrize("film", ["box", "gaussian"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("rows", ["albedo", "material_rows"])
@pytest.mark.parametrize("stage", ["side_lit", "facing"])
def test_every_direct_light_entry_point_meets_the_oracle_on_the_stages(oracle, stage, rows, ch, film, monkeypatch):
    """side_lit and facing(cutoff 74) at 96 x 80: render_fwd at 64 and 16 spp, the cache-writing forward, and the three adjoints (re-tracing,
    from the cache, folded into the forward) against the oracle's gradient.  The 3-channel cases carry the other texture shape: 104 x 88 for
    side_lit (7 x 6 tiles, where the floor spans more than sixteen), 40 x 24 for facing (24 x 40 otherwise).

    facing's spot stands INSIDE a tube of 1 536 triangles, a unit from its wall: in the 128 x 128 tiles a 74-degree cone gets by default every
    triangle spans dozens of them, the lists come to 111 608 entries against a capacity of 2 F + 16 384 = 20 000, and the spot's packets walk the
    tree (SPOT_GRID_N; the default is what test_envelopes_bins_and_walks... and test_spot_grid_at_its_cone_limits render).  Here the grid is
    32 x 32 (FFX_BIN_SPOT_N), so that all three grids and both envelopes serve the render with geometry behind and beside both apexes."""
    W, H = 96, 80
    if stage == "facing":
        monkeypatch.setenv("FFX_BIN_SPOT_N", SPOT_GRID_N)
    if stage == "side_lit":
        sc = ss.side_lit(W, H) if ch == 1 else ss.side_lit(W, H, 104, 88)
    else:
        sc = ss.facing(W, H, cutoff=74.0) if ch == 1 else ss.facing(W, H, 40, 24, cutoff=74.0)
    go, gd, _ = pair(oracle, sc)
    mats, stride, rel = _rows(sc, rows)
    sd = _desc(sc, tex_channels=ch, mat_stride=stride, rfilter=None if film == "box" else "gaussian")
    frac = FRAC_BOX if film == "box" else FRAC_GAUSS
    tex = _texture(sc, ch)
    what = f"{stage} {rows} ch={ch} {film}"
    img = {}
    for spp in (64, 16):
        img[spp] = gd.render_fwd(sd, dev(mats), tex, spp, seed=7)
        if spp == 64:
            _grids_and_envelopes(gd, sd, what)
        scale, _ = _close(host(img[spp]), go.render_fwd(sd, mats, host(tex), spp, seed=7), spp, frac, rel, f"{what} spp={spp}")
        assert scale > 0.02
    spp = 64
    gimg = np.random.default_rng(2).standard_normal((H, W, 3)).astype(np.float32)
    g_o = go.render_bwd(sd, mats, spp, 7, gimg)
    grad_close(host(gd.render_bwd(sd, dev(mats), spp, 7, dev(gimg))), g_o, f"{what} render_bwd", FRAC_GRAD)
    cache = torch.zeros(ops.render_cache_bytes_sd(sd, spp), dtype=torch.uint8, device="cuda")
    assert torch.equal(gd.render_fwd(sd, dev(mats), tex, spp, seed=7, cache=cache), img[spp]), f"{what}: the cache-writing forward's image"
    assert ops.render_cache_status(cache)[2] == 0
    grad_close(host(gd.render_bwd_cached(sd, dev(mats), cache, spp, dev(gimg), seed=7 if film == "gaussian" else None)), g_o, f"{what} render_bwd_cached", FRAC_GRAD)
    if film == "box" or ch == 1:  # (the filtered film folds the adjoint for 1-channel textures only)
        img_f, g_f = gd.render_fwd_adjoint(sd, dev(mats), tex, spp, 7, dev(gimg))
        assert torch.equal(img_f, img[spp]), f"{what}: the fused launch's image"
        grad_close(host(g_f), g_o, f"{what} render_fwd_adjoint", FRAC_GRAD)


# ------------------------------------------------------------------ b. the proofs change nothing
@pytest.mark.parametrize("stage", ["side_lit", "facing", "facing_spot_grid_32"])
def test_envelopes_bins_and_walks_leave_every_bit_of_the_stages_alone(oracle, stage, monkeypatch):
    """the default path's image against the same pose prepared again without envelopes, without bins (every packet walks the tree, 64-wide and
    binary) and under the short-render hint (shadows = 3: no envelope launch): torch.equal, at 64 and at 16 spp; the re-traced gradients agree
    to 1e-4 of their maximum (the order of the float atomics).  facing by default: the spot's 128 x 128 grid overflows (test a), its packets
    walk the tree beside a projector that is served by its bins and envelope; with 32 x 32 tiles both emitters are."""
    W, H = 96, 80
    sc = ss.side_lit(W, H) if stage == "side_lit" else ss.facing(W, H, cutoff=74.0)
    if stage == "facing_spot_grid_32":
        monkeypatch.setenv("FFX_BIN_SPOT_N", SPOT_GRID_N)
    spot_served = 0 if stage == "facing" else 1
    go, gd, _ = pair(oracle, sc)
    mats, stride, rel = _rows(sc, "material_rows")
    tex = _texture(sc, 1)
    gimg = dev(np.random.default_rng(2).standard_normal((H, W, 3)).astype(np.float32))
    xf, pose = np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)), gd._vert_off_host.copy()

    def run(shadows=True):
        gd.update(xf, pose)  # (a fresh pose: nothing of the previous setting's pre-pass is claimed)
        sd = _desc(sc, tex_channels=1, mat_stride=stride, shadows=shadows)
        out = [gd.render_fwd(sd, dev(mats), tex, spp, seed=5) for spp in (64, 16)]
        state = (bin_headers(gd), envelope(gd, 1, 8, 8)[0], envelope(gd, 2, 8, 8)[0])
        return out, gd.render_bwd(_desc(sc, tex_channels=1, mat_stride=stride), dev(mats), 64, 5, gimg), state

    ref, g_ref, state = run()
    assert state[1:] == (1, spot_served) and [h[0] for h in state[0]] == [1, 1, spot_served], state
    sd = _desc(sc, tex_channels=1, mat_stride=stride)
    _close(host(ref[0]), go.render_fwd(sd, mats, host(tex), 64, seed=5), 64, FRAC_BOX, rel, f"{stage} default path")
    gs = float(g_ref.abs().max())
    assert gs > 0
    for env, shadows in (({"FFX_ENVELOPE": "0"}, True), ({"FFX_BINS": "0"}, True), ({"FFX_BINS": "0", "FFX_WIDE": "0"}, True), ({}, 3)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out, g, state = run(shadows)
        if "FFX_ENVELOPE" in env or shadows == 3:
            assert state[1:] == (0, 0), (env, shadows, state)
        for spp, a, b in zip((64, 16), out, ref):
            assert torch.equal(a, b), f"{stage} {env} shadows={shadows} spp={spp}: {int((a != b).sum())} pixel channels differ, worst {float((a - b).abs().max()):.3g}"
        assert float((g - g_ref).abs().max()) <= 1e-4 * gs, (stage, env, shadows)
        for k in env:
            monkeypatch.delenv(k)


# ------------------------------------------------------------------ c. spot frames
@pytest.mark.parametrize("name", list(ss.spot_frames()))
def test_spot_frames_meet_the_oracle_and_take_the_instance_the_host_proves(oracle, name):
    """side_lit at 64 x 48 x 64 with the spot's local frame right-multiplied by each of stage_scenes.spot_frames(): image and re-traced gradient
    against the oracle (Lambert rows: the generic instance, whose spot arm branches on ShadeK.s_rigid), then with plain principled rows
    inline, a 1-channel texture and the box film the launcher's counters: a frame the host proves orthonormal (rigid, nearly_rigid — and
    mirrored: a reflection is orthonormal, tests/test_stage_cpu.py) takes the plain-scene instance, every other one the generic instance; and
    both meet the oracle.  scaled and mirrored describe rigid's cone: their images meet rigid's as well."""
    W, H, spp = 64, 48, 64
    sc = ss.side_lit(W, H)
    frame = ss.spot_frames()[name]
    go, gd, alb = pair(oracle, sc)
    tex = _texture(sc, 1)
    sd = _desc(sc, frame, tex_channels=1)
    assert (ss.spot_rigid_measure(sd) < ss.SPOT_RIGID_TOL) == (name in ("rigid", "nearly_rigid", "mirrored"))
    img_o = go.render_fwd(sd, alb, host(tex), spp, seed=4)
    img_d = host(gd.render_fwd(sd, dev(alb), tex, spp, seed=4))
    _close(img_d, img_o, spp, FRAC_BOX, 1e-4, f"spot frame {name}, Lambert")
    gimg = np.random.default_rng(6).standard_normal((H, W, 3)).astype(np.float32)
    grad_close(host(gd.render_bwd(sd, dev(alb), spp, 4, dev(gimg))), go.render_bwd(sd, alb, spp, 4, gimg), f"spot frame {name} render_bwd", FRAC_GRAD)
    # ---- the plain-scene instance and its refusal
    rows = np.stack([scenes.material_row(m.albedo, {}) for m in sc.meshes])
    sdp = _desc(sc, frame, tex_channels=1, mat_stride=16, host_mats=rows)
    assert sdp.n_mat_h == rows.size
    c0 = ops.k8_instance_launches()
    img_p = gd.render_fwd(sdp, None, tex, spp, seed=4)
    torch.cuda.synchronize()
    c1 = ops.k8_instance_launches()
    plain = name in ("rigid", "nearly_rigid", "mirrored")
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if plain else (0, 1)), f"{name}: (plain-scene, generic) launches {(c1[0] - c0[0], c1[1] - c0[1])}"
    img_po = go.render_fwd(sdp, rows, host(tex), spp, seed=4)
    _close(host(img_p), img_po, spp, FRAC_BOX, 1e-4, f"spot frame {name}, plain principled rows")
    # the fused adjoint takes the same instance
    img_f, g_f = gd.render_fwd_adjoint(sdp, None, tex, spp, 4, dev(gimg))
    torch.cuda.synchronize()
    c2 = ops.k8_instance_launches()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == ((1, 0) if plain else (0, 1)) and torch.equal(img_f, img_p)
    grad_close(host(g_f), go.render_bwd(sdp, rows, spp, 4, gimg), f"spot frame {name} fused adjoint, plain principled rows", FRAC_GRAD)
    if name in ("scaled", "mirrored"):  # (the same cone through the other arm / the other sign of l.x)
        _close(img_d, host(gd.render_fwd(_desc(sc, tex_channels=1), dev(alb), tex, spp, seed=4)), spp, FRAC_BOX, 1e-4, f"spot frame {name} against rigid, Lambert")
        sdr = _desc(sc, tex_channels=1, mat_stride=16, host_mats=rows)
        _close(host(img_p), host(gd.render_fwd(sdr, None, tex, spp, seed=4)), spp, FRAC_BOX, 1e-4, f"spot frame {name} against rigid, plain principled rows")


def test_the_squeezed_cone_is_another_cone(oracle):
    """guards the frames test against a set_spot_frame that writes nothing: the sheared frame's image is not the rigid one's"""
    sc = ss.side_lit(64, 48)
    go, gd, alb = pair(oracle, sc)
    tex = _texture(sc, 1)
    a = gd.render_fwd(_desc(sc, None, tex_channels=1), dev(alb), tex, 16, seed=4)
    b = gd.render_fwd(_desc(sc, ss.spot_frames()["squeezed"], tex_channels=1), dev(alb), tex, 16, seed=4)
    assert float((a - b).abs().max()) > 0.02 * float(a.max())


# ------------------------------------------------------------------ d. cone limits
def test_spot_grid_at_its_cone_limits(oracle, monkeypatch):
    """facing at 64 x 48 with the spot's cutoff at 75.5 (no grid: beyond 75 degrees a perspective grid is not built), 3 (the grid's lower clamp,
    8 x 8 tiles), 74 and 75 degrees (the upper clamp, 128 x 128: on, counted, and too fine for this tube — the lists overflow and the packets
    walk the tree), 64 and 16 spp, against the oracle; the headers say which grids this pose's pre-pass built; 75.5 rendered again behind 75
    on the same blob (whose spot header is then stale) is the first image bit for bit; with 32 x 32 tiles the 74 and 75 grids fit and the
    images are the same bits; and without bins the 75 and 75.5 images are what they were."""
    W, H = 64, 48
    sc = ss.facing(W, H, cutoff=74.0)
    go, gd, alb = pair(oracle, sc)
    tex = _texture(sc, 1)
    xf, pose = np.tile(np.eye(4, dtype=np.float32), (len(sc.meshes), 1, 1)), gd._vert_off_host.copy()
    kept = {}

    def render(cutoff, tag):
        sd = _desc(sc, tex_channels=1)
        sd.spot.cutoff_deg, sd.spot.beam_width_deg = cutoff, 0.75 * cutoff
        gd.update(xf, pose)
        out = {spp: gd.render_fwd(sd, dev(alb), tex, spp, seed=8) for spp in (64, 16)}
        hdrs = bin_headers(gd)
        for spp in (64, 16):
            scale, _ = _close(host(out[spp]), go.render_fwd(sd, alb, host(tex), spp, seed=8), spp, FRAC_BOX, 1e-4, f"facing cutoff {cutoff:g} spp={spp} {tag}")
            assert scale > 0.02
        return out, hdrs

    kept[75.5], hdrs = render(75.5, "first")
    assert hdrs[0][0] == 1 and hdrs[1][0] == 1 and hdrs[2] == (0, 0, 0), hdrs  # (a fresh blob: nobody has written the spot's header)
    out3, hdrs = render(3.0, "")
    assert all(h[0] == 1 and 0 < h[1] <= h[2] for h in hdrs), hdrs
    # 8 x 8 tiles: the list starts end with the total behind 64 tiles, and the words behind it are still the fresh blob's
    torch.cuda.synchronize()
    base = int(gd.info.off_bins) + 2 * int(gd.info.bins_stride)
    starts = gd.blob[base + 64: base + 64 + 4 * 68].cpu().numpy().view(np.uint32)
    assert ss.spot_grid_n(3.0) == 8 and starts[64] == hdrs[2][1] and not starts[65:].any(), starts[60:]
    assert float((out3[64] - kept[75.5][64]).abs().max()) > 0.02 * float(kept[75.5][64].max())  # (the narrow cone lights far less)
    for cutoff in (74.0, 75.0):
        kept[cutoff], hdrs = render(cutoff, "")
        # the grid is ON (this pose's pre-pass counted it: 128 x 128 tiles, the total stands behind the last tile's start) and its lists do not
        # fit — a tube of 1 536 triangles seen from inside — so the packets walk the tree, as they do beyond 75 degrees
        torch.cuda.synchronize()
        total = int(gd.blob[base + 64 + 4 * 16384: base + 64 + 4 * 16385].cpu().numpy().view(np.uint32)[0])
        assert ss.spot_grid_n(cutoff) == 128 and hdrs[0][0] == 1 and hdrs[1][0] == 1 and hdrs[2][0] == 0 and hdrs[2][1] == total > hdrs[2][2], (cutoff, hdrs, total)
    again, _ = render(75.5, "behind 75")
    assert all(torch.equal(again[spp], kept[75.5][spp]) for spp in (64, 16))
    monkeypatch.setenv("FFX_BIN_SPOT_N", SPOT_GRID_N)  # a grid whose lists fit, up to the limit: the same bits
    for cutoff in (74.0, 75.0):
        out, hdrs = render(cutoff, f"{SPOT_GRID_N} x {SPOT_GRID_N} tiles")
        assert all(h[0] == 1 and 0 < h[1] <= h[2] for h in hdrs), (cutoff, hdrs)
        for spp in (64, 16):
            assert torch.equal(out[spp], kept[cutoff][spp]), f"cutoff {cutoff} spp {spp}: the image depends on whether the spot's grid served it"
    monkeypatch.delenv("FFX_BIN_SPOT_N")
    monkeypatch.setenv("FFX_BINS", "0")
    for cutoff in (75.0, 75.5):
        out, _ = render(cutoff, "FFX_BINS=0")
        for spp in (64, 16):
            assert torch.equal(out[spp], kept[cutoff][spp]), f"cutoff {cutoff} spp {spp}: {int((out[spp] != kept[cutoff][spp]).sum())} pixel channels differ without bins"


# ------------------------------------------------------------------ e. emitters that see nothing
@pytest.mark.parametrize("stage", ["side_lit", "facing"])
def test_emitters_that_see_nothing_give_an_exactly_black_image(oracle, stage):
    """away(stage): empty grids, empty envelopes, every sample outside the frustum and the cone — the image is exactly zero (no NaN, no -0
    that is not 0) under both films and at 64 and 16 spp, the adjoints of a random gradient image are exactly zero; with ONE emitter away the
    image is the oracle's."""
    W, H = 64, 48
    base = ss.side_lit(W, H) if stage == "side_lit" else ss.facing(W, H, cutoff=74.0)
    go, gd, alb = pair(oracle, base)
    tex = _texture(base, 1)
    gimg = dev(np.random.default_rng(2).standard_normal((H, W, 3)).astype(np.float32))
    sc = ss.away(base)
    zero = torch.zeros((H, W, 3), device="cuda")
    for film in (None, "gaussian"):
        sd = _desc(sc, tex_channels=1, rfilter=film)
        for spp in (64, 16):
            img = gd.render_fwd(sd, dev(alb), tex, spp, seed=3)
            assert torch.equal(img, zero), f"{stage} {film} spp={spp}: {int((img != 0).sum())} pixel channels lit, {int(torch.isnan(img).sum())} NaN"
            g = gd.render_bwd(sd, dev(alb), spp, 3, gimg)
            assert torch.equal(g, torch.zeros_like(g)), f"{stage} {film} spp={spp}: gradient"
        img_f, g_f = gd.render_fwd_adjoint(sd, dev(alb), tex, 64, 3, gimg)
        assert torch.equal(img_f, zero) and torch.equal(g_f, torch.zeros_like(g_f))
    assert np.all(go.render_fwd(_desc(sc, tex_channels=1), alb, host(tex), 16, seed=3) == 0)
    for which in ("projector", "spot"):
        one = ss.away(base, (which,))
        sd = _desc(one, tex_channels=1)
        for spp in (64, 16):
            scale, _ = _close(host(gd.render_fwd(sd, dev(alb), tex, spp, seed=3)), go.render_fwd(sd, alb, host(tex), spp, seed=3), spp, FRAC_BOX, 1e-4,
                              f"{stage}, {which} away, spp={spp}")
            assert scale > 0.02
        g = gd.render_bwd(sd, dev(alb), 64, 3, gimg)
        if which == "projector":
            assert torch.equal(g, torch.zeros_like(g))
        else:
            grad_close(host(g), go.render_bwd(sd, alb, 64, 3, host(gimg)), f"{stage}, spot away, render_bwd", FRAC_GRAD)


# ------------------------------------------------------------------ f. one blob, re-prepared between arrangements
def test_a_blob_re_prepared_between_arrangements_of_the_emitters(oracle):
    """one DeviceGeometry, no update in between: side_lit under its own emitters, under the projector and the spot in each other's pose, under
    its own again — the third image is the first bit for bit (nothing of the other arrangement's grids, envelopes or apex records is read),
    the second is the oracle's."""
    W, H = 64, 48
    sc = ss.side_lit(W, H)
    go, gd, alb = pair(oracle, sc)
    tex = _texture(sc, 1)
    sd_own, sd_swap = _desc(sc, tex_channels=1), _desc(ss.swapped(sc), tex_channels=1)
    gimg = np.random.default_rng(2).standard_normal((H, W, 3)).astype(np.float32)
    for spp in (64, 16):
        first = gd.render_fwd(sd_own, dev(alb), tex, spp, seed=6)
        g_first = gd.render_bwd(sd_own, dev(alb), spp, 6, dev(gimg))
        second = gd.render_fwd(sd_swap, dev(alb), tex, spp, seed=6)
        _grids_and_envelopes(gd, sd_swap, "swapped")
        g_second = gd.render_bwd(sd_swap, dev(alb), spp, 6, dev(gimg))
        third = gd.render_fwd(sd_own, dev(alb), tex, spp, seed=6)
        assert torch.equal(third, first), f"spp={spp}: {int((third != first).sum())} pixel channels differ after the other arrangement"
        g_third = gd.render_bwd(sd_own, dev(alb), spp, 6, dev(gimg))
        assert float((g_third - g_first).abs().max()) <= 1e-4 * float(g_first.abs().max())
        _close(host(first), go.render_fwd(sd_own, alb, host(tex), spp, seed=6), spp, FRAC_BOX, 1e-4, f"side_lit own emitters spp={spp}")
        scale, _ = _close(host(second), go.render_fwd(sd_swap, alb, host(tex), spp, seed=6), spp, FRAC_BOX, 1e-4, f"side_lit swapped emitters spp={spp}")
        assert scale > 0.02 and float((second - first).abs().max()) > 0.02 * scale
        grad_close(host(g_second), go.render_bwd(sd_swap, alb, spp, 6, gimg), f"side_lit swapped emitters render_bwd spp={spp}", FRAC_GRAD)
