"""The packet render kernel's cache-writing plain-scene instance (ffx_trace.hip k_render_fwd_pk<..., PLAIN, CACHE>): for a scene the host proves
plain, the forward that also writes the adjoint cache (ffx_render_fwd_cache — the L1-loss step's render) takes a plain instance too.  It renders
the generic instance's image BIT FOR BIT, leaves the generic instance's cache for K9 (ffx_render_bwd_cached) bit for bit — the stray records as a
multiset: their order in the arena is the waves' order of arrival —, the launcher's counters say which instance ran, and what plain_scene refuses
goes to the generic instance with a cache as without one.

Scene: tests/k8_scenes.py — the vocal fold at 64 x 48, 8 x 8 fold lips in an 8 x 16 tube, a 4 x 4 laser on a 64^2 texture.  Every comparison
between the two instances is bit equality: the arithmetic is the same in the same order.  K9's OUTPUT is not such a comparison: where float atomics
of several writers meet in one texel the order of arrival decides last bits, and under gradient images that are non-zero on a pixel lattice 16 x 12
apart (moved over all 192 offsets; tests/test_k8_plain_gpu.py gives the geometry) a texel still has its pixel's footprint wave AND the threads
that replay that pixel's stray records as writers — two K9 launches from ONE cache differ (figures in the tests that print them)."""
import numpy as np
import pytest
import torch

from tests import k8_scenes
from tests.conftest import assert_image_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAT = "mat-Default OBJ.brdf_0."
H, W = 48, 64


def _scene(seed):
    wl, tex = k8_scenes.workload()
    k8_scenes.pose(wl, seed)
    return wl, tex.unsqueeze(-1).contiguous()


def _args(wl):
    sd = wl.mi_scene.scene_desc(tex_channels=1)
    return sd, wl.mi_scene.materials_arg(sd)


def _cache(sd, spp, fill=0xA5):
    """a cache buffer full of a byte pattern: what a launch does not write is the same on both sides, and never zero by luck"""
    from fireflies_amd import ops

    return torch.full((ops.render_cache_bytes_sd(sd, spp),), fill, dtype=torch.uint8, device=DEV)


def _counted(fn):
    """fn() -> (its result, launches of the plain instances, launches of the generic ones)"""
    from fireflies_amd import ops

    p0, g0 = ops.k8_instance_launches()
    out = fn()
    torch.cuda.synchronize()
    p1, g1 = ops.k8_instance_launches()
    return out, p1 - p0, g1 - g0


def _render_cached(monkeypatch, plain, geom, sd, mats, tex3, spp, seed, buf, **kw):
    """the cache-writing forward under the default launcher (plain) or FFX_K8_PLAIN=0 -> image; the counters are asserted"""
    if plain:
        monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    else:
        monkeypatch.setenv("FFX_K8_PLAIN", "0")
    if kw.get("cache_zeroed"):
        buf[:64].zero_()  # (FFX_RENDER_CACHE_ZEROED: the caller has cleared the header on this stream)
    img, n_plain, n_gen = _counted(lambda: geom.render_fwd(sd, mats, tex3, spp, seed, cache=buf, **kw))
    assert (n_plain, n_gen) == ((1, 0) if plain else (0, 1)), f"cache-writing forward, FFX_K8_PLAIN {'unset' if plain else '0'}: (plain, generic) launches"
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    return img


def _lattices(seed=5):
    g = torch.from_numpy(np.where(np.random.default_rng(seed).random((H, W, 3)) < 0.5, -1.0, 1.0).astype(np.float32) / (H * W * 3)).to(DEV)
    out = []
    for oy in range(12):
        for ox in range(16):
            l = torch.zeros_like(g)
            l[oy::12, ox::16] = g[oy::12, ox::16]
            out.append(l)
    return g, out


@pytest.mark.parametrize("spp", [64, 40])
def test_cache_writing_plain_instance_renders_the_generic_instances_bits(spp, monkeypatch):
    """three poses x sparse_adjoint on / off x cache_zeroed on / off, at 64 spp and at 40 (a part-filled wave): counters (1, 0) by default and (0, 1)
    under FFX_K8_PLAIN=0; the two images are equal and equal to the plain render without a cache; ops.render_cache_status is equal"""
    from fireflies_amd import ops

    wl, tex3 = _scene(11)
    geom = wl.mi_scene.geom
    for seed in (11, 12, 13):
        k8_scenes.pose(wl, seed)
        sd, mats = _args(wl)
        monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
        img0, n_plain, n_gen = _counted(lambda: geom.render_fwd(sd, mats, tex3, spp, seed))
        assert (n_plain, n_gen) == (1, 0), "the cache-less forward of a plain scene takes the plain instance"
        assert float(img0.max()) > 0.02
        for sparse in (False, True):
            for zeroed in (False, True):
                kw = dict(sparse_adjoint=sparse, cache_zeroed=zeroed)
                buf_p, buf_g = _cache(sd, spp), _cache(sd, spp)
                img_p = _render_cached(monkeypatch, True, geom, sd, mats, tex3, spp, seed, buf_p, **kw)
                img_g = _render_cached(monkeypatch, False, geom, sd, mats, tex3, spp, seed, buf_g, **kw)
                what = f"pose {seed}, {spp} spp, sparse_adjoint {sparse}, cache_zeroed {zeroed}"
                assert img_p.dtype == torch.float32 and torch.equal(img_p, img_g), what + ": image, plain against generic"
                assert torch.equal(img_p, img0), what + ": image, with against without a cache"
                st_p, st_g = ops.render_cache_status(buf_p), ops.render_cache_status(buf_g)
                assert st_p == st_g and st_p[2] == 0, f"{what}: cache status {st_p} against {st_g}"


def _status_holds(st, what):
    """(used, capacity, dropped) of a box film's cache: `used` counts every stray sample, kept or not.  A wave takes its samples' records with one
    atomic and keeps them iff they end inside the arena, so the kept records fill it to within one wave's 64: nothing dropped while used <= capacity,
    else used - capacity <= dropped < used - capacity + 64 — WHICH wave meets the arena's end is the order of arrival"""
    used, cap, dropped = st
    if used <= cap:
        assert dropped == 0, f"{what}: {st}"
    else:
        assert used - cap <= dropped < used - cap + 64, f"{what}: {st}"


def _assert_same_cache(buf_p, buf_g, st_p, st_g, what):
    """the two caches hold the same adjoint: header (stray samples, capacity), every pixel's slot and both footprints of every lit pixel byte for byte
    (what a launch does not write is _cache's fill on both sides), and — with nothing dropped — the stray records as a multiset: their place in the
    arena is the order in which the waves took them, and K9 replays record i in thread i whatever i is.  Layout: ffx_trace.hip, "adjoint cache":
    [0, 64) header | 8 bytes per pixel | 112-byte footprints from off_foot | 24-byte stray records from off_arena | the second footprints.
    -> stray records compared"""
    n_pix = H * W
    off_foot = (64 + 8 * n_pix + 127) & ~127
    off_arena = (off_foot + 112 * n_pix + 127) & ~127
    assert st_p[:2] == st_g[:2], f"{what}: (used, capacity) {st_p[:2]} against {st_g[:2]}"
    _status_holds(st_p, what + ", plain")
    _status_holds(st_g, what + ", generic")
    cap = st_p[1]
    a, b = buf_p.cpu().numpy(), buf_g.cpu().numpy()
    assert a.size == b.size and off_arena + 24 * cap <= a.size
    assert np.array_equal(a[:8], b[:8]) and np.array_equal(a[12:64], b[12:64]), what + ": cache header"
    assert np.array_equal(a[64:off_arena], b[64:off_arena]), what + ": pixel slots and footprints"
    assert np.array_equal(a[off_arena + 24 * cap:], b[off_arena + 24 * cap:]), what + ": second footprints"
    assert int((a[64:off_foot].view(np.uint16)[3::4] == 1).sum()) > 100, what + ": lit pixels"
    if st_p[2] or st_g[2]:
        return 0
    n = st_p[0]
    ra, rb = (x[off_arena:off_arena + 24 * n].view(np.uint32).reshape(n, 6) for x in (a, b))
    ra, rb = (r[np.lexsort(r.T[::-1])] for r in (ra, rb))
    assert np.array_equal(ra, rb), what + ": stray records, sorted"
    return n


def _k9_bits(geom, sd, mats, buf_p, buf_g, spp, lattices, what):
    """K9 from either cache under every lattice -> (values that differ, non-zero values, values that differ between two K9 launches from ONE cache)"""
    n_diff = n_nz = n_self = 0
    for g in lattices:
        gt_p = geom.render_bwd_cached(sd, mats, buf_p, spp, g)
        gt_g = geom.render_bwd_cached(sd, mats, buf_g, spp, g)
        gt_g2 = geom.render_bwd_cached(sd, mats, buf_g, spp, g)
        assert bool(torch.isfinite(gt_g).all()), what
        n_diff += int((gt_p != gt_g).sum())
        n_self += int((gt_g2 != gt_g).sum())
        n_nz += int((gt_g != 0).sum())
    return n_diff, n_nz, n_self


def test_either_instance_leaves_the_same_cache_for_k9(monkeypatch):
    """the cache itself: three poses, 64 spp, every footprint kept (sparse_adjoint off).  Meant as: under each of the 192 lattice gradient images
    ffx_render_bwd_cached's output from the plain instance's cache == its output from the generic instance's, raw float32.  That does not hold of K9
    from ONE cache: a pixel's footprint is scattered by one wave and each of its stray records by a thread of another, so a texel that the footprint
    and two strays reach is summed in the order of arrival (measured on this scene, MI355X, poses 11 / 12 / 13, which leave 974 / 1 530 / 1 453 stray
    records: 12 / 37 / 45 of ~12 000 values differ between two K9 launches from the generic instance's cache, 43 / 177 / 117 between the two
    instances' caches — whose records are the same, in another order).  K9's bits are a function of the cache and of that order; what
    the instance answers for is the cache, so THAT is held bit for bit (_assert_same_cache: everything K9 reads), and K9 runs from both caches under
    every lattice with its differences printed next to those of two launches from one cache."""
    from fireflies_amd import ops

    wl, tex3 = _scene(11)
    geom = wl.mi_scene.geom
    gfull, lattices = _lattices()
    for seed in (11, 12, 13):
        k8_scenes.pose(wl, seed)
        sd, mats = _args(wl)
        buf_p, buf_g = _cache(sd, 64), _cache(sd, 64)
        img_p = _render_cached(monkeypatch, True, geom, sd, mats, tex3, 64, seed, buf_p)
        img_g = _render_cached(monkeypatch, False, geom, sd, mats, tex3, 64, seed, buf_g)
        assert torch.equal(img_p, img_g)
        st_p, st_g = ops.render_cache_status(buf_p), ops.render_cache_status(buf_g)
        n_stray = _assert_same_cache(buf_p, buf_g, st_p, st_g, f"pose {seed}")
        assert st_p[2] == 0
        n_diff, n_nz, n_self = _k9_bits(geom, sd, mats, buf_p, buf_g, 64, lattices, f"pose {seed}")
        gd_p, gd_g = geom.render_bwd_cached(sd, mats, buf_p, 64, gfull), geom.render_bwd_cached(sd, mats, buf_g, 64, gfull)
        print(f"pose {seed}: caches equal ({n_stray} stray records); K9, lattice gradients: {n_diff} of {n_nz} values differ between the instances' caches, "
              f"{n_self} between two K9 launches from one cache; dense gradient image: {int((gd_p != gd_g).sum())} of {int((gd_g != 0).sum())} differ")
        assert n_nz > 1000 and n_stray > 0


@pytest.mark.parametrize("tex_side", [500, 96])
def test_stray_records_of_a_fine_texture_are_the_generic_instances(tex_side, monkeypatch):
    """a 500 x 500 projector texture: a camera pixel spans about 15 texels, most lit samples miss the pixel's 5 x 5 window and go to the stray arena.
    Stray records exist and the cache is the same from either instance (_assert_same_cache; the stray records themselves with nothing dropped).

    Measured on this scene (MI355X): 500^2 sends 44 497 samples to an arena of 4 096 records — it overflows, and `dropped` is then the order of
    arrival: 40 404 from the plain instance, 40 427 from the generic one in one run, 40 402 and 40 433 in the next (_status_holds: all within the 64
    that one wave's allocation can make of it; used and capacity equal).  So 500^2 holds the overflow path — counts, pixel slots, footprints — and
    96^2 (a pixel spans about 3 texels: 2 860 stray records, nothing dropped) the records themselves.  K9 from those caches: as in the test above,
    printed (264 of 18 886 lattice values differ between the instances' caches, 54 between two launches from one)."""
    from fireflies_amd import ops

    wl, _ = _scene(12)
    geom = wl.mi_scene.geom
    sd0, mats = _args(wl)
    sd, tex3 = k8_scenes.with_texture(sd0, tex_side, tex_side)
    _, lattices = _lattices()
    buf_p, buf_g = _cache(sd, 64), _cache(sd, 64)
    img_p = _render_cached(monkeypatch, True, geom, sd, mats, tex3, 64, 12, buf_p)
    img_g = _render_cached(monkeypatch, False, geom, sd, mats, tex3, 64, 12, buf_g)
    assert torch.equal(img_p, img_g) and float(img_p.max()) > 0.02
    st_p, st_g = ops.render_cache_status(buf_p), ops.render_cache_status(buf_g)
    print(f"{tex_side}^2 texture: plain (used, capacity, dropped) = {st_p}, generic {st_g}; dropped: {st_p[2]}")
    assert st_p[0] > 0, "a fine texture leaves stray records"
    n_stray = _assert_same_cache(buf_p, buf_g, st_p, st_g, f"{tex_side}^2 texture")
    print(f"{tex_side}^2 texture: caches equal; stray records compared: {n_stray}")
    if st_p[2] == 0 and st_g[2] == 0:
        n_diff, n_nz, n_self = _k9_bits(geom, sd, mats, buf_p, buf_g, 64, lattices, f"{tex_side}^2 texture")
        print(f"K9, lattice gradients: {n_diff} of {n_nz} values differ between the instances' caches, {n_self} between two K9 launches from one cache")
        assert n_nz > 1000


@pytest.mark.parametrize("case", ["fp16", "spp65", "sheen"])
def test_what_plain_scene_refuses_takes_the_generic_instance_with_a_cache_too(case, monkeypatch):
    """one refusal each — a half-precision film, a second pass, a row with an optional lobe: the cache-writing forward's counters show the generic instance"""
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    wl, tex3 = _scene(21)
    geom = wl.mi_scene.geom
    if case == "sheen":
        wl.params[MAT + "sheen.value"] = 0.6
        wl.params.update()
    sd, mats = _args(wl)
    spp = 65 if case == "spp65" else 64
    buf = _cache(sd, spp)
    img, n_plain, n_gen = _counted(lambda: geom.render_fwd(sd, mats, tex3, spp, 21, fp16=case == "fp16", cache=buf))
    assert (n_plain, n_gen) == (0, 1), f"{case}: generic instance"
    assert bool(torch.isfinite(img.float()).all()) and float(img.float().max()) > 0.02


def test_l1_steps_move_the_rays_to_the_same_bits(monkeypatch):
    """three PatternOptimizer steps under image_l1_loss (cache-writing forward + K9), by default and under FFX_K8_PLAIN=0: the rays are equal bit for
    bit after each step, step_paths shows the cache route, the counters show the instance"""
    from fireflies_amd import mi
    from fireflies_amd.optim import PatternOptimizer, image_l1_loss

    rays = {}
    for plain in (True, False):
        if plain:
            monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
        else:
            monkeypatch.setenv("FFX_K8_PLAIN", "0")
        wl, _ = _scene(31)
        with torch.no_grad():
            target = mi.render(wl.mi_scene, spp=64, seed=99).torch().clone()
        opt = PatternOptimizer(wl.mi_scene, wl.ff_scene, wl.laser, sigma=10.0, tex_size=(64, 64), spp=64, lr=5e-3, reg_weight=0.1, base_seed=7, loss_fn=image_l1_loss(target))
        rays[plain] = [wl.laser._rays.detach().clone()]

        def three_steps():
            for _ in range(3):
                opt.step()
                torch.cuda.synchronize()
                rays[plain].append(wl.laser._rays.detach().clone())

        _, n_plain, n_gen = _counted(three_steps)
        assert opt.step_paths == {"fused": 0, "cache_k9": 3, "retrace": 0}
        assert (n_plain, n_gen) == ((3, 0) if plain else (0, 3)), "the L1 step's render: (plain, generic) launches"
    monkeypatch.delenv("FFX_K8_PLAIN", raising=False)
    assert torch.equal(rays[True][0], rays[False][0])
    print("rays that differ after steps 1..3: " + ", ".join(str(int((a != b).sum())) for a, b in zip(rays[True][1:], rays[False][1:])))
    for k in (1, 2, 3):
        assert torch.equal(rays[True][k], rays[False][k]), f"rays after step {k}"
    assert not torch.equal(rays[True][3], rays[True][0])


def test_cache_writing_plain_image_is_the_oracles(oracle, monkeypatch):
    """the cache-writing plain instance's image against the CPU oracle at the suite's own bound for this scene (box film: 1e-4 of the scale for all but
    1e-3 of the pixel channels)"""
    from fireflies_amd import scenes

    wl, tex3 = _scene(21)
    geom = wl.mi_scene.geom
    sd, mats = _args(wl)
    img = _render_cached(monkeypatch, True, geom, sd, mats, tex3, 64, 21, _cache(sd, 64))
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(wl.data)
    go = oracle.Geometry(geom.src_verts.cpu().numpy(), tris, shape, off)
    go.update(wl.mi_scene._xforms.numpy(), wl.mi_scene._offs)
    ref = go.render_fwd(sd, wl.mi_scene._albedo_host, tex3[..., 0].cpu().numpy(), 64, seed=21).astype(np.float32)
    scale, _ = assert_image_close(img.cpu().numpy(), ref, 64, frac=1e-3, rel=1e-4, what="cache-writing plain instance")
    assert scale > 0.02
