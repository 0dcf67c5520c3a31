"""Pattern optimisation loop — the counterpart of the reference's EMPTY
examples/09_point_pattern_optimization.py and examples/11_domain_specific_pattern_optim.py
(SURVEY F3), reconstructed from the pieces the reference does ship:

    for step:
        pts  = laser.projectRaysToNDC()[:, :2]                    K1
        tex  = blur(sum(rasterize_points(pts, sigma, size)))      K2 + K3   (vocalfold_scene.py:56-63)
        for each scene sample k of this rank:
            seed RNGs; ff_scene.randomize()                       K5 + K6   (scene.py:360-384)
            img = mi.render(scene, spp)                           K8
            loss_k = task_loss(img); d loss_k / d tex             K9
        d loss / d rays through K3^T, K2-bwd, K1-bwd, + overlap regulariser L1(softor, sum)
                                                                  (rasterization.py:589-600)
        all-reduce [3N+2]; Adam step; laser.clamp_to_fov(); laser.normalize_rays()
                                                                  (laser.py:199-206,254-255)
"""
import contextlib
import os
import random

import torch

from . import _abi, dist, ops
from . import functional as Fn
from .scene import StaleDrawError


def coverage_loss(img):
    """default task loss: minus the mean laser (green) radiance reaching the camera — the pattern
    is pulled toward surfaces that are visible and well lit; the overlap regulariser keeps the
    points apart."""
    return -img[..., 1].mean()


_COVERAGE_GRAD = {}


def _coverage_grad(img):
    key = (tuple(img.shape), img.device)
    g = _COVERAGE_GRAD.get(key)
    if g is None:
        g = torch.zeros(img.shape, dtype=torch.float32, device=img.device)
        g[..., 1] = -1.0 / float(img.shape[0] * img.shape[1])
        _COVERAGE_GRAD[key] = g
    return g


def _coverage_value_and_grad(img):
    """coverage_loss and its (constant) gradient without an autograd graph."""
    return -img[..., 1].float().mean(), _coverage_grad(img)


def _coverage_accumulate(img, acc):
    """acc += coverage_loss(img) (two launches: reduction, subtract) -> its constant gradient"""
    g = _coverage_grad(img)
    acc.sub_(img[..., 1].mean(dtype=torch.float32))
    return g


# a task loss may carry `value_and_grad(img) -> (loss, d loss / d img)` and `accumulate_value_and_grad(img, acc) -> d loss / d img`
# (adds the value to the 0-dim tensor `acc`); otherwise autograd is used for it.  `linear_gradient(img) -> g` declares the loss
# LINEAR in the image, loss(img) = <g, img> with a constant g: the adjoint launch then also evaluates the loss
# (ffx_render_bwd_cached's dot_out) and the step needs no reduction launch at all
coverage_loss.value_and_grad = _coverage_value_and_grad
coverage_loss.accumulate_value_and_grad = _coverage_accumulate
coverage_loss.linear_gradient = _coverage_grad


def image_l1_loss(target):
    """A task loss that is NOT linear in the image: torch.nn.L1Loss()(img, target) against a fixed target render — the loss class
    the reference's own optimisation loop uses (fireflies/graphics/rasterization.py:579, 596-602), applied to the image as SURVEY 3.5's
    `task_loss(img | ...)`.  Its gradient sign(img - target) / n depends on the render, so a step takes the general adjoint path:
    cache-writing forward + ffx_render_bwd_cached (K9).  Value and gradient come from ONE launch (ffx_l1_value_grad)."""
    tgt = target.detach().float().contiguous()

    def loss(img):
        return (img.float() - tgt).abs().mean()

    def value_and_grad(img):
        a = img if img.dtype == torch.float32 else img.float()
        v, g = ops.l1_value_grad(a.reshape(-1), tgt.reshape(-1))
        return v, g.view(a.shape)

    def accumulate(img, acc):
        a = img if img.dtype == torch.float32 else img.float()
        if acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() >= 1:
            _, g = ops.l1_value_grad(a.reshape(-1), tgt.reshape(-1), acc=acc)  # (the value joins the step's running loss inside the reduction launch)
        else:
            v, g = ops.l1_value_grad(a.reshape(-1), tgt.reshape(-1))
            acc.add_(v)
        return g.view(a.shape)

    loss.value_and_grad = value_and_grad
    loss.accumulate_value_and_grad = accumulate
    loss.target = tgt
    loss.l1_target = (tgt, 1.0)  # (target, weight): PatternOptimizer folds value and gradient into K9 (ffx_render_bwd_cached_l1)
    return loss


class PatternOptimizer:
    def __init__(self, mi_scene, ff_scene, laser, sigma=10.0, tex_size=(500, 500), spp=64, lr=1e-3, reg_weight=0.1, samples_per_step=1,
                 base_seed=0, loss_fn=coverage_loss, blur=(5, 3.0), integrator=None):
        self.mi_scene, self.ff_scene, self.laser = mi_scene, ff_scene, laser
        # mi.load_dict's integrator: max_depth > 2 renders paths; its adjoint replays them (the "retrace" route).  `prb` is `path`
        # here: the optimiser differentiates tex.data only
        if getattr(integrator, "type", None) == "aov":
            raise ValueError("PatternOptimizer: an 'aov' integrator is served by mi.render only (its channels carry no derivatives); pass its nested integrator")
        self.max_depth, self.rr_depth = (2, 5) if integrator is None else (int(integrator.max_depth), int(integrator.rr_depth))
        if self.max_depth > 2 and ops.deterministic_mode():
            raise ValueError("PatternOptimizer: max_depth > 2 has no deterministic adjoint (FFX_DETERMINISTIC=1)")
        self.sigma, self.tex_size, self.spp = float(sigma), (int(tex_size[0]), int(tex_size[1])), int(spp)
        mi_scene.note_spp(self.spp)  # (the pre-pass of the poses to come: with or without the emitters' envelopes, mi.Scene.note_spp)
        self.reg_weight, self.samples_per_step, self.base_seed = float(reg_weight), int(samples_per_step), int(base_seed)
        self.loss_fn, self.blur = loss_fn, blur
        laser._rays = laser._rays.detach().clone().requires_grad_(True)
        try:  # one fused kernel for the single small parameter instead of ~10 launches
            self.opt = torch.optim.Adam([laser._rays], lr=lr, fused=laser._rays.is_cuda)
        except (RuntimeError, TypeError):
            self.opt = torch.optim.Adam([laser._rays], lr=lr)
        self.step_index = 0
        # scene samples per adjoint path (bench.py prints it): "fused" = forward + adjoint in one launch (a loss linear in the image),
        # "cache_k9" = cache-writing forward + ffx_render_bwd_cached (every other loss), "retrace" = ffx_render_bwd (no cache possible)
        self.step_paths = {"fused": 0, "cache_k9": 0, "retrace": 0}
        # What step() keeps between steps (made again when a size changes).  _pat_buf: the pattern launch's outputs (pts, tsum, tsor, ws[, tex]).
        # _arena: ONE allocation — texture gradient, the data term's partial sums (one slot per 8x8-pixel block: K9 adds <gimg, img> of its block to
        # its slot, other losses to slot 0), adjoint cache; _acc: what the pattern launch clears, those + the cache's 64-byte header; _cache: None
        # without a cache (bench.py reads it); _premade: _premade_key() of the texture made ahead.  The four are dropped together: _drop_arena().
        self._pat_buf = self._arena = self._acc = self._cache = self._premade = None
        self._cache_overflowed = False  # the box film's cache overflowed once: re-trace from then on
        self._ahead = None  # the next step's draws: ((step, seeds), factory of the appliers)
        self._lin_g = self._img_stack = self._dot_part = None  # a linear loss's constant gradient image, the step's renders, <gimg, img_k> partial sums
        self._scratch = None  # the gradient launch's spill buffer (footprints that do not fit the workgroup's LDS)
        self._adam_counter = torch.zeros(1, dtype=torch.int32, device=laser._rays.device)
        # ffx_pattern_step's sync words, kept pattern and epoch (made together: flags of an old epoch must never meet a count that starts again)
        self._pat_sync, self._rays_kept, self._pat_epoch = None, None, 0
        self._merged_last = False  # the last step took ffx_pattern_step
        self._last_flat = None  # the last exchanged [3N+2] buffer (alive until the update has run; tests read the exchanged count)
        self._watch = self._watch_pin = None  # _watch_cache's header copy in flight (pin, event, step, merged, with a cache) and its pinned buffer

    def _sample_seeds(self, step):
        """seeds of this rank's scene samples of optimisation step `step` (dist.sample_seed: independent of the world size)"""
        S = self.samples_per_step
        return [dist.sample_seed(self.base_seed, step, S, k) for k in dist.sample_ids(S, dist.rank(), dist.world_size())]

    # ------------------------------------------------------------------ texture from the current pattern
    def textures(self):
        pts = self.laser.projectRaysToNDC()[:, 0:2].contiguous()
        s0, s1 = self.tex_size
        tsum = Fn.splat(pts, self.sigma, s0, s1, "sum", -1)
        tex = Fn.gaussian_blur(tsum, self.blur[0], self.blur[1]) if self.blur else tsum
        return pts, tsum, tex

    def _render_sample(self, tex_value, seed):
        """one scene sample: randomise, render, adjoint.  Returns (d loss/d tex, loss)."""
        torch.manual_seed(seed)
        random.seed(seed)
        self.ff_scene.randomize()
        leaf = tex_value.detach().clone().requires_grad_(True)
        sd = self.mi_scene.scene_desc(tex_channels=1)
        img = Fn.render(leaf, self.mi_scene.geom, sd, self.mi_scene.materials_arg(sd), self.spp, seed, max_depth=self.max_depth, rr_depth=self.rr_depth,
                        **self.mi_scene.emitter_args())
        loss = self.loss_fn(img)
        (g,) = torch.autograd.grad(loss, leaf)
        return g, loss.detach()

    # ------------------------------------------------------------------ explicit-adjoint step (default)
    def _image_loss(self, img, acc):
        """acc += loss_fn(img) -> d loss / d img: the loss's own accumulate_value_and_grad or value_and_grad, else autograd"""
        fast = getattr(self.loss_fn, "accumulate_value_and_grad", None)
        if fast is not None:
            return fast(img, acc)
        vg = getattr(self.loss_fn, "value_and_grad", None)
        with torch.enable_grad():
            if vg is not None:
                l, gimg = vg(img)
            else:
                leaf = img.detach().float().requires_grad_(True)
                l = self.loss_fn(leaf)
                (gimg,) = torch.autograd.grad(l, leaf)
        acc += l.detach()
        return gimg.float().contiguous()

    def _adam_state(self, rays):
        """exp_avg / exp_avg_sq / step of torch.optim.Adam for `rays` (created like Adam._init_group does), so that
        step() and step_autograd() — and anything that inspects self.opt — share one optimiser state"""
        st = self.opt.state[rays]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=rays.device)
            st["exp_avg"] = torch.zeros_like(rays, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(rays, memory_format=torch.preserve_format)
        g = self.opt.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("PatternOptimizer.step: plain Adam only (use step_autograd for other settings)")
        if not (isinstance(st["step"], torch.Tensor) and st["step"].is_cuda):
            st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32, device=rays.device)
        return st, g

    @torch.no_grad()
    def step(self):
        """One optimisation step over `samples_per_step` scene samples (sharded over ranks).

        Same arithmetic, kernels and summation order as `step_autograd` (the tests compare the two trajectories), but every adjoint is called
        directly: the step's adjoint route (_route) runs this rank's samples into ONE texture-gradient buffer, and the pattern side is a few fused
        launches — ffx_pattern_fwd (K1 + K2 sum + softor + the regulariser's partial sums), then _update_local or _update_exchanged.  As ~30 separate
        launches the pattern side cost 0.11 ms per step next to a 0.75 ms render; through torch.autograd the step was host-bound."""
        rays, KF, ms = self.laser._rays, self.laser._KF, self.mi_scene
        if getattr(ms.data, "lights", None):
            raise NotImplementedError("PatternOptimizer.step: the scene has extra emitters (point lights, further spots), which the explicit adjoint routes do not "
                                      "render (DESIGN.md 4.7): use step_autograd")
        if getattr(ms.data, "ambient", None) is not None:
            raise NotImplementedError("PatternOptimizer.step: the scene has a constant emitter (ambient light), which the explicit adjoint routes do not "
                                      "render (DESIGN.md 4.8): use step_autograd")
        rd, (s0, s1), cam = rays.detach(), self.tex_size, ms.data.camera
        seeds = self._sample_seeds(self.step_index)
        sd0 = ms.scene_desc(tex_channels=1)  # (sizes only: the pose of the samples comes later)
        route = self._route(sd0, seeds)
        use_cache = route in ("lin_rf", "cache")
        # the arena: accumulator, loss slots, adjoint cache
        n_slots = ops.render_dot_slots(cam.width, cam.height)
        nbytes = ops.render_cache_bytes_sd(sd0, self.spp) if use_cache else 0
        acc_bytes = -(-4 * (s0 * s1 + n_slots) // 128) * 128
        if self._arena is None or self._arena.numel() != acc_bytes + max(nbytes, 64):
            self._arena = torch.empty(acc_bytes + max(nbytes, 64), dtype=torch.uint8, device=rd.device)
            self._acc = self._arena[: acc_bytes + 64].view(torch.float32)
            self._cache = self._arena[acc_bytes:] if use_cache else None
        # pattern -> texture (K1, K2, K3), or the texture the previous step made ahead
        tex, used_premade = self._pattern_fwd(rays, KF)
        tex3 = tex.unsqueeze(-1)
        gtex, loss_slots = self._acc[: s0 * s1].view(tex3.shape), self._acc[s0 * s1: s0 * s1 + n_slots]
        appliers = self._draw(seeds)
        # this rank's samples, accumulated into gtex and the loss slots
        used_rs = []
        if route == "det":
            self._samples_det(seeds, appliers, tex3, gtex, loss_slots)
        elif route == "fused":
            used_rs = self._samples_fused(sd0, seeds, appliers, tex3, gtex)
        elif route == "retrace":
            self._samples_retrace(seeds, appliers, tex3, gtex, loss_slots)
        else:
            self._samples_cached(route == "lin_rf", bool(sd0.rfilter), seeds, appliers, tex3, gtex, loss_slots)
        for rs in used_rs:  # (the step's renders on the render streams: the gradient launch waits for them)
            torch.cuda.current_stream().wait_stream(rs)
        # back through K3^T (inside the gradient launch, over the points' footprints only), K2-bwd, K1-bwd; the regulariser depends on the pattern only
        g2 = gtex.reshape(tex.shape) if (seeds or route == "det") else None
        # (a linear loss: <gimg, img_k> summed over the step's renders, gimg repeated, in the gradient launch)
        dot = (self._img_stack, self._lin_g, self._dot_part) if route in ("fused", "lin_rf") and seeds else None
        loss_in = None if dot is not None else loss_slots
        grad = torch.empty_like(rd)
        if self._scratch is None or self._scratch.shape != self._pat_buf[1].shape:
            self._scratch = torch.empty_like(self._pat_buf[1])
        self._merged_last = False
        guard = self._cache if use_cache else None
        if dist.exchanging() and route != "det":  # (det: the texture gradient has been exchanged — as integers; every rank holds the step's sum)
            loss = self._update_exchanged(g2, dot, loss_in, grad, guard)
        else:
            loss = self._update_local(g2, dot, loss_in, grad, guard, used_premade)
        rays.grad = grad
        self.step_index += 1
        self._watch_cache(every=1 if self.step_index <= 4 else 32)  # (an arena that is too small shows in the first steps)
        return {"loss": loss}

    def _route(self, sd0, seeds):
        """The adjoint route of this step, from the film, the loss and the knobs (read on every step — tests flip them between steps):
        - "det": FFX_DETERMINISTIC=1 — every sample re-traced twice into 64-bit fixed point (_samples_det);
        - "fused": a loss linear in the image — forward and adjoint in ONE launch (ffx_render_fwd_adjoint[_filtered]), no cache, no K9;
        - "lin_rf": the same loss under a filtered film — the filtered forward stores its per-sample records, K9 applies the constant gradient to them;
        - "cache": any other loss — cache-writing forward + K9 (its linear / L1 / general sub-cases: _samples_cached);
        - "retrace": no cache possible — forward, the loss's gradient image, ffx_render_bwd (always with max_depth > 2: the replay of the paths)."""
        if self.max_depth > 2:
            if ops.deterministic_mode():
                raise ValueError("PatternOptimizer.step: max_depth > 2 has no deterministic adjoint (FFX_DETERMINISTIC=1)")
            return "retrace"
        if ops.deterministic_mode() and sd0.proj.enabled:
            return "det"
        # a linear loss: <gimg, img> is evaluated in the gradient launch from the step's renders (the fused launch's own partial sums would cost more)
        if (getattr(self.loss_fn, "linear_gradient", None) is not None and int(sd0.n_base_tex) == 0 and bool(sd0.proj.enabled) and 1 <= len(seeds) <= 64
                and os.environ.get("FFX_FUSED_ADJOINT", "1") != "0"):
            # (round 5) under a gaussian film the fused launch is NOT the fast route: it needs two launches in front of the render (the weights every
            # pixel will receive, G = gimg / weight) and forms every lit sample's 25-term gradient inside K8 — 0.74 ms per sample against 0.57 for the
            # filtered forward that stores its per-sample records + the adjoint from them (tools/rfgrad.py)
            if sd0.rfilter and Fn.cache_supported(sd0, self.spp) and os.environ.get("FFX_FUSED_ADJOINT_FILTERED", "0") != "1":
                return "retrace" if self._cache_overflowed else "lin_rf"
            return "fused"
        return "cache" if Fn.cache_supported(sd0, self.spp) and not self._cache_overflowed else "retrace"

    def _pattern_fwd(self, rays, KF):
        """-> (the step's texture, made ahead?).  (Round 6) ffx_pattern_step made the texture of the updated pattern and cleared the accumulator: it is
        used while the pattern, buffers and settings are the ones it saw (_premade_key; `stale` on the device, read by _watch_cache).  Otherwise
        K1 + K2 (+ K3: the blur rides on the splat's tiles) in one launch that also clears the accumulator."""
        rd, (s0, s1), want_reg = rays.detach(), self.tex_size, self.reg_weight > 0
        buf = self._pat_buf
        if (buf is None or len(buf) != (5 if self.blur else 4) or buf[0].shape[0] != rd.shape[0] or tuple(buf[1].shape) != (s1, s0)
                or (buf[2] is None) == want_reg):
            buf = None
        pre, self._premade = self._premade, None
        if not self.blur:
            self._pat_buf = ops.pattern_fwd(rd, KF, self.sigma, s0, s1, want_softor=want_reg, out=buf, zero=self._acc)
            return self._pat_buf[1], False
        if pre is not None and buf is not None and pre == self._premade_key(rays, KF, want_reg, buf):
            return buf[4], True
        self._pat_buf = ops.pattern_fwd_blur(rd, KF, self.sigma, s0, s1, self.blur[0], self.blur[1], want_softor=want_reg, out=buf, zero=self._acc)
        return self._pat_buf[4], False

    def _draw(self, seeds):
        """the appliers of this rank's samples: all their draws up front (each under its own seed), ONE device-to-host transfer — or the ones drawn
        ahead.  The NEXT step's are drawn now, ahead of this step's renders: device draws issued behind a render that fills the GPU only complete when
        it ends.  Their seeds are a function of the step index alone; the generators are put back afterwards."""
        ahead, self._ahead = self._ahead, None
        appliers = None
        if ahead is not None and ahead[0] == (self.step_index, tuple(seeds)):
            try:
                appliers = ahead[1]()
            except StaleDrawError:  # a sampler range was changed since: draw again (anything else — a failed native call, a HIP error — propagates)
                pass
        if appliers is None:
            appliers = self.ff_scene.randomize_batch(seeds)
        if self.ff_scene._draw_stream() is not None and not self.ff_scene._host_drawable():  # (draws evaluated on the host have nothing to wait for)
            nxt = self._sample_seeds(self.step_index + 1)
            self._ahead = ((self.step_index + 1, tuple(nxt)), self.ff_scene.randomize_batch(nxt, lazy=True))
        return appliers

    def _linear_buffers(self, n, device):
        """a linear loss's constant gradient image and a stack for the step's n renders (and the partial sums of the dot product of the two)"""
        cam, n_rays = self.mi_scene.data.camera, self.laser._rays.shape[0]
        shape = (cam.height, cam.width, 3)
        if self._dot_part is None or self._dot_part.numel() < n_rays:
            self._dot_part = torch.empty(n_rays, dtype=torch.float32, device=device)
        if self._lin_g is None or tuple(self._lin_g.shape) != shape:
            self._lin_g = self.loss_fn.linear_gradient(torch.empty(shape, device=device)).float().contiguous()  # (constant by definition)
        if self._img_stack is None or tuple(self._img_stack.shape) != (n,) + shape:
            self._img_stack = torch.empty((n,) + shape, dtype=torch.float32, device=device)
        return self._lin_g, self._img_stack

    def _samples_det(self, seeds, appliers, tex3, gtex, loss_slots):
        """FFX_DETERMINISTIC=1 (round 6): a step whose result does not depend on the number of ranks, BIT FOR BIT.  Every sample is re-traced twice
        (ffx_render_bwd_det_part): for the largest tap — maximum over the samples, then over the ranks: every rank derives the SAME power-of-two
        scale —, then as 64-bit fixed-point sums, summed over the ranks as integers (the same in any order and grouping; the seeds do not depend on
        the world size).  Pattern, Adam state and loss of a 1-, 2-, 4- or 8-rank run are equal; the default mode's float exchange agrees to ~1e-7."""
        ms, geom, S, dev, cam = self.mi_scene, self.mi_scene.geom, self.samples_per_step, gtex.device, self.mi_scene.data.camera
        vmax = torch.zeros(1, dtype=torch.int32, device=dev)
        lossv = torch.zeros(max(S, 1), dtype=torch.float32, device=dev)  # one slot per sample of the STEP: each rank fills its own
        kept = []
        for kg, seed, apply_sample in zip(dist.sample_ids(S, dist.rank(), dist.world_size()), seeds, appliers):
            apply_sample()
            sd = ms.scene_desc(tex_channels=1)
            mats = ms.materials_arg(sd)
            img = geom.render_fwd(sd, mats, tex3, self.spp, seed, False)
            gimg = self._image_loss(img, lossv[kg])
            geom.render_bwd_det_part(sd, mats, self.spp, seed, gimg, 1, vmax)
            kept.append((seed, apply_sample, gimg))
            self.step_paths["retrace"] += 1
        dist.allreduce_max_(vmax)
        dist.allreduce_sum_(lossv)  # (x + 0 is x: the slots arrive as their owners wrote them)
        sh = ops.det_scale_log2(int(vmax.item()), 4 * cam.width * cam.height * self.spp * max(S, 1))
        fix = torch.zeros(tex3.shape, dtype=torch.int64, device=dev)
        if sh is not None:
            for seed, apply_sample, gimg in kept:
                apply_sample()  # (the pose again: the second re-trace of this sample)
                sd = ms.scene_desc(tex_channels=1)
                geom.render_bwd_det_part(sd, ms.materials_arg(sd), self.spp, seed, gimg, 2, fix, scale_log2=sh)
        dist.allreduce_sum_(fix)
        if sh is not None:
            ops.det_finish_(fix, sh, gtex)
        loss_sum = loss_slots[0]
        loss_sum += lossv.double().sum().float()  # (the same S floats in the same order on every rank, whatever the world size)

    def _samples_fused(self, sd0, seeds, appliers, tex3, gtex):
        """K8 scatters each pixel's footprint x gimg into gtex and writes its image into the step's stack.  (Round 6) SEVERAL samples take the
        scene's two render streams in turn, as consecutive mi.render calls do, if the material rows travel in the scene description (a device table
        is rewritten per sample on the caller's stream: mi.Scene._render_stream's condition; the route has no base textures).  FFX_STEP_STREAMS=1:
        the caller's stream.  -> the render streams used"""
        ms, geom = self.mi_scene, self.mi_scene.geom
        lin_g, stack = self._linear_buffers(len(seeds), gtex.device)
        streams = ms._render_streams if (len(seeds) > 1 and int(sd0.n_mat_h) > 0 and os.environ.get("FFX_STEP_STREAMS", "2") != "1") else None
        used = []
        for k, (seed, apply_sample) in enumerate(zip(seeds, appliers)):
            apply_sample()  # host 4x4 algebra + K5/K6 on the side stream
            sd = ms.scene_desc(tex_channels=1)
            rs = None
            if streams is not None:
                if k == 0:
                    ready = torch.cuda.Event()
                    ready.record()  # (the texture, the cleared accumulator, the constant gradient: everything issued on the caller's stream so far)
                rs = streams[k & 1]
                if rs not in used:
                    rs.wait_event(ready)
                    used.append(rs)
            with torch.cuda.stream(rs) if rs is not None else contextlib.nullcontext():
                geom.render_fwd_adjoint(sd, ms.materials_arg(sd), tex3, self.spp, seed, lin_g, out=gtex, sparse_adjoint=True, img_out=stack[k])
            self.step_paths["fused"] += 1
        return used

    def _samples_cached(self, lin_rf, rf, seeds, appliers, tex3, gtex, loss_slots):
        """Cache-writing forward + K9 per sample.  Only the step's first render may clear the cache header's count of dropped samples: the Adam guard
        and _watch_cache read it at the END of the step (FFX_RENDER_CACHE_KEEP_DROPPED).  Which K9: lin_rf — the constant gradient, the image joins
        the step's stack; a linear loss on the box film — K9 also adds <gimg, img> to the loss slots; the L1 loss on the box film (FFX_K9_L1=1) — K9
        forms sign(img - target) / n and the loss itself (ffx_render_bwd_cached_l1), a declined sample takes the general way; the general way —
        the loss's gradient image, then K9."""
        ms, geom, cache, loss_sum = self.mi_scene, self.mi_scene.geom, self._cache, loss_slots[0]
        lin_g, stack = self._linear_buffers(len(seeds), gtex.device) if lin_rf else (None, None)
        linear = None if (lin_rf or rf) else getattr(self.loss_fn, "linear_gradient", None)
        l1t = None if (lin_rf or rf or os.environ.get("FFX_K9_L1", "1") == "0") else getattr(self.loss_fn, "l1_target", None)
        for k, (seed, apply_sample) in enumerate(zip(seeds, appliers)):
            apply_sample()
            sd = ms.scene_desc(tex_channels=1)
            mats = ms.materials_arg(sd)  # (None: the rows are part of sd — no upload, no device tensor)
            img = geom.render_fwd(sd, mats, tex3, self.spp, seed, False, cache=cache, sparse_adjoint=True, cache_zeroed=k == 0, keep_dropped=k != 0,
                                  img_out=stack[k] if lin_rf else None)
            self.step_paths["cache_k9"] += 1
            if lin_rf:
                geom.render_bwd_cached(sd, mats, cache, self.spp, lin_g, out=gtex, seed=seed)
            elif linear is not None:
                geom.render_bwd_cached(sd, mats, cache, self.spp, linear(img), out=gtex, img=img, dot_out=loss_slots)
            elif l1t is None or geom.render_bwd_cached_l1(sd, mats, cache, self.spp, img, l1t[0], l1t[1], gtex, loss_slots) is None:
                gimg = self._image_loss(img, loss_sum)
                geom.render_bwd_cached(sd, mats, cache, self.spp, gimg, out=gtex, seed=seed if rf else None)

    def _samples_retrace(self, seeds, appliers, tex3, gtex, loss_slots):
        """forward, the loss's gradient image, ffx_render_bwd re-tracing the sample"""
        ms, geom, loss_sum = self.mi_scene, self.mi_scene.geom, loss_slots[0]
        for k, (seed, apply_sample) in enumerate(zip(seeds, appliers)):
            apply_sample()
            sd = ms.scene_desc(tex_channels=1)
            mats = ms.materials_arg(sd)
            img = geom.render_fwd(sd, mats, tex3, self.spp, seed, False, cache=None, sparse_adjoint=False, cache_zeroed=k == 0, keep_dropped=k != 0,
                                  max_depth=self.max_depth, rr_depth=self.rr_depth)
            self.step_paths["retrace"] += 1
            gimg = self._image_loss(img, loss_sum)
            gtex += geom.render_bwd(sd, mats, self.spp, seed, gimg, max_depth=self.max_depth, rr_depth=self.rr_depth).reshape(gtex.shape)

    def _pattern_bwd_args(self):
        """rays, KF, texture size, the pattern launch's buffers, blur taps and regulariser weight of the gradient launches"""
        s0, s1 = self.tex_size
        _, tsum, tsor, ws = self._pat_buf[:4]
        bk, bs = (self.blur[0], self.blur[1]) if self.blur else (0, 1.0)
        return self.laser._rays.detach(), self.laser._KF, s0, s1, tsum, tsor, ws, bk, bs, (self.reg_weight if self.reg_weight > 0 else 0.0)

    def _update_exchanged(self, g2, dot, loss_in, grad, guard):
        """Several ranks (or one rehearsing the exchange): this rank's data term from the gradient launch (Adam arguments without state: no update),
        the exchange, then grad = gsum / S (+ regulariser, identical on every rank); Adam; Laser.clamp_to_fov() + normalize_rays() -> the loss"""
        rd, KF, s0, s1, tsum, tsor, ws, bk, bs, reg_w = self._pattern_bwd_args()
        S = float(self.samples_per_step)
        st, g = self._adam_state(self.laser._rays)
        aa = ops.adam_args(rd, None, None, None, self._adam_counter, 0.0, 0.0, 0.0, 0.0, self.laser._KF_inv, 0.0, 1.0, dot=dot) if dot is not None else None
        gd, gr, val = ops.pattern_bwd_blur(rd, KF, self.sigma, s0, s1, tsum, tsor, g2, reg_w, ws, bk, bs, loss_in=loss_in, loss_div=S, adam=aa,
                                           scratch=self._scratch)
        # (round 5) the cache's count of dropped samples (K9 then poisoned THIS rank's gradient with NaN): summed, every rank's update skips
        dropped = guard[8:12].view(torch.int32).float() if guard is not None else torch.zeros(1, device=rd.device)
        self._last_flat, gsum, loss, guard_sum = dist.exchange_step(gd if gd is not None else torch.zeros_like(rd), val[2:3], dropped)
        loss = loss / S + val[0]
        ops.adam_clamp_step_(rd, gsum, st["exp_avg"], st["exp_avg_sq"], st["step"], g["lr"], g["betas"][0], g["betas"][1], g["eps"], KF, self.laser._KF_inv,
                             1 - 0.95, 0.95, 2, grad_b=gr, grad_div=S, grad_out=grad, guard=guard_sum)
        self.laser._edits = getattr(self.laser, "_edits", 0) + 1
        return loss

    def _update_local(self, g2, dot, loss_in, grad, guard, used_premade):
        """Nothing to exchange: the backward half is ONE launch — gradients of the data term and the regulariser, the step's loss, and (by the last
        workgroup) Adam + Laser.clamp_to_fov() + normalize_rays(), skipped when the cache header (`guard`) reports dropped samples.  (Round 6)
        ffx_pattern_step also makes the NEXT step's K1 + K2 + K3 behind the update; footprints that do not fit its LDS window take ffx_pattern_bwd
        (+ the next step's ffx_pattern_fwd).  -> the loss"""
        rd, KF, s0, s1, tsum, tsor, ws, bk, bs, reg_w = self._pattern_bwd_args()
        S = float(self.samples_per_step)
        st, g = self._adam_state(self.laser._rays)
        aa = ops.adam_args(rd, st["exp_avg"], st["exp_avg_sq"], st["step"], self._adam_counter, g["lr"], g["betas"][0], g["betas"][1], g["eps"], self.laser._KF_inv,
                           1 - 0.95, 0.95, 2, grad_div=S, grad_out=grad, dot=dot, guard=guard)
        res = None
        if self.blur and bk == 5 and g2 is not None and os.environ.get("FFX_PATTERN_STEP", "1") != "0":
            if self._rays_kept is None or tuple(self._rays_kept.shape[1:]) != tuple(rd.shape):
                self._pat_sync = torch.zeros(_abi.PATTERN_SYNC_BYTES, dtype=torch.uint8, device=rd.device)
                self._rays_kept = torch.empty((2,) + tuple(rd.shape), dtype=torch.float32, device=rd.device)
                self._pat_epoch = 0
                used_premade = False  # (nothing kept to compare with)
            res = ops.pattern_step(rd, KF, self.sigma, s0, s1, self._pat_buf, g2, reg_w, bk, bs, aa, self._acc, self._pat_sync, rays_kept=self._rays_kept,
                                   check_kept=used_premade, loss_in=loss_in, loss_div=S, epoch=self._pat_epoch % 0xFFFFFFF0 + 1)
            if res is not None:
                self._pat_epoch += 1
                self.laser._edits = getattr(self.laser, "_edits", 0) + 1  # (this update, counted before the key is taken: ANOTHER optimiser's is not in it)
                self._premade = self._premade_key(self.laser._rays, KF, self.reg_weight > 0, self._pat_buf)
                self._merged_last = True
        if res is None:
            res = ops.pattern_bwd_blur(rd, KF, self.sigma, s0, s1, tsum, tsor, g2, reg_w, ws, bk, bs, loss_in=loss_in, loss_div=S, adam=aa, scratch=self._scratch)
            self.laser._edits = getattr(self.laser, "_edits", 0) + 1  # (a native update of the pattern: torch's version counter does not see it)
        return res[2][1]

    def _premade_key(self, rays, KF, want_reg, buf):
        """what must be unchanged for the texture made by the previous step's pattern launch to be THIS step's texture: the pattern tensor (storage and
        torch's version counter: in-place edits through torch bump it; the native update does not), the laser's own edit count, the accumulator the launch
        cleared, the five texture buffers, and every setting of K1-K3.  (Edits torch cannot see — `rays.data` written in place — are caught on the device:
        ffx_pattern_step compares the pattern's bits with the ones it kept and raises `stale`, which _watch_cache turns into an error.)"""
        return (rays.data_ptr(), rays._version, tuple(rays.shape), getattr(self.laser, "_edits", 0), self._acc.data_ptr(), self._acc.numel(),
                tuple(b.data_ptr() if b is not None else 0 for b in buf), float(self.sigma), tuple(self.tex_size), tuple(self.blur) if self.blur else None, bool(want_reg),
                KF.tobytes() if hasattr(KF, "tobytes") else tuple(float(v) for v in torch.as_tensor(KF).reshape(-1).tolist()))

    def invalidate_texture(self):
        """forget the texture the last step made ahead for the next one (call after editing the pattern behind torch's back, e.g. through `rays.data`)"""
        self._premade = None

    def _drop_arena(self):
        """forget the arena and everything that lives in it — accumulator, adjoint cache, the texture made ahead into them; the next step makes a new one"""
        self._arena = self._acc = self._cache = self._premade = None

    def _watch_cache(self, every=32):
        """The adjoint cache is lossy once its arena of single-sample records is full (include/ffx.h
        ffx_render_cache_status; K9 then poisons the gradient with NaN).  Every `every` steps the 64-byte cache header is
        copied to pinned host memory behind the step's kernels and inspected once it has landed — the host never waits."""
        w = self._watch
        if w is not None and w[1].query():
            words = w[0].tolist()
            self._watch = None
            if w[3]:  # (behind ffx_pattern_step: its sync words — `stale` in word 4, the header as the step left it in words 18..33)
                if words[5]:
                    raise RuntimeError(f"PatternOptimizer: a pattern launch around step {w[2]} gave up waiting for its own update (ffx_pattern_step's `timeout`): "
                                       "the texture of the step after it is incomplete.  Set FFX_PATTERN_STEP=0 and report this.")
                if words[4]:
                    raise RuntimeError(
                        f"PatternOptimizer: the pattern was edited in place between two steps in a way torch does not record (around step {w[2]}: e.g. through "
                        "`laser._rays.data`), and the step after the edit rendered with the texture of the unedited pattern.  Call invalidate_texture() after "
                        "such an edit (or set FFX_PATTERN_STEP=0).")
                words = words[18:34]
            used, cap, dropped = words[:3] if w[4] else (0, 0, 0)
            if dropped:
                import warnings

                # the steps since then were NOT applied (ffx_adam_args.guard / ffx_adam_clamp_step's guard: the update launch skips when the header
                # — with several ranks: the exchanged sum of the ranks' headers — reports drops), so the optimiser state is intact and identical on
                # every rank.  One process switches to the re-tracing adjoint by itself; several ranks cannot decide that alone (a rank whose
                # OWN cache never overflowed would keep the cache: the ranks' launches must stay in step), so they raise — with clean state.
                if dist.world_size() > 1:
                    raise Fn.CacheOverflowError(
                        f"PatternOptimizer: the adjoint cache of step {w[2]} overflowed on this rank ({dropped} samples beyond its {cap} single-sample "
                        "records); the updates since then were skipped on every rank (rays and Adam state are intact). Set FFX_CACHE_LIMIT_GB=0 "
                        "(re-tracing adjoint) on all ranks and continue.")
                self._drop_arena()
                if getattr(self.mi_scene, "_rfilter", None) is not None and not getattr(self.mi_scene, "_cache_dense", False):
                    # the filtered film's cache: an arena with a share of the blocks (a quarter beyond 2^18) — a pattern that lights more of the film than
                    # that gets the dense layout (FFX_SHADOWS_CACHE_DENSE: cannot overflow) instead of the re-tracing adjoint
                    self.mi_scene.set_cache_dense(True)
                    warnings.warn(f"PatternOptimizer: the filtered film's adjoint cache of step {w[2]} overflowed ({dropped} blocks beyond its {cap}); the updates of the "
                                  "affected steps were skipped; from now on the cache keeps a block for every pass of every pixel.", stacklevel=3)
                    return
                self._cache_overflowed = True
                warnings.warn(f"PatternOptimizer: the adjoint cache of step {w[2]} overflowed ({dropped} samples beyond its {cap} single-sample records: a projector "
                              "texture much finer than the camera's pixels, or grazing views).  The updates of the affected steps were skipped; this optimiser "
                              "now uses the re-tracing adjoint (ffx_render_bwd).", stacklevel=3)
        merged = self._merged_last
        if self._watch is None and (self._cache is not None or merged) and (self.step_index - 1) % every == 0:
            if self._watch_pin is None:
                self._watch_pin = torch.empty(64, dtype=torch.int32, pin_memory=True)
            pin = self._watch_pin
            if merged:  # (the launch has cleared the cache's header for the next step; it kept a copy)
                pin.copy_(self._pat_sync[:256].view(torch.int32), non_blocking=True)
            else:
                pin[:16].copy_(self._cache[:64].view(torch.int32), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._watch = (pin, ev, self.step_index - 1, merged, self._cache is not None)

    # ------------------------------------------------------------------ the same step through autograd
    def step_autograd(self):
        """reference implementation of `step` on torch.autograd (kept for validation and for task
        losses / pipelines that need the graph)."""
        self.opt.zero_grad(set_to_none=True)
        rays = self.laser._rays
        pts, tsum, tex = self.textures()
        S = self.samples_per_step
        r, w = dist.rank(), dist.world_size()
        gtex = torch.zeros_like(tex)
        loss_sum = torch.zeros((), device=tex.device)
        for k in dist.sample_ids(S, r, w):
            g, l = self._render_sample(tex, dist.sample_seed(self.base_seed, self.step_index, S, k))
            gtex += g
            loss_sum += l
        # back through K3^T, K2-bwd, K1-bwd for this rank's share
        tex.backward(gtex, retain_graph=self.reg_weight > 0)
        flat, gsum, loss, _ = dist.exchange_step(rays.grad, loss_sum)  # ([3N+1]: nothing is dropped without a cache)
        flat /= float(S)
        rays.grad = gsum.clone()
        if self.reg_weight > 0:  # identical on every rank (depends on the pattern only)
            s0, s1 = self.tex_size
            tsor = Fn.splat(pts, self.sigma, s0, s1, "softor", -1)
            reg = self.reg_weight * (tsor - tsum).abs().mean()
            (greg,) = torch.autograd.grad(reg, rays)
            rays.grad += greg
            loss = loss + reg.detach()
        self.opt.step()
        self.laser.clamp_to_fov()
        self.laser.normalize_rays()
        self.step_index += 1
        return {"loss": loss}
