"""The path integrator's cost: ms per 512^2 x 64-spp vocal-fold render at max_depth 2 (the packet kernels), 3 and 4 (the per-lane
path kernel), box and gaussian film, and ms per gradient sample (forward + loss gradient image + replay adjoint) at max_depth 3.  HIP events
around repeated calls of one pose on one stream, after a warm-up.  Then the `prb` adjoint at max_depth 3 and 4:
render_bwd_prb with and without the material block next to render_bwd (k_path_bwd) at the same depth, and forward mode (render_jvp, DESIGN.md
4.5.3: primal + tangent image) next to render_fwd, all alternating in one loop, median of the repetitions after two warm-up rounds.  Prints one JSON line.

    python tools/pathbench.py [reps]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fireflies_amd import ops, workloads  # noqa: E402


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    wl = workloads.vocalfold(device="cuda", width=512, height=512, grid=16)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    geom, out = wl.mi_scene.geom, {"res": 512, "spp": 64, "reps": reps}
    for film in ("box", "gaussian"):
        wl.mi_scene.rfilter = film
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        for depth in (2, 3, 4):
            out[f"render_ms_{film}_d{depth}"] = round(_ms(lambda: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth), reps), 3)
        gimg = torch.full((sd.cam.height, sd.cam.width, 3), -1.0 / (sd.cam.height * sd.cam.width), device="cuda")

        def grad_sample():
            geom.render_fwd(sd, mats, tex, 64, 1, max_depth=3)
            geom.render_bwd(sd, mats, 64, 1, gimg, max_depth=3)

        out[f"grad_sample_ms_{film}_d3"] = round(_ms(grad_sample, reps), 3)
        S = sd.n_shapes
        tan = ops.AppearanceGrad(torch.rand((S, 3), device="cuda"), torch.rand(3, device="cuda"), [torch.rand_like(t) for _, t in wl.mi_scene._base_tex],
                                 torch.rand((S, 11), device="cuda") if sd.mat_stride == 16 else None)
        dtex = torch.rand_like(tex)
        for depth in (3, 4):
            calls = {"path_bwd": lambda: geom.render_bwd(sd, mats, 64, 1, gimg, max_depth=depth),
                     "prb_bwd": lambda: geom.render_bwd_prb(sd, mats, 64, 1, gimg, tex, depth),
                     "prb_material_bwd": lambda: geom.render_bwd_prb(sd, mats, 64, 1, gimg, tex, depth, material=True),
                     # forward mode: the whole call, primal render + tangent image through the bounces, and the render alone
                     "jvp": lambda: geom.render_jvp(sd, wl.mi_scene.albedo, tex, 64, 1, dtex=dtex, tangent=tan, max_depth=depth),
                     "fwd": lambda: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth)}
            times = {k: [] for k in calls}
            for rep in range(reps + 2):
                for k, fn in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    if rep >= 2:
                        times[k].append(a.elapsed_time(b))
            for k, v in times.items():
                out[f"{k}_ms_{film}_d{depth}"] = round(sorted(v)[len(v) // 2], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
