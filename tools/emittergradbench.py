"""The cost of the extra emitters' adjoint: ms per render_bwd call of the 512^2 x 64-spp vocal fold with and without emitters=True, for 1
point light, 1 sun, 1 point light + 1 sun + the constant emitter, and 8 records (points and suns in turn), at direct light and at max_depth 3, on the box
and the gaussian film — all alternating in one loop, HIP events around each call, median of the repetitions after two warm-up rounds.  The yardstick
is what the lights' pass costs the forward in the same run: render_fwd with the table minus render_fwd without it (the parent's code, measured beside
the new code).  The adjoint makes the same walk plus 27 multiply-adds per vertex, and one small launch that sums the pixels' slots.  There is no
threshold: the figures are what they are.  Prints one JSON line: per film, depth and case fwd_pass_ms (the yardstick), bwd_ms, bwd_emitters_ms and
grad_pass_ms (their difference).

    python tools/emittergradbench.py [reps]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fireflies_amd import ops, scenes, workloads  # noqa: E402

AMBIENT = (0.2, 0.25, 0.3)


def point_light(k=0):
    tw = np.eye(4, dtype=np.float32)
    tw[:3, 3] = (0.3 * np.cos(0.8 * k), 0.3 * np.sin(0.8 * k), 1.5)
    return scenes.LightData(f"emit-Light{k}", "point", tw, (2.0, 2.0, 2.0))


def sun(k=0):
    z = np.array([0.1 * np.cos(0.8 * k), -0.1 * np.sin(0.8 * k + 1.0), -1.0])
    z /= np.linalg.norm(z)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    tw = np.eye(4)
    tw[:3, 0], tw[:3, 1], tw[:3, 2] = x, np.cross(z, x), z
    return scenes.LightData(f"emit-Sun{k}", "directional", tw.astype(np.float32), (0.5, 0.5, 0.5))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    wl = workloads.vocalfold(device="cuda", width=512, height=512, grid=16)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    geom, out = wl.mi_scene.geom, {"res": 512, "spp": 64, "reps": reps}
    gimg = (0.5 + torch.rand((512, 512, 3), generator=torch.Generator().manual_seed(0))).to("cuda")
    # name -> (the lights, the constant emitter)
    cases = {"point": ([point_light()], None), "sun": ([sun()], None), "point_sun_ambient": ([point_light(), sun()], AMBIENT),
             "eight": ([point_light(k) if k % 2 == 0 else sun(k) for k in range(8)], None)}
    args = {k: dict(lights=ops.pack_lights(l).to("cuda"), ambient=a, lights_directional=ops.lights_directional(l)) for k, (l, a) in cases.items()}
    for film in ("box", "gaussian"):
        wl.mi_scene.rfilter = film
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        calls = {}
        for depth in (2, 3):
            calls[(depth, "none", "fwd")] = lambda depth=depth: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth)
            for k in cases:
                calls[(depth, k, "fwd")] = lambda depth=depth, k=k: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth, **args[k])
                calls[(depth, k, "bwd")] = lambda depth=depth, k=k: geom.render_bwd(sd, mats, 64, 1, gimg, max_depth=depth, **args[k])
                calls[(depth, k, "bwd_emitters")] = lambda depth=depth, k=k: geom.render_bwd(sd, mats, 64, 1, gimg, max_depth=depth, emitters=True, **args[k])
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
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for depth in (2, 3):
            for k in cases:
                pre = f"{film}_d{depth}_{k}"
                out[f"fwd_pass_ms_{pre}"] = round(med[(depth, k, "fwd")] - med[(depth, "none", "fwd")], 3)
                out[f"bwd_ms_{pre}"] = round(med[(depth, k, "bwd")], 3)
                out[f"bwd_emitters_ms_{pre}"] = round(med[(depth, k, "bwd_emitters")], 3)
                out[f"grad_pass_ms_{pre}"] = round(med[(depth, k, "bwd_emitters")] - med[(depth, k, "bwd")], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
