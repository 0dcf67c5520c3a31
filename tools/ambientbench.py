"""The constant emitter's cost: ms per render_fwd call of the 512^2 x 64-spp vocal fold with {no extras, ambient only, 1 point light,
1 point light + ambient}, on the box and the gaussian film, at direct light and at max_depth 3 — all alternating in one loop, HIP events around each
call, median of the repetitions after two warm-up rounds.  The comparison that matters: `light+ambient` against `light` is what the constant emitter
costs inside a walk that runs anyway (its closing ray, its adds); `ambient` against `plain` is what a pass of its own costs — sharing the walk saves the
difference.  No threshold, the figures are what they are.  Prints one JSON line.

    python tools/ambientbench.py [reps]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fireflies_amd import ops, scenes, workloads  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    wl = workloads.vocalfold(device="cuda", width=512, height=512, grid=16)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    geom, out = wl.mi_scene.geom, {"res": 512, "spp": 64, "reps": reps}
    tw = np.eye(4, dtype=np.float32)
    tw[:3, 3] = (0.3, 0.0, 1.5)
    light = ops.pack_lights([scenes.LightData("emit-Light0", "point", tw, (2.0, 2.0, 2.0))]).to("cuda")
    world = torch.tensor([0.2, 0.2, 0.25], device="cuda")  # (a device record: no host-to-device copy inside the bracket)
    arms = {"plain": {}, "ambient": {"ambient": world}, "light": {"lights": light}, "light_ambient": {"lights": light, "ambient": world}}
    for film in ("box", "gaussian"):
        wl.mi_scene.rfilter = film
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        calls = {(depth, arm): (lambda depth=depth, kw=kw: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth, **kw)) for depth in (2, 3) for arm, kw in arms.items()}
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
        for (depth, arm), v in times.items():
            out[f"render_ms_{film}_d{depth}_{arm}"] = round(sorted(v)[len(v) // 2], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
