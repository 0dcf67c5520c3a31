"""The extra emitters' cost: ms per render_fwd call of the 512^2 x 64-spp vocal fold with 0, 1, 4 and 8 extra point lights, on the box
and the gaussian film, at direct light and at max_depth 3 — all alternating in one loop next to the plain render_fwd (0 lights) of the same run, HIP
events around each call, median of the repetitions after two warm-up rounds.  The lights stand about the camera and look into the larynx.  A per-lane
pass behind the main image's launches: no threshold, the figures are what they are.  Prints one JSON line.

    python tools/lightsbench.py [reps]
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fireflies_amd import ops, scenes, workloads  # noqa: E402


def point_lights(n):
    out = []
    for k in range(n):
        a = 2.0 * math.pi * k / 8.0
        tw = np.eye(4, dtype=np.float32)
        tw[:3, 3] = (0.3 * math.cos(a), 0.3 * math.sin(a), 1.5 + 0.05 * k)
        out.append(scenes.LightData(f"emit-Light{k}", "point", tw, (2.0, 2.0, 2.0)))
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    wl = workloads.vocalfold(device="cuda", width=512, height=512, grid=16)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    geom, out = wl.mi_scene.geom, {"res": 512, "spp": 64, "reps": reps}
    tables = {n: (ops.pack_lights(point_lights(n)).to("cuda") if n else None) for n in (0, 1, 4, 8)}
    for film in ("box", "gaussian"):
        wl.mi_scene.rfilter = film
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        calls = {(depth, n): (lambda depth=depth, n=n: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth, lights=tables[n])) for depth in (2, 3) for n in tables}
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
        for (depth, n), v in times.items():
            out[f"render_ms_{film}_d{depth}_lights{n}"] = round(sorted(v)[len(v) // 2], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
