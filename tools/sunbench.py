"""The directional emitter's cost: ms per render_fwd call of the 512^2 x 64-spp vocal fold without extra emitters, with 1 point light,
with 1 sun, with 1 point light + 1 sun and with 1 sun + the constant emitter, on the box and the gaussian film, at direct light and at max_depth 3 — all
alternating in one loop, HIP events around each call, median of the repetitions after two warm-up rounds.  The point light is tools/lightsbench.py's
first (beside the camera, looking into the larynx); the sun shines down the larynx from the camera's side.  The 1-point-light figure of the same run is
the yardstick: the lights' pass is a per-lane pass behind the main image's launches, there is no threshold, the figures are what they are.  Prints one
JSON line.

    python tools/sunbench.py [reps]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fireflies_amd import ops, scenes, workloads  # noqa: E402

AMBIENT = (0.2, 0.25, 0.3)


def point_light():
    tw = np.eye(4, dtype=np.float32)
    tw[:3, 3] = (0.3, 0.0, 1.5)
    return scenes.LightData("emit-Light0", "point", tw, (2.0, 2.0, 2.0))


def sun():
    z = np.array([0.1, -0.1, -1.0])
    z /= np.linalg.norm(z)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    tw = np.eye(4)
    tw[:3, 0], tw[:3, 1], tw[:3, 2] = x, np.cross(z, x), z
    return scenes.LightData("emit-Sun", "directional", tw.astype(np.float32), (0.5, 0.5, 0.5))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    wl = workloads.vocalfold(device="cuda", width=512, height=512, grid=16)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    geom, out = wl.mi_scene.geom, {"res": 512, "spp": 64, "reps": reps}
    # name -> (the lights, the constant emitter)
    cases = {"none": ([], None), "point": ([point_light()], None), "sun": ([sun()], None), "point_sun": ([point_light(), sun()], None), "sun_ambient": ([sun()], AMBIENT)}
    args = {k: dict(lights=ops.pack_lights(l).to("cuda") if l else None, ambient=a, lights_directional=ops.lights_directional(l)) for k, (l, a) in cases.items()}
    for film in ("box", "gaussian"):
        wl.mi_scene.rfilter = film
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        calls = {(depth, k): (lambda depth=depth, k=k: geom.render_fwd(sd, mats, tex, 64, 1, max_depth=depth, **args[k])) for depth in (2, 3) for k in cases}
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
        for (depth, k), v in times.items():
            out[f"render_ms_{film}_d{depth}_{k}"] = round(sorted(v)[len(v) // 2], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
