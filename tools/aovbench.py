"""The AOV block's cost: ms per call on the 512^2 vocal fold at 64 and 16 samples per pixel, box and gaussian film — render_fwd,
render_aov (the whole call: the render and the block's launches) and trace_primary at the same sample count, alternating in one loop, HIP events
around each call, median of the repetitions after two warm-up rounds.  Prints one JSON line.

    python tools/aovbench.py [reps]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fireflies_amd import workloads  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    wl = workloads.vocalfold(device="cuda", width=512, height=512, grid=16)
    torch.manual_seed(0)
    wl.ff_scene.randomize()
    tex = workloads.build_texture(wl).detach().unsqueeze(-1).contiguous()
    geom, out = wl.mi_scene.geom, {"res": 512, "reps": reps}
    for film in ("box", "gaussian"):
        wl.mi_scene.rfilter = film
        sd = wl.mi_scene.scene_desc(tex_channels=1)
        mats = wl.mi_scene.materials_arg(sd)
        for spp in (64, 16):
            calls = {"render_fwd": lambda: geom.render_fwd(sd, mats, tex, spp, 1),
                     "render_aov": lambda: geom.render_aov(sd, mats, tex, spp, 1),
                     "trace_primary": lambda: geom.trace_primary(sd.cam, spp=spp, jitter=1, seed=1)}
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
                out[f"{k}_ms_{film}_{spp}spp"] = round(sorted(v)[len(v) // 2], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
