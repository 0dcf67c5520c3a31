"""Launch times of ffx_connected_components at 512 x 512 on two inputs: the mask "everything but the glottis" of one seeded
vocal-fold pose, and a random mask of density 0.593 (the 4-neighbour site-percolation threshold: long union chains).  Per input 20 full calls
(labels + statistics, 8-connected), then 20 count-only calls (what graphics.accept_segmentation runs), one after the other on one stream.
    rocprofv3 --kernel-trace --stats -d DIR -o cc --output-format csv -- python tools/cctime.py     the run
    python tools/cctime.py --parse DIR/.../cc_kernel_trace.csv                                    median time per k_cc_* launch and per call
"""
import csv
import os
import random
import statistics
import sys

REPEAT, WARM = 20, 3
PHASES = ("vocal fold, labels + stats", "random 0.593, labels + stats", "vocal fold, count only", "random 0.593, count only")


def run():
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fireflies_amd as ff
    from fireflies_amd import ops, workloads

    wl = workloads.vocalfold(device="cuda")
    torch.manual_seed(3)
    random.seed(3)
    wl.ff_scene.randomize()
    fold = (ff.graphics.depth.get_segmentation_from_camera(wl.mi_scene) != 2).contiguous()
    noise = torch.from_numpy(np.random.default_rng(0).random((512, 512)) < 0.593).cuda()
    for full in (True, False):
        for m in (fold, noise):
            for _ in range(WARM + REPEAT):
                c = ops.connected_components(m, 8, labels=full, stats=full)
            torch.cuda.synchronize()
            print(f"{tuple(m.shape)} foreground {float(m.float().mean()):.3f}: n_labels {int(c.n_labels)}")


def parse(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_cc_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:  # a call begins with its tile pass
        name = r["Kernel_Name"].replace("void ", "").split("(")[0].removesuffix(".kd")
        if "k_cc_tile" in name:
            calls.append([])
        calls[-1].append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    per = WARM + REPEAT
    assert len(calls) == per * len(PHASES), len(calls)
    for k, what in enumerate(PHASES):
        timed = calls[k * per + WARM:(k + 1) * per]
        names = [n for n, _, _ in timed[0]]
        parts = ", ".join(f"{n} {statistics.median(c[i][2] - c[i][1] for c in timed) / 1e3:.2f}" for i, n in enumerate(names))
        busy = statistics.median(sum(e - s for _, s, e in c) for c in timed) / 1e3
        span = statistics.median(c[-1][2] - c[0][1] for c in timed) / 1e3
        print(f"{what}: {parts}; kernels {busy:.2f} us, first start to last end {span:.2f} us (medians of {REPEAT})")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        run()
