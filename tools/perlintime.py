"""Launch times of ffx_perlin_texture at 1024 x 1024 in the renderer's layout on the corners of what the dataset loop's sampler
draws — lattice 2 and 64, one and four octaves — and on 20 seeded draws of the sampler itself.  Per configuration 20 calls behind 3 warm-up calls, one
after the other on one stream.
    rocprofv3 --kernel-trace --stats -d DIR -o perlin --output-format csv -- python tools/perlintime.py     the run
    python tools/perlintime.py --parse DIR/.../perlin_kernel_trace.csv                                    median time per k_perlin_* launch and per call
"""
import csv
import math
import os
import random
import statistics
import sys

REPEAT, WARM = 20, 3
SHAPE = (1024, 1024)
CONFIGS = ((2, 1), (2, 4), (64, 1), (64, 4))  # (lattice, octaves)
PHASES = tuple(f"lattice {r}, {o} octave{'s' if o > 1 else ''}" for r, o in CONFIGS) + ("the sampler's draws (seed 0)",)


def run():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fireflies_amd import ops
    from fireflies_amd.sampling import NoiseTextureLerpSampler
    from fireflies_amd.sampling.noise_texture_lerp import position_tables

    ca, cb = torch.rand(3, device="cuda"), torch.rand(3, device="cuda")
    for r, o in CONFIGS:
        angles = (2 * math.pi * torch.rand(ops.perlin_angle_count((r, r), o))).cuda()
        pos = position_tables(SHAPE, (r, r), o).cuda()
        for _ in range(WARM + REPEAT):
            t = ops.perlin_texture(angles, pos, o, (r, r), 0.7, SHAPE, ca, cb)
        torch.cuda.synchronize()
        print(f"lattice {r}, octaves {o}: texture {tuple(t.shape)}, mean {float(t.mean()):.4f}")
    smp = NoiseTextureLerpSampler(ca, cb, SHAPE, device="cuda", engine="device")
    torch.manual_seed(0)
    random.seed(0)
    for _ in range(WARM + REPEAT):
        t = smp.sample()
    torch.cuda.synchronize()
    print(f"sampler: texture {tuple(t.shape)}, mean {float(t.mean()):.4f}")


def parse(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_perlin_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:  # a call begins with its extremes pass over the tiles
        name = r["Kernel_Name"].replace("void ", "").split("(")[0].removesuffix(".kd")
        if "k_perlin_tile<false>" in name:
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
