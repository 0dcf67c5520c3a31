"""The dataset path of the reference's main.py:138-175 as a loop on the device: per sample
`ff_scene.randomize()` -> `mi.render(scene, spp)` -> grey image -> post-processing chain (blur p=0.5, silhouette,
white noise p=0.5) -> segmentation + depth map of the same pose.  Nothing leaves the GPU inside the loop (the
reference copies the render to the host and runs kornia / cv2 / numpy there).  Prints samples/s.
With `accept` the loop also covers main.py:168-180: per sample the flag "the segmentation is not empty and everything but the glottis
falls into at most two pieces" (graphics.accept_segmentation: connected components on the device, no host read), the loop is timed
without and with it in turn, all flags are read once behind the loop, and the host's route to the same flag — seg.cpu() plus
scipy.ndimage.label where scipy is importable, the numpy restatement tests/ref_components.py otherwise — is timed beside it.
With `perlin` the loop also covers main.py:147-153, its first lines: per sample two colour draws, a 1024 x 1024 NoiseTextureLerpSampler texture and its
assignment to `mat-Mucosa.brdf_0.base_color.data` of the workload with a textured larynx.  The loop is timed with the sampler's torch engine and with
its device engine (one call into the library) in turn, both under the same seeds, and one sample() with a synchronise behind it is
timed beside them for each engine.
    python tools/datasetbench.py [n_samples] [spp | mix] [accept | perlin]"""
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fireflies_amd as ff  # noqa: E402
import fireflies_amd.postprocessing as pp  # noqa: E402
from fireflies_amd import mi, workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
spp = sys.argv[2] if len(sys.argv) > 2 else "64"
MIX = spp == "mix"  # main.py:145 draws every sample's spp: fireflies.sampling.AnimationSampler(1, 100, 1, 100) — here uniform in 1..100 from python's `random`
spp = 64 if MIX else int(spp)
ACCEPT = len(sys.argv) > 3 and sys.argv[3] == "accept"
PERLIN = len(sys.argv) > 3 and sys.argv[3] == "perlin"
wl = workloads.vocalfold(device="cuda", textured=PERLIN)
with torch.no_grad():
    wl.params["tex.data"] = workloads.build_texture(wl).contiguous()
chain = pp.PostProcessor([pp.GaussianBlur((3, 3), (5, 5), 0.5), pp.ApplySilhouette(), pp.WhiteNoise(0.0, 0.05, 0.5, rng="device")])
torch.manual_seed(0)
random.seed(0)


def sample(i, flags=None, lerp=None):
    if lerp is not None:  # main.py:147-153
        lerp._color_a = torch.rand(3, device="cuda")
        lerp._color_b = torch.rand(3, device="cuda")
        wl.params["mat-Mucosa.brdf_0.base_color.data"] = mi.TensorXf(lerp.sample().moveaxis(0, -1))
    wl.ff_scene.randomize()
    img = mi.render(wl.mi_scene, spp=random.randint(1, 100) if MIX else spp, seed=i).torch()
    grey = pp.rgb_to_gray(img)  # cv2.COLOR_RGB2GRAY's weights, one launch (as a torch expression: five)
    out = chain.post_process(grey)
    seg = ff.graphics.depth.get_segmentation_from_camera(wl.mi_scene)
    depth = ff.graphics.depth.from_camera_non_wrapped(wl.mi_scene, spp=1)
    if ACCEPT and flags is not None:
        flags.append(ff.graphics.accept_segmentation(seg))
    return out, seg, depth


for i in range(10):
    sample(i)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(n):
    keep = sample(10 + i)
t_issue = time.perf_counter() - t0
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"host issued the {n} samples in {1e3 * t_issue / n:.3f} ms each; the device finished {1e3 * (dt - t_issue):.2f} ms after the last was issued")
print(f"dataset path: {n / dt:.1f} samples/s ({1e3 * dt / n:.3f} ms per sample: render {'1..100 (drawn per sample)' if MIX else spp} spp + post-processing + segmentation + depth, 512x512), "
      f"outputs {tuple(keep[0].shape)} {tuple(keep[1].shape)} {tuple(keep[2].shape)}")

if ACCEPT:
    import statistics

    import numpy as np

    def loop(flags):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for j in range(n):
            sample(10 + j, flags)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    without, with_flag, flags = [], [], []
    loop([])  # warm-up of the labelling launches
    for _ in range(7):  # in turn, so that both see the same drift
        without.append(loop(None))
        flags = []
        with_flag.append(loop(flags))
    kept = torch.stack(flags).cpu()  # the one host read: every flag of the last loop
    t_off, t_on = statistics.median(without), statistics.median(with_flag)
    print(f"acceptance (main.py:168-180), median of 7 loops of {n}: {n / t_off:.1f} samples/s without the flag, {n / t_on:.1f} with it "
          f"({1e6 * (t_on - t_off) / n:+.1f} us per sample); kept {int(kept.sum())} of {n} ({100.0 * float(kept.float().mean()):.1f} %)")
    try:  # the host's route to the same flag on the last pose
        from scipy import ndimage

        def host_label(mask):
            return ndimage.label(mask, structure=np.ones((3, 3), int))[1] + 1

        how = "scipy.ndimage.label"
    except ImportError:
        from tests import ref_components

        def host_label(mask):
            return ref_components.label(mask, 8)[0]

        how = "tests/ref_components.py (scipy is not importable here)"
    seg = keep[1]
    torch.cuda.synchronize()
    host_t = []
    for _ in range(7):
        t = time.perf_counter()
        h = seg.cpu().numpy()
        flag_h = bool(h.max() != 0 and host_label(h != 2) <= 3)
        host_t.append(time.perf_counter() - t)
    dev_t = []
    for _ in range(7):
        torch.cuda.synchronize()
        t = time.perf_counter()
        flag_d = ff.graphics.accept_segmentation(seg)
        torch.cuda.synchronize()
        dev_t.append(time.perf_counter() - t)
    assert bool(flag_d) is flag_h
    print(f"one flag on a {tuple(seg.shape)} label image, median of 7: host route (seg.cpu() + {how}) {1e6 * statistics.median(host_t):.0f} us, "
          f"device call with a synchronise behind it {1e6 * statistics.median(dev_t):.0f} us")

if PERLIN:
    import statistics

    from fireflies_amd.sampling import NoiseTextureLerpSampler

    SHAPE = (1024, 1024)
    lerps = {e: NoiseTextureLerpSampler(torch.zeros(3), torch.ones(3), SHAPE, device="cuda", engine=e) for e in ("torch", "device")}

    def loop(lerp, seed):
        torch.manual_seed(seed)  # (both engines draw the same lattices in a round)
        random.seed(seed)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for j in range(n):
            sample(10 + j, lerp=lerp)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    times = {e: [] for e in lerps}
    for e in lerps:
        loop(lerps[e], 0)  # warm-up: the position tables, the pinned buffers, torch's allocations
    for k in range(7):  # in turn, so that both see the same drift
        for e in lerps:
            times[e].append(loop(lerps[e], 1 + k))
    med = {e: statistics.median(v) for e, v in times.items()}
    print(f"textured dataset path (main.py:147-153 in front of each sample, {SHAPE[0]} x {SHAPE[1]} texture), median of 7 loops of {n}: "
          f"{n / med['torch']:.1f} samples/s with engine='torch', {n / med['device']:.1f} with engine='device' "
          f"({1e6 * (med['device'] - med['torch']) / n:+.1f} us per sample)")
    one = {}
    for e in lerps:
        torch.manual_seed(100)
        random.seed(100)
        ts = []
        for _ in range(3 + 21):
            torch.cuda.synchronize()
            t = time.perf_counter()
            tex = lerps[e].sample()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        one[e] = statistics.median(ts[3:])
    print(f"one sample() of {SHAPE[0]} x {SHAPE[1]} with a synchronise behind it, median of 21 under the same seeds: engine='torch' {1e6 * one['torch']:.0f} us, "
          f"engine='device' {1e6 * one['device']:.0f} us")

if os.environ.get("FFX_DS_PROFILE") == "1":  # where the host's time per sample goes (cProfile, 200 samples at 1 spp so that the device is not the limit)
    import cProfile
    import pstats

    spp = 1
    pr = cProfile.Profile()
    pr.enable()
    for i in range(200):
        sample(i)
    pr.disable()
    torch.cuda.synchronize()
    pstats.Stats(pr).sort_stats("cumulative").print_stats(45)
