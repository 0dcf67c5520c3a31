#!/usr/bin/env python3
"""Writes tests/golden/g15_depth_pyramid_grad.npz: the reference's own autograd through rasterize_depth and through
softor(rasterize_depth), level by level of a three-level pyramid, in float64 AND float32 on the CPU.

TEST INFRASTRUCTURE ONLY.  It needs a checkout of the reference (the torch-only half imports with the empty stub modules of SURVEY.md
Appendix C) and never runs where the GPU tests run; no test reads the reference, only the file written here.  No reference source text
is stored: inputs, weights and the numbers the reference computed for them.

    python tools/gen_golden_depth.py --reference <checkout of the reference> [--out tests/golden/g15_depth_pyramid_grad.npz]

Cases: n = 5 (golden g5's points), 40, 64 points x sizes (24,20), (33,47), (64,48), sigma = 6, levels size // 2^i, i = 0, 1, 2 — but for
g5's points at (64,48), which the tie rule below excludes (they are given, not drawn); `cases` lists the eight that are stored.  The drawn
points are float32 values in [-0.05, 1.05]^2 (some lie outside the texture) with depths in [0, 1]; a draw is repeated with the next seed
until no scaled coordinate is within 2^-8 texel of a rint tie at any level (there the layer maximum changes texel and the function
is not differentiable).  The weights of the losses sum(w * output) are multiples of 1/8 in [-1, 1], stored as int8 (w = w8 / 8).

Per case `c` and level `l` (key prefix c<n>_<s0>x<s1>_l<l>_):
  w8_dense [n,l1,l0], w8_fused [l1,l0]       int8 weights
  fused   [l1,l0]                            float64 softor plane
  dense_loss                                 float64 sum(w * layers)
  {dense,fused}_{gpts,gz}_{f64,f32}          gradients with respect to the points [n,2] and the depths [n]
and per case pts [n,2], depth [n] (float32), seed."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_sparse_depth as ref  # noqa: E402

NS, SIZES, LEVELS, SIGMA, TIE = (5, 40, 64), ((24, 20), (33, 47), (64, 48)), 3, 6.0, 2.0**-8


def import_reference(path):
    sys.path.insert(0, path)
    for name in ["mitsuba", "drjit", "pywavefront", "geomdl", "cv2", "kornia"]:
        sys.modules[name] = types.ModuleType(name)
    sys.modules["geomdl"].NURBS = types.SimpleNamespace(Curve=object)
    import fireflies  # noqa: F401
    import fireflies.graphics.rasterization as R

    return R


def clear_of_ties(pts, s0, s1):
    return all(ref.tie_distance(pts, l0, l1) >= TIE for l0, l1 in ref.level_sizes(s0, s1, LEVELS))


def draw(n, s0, s1, seed0):
    seed = seed0
    while True:
        rng = np.random.default_rng(seed)
        pts = (rng.random((n, 2)) * 1.1 - 0.05).astype(np.float32)
        depth = rng.random(n).astype(np.float32)
        if clear_of_ties(pts, s0, s1):
            return pts, depth, seed
        seed += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g15_depth_pyramid_grad.npz"))
    a = ap.parse_args()
    import torch

    R = import_reference(a.reference)
    g5 = np.load(os.path.join(ROOT, "tests", "golden", "g5_depth_lines.npz"))["depth_pts"].astype(np.float32)
    out = {"sigma": np.float64(SIGMA), "levels": np.int64(LEVELS), "ns": np.asarray(NS), "sizes": np.asarray(SIZES)}
    skipped = []
    for n in NS:
        for ci, (s0, s1) in enumerate(SIZES):
            case = f"c{n}_{s0}x{s1}"
            if n == 5:
                pts, depth, seed = np.ascontiguousarray(g5[:, 0:2]), np.ascontiguousarray(g5[:, 2]), -1
                if not clear_of_ties(pts, s0, s1):  # fixed points cannot be drawn again: the case is left out and listed
                    skipped.append(case)
                    continue
            else:
                pts, depth, seed = draw(n, s0, s1, 1000 * n + 100 * ci)
            out[f"{case}_pts"], out[f"{case}_depth"], out[f"{case}_seed"] = pts, depth, np.int64(seed)
            wr = np.random.default_rng(7 * n + ci)
            for lv, (l0, l1) in enumerate(ref.level_sizes(s0, s1, LEVELS)):
                key = f"{case}_l{lv}_"
                w8d = wr.integers(-8, 9, size=(n, l1, l0)).astype(np.int8)
                w8f = wr.integers(-8, 9, size=(l1, l0)).astype(np.int8)
                out[key + "w8_dense"], out[key + "w8_fused"] = w8d, w8f
                size = torch.tensor([l0, l1])
                for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                    for path, w8 in (("dense", w8d), ("fused", w8f)):
                        p = torch.tensor(pts, dtype=dt, requires_grad=True)
                        z = torch.tensor(depth, dtype=dt, requires_grad=True)
                        o = R.rasterize_depth(p, z.unsqueeze(-1), SIGMA, size, device="cpu")
                        assert tuple(o.shape) == (n, l1, l0) and o.dtype == dt
                        if path == "fused":
                            o = R.softor(o)
                        loss = (o * torch.tensor(w8.astype(np.float64) / 8.0, dtype=dt)).sum()
                        loss.backward()
                        out[key + f"{path}_gpts_{tag}"] = p.grad.numpy().copy()
                        out[key + f"{path}_gz_{tag}"] = z.grad.numpy().copy()
                        if tag == "f64":
                            if path == "fused":
                                out[key + "fused"] = o.detach().numpy().copy()
                            else:
                                out[key + "dense_loss"] = np.float64(loss.item())
                                if n == 5 and ci == 0:
                                    out[key + "dense"] = o.detach().numpy().copy()
    assert skipped == ["c5_64x48"], skipped  # (g5's points at 64 x 48: one coordinate 0.0029 texel from a tie)
    out["cases"] = np.asarray(sorted(k[:-4] for k in out if k.endswith("_pts")))
    np.savez_compressed(a.out, **out)
    worst = max(
        float(np.abs(out[k].astype(np.float64) - out[k[:-3] + "f64"]).max() / np.abs(out[k[:-3] + "f64"]).max()) for k in out if k.endswith("_f32"))
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(out)} arrays; worst float32-autograd deviation of a block {worst:.2e} of its largest magnitude")


if __name__ == "__main__":
    main()
