"""The appearance adjoint's cost: ms per 512^2 x 64-spp vocal-fold adjoint with FFX_RENDER_GRAD_APPEARANCE (the texture gradient's
launches + k_render_bwd_appearance), next to the same render_bwd without it, and with FFX_RENDER_GRAD_MATERIAL as well (k_render_bwd_material: the
BSDF parameters' adjoint), box and gaussian film; beside them forward mode (render_jvp, DESIGN.md 4.5.3: primal + tangent image) and the render
alone.  HIP events around repeated calls of one pose on
one stream, after a warm-up.  Prints one JSON line.

    python tools/appearancebench.py [reps]
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
        gimg = torch.full((sd.cam.height, sd.cam.width, 3), -1.0 / (sd.cam.height * sd.cam.width), device="cuda")
        out[f"render_bwd_ms_{film}"] = round(_ms(lambda: geom.render_bwd(sd, mats, 64, 1, gimg), reps), 3)
        out[f"appearance_bwd_ms_{film}"] = round(_ms(lambda: geom.render_bwd(sd, mats, 64, 1, gimg, appearance=True, tex=tex), reps), 3)
        out[f"material_bwd_ms_{film}"] = round(_ms(lambda: geom.render_bwd(sd, mats, 64, 1, gimg, appearance=True, tex=tex, material=True), reps), 3)
        # forward mode: the whole call — the primal render and the tangent image — and the render alone, in the same run
        S = sd.n_shapes
        tan = ops.AppearanceGrad(torch.rand((S, 3), device="cuda"), torch.rand(3, device="cuda"), [torch.rand_like(t) for _, t in wl.mi_scene._base_tex],
                                 torch.rand((S, 11), device="cuda") if sd.mat_stride == 16 else None)
        dtex = torch.rand_like(tex)
        out[f"render_fwd_ms_{film}"] = round(_ms(lambda: geom.render_fwd(sd, mats, tex, 64, 1), reps), 3)
        out[f"jvp_ms_{film}"] = round(_ms(lambda: geom.render_jvp(sd, wl.mi_scene.albedo, tex, 64, 1, dtex=dtex, tangent=tan), reps), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
