"""The refusals that a render entry point makes before its first launch, as every CPU suite provokes them: host dummy pointers that the library never
dereferences and a one-triangle bvh info without normals, apex areas or a wide tree, so that nothing can launch.  The suites hold the case tables;
here are the one statement of the entry points' parameter orders and the one call.  numpy, ctypes, _abi and _lib only."""
import ctypes as C

import numpy as np

from fireflies_amd import _abi, _lib

# the parameters of every render entry point, in order and under the names of include/ffx.h (`mats` is shape_albedo, `flags` also img_fp16, `dot` dot_out /
# loss_slots, `s` the stream)
RENDER_PARAMS = {
    "ffx_render_fwd": "bvh info sd mats tex spp seed flags img s",
    "ffx_render_fwd_cache": "bvh info sd mats tex spp seed flags img cache s",
    "ffx_render_fwd_adjoint": "bvh info sd mats tex spp seed flags img gimg gtex dot s",
    "ffx_render_fwd_filtered": "bvh info sd mats tex spp seed flags img scratch s",
    "ffx_render_fwd_adjoint_filtered": "bvh info sd mats tex spp seed flags img gimg gtex scratch s",
    "ffx_render_fwd_cache_filtered": "bvh info sd mats tex spp seed flags img cache scratch s",
    "ffx_render_bwd": "bvh info sd mats spp seed flags gimg gtex s",
    "ffx_render_bwd_filtered": "bvh info sd mats spp seed flags gimg gtex scratch s",
    "ffx_render_bwd_det": "bvh info sd mats spp seed flags gimg gtex workspace s",
    "ffx_render_bwd_det_part": "bvh info sd mats spp seed flags gimg part scale_log2 acc workspace s",
    "ffx_render_bwd_cached": "sd mats cache spp gimg gtex img flags dot s",
    "ffx_render_bwd_cached_l1": "sd mats cache spp img target weight gtex dot s",
    "ffx_render_bwd_cached_filtered": "sd mats cache spp seed gimg gtex s",
    "ffx_trace_primary": "bvh info cam spp flags seed t_out shape_out prim_out s",
}
GAUSS = {"rfilter": _abi.RFILTER_GAUSSIAN}
BUF, MISALIGNED = "buf", "misaligned"  # stand for a 16-byte aligned host address and for one 4 bytes off


def call(name, changes=None, arg_changes=None, *, monkeypatch):
    """`name` on a 4 x 4 film with a 4 x 4 one-channel projector, one shape and every pointer at a dummy host buffer -> (return code, ffx_last_error()).
    `changes` sets members of the scene description, or of the bvh info under "info." (dotted keys reach into members, a tuple fills the head of an
    array); `arg_changes` replaces arguments by the names of RENDER_PARAMS.  The walk's knobs are cleared: they choose what is refused"""
    for knob in ("FFX_TRAVERSAL", "FFX_WIDE"):
        monkeypatch.delenv(knob, raising=False)
    lib = _lib.api().lib
    buf = np.zeros(64, np.float32)
    addr = (buf.ctypes.data + 15) & ~15
    val = lambda v: addr if v == BUF else (addr + 4 if v == MISALIGNED else v)  # noqa: E731
    eye = _abi.mat16(np.eye(4))
    sd = _abi.SceneDesc()
    sd.cam.to_world, sd.cam.camera_to_sample, sd.cam.width, sd.cam.height = eye, eye, 4, 4
    sd.proj.to_world, sd.proj.camera_to_sample, sd.proj.tex_w, sd.proj.tex_h, sd.proj.tex_channels, sd.proj.enabled = eye, eye, 4, 4, 1, 1
    sd.n_shapes = 1
    info = _abi.BvhInfo(n_tris=1, n_nodes=1, max_depth=1, off_tq=64)
    for key, v in (changes or {}).items():
        obj, attr = (info, key[5:]) if key.startswith("info.") else (sd, key)
        while "." in attr:
            head, attr = attr.split(".", 1)
            obj = getattr(obj, head)
        if isinstance(v, tuple):
            getattr(obj, attr)[: len(v)] = [val(x) for x in v]
        else:
            setattr(obj, attr, val(v))
    args = dict(bvh=addr, info=C.byref(info), sd=C.byref(sd), cam=C.byref(sd.cam), mats=addr, tex=addr, spp=4, seed=1, flags=0, img=addr, cache=addr,
                scratch=addr, gimg=addr, gtex=addr, dot=addr, target=addr, weight=1.0, workspace=addr, part=1, scale_log2=0, acc=addr, t_out=addr,
                shape_out=addr, prim_out=addr, s=None)
    assert not set(arg_changes or {}) - set(args), (name, arg_changes)  # (a name the header does not use would change nothing)
    args.update({k: val(v) for k, v in (arg_changes or {}).items()})
    rc = getattr(lib, name)(*[args[p] for p in RENDER_PARAMS[name].split()])
    return rc, (lib.ffx_last_error() or b"").decode()
