"""The poses whose tile bins tests/test_bins_gpu.py reads back — TEST INFRASTRUCTURE (numpy only).  tests/test_bins_cpu.py proves on the float64
reference that between them they populate every class of the pre-pass, both orientations and every kind of entry.

CASES: name -> (builder() -> SceneData, pre-pass knobs, samples per pixel, the description's `shadows`, (seed of the shapes' transforms or None, frame)).
The smallest shapes at which each path of the pre-pass exists:
  side_lit            96 x 80: cast shadows under both emitters, a part-filled projector grid of 3 x 2 tiles, the floor across more than sixteen tiles
  facing_20           64 x 48, a 20-degree cone: geometry behind and beside the projector's apex, a spot grid most of the tube lies outside of
  facing_74_n32       the 74-degree cone on 32 x 32 tiles (the default 128 x 128 do not fit the capacity): all four classes in one grid
  away                facing with both emitters re-aimed at nothing: empty lists, empty envelopes
  vocalfold_a / _b    the vocal fold at 64 x 64 under two random poses, the second on the next animation frame: 3 840 triangles, 80 x 80 spot tiles
  hello_world         32 x 32, no projector: a grid that is off
  tile_4 / proj_tile_4    side_lit with 4-pixel camera tiles (24 x 20) / 4-texel projector tiles (10 x 6)
  plain_16spp         side_lit under the short-render hint: the spot's coarser grid (42 x 42), no envelope
"""
import numpy as np

from fireflies_amd import scenes
from tests import stage_scenes as ss


def rand_xforms(S, seed):
    """a small rotation about y, a stretch along x and a shift per shape (the poses tests/test_hip_parity.py renders)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(S):
        a = rng.uniform(-0.15, 0.15)
        R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
        Sx = np.diag([rng.uniform(0.8, 1.2), 1.0, 1.0, 1.0])
        T = np.eye(4)
        T[:3, 3] = rng.uniform(-0.05, 0.05, 3)
        out.append(T @ R @ Sx)
    return np.asarray(out, np.float32)


def _vocalfold():
    return scenes.vocalfold(width=64, height=64, tex=32, frames=3, n_fold=24, tube=(24, 32))


SHADOWS_PLAIN = 3  # include/ffx.h FFX_SHADOWS_ON | FFX_SHADOWS_PLAIN: what a render below 33 samples per pixel passes
CASES = {
    "side_lit": (lambda: ss.side_lit(96, 80), {}, 64, True, (None, 0)),
    "facing_20": (lambda: ss.facing(64, 48, cutoff=20.0), {}, 64, True, (None, 0)),
    "facing_74_n32": (lambda: ss.facing(64, 48, cutoff=74.0), {"FFX_BIN_SPOT_N": "32"}, 64, True, (None, 0)),
    "away": (lambda: ss.away(ss.facing(64, 48)), {}, 64, True, (None, 0)),
    "vocalfold_a": (_vocalfold, {}, 64, True, (7, 0)),
    "vocalfold_b": (_vocalfold, {}, 64, True, (8, 1)),
    "hello_world": (lambda: scenes.hello_world(32, 32), {}, 64, True, (None, 0)),
    "tile_4": (lambda: ss.side_lit(96, 80), {"FFX_BIN_TILE": "4"}, 64, True, (None, 0)),
    "proj_tile_4": (lambda: ss.side_lit(96, 80), {"FFX_BIN_TILE_PROJ": "4"}, 64, True, (None, 0)),
    "plain_16spp": (lambda: ss.side_lit(96, 80), {}, 16, SHADOWS_PLAIN, (None, 0)),
}


def knobs(env):
    """the pre-pass knobs of a case as tests/ref_bins.grids_of takes them"""
    return {"tile": int(env.get("FFX_BIN_TILE", 8)), "tile_proj": int(env["FFX_BIN_TILE_PROJ"]) if "FFX_BIN_TILE_PROJ" in env else None,
            "spot_n": int(env["FFX_BIN_SPOT_N"]) if "FFX_BIN_SPOT_N" in env else None}


def pose(sc, seed, frame):
    """-> (xforms [S,4,4] float32, frame offsets [S] int32) of a case's pose"""
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    S = len(sc.meshes)
    xf = np.tile(np.eye(4, dtype=np.float32), (S, 1, 1)) if seed is None else rand_xforms(S, seed)
    return xf, (off + np.minimum(frame, nfr - 1) * stride).astype(np.int32)


def posed_tris(sc, seed, frame):
    """[F,3,3] float64: the case's triangles as float32 arithmetic poses them (scene order; the device holds them in leaf-slot order)"""
    pool, tris, shape, off, stride, nfr, alb = scenes.flatten(sc)
    xf, offs = pose(sc, seed, frame)
    v = pool[(tris + offs[shape][:, None])].astype(np.float32)  # [F,3,3]
    m = xf[shape]
    return (np.einsum("fij,fkj->fki", m[:, :3, :3], v) + m[:, None, :3, 3]).astype(np.float32).astype(np.float64)
