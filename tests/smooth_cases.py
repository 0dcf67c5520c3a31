"""What tests/test_shading_walk_cpu.py and tests/test_shading_walk_gpu.py share: the films, sample counts and seed at which corner_scenes.smooth_corner
is rendered, the extra emitters, and the inputs of the float64 restatements.  The CPU file shows on exactly these cases that the scene does its job
and that every rule of the walk is visible at the GPU file's bounds.  numpy and fireflies_amd.scenes only."""
import numpy as np

from fireflies_amd import scenes
from tests import ambient_scenes as am
from tests import corner_scenes as cs
from tests import light_scenes as ls
from tests import sun_scenes as ss
from tests.support import world_arrays

FILMS = {"12x12": (12, 12), "13x11": (13, 11)}
SPP, SEED = 16, 7
# the tests whose reference is a difference of whole float64 renders; their seed is the one of 1 .. 15 whose 512 samples end most bounces below a facet
# and turn most shading normals away from their facet (tests/test_shading_walk_cpu.py holds it to that)
DIFF_FILM, DIFF_SPP, DIFF_SEED = (8, 8), 8, 8
DEPTHS = (2, 3, 4)
POINT, SPOT, SUN, RADIANCE = ls.POINT, ls.SPOT_B, ss.SUN_A, am.RADIANCE


def shading(sc, base_tex, uv):
    """ref_path.walk's keyword arguments for the scene of smooth_corner: one smooth flag per shape, the pool's uv (the floor is mesh 0), the textures"""
    n_verts = sum(m.frames.shape[0] * m.frames.shape[1] for m in sc.meshes)
    vuv = None
    if uv is not None:
        vuv = np.zeros((n_verts, 2))
        vuv[:len(uv)] = uv
    return dict(smooth=[bool(m.smooth) for m in sc.meshes], vert_uv=vuv, base_tex=None if base_tex is None else [np.asarray(base_tex, np.float64)])


def host_rows(sc):
    """the material table the loader builds, in float64: [S, 16] rows, or [S, 3] albedos where no mesh has a BSDF or a texture"""
    rows = scenes.material_rows(sc)
    return (world_arrays(sc)[3] if rows is None else rows).astype(np.float64)


def host_table(*lights):
    """the [n, 24] table of ops.pack_lights in float64, stated here so that a test without the package's device side can build it"""
    from fireflies_amd import ops

    return ops.pack_lights(list(lights)).numpy().astype(np.float64)


def scene(film, **kw):
    return cs.smooth_corner(*(FILMS[film] if isinstance(film, str) else film), **kw)
