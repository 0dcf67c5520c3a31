"""The scenes of the per-lane kernel tests (k_path_*, the appearance, material and prb adjoints, forward mode, the aov block), as tests/tie_scenes.py,
tests/seam_scenes.py and tests/stage_scenes.py are for the walks: the box corner — a floor and two walls with a cube on the floor, lit by a projector
and a spot — its smaller relatives, and the relay, whose camera sees a wall that only a bounce can light.  The geometry and the camera, projector and
spot numbers stand here once.  numpy and fireflies_amd.scenes only: a test without a GPU may import this."""
import numpy as np

from fireflies_amd import scenes

QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
R0 = scenes.MAT_COLUMN["roughness"]
NAMES = ["roughness", "anisotropic", "metallic", "spec_trans", "eta", "spec_tint", "sheen", "sheen_tint", "flatness", "clearcoat", "clearcoat_gloss"]
PRINCIPLED = {"roughness": 0.35, "metallic": 0.2, "specular": 0.6}
EVERY_LOBE = {"roughness": 0.4, "anisotropic": 0.5, "metallic": 0.3, "spec_trans": 0.2, "specular": 0.6, "spec_tint": 0.6, "sheen": 0.8, "sheen_tint": 0.7,
              "flatness": 0.4, "clearcoat": 0.7, "clearcoat_gloss": 0.3}
# (floor's BSDF, wall y = 0's BSDF, whether the floor's base colour is base_texture())
CASES = {
    "defaults": ({}, {}, None),
    "every_lobe": (EVERY_LOBE, {"roughness": 0.3, "metallic": 1.0, "clearcoat": 1.0, "clearcoat_gloss": 0.6, "spec_trans": 0.3, "sheen": 0.5}, None),
    "textured": ({"roughness": 0.35, "metallic": 0.2, "specular": 0.6, "spec_tint": 0.5, "sheen": 0.6, "sheen_tint": 0.5}, {"roughness": 0.6}, "tex"),
}
FLOOR_RGB, WALL_X_RGB, WALL_Y_RGB, CUBE_RGB = (0.6, 0.55, 0.5), (0.7, 0.7, 0.75), (0.5, 0.6, 0.7), (0.8, 0.4, 0.3)


def _quad(p):
    return np.asarray(p, np.float32)[None]


def _floor():
    return _quad([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]])


def _wall_x():
    return _quad([[0, 0, 0], [0, 2, 0], [0, 2, 2], [0, 0, 2]])


def _wall_y():
    return _quad([[0, 0, 0], [2, 0, 0], [2, 0, 2], [0, 0, 2]])


def _camera(W, H, eye=(3.2, 3.0, 2.4), target=(0.6, 0.6, 0.5)):
    return scenes.SensorData("PerspectiveCamera", scenes.look_at(eye, target, up=(0, 0, 1)), 50.0, 0.01, 100.0, W, H)


def _projector(tex):
    return scenes.SensorData("PerspectiveCamera_1", scenes.look_at((2.6, 1.2, 2.8), (0.7, 0.9, 0.2), up=(0, 0, 1)), 50.0, 0.01, 100.0, tex, tex)


def _spot():
    return scenes.SpotData("emit-Spot", scenes.look_at((1.8, 2.6, 2.5), (0.5, 0.5, 0.0), up=(0, 0, 1)), (8.0, 8.0, 8.0), 30.0, 20.0)


def base_texture():
    """the [8, 8, 3] base-colour texture of every textured floor"""
    return np.random.default_rng(5).uniform(0.2, 0.9, (8, 8, 3)).astype(np.float32)


def corner(floor_bsdf=None, wall_y_bsdf=None, *, shared=False, materials=True, W=24, H=24, tex=32, base_tex=None):
    """the box corner: floor, wall x = 0, wall y = 0 and a cube on the floor.  A BSDF of None is a Lambert row, a dict a principled one; wall x = 0 and
    the cube are Lambert.  shared: wall x = 0 shares the floor's material (colour and BSDF); base_tex: the floor's base colour is this [h, w, 3]
    texture; materials=False: no mesh names a material, so all four sit on mat-Default (mi.Scene builds its parameter map from the names)"""
    cv, ct = scenes.make_cube((1.2, 1.1, 0.3), 0.3)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32) if base_tex is not None else None

    def mat(name):
        return {"material": name} if materials else {}

    meshes = [scenes.MeshData("mesh-Floor", _floor(), QUAD, FLOOR_RGB, bsdf=floor_bsdf, uv=uv, base_tex=base_tex, **mat("mat-Floor")),
              scenes.MeshData("mesh-WallX", _wall_x(), QUAD, FLOOR_RGB if shared else WALL_X_RGB, bsdf=floor_bsdf if shared else None,
                              **mat("mat-Floor" if shared else "mat-WallX")),
              scenes.MeshData("mesh-WallY", _wall_y(), QUAD, WALL_Y_RGB, bsdf=wall_y_bsdf, **mat("mat-WallY")),
              scenes.MeshData("mesh-Cube", cv[None], ct, CUBE_RGB, **mat("mat-Cube"))]
    return scenes.SceneData(meshes, _camera(W, H), _projector(tex), _spot(), 1.0)


# the film (W, H), samples per pixel and projector texture size at which the GPU tests render mosaic: tests/test_leaf_arms_cpu.py shows that the rows of
# high index receive samples there (a film too small for that is grown here, for both)
MOSAIC_FILM, MOSAIC_SPP, MOSAIC_TEX = (32, 32), 16, 32
MOSAIC_TEX_SIZES = ([8, 8], [3, 5], [4, 4], [2, 7])  # [h, w] of mosaic's base-colour textures
# mosaic's camera is _camera from high above the floor: from corner()'s eye the cube hides a quarter of the floor's cells (its silhouette on z = 0 is
# the hull of its footprint and that footprint shifted by (-0.77, -0.73)), whatever the film's size, and those rows would never take a primary hit
MOSAIC_EYE, MOSAIC_TARGET = (2.0, 2.0, 5.5), (0.95, 0.95, 0.0)
# where mosaic's textured cells lie: floor points beside the cube that the camera and both emitters see
MOSAIC_TEX_POINTS = ((1.7, 0.45), (0.45, 1.7), (1.75, 1.15), (1.15, 1.75))


def mosaic_order(m):
    """the cell (iy * m + ix, x in 2 ix / m .. 2 (ix + 1) / m) of every floor mesh of mosaic: the cells of MOSAIC_TEX_POINTS first, the others in a
    stride over the grid (neighbouring indices lie far apart, so low and high rows both cover the whole floor), the cells whose centre lies under
    the cube last — no ray reaches them, and the last floor mesh takes what it can of them"""
    n = m * m
    first = []
    for x, y in MOSAIC_TEX_POINTS:
        c = int(y * m / 2) * m + int(x * m / 2)
        assert c not in first
        first.append(c)
    step = next(s for s in range(int(0.38 * n) | 1, n + 2) if np.gcd(s, n) == 1)
    rest = [c for c in (np.arange(n) * step) % n if c not in first]
    cx, cy = (np.array([c % m for c in rest]) + 0.5) * 2 / m, (np.array([c // m for c in rest]) + 0.5) * 2 / m
    under = (np.abs(cx - 1.2) < 0.3) & (np.abs(cy - 1.1) < 0.3)
    return first + [c for c, u in zip(rest, under) if not u] + [c for c, u in zip(rest, under) if u]


def mosaic(S, *, base_tex=0, lambert=False, hidden=False, W=None, H=None, tex=None, seed=17):
    """the box corner with its floor cut into an m x m grid of quads, m = ceil(sqrt(S - 3)): S shapes — S - 3 floor meshes (mosaic_order names their
    cells; the first S - 4 hold one cell, the last every remaining one), then wall x = 0, wall y = 0 and the cube.  Every floor mesh and wall y = 0
    has its own material, colour and principled BSDF (roughness 0.2 .. 0.8, metallic 0 .. 0.5, specular 0.2 .. 0.8, on every third row sheen,
    clearcoat and spec_tint in 0.1 .. 0.9) from a seeded generator whose draws depend on S and seed alone; wall x = 0 and the cube are Lambert rows
    of a stride-16 table.  base_tex = k (0 .. 4): the first k floor meshes take a base-colour texture of MOSAIC_TEX_SIZES each, uv over the cell.
    lambert: no mesh has a BSDF (without base_tex: a stride-3 table).  hidden: one more mesh behind every other index — a quad of side 0.02 under
    the middle of the floor at z = -0.05 with a principled row; a segment from any point of the corner's surfaces to it crosses the floor, so no
    camera, shadow or bounce ray reaches it"""
    assert S >= 8 and 0 <= base_tex <= len(MOSAIC_TEX_SIZES)
    W, H, tex = W or MOSAIC_FILM[0], H or MOSAIC_FILM[1], tex or MOSAIC_TEX
    n_floor = S - 3
    m = int(np.ceil(np.sqrt(n_floor)))
    order = mosaic_order(m)
    rng = np.random.default_rng(seed)
    n_rows = n_floor + 2  # (the floor meshes, wall y = 0, the hidden quad)
    rgb = rng.uniform(0.3, 0.8, (n_rows, 3))
    par = {"roughness": rng.uniform(0.2, 0.8, n_rows), "metallic": rng.uniform(0.0, 0.5, n_rows), "specular": rng.uniform(0.2, 0.8, n_rows)}
    extra = {k: rng.uniform(0.1, 0.9, n_rows) for k in ("sheen", "clearcoat", "spec_tint")}
    trng = np.random.default_rng(seed + 1)
    texs = [trng.uniform(0.2, 0.9, (h, w, 3)).astype(np.float32) for h, w in MOSAIC_TEX_SIZES]

    def bsdf(i):
        if lambert:
            return None
        b = {k: float(v[i]) for k, v in par.items()}
        if i % 3 == 0:
            b.update({k: float(v[i]) for k, v in extra.items()})
        return b

    def cells(cs_):
        v = []
        for c in cs_:
            x0, y0, d = 2.0 * (c % m) / m, 2.0 * (c // m) / m, 2.0 / m
            v += [[x0, y0, 0], [x0 + d, y0, 0], [x0 + d, y0 + d, 0], [x0, y0 + d, 0]]
        t = np.concatenate([QUAD + 4 * j for j in range(len(cs_))]).astype(np.int32)
        return np.asarray(v, np.float32)[None], t

    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    meshes = []
    for i in range(n_floor):
        v, t = cells(order[i:i + 1] if i < n_floor - 1 else order[i:])
        tx = texs[i] if i < base_tex else None
        meshes.append(scenes.MeshData(f"mesh-Cell{i}", v, t, tuple(rgb[i]), material=f"mat-Cell{i}", bsdf=bsdf(i), uv=uv if tx is not None else None, base_tex=tx))
    cv, ct = scenes.make_cube((1.2, 1.1, 0.3), 0.3)
    meshes += [scenes.MeshData("mesh-WallX", _wall_x(), QUAD, WALL_X_RGB, material="mat-WallX"),
               scenes.MeshData("mesh-WallY", _wall_y(), QUAD, tuple(rgb[n_floor]), material="mat-WallY", bsdf=bsdf(n_floor)),
               scenes.MeshData("mesh-Cube", cv[None], ct, CUBE_RGB, material="mat-Cube")]
    if hidden:
        q = _quad([[0.99, 0.99, -0.05], [1.01, 0.99, -0.05], [1.01, 1.01, -0.05], [0.99, 1.01, -0.05]])
        meshes.append(scenes.MeshData("mesh-Hidden", q, QUAD, tuple(rgb[n_floor + 1]), material="mat-Hidden",
                                      bsdf=None if lambert else dict(bsdf(n_floor + 1), sheen=0.5, clearcoat=0.5)))
    return scenes.SceneData(meshes, _camera(W, H, MOSAIC_EYE, MOSAIC_TARGET), _projector(tex), _spot(), 1.0)


def path_corner(principled, **kw):
    """tests/test_path_gpu.py's corner: Lambert rows or a principled floor and wall y = 0, no material names"""
    return corner(PRINCIPLED if principled else None, {"roughness": 0.6} if principled else None, materials=False, **kw)


def appearance_corner(principled, tint=False, shared=False, base_tex=None, **kw):
    """tests/test_appearance_gpu.py's corner.  tint: the floor's principled row carries spec_tint and sheen_tint"""
    bs = dict(PRINCIPLED) if principled or base_tex is not None else None
    if tint:
        bs = dict(bs, spec_tint=0.6, sheen=0.8, sheen_tint=0.7)
    return corner(bs, {"roughness": 0.6} if principled else None, shared=shared, base_tex=base_tex, **kw)


def case(name, **kw):
    """-> (the corner of CASES[name], its base texture or None)"""
    fb, wb, textured = CASES[name]
    bt = base_texture() if textured else None
    return corner(fb, wb, base_tex=bt, **kw), bt


def scene(name, **kw):
    """"lambert": the corner with Lambert rows only (a table of stride 3); "bounce": the relay under both emitters; a key of CASES; or a (floor, wall)
    pair of BSDF dictionaries"""
    if name == "lambert":
        return appearance_corner(False, **kw)
    if name == "bounce":
        return relay(True, True)
    return case(name, **kw)[0] if isinstance(name, str) else corner(*name, **kw)


def small_corner(W=6, H=6, tex=8):
    """the corner with every lobe of the floor active, small enough for the float64 restatement on the host"""
    return case("every_lobe", W=W, H=H, tex=tex)[0]


def spot_corner():
    """the principled floor and wall x = 0 under the spot alone, 6 x 6, no material names (tests/test_prb_cpu.py)"""
    meshes = [scenes.MeshData("mesh-Floor", _floor(), QUAD, FLOOR_RGB, bsdf=dict(PRINCIPLED)), scenes.MeshData("mesh-Wall", _wall_x(), QUAD, WALL_X_RGB)]
    return scenes.SceneData(meshes, _camera(6, 6), None, _spot())


def relay(proj_on=True, spot_on=False, W=16, H=16, tex=32, projector_scale=2.0):
    """the camera sees a Lambert wall (x = -1) only; the projector and the spot, straight above the floor (z = 0), light only the floor, which the
    camera cannot see: nothing arrives without a bounce"""
    wall = _quad([[-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2]])
    floor = _quad([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]])
    above = scenes.look_at((0.0, 0.0, 1.5), (0.0, 0.0, 0.0), up=(0, 1, 0))
    cam = scenes.SensorData("PerspectiveCamera", scenes.look_at((0.6, 0.0, 0.9), (-1.0, 0.0, 1.0), up=(0, 0, 1)), 20.0, 0.01, 100.0, W, H)
    proj = scenes.SensorData("PerspectiveCamera_1", above, 40.0, 0.01, 100.0, tex, tex) if proj_on else None
    spot = scenes.SpotData("emit-Spot", above, (10.0, 10.0, 10.0), 20.0, 15.0) if spot_on else None
    return scenes.SceneData([scenes.MeshData("mesh-Wall", wall, QUAD, (0.8, 0.7, 0.6)), scenes.MeshData("mesh-Floor", floor, QUAD, (0.5, 0.5, 0.5))],
                            cam, proj, spot, projector_scale)


SMOOTH_BALL = ((0.9, 0.9, 0.65), 0.6)  # (centre, radius) of smooth_corner's ball
SMOOTH_UV = np.array([[-0.5, 0.25], [2.5, 0.25], [2.5, 2.25], [-0.5, 2.25]], np.float32)  # (aov_corner's: beyond [0, 1], the lookup wraps)


def smooth_corner(W, H, lambert_only=False, every_lobe=False, smooth=True, tex=32):
    """the scene of tests/test_shading_walk_*.py, where the shading normal differs from the geometric one at every vertex of a walk: the floor
    z = 0 (a base-colour texture as aov_corner's, uv beyond [0, 1], a principled row), wall x = 0 (a Lambert row), wall y = 0 (a principled row) and,
    above the floor between them, a smooth ball of 8 x 4 facets — coarse on purpose: its interpolated normals stand tens of degrees off its
    facets', so that bounces drawn about n_s leave below a facet and shading normals face the other way than their facet.  lambert_only: no BSDF and
    no texture (a stride-3 table); every_lobe: EVERY_LOBE on the ball; smooth=False: the same geometry flat.
    -> (scene, base texture or None, the floor's uv or None)"""
    sv, st = scenes.make_uv_sphere(*SMOOTH_BALL, nu=8, nv=4)
    base_tex = None if lambert_only else base_texture()
    uv = None if lambert_only else SMOOTH_UV

    def bsdf(b):
        return None if lambert_only else b

    meshes = [scenes.MeshData("mesh-Floor", _floor(), QUAD, FLOOR_RGB, material="mat-Floor", bsdf=bsdf({"roughness": 0.4}), uv=uv, base_tex=base_tex),
              scenes.MeshData("mesh-WallX", _wall_x(), QUAD, WALL_X_RGB, material="mat-WallX"),
              scenes.MeshData("mesh-WallY", _wall_y(), QUAD, WALL_Y_RGB, material="mat-WallY", bsdf=bsdf({"roughness": 0.6})),
              scenes.MeshData("mesh-Ball", np.asarray(sv, np.float32)[None], np.asarray(st, np.int32), CUBE_RGB, material="mat-Ball",
                              bsdf=bsdf(dict(EVERY_LOBE)) if every_lobe else None, smooth=smooth)]
    return scenes.SceneData(meshes, _camera(W, H, (3.1, 2.7, 2.6), SMOOTH_BALL[0]), _projector(tex), _spot(), 1.0), base_tex, uv


def aov_corner(W, H, lambert_only=False):
    """a floor (textured base colour, flat) and a wall (Lambert row; smooth: its vertex normals are the plane's, bent at the shared seam by nothing — the
    wall is its own mesh) with a smooth sphere above the floor so that the interpolated normal differs from the geometric one.  lambert_only: no BSDF,
    no texture — mi.Scene then builds the stride-3 table.  The camera looks into the corner from above: no ray grazes the floor / wall seam.
    -> (scene, base texture, uv)"""
    sv, st = scenes.make_uv_sphere((1.1, 1.0, 0.45), 0.35, nu=8, nv=4)
    base_tex = None if lambert_only else base_texture()
    uv = None if lambert_only else np.array([[-0.5, 0.25], [2.5, 0.25], [2.5, 2.25], [-0.5, 2.25]], np.float32)  # (beyond [0, 1]: the lookup wraps, the channel not)
    meshes = [scenes.MeshData("mesh-Floor", _floor(), QUAD, FLOOR_RGB, material="mat-Floor", bsdf=None if lambert_only else {"roughness": 0.4}, uv=uv,
                              base_tex=base_tex),
              scenes.MeshData("mesh-Wall", _wall_x(), QUAD, WALL_X_RGB, material="mat-Wall"),
              scenes.MeshData("mesh-Ball", np.asarray(sv, np.float32)[None], np.asarray(st, np.int32), CUBE_RGB, material="mat-Ball", smooth=True)]
    return scenes.SceneData(meshes, _camera(W, H, (3.1, 2.7, 2.6), (0.6, 0.8, 0.4)), _projector(32), _spot(), 1.0), base_tex, uv
