"""The scenes of the constant-emitter tests (tests/test_ambient_cpu.py, tests/test_ambient_gpu.py): one Lambert quad that fills the film
under a camera that can be turned away from it (the closed forms), tests/light_scenes.py's box corner at 24 x 24 and the ragged 21 x 19, and the scene
file of the loader and mi tests.  numpy and fireflies_amd.scenes only: a test without a GPU may import this."""
import numpy as np

from fireflies_amd import loaders, scenes
from tests import corner_scenes as cs
from tests import light_scenes as ls

FILMS = ls.FILMS
# the world of the corner tests: bluish, of the order of the main emitters' image (the spot's intensity is 8 at a distance of ~3: ~0.5 on the floor)
RADIANCE = (0.8, 1.0, 1.3)
QUAD_RGB = (0.6, 0.45, 0.3)


def quad(W=24, H=24, away=False):
    """one Lambert quad in z = 0, 200 units wide, no projector and no spot; the camera 3 units above it looks straight down — the quad fills the film
    and no ray that leaves it upwards can meet it again — or (away) straight up, where there is nothing"""
    q = np.asarray([[-100, -100, 0], [100, -100, 0], [100, 100, 0], [-100, 100, 0]], np.float32)[None]
    cam = scenes.SensorData("PerspectiveCamera", scenes.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 6.0 if away else 0.0), up=(0, 1, 0)), 50.0, 0.01, 100.0, W, H)
    return scenes.SceneData([scenes.MeshData("mesh-Quad", q, cs.QUAD, QUAD_RGB, material="mat-Quad")], cam, None, None, 1.0)


def corner(film="24x24", principled=False, **kw):
    """light_scenes' box corner with projector and main spot: Lambert rows, or the floor with every lobe active"""
    return ls.corner(film, principled, **kw)


def dark_corner(film="24x24", principled=False):
    """the corner without projector and spot: the image of a call without extra emitters is zero, so that the ambient part is an image itself and not a
    difference of two float32 images"""
    sc = ls.corner(film, principled)
    sc.projector, sc.spot = None, None
    return sc


# a point light weak enough (image values below 0.1: half an ulp is 4e-9) that adding its image rounds the ambient part by far less than the
# tolerance of an identity
WEAK_POINT = scenes.LightData("emit-Weak", "point", ls.POINT.to_world, (1.0, 0.9, 0.75))


# ------------------------------------------------------------------ the scene file: the corner's three quads, projector, spot and a constant emitter
# whose id says neither "light" nor "spot"
def _lookat(eye, target):
    return f'<transform name="to_world"><lookat origin="{eye[0]},{eye[1]},{eye[2]}" target="{target[0]},{target[1]},{target[2]}" up="0,0,1"/></transform>'


WORLD = '<emitter type="constant" id="emit-World"><rgb name="radiance" value="0.8, 1.0, 1.3"/></emitter>'
XML = f"""<scene version="3.0.0">
  <integrator type="path"><integer name="max_depth" value="2"/></integrator>
  <sensor type="perspective" id="PerspectiveCamera">
    <float name="fov" value="50"/><float name="near_clip" value="0.01"/><float name="far_clip" value="100"/>
    {_lookat((3.2, 3.0, 2.4), (0.6, 0.6, 0.5))}
    <film type="hdrfilm"><integer name="width" value="24"/><integer name="height" value="24"/><rfilter type="box"/></film>
  </sensor>
  <sensor type="perspective" id="PerspectiveCamera_1">
    <float name="fov" value="50"/>
    {_lookat((2.6, 1.2, 2.8), (0.7, 0.9, 0.2))}
    <film type="hdrfilm"><integer name="width" value="32"/><integer name="height" value="32"/></film>
  </sensor>
  <shape type="obj" id="mesh-Floor"><string name="filename" value="floor.obj"/><bsdf type="diffuse" id="mat-Floor"><rgb name="reflectance" value="0.6, 0.55, 0.5"/></bsdf></shape>
  <shape type="obj" id="mesh-WallX"><string name="filename" value="wallx.obj"/><bsdf type="diffuse" id="mat-WallX"><rgb name="reflectance" value="0.7, 0.7, 0.75"/></bsdf></shape>
  <shape type="obj" id="mesh-WallY"><string name="filename" value="wally.obj"/><bsdf type="diffuse" id="mat-WallY"><rgb name="reflectance" value="0.5, 0.6, 0.7"/></bsdf></shape>
  <emitter type="projector" id="Projector"><float name="scale" value="1"/>{_lookat((2.6, 1.2, 2.8), (0.7, 0.9, 0.2))}</emitter>
  <emitter type="spot" id="emit-Spot"><rgb name="intensity" value="8"/><float name="cutoff_angle" value="30"/><float name="beam_width" value="20"/>
    {_lookat((1.8, 2.6, 2.5), (0.5, 0.5, 0.0))}</emitter>
  {WORLD}
</scene>"""


def write_scene(tmp_path, xml=XML, name="ambient.xml"):
    """the scene file and its three meshes under tmp_path -> the file's path"""
    for fn, v in (("floor.obj", cs._floor()), ("wallx.obj", cs._wall_x()), ("wally.obj", cs._wall_y())):
        loaders.save_obj(tmp_path / fn, v[0], cs.QUAD)
    (tmp_path / name).write_text(xml)
    return str(tmp_path / name)
