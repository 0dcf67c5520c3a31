"""The scenes of the directional-emitter tests (tests/test_sun_cpu.py, tests/test_sun_gpu.py): tests/light_scenes.py's box corner at
24 x 24 and the ragged 21 x 19 with two suns, one Lambert quad that fills the film with and without a roof the camera does not see (the closed forms),
the point light that stands in for a sun from far away, and the scene file of the loader and mi tests.  numpy and fireflies_amd.scenes only: a test
without a GPU may import this."""
import numpy as np

from fireflies_amd import loaders, scenes
from tests import corner_scenes as cs
from tests import light_scenes as ls

FILMS = ls.FILMS
QUAD_RGB = (0.6, 0.45, 0.3)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def frame(direction, origin=(0.0, 0.0, 0.0)):
    """a to_world whose +Z is the normalised direction; the translation (`origin`) is there to be ignored"""
    z = unit(direction)
    x = unit(np.cross((0.0, 0.0, 1.0) if abs(z[2]) < 0.9 else (1.0, 0.0, 0.0), z))
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, origin
    return m.astype(np.float32)


# the corner: floor z = 0, walls x = 0 and y = 0 of height 2, the cube on the floor.
# SUN_A travels towards the corner from the camera's side: it lights the floor and both walls; the cube's shadow (0.3 by 0.21 towards the corner) lies
# behind the cube as the camera sees it, so only bounce vertices meet it
DIR_A = unit((-0.5, -0.35, -1.0))
SUN_A = scenes.LightData("emit-SunA", "directional", frame(DIR_A, (7.0, -3.0, 9.0)), (2.0, 1.8, 1.5))
# SUN_B comes over the top edge of wall y = 0 (the edge y = 0, z = 2 shadows the floor up to y = 2 * 0.75 = 1.5) and faces neither wall: wall x = 0's
# normal is +x and the light travels along +x, wall y = 0's is +y and the light travels along +y
DIR_B = unit((0.2, 0.75, -1.0))
SUN_B = scenes.LightData("emit-SunB", "directional", frame(DIR_B), (1.2, 1.6, 2.2))
# the ball that holds the corner: every point of its surfaces lies within RADIUS of CENTRE
CENTRE, RADIUS = np.array([1.0, 1.0, 1.0]), float(np.sqrt(3.0))


def corner(film="24x24", principled=False, **kw):
    """light_scenes' box corner with projector and main spot: Lambert rows, or the floor with every lobe active"""
    return ls.corner(film, principled, **kw)


def far_point(sun, D, centre=CENTRE):
    """the point light that a sun is the limit of: at centre - D dir with intensity E D^2"""
    d = unit(np.asarray(sun.to_world, np.float64)[:3, 2])
    tw = np.eye(4)
    tw[:3, 3] = np.asarray(centre, np.float64) - D * d
    return scenes.LightData(sun.name + "-far", "point", tw.astype(np.float32), tuple(float(v) * D * D for v in sun.intensity))


# ------------------------------------------------------------------ the closed forms: a Lambert quad that fills the film
DIR_Q = unit((0.3, -0.2, -1.0))
SUN_Q = scenes.LightData("emit-SunQ", "directional", frame(DIR_Q), (3.0, 2.0, 1.0))
COS_Q = float(-DIR_Q[2])  # (the quad's normal is +z)


def quad(W=24, H=24, roof=False):
    """one Lambert quad in z = 0, 200 units wide, no projector and no spot, under a camera 3 units above it that looks straight down; roof: a quad
    2000 units wide in z = 5, above the camera — no camera ray meets it, every ray that leaves the floor upwards does"""
    q = np.asarray([[-100, -100, 0], [100, -100, 0], [100, 100, 0], [-100, 100, 0]], np.float32)[None]
    meshes = [scenes.MeshData("mesh-Quad", q, cs.QUAD, QUAD_RGB, material="mat-Quad")]
    if roof:
        r = np.asarray([[-1000, -1000, 5], [1000, -1000, 5], [1000, 1000, 5], [-1000, 1000, 5]], np.float32)[None]
        meshes.append(scenes.MeshData("mesh-Roof", r, cs.QUAD, (0.5, 0.5, 0.5), material="mat-Roof"))
    cam = scenes.SensorData("PerspectiveCamera", scenes.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), up=(0, 1, 0)), 50.0, 0.01, 100.0, W, H)
    return scenes.SceneData(meshes, cam, None, None, 1.0)


def quad_closed_form():
    """base * E cos(theta) / pi per channel"""
    return np.asarray(QUAD_RGB, np.float64) * np.asarray(SUN_Q.intensity, np.float64) * COS_Q / np.pi


def eight():
    """eight records about the corner of which three are suns: light_scenes' points and spots with a sun in slots 1, 4 and 6"""
    out = ls.eight()
    out[1] = SUN_A
    out[4] = SUN_B
    out[6] = scenes.LightData("emit-SunC", "directional", frame((-0.3, -0.6, -0.5)), (0.7, 0.9, 0.6))
    return out


# ------------------------------------------------------------------ the scene file: the corner's three quads, projector, spot, a point light, a sun
# given by `direction` whose id says neither "light" nor "spot", and a constant emitter
def _lookat(eye, target):
    return f'<transform name="to_world"><lookat origin="{eye[0]},{eye[1]},{eye[2]}" target="{target[0]},{target[1]},{target[2]}" up="0,0,1"/></transform>'


SUN_XML = '<emitter type="directional" id="emit-Sun"><rgb name="irradiance" value="2.0, 1.8, 1.5"/><vector name="direction" value="-0.5, -0.35, -1"/></emitter>'
WORLD_RADIANCE = (0.2, 0.25, 0.3)
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
  <emitter type="point" id="emit-Light"><rgb name="intensity" value="20, 18, 15"/><point name="position" x="1.0" y="-0.5" z="3.5"/></emitter>
  {SUN_XML}
  <emitter type="constant" id="emit-World"><rgb name="radiance" value="0.2, 0.25, 0.3"/></emitter>
</scene>"""
# the file's sun as the loader reads it (irradiance and direction; the frame about the direction is the loader's to choose)
FILE_SUN_DIR, FILE_SUN_IRRADIANCE = unit((-0.5, -0.35, -1.0)), (2.0, 1.8, 1.5)


def write_scene(tmp_path, xml=XML, name="sun.xml"):
    """the scene file and its three meshes under tmp_path -> the file's path"""
    for fn, v in (("floor.obj", cs._floor()), ("wallx.obj", cs._wall_x()), ("wally.obj", cs._wall_y())):
        loaders.save_obj(tmp_path / fn, v[0], cs.QUAD)
    (tmp_path / name).write_text(xml)
    return str(tmp_path / name)


def with_sun(sun_xml, xml=XML):
    """XML with its sun replaced by another emitter element (or by nothing)"""
    assert SUN_XML in xml
    return xml.replace(SUN_XML, sun_xml)


def with_extra_suns(n):
    """XML with n more suns behind the last emitter (the loader keeps scenes.MAX_EXTRA_LIGHTS extra emitters in all)"""
    more = "".join(f'<emitter type="directional" id="emit-More{k}"><vector name="direction" x="{0.1 * k}" y="0.2" z="-1"/></emitter>' for k in range(n))
    return XML.replace("</scene>", more + "</scene>")
