"""The scenes of the extra-emitter tests (tests/test_lights_cpu.py, tests/test_lights_gpu.py): tests/corner_scenes.py's box corner at
24 x 24 and at a ragged 21 x 19 with the lights that stand here once — a point light behind wall y = 0 whose top edge shadows a strip of the floor, a
second spot away from the main one, a point light and a wide spot at one position, eight lights — and the scene file of the loader and mi tests.
numpy and fireflies_amd.scenes only: a test without a GPU may import this."""
import numpy as np

from fireflies_amd import loaders, scenes
from tests import corner_scenes as cs

FILMS = {"24x24": (24, 24), "21x19": (21, 19)}
# behind wall y = 0 (its front faces +y: the light does not face it) and above it: the wall's top edge (y = 0, z = 2) shadows the floor up to
# y = 0.5 * 2 / 1.5 = 0.67, and the wall's shadow and the cube's fall onto wall x = 0 and the floor
POINT = scenes.LightData("emit-Light", "point", np.array([[1, 0, 0, 1.0], [0, 1, 0, -0.5], [0, 0, 1, 3.5], [0, 0, 0, 1]], np.float32), (20.0, 18.0, 15.0))
# from the other side of the corner than corner_scenes' spot at (1.8, 2.6, 2.5)
SPOT_B = scenes.LightData("emit-SecondSpot", "spot", scenes.look_at((2.7, 0.6, 2.2), (0.9, 1.2, 0.1), up=(0, 0, 1)), (6.0, 9.0, 12.0), 35.0, 22.0)
# a point light and, at the same position, a spot whose beam_width cone (80 degrees) holds the whole corner: the two render the same image
WIDE_AT = scenes.look_at((2.5, 2.4, 3.0), (0.7, 0.7, 0.5), up=(0, 0, 1))
WIDE_POINT = scenes.LightData("emit-WideP", "point", WIDE_AT, (9.0, 8.0, 7.0))
WIDE_SPOT = scenes.LightData("emit-WideS", "spot", WIDE_AT, (9.0, 8.0, 7.0), 85.0, 80.0)


def corner(film="24x24", principled=False, **kw):
    """the box corner with projector and main spot: Lambert rows (a stride-3 table), or the floor with every lobe active (corner_scenes.EVERY_LOBE)"""
    W, H = FILMS[film]
    if principled:
        return cs.case("every_lobe", W=W, H=H, **kw)[0]
    return cs.scene("lambert", W=W, H=H, **kw)


def eight():
    """eight lights about the corner: points and spots in turn, distinct colours"""
    out = []
    for k in range(8):
        a = 0.25 + 0.15 * k
        eye = (0.8 + 2.0 * np.cos(a), 0.8 + 2.0 * np.sin(a), 1.6 + 0.2 * k)
        col = (3.0 + k, 6.0 - 0.5 * k, 2.0 + 0.7 * k)
        if k % 2:
            out.append(scenes.LightData(f"emit-S{k}", "spot", scenes.look_at(eye, (0.6 + 0.1 * k, 0.9, 0.1), up=(0, 0, 1)), col, 30.0 + 2 * k, 18.0 + k))
        else:
            tw = np.eye(4, dtype=np.float32)
            tw[:3, 3] = eye
            out.append(scenes.LightData(f"emit-P{k}", "point", tw, col))
    return out


# (the names: ff.Scene gathers an entity's attributes from every key that CONTAINS its name, as the reference does — no emitter's name here is part of
# another's)
# ------------------------------------------------------------------ the scene file: projector, spot, a point light given by `position`, one given by
# `to_world`, a second spot — the loader keeps the first spot as SceneData.spot and lists [point, point, spot 2] in file order
def _lookat(eye, target):
    return f'<transform name="to_world"><lookat origin="{eye[0]},{eye[1]},{eye[2]}" target="{target[0]},{target[1]},{target[2]}" up="0,0,1"/></transform>'


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
  <emitter type="point" id="emit-PointLight"><rgb name="intensity" value="2"/><transform name="to_world"><translate x="0.5" y="1.5" z="1.0"/></transform></emitter>
  <emitter type="spot" id="emit-SecondSpot"><rgb name="intensity" value="6, 9, 12"/><float name="cutoff_angle" value="35"/><float name="beam_width" value="22"/>
    {_lookat((2.7, 0.6, 2.2), (0.9, 1.2, 0.1))}</emitter>
</scene>"""


def write_scene(tmp_path, xml=XML, name="lights.xml"):
    """the scene file and its three meshes under tmp_path -> the file's path"""
    for fn, v in (("floor.obj", cs._floor()), ("wallx.obj", cs._wall_x()), ("wally.obj", cs._wall_y())):
        loaders.save_obj(tmp_path / fn, v[0], cs.QUAD)
    (tmp_path / name).write_text(xml)
    return str(tmp_path / name)


def with_extra_points(n):
    """XML with n more point lights behind the last emitter (the loader keeps scenes.MAX_EXTRA_LIGHTS extra emitters in all)"""
    more = "".join(f'<emitter type="point" id="emit-More{k}"><point name="position" value="{0.2 * k}, 1, 2"/></emitter>' for k in range(n))
    return XML.replace("</scene>", more + "</scene>")
