"""Thin-lens sensor (src/sensors/thinlens.cpp), the parts that need no GPU: the entry points exist, every refusal comes back with its code and names its function
before any device call, and the front end (scene files, the scene description, the MISCENE2 writer, render.py) carries the aperture radius and the focus distance."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from tests.conftest import GOLDEN, ROOT

NEW_SYMBOLS = ["mi_scene_set_lens", "mi_scene_update_lens", "mi_debug_camera_rays_lens", "mi_render_debug_sensor_differentials"]
NEW_HOST_SYMBOLS = ["mi_host_set_lens"]
DOF_ROW = os.path.join(GOLDEN, "scenes", "dof_row.xml")
LENS_SCENE = """<scene version="0.5.0"><integrator type="path"/>
<sensor type="thinlens">{sensor}<film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="32"/></film></sensor>
<shape type="rectangle"><emitter type="area"><spectrum name="radiance" value="3"/></emitter></shape></scene>"""


def xml_scene():
    return importlib.import_module("mitsuba-im_amd.xml_scene")


def load_text(tmp_path, text):
    p = tmp_path / "s.xml"; p.write_text(text)
    return xml_scene().load_scene(str(p))


def test_lens_entry_points_are_declared_exported_and_bound(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); host = open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    L = C.CDLL(mi.api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(L, name) and name in mi.api.EXPORTS, name
    for name in NEW_HOST_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", host) and hasattr(L, name) and name in mi.api.HOST_EXPORTS, name
    for name in ("update_lens", "camera_rays"):
        assert callable(getattr(mi.api.Scene, name))
    assert callable(mi.api.HostIntegrator.set_lens)
    lib = mi.lib().L
    assert lib.mi_scene_set_lens.argtypes == [C.c_void_p, C.c_float, C.c_float] and lib.mi_scene_update_lens.argtypes == [C.c_void_p, C.c_float, C.c_float]
    assert len(lib.mi_debug_camera_rays_lens.argtypes) == 5


def test_lens_refusals_name_their_function(mi):
    """Every refusal of mi_scene_set_lens / mi_scene_update_lens / mi_debug_camera_rays_lens that needs no committed scene: MI_ERR_INVALID (1), the message starts with
    the function's name.  Nothing here reaches a device."""
    L = mi.lib(); h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h)))
    err = lambda: L.L.mi_last_error().decode()
    inf, nan = float("inf"), float("nan")
    assert L.L.mi_scene_set_lens(None, 0.1, 1.0) == 1 and err().startswith("mi_scene_set_lens: ") and "null" in err()
    assert L.L.mi_scene_update_lens(None, 0.1, 1.0) == 1 and err().startswith("mi_scene_update_lens: ") and "null" in err()
    for fn, name in ((L.L.mi_scene_set_lens, "mi_scene_set_lens"), (L.L.mi_scene_update_lens, "mi_scene_update_lens")):
        for radius in (-0.1, inf, nan):
            assert fn(h, radius, 1.0) == 1 and err().startswith(name + ": ") and "aperture radius" in err(), (name, radius, err())
        for focus in (0.0, -2.0, inf, nan):
            assert fn(h, 0.1, focus) == 1 and err().startswith(name + ": ") and "focus distance" in err(), (name, focus, err())
    # an update edits a committed scene; this one is not
    assert L.L.mi_scene_update_lens(h, 0.1, 1.0) == 1 and err().startswith("mi_scene_update_lens: ") and "not committed" in err()
    # the setter: a lens, then the pinhole again (the focus distance is ignored with radius 0)
    assert L.L.mi_scene_set_lens(h, 0.1, 1.0) == 0
    assert L.L.mi_scene_set_lens(h, 0.0, -5.0) == 0
    out = np.zeros(14, np.float32); pos = np.zeros(2, np.float32)
    assert L.L.mi_debug_camera_rays_lens(None, pos.ctypes.data, pos.ctypes.data, 1, out.ctypes.data) == 1 and err().startswith("mi_debug_camera_rays_lens: ")
    assert L.L.mi_debug_camera_rays_lens(h, pos.ctypes.data, pos.ctypes.data, 1, out.ctypes.data) == 1 and err().startswith("mi_debug_camera_rays_lens: ")      # not committed
    L.L.mi_scene_destroy(h)


def test_dof_row_loads_with_its_lens(mi):
    sc = xml_scene().load_scene(DOF_ROW)
    assert sc.aperture_radius == float(np.float32(0.15)) and sc.focus_distance == 6.0
    assert (sc.width, sc.height, sc.spp, sc.max_depth) == (96, 64, 8, 5) and len(sc.analytic) >= 3 and len(sc.textures) == 1
    # a perspective sensor carries no lens, whatever focusDistance says (ProjectiveCamera reads it, the pinhole ignores it)
    plain = xml_scene().load_scene(os.path.join(GOLDEN, "scenes", "fog_ball.xml"))
    assert plain.aperture_radius == 0.0 and plain.focus_distance == 0.0
    assert mi.scenes.cornell_box(16, 9, 1).aperture_radius == 0.0


def test_export_round_trips_the_lens(mi, tmp_path):
    X = xml_scene(); sc = X.load_scene(DOF_ROW)
    mi.scenes.with_lens(sc, 0.123456789, 7.654321)
    path = X.export_scene(sc, str(tmp_path / "a"), "lens")
    text = open(path).read(); assert '<sensor type="thinlens">' in text and "apertureRadius" in text and "focusDistance" in text
    back = X.load_scene(path)
    assert np.float32(back.aperture_radius) == np.float32(sc.aperture_radius) and np.float32(back.focus_distance) == np.float32(sc.focus_distance)
    assert back.aperture_radius > 0 and np.array_equal(back.cam_to_world, sc.cam_to_world) and back.xfov == sc.xfov
    # without a lens the sensor goes back as `perspective`
    mi.scenes.with_lens(sc, 0.0, 0.0); path = X.export_scene(sc, str(tmp_path / "b"), "pinhole")
    assert '<sensor type="perspective">' in open(path).read() and X.load_scene(path).aperture_radius == 0.0


def test_thinlens_properties(tmp_path):
    X = xml_scene()
    sc = load_text(tmp_path, LENS_SCENE.format(sensor='<float name="apertureRadius" value="0"/><float name="focusDistance" value="3"/>'))
    assert np.float32(sc.aperture_radius) == np.float32(1e-4) and sc.focus_distance == 3.0             # thinlens.cpp:134-138: zero becomes Epsilon
    sc = load_text(tmp_path, LENS_SCENE.format(sensor='<float name="apertureRadius" value="0.25"/><float name="farClip" value="50"/>'))
    assert sc.aperture_radius == 0.25 and sc.focus_distance == 50.0                                      # sensor.cpp:161: focusDistance defaults to farClip
    sc = load_text(tmp_path, LENS_SCENE.format(sensor='<float name="apertureRadius" value="0.25"/>'))
    assert sc.focus_distance == float(np.float32(1e4))
    with pytest.raises(X.SceneError, match="apertureRadius"):                                           # props.getFloat("apertureRadius") has no default
        load_text(tmp_path, LENS_SCENE.format(sensor=""))
    with pytest.raises(X.SceneError, match="Scale factors in the camera-to-world"):
        load_text(tmp_path, LENS_SCENE.format(sensor='<float name="apertureRadius" value="0.1"/><transform name="toWorld"><scale value="2"/></transform>'))
    with pytest.raises(X.SceneError, match="focusDistance"):
        load_text(tmp_path, LENS_SCENE.format(sensor='<float name="apertureRadius" value="0.1"/><float name="focusDistance" value="-1"/>'))
    with pytest.raises(X.SceneError, match=r'sensor "orthographic" is not supported \(perspective, thinlens\)'):
        load_text(tmp_path, LENS_SCENE.replace('type="thinlens"', 'type="orthographic"').format(sensor=""))


def test_miscene2_writer_refuses_a_lens(mi, tmp_path):
    sc = mi.scenes.cornell_box(16, 9, 1); path = str(tmp_path / "s.bin")
    mi.scenes.save_scene(sc, path); assert os.path.getsize(path) > 0                                     # the pinhole scene is written as before
    mi.scenes.with_lens(sc, 0.05, 2.0)
    with pytest.raises(ValueError, match="save_scene.*thin lens"):
        mi.scenes.save_scene(sc, str(tmp_path / "lens.bin"))
    assert not os.path.exists(str(tmp_path / "lens.bin"))
    with pytest.raises(ValueError, match="with_lens"):
        mi.scenes.with_lens(sc, 0.05, 0.0)


def test_focus_distances():
    R = importlib.import_module("mitsuba-im_amd.render")
    assert R.focus_distances(1, 2.0, 9.0) == [2.0] and R.focus_distances(3, 2.0, 4.0) == [2.0, 3.0, 4.0]
    d = R.focus_distances(7, 0.3, 11.1); assert d[0] == 0.3 and d[-1] == 11.1 and all(a < b for a, b in zip(d, d[1:]))


def test_focus_pull_needs_a_thinlens_sensor(tmp_path):
    """render.py --focus-pull on a perspective scene ends with its message before anything is committed"""
    xml = os.path.join(GOLDEN, "scenes", "fog_ball.xml")
    env = dict(os.environ); env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "mitsuba-im_amd.render", xml, "-o", str(tmp_path / "o.exr"), "--focus-pull", "3", "--focus-from", "2", "--focus-to", "4"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--focus-pull" in r.stderr and "thinlens" in r.stderr, r.stdout + r.stderr
    assert not list(tmp_path.glob("o*.exr"))
