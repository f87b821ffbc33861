"""In-place edits of a committed scene (mi_scene_update_*), the parts that need no GPU: the new entry points exist, refuse what they must before any device call, and
the host side of every edit -- the tables commitHost() / upload() derive -- equals a fresh commit (tests/host/live_edit_host.cpp, run under the sanitizers)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
from tests.conftest import ROOT

NEW_SYMBOLS = ["mi_scene_update_camera", "mi_scene_update_materials", "mi_scene_update_emitters", "mi_scene_update_envmap_transform", "mi_scene_revision"]
NEW_HOST_SYMBOLS = ["mi_host_set_camera", "mi_host_set_materials", "mi_host_set_emitters", "mi_host_set_envmap_transform"]


def test_update_entry_points_are_declared_and_exported(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); host = open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    L = C.CDLL(mi.api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(L, name) and name in mi.api.EXPORTS, name
    for name in NEW_HOST_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", host) and hasattr(L, name) and name in mi.api.HOST_EXPORTS, name
    for name in ("update_camera", "update_materials", "update_emitters", "update_envmap", "revision"):
        assert callable(getattr(mi.api.Scene, name))
    assert callable(mi.api.HostIntegrator.set_camera)


def test_updates_need_a_committed_scene_and_arguments(mi):
    """Each update on a scene that is not committed: MI_ERR_INVALID (1); null arguments are refused by name.  Nothing here reaches a device."""
    L = mi.lib(); h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h)))
    sc = mi.scenes.cornell_box(16, 9, 1); eye = np.eye(4, dtype=np.float32)
    mats = mi.api.pack_materials(sc.bsdfs); ems = mi.api.pack_emitters(sc.emitters)
    L.check(L.L.mi_scene_set_materials(h, C.cast(mats, C.c_void_p), len(sc.bsdfs))); L.check(L.L.mi_scene_set_emitters(h, C.cast(ems, C.c_void_p), len(sc.emitters)))
    err = lambda: L.L.mi_last_error().decode()
    assert L.L.mi_scene_update_camera(h, eye.ctypes.data, eye.ctypes.data, 0.1, 10.0) == 1 and "mi_scene_update_camera" in err() and "not committed" in err()
    assert L.L.mi_scene_update_materials(h, C.cast(mats, C.c_void_p), len(sc.bsdfs)) == 1 and "mi_scene_update_materials" in err() and "not committed" in err()
    assert L.L.mi_scene_update_emitters(h, C.cast(ems, C.c_void_p), len(sc.emitters)) == 1 and "mi_scene_update_emitters" in err() and "not committed" in err()
    assert L.L.mi_scene_update_envmap_transform(h, eye.ctypes.data, 1.0) == 1 and "mi_scene_update_envmap_transform" in err() and "not committed" in err()
    # null arguments
    assert L.L.mi_scene_update_camera(None, eye.ctypes.data, eye.ctypes.data, 0.1, 10.0) == 1 and "null" in err()
    assert L.L.mi_scene_update_camera(h, None, eye.ctypes.data, 0.1, 10.0) == 1 and "null" in err()
    assert L.L.mi_scene_update_camera(h, eye.ctypes.data, None, 0.1, 10.0) == 1
    assert L.L.mi_scene_update_materials(h, None, 4) == 1 and "null" in err()
    assert L.L.mi_scene_update_materials(h, C.cast(mats, C.c_void_p), 0) == 1
    assert L.L.mi_scene_update_materials(None, C.cast(mats, C.c_void_p), 4) == 1
    assert L.L.mi_scene_update_emitters(h, None, 1) == 1 and "null" in err()
    assert L.L.mi_scene_update_emitters(None, C.cast(ems, C.c_void_p), 1) == 1
    assert L.L.mi_scene_update_envmap_transform(h, None, 1.0) == 1 and "null" in err()
    assert L.L.mi_scene_update_envmap_transform(None, eye.ctypes.data, 1.0) == 1
    assert L.L.mi_scene_revision(None, None, None) == 1 and "null" in err()
    rev, builds = C.c_uint64(7), C.c_uint64(7)
    assert L.L.mi_scene_revision(h, C.byref(rev), C.byref(builds)) == 0 and (rev.value, builds.value) == (0, 0)      # nothing committed, nothing edited
    assert L.L.mi_scene_revision(h, None, None) == 0
    # the setters still un-commit as before and share their value checks with the updates: the same message from either door
    bad = mi.api.pack_materials(sc.bsdfs); bad[0].type = 99
    assert L.L.mi_scene_set_materials(h, C.cast(bad, C.c_void_p), len(sc.bsdfs)) == 3 and "implemented BSDFs" in err()
    L.L.mi_scene_destroy(h)


def test_host_side_of_every_edit_equals_a_fresh_commit(tmp_path):
    """tests/host/live_edit_host.cpp: a stand-alone program over scene_build.cpp alone, built with the address and undefined-behaviour sanitizers and run directly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"); exe = str(tmp_path / "live_edit_host")
    src = [os.path.join(ROOT, "tests", "host", "live_edit_host.cpp"), os.path.join(ROOT, "mitsuba-im_amd", "csrc", "scene_build.cpp")]
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] + src + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr


def test_orbit_cameras(mi):
    """render.py --orbit: frame 0 is the scene's own camera bit for bit; every frame keeps the distance to the centre of the scene's box and an orthonormal frame;
    N steps of 360 / N degrees about the chosen axis leave that axis' coordinate alone."""
    import importlib
    R = importlib.import_module("mitsuba-im_amd.render"); sc = mi.scenes.cornell_box(16, 9, 1)
    centre = (sc.pos.min(0).astype(np.float64) + sc.pos.max(0)) * 0.5
    for axis in "xyz":
        cams = R.orbit_cameras(sc, 8, axis); k = "xyz".index(axis)
        assert len(cams) == 8 and cams[0].dtype == np.float32 and cams[0].tobytes() == np.ascontiguousarray(sc.cam_to_world, np.float32).tobytes()
        d0 = np.linalg.norm(sc.cam_to_world[:3, 3] - centre)
        for c in cams:
            assert abs(np.linalg.norm(c[:3, 3] - centre) - d0) < 1e-3 * d0 and np.allclose(c[:3, :3].T @ c[:3, :3], np.eye(3), atol=1e-5)
            assert abs(c[k, 3] - sc.cam_to_world[k, 3]) < 1e-3 * d0
        assert np.allclose(cams[4][:3, 3] - centre, -(cams[0][:3, 3] - centre) * np.where(np.arange(3) == k, -1, 1), atol=1e-2)      # half a turn
        assert not np.allclose(cams[1][:3, 3], cams[7][:3, 3], atol=1.0)
