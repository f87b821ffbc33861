"""Geometry edits of a committed scene (mi_scene_update_geometry: vertices, shape-group members included, and / or instance transforms in one call), the parts that
need no GPU: the entry points exist, every refusal that is decided before a device call comes with its message, the garden generator's new keyword leaves the default
scene as it was, and the host side -- SceneHost::updateGeometry / refreshHostGeometry over csrc/geometry_records.h, the very header the device kernels are made of --
equals a fresh commit in any interleaving with the two older calls (tests/host/group_edit_host.cpp, run under the sanitizers)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
from tests.conftest import ROOT


def test_geometry_edit_entry_points_are_declared_and_exported(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); host = open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    L = C.CDLL(mi.api.LIB_PATH)
    assert re.search(r"\bmi_scene_update_geometry\s*\(", hdr) and hasattr(L, "mi_scene_update_geometry") and "mi_scene_update_geometry" in mi.api.EXPORTS
    assert re.search(r"\bmi_host_set_geometry\s*\(", host) and hasattr(L, "mi_host_set_geometry") and "mi_host_set_geometry" in mi.api.HOST_EXPORTS
    assert callable(mi.api.Scene.update_geometry) and callable(mi.api.HostIntegrator.set_geometry)
    assert hasattr(L, "mi_scene_update_vertices") and hasattr(L, "mi_scene_update_instances")      # the two older calls stay
    src = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "geometry_records.h")).read()
    assert "groupBox" in src and "geoInstanceRecord" in src


def test_geometry_edit_refusals_before_any_device_call(mi):
    """A scene that is not committed, a null scene, both parts null: MI_ERR_INVALID (1), the message starts with the function's name.  Nothing here reaches a device."""
    L = mi.lib(); h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h)))
    sc = mi.scenes.instanced_garden(16, 9, 1, n_side=2); arr = mi.api.pack_instances(sc.instances); n = len(sc.instances); p = C.cast(arr, C.c_void_p)
    pos = np.ascontiguousarray(sc.pos, np.float32); nrm = np.ascontiguousarray(sc.nrm, np.float32); nv = len(pos)
    err = lambda: L.L.mi_last_error().decode()
    call = L.L.mi_scene_update_geometry
    for args in ((pos.ctypes.data, nrm.ctypes.data, nv, p, n), (pos.ctypes.data, nrm.ctypes.data, nv, None, 0), (None, None, 0, p, n)):
        assert call(h, *args) == 1 and err().startswith("mi_scene_update_geometry: ") and "not committed" in err()
        assert call(None, *args) == 1 and err().startswith("mi_scene_update_geometry: ") and "null scene" in err()
    assert call(h, None, None, 0, None, 0) == 1 and err().startswith("mi_scene_update_geometry: ") and "null argument" in err() and "neither" in err()
    rev, builds = C.c_uint64(7), C.c_uint64(7)
    assert L.L.mi_scene_revision(h, C.byref(rev), C.byref(builds)) == 0 and (rev.value, builds.value) == (0, 0)
    L.L.mi_scene_destroy(h)


def test_host_side_of_a_geometry_edit_equals_a_fresh_commit(tmp_path):
    """tests/host/group_edit_host.cpp: a stand-alone program over scene_build.cpp and geometry_records.h, built with the address and undefined-behaviour sanitizers and
    run directly.  Vertices only, instances only, both; both node kinds; every tree conservative; back restores every byte; the interleavings with the two older
    calls; the refusals that need a committed scene with their codes and messages."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"); exe = str(tmp_path / "group_edit_host")
    src = [os.path.join(ROOT, "tests", "host", "group_edit_host.cpp"), os.path.join(ROOT, "mitsuba-im_amd", "csrc", "scene_build.cpp")]
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] + src + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr


def test_garden_bush_levels(mi):
    """scenes.instanced_garden(bush_levels=...): the default is the scene every fixture was made from; 4 levels give the 2048-triangle bush whose tree has levels wider
    than one workgroup; nothing but the bush changes."""
    S = mi.scenes; A = S.instanced_garden(48, 32, 4); B = S.instanced_garden(48, 32, 4, bush_levels=2)
    assert A.pos.tobytes() == B.pos.tobytes() and A.nrm.tobytes() == B.nrm.tobytes() and A.idx.tobytes() == B.idx.tobytes() and A.shapes == B.shapes
    assert all(a["group"] == b["group"] and np.array_equal(a["to_world"], b["to_world"]) for a, b in zip(A.instances, B.instances))
    assert len(A.idx) == 2 + 2 + 128 + 8 + 2 and A.shapes[2]["vert_count"] == 66
    D = S.instanced_garden(48, 32, 4, bush_levels=4)
    assert len(D.idx) == 2062 and D.shapes[2]["tri_count"] == 2048 and D.shapes[2]["vert_count"] == 1026 and D.shapes[2]["group"] == 1
    assert [s["group"] for s in D.shapes] == [s["group"] for s in A.shapes] and len(D.instances) == len(A.instances)
    assert (D.pos[:8] == A.pos[:8]).all() and (D.pos[-20:] == A.pos[-20:]).all()      # floor, light and crate as before
