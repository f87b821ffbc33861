"""Instance edits of a committed scene (mi_scene_update_instances), the parts that need no GPU: the entry points exist, every refusal that is decided before a device call
comes with its message, and the host side -- SceneHost::updateInstances / refreshHostGeometry over csrc/geometry_records.h, the very header the device kernels are made
of -- equals a fresh commit (tests/host/instance_edit_host.cpp, run under the sanitizers)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
from tests.conftest import ROOT


def test_instance_edit_entry_points_are_declared_and_exported(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); host = open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    L = C.CDLL(mi.api.LIB_PATH)
    assert re.search(r"\bmi_scene_update_instances\s*\(", hdr) and hasattr(L, "mi_scene_update_instances") and "mi_scene_update_instances" in mi.api.EXPORTS
    assert re.search(r"\bmi_host_set_instances\s*\(", host) and hasattr(L, "mi_host_set_instances") and "mi_host_set_instances" in mi.api.HOST_EXPORTS
    assert re.search(r"#define\s+MI_GEOMETRY_INSTANCES\s+6\b", hdr) and re.search(r"#define\s+MI_GEOMETRY_SCENE_BOX\s+7\b", hdr)
    assert mi.api.Scene.GEOMETRY_TABLES["instances"] == (6, 128) and mi.api.Scene.GEOMETRY_TABLES["scene_box"] == (7, 24)
    assert callable(mi.api.Scene.update_instances) and callable(mi.api.HostIntegrator.set_instances)
    src = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "kernels_geometry.hip")).read()
    assert "k_instance_records" in src and "geometry_records.h" in src


def test_instance_edit_refusals_before_any_device_call(mi):
    """A scene that is not committed and null arguments: MI_ERR_INVALID (1), the message starts with the function's name.  Nothing here reaches a device."""
    L = mi.lib(); h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h)))
    sc = mi.scenes.instanced_garden(16, 9, 1, n_side=2); arr = mi.api.pack_instances(sc.instances); n = len(sc.instances); p = C.cast(arr, C.c_void_p)
    err = lambda: L.L.mi_last_error().decode()
    assert L.L.mi_scene_update_instances(h, p, n) == 1 and err().startswith("mi_scene_update_instances") and "not committed" in err()
    assert L.L.mi_scene_update_instances(None, p, n) == 1 and err().startswith("mi_scene_update_instances") and "null" in err()
    assert L.L.mi_scene_update_instances(h, None, n) == 1 and err().startswith("mi_scene_update_instances") and "null" in err()
    rev, builds = C.c_uint64(7), C.c_uint64(7)
    assert L.L.mi_scene_revision(h, C.byref(rev), C.byref(builds)) == 0 and (rev.value, builds.value) == (0, 0)
    nb = C.c_uint64(5); buf = np.zeros(32, np.uint32)
    for what in (6, 7):
        assert L.L.mi_debug_read_geometry(h, what, buf.ctypes.data, 24) == 1 and "not committed" in err()
        assert L.L.mi_debug_geometry_bytes(h, what, C.byref(nb)) == 1 and "not committed" in err()
    L.L.mi_scene_destroy(h)


def test_host_side_of_an_instance_edit_equals_a_fresh_commit(tmp_path):
    """tests/host/instance_edit_host.cpp: a stand-alone program over scene_build.cpp and geometry_records.h, built with the address and undefined-behaviour sanitizers
    and run directly.  It also checks the refusals that need a committed scene (count, group, non-finite values, no instances) with their messages."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"); exe = str(tmp_path / "instance_edit_host")
    src = [os.path.join(ROOT, "tests", "host", "instance_edit_host.cpp"), os.path.join(ROOT, "mitsuba-im_amd", "csrc", "scene_build.cpp")]
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] + src + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr


def test_garden_placements_differ_by_seed_only(mi):
    """scenes.instanced_garden: `seed` moves the placements (and seeds the sampler) and nothing else -- what the GPU tests of the edit rely on."""
    S = mi.scenes; A = S.instanced_garden(48, 32, 4); B = S.instanced_garden(48, 32, 4, seed=1)
    assert (A.pos == B.pos).all() and (A.idx == B.idx).all() and A.shapes == B.shapes and len(A.instances) == len(B.instances) == 16
    assert [i["group"] for i in A.instances] == [i["group"] for i in B.instances]
    assert all(not np.array_equal(a["to_world"], b["to_world"]) for a, b in zip(A.instances, B.instances))
