"""Vertex edits of a committed scene (mi_scene_update_vertices), the parts that need no GPU: the entry points exist, every refusal that is decided before a device call
comes with its message, and the host side -- SceneHost::updateVertices / refreshHostGeometry over csrc/geometry_records.h, the very header the device kernels are made
of -- equals a fresh commit byte for byte (tests/host/geometry_edit_host.cpp, run under the sanitizers)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
from tests.conftest import ROOT

NEW_SYMBOLS = ["mi_scene_update_vertices", "mi_debug_read_geometry", "mi_debug_geometry_bytes"]
NEW_HOST_SYMBOLS = ["mi_host_set_vertices"]


def test_vertex_edit_entry_points_are_declared_and_exported(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); host = open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    L = C.CDLL(mi.api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(L, name) and name in mi.api.EXPORTS, name
    for name in NEW_HOST_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", host) and hasattr(L, name) and name in mi.api.HOST_EXPORTS, name
    for name in ("update_vertices", "read_geometry", "clone"):
        assert callable(getattr(mi.api.Scene, name))
    assert callable(mi.api.HostIntegrator.set_vertices)
    mk = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS :=.*\bkernels_geometry\b", mk, re.M)
    src = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "kernels_geometry.hip")).read()
    assert "k_tri_records" in src and "k_refit" in src and "geometry_records.h" in src


def test_vertex_edit_refusals_before_any_device_call(mi):
    """A scene that is not committed and null arguments: MI_ERR_INVALID (1), the message starts with the function's name.  Nothing here reaches a device."""
    L = mi.lib(); h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h)))
    sc = mi.scenes.cornell_box(16, 9, 1); pos = np.ascontiguousarray(sc.pos, np.float32)
    err = lambda: L.L.mi_last_error().decode()
    assert L.L.mi_scene_update_vertices(h, pos.ctypes.data, None, len(pos)) == 1 and err().startswith("mi_scene_update_vertices") and "not committed" in err()
    assert L.L.mi_scene_update_vertices(None, pos.ctypes.data, None, len(pos)) == 1 and err().startswith("mi_scene_update_vertices") and "null" in err()
    assert L.L.mi_scene_update_vertices(h, None, None, len(pos)) == 1 and err().startswith("mi_scene_update_vertices") and "null" in err()
    rev, builds = C.c_uint64(7), C.c_uint64(7)
    assert L.L.mi_scene_revision(h, C.byref(rev), C.byref(builds)) == 0 and (rev.value, builds.value) == (0, 0)
    n = C.c_uint64(5); buf = np.zeros(16, np.uint32)
    assert L.L.mi_debug_read_geometry(h, 0, buf.ctypes.data, 64) == 1 and "mi_debug_read_geometry" in err() and "not committed" in err()
    assert L.L.mi_debug_read_geometry(None, 0, buf.ctypes.data, 64) == 1 and "null" in err()
    assert L.L.mi_debug_geometry_bytes(h, 0, C.byref(n)) == 1 and "not committed" in err()
    assert L.L.mi_debug_geometry_bytes(h, 0, None) == 1 and "null" in err()
    L.L.mi_scene_destroy(h)


def test_host_side_of_a_vertex_edit_equals_a_fresh_commit(tmp_path):
    """tests/host/geometry_edit_host.cpp: a stand-alone program over scene_build.cpp and geometry_records.h, built with the address and undefined-behaviour sanitizers
    and run directly.  It also checks the refusals that need a committed scene (vertex count, normals, non-finite values, instances) with their messages."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"); exe = str(tmp_path / "geometry_edit_host")
    src = [os.path.join(ROOT, "tests", "host", "geometry_edit_host.cpp"), os.path.join(ROOT, "mitsuba-im_amd", "csrc", "scene_build.cpp")]
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] + src + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr


def test_wavy_sheet_keeps_its_structure(mi):
    """scenes.wavy_sheet: the parameters of an edit move positions and normals only"""
    S = mi.scenes; A = S.wavy_sheet(8); B = S.wavy_sheet(8, phase=1.3, amp=0.3, lift=2.5, light_size=0.2, light_x=0.5)
    assert len(A.idx) == 2 * 8 * 8 + 4 and (A.idx == B.idx).all() and (A.uv == B.uv).all() and A.shapes == B.shapes and len(A.pos) == len(A.nrm) == len(A.uv)
    assert not (A.pos == B.pos).all() and not (A.nrm == B.nrm).all() and np.allclose(np.linalg.norm(B.nrm, axis=1), 1.0, atol=1e-6)
    assert A.shapes[0]["face_normals"] == 0 and A.shapes[0]["has_uv"] == 1 and A.shapes[1]["emitter"] == 0
