"""Latency of a geometry edit on the atrium (default detail, 960 x 540 film): from "one shape's vertices translated" to "one sample plane finished",
  rebuild:  destroy the render, mi_scene_set_triangles with the new positions, mi_scene_commit (SAH build, every per-triangle table on one host thread, every table
            sent again), create the render, run one plane
  in place: mi_scene_update_vertices (per-triangle records and the refit of the existing tree on the device), mi_render_clear, run one plane on the same render handle.
Same method as scripts/perf_live_edit.py: median of 5 after one warm-up, time.perf_counter around synchronous calls.
python scripts/perf_geometry_edit.py [--detail D] [--out profiles/geometry_edit_latency.txt]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mi = importlib.import_module("mitsuba-im_amd")
from scripts.perf_live_edit import device_name      # noqa: E402


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--detail", type=float, default=1.0); ap.add_argument("--out", default=None); a = ap.parse_args()
    S = mi.scenes; W, H = 960, 540
    t0 = time.perf_counter(); sc = S.atrium(W, H, 4, detail=a.detail); t1 = time.perf_counter()
    gs = mi.Scene(sc); t2 = time.perf_counter(); L = gs.L
    shape = max(range(len(sc.shapes)), key=lambda i: sc.shapes[i]["tri_count"] if sc.shapes[i]["emitter"] < 0 else 0)      # the largest mesh that is not a light
    sl = slice(sc.shapes[shape]["first_vert"], sc.shapes[shape]["first_vert"] + sc.shapes[shape]["vert_count"])
    base = np.ascontiguousarray(sc.pos, np.float32); nrm = None if sc.nrm is None else np.ascontiguousarray(sc.nrm, np.float32)

    def positions(i):
        p = base.copy(); p[sl] += np.asarray((0.05 * (i + 1), 0.02 * (i + 1), -0.03 * (i + 1)), np.float32); return p

    shapes = (mi.api.MiShape * len(sc.shapes))()
    for i, s in enumerate(sc.shapes):
        shapes[i] = mi.api.MiShape(s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"], s["bsdf"], s["emitter"], (s["face_normals"] & 1) | ((s.get("has_uv", 0) & 1) << 1), s.get("group", 0))
    p_ = lambda x: None if x is None else x.ctypes.data
    state = {"render": mi.Render(gs)}; edit_only = []

    def rebuild(i):
        pos = positions(i); t = time.perf_counter()
        state["render"].close()               # a render handle does not survive a commit
        L.check(L.L.mi_scene_set_triangles(gs.h, p_(pos), p_(nrm), p_(sc.uv), p_(sc.idx), len(pos), len(sc.idx), C.cast(shapes, C.c_void_p), len(sc.shapes)))
        L.check(L.L.mi_scene_commit(gs.h, 0))
        state["render"] = mi.Render(gs); state["render"].run(s0=0, s1=1); return time.perf_counter() - t

    def in_place(i):
        pos = positions(i); t = time.perf_counter()
        gs.update_vertices(pos, nrm); edit_only.append(time.perf_counter() - t)      # synchronous: returns when the device has finished
        state["render"].clear(); state["render"].run(s0=0, s1=1); return time.perf_counter() - t

    slow = [rebuild(i) for i in range(6)][1:]          # every commit first: the handle of the in-place runs must not see one
    builds = gs.revision()[1]
    fast = [in_place(i) for i in range(6)][1:]
    after = gs.revision()[1]
    slow_ms, fast_ms = statistics.median(slow) * 1e3, statistics.median(fast) * 1e3
    lines = [f"machine: {device_name()}",
             f"scene: atrium detail {a.detail}, {len(sc.idx)} triangles, {len(sc.pos)} vertices, {W}x{H}, one sample plane per edit; build {t1 - t0:.1f} s (Python), first commit {t2 - t1:.3f} s",
             f"edit: shape {shape} ({sc.shapes[shape]['tri_count']} triangles, {sc.shapes[shape]['vert_count']} vertices) translated; the whole vertex array is sent either way",
             "median of 5 after one warm-up, milliseconds from the edit to the finished plane",
             f"vertices: rebuild (set_triangles + commit + new render) {slow_ms:.1f} ms | in place (update_vertices + clear) {fast_ms:.2f} ms | ratio {slow_ms / fast_ms:.1f}",
             f"in place, each: {' '.join(f'{x * 1e3:.2f}' for x in fast)} ms; rebuild, each: {' '.join(f'{x * 1e3:.1f}' for x in slow)} ms",
             f"update_vertices alone (upload of the vertex arrays, k_tri_records, k_refit level by level, small tables; returns after the device has finished): median {statistics.median(edit_only[1:]) * 1e3:.2f} ms, each {' '.join(f'{x * 1e3:.2f}' for x in edit_only[1:])} ms",
             f"tree builds: {builds} while rebuilding, {after - builds} during the 6 in-place edits"]
    text = "\n".join(lines) + "\n"; print(text, end="")
    assert after == builds and fast_ms < slow_ms, "the in-place edit must build no tree and beat the commit measured in the same run"
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
