"""Latency of a geometry edit on the instanced garden with the large bush (bush_levels = 4: a 2048-triangle group; n_side = 17: 289 instances):
  in place:  mi_scene_update_geometry with new vertices, normals and transforms (inputs up, k_tri_records, k_instance_records, k_refit over every tree level by level,
             returns when the device has finished)
  recommit:  mi_scene_set_triangles + mi_scene_set_instances + mi_scene_commit of the same description on the same handle -- every per-triangle record on one host
             thread, a SAH build of every group tree and of the scene tree, every table sent again; the only way to deform a group member before this call
Each frame sways the bush (a shear in x and z that grows with height, normals by the inverse transpose), stretches the crate and turns every instance about its
origin.  Every figure is a median of repeated runs, the two sides alternating, time.perf_counter around synchronous calls; the first in-place edit after a commit also
allocates the edit's own tables and is timed apart.
python scripts/perf_group_edit.py [--n-side N] [--bush-levels L] [--rounds R] [--out profiles/group_edit_latency.txt]"""
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
    ap = argparse.ArgumentParser(); ap.add_argument("--n-side", type=int, default=17); ap.add_argument("--bush-levels", type=int, default=4); ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None); a = ap.parse_args()
    S = mi.scenes; W, H, SPP = 96, 64, 4; f32 = np.float32
    sc = S.instanced_garden(W, H, SPP, n_side=a.n_side, bush_levels=a.bush_levels); t1 = time.perf_counter()
    gs = mi.Scene(sc); t2 = time.perf_counter(); L = gs.L; M = mi.api
    pos0 = np.array(sc.pos, f32, copy=True); nrm0 = np.array(sc.nrm, f32, copy=True); base = list(sc.instances)
    member = lambda g: np.concatenate([np.arange(s["first_vert"], s["first_vert"] + s["vert_count"]) for s in sc.shapes if s.get("group", 0) == g])
    bush, crate = member(1), member(2); rng = np.random.default_rng(7)
    shapes = (M.MiShape * len(sc.shapes))()
    for i, s in enumerate(sc.shapes):
        shapes[i] = M.MiShape(s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"], s["bsdf"], s["emitter"], (s["face_normals"] & 1) | ((s.get("has_uv", 0) & 1) << 1), s.get("group", 0))
    idx = np.ascontiguousarray(sc.idx); uv = None if sc.uv is None else np.ascontiguousarray(sc.uv); p = lambda x: None if x is None else x.ctypes.data

    def frame():
        """(pos, nrm, instances) of one frame"""
        kx, kz, sy = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.6)
        pos = pos0.copy(); nrm = nrm0.copy()
        pos[bush, 0] += f32(kx) * pos0[bush, 1]; pos[bush, 2] += f32(kz) * pos0[bush, 1]
        n = nrm0[bush].copy(); n[:, 1] -= f32(kx) * n[:, 0] + f32(kz) * n[:, 2]; nrm[bush] = n / np.linalg.norm(n, axis=1, keepdims=True)      # inverse transpose of the shear
        pos[crate, 1] *= f32(sy)
        insts = []
        for inst in base:
            tw = np.asarray(inst["to_world"], np.float64); o = tw[:3, 3]
            insts.append(S.make_instance(inst["group"], S.translate(*o) @ S.rotate((0, 1, 0), rng.uniform(-180, 180)) @ S.translate(*(-o)) @ tw))
        return np.ascontiguousarray(pos, f32), np.ascontiguousarray(nrm, f32), insts

    def recommit(pos, nrm, insts):
        arr = M.pack_instances(insts); t = time.perf_counter()
        L.check(L.L.mi_scene_set_triangles(gs.h, p(pos), p(nrm), p(uv), p(idx), len(pos), len(idx), C.cast(shapes, C.c_void_p), len(sc.shapes)))
        L.check(L.L.mi_scene_set_instances(gs.h, C.cast(arr, C.c_void_p), len(insts))); L.check(L.L.mi_scene_commit(gs.h, 0))
        return time.perf_counter() - t

    def in_place(pos, nrm, insts):
        arr = M.pack_instances(insts); t = time.perf_counter()
        L.check(L.L.mi_scene_update_geometry(gs.h, p(pos), p(nrm), len(pos), C.cast(arr, C.c_void_p), len(insts)))
        return time.perf_counter() - t

    slow, first, fast = [], [], []
    for _ in range(a.rounds + 1):                                      # one warm-up round
        slow.append(recommit(*frame())); builds = gs.revision()[1]
        first.append(in_place(*frame())); fast.append(in_place(*frame()))
        assert gs.revision()[1] == builds
    slow, first, fast = slow[1:], first[1:], fast[1:]
    ms = lambda v: statistics.median(v) * 1e3
    lines = [f"machine: {device_name()}",
             f"scene: instanced_garden n_side {a.n_side}, bush_levels {a.bush_levels}: {len(base)} instances of 2 shape groups, {len(sc.idx)} triangles, {len(pos0)} vertices; first commit {t2 - t1:.3f} s",
             "edit: the bush sheared, the crate stretched, every instance turned about its origin; all vertices, normals and transforms are sent either way",
             f"median of {a.rounds} after one warm-up round, the sides alternating; milliseconds from the call to its return (both return when the device holds the new scene)",
             f"geometry: recommit (set_triangles + set_instances + commit) {ms(slow):.2f} ms | in place (update_geometry) {ms(fast):.3f} ms | ratio {ms(slow) / ms(fast):.1f}",
             f"in place, each: {' '.join(f'{x * 1e3:.3f}' for x in fast)} ms; recommit, each: {' '.join(f'{x * 1e3:.2f}' for x in slow)} ms",
             f"first edit after a commit (allocates and fills the edit's own tables): median {ms(first):.3f} ms, each {' '.join(f'{x * 1e3:.3f}' for x in first)} ms"]
    text = "\n".join(lines) + "\n"; print(text, end="")
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
