"""Latency of an edit on the atrium (default detail, 960 x 540 film): from "camera / material changed" to "one sample plane finished",
  rebuild:  the only way before the in-place edits -- destroy the render, mi_scene_set_*, mi_scene_commit (tree build + upload of every table), create the render, run one plane
  in place: mi_scene_update_*, mi_render_clear, run one plane on the same render handle.
Median of 5 after one warm-up, time.perf_counter around synchronous calls.  python scripts/perf_live_edit.py [--detail D] [--out profiles/live_edit_latency.txt]"""
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


def device_name():
    """hipDeviceGetName of device 0 through the HIP runtime the library is linked to; where the runtime knows no product name, the agents' architectures"""
    try:
        hip = C.CDLL("libamdhip64.so"); buf = C.create_string_buffer(256)
        hip.hipDeviceGetName.argtypes = [C.c_char_p, C.c_int, C.c_int]
        if hip.hipDeviceGetName(buf, 256, 0) == 0 and buf.value.strip():
            return buf.value.decode().strip()
    except OSError:
        pass
    try:
        import subprocess
        archs = [a for a in subprocess.run(["rocm_agent_enumerator"], capture_output=True, text=True, timeout=30).stdout.split() if a != "gfx000"]
        return f"{archs[0]} (no product name reported by the runtime)" if archs else "unknown"
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--detail", type=float, default=1.0); ap.add_argument("--out", default=None); a = ap.parse_args()
    S = mi.scenes; W, H = 960, 540
    t0 = time.perf_counter(); sc = S.atrium(W, H, 4, detail=a.detail); t1 = time.perf_counter()
    gs = mi.Scene(sc); t2 = time.perf_counter(); L = gs.L
    views = [S.look_at((-14.4 + 2.0 * i, 3.2 + 0.2 * i, 0.5), (3.6, 1.2, -1.0 + 0.5 * i), (0, 1, 0)) for i in range(6)]
    s2c = np.ascontiguousarray(sc.sample_to_camera, np.float32)
    colours = [(0.3 + 0.1 * i, 0.5, 0.6 - 0.05 * i) for i in range(6)]

    def materials(i):
        b = [dict(x) for x in sc.bsdfs]; b[0]["reflectance"] = colours[i]; return b

    state = {"render": mi.Render(gs)}

    def rebuild(kind, i):
        t = time.perf_counter()
        state["render"].close()               # a render handle does not survive a commit
        if kind == "camera":
            L.check(L.L.mi_scene_set_camera(gs.h, s2c.ctypes.data, views[i].ctypes.data, sc.near, sc.far))
        else:
            m = mi.api.pack_materials(materials(i)); L.check(L.L.mi_scene_set_materials(gs.h, C.cast(m, C.c_void_p), len(sc.bsdfs)))
        L.check(L.L.mi_scene_commit(gs.h, 0))
        state["render"] = mi.Render(gs); state["render"].run(s0=0, s1=1); return time.perf_counter() - t

    def in_place(kind, i):
        t = time.perf_counter()
        if kind == "camera": gs.update_camera(s2c, views[i], sc.near, sc.far)
        else: gs.update_materials(materials(i))
        state["render"].clear(); state["render"].run(s0=0, s1=1); return time.perf_counter() - t

    lines = [f"machine: {device_name()}", f"scene: atrium detail {a.detail}, {len(sc.idx)} triangles, {W}x{H}, one sample plane per edit; build {t1 - t0:.1f} s (Python), first commit {t2 - t1:.3f} s",
             "median of 5 after one warm-up, milliseconds from the edit to the finished plane"]
    kinds = ("camera", "material colour")
    slow = {k: [rebuild(k.split()[0], i) for i in range(6)][1:] for k in kinds}          # every commit first: the handle of the in-place runs must not see one
    builds = gs.revision()[1]
    fast = {k: [in_place(k.split()[0], i) for i in range(6)][1:] for k in kinds}
    assert gs.revision()[1] == builds
    for k in kinds:
        lines.append(f"{k}: rebuild (set + commit + new render) {statistics.median(slow[k]) * 1e3:.1f} ms | in place (update + clear) {statistics.median(fast[k]) * 1e3:.2f} ms")
    lines.append(f"tree builds: {builds} while rebuilding, {gs.revision()[1] - builds} during the {2 * 6} in-place edits")
    text = "\n".join(lines) + "\n"; print(text, end="")
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
