"""What a thin lens costs on the Cornell box (1920 x 1080, Sobol, 64 spp, depth 8): the same job as a pinhole and with a lens (radius 2 % of the box, focal plane on the
back wall) -- Msamples/s and the per-stage device times of the profiled run -- and the latency of a focus pull (mi_scene_update_lens + clear + one sample plane) next to a
camera edit on the same render, by the method of scripts/perf_live_edit.py (median of 5 after one warm-up, time.perf_counter around synchronous calls).
The scene is bench.py's C2 workload at 64 spp.  python scripts/perf_thinlens.py [--spp N] [--out FILE]; the recorded run is the second part of profiles/thinlens_bench.txt"""
import argparse
import copy
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mi = importlib.import_module("mitsuba-im_amd")
from scripts.perf_live_edit import device_name  # noqa: E402


def clone(sc):
    return type(sc)({k: copy.deepcopy(v) for k, v in sc.items()})


def rate(scene, spp, runs=3):
    """best of `runs` un-profiled frames (device time of mi_render_run), then one profiled frame for the stage split"""
    r = mi.Render(scene, spp=spp); n = scene.sc.width * scene.sc.height * spp
    r.run(); r.clear()                                                         # warm-up: first launches, allocations
    ms = []
    for _ in range(runs):
        r.clear(); r.run(); ms.append(r.stats()["render_ms"])
    r.set_profiling(True); r.clear(); r.run(); st = r.stats(); r.close()
    return n / min(ms) / 1e3, ms, st


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--spp", type=int, default=64); ap.add_argument("--out", default=None); a = ap.parse_args()
    S = mi.scenes; W, H = 1920, 1080
    plain = S.cornell_box(W, H, a.spp, max_depth=8)
    lo = plain.pos.min(0).astype(np.float64); hi = plain.pos.max(0).astype(np.float64)
    back_wall = (np.linalg.inv(np.asarray(plain.cam_to_world, np.float64)) @ np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[2], 1.0]))[2]
    lens = S.with_lens(clone(plain), 0.02 * float((hi - lo).max()), back_wall)
    lines = [f"machine: {device_name()}", f"scene: Cornell box {W}x{H}, Sobol, {a.spp} spp, maxDepth 8; lens radius {lens.aperture_radius:g}, focus distance {lens.focus_distance:g} (back wall)"]
    gl = None
    for name, sc in (("pinhole", plain), ("lens", lens)):
        gs = mi.Scene(sc); best, ms, st = rate(gs, a.spp)
        lines.append(f"{name}: {best:.1f} Msamples/s (frames {', '.join(f'{m:.1f}' for m in ms)} ms); {st['rays'] / st['samples']:.3f} rays/sample; profiled frame: "
                     f"extend {st['extend_ms']:.1f} ms, shade {st['shade_ms']:.1f} ms, shadow {st['shadow_ms']:.1f} ms, other (generate, film) {st['other_ms']:.1f} ms of {st['render_ms']:.1f} ms")
        if name == "lens": gl = gs
    # edit latency on the lens scene: a focus pull against a camera move, from the edit to one finished sample plane
    r = mi.Render(gl); s2c = np.ascontiguousarray(lens.sample_to_camera, np.float32)
    views = [S.look_at((278 + 10.0 * i, 273, -800), (278, 273, -799), (0, 1, 0)) for i in range(6)]

    def edit(kind, i):
        t = time.perf_counter()
        if kind == "lens": gl.update_lens(lens.aperture_radius, lens.focus_distance * (1.0 - 0.05 * i))
        else: gl.update_camera(s2c, views[i], lens.near, lens.far)
        t_edit = time.perf_counter() - t
        r.clear(); r.run(s0=0, s1=1); return t_edit, time.perf_counter() - t
    builds = gl.revision()[1]
    for kind in ("camera", "lens"):
        t = [edit(kind, i) for i in range(6)][1:]
        lines.append(f"update_{kind}: the call alone {statistics.median(x[0] for x in t) * 1e6:.1f} us | update + clear + one sample plane {statistics.median(x[1] for x in t) * 1e3:.2f} ms (median of 5 after one warm-up)")
    assert gl.revision()[1] == builds
    text = "\n".join(lines) + "\n"; print(text, end="")
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
