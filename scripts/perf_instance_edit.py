"""Latency of an instance edit on the instanced garden (n_side = 32: 1024 instances, 960 x 540 film), and what the kept tree costs afterwards:
  in place:  mi_scene_update_instances (transform pairs up, k_instance_records, k_refit over the scene-level tree, returns when the device has finished)
  recommit:  mi_scene_set_instances + mi_scene_commit on the same handle -- every per-triangle record on one host thread, a SAH build of every group tree and of the
             scene tree, every table sent again; the only way to move an instance before the in-place edit (a render handle does not survive it)
  decay:     Msamples/s of a short render (4 planes) after 16 successive random edits on one tree, against the same render on a fresh commit of that final placement.
Every figure is a median of repeated runs, the two sides alternating (recommit, in place, recommit, ...; edited tree, fresh tree, ...), time.perf_counter around
synchronous calls.  An in-place edit right after a commit also allocates the edit's own tables; it is timed apart ("first edit") and the steady state is what the
comparison uses.  `--bench FILE` appends the lines of FILE (the bench.py headline of this commit and of its parent, measured apart) to the output.
python scripts/perf_instance_edit.py [--n-side N] [--rounds R] [--bench FILE] [--out profiles/instance_edit_latency.txt]"""
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
    ap = argparse.ArgumentParser(); ap.add_argument("--n-side", type=int, default=32); ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bench", default=None); ap.add_argument("--out", default=None); a = ap.parse_args()
    S = mi.scenes; W, H, SPP = 960, 540, 4
    t0 = time.perf_counter(); sc = S.instanced_garden(W, H, SPP, n_side=a.n_side); t1 = time.perf_counter()
    gs = mi.Scene(sc); t2 = time.perf_counter(); L = gs.L; base = list(sc.instances); n = len(base)
    rng = np.random.default_rng(7)

    def random_placement(frm, amount=1.0):
        """every instance turned about its own origin by up to 180 degrees and shifted by up to `amount` in x and z"""
        out = []
        for inst in frm:
            tw = np.asarray(inst["to_world"], np.float64); o = tw[:3, 3]
            m = S.translate(o[0] + rng.uniform(-amount, amount), o[1], o[2] + rng.uniform(-amount, amount)) @ S.rotate((0, 1, 0), rng.uniform(-180, 180)) @ S.translate(-o[0], -o[1], -o[2]) @ tw
            out.append(S.make_instance(inst["group"], m))
        return out

    def recommit(insts):
        arr = mi.api.pack_instances(insts); t = time.perf_counter()
        L.check(L.L.mi_scene_set_instances(gs.h, C.cast(arr, C.c_void_p), len(insts))); L.check(L.L.mi_scene_commit(gs.h, 0))
        dt = time.perf_counter() - t; gs.sc.instances = insts; return dt

    def in_place(insts):
        arr = mi.api.pack_instances(insts); t = time.perf_counter()
        L.check(L.L.mi_scene_update_instances(gs.h, C.cast(arr, C.c_void_p), len(insts)))
        dt = time.perf_counter() - t; gs.sc.instances = insts; return dt

    slow, first, fast = [], [], []
    for _ in range(a.rounds + 1):                                      # one warm-up round
        slow.append(recommit(random_placement(base))); builds = gs.revision()[1]
        first.append(in_place(random_placement(base))); fast.append(in_place(random_placement(base)))
        assert gs.revision()[1] == builds
    slow, first, fast = slow[1:], first[1:], fast[1:]

    def rate(scene):
        r = mi.Render(scene); r.run(); r.clear(); t = time.perf_counter(); r.run(); dt = time.perf_counter() - t; r.close(); return W * H * SPP / dt / 1e6
    edited, fresh = [], []
    for _ in range(max(3, a.rounds // 2)):
        recommit(base); cur = base
        for _ in range(16): cur = random_placement(cur, 0.5); in_place(cur)
        edited.append(rate(gs))
        fs = mi.Scene(type(sc)(sc, instances=cur)); fresh.append(rate(fs)); fs.close()
    ms = lambda v: statistics.median(v) * 1e3
    lines = [f"machine: {device_name()}",
             f"scene: instanced_garden n_side {a.n_side}, {n} instances of 2 shape groups, {len(sc.idx)} triangles, {W}x{H}; build {t1 - t0:.1f} s (Python), first commit {t2 - t1:.3f} s",
             "edit: every instance turned about its own origin and shifted; all transforms are sent either way",
             f"median of {a.rounds} after one warm-up round, the sides alternating; milliseconds from the call to its return (both return when the device holds the new scene)",
             f"instances: recommit (set_instances + commit) {ms(slow):.2f} ms | in place (update_instances) {ms(fast):.3f} ms | ratio {ms(slow) / ms(fast):.0f}",
             f"in place, each: {' '.join(f'{x * 1e3:.3f}' for x in fast)} ms; recommit, each: {' '.join(f'{x * 1e3:.2f}' for x in slow)} ms",
             f"first edit after a commit (allocates and fills the edit's own tables): median {ms(first):.3f} ms, each {' '.join(f'{x * 1e3:.3f}' for x in first)} ms",
             f"tree quality: {SPP} planes after 16 successive random edits on one tree {statistics.median(edited):.1f} Msamples/s | fresh commit of the same placement {statistics.median(fresh):.1f} Msamples/s | ratio {statistics.median(edited) / statistics.median(fresh):.3f}",
             f"edited tree, each: {' '.join(f'{x:.1f}' for x in edited)}; fresh tree, each: {' '.join(f'{x:.1f}' for x in fresh)}"]
    if a.bench and os.path.exists(a.bench):
        lines += [ln.rstrip("\n") for ln in open(a.bench)]
    text = "\n".join(lines) + "\n"; print(text, end="")
    assert ms(fast) < ms(slow), "the in-place edit must beat the recommit measured in the same run"
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
