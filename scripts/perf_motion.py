"""What the prevPosition / motion field channels and the frame mark cost on instanced_garden at 1920 x 1080 (4 spp, Sobol): the device time of a run (mi_stats.render_ms,
HIP events) without fields, with `position`, and with `position` + `prevPosition` + `motion` -- median of 9 runs after 2 warm-ups, the field stage's share being the
difference to the run without fields -- and the time of one Scene.mark_frame() (median of 20, time.perf_counter around the synchronous call) before any vertex edit
(the vertices go up from the host) and after one (the device copies its own array).  On a tree without the two kinds the third row is skipped, so the same script
measures the parent.  python scripts/perf_motion.py [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mi = importlib.import_module("mitsuba-im_amd")


def run_ms(gs, fields, warm=2, calls=9):
    r = mi.Render(gs, fields=fields); t = []
    for i in range(warm + calls):
        r.clear(); r.run()
        if i >= warm: t.append(r.stats()["render_ms"])
    r.close(); return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--out", default=None); a = ap.parse_args()
    S = mi.scenes; sc = S.instanced_garden(1920, 1080, 4); gs = mi.Scene(sc)
    lines = [f"scene: instanced_garden 1920x1080, 4 spp, {len(sc.idx)} triangles, {len(sc.pos)} vertices, {len(sc.instances)} instances", "fields | run ms (median of 9, min) | minus the run without fields"]
    base = None
    for fields in ([], ["position"], ["position", "prevPosition", "motion"]):
        try:
            med, lo = run_ms(gs, fields)
        except ValueError as e:
            lines.append(f"{'+'.join(fields)} | not in this tree ({e})"); continue
        base = med if base is None else base
        lines.append(f"{'+'.join(fields) or 'none'} | {med:.3f} ({lo:.3f}) | {med - base:.3f}")
    if hasattr(gs, "mark_frame"):
        def timed(n=20):
            t = []
            for _ in range(n):
                t0 = time.perf_counter(); gs.mark_frame(); t.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(t), min(t)
        gs.mark_frame(); h2d = timed()
        gs.update_geometry(sc.pos, sc.nrm); d2d = timed()
        lines.append(f"mark_frame ms (median of 20, min): vertices from the host {h2d[0]:.3f} ({h2d[1]:.3f}); from the device's own array, after a vertex edit {d2d[0]:.3f} ({d2d[1]:.3f})")
    text = "\n".join(lines) + "\n"; print(text, end="")
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
