"""What the a-trous denoiser costs and buys on the Cornell box (1920 x 1080, Sobol, depth 8; bench.py's C2 scene): for 1, 4 and 16 spp the render time, the time of one
Render.denoise at 5 iterations (median of 20 calls after 3 warm-ups, time.perf_counter around the synchronous call; the device-output form, and the host form with its
read-back) and the RMSE of the raw and the filtered image against a 4096-spp render of the same scene.  --sweep adds the 4-spp RMSE over a grid of widths (the values
the defaults of api.py were chosen from).  python scripts/perf_denoise.py [--ref-spp N] [--sweep] [--out FILE]; the recorded run is profiles/denoise_latency.txt"""
import argparse
import importlib
import itertools
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mi = importlib.import_module("mitsuba-im_amd")
from scripts.perf_live_edit import device_name  # noqa: E402

GUIDES = [("shNormal", 0.0), ("position", 0.0), "albedo"]


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def timed(fn, warm=3, calls=20):
    for _ in range(warm): fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--ref-spp", type=int, default=4096); ap.add_argument("--sweep", action="store_true"); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    S = mi.scenes; W, H = 1920, 1080
    dev = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")      # torch opens the device before the library does (as in bench.py)
    sc = S.cornell_box(W, H, 16, max_depth=8); gs = mi.Scene(sc)
    ref_r = mi.Render(gs, spp=a.ref_spp); t0 = time.perf_counter(); ref_r.run(); t_ref = time.perf_counter() - t0; ref = ref_r.read_film(2); ref_r.close()
    lines = [f"machine: {device_name()}", f"scene: Cornell box {W}x{H}, Sobol, maxDepth 8, fields shNormal + position + albedo; reference: {a.ref_spp} spp ({t_ref:.2f} s)",
             f"filter: {mi.api.DENOISE_DEFAULTS}", "spp | render ms | denoise ms, device output (median of 20, min) | denoise ms, host output | RMSE raw | RMSE filtered | ratio"]
    for spp in (1, 4, 16):
        r = mi.Render(gs, spp=spp, fields=GUIDES); r.run(); r.clear(); r.run(); t_render = r.stats()["render_ms"]
        raw = r.read_film(2); out = r.denoise()
        d_med, d_min = timed(lambda: r.denoise(device_ptr=dev.data_ptr())); h_med, _ = timed(lambda: r.denoise())
        e_raw, e_out = rmse(raw, ref), rmse(out, ref)
        lines.append(f"{spp:3d} | {t_render:9.2f} | {d_med:.3f} ({d_min:.3f}) | {h_med:.3f} | {e_raw:.5f} | {e_out:.5f} | {e_out / e_raw:.3f}   (resolved sigma_position {r.last_denoise_sigma_position:.3f})")
        if spp == 4 and a.sweep:
            lines.append("4 spp, RMSE filtered over iterations x sigma_color x sigma_normal x sigma_position:")
            for it, c, n, p in itertools.product((4, 5, 6), (0.5, 1.0, 2.0, 4.0, 8.0), (0.1, 0.3, 0.6), (-0.02, -0.05, -0.1)):
                lines.append(f"  K {it} colour {c:g} normal {n:g} position {p:g}: {rmse(r.denoise(iterations=it, sigma_color=c, sigma_normal=n, sigma_position=p), ref):.5f}")
        r.close()
    text = "\n".join(lines) + "\n"; print(text, end="")
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
