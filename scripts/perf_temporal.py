"""What the denoiser's temporal stage costs on the Cornell box (1920 x 1080, Sobol, depth 8, 4 spp; bench.py's C2 scene): the time of one Render.denoise_temporal
against one Render.denoise, both with device output and 5 iterations, in the same process (median of 20 synchronous calls after 3 warm-ups, time.perf_counter around
the call).  Between the temporal calls the camera alternates between two views 1 degree apart, so every call reprojects by a fraction of a pixel and gathers all
four taps (a static camera would find three of the four weights zero and skip their loads); the film is not rendered again, the work of the stage does not depend on
it.  --flicker adds the flicker measure of a 24-frame 1-spp orbit at 256 x 144 with and without the history: the mean absolute difference between consecutive
output frames, the earlier one looked up where the later frame's surface points fall under its projection (reproject below), over the pixels whose
reprojected position agrees within 1 % of the scene's diagonal.  python scripts/perf_temporal.py [--flicker] [--out FILE]; the recorded run is
profiles/temporal_latency.txt"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mi = importlib.import_module("mitsuba-im_amd")
render = importlib.import_module("mitsuba-im_amd.render")
from scripts.perf_live_edit import device_name  # noqa: E402

GUIDES = [("shNormal", 0.0), ("position", 0.0), "albedo"]


def timed(fn, before=None, warm=3, calls=20):
    t = []
    for i in range(warm + calls):
        if before: before(i)
        t0 = time.perf_counter(); fn(); dt = (time.perf_counter() - t0) * 1e3
        if i >= warm: t.append(dt)
    return statistics.median(t), min(t)


def reproject(prev_image, M_prev, Q, fill=np.nan):
    """`prev_image` (H x W x 3) looked up bilinearly where the points Q (H x W x 3, world) fall under the previous frame's projection, as the temporal stage's rules 3.1 - 3.4 do, without the
    history tests and in float64 (a measuring tool); pixels that fall outside get `fill`."""
    H, W = prev_image.shape[:2]; M = np.asarray(M_prev, np.float64).reshape(3, 4); Qh = np.concatenate([np.asarray(Q, np.float64), np.ones((H, W, 1))], -1)
    with np.errstate(all="ignore"):
        X, Y, Wc = (Qh @ M[r] for r in range(3)); fx, fy = X / Wc - 0.5, Y / Wc - 0.5
        ok = (Wc > 0) & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
    x0 = np.minimum(np.floor(fx).astype(int), W - 2) if W > 1 else np.zeros_like(fx, int); y0 = np.minimum(np.floor(fy).astype(int), H - 2) if H > 1 else np.zeros_like(fy, int)
    tx, ty = (fx - x0)[..., None], (fy - y0)[..., None]; x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1); p = np.asarray(prev_image, np.float64)
    v = (p[y0, x0] * (1 - tx) + p[y0, x1] * tx) * (1 - ty) + (p[y1, x0] * (1 - tx) + p[y1, x1] * tx) * ty
    return np.where(ok[..., None], v, fill)


def flicker(outs, Ms, Ps):
    d = []
    for k in range(1, len(outs)):
        prev = reproject(outs[k - 1], Ms[k - 1], Ps[k]); prevP = reproject(Ps[k - 1], Ms[k - 1], Ps[k])
        box = Ps[k].reshape(-1, 3); tol = 0.01 * float(np.linalg.norm(box.max(0) - box.min(0)))
        ok = np.isfinite(prev).all(-1) & (np.linalg.norm(prevP - Ps[k], axis=-1) <= tol)
        d.append(float(np.abs(prev[ok] - outs[k][ok]).mean()))
    return float(np.mean(d))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--flicker", action="store_true"); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    S = mi.scenes; W, H = 1920, 1080
    dev = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")      # torch opens the device before the library does (as in bench.py)
    sc = S.cornell_box(W, H, 4, max_depth=8); gs = mi.Scene(sc); r = mi.Render(gs, fields=GUIDES); r.run()
    cams = render.orbit_cameras(sc, 360)[:2]; hist = mi.History(W, H)
    d_med, d_min = timed(lambda: r.denoise(device_ptr=dev.data_ptr()))
    t_med, t_min = timed(lambda: r.denoise_temporal(hist, device_ptr=dev.data_ptr()), before=lambda i: gs.update_camera(sc.sample_to_camera, cams[i & 1], sc.near, sc.far))
    _, cnt = hist.read()
    z_med, z_min = timed(lambda: r.denoise_temporal(hist, iterations=0, device_ptr=dev.data_ptr()), before=lambda i: gs.update_camera(sc.sample_to_camera, cams[i & 1], sc.near, sc.far))
    lines = [f"machine: {device_name()}", f"scene: Cornell box {W}x{H}, Sobol, maxDepth 8, 4 spp, fields shNormal + position + albedo",
             f"filter: {mi.api.DENOISE_DEFAULTS}; temporal: {mi.api.TEMPORAL_DEFAULTS}",
             "ms per synchronous call, device output: median of 20 (min)",
             f"denoise                          {d_med:.3f} ({d_min:.3f})",
             f"denoise_temporal                 {t_med:.3f} ({t_min:.3f})   addition {t_med - d_med:+.3f}   (pixels with history after the timed calls: {float((cnt > 1).mean()):.3f}, tolerance {r.last_temporal_sigma_position:.3f})",
             f"denoise_temporal, 0 iterations   {z_med:.3f} ({z_min:.3f})   (prepare + box reduction + accumulate + output, no filter level)"]
    r.close(); hist.close()
    if a.flicker:
        w, h, n = 256, 144, 24
        sc = S.cornell_box(w, h, n, max_depth=8); gs = mi.Scene(sc)      # spp = n: frame f renders sample index f alone
        r = mi.Render(gs, fields=GUIDES); hist = mi.History(w, h); plain, temporal, Ms, Ps = [], [], [], []
        for f, cam in enumerate(render.orbit_cameras(sc, n)):
            gs.update_camera(sc.sample_to_camera, cam, sc.near, sc.far); r.clear(); r.run(s0=f, s1=f + 1)
            plain.append(r.denoise()); temporal.append(r.denoise_temporal(hist)); Ms.append(gs.world_to_pixel()); Ps.append(r.read_fields(2)[..., 3:6])
        lines.append(f"flicker, {n}-frame 1-spp orbit at {w}x{h} (mean |frame k - frame k-1 reprojected|): denoise {flicker(plain, Ms, Ps):.5f}, denoise_temporal {flicker(temporal, Ms, Ps):.5f}")
    text = "\n".join(lines) + "\n"; print(text, end="")
    if a.out:
        with open(a.out, "w") as f: f.write(text)


if __name__ == "__main__":
    main()
