"""Command-line front end: render a Mitsuba XML scene on the MI355X path tracer (what `mitsuba scene.xml` does for the `path` integrator).

    python -m mitsuba-im_amd.render scene.xml [-o out.exr|out.pfm|out.npy|out.png] [-D name=value ...] [--spp N] [--sampler sobol|independent] [--device K]

The image written is the developed film (sum / weight, linear RGB, as HDRFilm::develop would hand to its writer); `.exr` (FLOAT channels, ZIP), `.pfm` and `.npy`
keep the linear values; `.png` / `.jpg` get ldrfilm's default sRGB encoding (imageio.py).  There is no CPU fallback: without the HIP library / a GPU this exits with an error.

A scene whose integrator is `multichannel` (one of path / volpath_simple / volpath plus `field` integrators) writes one OpenEXR file holding the radiance and one channel
group per field, named by the film's `channelNames` (default: `color`, then the field kinds) and shaped by its `pixelFormat` list: `<name>.R/.G/.B` for `rgb`, `<name>.Y`
for `luminance`.  Other output formats cannot hold the groups: an error that names `.exr`.
"""
import argparse
import sys
import time

import numpy as np


def write_image(path, rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    if path.endswith(".npy"):
        np.save(path, rgb)
    elif path.endswith(".pfm"):
        with open(path, "wb") as f:
            f.write(b"PF\n%d %d\n-1.0\n" % (rgb.shape[1], rgb.shape[0]))
            f.write(rgb[::-1].astype("<f4").tobytes())
    elif path.endswith(".exr"):
        from . import imageio
        imageio.write_exr(path, rgb)
    elif path.endswith((".png", ".jpg", ".jpeg")):
        from . import imageio
        imageio.write_ldr(path, rgb)
    else:
        raise SystemExit(f"unsupported output format: {path} (.exr, .pfm, .npy, .png, .jpg)")


def field_channel_groups(sc, rgb, fields, field_names):
    """(planes [h, w, n], channel names) of a multichannel render: the developed radiance, then the developed field film (api.Render.read_fields(2)), one group per nested
    integrator.  `luminance` groups: a scalar field (distance, shapeIndex, primIndex) holds three equal values and its first component is written -- the reference's
    Bitmap conversion forms the weighted sum 0.212671 R + 0.715160 G + 0.072169 B of them, which can differ from the value itself by <= 1 ulp; the radiance and the
    vector-valued fields get that weighted sum."""
    from .api import SCALAR_FIELDS
    n = 1 + len(field_names)
    names = list(sc.get("channel_names") or []) or ["color"] + list(field_names)
    formats = list(sc.get("pixel_formats") or []) or ["rgb"] * n
    if len(names) != n or len(formats) != n:
        raise ValueError(f"{n} channel groups (the radiance and {n - 1} fields) need {n} channel names and pixel formats")
    groups = [np.asarray(rgb, np.float32)] + [np.asarray(fields[..., 3 * i:3 * i + 3], np.float32) for i in range(len(field_names))]
    kinds = [None] + list(field_names); planes = []; chan = []
    for name, fmt, img, kind in zip(names, formats, groups, kinds):
        if fmt == "rgb":
            planes += [img[..., 0], img[..., 1], img[..., 2]]; chan += [name + ".R", name + ".G", name + ".B"]
        elif fmt == "luminance":
            y = img[..., 0] if kind in SCALAR_FIELDS else (img[..., 0] * np.float32(0.212671) + img[..., 1] * np.float32(0.715160)) + img[..., 2] * np.float32(0.072169)
            planes.append(y); chan.append(name + ".Y")
        else:
            raise ValueError(f"pixelFormat \"{fmt}\" is not supported with field channels (rgb, luminance)")
    return np.stack(planes, 2), chan


def main(argv=None):
    from . import xml_scene
    from .api import Scene, Render, MiError
    ap = argparse.ArgumentParser(prog="python -m mitsuba-im_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("scene")
    ap.add_argument("-o", "--output", default=None)
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="name=value")
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--sampler", choices=["sobol", "independent"], default=None, help="replace the scene's sampler plugin (keeps its sampleCount)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    params = {}
    for d in a.defines:
        if "=" not in d:
            raise SystemExit(f"-D expects name=value, got {d!r}")
        k, v = d.split("=", 1); params[k] = v
    try:
        t0 = time.perf_counter()
        sc = xml_scene.load_scene(a.scene, params, sampler=a.sampler)
        if a.spp is not None:
            sc.spp = a.spp
        t1 = time.perf_counter()
        scene = Scene(sc, device=a.device)
        render = Render(scene, device=a.device)
        t2 = time.perf_counter()
        render.run()
        rgb = render.read_film(2)
        fields = render.read_fields(2) if render.field_names else None
        t3 = time.perf_counter()
    except (xml_scene.SceneError, MiError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    out = a.output or (a.scene.rsplit(".", 1)[0] + ".exr")          # hdrfilm's default fileFormat (src/films/hdrfilm.cpp: openexr)
    if fields is not None:
        if not out.endswith(".exr"):
            print(f"error: {out}: a render with field channels holds several channel groups, which only the .exr output can store", file=sys.stderr)
            return 1
        from . import imageio
        planes, chan = field_channel_groups(sc, rgb, fields, render.field_names)
        imageio.write_exr(out, planes, chan)
    else:
        write_image(out, rgb)
    n = sc.width * sc.height * sc.spp
    print(f"{sc.name}: {sc.width}x{sc.height}, {sc.spp} spp, {len(sc.idx)} triangles; load {t1 - t0:.2f} s, upload+BVH {t2 - t1:.2f} s, "
          f"render {t3 - t2:.3f} s ({n / (t3 - t2) / 1e6:.1f} Msamples/s) -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
