"""Command-line front end: render a Mitsuba XML scene on the MI355X path tracer (what `mitsuba scene.xml` does for the `path` integrator).

    python -m mitsuba-im_amd.render scene.xml [-o out.exr|out.pfm|out.npy|out.png] [-D name=value ...] [--spp N] [--sampler sobol|independent] [--device K] [--ao N [--ao-length L]]
                                    [--denoise [ITERATIONS] [--denoise-sigma C N P] [--denoise-raw PATH] [--denoise-temporal [MAX_HISTORY]]]

The image written is the developed film (sum / weight, linear RGB, as HDRFilm::develop would hand to its writer); `.exr` (FLOAT channels, ZIP), `.pfm` and `.npy`
keep the linear values; `.png` / `.jpg` get ldrfilm's default sRGB encoding (imageio.py).  There is no CPU fallback: without the HIP library / a GPU this exits with an error.

A scene whose integrator is `multichannel` (one of path / volpath_simple / volpath plus `field` integrators) writes one OpenEXR file holding the radiance and one channel
group per field, named by the film's `channelNames` (default: `color`, then the field kinds) and shaped by its `pixelFormat` list: `<name>.R/.G/.B` for `rgb`, `<name>.Y`
for `luminance`.  Other output formats cannot hold the groups: an error that names `.exr`.

`--ao N [--ao-length L]` renders any scene file with the ambient-occlusion integrator (`ao`: N shading samples, occlusion rays of length L, default automatic) in
place of the file's own integrator; the field channels of a `multichannel` scene stay.  A scene file whose integrator is `ao` needs no option.

`--adaptive [MAXERROR] [--max-sample-factor N]` wraps the file's `path` / `volpath_simple` / `volpath` integrator in per-pixel error control (the reference's `adaptive`
integrator: every pixel takes samples until the half width of its confidence interval is at most MAXERROR x its mean luminance, default 0.05, or N x spp samples are
spent, default 32); a scene file whose integrator is `adaptive` needs no option.  The independent sampler and a sample count of at least 8 are required.
`--sample-counts out.npy` writes the H x W map of samples per pixel (`out_000.npy`, ... for frames).  Both work with `--orbit`, `--spin` and `--focus-pull`: clear, edit,
adaptive run per frame.

`--denoise [ITERATIONS]` filters the radiance on the device before it is written: the edge-avoiding a-trous filter (api.Render.denoise; ITERATIONS levels, default 5)
guided by the render's own `shNormal` and `position` field channels and demodulated by its `albedo` channel.  The option adds the three fields (undefined 0 0 0) to
the render's field list unless the scene file's `multichannel` integrator already asks for them; the ones it added are not written, the scene file's own are written
as before.  On a scene whose BSDFs have no albedo field (plastic, roughplastic, coatings, a mask over a bumpmap / normalmap) it filters without demodulation and says
so.  `--denoise-sigma C N P` sets the colour, normal and position widths (P < 0: that fraction of the scene's extent); `--denoise-raw PATH` also writes the
unfiltered radiance (`PATH_000.ext`, ... for frames).  Works with `--orbit`, `--spin` and `--focus-pull`: one filter call per frame on the same render.  Not with
adaptive sampling, whose film has no field channels.

`--denoise-temporal [MAX_HISTORY]` (with `--denoise`, on `--orbit`, `--spin` and `--focus-pull` sequences of at least two frames) puts the temporal stage in front of
the filter levels: one history (api.History) serves all frames, every frame's accumulated colour is reprojected into the next through the camera of the edited scene
and blended with it (api.Render.denoise_temporal; a pixel keeps at most MAX_HISTORY frames, default 32).  Every frame marks the scene before its edit (Scene.mark_frame) and the
render carries a `prevPosition` field next to `position` (added like the other guides, not written): the instances a `--spin` moves are reprojected from where they
were in the previous frame and keep their history.  Not with adaptive sampling.  It implies `--sample-offset-per-frame`: frame
f renders the sample indices [f spp, (f + 1) spp) after its clear, so that frames carry independent noise.  The render is then created for frames x spp samples per
pixel, of which every frame takes its own slice (a run stays within the render's sample count; the Sobol' sampler's index layout and the scale of the ray
differentials follow that count).  Without the flag every frame renders the indices [0, spp) and the files are what they were.

`--orbit N [--orbit-axis x|y|z]` renders a turntable: N frames with the camera rotated in steps of 360 / N degrees about the axis through the centre of the scene's
box.  The scene is committed once; every frame is a frame mark (Scene.mark_frame: the state the prevPosition / motion fields call "previous"), an in-place camera edit of the committed scene
(Scene.update_camera), a clear and a run -- no tree build, no
upload -- and is written to `<output>_000.<ext>`, `<output>_001.<ext>`, ...

`--spin N [--spin-axis x|y|z]` renders N frames in which every instance of a shape group is turned by 360 k / N degrees (frame k) about the axis through its own placed
origin.  One commit again; every frame is an in-place instance edit (Scene.update_instances: the instance records and a refit of the scene-level tree on the device),
a clear and a run, written like the orbit's frames.  A scene without instances ends with a message.

`--focus-pull N --focus-from A --focus-to B` renders N frames of a `thinlens` scene with the focus distance going from A to B in equal steps (either end defaults to
the scene's own focusDistance; the aperture stays).  One commit; every frame is an in-place lens edit (Scene.update_lens: two scalars), a clear and a run, written
like the orbit's frames.  With `--orbit N` (the same N) every frame takes its camera and its focus distance.  A scene without a thinlens sensor ends with a message.
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


def orbit_cameras(sc, n, axis="y"):
    """The n camera-to-world matrices of a turntable: frame f is the scene's camera rotated by 360 f / n degrees about `axis` through the centre of the scene's box
    (the box of the mesh vertices and of the analytic shapes' origins).  Frame 0 is the scene's own camera, bit for bit."""
    pts = [np.asarray(sc.pos, np.float64).reshape(-1, 3)] + [np.asarray(a["to_world"], np.float64)[:3, 3].reshape(1, 3) for a in (sc.get("analytic") or [])]
    pts = np.concatenate(pts); centre = (pts.min(0) + pts.max(0)) * 0.5
    k = "xyz".index(axis); i, j = (k + 1) % 3, (k + 2) % 3
    c2w = np.asarray(sc.cam_to_world, np.float64); out = [np.ascontiguousarray(sc.cam_to_world, np.float32)]
    for f in range(1, n):
        t = 2.0 * np.pi * f / n; rot = np.eye(4); rot[i, i] = rot[j, j] = np.cos(t); rot[i, j] = -np.sin(t); rot[j, i] = np.sin(t)
        to_c = np.eye(4); to_c[:3, 3] = -centre; back = np.eye(4); back[:3, 3] = centre
        out.append(np.ascontiguousarray(back @ rot @ to_c @ c2w, np.float32))
    return out


def spin_instances(sc, n, axis="y"):
    """The n instance lists of a spin: in frame f every instance is turned by 360 f / n degrees about `axis` through its own placed origin, to_world (0, 0, 0, 1).
    Frame 0 holds the scene's own records."""
    from .scenes import make_instance
    k = "xyz".index(axis); i, j = (k + 1) % 3, (k + 2) % 3; out = [list(sc.instances)]
    for f in range(1, n):
        t = 2.0 * np.pi * f / n; rot = np.eye(4); rot[i, i] = rot[j, j] = np.cos(t); rot[i, j] = -np.sin(t); rot[j, i] = np.sin(t)
        frame = []
        for inst in sc.instances:
            tw = np.asarray(inst["to_world"], np.float64); to_o = np.eye(4); to_o[:3, 3] = -tw[:3, 3]; back = np.eye(4); back[:3, 3] = tw[:3, 3]
            frame.append(make_instance(inst["group"], back @ rot @ to_o @ tw))
        out.append(frame)
    return out


def focus_distances(n, a, b):
    """The n focus distances of a pull from a to b: equal steps, frame 0 = a exactly, frame n - 1 = b exactly."""
    return [float(a)] if n == 1 else [float(a) if f == 0 else float(b) if f == n - 1 else float(a + (b - a) * f / (n - 1)) for f in range(n)]


def use_ao(sc, shading_samples, ray_length=-1.0):
    """`--ao N [--ao-length L]`: the scene description with the ambient-occlusion integrator in place of its own (its field list, sampler and film stay)."""
    from .scenes import INTEGRATOR_AO
    if shading_samples < 1:
        raise ValueError("--ao expects a number of shading samples >= 1")
    sc.integrator = INTEGRATOR_AO; sc.shading_samples = int(shading_samples); sc.ray_length = float(ray_length)
    return sc


def use_adaptive(sc, max_error=0.05, max_sample_factor=None):
    """`--adaptive [MAXERROR] [--max-sample-factor N]`: the scene description with per-pixel error control around its path / volpath_simple / volpath integrator.  A scene
    file that holds an `adaptive` integrator keeps its own pValue (and whatever of the two is not given here)."""
    from .scenes import INTEGRATOR_DIRECT, INTEGRATOR_AO
    if (sc.get("integrator", 0) or 0) in (INTEGRATOR_DIRECT, INTEGRATOR_AO):
        raise ValueError("--adaptive wraps a path, volpath_simple or volpath integrator; direct and ao are not supported underneath")
    if sc.get("fields"):
        raise ValueError("--adaptive cannot be combined with the field channels of a multichannel scene")
    if max_error is not None and not max_error >= 0:
        raise ValueError("--adaptive expects a maximum relative error >= 0")
    if max_sample_factor is not None and max_sample_factor == 0:
        raise ValueError("--max-sample-factor must not be 0 (negative: no limit)")
    ad = dict(sc.get("adaptive") or dict(max_error=0.05, p_value=0.05, max_sample_factor=32))
    if max_error is not None: ad["max_error"] = float(max_error)
    if max_sample_factor is not None: ad["max_sample_factor"] = int(max_sample_factor)
    sc.adaptive = ad
    return sc


def use_denoise(sc, render, iterations=5, sigmas=None, raw=None, temporal=None, device=0):
    """`--denoise`: puts the guides the filter needs behind the scene's own field list (what the scene file asks for stays in front and is reused) and returns what
    `developed` needs: the filter's arguments, the count of the scene's own fields and the path of the unfiltered image."""
    from .api import normalize_fields, MiError, DENOISE_DEFAULTS
    own = normalize_fields(sc.get("fields") or []); names = [n for n, _ in own]
    guides = own + [(g, 0.0) for g in ("shNormal", "position") if g not in names]
    if temporal is not None and "position" not in names and "prevPosition" not in names:      # the temporal stage's previous positions: the frames mark the scene before their edits
        guides.append(("prevPosition", 0.0))
    widths = dict(DENOISE_DEFAULTS, iterations=int(iterations))
    if sigmas is not None: widths.update(sigma_color=float(sigmas[0]), sigma_normal=float(sigmas[1]), sigma_position=float(sigmas[2]))
    try:
        render.set_fields(guides + ([] if "albedo" in names else [("albedo", 0.0)]))
    except MiError as e:
        if e.code != 3 or "albedo" in names: raise
        print(f"{sc.name}: {e}; --denoise filters without albedo demodulation", file=sys.stderr)
        render.set_fields(guides)
    dn = dict(widths=widths, own=len(own), raw=raw)
    if temporal is not None:      # `--denoise-temporal`: one history for all frames
        from .api import History
        dn["history"] = History(sc.width, sc.height, device=device); dn["max_history"] = float(temporal)
    return dn


def developed(render, dn=None):
    """(radiance, fields or None, field names, unfiltered radiance or None) of the film as it stands; `dn` (use_denoise): the radiance filtered on the device, and
    only the scene's own fields"""
    rgb = render.read_film(2); names = list(render.field_names); fields = render.read_fields(2) if names else None
    if dn is None:
        return rgb, fields, names, None
    own = dn["own"]
    out = render.denoise_temporal(dn["history"], max_history=dn["max_history"], **dn["widths"]) if dn.get("history") is not None else render.denoise(**dn["widths"])
    return out, (fields[..., :3 * own] if own else None), names[:own], rgb


def write_outputs(sc, render, out, dev=None, dn=None, frame=None):
    """the developed film (and, for a multichannel scene, the field groups) of `render` -> `out`; False (message printed) when the format cannot hold them"""
    rgb, fields, names, raw = developed(render, dn) if dev is None else dev
    if raw is not None and dn["raw"]:
        stem, ext = dn["raw"].rsplit(".", 1)
        write_image(dn["raw"] if frame is None else f"{stem}_{frame:03d}.{ext}", raw)
    if fields is not None:
        if not out.endswith(".exr"):
            print(f"error: {out}: a render with field channels holds several channel groups, which only the .exr output can store", file=sys.stderr)
            return False
        from . import imageio
        planes, chan = field_channel_groups(sc, rgb, fields, names)
        imageio.write_exr(out, planes, chan)
    else:
        write_image(out, rgb)
    return True


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
    ap.add_argument("--ao", type=int, default=0, metavar="N", help="render with the ambient-occlusion integrator (N shading samples) in place of the scene's own integrator")
    ap.add_argument("--ao-length", type=float, default=None, metavar="L", help="length of the occlusion rays of --ao (default: automatic, half the radius of the scene's bounding sphere)")
    ap.add_argument("--adaptive", type=float, nargs="?", const=0.05, default=None, metavar="MAXERROR", help="per-pixel error control around the scene's path / volpath integrator (maximum relative error, default 0.05)")
    ap.add_argument("--max-sample-factor", type=int, default=None, metavar="N", help="with adaptive sampling: at most N x spp samples per pixel (negative: no limit; default 32)")
    ap.add_argument("--sample-counts", default=None, metavar="out.npy", help="with adaptive sampling: write the H x W map of samples per pixel")
    ap.add_argument("--denoise", type=int, nargs="?", const=5, default=None, metavar="ITERATIONS", help="filter the radiance on the device with the edge-avoiding a-trous filter, guided by the shNormal / position / albedo field channels (levels, default 5)")
    ap.add_argument("--denoise-sigma", type=float, nargs=3, default=None, metavar=("C", "N", "P"), help="with --denoise: colour, normal and position widths (P < 0: that fraction of the scene's extent)")
    ap.add_argument("--denoise-raw", default=None, metavar="PATH", help="with --denoise: also write the unfiltered radiance")
    ap.add_argument("--denoise-temporal", type=float, nargs="?", const=32.0, default=None, metavar="MAX_HISTORY", help="with --denoise on a frame sequence: reproject and accumulate the previous frames in front of the filter, moved instances from where they were (frames kept per pixel at the most, default 32); implies --sample-offset-per-frame")
    ap.add_argument("--sample-offset-per-frame", action="store_true", help="frame f of a sequence renders the sample indices [f spp, (f + 1) spp): independent noise per frame")
    ap.add_argument("--orbit", type=int, default=0, metavar="N", help="turntable of N frames about the scene box's centre: one commit, one in-place camera edit per frame")
    ap.add_argument("--orbit-axis", choices=["x", "y", "z"], default="y")
    ap.add_argument("--spin", type=int, default=0, metavar="N", help="N frames with every instance turned about its own origin: one commit, one in-place instance edit per frame")
    ap.add_argument("--spin-axis", choices=["x", "y", "z"], default="y")
    ap.add_argument("--focus-pull", type=int, default=0, metavar="N", help="N frames of a thinlens scene with the focus distance going from --focus-from to --focus-to: one commit, one in-place lens edit per frame")
    ap.add_argument("--focus-from", type=float, default=None, metavar="A")
    ap.add_argument("--focus-to", type=float, default=None, metavar="B")
    a = ap.parse_args(argv)
    params = {}
    for d in a.defines:
        if "=" not in d:
            raise SystemExit(f"-D expects name=value, got {d!r}")
        k, v = d.split("=", 1); params[k] = v
    if a.ao < 0 or (a.ao_length is not None and not a.ao):
        raise SystemExit("--ao expects a number of shading samples >= 1; --ao-length belongs to --ao N")
    if a.sample_counts is not None and not a.sample_counts.endswith(".npy"):
        raise SystemExit("--sample-counts expects a .npy file name")
    if a.adaptive is not None and a.ao:
        raise SystemExit("--adaptive cannot be combined with --ao (adaptive sampling runs over path, volpath_simple or volpath)")
    if a.denoise is None and (a.denoise_sigma is not None or a.denoise_raw is not None):
        raise SystemExit("--denoise-sigma / --denoise-raw belong to --denoise")
    if a.denoise is not None and not 0 <= a.denoise <= 8:
        raise SystemExit("--denoise expects 0 to 8 iterations")
    if a.orbit < 0:
        raise SystemExit("--orbit expects a frame count >= 1")
    if a.spin < 0 or (a.spin and a.orbit):
        raise SystemExit("--spin expects a frame count >= 1 and cannot be combined with --orbit")
    if a.focus_pull < 0 or (a.focus_pull and a.spin) or (a.focus_pull and a.orbit and a.orbit != a.focus_pull):
        raise SystemExit("--focus-pull expects a frame count >= 1, cannot be combined with --spin, and with --orbit both take the same frame count")
    if not a.focus_pull and (a.focus_from is not None or a.focus_to is not None):
        raise SystemExit("--focus-from / --focus-to belong to --focus-pull N")
    try:
        t0 = time.perf_counter()
        sc = xml_scene.load_scene(a.scene, params, sampler=a.sampler)
        if a.spp is not None:
            sc.spp = a.spp
        if a.ao:
            use_ao(sc, a.ao, -1.0 if a.ao_length is None else a.ao_length)
        if a.adaptive is not None or (a.max_sample_factor is not None and sc.get("adaptive")):
            try:
                use_adaptive(sc, a.adaptive, a.max_sample_factor)
            except ValueError as e:
                print(f"error: {e}", file=sys.stderr)
                return 1
        elif a.max_sample_factor is not None:
            print("error: --max-sample-factor belongs to --adaptive (or to a scene file with an adaptive integrator)", file=sys.stderr)
            return 1
        if a.sample_counts is not None and not sc.get("adaptive"):
            print("error: --sample-counts needs adaptive sampling (--adaptive, or a scene file with an adaptive integrator)", file=sys.stderr)
            return 1
        if a.denoise is not None and sc.get("adaptive"):
            print("error: --denoise cannot be combined with adaptive sampling (--adaptive, or a scene file with an adaptive integrator): an adaptive film has no field channels", file=sys.stderr)
            return 1
        n_frames = a.focus_pull or a.orbit or a.spin
        if a.denoise_temporal is not None:
            if a.denoise is None:
                print("error: --denoise-temporal belongs to --denoise", file=sys.stderr)
                return 1
            if n_frames < 2:
                print("error: --denoise-temporal needs a frame sequence (--orbit, --spin or --focus-pull with at least two frames): a single frame has no history", file=sys.stderr)
                return 1
            if not a.denoise_temporal >= 1:
                print("error: --denoise-temporal expects a history length >= 1", file=sys.stderr)
                return 1
        offset_frames = a.sample_offset_per_frame or a.denoise_temporal is not None
        if offset_frames and sc.get("adaptive"):
            print("error: --denoise-temporal / --sample-offset-per-frame cannot be combined with adaptive sampling (--adaptive, or a scene file with an adaptive integrator): an adaptive run chooses its own sample indices", file=sys.stderr)
            return 1
        out = a.output or (a.scene.rsplit(".", 1)[0] + ".exr")          # hdrfilm's default fileFormat (src/films/hdrfilm.cpp: openexr)
        if a.spin and not (sc.get("instances") or []):
            print(f"error: {a.scene}: --spin turns the instances of shape groups, and this scene has none", file=sys.stderr)
            return 1
        if a.focus_pull:
            if not float(sc.get("aperture_radius", 0.0) or 0.0):
                print(f"error: {a.scene}: --focus-pull moves the focal plane of a thinlens sensor, and this scene's sensor has no lens", file=sys.stderr)
                return 1
            pull = focus_distances(a.focus_pull, sc.focus_distance if a.focus_from is None else a.focus_from, sc.focus_distance if a.focus_to is None else a.focus_to)
            if not all(np.isfinite(d) and d > 0 for d in pull):
                print("error: --focus-from / --focus-to expect positive distances", file=sys.stderr)
                return 1
        t1 = time.perf_counter()
        scene = Scene(sc, device=a.device)
        render = Render(scene, device=a.device, spp=sc.spp * n_frames if offset_frames and n_frames else None)
        dn = use_denoise(sc, render, a.denoise, a.denoise_sigma, a.denoise_raw, a.denoise_temporal, a.device) if a.denoise is not None else None
        t2 = time.perf_counter()
        frame_no = [0]

        def go(f=0):      # frame f into the clear film: the adaptive run of a scene with adaptive parameters (api.Render picked them up), else every pixel's spp samples
            if not sc.get("adaptive"):
                return render.run(s0=f * sc.spp, s1=(f + 1) * sc.spp) if offset_frames else render.run()
            render.run_adaptive()
            if a.sample_counts is not None:
                frames = a.orbit or a.spin or a.focus_pull
                np.save(a.sample_counts[:-4] + f"_{frame_no[0]:03d}.npy" if frames else a.sample_counts, render.sample_counts())
            frame_no[0] += 1
        n = sc.width * sc.height * sc.spp
        if a.focus_pull:
            stem, ext = out.rsplit(".", 1); frame_s = []
            cams = orbit_cameras(sc, a.orbit, a.orbit_axis) if a.orbit else [None] * a.focus_pull
            for f, (dist, c2w) in enumerate(zip(pull, cams)):
                tf = time.perf_counter(); scene.mark_frame()
                if c2w is not None: scene.update_camera(sc.sample_to_camera, c2w, sc.near, sc.far)
                scene.update_lens(sc.aperture_radius, dist); render.clear(); go(f)
                frame_s.append(time.perf_counter() - tf)
                if not write_outputs(sc, render, f"{stem}_{f:03d}.{ext}", dn=dn, frame=f):
                    return 1
            rev, builds = scene.revision(); mean = sum(frame_s) / len(frame_s)
            print(f"{sc.name}: {sc.width}x{sc.height}, {sc.spp} spp, {len(sc.idx)} triangles; load {t1 - t0:.2f} s, upload+BVH {t2 - t1:.2f} s once ({builds} tree build, {rev} edits), "
                  f"{a.focus_pull} frames, focus {pull[0]:g} .. {pull[-1]:g}, render {mean:.3f} s per frame ({n / mean / 1e6:.1f} Msamples/s) -> {stem}_000.{ext} .. {stem}_{a.focus_pull - 1:03d}.{ext}")
            return 0
        if a.orbit:
            stem, ext = out.rsplit(".", 1); frame_s = []
            for f, c2w in enumerate(orbit_cameras(sc, a.orbit, a.orbit_axis)):
                tf = time.perf_counter(); scene.mark_frame()
                scene.update_camera(sc.sample_to_camera, c2w, sc.near, sc.far); render.clear(); go(f)
                frame_s.append(time.perf_counter() - tf)
                if not write_outputs(sc, render, f"{stem}_{f:03d}.{ext}", dn=dn, frame=f):
                    return 1
            rev, builds = scene.revision(); mean = sum(frame_s) / len(frame_s)
            print(f"{sc.name}: {sc.width}x{sc.height}, {sc.spp} spp, {len(sc.idx)} triangles; load {t1 - t0:.2f} s, upload+BVH {t2 - t1:.2f} s once ({builds} tree build, {rev} camera edits), "
                  f"{a.orbit} frames, render {mean:.3f} s per frame ({n / mean / 1e6:.1f} Msamples/s) -> {stem}_000.{ext} .. {stem}_{a.orbit - 1:03d}.{ext}")
            return 0
        if a.spin:
            stem, ext = out.rsplit(".", 1); frame_s = []
            for f, insts in enumerate(spin_instances(sc, a.spin, a.spin_axis)):
                tf = time.perf_counter(); scene.mark_frame()
                scene.update_instances(insts); render.clear(); go(f)
                frame_s.append(time.perf_counter() - tf)
                if not write_outputs(sc, render, f"{stem}_{f:03d}.{ext}", dn=dn, frame=f):
                    return 1
            rev, builds = scene.revision(); mean = sum(frame_s) / len(frame_s)
            print(f"{sc.name}: {sc.width}x{sc.height}, {sc.spp} spp, {len(sc.idx)} triangles, {len(insts)} instances; load {t1 - t0:.2f} s, upload+BVH {t2 - t1:.2f} s once ({builds} tree build, {rev} instance edits), "
                  f"{a.spin} frames, render {mean:.3f} s per frame ({n / mean / 1e6:.1f} Msamples/s) -> {stem}_000.{ext} .. {stem}_{a.spin - 1:03d}.{ext}")
            return 0
        go()
        dev = developed(render, dn)
        t3 = time.perf_counter()
    except (xml_scene.SceneError, MiError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    if not write_outputs(sc, render, out, dev, dn):
        return 1
    spp_text = f"{sc.spp} spp"
    if sc.get("adaptive"):      # the samples the adaptive run traced, and what it kept
        st = render.adaptive_stats(); n = st["samples_traced"]
        spp_text = f"adaptive from {sc.spp} spp ({st['min_count']} .. {st['max_count']} per pixel, mean {st['samples_used'] / (sc.width * sc.height):.1f}, {st['rounds']} rounds)"
    print(f"{sc.name}: {sc.width}x{sc.height}, {spp_text}, {len(sc.idx)} triangles; load {t1 - t0:.2f} s, upload+BVH {t2 - t1:.2f} s, "
          f"render {t3 - t2:.3f} s ({n / (t3 - t2) / 1e6:.1f} Msamples/s) -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
