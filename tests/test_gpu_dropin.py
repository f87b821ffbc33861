"""GPU: the drop-in boundary end to end.  The adapter plugin (mitsuba-im_amd/csrc/adapter/path_hip.cpp, built against the reference's
headers) is loaded by the REFERENCE's own PluginManager inside oracle/_ref/harness and driven through the reference's responsive interface
(preprocess -> allocate -> render(..., Controls, threadIdx, threadCount)) exactly like `path`; its target ImageBlock must match the one the
reference's `path` plugin produced through the same driver (fixture tests/golden/cornell_small_responsive.npz)."""
import os
import subprocess
import numpy as np
import pytest
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(ROOT, "oracle", "_ref", "harness")
PLUGIN = os.path.join(ROOT, "oracle", "_ref", "plugins", "path_hip.so")
# path_hip.so links libmi355pt.so: the harness runs against THIS tree's library, wherever the plugin was linked (the loader searches
# LD_LIBRARY_PATH before the plugin's own run path)
HARNESS_ENV = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(p for p in (os.path.join(ROOT, "mitsuba-im_amd"), os.environ.get("LD_LIBRARY_PATH")) if p))


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
def test_plugin_drop_in_through_reference_driver(mi, golden_scenes, tmp_path):
    sc = golden_scenes["cornell_small"]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path)
    out = str(tmp_path / "hip")
    subprocess.run([HARNESS, path, "responsive", "path_hip", "-1", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    got = np.load(out + "_target.npy"); meta = np.load(out + "_meta.npy")
    ref = np.load(os.path.join(GOLDEN, "cornell_small_responsive.npz"))["target"]
    assert meta[0] == 0                                   # return code 0 = all sample planes done (integrator.cpp:349-401)
    assert meta[2] == 2 and list(meta[3:5]) == [0.0, 8.0]   # one progress() per PAIR of 4-plane batches (the pair keeps both path pools / streams busy), first call at the start of plane 0
    assert got.shape == ref.shape == (sc.height + 2, sc.width + 2, 4)
    # interior without the last row/column: the reference's ImageOrderIntegrator also enumerates the bitmap's BORDER cells as pixels
    # (integrator.cpp:337-338 takes the bordered bitmap size as resolution), whose samples can splat into the last row/column
    g, r = got[1:-2, 1:-2], ref[1:-2, 1:-2]
    rel = np.abs(g - r).max(2) / (np.abs(r).max(2) + 1e-6)
    assert (rel < 1e-4).mean() > 0.995                    # a handful of paths fork under the reference's -ffast-math
    assert np.linalg.norm(g[..., :3] - r[..., :3]) / np.linalg.norm(r[..., :3]) < 1e-2
    assert np.allclose(g[..., 3], r[..., 3], rtol=1e-5)   # alpha sums = spp x table weight
    # external control: stop after two progress() calls -> the interrupt's value comes back as the return code
    subprocess.run([HARNESS, path, "responsive", "path_hip", "1", out + "_stop"], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    assert np.load(out + "_stop_meta.npy")[0] == 101


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
def test_plugin_drop_in_envmap_scene(mi, golden_scenes, tmp_path):
    """Same driver, S3-type scene: EnvironmentMap (bitmap pulled back out of the reference's MIP map), area lanterns, twosided diffuse walls,
    smooth-shaded meshes -- everything the adapter flattens from a live mitsuba::Scene."""
    sc = golden_scenes["atrium_small"]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path); out = str(tmp_path / "hip")
    subprocess.run([HARNESS, path, "responsive", "path_hip", "-1", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    got = np.load(out + "_target.npy"); ref = np.load(os.path.join(GOLDEN, "atrium_small_responsive.npz"))["target"]
    g, r = got[1:-2, 1:-2], ref[1:-2, 1:-2]
    rel = np.abs(g - r).max(2) / (np.abs(r).max(2) + 1e-6)
    assert (rel < 1e-3).mean() > 0.98 and np.linalg.norm(g[..., :3] - r[..., :3]) / np.linalg.norm(r[..., :3]) < 1e-2


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
def test_plugin_drop_in_analytic_shapes(mi, golden_scenes, tmp_path):
    """Same driver, scene with live Rectangle / Disk / Sphere / Cylinder objects (one of them the area light) and an un-wrapped roughconductor:
    the adapter rebuilds each shape's transform from its Properties like the shape's own constructor."""
    sc = golden_scenes["cbox_shapes"]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path); out = str(tmp_path / "hip")
    subprocess.run([HARNESS, path, "responsive", "path_hip", "-1", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    got = np.load(out + "_target.npy"); ref = np.load(os.path.join(GOLDEN, "cbox_shapes_responsive.npz"))["target"]
    g, r = got[1:-2, 1:-2], ref[1:-2, 1:-2]
    rel = np.abs(g - r).max(2) / (np.abs(r).max(2) + 1e-6)
    assert (rel < 1e-3).mean() > 0.99 and np.linalg.norm(g[..., :3] - r[..., :3]) / np.linalg.norm(r[..., :3]) < 1e-2


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
@pytest.mark.parametrize("name", ["cbox_lights", "cbox_collimated", "cbox_roughdiffuse", "cbox_phong", "cbox_ward", "ward_room", "cbox_coating", "blend_room", "open_constant", "cbox_materials", "veach_small", "instanced_garden", "cbox_translucent", "textured_room", "sky_view", "veach_microfacets", "textured_plastics_smooth", "glass_pane", "masked_room", "cornell_crop", "layered_room_procedural"])
def test_plugin_drop_in_scene_level_emitters(mi, golden_scenes, tmp_path, name):
    """Same driver; live PointEmitter / SpotEmitter / DirectionalEmitter / ConstantBackgroundEmitter objects, and (cbox_materials) SmoothDielectric /
    SmoothConductor / SmoothPlastic BSDFs, flattened from their Properties; twosided(conductor) and (veach_small, BASELINE config 3 at test size)
    twosided(roughconductor) wrappers are read through their serialised form.  sky_view: EnvironmentMap whose MIP pyramid the adapter rebuilds with the
    reference's own TMIPMap for the filtered camera-ray lookups.  layered_room_procedural: live MixtureBSDF / BumpMap (inside a ScaleTexture) / NormalMap objects, incl.
    bumpmap(mixture) and mask(bumpmap), flattened from their serialised forms."""
    sc = golden_scenes[name]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path); out = str(tmp_path / "hip")
    subprocess.run([HARNESS, path, "responsive", "path_hip", "-1", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    got = np.load(out + "_target.npy"); ref = np.load(os.path.join(GOLDEN, name + "_responsive.npz"))["target"]
    g, r = got[1:-2, 1:-2], ref[1:-2, 1:-2]
    rel = np.abs(g - r).max(2) / (np.abs(r).max(2) + 1e-6)
    assert (rel < 1e-3).mean() > 0.99 and np.linalg.norm(g[..., :3] - r[..., :3]) / np.linalg.norm(r[..., :3]) < 1e-2


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
@pytest.mark.parametrize("name", ["fog_box", "fog_box_global", "fog_mis", "fog_mis_global", "fog_sky", "fog_pane_mis", "fog_masked", "fog_masked_mis", "fog_layered_procedural"])
def test_plugin_drop_in_volumetric(mi, golden_scenes, tmp_path, name):
    """`volpath_simple` / `volpath` swapped for `path_hip` with integrator = "volpath_simple" / "volpath", same responsive driver: live HomogeneousMedium objects (sampling parameters read from their
    serialised form), IsotropicPhaseFunction / HGPhaseFunction, Null BSDFs, interior / exterior media of meshes and of an analytic sphere, the sensor's medium.
    fog_pane_mis / fog_masked* / fog_layered_procedural: live ThinDielectric, Mask (textured opacity) and MixtureBSDF / BumpMap / NormalMap objects inside the volumetric loops.
    Alpha (EOpacity, records.inl:124-137): 1 on an opaque hit, 1 - the transmittance of what lies behind a medium-transition shape, what the sensor's medium removes over two scene radii on a miss."""
    sc = golden_scenes[name]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path); out = str(tmp_path / "hip")
    subprocess.run([HARNESS, path, "responsive", "path_hip", "-1", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    got = np.load(out + "_target.npy"); ref = np.load(os.path.join(GOLDEN, name + "_responsive.npz"))["target"]
    g, r = got[1:-2, 1:-2, :3], ref[1:-2, 1:-2, :3]
    rel = np.abs(g - r).max(2) / (np.abs(r).max(2) + 1e-6)
    loose = name == "fog_sky" or name.startswith("fog_masked") or name.startswith("fog_layered")      # rough conductors / the environment map under the shipped build's -ffast-math: a few forked paths, as in the other drop-in tests
    assert (rel < (1e-3 if loose else 1e-4)).mean() > 0.99 and np.linalg.norm(g - r) / np.linalg.norm(r) < (1e-2 if loose else 1e-3)      # fog_sky: an environment map (device atan2 / acos, -ffast-math forks as in the other envmap drop-ins)
    assert (np.abs(got[1:-2, 1:-2, 3] - ref[1:-2, 1:-2, 3]) < 1e-3 * sc.spp).mean() > 0.99      # alpha incl. the transmittance behind medium-transition shapes (records.inl:124-137)


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
@pytest.mark.parametrize("name", ["sunsky_terrace", "sunsky_terrace_dirsun"])
def test_plugin_drop_in_sunsky(mi, golden_scenes, tmp_path, name):
    """The reference's `sunsky` emitter (src/emitters/sunsky.cpp over sky.cpp / sun.cpp, Hosek-Wilkie sky model) is a COMPOUND emitter: Scene::addChild
    (scene.cpp:530-539) adds its elements -- the sky (+ sun disc) rasterised into an `envmap`, and a `directional` sun when sunRadiusScale = 0 -- so inside a
    Mitsuba-IM build the drop-in plugin renders sunsky scenes through its envmap / directional paths.  (The sky model itself is not restated: the standalone
    front end and the oracle refuse the emitter by name.)"""
    sc = golden_scenes[name]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path); out = str(tmp_path / "hip")
    subprocess.run([HARNESS, path, "responsive", "path_hip", "-1", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
    got = np.load(out + "_target.npy"); ref = np.load(os.path.join(GOLDEN, name + "_responsive.npz"))["target"]
    g, r = got[1:-2, 1:-2], ref[1:-2, 1:-2]
    rel = np.abs(g - r).max(2) / (np.abs(r).max(2) + 1e-6)
    assert (rel < 1e-3).mean() > 0.99 and np.linalg.norm(g[..., :3] - r[..., :3]) / np.linalg.norm(r[..., :3]) < 1e-2
    with pytest.raises(Exception):
        mi.Scene(sc)                                   # the standalone path does not build the sky model


def test_host_mirror_controls(mi, golden_scenes):
    """C++ host mirror (csrc/integrator_host.cpp) through its C shim: return codes and error strings of the reference interface."""
    import ctypes as C
    L = mi.lib().L
    L.mi_host_create.restype = C.c_void_p; L.mi_host_last_error.restype = C.c_char_p; L.mi_host_statistics.restype = C.c_char_p
    L.mi_host_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    L.mi_host_preprocess.argtypes = [C.c_void_p, C.c_void_p]; L.mi_host_destroy.argtypes = [C.c_void_p]; L.mi_host_statistics.argtypes = [C.c_void_p]
    CB = C.CFUNCTYPE(C.c_int, C.c_double, C.c_void_p)
    L.mi_host_render.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), CB, C.c_void_p, C.c_int, C.c_int]
    assert L.mi_host_create(8, 0, 0, 0, 1, 4, 0, 0, 0) is None and b"rrDepth" in L.mi_host_last_error()
    assert L.mi_host_create(0, 5, 0, 0, 1, 4, 0, 0, 0) is None and b"maxDepth" in L.mi_host_last_error()
    sc = golden_scenes["cornell_small"]; gs = mi.Scene(sc)
    h = L.mi_host_create(sc.max_depth, sc.rr_depth, 0, 0, sc.sampler, sc.spp, 0, 0, 4)      # 4 planes per batch -> 4 batches
    assert h and L.mi_host_preprocess(h, gs.h) == 0
    target = np.zeros((sc.height + 2, sc.width + 2, 4), np.float32)
    calls = []
    cont, abort = C.c_int(1), C.c_int(0)
    rc = L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: calls.append(spp) or 0), None, 0, 1)
    assert rc == 0 and calls == [0.0, 8.0]                # one progress() per pair of batches (two path pools / streams), always on a new sample plane
    r = mi.Render(gs, opacity=True); r.run(); assert (r.read_film(1).view(np.uint32) == target.view(np.uint32)).all()
    assert b"rays/sample" in L.mi_host_statistics(h)
    assert L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: 0), None, 1, 4) == 0     # non-zero threads idle
    abort.value = 1; assert L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: 0), None, 0, 1) == -1
    abort.value = 0; cont.value = 0; assert L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: 0), None, 0, 1) == -2
    cont.value = 1; assert L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: 100 if spp >= 4 else 0), None, 0, 1) == 100
    # Integrator::cancel from another context (here: the progress callback) while the render is under way: not lost, render returns -1 early
    L.mi_host_cancel.argtypes = [C.c_void_p]; L.mi_host_cancel.restype = None
    seen = []
    rc = L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: (seen.append(spp), L.mi_host_cancel(h) if spp >= 8 else None, 0)[2]), None, 0, 1)
    assert rc == -1 and seen == [0.0, 8.0]
    assert L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: 0), None, 0, 1) == 0     # the flag is reset at the start of the next render()
    L.mi_host_destroy(h)


def test_host_mirror_devices_replicas(mi, golden_scenes):
    """Multi-device inside the product (SURVEY §8b `devices`, §8e): MIPathTracerHIP with devices = [0, 0] renders with TWO replicas -- a scene clone and a render
    handle each, one host thread each, film rows interleaved (mi_render_run_rows), films merged by addition (mi_render_merge_film; the reference merges worker
    blocks in src/librender/renderproc.cpp:142-149).  On one GPU both replicas share the device; the film must equal the single-replica film: bit for bit in
    every pixel whose samples were accumulated by one replica (all of them, for the box filter's own-pixel sums)."""
    import ctypes as C
    L = mi.lib().L
    L.mi_host_create_devices.restype = C.c_void_p
    L.mi_host_create_devices.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]
    L.mi_host_preprocess.argtypes = [C.c_void_p, C.c_void_p]; L.mi_host_destroy.argtypes = [C.c_void_p]
    L.mi_host_statistics.restype = C.c_char_p; L.mi_host_statistics.argtypes = [C.c_void_p]
    CB = C.CFUNCTYPE(C.c_int, C.c_double, C.c_void_p)
    L.mi_host_render.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), CB, C.c_void_p, C.c_int, C.c_int]
    for name in ("cornell_small", "cornell_small_gauss", "veach_small"):
        sc = golden_scenes[name]; gs = mi.Scene(sc)
        single = mi.Render(gs, opacity=True); single.run(); ref = single.read_film(1); rst = single.stats()
        devs = (C.c_uint32 * 3)(0, 0, 0)
        h = L.mi_host_create_devices(sc.max_depth, sc.rr_depth, 0, 0, sc.sampler, sc.spp, sc.seed, devs, 3, 4)
        assert h and L.mi_host_preprocess(h, gs.h) == 0
        target = np.zeros_like(ref); cont, abort = C.c_int(1), C.c_int(0); calls = []
        rc = L.mi_host_render(h, target.ctypes.data, C.byref(cont), C.byref(abort), CB(lambda spp, u: calls.append(spp) or 0), None, 0, 1)
        assert rc == 0 and len(calls) >= 1
        same = (target.view(np.uint32) == ref.view(np.uint32)).all(2)
        if name == "cornell_small":
            assert same[1:-1, 1:-1].mean() > 0.999 and np.allclose(target, ref, rtol=1e-6, atol=1e-7)      # box filter: own-pixel sums only (edge splats aside)
        else:
            assert np.allclose(target, ref, rtol=2e-5, atol=2e-6)      # wide filter / libm BSDFs: cross-pixel splats are float atomics in either case
        stats = L.mi_host_statistics(h).decode(); assert "rays/sample" in stats
        assert abs(float(stats.split("|")[1].split()[0]) - rst["rays"] / rst["samples"]) < 0.02      # the merged handle reports the replicas' ray counters too
        # classic face (no target, no controls): one submission per replica
        assert L.mi_host_render(h, None, None, None, CB(), None, 0, 1) == 0
        L.mi_host_destroy(h)


@pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(PLUGIN)), reason="reference build (oracle/_ref) or adapter plugin not present")
@pytest.mark.parametrize("name", ["cornell_small", "cornell_small_gauss", "cbox_materials"])
def test_plugin_classic_face_through_renderjob(mi, golden_scenes, tmp_path, name):
    """The CLASSIC interface end to end: the reference's own RenderJob::run (src/librender/renderjob.cpp:66-120) -> Scene::preprocess -> Scene::render
    (scene.cpp:475-479) -> Integrator::render -> Film::put drives first the reference's `path` (BlockedRenderProcess over the scheduler's local workers), then
    `path_hip` (PathTracerHIP::render: one submission, one Film::put of the whole frame, queue->signalRefresh).  A capturing Film records what each delivers."""
    sc = golden_scenes[name]
    path = str(tmp_path / "s.miscene"); mi.scenes.save_scene(sc, path)
    films = {}
    for plugin in ("path", "path_hip"):
        out = str(tmp_path / plugin)
        subprocess.run([HARNESS, path, "classic", plugin, "4", out], cwd=os.path.dirname(HARNESS), env=HARNESS_ENV, check=True, timeout=300)
        meta = np.load(out + "_meta.npy"); films[plugin] = np.load(out + "_film.npy")
        assert meta[0] == 1 and meta[2] >= 1                    # render() succeeded, Film::put was called
    a, b = films["path_hip"], films["path"]
    assert a.shape == b.shape == (sc.height, sc.width, 5)
    ia, ib = a[1:-1, 1:-1], b[1:-1, 1:-1]                      # interior: at the film edge the classic driver's blocks also carry samples of border pixels (high-quality edges)
    assert np.allclose(ia[..., 3:], ib[..., 3:], rtol=1e-5)    # alpha and weight sums
    rel = np.abs(ia[..., :3] - ib[..., :3]).max(2) / (np.abs(ib[..., :3]).max(2) + 1e-6)
    assert (rel < 1e-4).mean() > 0.99                          # the reference is a -ffast-math build: a handful of forked paths
    assert np.linalg.norm(ia[..., :3] - ib[..., :3]) / np.linalg.norm(ib[..., :3]) < 5e-3


@pytest.mark.gpu
def test_bench_faces_and_devices(tmp_path):
    """bench.py's product-path modes end to end on one GPU: both faces of the host mirror, and the in-process `devices` path with two replicas on device 0
    (MI355PT_BENCH_DEVICES=0,0) -- same JSON schema as the C-ABI line, the fixed job as `value` and the weak-scaling job beside it."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "1", "--spp", "8", "--width", "640", "--height", "360", "--full", "--no-cpu-baseline"]
    lines = {}
    for tag, extra, env in (("abi", [], {}), ("classic", ["--face", "classic"], {}), ("responsive", ["--face", "responsive"], {}),
                            ("devices", ["--gpus", "2", "--via", "devices", "--face", "responsive"], {"MI355PT_BENCH_DEVICES": "0,0"})):
        out = subprocess.run(base + extra, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines[tag] = json.loads(out.stdout.strip().splitlines()[-1])
        assert lines[tag]["value"] > 0 and lines[tag]["unit"] == "Msamples/s" and "face" in lines[tag]["config"]
    assert lines["devices"]["n_gpus"] == 2 and lines["devices"]["scaling"] == "strong" and lines["devices"]["weak"]["value"] > 0
    assert lines["abi"]["roofline"] is not None and lines["classic"]["roofline"] is None


@pytest.mark.gpu
def test_bench_dump_outputs(mi, tmp_path):
    """bench.py --dump-outputs: the raw film of the last timed step as float32, the same from run to run, and the film the C-ABI hands back for the same scene
    rendered directly; --steps sets the timed steps, a plain run carries the headline figure only."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    films = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "0", "--spp", "8", "--width", "320", "--height", "180",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and "roofline" not in line and "cpu_baseline" not in line
        assert sorted(os.listdir(d)) == ["film.npy"]
        films.append(np.load(d / "film.npy"))
    S = mi.scenes
    sc = S.cornell_box(320, 180, 8, sampler=S.SAMPLER_SOBOL, max_depth=8)
    r = mi.Render(mi.Scene(sc, device=0), device=0); r.run(); ref = r.read_film(0)
    for f in films:
        assert f.dtype == np.float32 and f.shape == ref.shape
        assert (f.view(np.uint32) == ref.view(np.uint32)).all(2).mean() > 0.995 and np.allclose(f, ref, rtol=2e-6, atol=1e-7)
