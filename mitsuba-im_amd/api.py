"""ctypes binding of libmi355pt.so (C-ABI: include/mi355pt.h).  Fails loudly when the HIP library is missing:
there is no CPU fallback on the product path."""
import ctypes as C
import os
import struct
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355PT_LIB") or os.path.join(_HERE, "libmi355pt.so")   # MI355PT_LIB: A/B another build of the same library
SOBOL_PATH = os.path.join(_HERE, "data", "sobol_tables.bin")


class MiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mi355pt error {code}: {msg}")
        self.code = code


class MiShape(C.Structure):
    _fields_ = [("first_tri", C.c_uint32), ("tri_count", C.c_uint32), ("first_vert", C.c_uint32), ("vert_count", C.c_uint32),
                ("bsdf", C.c_int32), ("emitter", C.c_int32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class MiMaterial(C.Structure):
    _fields_ = [("type", C.c_uint32), ("flags", C.c_uint32), ("distr", C.c_uint32), ("alpha", C.c_float),
                ("reflectance", C.c_float * 3), ("eta", C.c_float * 3), ("k", C.c_float * 3), ("specular", C.c_float * 3)]


class MiEmitter(C.Structure):
    _fields_ = [("type", C.c_uint32), ("shape", C.c_int32), ("radiance", C.c_float * 3), ("weight", C.c_float), ("cutoff", C.c_float), ("beam", C.c_float),
                ("to_world", C.c_float * 16)]


class MiAnalytic(C.Structure):
    _fields_ = [("type", C.c_uint32), ("bsdf", C.c_int32), ("emitter", C.c_int32), ("flags", C.c_uint32),
                ("to_world", C.c_float * 16), ("to_object", C.c_float * 16), ("radius", C.c_float), ("length", C.c_float), ("pad", C.c_float * 2)]


class MiTexture(C.Structure):
    _fields_ = [("type", C.c_uint32), ("color0", C.c_float * 3), ("color1", C.c_float * 3), ("line_width", C.c_float),
                ("uoffset", C.c_float), ("voffset", C.c_float), ("uscale", C.c_float), ("vscale", C.c_float),
                ("wrap_u", C.c_uint32), ("wrap_v", C.c_uint32), ("filter", C.c_uint32), ("max_anisotropy", C.c_float), ("first_level", C.c_uint32), ("n_levels", C.c_uint32)]


class MiInstance(C.Structure):
    _fields_ = [("group", C.c_uint32), ("pad", C.c_uint32 * 3), ("to_world", C.c_float * 16), ("to_object", C.c_float * 16)]


class MiRenderParams(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("rr_depth", C.c_int32), ("strict_normals", C.c_uint32), ("hide_emitters", C.c_uint32),
                ("sampler", C.c_uint32), ("spp", C.c_uint32), ("seed", C.c_uint64), ("device", C.c_uint32), ("planes_per_batch", C.c_uint32), ("opacity", C.c_uint32), ("integrator", C.c_uint32), ("emitter_samples", C.c_uint32), ("bsdf_samples", C.c_uint32),
                ("shading_samples", C.c_uint32), ("ray_length", C.c_float)]


class MiTile(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]


class MiStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("path_length_sum", C.c_uint64), ("samples", C.c_uint64),
                ("render_ms", C.c_double), ("extend_ms", C.c_double), ("shade_ms", C.c_double), ("shadow_ms", C.c_double), ("other_ms", C.c_double),
                ("extend_launches", C.c_uint64), ("extend_rays", C.c_uint64), ("extend_launches_all", C.c_uint64)]


class MiAdaptiveParams(C.Structure):
    _fields_ = [("max_error", C.c_float), ("p_value", C.c_float), ("max_sample_factor", C.c_int32), ("round_samples", C.c_uint32), ("average_luminance", C.c_float), ("pad", C.c_uint32 * 3)]


class MiAdaptiveStats(C.Structure):
    _fields_ = [("samples_used", C.c_uint64), ("samples_traced", C.c_uint64), ("rounds", C.c_uint32), ("pixels_at_cap", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32),
                ("average_luminance", C.c_float), ("quantile", C.c_float)]


class MiField(C.Structure):
    _fields_ = [("field", C.c_uint32), ("undefined", C.c_float * 3)]


class MiDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("demodulate", C.c_uint32), ("pad", C.c_uint32 * 3)]


class MiTemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_float), ("sigma_position", C.c_float), ("min_normal_dot", C.c_float), ("pad", C.c_uint32)]


# field kinds in the order of the reference's EField (src/integrators/misc/field.cpp:57-67), then the two that follow the scene's frame mark (Scene.mark_frame)
# = MI_FIELD_* of include/mi355pt.h
FIELD_NAMES = ("position", "relPosition", "distance", "geoNormal", "shNormal", "uv", "albedo", "shapeIndex", "primIndex", "prevPosition", "motion")
MOTION_FIELDS = ("prevPosition", "motion")      # need the marked state: refused where it is not followed (adaptive renders, the host mirror and its `devices` renders)
SCALAR_FIELDS = ("distance", "shapeIndex", "primIndex")      # the three values of these are equal


def normalize_fields(fields):
    """[(name, (r, g, b))] from a list of names or (name, undefined) pairs, `undefined` a float or an RGB triple (default 0)."""
    out = []
    for f in fields or []:
        name, undef = (f, 0.0) if isinstance(f, str) else (f[0], f[1])
        if name not in FIELD_NAMES:
            raise ValueError(f"unknown field \"{name}\": must be one of " + ", ".join(FIELD_NAMES))
        u = np.broadcast_to(np.asarray(undef, np.float32), (3,)) if np.ndim(undef) == 0 else np.asarray(undef, np.float32).reshape(3)
        out.append((name, tuple(float(x) for x in u)))
    return out


class MiPoolOverrides(C.Structure):
    """0 = unset (the library's default rule)"""
    _fields_ = [("segments", C.c_uint32), ("grid_extend", C.c_uint32), ("grid_shade", C.c_uint32), ("grid_shadow", C.c_uint32)]


class MiPoolShape(C.Structure):
    _fields_ = [("n_seg", C.c_uint32), ("cap", C.c_uint32), ("grid_extend", C.c_uint32), ("grid_shade", C.c_uint32), ("grid_shadow", C.c_uint32)]


class MiPoolInfo(C.Structure):
    _fields_ = [("n_seg", C.c_uint32), ("cap", C.c_uint32), ("n_pools", C.c_uint32), ("grid_extend", C.c_uint32), ("grid_shade", C.c_uint32), ("grid_shadow", C.c_uint32),
                ("lds_tables", C.c_uint32), ("sorted", C.c_uint32), ("has_roughconductor", C.c_uint32), ("integrator", C.c_uint32), ("shade_table_bytes", C.c_uint32), ("pad", C.c_uint32), ("pool_paths", C.c_uint64)]


class MiFusedDebugInfo(C.Structure):
    _fields_ = [("wide", C.c_uint32), ("bvh_depth", C.c_uint32), ("bvh_stack_direct", C.c_uint32), ("max_stack_seen", C.c_uint32), ("rays_counted", C.c_uint64)]


EXPORTS = ["mi_last_error", "mi_set_sobol_tables", "mi_load_sobol_tables", "mi_scene_create", "mi_scene_destroy", "mi_scene_set_triangles",
           "mi_scene_set_analytic", "mi_scene_set_instances", "mi_scene_set_media", "mi_scene_set_materials", "mi_scene_set_material_tables", "mi_scene_set_textures", "mi_scene_set_texture_data", "mi_scene_set_emitters", "mi_scene_set_envmap", "mi_scene_set_envmap_filter", "mi_scene_set_camera", "mi_scene_set_lens", "mi_scene_set_film",
           "mi_scene_commit", "mi_scene_ray_intersect", "mi_scene_clone", "mi_scene_update_camera", "mi_scene_update_lens", "mi_scene_update_materials", "mi_scene_update_emitters", "mi_scene_update_envmap_transform", "mi_scene_update_vertices", "mi_scene_update_instances", "mi_scene_update_geometry", "mi_scene_mark_frame", "mi_scene_revision", "mi_render_merge_film", "mi_render_create", "mi_render_destroy", "mi_render_run", "mi_render_run_rows", "mi_render_clear", "mi_render_cancel",
           "mi_render_set_adaptive", "mi_render_run_adaptive", "mi_render_read_sample_counts", "mi_render_adaptive_stats",
           "mi_render_set_fields", "mi_render_field_film_size", "mi_render_read_fields", "mi_render_field_samples", "mi_denoise_image", "mi_render_denoise", "mi_render_denoise_device", "mi_history_create", "mi_history_destroy", "mi_history_reset", "mi_history_frames", "mi_history_read", "mi_denoise_image_temporal", "mi_render_denoise_temporal", "mi_render_denoise_temporal_device", "mi_scene_world_to_pixel", "mi_render_film_size", "mi_render_read_film", "mi_render_read_film_device", "mi_render_samples", "mi_render_stats",
           "mi_render_set_profiling", "mi_render_debug_sensor_differentials", "mi_render_debug_film_put", "mi_debug_intersect", "mi_debug_intersect_inst", "mi_debug_intersect_fused", "mi_debug_sobol", "mi_debug_camera_rays", "mi_debug_camera_rays_lens", "mi_debug_sincosf", "mi_debug_libm", "mi_debug_bsdf", "mi_debug_texture", "mi_debug_emitter_sample", "mi_debug_emitter_eval", "mi_debug_medium", "mi_debug_surface", "mi_debug_geometry_bytes", "mi_debug_read_geometry", "mi_debug_pool_shape", "mi_render_debug_pool_info"]
HOST_EXPORTS = ["mi_host_last_error", "mi_host_create", "mi_host_create_devices", "mi_host_create_ex", "mi_host_create_direct", "mi_host_create_ao", "mi_host_destroy", "mi_host_preprocess", "mi_host_render", "mi_host_cancel", "mi_host_statistics",
                "mi_host_set_camera", "mi_host_set_lens", "mi_host_set_materials", "mi_host_set_emitters", "mi_host_set_envmap_transform", "mi_host_set_vertices", "mi_host_set_instances", "mi_host_set_geometry"]


def build(force=False):
    """Compile the HIP extension in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")] + (["-B"] if force else []))
    return LIB_PATH


class Lib:
    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise MiError(-1, f"{path} is missing: build it with `make -C mitsuba-im_amd/csrc` (there is no CPU fallback)")
        L = C.CDLL(path)
        self.L = L
        L.mi_last_error.restype = C.c_char_p
        vp, u32, u64, i32, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
        L.mi_set_sobol_tables.argtypes = [vp, u32, vp, vp]
        L.mi_scene_create.argtypes = [C.POINTER(vp)]
        L.mi_scene_destroy.argtypes = [vp]; L.mi_scene_destroy.restype = None
        L.mi_scene_set_triangles.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, u32]
        L.mi_scene_set_analytic.argtypes = [vp, vp, u32]
        L.mi_scene_set_instances.argtypes = [vp, vp, u32]
        L.mi_scene_set_media.argtypes = [vp, vp, u32, vp, u32, C.c_int32]
        L.mi_scene_set_material_tables.argtypes = [vp, vp, u32]
        L.mi_scene_set_textures.argtypes = [vp, vp, u32]
        L.mi_scene_set_texture_data.argtypes = [vp, vp, u32, vp, u64]
        L.mi_scene_set_materials.argtypes = [vp, vp, u32]
        L.mi_scene_set_emitters.argtypes = [vp, vp, u32]
        L.mi_scene_set_envmap.argtypes = [vp, vp, u32, u32, vp, f32]
        L.mi_scene_set_envmap_filter.argtypes = [vp, C.c_int32]
        L.mi_scene_set_camera.argtypes = [vp, vp, vp, f32, f32]
        L.mi_scene_set_lens.argtypes = [vp, f32, f32]
        L.mi_scene_set_film.argtypes = [vp, u32, u32, u32, f32, f32]
        L.mi_scene_commit.argtypes = [vp, u32]
        L.mi_scene_clone.argtypes = [vp, u32, C.POINTER(vp)]
        L.mi_scene_ray_intersect.argtypes = [vp, vp, u64, vp]
        L.mi_scene_update_camera.argtypes = [vp, vp, vp, f32, f32]
        L.mi_scene_update_lens.argtypes = [vp, f32, f32]
        L.mi_scene_update_materials.argtypes = [vp, vp, u32]
        L.mi_scene_update_emitters.argtypes = [vp, vp, u32]
        L.mi_scene_update_envmap_transform.argtypes = [vp, vp, f32]
        L.mi_scene_update_vertices.argtypes = [vp, vp, vp, u32]
        L.mi_scene_update_instances.argtypes = [vp, vp, u32]
        L.mi_scene_update_geometry.argtypes = [vp, vp, vp, u32, vp, u32]
        L.mi_scene_mark_frame.argtypes = [vp]
        L.mi_scene_revision.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.mi_render_merge_film.argtypes = [vp, vp]
        L.mi_render_create.argtypes = [vp, C.POINTER(MiRenderParams), C.POINTER(vp)]
        L.mi_render_destroy.argtypes = [vp]; L.mi_render_destroy.restype = None
        L.mi_render_run.argtypes = [vp, MiTile, u32, u32]
        L.mi_render_run_rows.argtypes = [vp, MiTile, u32, u32, u32]
        L.mi_render_clear.argtypes = [vp]
        L.mi_render_cancel.argtypes = [vp]; L.mi_render_cancel.restype = None
        L.mi_render_film_size.argtypes = [vp, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.mi_render_read_film.argtypes = [vp, i32, vp]
        L.mi_render_read_film_device.argtypes = [vp, i32, vp]
        L.mi_render_samples.argtypes = [vp, vp, u64, vp]
        L.mi_render_stats.argtypes = [vp, C.POINTER(MiStats)]
        L.mi_render_set_adaptive.argtypes = [vp, C.POINTER(MiAdaptiveParams)]
        L.mi_render_run_adaptive.argtypes = [vp, MiTile]
        L.mi_render_read_sample_counts.argtypes = [vp, vp]
        L.mi_render_adaptive_stats.argtypes = [vp, C.POINTER(MiAdaptiveStats)]
        L.mi_render_set_fields.argtypes = [vp, vp, u32]
        L.mi_render_field_film_size.argtypes = [vp, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.mi_render_read_fields.argtypes = [vp, i32, vp]
        L.mi_render_field_samples.argtypes = [vp, vp, u64, vp]
        L.mi_denoise_image.argtypes = [u32, u32, u32, vp, vp, vp, vp, C.POINTER(MiDenoiseParams), vp, C.POINTER(f32)]
        L.mi_render_denoise.argtypes = [vp, C.POINTER(MiDenoiseParams), vp, C.POINTER(f32)]
        L.mi_render_denoise_device.argtypes = [vp, C.POINTER(MiDenoiseParams), vp, C.POINTER(f32)]
        L.mi_history_create.argtypes = [u32, u32, u32, C.POINTER(vp)]
        L.mi_history_destroy.argtypes = [vp]; L.mi_history_destroy.restype = None
        L.mi_history_reset.argtypes = [vp]
        L.mi_history_frames.argtypes = [vp, C.POINTER(u32)]
        L.mi_history_read.argtypes = [vp, vp, vp]
        L.mi_denoise_image_temporal.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(MiDenoiseParams), C.POINTER(MiTemporalParams), vp, C.POINTER(f32), C.POINTER(f32)]
        L.mi_render_denoise_temporal.argtypes = [vp, vp, C.POINTER(MiDenoiseParams), C.POINTER(MiTemporalParams), vp, C.POINTER(f32), C.POINTER(f32)]
        L.mi_render_denoise_temporal_device.argtypes = [vp, vp, C.POINTER(MiDenoiseParams), C.POINTER(MiTemporalParams), vp, C.POINTER(f32), C.POINTER(f32)]
        L.mi_scene_world_to_pixel.argtypes = [vp, vp]
        L.mi_render_set_profiling.argtypes = [vp, i32]
        L.mi_render_debug_sensor_differentials.argtypes = [vp, vp, u64, vp]
        L.mi_render_debug_film_put.argtypes = [vp, i32, MiTile, u32, u32, u32, vp, vp]
        L.mi_debug_intersect.argtypes = [vp, vp, u64, i32, vp]
        L.mi_debug_intersect_inst.argtypes = [vp, vp, u64, i32, vp, vp]
        L.mi_debug_intersect_fused.argtypes = [vp, vp, u64, i32, vp, u32, u32, u32, u32, vp, C.POINTER(MiFusedDebugInfo)]
        L.mi_debug_sobol.argtypes = [vp, vp, u64, u32, vp, vp]
        L.mi_debug_camera_rays.argtypes = [vp, vp, u64, vp]
        L.mi_debug_camera_rays_lens.argtypes = [vp, vp, vp, u64, vp]
        L.mi_debug_sincosf.argtypes = [vp, u64, vp]
        L.mi_debug_libm.argtypes = [i32, vp, vp, u64, vp]
        L.mi_debug_bsdf.argtypes = [vp, u32, i32, vp, vp, vp, vp, u64, vp]
        L.mi_debug_texture.argtypes = [vp, u32, vp, vp, u64, vp]
        L.mi_debug_emitter_sample.argtypes = [vp, vp, vp, vp, u64, i32, vp]
        L.mi_debug_emitter_eval.argtypes = [vp, u32, vp, vp, vp, vp, vp, u64, vp]
        L.mi_debug_medium.argtypes = [vp, u32, i32, vp, u64, vp]
        L.mi_debug_surface.argtypes = [vp, i32, vp, vp, vp, vp, vp, u64, vp]
        L.mi_debug_geometry_bytes.argtypes = [vp, u32, C.POINTER(u64)]
        L.mi_debug_read_geometry.argtypes = [vp, u32, vp, u64]
        L.mi_debug_pool_shape.argtypes = [u64, i32, u32, C.POINTER(MiPoolOverrides), C.POINTER(MiPoolShape)]
        L.mi_render_debug_pool_info.argtypes = [vp, C.POINTER(MiPoolInfo)]

    def check(self, rc):
        if rc != 0:
            raise MiError(rc, self.L.mi_last_error().decode())


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = Lib()
        load_sobol_tables(_LIB)
    return _LIB


def load_sobol_tables(L, path=SOBOL_PATH):
    """mitsuba-im_amd/data/sobol_tables.bin: Sobol' direction matrices (first 128 dimensions) and the van-der-Corput
    matrices for m = 1..16 -- numeric table DATA of the reference's sampler (src/samplers/sobolseq.cpp:33,106537,107241)."""
    with open(path, "rb") as f:
        assert f.read(8) == b"MISOBOL1"
        dims, rows = struct.unpack("<2I", f.read(8))
        m32 = np.frombuffer(f.read(dims * 52 * 4), dtype="<u4").copy()
        vdc = np.frombuffer(f.read(rows * 52 * 8), dtype="<u8").copy()
        vdci = np.frombuffer(f.read(rows * 52 * 8), dtype="<u8").copy()
    L.check(L.L.mi_set_sobol_tables(m32.ctypes.data, dims, vdc.ctypes.data, vdci.ctypes.data))


def _p(a):
    return None if a is None else a.ctypes.data


def pool_shape(paths, has_roughconductor=False, integrator=0, segments=0, grid_extend=0, grid_shade=0, grid_shadow=0):
    """The shape a path pool of `paths` paths gets (mi_debug_pool_shape: host arithmetic, no device): dict of n_seg, cap and the three stage grids; the overrides are
    what MI355PT_SEGMENTS / MI355PT_GRID_* would set, 0 = unset.  A pool of 2^28 slots or more raises MiError (code 1)."""
    L = lib(); ov = MiPoolOverrides(segments, grid_extend, grid_shade, grid_shadow); out = MiPoolShape()
    L.check(L.L.mi_debug_pool_shape(paths, int(bool(has_roughconductor)), int(integrator), C.byref(ov), C.byref(out)))
    return {k: getattr(out, k) for k, _ in MiPoolShape._fields_}


def device_sincosf(x):
    """glibcSincosf of pt_device.h on an array of floats -> (sin, cos)."""
    L = lib(); a = np.ascontiguousarray(x, np.float32).reshape(-1); out = np.zeros((len(a), 2), np.float32)
    L.check(L.L.mi_debug_sincosf(_p(a), len(a), _p(out))); return out[:, 0], out[:, 1]


LIBM_FUNCTIONS = {"expf": 0, "logf": 1, "powf": 2, "tanf": 3, "atanf": 4, "atan2f": 5, "acosf": 6}


def device_libm(name, x, y=None):
    """The device's restatement of glibc's `name` (libm_glibc.h, as the kernels call it) on arrays of floats."""
    L = lib(); a = np.ascontiguousarray(x, np.float32).reshape(-1); out = np.zeros(len(a), np.float32)
    b = None if y is None else np.ascontiguousarray(y, np.float32).reshape(-1)
    L.check(L.L.mi_debug_libm(LIBM_FUNCTIONS[name], _p(a), _p(b) if b is not None else None, len(a), _p(out))); return out


# starting values of the denoiser's widths (nobody has tuned them on real renders yet)
DENOISE_DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05)


def denoise_image(color, normal, position, albedo=None, iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, device=0):
    """The edge-avoiding a-trous filter (mi_denoise_image, include/mi355pt.h) on H x W x 3 float32 arrays: `normal` and `position` guide it, `albedo` (optional)
    demodulates the colour first.  sigma_position < 0: that fraction of the diagonal of the finite positions' box.  -> (out, resolved_sigma_position)."""
    L = lib(); c = np.ascontiguousarray(color, np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("denoise_image: colour must be H x W x 3")
    n = np.ascontiguousarray(normal, np.float32); p = np.ascontiguousarray(position, np.float32)
    a = None if albedo is None else np.ascontiguousarray(albedo, np.float32)
    for name, g in (("normal", n), ("position", p), ("albedo", a)):
        if g is not None and g.shape != c.shape:
            raise ValueError(f"denoise_image: {name} has shape {g.shape}, the colour {c.shape}")
    prm = MiDenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position), 0 if a is None else 1)
    out = np.zeros_like(c); res = C.c_float(0.0)
    L.check(L.L.mi_denoise_image(int(device), c.shape[1], c.shape[0], _p(c), _p(n), _p(p), _p(a), C.byref(prm), _p(out), C.byref(res)))
    return out, float(res.value)


# starting values of the temporal stage (nobody has tuned them)
TEMPORAL_DEFAULTS = dict(max_history=32.0, temporal_sigma_position=-0.01, min_normal_dot=0.9)


class History:
    """mi_history handle: the accumulated colour, count and guides of the previous frame for one device and one image size (two record sets of 40 B per pixel on
    the device).  One history serves all frames of a sequence; reset() gives back the state after creation."""

    def __init__(self, width, height, device=0):
        L = lib(); self.L = L; self.width = int(width); self.height = int(height); self.device = int(device); self.h = None
        h = C.c_void_p(); L.check(L.L.mi_history_create(self.device, self.width, self.height, C.byref(h))); self.h = h

    def reset(self):
        self.L.check(self.L.L.mi_history_reset(self.h))

    @property
    def frames(self):
        """frames accumulated since creation or reset"""
        n = C.c_uint32(); self.L.check(self.L.L.mi_history_frames(self.h, C.byref(n))); return n.value

    def read(self):
        """-> (accumulated colour H x W x 3, still demodulated; count H x W).  Without a frame: MiError code 1."""
        col = np.zeros((self.height, self.width, 3), np.float32); cnt = np.zeros((self.height, self.width), np.float32)
        self.L.check(self.L.L.mi_history_read(self.h, _p(col), _p(cnt))); return col, cnt

    def close(self):
        if getattr(self, "h", None):
            self.L.L.mi_history_destroy(self.h); self.h = None

    def __del__(self):
        self.close()


def denoise_image_temporal(history, color, normal, position, albedo=None, prev_position=None, world_to_pixel=None, iterations=5, sigma_color=4.0, sigma_normal=0.3,
                           sigma_position=-0.05, max_history=32.0, temporal_sigma_position=-0.01, min_normal_dot=0.9):
    """One temporal frame (mi_denoise_image_temporal, include/mi355pt.h) on H x W x 3 float32 arrays: the history's accumulated colour is reprojected through the
    projection of the frame that wrote it, blended with this frame's (demodulated) colour, and the a-trous levels run on the result.  prev_position: the world
    position each pixel's surface point had in the previous frame (None: static geometry); world_to_pixel: this frame's 3 x 4 projection (Scene.world_to_pixel()).
    -> (out, resolved spatial position width, resolved temporal tolerance)."""
    L = history.L; c = np.ascontiguousarray(color, np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("denoise_image_temporal: colour must be H x W x 3")
    if c.shape[:2] != (history.height, history.width):
        raise MiError(1, f"denoise_image_temporal: the history has the image size {history.width} x {history.height}, the frame {c.shape[1]} x {c.shape[0]}")
    n = np.ascontiguousarray(normal, np.float32); p = np.ascontiguousarray(position, np.float32)
    a = None if albedo is None else np.ascontiguousarray(albedo, np.float32); q = None if prev_position is None else np.ascontiguousarray(prev_position, np.float32)
    for name, g in (("normal", n), ("position", p), ("albedo", a), ("prev_position", q)):
        if g is not None and g.shape != c.shape:
            raise ValueError(f"denoise_image_temporal: {name} has shape {g.shape}, the colour {c.shape}")
    m = None if world_to_pixel is None else np.ascontiguousarray(world_to_pixel, np.float32).reshape(12)
    prm = MiDenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position), 0 if a is None else 1)
    tpr = MiTemporalParams(float(max_history), float(temporal_sigma_position), float(min_normal_dot), 0)
    out = np.zeros_like(c); res = C.c_float(0.0); tres = C.c_float(0.0)
    L.check(L.L.mi_denoise_image_temporal(history.h, _p(c), _p(n), _p(p), _p(a), _p(q), _p(m), C.byref(prm), C.byref(tpr), _p(out), C.byref(res), C.byref(tres)))
    return out, float(res.value), float(tres.value)


def pack_materials(bsdfs):
    """mi_material records from the dict records of a flattened scene (scenes.py)."""
    mats = (MiMaterial * max(1, len(bsdfs)))()
    for i, b in enumerate(bsdfs):
        m = MiMaterial(b["type"], (b["twosided"] & 1) | ((b["sample_visible"] & 1) << 1) | ((b.get("nonlinear", 0) & 1) << 2) | ((b.get("aniso", 0) & 1) << 3) | ((b.get("texture", -1) + 1) << 8), b["distr"], b["alpha"])
        m.reflectance[:] = b["reflectance"]; m.eta[:] = b["eta"]; m.k[:] = b["k"]; m.specular[:] = b["specular"]
        mats[i] = m
    return mats


def pack_emitters(emitters):
    """mi_emitter records from the dict records of a flattened scene."""
    ems = (MiEmitter * max(1, len(emitters)))()
    for i, e in enumerate(emitters):
        em = MiEmitter(e["type"], e["shape"]); em.radiance[:] = e["radiance"]; em.weight = e["weight"]
        em.cutoff, em.beam = e.get("cutoff", 20.0), e.get("beam", 15.0)
        em.to_world[:] = np.asarray(e.get("to_world", np.eye(4)), np.float32).reshape(-1).tolist(); ems[i] = em
    return ems


def pack_instances(insts):
    """mi_instance records from the dict records of a flattened scene (scenes.make_instance)."""
    arr = (MiInstance * max(1, len(insts)))()
    for i, a in enumerate(insts):
        r = MiInstance(a["group"]); r.to_world[:] = np.asarray(a["to_world"], np.float32).reshape(-1).tolist(); r.to_object[:] = np.asarray(a["to_object"], np.float32).reshape(-1).tolist(); arr[i] = r
    return arr


class Scene:
    """mi_scene handle filled from a flattened scene (mitsuba-im_amd/scenes.py)."""

    def __init__(self, sc, device=0):
        L = lib(); self.L = L; self.sc = sc
        h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h))); self.h = h
        shapes = (MiShape * len(sc.shapes))()
        for i, s in enumerate(sc.shapes):
            shapes[i] = MiShape(s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"], s["bsdf"], s["emitter"], (s["face_normals"] & 1) | ((s.get("has_uv", 0) & 1) << 1), s.get("group", 0))
        mats = pack_materials(sc.bsdfs); ems = pack_emitters(sc.emitters)
        L.check(L.L.mi_scene_set_triangles(h, _p(sc.pos), _p(sc.nrm), _p(sc.uv), _p(sc.idx), len(sc.pos), len(sc.idx), C.cast(shapes, C.c_void_p), len(sc.shapes)))
        recs = sc.get("analytic") or []
        if recs:
            an = (MiAnalytic * len(recs))()
            for i, a in enumerate(recs):
                r = MiAnalytic(a["type"], a["bsdf"], a["emitter"], a["flags"])
                r.to_world[:] = a["to_world"].reshape(-1).tolist(); r.to_object[:] = a["to_object"].reshape(-1).tolist()
                r.radius, r.length = a["radius"], a["length"]
                an[i] = r
            L.check(L.L.mi_scene_set_analytic(h, C.cast(an, C.c_void_p), len(recs)))
        insts = sc.get("instances") or []
        if insts:
            L.check(L.L.mi_scene_set_instances(h, C.cast(pack_instances(insts), C.c_void_p), len(insts)))
        media = sc.get("media") or []
        if media:                                       # mi_medium has the layout of the oracle's record (oracle/binding.py OrcMedium): 6 floats, uint, 2 floats, uint, float, uint
            buf = np.zeros(len(media), dtype=[("sigma_a", np.float32, 3), ("sigma_s", np.float32, 3), ("strategy", np.uint32), ("sampling_density", np.float32),
                                              ("medium_sampling_weight", np.float32), ("phase", np.uint32), ("g", np.float32), ("pad", np.uint32)])
            for i, m in enumerate(media):
                buf[i] = (m["sigma_a"], m["sigma_s"], m["strategy"], m["sampling_density"], m["medium_sampling_weight"], m["phase"], m["g"], 0)
            sm = np.ascontiguousarray(sc.shape_media, np.int32)
            L.check(L.L.mi_scene_set_media(h, buf.ctypes.data_as(C.c_void_p), len(media), sm.ctypes.data_as(C.c_void_p), len(sm), int(sc.sensor_medium)))
        L.check(L.L.mi_scene_set_materials(h, C.cast(mats, C.c_void_p), len(sc.bsdfs)))
        texs = sc.get("textures") or []
        if texs:
            ta = (MiTexture * len(texs))()
            for i, t in enumerate(texs):
                r = MiTexture(t["type"]); r.color0[:] = t["color0"]; r.color1[:] = t["color1"]; r.line_width = t["line_width"]
                r.uoffset, r.voffset, r.uscale, r.vscale = t["uoffset"], t["voffset"], t["uscale"], t["vscale"]
                r.wrap_u, r.wrap_v, r.filter, r.max_anisotropy, r.first_level, r.n_levels = t.get("wrap_u", 1), t.get("wrap_v", 1), t.get("filter", 3), t.get("max_anisotropy", 20.0), t.get("first_level", 0), t.get("n_levels", 0); ta[i] = r
            L.check(L.L.mi_scene_set_textures(h, C.cast(ta, C.c_void_p), len(texs)))
            if sc.get("texture_levels") is not None:
                L.check(L.L.mi_scene_set_texture_data(h, _p(sc.texture_levels), len(sc.texture_levels), _p(sc.texture_texels), len(sc.texture_texels)))
        if sc.get("material_tables") is not None:
            L.check(L.L.mi_scene_set_material_tables(h, _p(sc.material_tables), len(sc.material_tables)))
        L.check(L.L.mi_scene_set_emitters(h, C.cast(ems, C.c_void_p), len(sc.emitters)))
        if sc.envmap is not None:
            rgb = np.ascontiguousarray(sc.envmap["rgb"], np.float32); tw = np.ascontiguousarray(sc.envmap["to_world"], np.float32)
            L.check(L.L.mi_scene_set_envmap(h, _p(rgb), rgb.shape[1], rgb.shape[0], _p(tw), float(sc.envmap["scale"])))
            if sc.get("env_texture", 0):
                L.check(L.L.mi_scene_set_envmap_filter(h, int(sc.env_texture) - 1))
        s2c = np.ascontiguousarray(sc.sample_to_camera, np.float32); c2w = np.ascontiguousarray(sc.cam_to_world, np.float32)
        L.check(L.L.mi_scene_set_camera(h, _p(s2c), _p(c2w), sc.near, sc.far))
        if float(sc.get("aperture_radius", 0.0) or 0.0) != 0.0:      # thin lens (scenes.py: aperture_radius / focus_distance; 0 = the pinhole)
            L.check(L.L.mi_scene_set_lens(h, float(sc.aperture_radius), float(sc.get("focus_distance", 0.0) or 0.0)))
        L.check(L.L.mi_scene_set_film(h, sc.width, sc.height, sc.filter, sc.filter_radius, sc.filter_stddev))
        L.check(L.L.mi_scene_commit(h, device))

    def clone(self, device=0):
        """mi_scene_clone: a replica on `device` (a scene of its own: the host-side build is reused, every table uploaded again).  The replica shares this
        object's description `sc`: give it a copy (`twin.sc = copy of sc`) before an update_* call on it, which records the new values there."""
        out = Scene.__new__(Scene); out.L = self.L; out.sc = self.sc; out.h = None
        h = C.c_void_p(); self.L.check(self.L.L.mi_scene_clone(self.h, device, C.byref(h))); out.h = h
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.L.mi_scene_destroy(self.h); self.h = None

    def __del__(self):
        self.close()

    # in-place edits of the committed scene (mi_scene_update_*): no tree build, no re-upload of the geometry.  Each keeps the description `sc` in step (a refused edit
    # leaves both as they were), so a later Render(scene) and an oracle built from scene.sc see the edited scene.
    def update_camera(self, sample_to_camera, cam_to_world, near, far):
        s2c = np.ascontiguousarray(sample_to_camera, np.float32).reshape(4, 4); c2w = np.ascontiguousarray(cam_to_world, np.float32).reshape(4, 4)
        self.L.check(self.L.L.mi_scene_update_camera(self.h, _p(s2c), _p(c2w), float(near), float(far)))
        self.sc.sample_to_camera = s2c; self.sc.cam_to_world = c2w; self.sc.near = float(near); self.sc.far = float(far)

    def update_lens(self, aperture_radius, focus_distance):
        """Focus pull / aperture change of a lens scene: two scalars in place.  Turning a lens on or off is refused (MiError code 3): it changes every path's sample layout."""
        self.L.check(self.L.L.mi_scene_update_lens(self.h, float(aperture_radius), float(focus_distance)))
        self.sc.aperture_radius = float(aperture_radius); self.sc.focus_distance = float(focus_distance)

    def update_materials(self, bsdfs):
        """bsdfs: the full list of dict records, as in the scene description; values may change, structure may not (MiError code 3 names the first offending record)."""
        bsdfs = list(bsdfs); mats = pack_materials(bsdfs)
        self.L.check(self.L.L.mi_scene_update_materials(self.h, C.cast(mats, C.c_void_p), len(bsdfs)))
        self.sc.bsdfs = bsdfs

    def update_emitters(self, emitters):
        emitters = list(emitters); ems = pack_emitters(emitters)
        self.L.check(self.L.L.mi_scene_update_emitters(self.h, C.cast(ems, C.c_void_p), len(emitters)))
        self.sc.emitters = emitters

    def update_envmap(self, to_world, scale):
        tw = np.ascontiguousarray(to_world, np.float32).reshape(4, 4)
        self.L.check(self.L.L.mi_scene_update_envmap_transform(self.h, _p(tw), float(scale)))
        self.sc.envmap = dict(self.sc.envmap, to_world=tw, scale=float(scale))

    def update_vertices(self, pos, nrm=None):
        """New positions [n_verts, 3] (and vertex normals, if and only if the scene has them) for the committed vertex array: per-triangle records and a refit of the
        existing tree on the device, no tree build.  Scenes with shape groups / instances are refused (MiError code 3)."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); nrm = None if nrm is None else np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        if nrm is not None and len(nrm) != len(pos): raise ValueError("update_vertices: one normal per vertex")
        self.L.check(self.L.L.mi_scene_update_vertices(self.h, _p(pos), _p(nrm), len(pos)))
        self.sc.pos = pos
        if nrm is not None: self.sc.nrm = nrm

    def update_instances(self, instances):
        """New to_world / to_object for all committed instances (a list of scenes.make_instance records, groups as committed): the instance records and a refit of the
        scene-level tree on the device, no tree build.  A changed group is refused (MiError code 3), a scene without instances or another count with code 1."""
        instances = list(instances)
        self.L.check(self.L.L.mi_scene_update_instances(self.h, C.cast(pack_instances(instances), C.c_void_p), len(instances)))
        self.sc.instances = instances

    def update_geometry(self, pos=None, nrm=None, instances=None):
        """One frame of an animation: new positions [n_verts, 3] (and normals, if and only if the scene has them) for the whole vertex array, shape-group members
        included, and / or new to_world / to_object for all committed instances.  Per-triangle records, group boxes, instance records and a refit of every tree on the
        device, no tree build.  Works on every committed scene; both parts None is refused (MiError code 1), a changed group with code 3."""
        if pos is not None: pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        if nrm is not None: nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        if nrm is not None and pos is not None and len(nrm) != len(pos): raise ValueError("update_geometry: one normal per vertex")
        if instances is not None: instances = list(instances)
        arr = None if instances is None else C.cast(pack_instances(instances), C.c_void_p)
        self.L.check(self.L.L.mi_scene_update_geometry(self.h, _p(pos), _p(nrm), 0 if pos is None else len(pos), arr, 0 if instances is None else len(instances)))
        if pos is not None: self.sc.pos = pos
        if pos is not None and nrm is not None: self.sc.nrm = nrm
        if instances is not None: self.sc.instances = instances

    def mark_frame(self):
        """mi_scene_mark_frame: the scene as it stands -- vertex positions, instance transforms, the projection and the camera origin -- becomes the "previous" state
        of the prevPosition / motion fields, until the next mark (or commit).  Call it before a frame's edits.  Renders nothing differently; no revision step."""
        self.L.check(self.L.L.mi_scene_mark_frame(self.h))

    GEOMETRY_TABLES = {"nodes": (0, 64), "leaf_records": (1, 48), "tri_shade": (2, 128), "tri_uv": (3, 48), "packet_exact": (4, 48), "packet_groups": (5, 48),
                       "instances": (6, 128), "scene_box": (7, 24), "prev_vertices": (8, 12), "prev_instances": (9, 48)}

    def read_geometry(self, what):
        """One device table as it is now -> uint32 array [records, words]: "nodes", "leaf_records" (word 10 = primitive), "tri_shade", "tri_uv", "packet_exact", "packet_groups", "instances" (word 27 = root node),
        "scene_box" (one record: aabb_lo, aabb_hi), "prev_vertices" / "prev_instances" (the vertex positions / rows 0..2 of every instance's to_world at the last
        mark_frame(); empty on a scene that was never marked)."""
        code, rec = self.GEOMETRY_TABLES[what]; n = C.c_uint64()
        self.L.check(self.L.L.mi_debug_geometry_bytes(self.h, code, C.byref(n)))
        out = np.zeros((n.value // rec, rec // 4), np.uint32)
        self.L.check(self.L.L.mi_debug_read_geometry(self.h, code, _p(out), n.value)); return out

    def world_to_pixel(self):
        """The 3 x 4 projection of the camera as it stands (mi_scene_world_to_pixel): rows X, Y, W of world -> pixel; pixel (i, j)'s centre is at (X / W, Y / W) =
        (i + 0.5, j + 0.5).  A thin lens projects through the lens centre."""
        out = np.zeros((3, 4), np.float32); self.L.check(self.L.L.mi_scene_world_to_pixel(self.h, _p(out))); return out

    def revision(self):
        """(revision, tree_builds): in-place edits applied so far / host-side tree builds (1 for the life of a committed scene)."""
        rev, builds = C.c_uint64(), C.c_uint64()
        self.L.check(self.L.L.mi_scene_revision(self.h, C.byref(rev), C.byref(builds))); return rev.value, builds.value

    def ray_intersect(self, rays8):
        """Scene::rayIntersect for a batch of rays -> structured array of mi_intersection records."""
        rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        dt = np.dtype([("valid", "<u4"), ("t", "<f4"), ("p", "<f4", 3), ("ng", "<f4", 3), ("ns", "<f4", 3), ("s", "<f4", 3), ("tt", "<f4", 3), ("uv", "<f4", 2), ("wi", "<f4", 3), ("bary", "<f4", 2),
                       ("prim", "<u4"), ("instance", "<i4"), ("material", "<i4"), ("emitter", "<i4")])
        out = np.zeros(len(rays8), dt)
        self.L.check(self.L.L.mi_scene_ray_intersect(self.h, _p(rays8), len(rays8), out.ctypes.data)); return out

    # unit-level device entry points
    def intersect(self, rays8, any_hit=False, with_instance=False):
        rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8); out = np.zeros((len(rays8), 4), np.float32)
        if with_instance:
            inst = np.zeros(len(rays8), np.int32)
            self.L.check(self.L.L.mi_debug_intersect_inst(self.h, _p(rays8), len(rays8), int(any_hit), _p(out), _p(inst))); return out, inst
        self.L.check(self.L.L.mi_debug_intersect(self.h, _p(rays8), len(rays8), int(any_hit), _p(out))); return out

    def intersect_fused(self, rays8, any_hit=False, seg_counts=None, thr=48, grid=1792, lds_stack=10):
        """The fused walk (csrc/trace_fused.h) on these rays, laid into queue segments of seg_counts rays each (default: segments of 1024).  Returns (hits, info):
        hits as intersect() gives them (t, u, v, prim; prim < 0: miss / unoccluded, any-hit: prim = 1 for an occluded ray); info = wide, bvh_depth, bvh_stack_direct,
        max_stack_seen, rays_counted, and `unretired` (closest hit: rays whose record still held the sentinel) or `acc_x` (any hit: how often each ray was found
        unoccluded -- 0 or 1; 2 = traced twice)."""
        rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8); n = len(rays8)
        if seg_counts is None: seg_counts = [1024] * (n // 1024) + ([n % 1024] if n % 1024 else [])
        seg = np.ascontiguousarray(seg_counts, np.uint32).reshape(-1); raw = np.zeros((n, 4), np.float32); inf = MiFusedDebugInfo()
        self.L.check(self.L.L.mi_debug_intersect_fused(self.h, _p(rays8), n, int(any_hit), _p(seg), len(seg), thr, grid, lds_stack, _p(raw), C.byref(inf)))
        info = {k: getattr(inf, k) for k, _ in MiFusedDebugInfo._fields_}; out = raw.copy(); w = raw.view(np.uint32)
        if any_hit:
            info["acc_x"] = raw[:, 0].copy(); out[:, 3] = np.where(raw[:, 0] == 0, 1.0, -1.0)
        else:
            info["unretired"] = int((w == 0xFFFFFFFE).all(1).sum()); out[:, 3] = np.where(w[:, 3] >= 0xFFFFFFFE, -1.0, w[:, 3].astype(np.float32))
        return out, info

    def sobol(self, px_py_k, ndims):
        a = np.ascontiguousarray(px_py_k, np.uint32).reshape(-1, 3); idx = np.zeros(len(a), np.uint64); vals = np.zeros((len(a), ndims), np.float32)
        self.L.check(self.L.L.mi_debug_sobol(self.h, _p(a), len(a), ndims, _p(idx), _p(vals))); return idx, vals

    def bsdf_units(self, material, wi, wo=None, uv=None, extra=None):
        """The device's BSDF routines on chosen inputs (mi_debug_bsdf), one call per row.  With `wo`: BSDF::eval + pdf -> [n, 4] = value rgb, pdf.  Without: BSDF::sample
        with the 2-D sample `uv` and the value `extra` for a BSDF that asks its sampler for one more (default 0.5) -> [n, 11] = weight rgb, pdf, wo xyz, eta, delta flag,
        null flag, extra-drawn flag.  Records that need a hit record (mask, bumpmap, normalmap, textured ones) raise MiError code 3 naming the kind."""
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3); n = len(wi)
        if wo is not None:
            wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3); out = np.zeros((n, 4), np.float32)
            if len(wo) != n: raise ValueError("bsdf_units: one wo per wi")
            self.L.check(self.L.L.mi_debug_bsdf(self.h, int(material), 1, _p(wi), _p(wo), None, None, n, _p(out))); return out
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2); ex = np.full(n, 0.5, np.float32) if extra is None else np.ascontiguousarray(extra, np.float32).reshape(-1)
        if len(uv) != n or len(ex) != n: raise ValueError("bsdf_units: one sample and one extra value per wi")
        out = np.zeros((n, 11), np.float32)
        self.L.check(self.L.L.mi_debug_bsdf(self.h, int(material), 0, _p(wi), None, _p(uv), _p(ex), n, _p(out))); return out

    def texture_units(self, texture, uv, partials=None):
        """The device's texture routines on chosen inputs (mi_debug_texture): record `texture` at uv [n, 2]; partials [n, 4] = (dudx, dvdx, dudy, dvdy) for the filtered
        lookup of a camera hit, None for the level-0 lookup of later bounces -> [n, 3]."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2); n = len(uv); out = np.zeros((n, 3), np.float32)
        pa = None if partials is None else np.ascontiguousarray(partials, np.float32).reshape(-1, 4)
        if pa is not None and len(pa) != n: raise ValueError("texture_units: one set of partials per lookup")
        self.L.check(self.L.L.mi_debug_texture(self.h, int(texture), _p(uv), _p(pa), n, _p(out))); return out

    def emitter_sample_units(self, ref, ref_n, uv, raw=False):
        """The device's Scene::sampleEmitterDirect on chosen inputs (mi_debug_emitter_sample), one call per row and no visibility test: ref [n, 3], ref_n [n, 3] (zero: a
        two-sided or medium vertex), uv [n, 2] -> [n, 17] = value rgb, p, d, dist, pdf, n, emitter index, delta flag, em_pdf.  raw: the volumetric integrators' form
        (the value not yet divided by the selection probability em_pdf; without raw em_pdf is 0)."""
        ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3); rn = np.ascontiguousarray(ref_n, np.float32).reshape(-1, 3); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = len(ref); out = np.zeros((n, 17), np.float32)
        if len(rn) != n or len(uv) != n: raise ValueError("emitter_sample_units: one normal and one sample per reference point")
        self.L.check(self.L.L.mi_debug_emitter_sample(self.h, _p(ref), _p(rn), _p(uv), n, int(bool(raw)), _p(out))); return out

    def emitter_eval_units(self, emitter, ref, d, nrm, dist, facing):
        """What a BSDF-sampled ray that finds emitter `emitter` evaluates (mi_debug_emitter_eval), one call per row -> [n, 8].  Area light: value rgb, pdfEmitterDirect.
        Envmap: evalEnvironment rgb, its solid-angle density, then value rgb and density of the fused routine.  Constant: value rgb.  Delta lights raise MiError code 3."""
        ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3); nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        dist = np.ascontiguousarray(dist, np.float32).reshape(-1); fc = np.ascontiguousarray(facing, np.float32).reshape(-1); n = len(ref); out = np.zeros((n, 8), np.float32)
        if not (len(d) == len(nrm) == len(dist) == len(fc) == n): raise ValueError("emitter_eval_units: one direction, normal, distance and flag per reference point")
        self.L.check(self.L.L.mi_debug_emitter_eval(self.h, int(emitter), _p(ref), _p(d), _p(nrm), _p(dist), _p(fc), n, _p(out))); return out

    MEDIUM_MODES = {"transmittance": 0, "distance": 1, "phase_sample": 2, "phase_eval": 3}

    def medium_units(self, medium, mode, inputs):
        """The device's medium routines on chosen inputs (mi_debug_medium), one call per row of inputs [n, 10] -> [n, 12].  "transmittance": columns 6, 7 = mint, maxt ->
        rgb.  "distance": o, d, mint, maxt and the two values drawn -> success, t, p, transmittance rgb, pdfSuccess, pdfFailure, values drawn.  "phase_sample": wi, the
        2-D sample -> wo, the phase function's value for it.  "phase_eval": wi, wo -> value."""
        a = np.ascontiguousarray(inputs, np.float32).reshape(-1, 10); out = np.zeros((len(a), 12), np.float32)
        self.L.check(self.L.L.mi_debug_medium(self.h, int(medium), self.MEDIUM_MODES[mode], _p(a), len(a), _p(out))); return out

    SURFACE_MODES = {"record": 0, "sample": 1, "eval": 2}

    def surface_units(self, mode, rays8, hits4, instance=None, diff6=None, query3=None):
        """The device's surface step on chosen hits (mi_debug_surface), one case per row: rays8 [n, 8], hits4 [n, 4] and instance [n] as intersect(with_instance=True)
        returns them, diff6 [n, 6] = the differential directions of a camera ray (None: a later bounce).  "record" -> [n, 51] (uv, tangents, partials, opacity, first
        textured value, flags, coating and leaf records, leaf reflectance, perturbed frame, wi of the query, the hit and its frame); "sample" with query3 = the 2-D sample
        and the extra value -> [n, 11]; "eval" with query3 = a world direction -> [n, 4]."""
        m = self.SURFACE_MODES[mode]; rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8); n = len(rays8); hits4 = np.ascontiguousarray(hits4, np.float32).reshape(-1, 4)
        ins = None if instance is None else np.ascontiguousarray(instance, np.int32).reshape(-1); d6 = None if diff6 is None else np.ascontiguousarray(diff6, np.float32).reshape(-1, 6)
        q = None if query3 is None else np.ascontiguousarray(query3, np.float32).reshape(-1, 3)
        if len(hits4) != n or any(a is not None and len(a) != n for a in (ins, d6, q)): raise ValueError("surface_units: one hit, instance, differential pair and query per ray")
        out = np.zeros((n, (51, 11, 4)[m]), np.float32)
        self.L.check(self.L.L.mi_debug_surface(self.h, m, _p(rays8), _p(hits4), _p(ins), _p(d6), _p(q), n, _p(out))); return out

    def camera_rays(self, pos2, aperture2=None, differentials=False):
        """Sensor rays (o, mint, d, maxt) at film positions pos2.  aperture2: the aperture sample of every ray of a lens scene (None: (0.5, 0.5), the reference's default
        when none is drawn; ignored without a lens).  differentials: six more floats per ray, the unscaled rx / ry directions."""
        a = np.ascontiguousarray(pos2, np.float32).reshape(-1, 2)
        if aperture2 is None and not differentials:
            out = np.zeros((len(a), 8), np.float32)
            self.L.check(self.L.L.mi_debug_camera_rays(self.h, _p(a), len(a), _p(out))); return out
        ap = np.full((len(a), 2), 0.5, np.float32) if aperture2 is None else np.ascontiguousarray(aperture2, np.float32).reshape(-1, 2)
        if len(ap) != len(a): raise ValueError("camera_rays: one aperture sample per film position")
        out = np.zeros((len(a), 14), np.float32)
        self.L.check(self.L.L.mi_debug_camera_rays_lens(self.h, _p(a), _p(ap), len(a), _p(out)))
        return out if differentials else np.ascontiguousarray(out[:, :8])


class Render:
    """mi_render handle: the integrator instance (MonteCarloIntegrator properties + sampler)."""

    def __init__(self, scene, max_depth=None, rr_depth=None, sampler=None, spp=None, seed=None, device=0, planes_per_batch=0,
                 strict_normals=None, hide_emitters=None, opacity=False, integrator=None, fields=None, emitter_samples=None, bsdf_samples=None,
                 shading_samples=None, ray_length=None):
        sc = scene.sc; L = scene.L; self.L = L; self.scene = scene
        # integrator = INTEGRATOR_DIRECT: emitterSamples / bsdfSamples of direct.cpp:96-107 (the scene description's keys, default 1 each); not read by the other integrators
        if emitter_samples is None: emitter_samples = sc.get("emitter_samples", 1)
        if bsdf_samples is None: bsdf_samples = sc.get("bsdf_samples", 1)
        # integrator = INTEGRATOR_AO: shadingSamples / rayLength of ao.cpp:40-48 (the scene description's keys, default 1 and -1 = automatic); not read by the other integrators
        if shading_samples is None: shading_samples = sc.get("shading_samples", 1)
        if ray_length is None: ray_length = sc.get("ray_length", -1.0)
        p = MiRenderParams(sc.max_depth if max_depth is None else max_depth, sc.rr_depth if rr_depth is None else rr_depth,
                           sc.strict_normals if strict_normals is None else int(strict_normals),
                           sc.hide_emitters if hide_emitters is None else int(hide_emitters),
                           sc.sampler if sampler is None else sampler, sc.spp if spp is None else spp,
                           sc.seed if seed is None else seed, device, planes_per_batch, int(opacity), int(sc.get("integrator", 0) or 0) if integrator is None else int(integrator),
                           1 if emitter_samples is None else int(emitter_samples), 1 if bsdf_samples is None else int(bsdf_samples),
                           1 if shading_samples is None else int(shading_samples), -1.0 if ray_length is None else float(ray_length))
        self.params = p
        h = C.c_void_p(); L.check(L.L.mi_render_create(scene.h, C.byref(p), C.byref(h))); self.h = h
        self.field_names = []; self.last_denoise_sigma_position = None; self.last_temporal_sigma_position = None
        if fields is None: fields = sc.get("fields")          # the scene description's own list (scene files with a `multichannel` integrator); [] = none
        if fields: self.set_fields(fields)
        ad = sc.get("adaptive")                               # the scene description's own parameters (scene files with an `adaptive` integrator); None = uniform sampling
        if ad: self.set_adaptive(**ad)

    def set_adaptive(self, max_error=0.05, p_value=0.05, max_sample_factor=32, round_samples=0, average_luminance=0.0):
        """Per-pixel error control (the reference's `adaptive` integrator over path / volpath_simple / volpath): run_adaptive() then gives every pixel samples until the
        half width of its confidence interval is at most max_error x max(mean luminance, 1 % of average_luminance), or max_sample_factor x spp samples are spent
        (negative: no cap).  round_samples: sample indices traced per round (0 = spp); average_luminance <= 0: estimated.  Only while the film is clear;
        max_error=None turns it off."""
        if max_error is None:
            self.L.check(self.L.L.mi_render_set_adaptive(self.h, None)); return
        p = MiAdaptiveParams(float(max_error), float(p_value), int(max_sample_factor), int(round_samples), float(average_luminance))
        self.L.check(self.L.L.mi_render_set_adaptive(self.h, C.byref(p)))

    def run_adaptive(self, tile=None):
        """One adaptive render of the tile (default: the film) into a clear film; one per clear()."""
        sc = self.scene.sc
        t = MiTile(0, 0, sc.width, sc.height) if tile is None else MiTile(*tile)
        self.L.check(self.L.L.mi_render_run_adaptive(self.h, t))

    def sample_counts(self):
        """H x W uint32: the samples each pixel took in the adaptive run (0 = not rendered)."""
        sc = self.scene.sc; out = np.zeros((sc.height, sc.width), np.uint32)
        self.L.check(self.L.L.mi_render_read_sample_counts(self.h, _p(out))); return out

    def adaptive_stats(self):
        """Of the last adaptive run: samples_used (sum of the counts), samples_traced, rounds, pixels_at_cap, min_count, max_count, average_luminance, quantile."""
        s = MiAdaptiveStats(); self.L.check(self.L.L.mi_render_adaptive_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in MiAdaptiveStats._fields_}

    def set_fields(self, fields):
        """Field channels of the first camera hit (the reference's `multichannel` + `field` integrators): names out of FIELD_NAMES, or (name, undefined) with a float or an
        RGB triple for camera rays that leave the scene.  Only while the film is clear; an empty list removes the fields."""
        fl = normalize_fields(fields); arr = (MiField * max(1, len(fl)))()
        for i, (name, undef) in enumerate(fl):
            arr[i].field = FIELD_NAMES.index(name); arr[i].undefined[:] = undef
        self.L.check(self.L.L.mi_render_set_fields(self.h, C.cast(arr, C.c_void_p), len(fl))); self.field_names = [n for n, _ in fl]

    def field_film_shape(self, layout=2):
        h, w, c, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.L.check(self.L.L.mi_render_field_film_size(self.h, layout, C.byref(h), C.byref(w), C.byref(c), C.byref(b)))
        return h.value, w.value, c.value, b.value

    def read_fields(self, layout=2):
        """layout 0: raw sums (H+2b) x (W+2b) x (3F+1), weight last; layout 2: developed H x W x 3F (field i in channels 3i .. 3i+2)."""
        h, w, c, _ = self.field_film_shape(layout); out = np.zeros((h, w, c), np.float32)
        self.L.check(self.L.L.mi_render_read_fields(self.h, layout, _p(out))); return out

    def denoise(self, iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, demodulate=None, device_ptr=None):
        """The edge-avoiding a-trous filter on this render's own films, on the device (mi_render_denoise): radiance = read_film(2), guides = the first shNormal and the
        first position field, albedo = the first albedo field.  demodulate=None: if the render holds an albedo field.  -> H x W x 3, or None with device_ptr (the
        address of H x W x 3 floats on the render's device, which then holds the result).  The resolved position width is left in last_denoise_sigma_position."""
        if demodulate is None: demodulate = "albedo" in self.field_names
        prm = MiDenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position), int(bool(demodulate))); res = C.c_float(0.0)
        if device_ptr is not None:
            self.L.check(self.L.L.mi_render_denoise_device(self.h, C.byref(prm), C.c_void_p(device_ptr), C.byref(res))); out = None
        else:
            sc = self.scene.sc; out = np.zeros((sc.height, sc.width, 3), np.float32)
            self.L.check(self.L.L.mi_render_denoise(self.h, C.byref(prm), _p(out), C.byref(res)))
        self.last_denoise_sigma_position = float(res.value); return out

    def denoise_temporal(self, history, iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, demodulate=None, max_history=32.0,
                         temporal_sigma_position=-0.01, min_normal_dot=0.9, device_ptr=None):
        """One temporal frame on this render's own films (mi_render_denoise_temporal): radiance and guides as denoise() takes them; the previous position of every
        pixel = the render's first prevPosition field (Scene.mark_frame() before each frame's edits: moved instances and deformed meshes keep their history), without that
        field = its position (static geometry: a surface that moved further than the tolerance drops its history); the projection = the scene's camera as it stands.
        `history` (api.History) must be on this render's device and of its film size.  -> H x W x 3, or None with device_ptr.  The resolved widths are left in
        last_denoise_sigma_position and last_temporal_sigma_position."""
        if demodulate is None: demodulate = "albedo" in self.field_names
        prm = MiDenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position), int(bool(demodulate)))
        tpr = MiTemporalParams(float(max_history), float(temporal_sigma_position), float(min_normal_dot), 0); res = C.c_float(0.0); tres = C.c_float(0.0)
        if device_ptr is not None:
            self.L.check(self.L.L.mi_render_denoise_temporal_device(self.h, history.h, C.byref(prm), C.byref(tpr), C.c_void_p(device_ptr), C.byref(res), C.byref(tres))); out = None
        else:
            sc = self.scene.sc; out = np.zeros((sc.height, sc.width, 3), np.float32)
            self.L.check(self.L.L.mi_render_denoise_temporal(self.h, history.h, C.byref(prm), C.byref(tpr), _p(out), C.byref(res), C.byref(tres)))
        self.last_denoise_sigma_position = float(res.value); self.last_temporal_sigma_position = float(tres.value); return out

    def field_samples(self, pairs):
        """The fields of individual (px, py, sampleIndex) triples -> [n, F, 3]."""
        a = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 3); out = np.zeros((len(a), max(1, len(self.field_names)), 3), np.float32)
        self.L.check(self.L.L.mi_render_field_samples(self.h, _p(a), len(a), _p(out))); return out

    def close(self):
        if getattr(self, "h", None):
            self.L.L.mi_render_destroy(self.h); self.h = None

    def __del__(self):
        self.close()

    def run(self, tile=None, s0=0, s1=None, row_stride=1):
        sc = self.scene.sc
        t = MiTile(0, 0, sc.width, sc.height) if tile is None else MiTile(*tile)
        self.L.check(self.L.L.mi_render_run_rows(self.h, t, row_stride, s0, self.params.spp if s1 is None else s1))

    def clear(self):
        self.L.check(self.L.L.mi_render_clear(self.h))

    def cancel(self):
        self.L.L.mi_render_cancel(self.h)

    def set_profiling(self, on):
        self.L.check(self.L.L.mi_render_set_profiling(self.h, int(on)))

    def film_shape(self, layout=0):
        h, w, c, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.L.check(self.L.L.mi_render_film_size(self.h, layout, C.byref(h), C.byref(w), C.byref(c), C.byref(b)))
        return h.value, w.value, c.value, b.value

    def read_film(self, layout=0):
        h, w, c, _ = self.film_shape(layout); out = np.zeros((h, w, c), np.float32)
        self.L.check(self.L.L.mi_render_read_film(self.h, layout, _p(out))); return out

    def read_film_device(self, layout, device_ptr):
        self.L.check(self.L.L.mi_render_read_film_device(self.h, layout, C.c_void_p(device_ptr)))

    def samples(self, pairs):
        a = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 3); out = np.zeros((len(a), 3), np.float32)
        self.L.check(self.L.L.mi_render_samples(self.h, _p(a), len(a), _p(out))); return out

    def sensor_differentials(self, pairs):
        """What the shading stages recompute for the sensor rays of (px, py, sampleIndex) triples from the path state -> [n, 8]: aperture sample, scaled rx / ry directions."""
        a = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 3); out = np.zeros((len(a), 8), np.float32)
        self.L.check(self.L.L.mi_render_debug_sensor_differentials(self.h, _p(a), len(a), _p(out))); return out

    def film_put_units(self, which, pos2, val4, n_planes, tile=None, row_stride=1, batch_planes=0):
        """Film units (mi_render_debug_film_put): caller-supplied samples through k_film (which = 0), k_adapt_accumulate (1) or k_field_film with every camera ray a miss
        (2).  pos2 [n_planes, n_pix, 2] film positions, val4 [n_planes, n_pix, 4] Li rgb + alpha, n_pix = the pixels of the tile's rows as run() counts them, pixel-minor;
        batch_planes = 0: one launch, k: launches of at most k planes."""
        sc = self.scene.sc; t = MiTile(0, 0, sc.width, sc.height) if tile is None else MiTile(*tile)
        rs = int(row_stride); n_pix = (t.x1 - t.x0) * ((t.y1 - t.y0 + rs - 1) // rs) if rs > 0 else 0          # (a stride of 0 is the library's to refuse: it reads nothing)
        pos2 = np.ascontiguousarray(pos2, np.float32); val4 = np.ascontiguousarray(val4, np.float32)
        if rs > 0 and (pos2.size != n_planes * n_pix * 2 or val4.size != n_planes * n_pix * 4):
            raise ValueError(f"film_put_units: {n_planes} planes of {n_pix} pixels need pos2 [{n_planes}, {n_pix}, 2] and val4 [{n_planes}, {n_pix}, 4]")
        self.L.check(self.L.L.mi_render_debug_film_put(self.h, int(which), t, int(row_stride), int(n_planes), int(batch_planes), _p(pos2), _p(val4)))

    def merge_film(self, other):
        """self += other (raw film sums, field planes included, ray counters): both renders idle, same film, same field list."""
        self.L.check(self.L.L.mi_render_merge_film(self.h, other.h))

    def pool_info(self):
        """The path pools as they are now (read-only): n_pools (the pools the render owns), lds_tables, has_roughconductor and integrator from creation on; n_seg, cap, the
        three stage grids and pool_paths once a run has allocated the pools; shade_table_bytes (dynamic LDS in front of the order list) and sorted (the segments were
        read through the class-sorted order list) of the last shade launch of the path integrator."""
        s = MiPoolInfo(); self.L.check(self.L.L.mi_render_debug_pool_info(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in MiPoolInfo._fields_ if k != "pad"}

    def stats(self):
        s = MiStats(); self.L.check(self.L.L.mi_render_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in MiStats._fields_}


class HostIntegrator:
    """The product path as a reference user sees it: the C++ host mirror mi355::MIPathTracerHIP (csrc/integrator_host.h) behind its C shim (include/mi355pt_host.h).
    face "classic" = Integrator::render as Scene::render drives it (no target, no controls: one submission); "responsive" = ResponsiveIntegrator::render with a target
    film and a progress callback between submissions (src/mitsuba/im_render.cpp:103-222).  devices = HIP devices the film rows are spread over (entries may repeat)."""
    _CB = C.CFUNCTYPE(C.c_int, C.c_double, C.c_void_p)

    def __init__(self, scene, spp=None, devices=(0,), planes_per_batch=0, integrator=None, preview_interval_ms=-1.0, max_depth=None, emitter_samples=None, bsdf_samples=None, shading_samples=None, ray_length=None):
        L = scene.L.L; self.L = L; self.scene = scene; sc = scene.sc
        if sc.get("adaptive"):      # never rendered uniformly without saying so
            raise MiError(3, "HostIntegrator: the host mirror does not offer adaptive sampling (the scene description holds `adaptive` parameters); use Render.run_adaptive")
        for name, _ in normalize_fields(sc.get("fields") or []):      # the replicas of a `devices` render are not marked with the scene: never rendered without saying so
            if name in MOTION_FIELDS:
                raise MiError(3, f"HostIntegrator: the host mirror and its `devices` renders do not follow the frame mark (the scene description holds the field `{name}`); use Render")
        L.mi_host_create_ex.restype = C.c_void_p; L.mi_host_last_error.restype = C.c_char_p; L.mi_host_statistics.restype = C.c_char_p
        L.mi_host_create_ex.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int, C.c_double]
        L.mi_host_preprocess.argtypes = [C.c_void_p, C.c_void_p]; L.mi_host_destroy.argtypes = [C.c_void_p]; L.mi_host_statistics.argtypes = [C.c_void_p]
        L.mi_host_render.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), self._CB, C.c_void_p, C.c_int, C.c_int]
        dev = (C.c_uint32 * len(devices))(*devices)
        self.spp = sc.spp if spp is None else spp
        integ = int(sc.get("integrator", 0) or 0) if integrator is None else int(integrator)
        if integ == 3:      # INTEGRATOR_DIRECT: its own properties (direct.cpp:96-107), the scene description's keys unless given
            L.mi_host_create_direct.restype = C.c_void_p
            L.mi_host_create_direct.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
            n_em = sc.get("emitter_samples", 1) if emitter_samples is None else emitter_samples; n_bs = sc.get("bsdf_samples", 1) if bsdf_samples is None else bsdf_samples
            self.h = L.mi_host_create_direct(sc.strict_normals, sc.hide_emitters, sc.sampler, self.spp, sc.seed, dev, len(devices), planes_per_batch, int(n_em), int(n_bs), float(preview_interval_ms))
        elif integ == 4:      # INTEGRATOR_AO: its own properties (ao.cpp:40-48), the scene description's keys unless given
            L.mi_host_create_ao.restype = C.c_void_p
            L.mi_host_create_ao.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double]
            n_sh = sc.get("shading_samples", 1) if shading_samples is None else shading_samples; length = sc.get("ray_length", -1.0) if ray_length is None else ray_length
            self.h = L.mi_host_create_ao(sc.sampler, self.spp, sc.seed, dev, len(devices), planes_per_batch, int(n_sh), float(length), float(preview_interval_ms))
        else:
            self.h = L.mi_host_create_ex(sc.max_depth if max_depth is None else max_depth, sc.rr_depth, sc.strict_normals, sc.hide_emitters, sc.sampler, self.spp, sc.seed, dev, len(devices),
                                         planes_per_batch, integ, float(preview_interval_ms))
        if not self.h:
            raise RuntimeError(L.mi_host_last_error().decode())
        if L.mi_host_preprocess(self.h, scene.h) != 0:
            raise RuntimeError(L.mi_host_last_error().decode())
        self.cont = C.c_int(1); self.abort = C.c_int(0); self.calls = 0

    def render(self, face="classic", target=None):
        """returns the integrator's return code (0 = all sample planes done)"""
        if face == "classic":
            return self.L.mi_host_render(self.h, None, None, None, self._CB(), None, 0, 1)

        def progress(spp, user):
            self.calls += 1; return 0
        cb = self._CB(progress)
        return self.L.mi_host_render(self.h, target.ctypes.data if target is not None else None, C.byref(self.cont), C.byref(self.abort), cb, None, 0, 1)

    def set_camera(self, sample_to_camera, cam_to_world, near, far):
        """MIPathTracerHIP::setCamera: the borrowed scene and every replica, between two render() calls.  (Use this OR Scene.update_camera on a scene, not both:
        the description scene.sc is kept in step here too.)"""
        s2c = np.ascontiguousarray(sample_to_camera, np.float32).reshape(4, 4); c2w = np.ascontiguousarray(cam_to_world, np.float32).reshape(4, 4)
        self.L.mi_host_set_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]
        if self.L.mi_host_set_camera(self.h, _p(s2c), _p(c2w), float(near), float(far)) != 0:
            raise RuntimeError(self.L.mi_host_last_error().decode())
        sc = self.scene.sc; sc.sample_to_camera = s2c; sc.cam_to_world = c2w; sc.near = float(near); sc.far = float(far)

    def set_lens(self, aperture_radius, focus_distance):
        """MIPathTracerHIP::setLens: mi_scene_update_lens on the borrowed scene and on every replica, between two render() calls."""
        self.L.mi_host_set_lens.argtypes = [C.c_void_p, C.c_float, C.c_float]
        if self.L.mi_host_set_lens(self.h, float(aperture_radius), float(focus_distance)) != 0:
            raise RuntimeError(self.L.mi_host_last_error().decode())
        self.scene.sc.aperture_radius = float(aperture_radius); self.scene.sc.focus_distance = float(focus_distance)

    def set_vertices(self, pos, nrm=None):
        """MIPathTracerHIP::setVertices: mi_scene_update_vertices on the borrowed scene and on every replica, between two render() calls."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); nrm = None if nrm is None else np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        self.L.mi_host_set_vertices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        if self.L.mi_host_set_vertices(self.h, _p(pos), _p(nrm), len(pos)) != 0:
            raise RuntimeError(self.L.mi_host_last_error().decode())
        self.scene.sc.pos = pos
        if nrm is not None: self.scene.sc.nrm = nrm

    def set_geometry(self, pos=None, nrm=None, instances=None):
        """MIPathTracerHIP::setGeometry: mi_scene_update_geometry on the borrowed scene and on every replica, between two render() calls."""
        if pos is not None: pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        if nrm is not None: nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        if instances is not None: instances = list(instances)
        arr = None if instances is None else C.cast(pack_instances(instances), C.c_void_p)
        self.L.mi_host_set_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        if self.L.mi_host_set_geometry(self.h, _p(pos), _p(nrm), 0 if pos is None else len(pos), arr, 0 if instances is None else len(instances)) != 0:
            raise RuntimeError(self.L.mi_host_last_error().decode())
        if pos is not None: self.scene.sc.pos = pos
        if pos is not None and nrm is not None: self.scene.sc.nrm = nrm
        if instances is not None: self.scene.sc.instances = instances

    def set_instances(self, instances):
        """MIPathTracerHIP::setInstances: mi_scene_update_instances on the borrowed scene and on every replica, between two render() calls."""
        instances = list(instances)
        self.L.mi_host_set_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        if self.L.mi_host_set_instances(self.h, C.cast(pack_instances(instances), C.c_void_p), len(instances)) != 0:
            raise RuntimeError(self.L.mi_host_last_error().decode())
        self.scene.sc.instances = instances

    def statistics(self):
        return (self.L.mi_host_statistics(self.h) or b"").decode()

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_host_destroy(self.h); self.h = None

    def __del__(self):
        self.close()
