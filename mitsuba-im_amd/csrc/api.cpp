// api.cpp -- C-ABI of libmi355pt.so (include/mi355pt.h): scene upload, wavefront batch scheduling, film read-back.
// Host orchestration only; all arithmetic on the sample path lives in the kernel translation units (kernels_*.hip over trace.h, trace_fused.h, shade.h, pt_device.h).
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <mutex>
#include <set>
#include "scene_host.h"
#include "geometry_records.h"
#include "queues.h"
#include "fields.h"
#include "direct_const.h"
#include "ao_const.h"
#include "adaptive.h"
#include "denoise.h"
#include "temporal.h"

extern "C" {
void mi_launch_generate(const DScene &, const RenderConst &, const Queues &, const BatchDesc &, uint32_t, hipStream_t);
void mi_launch_extend(const DScene &, const Queues &, int, int, uint32_t, hipStream_t);
void mi_launch_shade_d(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shade_d_env(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shade_rc(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shade_rc_env(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shade_rcw(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shade_rcw_env(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shadow(const DScene &, const Queues &, uint32_t, hipStream_t);
bool mi_fused_walk(const DScene &);
uint32_t mi_fused_grid(void);
void mi_launch_extend_fused(const DScene &, const Queues &, int, int, uint32_t *, hipStream_t);
void mi_launch_shadow_fused(const DScene &, const Queues &, uint32_t *, hipStream_t);
void mi_launch_shade_vol(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shadow_vol(const DScene &, const Queues &, uint32_t, hipStream_t);
void mi_launch_shade_volmis(const DScene &, const RenderConst &, const Queues &, int, uint32_t, size_t, hipStream_t);
void mi_launch_shadow_volmis(const DScene &, const Queues &, uint32_t, hipStream_t);
void mi_launch_film(const DScene &, const Queues &, const BatchDesc &, float *, float *, hipStream_t);
void mi_launch_direct_d(const DScene &, const RenderConst &, const DirectConst &, const Queues &, const BatchDesc &, int, uint32_t, size_t, hipStream_t);
void mi_launch_direct_d_env(const DScene &, const RenderConst &, const DirectConst &, const Queues &, const BatchDesc &, int, uint32_t, size_t, hipStream_t);
void mi_launch_direct_rc(const DScene &, const RenderConst &, const DirectConst &, const Queues &, const BatchDesc &, int, uint32_t, size_t, hipStream_t);
void mi_launch_direct_rc_env(const DScene &, const RenderConst &, const DirectConst &, const Queues &, const BatchDesc &, int, uint32_t, size_t, hipStream_t);
void mi_launch_direct_hit(const DScene &, const RenderConst &, const DirectConst &, const Queues &, uint32_t, hipStream_t);
void mi_launch_ao(const DScene &, const RenderConst &, const AoConst &, const Queues &, const BatchDesc &, uint32_t, size_t, hipStream_t);
void mi_launch_ao_resolve(const Queues &, float, uint32_t, hipStream_t);
void mi_launch_env_primary(const DScene &, const RenderConst &, const Queues &, int, uint32_t, hipStream_t);
void mi_launch_film_layout(const float *, const float *, float *, int, int, int, int, hipStream_t);
void mi_launch_gather_samples(const Queues &, const uint32_t *, uint64_t, float *, hipStream_t);
void mi_launch_film_add(float *, const float *, size_t, hipStream_t);
void mi_launch_debug_intersect(const DScene &, const float *, uint64_t, int, float *, int *, hipStream_t);
void mi_launch_ray_intersect(const DScene &, const float *, uint64_t, mi_intersection *, hipStream_t);
void mi_launch_debug_fused(const DScene &, const Queues &, int, uint32_t, uint32_t *, uint32_t, uint32_t, int *, hipStream_t);
uint32_t mi_fused_lds_stack(void);
void mi_launch_debug_sobol(const DScene &, const uint32_t *, uint64_t, uint32_t, unsigned long long *, float *, hipStream_t);
void mi_launch_debug_camera(const DScene &, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_camera_lens(const DScene &, const float *, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_sensor_differentials(const DScene &, const RenderConst &, const Queues &, uint64_t, float *, hipStream_t);
void mi_launch_debug_sincosf(const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_libm(int, const float *, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_bsdf(const DScene &, int, int, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_texture(const DScene &, uint32_t, const float *, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_emitter_sample(const DScene &, int, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_emitter_eval(const DScene &, int, int, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_medium(const DScene &, uint32_t, int, const float *, uint64_t, float *, hipStream_t);
void mi_launch_debug_surface(const DScene &, int, const float *, const float *, const int *, const float *, const float *, uint64_t, float *, hipStream_t);
void mi_launch_field_film(const DScene &, const FieldArgs &, const Queues &, const BatchDesc &, float *, float *, hipStream_t);
void mi_launch_field_samples(const DScene &, const FieldArgs &, const Queues &, uint64_t, float *, hipStream_t);
void mi_launch_field_layout(const float *, const float *, float *, int, int, int, int, int, hipStream_t);
void mi_launch_patch_material_flags(TriShade *, uint32_t, const uint32_t *, uint32_t, hipStream_t);
void mi_launch_tri_records(const mi::GeoEditTables &, hipStream_t);
void mi_launch_refit_level(const mi::GeoEditTables &, const uint32_t *, uint32_t, uint32_t, uint32_t, hipStream_t);
void mi_launch_instance_records(const mi::InstEditTables &, hipStream_t);
void mi_launch_adapt_tile(uint32_t *, mi_tile, uint32_t, uint32_t, hipStream_t);
void mi_launch_adapt_list(const uint32_t *, uint32_t, uint64_t, uint32_t, uint32_t, uint32_t *, hipStream_t);
void mi_launch_adapt_accumulate(const DScene &, const Queues &, const AdaptArgs &, const uint32_t *, uint32_t, uint32_t, float *, float *, hipStream_t);
void mi_launch_adapt_compact(const uint32_t *, uint32_t, const uint32_t *, uint32_t *, uint32_t *, uint32_t *, hipStream_t);
void mi_launch_dn_prepare_render(const DenoiseBufs &, const DenoiseFilmSrc &, float *, int, int, int, hipStream_t);
void mi_launch_dn_prepare_image(const DenoiseBufs &, const float *, const float *, const float *, const float *, int, int, int, hipStream_t);
void mi_launch_dn_bounds(const DenoiseBufs &, size_t, float, hipStream_t);
void mi_launch_dn_level(const DenoiseBufs &, int, const DenoiseLevel &, bool, float *, hipStream_t);
void mi_launch_tp_accumulate(const DenoiseBufs &, const TemporalSet &, const TemporalSet &, const TemporalFrame &, hipStream_t);
void mi_launch_tp_output(const DenoiseBufs &, float *, size_t, int, hipStream_t);
}

// Shading stage dispatch.  Dynamic LDS: Sobol nibble tables + (small scenes) the scene tables + (scenes with non-diffuse BSDFs) the per-wave path-order list.
// (Round 2 experiment, removed: two launches per bounce -- diffuse hits through the diffuse-only kernel, the rest through the full kernel -- measured SLOWER
// than one launch of the full kernel over the class-sorted list, 1579 vs 1675 Msamples/s on the Veach scene: a wave of diffuse hits already skips the other
// BSDFs' code at run time, and the stage runs at two waves per SIMD either way)
static bool mi_launch_shade(const DScene &scIn, bool ldsTables, const RenderConst &rc, const Queues &q, int buf, bool firstBounce, uint32_t grid, hipStream_t st, uint32_t *tableBytes = nullptr) {
    DScene sc = scIn; sc.small_tables = ldsTables ? 1u : 0u;
    size_t lds = rc.sampler == 1 ? (size_t) rc.nib_dims * rc.nib_count * 64 : 16;
    const bool env = sc.env_index >= 0;
    if (sc.small_tables) lds += 16 + 4 * ((size_t) sc.n_tris * (4 * MI_SHADE_WORDS) + sc.n_materials * 16 + sc.n_emitters * 12 + ((sc.n_emitters + 4) & ~3u) + sc.area_cdf_len);
    RenderConst rcl = rc; rcl.order_offset_words = 0; rcl.first_bounce = firstBounce ? 1u : 0u;
    if (tableBytes) *tableBytes = (uint32_t) lds;      // dynamic LDS in front of the order list (mi_render_debug_pool_info)
    if (sc.has_roughconductor && q.cap <= 8192u) {      // path-order list: only where it still fits the 64 KB a launch may request (else unsorted shading)
        const uint32_t off = (uint32_t) ((lds + 15) / 16 * 4); const size_t total = (size_t) off * 4 + (size_t) q.cap * 2 * 4 + 16;
        if (total <= 64 * 1024) { rcl.order_offset_words = off; lds = total; }
    }
    if (!sc.has_roughconductor) (env ? mi_launch_shade_d_env : mi_launch_shade_d)(sc, rcl, q, buf, grid, lds, st);
    else if (sc.has_adapters & 1u) (env ? mi_launch_shade_rcw_env : mi_launch_shade_rcw)(sc, rcl, q, buf, grid, lds, st);      // mixturebsdf / bumpmap / normalmap present
    else (env ? mi_launch_shade_rc_env : mi_launch_shade_rc)(sc, rcl, q, buf, grid, lds, st);
    return rcl.order_offset_words != 0 && q.cap <= 0xFFFFu;      // shade.h doSort: the segments were read through the class-sorted order list
}
// volpath_simple / volpath: the integrators whose stages walk media (kernels_vol.hip, kernels_volmis.hip); path and direct share the pool layout and the traversal stages
static inline bool isVolumetric(uint32_t integrator) { return integrator == MI_INTEGRATOR_VOLPATH_SIMPLE || integrator == MI_INTEGRATOR_VOLPATH; }
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(MI_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

static std::vector<uint32_t> g_sobolM32; static std::vector<uint64_t> g_sobolVdc, g_sobolVdcInv; static uint32_t g_sobolDims = 0;

// busy: renders executing on this scene (> 0), or an in-place update being applied (-1).  Updates are called between runs; the count turns a caller's mistake into an
// error instead of a table that changes under a running kernel.
struct mi_scene { mi::SceneHost h; std::atomic<int> busy{0}; };

struct mi_render {
    mi_scene *scene = nullptr; mi_render_params p{}; RenderConst rc{};
    DScene sc{};   // this render's view of the scene: the scene's record, with the triangle packet switched off for the volumetric integrators (their stages walk the tree, which every scene has)
    Queues q{}; std::vector<void *> allocs; uint64_t poolPaths = 0; uint32_t grid = 0, gridExtend = 0, gridShade = 0, gridShadow = 0;
    float *film = nullptr, *spill = nullptr; size_t filmFloats = 0; float *layoutTmp = nullptr, *mergeTmp = nullptr;   // mergeTmp: staging for another device's film (mi_render_merge_film)   // film: own-pixel sums; spill: cross-pixel splats (atomics)
    hipStream_t stream = nullptr; hipEvent_t evBegin = nullptr, evEnd = nullptr;
    std::atomic<int> cancel{0};
    bool profiling = false; std::vector<hipEvent_t> evPool; std::vector<int> evTag;   // tag: 0 generate/film, 1 extend, 2 shade, 3 shadow
    mi_stats stats{};
    uint64_t samplesTotal = 0, launchesAll = 0; uint64_t mergedRays = 0, mergedShadow = 0, mergedPathLen = 0, mergedSamples = 0;   // counters of replicas merged into this film
    uint32_t lastTableBytes = 0;   // dynamic LDS the last shade launch of the path integrator asked for in front of the order list
    bool lastSorted = false;  // the last shade launch read its segments through the class-sorted order list (mi_render_debug_pool_info)
    bool ldsTables = false;   // this render stages the scene tables in LDS (scene eligible and everything fits 64 KB together with the Sobol tables and the order list)
    uint32_t *pollHost = nullptr; size_t pollWords = 0; hipEvent_t pollEv = nullptr;   // unbounded depth: pinned landing buffer + event for the survivor-count poll
    uint32_t *dNib = nullptr; void *dSobolTabs = nullptr;   // dSobolTabs: the three look_up tables of k_generate (frame, px, py), one allocation
    // optional further path pools + streams: consecutive batches go round-robin through them, so the ALU-bound traversal kernels of one batch
    // overlap the latency-bound shading kernels of the others on the same CUs (MI355PT_STREAMS = 1..4 pools, default 2)
    enum { kMaxPools = 4 };
    Queues qx[kMaxPools - 1]{}; std::vector<void *> allocsx[kMaxPools - 1]; hipStream_t streamx[kMaxPools - 1] = {}; hipEvent_t filmDone[kMaxPools] = {}, joinEv[kMaxPools] = {}; int nStreams = 1;
    // field channels (mi_render_set_fields; kernels_field.hip): nothing below exists while nFields = 0.  fieldFilm / fieldSpill: 3 F + 1 SoA planes each; fieldDone[pool]: the
    // field kernel of the batch last traced on that pool has finished (chains consecutive batches across the streams, as filmDone chains k_film); lastFieldPool: pool of the previous batch of this run
    uint32_t nFields = 0; mi_field fields[MI_MAX_FIELDS] = {}; FieldArgs fa{}; float *fieldFilm = nullptr, *fieldSpill = nullptr, *fieldTmp = nullptr; size_t fieldFloats = 0; int32_t *dTriShape = nullptr;
    hipEvent_t fieldDone[kMaxPools] = {}; int lastFieldPool = -1; bool fieldChain = false;
    // direct integrator (direct.h): its constants, and per pool the hit array (+ instance indices) of the BSDF rays in buffer 1 -- Queues::hit keeps the camera hits for the whole batch
    DirectConst dc{}; float4 *hitB[kMaxPools] = {}; int32_t *hitInstB[kMaxPools] = {};
    AoConst ac{};   // ambient-occlusion integrator (ao.h): its constants; ray_length follows the scene under the automatic length (beginRun)
    // adaptive sampling (adaptive.h; mi_render_set_adaptive): nothing below is allocated before the first adaptive run.  adaptFilm: the film holds an adaptive run (weights of one
    // sample per pixel: no other run or merge may add to it).  adActive: the active list of this round and the next; adList[pool]: the triple list of the batch on that pool
    bool adaptOn = false, adaptFilm = false; mi_adaptive_params ap{}; mi_adaptive_stats as{}; AdaptArgs ad{}; float adQuantile = 0;
    uint32_t *adActive[2] = {}, *adWave = nullptr, *adNNext = nullptr, *adHostN = nullptr, *adList[kMaxPools] = {}; uint64_t adListPaths = 0; uint32_t adPix = 0;
    float *dnPprev = nullptr;   // H x W x 3: the developed prevPosition field, allocated by the first mi_render_denoise_temporal of a render that holds one
    void *dnMem = nullptr; DenoiseBufs dn{};   // denoiser scratch (denoise.h): two colour buffers + the packed guides, allocated at the first mi_render_denoise, freed with the render
    uint64_t sceneRev = 0, filmRev = 0;   // scene revision `sc` was copied from / the samples in the film (and the field film) were traced at
    Queues &pool(int i) { return i ? qx[i - 1] : q; }
    hipStream_t poolStream(int i) { return i ? streamx[i - 1] : stream; }
};

extern "C" {

const char *mi_last_error(void) { return g_err.c_str(); }

int mi_set_sobol_tables(const uint32_t *m32, uint32_t dims, const uint64_t *vdc, const uint64_t *vdcInv) {
    if (!m32 || !vdc || !vdcInv || dims < 2) return fail(MI_ERR_INVALID, "mi_set_sobol_tables: null table or dims < 2");
    g_sobolM32.assign(m32, m32 + (size_t) dims * MI_SOBOL_SIZE); g_sobolDims = dims;
    g_sobolVdc.assign(vdc, vdc + 16 * MI_SOBOL_SIZE); g_sobolVdcInv.assign(vdcInv, vdcInv + 16 * MI_SOBOL_SIZE);
    return MI_OK;
}

// Reads mitsuba-im_amd/data/sobol_tables.bin ("MISOBOL1", dims, rows, matrices32[dims][52], vdc[rows][52], vdc_inv[rows][52]).
int mi_load_sobol_tables(const char *path) {
    FILE *f = fopen(path, "rb"); if (!f) return fail(MI_ERR_INVALID, std::string("mi_load_sobol_tables: cannot open ") + path);
    char magic[8]; uint32_t hd[2]; bool ok = fread(magic, 1, 8, f) == 8 && !memcmp(magic, "MISOBOL1", 8) && fread(hd, 4, 2, f) == 2 && hd[1] == 16;
    std::vector<uint32_t> m32; std::vector<uint64_t> vdc, vdi;
    if (ok) { m32.resize((size_t) hd[0] * MI_SOBOL_SIZE); vdc.resize(16 * MI_SOBOL_SIZE); vdi.resize(16 * MI_SOBOL_SIZE);
              ok = fread(m32.data(), 4, m32.size(), f) == m32.size() && fread(vdc.data(), 8, vdc.size(), f) == vdc.size() && fread(vdi.data(), 8, vdi.size(), f) == vdi.size(); }
    fclose(f);
    if (!ok) return fail(MI_ERR_INVALID, std::string("mi_load_sobol_tables: malformed file ") + path);
    return mi_set_sobol_tables(m32.data(), hd[0], vdc.data(), vdi.data());
}
}  // extern "C"
#include <dlfcn.h>
// hosts that never call mi_set_sobol_tables (the adapter plugin): look for data/sobol_tables.bin next to this shared library
static void ensureSobolTables() {
    if (g_sobolDims) return;
    const char *env = getenv("MI355PT_DATA");
    if (env && mi_load_sobol_tables((std::string(env) + "/sobol_tables.bin").c_str()) == MI_OK) return;
    Dl_info info;
    if (dladdr((void *) &mi_set_sobol_tables, &info) && info.dli_fname) {
        std::string dir(info.dli_fname); size_t slash = dir.rfind('/'); dir = slash == std::string::npos ? "." : dir.substr(0, slash);
        (void) mi_load_sobol_tables((dir + "/data/sobol_tables.bin").c_str());
    }
}
extern "C" {

// ------------------------------------------------------------------------------------------------ scene
int mi_scene_create(mi_scene **out) { if (!out) return fail(MI_ERR_INVALID, "mi_scene_create: out is null"); *out = new mi_scene(); return MI_OK; }
void mi_scene_destroy(mi_scene *s) { delete s; }

int mi_scene_set_triangles(mi_scene *s, const float *pos, const float *nrm, const float *uv, const uint32_t *idx,
                           uint32_t nv, uint32_t nt, const mi_shape *shapes, uint32_t ns) {
    if (s && nt == 0 && ns == 0) { s->h.pos.clear(); s->h.idx.clear(); s->h.nrm.clear(); s->h.shapes.clear(); s->h.committed = false; return MI_OK; }   // analytic-only scene
    if (!s || !pos || !idx || !shapes || !ns) return fail(MI_ERR_INVALID, "mi_scene_set_triangles: null argument");
    for (uint32_t i = 0; i < ns; ++i) {
        const mi_shape &sh = shapes[i];
        if ((uint64_t) sh.first_tri + sh.tri_count > nt || (uint64_t) sh.first_vert + sh.vert_count > nv || sh.tri_count == 0)
            return fail(MI_ERR_INVALID, "mi_scene_set_triangles: shape range outside the arrays (or an empty mesh)");
    }
    for (uint64_t i = 0; i < (uint64_t) nt * 3; ++i) if (idx[i] >= nv) return fail(MI_ERR_INVALID, "mi_scene_set_triangles: vertex index out of range");
    s->h.pos.assign(pos, pos + (size_t) nv * 3); s->h.idx.assign(idx, idx + (size_t) nt * 3);
    if (nrm) s->h.nrm.assign(nrm, nrm + (size_t) nv * 3); else s->h.nrm.clear();
    if (uv) s->h.uv.assign(uv, uv + (size_t) nv * 2); else s->h.uv.clear();
    s->h.shapes.assign(shapes, shapes + ns); s->h.committed = false;
    return MI_OK;
}
int mi_scene_set_analytic(mi_scene *s, const mi_analytic *a, uint32_t n) {
    if (!s || (n && !a)) return fail(MI_ERR_INVALID, "mi_scene_set_analytic: null argument");
    for (uint32_t i = 0; i < n; ++i) {
        if (a[i].type > MI_SHAPE_CYLINDER) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_analytic: only rectangle, disk, sphere and cylinder are implemented");
        if (a[i].type >= MI_SHAPE_SPHERE && !(a[i].radius > 0)) return fail(MI_ERR_INVALID, "Cannot create spheres of radius <= 0");      // sphere.cpp:130-131
        if (a[i].type == MI_SHAPE_CYLINDER && !(a[i].length > 0)) return fail(MI_ERR_INVALID, "mi_scene_set_analytic: cylinder of length <= 0");
        if (a[i].to_world[12] != 0 || a[i].to_world[13] != 0 || a[i].to_world[14] != 0 || a[i].to_world[15] != 1.0f)
            return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_analytic: toWorld must be affine");
    }
    s->h.analytic.assign(a, a + n); s->h.committed = false; return MI_OK;
}
int mi_scene_set_textures(mi_scene *s, const mi_texture *t, uint32_t n) {
    if (!s || (n && !t)) return fail(MI_ERR_INVALID, "mi_scene_set_textures: null argument");
    for (uint32_t i = 0; i < n; ++i) {
        if (t[i].type > MI_TEXTURE_BITMAP) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_textures: implemented textures: checkerboard, gridtexture, bitmap");
        if (t[i].type == MI_TEXTURE_BITMAP && (t[i].wrap_u > 4 || t[i].wrap_v > 4 || t[i].filter > 3 || !t[i].n_levels)) return fail(MI_ERR_INVALID, "mi_scene_set_textures: bad wrap mode / filter type / level count");
    }
    s->h.textures.assign(t, t + n); s->h.committed = false; return MI_OK;
}
int mi_scene_set_texture_data(mi_scene *s, const uint32_t *levels, uint32_t nLevels, const float *texels, uint64_t nTexels) {
    if (!s || !levels || !texels || !nLevels || !nTexels) return fail(MI_ERR_INVALID, "mi_scene_set_texture_data: null argument");
    for (uint32_t i = 0; i < nLevels; ++i)
        if (!levels[i * 3] || !levels[i * 3 + 1] || (uint64_t) levels[i * 3 + 2] + (uint64_t) levels[i * 3] * levels[i * 3 + 1] * 3 > nTexels) return fail(MI_ERR_INVALID, "mi_scene_set_texture_data: MIP level outside the texel buffer");
    s->h.texLevels.assign(levels, levels + (size_t) nLevels * 3); s->h.texTexels.assign(texels, texels + nTexels); s->h.committed = false; return MI_OK;
}
int mi_scene_set_envmap_filter(mi_scene *s, int32_t texture) {
    if (!s) return fail(MI_ERR_INVALID, "mi_scene_set_envmap_filter: null argument");
    if (texture < -1) return fail(MI_ERR_INVALID, "mi_scene_set_envmap_filter: texture index must be >= -1");
    s->h.envTexture = texture; s->h.committed = false; return MI_OK;
}
int mi_scene_set_material_tables(mi_scene *s, const float *data, uint32_t n) {
    if (!s || (n && !data)) return fail(MI_ERR_INVALID, "mi_scene_set_material_tables: null argument");
    s->h.materialTables.assign(data, data + n); s->h.committed = false; return MI_OK;
}
int mi_scene_set_instances(mi_scene *s, const mi_instance *a, uint32_t n) {
    if (!s || (n && !a)) return fail(MI_ERR_INVALID, "mi_scene_set_instances: null argument");
    for (uint32_t i = 0; i < n; ++i)
        if (a[i].to_world[12] != 0 || a[i].to_world[13] != 0 || a[i].to_world[14] != 0 || a[i].to_world[15] != 1.0f) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_instances: toWorld must be affine");
    s->h.instances.assign(a, a + n); s->h.committed = false; return MI_OK;
}
int mi_scene_set_media(mi_scene *s, const mi_medium *media, uint32_t n, const int32_t *shapeMedia, uint32_t nPairs, int32_t sensorMedium) {
    if (!s || (n && (!media || !shapeMedia))) return fail(MI_ERR_INVALID, "mi_scene_set_media: null argument");
    if (n > 254) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_media: at most 254 media");
    for (uint32_t i = 0; i < n; ++i) {
        if (media[i].strategy > MI_MEDIUM_MANUAL) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_media: sampling strategies balance, single and manual are implemented (not `maximum`)");   // homogeneous.cpp:192-226
        if (media[i].phase > MI_PHASE_HG) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_media: phase functions isotropic and hg are implemented");
        if (media[i].phase == MI_PHASE_HG && !(media[i].g > -1 && media[i].g < 1)) return fail(MI_ERR_INVALID, "The anisotropy parameter 'g' must be in the range (-1, 1)!");   // hg.cpp:50-51
        for (int c = 0; c < 3; ++c) if (!(media[i].sigma_a[c] >= 0) || !(media[i].sigma_s[c] >= 0)) return fail(MI_ERR_INVALID, "mi_scene_set_media: negative coefficient");
    }
    for (uint32_t i = 0; i < nPairs * 2u; ++i) if (shapeMedia[i] < -1 || shapeMedia[i] >= (int32_t) n) return fail(MI_ERR_INVALID, "mi_scene_set_media: a shape refers to a missing medium");
    if (sensorMedium < -1 || sensorMedium >= (int32_t) n) return fail(MI_ERR_INVALID, "mi_scene_set_media: the sensor refers to a missing medium");
    s->h.media.assign(media, media + n); s->h.shapeMedia.assign(shapeMedia, shapeMedia + (size_t) nPairs * 2u); s->h.sensorMedium = sensorMedium; s->h.committed = false; return MI_OK;
}
int mi_scene_set_materials(mi_scene *s, const mi_material *m, uint32_t n) {
    if (!s || !m || !n) return fail(MI_ERR_INVALID, "mi_scene_set_materials: null argument");
    { std::string msg; const int rc = mi::validateMaterials(m, n, msg); if (rc) return fail(rc, msg); }
    s->h.materials.assign(m, m + n); s->h.committed = false; return MI_OK;
}
int mi_scene_set_emitters(mi_scene *s, const mi_emitter *e, uint32_t n) {
    if (!s || (n && !e)) return fail(MI_ERR_INVALID, "mi_scene_set_emitters: null argument");
    { std::string msg; const int rc = mi::validateEmitters(e, n, msg); if (rc) return fail(rc, msg); }
    s->h.emitters.assign(e, e + n); s->h.committed = false; return MI_OK;
}
int mi_scene_set_envmap(mi_scene *s, const float *rgb, uint32_t w, uint32_t h, const float *toWorld, float scale) {
    if (!s || !rgb || !toWorld || w < 2 || h < 2 || w > 0xFFFF || h > 0xFFFF) return fail(MI_ERR_INVALID, "mi_scene_set_envmap: bad argument (2..65535 texels per side)");
    s->h.envRGB.assign(rgb, rgb + (size_t) w * h * 3); s->h.envW = w; s->h.envH = h; memcpy(s->h.envToWorld, toWorld, 64); s->h.envScale = scale; s->h.committed = false;
    return MI_OK;
}
int mi_scene_set_camera(mi_scene *s, const float *s2c, const float *c2w, float nearClip, float farClip) {
    if (!s || !s2c || !c2w) return fail(MI_ERR_INVALID, "mi_scene_set_camera: null argument");
    memcpy(s->h.s2c, s2c, 64); memcpy(s->h.c2w, c2w, 64); s->h.nearClip = nearClip; s->h.farClip = farClip; s->h.haveCamera = true; s->h.committed = false;
    return MI_OK;
}
int mi_scene_set_lens(mi_scene *s, float apertureRadius, float focusDistance) {
    if (!s) return fail(MI_ERR_INVALID, "mi_scene_set_lens: null scene");
    std::string msg; if (const int rc = mi::validateLens("mi_scene_set_lens", apertureRadius, focusDistance, msg)) return fail(rc, msg);
    s->h.lensRadius = apertureRadius; s->h.focusDistance = apertureRadius != 0.0f ? focusDistance : 0.0f; s->h.committed = false;
    return MI_OK;
}
int mi_scene_set_film(mi_scene *s, uint32_t w, uint32_t h, uint32_t kind, float radius, float stddev) {
    if (!s || !w || !h || kind > 5 || (kind == 5 && !(radius >= 1))) return fail(MI_ERR_INVALID, "mi_scene_set_film: bad argument");
    s->h.width = w; s->h.height = h; s->h.filterKind = kind; s->h.filterRadius = radius; s->h.filterStddev = stddev; s->h.haveFilm = true; s->h.committed = false;
    return MI_OK;
}

}  // extern "C"

namespace mi {
static int bvhDepthOf(const std::vector<BvhNode> &nodes, int n) {
    if (n < 0) return 0;
    int a = bvhDepthOf(nodes, nodes[n].c0), b = bvhDepthOf(nodes, nodes[n].c1);
    return 1 + (a > b ? a : b);
}
template <typename T> static int up(void **dst, const std::vector<T> &v) {
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    hipError_t e = hipMalloc(dst, bytes); if (e != hipSuccess) return 1;
    if (!v.empty()) { e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); if (e != hipSuccess) return 1; }
    return 0;
}
void SceneHost::release() {
    eachDevicePointer([](void *&p) { if (p) { (void) hipFree(p); p = nullptr; } });
}
int SceneHost::allocMark() {
    auto raw = [](void **p, size_t bytes) { if (*p) return 0; if (hipMalloc(p, std::max<size_t>(bytes, 16)) != hipSuccess) { *p = nullptr; return 1; } return 0; };
    return raw(&dPrevPos, pos.size() * 4) | raw(&dPrevInst, instances.size() * 48);
}
int SceneHost::uploadMark() {
    if (allocMark()) return 1;
    if (!prevPos.empty() && hipMemcpy(dPrevPos, prevPos.data(), prevPos.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
    if (!prevInstXf.empty() && hipMemcpy(dPrevInst, prevInstXf.data(), prevInstXf.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
    return 0;
}
int SceneHost::upload(int dev) {
    release(); device = dev;
    if (hipSetDevice(dev) != hipSuccess) return 1;
    const std::vector<MaterialD> &mats = materialsD;      // buildMaterialTables() (scene_build.cpp), shared with mi_scene_update_materials
    std::vector<float> filt(filterValues, filterValues + MI_FILTER_RES + 1);
    // tree nodes and leaf records share ONE allocation (nodes first): the fused walk (trace_fused.h) addresses both through one base + a 32-bit byte offset
    std::vector<unsigned char> geo(nodes.size() * sizeof(BvhNode) + std::max<size_t>(tris.size(), 1) * sizeof(TriAccelD) + 16);
    if (!nodes.empty()) std::memcpy(geo.data(), nodes.data(), nodes.size() * sizeof(BvhNode));
    if (!tris.empty()) std::memcpy(geo.data() + nodes.size() * sizeof(BvhNode), tris.data(), tris.size() * sizeof(TriAccelD));
    dTris = nullptr;
    int bad = up(&dNodes, geo) | up(&dShade, shade) | up(&dI2, i2) | up(&dNrm, nrm) | up(&dMaterials, mats) |
              up(&dEmitters, emittersD) | up(&dAnalytic, analyticD) | up(&dInstances, instancesD) | up(&dMaterialTables, materialTables) | up(&dTriUV, triuv) | up(&dTextures, textures) | up(&dEmitterX, emitterX) | up(&dEmitterCdf, emitterCdf) | up(&dAreaCdf, areaCdf) | up(&dFilter, filt) | up(&dMaterialFlags, materialFlagTable);
    if (bad) return 1;
    d = DScene{};
    if (g_sobolDims && logRes <= 16) {
        const uint32_t row = logRes >= 1 ? logRes - 1 : 0;   // look_up is only used for logRes > 1 (sobol.cpp:209-215)
        std::vector<uint64_t> vdc(g_sobolVdc.begin() + row * MI_SOBOL_SIZE, g_sobolVdc.begin() + (row + 1) * MI_SOBOL_SIZE);
        std::vector<uint64_t> vdi(g_sobolVdcInv.begin() + row * MI_SOBOL_SIZE, g_sobolVdcInv.begin() + (row + 1) * MI_SOBOL_SIZE);
        if (up(&dSobolM32, g_sobolM32) | up(&dSobolVdc, vdc) | up(&dSobolVdcInv, vdi)) return 1;
        d.sobol_m32 = (const uint32_t *) dSobolM32; d.sobol_vdc = (const uint64_t *) dSobolVdc; d.sobol_vdc_inv = (const uint64_t *) dSobolVdcInv;
        d.sobol_dims = g_sobolDims;
    }
    d.nodes = (const BvhNode *) dNodes; d.tris = (const TriAccelD *) ((const unsigned char *) dNodes + nodes.size() * sizeof(BvhNode)); d.geo_bytes = geo.size(); d.shade = (const TriShade *) dShade; d.i2 = (const uint32_t *) dI2;
    d.nrm = (const float *) dNrm; d.materials = (const MaterialD *) dMaterials; d.emitters = (const EmitterD *) dEmitters;
    d.emitter_cdf = (const float *) dEmitterCdf; d.area_cdf = (const float *) dAreaCdf; d.filter_values = (const float *) dFilter;
    d.analytic = (const AnalyticD *) dAnalytic; d.n_analytic = (uint32_t) analyticD.size();
    {   // EWA weight table (mipmap.h:297-302; math::fastexp on Linux/x86_64 = (float) exp((double) x))
        std::vector<float> lut(64); for (int i = 0; i < 64; ++i) { float r2 = (float) i / 63.0f; lut[i] = (float) std::exp((double) (-2.0f * r2)) - (float) std::exp((double) -2.0f); }
        if (up(&dTexLevels, texLevels) | up(&dTexTexels, texTexels) | up(&dMipLut, lut)) return 1;
        d.tex_levels = (const uint32_t *) dTexLevels; d.tex_texels = (const float *) dTexTexels; d.mip_lut = (const float *) dMipLut;
    }
    d.material_tables = (const float *) dMaterialTables; d.triuv = (const TriUV *) dTriUV; d.textures = (const TextureD *) dTextures;
    bool matTextures = false; for (const auto &m : mats) if ((m.flags >> 8) & 0xFFFFu) matTextures = true;
    d.n_textures = matTextures ? (uint32_t) textures.size() : 0u; d.env_texture = envTexture >= 0 ? (uint32_t) envTexture + 1u : 0u;
    d.instances = (const InstanceD *) dInstances; d.n_instances = (uint32_t) instancesD.size();
    d.emitter_x = (const float *) dEmitterX; d.env_constant = envConstant ? 1u : 0u; d.ext = (!analyticD.empty() || !instancesD.empty() || hasDeltaEmitters || anyUV || matTextures) ? 1u : 0u;
    d.n_tris = nTris; d.n_nodes = (uint32_t) nodes.size(); d.n_emitters = (uint32_t) emittersD.size(); d.n_materials = (uint32_t) mats.size();
    syncEmittersD();
    for (int i = 0; i < 3; ++i) { d.aabb_lo[i] = aabbLo[i]; d.aabb_hi[i] = aabbHi[i]; }
    syncCameraD();      // camera matrices, clip planes, pixel differentials, bounding spheres
    d.inv_res_x = 1.0f / (float) width; d.inv_res_y = 1.0f / (float) height;
    d.width = width; d.height = height;
    d.filter_radius = filterRadiusEff; d.filter_scale = filterScale; d.border = border;
    d.log_res = logRes; d.resolution = resolution;
    d.env_index = envIndex;
    if (envIndex >= 0 && !envConstant) {
        if (up(&dEnvRGB, envRGB) | up(&dEnvCols, envCdfCols) | up(&dEnvRows, envCdfRows) | up(&dEnvWeights, envRowWeights)) return 1;
        if (!envGuideRows.empty()) { if (up(&dEnvGuideRows, envGuideRows) | up(&dEnvGuideCols, envGuideCols)) return 1;
            d.env_guide_rows_t = (const uint16_t *) dEnvGuideRows; d.env_guide_cols_t = (const uint16_t *) dEnvGuideCols; d.env_guide_rows = envGuideKR; d.env_guide_cols = envGuideKC; }
        d.env_rgb = (const float *) dEnvRGB; d.env_cdf_cols = (const float *) dEnvCols; d.env_cdf_rows = (const float *) dEnvRows; d.env_row_weights = (const float *) dEnvWeights;
        d.env_w = (int) envW; d.env_h = (int) envH; d.env_normalization = envNormalization;
        d.env_pixel_w = 2 * MI_PI / (float) envW; d.env_pixel_h = MI_PI / (float) envH;
        syncEnvD();
    }
    d.bvh_depth = (uint32_t) bvhDepth; d.bvh_wide = wideBvh ? 1u : 0u; d.bvh_stack_direct = (uint32_t) bvhStackDirect;
    d.area_cdf_len = (uint32_t) areaCdf.size();
    { uint32_t maxLightTris = 0; for (const EmitterD &e : emittersD) if (e.tri_count > maxLightTris) maxLightTris = e.tri_count;
      const char *sf = getenv("MI355PT_SEARCH"); d.search_flags = sf ? (uint32_t) atoi(sf) : ((emittersD.size() <= 3 ? 1u : 0u) | (maxLightTris <= 3u ? 2u : 0u)); }
    { const char *ns = getenv("MI355PT_NO_LDS_TABLES");
      d.small_tables = (nTris <= 400 && mats.size() <= 64 && emittersD.size() <= 32 && areaCdf.size() <= 2048 && !(ns && ns[0] == '1')) ? 1u : 0u; }   // ELIGIBLE for LDS staging; mi_render_create decides per render whether it fits next to the Sobol tables
    d.has_roughconductor = 0; d.has_diffuse = 0;
    d.has_adapters = 0;
    for (const mi_material &m : materials) { if (m.type != MI_BSDF_DIFFUSE) d.has_roughconductor = 1; else d.has_diffuse = 1; if (m.type == MI_BSDF_MIXTURE || m.type == MI_BSDF_BUMPMAP || m.type == MI_BSDF_NORMALMAP || m.type == MI_BSDF_COATING || m.type == MI_BSDF_ROUGHCOATING) d.has_adapters |= 1u; if (m.type == MI_BSDF_COATING || m.type == MI_BSDF_BLEND || m.type == MI_BSDF_ROUGHCOATING) d.has_adapters |= 4u; if (m.type == MI_BSDF_BLEND) d.has_adapters |= 1u; }   // any non-diffuse material -> k_shade<RC = true>; both kinds -> two shading launches per bounce (class split)
    // bit 1: ENull lobes the volumetric walks have to evaluate through a wrapper -- a `mask`, or a mixturebsdf with a `null` / `thindielectric` child (surfaceNullEval; the NX kernel variants)
    for (const mi_material &m : materials) {
        if (m.type == MI_BSDF_MASK) d.has_adapters |= 2u;
        if (m.type == MI_BSDF_MIXTURE) for (uint32_t c = 0; c < m.distr && c < 4; ++c) { const uint32_t ci = (uint32_t) (c < 3 ? m.reflectance[c] : m.eta[0]); if (ci < materials.size() && (materials[ci].type == MI_BSDF_NULL || materials[ci].type == MI_BSDF_THINDIELECTRIC)) d.has_adapters |= 2u; }
    }
    const char *noPacket = getenv("MI355PT_NO_PACKET");
    d.packet_n = (nTris <= MI_PACKET_MAX && analyticD.size() <= MI_ANALYTIC_PACKET_MAX && instancesD.empty() && media.empty() && !(noPacket && noPacket[0] == '1')) ? (uint32_t) tris.size() : 0;   // used as a flag
    if (up(&dPacketGroups, packetGroups) | up(&dPacketExact, packetExact)) return 1;
    // participating media: scenes that carry them always walk the tree (the transmittance walk of the volumetric shadow stage is a closest-hit traversal)
    if (!media.empty()) { if (up(&dMedia, mediaD) | up(&dPrimMedia, primMedia)) return 1; }
    d.media = (const MediumD *) dMedia; d.prim_media = (const uint32_t *) dPrimMedia; d.n_media = (uint32_t) mediaD.size(); d.sensor_medium = media.empty() ? -1 : sensorMedium;
    d.packet_groups = (const PacketGroupD *) dPacketGroups; d.packet_exact = (const TriAccelD *) dPacketExact; d.packet_scale = packetScale;
    for (int i = 0; i < 3; ++i) d.packet_gk[i] = packetGK[i];
    committed = true;
    return 0;
}
}  // namespace mi

extern "C" {

int mi_scene_commit(mi_scene *s, uint32_t device) {
    if (!s) return fail(MI_ERR_INVALID, "mi_scene_commit: null scene");
    if ((s->h.idx.empty() && s->h.analytic.empty()) || s->h.materials.empty() || !s->h.haveCamera || !s->h.haveFilm)
        return fail(MI_ERR_INVALID, "mi_scene_commit: geometry (triangles and / or analytic shapes), materials, camera and film must be set first");
    {   uint32_t ng = 0; for (const mi_shape &sh : s->h.shapes) ng = std::max(ng, sh.group);
        for (const mi_shape &sh : s->h.shapes) if (sh.group && sh.emitter >= 0) return fail(MI_ERR_INVALID, "Instancing of emitters is not supported");   // shapegroup.cpp:75-76
        for (const mi_instance &in : s->h.instances) if (in.group >= ng) return fail(MI_ERR_INVALID, "A reference to a 'shapegroup' must be specified!");   // instance.cpp:41-44
    }
    for (const mi_material &m : s->h.materials) {
        const uint32_t tex = (m.flags >> 8) & 0xFFFFu;
        if (tex && tex <= s->h.textures.size() && s->h.textures[tex - 1].type == MI_TEXTURE_BITMAP &&
            (size_t) s->h.textures[tex - 1].first_level + s->h.textures[tex - 1].n_levels > s->h.texLevels.size() / 3) return fail(MI_ERR_INVALID, "mi_scene_commit: bitmap texture without its MIP levels (mi_scene_set_texture_data)");
        if (tex && (tex > s->h.textures.size() || (m.type != MI_BSDF_DIFFUSE && m.type != MI_BSDF_ROUGHDIFFUSE && m.type != MI_BSDF_PLASTIC && m.type != MI_BSDF_ROUGHPLASTIC && m.type != MI_BSDF_DIFFTRANS && m.type != MI_BSDF_MASK && m.type != MI_BSDF_BLEND && m.type != MI_BSDF_BUMPMAP && m.type != MI_BSDF_NORMALMAP)))
            return fail(MI_ERR_UNSUPPORTED, "mi_scene_commit: textures bind to diffuse.reflectance, plastic / roughplastic.diffuseReflectance, difftrans.transmittance, mask.opacity or are the map of a bumpmap / normalmap (and must exist)");
    }
    if (s->h.envTexture >= 0) {       // MIP pyramid of the environment map (camera-ray lookups, envmap.cpp:398-411)
        if (!s->h.envW) return fail(MI_ERR_INVALID, "mi_scene_commit: mi_scene_set_envmap_filter without an environment map");
        if ((size_t) s->h.envTexture >= s->h.textures.size()) return fail(MI_ERR_INVALID, "mi_scene_commit: mi_scene_set_envmap_filter refers to a missing texture record");
        const mi_texture &t = s->h.textures[s->h.envTexture];
        if (t.type != MI_TEXTURE_BITMAP || (size_t) t.first_level + t.n_levels > s->h.texLevels.size() / 3 || s->h.texLevels[(size_t) t.first_level * 3] != s->h.envW || s->h.texLevels[(size_t) t.first_level * 3 + 1] != s->h.envH)
            return fail(MI_ERR_INVALID, "mi_scene_commit: the environment map's pyramid must be a bitmap texture record whose level 0 has the map's size");
    }
    auto wantsTangents = [&](int32_t b) {          // anisotropic roughness, or a bumpmap / normalmap anywhere under the shape's material (their components are EAnisotropic, bumpmap.cpp:99-100)
        if (b < 0 || (size_t) b >= s->h.materials.size()) return false;
        const mi_material *mm = &s->h.materials[b];
        if (mm->type == MI_BSDF_MASK && mm->distr < s->h.materials.size()) mm = &s->h.materials[mm->distr];
        if ((mm->type == MI_BSDF_COATING || mm->type == MI_BSDF_ROUGHCOATING) && mm->distr < s->h.materials.size()) mm = &s->h.materials[mm->distr];
        return (mm->flags & MI_BSDF_FLAG_ANISOTROPIC) != 0 || mm->type == MI_BSDF_BUMPMAP || mm->type == MI_BSDF_NORMALMAP;
    };
    for (const mi_shape &sh : s->h.shapes)         // TriMesh::computeUVTangents (trimesh.cpp:683-692): such BSDFs take their tangents from the texture coordinates
        if (wantsTangents(sh.bsdf) && !((sh.flags & 2u) && !s->h.uv.empty()))
            return fail(MI_ERR_INVALID, "computeUVTangents(): texture coordinates are required to generate tangent vectors. If you want to render with an anisotropic material, please make sure that all associated shapes have valid texture coordinates.");
    for (const mi_material &m : s->h.materials)
        if ((m.type == MI_BSDF_ROUGHPLASTIC || m.type == MI_BSDF_ROUGHCOATING) && (m.k[2] < 2 || m.k[1] < 0 || (size_t) m.k[1] + (size_t) m.k[2] > s->h.materialTables.size()))
            return fail(MI_ERR_INVALID, "mi_scene_commit: roughplastic material without its rough-transmittance slice (mi_scene_set_material_tables)");
    for (const mi_analytic &a : s->h.analytic) {
        if (a.bsdf < 0 || (size_t) a.bsdf >= s->h.materials.size()) return fail(MI_ERR_INVALID, "mi_scene_commit: analytic shape refers to a missing material");
        if (a.emitter >= (int32_t) s->h.emitters.size()) return fail(MI_ERR_INVALID, "mi_scene_commit: analytic shape refers to a missing emitter");
    }
    for (const mi_shape &sh : s->h.shapes) {
        if (sh.bsdf < 0 || (size_t) sh.bsdf >= s->h.materials.size()) return fail(MI_ERR_INVALID, "mi_scene_commit: shape refers to a missing material");
        if (sh.emitter >= (int32_t) s->h.emitters.size()) return fail(MI_ERR_INVALID, "mi_scene_commit: shape refers to a missing emitter");
        if (!(sh.flags & 1u) && s->h.nrm.empty()) return fail(MI_ERR_INVALID, "mi_scene_commit: smooth-shaded mesh without vertex normals (pass faceNormals or normals)");
    }
    for (const mi_emitter &e : s->h.emitters) {
        if (e.type == MI_EMITTER_AREA && (e.shape < 0 || (size_t) e.shape >= s->h.shapes.size() + s->h.analytic.size())) return fail(MI_ERR_INVALID, "mi_scene_commit: area emitter without a shape");
        if (e.type == MI_EMITTER_ENVMAP && s->h.envRGB.empty()) return fail(MI_ERR_INVALID, "mi_scene_commit: envmap emitter listed but mi_scene_set_envmap was not called");
    }
    if (!s->h.media.empty()) {
        if (s->h.shapeMedia.size() != (s->h.shapes.size() + s->h.analytic.size()) * 2u) return fail(MI_ERR_INVALID, "mi_scene_commit: mi_scene_set_media needs one (interior, exterior) pair per mesh and per analytic shape");
        for (size_t i = 0; i < s->h.shapes.size(); ++i)
            if (s->h.shapes[i].group && (s->h.shapeMedia[i * 2] >= 0 || s->h.shapeMedia[i * 2 + 1] >= 0)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_commit: media on the members of a shape group are not implemented");
    }
    if (s->h.emitters.empty()) return fail(MI_ERR_UNSUPPORTED, "mi_scene_commit: scene without emitters (the reference would add a sunsky emitter)");
    ensureSobolTables();
    s->h.marked = false; s->h.prevPos.clear(); s->h.prevInstXf.clear();      // a commit rebuilds the scene: previous = current until the next mi_scene_mark_frame (upload() frees the tables)
    s->h.commitHost();
    if (s->h.bvhDepth > 32) return fail(MI_ERR_UNSUPPORTED, "mi_scene_commit: BVH deeper than the traversal stack (32)");
    if (s->h.wideBvh && s->h.nodes.size() >= (1u << 23)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_commit: more than 2^23 BVH nodes");
    if (getenv("MI355PT_VERBOSE")) fprintf(stderr, "[mi355pt] %zu triangles, %zu analytic shapes, %zu instances, %zu BVH nodes, depth %d\n", s->h.idx.size() / 3, s->h.analytic.size(), s->h.instances.size(), s->h.nodes.size(), s->h.bvhDepth);
    int devCount = 0; HIPCHK(hipGetDeviceCount(&devCount));
    if ((int) device >= devCount) return fail(MI_ERR_DEVICE, "mi_scene_commit: no such HIP device");
    if (s->h.upload((int) device)) return fail(MI_ERR_DEVICE, std::string("mi_scene_commit: upload failed: ") + hipGetErrorString(hipGetLastError()));
    return MI_OK;
}

// A replica of a committed scene on another (or the same) HIP device: multi-device renders hold one full scene copy per device (the reference ships the
// serialized scene to every worker, src/librender/renderjob.cpp + sched_remote.cpp).  The host-side build (BVH, tables) is reused, only the upload is repeated.
int mi_scene_clone(mi_scene *s, uint32_t device, mi_scene **out) {
    if (!s || !out) return fail(MI_ERR_INVALID, "mi_scene_clone: null argument");
    if (!s->h.committed) return fail(MI_ERR_INVALID, "mi_scene_clone: scene not committed");
    int devCount = 0; HIPCHK(hipGetDeviceCount(&devCount));
    if ((int) device >= devCount) return fail(MI_ERR_DEVICE, "mi_scene_clone: no such HIP device");
    s->h.refreshHostGeometry();                     // after vertex / instance edits the per-triangle mirrors, the instance records and the nodes are brought up to date only when someone reads them
    mi_scene *c = new mi_scene();
    c->h = s->h;                                    // inputs + host-derived data
    {   // the copy must not own the source's device allocations
        c->h.eachDevicePointer([](void *&p) { p = nullptr; });
        c->h.committed = false;
    }
    if (c->h.upload((int) device) || (c->h.marked && c->h.uploadMark())) { std::string msg = std::string("mi_scene_clone: upload failed: ") + hipGetErrorString(hipGetLastError()); delete c; return fail(MI_ERR_DEVICE, msg); }      // the replica carries the frame mark
    *out = c; return MI_OK;
}

// ------------------------------------------------------------------------------------------------ in-place edits (SceneHost::update*, scene_build.cpp)
// The host side recomputes what commitHost() / upload() derive from the edited inputs; here the small tables go back into their EXISTING allocations (the record counts
// cannot change, so every size is the one upload() allocated) and, when a material's flag bits moved, one kernel rewrites those bits in the triangle records.
struct UpdateGuard {
    mi_scene *s = nullptr;
    bool enter(mi_scene *sc) { int v = 0; if (!sc->busy.compare_exchange_strong(v, -1)) return false; s = sc; return true; }
    ~UpdateGuard() { if (s) s->busy.store(0); }
};
}  // extern "C"
template <typename T> static hipError_t push(void *dst, const std::vector<T> &v) { return v.empty() || !dst ? hipSuccess : hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); }
extern "C" {
#define UPDATE_ENTER(name) \
    if (!s) return fail(MI_ERR_INVALID, std::string(name) + ": null scene"); \
    if (!s->h.committed) return fail(MI_ERR_INVALID, std::string(name) + ": scene not committed (an update edits a committed scene in place)"); \
    UpdateGuard updating; if (!updating.enter(s)) return fail(MI_ERR_INVALID, std::string(name) + ": a render is running on this scene (cancel it and wait for the run to return)")

int mi_scene_update_camera(mi_scene *s, const float *s2c, const float *c2w, float nearClip, float farClip) {
    if (!s || !s2c || !c2w) return fail(MI_ERR_INVALID, "mi_scene_update_camera: null argument");
    UPDATE_ENTER("mi_scene_update_camera");
    std::string msg; const int rc = s->h.updateCamera(s2c, c2w, nearClip, farClip, msg); if (rc) return fail(rc, msg);
    return MI_OK;      // the camera lives in the scene record alone: renders pick it up with their next run
}
int mi_scene_update_lens(mi_scene *s, float apertureRadius, float focusDistance) {
    if (!s) return fail(MI_ERR_INVALID, "mi_scene_update_lens: null scene");
    std::string msg; if (const int bad = mi::validateLens("mi_scene_update_lens", apertureRadius, focusDistance, msg)) return fail(bad, msg);      // value checks first: they need no scene state
    UPDATE_ENTER("mi_scene_update_lens");
    const int rc = s->h.updateLens(apertureRadius, focusDistance, msg); if (rc) return fail(rc, msg);
    return MI_OK;      // like the camera, the lens lives in the scene record alone
}
int mi_scene_update_materials(mi_scene *s, const mi_material *m, uint32_t n) {
    if (!s || !m || !n) return fail(MI_ERR_INVALID, "mi_scene_update_materials: null argument");
    UPDATE_ENTER("mi_scene_update_materials");
    mi::SceneHost &h = s->h; bool flagsChanged = false;
    std::string msg; const int rc = h.updateMaterials(m, n, msg, &flagsChanged); if (rc) return fail(rc, msg);
    if (h.materialsD.size() != h.d.n_materials || h.analyticD.size() != h.d.n_analytic || h.shade.size() != h.d.n_tris) return fail(MI_ERR_DEVICE, "mi_scene_update_materials: host tables and device tables disagree in size");
    HIPCHK(hipSetDevice(h.device));
    HIPCHK(push(h.dMaterials, h.materialsD));
    if (flagsChanged) {
        HIPCHK(push(h.dMaterialFlags, h.materialFlagTable)); HIPCHK(push(h.dAnalytic, h.analyticD));
        if (h.d.n_tris) { mi_launch_patch_material_flags((TriShade *) h.dShade, h.d.n_tris, (const uint32_t *) h.dMaterialFlags, h.d.n_materials, nullptr); HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(nullptr)); }
    }
    return MI_OK;
}
int mi_scene_update_emitters(mi_scene *s, const mi_emitter *e, uint32_t n) {
    if (!s || !e || !n) return fail(MI_ERR_INVALID, "mi_scene_update_emitters: null argument");
    UPDATE_ENTER("mi_scene_update_emitters");
    mi::SceneHost &h = s->h; const size_t cdfLen = h.areaCdf.size();
    std::string msg; const int rc = h.updateEmitters(e, n, msg); if (rc) return fail(rc, msg);
    if (h.emittersD.size() != h.d.n_emitters || h.areaCdf.size() != cdfLen) return fail(MI_ERR_DEVICE, "mi_scene_update_emitters: host tables and device tables disagree in size");
    HIPCHK(hipSetDevice(h.device));
    HIPCHK(push(h.dEmitters, h.emittersD)); HIPCHK(push(h.dEmitterCdf, h.emitterCdf)); HIPCHK(push(h.dEmitterX, h.emitterX));      // the area CDFs depend on geometry only
    return MI_OK;
}
int mi_scene_update_envmap_transform(mi_scene *s, const float *toWorld, float scale) {
    if (!s || !toWorld) return fail(MI_ERR_INVALID, "mi_scene_update_envmap_transform: null argument");
    UPDATE_ENTER("mi_scene_update_envmap_transform");
    std::string msg; const int rc = s->h.updateEnvmapTransform(toWorld, scale, msg); if (rc) return fail(rc, msg);
    return MI_OK;
}
// Geometry edit: one frame of an animation -- vertices (shape-group members included) and / or instance transforms; mi_scene_update_vertices and _instances are this
// chain under their own names and refusals.  Host: the checks, pos / nrm / instances, the group boxes, the scene box and what depends on it (SceneHost::applyGeometry).
// Device, one chain on the null stream: the inputs go up (vertex arrays and group boxes when vertices are given, transform pairs on a scene with instances),
// k_tri_records rewrites every per-triangle record and leaf box, k_instance_records takes the group boxes into InstanceD::glo / ghi and rewrites matrices and
// instance leaf boxes, k_refit refits level by level -- every tree when vertices moved (nodes of equal height of all trees share a launch), the scene level alone
// otherwise (the group trees are not reachable from node 0 and stay) -- and the small tables that follow the vertices go back into their allocations (the packet
// groups into a new one when their count grew).  Synchronous like the other updates.
static int updateGeometryOnDevice(mi::GeoEntry entry, mi_scene *s, const float *pos, const float *nrm, uint32_t nVerts, const mi_instance *instances, uint32_t nInstances) {
    const std::string name = mi::geoEntryName(entry); const bool moved = pos != nullptr;      // vertices given
    UPDATE_ENTER(name);
    mi::SceneHost &h = s->h; const size_t cdfLen = h.areaCdf.size(), nGroups = h.packetGroups.size();
    std::string msg; const int rc = h.checkGeometry(entry, pos, nrm, nVerts, instances, nInstances, msg); if (rc) return fail(rc, msg);
    if (!h.geoPrepared) h.prepareGeometryEdit();      // derived from the committed topology alone: the scene itself is not changed yet
    const uint32_t ni = (uint32_t) h.instances.size(), ng = (uint32_t) (h.groupBoxes.size() / 6);
    if (h.shade.size() != h.d.n_tris || h.nodes.size() != h.d.n_nodes || h.leafSlotOfPrim.size() != h.d.n_tris || h.instancesD.size() != h.d.n_instances || ni != h.d.n_instances || h.leafSlotOfInstance.size() != ni ||
        h.leafBoxes.size() != h.tris.size() * 6 || h.nodeBoxes.size() != h.nodes.size() * 6 || h.refitOrder.size() > h.nodes.size() || h.refitOrderAll.size() > h.nodes.size())
        return fail(MI_ERR_DEVICE, name + ": host tables and device tables disagree in size");
    for (uint32_t slot : h.leafSlotOfInstance) if (slot >= h.tris.size()) return fail(MI_ERR_DEVICE, name + ": host tables and device tables disagree in size");
    if (moved) for (const InstanceD &in : h.instancesD) if (in.group >= ng) return fail(MI_ERR_DEVICE, name + ": host tables and device tables disagree in size");      // the group boxes are indexed by it
    // one slot per triangle (a megabyte on a large mesh, cold in every call): checked when the table goes up.  The kernel reads the device copy, made once below from a
    // table that only prepareGeometryEdit() writes
    if (moved && !h.dLeafSlot) for (uint32_t slot : h.leafSlotOfPrim) if (slot >= h.tris.size()) return fail(MI_ERR_DEVICE, name + ": host tables and device tables disagree in size");
    HIPCHK(hipSetDevice(h.device));
    {   // The tables a commit does not need: each is allocated by the first edit that uses it, before the scene changes, and only when it is MISSING.  All but one are
        // staging space or copies of what prepareGeometryEdit() derived from the topology.  The one rule: the device's leaf boxes are newer than the mirror (stale from
        // the first edit until refreshHostGeometry()); never upload them twice.  A leaf-box table that does not exist yet means that no edit has run on this handle, so
        // the mirror is current.  dNodeBox stays uninitialised: a node's box is written by the refit of its level before any higher level reads it.
        std::vector<void **> mine; bool bad = false;
        auto raw = [&](bool used, void **p, size_t bytes) { if (!used || *p || bad) return; if (hipMalloc(p, std::max<size_t>(bytes, 16)) != hipSuccess) { *p = nullptr; bad = true; } else mine.push_back(p); };
        auto filled = [&](bool used, void **p, const auto &v) { if (!used || *p || bad) return; if (mi::up(p, v)) bad = true; if (*p) mine.push_back(p); };
        raw(moved, &h.dPos, h.pos.size() * 4); raw(true, &h.dNodeBox, h.nodeBoxes.size() * 4); raw(ni, &h.dInstXf, (size_t) ni * 96); raw(moved && ni, &h.dGroupBox, (size_t) ng * 24);
        filled(moved, &h.dLeafSlot, h.leafSlotOfPrim); filled(ni, &h.dLeafSlotInst, h.leafSlotOfInstance);
        filled(true, &h.dLeafBox, h.leafBoxes);      // slot tables, leaf boxes, refit order: the order in which the two older calls allocated them
        filled(!moved, &h.dRefitOrder, h.refitOrder); filled(moved, &h.dRefitOrderAll, h.refitOrderAll);
        if (bad) {
            const std::string why = hipGetErrorString(hipGetLastError());
            for (void **p : mine) { (void) hipFree(*p); *p = nullptr; }
            return fail(MI_ERR_DEVICE, name + ": allocation failed, the scene is unchanged: " + why);
        }
    }
    // from here on the scene changes; a device error below leaves host and device tables out of step (see the header)
    h.applyGeometry(pos, nrm, nVerts, instances, nInstances);
    if (h.emittersD.size() != h.d.n_emitters || h.areaCdf.size() != cdfLen || h.groupBoxes.size() != (size_t) ng * 6) return fail(MI_ERR_DEVICE, name + ": host tables and device tables disagree in size");
    const mi::GeoEditTables g = h.geoEditTables(true);
    if (pos) {
        HIPCHK(push(h.dPos, h.pos));
        HIPCHK(push(h.dNrm, h.nrm));
        mi_launch_tri_records(g, nullptr);
    }
    if (ni) {      // the new transforms, or the committed ones again: the instance box also follows the group box
        const std::vector<float> xf = h.instanceTransformPairs();
        HIPCHK(push(h.dInstXf, xf));
        if (pos) HIPCHK(push(h.dGroupBox, h.groupBoxes));      // without new vertices the records' glo / ghi are current
        mi_launch_instance_records(h.instEditTables(true, (const float *) h.dInstXf, moved), nullptr);
    }
    {   // bottom-up: level l reads the boxes levels < l wrote; stream order is the only synchronisation.  Vertices moved: every tree; instances only: the scene level
        const std::vector<uint32_t> &start = pos ? h.refitLevelStartAll : h.refitLevelStart; const uint32_t *order = (const uint32_t *) (pos ? h.dRefitOrderAll : h.dRefitOrder);
        for (size_t l = 0; l + 1 < start.size(); ++l) mi_launch_refit_level(g, order, start[l], start[l + 1] - start[l], h.d.n_nodes, nullptr);
    }
    HIPCHK(hipGetLastError());
    if (pos && !ni) {      // the packet tables: a scene with instances never runs in packet mode
        if (h.packetGroups.size() > nGroups) {      // pairs dissolved: the pass-1 table grew
            void *grown = nullptr; if (mi::up(&grown, h.packetGroups)) return fail(MI_ERR_DEVICE, name + ": allocation failed");
            HIPCHK(hipStreamSynchronize(nullptr)); (void) hipFree(h.dPacketGroups); h.dPacketGroups = grown; h.d.packet_groups = (const PacketGroupD *) grown;
        } else HIPCHK(push(h.dPacketGroups, h.packetGroups));
    }
    if (pos) {      // what buildEmitterTables() derives from the vertices; emitterCdf and emitterX follow the emitter records alone and are current on the device
        HIPCHK(push(h.dEmitters, h.emittersD));
        HIPCHK(push(h.dAreaCdf, h.areaCdf));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    return MI_OK;
}
int mi_scene_update_vertices(mi_scene *s, const float *pos, const float *nrm, uint32_t nVerts) {
    if (!s || !pos) return fail(MI_ERR_INVALID, "mi_scene_update_vertices: null argument");
    return updateGeometryOnDevice(mi::GeoEntry::Vertices, s, pos, nrm, nVerts, nullptr, 0);
}
int mi_scene_update_instances(mi_scene *s, const mi_instance *instances, uint32_t n) {
    if (!s || !instances) return fail(MI_ERR_INVALID, "mi_scene_update_instances: null argument");
    return updateGeometryOnDevice(mi::GeoEntry::Instances, s, nullptr, nullptr, 0, instances, n);
}
int mi_scene_update_geometry(mi_scene *s, const float *pos, const float *nrm, uint32_t nVerts, const mi_instance *instances, uint32_t nInstances) {
    if (!s) return fail(MI_ERR_INVALID, "mi_scene_update_geometry: null scene");
    if (!pos && !instances) return fail(MI_ERR_INVALID, "mi_scene_update_geometry: null argument: neither vertices nor instances given");
    return updateGeometryOnDevice(mi::GeoEntry::Geometry, s, pos, nrm, nVerts, instances, nInstances);
}
int mi_scene_revision(mi_scene *s, uint64_t *revision, uint64_t *treeBuilds) {
    if (!s) return fail(MI_ERR_INVALID, "mi_scene_revision: null scene");
    if (revision) *revision = s->h.revision;
    if (treeBuilds) *treeBuilds = s->h.treeBuilds;
    return MI_OK;
}

// Scene::getBSphere() (aabb.cpp:44-47) of the kd-tree box expanded by the sensor's and the point / spot emitters' positions (scene.cpp:394-421): the distance at which the
// volumetric integrators place environment hits.  Depends on the camera and on the emitters, so a render recomputes it when the scene has been edited.
static float alphaDistOf(const mi::SceneHost &h) {
    float lo[3], hi[3]; for (int i = 0; i < 3; ++i) { lo[i] = h.aabbLo[i]; hi[i] = h.aabbHi[i]; }
    auto expand = [&](float x, float y, float z) { const float v[3] = {x, y, z}; for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], v[i]); hi[i] = std::max(hi[i], v[i]); } };
    expand(h.c2w[3], h.c2w[7], h.c2w[11]);
    for (const mi_emitter &e : h.emitters) if (e.type == MI_EMITTER_POINT || e.type == MI_EMITTER_SPOT || e.type == MI_EMITTER_COLLIMATED) expand(e.to_world[3], e.to_world[7], e.to_world[11]);
    float c[3], d2 = 0; for (int i = 0; i < 3; ++i) { c[i] = (hi[i] + lo[i]) * 0.5f; const float d = c[i] - hi[i]; d2 += d * d; }
    (void) c; return std::sqrt(d2) * 2;
}
// AmbientOcclusionIntegrator::preprocess (ao.cpp:77-80): a negative rayLength becomes scene->getAABB().getBSphere().radius * 0.5f -- the sphere above, whose radius
// alphaDistOf hands out times 2 (both scalings by powers of two: exact)
static float aoRayLengthOf(const mi::SceneHost &h, float asked) { return asked < 0 ? alphaDistOf(h) * 0.25f : asked; }
// inverse of the sensor's (affine) world transform in double precision, rounded to float (the relPosition field); false: not invertible
static bool worldToCamera(const mi::SceneHost &h, float *w2c) {
    double m[3][3], t[3]; for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) m[i][j] = h.c2w[i * 4 + j]; t[i] = h.c2w[i * 4 + 3]; }
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    double inv[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        const int a = (j + 1) % 3, b = (j + 2) % 3, c = (i + 1) % 3, d = (i + 2) % 3;
        inv[i][j] = (m[a][c] * m[b][d] - m[a][d] * m[b][c]) / det;
    }
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) w2c[i * 4 + j] = (float) inv[i][j]; w2c[i * 4 + 3] = (float) -(inv[i][0] * t[0] + inv[i][1] * t[1] + inv[i][2] * t[2]); }
    return std::fabs(det) > 0;
}
// The part of the field arguments that follows the scene through its edits and frame marks (prevPosition / motion): the current and the marked projection and camera
// origin, the two tables of mi_scene_mark_frame.  A scene that was never marked has no tables and previous = current.  Renders without these kinds are not touched.
extern "C++" { static int sceneWorldToPixel(const std::string &fn, const mi::SceneHost &h, float *out12); }
#define MI_FIELD_MOTION_KINDS ((1u << MI_FIELD_PREV_POSITION) | (1u << MI_FIELD_MOTION))
static int fieldMotionArgs(const std::string &who, const mi::SceneHost &h, FieldArgs &fa) {
    if (!(fa.needs & MI_FIELD_MOTION_KINDS)) return MI_OK;
    { int rc = sceneWorldToPixel(who, h, fa.m_cur); if (rc) return rc; }
    for (int i = 0; i < 3; ++i) fa.o_cur[i] = h.c2w[i * 4 + 3];
    fa.prev_pos = h.marked && !h.prevPos.empty() ? (const float *) h.dPrevPos : nullptr;
    fa.prev_inst = h.marked && !h.prevInstXf.empty() ? (const float *) h.dPrevInst : nullptr;
    memcpy(fa.m_prev, h.marked ? h.prevW2P : fa.m_cur, 48); memcpy(fa.o_prev, h.marked ? h.prevOrigin : fa.o_cur, 12);
    return MI_OK;
}
// A render holds a copy of the scene record.  Every entry point that launches kernels calls this first: when the scene has been edited since (mi_scene_update_*), the
// copy is taken again -- keeping the per-render packet switch -- together with the two constants that depend on the camera.  Also counts the render as running on the
// scene, so that an update issued meanwhile is refused; RunGuard's destructor ends that.
struct RunGuard {
    mi_scene *s = nullptr;
    bool enter(mi_scene *sc) { int v = sc->busy.load(); while (v >= 0) if (sc->busy.compare_exchange_weak(v, v + 1)) { s = sc; return true; } return false; }
    ~RunGuard() { if (s) s->busy.fetch_sub(1); }
};
static int beginRun(mi_render *r, RunGuard &g, bool film, const char *who) {
    mi_scene *s = r->scene;
    if (!g.enter(s)) return fail(MI_ERR_INVALID, std::string(who) + ": the scene is being updated");
    if (film && (r->samplesTotal || r->mergedSamples) && r->filmRev != s->h.revision)
        return fail(MI_ERR_INVALID, std::string(who) + ": the film holds samples of the scene before its last update; call mi_render_clear first");
    if (r->sceneRev != s->h.revision) {
        r->sc = s->h.d; if (isVolumetric(r->rc.integrator)) r->sc.packet_n = 0;
        r->rc.alpha_dist = alphaDistOf(s->h);
        if (r->rc.integrator == MI_INTEGRATOR_AO) r->ac.ray_length = aoRayLengthOf(s->h, r->p.ray_length);
        if (r->nFields) (void) worldToCamera(s->h, r->fa.w2c);
        r->sceneRev = s->h.revision;
    }
    if (r->nFields) { const int rc = fieldMotionArgs(who, s->h, r->fa); if (rc) return rc; }      // a mark moves no revision: taken again for every run
    if (film) r->filmRev = s->h.revision;
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ render
static int allocQ(std::vector<void *> &allocs, void **p, size_t bytes) {
    HIPCHK(hipMalloc(p, bytes)); allocs.push_back(*p); return MI_OK;
}
#define ALLOC(ptr, type, count) do { void *p_ = nullptr; int rc_ = allocQ(allocs, &p_, sizeof(type) * (size_t) (count)); if (rc_) return rc_; ptr = (type *) p_; } while (0)

static void freePoolQ(Queues &Q, std::vector<void *> &allocs) { for (void *p : allocs) (void) hipFree(p); allocs.clear(); Q = Queues{}; }      // no dangling queue pointer survives
// The shape of a path pool (include/mi355pt.h): pure host arithmetic, exported so that tests can state the shape they mean to run at.
// segments (each owned by one wave in the shade stage): 16384, or -- where the shade stage sorts a segment's paths by material class and its
// index list must fit LDS -- as many as keep a segment at ~1000 slots (C3 at 64 M paths: 1916 Msamples/s with 16384 segments, 1983 with 65536)
extern "C" int mi_debug_pool_shape(uint64_t paths, int hasRC, uint32_t integrator, const mi_pool_overrides *ov, mi_pool_shape *out) {
    if (!out) return fail(MI_ERR_INVALID, "mi_debug_pool_shape: null argument");
    const mi_pool_overrides none{}; if (!ov) ov = &none;
    uint64_t grid = ov->segments ? ov->segments : hasRC ? std::min<uint64_t>(std::max<uint64_t>(16384u, paths / 1024u), 1u << 18) : 16384u;
    const uint64_t minGrid = (paths + 63) / 64; if (grid > minGrid) grid = std::max<uint64_t>(minGrid, 1);
    if (isVolumetric(integrator) && (paths + grid - 1) / grid > 65472u) grid = (paths + 65471u) / 65472u;      // the volumetric stages count two kinds of shadow records per segment in 16 bits each
    uint64_t cap = (paths + grid - 1) / grid; cap = (cap + 63) / 64 * 64;
    if (cap * grid >= (1ull << 28)) return fail(MI_ERR_INVALID, "mi_render_run: a path pool holds fewer than 2^28 slots (the stages address the queues through 32-bit byte offsets); lower planes_per_batch");
    out->n_seg = (uint32_t) grid; out->cap = (uint32_t) cap;
    // workgroups launched per stage (each walks segments b, b + grid, ...): sized to the stage's occupancy on 256 CUs
    out->grid_extend = (uint32_t) std::min<uint64_t>(grid, ov->grid_extend ? ov->grid_extend : 4096u);
    out->grid_shade = (uint32_t) std::min<uint64_t>(grid, ov->grid_shade ? ov->grid_shade : hasRC ? 512u : 768u);      // 3 workgroups per CU since the diffuse kernels hold 4 waves per SIMD (C2: 512 -> 2970, 640 -> 3022, 768 -> 3078, 896 -> 2890 Msamples/s); the 2-wave microfacet kernels stay at 2
    out->grid_shadow = (uint32_t) std::min<uint64_t>(grid, ov->grid_shadow ? ov->grid_shadow : 4096u);
    return MI_OK;
}
// Bytes one slot of a pool takes in the per-slot arrays allocPoolQ allocates (queues.h): what MI355PT_POOL_LIMIT is compared with.
//   two buffers of ray 24 + state 32 (+ eta 4, + st3 4), the camera rays' interval 8 (both buffers in the volumetric modes), hit 16 (+ instance 4; `direct`: a second hit array),
//   shadow record 44 (volumetric: two records of 80), accumulator 16, film position 8.  Plain diffuse `path`: 204 B (the four-float records of before: 224).
static uint64_t mi_pool_slot_bytes(bool vol, bool withEta, bool envConstant, bool instances, bool direct) {
    const uint64_t perBuf = 12 + 12 + 16 + 12 + 4 + (withEta ? 4 : 0) + (envConstant ? 4 : 0);
    const uint64_t hit = (16 + (instances ? 4 : 0)) * (direct ? 2 : 1);
    return 2 * perBuf + (vol ? 16 : 8) + hit + (vol ? 2 * 80 : 44) + 16 + 8;
}
// allocates the queues of ONE pool into an empty Q (freePoolQ first); on failure the caller releases whatever was allocated
static int allocPoolQ(mi_render *r, uint64_t paths, Queues &Q, std::vector<void *> &allocs) {
    // MI355PT_SEGMENTS / MI355PT_GRID_*: 0, a negative value or no number at all count as unset (a segment count of 0 would divide by zero below)
    auto envU = [](const char *name) -> uint32_t { const char *v = getenv(name); const long long x = v ? atoll(v) : 0; return x > 0 ? (uint32_t) std::min<long long>(x, 0xFFFFFFFFll) : 0u; };
    const mi_pool_overrides ov{envU("MI355PT_SEGMENTS"), envU("MI355PT_GRID_EXTEND"), envU("MI355PT_GRID_SHADE"), envU("MI355PT_GRID_SHADOW")};
    mi_pool_shape g{};
    { const int rc = mi_debug_pool_shape(paths, r->scene->h.d.has_roughconductor ? 1 : 0, r->rc.integrator, &ov, &g); if (rc) return rc; }
    const uint32_t grid = g.n_seg; const uint64_t cap = g.cap;
    r->grid = grid; Q.cap = g.cap; Q.n_seg = grid;
    r->gridExtend = g.grid_extend; r->gridShade = g.grid_shade; r->gridShadow = g.grid_shadow;
    const uint64_t slots = cap * grid;
    const bool vol = isVolumetric(r->rc.integrator);
    const bool withEta = vol || r->scene->h.d.has_roughconductor;      // the RC shade variants and the volumetric stages carry eta (queues.h); `direct` keeps a BSDF value in the throughput record and no eta
    {   // MI355PT_POOL_LIMIT (bytes per pool; tests): behave as if the card had no more room than this -- mi_render_run then falls back to smaller batches
        const char *lim = getenv("MI355PT_POOL_LIMIT");
        if (lim && atoll(lim) > 0 && slots * mi_pool_slot_bytes(vol, withEta, r->scene->h.d.env_constant != 0, r->scene->h.d.n_instances != 0, r->rc.integrator == MI_INTEGRATOR_DIRECT) > (uint64_t) atoll(lim))
            return fail(MI_ERR_DEVICE, "mi_render_run: path pool larger than MI355PT_POOL_LIMIT");
    }
    for (int b = 0; b < 2; ++b) {
        ALLOC(Q.rayO[b], QVec3, slots); ALLOC(Q.rayD[b], QVec3, slots);
        if (b == 0 || vol) ALLOC(Q.rayT[b], float2, slots); else Q.rayT[b] = nullptr;      // surface integrators: only the camera rays (always buffer 0) have an interval of their own
        ALLOC(Q.st0[b], uint4, slots); ALLOC(Q.st1[b], QVec3, slots); ALLOC(Q.st2[b], float, slots);
        if (withEta) ALLOC(Q.eta[b], float, slots); else Q.eta[b] = nullptr;
        if (r->scene->h.d.env_constant) ALLOC(Q.st3[b], float, slots); else Q.st3[b] = nullptr;
        ALLOC(Q.count[b], uint32_t, grid);
    }
    if (r->scene->h.d.n_instances) ALLOC(Q.hitInst, int32_t, slots); else Q.hitInst = nullptr;
    // shadow records: 44 B; the volumetric integrators keep a wide contribution and add throughput and BSDF / phase value (80 B); volpath leaves up to two records per path and pass (kernels_volmis.hip)
    const uint64_t shSlots = vol ? slots * 2 : slots;
    ALLOC(Q.hit, float4, slots); ALLOC(Q.shO, float4, shSlots); ALLOC(Q.shD, float4, shSlots);
    if (vol) { Q.shC = nullptr; ALLOC(Q.shCw, float4, shSlots); ALLOC(Q.shT, float4, shSlots); ALLOC(Q.shX, float4, shSlots); } else { ALLOC(Q.shC, QVec3, shSlots); Q.shCw = nullptr; Q.shT = nullptr; Q.shX = nullptr; }
    if (r->rc.integrator == MI_INTEGRATOR_DIRECT) {      // the BSDF rays of a pass are extended into a hit array of their own (direct.h)
        const int pi = &Q == &r->q ? 0 : (int) (&Q - r->qx) + 1;
        ALLOC(r->hitB[pi], float4, slots); if (r->scene->h.d.n_instances) ALLOC(r->hitInstB[pi], int32_t, slots); else r->hitInstB[pi] = nullptr;
    }
    ALLOC(Q.acc, float4, slots); ALLOC(Q.pos, float2, slots); ALLOC(Q.shCount, uint32_t, grid);
    ALLOC(Q.counters, unsigned long long, 4);
    ALLOC(Q.ticket, uint32_t, MI_TICKETS);
    Q.stkSpill = nullptr;
    if (mi_fused_walk(r->scene->h.d) && r->scene->h.d.bvh_stack_direct > 10u)      // FZ_LDS_STACK (trace_fused.h) entries live in LDS, the rest of the builder's bound here
        ALLOC(Q.stkSpill, int32_t, (size_t) (r->scene->h.d.bvh_stack_direct - 10u) * mi_fused_grid() * 256u);
    HIPCHK(hipMemset(Q.counters, 0, 32));
    return MI_OK;
}
// (Re)allocates every pool for `paths` paths.  The ray counters survive (they are cleared by mi_render_clear only).  Nothing is valid until ALL pools are
// allocated: on any failure every pool is released, every queue pointer nulled and poolPaths = 0, so a later run / samples call allocates afresh instead of
// launching on freed buffers; the counters saved before the release move into the handle's merged totals.
static int allocPool(mi_render *r, uint64_t paths) {
    unsigned long long keep[mi_render::kMaxPools][4] = {};
    for (int i = 0; i < r->nStreams; ++i) { Queues &Q = r->pool(i); if (Q.counters && hipMemcpy(keep[i], Q.counters, 32, hipMemcpyDeviceToHost) != hipSuccess) { (void) hipGetLastError(); memset(keep[i], 0, 32); } }
    r->poolPaths = 0;
    for (int i = 0; i < r->nStreams; ++i) freePoolQ(r->pool(i), i ? r->allocsx[i - 1] : r->allocs);
    int rc = MI_OK;
    for (int i = 0; i < r->nStreams && !rc; ++i) {
        rc = allocPoolQ(r, paths, r->pool(i), i ? r->allocsx[i - 1] : r->allocs);
        if (!rc && hipMemcpy(r->pool(i).counters, keep[i], 32, hipMemcpyHostToDevice) != hipSuccess) rc = fail(MI_ERR_DEVICE, "mi_render_run: cannot restore the ray counters");
    }
    if (rc) {
        (void) hipGetLastError();
        for (int i = 0; i < r->nStreams; ++i) { freePoolQ(r->pool(i), i ? r->allocsx[i - 1] : r->allocs); r->mergedRays += keep[i][0]; r->mergedShadow += keep[i][1]; r->mergedPathLen += keep[i][2]; }
        return rc;
    }
    r->poolPaths = paths;
    return MI_OK;
}

// LDS bytes k_shade stages for a small scene (shading records, materials, emitters, CDFs); must match mi_launch_shade (above) and shade.h
static size_t smallTableBytes(const mi::SceneHost &h) {
    if (!h.d.small_tables) return 0;
    return 16 + 4 * ((size_t) h.d.n_tris * (4 * MI_SHADE_WORDS) + h.d.n_materials * 16 + h.d.n_emitters * 12 + ((h.d.n_emitters + 4) & ~3u) + h.d.area_cdf_len);
}
int mi_render_create(mi_scene *s, const mi_render_params *p, mi_render **out) {
    if (!s || !p || !out) return fail(MI_ERR_INVALID, "mi_render_create: null argument");
    if (!s->h.committed) return fail(MI_ERR_INVALID, "mi_render_create: scene not committed");
    if (p->rr_depth <= 0) return fail(MI_ERR_INVALID, "'rrDepth' must be set to a value greater than zero!");                       // integrator.cpp:221-222
    if (p->max_depth <= 0 && p->max_depth != -1) return fail(MI_ERR_INVALID, "'maxDepth' must be set to -1 (infinite) or a value greater than zero!");   // :224-225
    if (p->max_depth > 250) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: maxDepth > 250");
    if (p->sampler > 1) return fail(MI_ERR_INVALID, "mi_render_create: unknown sampler");
    if (isVolumetric(p->integrator) && (s->h.d.has_adapters & 4u)) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: `coating`, `roughcoating` and `blendbsdf` are implemented for the path integrator only");
    if (p->integrator > MI_INTEGRATOR_AO) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: integrators path (0), volpath_simple (1), volpath (2), direct (3) and ao (4) are implemented");
    const bool vol = isVolumetric(p->integrator), direct = p->integrator == MI_INTEGRATOR_DIRECT, ao = p->integrator == MI_INTEGRATOR_AO, oneHit = direct || ao;      // oneHit: one camera hit with sample arrays, their sampler layout
    DirectConst dc{}; AoConst ac{}; uint32_t directDims = 0, directFrames = 0;      // Sobol' dimensions / look_up frames a direct / ao render can touch
    if (ao) {      // AmbientOcclusionIntegrator (ao.cpp:38-82).  No BSDF, emitter or medium is read: every scene is accepted
        const uint32_t N = p->shading_samples; const bool lens = s->h.lensRadius != 0.0f;
        if (N == 0) return fail(MI_ERR_INVALID, "mi_render_create: ao integrator: shadingSamples must be at least 1 (ao.cpp:122 divides by it)");
        if ((uint64_t) std::max(p->spp, 1u) * N > (1ull << 22)) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: ao integrator: spp x shadingSamples beyond 2^22 (the sample array numbers its Sobol' points m x N + j in 32 bits, and the look_up tables hold one entry per point)");
        if (!(p->ray_length == p->ray_length)) return fail(MI_ERR_INVALID, "mi_render_create: ao integrator: rayLength is not a number");
        if (p->opacity && !s->h.media.empty()) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: ao integrator: `opacity` on a scene with participating media needs the transmittance walk of records.inl:124-135, which this integrator does not have");
        ac.n = N; ac.recip = 1.0f / (float) N; ac.ray_length = aoRayLengthOf(s->h, p->ray_length);
        if (p->sampler == MI_SAMPLER_SOBOL) {      // sobol.cpp:171-250: the one array at dimensions 5 / 6; else next2D after the pixel offset / the aperture sample, skipping dimension 4
            if (N > 1) { ac.array = 5u; directDims = 7u; } else { ac.own_dim = lens ? 5u : 2u; directDims = ac.own_dim + 2u; }
            directFrames = std::max(p->spp, 1u) * N;
            if (N > 1 && s->h.logRes < 1) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: ao integrator: Sobol' sample arrays need a film of at least 2 x 2 pixels (sobol::look_up of a 1 x 1 film reads outside its tables)");
        } else {      // the build-defined stream: the own request is the next call after the camera's, array elements count down from call 255
            const uint32_t c = lens ? 2u : 1u;
            if (N > 1) ac.array = 255u; else ac.own_dim = c;
            if (N > 1 && (uint64_t) c + N > 256u) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: ao integrator: the independent sampler stream numbers 256 draws per sample; shadingSamples + the camera's draws exceed that (use the Sobol sampler or fewer shading samples)");
        }
    }
    if (direct) {      // MIDirectIntegrator (direct.cpp:93-144); what its kernels (direct.h) are not built for is refused by name
        if (s->h.d.has_adapters & 1u) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: the direct integrator does not implement `mixturebsdf`, `bumpmap`, `normalmap`, `coating`, `roughcoating` and `blendbsdf` (use the path integrator with maxDepth = 2)");
        if (!s->h.media.empty()) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: the direct integrator does not support participating media (direct.cpp:181-182)");
        for (const mi_material &m : s->h.materials) if (m.type == MI_BSDF_NULL) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: the direct integrator does not support `null` boundaries (index-matched medium transitions, direct.cpp:181-182)");
        const uint32_t N = p->emitter_samples, M = p->bsdf_samples;
        if (N == 0 && M == 0) return fail(MI_ERR_INVALID, "Assertion 'm_emitterSamples + m_bsdfSamples > 0' failed: emitterSamples and bsdfSamples must not both be 0");      // direct.cpp:107
        const uint32_t S = std::max(std::max(N, M), 1u);
        if ((uint64_t) std::max(p->spp, 1u) * S > (1ull << 22)) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: direct integrator: spp x max(emitterSamples, bsdfSamples) beyond 2^22 (the sample arrays number their Sobol' points m x S + j in 32 bits, and the look_up tables hold one entry per point)");
        dc.n_em = N; dc.n_bs = M; dc.weight_lum = 1.0f / (float) N; dc.weight_bsdf = 1.0f / (float) M; dc.frac_lum = (float) N / (float) (N + M); dc.frac_bsdf = (float) M / (float) (N + M);
        const bool lens = s->h.lensRadius != 0.0f;
        if (p->sampler == MI_SAMPLER_SOBOL) {      // sobol.cpp:171-250: arrays from dimension 5, two each, emitter side first; next2D / next1D skip the reserved range
            const uint32_t arrays = (N > 1 ? 1u : 0u) + (M > 1 ? 1u : 0u), arrayEnd = 5u + 2u * arrays; uint32_t dim = lens ? 4u : 2u;
            auto own2D = [&]() { if (dim + 1 >= 5u && dim < arrayEnd) dim = arrayEnd; const uint32_t d0 = dim; dim += 2; return d0; };
            if (N > 1) dc.em_array = 5u; else dc.em_dim = own2D();
            if (M > 1) dc.bs_array = 5u + (N > 1 ? 2u : 0u); else dc.bs_dim = own2D();
            dc.extra_dim = dim; dc.array_end = arrayEnd;
            bool usesSampler = false; for (const mi_material &m : s->h.materials) if (m.type == MI_BSDF_ROUGHDIELECTRIC) usesSampler = true;
            if (usesSampler) for (uint32_t j = 0; j < std::max(M, 1u); ++j) { if (dim >= 5u && dim < arrayEnd) dim = arrayEnd; ++dim; }      // one next1D per BSDF sub-sample at the most
            directDims = std::max(dim, arrayEnd); directFrames = std::max(p->spp, 1u) * (arrays ? S : 1u);
            if (arrays && s->h.logRes < 1) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: direct integrator: Sobol' sample arrays need a film of at least 2 x 2 pixels (sobol::look_up of a 1 x 1 film reads outside its tables)");
        } else {      // the build-defined stream: own requests and EUsesSampler draws count upwards as in `path`, array elements downwards from call 255
            uint32_t c = lens ? 2u : 1u, top = 256u;
            if (N > 1) { dc.em_array = top - 1u; top -= N; } else dc.em_dim = c++;
            if (M > 1) { dc.bs_array = top - 1u; top -= M; } else dc.bs_dim = c++;
            dc.extra_dim = c; dc.array_end = 0;
            if ((uint64_t) c + M > top || N > 255u || M > 255u) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: direct integrator: the independent sampler stream numbers 256 draws per sample; emitterSamples + 2 x bsdfSamples + the camera's draws exceed that (use the Sobol sampler or fewer shading samples)");
        }
    }
    if (vol) {       // what the volumetric stages (kernels_vol.hip) are built for
        // a bumpmap / normalmap over a `null` / `thindielectric` has an ENull lobe the transmittance walks would have to evaluate in a perturbed frame (the reference reads an unset shading frame there); plain records, `mask` and `mixturebsdf` are seen through (surfaceNullEval)
        auto nullLobe = [&](uint32_t i) { return i < s->h.materials.size() && (s->h.materials[i].type == MI_BSDF_NULL || s->h.materials[i].type == MI_BSDF_THINDIELECTRIC); };
        for (const mi_material &m : s->h.materials) {
            bool bad = false;
            if ((m.type == MI_BSDF_BUMPMAP || m.type == MI_BSDF_NORMALMAP) && m.distr < s->h.materials.size()) {
                const mi_material &nm = s->h.materials[m.distr]; bad = nullLobe(m.distr);
                if (nm.type == MI_BSDF_MIXTURE) for (uint32_t c = 0; c < nm.distr && c < 4; ++c) bad |= nullLobe((uint32_t) (c < 3 ? nm.reflectance[c] : nm.eta[0]));
            }
            if (bad) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: volpath_simple / volpath with a null / thindielectric BSDF inside a bumpmap / normalmap is not implemented");
        }
        if (p->max_depth > 250) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: maxDepth beyond 250");
    }
    if (p->sampler == MI_SAMPLER_SOBOL) {
        if (!s->h.d.sobol_m32) return fail(MI_ERR_INVALID, "mi_render_create: Sobol tables not loaded before mi_scene_commit (mi_set_sobol_tables)");
        // dimensions consumed: 2 + per bounce (2 NEE + 2 BSDF + 1 RR, + 1 where a BSDF draws from the sampler itself: roughdielectric, EUsesSampler) + the dim-4 skip
        // (sobol.cpp:218-251 aborts beyond the table)
        int depth = p->max_depth < 0 ? 250 : p->max_depth;
        int perBounce = 5; for (const mi_material &m : s->h.materials) if (m.type == MI_BSDF_ROUGHDIELECTRIC) perBounce = 6;
        if (vol) perBounce += 2;      // + the one or two draws of HomogeneousMedium::sampleDistance per iteration
        const int lensDims = s->h.lensRadius != 0.0f ? 2 : 0;      // the aperture sample: dimensions 2 / 3 (k_generate), every later draw moves by two
        if (lensDims && (uint32_t) (3 + lensDims) > s->h.d.sobol_dims) return fail(MI_ERR_INVALID, "Lookup dimension exceeds the direction number table size! The thin lens draws Sobol dimensions 2 and 3.");
        if (oneHit) {      // maxDepth plays no part: the dimensions of direct.cpp's / ao.cpp's requests (computed above)
            if (ao && directDims > s->h.d.sobol_dims) return fail(MI_ERR_INVALID, "Lookup dimension exceeds the direction number table size! The ao integrator's sample array draws Sobol dimensions 5 and 6 (7 dimensions are needed when shadingSamples > 1).");
            if (directDims > s->h.d.sobol_dims || directDims > 256u) return fail(MI_ERR_INVALID, "Lookup dimension exceeds the direction number table size! You may have to reduce 'bsdfSamples' (a roughdielectric draws one more dimension per BSDF sample).");
        } else {
        if (p->max_depth > 0 && (uint32_t) (3 + lensDims + perBounce * depth) > s->h.d.sobol_dims) return fail(MI_ERR_INVALID, "Lookup dimension exceeds the direction number table size! You may have to reduce the 'maxDepth' parameter of your integrator.");
        if (p->max_depth < 0) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: maxDepth = -1 with the Sobol sampler needs more dimensions than are loaded");
        // the state word st0.w carries the dimension in 8 bits: with the shipped 128-dimension tables the bound above is the tighter one, larger caller-supplied tables end here
        if (p->max_depth > 0 && 3 + lensDims + perBounce * depth > 256) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: the path state numbers a path's Sobol dimensions with 8 bits; maxDepth x draws per bounce exceeds 256 (reduce maxDepth)");
        }
    }
    if (p->sampler == MI_SAMPLER_INDEPENDENT && p->max_depth > 0 && !oneHit) {
        // the build-defined independent stream numbers a path's draws with 8 bits: a path that could draw more than 256 values would re-read
        // its own stream from call 0 -- refused by name rather than silently correlated (unbounded depth keeps the documented period)
        int perBounce = 5; for (const mi_material &m : s->h.materials) if (m.type == MI_BSDF_ROUGHDIELECTRIC) perBounce = 6;
        if (vol) perBounce += 2;
        if (2 + (s->h.lensRadius != 0.0f ? 2 : 0) + perBounce * p->max_depth > 256) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: the independent sampler stream numbers 256 draws per path; maxDepth x draws per bounce exceeds that (use the Sobol sampler or a smaller maxDepth)");
    }
    HIPCHK(hipSetDevice(s->h.device));
    mi_render *r = new mi_render(); r->scene = s;
    memcpy(&r->p, p, offsetof(mi_render_params, emitter_samples));      // the two trailing fields exist in a caller's struct only where it asks for the direct integrator
    if (direct) { r->p.emitter_samples = p->emitter_samples; r->p.bsdf_samples = p->bsdf_samples; r->dc = dc; }
    if (ao) { r->p.shading_samples = p->shading_samples; r->p.ray_length = p->ray_length; r->ac = ac; }      // (read only here: the other integrators' callers may pass the shorter struct)
    r->sc = s->h.d; r->sceneRev = r->filmRev = s->h.revision; if (vol) r->sc.packet_n = 0;      // packet or tree is decided per render: volpath / volpath_simple on a <= 64-triangle scene without media walk its tree
    struct Guard { mi_render *r; ~Guard() { if (r) mi_render_destroy(r); } } guard{r};      // every early return below releases what was created so far
    r->rc.max_depth = p->max_depth; r->rc.rr_depth = p->rr_depth; r->rc.strict_normals = p->strict_normals; r->rc.hide_emitters = p->hide_emitters; r->rc.opacity = p->opacity;
    r->rc.sobol_scramble = 0;
    // volumetric integrators: the radiance-type bits and the sensor's medium of a fresh path (kernels_vol.hip; volpath_simple.cpp:103-104: maxDepth = 1 gathers emitted radiance only)
    r->rc.alpha_dist = alphaDistOf(s->h);
    r->rc.integrator = p->integrator;
    r->rc.state_init = p->integrator == MI_INTEGRATOR_VOLPATH_SIMPLE ? (VS_EMITTED | (p->max_depth == 1 ? 0u : VS_OTHERS) | VS_NULLCHAIN | ((uint32_t) (s->h.d.sensor_medium + 1) << VS_MEDIUM_SHIFT))
                     : p->integrator == MI_INTEGRATOR_VOLPATH ? (VS_EMITTED | ((uint32_t) (s->h.d.sensor_medium + 1) << VS_MEDIUM_SHIFT)) : 0u;      // volpath: ERadiance, nothing else (kernels_volmis.hip)
    if (p->sampler == MI_SAMPLER_SOBOL && p->seed) {          // SobolSampler: a nonzero `scramble` goes through sampleTEA (sobol.cpp:96-102; qmc.h:146-156, 4 rounds)
        uint32_t v0 = (uint32_t) p->seed, v1 = (uint32_t) (p->seed >> 32), sum = 0;
        for (int i = 0; i < 4; ++i) {
            sum += 0x9e3779b9u;
            v0 += ((v1 << 4) + 0xA341316Cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xC8013EA4u);
            v1 += ((v0 << 4) + 0xAD90777Du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7E95761Eu);
        }
        r->rc.sobol_scramble = v0;                           // single precision build: the low 32 bits of (v1 << 32) + v0 (sobolseq.h:87-96)
    }
    r->rc.sampler = p->sampler; r->rc.seed_mix = (uint32_t) p->seed * 0x9E3779B9u; r->rc.inv_sqrt_spp = 1.0f / std::sqrt((float) (p->spp ? p->spp : 1u));
    if (p->sampler == MI_SAMPLER_SOBOL) {
        // fold the direction matrices into 4-bit lookup tables for the dimensions / index bits this render can touch
        int perBounceDims = 5; for (const mi_material &m : s->h.materials) if (m.type == MI_BSDF_ROUGHDIELECTRIC) perBounceDims = 6;
        if (vol) perBounceDims += 2;
        uint32_t sppBits = 0; while ((1ull << sppBits) < (oneHit ? directFrames : p->spp)) ++sppBits;      // (direct, ao: the array elements' frames m x S + j)
        const uint32_t bits = (s->h.logRes > 1 ? 2 * s->h.logRes : 0) + sppBits + 1;
        const uint32_t nibs = std::max<uint32_t>(8, (bits + 3) / 4), dims      /* at least the eight nibbles of the low index word (pt_device.h sobolBitsNib unrolls them) */ = std::min<uint32_t>(s->h.d.sobol_dims, oneHit ? std::max(directDims, 4u) : (uint32_t) (4 + (s->h.lensRadius != 0.0f ? 2 : 0) + perBounceDims * p->max_depth));
        std::vector<uint32_t> nib((size_t) dims * nibs * 16);
        for (uint32_t dmn = 0; dmn < dims; ++dmn) for (uint32_t n = 0; n < nibs; ++n) for (uint32_t v = 0; v < 16; ++v) {
            uint32_t x = 0; for (uint32_t b = 0; b < 4; ++b) if (((v >> b) & 1u) && 4 * n + b < MI_SOBOL_SIZE) x ^= g_sobolM32[(size_t) dmn * MI_SOBOL_SIZE + 4 * n + b];
            nib[((size_t) dmn * nibs + n) * 16 + v] = x;
        }
        if ((size_t) dims * nibs * 64 + 64 > 144 * 1024) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: the Sobol lookup tables (maxDepth x index bits) exceed the 144 KB of LDS the shading stage may request (reduce maxDepth or spp)");
        HIPCHK(hipMalloc((void **) &r->dNib, nib.size() * 4)); HIPCHK(hipMemcpy(r->dNib, nib.data(), nib.size() * 4, hipMemcpyHostToDevice));
        r->rc.sobol_nib = r->dNib; r->rc.nib_count = nibs; r->rc.nib_dims = dims;
        // look_up tables of k_generate.  index(frame, px, py) = (frame << 2m) ^ Inv * ((px << m | py) ^ Delta * frame)  (sobolseq.h:99-131, all XOR-linear) =
        // F[frame] ^ PX[px] ^ PY[py] with F = (frame << 2m) ^ Inv Delta frame, PX = Inv (px << m), PY = Inv py; and dimension d of the sample is M_d * index,
        // linear as well: every table entry carries {index lo, hi, M_0 * index, M_1 * index}.  The scramble flips pixel bits before the lookup and is XORed
        // into the sample afterwards (k_generate), so the tables do not depend on it.
        const uint32_t m = s->h.logRes;
        if (m > 1) {
            if (2 * m + sppBits > 52 || p->spp > (1u << 22) || (oneHit && directFrames > (1u << 22))) return fail(MI_ERR_UNSUPPORTED, "mi_render_create: Sobol index beyond 52 bits (film resolution x sample count)");
            const uint64_t *vdc = g_sobolVdc.data() + (size_t) (m - 1) * MI_SOBOL_SIZE, *vdi = g_sobolVdcInv.data() + (size_t) (m - 1) * MI_SOBOL_SIZE;
            auto mulVec = [&](const uint64_t *cols, uint64_t b) { uint64_t x = 0; for (uint32_t c = 0; b; b >>= 1, ++c) if (b & 1) x ^= cols[c]; return x; };
            auto dimBits = [&](uint32_t dmn, uint64_t index) { uint32_t x = 0; for (uint32_t c = 0; index; index >>= 1, ++c) if (index & 1) x ^= g_sobolM32[(size_t) dmn * MI_SOBOL_SIZE + c]; return x; };
            const size_t res = (size_t) 1 << m, nF = oneHit ? directFrames : std::max<uint32_t>(p->spp, 1u);
            std::vector<uint32_t> tab((nF + 2 * res) * 4);
            auto put = [&](size_t e, uint64_t idx) { tab[e * 4] = (uint32_t) idx; tab[e * 4 + 1] = (uint32_t) (idx >> 32); tab[e * 4 + 2] = dimBits(0, idx); tab[e * 4 + 3] = dimBits(1, idx); };
            for (size_t f = 0; f < nF; ++f) put(f, ((uint64_t) f << (2 * m)) ^ mulVec(vdi, mulVec(vdc, f)));
            for (size_t x = 0; x < res; ++x) { put(nF + x, mulVec(vdi, (uint64_t) x << m)); put(nF + res + x, mulVec(vdi, (uint64_t) x)); }
            HIPCHK(hipMalloc(&r->dSobolTabs, tab.size() * 4)); HIPCHK(hipMemcpy(r->dSobolTabs, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
            r->rc.sobol_frame = (const uint4 *) r->dSobolTabs; r->rc.sobol_nframes = (uint32_t) nF; r->rc.sobol_px = r->rc.sobol_frame + nF; r->rc.sobol_py = r->rc.sobol_px + res;
        }
    }
    HIPCHK(hipStreamCreate(&r->stream)); HIPCHK(hipEventCreate(&r->evBegin)); HIPCHK(hipEventCreate(&r->evEnd));
    { const char *ns = getenv("MI355PT_STREAMS"); r->nStreams = ns && ns[0] >= '1' && ns[0] <= '4' ? ns[0] - '0' : 2; }
    for (int i = 1; i < r->nStreams; ++i) HIPCHK(hipStreamCreate(&r->streamx[i - 1]));
    for (int i = 0; i < r->nStreams; ++i) { HIPCHK(hipEventCreateWithFlags(&r->filmDone[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&r->joinEv[i], hipEventDisableTiming)); }
    {   // scene tables in LDS: only if they fit next to the Sobol tables, leaving room for the order list of mixed-material scenes (8 KB at the default segment size)
        const size_t nibBytes = p->sampler == MI_SAMPLER_SOBOL ? (size_t) r->rc.nib_dims * r->rc.nib_count * 64 : 16;
        r->ldsTables = s->h.d.small_tables && nibBytes + smallTableBytes(s->h) + (s->h.d.has_roughconductor ? 8192 + 64 : 64) <= 64 * 1024;
    }
    const int W = (int) s->h.width + 2 * s->h.border, H = (int) s->h.height + 2 * s->h.border;
    r->filmFloats = (size_t) W * H * 5;
    HIPCHK(hipMalloc((void **) &r->film, r->filmFloats * 4)); HIPCHK(hipMemset(r->film, 0, r->filmFloats * 4));
    HIPCHK(hipMalloc((void **) &r->spill, r->filmFloats * 4)); HIPCHK(hipMemset(r->spill, 0, r->filmFloats * 4));
    HIPCHK(hipMalloc((void **) &r->layoutTmp, r->filmFloats * 4));
    guard.r = nullptr; *out = r; return MI_OK;
}
static void releaseFields(mi_render *r) {
    if (r->fieldFilm) (void) hipFree(r->fieldFilm);
    if (r->fieldSpill) (void) hipFree(r->fieldSpill);
    if (r->fieldTmp) (void) hipFree(r->fieldTmp);
    if (r->dTriShape) (void) hipFree(r->dTriShape);
    for (hipEvent_t &e : r->fieldDone) if (e) { (void) hipEventDestroy(e); e = nullptr; }
    r->fieldFilm = r->fieldSpill = r->fieldTmp = nullptr; r->dTriShape = nullptr; r->fieldFloats = 0; r->nFields = 0; r->fa = FieldArgs{};
}
static void releaseAdaptive(mi_render *r);
void mi_render_destroy(mi_render *r) {
    if (!r) return;
    (void) hipSetDevice(r->scene->h.device);
    for (void *p : r->allocs) (void) hipFree(p);
    for (auto &a : r->allocsx) for (void *p : a) (void) hipFree(p);
    for (hipEvent_t e : r->filmDone) if (e) (void) hipEventDestroy(e);
    for (hipEvent_t e : r->joinEv) if (e) (void) hipEventDestroy(e);
    for (hipStream_t st : r->streamx) if (st) (void) hipStreamDestroy(st);
    if (r->film) (void) hipFree(r->film);
    if (r->spill) (void) hipFree(r->spill);
    if (r->layoutTmp) (void) hipFree(r->layoutTmp);
    if (r->mergeTmp) (void) hipFree(r->mergeTmp);
    releaseFields(r);
    releaseAdaptive(r);
    if (r->dnMem) (void) hipFree(r->dnMem);
    if (r->dnPprev) (void) hipFree(r->dnPprev);
    if (r->dNib) (void) hipFree(r->dNib);
    if (r->pollHost) (void) hipHostFree(r->pollHost);
    if (r->pollEv) (void) hipEventDestroy(r->pollEv);
    if (r->dSobolTabs) (void) hipFree(r->dSobolTabs);
    for (hipEvent_t e : r->evPool) (void) hipEventDestroy(e);
    if (r->evBegin) (void) hipEventDestroy(r->evBegin);
    if (r->evEnd) (void) hipEventDestroy(r->evEnd);
    if (r->stream) (void) hipStreamDestroy(r->stream);
    delete r;
}
int mi_render_clear(mi_render *r) {
    if (!r) return fail(MI_ERR_INVALID, "mi_render_clear: null"); HIPCHK(hipSetDevice(r->scene->h.device));
    HIPCHK(hipMemsetAsync(r->film, 0, r->filmFloats * 4, r->stream)); HIPCHK(hipMemsetAsync(r->spill, 0, r->filmFloats * 4, r->stream));
    if (r->nFields) { HIPCHK(hipMemsetAsync(r->fieldFilm, 0, r->fieldFloats * 4, r->stream)); HIPCHK(hipMemsetAsync(r->fieldSpill, 0, r->fieldFloats * 4, r->stream)); }
    if (r->q.counters) HIPCHK(hipMemsetAsync(r->q.counters, 0, 32, r->stream));
    for (Queues &Q : r->qx) if (Q.counters) HIPCHK(hipMemsetAsync(Q.counters, 0, 32, r->stream));
    r->adaptFilm = false; r->as = mi_adaptive_stats{};      // adaptive state and counts are zeroed when the next adaptive run starts
    HIPCHK(hipStreamSynchronize(r->stream)); r->samplesTotal = 0; r->mergedRays = r->mergedShadow = r->mergedPathLen = r->mergedSamples = 0; r->filmRev = r->scene->h.revision; r->cancel.store(0); return MI_OK;
}
void mi_render_cancel(mi_render *r) { if (r) r->cancel.store(1); }
// Debug / parity: generate the listed paths, then read back what a shading stage would recompute for their sensor rays (k_debug_sensor_differentials)
int mi_render_debug_sensor_differentials(mi_render *r, const uint32_t *pairs, uint64_t n, float *out) {
    if (!r || !pairs || !out || !n) return fail(MI_ERR_INVALID, "mi_render_debug_sensor_differentials: null argument");
    const mi::SceneHost &h = r->scene->h; HIPCHK(hipSetDevice(h.device));
    for (uint64_t i = 0; i < n; ++i) if (pairs[i * 3] >= h.width || pairs[i * 3 + 1] >= h.height) return fail(MI_ERR_INVALID, "mi_render_debug_sensor_differentials: pixel outside the film");
    RunGuard running; { const int rc = beginRun(r, running, false, "mi_render_debug_sensor_differentials"); if (rc) return rc; }
    if (n > r->poolPaths) { int rc = allocPool(r, n); if (rc) return rc; }
    if (!r->q.counters) return fail(MI_ERR_DEVICE, "mi_render_debug_sensor_differentials: no path pool");
    uint32_t *dList = nullptr; float *dOut = nullptr;
    HIPCHK(hipMalloc((void **) &dList, n * 12));
    if (hipMalloc((void **) &dOut, n * 32) != hipSuccess) { (void) hipFree(dList); return fail(MI_ERR_DEVICE, "mi_render_debug_sensor_differentials: out of device memory"); }
    BatchDesc bd{}; bd.tile = mi_tile{0, 0, h.width, h.height}; bd.n_pix = (uint32_t) n; bd.n_planes = 1; bd.sample_begin = 0; bd.n_paths = n; bd.list = dList; bd.row_stride = 1;
    hipError_t e = hipMemcpy(dList, pairs, n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        mi_launch_generate(r->sc, r->rc, r->q, bd, r->grid, r->stream);
        mi_launch_debug_sensor_differentials(r->sc, r->rc, r->q, n, dOut, r->stream);
        e = hipStreamSynchronize(r->stream); if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dOut, n * 32, hipMemcpyDeviceToHost);
    (void) hipFree(dList); (void) hipFree(dOut);
    if (e != hipSuccess) return fail(MI_ERR_DEVICE, std::string("mi_render_debug_sensor_differentials: ") + hipGetErrorString(e));
    return MI_OK;
}
int mi_render_debug_pool_info(mi_render *r, mi_pool_info *out) {
    if (!r || !out) return fail(MI_ERR_INVALID, "mi_render_debug_pool_info: null argument");
    *out = mi_pool_info{}; out->n_pools = (uint32_t) r->nStreams; out->lds_tables = r->ldsTables ? 1u : 0u; out->sorted = r->lastSorted ? 1u : 0u; out->has_roughconductor = r->scene->h.d.has_roughconductor ? 1u : 0u; out->integrator = r->rc.integrator; out->shade_table_bytes = r->lastTableBytes; out->pool_paths = r->poolPaths;
    if (r->poolPaths) { out->n_seg = r->q.n_seg; out->cap = r->q.cap; out->grid_extend = r->gridExtend; out->grid_shade = r->gridShade; out->grid_shadow = r->gridShadow; }
    return MI_OK;
}
int mi_render_set_profiling(mi_render *r, int enabled) { if (!r) return fail(MI_ERR_INVALID, "null"); r->profiling = enabled != 0; return MI_OK; }

static void mark(mi_render *r, int tag, size_t &used, hipStream_t st = nullptr) {
    if (!r->profiling || (st && st != r->stream)) return;      // stage events are recorded on the first stream only
    if (used >= r->evPool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; r->evPool.push_back(e); r->evTag.push_back(0); }
    (void) hipEventRecord(r->evPool[used], r->stream); r->evTag[used] = tag; ++used;
}

// One pass of the direct integrator over the camera-hit queue (direct.h): emitter sub-sample j (bsdfPass = 0) or BSDF sub-sample j.  Dynamic LDS as mi_launch_shade,
// without the order list (a pass runs one half of the shade stage's code; its segments are read in queue order).
static void launchDirectPass(mi_render *r, const Queues &q, const BatchDesc &bd, int bsdfPass, uint32_t j, hipStream_t st) {
    DScene sc = r->sc; sc.small_tables = r->ldsTables ? 1u : 0u;
    size_t lds = r->rc.sampler == 1 ? (size_t) r->rc.nib_dims * r->rc.nib_count * 64 : 16;
    if (sc.small_tables) lds += 16 + 4 * ((size_t) sc.n_tris * (4 * MI_SHADE_WORDS) + sc.n_materials * 16 + sc.n_emitters * 12 + ((sc.n_emitters + 4) & ~3u) + sc.area_cdf_len);
    DirectConst dc = r->dc; dc.pass = j; const bool env = sc.env_index >= 0;
    if (!sc.has_roughconductor) (env ? mi_launch_direct_d_env : mi_launch_direct_d)(sc, r->rc, dc, q, bd, bsdfPass, r->gridShade, lds, st);
    else (env ? mi_launch_direct_rc_env : mi_launch_direct_rc)(sc, r->rc, dc, q, bd, bsdfPass, r->gridShade, lds, st);
}
// trace one batch of the direct integrator: one camera hit, then N emitter passes and M BSDF passes over it (direct.h; direct.cpp:146-309)
static int traceBatchDirect(mi_render *r, const BatchDesc &bd, size_t &evUsed, int pool) {
    const DScene &sc = r->sc; hipStream_t st = r->poolStream(pool); Queues &Q = r->pool(pool);
    Queues QB = Q; QB.hit = r->hitB[pool]; QB.hitInst = r->hitInstB[pool];      // the BSDF rays' view of the pool: buffer 1 with a hit array of its own
    mark(r, 0, evUsed, st);
    const bool fused = mi_fused_walk(sc); uint32_t ticket = 2;      // every fused traversal launch of the batch takes a zeroed ticket word; beyond MI_TICKETS launches the while-while kernels
    if (fused) HIPCHK(hipMemsetAsync(Q.ticket, 0, MI_TICKETS * sizeof(uint32_t), st));
    mi_launch_generate(sc, r->rc, Q, bd, r->grid, st);
    mark(r, 1, evUsed, st);
    if (fused) mi_launch_extend_fused(sc, Q, 0, 1, Q.ticket + ticket++, st); else mi_launch_extend(sc, Q, 0, 1, r->gridExtend, st);
    ++r->launchesAll;
    if (r->nFields && !bd.list) {      // field channels of the film samples, as in traceBatch
        mark(r, 0, evUsed, st);
        if (r->fieldChain && r->lastFieldPool >= 0 && r->lastFieldPool != pool) HIPCHK(hipStreamWaitEvent(st, r->fieldDone[r->lastFieldPool], 0));
        mi_launch_field_film(sc, r->fa, Q, bd, r->fieldFilm, r->fieldSpill, st);
        if (r->fieldChain) { HIPCHK(hipEventRecord(r->fieldDone[pool], st)); r->lastFieldPool = pool; }
    }
    if (sc.env_texture && !r->rc.hide_emitters) mi_launch_env_primary(sc, r->rc, Q, 0, r->gridExtend, st);
    const uint32_t N = r->dc.n_em, M = r->dc.n_bs;
    for (uint32_t j = 0; j < std::max(N, 1u); ++j) {      // (N = 0: one launch for Le, the environment and the alpha rule)
        mark(r, 2, evUsed, st); launchDirectPass(r, Q, bd, 0, j, st);
        if (N) { mark(r, 3, evUsed, st); if (fused && ticket < MI_TICKETS) mi_launch_shadow_fused(sc, Q, Q.ticket + ticket++, st); else mi_launch_shadow(sc, Q, r->gridShadow, st); }
    }
    for (uint32_t j = 0; j < M; ++j) {
        mark(r, 2, evUsed, st); launchDirectPass(r, Q, bd, 1, j, st);
        mark(r, 1, evUsed, st);
        if (fused && ticket < MI_TICKETS) mi_launch_extend_fused(sc, QB, 1, 0, Q.ticket + ticket++, st); else mi_launch_extend(sc, QB, 1, 0, r->gridExtend, st);      // BSDF rays: (Epsilon, inf)
        ++r->launchesAll;
        mark(r, 2, evUsed, st); mi_launch_direct_hit(sc, r->rc, r->dc, QB, r->gridExtend, st);
    }
    mark(r, 0, evUsed, st);
    HIPCHK(hipGetLastError());
    return MI_OK;
}
// trace one batch of the ambient-occlusion integrator: one camera hit, then N x (k_ao, shadow) over it and the resolve pass (ao.h; ao.cpp:84-125).  The camera-hit queue
// stays put as in traceBatchDirect; no second hit array, no environment launch (a camera miss is 1 whatever the environment is)
static int traceBatchAo(mi_render *r, const BatchDesc &bd, size_t &evUsed, int pool) {
    const DScene &scR = r->sc; hipStream_t st = r->poolStream(pool); Queues &Q = r->pool(pool);
    mark(r, 0, evUsed, st);
    const bool fused = mi_fused_walk(scR); uint32_t ticket = 2;
    if (fused) HIPCHK(hipMemsetAsync(Q.ticket, 0, MI_TICKETS * sizeof(uint32_t), st));
    mi_launch_generate(scR, r->rc, Q, bd, r->grid, st);
    mark(r, 1, evUsed, st);
    if (fused) mi_launch_extend_fused(scR, Q, 0, 1, Q.ticket + ticket++, st); else mi_launch_extend(scR, Q, 0, 1, r->gridExtend, st);
    ++r->launchesAll;
    if (r->nFields && !bd.list) {      // field channels of the film samples, as in traceBatch
        mark(r, 0, evUsed, st);
        if (r->fieldChain && r->lastFieldPool >= 0 && r->lastFieldPool != pool) HIPCHK(hipStreamWaitEvent(st, r->fieldDone[r->lastFieldPool], 0));
        mi_launch_field_film(scR, r->fa, Q, bd, r->fieldFilm, r->fieldSpill, st);
        if (r->fieldChain) { HIPCHK(hipEventRecord(r->fieldDone[pool], st)); r->lastFieldPool = pool; }
    }
    // dynamic LDS of k_ao: the Sobol' nibble tables, then (small scenes) the shading records -- no material, emitter or CDF table
    DScene sc = scR; sc.small_tables = r->ldsTables ? 1u : 0u;
    size_t lds = r->rc.sampler == 1 ? (size_t) r->rc.nib_dims * r->rc.nib_count * 64 : 16;
    if (sc.small_tables) lds += 16 + 4 * ((size_t) sc.n_tris * (4 * MI_SHADE_WORDS));
    AoConst ac = r->ac;
    for (uint32_t j = 0; j < ac.n; ++j) {
        ac.pass = j;
        mark(r, 2, evUsed, st); mi_launch_ao(sc, r->rc, ac, Q, bd, r->gridShade, lds, st);
        mark(r, 3, evUsed, st); if (fused && ticket < MI_TICKETS) mi_launch_shadow_fused(scR, Q, Q.ticket + ticket++, st); else mi_launch_shadow(scR, Q, r->gridShadow, st);
    }
    if (ac.n > 1u) { mark(r, 2, evUsed, st); mi_launch_ao_resolve(Q, ac.recip, r->gridShadow, st); }      // (N = 1: the reciprocal is 1)
    mark(r, 0, evUsed, st);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

// trace one batch: paths = tile pixels x planes (or an explicit list), all bounces
static int traceBatch(mi_render *r, const BatchDesc &bd, const uint32_t *list, size_t &evUsed, int pool = 0) {
    const DScene &sc = r->sc; hipStream_t st = r->poolStream(pool); Queues &Q = r->pool(pool);
    (void) list;
    if (r->rc.integrator == MI_INTEGRATOR_DIRECT) return traceBatchDirect(r, bd, evUsed, pool);
    if (r->rc.integrator == MI_INTEGRATOR_AO) return traceBatchAo(r, bd, evUsed, pool);
    mark(r, 0, evUsed, st);
    const bool fused = r->rc.integrator == MI_INTEGRATOR_PATH && mi_fused_walk(sc);      // trace_fused.h: persistent waves fetch segments through per-launch tickets
    if (fused) HIPCHK(hipMemsetAsync(Q.ticket, 0, MI_TICKETS * sizeof(uint32_t), st));
    mi_launch_generate(sc, r->rc, Q, bd, r->grid, st);
    int buf = 0; const int maxDepth = r->rc.max_depth > 0 ? r->rc.max_depth : 250;
    for (int depth = 1; depth <= maxDepth; ++depth) {
        mark(r, 1, evUsed, st);
        const int ownInterval = (depth == 1 || r->rc.integrator != MI_INTEGRATOR_PATH) ? 1 : 0;      // camera rays carry the near / far clip, the volumetric stages mint = 0 at medium vertices; a surface bounce ray is (Epsilon, inf)
        if (fused && 2 * depth + 1 < MI_TICKETS) mi_launch_extend_fused(sc, Q, buf, ownInterval, Q.ticket + 2 * depth, st); else mi_launch_extend(sc, Q, buf, ownInterval, r->gridExtend, st);
        ++r->launchesAll;
        if (depth == 1 && r->nFields && !bd.list) {      // field channels of the film samples: q.hit still holds the camera hits, slot = path id (kernels_field.hip)
            mark(r, 0, evUsed, st);
            // own-pixel sums are plain read-modify-writes: wait for the previous batch's field kernel on the other stream
            if (r->fieldChain && r->lastFieldPool >= 0 && r->lastFieldPool != pool) HIPCHK(hipStreamWaitEvent(st, r->fieldDone[r->lastFieldPool], 0));
            mi_launch_field_film(sc, r->fa, Q, bd, r->fieldFilm, r->fieldSpill, st);
            if (r->fieldChain) { HIPCHK(hipEventRecord(r->fieldDone[pool], st)); r->lastFieldPool = pool; }
        }
        if (r->rc.integrator != MI_INTEGRATOR_PATH) {      // the same loop over media: its own shade and shadow stages (kernels_vol.hip, kernels_volmis.hip)
            const size_t lds = r->rc.sampler == MI_SAMPLER_SOBOL ? (size_t) r->rc.nib_dims * r->rc.nib_count * 64 : 16; const bool mis = r->rc.integrator == MI_INTEGRATOR_VOLPATH;
            mark(r, 2, evUsed, st); (mis ? mi_launch_shade_volmis : mi_launch_shade_vol)(sc, r->rc, Q, buf, r->gridShade, lds, st);
            if (depth < maxDepth || (depth == 1 && r->rc.opacity)) { mark(r, 3, evUsed, st); (mis ? mi_launch_shadow_volmis : mi_launch_shadow_vol)(sc, Q, r->gridShadow, st); }      // (depth 1 with EOpacity: the alpha walks)
        } else {
        if (depth == 1 && sc.env_texture && !r->rc.hide_emitters) mi_launch_env_primary(sc, r->rc, Q, buf, r->gridExtend, st);   // camera rays that see the sky: filtered lookup (envmap.cpp:398-411)
        mark(r, 2, evUsed, st); r->lastSorted = mi_launch_shade(sc, r->ldsTables, r->rc, Q, buf, depth == 1, r->gridShade, st, &r->lastTableBytes);
        if (depth < maxDepth) { mark(r, 3, evUsed, st); if (fused && 2 * depth + 1 < MI_TICKETS) mi_launch_shadow_fused(sc, Q, Q.ticket + 2 * depth + 1, st); else mi_launch_shadow(sc, Q, r->gridShadow, st); }
        }
        buf ^= 1;
        if (r->rc.max_depth < 0 && (depth % 4) == 0) {   // unbounded depth: poll the survivor counts every few bounces
            // survivor counts land in a pinned buffer (a true asynchronous copy), the host waits on an event of THIS stream only -- the other pool's stream keeps running
            if (r->pollWords < r->grid) { if (r->pollHost) (void) hipHostFree(r->pollHost); r->pollHost = nullptr; HIPCHK(hipHostMalloc((void **) &r->pollHost, (size_t) r->grid * 4, hipHostMallocDefault)); r->pollWords = r->grid; }
            if (!r->pollEv) HIPCHK(hipEventCreateWithFlags(&r->pollEv, hipEventDisableTiming));
            HIPCHK(hipMemcpyAsync(r->pollHost, Q.count[buf], (size_t) r->grid * 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipEventRecord(r->pollEv, st)); HIPCHK(hipEventSynchronize(r->pollEv));
            uint64_t alive = 0; for (uint32_t k = 0; k < r->grid; ++k) alive += r->pollHost[k];
            if (!alive) break;
        }
    }
    mark(r, 0, evUsed, st);
    HIPCHK(hipGetLastError());
    return MI_OK;
}

int mi_render_run(mi_render *r, mi_tile tile, uint32_t s0, uint32_t s1) { return mi_render_run_rows(r, tile, 1, s0, s1); }

// The pixels of a tile's rows y0, y0 + stride, ... below y1, and the description of one batch of sample planes over them: path pid = plane x n_pix + tile pixel.
// mi_render_run_rows and the film-unit entry (mi_render_debug_film_put) describe their batches through these two.
static uint32_t tilePixels(mi_tile tile, uint32_t rowStride) {
    const uint32_t nrows = (tile.y1 - tile.y0 + rowStride - 1) / rowStride;
    return (tile.x1 - tile.x0) * nrows;
}
static BatchDesc tileBatch(mi_tile tile, uint32_t rowStride, uint32_t npix, uint32_t sampleBegin, uint32_t nPlanes) {
    BatchDesc bd{}; bd.tile = tile; bd.n_pix = npix; bd.n_planes = nPlanes; bd.sample_begin = sampleBegin; bd.n_paths = (uint64_t) npix * nPlanes; bd.list = nullptr; bd.row_stride = rowStride;
    return bd;
}

int mi_render_run_rows(mi_render *r, mi_tile tile, uint32_t rowStride, uint32_t s0, uint32_t s1) {
    if (!r) return fail(MI_ERR_INVALID, "mi_render_run: null");
    if (rowStride == 0) return fail(MI_ERR_INVALID, "mi_render_run_rows: row stride must be >= 1");
    if (r->adaptFilm) return fail(MI_ERR_INVALID, "mi_render_run: the film holds an adaptive run (weights of one sample per pixel); call mi_render_clear first");
    const mi::SceneHost &h = r->scene->h;
    if (tile.x1 <= tile.x0 || tile.y1 <= tile.y0 || tile.x1 > h.width || tile.y1 > h.height) return fail(MI_ERR_INVALID, "mi_render_run: tile outside the film");
    if (s1 < s0 || s1 > r->p.spp) return fail(MI_ERR_INVALID, "mi_render_run: sample range outside [0, spp]");
    if (r->p.sampler == MI_SAMPLER_INDEPENDENT && s1 > (1u << 24)) return fail(MI_ERR_INVALID, "mi_render_run: independent stream supports < 2^24 samples per pixel");
    RunGuard running; { const int rc = beginRun(r, running, true, "mi_render_run"); if (rc) return rc; }
    HIPCHK(hipSetDevice(h.device));
    const uint32_t npix = tilePixels(tile, rowStride);
    uint32_t planes = r->p.planes_per_batch;
    if (!planes) { static const uint64_t target = [] { const char *v = getenv("MI355PT_BATCH_PATHS"); return v && atoll(v) > 0 ? (uint64_t) atoll(v) : (uint64_t) (64u << 20); }(); planes = (uint32_t) std::max<uint64_t>(1, target / npix); }   // ~64 M paths in flight per pool (measured: 16 M 2873, 32 M 3025, 64 M 3055, 128 M 2993 Msamples/s on C2; C4 483 / 501 / 509 / 511)
    if (planes > s1 - s0) planes = std::max<uint32_t>(1, s1 - s0);
    if (!r->p.planes_per_batch && s1 - s0 >= (uint32_t) r->nStreams) {      // automatic batches: as many as keep every path pool / stream busy, equally sized (a job of one
        const uint32_t total = s1 - s0, ns = (uint32_t) r->nStreams;        // 64 M batch would run on one stream: 1569 instead of 1712 Msamples/s on a 32-spp 1080p frame)
        uint32_t nb = (total + planes - 1) / planes; nb = (nb + ns - 1) / ns * ns;
        planes = (total + nb - 1) / nb;
    }
    uint64_t need = (uint64_t) npix * planes;
    if (need > 0xFFFFFF00ull) return fail(MI_ERR_INVALID, "mi_render_run: batch larger than 2^32 paths");
    while (need > r->poolPaths) {      // the pool only grows: a short last batch or a smaller tile reuses it
        int rc = allocPool(r, need);
        if (!rc) break;
        // not enough free device memory for pools of this size (another process on the card, a smaller part): halve the automatic batch and try again
        (void) hipGetLastError(); r->poolPaths = 0;
        if (r->p.planes_per_batch || planes <= 1) return rc;
        planes = (planes + 1) / 2; need = (uint64_t) npix * planes;
    }
    size_t evUsed = 0; r->launchesAll = 0;
    HIPCHK(hipEventRecord(r->evBegin, r->stream));
    const uint32_t nBatches = (s1 - s0 + planes - 1) / planes;
    const int nPools = (int) std::min<uint32_t>((uint32_t) r->nStreams, std::max(nBatches, 1u));      // more than one batch: round-robin over the pools / streams
    if (nPools > 1) HIPCHK(hipEventRecord(r->joinEv[0], r->stream));
    for (int i = 1; i < nPools; ++i) HIPCHK(hipStreamWaitEvent(r->poolStream(i), r->joinEv[0], 0));
    int batch = 0, lastFilmPool = -1; r->lastFieldPool = -1; r->fieldChain = nPools > 1;
    for (uint32_t s = s0; s < s1; s += planes, ++batch) {
        if (r->cancel.exchange(0)) { HIPCHK(hipDeviceSynchronize()); return fail(MI_CANCELLED, "render cancelled"); }      // consumed where it is observed
        const int pool = batch % nPools; hipStream_t st = r->poolStream(pool);
        const BatchDesc bd = tileBatch(tile, rowStride, npix, s, std::min(planes, s1 - s));
        int rc = traceBatch(r, bd, nullptr, evUsed, pool); if (rc) return rc;
        // film accumulation stays in batch order (own-pixel sums are plain read-modify-writes): wait for the previous batch's film kernel
        if (nPools > 1 && lastFilmPool >= 0) HIPCHK(hipStreamWaitEvent(st, r->filmDone[lastFilmPool], 0));
        mi_launch_film(h.d, r->pool(pool), bd, r->film, r->spill, st);
        if (nPools > 1) { HIPCHK(hipEventRecord(r->filmDone[pool], st)); lastFilmPool = pool; }
        r->samplesTotal += bd.n_paths;
    }
    for (int i = 1; i < nPools; ++i) { HIPCHK(hipEventRecord(r->joinEv[i], r->poolStream(i))); HIPCHK(hipStreamWaitEvent(r->stream, r->joinEv[i], 0)); }
    mark(r, 0, evUsed);
    HIPCHK(hipEventRecord(r->evEnd, r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
    HIPCHK(hipGetLastError());
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, r->evBegin, r->evEnd)); r->stats.render_ms = ms;
    r->stats.extend_ms = r->stats.shade_ms = r->stats.shadow_ms = r->stats.other_ms = 0; r->stats.extend_launches = 0;
    if (r->profiling) {
        for (size_t i = 0; i + 1 < evUsed; ++i) {
            float t = 0; if (hipEventElapsedTime(&t, r->evPool[i], r->evPool[i + 1]) != hipSuccess) continue;
            switch (r->evTag[i]) { case 1: r->stats.extend_ms += t; r->stats.extend_launches++; break; case 2: r->stats.shade_ms += t; break; case 3: r->stats.shadow_ms += t; break; default: r->stats.other_ms += t; }
        }
    }
    return MI_OK;
}

int mi_render_stats(mi_render *r, mi_stats *out) {
    if (!r || !out) return fail(MI_ERR_INVALID, "mi_render_stats: null");
    HIPCHK(hipSetDevice(r->scene->h.device));
    unsigned long long c[4] = {0, 0, 0, 0};
    if (r->q.counters) HIPCHK(hipMemcpy(c, r->q.counters, 32, hipMemcpyDeviceToHost));
    for (Queues &Q : r->qx) if (Q.counters) { unsigned long long c2[4]; HIPCHK(hipMemcpy(c2, Q.counters, 32, hipMemcpyDeviceToHost)); for (int i = 0; i < 4; ++i) c[i] += c2[i]; }
    r->stats.rays = c[0] + r->mergedRays; r->stats.shadow_rays = c[1] + r->mergedShadow; r->stats.path_length_sum = c[2] + r->mergedPathLen; r->stats.samples = r->samplesTotal + r->mergedSamples; r->stats.extend_rays = c[0]; r->stats.extend_launches_all = r->launchesAll;
    *out = r->stats; return MI_OK;
}

int mi_render_film_size(mi_render *r, int layout, uint32_t *height, uint32_t *width, uint32_t *channels, uint32_t *border) {
    if (!r || layout < 0 || layout > 2) return fail(MI_ERR_INVALID, "mi_render_film_size: bad argument");
    const mi::SceneHost &h = r->scene->h; const uint32_t b = (uint32_t) h.border;
    if (height) *height = layout == 2 ? h.height : h.height + 2 * b;
    if (width) *width = layout == 2 ? h.width : h.width + 2 * b;
    if (channels) *channels = layout == 0 ? 5 : (layout == 1 ? 4 : 3);
    if (border) *border = layout == 2 ? 0 : b;
    return MI_OK;
}
static size_t layoutFloats(mi_render *r, int layout) { uint32_t hh, ww, cc, bb; mi_render_film_size(r, layout, &hh, &ww, &cc, &bb); return (size_t) hh * ww * cc; }
int mi_render_read_film_device(mi_render *r, int layout, void *dev) {
    if (!r || !dev || layout < 0 || layout > 2) return fail(MI_ERR_INVALID, "mi_render_read_film_device: bad argument");
    const mi::SceneHost &h = r->scene->h; HIPCHK(hipSetDevice(h.device));
    mi_launch_film_layout(r->film, r->spill, (float *) dev, (int) h.width + 2 * h.border, (int) h.height + 2 * h.border, h.border, layout, r->stream);
    HIPCHK(hipStreamSynchronize(r->stream)); HIPCHK(hipGetLastError());
    return MI_OK;
}
int mi_render_read_film(mi_render *r, int layout, float *host) {
    if (!r || !host) return fail(MI_ERR_INVALID, "mi_render_read_film: null");
    int rc = mi_render_read_film_device(r, layout, r->layoutTmp); if (rc) return rc;
    HIPCHK(hipMemcpy(host, r->layoutTmp, layoutFloats(r, layout) * 4, hipMemcpyDeviceToHost));
    return MI_OK;
}

// dst += src (raw film sums: own-pixel planes and spill planes).  The merge step of a multi-device render, where every device renders its own rows of the
// frame (mi_render_run_rows) into its own film: the reference merges worker blocks with Film::put under a mutex (src/librender/renderproc.cpp:142-149).
// Same device: one add kernel; different devices: peer copy (xGMI, peer access enabled once per pair) into a staging buffer on dst's device, then the add; devices
// without peer access: staged through the host.  Both renders must be idle.  The host mirror calls this along a reduction tree (integrator_host.cpp).
int mi_render_merge_film(mi_render *dst, mi_render *src) {
    if (!dst || !src || dst == src) return fail(MI_ERR_INVALID, "mi_render_merge_film: two different render handles are needed");
    if (dst->adaptFilm || src->adaptFilm) return fail(MI_ERR_INVALID, "mi_render_merge_film: a film that holds an adaptive run (weights of one sample per pixel) cannot be merged");
    if (dst->filmFloats != src->filmFloats) return fail(MI_ERR_INVALID, "mi_render_merge_film: the two renders have different films");
    if (dst->nFields != src->nFields || memcmp(dst->fields, src->fields, sizeof(mi_field) * dst->nFields)) return fail(MI_ERR_INVALID, "mi_render_merge_film: the two renders hold different field lists (mi_render_set_fields)");
    const int dd = dst->scene->h.device, sd = src->scene->h.device; const size_t n = dst->filmFloats;
    HIPCHK(hipSetDevice(dd));
    const float *sFilm = src->film, *sSpill = src->spill;
    if (dd != sd) {
        // Peer access is set up once per (destination, source) pair: where the two devices can reach each other (xGMI inside a node) the add kernel's input is copied
        // device to device; where they cannot, the film is staged through a host buffer -- never silently assumed.
        if (!dst->mergeTmp) HIPCHK(hipMalloc((void **) &dst->mergeTmp, 2 * n * 4));
        int can = 0; HIPCHK(hipDeviceCanAccessPeer(&can, dd, sd));
        if (can) {
            static std::mutex peerMutex; static std::set<std::pair<int, int> > enabled;
            { std::lock_guard<std::mutex> l(peerMutex);
              if (!enabled.count({dd, sd})) { hipError_t e = hipDeviceEnablePeerAccess(sd, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(MI_ERR_DEVICE, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e)); (void) hipGetLastError(); enabled.insert({dd, sd}); } }
            HIPCHK(hipMemcpyPeerAsync(dst->mergeTmp, dd, src->film, sd, n * 4, dst->stream));
            HIPCHK(hipMemcpyPeerAsync(dst->mergeTmp + n, dd, src->spill, sd, n * 4, dst->stream));
        } else {
            std::vector<float> host(2 * n);
            HIPCHK(hipSetDevice(sd)); HIPCHK(hipMemcpy(host.data(), src->film, n * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(host.data() + n, src->spill, n * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipSetDevice(dd)); HIPCHK(hipMemcpy(dst->mergeTmp, host.data(), 2 * n * 4, hipMemcpyHostToDevice));
        }
        sFilm = dst->mergeTmp; sSpill = dst->mergeTmp + n;
    }
    mi_launch_film_add(dst->film, sFilm, n, dst->stream); mi_launch_film_add(dst->spill, sSpill, n, dst->stream);
    HIPCHK(hipStreamSynchronize(dst->stream)); HIPCHK(hipGetLastError());
    if (dst->nFields) {      // the field planes, the same way (another device: staged through the host; field films are a debugging / compositing aid, not the multi-device hot path)
        const size_t nf = dst->fieldFloats; const float *fFilm = src->fieldFilm, *fSpill = src->fieldSpill; float *stage = nullptr;
        if (dd != sd) {
            std::vector<float> host(2 * nf);
            HIPCHK(hipSetDevice(sd)); HIPCHK(hipMemcpy(host.data(), src->fieldFilm, nf * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(host.data() + nf, src->fieldSpill, nf * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipSetDevice(dd)); HIPCHK(hipMalloc((void **) &stage, 2 * nf * 4));
            if (hipMemcpy(stage, host.data(), 2 * nf * 4, hipMemcpyHostToDevice) != hipSuccess) { (void) hipFree(stage); return fail(MI_ERR_DEVICE, "mi_render_merge_film: cannot stage the field film"); }
            fFilm = stage; fSpill = stage + nf;
        }
        mi_launch_film_add(dst->fieldFilm, fFilm, nf, dst->stream); mi_launch_film_add(dst->fieldSpill, fSpill, nf, dst->stream);
        hipError_t e = hipStreamSynchronize(dst->stream); if (e == hipSuccess) e = hipGetLastError();
        if (stage) (void) hipFree(stage);
        if (e != hipSuccess) return fail(MI_ERR_DEVICE, std::string("mi_render_merge_film: ") + hipGetErrorString(e));
    }
    unsigned long long c[4]; mi_stats st{};      // the merged handle reports the sum of the ray counters too
    (void) c; if (mi_render_stats(src, &st) == MI_OK) { dst->mergedRays += st.rays; dst->mergedShadow += st.shadow_rays; dst->mergedPathLen += st.path_length_sum; dst->mergedSamples += st.samples; }
    return MI_OK;
}

int mi_render_samples(mi_render *r, const uint32_t *pairs, uint64_t n, float *outLi) {
    if (!r || !pairs || !outLi || !n) return fail(MI_ERR_INVALID, "mi_render_samples: null argument");
    const mi::SceneHost &h = r->scene->h; HIPCHK(hipSetDevice(h.device));
    for (uint64_t i = 0; i < n; ++i) if (pairs[i * 3] >= h.width || pairs[i * 3 + 1] >= h.height) return fail(MI_ERR_INVALID, "mi_render_samples: pixel outside the film");
    RunGuard running; { const int rc = beginRun(r, running, false, "mi_render_samples"); if (rc) return rc; }
    if (n > r->poolPaths) { int rc = allocPool(r, n); if (rc) return rc; }
    uint32_t *dList = nullptr; float *dOut = nullptr; uint32_t *dSlots = nullptr;
    HIPCHK(hipMalloc((void **) &dList, n * 12)); HIPCHK(hipMalloc((void **) &dOut, n * 12)); HIPCHK(hipMalloc((void **) &dSlots, n * 4));
    HIPCHK(hipMemcpy(dList, pairs, n * 12, hipMemcpyHostToDevice));
    std::vector<uint32_t> slots(n); for (uint64_t i = 0; i < n; ++i) slots[i] = (uint32_t) i;
    HIPCHK(hipMemcpy(dSlots, slots.data(), n * 4, hipMemcpyHostToDevice));
    BatchDesc bd{}; bd.tile = mi_tile{0, 0, h.width, h.height}; bd.n_pix = (uint32_t) n; bd.n_planes = 1; bd.sample_begin = 0; bd.n_paths = n; bd.list = dList; bd.row_stride = 1;
    size_t evUsed = 0; bool prof = r->profiling; r->profiling = false;
    if (!r->q.counters) return fail(MI_ERR_DEVICE, "mi_render_samples: no path pool");
    unsigned long long keep[4]; HIPCHK(hipMemcpy(keep, r->q.counters, 32, hipMemcpyDeviceToHost));     // the parity entry point leaves the ray counters untouched
    int rc = traceBatch(r, bd, dList, evUsed); r->profiling = prof;
    if (!rc) { hipError_t e = hipStreamSynchronize(r->stream); if (e == hipSuccess) e = hipMemcpy(r->q.counters, keep, 32, hipMemcpyHostToDevice); if (e != hipSuccess) rc = fail(MI_ERR_DEVICE, hipGetErrorString(e)); }
    if (!rc) { mi_launch_gather_samples(r->q, dSlots, n, dOut, r->stream); hipError_t e = hipStreamSynchronize(r->stream); if (e != hipSuccess) rc = fail(MI_ERR_DEVICE, hipGetErrorString(e)); }
    if (!rc) { hipError_t e = hipMemcpy(outLi, dOut, n * 12, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = fail(MI_ERR_DEVICE, hipGetErrorString(e)); }
    (void) hipFree(dList); (void) hipFree(dOut); (void) hipFree(dSlots);
    return rc;
}

// ------------------------------------------------------------------------------------------------ adaptive sampling (adaptive.h, kernels_adaptive.hip)
// approx_erfinv of adaptive.cpp:26-60 (M. Giles' single-precision polynomial): its constants and operation order are part of the arithmetic contract, like the BSDF numerics
static float approxErfinv(float x) {
    float w = -std::log((1.0f - x) * (1.0f + x)), p;
    if (w < 5.000000f) {
        w = w - 2.500000f;
        p = 2.81022636e-08f; p = 3.43273939e-07f + p * w; p = -3.5233877e-06f + p * w; p = -4.39150654e-06f + p * w; p = 0.00021858087f + p * w;
        p = -0.00125372503f + p * w; p = -0.00417768164f + p * w; p = 0.246640727f + p * w; p = 1.50140941f + p * w;
    } else {
        w = sqrtf(w) - 3.000000f;
        p = -0.000200214257f; p = 0.000100950558f + p * w; p = 0.00134934322f + p * w; p = -0.00367342844f + p * w; p = 0.00573950773f + p * w;
        p = -0.0076224613f + p * w; p = 0.00943887047f + p * w; p = 1.00167406f + p * w; p = 2.83297682f + p * w;
    }
    return p * x;
}
static const uint32_t kAdaptLastIndex = (1u << 24) - 1u;      // last index of the independent stream: kept for the luminance estimate, never reached by a render
static bool filmHoldsSamples(const mi_render *r) { return r->samplesTotal || r->mergedSamples || r->adaptFilm; }
static void releaseAdaptive(mi_render *r) {
    void *ps[] = {r->ad.fp, r->ad.ms, r->ad.n, r->ad.counts, r->adActive[0], r->adActive[1], r->adWave, r->adNNext};
    for (void *p : ps) if (p) (void) hipFree(p);
    for (uint32_t *&l : r->adList) { if (l) (void) hipFree(l); l = nullptr; }
    if (r->adHostN) (void) hipHostFree(r->adHostN);
    r->ad = AdaptArgs{}; r->adActive[0] = r->adActive[1] = r->adWave = r->adNNext = r->adHostN = nullptr; r->adListPaths = 0; r->adPix = 0;
}
int mi_render_set_adaptive(mi_render *r, const mi_adaptive_params *p) {
    if (!r) return fail(MI_ERR_INVALID, "mi_render_set_adaptive: null render");
    if (filmHoldsSamples(r)) return fail(MI_ERR_INVALID, "mi_render_set_adaptive: the film holds samples (set the adaptive parameters after mi_render_create or mi_render_clear)");
    if (!p) { r->adaptOn = false; return MI_OK; }
    if (r->p.sampler != MI_SAMPLER_INDEPENDENT) return fail(MI_ERR_UNSUPPORTED, "The error-controlling integrator should only be used in conjunction with the independent sampler");      // adaptive.cpp:150-152
    if (r->p.spp < 8) return fail(MI_ERR_INVALID, "Starting the adaptive integrator with less than 8 samples per pixel does not make much sense -- giving up.");      // :210-212
    if (r->p.integrator == MI_INTEGRATOR_DIRECT || r->p.integrator == MI_INTEGRATOR_AO)
        return fail(MI_ERR_UNSUPPORTED, "mi_render_set_adaptive: adaptive sampling over the direct and ao integrators is not implemented (their adaptive queries renumber the sample arrays, direct.cpp:192, ao.cpp:102); use path, volpath_simple or volpath");
    if (r->nFields && (r->fa.needs & MI_FIELD_MOTION_KINDS)) return fail(MI_ERR_UNSUPPORTED, "mi_render_set_adaptive: the prevPosition / motion fields are set on this render (mi_render_set_fields); adaptive sampling fills no field film and does not follow the frame mark");
    if (r->nFields) return fail(MI_ERR_UNSUPPORTED, "mi_render_set_adaptive: field channels are set on this render (mi_render_set_fields); adaptive sampling does not fill a field film");
    if (p->max_sample_factor == 0) return fail(MI_ERR_INVALID, "mi_render_set_adaptive: max_sample_factor must not be 0 (negative: no cap, positive: at most max_sample_factor x spp samples per pixel)");
    if (!(p->max_error >= 0)) return fail(MI_ERR_INVALID, "mi_render_set_adaptive: max_error must be >= 0");
    if (!(p->p_value > 0 && p->p_value < 1)) return fail(MI_ERR_INVALID, "mi_render_set_adaptive: p_value must lie in (0, 1)");
    if (p->max_sample_factor > 0 && (uint64_t) p->max_sample_factor * r->p.spp >= kAdaptLastIndex)
        return fail(MI_ERR_INVALID, "mi_render_set_adaptive: max_sample_factor x spp reaches the end of the independent stream (2^24 - 1 samples per pixel; the last index is kept for the luminance estimate)");
    r->ap = *p; r->adaptOn = true;
    r->adQuantile = std::fabs(approxErfinv(-1 + p->p_value)) * 1.41421356237309504880f;      // the reference omits the absolute value: its quantile is negative (include/mi355pt.h)
    return MI_OK;
}
int mi_render_read_sample_counts(mi_render *r, uint32_t *out) {
    if (!r || !out) return fail(MI_ERR_INVALID, "mi_render_read_sample_counts: null argument");
    const mi::SceneHost &h = r->scene->h; const size_t n = (size_t) h.width * h.height;
    if (!r->ad.counts || !r->adaptFilm) { memset(out, 0, n * 4); return MI_OK; }      // nothing rendered adaptively since the last clear
    HIPCHK(hipSetDevice(h.device)); HIPCHK(hipMemcpy(out, r->ad.counts, n * 4, hipMemcpyDeviceToHost));
    return MI_OK;
}
int mi_render_adaptive_stats(mi_render *r, mi_adaptive_stats *out) {
    if (!r || !out) return fail(MI_ERR_INVALID, "mi_render_adaptive_stats: null argument");
    *out = r->as; return MI_OK;
}
}  // extern "C"
// The set-up of an adaptive film, shared by mi_render_run_adaptive and the film-unit entry (mi_render_debug_film_put), in two steps.
// adaptAlloc: the footprint, state and count buffers, allocated at the first adaptive run and freed with the render.
static int adaptAlloc(mi_render *r, const std::string &who) {
    if (r->ad.fp) return MI_OK;
    const mi::SceneHost &h = r->scene->h; const uint32_t nPixFilm = h.width * h.height;
    const int hb = (int) std::floor(h.filterRadiusEff + 0.5f), side = 2 * hb + 1;
    const uint64_t fpBytes = (uint64_t) nPixFilm * side * side * 5u * 4u, bytes = fpBytes + (uint64_t) nPixFilm * (8u + 4u + 4u + 4u + 4u) + MI_ADAPT_RANGES * 4u + 4u;
    const char *lim = getenv("MI355PT_POOL_LIMIT");
    if (lim && atoll(lim) > 0 && bytes > (uint64_t) atoll(lim)) return fail(MI_ERR_DEVICE, who + ": the footprint, state and count buffers (" + std::to_string(bytes) + " bytes) are larger than MI355PT_POOL_LIMIT");
    size_t freeB = 0, totalB = 0; HIPCHK(hipMemGetInfo(&freeB, &totalB));
    if (bytes > freeB) return fail(MI_ERR_DEVICE, who + ": the footprint, state and count buffers (" + std::to_string(bytes) + " bytes) are larger than the free device memory");
    hipError_t e = hipMalloc((void **) &r->ad.fp, fpBytes);
    if (e == hipSuccess) e = hipMalloc((void **) &r->ad.ms, (size_t) nPixFilm * 8);
    if (e == hipSuccess) e = hipMalloc((void **) &r->ad.n, (size_t) nPixFilm * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &r->ad.counts, (size_t) nPixFilm * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &r->adActive[0], (size_t) nPixFilm * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &r->adActive[1], (size_t) nPixFilm * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &r->adWave, MI_ADAPT_RANGES * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &r->adNNext, 4);
    if (e == hipSuccess) e = hipHostMalloc((void **) &r->adHostN, 4, hipHostMallocDefault);
    if (e != hipSuccess) { (void) hipGetLastError(); releaseAdaptive(r); return fail(MI_ERR_DEVICE, who + ": cannot allocate the footprint, state and count buffers: " + hipGetErrorString(e)); }
    r->adPix = nPixFilm;
    return MI_OK;
}
static uint32_t adaptCap(const mi_render *r) { return r->ap.max_sample_factor > 0 ? (uint32_t) r->ap.max_sample_factor * r->p.spp : kAdaptLastIndex - 1u; }
// adaptBegin: the kernels' arguments from the adaptive parameters and the average luminance, zeroed footprints / state / counts, the round-0 active list = the tile's
// pixels row by row; from here on the film is an adaptive one.
static int adaptBegin(mi_render *r, mi_tile tile, uint32_t npix, float avgLum) {
    const mi::SceneHost &h = r->scene->h; const uint32_t nPixFilm = h.width * h.height;
    const int hb = (int) std::floor(h.filterRadiusEff + 0.5f), side = 2 * hb + 1;
    r->ad.n_pix = nPixFilm; r->ad.hb = hb; r->ad.spp = r->p.spp; r->ad.cap = adaptCap(r); r->ad.max_error = r->ap.max_error; r->ad.quantile = r->adQuantile; r->ad.lum_floor = avgLum * 0.01f;
    r->as = mi_adaptive_stats{}; r->as.average_luminance = avgLum; r->as.quantile = r->adQuantile;
    r->adaptFilm = true;      // from here on the film is an adaptive one, whether the run completes or not
    HIPCHK(hipMemsetAsync(r->ad.fp, 0, (size_t) nPixFilm * side * side * 5u * 4u, r->stream)); HIPCHK(hipMemsetAsync(r->ad.ms, 0, (size_t) nPixFilm * 8, r->stream));
    HIPCHK(hipMemsetAsync(r->ad.n, 0, (size_t) nPixFilm * 4, r->stream)); HIPCHK(hipMemsetAsync(r->ad.counts, 0, (size_t) nPixFilm * 4, r->stream));
    mi_launch_adapt_tile(r->adActive[0], tile, h.width, npix, r->stream);
    return MI_OK;
}
extern "C" {
int mi_render_run_adaptive(mi_render *r, mi_tile tile) {
    if (!r) return fail(MI_ERR_INVALID, "mi_render_run_adaptive: null render");
    if (!r->adaptOn) return fail(MI_ERR_INVALID, "mi_render_run_adaptive: no adaptive parameters are set (mi_render_set_adaptive)");
    const mi::SceneHost &h = r->scene->h;
    if (tile.x1 <= tile.x0 || tile.y1 <= tile.y0 || tile.x1 > h.width || tile.y1 > h.height) return fail(MI_ERR_INVALID, "mi_render_run_adaptive: tile outside the film");
    if (filmHoldsSamples(r)) return fail(MI_ERR_INVALID, "mi_render_run_adaptive: the film holds samples; an adaptive run needs a clear film (one adaptive run per mi_render_clear)");
    if (r->nFields) return fail(MI_ERR_UNSUPPORTED, "mi_render_run_adaptive: field channels are set on this render (mi_render_set_fields)");
    HIPCHK(hipSetDevice(h.device));
    const uint32_t spp = r->p.spp, R = r->ap.round_samples ? r->ap.round_samples : spp;
    const uint32_t cap = adaptCap(r);
    const uint32_t nPixFilm = h.width * h.height, npix = tilePixels(tile, 1);
    { const int rc = adaptAlloc(r, "mi_render_run_adaptive"); if (rc) return rc; }
    // average luminance: given, or the estimate over N = min(10000, W x H) pixels at the stream's last sample index, through the route of mi_render_samples (taken again
    // at every run: the scene may have been edited); summed in double in index order
    float avgLum = r->ap.average_luminance;
    if (!(avgLum > 0)) {
        const uint64_t wh = nPixFilm, N = std::min<uint64_t>(10000u, wh);
        std::vector<uint32_t> pairs(N * 3); std::vector<float> li(N * 3);
        for (uint64_t i = 0; i < N; ++i) { const uint64_t p = i * wh / N; pairs[i * 3] = (uint32_t) (p % h.width); pairs[i * 3 + 1] = (uint32_t) (p / h.width); pairs[i * 3 + 2] = kAdaptLastIndex; }
        { const int rc = mi_render_samples(r, pairs.data(), N, li.data()); if (rc) return rc; }
        double sum = 0; for (uint64_t i = 0; i < N; ++i) sum += (double) (li[i * 3] * 0.212671f + li[i * 3 + 1] * 0.715160f + li[i * 3 + 2] * 0.072169f);
        avgLum = (float) (sum / (double) N);
    }
    RunGuard running; { const int rc = beginRun(r, running, true, "mi_render_run_adaptive"); if (rc) return rc; }
    // batches: a round of R sample indices over nAct pixels is cut into batches of `planes` indices that fit the pool, as mi_render_run_rows cuts the planes of a tile
    uint32_t planes = r->p.planes_per_batch;
    if (!planes) { const char *v = getenv("MI355PT_BATCH_PATHS"); const uint64_t target = v && atoll(v) > 0 ? (uint64_t) atoll(v) : (uint64_t) (64u << 20); planes = (uint32_t) std::max<uint64_t>(1, target / npix); }
    planes = std::min(planes, std::min(R, cap));
    if (!r->p.planes_per_batch && planes < R && R <= cap) { const uint32_t ns = (uint32_t) r->nStreams; uint32_t nb = (R + planes - 1) / planes; nb = (nb + ns - 1) / ns * ns; planes = (R + nb - 1) / nb; }
    uint64_t need = (uint64_t) npix * planes;
    if (need > 0xFFFFFF00ull) return fail(MI_ERR_INVALID, "mi_render_run_adaptive: batch larger than 2^32 paths");
    while (need > r->poolPaths) {
        int rc = allocPool(r, need);
        if (!rc) break;
        (void) hipGetLastError(); r->poolPaths = 0;
        if (r->p.planes_per_batch || planes <= 1) return rc;
        planes = (planes + 1) / 2; need = (uint64_t) npix * planes;
    }
    const int nPools = r->nStreams;
    if (need > r->adListPaths || !r->adList[nPools - 1]) {
        for (uint32_t *&l : r->adList) { if (l) (void) hipFree(l); l = nullptr; }
        r->adListPaths = 0;
        for (int i = 0; i < nPools; ++i) HIPCHK(hipMalloc((void **) &r->adList[i], need * 12));
        r->adListPaths = need;
    }
    { const int rc = adaptBegin(r, tile, npix, avgLum); if (rc) return rc; }
    size_t evUsed = 0; r->launchesAll = 0;
    HIPCHK(hipEventRecord(r->evBegin, r->stream));
    if (nPools > 1) HIPCHK(hipEventRecord(r->joinEv[0], r->stream));
    for (int i = 1; i < nPools; ++i) HIPCHK(hipStreamWaitEvent(r->poolStream(i), r->joinEv[0], 0));
    uint32_t nAct = npix, begin = 0; int cur = 0, batch = 0, lastPool = -1; uint64_t traced = 0; uint32_t rounds = 0;
    while (nAct) {
        const uint32_t roundLen = std::min(R, cap - begin);      // (begin < cap while a pixel is active: every pixel stops at cap)
        for (uint32_t s = 0; s < roundLen; s += planes, ++batch) {
            if (r->cancel.exchange(0)) { HIPCHK(hipDeviceSynchronize()); return fail(MI_CANCELLED, "render cancelled"); }
            const int pool = batch % nPools; hipStream_t st = r->poolStream(pool);
            BatchDesc bd{}; bd.tile = mi_tile{0, 0, h.width, h.height}; bd.n_pix = nAct; bd.n_planes = std::min(planes, roundLen - s); bd.sample_begin = begin + s;
            bd.n_paths = (uint64_t) nAct * bd.n_planes; bd.list = r->adList[pool]; bd.row_stride = 1;
            mi_launch_adapt_list(r->adActive[cur], nAct, bd.n_paths, bd.sample_begin, h.width, r->adList[pool], st);
            { const int rc = traceBatch(r, bd, bd.list, evUsed, pool); if (rc) return rc; }
            // a pixel's state and footprint are plain read-modify-writes in sample order: the accumulate kernels run in batch order, chained as filmDone chains k_film
            if (nPools > 1 && lastPool >= 0 && lastPool != pool) HIPCHK(hipStreamWaitEvent(st, r->filmDone[lastPool], 0));
            mi_launch_adapt_accumulate(h.d, r->pool(pool), r->ad, r->adActive[cur], nAct, bd.n_planes, r->film, r->spill, st);
            if (nPools > 1) { HIPCHK(hipEventRecord(r->filmDone[pool], st)); lastPool = pool; }
            mark(r, 0, evUsed, st);
            r->samplesTotal += bd.n_paths; traced += bd.n_paths;
        }
        // the next active list, behind the round's last accumulate kernel (which waited for all before it); one 4-byte read-back sizes the next round
        hipStream_t st = r->poolStream(lastPool < 0 ? 0 : lastPool);
        mi_launch_adapt_compact(r->adActive[cur], nAct, r->ad.counts, r->adWave, r->adActive[cur ^ 1], r->adNNext, st);
        HIPCHK(hipMemcpyAsync(r->adHostN, r->adNNext, 4, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipGetLastError());
        if (*r->adHostN > nAct) return fail(MI_ERR_DEVICE, "mi_render_run_adaptive: the compaction returned more pixels than it was given");
        nAct = *r->adHostN; cur ^= 1; begin += roundLen; ++rounds;
    }
    for (int i = 1; i < nPools; ++i) { HIPCHK(hipEventRecord(r->joinEv[i], r->poolStream(i))); HIPCHK(hipStreamWaitEvent(r->stream, r->joinEv[i], 0)); }
    mark(r, 0, evUsed);
    HIPCHK(hipEventRecord(r->evEnd, r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
    HIPCHK(hipGetLastError());
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, r->evBegin, r->evEnd)); r->stats.render_ms = ms;
    r->stats.extend_ms = r->stats.shade_ms = r->stats.shadow_ms = r->stats.other_ms = 0; r->stats.extend_launches = 0;
    if (r->profiling) {
        for (size_t i = 0; i + 1 < evUsed; ++i) {
            float t = 0; if (hipEventElapsedTime(&t, r->evPool[i], r->evPool[i + 1]) != hipSuccess) continue;
            switch (r->evTag[i]) { case 1: r->stats.extend_ms += t; r->stats.extend_launches++; break; case 2: r->stats.shade_ms += t; break; case 3: r->stats.shadow_ms += t; break; default: r->stats.other_ms += t; }
        }
    }
    std::vector<uint32_t> counts(nPixFilm); HIPCHK(hipMemcpy(counts.data(), r->ad.counts, (size_t) nPixFilm * 4, hipMemcpyDeviceToHost));
    r->as.samples_traced = traced; r->as.rounds = rounds; r->as.min_count = 0xFFFFFFFFu;
    for (uint32_t y = tile.y0; y < tile.y1; ++y) for (uint32_t x = tile.x0; x < tile.x1; ++x) {
        const uint32_t c = counts[(size_t) y * h.width + x];
        r->as.samples_used += c; r->as.min_count = std::min(r->as.min_count, c); r->as.max_count = std::max(r->as.max_count, c); if (c == cap) ++r->as.pixels_at_cap;
    }
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ film units (include/mi355pt.h)
// Caller-supplied samples through the film kernels a render launches: pool 0 sized as a run sizes it, the samples copied into its q.pos / q.acc, the batches described by
// tileBatch as mi_render_run_rows describes them, the product's launchers on the render's stream.  No kernel of its own.
int mi_render_debug_film_put(mi_render *r, int which, mi_tile tile, uint32_t rowStride, uint32_t nPlanes, uint32_t batchPlanes, const float *pos2, const float *val4) {
    const std::string fn = "mi_render_debug_film_put";
    if (!r || !pos2 || !val4) return fail(MI_ERR_INVALID, fn + ": null argument");
    if (which < 0 || which > 2) return fail(MI_ERR_INVALID, fn + ": which must be 0 (k_film), 1 (k_adapt_accumulate) or 2 (k_field_film)");
    if (rowStride == 0) return fail(MI_ERR_INVALID, fn + ": row stride must be >= 1");
    if (nPlanes == 0) return fail(MI_ERR_INVALID, fn + ": n_planes must be >= 1");
    const mi::SceneHost &h = r->scene->h;
    if (tile.x1 <= tile.x0 || tile.y1 <= tile.y0 || tile.x1 > h.width || tile.y1 > h.height) return fail(MI_ERR_INVALID, fn + ": tile outside the film");
    if (r->scene->busy.load() != 0) return fail(MI_ERR_INVALID, fn + ": a render is running on this scene (or the scene is being updated)");
    if (which == 0 && r->adaptFilm) return fail(MI_ERR_INVALID, fn + ": the film holds an adaptive run (weights of one sample per pixel); call mi_render_clear first");
    if (which == 1) {
        if (!r->adaptOn) return fail(MI_ERR_INVALID, fn + ": which = 1 needs adaptive parameters (mi_render_set_adaptive)");
        if (!(r->ap.average_luminance > 0)) return fail(MI_ERR_INVALID, fn + ": which = 1 needs a given average_luminance > 0 (there is no scene to estimate it from)");
        if (filmHoldsSamples(r)) return fail(MI_ERR_INVALID, fn + ": which = 1 needs a clear film (one adaptive film per mi_render_clear)");
        if (r->nFields) return fail(MI_ERR_INVALID, fn + ": which = 1 needs a render without field channels (mi_render_set_fields)");
        if (rowStride != 1) return fail(MI_ERR_INVALID, fn + ": which = 1 needs row_stride = 1 (the active list is the tile, row by row)");
        if (adaptCap(r) != nPlanes) return fail(MI_ERR_INVALID, fn + ": which = 1 needs n_planes = max_sample_factor x spp, so that every pixel has stopped by the last plane");
    }
    if (which == 2) {
        if (!r->nFields) return fail(MI_ERR_INVALID, fn + ": which = 2 needs fields (mi_render_set_fields)");
        if (r->adaptFilm) return fail(MI_ERR_INVALID, fn + ": the film holds an adaptive run; call mi_render_clear first");
    }
    const uint32_t npix = tilePixels(tile, rowStride);
    const uint64_t total = (uint64_t) npix * nPlanes;
    // the kernels' clamps make any finite position safe; the bound keeps the conversions to int defined in a CPU model too
    for (uint64_t i = 0; i < total * 2; ++i) if (!(std::fabs(pos2[i]) <= 1048576.0f)) return fail(MI_ERR_INVALID, fn + ": a film position is not finite or lies beyond 2^20");
    const uint32_t planes = batchPlanes ? std::min(batchPlanes, nPlanes) : nPlanes;
    const uint64_t need = (uint64_t) npix * planes;
    if (need > 0xFFFFFF00ull) return fail(MI_ERR_INVALID, fn + ": batch larger than 2^32 paths");
    HIPCHK(hipSetDevice(h.device));
    if (which == 1) { const int rc = adaptAlloc(r, fn); if (rc) return rc; }
    RunGuard running; { const int rc = beginRun(r, running, true, fn.c_str()); if (rc) return rc; }
    if (need > r->poolPaths) { const int rc = allocPool(r, need); if (rc) return rc; }
    Queues &Q = r->q; hipStream_t st = r->stream;
    if (which == 1) { const int rc = adaptBegin(r, tile, npix, r->ap.average_luminance); if (rc) return rc; }
    for (uint32_t s = 0; s < nPlanes; s += planes) {
        const BatchDesc bd = tileBatch(tile, rowStride, npix, s, std::min(planes, nPlanes - s));
        const uint64_t first = (uint64_t) s * npix;
        HIPCHK(hipMemcpy(Q.pos, pos2 + first * 2, bd.n_paths * sizeof(float2), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(Q.acc, val4 + first * 4, bd.n_paths * sizeof(float4), hipMemcpyHostToDevice));
        if (which == 2) HIPCHK(hipMemsetAsync(Q.hit, 0xFF, bd.n_paths * sizeof(float4), st));      // every camera ray leaves the scene (hit.w = 0xFFFFFFFF): the fields' `undefined` values
        if (which == 0) mi_launch_film(h.d, Q, bd, r->film, r->spill, st);
        else if (which == 1) mi_launch_adapt_accumulate(h.d, Q, r->ad, r->adActive[0], npix, bd.n_planes, r->film, r->spill, st);      // the full list every time: a finished pixel returns at once
        else mi_launch_field_film(r->sc, r->fa, Q, bd, r->fieldFilm, r->fieldSpill, st);
        HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipGetLastError());
        r->samplesTotal += bd.n_paths;
    }
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ field channels (kernels_field.hip)
int mi_render_set_fields(mi_render *r, const mi_field *fields, uint32_t n) {
    if (!r || (n && !fields)) return fail(MI_ERR_INVALID, "mi_render_set_fields: null argument");
    if (n > MI_MAX_FIELDS) return fail(MI_ERR_INVALID, "mi_render_set_fields: at most 8 fields");
    if (r->samplesTotal || r->mergedSamples) return fail(MI_ERR_INVALID, "mi_render_set_fields: the film holds samples (set the fields after mi_render_create or mi_render_clear)");
    const mi::SceneHost &h = r->scene->h; HIPCHK(hipSetDevice(h.device));
    uint32_t needs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (fields[i].field > MI_FIELD_MOTION) return fail(MI_ERR_UNSUPPORTED, "mi_render_set_fields: unknown field kind " + std::to_string(fields[i].field) + " (position, relPosition, distance, geoNormal, shNormal, uv, albedo, shapeIndex, primIndex, prevPosition, motion = 0..10)");
        needs |= 1u << fields[i].field;
    }
    if (needs & (1u << MI_FIELD_ALBEDO)) {
        for (const mi_material &m : h.materials) {
            const char *name = m.type == MI_BSDF_PLASTIC ? "plastic" : m.type == MI_BSDF_ROUGHPLASTIC ? "roughplastic" : m.type == MI_BSDF_COATING ? "coating" : m.type == MI_BSDF_ROUGHCOATING ? "roughcoating" : nullptr;
            if (name) return fail(MI_ERR_UNSUPPORTED, std::string("mi_render_set_fields: the albedo field is not implemented for the BSDF `") + name + "` (its external transmittance is not part of the material record)");
            if (m.type == MI_BSDF_MASK && m.distr < h.materials.size() && (h.materials[m.distr].type == MI_BSDF_BUMPMAP || h.materials[m.distr].type == MI_BSDF_NORMALMAP))
                return fail(MI_ERR_UNSUPPORTED, "mi_render_set_fields: the albedo field is not implemented for a `mask` over a bumpmap / normalmap (the generic rule evaluates the nested BSDF in the perturbed frame)");
        }
    }
    releaseFields(r);
    if (!n) return MI_OK;
    FieldArgs fa{}; fa.n = n; fa.needs = needs; fa.n_meshes = (uint32_t) h.shapes.size();
    for (uint32_t i = 0; i < n; ++i) { fa.kind[i] = fields[i].field; memcpy(fa.undefined[i], fields[i].undefined, 12); }
    if (!worldToCamera(h, fa.w2c) && (needs & (1u << MI_FIELD_REL_POSITION))) return fail(MI_ERR_INVALID, "mi_render_set_fields: relPosition needs an invertible camera transform");
    if ((needs & MI_FIELD_MOTION_KINDS) && r->adaptOn) return fail(MI_ERR_UNSUPPORTED, "mi_render_set_fields: prevPosition / motion on an adaptive render (mi_render_set_adaptive): adaptive sampling fills no field film and does not follow the frame mark");
    { const int rc = fieldMotionArgs("mi_render_set_fields", h, fa); if (rc) return rc; }
    struct Undo { mi_render *r; ~Undo() { if (r) releaseFields(r); } } undo{r};
    if (needs & (1u << MI_FIELD_SHAPE_INDEX)) {
        std::vector<int32_t> ts(std::max<size_t>(h.idx.size() / 3, 1), -1);
        for (size_t si = 0; si < h.shapes.size(); ++si) for (uint32_t k = 0; k < h.shapes[si].tri_count; ++k) ts[h.shapes[si].first_tri + k] = h.shapes[si].group ? -1 : (int32_t) si;
        HIPCHK(hipMalloc((void **) &r->dTriShape, ts.size() * 4)); HIPCHK(hipMemcpy(r->dTriShape, ts.data(), ts.size() * 4, hipMemcpyHostToDevice));
        fa.tri_shape = r->dTriShape;
    }
    const size_t W = h.width + 2 * (size_t) h.border, H = h.height + 2 * (size_t) h.border; const size_t floats = W * H * (3 * (size_t) n + 1);
    HIPCHK(hipMalloc((void **) &r->fieldFilm, floats * 4)); HIPCHK(hipMalloc((void **) &r->fieldSpill, floats * 4)); HIPCHK(hipMalloc((void **) &r->fieldTmp, floats * 4));
    HIPCHK(hipMemset(r->fieldFilm, 0, floats * 4)); HIPCHK(hipMemset(r->fieldSpill, 0, floats * 4));
    for (int i = 0; i < r->nStreams; ++i) HIPCHK(hipEventCreateWithFlags(&r->fieldDone[i], hipEventDisableTiming));
    r->fieldFloats = floats; r->fa = fa; r->nFields = n; memset(r->fields, 0, sizeof(r->fields)); memcpy(r->fields, fields, sizeof(mi_field) * n);
    undo.r = nullptr;
    return MI_OK;
}
int mi_render_field_film_size(mi_render *r, int layout, uint32_t *height, uint32_t *width, uint32_t *channels, uint32_t *border) {
    if (!r || (layout != 0 && layout != 2)) return fail(MI_ERR_INVALID, "mi_render_field_film_size: bad argument (layouts 0 and 2)");
    if (!r->nFields) return fail(MI_ERR_INVALID, "mi_render_field_film_size: the render has no fields (mi_render_set_fields)");
    const mi::SceneHost &h = r->scene->h; const uint32_t b = (uint32_t) h.border;
    if (height) *height = layout == 2 ? h.height : h.height + 2 * b;
    if (width) *width = layout == 2 ? h.width : h.width + 2 * b;
    if (channels) *channels = layout == 0 ? 3 * r->nFields + 1 : 3 * r->nFields;
    if (border) *border = layout == 2 ? 0 : b;
    return MI_OK;
}
int mi_render_read_fields(mi_render *r, int layout, float *host) {
    if (!r || !host || (layout != 0 && layout != 2)) return fail(MI_ERR_INVALID, "mi_render_read_fields: bad argument (layouts 0 and 2)");
    if (!r->nFields) return fail(MI_ERR_INVALID, "mi_render_read_fields: the render has no fields (mi_render_set_fields)");
    const mi::SceneHost &h = r->scene->h; HIPCHK(hipSetDevice(h.device));
    uint32_t hh, ww, cc, bb; mi_render_field_film_size(r, layout, &hh, &ww, &cc, &bb);
    mi_launch_field_layout(r->fieldFilm, r->fieldSpill, r->fieldTmp, (int) h.width + 2 * h.border, (int) h.height + 2 * h.border, h.border, (int) (3 * r->nFields + 1), layout, r->stream);
    HIPCHK(hipStreamSynchronize(r->stream)); HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(host, r->fieldTmp, (size_t) hh * ww * cc * 4, hipMemcpyDeviceToHost));
    return MI_OK;
}
int mi_render_field_samples(mi_render *r, const uint32_t *pairs, uint64_t n, float *out) {
    if (!r || !pairs || !out || !n) return fail(MI_ERR_INVALID, "mi_render_field_samples: null argument");
    if (!r->nFields) return fail(MI_ERR_INVALID, "mi_render_field_samples: the render has no fields (mi_render_set_fields)");
    const mi::SceneHost &h = r->scene->h; HIPCHK(hipSetDevice(h.device));
    for (uint64_t i = 0; i < n; ++i) if (pairs[i * 3] >= h.width || pairs[i * 3 + 1] >= h.height) return fail(MI_ERR_INVALID, "mi_render_field_samples: pixel outside the film");
    RunGuard running; { const int rc = beginRun(r, running, false, "mi_render_field_samples"); if (rc) return rc; }
    if (n > r->poolPaths) { int rc = allocPool(r, n); if (rc) return rc; }
    if (!r->q.counters) return fail(MI_ERR_DEVICE, "mi_render_field_samples: no path pool");
    const size_t outBytes = (size_t) n * 3 * r->nFields * 4;
    uint32_t *dList = nullptr; float *dOut = nullptr;
    HIPCHK(hipMalloc((void **) &dList, n * 12));
    if (hipMalloc((void **) &dOut, outBytes) != hipSuccess) { (void) hipFree(dList); return fail(MI_ERR_DEVICE, "mi_render_field_samples: out of device memory"); }
    BatchDesc bd{}; bd.tile = mi_tile{0, 0, h.width, h.height}; bd.n_pix = (uint32_t) n; bd.n_planes = 1; bd.sample_begin = 0; bd.n_paths = n; bd.list = dList; bd.row_stride = 1;
    const DScene &sc = r->sc; Queues &Q = r->q; hipStream_t st = r->stream; unsigned long long keep[4];
    hipError_t e = hipMemcpy(dList, pairs, n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(keep, Q.counters, 32, hipMemcpyDeviceToHost);      // like mi_render_samples, the parity entry point leaves the ray counters untouched
    if (e == hipSuccess) {
        const bool fused = !isVolumetric(r->rc.integrator) && mi_fused_walk(sc);
        if (fused) e = hipMemsetAsync(Q.ticket, 0, MI_TICKETS * sizeof(uint32_t), st);
        if (e == hipSuccess) {
            mi_launch_generate(sc, r->rc, Q, bd, r->grid, st);
            if (fused) mi_launch_extend_fused(sc, Q, 0, 1, Q.ticket + 2, st); else mi_launch_extend(sc, Q, 0, 1, r->gridExtend, st);
            mi_launch_field_samples(sc, r->fa, Q, n, dOut, st);
            e = hipStreamSynchronize(st); if (e == hipSuccess) e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipMemcpy(Q.counters, keep, 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);
    (void) hipFree(dList); (void) hipFree(dOut);
    if (e != hipSuccess) return fail(MI_ERR_DEVICE, std::string("mi_render_field_samples: ") + hipGetErrorString(e));
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ denoiser (denoise.h, kernels_denoise.hip)
}  // extern "C"
static int dnCheckParams(const std::string &fn, const mi_denoise_params *p) {
    if (p->iterations > 8) return fail(MI_ERR_INVALID, fn + ": iterations must be 0..8 (got " + std::to_string(p->iterations) + ")");
    if (!(p->sigma_color > 0) || !std::isfinite(p->sigma_color)) return fail(MI_ERR_INVALID, fn + ": sigma_color must be positive and finite");
    if (!(p->sigma_normal > 0) || !std::isfinite(p->sigma_normal)) return fail(MI_ERR_INVALID, fn + ": sigma_normal must be positive and finite");
    if (p->sigma_position == 0 || !std::isfinite(p->sigma_position)) return fail(MI_ERR_INVALID, fn + ": sigma_position must be non-zero and finite (negative: a fraction of the position box's diagonal)");
    if (p->demodulate > 1) return fail(MI_ERR_INVALID, fn + ": demodulate must be 0 or 1");
    return MI_OK;
}
static int dnCheckSize(const std::string &fn, uint32_t width, uint32_t height) {
    if (!width || !height) return fail(MI_ERR_INVALID, fn + ": zero width or height");
    if (width > (1u << 24) || height > 65535u * MI_DN_TILE_H) return fail(MI_ERR_INVALID, fn + ": width above 2^24 or height above " + std::to_string(65535u * MI_DN_TILE_H));
    return MI_OK;
}
// two colour buffers, the packed guides, the divisor and the partial boxes in ONE allocation
static int dnAlloc(const std::string &fn, size_t n, void **mem, DenoiseBufs *b) {
    const uint64_t bytes = (uint64_t) n * MI_DN_BYTES_PER_PIXEL + MI_DN_TAIL_FLOATS * 4u;
    const char *lim = getenv("MI355PT_POOL_LIMIT");
    if (lim && atoll(lim) > 0 && bytes > (uint64_t) atoll(lim)) return fail(MI_ERR_DEVICE, fn + ": the colour and guide buffers (" + std::to_string(bytes) + " bytes) are larger than MI355PT_POOL_LIMIT");
    size_t freeB = 0, totalB = 0; HIPCHK(hipMemGetInfo(&freeB, &totalB));
    if (bytes > freeB) return fail(MI_ERR_DEVICE, fn + ": the colour and guide buffers (" + std::to_string(bytes) + " bytes) are larger than the free device memory");
    hipError_t e = hipMalloc(mem, bytes);
    if (e != hipSuccess) { (void) hipGetLastError(); *mem = nullptr; return fail(MI_ERR_DEVICE, fn + ": cannot allocate the colour and guide buffers: " + hipGetErrorString(e)); }
    char *base = (char *) *mem;
    b->col[0] = (float4 *) base; b->col[1] = (float4 *) (base + n * 16); b->gA = (float4 *) (base + n * 32); b->dem = (float4 *) (base + n * 48);
    b->gB = (float2 *) (base + n * 64); b->partial = (float *) (base + n * 72); b->res = b->partial + MI_DN_BOUNDS_BLOCKS * 6u;
    return MI_OK;
}
// bounds (automatic width) and the levels over prepared records; iterations >= 1.  Synchronises `st`.
static int dnFilter(const DenoiseBufs &b, uint32_t width, uint32_t height, const mi_denoise_params *p, int demod, float *devOut, float *resolved, hipStream_t st) {
    const bool automatic = p->sigma_position < 0;
    if (automatic) mi_launch_dn_bounds(b, (size_t) width * height, std::fabs(p->sigma_position), st);
    DenoiseLevel L{}; L.w = (int) width; L.h = (int) height; L.demod = demod; L.res = automatic ? b.res : nullptr;
    L.kn = 1.0f / (p->sigma_normal * p->sigma_normal); L.kp = automatic ? 0.0f : 1.0f / (p->sigma_position * p->sigma_position);
    for (uint32_t i = 0; i < p->iterations; ++i) {
        const float sc = std::ldexp(p->sigma_color, -(int) i);
        L.step = 1 << i; L.kc = 1.0f / (sc * sc);
        mi_launch_dn_level(b, (int) (i & 1u), L, i + 1 == p->iterations, devOut, st);
    }
    HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipGetLastError());
    float sigma = p->sigma_position;
    if (automatic) HIPCHK(hipMemcpy(&sigma, b.res, 4, hipMemcpyDeviceToHost));
    if (resolved) *resolved = sigma;
    return MI_OK;
}
// where the render form finds radiance and guides: the film planes and the first shNormal / position / albedo entry of the field list; a missing one is refused by name
static int dnRenderSource(const std::string &fn, const mi_render *r, const mi_denoise_params *p, DenoiseFilmSrc *f) {
    const mi::SceneHost &h = r->scene->h;
    int fN = -1, fP = -1, fA = -1, fQ = -1;      // the first entry of each kind
    for (int i = (int) r->nFields - 1; i >= 0; --i) { if (r->fields[i].field == MI_FIELD_PREV_POSITION) fQ = i; if (r->fields[i].field == MI_FIELD_SH_NORMAL) fN = i; if (r->fields[i].field == MI_FIELD_POSITION) fP = i; if (r->fields[i].field == MI_FIELD_ALBEDO) fA = i; }
    const char *why = r->adaptFilm ? "; a film that holds an adaptive run has no field film" : "";
    if (fN < 0) return fail(MI_ERR_INVALID, fn + ": the render has no shNormal field (mi_render_set_fields" + why + ")");
    if (fP < 0) return fail(MI_ERR_INVALID, fn + ": the render has no position field (mi_render_set_fields" + why + ")");
    if (p->demodulate && fA < 0) return fail(MI_ERR_INVALID, fn + ": demodulate without albedo: the render has no albedo field (mi_render_set_fields)");
    f->film = r->film; f->spill = r->spill; f->ffilm = r->fieldFilm; f->fspill = r->fieldSpill; f->W = (int) h.width + 2 * h.border; f->H = (int) h.height + 2 * h.border; f->border = h.border;
    f->nv = 3 * (int) r->nFields; f->fN = fN; f->fP = fP; f->fA = fA; f->fQ = fQ;
    return MI_OK;
}
extern "C" {
int mi_denoise_image(uint32_t device, uint32_t width, uint32_t height, const float *color, const float *normal, const float *position, const float *albedo,
                     const mi_denoise_params *p, float *out, float *resolved_sigma_position) {
    const std::string fn = "mi_denoise_image";
    if (!color || !normal || !position || !p || !out) return fail(MI_ERR_INVALID, fn + ": null argument (color, normal, position, params, out)");
    { int rc = dnCheckSize(fn, width, height); if (rc) return rc; }
    { int rc = dnCheckParams(fn, p); if (rc) return rc; }
    if (p->demodulate && !albedo) return fail(MI_ERR_INVALID, fn + ": demodulate without albedo");
    const size_t n = (size_t) width * height;
    if (p->iterations == 0) { memcpy(out, color, n * 12); if (resolved_sigma_position) *resolved_sigma_position = p->sigma_position > 0 ? p->sigma_position : 0.0f; return MI_OK; }
    HIPCHK(hipSetDevice((int) device));
    struct Mem { void *scratch = nullptr, *io = nullptr; ~Mem() { if (scratch) (void) hipFree(scratch); if (io) (void) hipFree(io); } } mem;
    DenoiseBufs b{};
    { int rc = dnAlloc(fn, n, &mem.scratch, &b); if (rc) return rc; }
    const int demod = p->demodulate ? 1 : 0, nIn = demod ? 4 : 3;
    HIPCHK(hipMalloc(&mem.io, n * 12 * (size_t) (nIn + 1)));
    float *d = (float *) mem.io, *dC = d, *dN = d + n * 3, *dP = d + n * 6, *dA = demod ? d + n * 9 : nullptr, *dOut = d + n * 3 * (size_t) nIn;
    HIPCHK(hipMemcpy(dC, color, n * 12, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dN, normal, n * 12, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dP, position, n * 12, hipMemcpyHostToDevice));
    if (demod) HIPCHK(hipMemcpy(dA, albedo, n * 12, hipMemcpyHostToDevice));
    mi_launch_dn_prepare_image(b, dC, dN, dP, dA, (int) width, (int) height, demod, nullptr);
    { int rc = dnFilter(b, width, height, p, demod, dOut, resolved_sigma_position, nullptr); if (rc) return rc; }
    HIPCHK(hipMemcpy(out, dOut, n * 12, hipMemcpyDeviceToHost));
    return MI_OK;
}
int mi_render_denoise_device(mi_render *r, const mi_denoise_params *p, void *device_out, float *resolved_sigma_position) {
    const std::string fn = "mi_render_denoise";
    if (!r || !p || !device_out) return fail(MI_ERR_INVALID, fn + ": null argument");
    { int rc = dnCheckParams(fn, p); if (rc) return rc; }
    const mi::SceneHost &h = r->scene->h;
    { int rc = dnCheckSize(fn, h.width, h.height); if (rc) return rc; }
    DenoiseFilmSrc f{}; { int rc = dnRenderSource(fn, r, p, &f); if (rc) return rc; }
    HIPCHK(hipSetDevice(h.device));
    const int W = (int) h.width + 2 * h.border, H = (int) h.height + 2 * h.border;
    if (p->iterations == 0) {      // the radiance as layout 2 develops it
        mi_launch_film_layout(r->film, r->spill, (float *) device_out, W, H, h.border, 2, r->stream);
        HIPCHK(hipStreamSynchronize(r->stream)); HIPCHK(hipGetLastError());
        if (resolved_sigma_position) *resolved_sigma_position = p->sigma_position > 0 ? p->sigma_position : 0.0f;
        return MI_OK;
    }
    const size_t n = (size_t) h.width * h.height;
    if (!r->dnMem) { int rc = dnAlloc(fn, n, &r->dnMem, &r->dn); if (rc) return rc; }
    const int demod = p->demodulate ? 1 : 0;
    mi_launch_dn_prepare_render(r->dn, f, nullptr, (int) h.width, (int) h.height, demod, r->stream);
    return dnFilter(r->dn, h.width, h.height, p, demod, (float *) device_out, resolved_sigma_position, r->stream);
}
int mi_render_denoise(mi_render *r, const mi_denoise_params *p, float *host_out, float *resolved_sigma_position) {
    if (!r || !p || !host_out) return fail(MI_ERR_INVALID, "mi_render_denoise: null argument");
    int rc = mi_render_denoise_device(r, p, r->layoutTmp, resolved_sigma_position); if (rc) return rc;      // layoutTmp holds 5 floats per film pixel, border included
    HIPCHK(hipMemcpy(host_out, r->layoutTmp, (size_t) r->scene->h.width * r->scene->h.height * 12, hipMemcpyDeviceToHost));
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ denoiser, temporal stage (temporal.h, kernels_temporal.hip)
}  // extern "C"
struct mi_history {
    int device = 0; uint32_t width = 0, height = 0;
    void *mem = nullptr; TemporalSet set[2]{}; float *tail = nullptr;      // one allocation: two record sets + MI_TP_TAIL_FLOATS
    int cur = 0;                  // the set the last frame wrote
    uint32_t frames = 0; int demod = 0; float M[12] = {0};
};
static int tpCheckParams(const std::string &fn, const mi_temporal_params *t) {
    if (!(t->max_history >= 1) || !std::isfinite(t->max_history)) return fail(MI_ERR_INVALID, fn + ": max_history must be >= 1 and finite");
    if (t->sigma_position == 0 || !std::isfinite(t->sigma_position)) return fail(MI_ERR_INVALID, fn + ": the temporal sigma_position must be non-zero and finite (negative: a fraction of the position box's diagonal)");
    if (!(t->min_normal_dot >= -1.0f && t->min_normal_dot <= 1.0f)) return fail(MI_ERR_INVALID, fn + ": min_normal_dot must lie in [-1, 1]");
    return MI_OK;
}
static int tpCheckHistory(const std::string &fn, const mi_history *h, int device, uint32_t width, uint32_t height, int demod) {
    if (h->device != device) return fail(MI_ERR_INVALID, fn + ": the history is on device " + std::to_string(h->device) + ", the frame on device " + std::to_string(device));
    if (h->width != width || h->height != height)
        return fail(MI_ERR_INVALID, fn + ": the history has the image size " + std::to_string(h->width) + " x " + std::to_string(h->height) + ", the frame " + std::to_string(width) + " x " + std::to_string(height));
    if (h->frames && h->demod != demod) return fail(MI_ERR_INVALID, fn + ": demodulate differs from the history's last frame (the accumulated colour would mix the two): call mi_history_reset first");
    return MI_OK;
}
// Over prepared records: the temporal tolerance (on the device), the accumulation, then the spatial bounds and the levels (or, with 0 iterations, the output).
// Synchronises `st`; the history advances only when all of it succeeded.
static int tpRun(mi_history *h, const DenoiseBufs &b, const float *M, const float *devPprev, const mi_denoise_params *p, const mi_temporal_params *t, int demod, float *devOut,
                 float *resolved, float *resolvedTemporal, hipStream_t st) {
    const size_t n = (size_t) h->width * h->height;
    const bool automatic = t->sigma_position < 0;
    if (automatic) mi_launch_dn_bounds(b, n, std::fabs(t->sigma_position), st);
    TemporalFrame F{}; F.w = (int) h->width; F.h = (int) h->height; F.hasHistory = h->frames ? 1 : 0; memcpy(F.Mh, h->M, 48);
    F.maxHistory = t->max_history; F.minNormalDot = t->min_normal_dot; F.tp = automatic ? 0.0f : t->sigma_position; F.res = automatic ? b.res : nullptr;
    F.pprev = devPprev; F.tpOut = h->tail;
    mi_launch_tp_accumulate(b, h->set[h->cur], h->set[h->cur ^ 1], F, st);
    if (p->iterations == 0) {
        mi_launch_tp_output(b, devOut, n, demod, st);
        HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipGetLastError());
        if (resolved) *resolved = p->sigma_position > 0 ? p->sigma_position : 0.0f;
    } else { int rc = dnFilter(b, h->width, h->height, p, demod, devOut, resolved, st); if (rc) return rc; }
    if (resolvedTemporal) HIPCHK(hipMemcpy(resolvedTemporal, h->tail, 4, hipMemcpyDeviceToHost));
    h->cur ^= 1; ++h->frames; h->demod = demod; memcpy(h->M, M, 48);
    return MI_OK;
}
// inverse of a row-major 4 x 4 matrix in double (Gauss-Jordan, partial pivoting); false: singular
static bool invert4(const double *m, double *inv) {
    double a[4][8];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { a[r][c] = m[r * 4 + c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {
        int piv = c; for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (!(std::fabs(a[piv][c]) > 0) || !std::isfinite(a[piv][c])) return false;
        if (piv != c) for (int k = 0; k < 8; ++k) std::swap(a[piv][k], a[c][k]);
        const double d = a[c][c]; for (int k = 0; k < 8; ++k) a[c][k] /= d;
        for (int r = 0; r < 4; ++r) if (r != c) { const double f = a[r][c]; if (f != 0) for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k]; }
    }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) inv[r * 4 + c] = a[r][4 + c];
    return true;
}
static int sceneWorldToPixel(const std::string &fn, const mi::SceneHost &h, float *out12) {
    double s2c[16], c2w[16], is2c[16], ic2w[16];
    for (int i = 0; i < 16; ++i) { s2c[i] = h.s2c[i]; c2w[i] = h.c2w[i]; }
    if (!invert4(s2c, is2c) || !invert4(c2w, ic2w)) return fail(MI_ERR_INVALID, fn + ": the camera's sample_to_camera or to_world matrix is singular");
    const int rows[3] = {0, 1, 3}; const double scale[3] = {(double) h.width, (double) h.height, 1.0};
    for (int i = 0; i < 3; ++i) for (int c = 0; c < 4; ++c) {
        double v = 0; for (int k = 0; k < 4; ++k) v += is2c[rows[i] * 4 + k] * ic2w[k * 4 + c];
        out12[i * 4 + c] = (float) (scale[i] * v);
    }
    return MI_OK;
}
extern "C" {
int mi_history_create(uint32_t device, uint32_t width, uint32_t height, mi_history **out) {
    const std::string fn = "mi_history_create";
    if (!out) return fail(MI_ERR_INVALID, fn + ": null argument");
    { int rc = dnCheckSize(fn, width, height); if (rc) return rc; }
    const size_t n = (size_t) width * height;
    const uint64_t bytes = (uint64_t) n * MI_TP_BYTES_PER_PIXEL + MI_TP_TAIL_FLOATS * 4u;
    const char *lim = getenv("MI355PT_POOL_LIMIT");
    if (lim && atoll(lim) > 0 && bytes > (uint64_t) atoll(lim)) return fail(MI_ERR_DEVICE, fn + ": the history buffers (" + std::to_string(bytes) + " bytes) are larger than MI355PT_POOL_LIMIT");
    HIPCHK(hipSetDevice((int) device));
    size_t freeB = 0, totalB = 0; HIPCHK(hipMemGetInfo(&freeB, &totalB));
    if (bytes > freeB) return fail(MI_ERR_DEVICE, fn + ": the history buffers (" + std::to_string(bytes) + " bytes) are larger than the free device memory");
    void *mem = nullptr; hipError_t e = hipMalloc(&mem, bytes);
    if (e != hipSuccess) { (void) hipGetLastError(); return fail(MI_ERR_DEVICE, fn + ": cannot allocate the history buffers: " + hipGetErrorString(e)); }
    mi_history *h = new mi_history(); h->device = (int) device; h->width = width; h->height = height; h->mem = mem;
    char *base = (char *) mem;      // float4 arrays first, then the float2 arrays, then the tail
    h->set[0].c = (float4 *) base; h->set[1].c = (float4 *) (base + n * 16); h->set[0].gA = (float4 *) (base + n * 32); h->set[1].gA = (float4 *) (base + n * 48);
    h->set[0].gB = (float2 *) (base + n * 64); h->set[1].gB = (float2 *) (base + n * 72); h->tail = (float *) (base + n * 80);
    *out = h; return MI_OK;
}
void mi_history_destroy(mi_history *h) {
    if (!h) return;
    if (h->mem) { (void) hipSetDevice(h->device); (void) hipFree(h->mem); }
    delete h;
}
int mi_history_reset(mi_history *h) {
    if (!h) return fail(MI_ERR_INVALID, "mi_history_reset: null argument");
    h->cur = 0; h->frames = 0; h->demod = 0; memset(h->M, 0, 48); return MI_OK;      // frames = 0: no record is read before the next frame has rewritten it
}
int mi_history_frames(mi_history *h, uint32_t *frames) {
    if (!h || !frames) return fail(MI_ERR_INVALID, "mi_history_frames: null argument");
    *frames = h->frames; return MI_OK;
}
int mi_history_read(mi_history *h, float *color, float *count) {
    if (!h) return fail(MI_ERR_INVALID, "mi_history_read: null argument");
    if (!h->frames) return fail(MI_ERR_INVALID, "mi_history_read: the history holds no frame");
    const size_t n = (size_t) h->width * h->height; std::vector<float> rec(n * 4);
    HIPCHK(hipSetDevice(h->device)); HIPCHK(hipMemcpy(rec.data(), h->set[h->cur].c, n * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (color) { color[i * 3] = rec[i * 4]; color[i * 3 + 1] = rec[i * 4 + 1]; color[i * 3 + 2] = rec[i * 4 + 2]; }
        if (count) count[i] = rec[i * 4 + 3];
    }
    return MI_OK;
}
int mi_denoise_image_temporal(mi_history *h, const float *color, const float *normal, const float *position, const float *albedo, const float *prev_position,
                              const float *M, const mi_denoise_params *p, const mi_temporal_params *t, float *out, float *resolved_sigma_position,
                              float *resolved_temporal_position) {
    const std::string fn = "mi_denoise_image_temporal";
    if (!h || !color || !normal || !position || !p || !t || !out) return fail(MI_ERR_INVALID, fn + ": null argument (history, color, normal, position, params, temporal params, out)");
    if (!M) return fail(MI_ERR_INVALID, fn + ": null world_to_pixel (the frame's projection M)");
    { int rc = dnCheckParams(fn, p); if (rc) return rc; }
    { int rc = tpCheckParams(fn, t); if (rc) return rc; }
    if (p->demodulate && !albedo) return fail(MI_ERR_INVALID, fn + ": demodulate without albedo");
    const int demod = p->demodulate ? 1 : 0, nIn = 3 + demod + (prev_position ? 1 : 0);
    { int rc = tpCheckHistory(fn, h, h->device, h->width, h->height, demod); if (rc) return rc; }
    const uint32_t width = h->width, height = h->height; const size_t n = (size_t) width * height;
    HIPCHK(hipSetDevice(h->device));
    struct Mem { void *scratch = nullptr, *io = nullptr; ~Mem() { if (scratch) (void) hipFree(scratch); if (io) (void) hipFree(io); } } mem;
    DenoiseBufs b{};
    { int rc = dnAlloc(fn, n, &mem.scratch, &b); if (rc) return rc; }
    {   // the staging arrays of the host form, held to the same limits as the scratch
        const uint64_t bytes = (uint64_t) n * 12u * (uint64_t) (nIn + 1);
        const char *lim = getenv("MI355PT_POOL_LIMIT");
        if (lim && atoll(lim) > 0 && bytes > (uint64_t) atoll(lim)) return fail(MI_ERR_DEVICE, fn + ": the staging arrays (" + std::to_string(bytes) + " bytes) are larger than MI355PT_POOL_LIMIT");
        size_t freeB = 0, totalB = 0; HIPCHK(hipMemGetInfo(&freeB, &totalB));
        if (bytes > freeB) return fail(MI_ERR_DEVICE, fn + ": the staging arrays (" + std::to_string(bytes) + " bytes) are larger than the free device memory");
        hipError_t e = hipMalloc(&mem.io, bytes);
        if (e != hipSuccess) { (void) hipGetLastError(); mem.io = nullptr; return fail(MI_ERR_DEVICE, fn + ": cannot allocate the staging arrays: " + hipGetErrorString(e)); }
    }
    float *d = (float *) mem.io, *dC = d, *dN = d + n * 3, *dP = d + n * 6, *dA = demod ? d + n * 9 : nullptr, *dQ = prev_position ? d + n * 3 * (size_t) (3 + demod) : nullptr,
          *dOut = d + n * 3 * (size_t) nIn;
    HIPCHK(hipMemcpy(dC, color, n * 12, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dN, normal, n * 12, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dP, position, n * 12, hipMemcpyHostToDevice));
    if (demod) HIPCHK(hipMemcpy(dA, albedo, n * 12, hipMemcpyHostToDevice));
    if (dQ) HIPCHK(hipMemcpy(dQ, prev_position, n * 12, hipMemcpyHostToDevice));
    mi_launch_dn_prepare_image(b, dC, dN, dP, dA, (int) width, (int) height, demod, nullptr);
    { int rc = tpRun(h, b, M, dQ, p, t, demod, dOut, resolved_sigma_position, resolved_temporal_position, nullptr); if (rc) return rc; }
    HIPCHK(hipMemcpy(out, dOut, n * 12, hipMemcpyDeviceToHost));
    return MI_OK;
}
int mi_render_denoise_temporal_device(mi_render *r, mi_history *hist, const mi_denoise_params *p, const mi_temporal_params *t, void *device_out, float *resolved_sigma_position,
                                      float *resolved_temporal_position) {
    const std::string fn = "mi_render_denoise_temporal";
    if (!r || !hist || !p || !t || !device_out) return fail(MI_ERR_INVALID, fn + ": null argument");
    { int rc = dnCheckParams(fn, p); if (rc) return rc; }
    { int rc = tpCheckParams(fn, t); if (rc) return rc; }
    const mi::SceneHost &h = r->scene->h;
    { int rc = dnCheckSize(fn, h.width, h.height); if (rc) return rc; }
    DenoiseFilmSrc f{}; { int rc = dnRenderSource(fn, r, p, &f); if (rc) return rc; }
    const int demod = p->demodulate ? 1 : 0;
    { int rc = tpCheckHistory(fn, hist, h.device, h.width, h.height, demod); if (rc) return rc; }
    float M[12]; { int rc = sceneWorldToPixel(fn, h, M); if (rc) return rc; }
    HIPCHK(hipSetDevice(h.device));
    const size_t n = (size_t) h.width * h.height;
    if (!r->dnMem) { int rc = dnAlloc(fn, n, &r->dnMem, &r->dn); if (rc) return rc; }
    float *pprev = nullptr;      // with a prevPosition field: that field, developed, is Pprev; without one Pprev = P
    if (f.fQ >= 0) {
        if (!r->dnPprev && hipMalloc((void **) &r->dnPprev, n * 12) != hipSuccess) { (void) hipGetLastError(); r->dnPprev = nullptr; return fail(MI_ERR_DEVICE, fn + ": cannot allocate the previous-position buffer (" + std::to_string(n * 12) + " bytes)"); }
        pprev = r->dnPprev;
    }
    mi_launch_dn_prepare_render(r->dn, f, pprev, (int) h.width, (int) h.height, demod, r->stream);
    return tpRun(hist, r->dn, M, pprev, p, t, demod, (float *) device_out, resolved_sigma_position, resolved_temporal_position, r->stream);
}
int mi_render_denoise_temporal(mi_render *r, mi_history *hist, const mi_denoise_params *p, const mi_temporal_params *t, float *host_out, float *resolved_sigma_position,
                               float *resolved_temporal_position) {
    if (!r || !hist || !p || !t || !host_out) return fail(MI_ERR_INVALID, "mi_render_denoise_temporal: null argument");
    int rc = mi_render_denoise_temporal_device(r, hist, p, t, r->layoutTmp, resolved_sigma_position, resolved_temporal_position); if (rc) return rc;
    HIPCHK(hipMemcpy(host_out, r->layoutTmp, (size_t) r->scene->h.width * r->scene->h.height * 12, hipMemcpyDeviceToHost));
    return MI_OK;
}
int mi_scene_world_to_pixel(mi_scene *s, float *out12) {
    if (!s || !out12) return fail(MI_ERR_INVALID, "mi_scene_world_to_pixel: null argument");
    if (!s->h.committed) return fail(MI_ERR_INVALID, "mi_scene_world_to_pixel: scene not committed");
    return sceneWorldToPixel("mi_scene_world_to_pixel", s->h, out12);
}
// Frame mark: the "previous" state of the prevPosition / motion fields.  The host takes the snapshot (a replica uploads it from there); the device's copy of the
// vertices comes from the device's own vertex array where a vertex edit has made one -- it holds h.pos, pushed by every such edit -- and from the host otherwise.
// Both tables are allocated before anything changes: a failed allocation leaves the earlier mark as it was.
int mi_scene_mark_frame(mi_scene *s) {
    UPDATE_ENTER("mi_scene_mark_frame");
    mi::SceneHost &h = s->h;
    float M[12]; { int rc = sceneWorldToPixel("mi_scene_mark_frame", h, M); if (rc) return rc; }
    HIPCHK(hipSetDevice(h.device));
    if (h.allocMark()) { (void) hipGetLastError(); return fail(MI_ERR_DEVICE, "mi_scene_mark_frame: cannot allocate the tables of the previous frame; the earlier mark stays"); }
    h.prevPos = h.pos; h.prevInstXf.resize(h.instances.size() * 12);
    for (size_t i = 0; i < h.instances.size(); ++i) memcpy(&h.prevInstXf[i * 12], h.instances[i].to_world, 48);
    memcpy(h.prevW2P, M, 48); for (int i = 0; i < 3; ++i) h.prevOrigin[i] = h.c2w[i * 4 + 3];
    h.marked = true;
    if (h.dPos && !h.prevPos.empty()) HIPCHK(hipMemcpy(h.dPrevPos, h.dPos, h.prevPos.size() * 4, hipMemcpyDeviceToDevice));
    else HIPCHK(push(h.dPrevPos, h.prevPos));
    HIPCHK(push(h.dPrevInst, h.prevInstXf));
    HIPCHK(hipStreamSynchronize(nullptr));
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ unit-level device entry points
}  // extern "C"
template <typename F> static int withBuffers(const void *in, size_t inBytes, void *out, size_t outBytes, F f) {
    void *dIn = nullptr, *dOut = nullptr;
    HIPCHK(hipMalloc(&dIn, inBytes)); HIPCHK(hipMalloc(&dOut, outBytes));
    HIPCHK(hipMemcpy(dIn, in, inBytes, hipMemcpyHostToDevice));
    f(dIn, dOut);
    hipError_t e = hipDeviceSynchronize(); if (e == hipSuccess) e = hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);
    (void) hipFree(dIn); (void) hipFree(dOut);
    if (e != hipSuccess) return fail(MI_ERR_DEVICE, hipGetErrorString(e));
    return MI_OK;
}
extern "C" {
int mi_debug_intersect_inst(mi_scene *s, const float *rays, uint64_t n, int anyHit, float *out, int32_t *outInst) {
    if (!s || !s->h.committed || !rays || !out || !n) return fail(MI_ERR_INVALID, "mi_debug_intersect: bad argument");
    HIPCHK(hipSetDevice(s->h.device));
    void *dInst = nullptr; if (outInst) HIPCHK(hipMalloc(&dInst, n * 4));
    int rc = withBuffers(rays, n * 32, out, n * 16, [&](void *i, void *o) { mi_launch_debug_intersect(s->h.d, (const float *) i, n, anyHit, (float *) o, (int *) dInst, nullptr); });
    if (!rc && outInst) { hipError_t e = hipMemcpy(outInst, dInst, n * 4, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = fail(MI_ERR_DEVICE, hipGetErrorString(e)); }
    if (dInst) (void) hipFree(dInst);
    return rc;
}
int mi_scene_ray_intersect(mi_scene *s, const float *rays, uint64_t n, mi_intersection *out) {
    if (!s || !s->h.committed || !rays || !out || !n) return fail(MI_ERR_INVALID, "mi_scene_ray_intersect: bad argument (the scene must be committed)");
    HIPCHK(hipSetDevice(s->h.device));
    return withBuffers(rays, n * 32, out, n * sizeof(mi_intersection), [&](void *i, void *o) { mi_launch_ray_intersect(s->h.d, (const float *) i, n, (mi_intersection *) o, nullptr); });
}
int mi_debug_intersect(mi_scene *s, const float *rays, uint64_t n, int anyHit, float *out) { return mi_debug_intersect_inst(s, rays, n, anyHit, out, nullptr); }

// The fused walk of trace_fused.h on caller-supplied rays: a minimal Queues (rays laid into segments as `seg_counts` says, a zeroed ticket, a spill area sized for
// the worst case 3 * bvh_depth + 4 entries per lane rather than for the builder's bound -- a wrong bound then fails the caller's comparison instead of writing
// astray) and ONE launch of the stage production runs.  The refusals read host data only, so they are decided (and testable) before any device call.
int mi_debug_intersect_fused(mi_scene *s, const float *rays, uint64_t n, int anyHit, const uint32_t *segCounts, uint32_t nSeg, uint32_t thr, uint32_t grid, uint32_t ldsStack,
                             float *out, mi_fused_debug_info *info) {
    if (!s || !rays || !out || !info || !segCounts || !n || !nSeg) return fail(MI_ERR_INVALID, "mi_debug_intersect_fused: null argument");
    const mi::SceneHost &h = s->h;
    if (!h.analytic.empty()) return fail(MI_ERR_UNSUPPORTED, "mi_debug_intersect_fused: the fused walk serves triangle-only trees, this scene has analytic shapes");
    if (!h.instances.empty()) return fail(MI_ERR_UNSUPPORTED, "mi_debug_intersect_fused: the fused walk serves triangle-only trees, this scene has instances");
    {   // committed: what upload() decided; before that: the same rule on the host data
        const char *noPacket = getenv("MI355PT_NO_PACKET");
        const bool packet = h.committed ? h.d.packet_n != 0 : (h.idx.size() / 3 <= MI_PACKET_MAX && h.media.empty() && !(noPacket && noPacket[0] == '1'));
        if (packet) return fail(MI_ERR_UNSUPPORTED, "mi_debug_intersect_fused: this scene is traced as one triangle packet (at most 64 triangles), it has no tree to walk; set MI355PT_NO_PACKET=1");
    }
    if (!h.committed) return fail(MI_ERR_INVALID, "mi_debug_intersect_fused: the scene must be committed");
    const DScene &sc = h.d;
    if (sc.geo_bytes >= 0xFFFFFF00ull) return fail(MI_ERR_UNSUPPORTED, "mi_debug_intersect_fused: nodes and leaf records exceed the 4 GB the fused walk addresses");
    if (thr < 1 || thr > 64 || grid < 1 || grid > 16384 || (ldsStack != 4u && ldsStack != mi_fused_lds_stack())) return fail(MI_ERR_INVALID, "mi_debug_intersect_fused: thr in 1..64, grid in 1..16384, lds_stack 4 or 10");
    uint64_t total = 0; uint32_t cap = 64;
    for (uint32_t i = 0; i < nSeg; ++i) { total += segCounts[i]; cap = std::max(cap, (segCounts[i] + 63u) / 64u * 64u); }
    if (total != n) return fail(MI_ERR_INVALID, "mi_debug_intersect_fused: seg_counts must add up to n");
    const uint64_t slots = (uint64_t) cap * nSeg;
    if (slots >= (1ull << 28) || n >= (1ull << 28)) return fail(MI_ERR_INVALID, "mi_debug_intersect_fused: fewer than 2^28 slots");
    if (anyHit) for (uint64_t i = 0; i < n; ++i) if (rays[i * 8 + 3] != MI_EPSILON) return fail(MI_ERR_INVALID, "mi_debug_intersect_fused: a shadow record has no mint of its own, any-hit rays start at MI_EPSILON (1e-4)");
    HIPCHK(hipSetDevice(h.device));
    // slot of ray i: segment by segment, in input order
    std::vector<uint64_t> slotOf(n); { uint64_t i = 0; for (uint32_t sg = 0; sg < nSeg; ++sg) for (uint32_t j = 0; j < segCounts[sg]; ++j) slotOf[i++] = (uint64_t) sg * cap + j; }
    const uint32_t sentinel = 0xFFFFFFFEu;      // no retired ray leaves this in Queues::hit: prim is a triangle index or 0xFFFFFFFF
    // the layout of queues.h: shadow records are (o | maxt), (d | path id), contribution rgb; extension rays are origin, direction and the interval in the side array
    std::vector<float4> hO(anyHit ? slots : 0, make_float4(0, 0, 0, 0)), hD(anyHit ? slots : 0, make_float4(0, 0, 0, 0));
    std::vector<QVec3> hC(anyHit ? slots : 0, QVec3{1.0f, 0.0f, 0.0f}), hO3(anyHit ? 0 : slots, QVec3{0, 0, 0}), hD3(anyHit ? 0 : slots, QVec3{0, 0, 0});
    std::vector<float2> hT(anyHit ? 0 : slots, make_float2(0, 0));
    for (uint64_t i = 0; i < n; ++i) {
        const float *r = rays + i * 8; const uint32_t pid = (uint32_t) i; float pidf; memcpy(&pidf, &pid, 4);
        if (anyHit) { hO[slotOf[i]] = make_float4(r[0], r[1], r[2], r[7]); hD[slotOf[i]] = make_float4(r[4], r[5], r[6], pidf); }
        else { hO3[slotOf[i]] = QVec3{r[0], r[1], r[2]}; hD3[slotOf[i]] = QVec3{r[4], r[5], r[6]}; hT[slotOf[i]] = make_float2(r[3], r[7]); }
    }
    std::vector<void *> bufs; int rc = MI_OK;
    auto alloc = [&](size_t bytes) -> void * { void *p = nullptr; if (rc) return p; hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16)); if (e != hipSuccess) { rc = fail(MI_ERR_DEVICE, std::string("mi_debug_intersect_fused: ") + hipGetErrorString(e)); return nullptr; } bufs.push_back(p); return p; };
    auto chk = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = fail(MI_ERR_DEVICE, std::string("mi_debug_intersect_fused: ") + hipGetErrorString(e)); };
    Queues q{}; q.cap = cap; q.n_seg = nSeg;
    const size_t rayBytes = anyHit ? sizeof(float4) : sizeof(QVec3);
    void *dO = alloc(slots * rayBytes), *dD = alloc(slots * rayBytes);
    uint32_t *dCount = (uint32_t *) alloc((size_t) nSeg * 4), *dTicket = (uint32_t *) alloc(4); int *dMaxSp = (int *) alloc(4);
    q.counters = (unsigned long long *) alloc(32);
    const size_t spillEntries = (size_t) 3 * sc.bvh_depth + 4;
    q.stkSpill = (int32_t *) alloc(spillEntries * grid * 256u * 4);      // one column per lane of the grid (workgroups of 256)
    if (anyHit) { q.shO = (float4 *) dO; q.shD = (float4 *) dD; q.shC = (QVec3 *) alloc(slots * sizeof(QVec3)); q.acc = (float4 *) alloc(n * 16); q.shCount = dCount; }
    else { q.rayO[0] = (QVec3 *) dO; q.rayD[0] = (QVec3 *) dD; q.rayT[0] = (float2 *) alloc(slots * sizeof(float2)); q.count[0] = dCount; q.hit = (float4 *) alloc(slots * 16); }
    if (!rc) {
        chk(hipMemcpy(dO, anyHit ? (const void *) hO.data() : (const void *) hO3.data(), slots * rayBytes, hipMemcpyHostToDevice));
        chk(hipMemcpy(dD, anyHit ? (const void *) hD.data() : (const void *) hD3.data(), slots * rayBytes, hipMemcpyHostToDevice));
        chk(hipMemcpy(dCount, segCounts, (size_t) nSeg * 4, hipMemcpyHostToDevice)); chk(hipMemset(dTicket, 0, 4)); chk(hipMemset(dMaxSp, 0, 4)); chk(hipMemset(q.counters, 0, 32));
        if (anyHit) { chk(hipMemcpy(q.shC, hC.data(), slots * sizeof(QVec3), hipMemcpyHostToDevice)); chk(hipMemset(q.acc, 0, n * 16)); }
        else {
            chk(hipMemcpy(q.rayT[0], hT.data(), slots * sizeof(float2), hipMemcpyHostToDevice));
            std::vector<uint32_t> fill(slots * 4, sentinel); chk(hipMemcpy(q.hit, fill.data(), slots * 16, hipMemcpyHostToDevice));
        }
    }
    std::vector<float4> res(anyHit ? n : slots);
    if (!rc) {
        mi_launch_debug_fused(sc, q, anyHit, ldsStack, dTicket, thr, grid, dMaxSp, nullptr);
        chk(hipGetLastError()); chk(hipDeviceSynchronize());
        int maxSp = 0; unsigned long long cnt[4] = {};
        chk(hipMemcpy(res.data(), anyHit ? q.acc : q.hit, res.size() * 16, hipMemcpyDeviceToHost)); chk(hipMemcpy(&maxSp, dMaxSp, 4, hipMemcpyDeviceToHost)); chk(hipMemcpy(cnt, q.counters, 32, hipMemcpyDeviceToHost));
        if (!rc) {
            for (uint64_t i = 0; i < n; ++i) memcpy(out + i * 4, &res[anyHit ? i : slotOf[i]], 16);
            info->wide = sc.bvh_wide; info->bvh_depth = sc.bvh_depth; info->bvh_stack_direct = sc.bvh_stack_direct; info->max_stack_seen = (uint32_t) maxSp; info->rays_counted = cnt[0];
        }
    }
    for (void *p : bufs) (void) hipFree(p);
    return rc;
}
// One device table of the scene as it is now: 0 nodes, 1 leaf records, 2 TriShade, 3 TriUV, 4 packet-exact records, 5 packet groups, 6 instance records; 7 = the box
// of the scene record (held on the host: every run passes the record by value); 8, 9 = the vertices and instance transforms of the last frame mark.  mi_debug_geometry_bytes gives the size.
static int geometryTable(mi_scene *s, uint32_t what, const void **ptr, uint64_t *bytes, const char *who) {
    if (!s) return fail(MI_ERR_INVALID, std::string(who) + ": null scene");
    if (!s->h.committed) return fail(MI_ERR_INVALID, std::string(who) + ": scene not committed");
    const mi::SceneHost &h = s->h;
    switch (what) {
    case 0: *ptr = h.dNodes; *bytes = (uint64_t) h.nodes.size() * sizeof(BvhNode); break;
    case 1: *ptr = h.d.tris; *bytes = (uint64_t) h.tris.size() * sizeof(TriAccelD); break;
    case 2: *ptr = h.dShade; *bytes = (uint64_t) h.shade.size() * sizeof(TriShade); break;
    case 3: *ptr = h.dTriUV; *bytes = (uint64_t) h.triuv.size() * sizeof(TriUV); break;
    case 4: *ptr = h.dPacketExact; *bytes = (uint64_t) h.packetExact.size() * sizeof(TriAccelD); break;
    case 5: *ptr = h.dPacketGroups; *bytes = (uint64_t) h.packetGroups.size() * sizeof(PacketGroupD); break;
    case MI_GEOMETRY_INSTANCES: *ptr = h.dInstances; *bytes = (uint64_t) h.instancesD.size() * sizeof(InstanceD); break;
    case MI_GEOMETRY_SCENE_BOX: *ptr = nullptr; *bytes = 24; break;
    case MI_GEOMETRY_PREV_VERTICES: *ptr = h.dPrevPos; *bytes = h.marked ? (uint64_t) h.prevPos.size() * 4 : 0; break;          // the two tables of mi_scene_mark_frame
    case MI_GEOMETRY_PREV_INSTANCES: *ptr = h.dPrevInst; *bytes = h.marked ? (uint64_t) h.prevInstXf.size() * 4 : 0; break;
    default: return fail(MI_ERR_INVALID, std::string(who) + ": unknown table " + std::to_string(what));
    }
    return MI_OK;
}
int mi_debug_geometry_bytes(mi_scene *s, uint32_t what, uint64_t *bytes) {
    const void *p = nullptr; uint64_t n = 0; if (!bytes) return fail(MI_ERR_INVALID, "mi_debug_geometry_bytes: null argument");
    const int rc = geometryTable(s, what, &p, &n, "mi_debug_geometry_bytes"); if (rc) return rc;
    *bytes = n; return MI_OK;
}
int mi_debug_read_geometry(mi_scene *s, uint32_t what, void *out, uint64_t bytes) {
    const void *p = nullptr; uint64_t n = 0; const int rc = geometryTable(s, what, &p, &n, "mi_debug_read_geometry"); if (rc) return rc;
    if (bytes != n) return fail(MI_ERR_INVALID, "mi_debug_read_geometry: table " + std::to_string(what) + " holds " + std::to_string(n) + " bytes, the caller gave " + std::to_string(bytes));
    if (!n) return MI_OK;
    if (!out) return fail(MI_ERR_INVALID, "mi_debug_read_geometry: null argument");
    if (what == MI_GEOMETRY_SCENE_BOX) { memcpy(out, s->h.d.aabb_lo, 12); memcpy((char *) out + 12, s->h.d.aabb_hi, 12); return MI_OK; }
    HIPCHK(hipSetDevice(s->h.device)); HIPCHK(hipMemcpy(out, p, n, hipMemcpyDeviceToHost));
    return MI_OK;
}
int mi_debug_sobol(mi_scene *s, const uint32_t *in, uint64_t n, uint32_t ndims, uint64_t *outIdx, float *outVals) {
    if (!s || !s->h.committed || !in || !outIdx || !outVals || !n || !s->h.d.sobol_m32 || ndims > s->h.d.sobol_dims) return fail(MI_ERR_INVALID, "mi_debug_sobol: bad argument");
    HIPCHK(hipSetDevice(s->h.device));
    void *dIdx = nullptr; HIPCHK(hipMalloc(&dIdx, n * 8));
    int rc = withBuffers(in, n * 12, outVals, n * ndims * 4, [&](void *i, void *o) { mi_launch_debug_sobol(s->h.d, (const uint32_t *) i, n, ndims, (unsigned long long *) dIdx, (float *) o, nullptr); });
    if (!rc) { hipError_t e = hipMemcpy(outIdx, dIdx, n * 8, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = fail(MI_ERR_DEVICE, hipGetErrorString(e)); }
    (void) hipFree(dIdx); return rc;
}
int mi_debug_sincosf(const float *x, uint64_t n, float *out) {
    if (!x || !out || !n) return fail(MI_ERR_INVALID, "mi_debug_sincosf: bad argument");
    return withBuffers(x, n * 4, out, n * 8, [&](void *i, void *o) { mi_launch_debug_sincosf((const float *) i, n, (float *) o, nullptr); });
}
int mi_debug_libm(int fn, const float *x, const float *y, uint64_t n, float *out) {
    if (!x || !out || !n || fn < 0 || fn > 6 || ((fn == 2 || fn == 5) && !y)) return fail(MI_ERR_INVALID, "mi_debug_libm: bad argument");
    std::vector<float> xy(2 * n); memcpy(xy.data(), x, n * 4); if (y) memcpy(xy.data() + n, y, n * 4);
    return withBuffers(xy.data(), n * 8, out, n * 4, [&](void *i, void *o) { mi_launch_debug_libm(fn, (const float *) i, y ? (const float *) i + n : nullptr, n, (float *) o, nullptr); });
}
// Unit entry points over the BSDF and texture routines (kernels_units.hip).  A record whose evaluation needs a hit record is refused by name: the mask's logic is
// inline in the shade stage, bumpmap / normalmap perturb a hit's frame, a bound texture is looked up at a hit's uv.
static const char *unitNeedsHit(const mi::SceneHost &h, uint32_t material, int depth = 0) {
    if (material >= h.materials.size() || depth > 4) return "a record out of range";
    const mi_material &m = h.materials[material];
    if (m.type == MI_BSDF_MASK) return "mask";
    if (m.type == MI_BSDF_BUMPMAP) return "bumpmap";
    if (m.type == MI_BSDF_NORMALMAP) return "normalmap";
    if ((m.flags >> 8) & 0xFFFFu) return "a record with a bound texture";
    if (m.type == MI_BSDF_COATING || m.type == MI_BSDF_ROUGHCOATING) return unitNeedsHit(h, m.distr, depth + 1);
    if (m.type == MI_BSDF_MIXTURE) {
        for (uint32_t i = 0; i < m.distr && i < 4; ++i) if (const char *r = unitNeedsHit(h, (uint32_t) (i < 3 ? m.reflectance[i] : m.eta[0]), depth + 1)) return r;
    }
    if (m.type == MI_BSDF_BLEND) {
        for (uint32_t i = 0; i < 2; ++i) if (const char *r = unitNeedsHit(h, (uint32_t) m.eta[i], depth + 1)) return r;
    }
    return nullptr;
}
int mi_debug_bsdf(mi_scene *s, uint32_t material, int mode, const float *wi, const float *wo, const float *uv, const float *extra, uint64_t n, float *out) {
    if (!s || !s->h.committed || !wi || !out || !n || mode < 0 || mode > 1 || (mode == 0 && (!uv || !extra)) || (mode == 1 && !wo)) return fail(MI_ERR_INVALID, "mi_debug_bsdf: bad argument");
    if (material >= s->h.materials.size()) return fail(MI_ERR_INVALID, "mi_debug_bsdf: material " + std::to_string(material) + " of " + std::to_string(s->h.materials.size()));
    if (const char *why = unitNeedsHit(s->h, material)) return fail(MI_ERR_UNSUPPORTED, "mi_debug_bsdf: material " + std::to_string(material) + " is or holds " + why + ", which needs a hit record");
    HIPCHK(hipSetDevice(s->h.device));
    std::vector<float> in(n * 9, 0.0f);
    for (uint64_t i = 0; i < n; ++i) {
        float *p = &in[i * 9]; memcpy(p, wi + 3 * i, 12);
        if (wo) memcpy(p + 3, wo + 3 * i, 12);
        if (uv) memcpy(p + 6, uv + 2 * i, 8);
        if (extra) p[8] = extra[i];
    }
    const int per = mode == 0 ? 11 : 4; std::vector<float> raw(n * 12);
    int rc = withBuffers(in.data(), n * 36, raw.data(), n * 48, [&](void *i, void *o) { mi_launch_debug_bsdf(s->h.d, (int) material, mode, (const float *) i, n, (float *) o, nullptr); });
    if (rc) return rc;
    for (uint64_t i = 0; i < n; ++i) memcpy(out + i * per, &raw[i * 12], per * 4);
    return MI_OK;
}
// The surface step between a hit and the BSDF query (kernels_units.hip).  The hits are caller-supplied, so every primitive and instance index is checked against the
// committed tables here, before any device work.
int mi_debug_surface(mi_scene *s, int mode, const float *rays, const float *hits, const int32_t *inst, const float *diff, const float *query, uint64_t n, float *out) {
    if (!s || !rays || !hits || !out || !n || mode < 0 || mode > 2 || (mode != 0 && !query)) return fail(MI_ERR_INVALID, "mi_debug_surface: bad argument");
    if (!s->h.committed) return fail(MI_ERR_INVALID, "mi_debug_surface: the scene must be committed");
    const DScene &d = s->h.d;
    for (uint64_t i = 0; i < n; ++i) {
        const float p = hits[4 * i + 3]; const int32_t in = inst ? inst[i] : -1;
        if (!(p >= 0)) continue;                                            // a miss
        if (in < -1 || (in >= 0 && ((uint32_t) in >= d.n_instances || !d.instances)) || !(p < (float) (in >= 0 ? d.n_tris : d.n_tris + d.n_analytic)))
            return fail(MI_ERR_INVALID, "mi_debug_surface: hit " + std::to_string(i) + " names a primitive or an instance the scene does not have");
    }
    HIPCHK(hipSetDevice(s->h.device));
    const uint64_t words = n * (8 + 4 + 1 + (diff ? 6 : 0) + (query ? 3 : 0)); std::vector<float> in(words);
    float *pr = in.data(), *ph = pr + 8 * n, *pi = ph + 4 * n, *pd = pi + n, *pq = pd + (diff ? 6 * n : 0);
    memcpy(pr, rays, n * 32); memcpy(ph, hits, n * 16);
    for (uint64_t i = 0; i < n; ++i) { const int32_t v = inst ? inst[i] : -1; memcpy(pi + i, &v, 4); }
    if (diff) memcpy(pd, diff, n * 24);
    if (query) memcpy(pq, query, n * 12);
    const int per = mode == 0 ? 51 : mode == 1 ? 11 : 4;
    return withBuffers(in.data(), words * 4, out, n * per * 4, [&](void *i, void *o) {
        const float *b = (const float *) i;
        mi_launch_debug_surface(s->h.d, mode, b, b + 8 * n, (const int *) (b + 12 * n), diff ? b + 13 * n : nullptr, query ? b + 13 * n + (diff ? 6 * n : 0) : nullptr, n, (float *) o, nullptr);
    });
}
int mi_debug_texture(mi_scene *s, uint32_t texture, const float *uv, const float *partials, uint64_t n, float *out) {
    if (!s || !s->h.committed || !uv || !out || !n) return fail(MI_ERR_INVALID, "mi_debug_texture: bad argument");
    if (texture >= s->h.textures.size() || !s->h.d.textures) return fail(MI_ERR_INVALID, "mi_debug_texture: texture " + std::to_string(texture) + " of " + std::to_string(s->h.textures.size()));
    HIPCHK(hipSetDevice(s->h.device));
    std::vector<float> in(n * 6, 0.0f); memcpy(in.data(), uv, n * 8); if (partials) memcpy(in.data() + n * 2, partials, n * 16);
    return withBuffers(in.data(), n * 24, out, n * 12, [&](void *i, void *o) { mi_launch_debug_texture(s->h.d, texture, (const float *) i, partials ? (const float *) i + n * 2 : nullptr, n, (float *) o, nullptr); });
}
// Unit entry points over the emitter routines (kernels_units.hip): Scene::sampleEmitterDirect on chosen reference points and sample values, and what a BSDF-sampled
// ray that finds an emitter evaluates.
int mi_debug_emitter_sample(mi_scene *s, const float *ref, const float *refN, const float *uv, uint64_t n, int raw, float *out) {
    if (!s || !s->h.committed || !ref || !refN || !uv || !out || !n || raw < 0 || raw > 1) return fail(MI_ERR_INVALID, "mi_debug_emitter_sample: bad argument");
    if (s->h.emitters.empty()) return fail(MI_ERR_INVALID, "mi_debug_emitter_sample: the scene has no emitter");
    HIPCHK(hipSetDevice(s->h.device));
    std::vector<float> in(n * 8);
    for (uint64_t i = 0; i < n; ++i) { float *p = &in[i * 8]; memcpy(p, ref + 3 * i, 12); memcpy(p + 3, refN + 3 * i, 12); memcpy(p + 6, uv + 2 * i, 8); }
    return withBuffers(in.data(), n * 32, out, n * 68, [&](void *i, void *o) { mi_launch_debug_emitter_sample(s->h.d, raw, (const float *) i, n, (float *) o, nullptr); });
}
int mi_debug_emitter_eval(mi_scene *s, uint32_t emitter, const float *ref, const float *d, const float *nrm, const float *dist, const float *facing, uint64_t n, float *out) {
    if (!s || !s->h.committed || !ref || !d || !nrm || !dist || !facing || !out || !n) return fail(MI_ERR_INVALID, "mi_debug_emitter_eval: bad argument");
    if (emitter >= s->h.emitters.size()) return fail(MI_ERR_INVALID, "mi_debug_emitter_eval: emitter " + std::to_string(emitter) + " of " + std::to_string(s->h.emitters.size()));
    const uint32_t type = s->h.emitters[emitter].type;
    if (type != MI_EMITTER_AREA && type != MI_EMITTER_ENVMAP && type != MI_EMITTER_CONSTANT) {
        const char *name = type == MI_EMITTER_POINT ? "point" : type == MI_EMITTER_SPOT ? "spot" : type == MI_EMITTER_DIRECTIONAL ? "directional" : type == MI_EMITTER_COLLIMATED ? "collimated" : "unknown";
        return fail(MI_ERR_UNSUPPORTED, "mi_debug_emitter_eval: emitter " + std::to_string(emitter) + " is a " + name + " light, which no ray can find");
    }
    HIPCHK(hipSetDevice(s->h.device));
    std::vector<float> in(n * 11);
    for (uint64_t i = 0; i < n; ++i) { float *p = &in[i * 11]; memcpy(p, ref + 3 * i, 12); memcpy(p + 3, d + 3 * i, 12); memcpy(p + 6, nrm + 3 * i, 12); p[9] = dist[i]; p[10] = facing[i]; }
    const int kind = type == MI_EMITTER_AREA ? 0 : type == MI_EMITTER_ENVMAP ? 1 : 2;
    return withBuffers(in.data(), n * 44, out, n * 32, [&](void *i, void *o) { mi_launch_debug_emitter_eval(s->h.d, (int) emitter, kind, (const float *) i, n, (float *) o, nullptr); });
}
int mi_debug_medium(mi_scene *s, uint32_t medium, int mode, const float *in, uint64_t n, float *out) {
    if (!s || !s->h.committed || !in || !out || !n || mode < 0 || mode > 3) return fail(MI_ERR_INVALID, "mi_debug_medium: bad argument");
    if (medium >= s->h.media.size() || !s->h.d.media) return fail(MI_ERR_INVALID, "mi_debug_medium: medium " + std::to_string(medium) + " of " + std::to_string(s->h.media.size()));
    HIPCHK(hipSetDevice(s->h.device));
    return withBuffers(in, n * 40, out, n * 48, [&](void *i, void *o) { mi_launch_debug_medium(s->h.d, medium, mode, (const float *) i, n, (float *) o, nullptr); });
}
int mi_debug_camera_rays(mi_scene *s, const float *pos, uint64_t n, float *out) {
    if (!s || !s->h.committed || !pos || !out || !n) return fail(MI_ERR_INVALID, "mi_debug_camera_rays: bad argument");
    HIPCHK(hipSetDevice(s->h.device));
    return withBuffers(pos, n * 8, out, n * 32, [&](void *i, void *o) { mi_launch_debug_camera(s->h.d, (const float *) i, n, (float *) o, nullptr); });
}

int mi_debug_camera_rays_lens(mi_scene *s, const float *pos, const float *aperture, uint64_t n, float *out) {
    if (!s || !s->h.committed || !pos || !out || !n || (s->h.lensRadius != 0.0f && !aperture)) return fail(MI_ERR_INVALID, "mi_debug_camera_rays_lens: bad argument");
    HIPCHK(hipSetDevice(s->h.device));
    const bool lens = s->h.lensRadius != 0.0f;
    std::vector<float> in(n * 4, 0.5f); memcpy(in.data(), pos, n * 8); if (lens) memcpy(in.data() + n * 2, aperture, n * 8);
    return withBuffers(in.data(), n * 16, out, n * 56, [&](void *i, void *o) { mi_launch_debug_camera_lens(s->h.d, (const float *) i, (const float *) i + n * 2, n, (float *) o, nullptr); });
}

}  // extern "C"
