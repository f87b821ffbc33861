/* include/mi355pt_host.h -- C shim over the C++ host mirror mi355::MIPathTracerHIP (mitsuba-im_amd/csrc/integrator_host.h), exported by
 * libmi355pt.so so that non-C++ hosts and the ctypes tests can drive the reference-shaped interface:
 * ResponsiveIntegrator::preprocess / render(..., Controls, threadIdx, threadCount) (reference include/mitsuba/render/integrator2.h:49-100),
 * Integrator::cancel (include/mitsuba/render/integrator.h:89-94), MonteCarloIntegrator's properties (src/librender/integrator.cpp:191-226). */
#ifndef MI355PT_HOST_H
#define MI355PT_HOST_H
#include "mi355pt.h"
#ifdef __cplusplus
extern "C" {
#endif
const char *mi_host_last_error(void);
/* returns NULL (message in mi_host_last_error) when rrDepth <= 0 or maxDepth is neither -1 nor > 0 -- the reference's Log(EError) texts */
void *mi_host_create(int maxDepth, int rrDepth, int strictNormals, int hideEmitters, int sampler, uint32_t spp, uint64_t seed, uint32_t device, uint32_t planes_per_batch);
/* the same with the build-specific `devices` property: the film rows are spread over these HIP devices (an entry may repeat); the scene given to
 * mi_host_preprocess must live on devices[0], the other devices receive replicas (mi_scene_clone) and their films are merged (mi_render_merge_film) */
void *mi_host_create_devices(int maxDepth, int rrDepth, int strictNormals, int hideEmitters, int sampler, uint32_t spp, uint64_t seed, const uint32_t *devices, uint32_t n_devices, uint32_t planes_per_batch);
/* everything at once: `integrator` = MI_INTEGRATOR_PATH / _VOLPATH_SIMPLE / _VOLPATH (the plugin's `integrator` property), preview_interval_ms < 0 = the default (100 ms) */
void *mi_host_create_ex(int maxDepth, int rrDepth, int strictNormals, int hideEmitters, int sampler, uint32_t spp, uint64_t seed, const uint32_t *devices, uint32_t n_devices, uint32_t planes_per_batch, int integrator, double preview_interval_ms);
/* integrator = MI_INTEGRATOR_DIRECT: emitterSamples / bsdfSamples of direct.cpp:96-107; NULL with the reference's assertion when both are 0.
   The host mirror keeps each count in 16 bits (mi355::Properties, integrator_host.h): at most 65535 each, NULL with "at most 65535 emitter / BSDF samples" beyond that --
   narrower than mi_render_params, whose two fields are uint32_t */
void *mi_host_create_direct(int strictNormals, int hideEmitters, int sampler, uint32_t spp, uint64_t seed, const uint32_t *devices, uint32_t n_devices, uint32_t planes_per_batch, uint32_t emitterSamples, uint32_t bsdfSamples, double preview_interval_ms);
/* integrator = MI_INTEGRATOR_AO: shadingSamples / rayLength of ao.cpp:40-48 (rayLength < 0: automatic, half the radius of the scene's bounding sphere); NULL when
   shadingSamples is 0.  maxDepth, rrDepth, strictNormals and hideEmitters play no part in this integrator and are not asked for */
void *mi_host_create_ao(int sampler, uint32_t spp, uint64_t seed, const uint32_t *devices, uint32_t n_devices, uint32_t planes_per_batch, uint32_t shadingSamples, float rayLength, double preview_interval_ms);
void mi_host_destroy(void *integrator);
int mi_host_preprocess(void *integrator, mi_scene *scene);
/* Controls = {continu, abort, interrupt}: returns 0 done, -1 *abort set, -2 *continu cleared, otherwise progress()'s non-zero value;
 * targetRGBA: (H+2b)x(W+2b)x4 un-normalised sums; all work on threadIdx 0 */
int mi_host_render(void *integrator, float *targetRGBA, const int *continu, const int *abort_flag, int (*progress)(double spp, void *user), void *user, int threadIdx, int threadCount);
/* in-place edits (mi_scene_update_* of mi355pt.h) of the scene given to mi_host_preprocess and of every replica, between two mi_host_render calls; 0 = applied,
 * otherwise refused (message in mi_host_last_error) and nothing changed */
int mi_host_set_camera(void *integrator, const float *sample_to_camera16, const float *to_world16, float near_clip, float far_clip);
int mi_host_set_lens(void *integrator, float aperture_radius, float focus_distance);   /* mi_scene_update_lens on the borrowed scene and every replica */
int mi_host_set_materials(void *integrator, const mi_material *materials, uint32_t n);
int mi_host_set_emitters(void *integrator, const mi_emitter *emitters, uint32_t n);
int mi_host_set_envmap_transform(void *integrator, const float *to_world16, float scale);
int mi_host_set_vertices(void *integrator, const float *pos, const float *nrm, uint32_t n_verts);   /* mi_scene_update_vertices */
int mi_host_set_instances(void *integrator, const mi_instance *instances, uint32_t n);   /* mi_scene_update_instances */
int mi_host_set_geometry(void *integrator, const float *pos, const float *nrm, uint32_t n_verts, const mi_instance *instances, uint32_t n_instances);   /* mi_scene_update_geometry */
void mi_host_cancel(void *integrator);
const char *mi_host_statistics(void *integrator);
#ifdef __cplusplus
}
#endif
#endif
