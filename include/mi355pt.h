/* include/mi355pt.h -- C-ABI of libmi355pt.so: the MI355X (gfx950) wavefront path tracer behind the reference's
 * Integrator / ResponsiveIntegrator boundary.
 *
 * Plain C: opaque handles, plain pointers and sizes, every call returns an int status (0 = MI_OK) and leaves a
 * message for mi_last_error().  No exceptions cross this boundary.  What each entry point replaces in the reference
 * (paths relative to the reference tree) is cited next to it; the adapter plugin (mitsuba-im_amd/csrc/adapter/path_hip.cpp,
 * INTEGRATION.md) fills these calls from a live mitsuba::Scene.
 */
#ifndef MI355PT_H
#define MI355PT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_ERR_INVALID 1     /* bad argument / call order            */
#define MI_ERR_DEVICE 2      /* HIP error (message has the HIP text)  */
#define MI_ERR_UNSUPPORTED 3 /* scene feature outside the hot path    */
#define MI_CANCELLED 4       /* mi_render_cancel() was observed       */

typedef struct mi_scene mi_scene;
typedef struct mi_render mi_render;

/* One mesh of the flattened scene = one mitsuba::TriMesh (include/mitsuba/render/trimesh.h:122-160). */
typedef struct {
    uint32_t first_tri, tri_count, first_vert, vert_count;
    int32_t bsdf;        /* index into the material table (Shape::getBSDF, include/mitsuba/render/shape.h) */
    int32_t emitter;     /* index into the emitter table or -1 (Shape::getEmitter)                          */
    uint32_t flags;      /* bit0: face normals (TriMesh "faceNormals", src/librender/trimesh.cpp:70); bit1: the mesh has texture coordinates
                            (`uv` of mi_scene_set_triangles): its.uv is interpolated from them and the triangle's UV tangent replaces the first
                            edge as dpdu (TriMesh::computeUVTangents, trimesh.cpp:683-736; skdtree.h:373-376, 402-408) */
    uint32_t group;      /* 0: the mesh is a scene shape; g > 0: it is a member of shape group g - 1 (src/shapes/shapegroup.cpp) and
                            appears in the scene only through mi_instance records; group members cannot be emitters (shapegroup.cpp:75-76) */
} mi_shape;

/* src/shapes/instance.cpp: one placement of shape group `group`; to_world = the instance transform, to_object = its inverse as the
 * reference computes it.  Groups hold triangle meshes; nested instancing is not permitted (shapegroup.cpp:71-72). */
typedef struct { uint32_t group; uint32_t pad[3]; float to_world[16], to_object[16]; } mi_instance;
/* Participating medium: HomogeneousMedium (src/medium/homogeneous.cpp) with its phase function (src/phase/isotropic.cpp, src/phase/hg.cpp).  sigma_a / sigma_s:
 * the final coefficients (`scale` and presets folded in by the caller, medium.cpp:27-37); strategy: MI_MEDIUM_BALANCE / SINGLE / MANUAL (`maximum` is refused);
 * sampling_density, medium_sampling_weight: as the constructor derives them (homogeneous.cpp:168-222); phase: MI_PHASE_ISOTROPIC / MI_PHASE_HG with mean cosine g */
#define MI_MEDIUM_BALANCE 0
#define MI_MEDIUM_SINGLE 1
#define MI_MEDIUM_MANUAL 2
#define MI_PHASE_ISOTROPIC 0
#define MI_PHASE_HG 1
typedef struct { float sigma_a[3], sigma_s[3]; uint32_t strategy; float sampling_density, medium_sampling_weight; uint32_t phase; float g; uint32_t pad; } mi_medium;
#define MI_INTEGRATOR_PATH 0            /* MIPathTracer, src/integrators/path/path.cpp */
#define MI_INTEGRATOR_VOLPATH_SIMPLE 1  /* SimpleVolumetricPathTracer, src/integrators/path/volpath_simple.cpp */
#define MI_INTEGRATOR_VOLPATH 2         /* VolumetricPathTracer, src/integrators/path/volpath.cpp: multiple importance sampling, emitters found through index-matched boundaries */
#define MI_INTEGRATOR_DIRECT 3          /* MIDirectIntegrator, src/integrators/direct/direct.cpp: one camera hit, emitter_samples emitter + bsdf_samples BSDF samples, power heuristic */
#define MI_INTEGRATOR_AO 4              /* AmbientOcclusionIntegrator, src/integrators/direct/ao.cpp: one camera hit, shading_samples cosine-distributed any-hit rays of length ray_length */

#define MI_BSDF_DIFFUSE 0         /* src/bsdfs/diffuse.cpp: reflectance                                                              */
#define MI_BSDF_ROUGHCONDUCTOR 1  /* src/bsdfs/roughconductor.cpp + microfacet.h: alpha (alphaU), distr, eta, k, specular; flags: sampleVisible, anisotropic */
#define MI_BSDF_CONDUCTOR 2       /* src/bsdfs/conductor.cpp: eta, k (already divided by the exterior index), specular               */
#define MI_BSDF_DIELECTRIC 3      /* src/bsdfs/dielectric.cpp: eta[0] = intIOR / extIOR, specular = specularReflectance, reflectance = specularTransmittance */
#define MI_BSDF_PLASTIC 4         /* src/bsdfs/plastic.cpp: eta[0] = intIOR / extIOR, specular = specularReflectance, reflectance = diffuseReflectance,
                                     k[0] = fresnelDiffuseReflectance(1 / eta, false) (SmoothPlastic::m_fdrInt, plastic.cpp:200)       */
#define MI_BSDF_ROUGHDIELECTRIC 5 /* src/bsdfs/roughdielectric.cpp: alpha, distr, eta[0], specular = specularReflectance, reflectance = specularTransmittance */
#define MI_BSDF_DIFFTRANS 6       /* src/bsdfs/difftrans.cpp: reflectance = transmittance                                            */
#define MI_BSDF_ROUGHPLASTIC 7    /* src/bsdfs/roughplastic.cpp: alpha, distr, eta[0], specular, reflectance = diffuseReflectance; k[0] = internal diffuse rough
                                     transmittance (m_internalRoughTransmittance->evalDiffuse(alpha), roughplastic.cpp:372), k[1] / k[2] = offset / length of the
                                     external rough-transmittance slice (RoughTransmittance after setEta + setAlpha, src/bsdfs/rtrans.h:292-388) in the table
                                     buffer of mi_scene_set_material_tables */
#define MI_BSDF_THINDIELECTRIC 8  /* src/bsdfs/thindielectric.cpp: eta[0] = intIOR / extIOR, specular = specularReflectance, reflectance = specularTransmittance (ENull transmission) */
#define MI_BSDF_MASK 9            /* src/bsdfs/mask.cpp: reflectance = opacity (constant or a bound texture), distr = index of the nested material record; ENull pass-through lobe */
#define MI_BSDF_MIXTURE 10        /* src/bsdfs/mixturebsdf.cpp: distr = number of children (2..4); their material record indices as numbers in reflectance[0..2], eta[0],
                                     their weights in k[0..2], specular[0] (rescaled when they sum to more than one, ensureEnergyConservation).  Children are plain
                                     BSDF records without textures, at most one of them with a Dirac delta component */
#define MI_BSDF_BUMPMAP 11        /* src/bsdfs/bumpmap.cpp: distr = index of the nested record (a plain BSDF or a mixturebsdf), bound texture (MI_BSDF_TEXTURE) = the displacement,
                                     alpha = the factor of an enclosing <texture type="scale"> (1 = none); meshes need texture coordinates */
#define MI_BSDF_NORMALMAP 12      /* src/bsdfs/normalmap.cpp: distr = nested record, bound texture = tangent-space normals (rgb = 0.5 + 0.5 n).  Adapters nest in the
                                     order mask -> bumpmap / normalmap -> mixturebsdf -> plain BSDF */
#define MI_BSDF_NULL 13           /* src/bsdfs/null.cpp: the index-matched boundary of a participating medium (straight pass-through, ENull; no parameters) */
#define MI_BSDF_ROUGHDIFFUSE 14    /* src/bsdfs/roughdiffuse.cpp (Oren-Nayar): reflectance (constant or a bound texture), alpha, distr = 1: useFastApprox */
#define MI_BSDF_PHONG 15           /* src/bsdfs/phong.cpp (modified Phong): reflectance = diffuseReflectance, specular = specularReflectance, alpha = exponent,
                                      k[0] = specular sampling weight = lum(specular) / (lum(diffuse) + lum(specular)) (phong.cpp:104-108); constants only */
#define MI_BSDF_WARD 16            /* src/bsdfs/ward.cpp: reflectance = diffuseReflectance, specular = specularReflectance, alpha = alphaU, k[1] = alphaV, distr = variant
                                      (0 ward, 1 ward-duer, 2 balanced), k[0] = specular sampling weight as for phong; constants only */
#define MI_BSDF_COATING 17         /* src/bsdfs/coating.cpp (smooth dielectric layer): distr = nested record (a plain BSDF without transmission, not twosided itself), eta[0] = intIOR /
                                      extIOR, alpha = thickness, reflectance = sigmaA, specular = specularReflectance; may be twosided, and may sit under a mask / bumpmap / normalmap.
                                      Path integrator only */
#define MI_BSDF_BLEND 18           /* src/bsdfs/blendbsdf.cpp: eta[0], eta[1] = the two child records (plain BSDFs, as for mixturebsdf), reflectance = (w, w, w) for a constant
                                      weight or the value of the bound `weight` texture; may be twosided and may sit under a mask / bumpmap / normalmap.  Path integrator only */
#define MI_BSDF_ROUGHCOATING 19    /* src/bsdfs/roughcoating.cpp (rough dielectric layer): distr = nested record (a plain reflective BSDF without a delta lobe), eta[0] = intIOR / extIOR,
                                      eta[1] = thickness, eta[2] = microfacet distribution (0 beckmann, 1 ggx, 2 phong), alpha, flags bit 1 = sampleVisible, reflectance = sigmaA, specular,
                                      k[1], k[2] = offset / length of its rough-transmittance slice in the material tables (as for roughplastic).  Path integrator only */
#define MI_BSDF_FLAG_TWOSIDED 1u  /* wrapped in src/bsdfs/twosided.cpp             */
#define MI_BSDF_FLAG_SAMPLE_VISIBLE 2u
#define MI_BSDF_FLAG_NONLINEAR 4u /* plastic "nonlinear" */
#define MI_BSDF_FLAG_ANISOTROPIC 8u /* alphaU = alpha, alphaV = reflectance[0] (roughconductor) / k[0] (roughdielectric) (src/bsdfs/microfacet.h:116-127); mesh shapes need texture coordinates */
#define MI_BSDF_TEXTURE(i) (((uint32_t) (i) + 1u) << 8)   /* flags bits 8..23: texture i (mi_scene_set_textures) bound to `reflectance`: diffuse.reflectance, plastic / roughplastic.diffuseReflectance, difftrans.transmittance, mask.opacity; a bitmap texture record carries its average in color0 (plastic lobe weights, plastic.cpp:204-207) */

/* 2-D procedural textures over Texture2D (src/librender/texture.cpp:81-121: uv * scale + offset): src/textures/checkerboard.cpp, gridtexture.cpp */
#define MI_TEXTURE_CHECKERBOARD 0
#define MI_TEXTURE_GRID 1
#define MI_TEXTURE_BITMAP 2       /* src/textures/bitmap.cpp over TMIPMap (include/mitsuba/render/mipmap.h).  The MIP pyramid is INPUT DATA: levels
                                     [first_level, first_level + n_levels) of mi_scene_set_texture_data, exactly as the reference builds them (Bitmap::resample
                                     with a 2-lobed Lanczos filter, texels rounded to half; the adapter obtains them from the reference's own code).
                                     wrap_u / wrap_v: 0 clamp, 1 repeat, 2 mirror, 3 zero, 4 one (ReconstructionFilter::EBoundaryCondition); filter: 0 nearest,
                                     1 bilinear, 2 trilinear, 3 ewa (EMIPFilterType); camera hits filter through Intersection::computePartials */
typedef struct { uint32_t type; float color0[3], color1[3]; float line_width; float uoffset, voffset, uscale, vscale;
                 uint32_t wrap_u, wrap_v, filter; float max_anisotropy; uint32_t first_level, n_levels; } mi_texture;
typedef struct {
    uint32_t type, flags, distr;  /* distr: 0 beckmann, 1 ggx, 2 phong / Ashikhmin-Shirley (roughconductor, roughdielectric, roughplastic; samples all normals, microfacet.h:141-145) */
    float alpha;
    float reflectance[3], eta[3], k[3], specular[3];
} mi_material;

#define MI_EMITTER_AREA 0         /* src/emitters/area.cpp   */
#define MI_EMITTER_ENVMAP 1       /* src/emitters/envmap.cpp */
#define MI_EMITTER_CONSTANT 2     /* src/emitters/constant.cpp: `radiance`                                                   */
#define MI_EMITTER_POINT 3        /* src/emitters/point.cpp: `radiance` = intensity, position = translation of to_world     */
#define MI_EMITTER_SPOT 4         /* src/emitters/spot.cpp: intensity, to_world, cutoff / beam = cutoffAngle / beamWidth in degrees (no texture) */
#define MI_EMITTER_DIRECTIONAL 5  /* src/emitters/directional.cpp: `radiance` = irradiance, travel direction = to_world z axis */
/* 6: reserved (scene files: the compound `sunsky`, expanded by the reference itself inside the drop-in plugin) */
#define MI_EMITTER_COLLIMATED 7   /* src/emitters/collimated.cpp: `radiance` = power, position = translation of to_world.  A 0-D emitter: sampleDirect always fails (collimated.cpp:129-133), so in this
                                     unidirectional integrator it contributes nothing itself -- but it takes its share of the emitter-selection probability, exactly as in the reference */
/* shape: area lights only (index into the shape list; >= n_shapes: analytic shape shape - n_shapes), else -1 */
typedef struct { uint32_t type; int32_t shape; float radiance[3]; float weight; float cutoff, beam; float to_world[16]; } mi_emitter;

/* Analytic shapes behind Scene::rayIntersect (kd-tree leaf redirect, include/mitsuba/render/skdtree.h:292-301): src/shapes/rectangle.cpp,
 * disk.cpp, sphere.cpp, cylinder.cpp.  to_world = the shape's objectToWorld AFTER its constructor (sphere.cpp:113-123 and
 * cylinder.cpp:85-106 split the scale off into radius / length; rectangle.cpp:82-84 and disk.cpp:83-87 fold flipNormals into the
 * transform), to_object = its inverse as the reference computes it; radius: sphere, cylinder; length: cylinder. */
#define MI_SHAPE_RECTANGLE 0
#define MI_SHAPE_DISK 1
#define MI_SHAPE_SPHERE 2
#define MI_SHAPE_CYLINDER 3
#define MI_ANALYTIC_FLIP_NORMALS 1u   /* sphere / cylinder "flipNormals" */
typedef struct {
    uint32_t type; int32_t bsdf, emitter; uint32_t flags;
    float to_world[16], to_object[16];
    float radius, length; float pad[2];
} mi_analytic;

/* Integrator + sampler parameters: MonteCarloIntegrator properties (src/librender/integrator.cpp:191-226),
 * sampler properties (src/samplers/sobol.cpp:86-107; src/samplers/independent.cpp:51-60). */
#define MI_SAMPLER_INDEPENDENT 0  /* build-defined counter-based stream, seedable */
#define MI_SAMPLER_SOBOL 1
typedef struct {
    int32_t max_depth, rr_depth;
    uint32_t strict_normals, hide_emitters;
    uint32_t sampler, spp;
    uint64_t seed;               /* independent: seed of the counter stream; sobol: the sampler's `scramble` value (0 = unscrambled; src/samplers/sobol.cpp:92-102) */
    uint32_t device;             /* HIP device ordinal */
    uint32_t planes_per_batch;   /* sample planes traced per wavefront batch (0 = auto) */
    uint32_t opacity;            /* 1: alpha = 1 where the camera ray hits a surface, else 0 (RadianceQueryRecord::EOpacity, records.inl:121-137:
                                    the responsive drivers and films with an alpha channel); 0: alpha = 1 (classic film without alpha, integrator.cpp:160-161) */
    uint32_t integrator;         /* MI_INTEGRATOR_PATH (0, default), MI_INTEGRATOR_VOLPATH_SIMPLE or MI_INTEGRATOR_VOLPATH: the same loop over participating media (mi_scene_set_media);
                                    MI_INTEGRATOR_DIRECT: direct illumination (no media, no mixturebsdf / bumpmap / normalmap / coating / roughcoating / blendbsdf / null records; max_depth and
                                    rr_depth are validated and otherwise ignored); MI_INTEGRATOR_AO: ambient occlusion (reads no BSDF, emitter or medium: every scene is accepted; max_depth, rr_depth, strict_normals
                                    and hide_emitters play no part); anything else: MI_ERR_UNSUPPORTED.  (Round 1 had `fast_math` here; one set of kernels ships: strict IEEE arithmetic) */
    uint32_t emitter_samples;    /* MI_INTEGRATOR_DIRECT only (not read otherwise: callers of the other integrators may pass the struct without these two fields): */
    uint32_t bsdf_samples;       /* `emitterSamples` / `bsdfSamples` of direct.cpp:96-107 (`shadingSamples` sets both); either may be 0, not both */
    uint32_t shading_samples;    /* MI_INTEGRATOR_AO only (not read otherwise: callers of the other integrators may pass the struct without these two fields): */
    float ray_length;            /* `shadingSamples` (>= 1) / `rayLength` of ao.cpp:72-80; ray_length < 0: automatic, half the radius of the scene's bounding sphere */
} mi_render_params;

typedef struct { uint32_t x0, y0, x1, y1; } mi_tile;   /* pixel rectangle [x0,x1) x [y0,y1) in GLOBAL film coordinates */

typedef struct {
    uint64_t rays, shadow_rays, path_length_sum, samples;  /* = reference StatsCounters "Normal rays traced", "Shadow rays traced",
                                                              avgPathLength (src/librender/skdtree.cpp:46-47, src/integrators/path/path.cpp:24) */
    double render_ms;                                      /* device time of the last mi_render_run (HIP events) */
    double extend_ms, shade_ms, shadow_ms, other_ms;       /* per-stage device time of the last run (0 unless profiling enabled) */
    uint64_t extend_launches, extend_rays;                 /* extend launches TIMED in the last run (first stream only) / closest-hit rays since clear */
    uint64_t extend_launches_all;                          /* extend launches of the last run on all streams */
} mi_stats;

const char *mi_last_error(void);

/* Sobol' tables (data): matrices32[dims][52], vdc[16][52], vdc_inv[16][52] (the tables of src/samplers/sobolseq.cpp:33,106537,107241).
 * Must be called once before a Sobol render; mitsuba-im_amd loads them from mitsuba-im_amd/data/sobol_tables.bin. */
int mi_set_sobol_tables(const uint32_t *matrices32, uint32_t dims, const uint64_t *vdc, const uint64_t *vdc_inv);
/* Same from a file; mi_scene_commit loads <dir of libmi355pt.so>/data/sobol_tables.bin (or $MI355PT_DATA/sobol_tables.bin) by itself
 * when no tables were set. */
int mi_load_sobol_tables(const char *path);

/* -- scene: replaces Scene::initialize -> ShapeKDTree::build (src/librender/scene.cpp:330-392, src/librender/skdtree.cpp:68-105) -- */
int mi_scene_create(mi_scene **out);
void mi_scene_destroy(mi_scene *s);
/* TriMesh::getVertexPositions/getVertexNormals/getVertexTexcoords/getTriangles of all meshes, concatenated; nrm/uv may be NULL */
int mi_scene_set_triangles(mi_scene *s, const float *pos, const float *nrm, const float *uv, const uint32_t *idx,
                           uint32_t n_verts, uint32_t n_tris, const mi_shape *shapes, uint32_t n_shapes);
/* analytic shapes, numbered after the meshes: shape index n_shapes + i, primitive index n_tris + i (Scene::getShapes order with the
 * meshes first).  Either call may be omitted, but a scene needs at least one primitive. */
int mi_scene_set_analytic(mi_scene *s, const mi_analytic *shapes, uint32_t n);
/* instances of shape groups; primitive index of the i-th: n_tris + n_analytic + i (they come last in Scene::getShapes order here) */
int mi_scene_set_instances(mi_scene *s, const mi_instance *instances, uint32_t n);
/* Media of the scene and who refers to them (Shape::addChild "interior" / "exterior", src/librender/shape.cpp:156-170; Sensor medium, src/librender/emitter.cpp:51-54):
 * shape_media[(n_shapes + n_analytic)][2] = (interior, exterior) medium index of every mesh, then every analytic shape, -1 = none; sensor_medium = the medium the
 * camera sits in or -1.  Only the volumetric integrators look at them. */
int mi_scene_set_media(mi_scene *s, const mi_medium *media, uint32_t n, const int32_t *shape_media, uint32_t n_pairs, int32_t sensor_medium);
int mi_scene_set_materials(mi_scene *s, const mi_material *materials, uint32_t n);
int mi_scene_set_textures(mi_scene *s, const mi_texture *textures, uint32_t n);
/* MIP levels of the bitmap textures: levels[n_levels][3] = (width, height, offset of the level's first float in `texels`), RGB floats row-major */
int mi_scene_set_texture_data(mi_scene *s, const uint32_t *levels, uint32_t n_levels, const float *texels, uint64_t n_texels);
int mi_scene_set_material_tables(mi_scene *s, const float *data, uint32_t n);   /* float tables the materials refer to by offset (roughplastic) */
int mi_scene_set_emitters(mi_scene *s, const mi_emitter *emitters, uint32_t n);    /* Scene::getEmitters order; samplingWeight in .weight */
int mi_scene_set_envmap(mi_scene *s, const float *rgb, uint32_t w, uint32_t h, const float *to_world16, float scale);
/* MIP pyramid of the environment map = record `texture` of mi_scene_set_textures (type bitmap, u repeats, v clamps, EWA, anisotropy 10: the settings of
 * src/emitters/envmap.cpp:144-145, 182-185; level 0 = the map itself): camera rays that leave the scene then get the filtered lookup of
 * EnvironmentMap::evalEnvironment (envmap.cpp:398-411).  -1 (default): level-0 bilinear lookups for them as for every other ray */
int mi_scene_set_envmap_filter(mi_scene *s, int32_t texture);
/* PerspectiveCameraImpl: m_sampleToCamera, world transform, clip planes (src/sensors/perspective.cpp:126-178) */
int mi_scene_set_camera(mi_scene *s, const float *sample_to_camera16, const float *to_world16, float near_clip, float far_clip);
/* Thin lens on top of the perspective camera (src/sensors/thinlens.cpp:324-361): aperture radius in world units and the distance of the focal plane along the camera's
 * z axis.  Every sample then draws an aperture point -- the sampler's next 2-D value after the pixel offset (src/librender/integrator.cpp:172-175): Sobol dimensions 2 / 3 --
 * and every later draw of the path moves by two dimensions.  Before mi_scene_commit; radius 0 removes the lens (the pinhole, the default; focus_distance is then ignored).
 * MI_ERR_INVALID: null scene, a negative or non-finite radius, a non-positive or non-finite focus distance with a positive radius. */
int mi_scene_set_lens(mi_scene *s, float aperture_radius, float focus_distance);
/* Film crop size + reconstruction filter (src/librender/film.cpp:92; src/rfilters/<name>.cpp): kind 0 box(radius), 1 gaussian(stddev), 2 tent,
 * 3 mitchell (B in `radius`, C in `stddev`), 4 catmullrom, 5 lanczos (lobes in `radius`) */
int mi_scene_set_film(mi_scene *s, uint32_t width, uint32_t height, uint32_t filter_kind, float radius, float stddev);
int mi_scene_commit(mi_scene *s, uint32_t device);   /* BVH build + TriAccel table + upload */
/* A replica of a committed scene on HIP device `device` (may be the source's own): multi-device renders keep one scene copy per device, as the reference
 * ships the scene to every worker (src/librender/renderjob.cpp, sched_remote.cpp).  The host-side build is reused, only the upload is repeated. */
int mi_scene_clone(mi_scene *s, uint32_t device, mi_scene **out);

/* -- in-place edits of a COMMITTED scene: what the interactive shell does between two short renders (src/im-mts/shell.cpp:236-242 restarts a frame without
 *    preprocess).  The scene stays committed; the tree, the triangle records, textures, Sobol tables, the environment image and its CDFs are neither rebuilt nor
 *    sent again.  After an update every result equals that of a fresh mi_scene_create ... mi_scene_commit with the new parameters.
 *    Values only: the record count, a record's type, a material's texture binding (flags bits 8..23), its anisotropic / nonlinear / sampleVisible bits, `distr` of a
 *    wrapper (mask, mixturebsdf, bumpmap, normalmap, coating, roughcoating, blendbsdf), the child indices of a mixturebsdf / blendbsdf, the rough-transmittance slice
 *    (k[1], k[2]) and an emitter's `shape` select kernel variants, table sizes or the per-triangle layout: a change of one of them is MI_ERR_UNSUPPORTED, the message
 *    names the first offending record, the scene is left as it was.  `twosided` may change.  The value checks of mi_scene_set_materials / _emitters apply.
 *    Call them between runs: while a render runs on the scene an update returns MI_ERR_INVALID (cancel the run and wait for it first).  A render handle follows the
 *    scene: its next run traces the edited scene -- after mi_render_clear; a run that would add to a film holding samples of the earlier scene returns MI_ERR_INVALID.
 *    A replica (mi_scene_clone) is a scene of its own and is updated by its owner. */
int mi_scene_update_camera(mi_scene *s, const float *sample_to_camera16, const float *to_world16, float near_clip, float far_clip);
/* Focus pull / aperture change on a committed lens scene: both values in place, nothing else is recomputed or sent.  The checks of mi_scene_set_lens apply (messages
 * start with "mi_scene_update_lens: "); turning a lens on (scene committed without one) or off (radius 0 on a lens scene) changes the sample layout of every path:
 * MI_ERR_UNSUPPORTED, the scene is left as it was. */
int mi_scene_update_lens(mi_scene *s, float aperture_radius, float focus_distance);
int mi_scene_update_materials(mi_scene *s, const mi_material *materials, uint32_t n);
int mi_scene_update_emitters(mi_scene *s, const mi_emitter *emitters, uint32_t n);
int mi_scene_update_envmap_transform(mi_scene *s, const float *to_world16, float scale);   /* envmap scenes only */
/* Vertex edit: new positions pos[n_verts * 3] for the WHOLE concatenated vertex array of mi_scene_set_triangles, and new vertex normals nrm[n_verts * 3] if and only if
 * the scene was committed with normals.  Indices, texture coordinates and shapes stay as committed.  The device recomputes every per-triangle record (Wald records, the
 * geometric words of the shading records, UV tangents) and REFITS the existing tree bottom-up: topology, child codes and node numbering stay, every box is recomputed
 * from the boxes below it.  The scene box, the packet tables of small scenes, the area lights' CDFs and the bounding spheres follow on the host.  Results equal those of
 * a fresh commit of the new vertices bit for bit (the nearest hit does not depend on the tree).  Like the other updates: between runs, advances `revision`, never moves
 * `tree_builds`, a render handle follows after mi_render_clear, a replica is a scene of its own.  Returns when the device has finished.
 * MI_ERR_INVALID: scene not committed, null argument, n_verts differs from the committed count, nrm given for a scene without normals or missing for one with, a
 * non-finite position or normal (the message names the first vertex), a run in flight.  MI_ERR_UNSUPPORTED: scenes with shape groups / instances (the message names
 * the first instance): group boxes, instance boxes and the two-level tree are not refitted.  A refused call leaves the scene untouched, and so does a failed allocation
 * of the edit's own device tables (MI_ERR_DEVICE, "the scene is unchanged").  Any other MI_ERR_DEVICE (a failed copy or launch) comes after the host side has taken the
 * new vertices: host and device tables are then out of step and the scene must be committed again.
 * The tree keeps the topology the SAH build chose for the committed vertices; after a large deformation it is no longer the optimum for the new ones and traversal slows
 * down (results stay exact).  A fresh mi_scene_commit is the remedy. */
int mi_scene_update_vertices(mi_scene *s, const float *pos, const float *nrm, uint32_t n_verts);
/* Instance edit: new to_world / to_object for ALL committed instances, in the order of mi_scene_set_instances; `group` of every record must be the committed one.
 * to_object is taken from the caller, as mi_scene_set_instances takes it: nothing is inverted here.  The device rewrites the two matrices of every instance record and
 * the box of its leaf in the scene-level tree, then REFITS the scene-level tree bottom-up as a vertex edit does (topology, child codes and node numbering stay).  The
 * groups' geometry, trees and boxes and every per-triangle record are untouched; the scene box and the bounding spheres that depend on it follow on the host.  Results
 * equal those of a fresh commit with the new instances bit for bit.  Like the other updates: between runs, advances `revision`, never moves `tree_builds`, a render
 * handle follows after mi_render_clear, a replica is a scene of its own.  Returns when the device has finished.
 * MI_ERR_INVALID: null argument, scene not committed, a run in flight, a scene committed without instances ("the scene has no instances"), n differs from the committed
 * count (the message gives both), a non-finite entry in to_world or to_object (the message names the first instance).  MI_ERR_UNSUPPORTED: an instance whose `group`
 * differs from the committed one (structural: it selects another tree; the message names the first instance).  A refused call leaves the scene untouched, and so does a
 * failed allocation of the edit's own device tables (MI_ERR_DEVICE, "the scene is unchanged").  Any other MI_ERR_DEVICE (a failed copy or launch) comes after the host
 * side has taken the new instances: host and device tables are then out of step and the scene must be committed again.
 * The scene-level tree keeps the topology the SAH build chose for the committed placement; after large moves traversal slows down (results stay exact).  A fresh
 * mi_scene_commit is the remedy.  mi_scene_update_vertices still refuses scenes with instances: mi_scene_update_geometry (below) moves the vertices of group members. */
int mi_scene_update_instances(mi_scene *s, const mi_instance *instances, uint32_t n);
/* Geometry edit: one frame of an animation in one call -- new positions pos[n_verts * 3] (and normals, if and only if the scene was committed with them) for the WHOLE
 * vertex array, the members of shape groups included, and / or new to_world / to_object for ALL committed instances.  pos = nrm = NULL, n_verts = 0: the vertices stay;
 * instances = NULL, n_instances = 0: the placements stay; both NULL: MI_ERR_INVALID.  Works on every committed scene: without instances and with instances = NULL it
 * does what mi_scene_update_vertices does (packet tables included), with `instances` alone what mi_scene_update_instances does.  With vertices on a scene with shape
 * groups it also recomputes, by the commit's own rules, the group boxes (host), from them glo / ghi of every instance record and the box of its leaf (device), every
 * per-triangle record and leaf box (device), and REFITS every tree -- the scene level and each group's -- bottom-up on the device; the scene box, the scene-level area
 * lights' CDFs and the bounding spheres follow on the host.  One push of the inputs, one chain of launches on one stream, one `revision` step; `tree_builds` never
 * moves.  Results and device tables equal those of a fresh commit of the new description bit for bit.  Returns when the device has finished.
 * MI_ERR_INVALID: null scene, scene not committed, a run in flight, both parts NULL, a count without its array, n_verts differs from the committed count, nrm given for a
 * scene without normals or missing for one with, a non-finite position or normal (the message names the first vertex), `instances` on a scene without instances,
 * n_instances differs from the committed count, a non-finite entry in to_world / to_object (the message names the first instance).  MI_ERR_UNSUPPORTED: an instance
 * whose `group` differs from the committed one (the message names it).  Every message starts with "mi_scene_update_geometry: ".  All checks come before any change: a
 * refused call leaves the scene, its revision and its device tables untouched, and so does a failed allocation of the edit's own device tables (MI_ERR_DEVICE, "the
 * scene is unchanged").  Any other MI_ERR_DEVICE leaves host and device out of step: commit again.  May be mixed freely with mi_scene_update_vertices / _instances,
 * which are that call under their own names and refusals (the former keeps refusing scenes with shape groups or instances).  Counts, indices, an instance's group, media on group members and analytic
 * group members are out of reach of an update.  The trees keep the committed topology: after large deformations traversal slows down, a fresh commit is the remedy. */
int mi_scene_update_geometry(mi_scene *s, const float *pos, const float *nrm, uint32_t n_verts, const mi_instance *instances, uint32_t n_instances);
/* Frame mark: snapshots what a geometry or camera edit can change -- the vertex positions (shape-group members included), every instance's to_world, the 12 floats of
 * mi_scene_world_to_pixel and the camera origin -- as the "previous" state of the prevPosition / motion fields (below).  Previous = the state at the LAST mark, however
 * many edits followed it; a scene that was never marked, or was committed again since, has previous = current.  The device tables (vertex array, 48 B per instance) are
 * allocated by the first mark and freed with the scene; the host keeps the snapshot too, so that a replica (mi_scene_clone) carries it.  A mark renders nothing
 * differently and moves neither `revision` nor `tree_builds`.  Returns when the device has finished.  MI_ERR_INVALID: null scene, scene not committed, a run in flight,
 * a singular camera matrix; a failed allocation (MI_ERR_DEVICE) leaves the earlier mark in place. */
int mi_scene_mark_frame(mi_scene *s);
/* revision: in-place edits applied so far; tree_builds: host-side builds (tree, triangle records) this scene has gone through -- an update never moves it.  Either may be NULL */
int mi_scene_revision(mi_scene *s, uint64_t *revision, uint64_t *tree_builds);

/* -- render: replaces SamplingIntegrator::renderBlock / ImageOrderIntegrator::render over MIPathTracer::Li
 *    (src/librender/integrator.cpp:141-189, :336-402, :469-486; src/integrators/path/path.cpp:119-294) -- */
int mi_render_create(mi_scene *s, const mi_render_params *p, mi_render **out);
void mi_render_destroy(mi_render *r);
/* Trace sample planes [sample_begin, sample_end) of every pixel of `tile` and accumulate them into the device film
 * (ImageBlock::put, include/mitsuba/render/imageblock.h:161-221).  One caller per handle. */
int mi_render_run(mi_render *r, mi_tile tile, uint32_t sample_begin, uint32_t sample_end);
/* Same for the rows y0, y0 + row_stride, ... (< y1) of the tile only: interleaved row ownership across ranks for multi-GPU load balance
 * (rank k of N renders tile {0, k, W, H} with row_stride N). */
int mi_render_run_rows(mi_render *r, mi_tile tile, uint32_t row_stride, uint32_t sample_begin, uint32_t sample_end);
int mi_render_clear(mi_render *r);                  /* ImageBlock::clear */
void mi_render_cancel(mi_render *r);                /* Integrator::cancel: thread-safe flag, observed before every batch: the run that sees it returns MI_CANCELLED
                                                       and consumes it (a cancel issued between two runs stops the next one); mi_render_clear drops a pending cancel */
/* Film read-back.  layout 0: raw ImageBlock sums (H+2b) x (W+2b) x 5 {R,G,B,alpha,weight} incl. border (classic, ESpectrumAlphaWeight);
 * layout 1: (H+2b) x (W+2b) x 4 RGBA sums (responsive target, src/im-mts/scene.cpp:317-321); layout 2: H x W x 3 developed RGB = sum/weight. */
int mi_render_film_size(mi_render *r, int layout, uint32_t *height, uint32_t *width, uint32_t *channels, uint32_t *border);
int mi_render_read_film(mi_render *r, int layout, float *host_out);
int mi_render_read_film_device(mi_render *r, int layout, void *device_out);   /* device pointer (e.g. a torch tensor) for the RCCL reduce */
/* dst += src (raw film sums + ray counters): merge step of a render whose rows were split over several handles / devices with mi_render_run_rows; replaces
 * Film::put(block) under the RenderQueue mutex (src/librender/renderproc.cpp:142-149).  Other device: peer copy over xGMI, then one add kernel.  Both idle. */
int mi_render_merge_film(mi_render *dst, mi_render *src);
/* Debug / parity: Li of individual (px, py, sampleIndex) triples through the very same kernels; out_li[n*3] */
int mi_render_samples(mi_render *r, const uint32_t *pairs, uint64_t n, float *out_li);
int mi_render_stats(mi_render *r, mi_stats *out);

/* -- adaptive sampling: replaces the `adaptive` integrator wrapped around `path` / `volpath_simple` / `volpath` (src/integrators/misc/adaptive.cpp:202-319).
 *    Pixel p takes its samples k = 0, 1, 2, ... in order (the values mi_render_samples gives at (px, py, k)); each goes through ImageBlock::put (a rejected sample
 *    counts with luminance 0) and the online variance of :278-282; the pixel stops at max_sample_factor x spp samples, or, from spp samples on, as soon as
 *    sqrtf(variance / n) x quantile <= max_error x max(mean, average_luminance x 0.01f).  Its footprint enters the film scaled by 1.0f / n (:307-317), so the film's weights
 *    are those of ONE sample per pixel.  All float32, one rounding per operation: the count map equals a sequential model bit for bit whatever round_samples,
 *    planes_per_batch and the pool shape are.  Two deviations from the reference: quantile = |approx_erfinv(-1 + p_value)| x SQRT_TWO (the reference omits the absolute
 *    value and with it stops every pixel at spp); average_luminance <= 0 asks for the estimate over min(10000, W x H) pixels (i x W x H) / N at sample index 2^24 - 1.
 *    Independent sampler only (adaptive.cpp:150-152), spp >= 8 (:210-212), integrators path / volpath_simple / volpath, no field channels. */
typedef struct { float max_error, p_value; int32_t max_sample_factor; uint32_t round_samples; float average_luminance; uint32_t pad[3]; } mi_adaptive_params;   /* max_sample_factor < 0: no cap but the stream's 2^24 - 2; round_samples: sample indices per round, 0 = spp */
typedef struct { uint64_t samples_used, samples_traced; uint32_t rounds, pixels_at_cap, min_count, max_count; float average_luminance, quantile; } mi_adaptive_stats;   /* of the last adaptive run: used = sum of the counts, traced = used + the samples of a round that followed a pixel's stop */
int mi_render_set_adaptive(mi_render *r, const mi_adaptive_params *p);       /* NULL: off; only while the film is clear */
/* One adaptive render of `tile` into a CLEAR film; there is one adaptive run per mi_render_clear, and mi_render_run / mi_render_run_rows / mi_render_merge_film refuse a
 * film that holds one.  Rounds of round_samples sample indices over the compacted list of active pixels; the cancel flag is observed before every batch. */
int mi_render_run_adaptive(mi_render *r, mi_tile tile);
int mi_render_read_sample_counts(mi_render *r, uint32_t *out /* H x W, 0 = not rendered */);
int mi_render_adaptive_stats(mi_render *r, mi_adaptive_stats *out);

/* -- field channels: replaces the `multichannel` integrator with nested `field` integrators (src/integrators/misc/multichannel.cpp:164-221,
 *    src/integrators/misc/field.cpp:124-177).  Every sample of the radiance film also puts the data of its first camera hit into a field film, at the same film
 *    position through the same reconstruction filter; the radiance film is what it is without fields.  Kinds in the order of field.cpp's EField; each field is three
 *    values (a Spectrum), `undefined` is what a camera ray that leaves the scene returns:
 *      position        its.p
 *      relPosition     its.p through the inverse of the sensor's world transform: a 3 x 4 matrix, the inverse of mi_scene_set_camera's to_world computed on the host
 *                      in double precision and rounded to float, applied as a four-term float sum per component
 *      distance        (t, t, t)
 *      geoNormal       its.geoFrame.n          shNormal   its.shFrame.n          uv   (u, v, 0)
 *      albedo          its.shape->getBSDF()->getDiffuseReflectance(its): the (possibly textured, unfiltered lookup: there are no UV partials) diffuse reflectance of
 *                      diffuse / roughdiffuse / phong / ward, through twosided / bumpmap / normalmap; everything else by the generic rule of src/librender/bsdf.cpp:82-86
 *                      (eval with wi = wo = (0, 0, 1) under the diffuse-reflection mask, times pi): 0 for the conductors, dielectrics, difftrans and null, opacity x nested
 *                      for mask, the weighted sum of the children for mixturebsdf / blendbsdf.  Refused (MI_ERR_UNSUPPORTED naming the BSDF) on scenes holding a plastic,
 *                      roughplastic, coating or roughcoating record -- the material record does not carry their external transmittance -- or a mask over a bumpmap / normalmap
 *      shapeIndex      index of the hit shape: meshes in mi_scene_set_triangles order, then the analytic shapes; -1 for a hit through an instance (its.shape is then the group
 *                      member, which is not in the scene's shape list: field.cpp:158-167, skdtree.h:416)
 *      primIndex       triangle index within its mesh, also for instanced meshes (skdtree.h:418); 0 for analytic shapes (the reference leaves its.primIndex unset there)
 *    Two kinds beyond field.cpp's nine follow the scene through its in-place edits; "previous" is the scene's state at the last mi_scene_mark_frame (never marked, or
 *    committed again since: previous = current).  binary32, one rounding per operation, in the order written (tests/motion_model.py restates it):
 *      prevPosition    P + (Bprev - Bcur), P = the `position` value.  With b = (1 - u - v, u, v) of the hit and bary(c0, c1, c2) = (c0 b.x + c1 b.y) + c2 b.z per component:
 *                      a triangle outside a group: Bcur = bary of the corners in its shading record (the expression that gave P), Bprev = bary of the three marked vertices
 *                      with the triangle's indices; a member of a shape group hit through instance k: Bcur = T(bary of the current object-space corners), Bprev =
 *                      Tprev(bary of the marked object-space corners), T / Tprev = rows 0..2 of instance k's current / marked to_world applied as
 *                      ((m0 x + m1 y) + m2 z) + m3 per row; an analytic shape cannot move in place: P.  What did not move since the mark -- the static part of a partly
 *                      deformed mesh included -- therefore has prevPosition == position bit for bit
 *      motion          the reference's `motion` integrator in its configuration "d" (src/integrators/misc/motion.cpp:176-201, 258-269) with the marked frame as the target:
 *                      (Xprev - Xcur, Yprev - Ycur, dprev - dcur).  For q = prevPosition and the projection M marked by mi_scene_mark_frame (the 12 floats of
 *                      mi_scene_world_to_pixel): Wc = ((M[8] q.x + M[9] q.y) + M[10] q.z) + M[11], Xprev = (the same sum of M[0..3]) / Wc, Yprev likewise from M[4..7];
 *                      Xcur, Ycur from P and the current projection; d = sqrtf((e.x e.x + e.y e.y) + e.z e.z) with e = q - the marked camera origin (the translation column
 *                      of the camera's to_world), and with e = P - the current origin.  !(Wc > 0) on either side: the field's `undefined` value
 *    The host mirror, the drop-in plugin, multi-device renders and adaptive renders do not follow the marked state; the reference's specular configurations ("rd", "ttd", ...)
 *    are not built.
 *    No finite / non-negative check is applied to field values (multichannel.cpp:41-44). */
#define MI_FIELD_POSITION 0
#define MI_FIELD_REL_POSITION 1
#define MI_FIELD_DISTANCE 2
#define MI_FIELD_GEO_NORMAL 3
#define MI_FIELD_SH_NORMAL 4
#define MI_FIELD_UV 5
#define MI_FIELD_ALBEDO 6
#define MI_FIELD_SHAPE_INDEX 7
#define MI_FIELD_PRIM_INDEX 8
#define MI_FIELD_PREV_POSITION 9
#define MI_FIELD_MOTION 10
typedef struct { uint32_t field; float undefined[3]; } mi_field;
/* n <= 8 fields; n = 0 removes them and frees the field film.  Allowed only while the film is clear (no samples since mi_render_create / mi_render_clear), else
 * MI_ERR_INVALID; an unknown kind or an albedo the scene's BSDFs do not support: MI_ERR_UNSUPPORTED.  Without fields a render launches, allocates and records nothing extra. */
int mi_render_set_fields(mi_render *r, const mi_field *fields, uint32_t n);
/* Field film read-back.  layout 0: raw sums (H+2b) x (W+2b) x (3F+1), the three values of every field in list order, then the film's own weight; layout 2: developed
 * H x W x 3F = sum x invWeight with invWeight = weight == 0 ? 0 : 1 / weight, two float roundings (src/libcore/bitmap.cpp:1621-1625).  Without fields: MI_ERR_INVALID.  mi_render_clear zeroes the field film, mi_render_run_rows fills its rows, mi_render_merge_film adds it
 * too when both handles hold the same field list (and fails with MI_ERR_INVALID when they do not). */
int mi_render_field_film_size(mi_render *r, int layout, uint32_t *height, uint32_t *width, uint32_t *channels, uint32_t *border);
int mi_render_read_fields(mi_render *r, int layout, float *host_out);
/* Debug / parity: the fields of individual (px, py, sampleIndex) triples, batched as mi_render_samples: generate, one extend, the field stage (no shading); out[n * 3F] */
int mi_render_field_samples(mi_render *r, const uint32_t *pairs, uint64_t n, float *out);

/* -- denoiser: the edge-avoiding a-trous filter of Dammertz, Sewtz, Hanika and Lensch (HPG 2010) with albedo demodulation, guided by the field channels; on the device
 *    (csrc/denoise.h, csrc/kernels_denoise.hip).  The reference has no such component.  All values are float32 and every operation is one rounding, in the order written,
 *    so the result equals a sequential model bit for bit (tests/denoise_model.py).
 *    Inputs: C, N, P = H x W x 3 colour, normal guide, position guide; A = H x W x 3 albedo (optional); iterations K in 0..8, sigma_color > 0, sigma_normal > 0,
 *    sigma_position != 0, demodulate 0 / 1.
 *      1. K = 0: the output is C bit for bit; nothing below runs (the resolved width returned is sigma_position if positive, else 0).
 *      2. sigma_position < 0 (automatic): over the pixels of P whose three components are all finite take the box, d = its extent per axis; the resolved width is
 *         |sigma_position| x sqrtf((d.x d.x + d.y d.y) + d.z d.z); no such pixel, or a diagonal of 0: the position term is off (kp = 0, resolved width 0).
 *      3. demodulate: D = A > 1e-3f ? A : 1e-3f per component (a NaN albedo gives 1e-3f), c_0 = C / D; otherwise c_0 = C.
 *      4. levels i = 0 .. K - 1, step s = 2^i: sc = sigma_color x 2^-i, kc = 1.0f / (sc sc), kn = 1.0f / (sigma_normal sigma_normal), kp = 1.0f / (sp sp) or 0.
 *         Pixel p visits the taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner; taps outside the image are skipped.  h = (1/16, 1/4, 3/8, 1/4, 1/16).
 *         d2(a) = (e.x e.x + e.y e.y) + e.z e.z with e = a(p) - a(q);  x = -((d2(c_i) kc + d2(N) kn) + d2(P) kp);  w = x >= -80.0f ? (h[dy] h[dx]) expf(x) : 0
 *         (glibc's expf; a NaN x fails the comparison, which drops every non-finite colour or guide).  A tap with w = 0 is skipped; otherwise sw += w and
 *         sum.k += w c_i(q).k for k = r, g, b.  c_{i+1}(p) = sw > 0 ? sum / sw : c_i(p): a pixel whose own colour or guides are non-finite keeps its value.
 *      5. output: c_K x D when demodulated, else c_K.
 *    Refused with MI_ERR_INVALID, the message naming the parameter: iterations > 8, a non-positive or non-finite sigma_color / sigma_normal, a zero or non-finite
 *    sigma_position, demodulate without albedo, zero width or height, NULL pointers. */
typedef struct { uint32_t iterations; float sigma_color, sigma_normal, sigma_position; uint32_t demodulate; uint32_t pad[3]; } mi_denoise_params;
/* the filter on host arrays (H x W x 3 each; albedo may be NULL when demodulate is 0); resolved_sigma_position may be NULL */
int mi_denoise_image(uint32_t device, uint32_t width, uint32_t height, const float *color, const float *normal, const float *position,
                     const float *albedo, const mi_denoise_params *p, float *out, float *resolved_sigma_position);
/* The filter on a render's own films, on the device: radiance = film layout 2, guides = the FIRST shNormal and the FIRST position entry of the render's field list,
 * albedo (demodulate) = its first albedo entry, each as layout 2 of the field film develops it -- the fields' `undefined` values included, as they stand.  A missing
 * field: MI_ERR_INVALID naming it (a film that holds an adaptive run has no field film and is refused by this rule).  The films are read, never written: rendering more
 * samples and filtering again is allowed.  Scratch (two colour buffers and the packed guides, 72 B per pixel) is allocated at the first call and freed with the render; a
 * request beyond MI355PT_POOL_LIMIT or the free device memory is MI_ERR_DEVICE naming it.  A render that never calls this launches, allocates and records nothing extra. */
int mi_render_denoise(mi_render *r, const mi_denoise_params *p, float *host_out /* H x W x 3 */, float *resolved_sigma_position);
int mi_render_denoise_device(mi_render *r, const mi_denoise_params *p, void *device_out, float *resolved_sigma_position);

/* -- denoiser, temporal stage: the accumulated colour of the previous frame is reprojected into the current one and blended with it in front of the filter levels
 *    (csrc/temporal.h, csrc/kernels_temporal.hip).  float32, one rounding per operation, in the order written: the result equals a sequential model bit for bit
 *    (tests/temporal_model.py).
 *    A history (mi_history) belongs to one device and one image size w x h.  It holds, per pixel, the accumulated colour a (3 floats, still demodulated), a count n
 *    (float; 0 = no history here), a normal Nh and a position Ph; the projection Mh of the frame that wrote it (12 floats); whether that frame was demodulated; and
 *    the number of frames accumulated since creation or reset.
 *    A projection M is rows X, Y, W of the world -> pixel map of the film: for a world point q, X = ((M[0] q.x + M[1] q.y) + M[2] q.z) + M[3], Y likewise from
 *    M[4..7], Wc likewise from M[8..11]; the centre of pixel (i, j) of the rendered window is at (X / Wc, Y / Wc) = (i + 0.5, j + 0.5).
 *    Inputs of one frame: C, N, P and optionally A as mi_denoise_image takes them; optionally Pprev (H x W x 3), the world position each pixel's surface point had in
 *    the previous frame (NULL: Pprev = P, static geometry); the frame's M; mi_denoise_params; mi_temporal_params.
 *      1. demodulation: rule 3 of mi_denoise_image, unchanged, gives c0 and D.
 *      2. tp, the temporal position tolerance: sigma_position > 0 gives that value; sigma_position < 0 gives |sigma_position| x the diagonal of the box of the finite
 *         pixels of the current P, exactly as rule 2 of mi_denoise_image resolves it; no finite pixel or a diagonal of 0: tp = 0.
 *      3. pixel p is "alone" when any component of c0(p), N(p), P(p) or Pprev(p) is non-finite, or when the history holds no frame: a(p) = c0(p), n(p) = 0 if
 *         non-finite, 1 otherwise.  Every other pixel:
 *         1. q = Pprev(p); X, Y, Wc from the history's Mh; !(Wc > 0): no history.
 *         2. fx = X / Wc - 0.5f, fy = Y / Wc - 0.5f; !(fx > -1 && fx < w && fy > -1 && fy < h): no history.
 *         3. x0 = floorf(fx), y0 = floorf(fy), tx = fx - x0, ty = fy - y0.
 *         4. taps (x0 + i, y0 + j), j outer, i inner over 0..1, weight b = (i ? tx : 1 - tx) (j ? ty : 1 - ty).  A tap counts when it lies inside the image, b > 0,
 *            the history count there is > 0, d2(q - Ph(tap)) <= tp tp, and (N(p).x Nh.x + N(p).y Nh.y) + N(p).z Nh.z >= min_normal_dot (a NaN fails each
 *            comparison).  Counted taps add sw += b, sn += b n(tap), s.k += b a(tap).k.
 *         5. sw > 0: hist = s / sw, nh = sn / sw, n' = min(nh + 1, max_history), alpha = 1 / n', a(p).k = hist.k + (c0(p).k - hist.k) alpha, n(p) = n'.
 *            Otherwise no history: a(p) = c0(p), n(p) = 1.
 *      4. the new history is (a, n, N, P) of every pixel with Mh := M; the stage reads the old history while it writes the new one (two buffer sets that ping-pong).
 *      5. filter: rule 4 of mi_denoise_image with c_0 := a, and rule 5 gives the output; iterations = 0 gives a x D (a without demodulation).
 *    The first frame of a history equals mi_denoise_image bit for bit (iterations >= 1); a moved surface whose displacement exceeds tp drops its history.
 *    Refused with MI_ERR_INVALID naming the cause: the checks of mi_denoise_image; max_history < 1 or non-finite; a zero or non-finite temporal sigma_position;
 *    min_normal_dot outside [-1, 1]; an image size or device other than the history's; a demodulate value that differs from the history's last frame (reset first);
 *    NULL M. */
typedef struct mi_history mi_history;
typedef struct { float max_history, sigma_position, min_normal_dot; uint32_t pad; } mi_temporal_params;
/* Two sets of history records (40 B per pixel each: float4 (a.r, a.g, a.b, n), float4 (N, P.x), float2 (P.y, P.z)) in one device allocation; a request beyond
 * MI355PT_POOL_LIMIT or the free device memory is MI_ERR_DEVICE naming it.  reset gives back the state after create (no frame; nothing is written to the device). */
int mi_history_create(uint32_t device, uint32_t width, uint32_t height, mi_history **out);
void mi_history_destroy(mi_history *h);
int mi_history_reset(mi_history *h);
int mi_history_frames(mi_history *h, uint32_t *frames);
/* the current records: color = H x W x 3, the accumulated colour, still demodulated; count = H x W.  Either may be NULL.  Without a frame: MI_ERR_INVALID */
int mi_history_read(mi_history *h, float *color, float *count);
/* one temporal frame on host arrays (albedo NULL when demodulate is 0, prev_position NULL for static geometry); the two resolved widths may be NULL */
int mi_denoise_image_temporal(mi_history *h, const float *color, const float *normal, const float *position, const float *albedo, const float *prev_position,
                              const float *world_to_pixel12, const mi_denoise_params *p, const mi_temporal_params *t, float *out,
                              float *resolved_sigma_position, float *resolved_temporal_position);
/* One temporal frame on a render's own films: radiance and guides as mi_render_denoise takes them, with the same field rules and refusals; Pprev = the FIRST prevPosition
 * entry of the render's field list as layout 2 of the field film develops it (the caller marks the scene before each frame's edit, mi_scene_mark_frame), without such a
 * field Pprev = P; M = the scene's current projection (mi_scene_world_to_pixel).  The history must be on the render's device and of its film size.  The films are read, never written. */
int mi_render_denoise_temporal(mi_render *r, mi_history *h, const mi_denoise_params *p, const mi_temporal_params *t, float *host_out /* H x W x 3 */,
                               float *resolved_sigma_position, float *resolved_temporal_position);
int mi_render_denoise_temporal_device(mi_render *r, mi_history *h, const mi_denoise_params *p, const mi_temporal_params *t, void *device_out,
                                      float *resolved_sigma_position, float *resolved_temporal_position);
/* The projection of a committed scene: rows 0, 1 and 3 of diag(width, height, 1, 1) x inverse(sample_to_camera) x inverse(to_world), computed in double from the camera
 * as it stands after the last mi_scene_update_camera and rounded to float once.  The sample space spans the rendered crop window; a thin lens projects through the
 * lens centre.  A singular camera matrix: MI_ERR_INVALID. */
int mi_scene_world_to_pixel(mi_scene *s, float *out12);
/* A process that never calls the functions of this section allocates and launches nothing extra. */

/* Debug / parity: what a shading stage recomputes for the sensor rays of individual (px, py, sampleIndex) triples from the path state in the queues, batched as
 * mi_render_samples (generate only): out8 = the path's aperture sample ((0.5, 0.5) without a lens), then the rx / ry directions scaled by 1 / sqrt(spp).  A parity hook, not a
 * product call.  Its kernel looks Sobol values up in the render's GLOBAL nibble tables from st0.y / st0.z, as k_env_primary does; the shade kernels call the same functions on
 * their LDS copy of the tables -- that path is checked through renders (tests/test_gpu_thinlens.py), not here. */
int mi_render_debug_sensor_differentials(mi_render *r, const uint32_t *pairs, uint64_t n, float *out8);
/* Debug / parity, film units: caller-supplied samples through the film kernels a render launches -- no kernel of its own.  Sample (plane s, tile pixel pl) sits at index
 * s x n_pix + pl, as the kernels index the queues; n_pix = the pixels of the tile's rows y0, y0 + row_stride, ... as mi_render_run_rows counts them; pos2 = the film
 * position (sx, sy), val4 = Li rgb, alpha.  Pool 0 is sized as a run sizes it, the arrays are copied into its position / accumulator queues, the batch descriptions come
 * from the code mi_render_run_rows uses, the launch goes to the render's stream and is waited for.  batch_planes = 0: one launch; k: consecutive launches of at most k planes.
 *   which = 0  k_film (mi_render_run_rows' film stage)
 *   which = 1  k_adapt_accumulate over the active list of the tile, with the set-up of mi_render_run_adaptive (buffers, zeroing, arguments from mi_render_set_adaptive and
 *              its GIVEN average_luminance > 0); needs a clear film, no fields, row_stride = 1 and n_planes = max_sample_factor x spp (every pixel stops by the last plane).
 *              No compaction between launches: every launch sees the full list, finished pixels return at once.  Afterwards the film and mi_render_read_sample_counts
 *              read as after an adaptive run
 *   which = 2  k_field_film with every hit record of the batch set to a miss: each sample puts the fields' `undefined` triples (val4 is not read); needs fields
 * MI_ERR_INVALID, by name: a null argument, a tile outside the film, n_planes = 0, a render running on the scene, a missing precondition of `which`, a position that is
 * not finite or beyond 2^20 in magnitude (the kernels' clamps make any finite position safe; the bound keeps the int conversions of a CPU model defined). */
int mi_render_debug_film_put(mi_render *r, int which, mi_tile tile, uint32_t row_stride, uint32_t n_planes, uint32_t batch_planes, const float *pos2, const float *val4);
int mi_render_set_profiling(mi_render *r, int enabled);   /* per-stage HIP-event timing: events are recorded between the stage launches of the first stream, nothing is serialised (off by default) */

/* bool Scene::rayIntersect(const Ray &ray, Intersection &its) for a batch of rays (include/mitsuba/render/scene.h:187-243): rays8 = (o.xyz, mint, d.xyz, maxt) per
 * ray, host pointers; the scene must be committed.  Record = the fields of mitsuba::Intersection the path consumes (include/mitsuba/render/shape.h:36-170). */
typedef struct {
    uint32_t valid;                      /* 0: no intersection in [mint, maxt]; the other fields are then unset */
    float t, p[3], ng[3];                /* its.t, its.p, its.geoFrame.n */
    float ns[3], s[3], tt[3];            /* its.shFrame.n / .s / .t */
    float uv[2], wi[3], bary[2];         /* its.uv, its.wi (local), the barycentrics (u, v) of a triangle hit / the shape's temp data */
    uint32_t prim; int32_t instance;     /* global primitive index (triangles first, then analytic shapes); instance index or -1 */
    int32_t material, emitter;           /* material / emitter table index (its.shape->getBSDF() / getEmitter()), -1: none */
} mi_intersection;
int mi_scene_ray_intersect(mi_scene *s, const float *rays8, uint64_t n, mi_intersection *out);

/* Unit-level device entry points used by the parity tests (each runs a small kernel over n items) */
int mi_debug_intersect(mi_scene *s, const float *rays8, uint64_t n, int any_hit, float *out_hits4);   /* t,u,v,prim (prim<0: miss) */
int mi_debug_intersect_inst(mi_scene *s, const float *rays8, uint64_t n, int any_hit, float *out_hits4, int32_t *out_instance);   /* + instance index of the hit (-1: scene-level primitive) */
/* The fused tree walk (the ray cast of large triangle-only scenes) on caller-supplied rays, through the stage the renderer launches.  The n rays are laid, in order,
 * into n_seg queue segments of seg_counts[i] rays each (counts add up to n; empty segments allowed); thr = refill threshold (1..64 busy lanes), grid = persistent
 * workgroups (1..16384), lds_stack = stack entries per lane kept in LDS (4 or 10; deeper entries spill to memory).
 * any_hit = 0: out_hits4 = (t, u, v, prim as its bit pattern; 0xFFFFFFFF: miss); a record still holding 0xFFFFFFFE in all four words belongs to a ray the walk never
 *              retired.  rays_counted = what the launch added to the closest-hit ray counter.
 * any_hit = 1: out_hits4 = the accumulator of ray i after `+= (1, 0, 0)` for every unoccluded trace of it: x = 0 occluded, 1 unoccluded, 2 traced twice.  Shadow
 *              records carry no mint: every ray's mint must be 1e-4.
 * Scenes with analytic shapes or instances and scenes traced as a triangle packet have no such walk: MI_ERR_UNSUPPORTED (decided before any device work). */
typedef struct { uint32_t wide, bvh_depth, bvh_stack_direct, max_stack_seen; uint64_t rays_counted; } mi_fused_debug_info;   /* node kind (1: 4-wide), the builder's stack bounds, deepest stack any ray of this call held */
int mi_debug_intersect_fused(mi_scene *s, const float *rays8, uint64_t n, int any_hit, const uint32_t *seg_counts, uint32_t n_seg, uint32_t thr, uint32_t grid, uint32_t lds_stack,
                             float *out_hits4, mi_fused_debug_info *info);
/* One device table of a committed scene as it is now, read back whole: what = MI_GEOMETRY_NODES (64-B tree nodes), _LEAF_RECORDS (48-B Wald records in leaf order,
 * word 10 = primitive index), _TRI_SHADE (128-B shading records, triangle order), _TRI_UV (48 B, only scenes with texture coordinates), _PACKET_EXACT (48-B Wald records,
 * triangle order), _PACKET_GROUPS (48-B pass-1 records), _INSTANCES (128-B instance records in instance order: to_world 3 x 4, to_object 3 x 4, group box lo, root node,
 * group box hi, group; size 0 on a scene without instances), _SCENE_BOX (24 B: aabb_lo, then aabb_hi of the scene record the kernels receive), _PREV_VERTICES (12 B per vertex of mi_scene_set_triangles: the
 * positions at the last mi_scene_mark_frame), _PREV_INSTANCES (48 B per instance: rows 0..2 of its to_world at the last mark); the last two have size 0 on a scene that was never marked.  The caller gives the size in bytes (mi_debug_geometry_bytes); a wrong size is MI_ERR_INVALID. */
#define MI_GEOMETRY_NODES 0
#define MI_GEOMETRY_LEAF_RECORDS 1
#define MI_GEOMETRY_TRI_SHADE 2
#define MI_GEOMETRY_TRI_UV 3
#define MI_GEOMETRY_PACKET_EXACT 4
#define MI_GEOMETRY_PACKET_GROUPS 5
#define MI_GEOMETRY_INSTANCES 6
#define MI_GEOMETRY_SCENE_BOX 7
#define MI_GEOMETRY_PREV_VERTICES 8
#define MI_GEOMETRY_PREV_INSTANCES 9
int mi_debug_geometry_bytes(mi_scene *s, uint32_t what, uint64_t *bytes);
int mi_debug_read_geometry(mi_scene *s, uint32_t what, void *out, uint64_t bytes);
int mi_debug_sobol(mi_scene *s, const uint32_t *px_py_k, uint64_t n, uint32_t ndims, uint64_t *out_index, float *out_values);
int mi_debug_camera_rays(mi_scene *s, const float *sample_pos2, uint64_t n, float *out_rays8);   /* on a lens scene: the aperture sample (0.5, 0.5), the reference's default when none is drawn */
/* The sensor ray with its differentials, unscaled (RayDifferential::scaleDifferential not applied): out14 = origin, mint, direction, maxt, rx direction, ry direction per
 * ray; aperture2 = the aperture sample of every ray, ignored (may be NULL) on a scene without a lens, which returns mi_debug_camera_rays' ray + the perspective differentials */
int mi_debug_camera_rays_lens(mi_scene *s, const float *sample_pos2, const float *aperture2, uint64_t n, float *out14);
int mi_debug_libm(int fn, const float *x, const float *y, uint64_t n, float *out);   /* the device restatements of glibc's routines (libm_glibc.h) as the kernels call them:
                                      fn 0 expf(x), 1 logf(x), 2 powf(x, y), 3 tanf(x), 4 atanf(x), 5 atan2f(x, y), 6 acosf(x); y may be NULL for the one-argument routines */
/* The BSDF routines one call at a time.  Record `material` is resolved as the shade stage resolves the material of an untextured hit (a coating / roughcoating record with
 * its nested record) and queried through the widest instantiation of the stage's own sample / eval / pdf functions (every BSDF type and wrapper, tables in global memory).
 * mode 0 = BSDF::sample(bRec, pdf, sample): wi3, uv2 = the 2-D sample, extra1 = the value handed out if the sampled BSDF asks its sampler for one more (BSDF::EUsesSampler);
 *          wo3 is ignored (may be NULL); out11 = weight rgb, pdf, wo xyz, eta, sampled component is a Dirac delta (0 / 1), is ENull (0 / 1), extra value drawn (0 / 1).
 * mode 1 = BSDF::eval + BSDF::pdf (all components, solid angle): wi3, wo3; uv2 / extra1 are ignored (may be NULL); out4 = value rgb, pdf.
 * Records whose evaluation needs a hit record are refused by name with MI_ERR_UNSUPPORTED: mask (its logic is inline in the shade stage), bumpmap, normalmap, a record with
 * a bound texture, and a coating / mixturebsdf / blendbsdf over one of them. */
int mi_debug_bsdf(mi_scene *s, uint32_t material, int mode, const float *wi3, const float *wo3, const float *uv2, const float *extra1, uint64_t n, float *out);
/* The surface step between a hit and the BSDF query, one caller-supplied hit per case: picking its.dpdu / its.dpdv, Intersection::computePartials and the filtered lookup,
 * the perturbed frame of a bumpmap / normalmap, and the unwrap mask -> bumpmap / normalmap -> coating with the textured parameters loaded into the nested records -- the
 * routines the shade stages call, in their order, through the widest instantiation (texcoords, analytic shapes, instances, tables in global memory).
 * rays8 = o, mint, d, maxt; hits4 / instance1 = t, u, v, prim and the instance index exactly as mi_debug_intersect_inst returns them (instance1 may be NULL: none; prim < 0:
 * a miss, whose outputs are all zero); diff6 = the two differential directions rxd, ryd (common origin o) of a camera ray, NULL = a later bounce: level-0 lookups, no partials.
 * mode 0 (record), out51 = its.uv as the lookups use it (an analytic shape's own parameterisation) 2, dpdu 3, dpdv 3, dudx dvdx dudy dvdy (zero without differentials),
 *          opacity 3 (zero without a mask), the value loaded into the first textured parameter on the chain 3 (zero: none), masked (0 / 1), bumped (0 / 1), coating record
 *          (-1: none), leaf record, the leaf's `reflectance` after its texture was applied 3, perturbed frame s 3, t 3, n 3 (zero when not bumped), wi in the frame the query
 *          uses 3, then the hit as given: t, u, v, prim, instance, and its shading frame n 3, s 3, t 3.
 * mode 1 (sample), query3 = the 2-D sample and the extra sampler value: out11 as mi_debug_bsdf's mode 0 on the resolved (coating, leaf) with that wi; wo in query-frame
 *          coordinates; the values are those before the mask's lobe choice, the opacity multiply and the sign rejection of a perturbed frame.
 * mode 2 (eval + pdf), query3 = a WORLD direction, taken into the query frame by the same routines: out4 as mi_debug_bsdf's mode 1.
 * A NULL pointer, n == 0, a mode outside 0..2, modes 1 / 2 without query3, or a hit that names a primitive or instance the scene does not have: MI_ERR_INVALID. */
int mi_debug_surface(mi_scene *s, int mode, const float *rays8, const float *hits4, const int32_t *instance1, const float *diff6, const float *query3, uint64_t n, float *out);
/* The texture routines one call at a time: record `texture` of mi_scene_set_textures at uv2.  Bitmaps: scale and offset as the shade stage applies them; partials4 = (dudx,
 * dvdx, dudy, dvdy) per lookup selects the filtered lookup of a camera hit (TMIPMap::eval under the record's filter), NULL the level-0 lookup of every later bounce
 * (bilinear, or the nearest texel under the nearest filter).  Procedural textures ignore the partials.  The EWA loops run over the footprint's bounding box: the caller
 * keeps footprints bounded. */
int mi_debug_texture(mi_scene *s, uint32_t texture, const float *uv2, const float *partials4, uint64_t n, float *out3);
/* Scene::sampleEmitterDirect one call at a time, through the widest instantiation the stages have (every emitter kind, analytic shapes, tables in global memory): ref3 =
 * the reference point, refN3 = its normal ((0, 0, 0): a two-sided or medium vertex), uv2 = the 2-D sample.  raw = 1 is the volumetric integrators' form
 * (Scene::sampleAttenuatedEmitterDirect): the value is not yet divided by the emitter-selection probability, which comes back as em_pdf.  No visibility test is made
 * (the shadow queue does that).  out17 = value rgb, p xyz, d xyz, dist, pdf, n xyz, emitter index, !isOnSurface (0 / 1), em_pdf (raw only, else 0); the record starts
 * out zero, and where the returned pdf is 0 everything but value and pdf is whatever the routine left there.  A scene without emitters: MI_ERR_INVALID. */
int mi_debug_emitter_sample(mi_scene *s, const float *ref3, const float *refN3, const float *uv2, uint64_t n, int raw, float *out17);
/* What a BSDF-sampled ray that finds emitter `emitter` evaluates: the ray left ref3 in direction d3 and met the emitter after dist1 at a point with shading normal n3;
 * facing1 (0 / 1) = dot(d, refN) >= 0, evaluated where the reference normal was still known.  out8 =
 *   area light:  Emitter::eval(n, -d) rgb, Scene::pdfEmitterDirect, 0 0 0 0
 *   envmap:      evalEnvironment(d) rgb, EnvironmentMap::pdfDirect's solid-angle density, then the value rgb and density of the fused routine the shade stage calls
 *                for both at once (ref, n, dist, facing are ignored)
 *   constant:    evalEnvironment rgb, 0 0 0 0 0 (its density is one line inside the shade stage)
 * A point, spot, directional or collimated emitter is refused by name (MI_ERR_UNSUPPORTED: no ray finds one); an index out of range is MI_ERR_INVALID. */
int mi_debug_emitter_eval(mi_scene *s, uint32_t emitter, const float *ref3, const float *d3, const float *n3, const float *dist1, const float *facing1, uint64_t n, float *out8);
/* The medium routines of the volumetric stages one call at a time, on record `medium` of mi_scene_set_media.  in10 / out12 per case:
 *   mode 0  HomogeneousMedium::evalTransmittance over [mint, maxt]: in[6], in[7] (the rest ignored) -> transmittance rgb
 *   mode 1  HomogeneousMedium::sampleDistance: o xyz, d xyz, mint, maxt, and the two values its sampler hands out (the second is drawn only by the balance strategy when the
 *           medium is chosen) -> success (0 / 1), t, p xyz, transmittance rgb, pdfSuccess, pdfFailure, values drawn; t and p start out zero
 *   mode 2  PhaseFunction::sample, then eval of its own result: wi xyz, the 2-D sample -> wo xyz, eval
 *   mode 3  PhaseFunction::eval: wi xyz, wo xyz -> eval
 * the rest of out12 is 0.  A medium index out of range or a mode outside 0..3: MI_ERR_INVALID. */
int mi_debug_medium(mi_scene *s, uint32_t medium, int mode, const float *in10, uint64_t n, float *out12);
int mi_debug_sincosf(const float *x, uint64_t n, float *out_sin_cos2);   /* the device restatement of glibc's sincosf (warps): out[2i] = sin, out[2i+1] = cos */
/* The shape of a path pool.  A pool of `paths` paths is cut into n_seg segments of cap slots (cap a multiple of 64; segment s holds the paths s * cap ..); the shade stages
 * give every segment to one wave, which walks it in chunks of 64.  The rule, a pure host function (no device, no environment): n_seg = the override, else 16384, or -- on a
 * scene with rough conductors -- paths / 1024 kept within [16384, 2^18]; never more than ceil(paths / 64) segments (and never fewer than one); the volumetric integrators
 * keep a segment at <= 65472 slots (their stages pack two per-segment record counts into 16 bits each) by raising n_seg to ceil(paths / 65472); cap = ceil(paths / n_seg)
 * rounded up to a multiple of 64; the three stage grids = min(n_seg, override or the default 4096 / 768 (512 with rough conductors) / 4096).  An override of 0 means unset
 * (so do MI355PT_SEGMENTS and MI355PT_GRID_EXTEND / _SHADE / _SHADOW when they are 0, negative or no number).  A pool of 2^28 slots or more is refused: MI_ERR_INVALID. */
typedef struct { uint32_t segments, grid_extend, grid_shade, grid_shadow; } mi_pool_overrides;
typedef struct { uint32_t n_seg, cap, grid_extend, grid_shade, grid_shadow; } mi_pool_shape;
int mi_debug_pool_shape(uint64_t paths, int has_roughconductor, uint32_t integrator, const mi_pool_overrides *overrides /* NULL: none */, mi_pool_shape *out);
/* The pools of a render as they are now.  Known from mi_render_create on: n_pools = the pools / streams the render owns (MI355PT_STREAMS; a job of fewer batches uses
 * fewer of them: 3 batches on a render of 4 pools run on 3), lds_tables = this render stages the scene tables in LDS, has_roughconductor / integrator = what the rule above
 * is given.  Zero until the first run / samples call allocates the pools: n_seg, cap, the three stage grids and pool_paths (a pool only grows, so a smaller job reports
 * the shape it runs in).  Of the last launch of the path integrator's shade stage (zero before it, and for the volumetric integrators): shade_table_bytes = the dynamic
 * LDS it asked for in front of the order list (Sobol tables, scene tables), sorted = it read its segments through the class-sorted order list, which takes a scene with
 * rough conductors, cap <= 8192 and shade_table_bytes rounded up to 16 + 8 * cap + 16 <= 65536. */
typedef struct { uint32_t n_seg, cap, n_pools, grid_extend, grid_shade, grid_shadow, lds_tables, sorted, has_roughconductor, integrator, shade_table_bytes, pad; uint64_t pool_paths; } mi_pool_info;
int mi_render_debug_pool_info(mi_render *r, mi_pool_info *out);

#ifdef __cplusplus
}
#endif
#endif
