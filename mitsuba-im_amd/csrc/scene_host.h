// scene_host.h -- host-side scene object behind the mi_scene handle.
#pragma once
#include "../../include/mi355pt.h"
#include "pt_types.h"
#include <string>
#include <vector>

namespace mi {

struct GeoEditTables; struct InstEditTables;      // geometry_records.h
enum class GeoEntry { Vertices, Instances, Geometry };      // which of mi_scene_update_vertices / _instances / _geometry an edit came in through
inline const char *geoEntryName(GeoEntry e) { return e == GeoEntry::Vertices ? "mi_scene_update_vertices" : e == GeoEntry::Instances ? "mi_scene_update_instances" : "mi_scene_update_geometry"; }

struct SceneHost {
    // inputs (mi_scene_set_*)
    std::vector<float> pos, nrm, uv; std::vector<uint32_t> idx; std::vector<mi_shape> shapes;
    std::vector<mi_material> materials; std::vector<mi_emitter> emitters; std::vector<mi_analytic> analytic; std::vector<mi_instance> instances; std::vector<float> materialTables; std::vector<mi_texture> textures; std::vector<uint32_t> texLevels; std::vector<float> texTexels; int32_t envTexture = -1;
    std::vector<mi_medium> media; std::vector<int32_t> shapeMedia; int32_t sensorMedium = -1;   // mi_scene_set_media
    std::vector<uint16_t> envGuideRows, envGuideCols; uint32_t envGuideKR = 0, envGuideKC = 0; void *dEnvGuideRows = nullptr, *dEnvGuideCols = nullptr;
    std::vector<MediumD> mediaD; std::vector<uint32_t> primMedia;   // derived: device records; per primitive (interior + 1) | (exterior + 1) << 16
    void *dMedia = nullptr, *dPrimMedia = nullptr;
    float s2c[16] = {0}, c2w[16] = {0}; float nearClip = 0, farClip = 0; bool haveCamera = false;
    float lensRadius = 0, focusDistance = 0;   // mi_scene_set_lens: thin lens (src/sensors/thinlens.cpp); radius 0 = none
    uint32_t width = 0, height = 0, filterKind = 0; float filterRadius = 0.5f, filterStddev = 0.5f; bool haveFilm = false;
    std::vector<float> envRGB; uint32_t envW = 0, envH = 0; float envToWorld[16] = {0}, envScale = 1.0f;
    // derived on the host (scene_build.cpp)
    std::vector<uint32_t> triShape, i2; std::vector<TriAccelD> tris; std::vector<TriShade> shade; std::vector<BvhNode> nodes;
    std::vector<TriUV> triuv; bool anyUV = false;   // per-triangle uv + UV tangents (only when some mesh has texcoords)
    bool wideBvh = true;   // 4-wide quantised nodes (default) or the binary tree (MI355PT_BVH2=1)
    std::vector<InstanceD> instancesD; int bvhStackDirect = 0;   // stack entries of the fused walk (trace_fused.h: child codes pushed one by one), scene-level tree
    int bvhDepth = 0;   // stack entries the traversal needs (scene tree + return marker + deepest group tree)
    std::vector<AnalyticD> analyticD; uint32_t nTris = 0;   // analytic shapes: primitive index nTris + i; `tris` (BVH leaf order) holds a k = MI_K_ANALYTIC record for each
    std::vector<TriAccelD> packetExact;   // Wald records in ORIGINAL triangle order (packet mode, <= MI_PACKET_MAX triangles): pass 2 of trace.h
    std::vector<PacketGroupD> packetGroups; uint32_t packetGK[3] = {0, 0, 0}; float packetScale = 1.0f;   // pass-1 records sorted by projection axis
    std::vector<EmitterD> emittersD; std::vector<float> emitterCdf, areaCdf, emitterX; float emitterNorm = 0;
    bool envConstant = false, hasDeltaEmitters = false; float dirBsCenter[3] = {0, 0, 0}, dirBsRadius = 0;
    float aabbLo[3], aabbHi[3];
    float filterValues[MI_FILTER_RES + 1]; float filterRadiusEff = 0, filterScale = 0; int border = 0;
    float resolution = 1; uint32_t logRes = 0;
    int envIndex = -1; std::vector<float> envCdfCols, envCdfRows, envRowWeights; float envNormalization = 0, envToWorld3[9], envToLocal3[9], envBsCenter[3], envBsRadius = 0;
    // device
    bool committed = false; int device = 0;
    void *dNodes = nullptr, *dTris = nullptr, *dShade = nullptr, *dI2 = nullptr, *dNrm = nullptr, *dMaterials = nullptr, *dEmitters = nullptr,
         *dEmitterCdf = nullptr, *dAnalytic = nullptr, *dInstances = nullptr, *dMaterialTables = nullptr, *dTriUV = nullptr, *dTextures = nullptr, *dTexLevels = nullptr, *dTexTexels = nullptr, *dMipLut = nullptr, *dEmitterX = nullptr, *dAreaCdf = nullptr, *dFilter = nullptr, *dEnvRGB = nullptr, *dEnvCols = nullptr, *dEnvRows = nullptr, *dEnvWeights = nullptr, *dPacketGroups = nullptr, *dPacketExact = nullptr, *dSobolM32 = nullptr, *dSobolVdc = nullptr, *dSobolVdcInv = nullptr;
    DScene d{};
    // derived from the materials alone (scene_build.cpp): the records the device reads (MaterialD with the sampling weights the reference's configure() computes) and,
    // per material, the three flag bits of TriShade::flags / AnalyticD::flags (MI_MATERIAL_FLAG_BITS) of every primitive that uses it
    std::vector<MaterialD> materialsD; std::vector<uint32_t> materialFlagTable; void *dMaterialFlags = nullptr;
    // in-place edits of a committed scene (mi_scene_update_*): `revision` counts them, `treeBuilds` counts commitHost() runs -- an edit never moves it
    uint64_t revision = 0, treeBuilds = 0;

    void commitHost();          // scene_build.cpp
    int upload(int device);     // api.cpp
    void release();
    // pieces of commitHost() / upload() that an edit repeats (scene_build.cpp; no device calls)
    uint32_t materialFlagBits(uint32_t bsdf) const;
    void buildMaterialTables();         // materialsD + materialFlagTable
    void buildEmitterTables();          // emittersD, emitterCdf, emitterNorm, emitterX, areaCdf, hasDeltaEmitters, envIndex, envConstant
    void buildBoundingSpheres();        // dirBs*, envBs* (the latter includes the sensor position)
    void buildEnvTransform();           // envToWorld3, envToLocal3
    void buildSceneBox(const float *extraBoxes, uint32_t n);   // aabbLo / aabbHi from the vertices, the analytic shapes and n further boxes (lo, hi: the instances)
    void buildPacketTables();           // packetScale, packetGroups, packetGK
    void syncCameraD();                 // d.s2c, d.c2w, clip planes, cam_dx / cam_dy, lens radius / focus distance, env bounding sphere
    void syncEmittersD();               // d.emitter_norm
    void syncEnvD();                    // d.env_to_world, d.env_to_local, d.env_scale
    // The edits.  Each returns MI_OK or an error code with `msg` set and then leaves the scene as it was; on success the host tables above and `d` are those of a
    // fresh commit with the new inputs, `revision` has advanced, and the caller re-sends the small device tables (api.cpp).
    int updateCamera(const float *s2c16, const float *c2w16, float nearClip, float farClip, std::string &msg);
    int updateLens(float apertureRadius, float focusDistance, std::string &msg);      // values only: a lens appearing or vanishing changes every path's sample layout
    int updateMaterials(const mi_material *m, uint32_t n, std::string &msg, bool *flagsChanged);
    int updateEmitters(const mi_emitter *e, uint32_t n, std::string &msg);
    int updateEnvmapTransform(const float *toWorld16, float scale, std::string &msg);
    // Geometry edits: one frame of an animation -- new positions (and normals) for the whole vertex array, shape-group members included, and / or new to_world /
    // to_object for every committed instance (the groups stay).  Replaces pos / nrm / instances, the group boxes, the scene box and the small tables at once; the
    // per-triangle mirrors (tris, shade, triuv, packetExact), instancesD (glo / ghi included) and `nodes` -- scene level AND group trees -- become STALE: the device
    // recomputes its copies (kernels_geometry.hip) and refreshHostGeometry() repeats its steps on the mirrors with the same arithmetic (geometry_records.h) before
    // anything reads them.  Keeping them current eagerly would put the per-triangle host loop back into every edit.
    // One check and one apply serve the three entry points; `entry` names the caller in every message and turns on the two refusals only mi_scene_update_vertices makes
    // (a scene with instances, a shape that is a group member).
    int updateVertices(const float *pos, const float *nrm, uint32_t nVerts, std::string &msg);      // = checkGeometry as GeoEntry::Vertices, then applyGeometry
    int updateInstances(const mi_instance *in, uint32_t n, std::string &msg);                        // ... as GeoEntry::Instances ...
    int updateGeometry(const float *pos, const float *nrm, uint32_t nVerts, const mi_instance *in, uint32_t nInstances, std::string &msg);      // ... as GeoEntry::Geometry ...
    int checkGeometry(GeoEntry entry, const float *pos, const float *nrm, uint32_t nVerts, const mi_instance *in, uint32_t nInstances, std::string &msg) const;   // every refusal; changes nothing
    void applyGeometry(const float *pos, const float *nrm, uint32_t nVerts, const mi_instance *in, uint32_t nInstances);      // checked arguments only; a null part stays, and so does what is derived from it alone
    // The argument records of the three edit steps (geometry_records.h) over the device tables or over the host mirrors: the device chain (api.cpp) and
    // refreshHostGeometry() run the same steps on the same layout.  xf = the packed transform pairs where the step reads them.
    GeoEditTables geoEditTables(bool onDevice);
    InstEditTables instEditTables(bool onDevice, const float *xf, bool withGroupBoxes);
    std::vector<float> instanceTransformPairs() const;      // 24 floats per instance: rows 0..2 of to_world, then of to_object
    void buildGroupBoxes();             // groupBoxes: per shape group the union of its member shapes' vertices in shape order, enlarged like a kd-tree root (commitHost() and the geometry edit)
    std::vector<float> groupBoxes;      // 6 floats (lo, hi) per shape group
    std::vector<int> groupRoot;         // root node of every group's tree in `nodes`
    void prepareGeometryEdit();         // first edit: leafSlotOfPrim / leafSlotOfInstance, leafBoxes of the records that do not move, refitOrder / refitLevelStart (scene level), refitOrderAll / refitLevelStartAll (+ the group trees)
    void refreshHostGeometry();
    std::vector<uint32_t> leafSlotOfInstance;   // instance -> its MI_K_INSTANCE record in `tris`
    std::vector<uint32_t> leafSlotOfPrim, refitOrder, refitLevelStart;   // triangle -> its record in `tris`; node indices sorted by height (0 = all children are leaves), level l = refitOrder[refitLevelStart[l] .. refitLevelStart[l + 1])
    std::vector<uint32_t> refitOrderAll, refitLevelStartAll;   // the same over the scene-level tree and every group tree: nodes of equal height share a level, no tree reads another tree's nodes
    std::vector<float> leafBoxes, nodeBoxes;   // padded box (lo, hi) per leaf record; exact union of the child boxes per node (a group tree's: valid after its first refit only)
    bool geoPrepared = false, geoStale = false, instStale = false;
    // device side of the geometry edits, each table allocated by the first edit that needs it (api.cpp): the vertex array, leafSlotOfPrim, the leaf and node boxes,
    // refitOrder, refitOrderAll, the group boxes of the current edit, the 24-float transform pairs, leafSlotOfInstance
    void *dPos = nullptr, *dLeafSlot = nullptr, *dLeafBox = nullptr, *dNodeBox = nullptr, *dRefitOrder = nullptr, *dRefitOrderAll = nullptr, *dGroupBox = nullptr, *dInstXf = nullptr, *dLeafSlotInst = nullptr;
    // Frame mark (mi_scene_mark_frame, api.cpp): the "previous" state of the prevPosition / motion fields.  The host keeps the snapshot (a replica uploads it from
    // here); the two device tables are allocated by the first mark.  A commit clears the mark: previous = current again.
    bool marked = false; std::vector<float> prevPos, prevInstXf;      // the vertex array; rows 0..2 of every instance's to_world (12 floats each)
    float prevW2P[12] = {0}, prevOrigin[3] = {0, 0, 0};                   // mi_scene_world_to_pixel's rows and the camera origin at the mark
    void *dPrevPos = nullptr, *dPrevInst = nullptr;
    int allocMark();                    // api.cpp: the two device tables, each allocated when missing (sizes follow pos / instances, which no edit changes); 0 = ok
    int uploadMark();                   // api.cpp: allocMark(), then the host snapshot into them (a replica's upload); 0 = ok
    // Every device allocation the scene owns, listed here and nowhere else: release() frees and clears each, mi_scene_clone clears those of the copy it is about to upload.
    template <typename F> void eachDevicePointer(F f) {
        void **ps[] = {&dPrevPos, &dPrevInst, &dRefitOrderAll, &dGroupBox, &dPos, &dLeafSlot, &dLeafBox, &dNodeBox, &dRefitOrder, &dInstXf, &dLeafSlotInst, &dMaterialFlags, &dMedia, &dPrimMedia, &dPacketGroups, &dPacketExact, &dTexLevels, &dTexTexels, &dMipLut, &dTriUV, &dTextures, &dMaterialTables, &dInstances, &dEmitterX, &dAnalytic, &dNodes, &dTris, &dShade, &dI2, &dNrm, &dMaterials, &dEmitters, &dEmitterCdf, &dAreaCdf, &dFilter, &dSobolM32, &dSobolVdc, &dSobolVdcInv, &dEnvRGB, &dEnvCols, &dEnvRows, &dEnvWeights, &dEnvGuideRows, &dEnvGuideCols};
        for (void **p : ps) f(*p);
    }
    ~SceneHost() { release(); }
};

#define MI_MATERIAL_FLAG_BITS 14u       // bit1 back side, bit2 no smooth component, bit3 not a plain diffuse record
// value checks of mi_scene_set_materials / mi_scene_set_emitters, shared with the in-place updates (scene_build.cpp)
int validateMaterials(const mi_material *m, uint32_t n, std::string &msg);
int validateEmitters(const mi_emitter *e, uint32_t n, std::string &msg);
// value checks of mi_scene_set_lens / mi_scene_update_lens; `who` starts the message
int validateLens(const char *who, float apertureRadius, float focusDistance, std::string &msg);

}  // namespace mi
