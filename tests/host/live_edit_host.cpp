// live_edit_host.cpp -- stand-alone check of the host side of the in-place scene edits (SceneHost::update*, mitsuba-im_amd/csrc/scene_build.cpp).
// Built and run by tests/test_live_edit.py with the address and undefined-behaviour sanitizers; links scene_build.cpp only and makes no device call.
//
// A small scene is built in code -- two meshes, a shape group with one member mesh and one instance, an analytic sphere, four emitters of different kinds (area, envmap,
// point, spot) -- and committed on the host.  Each edit kind is applied through the functions the C-ABI uses; every derived host table must then equal, byte for byte,
// that of a second scene committed from scratch with the edited inputs, without a further tree build.  Then every refusal of "values only", one case per rule.
#include "../../mitsuba-im_amd/csrc/scene_host.h"
#include <cmath>
#include <cstdio>
#include <cstring>

namespace mi { void SceneHost::release() {} }      // no device tables here
using mi::SceneHost;

static int g_failed = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, what); ++g_failed; } } while (0)

static mi_material mat(uint32_t type, uint32_t flags = 0, uint32_t distr = 0, float alpha = 0.1f, float r = 0.5f, float e0 = 0, float e1 = 0, float k0 = 0, float k1 = 0, float k2 = 0) {
    mi_material m{}; m.type = type; m.flags = flags; m.distr = distr; m.alpha = alpha;
    m.reflectance[0] = r; m.reflectance[1] = r * 0.5f; m.reflectance[2] = r * 0.25f; m.eta[0] = e0; m.eta[1] = e1; m.k[0] = k0; m.k[1] = k1; m.k[2] = k2;
    m.specular[0] = m.specular[1] = m.specular[2] = 1.0f; return m;
}
static void identity(float *m) { std::memset(m, 0, 64); m[0] = m[5] = m[10] = m[15] = 1.0f; }

struct Inputs {
    std::vector<mi_material> materials; std::vector<mi_emitter> emitters;
    float s2c[16], c2w[16], nearClip = 0.1f, farClip = 100.0f, envToWorld[16], envScale = 1.0f;
};
static Inputs baseInputs() {
    Inputs in;
    in.materials = {
        mat(MI_BSDF_DIFFUSE, 0, 0, 0.1f, 0.6f),                                  // 0: floor
        mat(MI_BSDF_DIFFUSE, 0, 0, 0.1f, 0.4f),                                  // 1: light quad
        mat(MI_BSDF_DIFFUSE, 0, 0, 0.1f, 0.3f),                                  // 2: the group's member mesh
        mat(MI_BSDF_ROUGHCONDUCTOR, MI_BSDF_FLAG_SAMPLE_VISIBLE, 1, 0.2f, 0.0f, 0.2f, 0.0f, 3.0f),   // 3: the sphere
        mat(MI_BSDF_PLASTIC, 0, 0, 0.1f, 0.5f, 1.5f, 0, 0.04f),                  // 4: derived eta[1]
        mat(MI_BSDF_COATING, 0, 1, 0.7f, 0.2f, 1.5f),                            // 5: over record 1; derived k[0]
        mat(MI_BSDF_MIXTURE, 0, 2, 0.0f, 0.0f),                                  // 6: children 0 and 1 (set below)
        mat(MI_BSDF_BLEND, 0, 0, 0.0f, 0.5f, 0.0f, 1.0f),                        // 7: children 0 and 1 in eta[0], eta[1]
        mat(MI_BSDF_ROUGHPLASTIC, 0, 0, 0.1f, 0.5f, 1.5f, 0, 0.4f, 0.0f, 4.0f),  // 8: slice offset 0, length 4
    };
    in.materials[6].reflectance[0] = 0.0f; in.materials[6].reflectance[1] = 1.0f; in.materials[6].reflectance[2] = 0.0f; in.materials[6].k[0] = 0.5f; in.materials[6].k[1] = 0.5f;
    in.emitters.resize(4);
    for (mi_emitter &e : in.emitters) { e = mi_emitter{}; e.shape = -1; e.weight = 1.0f; e.radiance[0] = 1; e.radiance[1] = 2; e.radiance[2] = 3; identity(e.to_world); e.cutoff = 20; e.beam = 15; }
    in.emitters[0].type = MI_EMITTER_AREA; in.emitters[0].shape = 1;
    in.emitters[1].type = MI_EMITTER_ENVMAP;
    in.emitters[2].type = MI_EMITTER_POINT; in.emitters[2].to_world[3] = 0.5f; in.emitters[2].to_world[7] = 1.5f; in.emitters[2].to_world[11] = -0.5f;
    in.emitters[3].type = MI_EMITTER_SPOT; in.emitters[3].to_world[3] = -1.0f; in.emitters[3].to_world[7] = 1.8f; in.emitters[3].weight = 2.0f;
    identity(in.s2c); in.s2c[0] = 0.8f; in.s2c[5] = 0.6f; in.s2c[3] = -0.4f; in.s2c[7] = -0.3f; in.s2c[11] = 1.0f;
    identity(in.c2w); in.c2w[3] = 0.2f; in.c2w[7] = 1.0f; in.c2w[11] = -1.5f;
    identity(in.envToWorld);
    return in;
}
// the geometry never changes: floor, light quad, one member triangle pair of group 0 placed once, a sphere
static void fill(SceneHost &h, const Inputs &in) {
    const float P[][3] = {{2, 0, -2}, {-2, 0, -2}, {-2, 0, 2}, {2, 0, 2},   {0.5f, 2, -0.5f}, {0.5f, 2, 0.5f}, {-0.5f, 2, 0.5f}, {-0.5f, 2, -0.5f},
                          {0, 0, 0}, {0.3f, 0, 0}, {0.3f, 0.4f, 0}, {0, 0.4f, 0.1f}};
    const uint32_t I[][3] = {{0, 1, 2}, {0, 2, 3}, {4, 5, 6}, {4, 6, 7}, {8, 9, 10}, {8, 10, 11}};
    for (auto &p : P) h.pos.insert(h.pos.end(), p, p + 3);
    for (auto &t : I) h.idx.insert(h.idx.end(), t, t + 3);
    mi_shape floor{0, 2, 0, 4, 0, -1, 1, 0}, light{2, 2, 4, 4, 1, 0, 1, 0}, member{4, 2, 8, 4, 2, -1, 1, 1};
    h.shapes = {floor, light, member};
    mi_analytic sph{}; sph.type = MI_SHAPE_SPHERE; sph.bsdf = 3; sph.emitter = -1; identity(sph.to_world); identity(sph.to_object); sph.radius = 0.4f;
    sph.to_world[3] = 1.0f; sph.to_world[7] = 0.4f; sph.to_object[3] = -1.0f; sph.to_object[7] = -0.4f;
    h.analytic = {sph};
    mi_instance inst{}; inst.group = 0; identity(inst.to_world); identity(inst.to_object); inst.to_world[3] = -1.0f; inst.to_object[3] = 1.0f;
    h.instances = {inst};
    h.materials = in.materials; h.emitters = in.emitters;
    h.envW = 4; h.envH = 2; h.envRGB.resize(4 * 2 * 3); for (size_t i = 0; i < h.envRGB.size(); ++i) h.envRGB[i] = 0.1f + 0.05f * (float) (i % 7);
    std::memcpy(h.envToWorld, in.envToWorld, 64); h.envScale = in.envScale;
    std::memcpy(h.s2c, in.s2c, 64); std::memcpy(h.c2w, in.c2w, 64); h.nearClip = in.nearClip; h.farClip = in.farClip; h.haveCamera = true;
    h.width = 16; h.height = 12; h.filterKind = 0; h.haveFilm = true;
    h.commitHost();
    h.d = DScene{}; h.committed = true;       // upload() without a device: the parts of the scene record the edits maintain
    h.syncCameraD(); h.syncEmittersD(); h.syncEnvD();
}
template <typename T> static bool sameBytes(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T))); }
// every derived table an edit is responsible for
static void compare(const SceneHost &a, const SceneHost &b, const char *tag) {
    auto ck = [&](bool ok, const char *what) { if (!ok) { std::printf("FAIL [%s] %s differs from a fresh commit\n", tag, what); ++g_failed; } };
    ck(sameBytes(a.emittersD, b.emittersD), "emittersD"); ck(sameBytes(a.emitterCdf, b.emitterCdf), "emitterCdf"); ck(sameBytes(a.emitterX, b.emitterX), "emitterX");
    ck(sameBytes(a.areaCdf, b.areaCdf), "areaCdf"); ck(!std::memcmp(&a.emitterNorm, &b.emitterNorm, 4), "emitterNorm");
    ck(sameBytes(a.materialFlagTable, b.materialFlagTable), "materialFlagTable"); ck(sameBytes(a.materialsD, b.materialsD), "materialsD (derived material values)");
    ck(a.shade.size() == b.shade.size() && a.analyticD.size() == b.analyticD.size(), "record counts");
    for (size_t i = 0; i < a.shade.size() && i < b.shade.size(); ++i) ck(a.shade[i].flags == b.shade[i].flags, "shade[*].flags");
    for (size_t i = 0; i < a.analyticD.size() && i < b.analyticD.size(); ++i) ck(a.analyticD[i].flags == b.analyticD[i].flags, "analyticD[*].flags");
    ck(sameBytes(a.shade, b.shade), "shade"); ck(sameBytes(a.analyticD, b.analyticD), "analyticD");
    ck(!std::memcmp(a.envBsCenter, b.envBsCenter, 12) && !std::memcmp(&a.envBsRadius, &b.envBsRadius, 4), "env bounding sphere");
    ck(!std::memcmp(a.dirBsCenter, b.dirBsCenter, 12) && !std::memcmp(&a.dirBsRadius, &b.dirBsRadius, 4), "directional bounding sphere");
    ck(!std::memcmp(a.envToWorld3, b.envToWorld3, 36) && !std::memcmp(a.envToLocal3, b.envToLocal3, 36) && !std::memcmp(&a.envScale, &b.envScale, 4), "envmap transform");
    ck(a.hasDeltaEmitters == b.hasDeltaEmitters && a.envIndex == b.envIndex && a.envConstant == b.envConstant, "emitter summary");
    // ... and the scene record the kernels receive
    ck(!std::memcmp(a.d.s2c, b.d.s2c, 64) && !std::memcmp(a.d.c2w, b.d.c2w, 64) && a.d.near_clip == b.d.near_clip && a.d.far_clip == b.d.far_clip, "d camera");
    ck(!std::memcmp(a.d.cam_dx, b.d.cam_dx, 12) && !std::memcmp(a.d.cam_dy, b.d.cam_dy, 12), "d.cam_dx / cam_dy");
    ck(!std::memcmp(a.d.env_bs_center, b.d.env_bs_center, 12) && !std::memcmp(&a.d.env_bs_radius, &b.d.env_bs_radius, 4), "d env bounding sphere");
    ck(!std::memcmp(&a.d.emitter_norm, &b.d.emitter_norm, 4), "d.emitter_norm");
    ck(!std::memcmp(a.d.env_to_world, b.d.env_to_world, 36) && !std::memcmp(a.d.env_to_local, b.d.env_to_local, 36) && !std::memcmp(&a.d.env_scale, &b.d.env_scale, 4), "d envmap transform");
}

int main() {
    Inputs in = baseInputs();
    SceneHost live; fill(live, in);
    CHECK(live.treeBuilds == 1 && live.revision == 0, "one tree build, no edit yet");
    { SceneHost twin; fill(twin, in); compare(live, twin, "two commits of the same inputs"); }
    CHECK(live.materialFlagTable.size() == in.materials.size() && live.shade.size() == 6 && live.analyticD.size() == 1, "table sizes");
    std::string msg; uint64_t rev = 0;
    auto fresh = [&](const char *tag) { SceneHost f; fill(f, in); compare(live, f, tag); CHECK(live.treeBuilds == 1, "an edit must not rebuild the tree"); CHECK(live.revision == ++rev, "revision counts the edit"); };

    // --- camera: far outside the scene box (the environment emitter's bounding sphere follows), another projection
    in.c2w[3] = 30.0f; in.c2w[7] = 12.0f; in.c2w[11] = -40.0f; in.c2w[0] = 0.6f; in.c2w[2] = 0.8f; in.c2w[8] = -0.8f; in.c2w[10] = 0.6f; in.s2c[0] = 1.1f; in.s2c[3] = -0.55f; in.nearClip = 0.5f; in.farClip = 500.0f;
    const float radiusBefore = live.envBsRadius;
    CHECK(live.updateCamera(in.s2c, in.c2w, in.nearClip, in.farClip, msg) == MI_OK, "updateCamera"); fresh("camera");
    CHECK(live.envBsRadius > 2 * radiusBefore, "the camera left the box: the env bounding sphere must grow");

    // --- materials: flag flips on a scene mesh, on a group member and on the analytic sphere's record; derived sampling weights
    const std::vector<uint32_t> flagsBefore = live.materialFlagTable; bool flagsChanged = false;
    in.materials[0].flags |= MI_BSDF_FLAG_TWOSIDED;                                                        // back-side bit
    for (int c = 0; c < 3; ++c) in.materials[2].reflectance[c] = 0.0f;                                     // a diffuse without reflectance has no smooth component
    in.materials[3].alpha = 0.35f; in.materials[3].eta[0] = 1.1f; in.materials[3].k[0] = 2.0f; in.materials[3].flags |= MI_BSDF_FLAG_TWOSIDED;
    in.materials[4].reflectance[0] = 0.9f; in.materials[5].reflectance[1] = 0.8f; in.materials[5].alpha = 1.3f; in.materials[6].k[0] = 0.2f; in.materials[7].reflectance[0] = 0.25f;
    CHECK(live.updateMaterials(in.materials.data(), (uint32_t) in.materials.size(), msg, &flagsChanged) == MI_OK, "updateMaterials"); fresh("materials");
    CHECK(flagsChanged && live.materialFlagTable[0] != flagsBefore[0] && live.materialFlagTable[2] != flagsBefore[2] && live.materialFlagTable[3] != flagsBefore[3], "three materials change their flag bits");
    CHECK((live.shade[0].flags & 2u) && (live.shade[4].flags & 4u) && (live.analyticD[0].flags & 2u) && !(live.shade[2].flags & 6u), "the bits arrive in the primitives that use the material, and only there");
    in.materials[1].reflectance[2] = 0.9f;                                                                 // values only: no flag moves, nothing to patch
    CHECK(live.updateMaterials(in.materials.data(), (uint32_t) in.materials.size(), msg, &flagsChanged) == MI_OK && !flagsChanged, "a colour change moves no flag"); fresh("materials, colour only");
    for (int c = 0; c < 3; ++c) in.materials[2].reflectance[c] = 0.3f;                                     // ... and back
    CHECK(live.updateMaterials(in.materials.data(), (uint32_t) in.materials.size(), msg, &flagsChanged) == MI_OK && flagsChanged, "flip back"); fresh("materials, back");

    // --- emitters: radiance, weights, a moved point light, other spot angles and orientation
    in.emitters[0].radiance[1] = 9.0f; in.emitters[0].weight = 0.25f; in.emitters[1].weight = 3.0f;
    in.emitters[2].to_world[3] = -1.5f; in.emitters[2].to_world[11] = 2.0f; in.emitters[2].radiance[0] = 50.0f;
    in.emitters[3].cutoff = 35.0f; in.emitters[3].beam = 10.0f; in.emitters[3].to_world[0] = 0.0f; in.emitters[3].to_world[2] = 1.0f; in.emitters[3].to_world[8] = -1.0f; in.emitters[3].to_world[10] = 0.0f;
    CHECK(live.updateEmitters(in.emitters.data(), 4, msg) == MI_OK, "updateEmitters"); fresh("emitters");

    // --- envmap transform: a rotation about y and another scale
    in.envToWorld[0] = 0.0f; in.envToWorld[2] = 1.0f; in.envToWorld[8] = -1.0f; in.envToWorld[10] = 0.0f; in.envScale = 0.5f;
    CHECK(live.updateEnvmapTransform(in.envToWorld, in.envScale, msg) == MI_OK, "updateEnvmapTransform"); fresh("envmap transform");

    // --- refusals: one per rule; each leaves the scene as it was
    auto refusedM = [&](std::vector<mi_material> m, int code, const char *word) {
        msg.clear(); const int rc = live.updateMaterials(m.data(), (uint32_t) m.size(), msg, nullptr);
        if (rc != code || msg.find(word) == std::string::npos) { std::printf("FAIL refusal \"%s\": rc %d, message \"%s\"\n", word, rc, msg.c_str()); ++g_failed; }
        SceneHost f; fill(f, in); compare(live, f, word); CHECK(live.revision == rev && live.treeBuilds == 1, "a refused edit counts nothing");
    };
    auto refusedE = [&](std::vector<mi_emitter> e, int code, const char *word) {
        msg.clear(); const int rc = live.updateEmitters(e.data(), (uint32_t) e.size(), msg);
        if (rc != code || msg.find(word) == std::string::npos) { std::printf("FAIL refusal \"%s\": rc %d, message \"%s\"\n", word, rc, msg.c_str()); ++g_failed; }
        SceneHost f; fill(f, in); compare(live, f, word); CHECK(live.revision == rev && live.treeBuilds == 1, "a refused edit counts nothing");
    };
    std::vector<mi_material> m;
    m = in.materials; m.push_back(m[0]);                         refusedM(m, MI_ERR_UNSUPPORTED, "record count");
    m = in.materials; m[2].type = MI_BSDF_CONDUCTOR;             refusedM(m, MI_ERR_UNSUPPORTED, "material 2 changes its type");
    m = in.materials; m[0].flags |= MI_BSDF_TEXTURE(0);          refusedM(m, MI_ERR_UNSUPPORTED, "material 0 changes its texture binding");
    m = in.materials; m[3].flags |= MI_BSDF_FLAG_ANISOTROPIC;    refusedM(m, MI_ERR_UNSUPPORTED, "material 3 changes its anisotropic");
    m = in.materials; m[4].flags |= MI_BSDF_FLAG_NONLINEAR;      refusedM(m, MI_ERR_UNSUPPORTED, "material 4 changes its anisotropic / nonlinear");
    m = in.materials; m[3].flags &= ~MI_BSDF_FLAG_SAMPLE_VISIBLE; refusedM(m, MI_ERR_UNSUPPORTED, "material 3 changes its anisotropic / nonlinear / sampleVisible");
    m = in.materials; m[5].distr = 2;                            refusedM(m, MI_ERR_UNSUPPORTED, "material 5 changes `distr` of a wrapper");
    m = in.materials; m[6].reflectance[1] = 2.0f;                refusedM(m, MI_ERR_UNSUPPORTED, "material 6 changes the child indices of a mixturebsdf");
    m = in.materials; m[7].eta[1] = 2.0f;                        refusedM(m, MI_ERR_UNSUPPORTED, "material 7 changes the child indices of a blendbsdf");
    m = in.materials; m[8].k[2] = 3.0f;                          refusedM(m, MI_ERR_UNSUPPORTED, "material 8 changes the offset / length");
    m = in.materials; m[8].k[1] = 1.0f;                          refusedM(m, MI_ERR_UNSUPPORTED, "material 8 changes the offset / length");
    m = in.materials; m[4].eta[0] = -1.0f;                       refusedM(m, MI_ERR_INVALID, "indices of refraction must be positive");      // the shared value checks
    m = in.materials; m[6].k[0] = -0.5f;                         refusedM(m, MI_ERR_INVALID, "Invalid BSDF weight");
    std::vector<mi_emitter> e;
    e = in.emitters; e.pop_back();                               refusedE(e, MI_ERR_UNSUPPORTED, "record count");
    e = in.emitters; e[2].type = MI_EMITTER_DIRECTIONAL;         refusedE(e, MI_ERR_UNSUPPORTED, "emitter 2 changes its type");
    e = in.emitters; e[0].shape = 0;                             refusedE(e, MI_ERR_UNSUPPORTED, "emitter 0 changes its shape");
    e = in.emitters; e[3].beam = 50.0f;                          refusedE(e, MI_ERR_INVALID, "cutoffAngle >= beamWidth");
    {   // null arguments, and a scene that is not committed
        CHECK(live.updateCamera(nullptr, in.c2w, 1, 2, msg) == MI_ERR_INVALID && live.updateMaterials(nullptr, 0, msg, nullptr) == MI_ERR_INVALID && live.updateEmitters(nullptr, 0, msg) == MI_ERR_INVALID
              && live.updateEnvmapTransform(nullptr, 1, msg) == MI_ERR_INVALID, "null arguments");
        SceneHost raw; raw.materials = in.materials; raw.emitters = in.emitters;
        CHECK(raw.updateCamera(in.s2c, in.c2w, 1, 2, msg) == MI_ERR_INVALID && msg.find("not committed") != std::string::npos, "camera of an uncommitted scene");
        CHECK(raw.updateMaterials(in.materials.data(), (uint32_t) in.materials.size(), msg, nullptr) == MI_ERR_INVALID, "materials of an uncommitted scene");
        CHECK(raw.updateEmitters(in.emitters.data(), 4, msg) == MI_ERR_INVALID, "emitters of an uncommitted scene");
        CHECK(raw.updateEnvmapTransform(in.envToWorld, 1, msg) == MI_ERR_INVALID, "envmap of an uncommitted scene");
        SceneHost f; fill(f, in); compare(live, f, "after the refusals");
    }
    {   // an envmap transform needs an envmap
        Inputs c = baseInputs(); c.emitters[1].type = MI_EMITTER_CONSTANT; SceneHost h; fill(h, c);
        CHECK(h.updateEnvmapTransform(in.envToWorld, 1, msg) == MI_ERR_INVALID && msg.find("no envmap") != std::string::npos, "envmap transform without an envmap");
    }
    std::printf(g_failed ? "live_edit_host: %d check(s) FAILED\n" : "live_edit_host: all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
