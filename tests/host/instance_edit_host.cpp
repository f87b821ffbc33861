// instance_edit_host.cpp -- stand-alone check of the host side of mi_scene_update_instances (SceneHost::updateInstances / refreshHostGeometry,
// mitsuba-im_amd/csrc/scene_build.cpp over geometry_records.h -- the header k_instance_records and k_refit of kernels_geometry.hip are made of).
// Built and run by tests/test_instance_edit.py with the address and undefined-behaviour sanitizers; links scene_build.cpp only and makes no device call.
//
// Scene: a floor and a light quad at the scene level, an analytic sphere, and two shape groups (a tetrahedron, a slab of four triangles) placed seven times, built with
// binary and with 4-wide nodes.  The edit turns, scales and moves every instance and sends one far outside the old scene box.  After the edit the instance records
// equal a fresh commit's in every word but `root` (the trees differ by design), the scene box and the bounding spheres are byte-equal, the scene-level tree keeps its
// topology and stays conservative, the group trees are untouched, and the edit back restores every table.
#include "../../mitsuba-im_amd/csrc/scene_host.h"
#include "../../mitsuba-im_amd/csrc/geometry_records.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace mi { void SceneHost::release() {} }      // no device tables here
using mi::SceneHost; using mi::V3;

static int g_failed = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, what); ++g_failed; } } while (0)

static void identity(float *m) { std::memset(m, 0, 64); m[0] = m[5] = m[10] = m[15] = 1.0f; }
template <typename T> static bool sameBytes(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T))); }

// translate(t) * rotate(y, deg) * scale(s), and its inverse written out (nothing is inverted numerically: the library takes to_object from the caller)
static mi_instance place(uint32_t group, float tx, float ty, float tz, float deg, float sx, float sy, float sz) {
    mi_instance in{}; in.group = group; identity(in.to_world); identity(in.to_object);
    const float a = deg * 3.14159265358979f / 180.0f, c = std::cos(a), s = std::sin(a);
    float *w = in.to_world, *o = in.to_object;
    w[0] = c * sx; w[2] = s * sz; w[5] = sy; w[8] = -s * sx; w[10] = c * sz; w[3] = tx; w[7] = ty; w[11] = tz;
    o[0] = c / sx; o[2] = -s / sx; o[5] = 1 / sy; o[8] = s / sz; o[10] = c / sz;
    o[3] = -(o[0] * tx + o[2] * tz); o[7] = -ty / sy; o[11] = -(o[8] * tx + o[10] * tz);
    return in;
}
static std::vector<mi_instance> placement(int which) {
    std::vector<mi_instance> v;
    for (int i = 0; i < 7; ++i) {
        const float fi = (float) i;
        if (which == 0) v.push_back(place((uint32_t) (i & 1), -3.0f + fi, 0.0f, -1.0f + 0.5f * (float) (i % 3), 20.0f * fi, 1.0f, 1.0f + 0.1f * fi, 1.0f));
        else v.push_back(place((uint32_t) (i & 1), 2.5f - 0.8f * fi, 0.1f * fi, 1.5f - 0.6f * (float) (i % 4), 77.0f + 31.0f * fi, 0.7f + 0.2f * fi, 1.3f, 1.6f - 0.1f * fi));
    }
    if (which == 1) v[3] = place(1, 30.0f, 25.0f, 40.0f, 30.0f, 3.0f, 2.0f, 3.0f);      // far outside the old scene box
    return v;
}
static void fill(SceneHost &h, const std::vector<mi_instance> &inst, bool withInstances = true) {
    const float P[][3] = {{4, 0, -4}, {-4, 0, -4}, {-4, 0, 4}, {4, 0, 4},   {0.5f, 3, -0.5f}, {0.5f, 3, 0.5f}, {-0.5f, 3, 0.5f}, {-0.5f, 3, -0.5f},
                          {0, 0, 0}, {0.4f, 0, 0}, {0.2f, 0, 0.35f}, {0.2f, 0.5f, 0.12f},                                   // group 0: tetrahedron
                          {-0.3f, 0, -0.2f}, {0.3f, 0, -0.2f}, {0.3f, 0.25f, -0.2f}, {-0.3f, 0.25f, -0.2f}, {-0.3f, 0.25f, 0.2f}, {0.3f, 0.25f, 0.2f}};   // group 1: slab
    const uint32_t I[][3] = {{0, 1, 2}, {0, 2, 3}, {4, 5, 6}, {4, 6, 7},   {8, 9, 10}, {8, 9, 11}, {9, 10, 11}, {10, 8, 11},   {12, 13, 14}, {12, 14, 15}, {15, 14, 17}, {15, 17, 16}};
    for (auto &p : P) h.pos.insert(h.pos.end(), p, p + 3);
    for (auto &t : I) h.idx.insert(h.idx.end(), t, t + 3);
    mi_shape floor{0, 2, 0, 4, 0, -1, 1, 0}, light{2, 2, 4, 4, 1, 0, 1, 0}, tetra{4, 4, 8, 4, 2, -1, 1, withInstances ? 1u : 0u}, slab{8, 4, 12, 6, 2, -1, 1, withInstances ? 2u : 0u};
    h.shapes = {floor, light, tetra, slab};
    mi_analytic sph{}; sph.type = MI_SHAPE_SPHERE; sph.bsdf = 0; sph.emitter = -1; identity(sph.to_world); identity(sph.to_object); sph.radius = 0.4f;
    sph.to_world[3] = 1.0f; sph.to_world[7] = 0.4f; sph.to_world[11] = 2.0f; sph.to_object[3] = -1.0f; sph.to_object[7] = -0.4f; sph.to_object[11] = -2.0f;
    h.analytic = {sph};
    if (withInstances) h.instances = inst;
    mi_material m{}; m.type = MI_BSDF_DIFFUSE; m.reflectance[0] = m.reflectance[1] = m.reflectance[2] = 0.5f; h.materials = {m, m, m};
    mi_emitter e{}; e.type = MI_EMITTER_AREA; e.shape = 1; e.weight = 1; e.radiance[0] = e.radiance[1] = e.radiance[2] = 10; identity(e.to_world);
    mi_emitter sky{}; sky.type = MI_EMITTER_CONSTANT; sky.shape = -1; sky.weight = 1; sky.radiance[0] = sky.radiance[1] = sky.radiance[2] = 0.3f; identity(sky.to_world);
    h.emitters = {e, sky};
    identity(h.s2c); h.s2c[0] = 0.8f; h.s2c[5] = 0.6f; h.s2c[3] = -0.4f; h.s2c[7] = -0.3f; h.s2c[11] = 1.0f;
    identity(h.c2w); h.c2w[3] = 0.2f; h.c2w[7] = 1.0f; h.c2w[11] = -4.5f; h.nearClip = 0.1f; h.farClip = 100.0f; h.haveCamera = true;
    h.width = 16; h.height = 12; h.filterKind = 0; h.haveFilm = true;
    h.commitHost();
    h.d = DScene{}; h.committed = true;       // upload() without a device: the parts of the scene record the edits maintain
    for (int i = 0; i < 3; ++i) { h.d.aabb_lo[i] = h.aabbLo[i]; h.d.aabb_hi[i] = h.aabbHi[i]; }
    h.syncCameraD(); h.syncEmittersD(); h.syncEnvD();
}
static void compareFresh(const SceneHost &a, const SceneHost &b, const char *tag) {
    auto ck = [&](bool ok, const char *what) { if (!ok) { std::printf("FAIL [%s] %s differs from a fresh commit\n", tag, what); ++g_failed; } };
    ck(a.instancesD.size() == b.instancesD.size(), "instance record count");
    for (size_t i = 0; i < a.instancesD.size() && i < b.instancesD.size(); ++i) {
        InstanceD x = a.instancesD[i], y = b.instancesD[i]; x.root = y.root = 0;
        ck(!std::memcmp(&x, &y, sizeof(x)), "InstanceD (every word but root)");
        ck(!std::memcmp(a.instances[i].to_world, b.instances[i].to_world, 64) && !std::memcmp(a.instances[i].to_object, b.instances[i].to_object, 64) && a.instances[i].group == b.instances[i].group, "instances (inputs)");
    }
    ck(!std::memcmp(a.aabbLo, b.aabbLo, 12) && !std::memcmp(a.aabbHi, b.aabbHi, 12), "scene AABB");
    ck(!std::memcmp(a.envBsCenter, b.envBsCenter, 12) && !std::memcmp(&a.envBsRadius, &b.envBsRadius, 4), "env bounding sphere");
    ck(!std::memcmp(a.dirBsCenter, b.dirBsCenter, 12) && !std::memcmp(&a.dirBsRadius, &b.dirBsRadius, 4), "directional bounding sphere");
    ck(!std::memcmp(a.d.aabb_lo, b.d.aabb_lo, 12) && !std::memcmp(a.d.aabb_hi, b.d.aabb_hi, 12), "d.aabb");
    ck(!std::memcmp(a.d.dir_bs_center, b.d.dir_bs_center, 12) && !std::memcmp(&a.d.dir_bs_radius, &b.d.dir_bs_radius, 4), "d directional bounding sphere");
    ck(!std::memcmp(a.d.env_bs_center, b.d.env_bs_center, 12) && !std::memcmp(&a.d.env_bs_radius, &b.d.env_bs_radius, 4), "d env bounding sphere");
    ck(!std::memcmp(&a.d.emitter_norm, &b.d.emitter_norm, 4), "d.emitter_norm");
    ck(sameBytes(a.shade, b.shade) && sameBytes(a.analyticD, b.analyticD) && sameBytes(a.emittersD, b.emittersD) && sameBytes(a.areaCdf, b.areaCdf) && sameBytes(a.emitterX, b.emitterX), "tables an instance edit does not touch");
}
static std::vector<int32_t> childCodes(const SceneHost &h) {
    std::vector<int32_t> c;
    for (const BvhNode &n : h.nodes) { if (h.wideBvh) { Bvh4Node w; std::memcpy(&w, &n, sizeof(w)); c.insert(c.end(), w.child, w.child + 4); } else { c.push_back(n.c0); c.push_back(n.c1); } }
    return c;
}
// Every child box of the scene-level tree -- for 4-wide nodes the float reconstruction org + q * step the walks compute -- encloses the padded boxes of all primitives
// below it: scene-level triangles, the analytic shape, and the instances with their CURRENT transforms.
struct Enclose {
    const SceneHost &h; size_t violations = 0, leaves = 0, instancesSeen = 0;
    explicit Enclose(const SceneHost &hh) : h(hh) {}
    bool boxOf(const TriAccelD &r, V3 &lo, V3 &hi) {
        V3 c;
        if (r.k == MI_K_INSTANCE) { const InstanceD &in = h.instancesD[r.prim]; V3 bl, bh; mi::instanceBoxes(h.instances[r.prim].to_world, mi::load3(in.glo), mi::load3(in.ghi), bl, bh, lo, hi, c); ++instancesSeen; return true; }
        if (r.k == MI_K_ANALYTIC) { const size_t slot = (size_t) (&r - h.tris.data()); lo = mi::load3(&h.leafBoxes[slot * 6]); hi = mi::load3(&h.leafBoxes[slot * 6 + 3]); return true; }
        if (r.prim >= h.nTris) return false;      // the never-hit record of unused 4-wide slots
        mi::triPaddedBox(mi::load3(&h.pos[(size_t) h.idx[r.prim * 3] * 3]), mi::load3(&h.pos[(size_t) h.idx[r.prim * 3 + 1] * 3]), mi::load3(&h.pos[(size_t) h.idx[r.prim * 3 + 2] * 3]), lo, hi, c);
        return true;
    }
    void below(int32_t code, V3 &lo, V3 &hi) {
        const float inf = std::numeric_limits<float>::infinity(); lo = mi::mk(inf, inf, inf); hi = mi::mk(-inf, -inf, -inf);
        if (code < 0) {
            const uint32_t leaf = (uint32_t) ~code, first = leaf >> 3, count = (leaf & 7u) + 1u; ++leaves;
            for (uint32_t i = 0; i < count; ++i) { V3 l, hh2; if (boxOf(h.tris[first + i], l, hh2)) { lo = mi::vmin(lo, l); hi = mi::vmax(hi, hh2); } }
            return;
        }
        const BvhNode &n = h.nodes[code];
        auto inside = [&](V3 blo, V3 bhi, V3 l, V3 hh2) { if (l.x > hh2.x) return; if (!(blo.x <= l.x && blo.y <= l.y && blo.z <= l.z && bhi.x >= hh2.x && bhi.y >= hh2.y && bhi.z >= hh2.z)) ++violations; };
        if (h.wideBvh) {
            Bvh4Node w; std::memcpy(&w, &n, sizeof(w)); const float st[3] = {w.step_x, w.step_y, w.step_z};
            for (int c = 0; c < 4; ++c) {
                if (mi::wideSlotUnused(w, c)) continue;
                V3 l, hh2; below(w.child[c], l, hh2); float bl[3], bh[3];
                for (int a = 0; a < 3; ++a) { bl[a] = w.org[a] + (float) ((w.qlo[a] >> (8 * c)) & 0xFFu) * st[a]; bh[a] = w.org[a] + (float) ((w.qhi[a] >> (8 * c)) & 0xFFu) * st[a]; }
                inside(mi::load3(bl), mi::load3(bh), l, hh2); lo = mi::vmin(lo, l); hi = mi::vmax(hi, hh2);
            }
        } else {
            V3 l, hh2;
            if (!(n.lo0[0] > n.hi0[0])) { below(n.c0, l, hh2); inside(mi::load3(n.lo0), mi::load3(n.hi0), l, hh2); lo = mi::vmin(lo, l); hi = mi::vmax(hi, hh2); }
            if (!(n.lo1[0] > n.hi1[0])) { below(n.c1, l, hh2); inside(mi::load3(n.lo1), mi::load3(n.hi1), l, hh2); lo = mi::vmin(lo, l); hi = mi::vmax(hi, hh2); }
        }
    }
};
static void enclosed(const SceneHost &h, const char *tag) {
    Enclose e(h); V3 lo, hi; e.below(0, lo, hi);
    if (e.violations) std::printf("  [%s] %zu child boxes do not enclose their primitives\n", tag, e.violations);
    CHECK(e.violations == 0 && e.leaves > 0 && e.instancesSeen == h.instances.size(), "every scene-level child box encloses the padded boxes below it, every instance is reached");
}
// nodes of the group trees = those the refit order does not name
static bool groupNodesEqual(const SceneHost &h, const std::vector<BvhNode> &before, size_t &nGroupNodes) {
    std::vector<uint8_t> sceneLevel(h.nodes.size(), 0); for (uint32_t n : h.refitOrder) sceneLevel[n] = 1;
    bool same = h.nodes.size() == before.size(); nGroupNodes = 0;
    for (size_t i = 0; same && i < h.nodes.size(); ++i) if (!sceneLevel[i]) { ++nGroupNodes; if (std::memcmp(&h.nodes[i], &before[i], sizeof(BvhNode))) same = false; }
    return same;
}

static void editCycle(const char *tag) {
    const std::vector<mi_instance> A = placement(0), B = placement(1);
    SceneHost live; fill(live, A);
    CHECK(live.treeBuilds == 1 && live.revision == 0, "one tree build, no edit yet");
    const std::vector<BvhNode> nodes0 = live.nodes; const std::vector<InstanceD> inst0 = live.instancesD; const std::vector<TriAccelD> tris0 = live.tris; const std::vector<int32_t> codes = childCodes(live);
    float box0[6]; std::memcpy(box0, live.aabbLo, 12); std::memcpy(box0 + 3, live.aabbHi, 12);
    std::string msg;
    CHECK(live.updateInstances(B.data(), (uint32_t) B.size(), msg) == MI_OK, "updateInstances"); if (!msg.empty()) std::printf("  %s\n", msg.c_str());
    CHECK(live.instStale && !live.geoStale && live.revision == 1 && live.treeBuilds == 1, "an edit advances the revision, marks the mirrors stale and builds no tree");
    live.refreshHostGeometry(); CHECK(!live.instStale, "refreshHostGeometry() clears the stale mark");
    { SceneHost fresh; fill(fresh, B); compareFresh(live, fresh, tag); }
    CHECK(live.aabbHi[0] > 30.0f && live.aabbHi[1] > 25.0f && live.aabbHi[2] > 40.0f && box0[3] < 10.0f, "the edit sends an instance far outside the old scene box");
    CHECK(childCodes(live) == codes && sameBytes(live.tris, tris0), "child codes and leaf records are unchanged");
    CHECK(!sameBytes(live.nodes, nodes0) && !sameBytes(live.instancesD, inst0), "the edit changes the scene-level boxes and the instance records");
    for (size_t i = 0; i < inst0.size(); ++i) CHECK(live.instancesD[i].root == inst0[i].root && live.instancesD[i].group == inst0[i].group && !std::memcmp(live.instancesD[i].glo, inst0[i].glo, 12) && !std::memcmp(live.instancesD[i].ghi, inst0[i].ghi, 12), "root, group, glo, ghi stay");
    { size_t ng = 0; CHECK(groupNodesEqual(live, nodes0, ng) && ng >= 2 && live.refitOrder.size() + ng == live.nodes.size(), "the group trees' nodes are byte-identical; the refit covers exactly the scene-level tree"); }
    CHECK(live.leafSlotOfInstance.size() == A.size(), "one leaf slot per instance");
    for (size_t i = 0; i < live.leafSlotOfInstance.size(); ++i) { const TriAccelD &r = live.tris[live.leafSlotOfInstance[i]]; CHECK(r.k == MI_K_INSTANCE && r.prim == i, "leafSlotOfInstance names the instance's record"); }
    enclosed(live, tag);
    // a second edit without a refresh in between, then back: every table as committed
    CHECK(live.updateInstances(B.data(), (uint32_t) B.size(), msg) == MI_OK && live.updateInstances(A.data(), (uint32_t) A.size(), msg) == MI_OK, "updateInstances back");
    live.refreshHostGeometry();
    CHECK(live.revision == 3 && live.treeBuilds == 1, "three edits, one tree build");
    CHECK(sameBytes(live.nodes, nodes0), "back: nodes"); CHECK(sameBytes(live.instancesD, inst0), "back: instance records"); CHECK(sameBytes(live.tris, tris0), "back: leaf records");
    CHECK(!std::memcmp(box0, live.aabbLo, 12) && !std::memcmp(box0 + 3, live.aabbHi, 12), "back: scene box");
    { SceneHost fresh; fill(fresh, A); compareFresh(live, fresh, "back"); CHECK(sameBytes(live.nodes, fresh.nodes), "back: the tree is the fresh scene's tree"); }
    enclosed(live, "back");
    // recommit on the same object: the edit state of the old tree must be gone, and an edit of the new tree works
    CHECK(live.updateInstances(B.data(), (uint32_t) B.size(), msg) == MI_OK && live.instStale, "edit before the recommit");
    live.commitHost();
    CHECK(live.treeBuilds == 2 && !live.instStale && !live.geoPrepared && live.leafSlotOfInstance.empty() && live.refitOrder.empty() && live.leafBoxes.empty() && live.nodeBoxes.empty(), "a commit drops the instance-edit state of the previous tree");
    for (int i = 0; i < 3; ++i) { live.d.aabb_lo[i] = live.aabbLo[i]; live.d.aabb_hi[i] = live.aabbHi[i]; } live.syncCameraD(); live.syncEmittersD();
    { SceneHost fresh; fill(fresh, B); const std::vector<BvhNode> committed = live.nodes; live.refreshHostGeometry(); CHECK(sameBytes(live.nodes, committed) && sameBytes(live.nodes, fresh.nodes) && sameBytes(live.instancesD, fresh.instancesD), "the recommitted tables are the fresh scene's"); }
    CHECK(live.updateInstances(A.data(), (uint32_t) A.size(), msg) == MI_OK, "edit after the recommit"); live.refreshHostGeometry();
    { SceneHost fresh; fill(fresh, A); compareFresh(live, fresh, "after the recommit"); } enclosed(live, "after the recommit");
}

int main() {
    setenv("MI355PT_BVH2", "1", 1); editCycle("binary nodes");
    { SceneHost h; fill(h, placement(0)); CHECK(!h.wideBvh, "MI355PT_BVH2=1 gives binary nodes"); }
    setenv("MI355PT_BVH2", "0", 1); editCycle("4-wide nodes");
    { SceneHost h; fill(h, placement(0)); CHECK(h.wideBvh, "MI355PT_BVH2=0 gives 4-wide nodes"); }
    // refusals: each names the function, leaves the scene as it was and counts nothing
    {
        setenv("MI355PT_BVH2", "1", 1);
        const std::vector<mi_instance> A = placement(0); SceneHost h; fill(h, A); const std::vector<BvhNode> nodes0 = h.nodes; const std::vector<InstanceD> inst0 = h.instancesD; std::string msg; const uint32_t n = (uint32_t) A.size();
        auto refused = [&](int rc, int code, const char *word) {
            if (rc != code || msg.find("mi_scene_update_instances") != 0 || msg.find(word) == std::string::npos) { std::printf("FAIL refusal \"%s\": rc %d, message \"%s\"\n", word, rc, msg.c_str()); ++g_failed; }
            CHECK(sameBytes(h.nodes, nodes0) && sameBytes(h.instancesD, inst0) && h.revision == 0 && h.treeBuilds == 1 && !h.instStale && !std::memcmp(h.instances.data(), A.data(), A.size() * sizeof(mi_instance)), "a refused edit leaves the scene untouched");
        };
        refused(h.updateInstances(nullptr, n, msg), MI_ERR_INVALID, "null");
        refused(h.updateInstances(A.data(), n - 1, msg), MI_ERR_INVALID, "7 -> 6");
        refused(h.updateInstances(A.data(), 0, msg), MI_ERR_INVALID, "7 -> 0");
        { std::vector<mi_instance> b = A; b[5].group = 0; b[6].group = 1; refused(h.updateInstances(b.data(), n, msg), MI_ERR_UNSUPPORTED, "instance 5"); }
        { std::vector<mi_instance> b = A; b[2].to_world[7] = std::numeric_limits<float>::infinity(); b[5].to_world[0] = std::nanf(""); refused(h.updateInstances(b.data(), n, msg), MI_ERR_INVALID, "instance 2"); }
        { std::vector<mi_instance> b = A; b[3].to_object[11] = std::nanf(""); refused(h.updateInstances(b.data(), n, msg), MI_ERR_INVALID, "instance 3"); CHECK(msg.find("to_object") != std::string::npos, "the message names to_object"); }
        { SceneHost raw; raw.instances = A; CHECK(raw.updateInstances(A.data(), n, msg) == MI_ERR_INVALID && msg.find("mi_scene_update_instances") == 0 && msg.find("not committed") != std::string::npos, "a scene that is not committed"); }
        { SceneHost plain; fill(plain, A, false); CHECK(plain.updateInstances(A.data(), n, msg) == MI_ERR_INVALID && msg.find("mi_scene_update_instances") == 0 && msg.find("the scene has no instances") != std::string::npos && plain.revision == 0, "a scene without instances"); }
        // vertex edits of an instanced scene stay refused
        CHECK(h.updateVertices(h.pos.data(), nullptr, (uint32_t) (h.pos.size() / 3), msg) == MI_ERR_UNSUPPORTED && msg.find("instance 0") != std::string::npos, "mi_scene_update_vertices still refuses instanced scenes");
    }
    std::printf(g_failed ? "instance_edit_host: %d check(s) FAILED\n" : "instance_edit_host: all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
