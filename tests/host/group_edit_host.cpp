// group_edit_host.cpp -- stand-alone check of the host side of mi_scene_update_geometry (SceneHost::updateGeometry / refreshHostGeometry,
// mitsuba-im_amd/csrc/scene_build.cpp over geometry_records.h -- the header k_tri_records, k_instance_records and k_refit of kernels_geometry.hip are made of).
// Built and run by tests/test_group_edit.py with the address and undefined-behaviour sanitizers; links scene_build.cpp only and makes no device call.
//
// Scene: a textured floor and a light quad at the scene level, an analytic sphere, and two shape groups (a smooth-shaded tetrahedron, a slab of four triangles) placed
// seven times, built with binary and with 4-wide nodes.  The vertex edit scales both groups' members, lifts a floor corner and moves a corner of the light; the
// instance edit is the one of instance_edit_host.cpp.  After refreshHostGeometry() -- the CPU twin of every device step -- the tables equal a fresh commit's, every
// tree (scene level and groups) keeps its topology and stays conservative, the edit back restores every byte, and any interleaving with the two older calls ends in
// the tables of the single combined call.
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
// vertices 0..3 floor, 4..7 light, 8..11 group 0 (tetrahedron, smooth), 12..17 group 1 (slab)
struct Verts { std::vector<float> pos, nrm; };
static Verts vertices(int which) {
    const float P[][3] = {{4, 0, -4}, {-4, 0, -4}, {-4, 0, 4}, {4, 0, 4},   {0.5f, 3, -0.5f}, {0.5f, 3, 0.5f}, {-0.5f, 3, 0.5f}, {-0.5f, 3, -0.5f},
                          {0, 0, 0}, {0.4f, 0, 0}, {0.2f, 0, 0.35f}, {0.2f, 0.5f, 0.12f},
                          {-0.3f, 0, -0.2f}, {0.3f, 0, -0.2f}, {0.3f, 0.25f, -0.2f}, {-0.3f, 0.25f, -0.2f}, {-0.3f, 0.25f, 0.2f}, {0.3f, 0.25f, 0.2f}};
    Verts v;
    for (int i = 0; i < 18; ++i) {
        float p[3] = {P[i][0], P[i][1], P[i][2]}, n[3] = {0, 1, 0};
        if (i >= 8 && i < 12) { n[0] = p[0] - 0.2f; n[1] = p[1] - 0.12f; n[2] = p[2] - 0.12f; }
        if (which == 1) {
            if (i == 0) p[1] = 2.0f;                                            // a floor corner: a scene-level vertex of an instanced scene
            if (i == 4) { p[0] += 0.1f; p[1] += 0.2f; }                         // a corner of the light: its area CDF follows
            if (i >= 8 && i < 12) { p[0] *= 1.3f; p[1] *= 1.5f; p[2] *= 1.2f; n[0] /= 1.3f; n[1] /= 1.5f; n[2] /= 1.2f; }
            if (i >= 12) p[1] *= 1.8f;
        }
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int k = 0; k < 3; ++k) { v.pos.push_back(p[k]); v.nrm.push_back(n[k] / len); }
    }
    return v;
}
static void fill(SceneHost &h, const Verts &v, const std::vector<mi_instance> &inst, bool withInstances = true) {
    const uint32_t I[][3] = {{0, 1, 2}, {0, 2, 3}, {4, 5, 6}, {4, 6, 7},   {8, 9, 10}, {8, 9, 11}, {9, 10, 11}, {10, 8, 11},   {12, 13, 14}, {12, 14, 15}, {15, 14, 17}, {15, 17, 16}};
    h.pos = v.pos; h.nrm = v.nrm;
    { const Verts v0 = vertices(0); for (size_t i = 0; i < v0.pos.size() / 3; ++i) { h.uv.push_back(0.1f * v0.pos[i * 3] + 0.03f * (float) i); h.uv.push_back(0.1f * v0.pos[i * 3 + 2]); } }      // texture coordinates never move: those of description 0, whatever the vertices
    for (auto &t : I) h.idx.insert(h.idx.end(), t, t + 3);
    mi_shape floor{0, 2, 0, 4, 0, -1, 3, 0}, light{2, 2, 4, 4, 1, 0, 1, 0}, tetra{4, 4, 8, 4, 2, -1, 0, withInstances ? 1u : 0u}, slab{8, 4, 12, 6, 2, -1, 1, withInstances ? 2u : 0u};
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
    for (int i = 0; i < 3; ++i) { h.d.aabb_lo[i] = h.aabbLo[i]; h.d.aabb_hi[i] = h.aabbHi[i]; h.d.packet_gk[i] = h.packetGK[i]; }
    h.d.packet_scale = h.packetScale; h.syncCameraD(); h.syncEmittersD(); h.syncEnvD();
}
static void fillFrom(SceneHost &h, int verts, int inst, bool withInstances = true) { fill(h, vertices(verts), placement(inst), withInstances); }
static uint64_t keyOf(const SceneHost &h, const TriAccelD &r) {
    if (r.k == MI_K_INSTANCE) return (uint64_t) h.nTris + h.analytic.size() + r.prim;
    return r.prim;      // triangles: the triangle; analytic shapes: nTris + i; the never-hit record: 0xFFFFFFFF (skipped)
}
// every table a geometry edit is responsible for, against a fresh commit of the new description
static void compareFresh(const SceneHost &a, const SceneHost &b, const char *tag) {
    auto ck = [&](bool ok, const char *what) { if (!ok) { std::printf("FAIL [%s] %s differs from a fresh commit\n", tag, what); ++g_failed; } };
    {   // leaf records: a fresh commit may order them differently (its trees are built for the new vertices), so per primitive
        const size_t np = (size_t) a.nTris + a.analytic.size() + a.instances.size(); std::vector<const TriAccelD *> byPrim(np, nullptr);
        for (const TriAccelD &r : b.tris) if (keyOf(b, r) < np) byPrim[keyOf(b, r)] = &r;
        size_t seen = 0, bad = 0;
        for (const TriAccelD &r : a.tris) { const uint64_t k = keyOf(a, r); if (k >= np) continue; ++seen; if (!byPrim[k] || std::memcmp(&r, byPrim[k], sizeof(r))) ++bad; }
        ck(seen == np && bad == 0 && a.tris.size() == b.tris.size(), "tris (leaf records, by primitive)");
    }
    ck(sameBytes(a.shade, b.shade), "shade"); ck(sameBytes(a.triuv, b.triuv) && !a.triuv.empty(), "triuv"); ck(sameBytes(a.packetExact, b.packetExact), "packetExact");
    ck(a.instancesD.size() == b.instancesD.size(), "instance record count");
    for (size_t i = 0; i < a.instancesD.size() && i < b.instancesD.size(); ++i) {
        InstanceD x = a.instancesD[i], y = b.instancesD[i]; x.root = y.root = 0;
        ck(!std::memcmp(&x, &y, sizeof(x)), "InstanceD (every word but root)");
    }
    ck(sameBytes(a.groupBoxes, b.groupBoxes), "group boxes");
    ck(!std::memcmp(a.aabbLo, b.aabbLo, 12) && !std::memcmp(a.aabbHi, b.aabbHi, 12), "scene AABB");
    ck(!std::memcmp(a.envBsCenter, b.envBsCenter, 12) && !std::memcmp(&a.envBsRadius, &b.envBsRadius, 4), "env bounding sphere");
    ck(!std::memcmp(a.dirBsCenter, b.dirBsCenter, 12) && !std::memcmp(&a.dirBsRadius, &b.dirBsRadius, 4), "directional bounding sphere");
    ck(!std::memcmp(a.d.aabb_lo, b.d.aabb_lo, 12) && !std::memcmp(a.d.aabb_hi, b.d.aabb_hi, 12), "d.aabb");
    ck(!std::memcmp(a.d.dir_bs_center, b.d.dir_bs_center, 12) && !std::memcmp(&a.d.dir_bs_radius, &b.d.dir_bs_radius, 4), "d directional bounding sphere");
    ck(!std::memcmp(a.d.env_bs_center, b.d.env_bs_center, 12) && !std::memcmp(&a.d.env_bs_radius, &b.d.env_bs_radius, 4), "d env bounding sphere");
    ck(!std::memcmp(&a.d.emitter_norm, &b.d.emitter_norm, 4), "d.emitter_norm");
    ck(sameBytes(a.emittersD, b.emittersD) && sameBytes(a.areaCdf, b.areaCdf) && sameBytes(a.emitterCdf, b.emitterCdf) && sameBytes(a.emitterX, b.emitterX), "emitter tables");
    ck(sameBytes(a.analyticD, b.analyticD), "analytic records");
    if (a.instances.empty()) ck(sameBytes(a.packetGroups, b.packetGroups) && !std::memcmp(a.packetGK, b.packetGK, 12) && !std::memcmp(&a.packetScale, &b.packetScale, 4) && !std::memcmp(a.d.packet_gk, b.d.packet_gk, 12) && !std::memcmp(&a.d.packet_scale, &b.d.packet_scale, 4), "packet tables");
}
// two scenes that share one commit (the same trees): every mirror byte for byte
static bool sameTables(const SceneHost &a, const SceneHost &b) {
    return sameBytes(a.nodes, b.nodes) && sameBytes(a.tris, b.tris) && sameBytes(a.shade, b.shade) && sameBytes(a.triuv, b.triuv) && sameBytes(a.packetExact, b.packetExact) && sameBytes(a.packetGroups, b.packetGroups) &&
           sameBytes(a.instancesD, b.instancesD) && sameBytes(a.groupBoxes, b.groupBoxes) && sameBytes(a.emittersD, b.emittersD) && sameBytes(a.areaCdf, b.areaCdf) && !std::memcmp(a.aabbLo, b.aabbLo, 12) && !std::memcmp(a.aabbHi, b.aabbHi, 12) &&
           !std::memcmp(a.d.aabb_lo, b.d.aabb_lo, 12) && !std::memcmp(a.d.aabb_hi, b.d.aabb_hi, 12) && !std::memcmp(&a.d.env_bs_radius, &b.d.env_bs_radius, 4) && sameBytes(a.pos, b.pos) && sameBytes(a.nrm, b.nrm);
}
static std::vector<int32_t> childCodes(const SceneHost &h) {
    std::vector<int32_t> c;
    for (const BvhNode &n : h.nodes) { if (h.wideBvh) { Bvh4Node w; std::memcpy(&w, &n, sizeof(w)); c.insert(c.end(), w.child, w.child + 4); } else { c.push_back(n.c0); c.push_back(n.c1); } }
    return c;
}
// which slots carry an inverted box (unused 4-wide slots, the empty child of a one-leaf binary tree)
static std::vector<uint8_t> invertedSlots(const SceneHost &h) {
    std::vector<uint8_t> v;
    for (const BvhNode &n : h.nodes) {
        if (h.wideBvh) { Bvh4Node w; std::memcpy(&w, &n, sizeof(w)); for (int c = 0; c < 4; ++c) { bool inv = true; for (int a = 0; a < 3; ++a) inv = inv && ((w.qlo[a] >> (8 * c)) & 0xFFu) == 255u && ((w.qhi[a] >> (8 * c)) & 0xFFu) == 0u; v.push_back(inv); } }
        else { v.push_back(n.lo0[0] > n.hi0[0]); v.push_back(n.lo1[0] > n.hi1[0]); }
    }
    return v;
}
// Every child box of a tree -- for 4-wide nodes the float reconstruction org + q * step the walks compute -- encloses the padded boxes of all primitives below it,
// derived here from the CURRENT vertices and transforms.
struct Enclose {
    const SceneHost &h; size_t violations = 0, leaves = 0, instancesSeen = 0, trisSeen = 0;
    explicit Enclose(const SceneHost &hh) : h(hh) {}
    bool boxOf(const TriAccelD &r, V3 &lo, V3 &hi) {
        V3 c;
        if (r.k == MI_K_INSTANCE) { const InstanceD &in = h.instancesD[r.prim]; V3 bl, bh; mi::instanceBoxes(h.instances[r.prim].to_world, mi::load3(in.glo), mi::load3(in.ghi), bl, bh, lo, hi, c); ++instancesSeen; return true; }
        if (r.k == MI_K_ANALYTIC) { const size_t slot = (size_t) (&r - h.tris.data()); lo = mi::load3(&h.leafBoxes[slot * 6]); hi = mi::load3(&h.leafBoxes[slot * 6 + 3]); return true; }
        if (r.prim >= h.nTris) return false;      // the never-hit record of unused 4-wide slots
        mi::triPaddedBox(mi::load3(&h.pos[(size_t) h.idx[r.prim * 3] * 3]), mi::load3(&h.pos[(size_t) h.idx[r.prim * 3 + 1] * 3]), mi::load3(&h.pos[(size_t) h.idx[r.prim * 3 + 2] * 3]), lo, hi, c);
        ++trisSeen; return true;
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
    for (int root : h.groupRoot) e.below(root, lo, hi);
    if (e.violations) std::printf("  [%s] %zu child boxes do not enclose their primitives\n", tag, e.violations);
    CHECK(e.violations == 0 && e.leaves > 0 && e.instancesSeen == h.instances.size() && e.trisSeen == h.nTris, "every child box of every tree encloses the padded boxes below it; every instance and every triangle is reached once");
}

struct Snapshot {
    std::vector<BvhNode> nodes; std::vector<TriAccelD> tris, packetExact; std::vector<TriShade> shade; std::vector<TriUV> triuv; std::vector<InstanceD> inst; std::vector<float> groupBoxes, areaCdf; float box[6];
    explicit Snapshot(const SceneHost &h) : nodes(h.nodes), tris(h.tris), packetExact(h.packetExact), shade(h.shade), triuv(h.triuv), inst(h.instancesD), groupBoxes(h.groupBoxes), areaCdf(h.areaCdf) { std::memcpy(box, h.aabbLo, 12); std::memcpy(box + 3, h.aabbHi, 12); }
    bool equals(const SceneHost &h) const { return sameBytes(nodes, h.nodes) && sameBytes(tris, h.tris) && sameBytes(packetExact, h.packetExact) && sameBytes(shade, h.shade) && sameBytes(triuv, h.triuv) && sameBytes(inst, h.instancesD) && sameBytes(groupBoxes, h.groupBoxes) && sameBytes(areaCdf, h.areaCdf) && !std::memcmp(box, h.aabbLo, 12) && !std::memcmp(box + 3, h.aabbHi, 12); }
};

// A -> (verts, inst) by ONE updateGeometry call; which parts are passed follows from what differs from (0, 0)
static int geometryCall(SceneHost &h, int verts, int inst, bool passVerts, bool passInst, std::string &msg) {
    const Verts v = vertices(verts); const std::vector<mi_instance> I = placement(inst);
    return h.updateGeometry(passVerts ? v.pos.data() : nullptr, passVerts ? v.nrm.data() : nullptr, passVerts ? (uint32_t) (v.pos.size() / 3) : 0u, passInst ? I.data() : nullptr, passInst ? (uint32_t) I.size() : 0u, msg);
}

static void editCycle(const char *kind, int verts, int inst) {
    char tag[96]; std::snprintf(tag, sizeof(tag), "%s, %s", kind, verts && inst ? "vertices + instances" : verts ? "vertices only" : "instances only");
    SceneHost live; fillFrom(live, 0, 0);
    CHECK(live.treeBuilds == 1 && live.revision == 0 && live.groupRoot.size() == 2 && live.groupBoxes.size() == 12, "one tree build, no edit yet, two groups");
    const Snapshot first(live); const std::vector<int32_t> codes = childCodes(live); const std::vector<uint8_t> inverted = invertedSlots(live);
    std::string msg;
    CHECK(geometryCall(live, verts, inst, verts != 0, inst != 0, msg) == MI_OK, "updateGeometry"); if (!msg.empty()) std::printf("  %s\n", msg.c_str());
    CHECK(live.geoStale == (verts != 0) && live.instStale && live.revision == 1 && live.treeBuilds == 1, "an edit advances the revision once, marks the mirrors stale and builds no tree");
    live.refreshHostGeometry(); CHECK(!live.instStale && !live.geoStale, "refreshHostGeometry() clears the stale marks");
    { SceneHost fresh; fillFrom(fresh, verts, inst); compareFresh(live, fresh, tag); }
    CHECK(childCodes(live) == codes && invertedSlots(live) == inverted, "topology, child codes and the inverted boxes of unused slots are unchanged");
    CHECK(!sameBytes(live.nodes, first.nodes) && !sameBytes(live.instancesD, first.inst), "the edit changes boxes and instance records");
    CHECK(sameBytes(live.groupBoxes, first.groupBoxes) == (verts == 0), "the group boxes follow the vertices");
    for (size_t i = 0; i < first.inst.size(); ++i) CHECK(live.instancesD[i].root == first.inst[i].root && live.instancesD[i].group == first.inst[i].group, "root and group stay");
    CHECK(live.refitOrderAll.size() == live.nodes.size() && live.refitOrder.size() < live.nodes.size(), "the full order names every node once, the scene-level order fewer");
    { std::vector<uint8_t> seen(live.nodes.size(), 0); bool once = true; for (uint32_t n : live.refitOrderAll) { once = once && n < seen.size() && !seen[n]; if (n < seen.size()) seen[n] = 1; } CHECK(once, "no node twice in the full order"); }
    enclosed(live, tag);
    // the same edit again without a refresh in between, then back to the first description: every table as committed (a refit that only grows boxes fails here)
    CHECK(geometryCall(live, verts, inst, verts != 0, inst != 0, msg) == MI_OK && geometryCall(live, 0, 0, verts != 0, inst != 0, msg) == MI_OK, "updateGeometry back");
    live.refreshHostGeometry();
    CHECK(live.revision == 3 && live.treeBuilds == 1, "three edits, one tree build");
    CHECK(first.equals(live), "back: nodes, leaf records, shading records, instance records, group boxes, scene box");
    { SceneHost fresh; fillFrom(fresh, 0, 0); compareFresh(live, fresh, "back"); CHECK(sameBytes(live.nodes, fresh.nodes) && sameBytes(live.tris, fresh.tris) && sameBytes(live.instancesD, fresh.instancesD), "back: the trees are the fresh scene's trees"); }
    enclosed(live, "back");
    // recommit on the same object: the edit state of the old trees must be gone, and an edit of the new trees works
    CHECK(geometryCall(live, 1, 1, true, true, msg) == MI_OK && live.instStale && live.geoStale, "edit before the recommit");
    live.commitHost();
    CHECK(live.treeBuilds == 2 && !live.instStale && !live.geoStale && !live.geoPrepared && live.refitOrderAll.empty() && live.refitLevelStartAll.empty() && live.refitOrder.empty() && live.leafBoxes.empty() && live.nodeBoxes.empty(), "a commit drops the edit state of the previous trees");
    for (int i = 0; i < 3; ++i) { live.d.aabb_lo[i] = live.aabbLo[i]; live.d.aabb_hi[i] = live.aabbHi[i]; } live.syncCameraD(); live.syncEmittersD();
    { SceneHost fresh; fillFrom(fresh, 1, 1); const Snapshot committed(live); live.refreshHostGeometry(); CHECK(committed.equals(live) && sameBytes(live.nodes, fresh.nodes) && sameBytes(live.instancesD, fresh.instancesD), "the recommitted tables are the fresh scene's"); }
    CHECK(geometryCall(live, 0, 0, true, true, msg) == MI_OK, "edit after the recommit"); live.refreshHostGeometry();
    { SceneHost fresh; fillFrom(fresh, 0, 0); compareFresh(live, fresh, "after the recommit"); } enclosed(live, "after the recommit");
}

// any interleaving of the three geometry calls ends in the tables of the single combined call
static void interleavings(const char *kind) {
    const Verts VB = vertices(1), VA = vertices(0); const std::vector<mi_instance> IB = placement(1), IA = placement(0); const uint32_t nv = (uint32_t) (VB.pos.size() / 3), ni = (uint32_t) IB.size(); std::string msg;
    SceneHost one; fillFrom(one, 0, 0); CHECK(one.updateGeometry(VB.pos.data(), VB.nrm.data(), nv, IB.data(), ni, msg) == MI_OK, "the combined call"); one.refreshHostGeometry();
    for (int refreshBetween = 0; refreshBetween < 2; ++refreshBetween) {
        {   SceneHost h; fillFrom(h, 0, 0);      // instances (old call) -> geometry (vertices only)
            CHECK(h.updateInstances(IB.data(), ni, msg) == MI_OK, "updateInstances"); if (refreshBetween) h.refreshHostGeometry();
            CHECK(h.updateGeometry(VB.pos.data(), VB.nrm.data(), nv, nullptr, 0, msg) == MI_OK && h.revision == 2, "updateGeometry after updateInstances"); h.refreshHostGeometry();
            if (!sameTables(h, one)) { std::printf("FAIL [%s] instances -> geometry (refresh between: %d) differs from the combined call\n", kind, refreshBetween); ++g_failed; }
            enclosed(h, "instances -> geometry"); }
        {   SceneHost h; fillFrom(h, 0, 0);      // geometry (vertices only) -> instances (old call)
            CHECK(h.updateGeometry(VB.pos.data(), VB.nrm.data(), nv, nullptr, 0, msg) == MI_OK, "updateGeometry"); if (refreshBetween) h.refreshHostGeometry();
            CHECK(h.updateInstances(IB.data(), ni, msg) == MI_OK && h.revision == 2, "updateInstances after updateGeometry"); h.refreshHostGeometry();
            if (!sameTables(h, one)) { std::printf("FAIL [%s] geometry -> instances (refresh between: %d) differs from the combined call\n", kind, refreshBetween); ++g_failed; }
            enclosed(h, "geometry -> instances"); }
        {   SceneHost h; fillFrom(h, 0, 0);      // geometry (instances only) -> geometry (vertices only) -> both back, against a scene never edited
            CHECK(h.updateGeometry(nullptr, nullptr, 0, IB.data(), ni, msg) == MI_OK, "updateGeometry, instances"); if (refreshBetween) h.refreshHostGeometry();
            CHECK(h.updateGeometry(VB.pos.data(), VB.nrm.data(), nv, nullptr, 0, msg) == MI_OK, "updateGeometry, vertices"); h.refreshHostGeometry();
            if (!sameTables(h, one)) { std::printf("FAIL [%s] two geometry calls (refresh between: %d) differ from the combined call\n", kind, refreshBetween); ++g_failed; }
            CHECK(h.updateInstances(IA.data(), ni, msg) == MI_OK, "instances back"); if (refreshBetween) h.refreshHostGeometry();
            CHECK(h.updateGeometry(VA.pos.data(), VA.nrm.data(), nv, nullptr, 0, msg) == MI_OK, "vertices back"); h.refreshHostGeometry();
            SceneHost never; fillFrom(never, 0, 0); CHECK(sameTables(h, never), "back through both calls: the committed tables"); }
    }
    {   // a copy taken mid-sequence, as mi_scene_clone takes it (after refreshHostGeometry()): its first edit finds the edit state prepared; the source keeps its tables
        SceneHost h; fillFrom(h, 0, 0);
        CHECK(h.updateGeometry(VB.pos.data(), VB.nrm.data(), nv, nullptr, 0, msg) == MI_OK && h.updateInstances(IB.data(), ni, msg) == MI_OK, "two edits before the copy"); h.refreshHostGeometry();
        SceneHost twin(h); CHECK(twin.geoPrepared && !twin.geoStale && !twin.instStale && twin.revision == 2, "the copy carries the edit state");
        CHECK(twin.updateGeometry(VA.pos.data(), VA.nrm.data(), nv, IA.data(), ni, msg) == MI_OK && twin.revision == 3 && h.revision == 2, "the copy's edit advances its own revision"); twin.refreshHostGeometry();
        SceneHost never; fillFrom(never, 0, 0); CHECK(sameTables(twin, never), "the edited copy holds the committed tables"); enclosed(twin, "edited copy");
        CHECK(sameTables(h, one), "the source of the copy keeps its tables"); }
    // a scene without instances and without groups: updateGeometry(vertices) is updateVertices, packet tables included, and the two mix
    {   SceneHost a, b; fillFrom(a, 0, 0, false); fillFrom(b, 0, 0, false);
        CHECK(a.updateVertices(VB.pos.data(), VB.nrm.data(), nv, msg) == MI_OK && b.updateGeometry(VB.pos.data(), VB.nrm.data(), nv, nullptr, 0, msg) == MI_OK, "both calls on a scene without instances");
        CHECK(a.geoStale && b.geoStale && !b.instStale && a.revision == 1 && b.revision == 1, "stale marks of a vertex edit");
        a.refreshHostGeometry(); b.refreshHostGeometry();
        CHECK(sameTables(a, b) && !std::memcmp(a.packetGK, b.packetGK, 12) && !std::memcmp(&a.packetScale, &b.packetScale, 4) && !std::memcmp(a.d.packet_gk, b.d.packet_gk, 12) && !std::memcmp(&a.d.packet_scale, &b.d.packet_scale, 4), "updateGeometry(vertices) = updateVertices on a scene without instances");
        { SceneHost fresh; fillFrom(fresh, 1, 0, false); compareFresh(b, fresh, "no instances"); } enclosed(b, "no instances");
        CHECK(a.updateGeometry(VA.pos.data(), VA.nrm.data(), nv, nullptr, 0, msg) == MI_OK && b.updateVertices(VA.pos.data(), VA.nrm.data(), nv, msg) == MI_OK, "back through the other call");
        a.refreshHostGeometry(); b.refreshHostGeometry(); SceneHost never; fillFrom(never, 0, 0, false);
        CHECK(sameTables(a, b) && sameTables(a, never), "mixed calls on a scene without instances end in the committed tables");
        CHECK(b.updateGeometry(nullptr, nullptr, 0, IB.data(), ni, msg) == MI_ERR_INVALID && msg.find("mi_scene_update_geometry: ") == 0 && msg.find("the scene has no instances") != std::string::npos && b.revision == 2, "instances on a scene without instances"); }
}

int main() {
    for (int wide = 0; wide < 2; ++wide) {
        setenv("MI355PT_BVH2", wide ? "0" : "1", 1); const char *kind = wide ? "4-wide nodes" : "binary nodes";
        { SceneHost h; fillFrom(h, 0, 0); CHECK(h.wideBvh == (wide != 0), "MI355PT_BVH2 selects the node kind"); }
        editCycle(kind, 1, 0); editCycle(kind, 0, 1); editCycle(kind, 1, 1);
        interleavings(kind);
    }
    // refusals: each names the function, leaves the scene as it was and counts nothing
    {
        setenv("MI355PT_BVH2", "1", 1);
        const Verts VA = vertices(0); const std::vector<mi_instance> A = placement(0); SceneHost h; fillFrom(h, 0, 0); const Snapshot first(h); std::string msg; const uint32_t n = (uint32_t) A.size(), nv = (uint32_t) (VA.pos.size() / 3);
        auto refused = [&](int rc, int code, const char *word) {
            if (rc != code || msg.find("mi_scene_update_geometry: ") != 0 || msg.find(word) == std::string::npos) { std::printf("FAIL refusal \"%s\": rc %d, message \"%s\"\n", word, rc, msg.c_str()); ++g_failed; }
            CHECK(first.equals(h) && h.revision == 0 && h.treeBuilds == 1 && !h.instStale && !h.geoStale && sameBytes(h.pos, VA.pos) && sameBytes(h.nrm, VA.nrm) && !std::memcmp(h.instances.data(), A.data(), A.size() * sizeof(mi_instance)), "a refused edit leaves the scene untouched");
        };
        refused(h.updateGeometry(nullptr, nullptr, 0, nullptr, 0, msg), MI_ERR_INVALID, "null");
        refused(h.updateGeometry(nullptr, VA.nrm.data(), nv, nullptr, 0, msg), MI_ERR_INVALID, "null");
        refused(h.updateGeometry(nullptr, nullptr, 0, nullptr, n, msg), MI_ERR_INVALID, "null");
        refused(h.updateGeometry(VA.pos.data(), VA.nrm.data(), nv - 1, nullptr, 0, msg), MI_ERR_INVALID, "18 -> 17");
        refused(h.updateGeometry(VA.pos.data(), nullptr, nv, nullptr, 0, msg), MI_ERR_INVALID, "normals are required");
        { Verts b = VA; b.pos[3 * 9 + 1] = std::nanf(""); refused(h.updateGeometry(b.pos.data(), b.nrm.data(), nv, A.data(), n, msg), MI_ERR_INVALID, "vertex 9"); }
        { Verts b = VA; b.nrm[3 * 13] = std::numeric_limits<float>::infinity(); refused(h.updateGeometry(b.pos.data(), b.nrm.data(), nv, nullptr, 0, msg), MI_ERR_INVALID, "vertex 13"); }
        refused(h.updateGeometry(nullptr, nullptr, 0, A.data(), n - 1, msg), MI_ERR_INVALID, "7 -> 6");
        refused(h.updateGeometry(VA.pos.data(), VA.nrm.data(), nv, A.data(), n + 1, msg), MI_ERR_INVALID, "7 -> 8");
        { std::vector<mi_instance> b = A; b[5].group = 0; b[6].group = 1; refused(h.updateGeometry(VA.pos.data(), VA.nrm.data(), nv, b.data(), n, msg), MI_ERR_UNSUPPORTED, "instance 5"); }
        { std::vector<mi_instance> b = A; b[3].to_object[11] = std::nanf(""); refused(h.updateGeometry(nullptr, nullptr, 0, b.data(), n, msg), MI_ERR_INVALID, "instance 3"); CHECK(msg.find("to_object") != std::string::npos, "the message names to_object"); }
        { SceneHost raw; raw.pos = VA.pos; raw.instances = A; CHECK(raw.updateGeometry(VA.pos.data(), nullptr, nv, A.data(), n, msg) == MI_ERR_INVALID && msg.find("mi_scene_update_geometry: ") == 0 && msg.find("not committed") != std::string::npos, "a scene that is not committed"); }
        { SceneHost noNormals; Verts v = VA; fill(noNormals, v, A); noNormals.nrm.clear();      // (the tables are not used: only the rule "normals given if and only if committed")
          CHECK(noNormals.updateGeometry(VA.pos.data(), VA.nrm.data(), nv, nullptr, 0, msg) == MI_ERR_INVALID && msg.find("mi_scene_update_geometry: ") == 0 && msg.find("without normals") != std::string::npos && noNormals.revision == 0, "normals for a scene committed without"); }
        // the older call keeps its refusal of instanced scenes, by code and message
        CHECK(h.updateVertices(h.pos.data(), h.nrm.data(), nv, msg) == MI_ERR_UNSUPPORTED && msg.find("mi_scene_update_vertices: ") == 0 && msg.find("instance 0") != std::string::npos, "mi_scene_update_vertices still refuses instanced scenes");
    }
    std::printf(g_failed ? "group_edit_host: %d check(s) FAILED\n" : "group_edit_host: all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
