// geometry_edit_host.cpp -- stand-alone check of the host side of mi_scene_update_vertices (SceneHost::updateVertices / refreshHostGeometry,
// mitsuba-im_amd/csrc/scene_build.cpp over geometry_records.h -- the header the device kernels of kernels_geometry.hip are made of).
// Built and run by tests/test_geometry_edit.py with the address and undefined-behaviour sanitizers; links scene_build.cpp only and makes no device call.
//
// Scenes: (i) a 32-triangle packet scene (4 x 4 separate quads, the last one a light) whose edit bends the quads, so the pass-1 pairs dissolve and the group count
// grows; (ii) a wavy sheet of 32 x 32 quads (2048 triangles) with vertex normals and texture coordinates, a two-triangle area light and an analytic sphere, built with
// binary and with 4-wide nodes.  The edit gives the sheet another wave, lifts it above the old scene box and moves and shrinks the light.  After the edit every
// derived table must equal, byte for byte, that of a scene committed from scratch on the new vertices (leaf records looked up by primitive: the trees differ by
// design), the tree keeps its topology and stays conservative, and the edit back restores every table.
#include "../../mitsuba-im_amd/csrc/scene_host.h"
#include "../../mitsuba-im_amd/csrc/geometry_records.h"
#include <algorithm>
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

struct Geo { std::vector<float> pos, nrm, uv; std::vector<uint32_t> idx; std::vector<mi_shape> shapes; bool sphere = false; };
static void vertex(Geo &g, float x, float y, float z) { g.pos.push_back(x); g.pos.push_back(y); g.pos.push_back(z); }
static void quadIdx(Geo &g, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { const uint32_t t[6] = {a, b, c, a, c, d}; g.idx.insert(g.idx.end(), t, t + 6); }

// (i) 16 quads with four vertices of their own each; bend = 0: flat parallelograms (16 pairs), bend > 0: every vertex gets a height of its own
static Geo packetGeo(float bend) {
    Geo g;
    for (int q = 0; q < 16; ++q) {
        const float x = (float) (q % 4) * 1.25f - 2.5f, z = (float) (q / 4) * 1.25f - 2.5f, y = q == 15 ? 2.0f : 0.0f;
        for (int c = 0; c < 4; ++c) {
            const float dx = (c == 1 || c == 2) ? 1.0f : 0.0f, dz = c >= 2 ? 1.0f : 0.0f;
            vertex(g, x + dx + bend * 0.1f * (float) q, y + bend * std::sin((float) (q * 4 + c) * 1.7f), z + dz);
        }
        quadIdx(g, q * 4, q * 4 + 1, q * 4 + 2, q * 4 + 3);
    }
    g.shapes = {mi_shape{0, 30, 0, 60, 0, -1, 1, 0}, mi_shape{30, 2, 60, 4, 1, 0, 1, 0}};
    return g;
}
// (ii) the sheet y = lift + amp sin(3 x + phase) cos(2 z) over [-1, 1]^2, n x n quads on a shared (n + 1)^2 grid with analytic normals and uv = grid coordinates;
// a light quad above it, scaled and shifted
static Geo sheetGeo(int n, float phase, float amp, float lift, float lightSize, float lightX) {
    Geo g; g.sphere = true;
    for (int j = 0; j <= n; ++j) for (int i = 0; i <= n; ++i) {
        const float u = (float) i / (float) n, v = (float) j / (float) n, x = 2 * u - 1, z = 2 * v - 1;
        vertex(g, x, lift + amp * std::sin(3 * x + phase) * std::cos(2 * z), z);
        const float dydx = amp * 3 * std::cos(3 * x + phase) * std::cos(2 * z), dydz = -amp * 2 * std::sin(3 * x + phase) * std::sin(2 * z), l = std::sqrt(dydx * dydx + 1 + dydz * dydz);
        g.nrm.push_back(-dydx / l); g.nrm.push_back(1 / l); g.nrm.push_back(-dydz / l);
        g.uv.push_back(u * 4); g.uv.push_back(i == n / 2 ? u * 4 : v * 4);      // one grid column with u == v on both of its vertices' rows: some triangles get a zero determinant
    }
    for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) { const uint32_t a = (uint32_t) (j * (n + 1) + i); quadIdx(g, a, a + 1, a + (uint32_t) n + 2, a + (uint32_t) n + 1); }
    const uint32_t nv = (uint32_t) ((n + 1) * (n + 1)), nt = (uint32_t) (2 * n * n);
    const float h = lift + 1.5f;
    vertex(g, lightX - lightSize, h, -lightSize); vertex(g, lightX + lightSize, h, -lightSize); vertex(g, lightX + lightSize, h, lightSize); vertex(g, lightX - lightSize, h, lightSize);
    for (int c = 0; c < 4; ++c) { g.nrm.push_back(0); g.nrm.push_back(-1); g.nrm.push_back(0); g.uv.push_back(0); g.uv.push_back(0); }
    quadIdx(g, nv, nv + 3, nv + 2, nv + 1);      // facing down
    g.shapes = {mi_shape{0, nt, 0, nv, 0, -1, 2, 0}, mi_shape{nt, 2, nv, 4, 1, 0, 1, 0}};      // the sheet: smooth, with texture coordinates; the light: face normals
    return g;
}
static void fill(SceneHost &h, const Geo &g) {
    h.pos = g.pos; h.nrm = g.nrm; h.uv = g.uv; h.idx = g.idx; h.shapes = g.shapes;
    if (g.sphere) {
        mi_analytic sph{}; sph.type = MI_SHAPE_SPHERE; sph.bsdf = 0; sph.emitter = -1; identity(sph.to_world); identity(sph.to_object); sph.radius = 0.3f;
        sph.to_world[3] = 0.2f; sph.to_world[7] = 0.9f; sph.to_object[3] = -0.2f; sph.to_object[7] = -0.9f; h.analytic = {sph};
    }
    mi_material m{}; m.type = MI_BSDF_DIFFUSE; m.reflectance[0] = m.reflectance[1] = m.reflectance[2] = 0.5f; h.materials = {m, m};
    mi_emitter e{}; e.type = MI_EMITTER_AREA; e.shape = 1; e.weight = 1; e.radiance[0] = e.radiance[1] = e.radiance[2] = 10; identity(e.to_world); h.emitters = {e};
    identity(h.s2c); h.s2c[0] = 0.8f; h.s2c[5] = 0.6f; h.s2c[3] = -0.4f; h.s2c[7] = -0.3f; h.s2c[11] = 1.0f;
    identity(h.c2w); h.c2w[3] = 0.2f; h.c2w[7] = 1.0f; h.c2w[11] = -4.5f; h.nearClip = 0.1f; h.farClip = 100.0f; h.haveCamera = true;
    h.width = 16; h.height = 12; h.filterKind = 0; h.haveFilm = true;
    h.commitHost();
    h.d = DScene{}; h.committed = true;       // upload() without a device: the parts of the scene record the edits maintain
    for (int i = 0; i < 3; ++i) { h.d.aabb_lo[i] = h.aabbLo[i]; h.d.aabb_hi[i] = h.aabbHi[i]; h.d.packet_gk[i] = h.packetGK[i]; }
    h.d.packet_scale = h.packetScale; h.syncCameraD(); h.syncEmittersD(); h.syncEnvD();
}
template <typename T> static bool sameBytes(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T))); }

// every table a vertex edit is responsible for, against a fresh commit
static void compareFresh(const SceneHost &a, const SceneHost &b, const char *tag) {
    auto ck = [&](bool ok, const char *what) { if (!ok) { std::printf("FAIL [%s] %s differs from a fresh commit\n", tag, what); ++g_failed; } };
    ck(a.tris.size() == b.tris.size(), "leaf record count");
    std::vector<const TriAccelD *> byPrim(a.nTris + a.analytic.size(), nullptr);
    for (const TriAccelD &r : b.tris) if (r.prim < byPrim.size()) byPrim[r.prim] = &r;
    size_t seen = 0, bad = 0;
    for (const TriAccelD &r : a.tris) { if (r.prim >= byPrim.size()) continue; ++seen; if (!byPrim[r.prim] || std::memcmp(&r, byPrim[r.prim], sizeof(r))) ++bad; }
    ck(seen == byPrim.size() && bad == 0, "TriAccelD leaf records (by prim)");
    ck(sameBytes(a.shade, b.shade), "TriShade"); ck(sameBytes(a.triuv, b.triuv), "TriUV"); ck(sameBytes(a.packetExact, b.packetExact), "packetExact");
    ck(sameBytes(a.packetGroups, b.packetGroups), "packetGroups"); ck(!std::memcmp(a.packetGK, b.packetGK, 12) && !std::memcmp(&a.packetScale, &b.packetScale, 4), "packetGK / packetScale");
    ck(!std::memcmp(a.aabbLo, b.aabbLo, 12) && !std::memcmp(a.aabbHi, b.aabbHi, 12), "scene AABB");
    ck(!std::memcmp(a.envBsCenter, b.envBsCenter, 12) && !std::memcmp(&a.envBsRadius, &b.envBsRadius, 4), "env bounding sphere");
    ck(!std::memcmp(a.dirBsCenter, b.dirBsCenter, 12) && !std::memcmp(&a.dirBsRadius, &b.dirBsRadius, 4), "directional bounding sphere");
    ck(sameBytes(a.emittersD, b.emittersD), "emittersD"); ck(sameBytes(a.areaCdf, b.areaCdf), "areaCdf"); ck(sameBytes(a.emitterCdf, b.emitterCdf), "emitterCdf");
    ck(sameBytes(a.analyticD, b.analyticD), "analyticD"); ck(sameBytes(a.pos, b.pos) && sameBytes(a.nrm, b.nrm), "pos / nrm");
    ck(!std::memcmp(a.d.aabb_lo, b.d.aabb_lo, 12) && !std::memcmp(a.d.aabb_hi, b.d.aabb_hi, 12), "d.aabb");
    ck(!std::memcmp(a.d.packet_gk, b.d.packet_gk, 12) && !std::memcmp(&a.d.packet_scale, &b.d.packet_scale, 4), "d.packet_gk / d.packet_scale");
    ck(!std::memcmp(a.d.dir_bs_center, b.d.dir_bs_center, 12) && !std::memcmp(&a.d.dir_bs_radius, &b.d.dir_bs_radius, 4), "d directional bounding sphere");
    ck(!std::memcmp(a.d.env_bs_center, b.d.env_bs_center, 12) && !std::memcmp(&a.d.env_bs_radius, &b.d.env_bs_radius, 4), "d env bounding sphere");
}
struct Snapshot {
    std::vector<TriAccelD> tris, packetExact; std::vector<TriShade> shade; std::vector<TriUV> triuv; std::vector<BvhNode> nodes; std::vector<PacketGroupD> groups; std::vector<EmitterD> emittersD; std::vector<float> areaCdf;
    float aabb[6], scale; uint32_t gk[3];
    explicit Snapshot(const SceneHost &h) : tris(h.tris), packetExact(h.packetExact), shade(h.shade), triuv(h.triuv), nodes(h.nodes), groups(h.packetGroups), emittersD(h.emittersD), areaCdf(h.areaCdf) {
        std::memcpy(aabb, h.aabbLo, 12); std::memcpy(aabb + 3, h.aabbHi, 12); scale = h.packetScale; std::memcpy(gk, h.packetGK, 12); }
};
static std::vector<int32_t> childCodes(const SceneHost &h) {
    std::vector<int32_t> c;
    for (const BvhNode &n : h.nodes) { if (h.wideBvh) { Bvh4Node w; std::memcpy(&w, &n, sizeof(w)); c.insert(c.end(), w.child, w.child + 4); } else { c.push_back(n.c0); c.push_back(n.c1); } }
    return c;
}
// Every node's child box -- for 4-wide nodes the float reconstruction org + q * step the walks compute -- encloses the padded boxes of all primitives below it.
struct Enclose {
    const SceneHost &h; std::vector<V3> plo, phi; size_t violations = 0, leaves = 0;
    explicit Enclose(const SceneHost &hh) : h(hh) {
        const size_t np = h.nTris + h.analytic.size(); plo.resize(np); phi.resize(np);
        for (uint32_t t = 0; t < h.nTris; ++t) { V3 c; mi::triPaddedBox(mi::load3(&h.pos[(size_t) h.idx[t * 3] * 3]), mi::load3(&h.pos[(size_t) h.idx[t * 3 + 1] * 3]), mi::load3(&h.pos[(size_t) h.idx[t * 3 + 2] * 3]), plo[t], phi[t], c); }
        for (size_t slot = 0; slot < h.tris.size(); ++slot) if (h.tris[slot].k == MI_K_ANALYTIC) { plo[h.tris[slot].prim] = mi::load3(&h.leafBoxes[slot * 6]); phi[h.tris[slot].prim] = mi::load3(&h.leafBoxes[slot * 6 + 3]); }
    }
    void below(int32_t code, V3 &lo, V3 &hi) {      // exact union of the padded primitive boxes under a child code; checks the subtree on the way
        const float inf = std::numeric_limits<float>::infinity(); lo = mi::mk(inf, inf, inf); hi = mi::mk(-inf, -inf, -inf);
        if (code < 0) {
            const uint32_t leaf = (uint32_t) ~code, first = leaf >> 3, count = (leaf & 7u) + 1u; ++leaves;
            for (uint32_t i = 0; i < count; ++i) { const uint32_t p = h.tris[first + i].prim; if (p < plo.size()) { lo = mi::vmin(lo, plo[p]); hi = mi::vmax(hi, phi[p]); } }
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

static void editCycle(const Geo &A, const Geo &B, const char *tag, bool expectLevels) {
    SceneHost live; fill(live, A);
    CHECK(live.treeBuilds == 1 && live.revision == 0, "one tree build, no edit yet");
    const Snapshot before(live); const std::vector<int32_t> codes = childCodes(live); std::string msg;
    const float topBefore = live.aabbHi[1];
    CHECK(live.updateVertices(B.pos.data(), B.nrm.empty() ? nullptr : B.nrm.data(), (uint32_t) (B.pos.size() / 3), msg) == MI_OK, "updateVertices"); if (!msg.empty()) std::printf("  %s\n", msg.c_str());
    CHECK(live.geoStale && live.revision == 1 && live.treeBuilds == 1, "an edit advances the revision, marks the mirrors stale and builds no tree");
    live.refreshHostGeometry(); CHECK(!live.geoStale, "refreshHostGeometry() clears the stale mark");
    { SceneHost fresh; fill(fresh, B); compareFresh(live, fresh, tag); if (A.sphere) CHECK(live.aabbHi[1] > topBefore + 0.5f, "the edit lifts the geometry above the old scene box"); }
    CHECK(childCodes(live) == codes && live.nodes.size() == before.nodes.size(), "every child code is unchanged");
    CHECK(!sameBytes(live.nodes, before.nodes) && !sameBytes(live.shade, before.shade), "the edit changes the node boxes and the records");
    { Enclose e(live); V3 lo, hi; e.below(0, lo, hi); if (e.violations) std::printf("  [%s] %zu child boxes do not enclose their primitives\n", tag, e.violations); CHECK(e.violations == 0 && e.leaves > 0, "every child box encloses the padded boxes below it"); }
    if (expectLevels) CHECK(live.refitLevelStart.size() >= 4, "the tree has several levels of inner nodes");
    CHECK(live.refitOrder.size() == live.nodes.size(), "every node is refitted");
    // ... and back: every table as committed
    CHECK(live.updateVertices(A.pos.data(), A.nrm.empty() ? nullptr : A.nrm.data(), (uint32_t) (A.pos.size() / 3), msg) == MI_OK, "updateVertices back");
    live.refreshHostGeometry();
    CHECK(live.revision == 2 && live.treeBuilds == 1, "two edits, one tree build");
    const Snapshot after(live);
    CHECK(sameBytes(after.tris, before.tris), "back: leaf records"); CHECK(sameBytes(after.shade, before.shade), "back: TriShade"); CHECK(sameBytes(after.triuv, before.triuv), "back: TriUV");
    CHECK(sameBytes(after.packetExact, before.packetExact), "back: packetExact"); CHECK(sameBytes(after.nodes, before.nodes), "back: nodes"); CHECK(sameBytes(after.groups, before.groups), "back: packetGroups");
    CHECK(sameBytes(after.emittersD, before.emittersD) && sameBytes(after.areaCdf, before.areaCdf), "back: emitter tables");
    CHECK(!std::memcmp(after.aabb, before.aabb, 24) && !std::memcmp(&after.scale, &before.scale, 4) && !std::memcmp(after.gk, before.gk, 12), "back: AABB, packetScale, packetGK");
    { SceneHost fresh; fill(fresh, A); compareFresh(live, fresh, "back"); }
}

// edit, commit again on the same object, edit: the second commit builds another tree (for other vertices), so everything the first edit derived from the old tree --
// slot table, level order, box scratch, the stale mark -- must be gone; what mi_scene_clone does after a recommit (refreshHostGeometry) must leave the new mirrors alone
static void recommitCycle(const Geo &A, const Geo &B, const char *tag) {
    SceneHost live; fill(live, A); std::string msg;
    CHECK(live.updateVertices(B.pos.data(), B.nrm.empty() ? nullptr : B.nrm.data(), (uint32_t) (B.pos.size() / 3), msg) == MI_OK && live.geoStale && live.geoPrepared, "first edit");
    live.pos = B.pos; live.nrm = B.nrm; live.commitHost();      // mi_scene_set_triangles + mi_scene_commit with the edited vertices, without a refresh in between
    CHECK(live.treeBuilds == 2 && !live.geoStale && !live.geoPrepared && live.leafSlotOfPrim.empty() && live.refitOrder.empty() && live.refitLevelStart.empty() && live.leafBoxes.empty() && live.nodeBoxes.empty(),
          "a commit drops the vertex-edit state of the previous tree");
    for (int i = 0; i < 3; ++i) { live.d.aabb_lo[i] = live.aabbLo[i]; live.d.aabb_hi[i] = live.aabbHi[i]; live.d.packet_gk[i] = live.packetGK[i]; }
    live.d.packet_scale = live.packetScale; live.syncCameraD(); live.syncEmittersD();
    { const Snapshot committed(live); live.refreshHostGeometry(); const Snapshot now(live);      // the clone's call
      CHECK(sameBytes(now.tris, committed.tris) && sameBytes(now.shade, committed.shade) && sameBytes(now.nodes, committed.nodes) && sameBytes(now.packetExact, committed.packetExact), "a refresh right after a commit changes nothing");
      SceneHost fresh; fill(fresh, B); compareFresh(live, fresh, "recommitted"); CHECK(sameBytes(live.nodes, fresh.nodes), "the recommitted tree is the fresh scene's tree"); }
    const std::vector<int32_t> codes = childCodes(live);
    CHECK(live.updateVertices(A.pos.data(), A.nrm.empty() ? nullptr : A.nrm.data(), (uint32_t) (A.pos.size() / 3), msg) == MI_OK, "edit after the recommit");
    live.refreshHostGeometry();
    CHECK(live.treeBuilds == 2 && live.refitOrder.size() == live.nodes.size() && childCodes(live) == codes, "the second edit refits the second tree");
    { SceneHost fresh; fill(fresh, A); compareFresh(live, fresh, tag); }
    { Enclose e(live); V3 lo, hi; e.below(0, lo, hi); if (e.violations) std::printf("  [%s] %zu child boxes do not enclose their primitives\n", tag, e.violations); CHECK(e.violations == 0 && e.leaves > 0, "after a recommit every child box encloses the padded boxes below it"); }
}

// The shared header restates three pieces of the builder in a form the device compiles too.  Pin them against the builder's original wording (scene_build.cpp before
// the header existed): the step exponent against std::frexp, the step against std::ldexp, triaccelLoad against the memset / wald[] table version.
static int builderStepExponent(float ext) { int e = 0; std::frexp(ext > 0 ? ext / 254.0f : 1e-30f, &e); return std::min(std::max(e + 127, 1), 254); }
static void builderTriaccelLoad(TriAccelD &ta, V3 A, V3 B, V3 C) {
    static const int wald[4] = {1, 2, 0, 1};
    V3 b = C - A, c = B - A, N = mi::cross(c, b);
    int k = 0;
    for (int j = 0; j < 3; ++j) if (std::fabs(mi::comp(N, j)) > std::fabs(mi::comp(N, k))) k = j;
    int u = wald[k], v = wald[k + 1];
    float n_k = mi::comp(N, k), denom = mi::comp(b, u) * mi::comp(c, v) - mi::comp(b, v) * mi::comp(c, u);
    std::memset(&ta, 0, sizeof(ta));
    if (denom == 0) { ta.k = 3; return; }
    ta.k = (uint32_t) k;
    ta.n_u = mi::comp(N, u) / n_k; ta.n_v = mi::comp(N, v) / n_k; ta.n_d = mi::dot(A, N) / n_k;
    ta.b_nu = mi::comp(b, u) / denom; ta.b_nv = -mi::comp(b, v) / denom;
    ta.a_u = mi::comp(A, u); ta.a_v = mi::comp(A, v);
    ta.c_nu = mi::comp(c, v) / denom; ta.c_nv = -mi::comp(c, u) / denom;
}
static void restatementsEqualTheBuilder() {
    size_t bad = 0, n = 0;
    auto one = [&](float ext) { ++n; if (mi::wideStepExponent(ext) != builderStepExponent(ext)) { if (!bad) { uint32_t b; std::memcpy(&b, &ext, 4); std::printf("  step exponent differs for extent bits %08x\n", b); } ++bad; } };
    for (uint32_t E = 0; E < 256; ++E) for (uint32_t m : {0u, 1u, 0x3FFFFFu, 0x400000u, 0x7E0000u, 0x7EFFFFu, 0x7F0000u, 0x7FFFFFu}) for (uint32_t sgn : {0u, 0x80000000u}) {   // every exponent, both signs: zeros, subnormals, the mantissas around 254 / 256, infinities, NaNs
        const uint32_t bits = sgn | (E << 23) | m; float x; std::memcpy(&x, &bits, 4); one(x); }
    uint32_t r = 12345u; for (int i = 0; i < 200000; ++i) { r = r * 1664525u + 1013904223u; float x; const uint32_t bits = r & 0x7FFFFFFFu; std::memcpy(&x, &bits, 4); one(x); }
    CHECK(bad == 0 && n > 200000, "wideStepExponent == the builder's frexp rule for every kind of extent");
    bool stepsOk = true; for (int e = 1; e <= 254; ++e) { const float a = mi::wideStepOf(e), b = std::ldexp(1.0f, e - 127); if (std::memcmp(&a, &b, 4)) stepsOk = false; }
    CHECK(stepsOk, "wideStepOf(e) == ldexp(1, e - 127) for 1 <= e <= 254");
    size_t tbad = 0; auto rnd = [&]() { r = r * 1664525u + 1013904223u; return ((float) (r >> 8) / 8388608.0f - 1.0f) * 3.0f; };
    for (int i = 0; i < 20000; ++i) {
        V3 A = mi::mk(rnd(), rnd(), rnd()), B = mi::mk(rnd(), rnd(), rnd()), C = mi::mk(rnd(), rnd(), rnd());
        if (i % 7 == 0) C = B; if (i % 11 == 0) { A.y = B.y = C.y = 0.5f; } if (i % 13 == 0) C = A + (B - A) * 2.0f;      // degenerate, axis-aligned, collinear
        TriAccelD x, y; std::memset(&x, 0xAB, sizeof(x)); std::memset(&y, 0xCD, sizeof(y)); mi::triaccelLoad(x, A, B, C); builderTriaccelLoad(y, A, B, C);
        if (std::memcmp(&x, &y, sizeof(x))) ++tbad;
    }
    CHECK(tbad == 0, "triaccelLoad == the builder's version, all 48 bytes");
}

int main() {
    // (i) the packet scene: pairs dissolve, the group table grows
    {
        const Geo A = packetGeo(0.0f), B = packetGeo(0.35f);
        { SceneHost a, b; fill(a, A); fill(b, B); CHECK(A.idx.size() == 96 && a.packetGK[2] == 16 && b.packetGK[2] > 16, "32 triangles: 16 pairs before the edit, more groups after"); }
        setenv("MI355PT_BVH2", "1", 1); editCycle(A, B, "packet scene", false);
    }
    // (ii) the wavy sheet, both node kinds
    {
        const Geo A = sheetGeo(32, 0.0f, 0.15f, 0.0f, 0.4f, 0.0f), B = sheetGeo(32, 1.3f, 0.3f, 2.5f, 0.2f, 0.5f);
        CHECK(A.idx.size() / 3 == 2050, "2048 sheet triangles and the light");
        setenv("MI355PT_BVH2", "1", 1); editCycle(A, B, "sheet, binary nodes", true);
        setenv("MI355PT_BVH2", "0", 1); editCycle(A, B, "sheet, 4-wide nodes", true);
        { SceneHost h; fill(h, A); CHECK(h.wideBvh, "MI355PT_BVH2=0 gives 4-wide nodes"); }
    }
    // edit, recommit on the same object, edit again -- with a tree of either kind, and on the packet scene
    {
        const Geo A = sheetGeo(32, 0.0f, 0.15f, 0.0f, 0.4f, 0.0f), B = sheetGeo(32, 1.3f, 0.3f, 2.5f, 0.2f, 0.5f);
        setenv("MI355PT_BVH2", "1", 1); recommitCycle(A, B, "recommit, binary nodes");
        setenv("MI355PT_BVH2", "0", 1); recommitCycle(A, B, "recommit, 4-wide nodes");
        setenv("MI355PT_BVH2", "1", 1); recommitCycle(packetGeo(0.0f), packetGeo(0.35f), "recommit, packet scene");
    }
    restatementsEqualTheBuilder();
    // refusals: each names the function, leaves the scene as it was and counts nothing
    {
        setenv("MI355PT_BVH2", "1", 1);
        const Geo A = sheetGeo(4, 0.0f, 0.15f, 0.0f, 0.4f, 0.0f); SceneHost h; fill(h, A); const Snapshot before(h); std::string msg; const uint32_t nv = (uint32_t) (A.pos.size() / 3);
        auto refused = [&](int rc, int code, const char *word) {
            if (rc != code || msg.find("mi_scene_update_vertices") != 0 || msg.find(word) == std::string::npos) { std::printf("FAIL refusal \"%s\": rc %d, message \"%s\"\n", word, rc, msg.c_str()); ++g_failed; }
            const Snapshot now(h); CHECK(sameBytes(now.shade, before.shade) && sameBytes(now.nodes, before.nodes) && h.pos == A.pos && h.nrm == A.nrm && h.revision == 0 && h.treeBuilds == 1 && !h.geoStale, "a refused edit leaves the scene untouched");
        };
        refused(h.updateVertices(nullptr, A.nrm.data(), nv, msg), MI_ERR_INVALID, "null");
        refused(h.updateVertices(A.pos.data(), A.nrm.data(), nv - 1, msg), MI_ERR_INVALID, "vertex count");
        refused(h.updateVertices(A.pos.data(), nullptr, nv, msg), MI_ERR_INVALID, "normals");
        { std::vector<float> p = A.pos; p[3 * 7 + 1] = std::numeric_limits<float>::infinity(); p[3 * 9] = std::nanf(""); refused(h.updateVertices(p.data(), A.nrm.data(), nv, msg), MI_ERR_INVALID, "vertex 7"); }
        { std::vector<float> n = A.nrm; n[3 * 5 + 2] = std::nanf(""); refused(h.updateVertices(A.pos.data(), n.data(), nv, msg), MI_ERR_INVALID, "vertex 5"); }
        { SceneHost raw; raw.pos = A.pos; CHECK(raw.updateVertices(A.pos.data(), nullptr, nv, msg) == MI_ERR_INVALID && msg.find("not committed") != std::string::npos, "a scene that is not committed"); }
        { const Geo P = packetGeo(0.0f); SceneHost p; fill(p, P); refused(p.updateVertices(P.pos.data(), P.pos.data(), 64, msg), MI_ERR_INVALID, "without normals"); }
        {   // a scene with a shape group and an instance
            Geo G = packetGeo(0.0f); G.shapes[0].group = 1; SceneHost gi; gi.instances.resize(1); gi.instances[0] = mi_instance{}; identity(gi.instances[0].to_world); identity(gi.instances[0].to_object); fill(gi, G);
            const int rc = gi.updateVertices(G.pos.data(), nullptr, 64, msg);
            CHECK(rc == MI_ERR_UNSUPPORTED && msg.find("mi_scene_update_vertices") == 0 && msg.find("instance 0") != std::string::npos && gi.revision == 0, "instances are refused by name");
        }
    }
    std::printf(g_failed ? "geometry_edit_host: %d check(s) FAILED\n" : "geometry_edit_host: all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
