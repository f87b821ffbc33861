// scene_build.cpp -- host side of mi_scene_commit: Wald triangle table, per-triangle shading records, emitter CDFs,
// reconstruction-filter table and a binned-SAH BVH2 laid out for the gfx950 traversal kernel.
//
// Replaces (reference): ShapeKDTree::build + TriAccel::load (src/librender/skdtree.cpp:68-105,
// include/mitsuba/render/triaccel.h:61-94), Scene::initialize's emitter PDF (src/librender/scene.cpp:383-388),
// TriMesh::prepareSamplingTable (src/librender/trimesh.cpp:389-402), ReconstructionFilter::configure
// (src/libcore/rfilter.cpp:37-56).  The kd-tree itself is NOT reproduced: the contract is the nearest hit
// (t, prim, u, v), not the tree layout.  Compiled with -ffp-contract=off: the values computed
// here feed the bit-exact parity tests.
#include "scene_host.h"
#include "geometry_records.h"      // V3, triaccelLoad, the per-triangle derivation, node quantisation: shared with the device (kernels_geometry.hip)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace mi {

// Analytic shapes: derived constants + Shape::getAABB (rectangle.cpp:100-119, disk.cpp:100-130, sphere.cpp:127-142, cylinder.cpp:105-107, :256-276); xfPoint: geometry_records.h
static inline V3 xfVector(const float *m, V3 v) { return mk(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z); }
static inline V3 xfNormal(const float *inv, V3 n) { return mk(inv[0] * n.x + inv[4] * n.y + inv[8] * n.z, inv[1] * n.x + inv[5] * n.y + inv[9] * n.z, inv[2] * n.x + inv[6] * n.y + inv[10] * n.z); }
static inline float length3(V3 a) { return std::sqrt(dot(a, a)); }
static void analyticPrepare(const mi_analytic &a, AnalyticD &d, V3 &lo, V3 &hi, V3 &tightLo, V3 &tightHi) {
    const float inf = std::numeric_limits<float>::infinity();
    std::memset(&d, 0, sizeof(d));
    std::memcpy(d.to_world, a.to_world, 48); std::memcpy(d.to_object, a.to_object, 48);
    d.type = a.type; d.radius = a.radius; d.length = a.length; d.material = a.bsdf; d.emitter = a.emitter;
    const float *M = a.to_world;
    lo = mk(inf, inf, inf); hi = mk(-inf, -inf, -inf);
    auto expand = [&](V3 q) { lo = vmin(lo, q); hi = vmax(hi, q); };
    V3 n = mk(0, 0, 0), dpdu = mk(0, 0, 0), center = mk(0, 0, 0);
    switch (a.type) {
    case MI_SHAPE_RECTANGLE: {
        dpdu = xfVector(M, mk(2, 0, 0)); V3 dpdv = xfVector(M, mk(0, 2, 0));
        n = normalize(xfNormal(a.to_object, mk(0, 0, 1)));
        d.inv_area = 1.0f / (length3(dpdu) * length3(dpdv));
        expand(xfPoint(M, mk(-1, -1, 0))); expand(xfPoint(M, mk(1, -1, 0))); expand(xfPoint(M, mk(1, 1, 0))); expand(xfPoint(M, mk(-1, 1, 0)));
        tightLo = lo; tightHi = hi; break;
    }
    case MI_SHAPE_DISK: {
        V3 du = xfVector(M, mk(1, 0, 0));
        n = normalize(xfNormal(a.to_object, mk(0, 0, 1)));
        d.inv_area = 1.0f / (MI_PI * length3(du) * length3(du));
        expand(xfPoint(M, mk(1, 0, 0))); expand(xfPoint(M, mk(-1, 0, 0))); expand(xfPoint(M, mk(0, 1, 0))); expand(xfPoint(M, mk(0, -1, 0)));
        // Disk::getAABB bounds four rim points only; the BVH needs the whole rim
        V3 c = xfPoint(M, mk(0, 0, 0)); float r = length3(du);
        tightLo = vmin(lo, c - mk(r, r, r)); tightHi = vmax(hi, c + mk(r, r, r)); break;
    }
    case MI_SHAPE_SPHERE: {
        center = xfPoint(M, mk(0, 0, 0));
        d.inv_area = 1 / (4 * MI_PI * a.radius * a.radius);
        lo = center - mk(a.radius, a.radius, a.radius); hi = center + mk(a.radius, a.radius, a.radius);
        tightLo = lo; tightHi = hi; break;
    }
    default: {
        d.inv_area = 1 / (2 * MI_PI * a.radius * a.length);
        V3 x1 = xfVector(M, mk(a.radius, 0, 0)), x2 = xfVector(M, mk(0, a.radius, 0));
        V3 p0 = xfPoint(M, mk(0, 0, 0)), p1 = xfPoint(M, mk(0, 0, a.length));
        float l[3], h[3];
        for (int i = 0; i < 3; ++i) {
            float range = std::sqrt(comp(x1, i) * comp(x1, i) + comp(x2, i) * comp(x2, i));
            l[i] = std::min(std::min(inf, comp(p0, i) - range), comp(p1, i) - range);
            h[i] = std::max(std::max(-inf, comp(p0, i) + range), comp(p1, i) + range);
        }
        lo = mk(l[0], l[1], l[2]); hi = mk(h[0], h[1], h[2]);
        tightLo = lo; tightHi = hi; break;
    }
    }
    d.n[0] = n.x; d.n[1] = n.y; d.n[2] = n.z; d.dpdu[0] = dpdu.x; d.dpdu[1] = dpdu.y; d.dpdu[2] = dpdu.z;
    d.center[0] = center.x; d.center[1] = center.y; d.center[2] = center.z;
}

// kd-tree box of the scene = union of the scene-level shapes' AABBs (ShapeKDTree::addShape, skdtree.cpp:68-77) -- meshes outside shape groups, analytic shapes
// (Shape::getAABB), then `n` further boxes (lo, hi: the instances) -- enlarged like the kd-tree root (gkdtree.h:1213-1220)
static void enlargeBox(V3 &lo, V3 &hi) { const float eps = 1e-3f; V3 e1 = hi - lo; lo = lo - mk(e1.x * eps + eps, e1.y * eps + eps, e1.z * eps + eps);
                                         V3 e2 = hi - lo; hi = hi + mk(e2.x * eps + eps, e2.y * eps + eps, e2.z * eps + eps); }
void SceneHost::buildSceneBox(const float *extra, uint32_t n) {
    const float inf = std::numeric_limits<float>::infinity(); V3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
    for (const mi_shape &sh : shapes) { if (sh.group) continue; for (uint32_t v = 0; v < sh.vert_count; ++v) { V3 p = load3(&pos[(size_t) (sh.first_vert + v) * 3]); lo = vmin(lo, p); hi = vmax(hi, p); } }
    for (const mi_analytic &a : analytic) { AnalyticD d; V3 alo, ahi, tl, th; analyticPrepare(a, d, alo, ahi, tl, th); lo = vmin(lo, alo); hi = vmax(hi, ahi); }
    for (uint32_t i = 0; i < n; ++i) { lo = vmin(lo, load3(extra + (size_t) i * 6)); hi = vmax(hi, load3(extra + (size_t) i * 6 + 3)); }
    enlargeBox(lo, hi);
    store3(aabbLo, lo); store3(aabbHi, hi);
}

// kd-tree box of every shape group = union of the member shapes' AABBs in shape order (ShapeKDTree::addShape, skdtree.cpp:68-77), enlarged like the kd-tree root
void SceneHost::buildGroupBoxes() {
    const float inf = std::numeric_limits<float>::infinity();
    uint32_t ng = 0; for (const mi_shape &sh : shapes) ng = std::max(ng, sh.group);
    std::vector<V3> glo(ng, mk(inf, inf, inf)), ghi(ng, mk(-inf, -inf, -inf));
    for (const mi_shape &sh : shapes) { if (!sh.group) continue; const uint32_t g = sh.group - 1; for (uint32_t v = 0; v < sh.vert_count; ++v) { V3 p = load3(&pos[(size_t) (sh.first_vert + v) * 3]); glo[g] = vmin(glo[g], p); ghi[g] = vmax(ghi[g], p); } }
    groupBoxes.assign((size_t) ng * 6, 0.0f);
    for (uint32_t g = 0; g < ng; ++g) { enlargeBox(glo[g], ghi[g]); store3(&groupBoxes[(size_t) g * 6], glo[g]); store3(&groupBoxes[(size_t) g * 6 + 3], ghi[g]); }
}

struct BuildNode { V3 lo, hi; int left = -1, right = -1, first = 0, count = 0; };
struct Builder {
    std::vector<BuildNode> nodes; std::vector<uint32_t> order; const std::vector<V3> *tlo, *thi, *cen;
    const std::vector<uint8_t> *single = nullptr;   // primitives that must sit alone in their leaf (instances: the traversal enters them one at a time)
    int build(int first, int count, int depth) {
        int id = (int) nodes.size(); nodes.emplace_back();
        const float inf = std::numeric_limits<float>::infinity();
        V3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf), clo = lo, chi = hi;
        for (int i = first; i < first + count; ++i) { uint32_t t = order[i]; lo = vmin(lo, (*tlo)[t]); hi = vmax(hi, (*thi)[t]); clo = vmin(clo, (*cen)[t]); chi = vmax(chi, (*cen)[t]); }
        nodes[id].lo = lo; nodes[id].hi = hi;
        auto makeLeaf = [&]() { nodes[id].first = first; nodes[id].count = count; return id; };
        bool mustSplit = false;
        if (single && count > 1) for (int i = first; i < first + count; ++i) mustSplit |= (*single)[order[i]] != 0;
        if (mustSplit) {              // keep splitting (object median) until the singleton primitives are alone
            V3 ce0 = chi - clo; int ax = ce0.x > ce0.y ? (ce0.x > ce0.z ? 0 : 2) : (ce0.y > ce0.z ? 1 : 2);
            std::sort(order.begin() + first, order.begin() + first + count, [&](uint32_t a, uint32_t b) { float x = comp((*cen)[a], ax), y = comp((*cen)[b], ax); return x < y || (x == y && a < b); });
            int m = first + count / 2;
            int l = build(first, m - first, depth + 1), r = build(m, first + count - m, depth + 1);
            nodes[id].left = l; nodes[id].right = r; return id;
        }
        if (count <= 2 || depth > 60) { if (count <= 8) return makeLeaf(); }
        // binned SAH, 16 bins per axis, all three centroid axes tried (round 1 / early round 2: the widest axis only; MI355PT_SAH1=1 restores that for A/B runs)
        static const bool widestOnly = [] { const char *e = getenv("MI355PT_SAH1"); return e && e[0] == '1'; }();
        V3 ce = chi - clo; const int widest = ce.x > ce.y ? (ce.x > ce.z ? 0 : 2) : (ce.y > ce.z ? 1 : 2);
        int mid = -1;
        {
            const int NB = 16; auto area = [](V3 l, V3 h) { V3 e = h - l; return 2.0f * (e.x * e.y + e.y * e.z + e.z * e.x); };
            float best = inf; int bestSplit = -1, bestAxis = -1;
            for (int axis = 0; axis < 3; ++axis) {
                if (widestOnly && axis != widest) continue;
                const float cmin = comp(clo, axis), cext = comp(ce, axis);
                if (!(cext > 0)) continue;
                int cnt[NB] = {0}; V3 blo[NB], bhi[NB];
                for (int b = 0; b < NB; ++b) { blo[b] = mk(inf, inf, inf); bhi[b] = mk(-inf, -inf, -inf); }
                auto binOf = [&](uint32_t t) { int b = (int) ((comp((*cen)[t], axis) - cmin) / cext * NB); return b < 0 ? 0 : (b >= NB ? NB - 1 : b); };
                for (int i = first; i < first + count; ++i) { uint32_t t = order[i]; int b = binOf(t); cnt[b]++; blo[b] = vmin(blo[b], (*tlo)[t]); bhi[b] = vmax(bhi[b], (*thi)[t]); }
                float rightArea[NB]; int rightCnt[NB]; V3 rl = mk(inf, inf, inf), rh = mk(-inf, -inf, -inf); int rc = 0;
                for (int b = NB - 1; b > 0; --b) { if (cnt[b]) { rl = vmin(rl, blo[b]); rh = vmax(rh, bhi[b]); } rc += cnt[b]; rightArea[b] = rc ? area(rl, rh) : 0; rightCnt[b] = rc; }
                V3 ll = mk(inf, inf, inf), lh = mk(-inf, -inf, -inf); int lc = 0;
                for (int b = 0; b < NB - 1; ++b) {
                    if (cnt[b]) { ll = vmin(ll, blo[b]); lh = vmax(lh, bhi[b]); } lc += cnt[b];
                    if (lc == 0 || rightCnt[b + 1] == 0) continue;
                    const float cost = area(ll, lh) * lc + rightArea[b + 1] * rightCnt[b + 1];
                    if (cost < best) { best = cost; bestSplit = b; bestAxis = axis; }
                }
            }
            const float leafCost = area(lo, hi) * count;
            if (bestSplit >= 0 && (count > 4 ? true : best + area(lo, hi) * 1.0f < leafCost)) {
                const int axis = bestAxis; const float cmin = comp(clo, axis), cext = comp(ce, axis);
                auto binOf = [&](uint32_t t) { int b = (int) ((comp((*cen)[t], axis) - cmin) / cext * NB); return b < 0 ? 0 : (b >= NB ? NB - 1 : b); };
                auto it = std::partition(order.begin() + first, order.begin() + first + count, [&](uint32_t t) { return binOf(t) <= bestSplit; });
                mid = (int) (it - order.begin());
            } else if (count <= 8 && (comp(ce, 0) > 0 || comp(ce, 1) > 0 || comp(ce, 2) > 0)) return makeLeaf();
        }
        if (mid <= first || mid >= first + count) {   // degenerate: all centroids equal -> split in the middle
            if (count <= 8) return makeLeaf();
            mid = first + count / 2;
        }
        int l = build(first, mid - first, depth + 1);
        int r = build(mid, first + count - mid, depth + 1);
        nodes[id].left = l; nodes[id].right = r;
        return id;
    }
};

static inline int32_t leafCode(int first, int count) { return ~(int32_t) (first * 8 + (count - 1)); }
// Unused slots of a 4-wide node carry an inverted box (qlo 255, qhi 0), but the conservative box tests of trace.h / trace_fused.h can still pass it: the slack
// 2e-6 * t outgrows the box once the node's extent is below ~2e-6 * t on every axis (small geometry seen from far away).  So the slot's CODE must be harmless
// too: it names a one-record leaf whose record (k = MI_K_NONE, appended after the tree's own leaf records) no triangle test accepts.

void SceneHost::commitHost() {
    ++treeBuilds;
    // a new tree: whatever the vertex or instance edits of the previous one derived (slot tables, level order, box scratch, the stale marks) describes a tree that no longer exists
    geoPrepared = geoStale = instStale = false; leafSlotOfPrim.clear(); leafSlotOfInstance.clear(); refitOrder.clear(); refitLevelStart.clear(); refitOrderAll.clear(); refitLevelStartAll.clear(); leafBoxes.clear(); nodeBoxes.clear();
    const uint32_t nt = (uint32_t) (idx.size() / 3), na = (uint32_t) analytic.size(), ni = (uint32_t) instances.size(), np = nt + na + ni;
    nTris = nt;
    auto vert = [&](uint32_t i) { return mk(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]); };
    triShape.assign(nt, 0);
    for (uint32_t si = 0; si < shapes.size(); ++si) for (uint32_t t = 0; t < shapes[si].tri_count; ++t) triShape[shapes[si].first_tri + t] = si;

    // --- triangle records
    std::vector<TriAccelD> accel(nt); shade.assign(nt, TriShade{}); i2.assign(nt, 0);
    triuv.assign(uv.empty() ? 0 : nt, TriUV{}); anyUV = false;
    std::vector<V3> tlo(np), thi(np), cen(np);
    buildMaterialTables();      // per-material flag bits of the records below (materialFlagBits)
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t a = idx[t * 3], b = idx[t * 3 + 1], c = idx[t * 3 + 2];
        V3 p0 = vert(a), p1 = vert(b), p2 = vert(c);
        triaccelLoad(accel[t], p0, p1, p2); accel[t].prim = t;
        const mi_shape &sh = shapes[triShape[t]];
        TriShade &ts = shade[t];
        ts.material = sh.bsdf; ts.emitter = sh.emitter;
        bool faceN = (sh.flags & 1u) || nrm.empty();
        const bool hasUV = (sh.flags & 2u) && !uv.empty();
        ts.flags = (faceN ? 1u : 0u) | materialFlagTable[sh.bsdf] | (hasUV ? 16u : 0u);
        ts.local_prim = t - sh.first_tri; ts.i0 = a; ts.i1 = b; i2[t] = c;
        if (hasUV) {
            TriUV &tu = triuv[t]; anyUV = true;
            tu.uv0[0] = uv[a * 2]; tu.uv0[1] = uv[a * 2 + 1]; tu.uv1[0] = uv[b * 2]; tu.uv1[1] = uv[b * 2 + 1]; tu.uv2[0] = uv[c * 2]; tu.uv2[1] = uv[c * 2 + 1];
        }
        triShadeGeometry(ts, hasUV ? &triuv[t] : nullptr, p0, p1, p2);      // p0..p2, face normal, face frame, UV tangents (geometry_records.h)
        ts.i2 = c;
        if (!faceN) {      // a smooth triangle carries its three vertex normals instead of the (unused) face frame
            for (int k = 0; k < 3; ++k) { ts.s[k] = nrm[a * 3 + k]; ts.t[k] = nrm[b * 3 + k]; ts.n2[k] = nrm[c * 3 + k]; }
        }
        triPaddedBox(p0, p1, p2, tlo[t], thi[t], cen[t]);      // conservative padding (geometry_records.h)
    }
    // --- analytic shapes: device records, boxes
    analyticD.assign(na, AnalyticD{});
    std::vector<V3> alo(na), ahi(na);
    for (uint32_t i = 0; i < na; ++i) {
        V3 tl, th; analyticPrepare(analytic[i], analyticD[i], alo[i], ahi[i], tl, th);
        analyticD[i].flags = (analytic[i].flags & 1u) | materialFlagTable[analytic[i].bsdf];
        padBox(tl, th, tlo[nt + i], thi[nt + i], cen[nt + i]);
        TriAccelD rec{}; rec.k = MI_K_ANALYTIC; rec.prim = nt + i; accel.push_back(rec);
    }
    // --- kd-tree boxes of the shape groups and of the scene = union of the member shapes' AABBs (ShapeKDTree::addShape, skdtree.cpp:68-77),
    //     enlarged like the kd-tree root (gkdtree.h:1213-1220); instance boxes = the 8 transformed corners of the group box (instance.cpp:46-64)
    uint32_t ng = 0; for (const mi_shape &sh : shapes) ng = std::max(ng, sh.group);
    auto slotOf = [&](const mi_shape &sh) { return sh.group ? sh.group - 1 : ng; };      // slot ng (the scene level) is used by the member lists below; the scene's box is buildSceneBox()
    buildGroupBoxes();      // shared with the geometry edit
    std::vector<V3> glo(ng), ghi(ng);
    for (uint32_t g = 0; g < ng; ++g) { glo[g] = load3(&groupBoxes[(size_t) g * 6]); ghi[g] = load3(&groupBoxes[(size_t) g * 6 + 3]); }
    instancesD.assign(ni, InstanceD{});
    std::vector<float> instBoxes((size_t) ni * 6);
    for (uint32_t i = 0; i < ni; ++i) {
        const mi_instance &in = instances[i]; const uint32_t g = in.group; V3 blo, bhi;
        instanceBoxes(in.to_world, glo[g], ghi[g], blo, bhi, tlo[nt + na + i], thi[nt + na + i], cen[nt + na + i]);      // geometry_records.h: shared with the instance edit
        store3(&instBoxes[(size_t) i * 6], blo); store3(&instBoxes[(size_t) i * 6 + 3], bhi);
        TriAccelD rec{}; rec.k = MI_K_INSTANCE; rec.prim = i; accel.push_back(rec);
        InstanceD &d = instancesD[i]; std::memcpy(d.to_world, in.to_world, 48); std::memcpy(d.to_object, in.to_object, 48);
        d.glo[0] = glo[g].x; d.glo[1] = glo[g].y; d.glo[2] = glo[g].z; d.ghi[0] = ghi[g].x; d.ghi[1] = ghi[g].y; d.ghi[2] = ghi[g].z; d.group = g; d.root = 0;
    }
    buildSceneBox(instBoxes.data(), ni);      // aabbLo / aabbHi: scene-level meshes, analytic shapes, instances; enlarged

    // --- participating media: device records; per primitive the (interior, exterior) pair of its shape (triangles, then analytic shapes)
    mediaD.assign(media.size(), MediumD{});
    for (size_t i = 0; i < media.size(); ++i) {
        MediumD &m = mediaD[i]; const mi_medium &in = media[i];
        for (int c = 0; c < 3; ++c) { m.sigma_s[c] = in.sigma_s[c]; m.sigma_t[c] = in.sigma_a[c] + in.sigma_s[c]; }     // Medium: m_sigmaT = m_sigmaA + m_sigmaS (medium.cpp:36)
        m.strategy = in.strategy; m.phase = in.phase; m.sampling_density = in.sampling_density; m.medium_sampling_weight = in.medium_sampling_weight; m.g = in.g;
    }
    primMedia.clear();
    if (!media.empty()) {
        primMedia.assign(nt + na, 0u);
        auto pairOf = [&](size_t shapeIndex) { return (uint32_t) (shapeMedia[shapeIndex * 2] + 1) | ((uint32_t) (shapeMedia[shapeIndex * 2 + 1] + 1) << 16); };
        for (uint32_t t = 0; t < nt; ++t) primMedia[t] = pairOf(triShape[t]);
        for (uint32_t i = 0; i < na; ++i) primMedia[nt + i] = pairOf(shapes.size() + i);
    }
    // --- BVHs: one per shape group, then the scene level (root = node 0 of its own range; the scene level is built LAST but must be node 0,
    //     so its nodes are emitted first and the groups appended)
    std::vector<uint8_t> single(np, 0); for (uint32_t i = 0; i < ni; ++i) single[nt + na + i] = 1;
    auto setBox = [](float *lo, float *hi, const BuildNode &n) { lo[0] = n.lo.x; lo[1] = n.lo.y; lo[2] = n.lo.z; hi[0] = n.hi.x; hi[1] = n.hi.y; hi[2] = n.hi.z; };
    auto emptyBox = [](float *lo, float *hi) { for (int i = 0; i < 3; ++i) { lo[i] = std::numeric_limits<float>::infinity(); hi[i] = -std::numeric_limits<float>::infinity(); } };
    nodes.clear(); tris.clear();
    std::vector<int> depthOf;     // depth of each emitted tree
    // builds the tree over `prims`, appends its nodes / leaf records, returns the device index of its root (always an inner node)
    // Node kind (measured, DESIGN.md "Tree scenes"): 4-wide quantised nodes win once the tree outgrows the caches close to the CUs (atrium, 0.6 M triangles:
    // +12 %); on small trees and on the two-level trees of instanced scenes the binary nodes' cheaper per-node arithmetic wins (instanced garden: +5 %).
    // MI355PT_BVH2 = 1 / 0 forces binary / wide (A/B runs, parity tests of both kinds).
    { const char *e2 = getenv("MI355PT_BVH2"); wideBvh = e2 && e2[0] ? e2[0] == '0' : (ni == 0 && nt >= 16384u); }
    std::vector<int> treeNeed, treeNeedDirect;    // traversal stack entries each emitted tree can need (one entry per level / child codes pushed one by one)
    auto emitTree = [&](const std::vector<uint32_t> &prims) -> int {
        Builder bld; bld.order = prims; bld.tlo = &tlo; bld.thi = &thi; bld.cen = &cen; bld.single = &single; bld.nodes.reserve(2 * prims.size() + 2);
        const int nodeBase = (int) nodes.size(), triBase = (int) tris.size();
        int root = prims.empty() ? -1 : bld.build(0, (int) prims.size(), 0);
        for (uint32_t i = 0; i < prims.size(); ++i) tris.push_back(accel[bld.order[i]]);
        if (wideBvh) {
            const int32_t emptyChild = leafCode((int) tris.size(), 1);      // the never-hit record behind every unused slot of this tree
            { TriAccelD none{}; none.k = MI_K_NONE; none.prim = 0xFFFFFFFFu; tris.push_back(none); }
            // Collapse the binary tree into 4-wide nodes (the inner child with the largest surface area is replaced by its two children until four slots are
            // taken), quantise the child boxes against the node's own box.  Returns the device index; `need` = stack entries from this node down.
            static_assert(sizeof(Bvh4Node) == sizeof(BvhNode), "both node kinds share one array");
            auto area = [](const BuildNode &n) { V3 e = n.hi - n.lo; return e.x * e.y + e.y * e.z + e.z * e.x; };
            struct Emit { std::vector<BvhNode> &nodes; Builder &bld; int triBase; int32_t emptyChild; decltype(area) &areaOf;
                int run(int id, int &need, int &needD) {
                    std::vector<int> kids;
                    if (id < 0) { /* empty tree */ } else if (bld.nodes[id].count > 0) kids.push_back(id); else { kids.push_back(bld.nodes[id].left); kids.push_back(bld.nodes[id].right); }
                    while (kids.size() < 4) {
                        int pick = -1; float best = -1;
                        for (size_t i = 0; i < kids.size(); ++i) if (bld.nodes[kids[i]].count == 0 && areaOf(bld.nodes[kids[i]]) > best) { best = areaOf(bld.nodes[kids[i]]); pick = (int) i; }
                        if (pick < 0) break;
                        const int k = kids[pick]; kids[pick] = bld.nodes[k].left; kids.insert(kids.begin() + pick + 1, bld.nodes[k].right);
                    }
                    const int dev = (int) nodes.size(); nodes.emplace_back();
                    const float inf = std::numeric_limits<float>::infinity(); V3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
                    for (int k : kids) { lo = vmin(lo, bld.nodes[k].lo); hi = vmax(hi, bld.nodes[k].hi); }
                    if (kids.empty()) { lo = mk(0, 0, 0); hi = mk(0, 0, 0); }
                    Bvh4Node w; std::memset(&w, 0, sizeof(w));
                    int ex[3]; wideNodeFrame(w, lo, hi, ex);      // org + the three steps (geometry_records.h: the refit of a vertex edit re-derives them by the same rule)
                    int sub = 0, subD = 0;
                    for (int c = 0; c < 4; ++c) {
                        if (c >= (int) kids.size()) { wideNodeUnused(w, c); w.child[c] = emptyChild; continue; }
                        const BuildNode &k = bld.nodes[kids[c]];
                        wideNodeChild(w, c, ex, lo, k.lo, k.hi);
                        if (k.count > 0) w.child[c] = leafCode(triBase + k.first, k.count);
                        else { int need = 0, needD = 0; w.child[c] = run(kids[c], need, needD); sub = std::max(sub, need); subD = std::max(subD, needD); }
                    }
                    std::memcpy(&nodes[dev], &w, sizeof(w));
                    // An unused slot can pass the box test (see MI_K_NONE), so every node counts as if all four slots were taken:
                    need = sub + 1;       // one stack entry per level: the node's pending children (trace.h)
                    needD = subD + 3;     // child codes pushed one by one (trace_fused.h): up to three siblings wait while a subtree is walked
                    return dev;
                } };
            Emit em{nodes, bld, triBase, emptyChild, area}; int need = 0, needD = 0; const int dev = em.run(root, need, needD); treeNeed.push_back(need + 1); treeNeedDirect.push_back(needD + 1);
            (void) nodeBase; return dev;
        }
        std::vector<int> devIndex(bld.nodes.size(), -1); int nInner = 0;
        for (size_t i = 0; i < bld.nodes.size(); ++i) if (bld.nodes[i].count == 0) devIndex[i] = nodeBase + nInner++;
        auto childCode = [&](int c) { const BuildNode &n = bld.nodes[c]; return n.count > 0 ? leafCode(triBase + n.first, n.count) : (int32_t) devIndex[c]; };
        if (root < 0) { BvhNode n{}; emptyBox(n.lo0, n.hi0); emptyBox(n.lo1, n.hi1); n.c0 = n.c1 = leafCode(0, 1); nodes.push_back(n); return nodeBase; }
        if (bld.nodes[root].count > 0) {      // the whole tree is one leaf: synthesise a root with one empty child
            BvhNode n{}; setBox(n.lo0, n.hi0, bld.nodes[root]); n.c0 = leafCode(triBase + bld.nodes[root].first, bld.nodes[root].count);
            emptyBox(n.lo1, n.hi1); n.c1 = n.c0; nodes.push_back(n); return nodeBase;
        }
        nodes.resize(nodeBase + nInner);
        for (size_t i = 0; i < bld.nodes.size(); ++i) {
            const BuildNode &b = bld.nodes[i]; if (b.count > 0) continue;
            BvhNode &n = nodes[devIndex[i]]; std::memset(&n, 0, sizeof(n));
            setBox(n.lo0, n.hi0, bld.nodes[b.left]); setBox(n.lo1, n.hi1, bld.nodes[b.right]);
            n.c0 = childCode(b.left); n.c1 = childCode(b.right);
        }
        return devIndex[root];
    };
    std::vector<std::vector<uint32_t> > members(ng + 1);
    for (const mi_shape &sh : shapes) { uint32_t g = slotOf(sh); for (uint32_t t = 0; t < sh.tri_count; ++t) members[g].push_back(sh.first_tri + t); }
    for (uint32_t t = nt; t < np; ++t) members[ng].push_back(t);
    emitTree(members[ng]);                 // the scene level first: a tree's root is the first node it emits, so the scene root is node 0
    // Hot nodes first (wide scene-level tree without instances): a node is visited about as often as its box is large (surface area heuristic) -- on the atrium the
    // 128 most visited of 62 k nodes take 64 % of all node visits -- so sorting the array by box area packs the nodes every ray reads into a few cache lines that
    // stay resident (the fused walk of trace_fused.h reads nodes from global memory; it keeps only its stack and the ray in LDS).  A pure renumbering (root stays
    // node 0, leaf codes -- unused slots included -- are negative and untouched): every traversal sees the same tree.
    if (wideBvh && ni == 0 && ng == 0 && nodes.size() > 1) {
        Bvh4Node *w = reinterpret_cast<Bvh4Node *>(nodes.data()); const size_t nn = nodes.size();
        std::vector<float> areaOf(nn, 0.0f); areaOf[0] = std::numeric_limits<float>::infinity();
        for (size_t i = 0; i < nn; ++i) for (int c = 0; c < 4; ++c) if (w[i].child[c] >= 0) {
            const float st[3] = {w[i].step_x, w[i].step_y, w[i].step_z}; float e[3];
            for (int a = 0; a < 3; ++a) e[a] = (float) ((int) ((w[i].qhi[a] >> (8 * c)) & 0xFFu) - (int) ((w[i].qlo[a] >> (8 * c)) & 0xFFu)) * st[a];
            areaOf[w[i].child[c]] = e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
        }
        std::vector<uint32_t> byArea(nn); for (size_t i = 0; i < nn; ++i) byArea[i] = (uint32_t) i;
        std::stable_sort(byArea.begin(), byArea.end(), [&](uint32_t a, uint32_t b) { return areaOf[a] > areaOf[b]; });
        std::vector<int32_t> newIndex(nn); for (size_t i = 0; i < nn; ++i) newIndex[byArea[i]] = (int32_t) i;
        std::vector<BvhNode> re(nn);
        for (size_t i = 0; i < nn; ++i) {
            Bvh4Node n = w[byArea[i]];
            for (int c = 0; c < 4; ++c) if (n.child[c] >= 0) n.child[c] = newIndex[n.child[c]];
            std::memcpy(&re[i], &n, sizeof(n));
        }
        nodes.swap(re);
    }
    groupRoot.assign(ng, 0);
    for (uint32_t g = 0; g < ng; ++g) groupRoot[g] = emitTree(members[g]);
    for (uint32_t i = 0; i < ni; ++i) instancesD[i].root = groupRoot[instances[i].group];
    // traversal stack need: scene tree + one return marker + the deepest group tree
    if (wideBvh) {      // treeNeed[0]: the scene level, then one entry per group
        int groupNeed = 0; for (uint32_t g = 0; g < ng; ++g) groupNeed = std::max(groupNeed, treeNeed[1 + g]);
        bvhDepth = treeNeed[0] + (ni ? 1 + groupNeed : 0);
        bvhStackDirect = treeNeedDirect[0];
    } else {
        struct Depth { const std::vector<BvhNode> &n; int of(int i) const { if (i < 0) return 0; int a = of(n[i].c0), b = of(n[i].c1); return 1 + (a > b ? a : b); } } dep{nodes};
        int groupDepth = 0; for (uint32_t g = 0; g < ng; ++g) groupDepth = std::max(groupDepth, dep.of(groupRoot[g]));
        bvhDepth = dep.of(0) + (ni ? 1 + groupDepth : 0);
        bvhStackDirect = dep.of(0);
    }
    // packet mode (no instances, <= MI_PACKET_MAX triangles): exact records in original order + pass-1 group records (pt_types.h PacketGroupD).  Coplanar
    // pairs that form a parallelogram (the two halves of a quad) share one record: for the vertices (X, Y, Z) of a triangle, taken cyclically, the partner is
    // the triangle on {Y, Z, Y + Z - X}.  Degenerate triangles (k = 3) never hit and are dropped.
    packetExact.assign(accel.begin(), accel.begin() + nt);
    buildPacketTables();
    if (packetExact.empty()) packetExact.push_back(TriAccelD{});

    buildEmitterTables();

    /* --- reconstruction filter table (src/libcore/rfilter.cpp:37-56; eval of src/rfilters/box.cpp:31-48, gaussian.cpp:30-57, tent.cpp:36-38,
     * mitchell.cpp:49-61, catmullrom.cpp:36-49, lanczos.cpp:36-46).  filter_radius / filter_stddev carry: box radius; gaussian stddev (in
     * filter_stddev); mitchell B, C; lanczos lobes (in filter_radius) */
    {
        const uint32_t kind = filterKind;
        float radius = kind == 0 ? filterRadius + 1e-5f : kind == 1 ? 4.0f * filterStddev : kind == 2 ? 1.0f : kind == 5 ? (float) (int) filterRadius : 2.0f;
        float alpha = -1.0f / (2.0f * filterStddev * filterStddev), bias = std::exp(alpha * radius * radius);
        const float B = kind == 3 ? filterRadius : 0.0f, C = kind == 3 ? filterStddev : 0.5f;
        float sum = 0.0f;
        for (int i = 0; i < MI_FILTER_RES; ++i) {
            float x = (radius * (float) i) / (float) MI_FILTER_RES, v;
            if (kind == 0) v = std::fabs(x) <= radius ? 1.0f : 0.0f;
            else if (kind == 1) v = std::max(0.0f, std::exp(alpha * x * x) - bias);
            else if (kind == 2) v = std::max(0.0f, 1.0f - std::fabs(x / radius));
            else if (kind == 5) {
                float ax = std::fabs(x);
                if (ax < 1e-4f) v = 1.0f; else if (ax > radius) v = 0.0f;
                else { float x1 = MI_PI * ax, x2 = x1 / radius; v = (std::sin(x1) * std::sin(x2)) / (x1 * x2); }
            } else {
                float ax = std::fabs(x), x2 = ax * ax, x3 = x2 * ax;
                if (ax < 1) v = 1.0f / 6.0f * ((12 - 9 * B - 6 * C) * x3 + (-18 + 12 * B + 6 * C) * x2 + (6 - 2 * B));
                else if (ax < 2) v = 1.0f / 6.0f * ((-B - 6 * C) * x3 + (6 * B + 30 * C) * x2 + (-12 * B - 48 * C) * ax + (8 * B + 24 * C));
                else v = 0.0f;
            }
            filterValues[i] = v; sum += v;
        }
        filterValues[MI_FILTER_RES] = 0.0f;
        filterScale = (float) MI_FILTER_RES / radius; filterRadiusEff = radius;
        border = (int) std::ceil(radius - 0.5f);
        sum *= 2 * radius / (float) MI_FILTER_RES;
        float norm = 1.0f / sum;
        for (int i = 0; i < MI_FILTER_RES; ++i) filterValues[i] *= norm;
    }
    // --- environment emitter tables (envmap.cpp:264-330 configure)
    buildBoundingSpheres();
    if (envIndex >= 0 && !envConstant) {
        const int W = (int) envW, H = (int) envH;
        auto texel = [&](int x, int y) { const float *p = &envRGB[((size_t) y * W + x) * 3]; return mk(p[0], p[1], p[2]); };
        auto lum = [](V3 c) { return c.x * 0.212671f + c.y * 0.715160f + c.z * 0.072169f; };
        buildEnvTransform();
        envCdfCols.assign((size_t) (W + 1) * H, 0.0f); envCdfRows.assign((size_t) H + 1, 0.0f); envRowWeights.assign((size_t) H, 0.0f);
        size_t colPos = 0, rowPos = 0; float rowSum = 0.0f;
        envCdfRows[rowPos++] = 0;
        for (int y = 0; y < H; ++y) {
            float colSum = 0; envCdfCols[colPos++] = 0;
            for (int x = 0; x < W; ++x) { colSum += lum(texel(x, y)); envCdfCols[colPos++] = colSum; }
            float normalization = 1.0f / colSum;
            for (int x = 1; x < W; ++x) envCdfCols[colPos - x - 1] *= normalization;
            envCdfCols[colPos - 1] = 1.0f;
            float weight = std::sin(((float) y + 0.5f) * MI_PI / (float) H);
            envRowWeights[y] = weight; rowSum += colSum * weight; envCdfRows[rowPos++] = rowSum;
        }
        float normalization = 1.0f / rowSum;
        for (int y = 1; y < H; ++y) envCdfRows[rowPos - y - 1] *= normalization;
        envCdfRows[rowPos - 1] = 1.0f;
        // guide tables: the index lower_bound(cdf, b / K) for every bucket boundary (b / K is exact: K is a power of two), one table for the rows, one per row for the columns
        auto pow2ge = [](uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; };
        envGuideKR = std::min<uint32_t>(pow2ge((uint32_t) H), 4096u); envGuideKC = std::min<uint32_t>(pow2ge((uint32_t) W) / 4u > 0 ? pow2ge((uint32_t) W) / 4u : 1u, 1024u);
        auto guideOf = [](const float *cdf, uint32_t size, uint32_t K, uint16_t *out) {
            for (uint32_t b = 0; b <= K; ++b) { const float x = (float) b / (float) K; out[b] = b == K ? (uint16_t) (size + 1) : (uint16_t) (std::lower_bound(cdf, cdf + size + 1, x) - cdf); }
        };
        if ((uint32_t) W + 1 < 65535u && (uint32_t) H + 1 < 65535u) {
            envGuideRows.assign(envGuideKR + 1, 0); guideOf(envCdfRows.data(), (uint32_t) H, envGuideKR, envGuideRows.data());
            envGuideCols.assign((size_t) H * (envGuideKC + 1), 0);
            for (int y = 0; y < H; ++y) guideOf(envCdfCols.data() + (size_t) y * (W + 1), (uint32_t) W, envGuideKC, envGuideCols.data() + (size_t) y * (envGuideKC + 1));
        } else { envGuideRows.clear(); envGuideCols.clear(); envGuideKR = envGuideKC = 0; }
        envNormalization = 1.0f / (rowSum * (2 * MI_PI / (float) W) * (MI_PI / (float) H));
    }
    // Sobol film resolution (src/samplers/sobol.cpp:147-157)
    { uint32_t r = std::max(width, height), p = 1, l = 0; while (p < r) { p <<= 1; ++l; } resolution = (float) p; logRes = l; }
}

// ------------------------------------------------------------------------------------------------ pieces shared by commitHost() / upload() and the in-place edits
uint32_t SceneHost::materialFlagBits(uint32_t bsdf) const {
    // flags of a shape's material as MIPathTracer::Li sees the (possibly nested) BSDF: bit1 EBackSide / ETransmission somewhere (dRec.refN = 0, records.inl:160-164),
    // bit2 no smooth component (no emitter sampling, path.cpp:173-174), bit3 anything but a plain diffuse record (class bit of the shading stage)
    auto leafBackside = [&](const mi_material &mat) { return (mat.flags & MI_BSDF_FLAG_TWOSIDED) != 0 || mat.type == MI_BSDF_DIELECTRIC || mat.type == MI_BSDF_ROUGHDIELECTRIC || mat.type == MI_BSDF_DIFFTRANS || mat.type == MI_BSDF_THINDIELECTRIC || mat.type == MI_BSDF_NULL; };
    // a `diffuse` with zero reflectance has no component at all -> not ESmooth -> Li skips emitter sampling (diffuse.cpp:99-102, path.cpp:174-176);
    // conductor / dielectric register delta components only
    auto leafSmooth = [&](const mi_material &mat) { return mat.type == MI_BSDF_DIFFUSE ? (((mat.flags >> 8) & 0xFFFFu) != 0 || std::max(std::max(mat.reflectance[0], mat.reflectance[1]), mat.reflectance[2]) > 0)
                                                                                         : (mat.type != MI_BSDF_CONDUCTOR && mat.type != MI_BSDF_DIELECTRIC && mat.type != MI_BSDF_THINDIELECTRIC && mat.type != MI_BSDF_NULL); };
        const mi_material *mat = &materials[bsdf]; bool masked = false, wrapped = false;
        if (mat->type == MI_BSDF_MASK) { masked = true; mat = &materials[mat->distr]; }          // mask.cpp:104-121: the nested BSDF's components + an ENull | EFrontSide | EBackSide one
        if (mat->type == MI_BSDF_BUMPMAP || mat->type == MI_BSDF_NORMALMAP) { wrapped = true; mat = &materials[mat->distr]; }     // the nested BSDF's component types (bumpmap.cpp:97-100)
        bool backside, smooth, coated = false;
        if (mat->type == MI_BSDF_COATING || mat->type == MI_BSDF_ROUGHCOATING) { coated = true; wrapped = true; mat = &materials[mat->distr]; }      // coating.cpp:166-173: the nested components + a delta reflection that is EFrontSide | EBackSide
        if (mat->type == MI_BSDF_BLEND) {                                                           // the two BSDFs' components (blendbsdf.cpp:103-134)
            backside = (mat->flags & MI_BSDF_FLAG_TWOSIDED) != 0; smooth = false; wrapped = true;
            for (int c = 0; c < 2; ++c) { const mi_material &ch = materials[(uint32_t) mat->eta[c]]; backside |= leafBackside(ch); smooth |= leafSmooth(ch); }
        } else if (mat->type == MI_BSDF_MIXTURE) {                                                         // the children's components (mixturebsdf.cpp:150-166)
            backside = (mat->flags & MI_BSDF_FLAG_TWOSIDED) != 0; smooth = false; wrapped = true;
            for (uint32_t c = 0; c < mat->distr; ++c) { const mi_material &ch = materials[(uint32_t) (c < 3 ? mat->reflectance[c] : mat->eta[0])]; backside |= leafBackside(ch); smooth |= leafSmooth(ch); }
        } else { backside = leafBackside(*mat); smooth = leafSmooth(*mat); }
        return ((backside || masked || coated) ? 2u : 0u) | (smooth ? 0u : 4u) | ((mat->type != MI_BSDF_DIFFUSE || masked || wrapped) ? 8u : 0u);
}
void SceneHost::buildMaterialTables() {
    materialFlagTable.resize(materials.size());
    for (uint32_t i = 0; i < materials.size(); ++i) materialFlagTable[i] = materialFlagBits(i);
    // what the reference's configure() derives from a BSDF's own parameters
    std::vector<MaterialD> &mats = materialsD; mats.resize(materials.size());
    for (size_t i = 0; i < materials.size(); ++i) memcpy(&mats[i], &materials[i], sizeof(MaterialD));
    for (MaterialD &m : mats) if (m.type == MI_BSDF_ROUGHCOATING) {      // RoughCoating::configure (roughcoating.cpp:205-209): the same weight, thickness in eta[1]
        float avg = 0.0f; for (int c = 0; c < 3; ++c) avg += (float) exp((double) (m.reflectance[c] * (-2 * m.eta[1])));
        avg = avg * (1.0f / 3); m.k[0] = 1.0f / (avg + 1.0f);
    }
    for (MaterialD &m : mats) if (m.type == MI_BSDF_COATING) {      // SmoothCoating::configure (coating.cpp:182-186): m_specularSamplingWeight from the layer's average absorption -> k[0]
        float avg = 0.0f; for (int c = 0; c < 3; ++c) avg += (float) exp((double) (m.reflectance[c] * (-2 * m.alpha)));      // Spectrum::exp = math::fastexp per channel, then average()
        avg = avg * (1.0f / 3); m.k[0] = 1.0f / (avg + 1.0f);
    }
    for (MaterialD &m : mats) {          // plastic / roughplastic: m_specularSamplingWeight = sAvg / (dAvg + sAvg) over Texture::getAverage() (plastic.cpp:204-207, roughplastic.cpp:244-246) -> eta[1]
        if (m.type != MI_BSDF_PLASTIC && m.type != MI_BSDF_ROUGHPLASTIC) continue;
        float d[3] = {m.reflectance[0], m.reflectance[1], m.reflectance[2]}; const uint32_t tex = (m.flags >> 8) & 0xFFFFu;
        if (tex && tex <= textures.size()) {     // checkerboard.cpp:102-104, gridtexture.cpp:116-121; a bitmap's average is input (color0, from TMIPMap::getAverage)
            const mi_texture &t = textures[tex - 1];
            for (int c = 0; c < 3; ++c) {
                if (t.type == MI_TEXTURE_CHECKERBOARD) d[c] = (t.color0[c] + t.color1[c]) * 0.5f;
                else if (t.type == MI_TEXTURE_GRID) { const float iw = std::max(0.0f, 1 - 2 * t.line_width), ia = iw * iw, la = 1 - ia; d[c] = t.color1[c] * la + t.color0[c] * ia; }
                else d[c] = t.color0[c];
            }
        }
        const float dl = d[0] * 0.212671f + d[1] * 0.715160f + d[2] * 0.072169f, sl = m.specular[0] * 0.212671f + m.specular[1] * 0.715160f + m.specular[2] * 0.072169f;
        m.eta[1] = sl / (dl + sl);
    }
}
// Packet mode tables that depend on the vertex positions: packetScale, the pass-1 group records (pair detection over <= MI_PACKET_MAX triangles) and their axis ranges.
void SceneHost::buildPacketTables() {
    const uint32_t nt = (uint32_t) (idx.size() / 3), ni = (uint32_t) instances.size();
    auto vert = [&](uint32_t i) { return mk(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]); };
    std::vector<uint32_t> kOf;      // projection axis of every triangle's Wald record (3: degenerate); only the packet needs it
    if (nt <= MI_PACKET_MAX && ni == 0) { kOf.resize(nt); for (uint32_t t = 0; t < nt; ++t) { TriAccelD ta; triaccelLoad(ta, vert(idx[t * 3]), vert(idx[t * 3 + 1]), vert(idx[t * 3 + 2])); kOf[t] = ta.k; } }
    packetGroups.clear(); packetGK[0] = packetGK[1] = packetGK[2] = 0;
    {
        float sx = 0; for (int i = 0; i < 3; ++i) sx = std::max(sx, std::max(std::fabs(aabbLo[i]), std::fabs(aabbHi[i])));
        packetScale = sx;
        if (nt <= MI_PACKET_MAX && ni == 0) {
            const float tol = 1e-6f * std::max(sx, 1e-20f);
            auto near = [&](V3 a, V3 b) { return std::fabs(a.x - b.x) <= tol && std::fabs(a.y - b.y) <= tol && std::fabs(a.z - b.z) <= tol; };
            std::vector<uint8_t> used(nt, 0); std::vector<PacketGroupD> byAxis[3];
            for (uint32_t t1 = 0; t1 < nt; ++t1) {
                if (used[t1] || kOf[t1] > 2) continue;
                used[t1] = 1;
                const V3 P[3] = {vert(idx[t1 * 3]), vert(idx[t1 * 3 + 1]), vert(idx[t1 * 3 + 2])};
                int partner = -1, rot = 0;
                for (uint32_t t2 = t1 + 1; t2 < nt && partner < 0; ++t2) {
                    if (used[t2] || kOf[t2] != kOf[t1]) continue;
                    const V3 Q[3] = {vert(idx[t2 * 3]), vert(idx[t2 * 3 + 1]), vert(idx[t2 * 3 + 2])};
                    for (int r = 0; r < 3 && partner < 0; ++r) {
                        const V3 X = P[r], Y = P[(r + 1) % 3], Z = P[(r + 2) % 3], X2 = Y + Z - X;
                        for (int a = 0; a < 3 && partner < 0; ++a)      // t2's vertex set == {Y, Z, X2} in any order
                            for (int b = 0; b < 3 && partner < 0; ++b) { if (b == a) continue; const int c = 3 - a - b;
                                if (near(Q[a], Y) && near(Q[b], Z) && near(Q[c], X2)) { partner = (int) t2; rot = r; } }
                    }
                }
                // relabel (X, Y, Z) -> (A*, B*, C*) = (Z, X, Y): a cyclic rotation (same plane, same orientation), shared edge YZ = C*A* <-> u* = 0
                const V3 X = P[rot], Y = P[(rot + 1) % 3], Z = P[(rot + 2) % 3];
                TriAccelD ta; triaccelLoad(ta, partner >= 0 ? Z : P[0], partner >= 0 ? X : P[1], partner >= 0 ? Y : P[2]);
                if (ta.k > 2) continue;
                if (partner >= 0) used[partner] = 1;
                PacketGroupD g; g.n_u = ta.n_u; g.n_v = ta.n_v; g.n_d = ta.n_d; g.a_u = ta.a_u; g.a_v = ta.a_v; g.b_nu = ta.b_nu; g.b_nv = ta.b_nv; g.c_nu = ta.c_nu; g.c_nv = ta.c_nv;
                g.margin = 1.1f * (std::fabs(ta.b_nu) + std::fabs(ta.b_nv) + std::fabs(ta.c_nu) + std::fabs(ta.c_nv));
                g.prim0 = t1; g.prim1 = partner >= 0 ? (uint32_t) partner : 0xFFFFFFFFu;
                byAxis[ta.k].push_back(g);
            }
            for (int axis = 0; axis < 3; ++axis) { packetGroups.insert(packetGroups.end(), byAxis[axis].begin(), byAxis[axis].end()); packetGK[axis] = (uint32_t) packetGroups.size(); }
        }
    }
    if (packetGroups.empty()) packetGroups.push_back(PacketGroupD{});
}
void SceneHost::buildEmitterTables() {
    auto vert = [&](uint32_t i) { return mk(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]); };
    // --- emitters (scene.cpp:383-388; pmf.h:56-58,103-116; trimesh.cpp:389-402; triangle.cpp:61-67)
    const uint32_t ne = (uint32_t) emitters.size();
    emitterCdf.assign(ne + 1, 0.0f); emittersD.assign(ne, EmitterD{}); areaCdf.clear(); emitterNorm = 0.0f;
    emitterX.assign((size_t) std::max(ne, 1u) * 16, 0.0f); hasDeltaEmitters = false;
    for (uint32_t e = 0; e < ne; ++e) emitterCdf[e + 1] = emitterCdf[e] + emitters[e].weight;
    if (ne) { float sum = emitterCdf[ne]; emitterNorm = sum > 0 ? 1.0f / sum : 0.0f; for (uint32_t e = 1; e <= ne; ++e) emitterCdf[e] *= emitterNorm; emitterCdf[ne] = 1.0f; }
    for (uint32_t e = 0; e < ne; ++e) {
        EmitterD &d = emittersD[e]; const mi_emitter &src = emitters[e];
        d.radiance[0] = src.radiance[0]; d.radiance[1] = src.radiance[1]; d.radiance[2] = src.radiance[2]; d.weight = src.weight;
        d.type = src.type; d.shape = src.shape;
        d.analytic = -1;
        float *x = &emitterX[e * 16];
        if (src.type == MI_EMITTER_POINT || src.type == MI_EMITTER_SPOT) { x[0] = src.to_world[3]; x[1] = src.to_world[7]; x[2] = src.to_world[11]; hasDeltaEmitters = true; }
        if (src.type == MI_EMITTER_COLLIMATED) { x[0] = src.to_world[3]; x[1] = src.to_world[7]; x[2] = src.to_world[11]; hasDeltaEmitters = true; }      // (selects the kernel variants whose sampleEmitterDirect knows emitter types >= 2)
        if (src.type == MI_EMITTER_DIRECTIONAL) { x[0] = src.to_world[2]; x[1] = src.to_world[6]; x[2] = src.to_world[10]; hasDeltaEmitters = true; }
        if (src.type == MI_EMITTER_SPOT) {                        // SpotEmitter constructor + configure (spot.cpp:70-96); trafo.inverse() of the rigid toWorld
            float beam = src.beam * (MI_PI / 180.0f), cutoff = src.cutoff * (MI_PI / 180.0f);
            x[13] = std::cos(beam); x[3] = std::cos(cutoff); x[14] = cutoff; x[15] = 1.0f / (cutoff - beam);
            const float *m = src.to_world; float *o = x + 4;
            float a[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
            float det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]); float id = 1.0f / det;
            o[0] = (a[4] * a[8] - a[5] * a[7]) * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
            o[3] = (a[5] * a[6] - a[3] * a[8]) * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
            o[6] = (a[3] * a[7] - a[4] * a[6]) * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
        }
        if (src.type != MI_EMITTER_AREA) continue;
        if ((size_t) src.shape >= shapes.size()) {               // area light on an analytic shape: no triangle CDF
            d.analytic = src.shape - (int32_t) shapes.size(); d.inv_area = analyticD[d.analytic].inv_area; continue;
        }
        const mi_shape &sh = shapes[src.shape];
        d.first_tri = sh.first_tri; d.tri_count = sh.tri_count; d.cdf_offset = (uint32_t) areaCdf.size();
        size_t base = areaCdf.size(); areaCdf.resize(base + sh.tri_count + 1); areaCdf[base] = 0.0f;
        for (uint32_t t = 0; t < sh.tri_count; ++t) {
            uint32_t prim = sh.first_tri + t;
            V3 p0 = vert(idx[prim * 3]), p1 = vert(idx[prim * 3 + 1]), p2 = vert(idx[prim * 3 + 2]);
            V3 c = cross(p1 - p0, p2 - p0);
            areaCdf[base + t + 1] = areaCdf[base + t] + 0.5f * std::sqrt(dot(c, c));
        }
        float sum = areaCdf[base + sh.tri_count], norm = 1.0f / sum;
        for (uint32_t t = 1; t <= sh.tri_count; ++t) areaCdf[base + t] *= norm;
        areaCdf[base + sh.tri_count] = 1.0f;
        d.inv_area = 1.0f / sum;
    }
    if (areaCdf.empty()) areaCdf.push_back(0.0f);
    envIndex = -1; envConstant = false;
    for (uint32_t e = 0; e < ne; ++e) if (emitters[e].type == MI_EMITTER_ENVMAP || emitters[e].type == MI_EMITTER_CONSTANT) { envIndex = (int) e; envConstant = emitters[e].type == MI_EMITTER_CONSTANT; }
}
void SceneHost::buildBoundingSpheres() {
    {   // bounding spheres: environment emitters (envmap.cpp:336-347, constant.cpp:69-74: scene box incl. the sensor, x 1.5); directional.cpp:87-93 (kd-tree box, x 1.1)
        V3 blo = mk(aabbLo[0], aabbLo[1], aabbLo[2]), bhi = mk(aabbHi[0], aabbHi[1], aabbHi[2]);
        V3 c0 = (bhi + blo) * 0.5f, cm0 = c0 - bhi;
        dirBsCenter[0] = c0.x; dirBsCenter[1] = c0.y; dirBsCenter[2] = c0.z; dirBsRadius = std::sqrt(dot(cm0, cm0)) * 1.1f;
        V3 cam = mk(c2w[3], c2w[7], c2w[11]);
        blo = vmin(blo, cam); bhi = vmax(bhi, cam);
        V3 c = (bhi + blo) * 0.5f, cm = c - bhi;
        envBsCenter[0] = c.x; envBsCenter[1] = c.y; envBsCenter[2] = c.z; envBsRadius = std::max(MI_EPSILON, std::sqrt(dot(cm, cm)) * 1.5f);
    }
}
void SceneHost::buildEnvTransform() {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) envToWorld3[i * 3 + j] = envToWorld[i * 4 + j];
    { const float *m = envToWorld3; float det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]); float id = 1.0f / det;
      float *o = envToLocal3;
      o[0] = (m[4] * m[8] - m[5] * m[7]) * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
      o[3] = (m[5] * m[6] - m[3] * m[8]) * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
      o[6] = (m[3] * m[7] - m[4] * m[6]) * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id; }
}
// d.cam_dx / d.cam_dy: PerspectiveCameraImpl::m_dx / m_dy (perspective.cpp:159-163)
void SceneHost::syncCameraD() {
    memcpy(d.s2c, s2c, 64); memcpy(d.c2w, c2w, 64); d.near_clip = nearClip; d.far_clip = farClip;
    d.lens_radius = lensRadius; d.focus_distance = lensRadius != 0.0f ? focusDistance : 0.0f;
    const float *m = s2c; const float irx = 1.0f / (float) width, iry = 1.0f / (float) height;
    auto pt = [&](float px, float py, float *o) {
        float x = m[0] * px + m[1] * py + m[2] * 0.0f + m[3], y = m[4] * px + m[5] * py + m[6] * 0.0f + m[7], z = m[8] * px + m[9] * py + m[10] * 0.0f + m[11], w = m[12] * px + m[13] * py + m[14] * 0.0f + m[15];
        if (w != 1.0f) { float r = 1.0f / w; x *= r; y *= r; z *= r; }
        o[0] = x; o[1] = y; o[2] = z; };
    float p0[3], px[3], py[3]; pt(0.0f, 0.0f, p0); pt(irx, 0.0f, px); pt(0.0f, iry, py);
    for (int i = 0; i < 3; ++i) { d.cam_dx[i] = px[i] - p0[i]; d.cam_dy[i] = py[i] - p0[i]; }
    memcpy(d.dir_bs_center, dirBsCenter, 12); d.dir_bs_radius = dirBsRadius;
    d.env_bs_radius = envBsRadius; memcpy(d.env_bs_center, envBsCenter, 12);
}
void SceneHost::syncEmittersD() { d.emitter_norm = emitterNorm; }
void SceneHost::syncEnvD() {
    if (envIndex < 0 || envConstant) return;
    d.env_scale = envScale; memcpy(d.env_to_world, envToWorld3, 36); memcpy(d.env_to_local, envToLocal3, 36);
}

// ------------------------------------------------------------------------------------------------ in-place edits of a committed scene
// An edit changes numbers.  Whatever selects kernel variants, table sizes or the per-triangle layout is fixed at commit: such a change is refused, naming the first record.
int SceneHost::updateCamera(const float *s2cIn, const float *c2wIn, float nearIn, float farIn, std::string &msg) {
    if (!s2cIn || !c2wIn) { msg = "mi_scene_update_camera: null argument"; return MI_ERR_INVALID; }
    if (!committed) { msg = "mi_scene_update_camera: scene not committed"; return MI_ERR_INVALID; }
    memcpy(s2c, s2cIn, 64); memcpy(c2w, c2wIn, 64); nearClip = nearIn; farClip = farIn;
    buildBoundingSpheres();      // the environment emitters' sphere includes the sensor position
    syncCameraD(); ++revision;
    return MI_OK;
}
int validateLens(const char *who, float apertureRadius, float focusDistance, std::string &msg) {
    if (!std::isfinite(apertureRadius) || apertureRadius < 0.0f) { msg = std::string(who) + ": the aperture radius must be finite and >= 0"; return MI_ERR_INVALID; }
    if (apertureRadius > 0.0f && (!std::isfinite(focusDistance) || !(focusDistance > 0.0f))) { msg = std::string(who) + ": the focus distance must be finite and > 0 when the aperture radius is positive"; return MI_ERR_INVALID; }
    return MI_OK;
}
// The lens lives in the scene record alone, like the camera: syncCameraD() is all an edit recomputes.
int SceneHost::updateLens(float apertureRadius, float focusDistanceIn, std::string &msg) {
    if (!committed) { msg = "mi_scene_update_lens: scene not committed"; return MI_ERR_INVALID; }
    if (const int rc = validateLens("mi_scene_update_lens", apertureRadius, focusDistanceIn, msg)) return rc;
    if ((apertureRadius != 0.0f) != (lensRadius != 0.0f)) {
        msg = std::string("mi_scene_update_lens: the scene was committed ") + (lensRadius != 0.0f ? "with" : "without") + " a lens; turning it " + (lensRadius != 0.0f ? "off" : "on") + " changes the sample layout of every path, commit a new scene";
        return MI_ERR_UNSUPPORTED;
    }
    lensRadius = apertureRadius; focusDistance = apertureRadius != 0.0f ? focusDistanceIn : 0.0f;
    syncCameraD(); ++revision;
    return MI_OK;
}
int SceneHost::updateMaterials(const mi_material *m, uint32_t n, std::string &msg, bool *flagsChanged) {
    if (flagsChanged) *flagsChanged = false;
    if (!m || !n) { msg = "mi_scene_update_materials: null argument"; return MI_ERR_INVALID; }
    if (!committed) { msg = "mi_scene_update_materials: scene not committed"; return MI_ERR_INVALID; }
    if (n != materials.size()) { msg = "mi_scene_update_materials: the record count changes (" + std::to_string(materials.size()) + " -> " + std::to_string(n) + "); commit a new scene"; return MI_ERR_UNSUPPORTED; }
    auto refuse = [&](uint32_t i, const char *what) { msg = "mi_scene_update_materials: material " + std::to_string(i) + " changes " + what + "; an update changes values only, commit a new scene"; return MI_ERR_UNSUPPORTED; };
    for (uint32_t i = 0; i < n; ++i) {
        const mi_material &a = materials[i], &b = m[i];
        if (a.type != b.type) return refuse(i, "its type");
        if ((a.flags ^ b.flags) & 0xFFFF00u) return refuse(i, "its texture binding");
        if ((a.flags ^ b.flags) & (MI_BSDF_FLAG_ANISOTROPIC | MI_BSDF_FLAG_NONLINEAR | MI_BSDF_FLAG_SAMPLE_VISIBLE)) return refuse(i, "its anisotropic / nonlinear / sampleVisible bit");
        const uint32_t t = a.type;
        if ((t == MI_BSDF_MASK || t == MI_BSDF_MIXTURE || t == MI_BSDF_BUMPMAP || t == MI_BSDF_NORMALMAP || t == MI_BSDF_COATING || t == MI_BSDF_ROUGHCOATING || t == MI_BSDF_BLEND) && a.distr != b.distr)
            return refuse(i, "`distr` of a wrapper (its nested record / child count)");
        if (t == MI_BSDF_MIXTURE) for (uint32_t c = 0; c < a.distr && c < 4; ++c) if ((c < 3 ? a.reflectance[c] : a.eta[0]) != (c < 3 ? b.reflectance[c] : b.eta[0])) return refuse(i, "the child indices of a mixturebsdf");
        if (t == MI_BSDF_BLEND && (a.eta[0] != b.eta[0] || a.eta[1] != b.eta[1])) return refuse(i, "the child indices of a blendbsdf");
        if ((t == MI_BSDF_ROUGHPLASTIC || t == MI_BSDF_ROUGHCOATING) && (a.k[1] != b.k[1] || a.k[2] != b.k[2])) return refuse(i, "the offset / length of its rough-transmittance slice (k[1], k[2])");
    }
    { const int rc = validateMaterials(m, n, msg); if (rc) return rc; }
    materials.assign(m, m + n);
    const std::vector<uint32_t> before = materialFlagTable;
    buildMaterialTables();
    if (before != materialFlagTable) {      // the bits sit in every primitive that uses the material, group members included
        for (TriShade &ts : shade) ts.flags = (ts.flags & ~MI_MATERIAL_FLAG_BITS) | materialFlagTable[ts.material];
        for (size_t i = 0; i < analyticD.size(); ++i) analyticD[i].flags = (analyticD[i].flags & ~MI_MATERIAL_FLAG_BITS) | materialFlagTable[analytic[i].bsdf];
        if (flagsChanged) *flagsChanged = true;
    }
    ++revision;
    return MI_OK;
}
int SceneHost::updateEmitters(const mi_emitter *e, uint32_t n, std::string &msg) {
    if (!e || !n) { msg = "mi_scene_update_emitters: null argument"; return MI_ERR_INVALID; }
    if (!committed) { msg = "mi_scene_update_emitters: scene not committed"; return MI_ERR_INVALID; }
    if (n != emitters.size()) { msg = "mi_scene_update_emitters: the record count changes (" + std::to_string(emitters.size()) + " -> " + std::to_string(n) + "); commit a new scene"; return MI_ERR_UNSUPPORTED; }
    for (uint32_t i = 0; i < n; ++i) {
        const char *what = emitters[i].type != e[i].type ? "its type" : emitters[i].shape != e[i].shape ? "its shape" : nullptr;
        if (what) { msg = "mi_scene_update_emitters: emitter " + std::to_string(i) + " changes " + what + "; an update changes values only, commit a new scene"; return MI_ERR_UNSUPPORTED; }
    }
    { const int rc = validateEmitters(e, n, msg); if (rc) return rc; }
    emitters.assign(e, e + n);
    buildEmitterTables(); syncEmittersD(); ++revision;
    return MI_OK;
}
int SceneHost::updateEnvmapTransform(const float *toWorld16, float scale, std::string &msg) {
    if (!toWorld16) { msg = "mi_scene_update_envmap_transform: null argument"; return MI_ERR_INVALID; }
    if (!committed) { msg = "mi_scene_update_envmap_transform: scene not committed"; return MI_ERR_INVALID; }
    if (envIndex < 0 || envConstant) { msg = "mi_scene_update_envmap_transform: the scene has no envmap emitter"; return MI_ERR_INVALID; }
    memcpy(envToWorld, toWorld16, 64); envScale = scale;
    buildEnvTransform(); syncEnvD(); ++revision;      // the CDFs are over unscaled luminance: they stay
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ geometry edits (mi_scene_update_vertices, _instances, _geometry)
// What a vertex or an instance edit needs beyond the committed tables, derived once at the first edit: where each triangle's and each instance's leaf record sits, the
// padded boxes of the leaf records that the edit's kernel does not write (analytic shapes; on a scene with instances, where only instances move, also the triangles;
// the never-hit record of unused 4-wide slots stays empty), and the order in which the existing nodes are refitted -- by height, height 0 = every child is a leaf,
// so that a node comes after all of its inner children.  The walk starts at node 0 and an instance is a leaf, so that order (refitOrder) covers the scene-level tree
// only; a second order (refitOrderAll, for mi_scene_update_geometry) repeats the walk from every group root and covers every tree.
void SceneHost::prepareGeometryEdit() {
    const uint32_t nt = nTris; const float inf = std::numeric_limits<float>::infinity();
    leafSlotOfPrim.assign(nt, 0u); leafSlotOfInstance.assign(instances.size(), 0u); leafBoxes.assign(tris.size() * 6, 0.0f);
    for (size_t slot = 0; slot < tris.size(); ++slot) {
        const TriAccelD &r = tris[slot]; float *box = &leafBoxes[slot * 6];
        store3(box, mk(inf, inf, inf)); store3(box + 3, mk(-inf, -inf, -inf));
        if (r.k == MI_K_ANALYTIC && r.prim >= nt && r.prim - nt < analytic.size()) {
            AnalyticD d; V3 alo, ahi, tl, th, plo, phi, cen; analyticPrepare(analytic[r.prim - nt], d, alo, ahi, tl, th); padBox(tl, th, plo, phi, cen);
            store3(box, plo); store3(box + 3, phi);
        } else if (r.k == MI_K_INSTANCE && r.prim < instances.size()) {
            leafSlotOfInstance[r.prim] = (uint32_t) slot;
            const InstanceD &in = instancesD[r.prim]; V3 blo, bhi, plo, phi, cen; instanceBoxes(in.to_world, load3(in.glo), load3(in.ghi), blo, bhi, plo, phi, cen);
            store3(box, plo); store3(box + 3, phi);
        } else if (r.k <= MI_K_NONE && r.prim < nt) {
            leafSlotOfPrim[r.prim] = (uint32_t) slot;
            if (!instances.empty() && !shapes[triShape[r.prim]].group) {      // no k_tri_records on a scene with instances: the refit reads the scene-level triangles' boxes from here
                V3 plo, phi, cen; triPaddedBox(load3(&pos[(size_t) idx[(size_t) r.prim * 3] * 3]), load3(&pos[(size_t) idx[(size_t) r.prim * 3 + 1] * 3]), load3(&pos[(size_t) idx[(size_t) r.prim * 3 + 2] * 3]), plo, phi, cen);
                store3(box, plo); store3(box + 3, phi);
            }
        }
    }
    const size_t nn = nodes.size(); std::vector<int> height(nn, -1);
    struct Walk { const std::vector<BvhNode> &nodes; std::vector<int> &height; bool wide;
        int of(int32_t n) {
            int h = 0;
            if (wide) { Bvh4Node w; std::memcpy(&w, &nodes[n], sizeof(w)); for (int c = 0; c < 4; ++c) if (!wideSlotUnused(w, c) && w.child[c] >= 0) h = std::max(h, of(w.child[c]) + 1); }
            else { const BvhNode &b = nodes[n]; if (b.c0 >= 0) h = std::max(h, of(b.c0) + 1); if (b.c1 >= 0) h = std::max(h, of(b.c1) + 1); }
            height[n] = h; return h;
        } } walk{nodes, height, wideBvh};
    int top = nn ? walk.of(0) : -1;
    auto byHeight = [&](std::vector<uint32_t> &order, std::vector<uint32_t> &levelStart) {      // counting sort of the nodes walked so far
        levelStart.assign((size_t) top + 2, 0u); order.clear();
        for (size_t i = 0; i < nn; ++i) if (height[i] >= 0) ++levelStart[(size_t) height[i] + 1];
        for (size_t l = 1; l < levelStart.size(); ++l) levelStart[l] += levelStart[l - 1];
        order.resize(levelStart.back());
        std::vector<uint32_t> fill(levelStart.begin(), levelStart.end() - 1); for (size_t i = 0; i < nn; ++i) if (height[i] >= 0) order[fill[(size_t) height[i]]++] = (uint32_t) i;
    };
    byHeight(refitOrder, refitLevelStart);
    // the geometry edit's order: the group trees as well, each walked from its own root.  The trees are disjoint, and an instance's leaf box comes from the group box
    // (a vertex min / max), not from the group tree's root, so nodes of equal height share a level whatever tree they belong to.
    for (int root : groupRoot) if (root >= 0 && (size_t) root < nn && height[root] < 0) top = std::max(top, walk.of(root));
    byHeight(refitOrderAll, refitLevelStartAll);
    nodeBoxes.assign(nn * 6, 0.0f);
    geoPrepared = true;
}
// The scan over every vertex of every edit: one pass over both arrays, position before normal, in a function of its own.  Inside checkGeometry() the same loop ran
// 15 % slower, and as two passes (positions, then normals) it cost the call 0.1 ms on a 150 000-vertex mesh, a quarter of the host side of a vertex edit.
static size_t firstNonFinite(const float *pos, const float *nrm, size_t n, bool &normal) {
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(pos[i])) { normal = false; return i; }
        if (nrm && !std::isfinite(nrm[i])) { normal = true; return i; }
    }
    return n;
}
// One check for mi_scene_update_vertices, _instances and _geometry.  `entry` starts every message and turns on the two refusals that only the vertex call makes:
// it refits neither group boxes nor group trees by contract.
int SceneHost::checkGeometry(GeoEntry entry, const float *posIn, const float *nrmIn, uint32_t nVerts, const mi_instance *in, uint32_t nInstances, std::string &msg) const {
    const std::string who = std::string(geoEntryName(entry)) + ": "; const bool verticesOnly = entry == GeoEntry::Vertices;
    if (!posIn && !in) { msg = who + (entry == GeoEntry::Geometry ? "null argument: neither vertices nor instances given" : "null argument"); return MI_ERR_INVALID; }
    if (!committed) { msg = who + "scene not committed"; return MI_ERR_INVALID; }
    if (!posIn && (nrmIn || nVerts)) { msg = who + "null argument: normals or a vertex count without positions"; return MI_ERR_INVALID; }
    if (posIn) {
        if (verticesOnly && !instances.empty()) { msg = who + "instance 0 (of shape group " + std::to_string(instances[0].group) + "): group boxes, instance boxes and the two-level tree are not refitted; commit a new scene"; return MI_ERR_UNSUPPORTED; }
        if (verticesOnly) for (size_t i = 0; i < shapes.size(); ++i) if (shapes[i].group) { msg = who + "shape " + std::to_string(i) + " is a member of shape group " + std::to_string(shapes[i].group - 1) + " (instances): group boxes are not refitted; commit a new scene"; return MI_ERR_UNSUPPORTED; }
        if ((size_t) nVerts * 3 != pos.size() || !nTris) { msg = who + "the vertex count changes (" + std::to_string(pos.size() / 3) + " -> " + std::to_string(nVerts) + "); an update moves the committed vertices, commit a new scene"; return MI_ERR_INVALID; }
        if (nrmIn && nrm.empty()) { msg = who + "vertex normals given, but the scene was committed without normals"; return MI_ERR_INVALID; }
        if (!nrmIn && !nrm.empty()) { msg = who + "the scene was committed with vertex normals: new normals are required"; return MI_ERR_INVALID; }
        bool normal = false; const size_t n3 = (size_t) nVerts * 3, bad = firstNonFinite(posIn, nrmIn, n3, normal);
        if (bad < n3) { msg = who + "vertex " + std::to_string(bad / 3) + (normal ? " has a non-finite normal" : " has a non-finite position"); return MI_ERR_INVALID; }
    }
    if (in) {
        const uint32_t n = nInstances;
        if (instances.empty()) { msg = who + "the scene has no instances"; return MI_ERR_INVALID; }
        if (n != instances.size()) { msg = who + "the instance count changes (" + std::to_string(instances.size()) + " -> " + std::to_string(n) + "); an update moves the committed instances, commit a new scene"; return MI_ERR_INVALID; }
        for (uint32_t i = 0; i < n; ++i) for (int k = 0; k < 16; ++k) {
            if (!std::isfinite(in[i].to_world[k])) { msg = who + "instance " + std::to_string(i) + " has a non-finite to_world"; return MI_ERR_INVALID; }
            if (!std::isfinite(in[i].to_object[k])) { msg = who + "instance " + std::to_string(i) + " has a non-finite to_object"; return MI_ERR_INVALID; }
        }
        for (uint32_t i = 0; i < n; ++i) if (in[i].group != instances[i].group) {
            msg = who + "instance " + std::to_string(i) + " changes its shape group (" + std::to_string(instances[i].group) + " -> " + std::to_string(in[i].group) + "): that selects another tree; an update changes transforms only, commit a new scene"; return MI_ERR_UNSUPPORTED; }
    } else if (nInstances) { msg = who + "null argument: an instance count without instances"; return MI_ERR_INVALID; }
    return MI_OK;
}
int SceneHost::updateVertices(const float *posIn, const float *nrmIn, uint32_t nVerts, std::string &msg) {
    { const int rc = checkGeometry(GeoEntry::Vertices, posIn, nrmIn, nVerts, nullptr, 0, msg); if (rc) return rc; }
    applyGeometry(posIn, nrmIn, nVerts, nullptr, 0); return MI_OK;
}
int SceneHost::updateInstances(const mi_instance *in, uint32_t n, std::string &msg) {
    { const int rc = checkGeometry(GeoEntry::Instances, nullptr, nullptr, 0, in, n, msg); if (rc) return rc; }
    applyGeometry(nullptr, nullptr, 0, in, n); return MI_OK;
}
int SceneHost::updateGeometry(const float *posIn, const float *nrmIn, uint32_t nVerts, const mi_instance *in, uint32_t nInstances, std::string &msg) {
    { const int rc = checkGeometry(GeoEntry::Geometry, posIn, nrmIn, nVerts, in, nInstances, msg); if (rc) return rc; }
    applyGeometry(posIn, nrmIn, nVerts, in, nInstances); return MI_OK;
}
// The commit's own pieces in the commit's order, each only where its inputs changed: group boxes, emitter tables and packet tables are functions of pos, idx, shapes
// and emitters alone, so without new vertices they are current and stay.
void SceneHost::applyGeometry(const float *posIn, const float *nrmIn, uint32_t nVerts, const mi_instance *in, uint32_t nInstances) {
    if (!geoPrepared) prepareGeometryEdit();      // reads topology, leaf slots and the boxes of records that never move: valid whatever was edited before
    if (posIn) { pos.assign(posIn, posIn + (size_t) nVerts * 3); if (nrmIn) nrm.assign(nrmIn, nrmIn + (size_t) nVerts * 3); }
    if (in) instances.assign(in, in + nInstances);
    if (posIn) buildGroupBoxes();
    // the scene box takes the unpadded instance boxes in instance order, as commitHost() does: the same sequence of min / max, down to the sign of a zero
    const uint32_t ni = (uint32_t) instances.size(); std::vector<float> instBoxes((size_t) ni * 6);
    for (uint32_t i = 0; i < ni; ++i) {
        const float *gb = &groupBoxes[(size_t) instances[i].group * 6]; V3 blo, bhi, plo, phi, cen;      // the group boxes of the current vertices (instancesD may be stale)
        instanceBoxes(instances[i].to_world, load3(gb), load3(gb + 3), blo, bhi, plo, phi, cen);
        store3(&instBoxes[(size_t) i * 6], blo); store3(&instBoxes[(size_t) i * 6 + 3], bhi);
    }
    buildSceneBox(instBoxes.data(), ni);
    if (posIn && !ni) { buildPacketTables(); for (int i = 0; i < 3; ++i) d.packet_gk[i] = packetGK[i]; d.packet_scale = packetScale; }      // a scene with instances never runs in packet mode
    if (posIn) buildEmitterTables();      // scene-level mesh lights may move (group members cannot be emitters)
    buildBoundingSpheres();
    for (int i = 0; i < 3; ++i) { d.aabb_lo[i] = aabbLo[i]; d.aabb_hi[i] = aabbHi[i]; }
    syncCameraD(); syncEmittersD();
    if (posIn) geoStale = true;      // tris, shade, triuv, packetExact, every tree
    if (ni) instStale = true;        // instancesD (glo / ghi follow the vertices, the matrices the instances), the scene-level tree
    ++revision;
}
std::vector<float> SceneHost::instanceTransformPairs() const {
    std::vector<float> xf(instances.size() * 24);
    for (size_t i = 0; i < instances.size(); ++i) { std::memcpy(&xf[i * 24], instances[i].to_world, 48); std::memcpy(&xf[i * 24 + 12], instances[i].to_object, 48); }
    return xf;
}
GeoEditTables SceneHost::geoEditTables(bool dev) {
    GeoEditTables g{};
    g.pos = dev ? (const float *) dPos : pos.data(); g.nrm = nrm.empty() ? nullptr : dev ? (const float *) dNrm : nrm.data();
    g.shade = dev ? (TriShade *) dShade : shade.data(); g.triuv = triuv.empty() ? nullptr : dev ? (TriUV *) dTriUV : triuv.data();
    g.tris = dev ? const_cast<TriAccelD *>(d.tris) : tris.data(); g.packetExact = dev ? (TriAccelD *) dPacketExact : packetExact.data();
    g.leafSlot = dev ? (const uint32_t *) dLeafSlot : leafSlotOfPrim.data(); g.leafBox = dev ? (float *) dLeafBox : leafBoxes.data();
    g.nodes = dev ? (BvhNode *) dNodes : nodes.data(); g.nodeBox = dev ? (float *) dNodeBox : nodeBoxes.data();
    g.nTris = nTris; g.nPacketExact = (uint32_t) std::min<size_t>(packetExact.size(), nTris); g.wide = wideBvh ? 1u : 0u;
    return g;
}
// withGroupBoxes: the groups' boxes of the current vertices go into the records' glo / ghi first; without them the records' own are taken to be current
InstEditTables SceneHost::instEditTables(bool dev, const float *xf, bool withGroupBoxes) {
    InstEditTables it{}; it.xf = xf; it.inst = dev ? (InstanceD *) dInstances : instancesD.data(); it.n = (uint32_t) instancesD.size();
    it.leafSlot = dev ? (const uint32_t *) dLeafSlotInst : leafSlotOfInstance.data(); it.leafBox = dev ? (float *) dLeafBox : leafBoxes.data();
    if (withGroupBoxes) { it.groupBox = dev ? (const float *) dGroupBox : groupBoxes.data(); it.nGroups = (uint32_t) (groupBoxes.size() / 6); }
    return it;
}
// The host mirrors of the per-triangle records, of the instance records and of the trees after geometry edits, in any interleaving: the steps the device runs
// (geometry_records.h), in the device's order, from the CURRENT inputs -- triangle records, group boxes into the instance records, instance records, then the refit:
// over every tree when vertices moved, over the scene level alone otherwise.
void SceneHost::refreshHostGeometry() {
    if (!geoStale && !instStale) return;
    const GeoEditTables g = geoEditTables(false);
    if (geoStale) for (uint32_t t = 0; t < nTris; ++t) geoTriRecord(g, t);
    if (instStale) {
        const std::vector<float> xf = instanceTransformPairs();
        const InstEditTables it = instEditTables(false, xf.data(), true);      // the group boxes of the current vertices: the committed ones' unless an edit moved them
        for (uint32_t i = 0; i < it.n; ++i) geoInstanceRecord(it, i);
    }
    for (uint32_t n : (geoStale ? refitOrderAll : refitOrder)) geoRefitNode(g, n);
    geoStale = instStale = false;
}

int validateMaterials(const mi_material *m, uint32_t n, std::string &msg) {
    auto fail = [&](int code, const char *text) { msg = text; return code; };
    auto isWrapper = [](uint32_t t) { return t == MI_BSDF_MASK || t == MI_BSDF_MIXTURE || t == MI_BSDF_BUMPMAP || t == MI_BSDF_NORMALMAP || t == MI_BSDF_COATING || t == MI_BSDF_BLEND || t == MI_BSDF_ROUGHCOATING; };
    auto hasDelta = [](uint32_t t) { return t == MI_BSDF_CONDUCTOR || t == MI_BSDF_DIELECTRIC || t == MI_BSDF_THINDIELECTRIC || t == MI_BSDF_PLASTIC; };
    for (uint32_t i = 0; i < n; ++i) {
        if (m[i].type > MI_BSDF_ROUGHCOATING) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: implemented BSDFs: diffuse, roughdiffuse, phong, ward, coating, roughcoating, blendbsdf, roughconductor, conductor, dielectric, plastic, roughdielectric, difftrans, roughplastic, thindielectric, mask, mixturebsdf, bumpmap, normalmap (those without transmission optionally twosided)");
        if (m[i].type == MI_BSDF_MASK && (m[i].distr >= n || m[m[i].distr].type == MI_BSDF_MASK || (m[i].flags & MI_BSDF_FLAG_TWOSIDED))) return fail(MI_ERR_INVALID, "mi_scene_set_materials: a mask refers to its nested material record by index (not another mask) and cannot itself be twosided");
        if (m[i].type == MI_BSDF_BLEND) {
            int deltas = 0;
            for (int c = 0; c < 2; ++c) {
                const float idxf = m[i].eta[c];
                if (!(idxf >= 0) || idxf >= (float) n || isWrapper(m[(uint32_t) idxf].type)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: the two BSDFs of a blendbsdf are plain BSDF records (indices in eta[0], eta[1])");
                if (((m[(uint32_t) idxf].flags >> 8) & 0xFFFFu)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: textures on the BSDFs inside a blendbsdf are not implemented");
                deltas += hasDelta(m[(uint32_t) idxf].type);
            }
            if (deltas > 1) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a blendbsdf of two BSDFs that both have a Dirac delta component is not implemented");
        }
        if (m[i].type == MI_BSDF_ROUGHCOATING) {
            if (m[i].distr >= n || isWrapper(m[m[i].distr].type)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a roughcoating nests a plain BSDF record (index in `distr`)");
            const mi_material &nm = m[m[i].distr];
            if ((nm.flags & MI_BSDF_FLAG_TWOSIDED) || hasDelta(nm.type) || nm.type == MI_BSDF_ROUGHDIELECTRIC || nm.type == MI_BSDF_DIFFTRANS || nm.type == MI_BSDF_NULL)
                return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: the BSDF under a roughcoating is a reflective one without a Dirac delta lobe, `twosided` goes on the coating");
            if (!(m[i].eta[0] > 0) || m[i].eta[0] == 1.0f) return fail(MI_ERR_INVALID, "The interior and exterior indices of refraction must be positive and differ!");      // roughcoating.cpp:126-128
            if (m[i].eta[2] != 0.0f && m[i].eta[2] != 1.0f && m[i].eta[2] != 2.0f) return fail(MI_ERR_INVALID, "Specified an invalid distribution, must be \"beckmann\", \"ggx\", or \"phong\"/\"as\"!");
            if ((m[i].flags >> 8) & 0xFFFFu) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a textured sigmaA is not implemented");
        }
        if (m[i].type == MI_BSDF_COATING) {
            // adapters nest in the order mask -> bumpmap / normalmap -> coating -> plain BSDF (a coating over a mixturebsdf, or as the child of one, is not implemented)
            if (m[i].distr >= n || isWrapper(m[m[i].distr].type)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a coating nests a plain BSDF record (index in `distr`)");
            const mi_material &nm = m[m[i].distr];
            if ((nm.flags & MI_BSDF_FLAG_TWOSIDED) || nm.type == MI_BSDF_DIELECTRIC || nm.type == MI_BSDF_ROUGHDIELECTRIC || nm.type == MI_BSDF_DIFFTRANS || nm.type == MI_BSDF_THINDIELECTRIC || nm.type == MI_BSDF_NULL)
                return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: the BSDF under a coating is a reflective one, `twosided` goes on the coating");
            if (!(m[i].eta[0] > 0) || m[i].eta[0] == 1.0f) return fail(MI_ERR_INVALID, "The interior and exterior indices of refraction must be positive and differ!");      // coating.cpp:119-121
            if ((m[i].flags >> 8) & 0xFFFFu) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a textured sigmaA is not implemented");
        }
        if (m[i].type == MI_BSDF_BUMPMAP || m[i].type == MI_BSDF_NORMALMAP) {
            // adapters nest in the order mask -> bumpmap / normalmap -> mixturebsdf -> plain BSDF
            if (m[i].distr >= n || m[m[i].distr].type == MI_BSDF_MASK || m[m[i].distr].type == MI_BSDF_BUMPMAP || m[m[i].distr].type == MI_BSDF_NORMALMAP) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a bumpmap / normalmap nests a plain BSDF or a mixturebsdf (record index in `distr`)");
            if (m[i].flags & MI_BSDF_FLAG_TWOSIDED) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: put `twosided` on the BSDF nested in a bumpmap / normalmap, not on the adapter");
            if (!((m[i].flags >> 8) & 0xFFFFu)) return fail(MI_ERR_INVALID, m[i].type == MI_BSDF_BUMPMAP ? "A displacement texture must be specified" : "A normal map texture must be specified");   // bumpmap.cpp:88-89
        }
        if (m[i].type == MI_BSDF_MIXTURE) {
            if (m[i].distr < 2 || m[i].distr > 4) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a mixturebsdf holds 2..4 BSDFs");
            float total = 0; int deltas = 0;
            for (uint32_t c = 0; c < m[i].distr; ++c) {
                const float idxf = c < 3 ? m[i].reflectance[c] : m[i].eta[0], w = c < 3 ? m[i].k[c] : m[i].specular[0];
                if (!(idxf >= 0) || idxf >= (float) n || isWrapper(m[(uint32_t) idxf].type)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: the children of a mixturebsdf are plain BSDF records (indices in reflectance[0..2], eta[0])");
                if (((m[(uint32_t) idxf].flags >> 8) & 0xFFFFu)) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: textures on the children of a mixturebsdf are not implemented");
                if (!(w >= 0)) return fail(MI_ERR_INVALID, "Invalid BSDF weight!");                                    // mixturebsdf.cpp:82-83
                total += w; deltas += hasDelta(m[(uint32_t) idxf].type);
            }
            if (!(total > 0)) return fail(MI_ERR_INVALID, "The weights must sum to a value greater than zero!");       // mixturebsdf.cpp:126-127
            if (deltas > 1) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: a mixturebsdf with more than one child that has a Dirac delta component is not implemented");
        }
        if ((m[i].type == MI_BSDF_DIELECTRIC || m[i].type == MI_BSDF_ROUGHDIELECTRIC || m[i].type == MI_BSDF_DIFFTRANS || m[i].type == MI_BSDF_THINDIELECTRIC) && (m[i].flags & MI_BSDF_FLAG_TWOSIDED)) return fail(MI_ERR_INVALID, "Only BSDFs without a transmission component can be nested!");   // twosided.cpp:86-88
        if ((m[i].type == MI_BSDF_DIELECTRIC || m[i].type == MI_BSDF_PLASTIC || m[i].type == MI_BSDF_ROUGHDIELECTRIC || m[i].type == MI_BSDF_ROUGHPLASTIC || m[i].type == MI_BSDF_THINDIELECTRIC) && !(m[i].eta[0] > 0)) return fail(MI_ERR_INVALID, "The interior and exterior indices of refraction must be positive!");
        if (m[i].type == MI_BSDF_ROUGHPLASTIC && (m[i].distr > 2 || (m[i].flags & MI_BSDF_FLAG_ANISOTROPIC)))
            return fail(MI_ERR_INVALID, "The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!");        // roughplastic.cpp:225-227
        if ((m[i].type == MI_BSDF_ROUGHCONDUCTOR || m[i].type == MI_BSDF_ROUGHDIELECTRIC) && m[i].distr > 2) return fail(MI_ERR_INVALID, "Specified an invalid distribution, must be \"beckmann\", \"ggx\", or \"phong\"/\"as\"!");   // microfacet.h:113-115
        if ((m[i].flags & MI_BSDF_FLAG_ANISOTROPIC) && m[i].type != MI_BSDF_ROUGHCONDUCTOR && m[i].type != MI_BSDF_ROUGHDIELECTRIC && m[i].type != MI_BSDF_WARD) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_materials: anisotropic roughness is implemented for roughconductor and roughdielectric");
    }
    return MI_OK;
}
int validateEmitters(const mi_emitter *e, uint32_t n, std::string &msg) {
    auto fail = [&](int code, const char *text) { msg = text; return code; };
    uint32_t nEnv = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (e[i].type > MI_EMITTER_COLLIMATED || e[i].type == 6u) return fail(MI_ERR_UNSUPPORTED, "mi_scene_set_emitters: implemented emitters: area, envmap, constant, point, spot, directional, collimated");
        nEnv += e[i].type == MI_EMITTER_ENVMAP || e[i].type == MI_EMITTER_CONSTANT;
        if (e[i].type == MI_EMITTER_SPOT && !(e[i].cutoff >= e[i].beam && e[i].beam >= 0 && e[i].cutoff > 0)) return fail(MI_ERR_INVALID, "mi_scene_set_emitters: spot needs cutoffAngle >= beamWidth >= 0");   // spot.cpp:77
    }
    if (nEnv > 1) return fail(MI_ERR_INVALID, "The scene may only contain one environment emitter");      // scene.cpp:542-543
    return MI_OK;
}

}  // namespace mi
