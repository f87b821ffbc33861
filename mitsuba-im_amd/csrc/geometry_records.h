// geometry_records.h -- the arithmetic that turns vertex positions into device records, once, for the host and for the device.
//
// mi_scene_commit derives these records on the host (scene_build.cpp, commitHost()); mi_scene_update_vertices, _instances and _geometry derive them again on the
// device (kernels_geometry.hip) and, when a host mirror is needed, on the host (SceneHost::refreshHostGeometry()).  "After an update every result equals that of a fresh commit" holds bit for bit only
// if all three run the very same operations in the very same order, so they all call the functions below.  Everything here is strict IEEE binary32 / binary64: the
// translation units that include it are compiled with -ffp-contract=off and correctly rounded divide / square root on both sides.  min / max are the ternaries of
// std::min / std::max (they differ from fminf / fmaxf on NaN and on signed zeros).
//
// Reference: TriAccel::load (include/mitsuba/render/triaccel.h:61-94), face frame (skdtree.h:367-371, util.cpp:605-610), TriMesh::computeUVTangents
// (src/librender/trimesh.cpp:683-736), coordinateSystem (util.cpp:594-603).
#pragma once
#include "pt_types.h"
#include <cmath>
#include <cstring>

#define MI_HD __host__ __device__

#define MI_K_NONE 3u                    // TriAccelD::k of a record that is never hit (the value triaccelLoad gives degenerate triangles)

namespace mi {

struct V3 { float x, y, z; };
MI_HD static inline V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
MI_HD static inline V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
MI_HD static inline V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
MI_HD static inline V3 operator*(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
MI_HD static inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
MI_HD static inline V3 cross(V3 a, V3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
MI_HD static inline float comp(V3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
MI_HD static inline float minOf(float a, float b) { return b < a ? b : a; }      // std::min
MI_HD static inline float maxOf(float a, float b) { return a < b ? b : a; }      // std::max
MI_HD static inline int minOf(int a, int b) { return b < a ? b : a; }
MI_HD static inline int maxOf(int a, int b) { return a < b ? b : a; }
MI_HD static inline float absOf(float a) { return fabsf(a); }
MI_HD static inline float sqrtOf(float a) { return sqrtf(a); }
MI_HD static inline V3 normalize(V3 a) { float inv = 1.0f / sqrtOf(dot(a, a)); return a * inv; }
MI_HD static inline V3 vmin(V3 a, V3 b) { return mk(minOf(a.x, b.x), minOf(a.y, b.y), minOf(a.z, b.z)); }
MI_HD static inline V3 vmax(V3 a, V3 b) { return mk(maxOf(a.x, b.x), maxOf(a.y, b.y), maxOf(a.z, b.z)); }
MI_HD static inline V3 load3(const float *p) { return mk(p[0], p[1], p[2]); }
MI_HD static inline void store3(float *p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

// reference include/mitsuba/render/triaccel.h:61-94.  `prim` and `pad` are left zero: the caller numbers the record.
MI_HD static inline void triaccelLoad(TriAccelD &ta, V3 A, V3 B, V3 C) {
    V3 b = C - A, c = B - A, N = cross(c, b);
    int k = 0;
    for (int j = 0; j < 3; ++j) if (absOf(comp(N, j)) > absOf(comp(N, k))) k = j;
    const int u = k == 0 ? 1 : (k == 1 ? 2 : 0), v = k == 0 ? 2 : (k == 1 ? 0 : 1);      // the Wald axes {1, 2, 0, 1}[k], [k + 1]
    float n_k = comp(N, k), denom = comp(b, u) * comp(c, v) - comp(b, v) * comp(c, u);
    ta.k = 0; ta.n_u = ta.n_v = ta.n_d = 0.0f; ta.a_u = ta.a_v = ta.b_nu = ta.b_nv = 0.0f; ta.c_nu = ta.c_nv = 0.0f; ta.prim = 0; ta.pad = 0;
    if (denom == 0) { ta.k = MI_K_NONE; return; }
    ta.k = (uint32_t) k;
    ta.n_u = comp(N, u) / n_k; ta.n_v = comp(N, v) / n_k; ta.n_d = dot(A, N) / n_k;
    ta.b_nu = comp(b, u) / denom; ta.b_nv = -comp(b, v) / denom;
    ta.a_u = comp(A, u); ta.a_v = comp(A, v);
    ta.c_nu = comp(c, v) / denom; ta.c_nv = -comp(c, u) / denom;
}

// The geometric words of a triangle's shading record: p0..p2, the face normal ng and the face frame (s, t).  With a TriUV record (the mesh has texture coordinates;
// its uv0..uv2 are already in place) the UV tangents go into it and dpdu replaces the first edge in the frame.  A smooth triangle's caller then overwrites s, t, n2
// with its three vertex normals.  material, emitter, flags, local_prim, i0..i2 and pad are not touched.
MI_HD static inline void triShadeGeometry(TriShade &ts, TriUV *tu, V3 p0, V3 p1, V3 p2) {
    store3(ts.p0, p0); store3(ts.p1, p1); store3(ts.p2, p2);
    // face frame: skdtree.h:367-371 (face normal), util.cpp:605-610 (computeShadingFrame with dpdu = p1 - p0)
    V3 side1 = p1 - p0, side2 = p2 - p0, fn = cross(side1, side2);
    float len = sqrtOf(dot(fn, fn));
    if (!(fn.x == 0 && fn.y == 0 && fn.z == 0)) { float r = 1.0f / len; fn = fn * r; }
    V3 dpdu = side1;
    if (tu) {                                                // TriMesh::computeUVTangents (trimesh.cpp:683-736)
        float du1 = tu->uv1[0] - tu->uv0[0], dv1 = tu->uv1[1] - tu->uv0[1], du2 = tu->uv2[0] - tu->uv0[0], dv2 = tu->uv2[1] - tu->uv0[1];
        V3 n = cross(side1, side2); float length = sqrtOf(dot(n, n)); V3 tdu = mk(0, 0, 0), tdv = mk(0, 0, 0);
        if (length != 0) {
            float determinant = du1 * dv2 - dv1 * du2;
            if (determinant == 0) {                         // coordinateSystem(n / length, dpdu, dpdv), util.cpp:594-603
                float r = 1.0f / length; V3 an = n * r;
                if (absOf(an.x) > absOf(an.y)) { float invLen = 1.0f / sqrtOf(an.x * an.x + an.z * an.z); tdv = mk(an.z * invLen, 0.0f, -an.x * invLen); }
                else { float invLen = 1.0f / sqrtOf(an.y * an.y + an.z * an.z); tdv = mk(0.0f, an.z * invLen, -an.y * invLen); }
                tdu = cross(tdv, an);
            } else {
                float invDet = 1.0f / determinant;
                tdu = (side1 * dv2 - side2 * dv1) * invDet;
                tdv = (side1 * (-du2) + side2 * du1) * invDet;
            }
        }
        store3(tu->dpdu, tdu); store3(tu->dpdv, tdv);
        dpdu = tdu;
    }
    V3 s = normalize(dpdu - fn * dot(fn, dpdu)), tt = cross(fn, s);
    store3(ts.ng, fn); store3(ts.s, s); store3(ts.t, tt);
}

// Conservative padding of a primitive's box: the Wald test is evaluated in its own arithmetic, boxes may only over-approximate.  cen = centre of the unpadded box.
MI_HD static inline void padBox(V3 lo, V3 hi, V3 &plo, V3 &phi, V3 &cen) {
    V3 e = hi - lo; float mag = maxOf(maxOf(absOf(lo.x) + absOf(hi.x), absOf(lo.y) + absOf(hi.y)), absOf(lo.z) + absOf(hi.z));
    float pad = 1e-4f * maxOf(maxOf(e.x, e.y), e.z) + 2e-5f * mag + 1e-7f;
    plo = lo - mk(pad, pad, pad); phi = hi + mk(pad, pad, pad); cen = (lo + hi) * 0.5f;
}
MI_HD static inline void triPaddedBox(V3 p0, V3 p1, V3 p2, V3 &plo, V3 &phi, V3 &cen) {
    V3 lo = vmin(vmin(p0, p1), p2), hi = vmax(vmax(p0, p1), p2);
    padBox(lo, hi, plo, phi, cen);
}

// A point through rows 0..2 of a row-major affine matrix (3 x 4 or 4 x 4).
MI_HD static inline V3 xfPoint(const float *m, V3 p) { return mk(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7], m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]); }
// Box of one placement of a shape group = the 8 transformed corners of the group's box (instance.cpp:46-64): [blo, bhi] is what the scene box takes, [plo, phi] the
// padded box of the instance's leaf record in the scene-level tree.
MI_HD static inline void instanceBoxes(const float *toWorld, V3 glo, V3 ghi, V3 &blo, V3 &bhi, V3 &plo, V3 &phi, V3 &cen) {
    const float inf = INFINITY; blo = mk(inf, inf, inf); bhi = mk(-inf, -inf, -inf);
    for (int c = 0; c < 8; ++c) {
        V3 q = xfPoint(toWorld, mk(c & 1 ? ghi.x : glo.x, c & 2 ? ghi.y : glo.y, c & 4 ? ghi.z : glo.z));
        blo = vmin(blo, q); bhi = vmax(bhi, q);
    }
    padBox(blo, bhi, plo, phi, cen);
}

// ---- 4-wide nodes: child box c = org + q * step per axis (pt_types.h Bvh4Node)
// Biased exponent of the step of one axis: 2^(e - 127) is the smallest power of two with 254 steps covering the extent, clamped to the normal floats.  This is
// frexp(ext > 0 ? ext / 254 : 1e-30f) read off the bit pattern: a normal float m 2^(E - 127), m in [1, 2), is m / 2 * 2^(E - 126); anything below the normal range
// clamps to 1 either way.  tests/host/geometry_edit_host.cpp pins this, wideStepOf and triaccelLoad against the builder's original wording (std::frexp, std::ldexp, memset + wald[]).
MI_HD static inline int wideStepExponent(float ext) {
    const float x = ext > 0 ? ext / 254.0f : 1e-30f;
    uint32_t bits; memcpy(&bits, &x, 4);
    const int E = (int) ((bits >> 23) & 0xFFu);
    const int e = (E == 255 || x == 0) ? 0 : E - 126;     // frexp leaves the exponent at 0 for an infinite extent (overflowed coordinates) and for a zero (an extent so small that ext / 254 underflows)
    return minOf(maxOf(e + 127, 1), 254);
}
MI_HD static inline float wideStepOf(int e) { const uint32_t bits = (uint32_t) e << 23; float s; memcpy(&s, &bits, 4); return s; }      // ldexp(1.0f, e - 127), 1 <= e <= 254
// org and the three steps of a node whose children span [lo, hi]; clears the quantised words.  ex[3] = the biased step exponents for wideNodeChild.
MI_HD static inline void wideNodeFrame(Bvh4Node &w, V3 lo, V3 hi, int ex[3]) {
    w.org[0] = lo.x; w.org[1] = lo.y; w.org[2] = lo.z;
    for (int a = 0; a < 3; ++a) {      // step 2^e with 255 steps covering the extent (+ one step of slack for the rounding of org + q * step)
        const float ext = comp(hi, a) - comp(lo, a); const int e = wideStepExponent(ext);
        ex[a] = e; const float st = wideStepOf(e);
        if (a == 0) w.step_x = st; else if (a == 1) w.step_y = st; else w.step_z = st;
        w.qlo[a] = 0; w.qhi[a] = 0;
    }
}
MI_HD static inline void wideNodeUnused(Bvh4Node &w, int c) { for (int a = 0; a < 3; ++a) w.qlo[a] |= 255u << (8 * c); }      // inverted box: lo 255, hi 0
MI_HD static inline bool wideSlotUnused(const Bvh4Node &w, int c) { return ((w.qlo[0] >> (8 * c)) & 0xFFu) == 255u && ((w.qhi[0] >> (8 * c)) & 0xFFu) == 0u; }   // a real child has qlo <= qhi
// quantises child c's box [klo, khi] against the node's frame (lo = the node's org): lo rounded down, hi rounded up, then fixed up until the FLOAT reconstruction
// org + q * step the walks compute encloses the child box
MI_HD static inline void wideNodeChild(Bvh4Node &w, int c, const int ex[3], V3 lo, V3 klo, V3 khi) {
    for (int a = 0; a < 3; ++a) {
        const uint32_t sbits = (uint32_t) ex[a] << 23; float stepf; memcpy(&stepf, &sbits, 4);
        const double step = (double) stepf, o = comp(lo, a);
        int ql = (int) floor(((double) comp(klo, a) - o) / step), qh = (int) ceil(((double) comp(khi, a) - o) / step);
        ql = minOf(maxOf(ql, 0), 255); qh = minOf(maxOf(qh, 0), 255);
        while (ql > 0 && (float) ((float) o + (float) ql * (float) step) > comp(klo, a)) --ql;          // the float reconstruction must enclose the child box
        while (qh < 255 && (float) ((float) o + (float) qh * (float) step) < comp(khi, a)) ++qh;
        w.qlo[a] |= (uint32_t) ql << (8 * c); w.qhi[a] |= (uint32_t) qh << (8 * c);
    }
}

// ------------------------------------------------------------------------------------------------ the two steps of a vertex edit, one item each
// Tables of a vertex edit.  pos / nrm: the new vertex arrays; shade, triuv, packetExact in original triangle order; tris = the leaf records; leafSlot[t] = position of
// triangle t in `tris`; leafBox[6 * slot] = padded box of the leaf record (lo, hi); nodeBox[6 * node] = exact union of a node's child boxes.
struct GeoEditTables {
    const float *pos, *nrm; TriShade *shade; TriUV *triuv; TriAccelD *tris, *packetExact; const uint32_t *leafSlot; float *leafBox;
    BvhNode *nodes; float *nodeBox; uint32_t nTris, nPacketExact, wide;
};
// Triangle t: Wald record into its leaf slot and into packetExact[t], the geometric words of TriShade, the UV tangents, the padded leaf box.
MI_HD static inline void geoTriRecord(const GeoEditTables &g, uint32_t t) {
    TriShade &ts = g.shade[t];
    const uint32_t a = ts.i0, b = ts.i1, c = ts.i2;
    const V3 p0 = load3(g.pos + (size_t) a * 3), p1 = load3(g.pos + (size_t) b * 3), p2 = load3(g.pos + (size_t) c * 3);
    TriAccelD ta; triaccelLoad(ta, p0, p1, p2); ta.prim = t;
    const uint32_t slot = g.leafSlot[t];
    g.tris[slot] = ta;
    if (t < g.nPacketExact) g.packetExact[t] = ta;
    triShadeGeometry(ts, (ts.flags & 16u) ? &g.triuv[t] : nullptr, p0, p1, p2);
    if (!(ts.flags & 1u)) {      // a smooth triangle carries its three vertex normals instead of the (unused) face frame
        for (int k = 0; k < 3; ++k) { ts.s[k] = g.nrm[(size_t) a * 3 + k]; ts.t[k] = g.nrm[(size_t) b * 3 + k]; ts.n2[k] = g.nrm[(size_t) c * 3 + k]; }
    }
    V3 plo, phi, cen; triPaddedBox(p0, p1, p2, plo, phi, cen);
    store3(g.leafBox + (size_t) slot * 6, plo); store3(g.leafBox + (size_t) slot * 6 + 3, phi);
}
// box of the subtree behind a child code: a leaf's is the union of its <= 8 leaf boxes, an inner node's its nodeBox (written by an earlier level)
MI_HD static inline void geoChildBox(const GeoEditTables &g, int32_t code, V3 &lo, V3 &hi) {
    if (code >= 0) { lo = load3(g.nodeBox + (size_t) code * 6); hi = load3(g.nodeBox + (size_t) code * 6 + 3); return; }
    const uint32_t leaf = (uint32_t) ~code, first = leaf >> 3, count = (leaf & 7u) + 1u;
    lo = load3(g.leafBox + (size_t) first * 6); hi = load3(g.leafBox + (size_t) first * 6 + 3);
    for (uint32_t i = 1; i < count; ++i) { lo = vmin(lo, load3(g.leafBox + (size_t) (first + i) * 6)); hi = vmax(hi, load3(g.leafBox + (size_t) (first + i) * 6 + 3)); }
}
// Node n, all of whose inner children are done: new child boxes from the children's boxes; topology, child codes and unused slots stay.
MI_HD static inline void geoRefitNode(const GeoEditTables &g, uint32_t n) {
    const float inf = INFINITY; V3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
    if (g.wide) {
        Bvh4Node w; memcpy(&w, &g.nodes[n], sizeof(w));
        V3 klo[4], khi[4]; bool used[4]; int nUsed = 0;
        for (int c = 0; c < 4; ++c) {
            used[c] = !wideSlotUnused(w, c);
            if (used[c]) { geoChildBox(g, w.child[c], klo[c], khi[c]); lo = vmin(lo, klo[c]); hi = vmax(hi, khi[c]); ++nUsed; }
        }
        if (!nUsed) { lo = mk(0, 0, 0); hi = mk(0, 0, 0); }
        int ex[3]; wideNodeFrame(w, lo, hi, ex);
        for (int c = 0; c < 4; ++c) { if (used[c]) wideNodeChild(w, c, ex, lo, klo[c], khi[c]); else wideNodeUnused(w, c); }
        memcpy(&g.nodes[n], &w, sizeof(w));
    } else {
        BvhNode b = g.nodes[n];
        if (!(b.lo0[0] > b.hi0[0])) { V3 l, h; geoChildBox(g, b.c0, l, h); store3(b.lo0, l); store3(b.hi0, h); lo = vmin(lo, l); hi = vmax(hi, h); }      // an empty slot (inverted box) stays empty
        if (!(b.lo1[0] > b.hi1[0])) { V3 l, h; geoChildBox(g, b.c1, l, h); store3(b.lo1, l); store3(b.hi1, h); lo = vmin(lo, l); hi = vmax(hi, h); }
        g.nodes[n] = b;
    }
    store3(g.nodeBox + (size_t) n * 6, lo); store3(g.nodeBox + (size_t) n * 6 + 3, hi);
}


// ------------------------------------------------------------------------------------------------ the first step of an instance edit (the second is geoRefitNode)
// xf[24 * i] = rows 0..2 of the new to_world of instance i, then rows 0..2 of its to_object; leafSlot[i] = position of the instance's MI_K_INSTANCE record among the
// leaf records.  Rewrites the two matrices of InstanceD[i] (96 of its 128 bytes) and the padded box of its leaf record.  groupBox (optional; 6 floats per shape group:
// lo, hi): the groups' boxes after a geometry edit moved their vertices -- the record's glo / ghi (words 24..26, 28..30) are rewritten from the box of the record's own
// `group` before the instance box is derived from them.  Without it glo / ghi stay; `root` and `group` always stay.
struct InstEditTables { const float *xf; InstanceD *inst; const uint32_t *leafSlot; float *leafBox; uint32_t n; const float *groupBox; uint32_t nGroups; };
MI_HD static inline void geoInstanceRecord(const InstEditTables &g, uint32_t i) {
    InstanceD &d = g.inst[i]; const float *x = g.xf + (size_t) i * 24;
    for (int k = 0; k < 12; ++k) { d.to_world[k] = x[k]; d.to_object[k] = x[12 + k]; }
    V3 glo = load3(d.glo), ghi = load3(d.ghi);
    if (g.groupBox && d.group < g.nGroups) {
        const float *b = g.groupBox + (size_t) d.group * 6; glo = load3(b); ghi = load3(b + 3);
        store3(d.glo, glo); store3(d.ghi, ghi);
    }
    V3 blo, bhi, plo, phi, cen; instanceBoxes(x, glo, ghi, blo, bhi, plo, phi, cen);
    const uint32_t slot = g.leafSlot[i];
    store3(g.leafBox + (size_t) slot * 6, plo); store3(g.leafBox + (size_t) slot * 6 + 3, phi);
}

}  // namespace mi
