// kernels_field.hip -- field channels: the data of the first camera hit (position, distance, normals, uv, albedo, shape / primitive index) of the very samples the
// radiance film is made of.  Replaces the reference's `multichannel` integrator with nested `field` integrators (src/integrators/misc/multichannel.cpp:164-221,
// src/integrators/misc/field.cpp:124-177): one film position, one sensor ray and one intersection per sample, every nested result put at the same position through
// the same reconstruction filter.
//
// At depth 1 of a batch the queue slot of a path IS its path id (k_generate writes slot = pid), so between the first extend launch and the first shade launch path
// `pid` is fully described by q.hit[pid], q.rayO[0][pid] / q.rayD[0][pid], q.pos[pid] and (scenes with instances) q.hitInst[pid]: no per-path field buffer exists.
#include "kernels_common.h"
#include "surface.h"
#include "fields.h"

// The unfiltered lookup of Texture2D::eval(uv) (src/librender/texture.cpp:112-121): `field` hands the BSDF an intersection without UV partials, which is the lookup
// the shade stage uses at depth > 1 (shade.h).  Returns the record's (possibly textured) `reflectance`.
DEV v3 fieldReflectance(const DScene &sc, const MaterialD &m, float u, float v) {
    const uint32_t tex = (m.type == MI_BSDF_T_BUMPMAP || m.type == MI_BSDF_T_NORMALMAP) ? 0u : (m.flags >> 8) & 0xFFFFu;
    if (!tex) return ld3(m.reflectance);
    const TextureD &tx = sc.textures[tex - 1];
    if (tx.type == 2u) {
        const float uvx = u * tx.uscale + tx.uoffset, uvy = v * tx.vscale + tx.voffset;
        return tx.filter != 0u ? mipBilinear(sc, tx, 0, uvx, uvy) : mipBox(sc, tx, 0, uvx, uvy);
    }
    return textureEval(tx, u, v);
}
// BSDF::eval with wi = wo = (0, 0, 1) under the EDiffuseReflection type mask -- the query of the generic BSDF::getDiffuseReflectance (src/librender/bsdf.cpp:82-86) --
// for a plain record: diffuse.cpp:112-121, phong.cpp:125-150 and ward.cpp:180-227 keep their diffuse lobe (reflectance * INV_PI, cosTheta(wo) = 1); roughdiffuse is a
// glossy lobe (roughdiffuse.cpp:131-135), the conductors, dielectrics, difftrans and null have no diffuse reflection: zero.
DEV v3 fieldDiffuseEvalPlain(const DScene &sc, const MaterialD &m, float u, float v) {
    if (m.type == MI_BSDF_DIFFUSE) return fieldReflectance(sc, m, u, v) * (MI_INV_PI * 1.0f);
    if (m.type == MI_BSDF_T_PHONG || m.type == MI_BSDF_T_WARD) return ((V(0, 0, 0) + ld3(m.reflectance) * MI_INV_PI)) * 1.0f;
    return V(0, 0, 0);
}
// the same query for a record that may be a mixturebsdf / blendbsdf (mixturebsdf.cpp:176-191, blendbsdf.cpp:137-144: the children's values times the weights the
// shade stage uses, mixOf)
DEV v3 fieldDiffuseEval(const DScene &sc, const Tabs<false> &tb, MaterialD m, float u, float v) {
    if (m.type != MI_BSDF_T_MIXTURE && m.type != MI_BSDF_T_BLEND) return fieldDiffuseEvalPlain(sc, m, u, v);
    if (m.type == MI_BSDF_T_BLEND) { const v3 w = fieldReflectance(sc, m, u, v); m.reflectance[0] = w.x; m.reflectance[1] = w.y; m.reflectance[2] = w.z; }
    const MixD x = mixOf(m); v3 r = V(0, 0, 0);
    for (int i = 0; i < 4; ++i) if (i < x.n) r = r + fieldDiffuseEvalPlain(sc, loadMaterial(tb, (int) mixChild(x, i)), u, v) * mixWeight(x, i);
    return r;
}
// its.shape->getBSDF()->getDiffuseReflectance(its) (field.cpp:155).  Overrides: diffuse, roughdiffuse, phong, ward return their diffuse reflectance; twosided, bumpmap and
// normalmap forward to the nested BSDF; everything else takes the generic rule eval * M_PI; mask.cpp:116-120 multiplies the nested value by the opacity.
// (plastic, roughplastic, coating, roughcoating and a mask over a bumpmap / normalmap are refused by mi_render_set_fields.)
DEV v3 fieldAlbedo(const DScene &sc, const Tabs<false> &tb, int material, float u, float v) {
    MaterialD m = loadMaterial(tb, material);
    if (m.type == MI_BSDF_T_MASK) {
        const v3 opacity = fieldReflectance(sc, m, u, v);
        return (fieldDiffuseEval(sc, tb, loadMaterial(tb, (int) m.distr), u, v) * opacity) * MI_PI;
    }
    if (m.type == MI_BSDF_T_BUMPMAP || m.type == MI_BSDF_T_NORMALMAP) m = loadMaterial(tb, (int) m.distr);
    if (m.type == MI_BSDF_DIFFUSE || m.type == MI_BSDF_T_ROUGHDIFFUSE || m.type == MI_BSDF_T_PHONG || m.type == MI_BSDF_T_WARD) return fieldReflectance(sc, m, u, v);
    return fieldDiffuseEval(sc, tb, m, u, v) * MI_PI;
}

// prevPosition (include/mi355pt.h has the normative wording): Bprev - Bcur, the displacement since the last mi_scene_mark_frame of the point with the hit's barycentrics
// on the hit triangle.  Bcur repeats fillHit's expression on the record's corners, Bprev is the same expression on the marked vertices, gathered through the record's
// own i0..i2 (< n_verts: the indices k_tri_records gathers with); a member of a shape group takes both through its instance's to_world, current and marked
// (inst < n_instances).  Null tables -- a scene that was never marked -- stand for the current ones.  What did not move gives the same bits twice, so the difference is 0.
DEV v3 fieldDisplacement(const DScene &sc, const FieldArgs &fa, int inst, uint32_t prim, float u, float v) {
    const TriShade &ts = sc.shade[prim];
    const float bx = 1 - u - v, by = u, bz = v;
    v3 bcur = (ld3(ts.p0) * bx + ld3(ts.p1) * by) + ld3(ts.p2) * bz, bprev = bcur;
    if (fa.prev_pos) bprev = (ld3(fa.prev_pos + (size_t) ts.i0 * 3) * bx + ld3(fa.prev_pos + (size_t) ts.i1 * 3) * by) + ld3(fa.prev_pos + (size_t) ts.i2 * 3) * bz;
    if (inst >= 0) {
        const float *cur = sc.instances[inst].to_world;
        bprev = xfPoint(fa.prev_inst ? fa.prev_inst + (size_t) inst * 12 : cur, bprev); bcur = xfPoint(cur, bcur);
    }
    return bprev - bcur;
}
// motion, the reference's `d` configuration (src/integrators/misc/motion.cpp:258-269) with the marked frame as the target: the film position and the camera distance
// of `pprev` under the marked camera minus those of `p` under the current one.  false: a point at or behind one of the two cameras
DEV bool fieldMotion(const FieldArgs &fa, v3 p, v3 pprev, v3 &motion) {
    const float *a = fa.m_prev, *b = fa.m_cur;
    const float wp = ((a[8] * pprev.x + a[9] * pprev.y) + a[10] * pprev.z) + a[11], wc = ((b[8] * p.x + b[9] * p.y) + b[10] * p.z) + b[11];
    if (!(wp > 0) || !(wc > 0)) return false;
    const float xp = (((a[0] * pprev.x + a[1] * pprev.y) + a[2] * pprev.z) + a[3]) / wp, yp = (((a[4] * pprev.x + a[5] * pprev.y) + a[6] * pprev.z) + a[7]) / wp;
    const float xc = (((b[0] * p.x + b[1] * p.y) + b[2] * p.z) + b[3]) / wc, yc = (((b[4] * p.x + b[5] * p.y) + b[6] * p.z) + b[7]) / wc;
    const v3 ep = pprev - ld3(fa.o_prev), ec = p - ld3(fa.o_cur);
    const float dp = sqrtf((ep.x * ep.x + ep.y * ep.y) + ep.z * ep.z), dc = sqrtf((ec.x * ec.x + ec.y * ec.y) + ec.z * ec.z);
    motion = V(xp - xc, yp - yc, dp - dc);
    return true;
}

// All fields of path `pid`: out[3 f + c].  The interaction is rebuilt as k_ray_intersect does (kernels_trace.hip), from the hit record the extend stage left.
DEV void fieldEval(const DScene &sc, const FieldArgs &fa, const Queues &q, uint64_t pid, float *out) {
    const float4 hr = q.hit[pid]; const uint32_t prim = __float_as_uint(hr.w);
    if (prim == 0xFFFFFFFFu) {
#pragma unroll
        for (int f = 0; f < MI_MAX_FIELDS; ++f) if ((uint32_t) f < fa.n) { out[3 * f] = fa.undefined[f][0]; out[3 * f + 1] = fa.undefined[f][1]; out[3 * f + 2] = fa.undefined[f][2]; }
        return;
    }
    const auto ro = qRayOrigin(q, 0, (uint32_t) pid), rd = qRayDirection(q, 0, (uint32_t) pid);
    const v3 o = V(ro.x, ro.y, ro.z), d = V(rd.x, rd.y, rd.z); const float t = hr.x, u = hr.y, v = hr.z;
    const int inst = (sc.n_instances && q.hitInst) ? q.hitInst[pid] : -1;
    const Tabs<false> tb = globalTabs(sc);
    Hit h; const bool analytic = inst < 0 && prim >= sc.n_tris;
    fillHitAny<false, true>(sc, tb, inst, o, d, t, u, v, prim, h);      // (past the instance test, prim >= sc.n_tris is `analytic`)
    if (analytic) { v3 du, dv; analyticUV(sc.analytic[prim - sc.n_tris], u, v, o + d * t, h.uvx, h.uvy, du, dv); }
    v3 rel = V(0, 0, 0), albedo = V(0, 0, 0); float shapeIndex = -1.0f, primIndex = 0.0f;
    if (fa.needs & (1u << MI_FIELD_REL_POSITION)) rel = xfPoint(fa.w2c, h.p);
    if (fa.needs & (1u << MI_FIELD_ALBEDO)) albedo = fieldAlbedo(sc, tb, h.material, h.uvx, h.uvy);
    if (fa.needs & (1u << MI_FIELD_SHAPE_INDEX)) shapeIndex = inst >= 0 ? -1.0f : (analytic ? (float) (fa.n_meshes + (prim - sc.n_tris)) : (float) fa.tri_shape[prim]);
    if ((fa.needs & (1u << MI_FIELD_PRIM_INDEX)) && !analytic) primIndex = (float) sc.shade[prim].local_prim;
    v3 pprev = h.p, motion = V(0, 0, 0); bool motionDefined = true;
    if (fa.needs & ((1u << MI_FIELD_PREV_POSITION) | (1u << MI_FIELD_MOTION))) {
        if (!analytic) pprev = h.p + fieldDisplacement(sc, fa, inst, prim, u, v);      // an analytic shape cannot move in place
        if (fa.needs & (1u << MI_FIELD_MOTION)) motionDefined = fieldMotion(fa, h.p, pprev, motion);
    }
#pragma unroll
    for (int f = 0; f < MI_MAX_FIELDS; ++f) if ((uint32_t) f < fa.n) {
        v3 val;
        switch (fa.kind[f]) {
            case MI_FIELD_POSITION: val = h.p; break;
            case MI_FIELD_REL_POSITION: val = rel; break;
            case MI_FIELD_DISTANCE: val = V(t, t, t); break;
            case MI_FIELD_GEO_NORMAL: val = h.ng; break;
            case MI_FIELD_SH_NORMAL: val = h.ns; break;
            case MI_FIELD_UV: val = V(h.uvx, h.uvy, 0.0f); break;
            case MI_FIELD_ALBEDO: val = albedo; break;
            case MI_FIELD_SHAPE_INDEX: val = V(shapeIndex, shapeIndex, shapeIndex); break;
            case MI_FIELD_PREV_POSITION: val = pprev; break;
            case MI_FIELD_MOTION: val = motionDefined ? motion : V(fa.undefined[f][0], fa.undefined[f][1], fa.undefined[f][2]); break;
            default: val = V(primIndex, primIndex, primIndex); break;
        }
        out[3 * f] = val.x; out[3 * f + 1] = val.y; out[3 * f + 2] = val.z;
    }
}

// ---------------------------------------------------------------------------------------------- field film
// ImageBlock::put of every sample of the batch into the field film: 3 F + 1 SoA planes (the fields' values, then a weight plane of its own), the same footprint,
// border and filterEvalDiscretized weights as k_film (kernels_misc.hip) -- but WITHOUT its `< 0` / isfinite rejection: multichannel switches the check off
// (multichannel.cpp:41-44), normals and positions are signed.  One thread per tile pixel walks its planes in sample order; the own pixel is a plain
// read-modify-write, spills go to the separate spill planes with float atomics.  Launched between the first extend and the first shade of a batch; the host chains
// consecutive batches' launches (fieldDone events, api.cpp), so the own-pixel sums are deterministic.
#define MI_FIELD_PLANES (3 * MI_MAX_FIELDS + 1)
__global__ __launch_bounds__(WG) void k_field_film(DScene sc, FieldArgs fa, Queues q, BatchDesc bd, float *film, float *spill) {
    const uint32_t pl = blockIdx.x * WG + threadIdx.x;
    if (pl >= bd.n_pix) return;
    const uint32_t tw = bd.tile.x1 - bd.tile.x0;
    const int px = (int) (bd.tile.x0 + pl % tw), py = (int) (bd.tile.y0 + (pl / tw) * bd.row_stride);
    const int W = (int) sc.width + 2 * sc.border, H = (int) sc.height + 2 * sc.border;
    const size_t plane = (size_t) W * H;
    const int ownX = px + sc.border, ownY = py + sc.border;
    const size_t ownIdx = (size_t) ownY * W + ownX;
    const int nv = 3 * (int) fa.n;       // value planes; plane nv = weight
    float own[MI_FIELD_PLANES];
#pragma unroll
    for (int k = 0; k < MI_FIELD_PLANES; ++k) own[k] = k <= nv ? film[k * plane + ownIdx] : 0.0f;
    const float r = sc.filter_radius;
    for (uint32_t s = 0; s < bd.n_planes; ++s) {
        const uint64_t pid = (uint64_t) s * bd.n_pix + pl;
        float vals[MI_FIELD_PLANES];
        fieldEval(sc, fa, q, pid, vals);
        const float2 sp = q.pos[pid];
        float posx = sp.x - 0.5f - (float) (0 - sc.border), posy = sp.y - 0.5f - (float) (0 - sc.border);
        int minx = (int) ceilf(posx - r), miny = (int) ceilf(posy - r), maxx = (int) floorf(posx + r), maxy = (int) floorf(posy + r);
        minx = max(minx, 0); miny = max(miny, 0); maxx = min(maxx, W - 1); maxy = min(maxy, H - 1);
        for (int y = miny; y <= maxy; ++y) {
            float wy = filterEvalDiscretized(sc, (float) y - posy);
            for (int x = minx; x <= maxx; ++x) {
                float w = filterEvalDiscretized(sc, (float) x - posx) * wy;
                if (x == ownX && y == ownY) {
#pragma unroll
                    for (int k = 0; k < MI_FIELD_PLANES - 1; ++k) if (k < nv) own[k] += w * vals[k];
#pragma unroll
                    for (int k = 0; k < MI_FIELD_PLANES; ++k) if (k == nv) own[k] += w * 1.0f;
                } else {
                    float *dst = spill + (size_t) y * W + x;
#pragma unroll
                    for (int k = 0; k < MI_FIELD_PLANES - 1; ++k) if (k < nv) atomicAdd(dst + k * plane, w * vals[k]);
                    atomicAdd(dst + (size_t) nv * plane, w * 1.0f);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < MI_FIELD_PLANES; ++k) if (k <= nv) film[k * plane + ownIdx] = own[k];
}

// explicit-list mode (mi_render_field_samples): 3 F floats per listed sample, path i = sample i
__global__ __launch_bounds__(WG) void k_field_samples(DScene sc, FieldArgs fa, Queues q, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    float vals[MI_FIELD_PLANES];
    fieldEval(sc, fa, q, i, vals);
    float *dst = out + i * (3 * fa.n);
#pragma unroll
    for (int k = 0; k < MI_FIELD_PLANES - 1; ++k) if (k < 3 * (int) fa.n) dst[k] = vals[k];
}

// dst[i] += src[i] over the field planes is k_film_add's job (kernels_misc.hip); read-back: SoA planes -> interleaved.  layout 0: raw sums incl. border, nch = 3 F + 1
// channels (weight last); layout 2: developed, 3 F channels = sum x (weight != 0 ? 1 / weight : 0) as k_film_layout and the reference's multichannel develop
// (src/libcore/bitmap.cpp:1621-1625) compute it, crop window only
__global__ void k_field_layout(const float *film, const float *spill, float *out, int W, int H, int border, int nch, int layout) {
    const size_t plane = (size_t) W * H;
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (layout == 0) { if (i < plane) for (int k = 0; k < nch; ++k) out[i * nch + k] = film[k * plane + i] + spill[k * plane + i]; }
    else {
        const int w = W - 2 * border, h = H - 2 * border, nv = nch - 1;
        if (i < (size_t) w * h) {
            const int x = (int) (i % w), y = (int) (i / w); const size_t src = (size_t) (y + border) * W + (x + border);
            const float wgt = film[nv * plane + src] + spill[nv * plane + src], inv = wgt != 0 ? 1.0f / wgt : 0.0f;
            for (int k = 0; k < nv; ++k) out[i * nv + k] = (film[k * plane + src] + spill[k * plane + src]) * inv;
        }
    }
}

extern "C" {
void mi_launch_field_film(const DScene &sc, const FieldArgs &fa, const Queues &q, const BatchDesc &bd, float *film, float *spill, hipStream_t st) {
    hipLaunchKernelGGL(k_field_film, dim3((bd.n_pix + WG - 1) / WG), dim3(WG), 0, st, sc, fa, q, bd, film, spill);
}
void mi_launch_field_samples(const DScene &sc, const FieldArgs &fa, const Queues &q, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_field_samples, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, fa, q, n, out);
}
void mi_launch_field_layout(const float *film, const float *spill, float *out, int W, int H, int border, int nch, int layout, hipStream_t st) {
    size_t n = (size_t) W * H; hipLaunchKernelGGL(k_field_layout, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, film, spill, out, W, H, border, nch, layout);
}
}
