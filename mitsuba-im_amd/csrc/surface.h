// surface.h -- the surface step: what runs between a hit record and the BSDF query, once, for every stage that shades a surface (shade.h, direct.h, kernels_vol.hip,
// kernels_volmis.hip) and for the unit kernel that holds it to the oracle one hit at a time (kernels_units.hip k_debug_surface):
//     fill the Hit -> load the material -> textured parameters (the filtered MIP lookup on the camera hit) -> mask -> bumpmap / normalmap (perturbFrame) -> coating,
//     then wi / wo into the perturbed frame and the mask's lobe choice around the nested sample.
// Every gate is a template parameter and every routine is inlined, so a stage compiles to what it compiled to with the sequence pasted into it.
#pragma once
#include "pt_device.h"

// the scene tables in global memory
DEV Tabs<false> globalTabs(const DScene &sc) {
    Tabs<false> tb; tb.shade4 = (AS<false>::p4) sc.shade; tb.materials4 = (AS<false>::p4) sc.materials; tb.emitters4 = (AS<false>::p4) sc.emitters; tb.emitter_cdf = sc.emitter_cdf; tb.area_cdf = sc.area_cdf;
    return tb;
}
// Scene tables of a shading stage: shading records, materials, emitters, CDFs.  Small scenes (<= 128 triangles ...) are staged in LDS at `base` by the N threads of the
// workgroup: the stage chases hit -> triangle record -> material -> emitter CDF -> light triangle, and each hop is an L2 round trip otherwise.  The caller's barrier follows.
template <bool L, uint32_t N>
DEV void stageTables(const DScene &sc, uint32_t *base, uint32_t tid, Tabs<L> &tb) {
    if (L) {
        const uint32_t wShade = sc.n_tris * (4u * MI_SHADE_WORDS), wMat = sc.n_materials * 16u, wEm = sc.n_emitters * 12u, wEc = (sc.n_emitters + 1u + 3u) & ~3u, wAc = sc.area_cdf_len;
        uint32_t *pS = base, *pM = pS + wShade, *pE = pM + wMat, *pEc = pE + wEm, *pAc = pEc + wEc;
        const uint32_t *gS = (const uint32_t *) sc.shade, *gM = (const uint32_t *) sc.materials, *gE = (const uint32_t *) sc.emitters, *gEc = (const uint32_t *) sc.emitter_cdf, *gAc = (const uint32_t *) sc.area_cdf;
        for (uint32_t i = tid; i < wShade; i += N) pS[i] = gS[i];
        for (uint32_t i = tid; i < wMat; i += N) pM[i] = gM[i];
        for (uint32_t i = tid; i < wEm; i += N) pE[i] = gE[i];
        for (uint32_t i = tid; i < sc.n_emitters + 1u; i += N) pEc[i] = gEc[i];
        for (uint32_t i = tid; i < wAc; i += N) pAc[i] = gAc[i];
        tb.shade4 = (typename AS<L>::p4) pS; tb.materials4 = (typename AS<L>::p4) pM; tb.emitters4 = (typename AS<L>::p4) pE;
        tb.emitter_cdf = (typename AS<L>::pf) pEc; tb.area_cdf = (typename AS<L>::pf) pAc;
    } else {
        tb.shade4 = (typename AS<L>::p4) sc.shade; tb.materials4 = (typename AS<L>::p4) sc.materials; tb.emitters4 = (typename AS<L>::p4) sc.emitters;
        tb.emitter_cdf = (typename AS<L>::pf) sc.emitter_cdf; tb.area_cdf = (typename AS<L>::pf) sc.area_cdf;
    }
}

// The hit record of (t, u, v, prim) on the ray (o, d): the member of an instance, an analytic shape, or a triangle.  AN = false: triangles only (`inst` and `o` are unused).
// sc.analytic is read for prim >= sc.n_tris only.
template <bool L, bool AN>
DEV void fillHitAny(const DScene &sc, const Tabs<L> &tb, int inst, v3 o, v3 d, float t, float u, float v, uint32_t prim, Hit &h) {
    if (AN && inst >= 0) fillHitInstanced(sc, tb, sc.instances[inst], o, d, t, prim, u, v, h);
    else if (AN && prim >= sc.n_tris) fillHitAnalytic(sc.analytic[prim - sc.n_tris], o, d, t, u, v, h);
    else fillHit<L, AN>(sc, tb, d, t, prim, u, v, h);
}

// A textured parameter: m_reflectance->eval(bRec.its) (diffuse.cpp:112-121) and its siblings, into mm.reflectance; true when the record has one.  hr = (t, u, v, prim) of the
// hit on the ray (o, d).  ADAPT: a bumpmap / normalmap record's texture is its displacement / normal map, not a parameter.  `filtered`: the camera hit -- its.getBSDF(ray) ->
// computePartials: only the camera ray carries differentials (records.inl:68-75); diffs(rxd, ryd) yields them and is called only there.
template <bool L, bool AN, bool ADAPT, typename D>
DEV bool loadTexturedParameter(const DScene &sc, const Tabs<L> &tb, const Hit &h, uint32_t prim, int inst, float4 hr, v3 o, v3 d, bool filtered, D diffs, MaterialD &mm) {
    const uint32_t tex = (ADAPT && (mm.type == MI_BSDF_T_BUMPMAP || mm.type == MI_BSDF_T_NORMALMAP)) ? 0u : (mm.flags >> 8) & 0xFFFFu;
    if (!tex) return false;
    const TextureD &tx = sc.textures[tex - 1]; v3 c;
    float huvx = h.uvx, huvy = h.uvy;
    const bool onAnalytic = AN && inst < 0 && prim >= sc.n_tris;         // an analytic shape: its own parameterisation, evaluated on demand
    if (onAnalytic) { v3 du, dv; analyticUV(sc.analytic[prim - sc.n_tris], hr.y, hr.z, o + d * hr.x, huvx, huvy, du, dv); }   // (tangents: recomputed below where a filtered lookup needs them)
    if (tx.type == 2u) {                                                 // BitmapTexture::eval (src/textures/bitmap.cpp:434-502) under Texture2D::eval (texture.cpp:112-121)
        const float uvx = huvx * tx.uscale + tx.uoffset, uvy = huvy * tx.vscale + tx.voffset;
        if (filtered) {
            v3 dpdu, dpdv; float tu_, tv_;
            surfaceTangents<L>(sc, tb, h, prim, inst, hr.y, hr.z, o + d * hr.x, tu_, tv_, dpdu, dpdv);
            v3 rxd, ryd; diffs(rxd, ryd);
            float pa[4]; computePartials(h.p, h.ng, dpdu, dpdv, o, rxd, ryd, pa);
            c = mipEval(sc, tx, uvx, uvy, pa[0] * tx.uscale, pa[1] * tx.vscale, pa[2] * tx.uscale, pa[3] * tx.vscale);
        } else c = tx.filter != 0u ? mipBilinear(sc, tx, 0, uvx, uvy) : mipBox(sc, tx, 0, uvx, uvy);
    } else c = textureEval(tx, huvx, huvy);
    mm.reflectance[0] = c.x; mm.reflectance[1] = c.y; mm.reflectance[2] = c.z;
    return true;
}

// What the BSDF query needs of a resolved surface: the leaf record, the opacity of a mask in front of it, the frame of a bumpmap / normalmap around it, the coating
// record around it (-1: none).  The defaults are those of a plain record.
struct SurfaceBsdf { MaterialD bsdf; v3 opac = {1, 1, 1}; v3 ps = {0, 0, 0}, pt = {0, 0, 0}, pn = {0, 0, 0}; int coat = -1, leaf = -1; bool masked = false, bumped = false; };

// Load h.material and unwrap it: texture -> mask -> bumpmap / normalmap -> coating, each nested record followed by its textured load.  The gates are the caller's:
// TEX: textures bound to materials; MASK (mask.cpp: the record's (textured) `reflectance` is the opacity in front of the nested record `distr`); BUMP (bumpmap.cpp /
// normalmap.cpp: getFrame(its), then the nested record); COAT (coating.cpp: the layer around the nested record).  `loaded(colour)` sees every textured load that happened.
template <bool L, bool AN, bool TEX, bool MASK, bool BUMP, bool COAT, bool ADAPT, typename D, typename F>
DEV SurfaceBsdf resolveSurface(const DScene &sc, const Tabs<L> &tb, const Hit &h, uint32_t prim, int inst, float4 hr, v3 o, v3 d, bool filtered, D diffs, F loaded) {
    SurfaceBsdf s; int cur = h.material;
    auto next = [&](int id) {
        cur = id; s.bsdf = loadMaterial(tb, id);
        if (TEX) { if (loadTexturedParameter<L, AN, ADAPT>(sc, tb, h, prim, inst, hr, o, d, filtered, diffs, s.bsdf)) loaded(ld3(s.bsdf.reflectance)); }
    };
    next(cur);
    if (MASK && s.bsdf.type == MI_BSDF_T_MASK) { s.opac = ld3(s.bsdf.reflectance); s.masked = true; next((int) s.bsdf.distr); }
    if (BUMP && (s.bsdf.type == MI_BSDF_T_BUMPMAP || s.bsdf.type == MI_BSDF_T_NORMALMAP)) {
        float huvx = h.uvx, huvy = h.uvy; v3 dpdu, dpdv;
        surfaceTangents<L>(sc, tb, h, prim, inst, hr.y, hr.z, o + d * hr.x, huvx, huvy, dpdu, dpdv);
        perturbFrame(sc, s.bsdf, h, huvx, huvy, dpdu, dpdv, s.ps, s.pt, s.pn); s.bumped = true;
        next((int) s.bsdf.distr);
    }
    if (COAT && (s.bsdf.type == MI_BSDF_T_COATING || s.bsdf.type == MI_BSDF_T_ROUGHCOATING)) { s.coat = cur; next((int) s.bsdf.distr); }
    s.leaf = cur;
    return s;
}
template <bool L, bool AN, bool TEX, bool MASK, bool BUMP, bool COAT, bool ADAPT, typename D>
DEV SurfaceBsdf resolveSurface(const DScene &sc, const Tabs<L> &tb, const Hit &h, uint32_t prim, int inst, float4 hr, v3 o, v3 d, bool filtered, D diffs) {
    return resolveSurface<L, AN, TEX, MASK, BUMP, COAT, ADAPT>(sc, tb, h, prim, inst, hr, o, d, filtered, diffs, [](v3) {});
}

// ---- the query frame: under a bumpmap / normalmap the BSDF is queried in the perturbed frame (bumpmap.cpp:165-180); BUMP = false: h's own frame
template <bool BUMP>
DEV v3 queryWi(const Hit &h, const SurfaceBsdf &s) { return (BUMP && s.bumped) ? frameToLocal(s.ps, s.pt, s.pn, toWorld(h, h.wi)) : h.wi; }
// wi and the local direction wo in the query frame; rejected: wo changed sides on the way
template <bool BUMP>
DEV void queryFrame(const Hit &h, const SurfaceBsdf &s, v3 wo, v3 &wiQ, v3 &woQ, bool &rejected) {
    wiQ = h.wi; woQ = wo; rejected = false;
    if (BUMP && s.bumped) { wiQ = frameToLocal(s.ps, s.pt, s.pn, toWorld(h, h.wi)); woQ = frameToLocal(s.ps, s.pt, s.pn, toWorld(h, wo)); rejected = wo.z * woQ.z <= 0; }
}
// sample(wi, wo) -- the caller's ctSample / mxSample -- in the query frame, the direction brought back into h's frame (bumpmap.cpp:199-222); returns the weight
// (`sample` is called from two places, as the stages always had it: a lambda passed here is marked always_inline, or the compiler keeps one copy and calls it)
template <bool BUMP, typename F>
DEV v3 sampleInQueryFrame(const Hit &h, const SurfaceBsdf &s, F sample, v3 &woL) {
    if (BUMP && s.bumped) {
        const v3 wiQ = frameToLocal(s.ps, s.pt, s.pn, toWorld(h, h.wi)); v3 woQ = V(0, 0, 0);
        v3 bw = sample(wiQ, woQ);
        if (!isZero(bw)) { woL = toLocal(h, frameToWorld(s.ps, s.pt, s.pn, woQ)); if (woL.z * woQ.z <= 0) bw = V(0, 0, 0); }
        return bw;
    }
    return sample(h.wi, woL);
}

// ---- mask.cpp:196-208, sampling: the nested BSDF with probability luminance(opacity), else straight through.  How the nested sample is weighted afterwards differs
// between the reference's overloads (with / without a pdf) and stays with each caller.
// true: straight through; false: the nested BSDF, with sx stretched back to [0, 1)
DEV bool maskChooseLobe(v3 opac, float &sx) { const float prob = luminance3(opac); if (sx < prob) { sx /= prob; return false; } return true; }
// the straight-through sample: a delta, null component along -wi; returns its weight
DEV v3 maskPassThrough(const Hit &h, v3 opac, v3 &woL, float &pdf, bool &delta, bool &nullComp) {
    const float p = 1 - luminance3(opac);
    woL = V(-h.wi.x, -h.wi.y, -h.wi.z); pdf = p; delta = true; nullComp = true;
    return V((1.0f - opac.x) / p, (1.0f - opac.y) / p, (1.0f - opac.z) / p);
}
