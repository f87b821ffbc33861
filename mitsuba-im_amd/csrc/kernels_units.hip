// kernels_units.hip -- unit-level parity entry points over the BSDF, texture and emitter routines of pt_device.h (mi_debug_bsdf, mi_debug_texture, mi_debug_emitter_sample,
// mi_debug_emitter_eval) and the medium routines of the volumetric stages (mi_debug_medium): one call of the
// routine per thread on caller-supplied inputs, so that directions, sample values and footprints a camera-driven path almost never produces can be compared with the
// oracle's orc_bsdf_sample_ex / orc_bsdf_eval / orc_texture_eval; and the surface step between a hit and the BSDF query on caller-supplied hits (mi_debug_surface against
// orc_surface_units).  Nothing here restates a routine: the kernels call what the shade stage calls.
#include "kernels_common.h"
#include "surface.h"

// in9 = wi xyz, wo xyz, u, v, extra.  The record is resolved as the shade stage resolves an untextured hit (shade.h: a coating / roughcoating record becomes `coat`,
// its nested record `bsdf`; mask, bumpmap, normalmap and textured records are refused on the host), then queried through ctSample / ctEval / ctPdf<true, true, false>:
// every BSDF type, every wrapper, tables in global memory -- the widest instantiation the shade stage has.
// mode 0 (sample): out12 = weight rgb, pdf, wo xyz, eta, delta, null, extra drawn, 0;  mode 1 (eval + pdf): out12 = value rgb, pdf, 0...
__global__ __launch_bounds__(WG) void k_debug_bsdf(DScene sc, int material, int mode, const float *in, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const Tabs<false> tb = globalTabs(sc);
    const float *p = in + i * 9; float *o = out + i * 12;
    const v3 wi = V(p[0], p[1], p[2]), woIn = V(p[3], p[4], p[5]);
    int coat = -1; MaterialD bsdf = loadMaterial(tb, material);
    if (bsdf.type == MI_BSDF_T_COATING || bsdf.type == MI_BSDF_T_ROUGHCOATING) { coat = material; bsdf = loadMaterial(tb, (int) bsdf.distr); }
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = 0.0f;
    if (mode == 0) {
        const float extraValue = p[8]; bool drawn = false;
        auto drawExtra = [&]() { drawn = true; return extraValue; };
        v3 wo = V(0, 0, 0); float pdf = 0.0f, eta = 0.0f; bool delta = false, nullComp = false;
        const v3 w = ctSample<true, true>(sc, tb, coat, bsdf, wi, p[6], p[7], drawExtra, wo, pdf, eta, delta, nullComp);
        o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = pdf; o[4] = wo.x; o[5] = wo.y; o[6] = wo.z; o[7] = eta;
        o[8] = delta ? 1.0f : 0.0f; o[9] = nullComp ? 1.0f : 0.0f; o[10] = drawn ? 1.0f : 0.0f;
    } else {
        const v3 e = ctEval<true, true>(sc, tb, coat, bsdf, wi, woIn);
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = ctPdf<true, true>(sc, tb, coat, bsdf, wi, woIn);
    }
}

// One texture lookup per thread.  Bitmaps: scale and offset as the shade stage applies them; with partials (dudx, dvdx, dudy, dvdy) the filtered lookup of a camera
// hit (mipEval), without them the level-0 lookup of every later bounce.  Procedural textures: textureEval.
__global__ __launch_bounds__(WG) void k_debug_texture(DScene sc, uint32_t texture, const float *uv, const float *partials, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const TextureD &tx = sc.textures[texture]; const float u = uv[2 * i], v = uv[2 * i + 1]; v3 c;
    if (tx.type == 2u) {
        const float uvx = u * tx.uscale + tx.uoffset, uvy = v * tx.vscale + tx.voffset;
        if (partials) { const float *pa = partials + 4 * i; c = mipEval(sc, tx, uvx, uvy, pa[0] * tx.uscale, pa[1] * tx.vscale, pa[2] * tx.uscale, pa[3] * tx.vscale); }
        else c = tx.filter != 0u ? mipBilinear(sc, tx, 0, uvx, uvy) : mipBox(sc, tx, 0, uvx, uvy);
    } else c = textureEval(tx, u, v);
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
}

// One call of sampleEmitterDirect<true, true, false, RAW> per thread: every emitter kind, analytic shapes, tables in global memory -- the widest instantiation the stages
// have.  in8 = ref xyz, refN xyz, u, v.  out17 = value rgb, p xyz, d xyz, dist, pdf, n xyz, emitter index, delta flag, em_pdf (RAW only).  The record starts out zero;
// no visibility test (the shadow queue makes it).
template <bool RAW>
__global__ __launch_bounds__(WG) void k_debug_emitter_sample(DScene sc, const float *in, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const Tabs<false> tb = globalTabs(sc);
    const float *p = in + i * 8; float *o = out + i * 17;
    Direct dr; dr.p = V(0, 0, 0); dr.n = V(0, 0, 0); dr.d = V(0, 0, 0); dr.dist = 0.0f; dr.pdf = 0.0f; dr.em_pdf = 0.0f; dr.emitter = 0; dr.delta = false;
    const v3 value = sampleEmitterDirect<true, true, false, RAW>(sc, tb, V(p[0], p[1], p[2]), V(p[3], p[4], p[5]), p[6], p[7], dr);
    o[0] = value.x; o[1] = value.y; o[2] = value.z; o[3] = dr.p.x; o[4] = dr.p.y; o[5] = dr.p.z; o[6] = dr.d.x; o[7] = dr.d.y; o[8] = dr.d.z; o[9] = dr.dist; o[10] = dr.pdf;
    o[11] = dr.n.x; o[12] = dr.n.y; o[13] = dr.n.z; o[14] = (float) dr.emitter; o[15] = dr.delta ? 1.0f : 0.0f; o[16] = RAW ? dr.em_pdf : 0.0f;
}

// What a BSDF-sampled ray that finds emitter `emitter` evaluates.  in11 = ref xyz, d xyz, n xyz, dist, facingRef (0 / 1).  out8:
// kind 0 (area light): emitterEval(tb, e, n, -d) rgb, pdfEmitterDirect<true>(..., facingRef), 0...
// kind 1 (envmap): envEval(d) rgb, envPdfDirection(to_local d), then value rgb and density of envEvalAndPdf(d)
// kind 2 (constant): envEval rgb, 0... (its density is one line inside the shade stage)
__global__ __launch_bounds__(WG) void k_debug_emitter_eval(DScene sc, int emitter, int kind, const float *in, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const Tabs<false> tb = globalTabs(sc);
    const float *p = in + i * 11; float *o = out + i * 8;
    const v3 ref = V(p[0], p[1], p[2]), d = V(p[3], p[4], p[5]), nrm = V(p[6], p[7], p[8]);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = 0.0f;
    if (kind == 0) {
        const v3 e = emitterEval(tb, emitter, nrm, -d);
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = pdfEmitterDirect<true>(sc, tb, emitter, ref, d, nrm, p[9], p[10] != 0.0f);
    } else {
        const v3 e = envEval(sc, d); o[0] = e.x; o[1] = e.y; o[2] = e.z;
        if (kind == 1) {
            o[3] = envPdfDirection(sc, mat3(sc.env_to_local, d));
            v3 value; float pdfSA; envEvalAndPdf(sc, d, value, pdfSA);
            o[4] = value.x; o[5] = value.y; o[6] = value.z; o[7] = pdfSA;
        }
    }
}

// The medium routines of the volumetric stages, one call per thread.  in10 / out12 per case:
// mode 0 mediumTransmittance over [mint, maxt]: in[6], in[7] -> transmittance rgb
// mode 1 mediumSampleDistance: o xyz, d xyz, mint, maxt, the two values its draw source hands out -> success, t, p xyz, transmittance rgb, pdfSuccess, pdfFailure, values drawn
// mode 2 phaseSample, then phaseEval of its own result: wi xyz, the 2-D sample -> wo xyz, eval;  mode 3 phaseEval: wi xyz, wo xyz -> eval
__global__ __launch_bounds__(WG) void k_debug_medium(DScene sc, uint32_t medium, int mode, const float *in, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const MediumD md = sc.media[medium]; const float *p = in + i * 10; float *o = out + i * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = 0.0f;
    if (mode == 0) { const v3 t = mediumTransmittance(md, p[6], p[7]); o[0] = t.x; o[1] = t.y; o[2] = t.z; }
    else if (mode == 1) {
        int drawn = 0; const float r0 = p[8], r1 = p[9];
        MediumRec r; r.t = 0.0f; r.p = V(0, 0, 0); r.transmittance = V(0, 0, 0); r.pdfSuccess = 0.0f; r.pdfFailure = 0.0f;
        const bool ok = mediumSampleDistance(md, V(p[0], p[1], p[2]), V(p[3], p[4], p[5]), p[6], p[7], [&]() { return drawn++ == 0 ? r0 : r1; }, r);
        o[0] = ok ? 1.0f : 0.0f; o[1] = r.t; o[2] = r.p.x; o[3] = r.p.y; o[4] = r.p.z; o[5] = r.transmittance.x; o[6] = r.transmittance.y; o[7] = r.transmittance.z;
        o[8] = r.pdfSuccess; o[9] = r.pdfFailure; o[10] = (float) drawn;
    } else if (mode == 2) {
        const v3 wi = V(p[0], p[1], p[2]), wo = phaseSample(md, wi, p[3], p[4]);
        o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = phaseEval(md, wi, wo);
    } else o[0] = phaseEval(md, V(p[0], p[1], p[2]), V(p[3], p[4], p[5]));
}

// The surface step between a hit and the BSDF query, for one caller-supplied hit per thread: rays8 = o, mint, d, maxt; hits4 = t, u, v, prim as mi_debug_intersect_inst
// returns them (prim < 0: a miss, which writes zeros), insts = its instance indices (NULL: none); diffs6 = the two differential directions rxd, ryd of a camera ray
// (NULL: a later bounce -- level-0 lookups, no partials); query3 = mode 1: the 2-D sample and the extra sampler value, mode 2: a WORLD direction.  The widest
// instantiation the stages have: fillHit<false, true>, tables in global memory, ctSample / ctEval / ctPdf<true, true>.  The kernel calls routines and nothing else: the
// unwrap sequence (texture -> mask -> bump / normal map -> coating, each followed by the textured load) is resolveSurface, and the query frame queryWi / queryFrame, of
// surface.h -- the routines the shade, direct and volumetric stages run, with every gate on.
// mode 0 (record): out51 = uv as the lookups use it 2, dpdu 3, dpdv 3, partials 4 (zero without differentials), opacity 3 (zero without a mask), the value loaded into the
//   first textured parameter on the chain 3, masked, bumped, coating record (-1: none), leaf record, the leaf's reflectance after applyTexture 3, ps 3, pt 3, pn 3 (zero when
//   not bumped), wi in the frame the query uses 3, the hit as given: t, u, v, prim, instance, and its shading frame ns 3, s 3, t 3
// mode 1 (sample): out11 as k_debug_bsdf's mode 0, on the resolved (coat, leaf) with that wi; wo in query-frame coordinates; taken before the mask's lobe choice, the
//   opacity multiply and the sign rejection.  mode 2 (eval + pdf): the direction goes into the query frame by toLocal (and toWorld / frameToLocal when bumped); out4
__global__ __launch_bounds__(WG) void k_debug_surface(DScene sc, int mode, const float *rays, const float *hits, const int *insts, const float *diffs, const float *query, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const Tabs<false> tb = globalTabs(sc);
    const int per = mode == 0 ? 51 : mode == 1 ? 11 : 4; float *o = out + i * per;
    for (int k = 0; k < per; ++k) o[k] = 0.0f;
    const float *r = rays + i * 8; const v3 ro3 = V(r[0], r[1], r[2]), d = V(r[4], r[5], r[6]);
    const float4 hr = make_float4(hits[4 * i], hits[4 * i + 1], hits[4 * i + 2], hits[4 * i + 3]);
    if (!(hr.w >= 0)) return;
    const uint32_t prim = (uint32_t) hr.w; const int inst = insts ? insts[i] : -1;
    Hit h; fillHitAny<false, true>(sc, tb, inst, ro3, d, hr.x, hr.y, hr.z, prim, h);
    if (h.material < 0 || (uint32_t) h.material >= sc.n_materials) return;
    // the record's own uv, tangents and partials
    float ruvx = h.uvx, ruvy = h.uvy; v3 rdpdu, rdpdv; surfaceTangents<false>(sc, tb, h, prim, inst, hr.y, hr.z, ro3 + d * hr.x, ruvx, ruvy, rdpdu, rdpdv);
    v3 rxd = V(0, 0, 0), ryd = V(0, 0, 0); float rpa[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (diffs) { rxd = V(diffs[6 * i], diffs[6 * i + 1], diffs[6 * i + 2]); ryd = V(diffs[6 * i + 3], diffs[6 * i + 4], diffs[6 * i + 5]); computePartials(h.p, h.ng, rdpdu, rdpdv, ro3, rxd, ryd, rpa); }
    // ---- the surface step, every gate on; the differentials are the caller's, the first textured value is kept for the record
    v3 firstValue = V(0, 0, 0); bool haveFirst = false;
    const SurfaceBsdf sf = resolveSurface<false, true, true, true, true, true, true>(sc, tb, h, prim, inst, hr, ro3, d, diffs != nullptr, [&](v3 &a, v3 &b) { a = rxd; b = ryd; },
                                                                                   [&](v3 c) { if (!haveFirst) { firstValue = c; haveFirst = true; } });
    const v3 wiQ = queryWi<true>(h, sf);
    if (mode == 0) {
        const v3 opac = sf.masked ? sf.opac : V(0, 0, 0);                    // (the stages' default opacity is 1; the record's is zero without a mask)
        o[0] = ruvx; o[1] = ruvy; o[2] = rdpdu.x; o[3] = rdpdu.y; o[4] = rdpdu.z; o[5] = rdpdv.x; o[6] = rdpdv.y; o[7] = rdpdv.z;
        o[8] = rpa[0]; o[9] = rpa[1]; o[10] = rpa[2]; o[11] = rpa[3];
        o[12] = opac.x; o[13] = opac.y; o[14] = opac.z; o[15] = firstValue.x; o[16] = firstValue.y; o[17] = firstValue.z;
        o[18] = sf.masked ? 1.0f : 0.0f; o[19] = sf.bumped ? 1.0f : 0.0f; o[20] = (float) sf.coat; o[21] = (float) sf.leaf;
        o[22] = sf.bsdf.reflectance[0]; o[23] = sf.bsdf.reflectance[1]; o[24] = sf.bsdf.reflectance[2];
        o[25] = sf.ps.x; o[26] = sf.ps.y; o[27] = sf.ps.z; o[28] = sf.pt.x; o[29] = sf.pt.y; o[30] = sf.pt.z; o[31] = sf.pn.x; o[32] = sf.pn.y; o[33] = sf.pn.z;
        o[34] = wiQ.x; o[35] = wiQ.y; o[36] = wiQ.z; o[37] = hr.x; o[38] = hr.y; o[39] = hr.z; o[40] = hr.w; o[41] = (float) inst;
        o[42] = h.ns.x; o[43] = h.ns.y; o[44] = h.ns.z; o[45] = h.s.x; o[46] = h.s.y; o[47] = h.s.z; o[48] = h.t.x; o[49] = h.t.y; o[50] = h.t.z;
    } else if (mode == 1) {
        const float *p = query + 3 * i; const float extraValue = p[2]; bool drawn = false;
        auto drawExtra = [&]() { drawn = true; return extraValue; };
        v3 wo = V(0, 0, 0); float pdf = 0.0f, eta = 0.0f; bool delta = false, nullComp = false;
        const v3 w = ctSample<true, true>(sc, tb, sf.coat, sf.bsdf, wiQ, p[0], p[1], drawExtra, wo, pdf, eta, delta, nullComp);
        o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = pdf; o[4] = wo.x; o[5] = wo.y; o[6] = wo.z; o[7] = eta;
        o[8] = delta ? 1.0f : 0.0f; o[9] = nullComp ? 1.0f : 0.0f; o[10] = drawn ? 1.0f : 0.0f;
    } else {
        const float *p = query + 3 * i; const v3 wo = toLocal(h, V(p[0], p[1], p[2]));
        v3 wiE, woQ; bool rejected; queryFrame<true>(h, sf, wo, wiE, woQ, rejected);      // (the sign rejection is applied by the stages after this query, not here)
        const v3 e = ctEval<true, true>(sc, tb, sf.coat, sf.bsdf, wiE, woQ);
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = ctPdf<true, true>(sc, tb, sf.coat, sf.bsdf, wiE, woQ);
    }
}

extern "C" {
void mi_launch_debug_surface(const DScene &sc, int mode, const float *rays, const float *hits, const int *insts, const float *diffs, const float *query, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_surface, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, mode, rays, hits, insts, diffs, query, n, out);
}
void mi_launch_debug_bsdf(const DScene &sc, int material, int mode, const float *in, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_bsdf, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, material, mode, in, n, out);
}
void mi_launch_debug_texture(const DScene &sc, uint32_t texture, const float *uv, const float *partials, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_texture, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, texture, uv, partials, n, out);
}
void mi_launch_debug_emitter_sample(const DScene &sc, int raw, const float *in, uint64_t n, float *out, hipStream_t st) {
    if (raw) hipLaunchKernelGGL(k_debug_emitter_sample<true>, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, in, n, out);
    else hipLaunchKernelGGL(k_debug_emitter_sample<false>, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, in, n, out);
}
void mi_launch_debug_emitter_eval(const DScene &sc, int emitter, int kind, const float *in, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_emitter_eval, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, emitter, kind, in, n, out);
}
void mi_launch_debug_medium(const DScene &sc, uint32_t medium, int mode, const float *in, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_medium, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, medium, mode, in, n, out);
}
}
