// shade.h -- the shading stage: one bounce of MIPathTracer::Li per launch (see kernels_common.h).  Instantiated by kernels_shade_*.hip, one translation
// unit per (RC, ENV) pair so that `make -j` compiles the variants side by side.
#pragma once
#include "kernels_common.h"
#include "surface.h"
#ifndef MI_SHADE_MIN_WAVES
#define MI_SHADE_MIN_WAVES 1      // waves per SIMD asked of the compiler (A/B builds; DESIGN.md §3: a register cap only moves the live set into scratch)
#endif

// ---------------------------------------------------------------------------------------------- shade
// One bounce of MIPathTracer::Li (src/integrators/path/path.cpp:135-287) for every live path of the segment:
//   tail of the previous iteration (emitter hit by the BSDF ray -> MIS term :257-264, Russian roulette :276-286), then
//   emitted radiance :148-150, depth test :156-165, emitter sampling :172-200 (visibility deferred to the shadow queue),
//   BSDF sampling :207-226.  Survivors are compacted into the other ray/state buffer, shadow rays into the shadow queue.
// WRAP: the BSDF adapters mixturebsdf / bumpmap / normalmap are present (only with RC and AN): scenes without them keep the leaner kernels
template <bool RC, bool ENV, bool SMALL, bool AN, bool TEX, bool WRAP>   // TEX: textures bound to materials (implies AN); RC: rough conductors present; ENV: environment emitter present; SMALL: scene tables staged in LDS; AN ("extended"): analytic shapes or delta emitters (point / spot / directional) present
__global__ __launch_bounds__(WG, MI_SHADE_MIN_WAVES) void k_shade(DScene sc, RenderConst rc, Queues q, int buf) {
    extern __shared__ uint32_t s_dyn[];
    uint32_t *s_nib = s_dyn;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = buf ^ 1;
    const SobolTabLds m32{(lds_u32_ptr) s_nib, rc.nib_count, rc.sobol_scramble};   // always the LDS copy (ds_read lookups); unused by the independent stream
    const uint32_t nibWords = rc.sampler == 1 ? rc.nib_dims * rc.nib_count * 16u : 4u;
    if (rc.sampler == 1) {   // stage the Sobol' nibble tables in LDS (nib_dims x nib_count x 16 words)
        for (uint32_t i = tid; i < nibWords; i += WG) s_nib[i] = rc.sobol_nib[i];
    }
    Tabs<SMALL> tb; stageTables<SMALL, WG>(sc, s_dyn + ((nibWords + 3u) & ~3u), tid, tb);      // scene tables: small scenes are staged in LDS (surface.h)
    // Material-sorted shading (scenes that mix BSDF classes): the paths of a segment are first ordered by the class of the surface
    // they hit -- diffuse-like from the front, rough conductors from the back of an LDS index list (wave64 ballots, order preserving) --
    // so a wave runs either the cheap diffuse code or the microfacet code, not both.  The queues are then read through that list.
    // In this stage a SEGMENT IS OWNED BY ONE WAVE: compaction is a pair of wave64 ballots with the running output offsets kept in
    // (uniform) registers -- no LDS exchange and no workgroup barrier anywhere in the loop; the four waves of a workgroup only share the
    // LDS copies of the tables above.
    uint16_t *s_order = reinterpret_cast<uint16_t *>(s_dyn + rc.order_offset_words) + (size_t) wave * q.cap;
    const bool doSort = RC && rc.order_offset_words != 0 && q.cap <= 0xFFFFu;
    unsigned long long pathLen = 0, shadowRays = 0;
    __syncthreads();                                         // tables staged
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t seg = blockIdx.x * (WG / 64) + wave; seg < q.n_seg; seg += gridDim.x * (WG / 64)) {
    const uint32_t n = q.count[buf][seg];
    const uint32_t segBase = seg * q.cap;                    // (a pool has fewer than 2^28 slots: queues.h qat)
    uint32_t outA = 0, outS = 0;                             // survivors / shadow records written so far (uniform)
    uint32_t done0 = 0, done1 = 0;                           // uniform running counts (front / back)
    if (doSort) {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane; int cls = 2;
            if (i < n) {
                const uint32_t prim = __float_as_uint(qat(q.hit, segBase + i).w);
                if (prim == 0xFFFFFFFFu) cls = 0;
                else if (AN && prim >= sc.n_tris) cls = (sc.analytic[prim - sc.n_tris].flags & 8u) ? 1 : 0;
                else cls = (__float_as_uint(tb.shade4[prim * (uint32_t) MI_SHADE_WORDS + 2u].w) & 8u) ? 1 : 0;
            }
            const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1);
            if (cls == 0) s_order[done0 + (uint32_t) __popcll(m0 & lt)] = (uint16_t) i;
            else if (cls == 1) s_order[n - 1u - (done1 + (uint32_t) __popcll(m1 & lt))] = (uint16_t) i;
            done0 += (uint32_t) __popcll(m0); done1 += (uint32_t) __popcll(m1);
        }
    }
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        // Two phases per chunk, each closed by its own wave64 ballot, so that the 12 registers of a shadow record are written out before
        // the BSDF-sampling code runs (register budget -> one more resident wave per SIMD):
        //   A: tail of the previous bounce, emitted radiance, emitter sampling  -> shadow queue
        //   B: BSDF sampling                                                     -> next ray / state
        bool alive = false, wantShadow = false, toSample = false;
        float4 shO, shD; v3 shC = V(0, 0, 0);
        Hit h; SurfaceBsdf sf; SamplerState ss; v3 T = V(0, 0, 0); float eta = 1.0f; uint32_t pid = 0; int depth = 0; bool unscattered = false;   // sf: the resolved surface (surface.h) -- leaf record, mask opacity (RC variants), perturbed frame and coating (WRAP variants)
        if (i < n) {
            const uint32_t slot = segBase + (doSort ? (uint32_t) s_order[i] : i);
            const auto rd = qRayDirection(q, buf, slot); float4 hr = qat(q.hit, slot); uint4 s0 = qat(q.st0[buf], slot);
            // the first launch of a batch (rc.first_bounce, launch-uniform) sees fresh paths only: throughput (1,1,1), eta 1, bsdfPdf 0 -- k_generate stores none of them.
            // eta leaves 1 only through a BSDF of the RC variants (every sampler of the others sets it to 1, pt_device.h bsdfSample): they alone have the array
            float prevPdf = 0.0f; T = V(1, 1, 1);
            if (!rc.first_bounce) { const auto s1 = qThroughput(q, buf, slot); T = V(s1.x, s1.y, s1.z); prevPdf = qat(q.st2[buf], slot); if (RC) eta = qEta(q, buf, slot); }
            pid = s0.x; ss.a = s0.y; ss.b = s0.z; ss.dim = s0.w & 0xFFu;
            depth = (int) ((s0.w >> 8) & 0xFFu); const bool facingRef = ((s0.w >> 16) & 1u) != 0;
            const bool prevDelta = RC && ((s0.w >> 17) & 1u) != 0;      // the BSDF sample that spawned this ray was a delta component -> lumPdf = 0 (path.cpp:259-260)
            unscattered = RC && ((s0.w >> 18) & 1u) != 0;    // every component sampled so far was ENull (thin dielectric panes): `scattered` is still false (path.cpp:213)
            v3 d = V(rd.x, rd.y, rd.z);
            const uint32_t prim = __float_as_uint(hr.w);
            v3 add = V(0, 0, 0); bool haveAdd = false;
            do {
                if (prim == 0xFFFFFFFFu) {                                     // miss: path.cpp:136-143 / :234-248
                    pathLen += (unsigned) (depth > 1 ? depth - 1 : 1);
                    // the pixel's accumulator is read HERE, next to the ray origin, so that its round trip to HBM overlaps the environment lookup instead of following it
                    const bool clearAlpha = depth == 1 && rc.opacity;                                                 // records.inl:121-137: alpha = 0 on a camera-ray miss
                    float4 accum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (ENV || clearAlpha) accum = qat(q.acc, pid);
                    if (clearAlpha) accum.w = 0.0f;
                    if (ENV) {
                        if (depth == 1) { if (!rc.hide_emitters && !sc.env_texture) { add = T * envEval(sc, d); haveAdd = true; } }     // path.cpp:139-141; with a MIP pyramid k_env_primary has added the filtered lookup
                        else {
                            // BSDF ray left the scene: env->evalEnvironment + fillDirectSamplingRecord (envmap.cpp:362-378), MIS term path.cpp:257-264
                            // (the ray origin is only needed for the bounding-sphere test: it is requested first and consumed after the environment lookup, whose
                            // atan2f / acosf and texel fetches then cover its round trip to HBM)
                            const auto ro = qRayOrigin(q, buf, slot); float nearT, farT;
                            if (!(rc.hide_emitters && unscattered)) {   // path.cpp:238-239: hideEmitters && !scattered
                                v3 value; float pdfSA;
                                if (sc.env_constant) {      // ConstantBackgroundEmitter::pdfDirect (constant.cpp:219-233): needs the reference normal of the previous vertex
                                    value = envEval(sc, d);
                                    const float c = qat(q.st3[buf], slot); pdfSA = c != 2.0f ? MI_INV_PI * maxf(0.0f, c) : MI_INV_FOURPI;
                                } else envEvalAndPdf(sc, d, value, pdfSA);      // one atan2f / acosf and one set of texels for both
                                if (bsphereIntersect(sc, V(ro.x, ro.y, ro.z), d, nearT, farT) && !(nearT > 0) && !(farT < 0)) {
                                float lumPdf = prevDelta ? 0.0f : pdfSA * (loadEmitter(tb, sc.env_index).weight * sc.emitter_norm);
                                add = (T * value) * miWeight(prevPdf, lumPdf); haveAdd = true;
                                }
                            }
                        }
                    }
                    if (haveAdd) { accum.x += add.x; accum.y += add.y; accum.z += add.z; }
                    if (haveAdd || clearAlpha) qat(q.acc, pid) = accum;
                    haveAdd = false;
                    break;
                }
                v3 ro3 = V(0, 0, 0);
                if (AN) { const auto ro = qRayOrigin(q, buf, slot); ro3 = V(ro.x, ro.y, ro.z); }      // analytic shapes: hit point = o + t d; sphere lights: reference point of pdfDirect
                const int inst = (AN && q.hitInst) ? qat(q.hitInst, slot) : -1;
                fillHitAny<SMALL, AN>(sc, tb, inst, ro3, d, hr.x, hr.y, hr.z, prim, h);
                if (depth > 1) {
                    if (h.emitter >= 0) {                                    // path.cpp:229-233, 257-264
                        v3 value = emitterEval(tb, h.emitter, h.ns, -d);
                        float lumPdf = prevDelta ? 0.0f : pdfEmitterDirect<AN>(sc, tb, h.emitter, ro3, d, h.ns, h.dist, facingRef);
                        add = (T * value) * miWeight(prevPdf, lumPdf); haveAdd = true;
                    }
                    const int prevDepth = depth - 1;                         // rRec.depth++ >= m_rrDepth (path.cpp:276)
                    if (prevDepth >= rc.rr_depth) {
                        float qq = minf(maxf(maxf(T.x, T.y), T.z) * eta * eta, 0.95f);
                        if (next1D(ss, rc.sampler, m32) >= qq) { pathLen += (unsigned) depth; break; }
                        float r = 1.0f / qq; T = T * r;
                    }
                }
                if (!(depth <= rc.max_depth || rc.max_depth < 0)) { pathLen += (unsigned) depth; break; }   // loop guard path.cpp:135
                // the surface step (surface.h): material, textured parameters (filtered on the camera hit, whose differentials come from the film position), mask, bump / normal map, coating
                auto diffs = [&](v3 &rxd, v3 &ryd) { const float2 sp = qat(q.pos, pid); sensorDifferentials(sc, rc, m32, ss.a, ss.b, sp.x, sp.y, d, rxd, ryd); };
                sf = resolveSurface<SMALL, AN, TEX, RC, WRAP && TEX, WRAP, true>(sc, tb, h, prim, inst, hr, ro3, d, depth == 1, diffs);
                if (depth == 1 && h.emitter >= 0 && !rc.hide_emitters) {    // path.cpp:148-150 (EEmittedRadiance only on the camera segment)
                    add = T * emitterEval(tb, h.emitter, h.ns, -d); haveAdd = true;
                }
                if ((depth >= rc.max_depth && rc.max_depth > 0) || (rc.strict_normals && dot(d, h.ng) * h.wi.z >= 0)) { pathLen += (unsigned) depth; break; }
                // emitter sampling (path.cpp:172-200)
                v3 refN = (h.flags & 2u) ? V(0, 0, 0) : h.ns;               // records.inl:160-164
                if (!(h.flags & 4u)) {                                       // bsdf->getType() & BSDF::ESmooth
                    float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                    Direct dr; v3 value = sampleEmitterDirect<ENV, AN>(sc, tb, h.p, refN, sx, sy, dr);
                    if (dr.pdf != 0) {
                        ++shadowRays;                                        // scene.cpp:871-875: a shadow ray is cast whenever pdf != 0
                        v3 wo = toLocal(h, dr.d);
                        v3 wiQ, woQ; bool rejected; queryFrame<WRAP>(h, sf, wo, wiQ, woQ, rejected);      // bumpmap.cpp:165-180: the query in the perturbed frame
                        v3 bsdfVal = rejected ? V(0, 0, 0) : ctEval<RC, WRAP>(sc, tb, sf.coat, sf.bsdf, wiQ, woQ);
                        if (RC && sf.masked) bsdfVal = bsdfVal * sf.opac;                    // mask.cpp:124-127
                        if (!isZero(value) && !isZero(bsdfVal) && (!rc.strict_normals || dot(h.ng, dr.d) * wo.z > 0)) {
                            float bp = (dr.delta || rejected) ? 0.0f : ctPdf<RC, WRAP>(sc, tb, sf.coat, sf.bsdf, wiQ, woQ);     // emitter->isOnSurface() && measure == ESolidAngle (path.cpp:191-192)
                            if (RC && sf.masked) bp *= luminance3(sf.opac);                    // mask.cpp:141-146
                            float weight = miWeight(dr.pdf, bp);
                            v3 c = ((T * value) * bsdfVal) * weight;
                            wantShadow = true;
                            shO = make_float4(h.p.x, h.p.y, h.p.z, dr.dist * (1 - MI_SHADOW_EPSILON));
                            shD = make_float4(dr.d.x, dr.d.y, dr.d.z, __uint_as_float(pid));
                            shC = c;
                        }
                    }
                }
                toSample = true;
            } while (false);
            if (haveAdd) { float4 a = qat(q.acc, pid); a.x += add.x; a.y += add.y; a.z += add.z; qat(q.acc, pid) = a; }
        }
        // wave64 ballots: order-preserving compaction inside the (wave-owned) segment
        const unsigned long long mS = __ballot(wantShadow);
        if (wantShadow) {
            const uint32_t o = segBase + outS + (uint32_t) __popcll(mS & lt);
            qat(q.shO, o) = shO; qat(q.shD, o) = shD; qSetShadowContribution(q, o, shC.x, shC.y, shC.z);
        }
        outS += (uint32_t) __popcll(mS);
        v3 nrO = V(0, 0, 0), nrD = V(0, 0, 0); uint4 nS0; float nS2 = 0, nS3 = 0;      // (the bounce ray's interval is (Epsilon, inf) for every survivor: the next extend launch knows it)
        if (toSample) {
            // BSDF sampling (path.cpp:207-226)
            float bPdf = 0, bEta = 1; v3 woL = V(0, 0, 0);
            float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
            bool sampledDelta, sampledNull; v3 bw;
            bool passThrough = false;                                                   // mask.cpp:196-208: the nested BSDF with probability luminance(opacity), else straight through
            if (RC && sf.masked) passThrough = maskChooseLobe(sf.opac, sx);
            if (RC && passThrough) bw = maskPassThrough(h, sf.opac, woL, bPdf, sampledDelta, sampledNull);
            else {
                auto drawExtra = [&]() { return next1D(ss, rc.sampler, m32); };        // bRec.sampler->next1D() inside BSDF::sample (EUsesSampler), only if the sampled BSDF asks
                bw = sampleInQueryFrame<WRAP>(h, sf, [&](v3 wi, v3 &wo) __attribute__((always_inline)) { return ctSample<RC, WRAP>(sc, tb, sf.coat, sf.bsdf, wi, sx, sy, drawExtra, wo, bPdf, bEta, sampledDelta, sampledNull); }, woL);
                if (RC && sf.masked) { const float prob = luminance3(sf.opac); bw = V(bw.x * sf.opac.x / prob, bw.y * sf.opac.y / prob, bw.z * sf.opac.z / prob); bPdf *= prob; }
            }
            v3 wo = toWorld(h, woL);
            if (isZero(bw) || (rc.strict_normals && dot(h.ng, wo) * woL.z <= 0)) pathLen += (unsigned) depth;
            else {
                T = T * bw; eta *= bEta;
                alive = true;
                nrO = h.p; nrD = wo;
                v3 refN = (h.flags & 2u) ? V(0, 0, 0) : h.ns;           // records.inl:160-164
                const float cosRef = dot(wo, refN);
                uint32_t fl = cosRef >= 0 ? 1u : 0u;
                nS3 = (h.flags & 2u) ? 2.0f : cosRef;
                nS0 = make_uint4(pid, ss.a, ss.b, (ss.dim & 0xFFu) | ((uint32_t) (depth + 1) << 8) | (fl << 16) | ((RC && sampledDelta) ? (1u << 17) : 0u) | ((RC && sampledNull && (depth == 1 || unscattered)) ? (1u << 18) : 0u));
                nS2 = bPdf;
            }
        }
        const unsigned long long mA = __ballot(alive);
        if (alive) {
            const uint32_t o = segBase + outA + (uint32_t) __popcll(mA & lt);
            qSetRayOrigin(q, nb, o, nrO.x, nrO.y, nrO.z); qSetRayDirection(q, nb, o, nrD.x, nrD.y, nrD.z); qat(q.st0[nb], o) = nS0; qSetThroughput(q, nb, o, T.x, T.y, T.z); qat(q.st2[nb], o) = nS2;
            if (RC) qSetEta(q, nb, o, eta);
            if (ENV && sc.env_constant) qat(q.st3[nb], o) = nS3;
        }
        outA += (uint32_t) __popcll(mA);
    }
    if (lane == 0) { q.count[nb][seg] = outA; q.shCount[seg] = outS; }
    }
    // counters: wave reduction, one atomic per wave
    for (int off = 32; off > 0; off >>= 1) { pathLen += __shfl_down(pathLen, off); shadowRays += __shfl_down(shadowRays, off); }
    if (lane == 0) { if (pathLen) atomicAdd(&q.counters[2], pathLen); if (shadowRays) atomicAdd(&q.counters[1], shadowRays); }
}



// launch the (AN, TEX) variant of one (RC, ENV, WRAP, SMALL) combination that fits the scene; WRAP variants exist for AN = true only
template <bool RC, bool ENV, bool WRAP, bool SM>
static void launchShadeVariantSM(const DScene &sc, const RenderConst &rc, const Queues &q, int buf, uint32_t grid, size_t lds, hipStream_t st) {
    if ((sc.ext || WRAP) && sc.n_textures) launchWithLds(k_shade<RC, ENV, SM, true, true, WRAP>, grid, lds, st, sc, rc, q, buf);
    else if (sc.ext || WRAP) launchWithLds(k_shade<RC, ENV, SM, true, false, WRAP>, grid, lds, st, sc, rc, q, buf);
    else launchWithLds(k_shade<RC, ENV, SM, WRAP, false, WRAP>, grid, lds, st, sc, rc, q, buf);
}
// both SMALL halves from one translation unit (the WRAP combinations compile theirs in two: kernels_shade_rcw*_small.hip, for the build time)
template <bool RC, bool ENV, bool WRAP>
static void launchShadeVariant(const DScene &sc, const RenderConst &rc, const Queues &q, int buf, uint32_t grid, size_t lds, hipStream_t st) {
    if (sc.small_tables != 0) launchShadeVariantSM<RC, ENV, WRAP, true>(sc, rc, q, buf, grid, lds, st);
    else launchShadeVariantSM<RC, ENV, WRAP, false>(sc, rc, q, buf, grid, lds, st);
}
