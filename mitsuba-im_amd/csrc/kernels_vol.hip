// kernels_vol.hip -- the volumetric variant of the path: SimpleVolumetricPathTracer::Li (reference src/integrators/path/volpath_simple.cpp:84-289) over homogeneous
// media (src/medium/homogeneous.cpp, src/phase/isotropic.cpp, hg.cpp) and index-matched boundaries (src/bsdfs/null.cpp), as two stages next to generate / extend / film:
//   k_shade_vol   one iteration of the loop per launch: tail of the previous one (Russian roulette :278-287), distance sampling in the current medium :114, then either
//                 the medium interaction (emitter sampling :127-138, phase-function sampling :149-162) or the surface interaction (:163-275) -- both leave at most one
//                 shadow RECORD and one continuation ray;
//   k_shadow_vol  Scene::sampleAttenuatedEmitterDirect's second half: Scene::evalTransmittance (src/librender/scene.cpp:650-713) walks from the reference point to the
//                 emitter sample through `null` boundaries and media, then `Li += throughput * (value * transmittance / emitterPdf) * (BSDF | phase) value`.
// No MIS in this integrator: emitters seen by continuation rays count only while the radiance-type bits say so (camera ray, chains of delta / null interactions).
// The state word (VS_*), the shadow record (SR_*) and everything this file shares with kernels_volmis.hip: volume.h.
// Built for: meshes + analytic shapes (media on scene-level shapes), every plain BSDF incl. `null`, textures, area / point / spot / directional emitters.  Refused at
// mi_render_create: adapters (mixturebsdf / bumpmap / normalmap) that nest a `null` / `thindielectric`.  A `mask` attenuates the walks by 1 - opacity (surfaceNullEval).
#include "volume.h"

template <bool TEX, bool ENV, bool WRAP>      // forShadeVariant (volume.h)
__global__ __launch_bounds__(WG) void k_shade_vol(DScene sc, RenderConst rc, Queues q, int buf) {
    extern __shared__ uint32_t s_dyn[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = buf ^ 1;
    const SobolTabLds m32 = stageSobolTables(rc, s_dyn, tid);
    const Tabs<false> tb = globalTabs(sc);
    unsigned long long pathLen = 0;
    __syncthreads();
    forEachChunkOfOwnedSegments(q, buf, lane, wave, [&](uint32_t i, uint32_t n, SegmentWriter &out) __attribute__((always_inline)) {
        bool alive = false, wantShadow = false, wantAlpha = false;
        ShadowRec sh, al; float4 nrO, nrD, nS1; uint4 nS0;
        if (i < n) {
            const uint64_t slot = out.segBase + i;
            float4 ro, rd; loadRayWithInterval(q, buf, slot, ro, rd); const float4 hr = q.hit[slot]; const uint4 s0 = q.st0[buf][slot];
            SamplerState ss; uint32_t pid; int depth, medium; v3 T; float eta; unpackPathState(s0, loadThroughputEta(q, buf, slot), pid, ss, depth, medium, T, eta);
            uint32_t fl = s0.w & (VS_EMITTED | VS_OTHERS | VS_NULLCHAIN | VS_SCATTERED);
            const v3 o = V(ro.x, ro.y, ro.z), d = V(rd.x, rd.y, rd.z);
            const uint32_t prim = __float_as_uint(hr.w); const float tHit = prim == 0xFFFFFFFFu ? INFINITY : hr.x;
            v3 add = V(0, 0, 0); bool haveAdd = false;
            do {
                if (depth > 1 && depth - 1 >= rc.rr_depth && !russianRoulette(T, eta, [&]() { return next1D(ss, rc.sampler, m32); })) { pathLen += (unsigned) depth; break; }
                if (!(depth <= rc.max_depth || rc.max_depth < 0)) { pathLen += (unsigned) depth; break; }
                const bool others = (fl & VS_OTHERS) != 0, emitted = (fl & VS_EMITTED) != 0, scattered = (fl & VS_SCATTERED) != 0;
                MediumRec mRec; bool mediumEvent = false; MediumD md;
                if (medium >= 0) { md = sc.media[medium]; mediumEvent = mediumSampleDistance(md, o, d, 0.0f, tHit, [&]() { return next1D(ss, rc.sampler, m32); }, mRec); }
                if (depth == 1 && rc.opacity) wantAlpha = sensorRayOpacity(sc, rc, q, tb, slot, pid, o, d, hr, medium, md, al);
                const int interactions = rc.max_depth - depth - 1;
                // ---- the interaction: a point in the medium, or the surface at the end of the segment
                bool nee = false; v3 nref = V(0, 0, 0), nrefN = V(0, 0, 0); Hit h; SurfaceBsdf sf; uint32_t pm = 0;
                if (mediumEvent) {
                    { const float r = 1.0f / mRec.pdfSuccess; T = T * ((ld3(md.sigma_s) * mRec.transmittance) * r); }
                    nee = others; nref = mRec.p;                             // EDirectMediumRadiance
                } else {
                    if (medium >= 0) { const float r = 1.0f / mRec.pdfFailure; T = T * (mRec.transmittance * r); }
                    if (prim == 0xFFFFFFFFu) {                               // volpath_simple.cpp:172-183: possibly attenuated radiance from the environment
                        if (ENV && emitted && (!rc.hide_emitters || scattered)) {
                            v3 value = T * (depth == 1 ? envEvalSensorRay(sc, rc, m32, ss, d, q.pos[pid]) : envEval(sc, d));
                            if (medium >= 0) value = value * mediumTransmittance(md, ro.w, rd.w);
                            add = value; haveAdd = true;
                        }
                        pathLen += (unsigned) depth; break;
                    }
                    const int inst = q.hitInst ? q.hitInst[slot] : -1;
                    fillHitAny<false, true>(sc, tb, inst, o, d, hr.x, hr.y, hr.z, prim, h);
                    if (h.emitter >= 0 && emitted && (!rc.hide_emitters || scattered)) { add = T * emitterEval(tb, h.emitter, h.ns, -d); haveAdd = true; }
                    if (rc.strict_normals && (-dot(h.ng, d)) * h.wi.z < 0) { pathLen += (unsigned) depth; break; }
                    // the surface step (surface.h): material, textured reflectance (only the sensor ray carries differentials), mask, bump / normal map
                    auto diffs = [&](v3 &rxd, v3 &ryd) { const float2 sp = q.pos[pid]; sensorDifferentials(sc, rc, m32, ss.a, ss.b, sp.x, sp.y, d, rxd, ryd); };
                    sf = resolveSurface<false, true, TEX, true, WRAP && TEX, false, WRAP>(sc, tb, h, prim, inst, hr, o, d, depth == 1, diffs);
                    pm = sc.prim_media ? sc.prim_media[prim] : 0u;           // (interior + 1) | (exterior + 1) << 16 of the shape that was hit; 0: not a medium transition
                    nee = others && !(h.flags & 4u); nref = h.p;            // EDirectSurfaceRadiance, BSDFs with a smooth component
                    if (!(h.flags & 2u)) nrefN = h.ns;                       // records.inl:160-164
                }
                // ---- emitter sampling for either interaction (volpath_simple.cpp:127-138 / :197-216): the record goes to k_shadow_vol, which attenuates and adds it
                if (nee) {
                    float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                    Direct dr; const v3 value = sampleEmitterDirect<ENV, true, false, true>(sc, tb, nref, nrefN, sx, sy, dr);
                    if (dr.pdf != 0) {
                        v3 x; int m2 = medium;
                        if (mediumEvent) { const float ph = phaseEval(md, -d, dr.d); x = V(ph, ph, ph); }
                        else {
                            const v3 wo = toLocal(h, dr.d);
                            v3 wiQ, woQ; bool rejected; queryFrame<WRAP>(h, sf, wo, wiQ, woQ, rejected);      // bumpmap.cpp:165-180
                            x = (!rejected && (!rc.strict_normals || dot(h.ng, dr.d) * wo.z > 0)) ? mxEval<true, WRAP>(sc, tb, sf.bsdf, wiQ, woQ) : V(0, 0, 0);
                            if (sf.masked) x = x * sf.opac;                      // mask.cpp:117-118
                            if (pm) m2 = targetMedium(pm, h.ng, dr.d);      // scene.cpp:920-921
                        }
                        wantShadow = true;
                        sh = emitterSampleRecord(nref, m2, interactions, !mediumEvent, dr, value, pid, T, x, 0.0f);
                    }
                }
                // ---- the continuation ray
                if (mediumEvent) {                                           // phase-function sampling (volpath_simple.cpp:141-162)
                    if ((depth + 1 >= rc.max_depth && rc.max_depth > 0) || !others) { pathLen += (unsigned) depth; break; }
                    float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                    const v3 wo = phaseSample(md, -d, sx, sy);
                    fl = (fl & ~VS_NULLCHAIN) | VS_SCATTERED;
                    alive = true;
                    nrO = make_float4(mRec.p.x, mRec.p.y, mRec.p.z, 0.0f); nrD = make_float4(wo.x, wo.y, wo.z, INFINITY);
                    break;
                }
                float bPdf = 0, bEta = 1; v3 woL = V(0, 0, 0); bool sampledDelta, sampledNull;
                float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                auto drawExtra = [&]() { return next1D(ss, rc.sampler, m32); };
                if (sf.bsdf.type == MI_BSDF_T_THINDIELECTRIC) sf.bsdf.flags |= MI_THIN_SIGNED_COS;      // the pdf-less ThinDielectric::sample overload this integrator calls (pt_device.h)
                v3 bw; bool passThrough = false; float invProb = 1.0f;      // mask.cpp:152-172, the overload WITHOUT a pdf: sample.x *= 1 / prob, result * opacity * (1 / prob) -- not maskChooseLobe's division
                if (sf.masked) { const float prob = luminance3(sf.opac); if (sx < prob) { invProb = 1.0f / prob; sx *= invProb; } else passThrough = true; }
                if (passThrough) bw = maskPassThrough(h, sf.opac, woL, bPdf, sampledDelta, sampledNull);
                else bw = sampleInQueryFrame<WRAP>(h, sf, [&](v3 wi, v3 &wo) __attribute__((always_inline)) { return mxSample<true, WRAP>(sc, tb, sf.bsdf, wi, sx, sy, drawExtra, wo, bPdf, bEta, sampledDelta, sampledNull); }, woL);      // bumpmap.cpp:196-216
                if (sf.masked && !passThrough) bw = V(bw.x * sf.opac.x * invProb, bw.y * sf.opac.y * invProb, bw.z * sf.opac.z * invProb);
                if (isZero(bw)) { pathLen += (unsigned) depth; break; }
                // which radiance types the next iteration gathers (volpath_simple.cpp:236-257)
                const bool rtOthers = (depth + 1 < rc.max_depth || rc.max_depth < 0) && others; bool rtEmitted = false; bool nullChain = (fl & VS_NULLCHAIN) != 0;
                if ((depth < rc.max_depth || rc.max_depth < 0) && others && sampledDelta && (!sampledNull || nullChain)) { rtEmitted = true; nullChain = true; }
                else nullChain = nullChain && sampledNull;
                if (!rtOthers && !rtEmitted) { pathLen += (unsigned) depth; break; }
                const v3 wo = toWorld(h, woL);
                if (dot(h.ng, wo) * woL.z <= 0 && rc.strict_normals) { pathLen += (unsigned) depth; break; }
                T = T * bw; eta *= bEta;
                if (pm) medium = targetMedium(pm, h.ng, wo);                 // its.isMediumTransition(): rRec.medium = its.getTargetMedium(wo)
                fl = (rtOthers ? VS_OTHERS : 0u) | (rtEmitted ? VS_EMITTED : 0u) | (nullChain ? VS_NULLCHAIN : 0u) | ((scattered || !sampledNull) ? VS_SCATTERED : 0u);
                alive = true;
                nrO = make_float4(h.p.x, h.p.y, h.p.z, MI_EPSILON); nrD = make_float4(wo.x, wo.y, wo.z, INFINITY);
            } while (false);
            if (alive) packPathState(pid, ss, depth, fl, medium, T, eta, nS0, nS1);
            if (haveAdd) addRadiance(q, pid, add);
        }
        const uint64_t wE = out.backRecord(q, wantAlpha), wS = out.frontRecord(wantShadow), wA = out.survivor(alive);
        if (wantAlpha) { q.shO[wE] = al.o; q.shD[wE] = al.d; }
        if (wantShadow) storeShadowRecord(q, wS, sh);
        if (alive) { storeRayWithInterval(q, nb, wA, nrO, nrD); q.st0[nb][wA] = nS0; storeThroughputEta(q, nb, wA, nS1); q.st2[nb][wA] = 0.0f; }
    });
    waveAddCounter(&q.counters[2], pathLen, lane);
}

// Scene::evalTransmittance for every shadow record of the segment, then the deferred `Li +=` (volume.h)
template <bool WIDE, bool NX>      // forShadowVariant (volume.h)
__global__ __launch_bounds__(WG) void k_shadow_vol(DScene sc, Queues q) {
    __shared__ int s_stk[STACK_DEPTH * WG];
    const uint32_t tid = threadIdx.x;
    const Tabs<false> tb = globalTabs(sc);
    unsigned long long rays = 0;
    for (uint32_t seg = blockIdx.x; seg < q.n_seg; seg += gridDim.x)
        forEachShadowRecord(q, seg, tid, [&](uint64_t w) __attribute__((always_inline)) {
            const float4 so = q.shO[w], sd = q.shD[w];
            const uint32_t bits = __float_as_uint(so.w), pid = __float_as_uint(sd.w);
            bool blocked; const v3 tr = transmittanceWalk<WIDE, NX>(sc, tb, s_stk + tid, V(so.x, so.y, so.z), V(sd.x, sd.y, sd.z), bits, rays, blocked);
            addTransmittedSample<false>(q, w, bits, pid, tr, blocked);
        });
    waveAddCounter(&q.counters[1], rays, tid & 63u);
}

extern "C" {
void mi_launch_shade_vol(const DScene &sc, const RenderConst &rc, const Queues &q, int buf, uint32_t grid, size_t lds, hipStream_t st) {
    forShadeVariant(sc, [&](auto tex, auto env, auto wrap) { launchWithLds(k_shade_vol<decltype(tex)::value, decltype(env)::value, decltype(wrap)::value>, grid, lds, st, sc, rc, q, buf); });
}
void mi_launch_shadow_vol(const DScene &sc, const Queues &q, uint32_t grid, hipStream_t st) {
    forShadowVariant(sc, [&](auto wide, auto, auto nx) { hipLaunchKernelGGL((k_shadow_vol<decltype(wide)::value, decltype(nx)::value>), dim3(grid), dim3(WG), 0, st, sc, q); });
}
}
