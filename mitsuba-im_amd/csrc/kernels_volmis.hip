// kernels_volmis.hip -- VolumetricPathTracer::Li (reference src/integrators/path/volpath.cpp:84-343): the volumetric loop of kernels_vol.hip WITH multiple importance
// sampling.  Differences to the simple variant, stage by stage:
//   k_shade_volmis   * emitter sampling (:127-150 / :215-250) carries the power-heuristic weight against the phase-function / BSDF density (known here) in its shadow record;
//                    * the ray spawned by phase-function / BSDF sampling looks for an emitter (rayIntersectAndLookForEmitter, :370-431): its FIRST hit comes from k_extend and
//                      is judged at the start of the next pass -- an emitter: `Li += throughput * (T_medium Le) * w(samplingPdf, emitterPdf)`; an index-matched boundary:
//                      the search goes on BEHIND it, as a record of its own in the shadow queue (the boundary itself is where the path continues, and `null` surfaces
//                      sample no emitters, so a pass leaves at most one record of each kind per path: the shadow queue holds 2 x cap records per segment here);
//                    * a `null` pass-through (:268-276) is not an iteration of its own: no Russian roulette, `scattered` unchanged, radiance type reset.
//   k_shadow_volmis  kind 0: Scene::evalTransmittance (transmittanceWalk, volume.h), contribution times the stored weight; kind 1 (SR_SEARCH): the emitter search (closest-hit
//                    walk with full intersections through `null` boundaries and media; DirectSamplingRecord::setQuery keeps the LAST segment's length as `dist`, records.inl:170-178).
// The state word (VS_*), the shadow record (SR_*) and everything this file shares with kernels_vol.hip: volume.h; st2 = the sampling density.
// The emitter-search record: shO = the point on the boundary | SR_SEARCH, SR_FACING, SR_DELTA; shD = d | path id; shC = the transmittance so far | the sampling density;
// shT = throughput; shX = the spawning vertex | the cosine a `constant` environment's density needs.
#include "volume.h"

// density of the environment emitter for the direction d as Scene::pdfEmitterDirect reports it: EnvironmentMap::pdfDirect (envmap.cpp:549-560) or
// ConstantBackgroundEmitter::pdfDirect (constant.cpp:219-233: cosine-weighted about the spawning vertex' reference normal -- `cosRef` = dot(d, refN), 2 = none)
template <bool L> DEV float envLumPdf(const DScene &sc, const Tabs<L> &tb, v3 d, float cosRef) {
    const float pdfSA = sc.env_constant ? (cosRef != 2.0f ? MI_INV_PI * maxf(0.0f, cosRef) : MI_INV_FOURPI) : envPdfDirection(sc, mat3(sc.env_to_local, d));
    return pdfSA * (loadEmitter(tb, sc.env_index).weight * sc.emitter_norm);
}

template <bool TEX, bool ENV, bool WRAP>      // forShadeVariant (volume.h)
__global__ __launch_bounds__(WG) void k_shade_volmis(DScene sc, RenderConst rc, Queues q, int buf) {
    extern __shared__ uint32_t s_dyn[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = buf ^ 1;
    const SobolTabLds m32 = stageSobolTables(rc, s_dyn, tid);
    const Tabs<false> tb = globalTabs(sc);
    unsigned long long pathLen = 0;
    __syncthreads();
    forEachChunkOfOwnedSegments(q, buf, lane, wave, [&](uint32_t i, uint32_t n, SegmentWriter &out) __attribute__((always_inline)) {
        bool alive = false, wantShadow = false, wantSearch = false, wantAlpha = false;
        ShadowRec sh, se, al; float4 nrO, nrD, nS1; uint4 nS0; float nS2 = 0, nS3 = 2.0f;
        if (i < n) {
            const uint64_t slot = out.segBase + i;
            float4 ro, rd; loadRayWithInterval(q, buf, slot, ro, rd); const float4 hr = q.hit[slot]; const uint4 s0 = q.st0[buf][slot]; const float4 s1 = loadThroughputEta(q, buf, slot); const float prevPdf = q.st2[buf][slot]; const float prevCos = (ENV && sc.env_constant) ? q.st3[buf][slot] : 2.0f;
            SamplerState ss; uint32_t pid; int depth, medium; v3 T; float eta; unpackPathState(s0, s1, pid, ss, depth, medium, T, eta);
            uint32_t fl = s0.w;
            const v3 o = V(ro.x, ro.y, ro.z), d = V(rd.x, rd.y, rd.z);
            const uint32_t prim = __float_as_uint(hr.w); const float tHit = prim == 0xFFFFFFFFu ? INFINITY : hr.x;
            v3 add = V(0, 0, 0); bool haveAdd = false;
            MediumD md; if (medium >= 0) md = sc.media[medium];
            Hit h; bool haveHit = false; const int inst = (q.hitInst && prim != 0xFFFFFFFFu) ? q.hitInst[slot] : -1;
            auto fill = [&]() {
                if (haveHit) return; haveHit = true;
                fillHitAny<false, true>(sc, tb, inst, o, d, hr.x, hr.y, hr.z, prim, h);
            };
            do {
                // ---- rayIntersectAndLookForEmitter, first intersection (volpath.cpp:370-431) for the ray the previous pass sampled
                if ((fl & VS_SEARCH) && prim != 0xFFFFFFFFu) {
                    const v3 segT = medium >= 0 ? mediumTransmittance(md, 0.0f, tHit) : V(1, 1, 1);
                    fill();
                    const int maxInteractions = rc.max_depth - depth;           // m_maxDepth - rRec.depth - 1 at the spawning vertex (depth has advanced by one since)
                    const MaterialD hm = loadMaterial(tb, h.material); const bool isNull = surfaceHasNull(tb, hm);
                    if (h.emitter >= 0) {                                        // an emitter (also one behind a `null` BSDF, :388-390)
                        const v3 value = segT * emitterEval(tb, h.emitter, h.ns, -d);
                        if (!isZero(value)) {
                            const float lumPdf = (fl & VS_DELTA) ? 0.0f : pdfEmitterDirect<true>(sc, tb, h.emitter, o, d, h.ns, hr.x, (fl & VS_FACING) != 0);
                            add = (T * value) * miWeight(prevPdf, lumPdf); haveAdd = true;
                        }
                    } else if (isNull && maxInteractions != 0 && !isZero(segT)) {   // the search continues behind the boundary: a record for k_shadow_volmis
                        const uint32_t pm = sc.prim_media ? sc.prim_media[prim] : 0u;
                        const int m2 = pm ? targetMedium(pm, h.ng, d) : medium;
                        const v3 p = o + d * hr.x;                              // ray.o = ray(its->t)
                        wantSearch = true;
                        se.o = make_float4(p.x, p.y, p.z, __uint_as_float(recordBits(m2, maxInteractions, SR_SEARCH | ((fl & VS_FACING) ? SR_FACING : 0u) | ((fl & VS_DELTA) ? SR_DELTA : 0u))));
                        const v3 segN = segT * surfaceNullEval(sc, tb, hm, o, d, hr.x, prim, hr.y, hr.z, inst, -dot(d, h.ns), false);      // wo = shFrame.toLocal(ray.d): cosTheta(wi) = -dot(d, ns) (volpath.cpp:399-402)
                        se.d = make_float4(d.x, d.y, d.z, __uint_as_float(pid)); se.c = make_float4(segN.x, segN.y, segN.z, prevPdf);
                        se.t = make_float4(T.x, T.y, T.z, 0.0f); se.x = make_float4(o.x, o.y, o.z, prevCos);     // dRec.ref = the spawning vertex (+ the cosine a `constant` environment's density needs)
                    }
                }
                if (ENV && (fl & VS_SEARCH) && prim == 0xFFFFFFFFu && medium < 0) {      // :421-426: the ray left the scene -> the environment map (inside a medium the unbounded segment has zero transmittance)
                    float nearT, farT;
                    if (bsphereIntersect(sc, o, d, nearT, farT) && !(nearT > 0) && !(farT < 0)) {        // EnvironmentMap::fillDirectSamplingRecord (envmap.cpp:362-378)
                        const v3 value = envEval(sc, d);
                        if (!isZero(value)) {
                            const float lumPdf = (fl & VS_DELTA) ? 0.0f : envLumPdf(sc, tb, d, prevCos);
                            add = (T * value) * miWeight(prevPdf, lumPdf); haveAdd = true;
                        }
                    }
                }
                if (depth > 1 && !(fl & VS_SKIPRR) && depth - 1 >= rc.rr_depth && !russianRoulette(T, eta, [&]() { return next1D(ss, rc.sampler, m32); })) { pathLen += (unsigned) depth; break; }
                if (!(depth <= rc.max_depth || rc.max_depth < 0)) { pathLen += (unsigned) depth; break; }
                const bool emitted = (fl & VS_EMITTED) != 0, scattered = (fl & VS_SCATTERED) != 0;
                MediumRec mRec; bool mediumEvent = false;
                if (medium >= 0) mediumEvent = mediumSampleDistance(md, o, d, 0.0f, tHit, [&]() { return next1D(ss, rc.sampler, m32); }, mRec);
                if (depth == 1 && rc.opacity) wantAlpha = sensorRayOpacity(sc, rc, q, tb, slot, pid, o, d, hr, medium, md, al);
                const int interactions = rc.max_depth - depth - 1;
                bool nee = false; v3 nref = V(0, 0, 0), nrefN = V(0, 0, 0); SurfaceBsdf sf; uint32_t pm = 0;
                if (mediumEvent) {
                    if (depth >= rc.max_depth && rc.max_depth != -1) { pathLen += (unsigned) depth; break; }      // :112-113
                    { const float r = 1.0f / mRec.pdfSuccess; T = T * ((ld3(md.sigma_s) * mRec.transmittance) * r); }
                    nee = true; nref = mRec.p;
                } else {
                    if (medium >= 0) { const float r = 1.0f / mRec.pdfFailure; T = T * (mRec.transmittance * r); }
                    if (prim == 0xFFFFFFFFu) {                               // volpath.cpp:181-192
                        if (ENV && emitted && (!rc.hide_emitters || scattered)) {
                            v3 value = T * (depth == 1 ? envEvalSensorRay(sc, rc, m32, ss, d, q.pos[pid]) : envEval(sc, d));
                            if (medium >= 0) value = value * mediumTransmittance(md, ro.w, rd.w);
                            add = haveAdd ? add + value : value; haveAdd = true;
                        }
                        pathLen += (unsigned) depth; break;
                    }
                    fill();
                    if (h.emitter >= 0 && emitted && (!rc.hide_emitters || scattered)) { const v3 e = T * emitterEval(tb, h.emitter, h.ns, -d); add = haveAdd ? add + e : e; haveAdd = true; }
                    if (depth >= rc.max_depth && rc.max_depth != -1) { pathLen += (unsigned) depth; break; }      // :203-204
                    if ((-dot(h.ng, d)) * h.wi.z < 0 && rc.strict_normals) { pathLen += (unsigned) depth; break; }
                    // the surface step (surface.h): material, textured reflectance (only the sensor ray carries differentials), mask, bump / normal map
                    auto diffs = [&](v3 &rxd, v3 &ryd) { const float2 sp = q.pos[pid]; sensorDifferentials(sc, rc, m32, ss.a, ss.b, sp.x, sp.y, d, rxd, ryd); };
                    sf = resolveSurface<false, true, TEX, true, WRAP && TEX, false, WRAP>(sc, tb, h, prim, inst, hr, o, d, depth == 1, diffs);
                    pm = sc.prim_media ? sc.prim_media[prim] : 0u;
                    nee = !(h.flags & 4u); nref = h.p;
                    if (!(h.flags & 2u)) nrefN = h.ns;
                }
                // ---- emitter sampling with the power heuristic (volpath.cpp:127-150 / :215-250)
                if (nee) {
                    float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                    Direct dr; const v3 value = sampleEmitterDirect<ENV, true, false, true>(sc, tb, nref, nrefN, sx, sy, dr);
                    if (dr.pdf != 0) {
                        v3 x; float w; int m2 = medium;
                        if (mediumEvent) { const float ph = phaseEval(md, -d, dr.d); x = V(ph, ph, ph); w = miWeight(dr.pdf, dr.delta ? 0.0f : ph); }      // PhaseFunction::pdf = eval (phase.cpp:21-23)
                        else {
                            const v3 wo = toLocal(h, dr.d);
                            v3 wiQ, woQ; bool rejected; queryFrame<WRAP>(h, sf, wo, wiQ, woQ, rejected);      // bumpmap.cpp:165-180
                            v3 bv = rejected ? V(0, 0, 0) : mxEval<true, WRAP>(sc, tb, sf.bsdf, wiQ, woQ);
                            if (sf.masked) bv = bv * sf.opac;                     // mask.cpp:117-118
                            const bool ok = !isZero(bv) && (!rc.strict_normals || dot(h.ng, dr.d) * wo.z > 0);
                            float bp = 0.0f;
                            if (ok && !dr.delta) { bp = mxPdf<true, WRAP>(sc, tb, sf.bsdf, wiQ, woQ); if (sf.masked) bp *= luminance3(sf.opac); }      // mask.cpp:141-146
                            x = ok ? bv : V(0, 0, 0); w = ok ? miWeight(dr.pdf, bp) : 0.0f;
                            if (pm) m2 = targetMedium(pm, h.ng, dr.d);
                        }
                        wantShadow = true;
                        sh = emitterSampleRecord(nref, m2, interactions, !mediumEvent, dr, value, pid, T, x, w);
                    }
                }
                // ---- the continuation ray
                if (mediumEvent) {                                           // phase-function sampling (volpath.cpp:156-166); its density = its value
                    float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                    const v3 wo = phaseSample(md, -d, sx, sy);
                    nS2 = phaseEval(md, -d, wo);
                    fl = VS_SEARCH | VS_SCATTERED | VS_FACING;              // type = ERadianceNoEmission; refN = 0 -> dot(d, refN) >= 0 holds
                    nS3 = 2.0f;
                    alive = true;
                    nrO = make_float4(mRec.p.x, mRec.p.y, mRec.p.z, 0.0f); nrD = make_float4(wo.x, wo.y, wo.z, INFINITY);
                    break;
                }
                float bPdf = 0, bEta = 1; v3 woL = V(0, 0, 0); bool sampledDelta, sampledNull;
                float sx, sy; next2D(ss, rc.sampler, m32, sx, sy);
                auto drawExtra = [&]() { return next1D(ss, rc.sampler, m32); };
                v3 bw; bool passThrough = false;                            // mask.cpp:174-214 (shade.h)
                if (sf.masked) passThrough = maskChooseLobe(sf.opac, sx);
                if (passThrough) bw = maskPassThrough(h, sf.opac, woL, bPdf, sampledDelta, sampledNull);
                else bw = sampleInQueryFrame<WRAP>(h, sf, [&](v3 wi, v3 &wo) __attribute__((always_inline)) { return mxSample<true, WRAP>(sc, tb, sf.bsdf, wi, sx, sy, drawExtra, wo, bPdf, bEta, sampledDelta, sampledNull); }, woL);      // bumpmap.cpp:218-240
                if (sf.masked && !passThrough) { const float prob = luminance3(sf.opac); bw = V(bw.x * sf.opac.x / prob, bw.y * sf.opac.y / prob, bw.z * sf.opac.z / prob); bPdf *= prob; }
                if (isZero(bw)) { pathLen += (unsigned) depth; break; }
                const v3 wo = toWorld(h, woL);
                if (dot(h.ng, wo) * woL.z <= 0 && rc.strict_normals) { pathLen += (unsigned) depth; break; }
                T = T * bw; eta *= bEta;
                if (pm) medium = targetMedium(pm, h.ng, wo);
                if (sampledNull) fl = (scattered ? VS_SCATTERED : VS_EMITTED) | VS_SKIPRR;           // :268-276: type = scattered ? ERadianceNoEmission : ERadiance; no emitter search; depth++ without the roulette
                else fl = VS_SEARCH | VS_SCATTERED | (sampledDelta ? VS_DELTA : 0u) | (dot(wo, nrefN) >= 0 ? VS_FACING : 0u);
                nS2 = bPdf; nS3 = (h.flags & 2u) ? 2.0f : dot(wo, nrefN);
                alive = true;
                nrO = make_float4(h.p.x, h.p.y, h.p.z, MI_EPSILON); nrD = make_float4(wo.x, wo.y, wo.z, INFINITY);
            } while (false);
            if (alive) packPathState(pid, ss, depth, fl, medium, T, eta, nS0, nS1);
            if (haveAdd) addRadiance(q, pid, add);
        }
        // search / alpha records share the back of the area (never both: the alpha walk belongs to the sensor ray, which searches for nothing); the reference adds the
        // emitter found by the search first, volpath.cpp:166-173 before :127-150 of the next iteration
        const uint64_t wE = out.backRecord(q, wantSearch | wantAlpha), wS = out.frontRecord(wantShadow), wA = out.survivor(alive);
        if (wantSearch) storeShadowRecord(q, wE, se);
        else if (wantAlpha) { q.shO[wE] = al.o; q.shD[wE] = al.d; }
        if (wantShadow) storeShadowRecord(q, wS, sh);
        if (alive) { storeRayWithInterval(q, nb, wA, nrO, nrD); q.st0[nb][wA] = nS0; storeThroughputEta(q, nb, wA, nS1); q.st2[nb][wA] = nS2; if (ENV && sc.env_constant) q.st3[nb][wA] = nS3; }
    });
    waveAddCounter(&q.counters[2], pathLen, lane);
}

template <bool WIDE, bool ENV, bool NX>      // forShadowVariant (volume.h)
__global__ __launch_bounds__(WG) void k_shadow_volmis(DScene sc, Queues q) {
    __shared__ int s_stk[STACK_DEPTH * WG];
    const uint32_t tid = threadIdx.x;
    const Tabs<false> tb = globalTabs(sc);
    unsigned long long shadowRays = 0, normalRays = 0;
    for (uint32_t seg = blockIdx.x; seg < q.n_seg; seg += gridDim.x)
        forEachShadowRecord(q, seg, tid, [&](uint64_t w) __attribute__((always_inline)) {
            const float4 so = q.shO[w], sd = q.shD[w];
            const uint32_t bits = __float_as_uint(so.w), pid = __float_as_uint(sd.w);
            if (bits & SR_SEARCH) {
                // ---- kind 1: rayIntersectAndLookForEmitter behind the first index-matched boundary (volpath.cpp:381-419); interactions = 1 so far
                int medium = recordMedium(bits); const int maxInteractions = recordMaxInteractions(bits);
                v3 o = V(so.x, so.y, so.z); const v3 d = V(sd.x, sd.y, sd.z);
                const float4 c = qShadowContributionWide(q, w); v3 tr = V(c.x, c.y, c.z); int interactions = 1; bool surface = false; Hit h; float t = INFINITY;
                while (true) {
                    float mint, maxt, u = 0, v = 0; uint32_t prim = 0xFFFFFFFFu; int inst = -1; t = INFINITY; surface = false;
                    ++normalRays;                                                    // Scene::rayIntersect(ray, its): a "normal" ray (skdtree.cpp:118)
                    if (clipInterval(sc, o, d, MI_EPSILON, INFINITY, false, mint, maxt)) surface = traverse<false, 3, WIDE>(sc, o, d, mint, maxt, s_stk + tid, t, prim, u, v, inst);
                    if (!surface) t = INFINITY;
                    if (medium >= 0) tr = tr * mediumTransmittance(sc.media[medium], 0.0f, t);
                    if (!surface) break;
                    fillHitAny<false, true>(sc, tb, inst, o, d, t, u, v, prim, h);
                    const MaterialD hm = loadMaterial(tb, h.material);
                    if (interactions == maxInteractions || !(NX ? surfaceHasNull(tb, hm) : materialHasNull(hm.type)) || h.emitter >= 0) break;
                    if (isZero(tr)) { surface = false; break; }
                    const uint32_t pm = sc.prim_media ? sc.prim_media[prim] : 0u;
                    if (pm) medium = targetMedium(pm, h.ng, d);
                    tr = tr * (NX ? surfaceNullEval(sc, tb, hm, o, d, t, prim, u, v, inst, -dot(d, h.ns), false) : materialNullEval(hm, -dot(d, h.ns)));
                    o = o + d * t;
                    if (++interactions > 100) { surface = false; break; }
                }
                if (ENV && !surface && interactions <= 100 && !isZero(tr)) {        // the search left the scene: the environment map, from the ADVANCED origin (volpath.cpp:421-426)
                    float nearT, farT;
                    if (bsphereIntersect(sc, o, d, nearT, farT) && !(nearT > 0) && !(farT < 0)) {
                        const v3 value = tr * envEval(sc, d);
                        if (!isZero(value)) {
                            const float4 tt = q.shT[w];
                            const float lumPdf = (bits & SR_DELTA) ? 0.0f : envLumPdf(sc, tb, d, q.shX[w].w);
                            addRadiance(q, pid, (V(tt.x, tt.y, tt.z) * value) * miWeight(c.w, lumPdf));
                        }
                    }
                }
                if (surface && h.emitter >= 0) {
                    const v3 value = tr * emitterEval(tb, h.emitter, h.ns, -d);
                    if (!isZero(value)) {
                        const float4 tt = q.shT[w], xx = q.shX[w];
                        const float lumPdf = (bits & SR_DELTA) ? 0.0f : pdfEmitterDirect<true>(sc, tb, h.emitter, V(xx.x, xx.y, xx.z), d, h.ns, t, (bits & SR_FACING) != 0);
                        addRadiance(q, pid, (V(tt.x, tt.y, tt.z) * value) * miWeight(c.w, lumPdf));
                    }
                }
                return;
            }
            // ---- kind 0: Scene::evalTransmittance, the contribution times the stored weight
            bool blocked; const v3 tr = transmittanceWalk<WIDE, NX>(sc, tb, s_stk + tid, V(so.x, so.y, so.z), V(sd.x, sd.y, sd.z), bits, shadowRays, blocked);
            addTransmittedSample<true>(q, w, bits, pid, tr, blocked);
        });
    waveAddCounter(&q.counters[1], shadowRays, tid & 63u);
    waveAddCounter(&q.counters[0], normalRays, tid & 63u);
}

extern "C" {
void mi_launch_shade_volmis(const DScene &sc, const RenderConst &rc, const Queues &q, int buf, uint32_t grid, size_t lds, hipStream_t st) {
    forShadeVariant(sc, [&](auto tex, auto env, auto wrap) { launchWithLds(k_shade_volmis<decltype(tex)::value, decltype(env)::value, decltype(wrap)::value>, grid, lds, st, sc, rc, q, buf); });
}
void mi_launch_shadow_volmis(const DScene &sc, const Queues &q, uint32_t grid, hipStream_t st) {
    forShadowVariant(sc, [&](auto wide, auto env, auto nx) { hipLaunchKernelGGL((k_shadow_volmis<decltype(wide)::value, decltype(env)::value, decltype(nx)::value>), dim3(grid), dim3(WG), 0, st, sc, q); });
}
}
