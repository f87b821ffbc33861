// volume.h -- what the two volumetric stage pairs share: kernels_vol.hip (k_shade_vol / k_shadow_vol, `volpath_simple`) and kernels_volmis.hip (k_shade_volmis /
// k_shadow_volmis, `volpath`).  The loop bodies of the two shade kernels restate two different reference files and stay where they are; here is the bookkeeping around them:
//     the state word and the shadow-record bits, the path-state unpack / repack, the Russian roulette, EOpacity on the sensor ray, the emitter-sampling record,
//     the segment's three compactions, the two-pass record loop of the shadow stage, Scene::evalTransmittance with what follows it, and the launchers' flag ladders.
// Every routine is inlined; none adds LDS, a barrier or an atomic to what the stages had with the text pasted into them.
#pragma once
#include <type_traits>
#include "kernels_common.h"
#include "surface.h"
#include "trace.h"

// ---- the state word st0.w: VS_* in pt_types.h, next to RenderConst::state_init, where api.cpp composes the word of a fresh path
// ---- the shadow record.  shO = p1 | these bits; shD = p2 | path id; shC = emitter value BEFORE the division by the emitter-selection probability | that probability;
// shT = throughput; shX = BSDF value (or the phase value in all three channels) | MIS weight (volpath).  An alpha record has shO and shD only; for the emitter search
// (SR_SEARCH, k_shadow_volmis) see kernels_volmis.hip.
#define SR_MEDIUM_MASK 0xFFu           // bits 0..7 medium + 1
#define SR_MAXINT_SHIFT 8              // bits 8..23 maxInteractions (int16)
#define SR_P1_ON_SURFACE (1u << 24)
#define SR_P2_ON_SURFACE (1u << 25)
#define SR_SEARCH (1u << 26)           // kind = emitter search
#define SR_FACING (1u << 27)           // emitter search: facingRef
#define SR_DELTA (1u << 28)            // emitter search: delta sample
#define SR_ALPHA (1u << 29)            // the alpha walk of a sensor ray: the transmittance goes to the accumulator's alpha
struct ShadowRec { float4 o, d, c, t, x; };

DEV uint32_t recordBits(int medium, int maxInteractions, uint32_t flags) { return (uint32_t) (medium + 1) | (((uint32_t) maxInteractions & 0xFFFFu) << SR_MAXINT_SHIFT) | flags; }
DEV int recordMedium(uint32_t bits) { return (int) (bits & SR_MEDIUM_MASK) - 1; }
DEV int recordMaxInteractions(uint32_t bits) { return (int) (int16_t) ((bits >> SR_MAXINT_SHIFT) & 0xFFFFu); }

DEV void addRadiance(const Queues &q, uint32_t pid, v3 li) { float4 a = q.acc[pid]; a.x += li.x; a.y += li.y; a.z += li.z; q.acc[pid] = a; }
DEV void setAlpha(const Queues &q, uint32_t pid, float al) { float4 a = q.acc[pid]; a.w = al; q.acc[pid] = a; }
DEV float alphaOfTransmittance(v3 tr) { return 1 - ((0.0f + tr.x) + tr.y + tr.z) * (1.0f / 3); }
// sum over the wave, one atomic per counter
DEV void waveAddCounter(unsigned long long *counter, unsigned long long v, uint32_t lane) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0 && v) atomicAdd(counter, v);
}

// ---- shade stage
// the Sobol' nibble tables into LDS; the caller's barrier follows
DEV SobolTabLds stageSobolTables(const RenderConst &rc, uint32_t *s_nib, uint32_t tid) {
    if (rc.sampler == 1) { const uint32_t nibWords = rc.nib_dims * rc.nib_count * 16u; for (uint32_t i = tid; i < nibWords; i += WG) s_nib[i] = rc.sobol_nib[i]; }
    return SobolTabLds{(lds_u32_ptr) s_nib, rc.nib_count, rc.sobol_scramble};
}
// The volumetric stages hold a ray as (o | mint), (d | maxt) and the second state word as (throughput | eta) in registers; in the queues these are the 12-byte
// records plus the interval and eta arrays (queues.h) -- both are per path here: a medium vertex starts its ray at mint = 0, a surface vertex at Epsilon
DEV void loadRayWithInterval(const Queues &q, int buf, uint64_t slot, float4 &ro, float4 &rd) {
    const auto o = qRayOrigin(q, buf, (uint32_t) slot), d = qRayDirection(q, buf, (uint32_t) slot); const float2 iv = qRayInterval(q, buf, (uint32_t) slot);
    ro = make_float4(o.x, o.y, o.z, iv.x); rd = make_float4(d.x, d.y, d.z, iv.y);
}
DEV void storeRayWithInterval(const Queues &q, int buf, uint64_t slot, float4 ro, float4 rd) {
    qSetRayOrigin(q, buf, (uint32_t) slot, ro.x, ro.y, ro.z); qSetRayDirection(q, buf, (uint32_t) slot, rd.x, rd.y, rd.z); qSetRayInterval(q, buf, (uint32_t) slot, ro.w, rd.w);
}
DEV float4 loadThroughputEta(const Queues &q, int buf, uint64_t slot) { const auto t = qThroughput(q, buf, (uint32_t) slot); return make_float4(t.x, t.y, t.z, qEta(q, buf, (uint32_t) slot)); }
DEV void storeThroughputEta(const Queues &q, int buf, uint64_t slot, float4 s1) { qSetThroughput(q, buf, (uint32_t) slot, s1.x, s1.y, s1.z); qSetEta(q, buf, (uint32_t) slot, s1.w); }
DEV void unpackPathState(uint4 s0, float4 s1, uint32_t &pid, SamplerState &ss, int &depth, int &medium, v3 &T, float &eta) {
    pid = s0.x; ss.a = s0.y; ss.b = s0.z; ss.dim = s0.w & VS_DIM_MASK;
    depth = (int) ((s0.w >> VS_DEPTH_SHIFT) & 0xFFu); medium = (int) ((s0.w >> VS_MEDIUM_SHIFT) & 0xFFu) - 1;
    T = V(s1.x, s1.y, s1.z); eta = s1.w;
}
// the state of the next iteration: depth + 1, `fl` = the integrator's flag bits
DEV void packPathState(uint32_t pid, const SamplerState &ss, int depth, uint32_t fl, int medium, v3 T, float eta, uint4 &nS0, float4 &nS1) {
    nS0 = make_uint4(pid, ss.a, ss.b, (ss.dim & VS_DIM_MASK) | ((uint32_t) (depth + 1) << VS_DEPTH_SHIFT) | fl | ((uint32_t) (medium + 1) << VS_MEDIUM_SHIFT));
    nS1 = make_float4(T.x, T.y, T.z, eta);
}
// Russian roulette, the tail of the previous iteration (volpath_simple.cpp:278-287, volpath.cpp:326-337); false: the path ends
template <typename R> DEV bool russianRoulette(v3 &T, float eta, R next) {
    const float qq = minf(maxf(maxf(T.x, T.y), T.z) * eta * eta, 0.95f);
    if (next() >= qq) return false;
    const float r = 1.0f / qq; T = T * r;
    return true;
}
// EnvironmentMap::evalEnvironment for the sensor ray, the one that carries differentials
DEV v3 envEvalSensorRay(const DScene &sc, const RenderConst &rc, SobolTabLds m32, const SamplerState &ss, v3 d, float2 sp) {
    if (!sc.env_texture) return envEval(sc, d);
    v3 rxd, ryd; sensorDifferentials(sc, rc, m32, ss.a, ss.b, sp.x, sp.y, d, rxd, ryd);
    return envEvalFiltered(sc, d, rxd, ryd);
}
// EOpacity on the sensor ray (o, d) with the hit record hr, in `medium` (md: its record when medium >= 0).  True: `al` is the alpha record of the walk behind the shape.
DEV bool sensorRayOpacity(const DScene &sc, const RenderConst &rc, const Queues &q, const Tabs<false> &tb, uint64_t slot, uint32_t pid, v3 o, v3 d, float4 hr, int medium, const MediumD &md, ShadowRec &al) {
    const uint32_t prim = __float_as_uint(hr.w);
    if (prim == 0xFFFFFFFFu) {               // records.inl:131-137: a sensor ray that hits nothing -- what the medium in front of the sensor absorbs / scatters, or 0
        float alpha = 0.0f;
        if (medium >= 0) { const v3 p2 = o + d * rc.alpha_dist, dd = p2 - o; alpha = alphaOfTransmittance(mediumTransmittance(md, 0.0f, sqrtf(dot(dd, dd)))); }
        setAlpha(q, pid, alpha);
        return false;
    }
    const uint32_t pmA = sc.prim_media ? sc.prim_media[prim] : 0u;      // records.inl:124-130: a sensor ray that hits a medium-transition shape -- alpha = 1 - the transmittance of what lies behind it
    if (!pmA) return false;
    Hit ha; const int instA = q.hitInst ? q.hitInst[slot] : -1;
    fillHitAny<false, true>(sc, tb, instA, o, d, hr.x, hr.y, hr.z, prim, ha);
    const v3 p2 = o + d * rc.alpha_dist; const int mA = targetMedium(pmA, ha.ng, d);
    al.o = make_float4(ha.p.x, ha.p.y, ha.p.z, __uint_as_float(recordBits(mA, 0x7FFF, SR_P1_ON_SURFACE | SR_ALPHA)));
    al.d = make_float4(p2.x, p2.y, p2.z, __uint_as_float(pid));
    return true;
}
// the record of an emitter sample `dr` (value = its radiance) taken at `nref`: x = the BSDF / phase value, w = the MIS weight (volpath), m2 = the medium the walk starts in
DEV ShadowRec emitterSampleRecord(v3 nref, int m2, int interactions, bool onSurface, const Direct &dr, v3 value, uint32_t pid, v3 T, v3 x, float w) {
    ShadowRec r;
    r.o = make_float4(nref.x, nref.y, nref.z, __uint_as_float(recordBits(m2, interactions, (onSurface ? SR_P1_ON_SURFACE : 0u) | (dr.delta ? 0u : SR_P2_ON_SURFACE))));
    r.d = make_float4(dr.p.x, dr.p.y, dr.p.z, __uint_as_float(pid)); r.c = make_float4(value.x, value.y, value.z, dr.em_pdf);
    r.t = make_float4(T.x, T.y, T.z, 0.0f); r.x = make_float4(x.x, x.y, x.z, w);
    return r;
}
DEV void storeShadowRecord(const Queues &q, uint64_t w, const ShadowRec &r) { q.shO[w] = r.o; q.shD[w] = r.d; qSetShadowContributionWide(q, w, r.c); q.shT[w] = r.t; q.shX[w] = r.x; }

// The shadow queue holds two records per path slot: a pass leaves at most one emitter-sampling record per path, written from the FRONT of the segment's area, and at most
// one alpha walk (or, volpath, one emitter search) written from the BACK; the shadow stage runs the back records first.
DEV uint64_t backRecordSlot(const Queues &q, uint64_t areaBase, uint32_t k) { return areaBase + 2u * q.cap - 1u - k; }
// The three compactions of a segment, which one wave owns (shade.h): each call is a ballot over the whole wave and returns this lane's slot (meaningful where `want`);
// the running offsets are uniform.  No LDS, no barrier, no atomics.
struct SegmentWriter {
    uint64_t segBase, shBase; unsigned long long lt; uint32_t outA, outS, outE;
    DEV SegmentWriter(const Queues &q, uint32_t seg, uint32_t lane) : segBase((uint64_t) seg * q.cap), shBase(segBase * 2u), lt((1ull << lane) - 1ull), outA(0), outS(0), outE(0) {}
    DEV uint64_t backRecord(const Queues &q, bool want) { const unsigned long long m = __ballot(want); const uint64_t w = backRecordSlot(q, shBase, outE + (uint32_t) __popcll(m & lt)); outE += (uint32_t) __popcll(m); return w; }
    DEV uint64_t frontRecord(bool want) { const unsigned long long m = __ballot(want); const uint64_t w = shBase + outS + (uint32_t) __popcll(m & lt); outS += (uint32_t) __popcll(m); return w; }
    DEV uint64_t survivor(bool want) { const unsigned long long m = __ballot(want); const uint64_t w = segBase + outA + (uint32_t) __popcll(m & lt); outA += (uint32_t) __popcll(m); return w; }
    DEV void finish(const Queues &q, int nb, uint32_t seg, uint32_t lane) const { if (lane == 0) { q.count[nb][seg] = outA; q.shCount[seg] = outS | (outE << 16); } }      // (cap <= 65535 in the volumetric modes, api.cpp)
};
// The segments of this wave (a segment is owned by one wave, shade.h), chunk by chunk: body(i, n, out) for every lane, slot i of the segment's n paths in buffer `buf`
// (the lanes with i >= n take part in the compactions only); the counts of buffer buf ^ 1 and of the shadow queue follow each segment.
template <typename F> DEV void forEachChunkOfOwnedSegments(const Queues &q, int buf, uint32_t lane, uint32_t wave, F body) {
    for (uint32_t seg = blockIdx.x * (WG / 64) + wave; seg < q.n_seg; seg += gridDim.x * (WG / 64)) {
        const uint32_t n = q.count[buf][seg];
        SegmentWriter out(q, seg, lane);
        for (uint32_t base = 0; base < n; base += 64) body(base + lane, n, out);
        out.finish(q, buf ^ 1, seg, lane);
    }
}

// ---- shadow stage
// Two passes over the segment's records, a workgroup barrier in between: first the records written from the back of the area, then the emitter-sampling records -- a path
// can own one of each, and its accumulator is a plain read-modify-write.  body(w): the record in slot w.
template <typename F> DEV void forEachShadowRecord(const Queues &q, uint32_t seg, uint32_t tid, F body) {
    const uint32_t cnt = q.shCount[seg], nFront = cnt & 0xFFFFu, nBack = cnt >> 16;
    const uint64_t areaBase = (uint64_t) seg * q.cap * 2u;
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1) __syncthreads();
        const uint32_t n = phase == 0 ? nBack : nFront;
        for (uint32_t i = tid; i < n; i += WG) body(phase == 0 ? backRecordSlot(q, areaBase, i) : areaBase + i);
    }
}
// Scene::evalTransmittance (scene.cpp:650-713) from p1 to p2 for a record with `bits`: through `null` boundaries and media; `blocked`: an occluder or a medium inconsistency
// (zero transmittance).  stk: the lane's traversal stack; every ray counts in `rays`.  NX: ENull lobes behind a wrapper (mask, mixturebsdf with an index-matched child) are
// present: surfaceNullEval instead of the plain records' pass-through value.
template <bool WIDE, bool NX>
DEV v3 transmittanceWalk(const DScene &sc, const Tabs<false> &tb, int *stk, v3 p1, v3 p2, uint32_t bits, unsigned long long &rays, bool &blocked) {
    int medium = recordMedium(bits); const int maxInteractions = recordMaxInteractions(bits); const bool p1OnSurface = (bits & SR_P1_ON_SURFACE) != 0, p2OnSurface = (bits & SR_P2_ON_SURFACE) != 0;
    v3 d = p2 - p1; float remaining = sqrtf(dot(d, d)); { const float r = 1.0f / remaining; d = d * r; }
    const float lengthFactor = p2OnSurface ? (1 - MI_SHADOW_EPSILON) : 1;
    v3 o = p1; float rmint = p1OnSurface ? MI_EPSILON : 0.0f, rmaxt = remaining * lengthFactor;
    v3 tr = V(1, 1, 1); int interactions = 0; blocked = false;
    while (remaining > 0) {
        float mint, maxt, t = INFINITY, u = 0, v = 0; uint32_t prim = 0xFFFFFFFFu; int inst = -1; bool surface = false;
        ++rays;                                                          // skdtree.cpp:152 ++shadowRaysTraced
        if (clipInterval(sc, o, d, rmint, rmaxt, true, mint, maxt)) surface = traverse<false, 3, WIDE>(sc, o, d, mint, maxt, stk, t, prim, u, v, inst);
        if (!surface) t = INFINITY;
        int material = -1; v3 n = V(0, 0, 0);
        if (surface) {
            if (prim >= sc.n_tris) { const AnalyticD &a = sc.analytic[prim - sc.n_tris]; material = a.material; Hit h; fillHitAnalytic(a, o, d, t, u, v, h); n = h.ng; }
            else {                                                       // skdtree.cpp:165-171: n = normalize(cross(p1 - p0, p2 - p0)), NOT flipped towards the shading normal
                AS<false>::p4 rec = tb.shade4 + prim * (uint32_t) MI_SHADE_WORDS; const f4 r0 = rec[0], r1 = rec[1], r2 = rec[2]; material = __float_as_int(r0.w);
                v3 fn = cross(V(r1.x - r0.x, r1.y - r0.y, r1.z - r0.z), V(r2.x - r0.x, r2.y - r0.y, r2.z - r0.z)); const float len = sqrtf(dot(fn, fn));
                if (!isZero(fn)) { const float r = 1.0f / len; fn = fn * r; }
                n = fn;
            }
            if (interactions == maxInteractions || !(NX ? surfaceHasNull(tb, loadMaterial(tb, material)) : materialHasNull(loadMaterial(tb, material).type))) { blocked = true; break; }   // an occluder: zero transmittance
        }
        if (medium >= 0) tr = tr * mediumTransmittance(sc.media[medium], 0.0f, minf(t, remaining));
        if (!surface || isZero(tr)) break;
        tr = tr * (NX ? surfaceNullEval(sc, tb, loadMaterial(tb, material), o, d, t, prim, u, v, inst, -dot(d, n), true) : materialNullEval(loadMaterial(tb, material), -dot(d, n)));      // its.geoFrame = Frame(n): cosTheta(wi) = -dot(d, n)
        const uint32_t pm = sc.prim_media ? sc.prim_media[prim] : 0u;   // `null`: bsdf->eval(bRec, EDiscrete) with typeMask = ENull is 1 (null.cpp:48-50)
        if (pm) {
            if (medium != targetMedium(pm, n, -d)) { blocked = true; break; }      // medium inconsistency (scene.cpp:689-692)
            medium = targetMedium(pm, n, d);
        }
        if (++interactions > 100) break;
        o = o + d * t; remaining -= t; rmaxt = remaining * lengthFactor; rmint = MI_EPSILON;
    }
    return tr;
}
// What follows the walk of the record in slot w: the alpha of a sensor ray's alpha record (records.inl:128-130), or the deferred
// `Li += throughput * (value * transmittance / emitterPdf) * (BSDF | phase) value` (scene.cpp:897-899), WEIGHTED: times the MIS weight in shX.w, nothing where that is 0
// (phaseVal != 0 / !bsdfVal.isZero(), volpath.cpp:139, :232)
template <bool WEIGHTED>
DEV void addTransmittedSample(const Queues &q, uint64_t w, uint32_t bits, uint32_t pid, v3 tr, bool blocked) {
    if (bits & SR_ALPHA) { setAlpha(q, pid, alphaOfTransmittance(blocked ? V(0, 0, 0) : tr)); return; }
    if (blocked) return;
    const float4 c = qShadowContributionWide(q, w), tt = q.shT[w], xx = q.shX[w];
    const float r = 1.0f / c.w;
    const v3 value = V(c.x, c.y, c.z) * (tr * r);                       // value *= evalTransmittance(...) / emPdf
    if (isZero(value) || (WEIGHTED && xx.w == 0.0f)) return;
    const v3 li = (V(tt.x, tt.y, tt.z) * value) * V(xx.x, xx.y, xx.z);
    addRadiance(q, pid, WEIGHTED ? li * xx.w : li);
}

// ---- launchers: run-time flags -> template booleans, handed to f as std::true_type / std::false_type
// shade: TEX textures bound to materials; ENV an environment map among the emitters; WRAP mixturebsdf / bumpmap / normalmap records present (with TEX)
template <typename F> static inline void withBool(bool b, F f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <typename F> static inline void forShadeVariant(const DScene &sc, F f) {
    const std::true_type y; const std::false_type n;
    withBool(sc.env_index >= 0, [&](auto env) { if (sc.has_adapters & 1u) f(y, env, y); else if (sc.n_textures) f(y, env, n); else f(n, env, n); });
}
// shadow: WIDE the wide BVH; ENV as above; NX as transmittanceWalk's
template <typename F> static inline void forShadowVariant(const DScene &sc, F f) {
    withBool(sc.bvh_wide, [&](auto wide) { withBool(sc.env_index >= 0, [&](auto env) { withBool((sc.has_adapters & 2u) != 0, [&](auto nx) { f(wide, env, nx); }); }); });
}
