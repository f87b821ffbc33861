// ao.h -- the ambient-occlusion integrator: AmbientOcclusionIntegrator::Li (src/integrators/direct/ao.cpp:84-125) as wavefront passes over ONE camera-hit queue.
// Instantiated by kernels_ao.hip; the existing stages generate / extend / shadow / film are reused as they are.  Per batch (api.cpp traceBatchAo):
//     generate -> extend (buffer 0) -> [field stage]
//     shading sample j = 0 .. N - 1:  k_ao (pass 0 also writes the value and the alpha of a camera miss)  -> shadow queue -> k_shadow
//     k_ao_resolve (N > 1): acc.xyz *= 1.0f / N on camera hits
// The camera-hit queue (ray, hit, state in buffer 0) stays put for the whole batch, as in direct.h.  A shadow record carries (1, 1, 1): the shadow stage adds it for every
// unoccluded ray, so `acc` counts them (exact in float up to 2^24), and the resolve pass applies `Li /= (Float) N` as the one multiplication it is in the reference.
// No BSDF, emitter, texture or medium is read: the kernel resolves the hit point and the shading frame, nothing else.
#pragma once
#include "direct.h"      // directPathPixel, directSample2D: the sample arrays of sobol.cpp:171-198 / the own request
#include "ao_const.h"

// One pass over the camera-hit queue: shading sample ac.pass (ao.cpp:114-120) -> shadow queue.  A segment is owned by one wave, compaction is a wave64 ballot, the records
// of a segment are written contiguously (the shape of k_direct<BS = false>).  SMALL: the shading records are staged in LDS; AN: analytic shapes / instances / UV tangents.
template <bool SMALL, bool AN>
__global__ __launch_bounds__(WG) void k_ao(DScene sc, RenderConst rc, AoConst ac, Queues q, BatchDesc bd) {
    extern __shared__ uint32_t s_dyn[];
    uint32_t *s_nib = s_dyn;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SobolTabLds m32{(lds_u32_ptr) s_nib, rc.nib_count, rc.sobol_scramble};
    const uint32_t nibWords = rc.sampler == 1 ? rc.nib_dims * rc.nib_count * 16u : 4u;
    if (rc.sampler == 1) { for (uint32_t i = tid; i < nibWords; i += WG) s_nib[i] = rc.sobol_nib[i]; }
    Tabs<SMALL> tb{};      // fillHit / fillHitInstanced read the shading records only
    if (SMALL) {
        uint32_t *pS = s_dyn + ((nibWords + 3u) & ~3u);
        const uint32_t wShade = sc.n_tris * (4u * MI_SHADE_WORDS); const uint32_t *gS = (const uint32_t *) sc.shade;
        for (uint32_t i = tid; i < wShade; i += WG) pS[i] = gS[i];
        tb.shade4 = (typename AS<SMALL>::p4) pS;
    } else tb.shade4 = (typename AS<SMALL>::p4) sc.shade;
    unsigned long long shadowRays = 0;
    __syncthreads();                                         // tables staged
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool first = ac.pass == 0u;                        // the launch that writes the value and the alpha of a camera miss
    for (uint32_t seg = blockIdx.x * (WG / 64) + wave; seg < q.n_seg; seg += gridDim.x * (WG / 64)) {
    const uint32_t n = q.count[0][seg];
    const uint32_t segBase = seg * q.cap;                    // (a pool has fewer than 2^28 slots: queues.h qat)
    uint32_t out = 0;                                        // records written so far (uniform)
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        bool want = false;
        float4 oA, oB;
        if (i < n) {
            const uint32_t slot = segBase + i;
            const auto rd = qRayDirection(q, 0, slot); const float4 hr = qat(q.hit, slot); const uint4 s0 = qat(q.st0[0], slot);
            const uint32_t pid = s0.x; const v3 d = V(rd.x, rd.y, rd.z);
            const uint32_t prim = __float_as_uint(hr.w);
            if (prim == 0xFFFFFFFFu) {                       // camera miss: Spectrum(1.0f) whatever the environment is (ao.cpp:91-95); alpha = 0 under EOpacity (records.inl:121-137)
                if (first) qat(q.acc, pid) = make_float4(1.0f, 1.0f, 1.0f, rc.opacity ? 0.0f : 1.0f);
            } else {
                v3 ro3 = V(0, 0, 0);
                if (AN) { const auto ro = qRayOrigin(q, 0, slot); ro3 = V(ro.x, ro.y, ro.z); }
                const int inst = (AN && q.hitInst) ? qat(q.hitInst, slot) : -1;
                Hit h;
                fillHitAny<SMALL, AN>(sc, tb, inst, ro3, d, hr.x, hr.y, hr.z, prim, h);
                float sx, sy; directSample2D(sc, rc, m32, q, bd, pid, s0.y, s0.z, ac.n, ac.array, ac.own_dim, ac.pass, sx, sy);
                const v3 wo = toWorld(h, cosHemisphere(sx, sy));      // its.toWorld(squareToCosineHemisphere(sample)): the shading frame, no flip, no normal test (:115)
                ++shadowRays;
                want = true;
                oA = make_float4(h.p.x, h.p.y, h.p.z, ac.ray_length);      // Ray(its.p, d, Epsilon, m_rayLength) (:117); the shadow stage's mint is Epsilon
                oB = make_float4(wo.x, wo.y, wo.z, __uint_as_float(pid));
            }
        }
        const unsigned long long m = __ballot(want);
        if (want) {
            const uint32_t o = segBase + out + (uint32_t) __popcll(m & lt);
            qat(q.shO, o) = oA; qat(q.shD, o) = oB; qSetShadowContribution(q, o, 1.0f, 1.0f, 1.0f);
        }
        out += (uint32_t) __popcll(m);
    }
    if (lane == 0) q.shCount[seg] = out;
    }
    for (int off = 32; off > 0; off >>= 1) shadowRays += __shfl_down(shadowRays, off);      // counter: wave reduction, one atomic per wave
    if (lane == 0 && shadowRays) atomicAdd(&q.counters[1], shadowRays);
}

// After the last shadow launch: `Li /= (Float) N` (ao.cpp:122) on the paths whose camera ray hit; a miss keeps its 1.  One thread per slot, workgroups walk segments.
__global__ __launch_bounds__(WG) void k_ao_resolve(Queues q, float recip) {
    for (uint32_t seg = blockIdx.x; seg < q.n_seg; seg += gridDim.x) {
        const uint32_t n = q.count[0][seg]; const uint32_t segBase = seg * q.cap;
        for (uint32_t i = threadIdx.x; i < n; i += WG) {
            const uint32_t slot = segBase + i;
            if (__float_as_uint(qat(q.hit, slot).w) == 0xFFFFFFFFu) continue;
            const uint32_t pid = qat(q.st0[0], slot).x;
            float4 a = qat(q.acc, pid); a.x *= recip; a.y *= recip; a.z *= recip; qat(q.acc, pid) = a;
        }
    }
}
