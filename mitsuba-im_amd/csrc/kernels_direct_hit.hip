// kernels_direct_hit.hip -- the tail of a BSDF sub-sample of the direct integrator (direct.h): what the BSDF ray found (direct.cpp:276-305)
#include "direct.h"

// Reads buffer 1 (ray, state: bsdfVal in the throughput slot, bsdfPdf, delta / null bits, reference-normal cosine) and the hit array the extend stage filled for it.
// A non-emitter hit drops the sub-sample (:279-280); an emitter hit takes Le and pdfEmitterDirect of the hit (:282-283, :298-299); a miss takes the environment
// through fillDirectSamplingRecord (:286-293), skipped under hideEmitters when the sampled component was ENull.  One thread per record, workgroups walk segments.
template <bool ENV, bool AN>
__global__ __launch_bounds__(WG) void k_direct_hit(DScene sc, RenderConst rc, DirectConst dc, Queues q) {
    const Tabs<false> tb = globalTabs(sc);
    for (uint32_t seg = blockIdx.x; seg < q.n_seg; seg += gridDim.x) {
        const uint32_t n = q.count[1][seg]; const uint32_t segBase = seg * q.cap;
        for (uint32_t i = threadIdx.x; i < n; i += WG) {
            const uint32_t slot = segBase + i;
            const auto rd = qRayDirection(q, 1, slot), s1 = qThroughput(q, 1, slot); const float4 hr = qat(q.hit, slot); const uint4 s0 = qat(q.st0[1], slot);
            const float bsdfPdf = qat(q.st2[1], slot);
            const uint32_t pid = s0.x; const v3 d = V(rd.x, rd.y, rd.z), bsdfVal = V(s1.x, s1.y, s1.z);
            const bool facingRef = ((s0.w >> 16) & 1u) != 0, sampledDelta = ((s0.w >> 17) & 1u) != 0, sampledNull = ((s0.w >> 18) & 1u) != 0;
            const uint32_t prim = __float_as_uint(hr.w);
            v3 value; float lumPdf;
            if (prim == 0xFFFFFFFFu) {
                if (!ENV || (rc.hide_emitters && sampledNull)) continue;      // :288
                const auto ro = qRayOrigin(q, 1, slot); float nearT, farT, pdfSA;
                if (sc.env_constant) {      // ConstantBackgroundEmitter::pdfDirect (constant.cpp:219-233): the reference normal of the camera hit
                    value = envEval(sc, d);
                    const float c = qat(q.st3[1], slot); pdfSA = c != 2.0f ? MI_INV_PI * maxf(0.0f, c) : MI_INV_FOURPI;
                } else envEvalAndPdf(sc, d, value, pdfSA);
                if (!(bsphereIntersect(sc, V(ro.x, ro.y, ro.z), d, nearT, farT) && !(nearT > 0) && !(farT < 0))) continue;      // fillDirectSamplingRecord failed (:292-293)
                lumPdf = sampledDelta ? 0.0f : pdfSA * (loadEmitter(tb, sc.env_index).weight * sc.emitter_norm);
            } else {
                v3 ro3 = V(0, 0, 0);
                if (AN) { const auto ro = qRayOrigin(q, 1, slot); ro3 = V(ro.x, ro.y, ro.z); }
                const int inst = (AN && q.hitInst) ? qat(q.hitInst, slot) : -1;
                Hit h;
                fillHitAny<false, AN>(sc, tb, inst, ro3, d, hr.x, hr.y, hr.z, prim, h);
                if (h.emitter < 0) continue;                                   // :279-280
                value = emitterEval(tb, h.emitter, h.ns, -d);
                lumPdf = sampledDelta ? 0.0f : pdfEmitterDirect<AN>(sc, tb, h.emitter, ro3, d, h.ns, h.dist, facingRef);
            }
            const float weight = miWeight(bsdfPdf * dc.frac_bsdf, lumPdf * dc.frac_lum) * dc.weight_bsdf;      // :302-303
            const v3 c = (value * bsdfVal) * weight;                                                          // :305
            float4 a = qat(q.acc, pid); a.x += c.x; a.y += c.y; a.z += c.z; qat(q.acc, pid) = a;
        }
    }
}

extern "C" void mi_launch_direct_hit(const DScene &sc, const RenderConst &rc, const DirectConst &dc, const Queues &q, uint32_t grid, hipStream_t st) {
    const bool env = sc.env_index >= 0;
    if (sc.ext) { if (env) hipLaunchKernelGGL((k_direct_hit<true, true>), dim3(grid), dim3(WG), 0, st, sc, rc, dc, q); else hipLaunchKernelGGL((k_direct_hit<false, true>), dim3(grid), dim3(WG), 0, st, sc, rc, dc, q); }
    else if (env) hipLaunchKernelGGL((k_direct_hit<true, false>), dim3(grid), dim3(WG), 0, st, sc, rc, dc, q);
    else hipLaunchKernelGGL((k_direct_hit<false, false>), dim3(grid), dim3(WG), 0, st, sc, rc, dc, q);
}
