// direct.h -- the direct-illumination integrator: MIDirectIntegrator::Li (src/integrators/direct/direct.cpp:146-309) as wavefront passes over ONE camera-hit queue.
// Instantiated by kernels_direct_*.hip, one translation unit per (RC, ENV) pair like the shade units (shade.h); the existing stages generate / extend / shadow / film
// are reused as they are.  Per batch (api.cpp traceBatchDirect):
//     generate -> extend (buffer 0) -> [env_primary]
//     emitter pass j = 0 .. max(N, 1) - 1:  k_direct<BS = false>  (pass 0 also adds Le / the environment and writes the alpha rule)  -> shadow queue -> k_shadow
//     BSDF pass j = 0 .. M - 1:             k_direct<BS = true>   -> ray / state in buffer 1 -> extend (buffer 1, its own hit array) -> k_direct_hit
// The camera-hit queue (ray, hit, state in buffer 0) stays put for the whole batch: every pass reads it again and resolves hit, material and textures once more --
// the camera ray, the first traversal and the film are paid once for N + M light-transport samples.  Every pass adds into `acc` in launch order, so the float sum
// has the reference's order: Le, emitter terms 0 .. N-1, BSDF terms 0 .. M-1 (direct.cpp:167, :241, :305).
#pragma once
#include "kernels_common.h"
#include "surface.h"
#include "direct_const.h"

// (px, py, sample index) of a path, as k_generate derived them from the path id
DEV void directPathPixel(const Queues &q, const BatchDesc &bd, uint32_t pid, uint32_t &px, uint32_t &py, uint32_t &sidx) {
    if (bd.list) { px = bd.list[(uint64_t) pid * 3]; py = bd.list[(uint64_t) pid * 3 + 1]; sidx = bd.list[(uint64_t) pid * 3 + 2]; return; }
    const uint32_t tw = bd.tile.x1 - bd.tile.x0; const uint32_t plane = pid / bd.n_pix, pl = pid % bd.n_pix;
    px = bd.tile.x0 + pl % tw; py = bd.tile.y0 + (pl / tw) * bd.row_stride; sidx = bd.sample_begin + plane;
}
// The 2-D sample of sub-sample j of one side.  count > 1: element j of the side's array -- Sobol': the point of index look_up(logRes, m * count + j, px, py) at the
// array's two dimensions (sobol.cpp:189-197 with sampler.cpp:83-90), NOT the sample's own index; count <= 1: next2D on the sample's own index.
template <typename P>
DEV void directSample2D(const DScene &sc, const RenderConst &rc, SobolTabT<P> m32, const Queues &q, const BatchDesc &bd, uint32_t pid, uint32_t a, uint32_t b,
                        uint32_t count, uint32_t arrayDim, uint32_t ownDim, uint32_t j, float &x, float &y) {
    if (count > 1u) {
        if (rc.sampler == 1) {
            uint32_t px, py, sidx; directPathPixel(q, bd, pid, px, py, sidx);
            const uint32_t frame = sidx * count + j; uint32_t lo, hi;
            if (rc.sobol_frame && frame < rc.sobol_nframes) {      // the XOR-linear look_up tables of k_generate, built for spp x max(N, M) frames (api.cpp)
                const uint32_t scr = rc.sobol_scramble >> (32u - sc.log_res);
                const uint4 fa = rc.sobol_frame[frame], fb = rc.sobol_px[px ^ scr], fc = rc.sobol_py[py ^ scr];
                lo = fa.x ^ fb.x ^ fc.x; hi = fa.y ^ fb.y ^ fc.y;
            } else { const uint64_t idx = sobolLookUp(sc.sobol_vdc, sc.sobol_vdc_inv, sc.log_res, frame, px, py, rc.sobol_scramble); lo = (uint32_t) idx; hi = (uint32_t) (idx >> 32); }
            x = sobolSampleNib(m32, lo, hi, arrayDim); y = sobolSampleNib(m32, lo, hi, arrayDim + 1u);
        } else { SamplerState t; t.a = a; t.b = b; t.dim = arrayDim - j; next2D(t, 0u, m32, x, y); }
    } else if (rc.sampler == 1) { x = sobolSampleNib(m32, a, b, ownDim); y = sobolSampleNib(m32, a, b, ownDim + 1u); }
    else { SamplerState t; t.a = a; t.b = b; t.dim = ownDim; next2D(t, 0u, m32, x, y); }
}

// One pass over the camera-hit queue.  BS = false: emitter sub-sample dc.pass (direct.cpp:210-245) -> shadow queue; BS = true: BSDF sub-sample dc.pass
// (:251-274) -> ray / state in buffer 1.  Template parameters as k_shade (shade.h); a segment is owned by one wave, compaction is a wave64 ballot.
template <bool RC, bool ENV, bool SMALL, bool AN, bool TEX, bool BS>
__global__ __launch_bounds__(WG) void k_direct(DScene sc, RenderConst rc, DirectConst dc, Queues q, BatchDesc bd) {
    extern __shared__ uint32_t s_dyn[];
    uint32_t *s_nib = s_dyn;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SobolTabLds m32{(lds_u32_ptr) s_nib, rc.nib_count, rc.sobol_scramble};
    const uint32_t nibWords = rc.sampler == 1 ? rc.nib_dims * rc.nib_count * 16u : 4u;
    if (rc.sampler == 1) { for (uint32_t i = tid; i < nibWords; i += WG) s_nib[i] = rc.sobol_nib[i]; }
    Tabs<SMALL> tb; stageTables<SMALL, WG>(sc, s_dyn + ((nibWords + 3u) & ~3u), tid, tb);      // scene tables staged in LDS, the layout of k_shade
    unsigned long long shadowRays = 0;
    __syncthreads();                                         // tables staged
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool first = !BS && dc.pass == 0u;                 // the launch that adds Le / the environment and writes the alpha rule
    for (uint32_t seg = blockIdx.x * (WG / 64) + wave; seg < q.n_seg; seg += gridDim.x * (WG / 64)) {
    const uint32_t n = q.count[0][seg];
    const uint32_t segBase = seg * q.cap;                    // (a pool has fewer than 2^28 slots: queues.h qat)
    uint32_t out = 0;                                        // records written so far (uniform)
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        bool want = false;
        float4 oA, oB, oC; uint4 oS0 = make_uint4(0, 0, 0, 0); float oPdf = 0, oCos = 0;
        if (i < n) {
            const uint32_t slot = segBase + i;
            const auto rd = qRayDirection(q, 0, slot); const float4 hr = qat(q.hit, slot); const uint4 s0 = qat(q.st0[0], slot);
            const uint32_t pid = s0.x; const v3 d = V(rd.x, rd.y, rd.z);
            const uint32_t prim = __float_as_uint(hr.w);
            do {
                if (prim == 0xFFFFFFFFu) {                                         // camera miss: direct.cpp:156-163
                    if (!first) break;
                    const bool addEnv = ENV && !rc.hide_emitters && !sc.env_texture;      // with a MIP pyramid k_env_primary has added the filtered lookup
                    if (addEnv || rc.opacity) {
                        float4 accum = qat(q.acc, pid);
                        if (rc.opacity) accum.w = 0.0f;                                // records.inl:121-137: alpha = 0 on a camera-ray miss
                        if (addEnv) { const v3 e = envEval(sc, d); accum.x += e.x; accum.y += e.y; accum.z += e.z; }
                        qat(q.acc, pid) = accum;
                    }
                    break;
                }
                v3 ro3 = V(0, 0, 0);
                if (AN || TEX) { const auto ro = qRayOrigin(q, 0, slot); ro3 = V(ro.x, ro.y, ro.z); }
                const int inst = (AN && q.hitInst) ? qat(q.hitInst, slot) : -1;
                Hit h;
                fillHitAny<SMALL, AN>(sc, tb, inst, ro3, d, hr.x, hr.y, hr.z, prim, h);
                if (first && h.emitter >= 0 && !rc.hide_emitters) {              // direct.cpp:166-167
                    const v3 le = emitterEval(tb, h.emitter, h.ns, -d);
                    float4 a = qat(q.acc, pid); a.x += le.x; a.y += le.y; a.z += le.z; qat(q.acc, pid) = a;
                }
                if (rc.strict_normals && dot(d, h.ng) * h.wi.z >= 0) break;        // :175-187
                if (!BS && (dc.n_em == 0u || (h.flags & 4u))) break;                // no emitter sub-samples; bsdf->getType() & BSDF::ESmooth (:217) -- the 2-D sample was requested before the test (:210-214)
                // the surface step (surface.h): every pass resolves the camera hit again, so the textured parameters always take the filtered lookup (its.getBSDF(ray) -> computePartials)
                auto diffs = [&](v3 &rxd, v3 &ryd) { const float2 sp = qat(q.pos, pid); sensorDifferentials(sc, rc, m32, s0.y, s0.z, sp.x, sp.y, d, rxd, ryd); };
                const SurfaceBsdf sf = resolveSurface<SMALL, AN, TEX, RC, false, false, false>(sc, tb, h, prim, inst, hr, ro3, d, true, diffs);
                const v3 refN = (h.flags & 2u) ? V(0, 0, 0) : h.ns;               // records.inl:160-164
                if (!BS) {
                    // emitter sub-sample (direct.cpp:220-244); visibility is deferred to the shadow queue
                    float sx, sy; directSample2D(sc, rc, m32, q, bd, pid, s0.y, s0.z, dc.n_em, dc.em_array, dc.em_dim, dc.pass, sx, sy);
                    Direct dr; const v3 value = sampleEmitterDirect<ENV, AN>(sc, tb, h.p, refN, sx, sy, dr);
                    if (dr.pdf == 0) break;
                    ++shadowRays;                                                // scene.cpp:871-875: a shadow ray is cast whenever pdf != 0
                    const v3 wo = toLocal(h, dr.d);
                    v3 bsdfVal = ctEval<RC, false>(sc, tb, -1, sf.bsdf, h.wi, wo);
                    if (RC && sf.masked) bsdfVal = bsdfVal * sf.opac;                  // mask.cpp:124-127
                    if (isZero(value) || isZero(bsdfVal) || (rc.strict_normals && !(dot(h.ng, dr.d) * wo.z > 0))) break;
                    float bp = dr.delta ? 0.0f : ctPdf<RC, false>(sc, tb, -1, sf.bsdf, h.wi, wo);      // emitter->isOnSurface() (:235)
                    if (RC && sf.masked) bp *= luminance3(sf.opac);                    // mask.cpp:141-146
                    const float weight = miWeight(dr.pdf * dc.frac_lum, bp * dc.frac_bsdf) * dc.weight_lum;      // :238-239
                    const v3 c = (value * bsdfVal) * weight;                     // :241
                    want = true;
                    oA = make_float4(h.p.x, h.p.y, h.p.z, dr.dist * (1 - MI_SHADOW_EPSILON));
                    oB = make_float4(dr.d.x, dr.d.y, dr.d.z, __uint_as_float(pid));
                    oC = make_float4(c.x, c.y, c.z, 0.0f);
                } else {
                    // BSDF sub-sample (direct.cpp:258-274); the hit of its ray is judged by k_direct_hit
                    SamplerState ss; ss.a = s0.y; ss.b = s0.z; ss.dim = dc.pass == 0u ? dc.extra_dim : (s0.w & 0xFFu);
                    const uint32_t dim0 = s0.w & 0xFFu;
                    float sx, sy; directSample2D(sc, rc, m32, q, bd, pid, s0.y, s0.z, dc.n_bs, dc.bs_array, dc.bs_dim, dc.pass, sx, sy);
                    float bPdf = 0, bEta = 1; v3 woL = V(0, 0, 0); bool sampledDelta, sampledNull; v3 bw;
                    bool passThrough = false;                                    // mask.cpp:196-208
                    if (RC && sf.masked) passThrough = maskChooseLobe(sf.opac, sx);
                    if (RC && passThrough) bw = maskPassThrough(h, sf.opac, woL, bPdf, sampledDelta, sampledNull);
                    else {
                        // bRec.sampler->next1D() inside BSDF::sample (EUsesSampler): the sample's RUNNING dimension, one draw after another over the sub-samples (sobol.cpp:218-228)
                        auto drawExtra = [&]() { if (rc.sampler == 1 && ss.dim >= 5u && ss.dim < dc.array_end) ss.dim = dc.array_end; return next1D(ss, rc.sampler, m32); };
                        bw = ctSample<RC, false>(sc, tb, -1, sf.bsdf, h.wi, sx, sy, drawExtra, woL, bPdf, bEta, sampledDelta, sampledNull);
                        if (RC && sf.masked) { const float prob = luminance3(sf.opac); bw = V(bw.x * sf.opac.x / prob, bw.y * sf.opac.y / prob, bw.z * sf.opac.z / prob); bPdf *= prob; }
                    }
                    if (ss.dim != dim0) qat(q.st0[0], slot) = make_uint4(s0.x, s0.y, s0.z, (s0.w & ~0xFFu) | (ss.dim & 0xFFu));      // the running dimension of the next sub-sample
                    const v3 wo = toWorld(h, woL);
                    if (isZero(bw) || (rc.strict_normals && dot(h.ng, wo) * woL.z <= 0)) break;      // :264-271
                    want = true;
                    oA = make_float4(h.p.x, h.p.y, h.p.z, MI_EPSILON);
                    oB = make_float4(wo.x, wo.y, wo.z, INFINITY);
                    const float cosRef = dot(wo, refN);
                    oCos = (h.flags & 2u) ? 2.0f : cosRef;
                    oS0 = make_uint4(pid, s0.y, s0.z, (2u << 8) | ((cosRef >= 0 ? 1u : 0u) << 16) | ((RC && sampledDelta) ? (1u << 17) : 0u) | ((RC && sampledNull) ? (1u << 18) : 0u));
                    oC = make_float4(bw.x, bw.y, bw.z, 1.0f); oPdf = bPdf;     // bsdfVal in the throughput slot
                }
            } while (false);
        }
        const unsigned long long m = __ballot(want);
        if (want) {
            const uint32_t o = segBase + out + (uint32_t) __popcll(m & lt);
            if (!BS) { qat(q.shO, o) = oA; qat(q.shD, o) = oB; qSetShadowContribution(q, o, oC.x, oC.y, oC.z); }
            else {      // the BSDF ray's interval is (Epsilon, inf) for every record: the extend launch knows it; no eta (direct.cpp never reads it)
                qSetRayOrigin(q, 1, o, oA.x, oA.y, oA.z); qSetRayDirection(q, 1, o, oB.x, oB.y, oB.z); qat(q.st0[1], o) = oS0; qSetThroughput(q, 1, o, oC.x, oC.y, oC.z); qat(q.st2[1], o) = oPdf;
                if (ENV && sc.env_constant) qat(q.st3[1], o) = oCos;
            }
        }
        out += (uint32_t) __popcll(m);
    }
    if (lane == 0) { if (BS) q.count[1][seg] = out; else q.shCount[seg] = out; }
    }
    if (!BS) {      // counter: wave reduction, one atomic per wave
        for (int off = 32; off > 0; off >>= 1) shadowRays += __shfl_down(shadowRays, off);
        if (lane == 0 && shadowRays) atomicAdd(&q.counters[1], shadowRays);
    }
}

// launch the (AN, TEX) variant of one (RC, ENV, SMALL, BS) combination that fits the scene (the rule of launchShadeVariantSM)
template <bool RC, bool ENV, bool SM, bool BS>
static void launchDirectVariantSM(const DScene &sc, const RenderConst &rc, const DirectConst &dc, const Queues &q, const BatchDesc &bd, uint32_t grid, size_t lds, hipStream_t st) {
    if (sc.ext && sc.n_textures) launchWithLds(k_direct<RC, ENV, SM, true, true, BS>, grid, lds, st, sc, rc, dc, q, bd);
    else if (sc.ext) launchWithLds(k_direct<RC, ENV, SM, true, false, BS>, grid, lds, st, sc, rc, dc, q, bd);
    else launchWithLds(k_direct<RC, ENV, SM, false, false, BS>, grid, lds, st, sc, rc, dc, q, bd);
}
template <bool RC, bool ENV>
static void launchDirectVariant(const DScene &sc, const RenderConst &rc, const DirectConst &dc, const Queues &q, const BatchDesc &bd, int bsdfPass, uint32_t grid, size_t lds, hipStream_t st) {
    if (sc.small_tables != 0) { if (bsdfPass) launchDirectVariantSM<RC, ENV, true, true>(sc, rc, dc, q, bd, grid, lds, st); else launchDirectVariantSM<RC, ENV, true, false>(sc, rc, dc, q, bd, grid, lds, st); }
    else { if (bsdfPass) launchDirectVariantSM<RC, ENV, false, true>(sc, rc, dc, q, bd, grid, lds, st); else launchDirectVariantSM<RC, ENV, false, false>(sc, rc, dc, q, bd, grid, lds, st); }
}
