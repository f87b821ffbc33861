// kernels_units.hip -- unit-level parity entry points over the BSDF and texture routines of pt_device.h (mi_debug_bsdf, mi_debug_texture): one call of the
// routine per thread on caller-supplied inputs, so that directions, sample values and footprints a camera-driven path almost never produces can be compared with the
// oracle's orc_bsdf_sample_ex / orc_bsdf_eval / orc_texture_eval.  Nothing here restates a routine: the kernels call what the shade stage calls.
#include "kernels_common.h"

// in9 = wi xyz, wo xyz, u, v, extra.  The record is resolved as the shade stage resolves an untextured hit (shade.h: a coating / roughcoating record becomes `coat`,
// its nested record `bsdf`; mask, bumpmap, normalmap and textured records are refused on the host), then queried through ctSample / ctEval / ctPdf<true, true, false>:
// every BSDF type, every wrapper, tables in global memory -- the widest instantiation the shade stage has.
// mode 0 (sample): out12 = weight rgb, pdf, wo xyz, eta, delta, null, extra drawn, 0;  mode 1 (eval + pdf): out12 = value rgb, pdf, 0...
__global__ __launch_bounds__(WG) void k_debug_bsdf(DScene sc, int material, int mode, const float *in, uint64_t n, float *out) {
    const uint64_t i = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    Tabs<false> tb; tb.shade4 = (AS<false>::p4) sc.shade; tb.materials4 = (AS<false>::p4) sc.materials; tb.emitters4 = (AS<false>::p4) sc.emitters; tb.emitter_cdf = sc.emitter_cdf; tb.area_cdf = sc.area_cdf;
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

extern "C" {
void mi_launch_debug_bsdf(const DScene &sc, int material, int mode, const float *in, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_bsdf, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, material, mode, in, n, out);
}
void mi_launch_debug_texture(const DScene &sc, uint32_t texture, const float *uv, const float *partials, uint64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_debug_texture, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, sc, texture, uv, partials, n, out);
}
}
