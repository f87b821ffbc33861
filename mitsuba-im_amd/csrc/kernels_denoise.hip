// kernels_denoise.hip -- edge-avoiding a-trous filter guided by the field channels (denoise.h; the definition is mi_denoise_image's comment in include/mi355pt.h).
// Every float operation below is one rounding, in the order of the definition (-ffp-contract=off, IEEE divide and square root, glibc's expf as mi_expf restates it):
// tests/denoise_model.py computes the same bits.
#include "kernels_common.h"
#include "denoise.h"

// ---------------------------------------------------------------------------------------------- prepare
// RENDER: radiance = film layout 2 (k_film_layout: sum x (weight != 0 ? 1 / weight : 0)), guides = field layout 2 (k_field_layout: the same expression on the field film's own weight),
// read from the planes in place.  Image form: interleaved H x W x 3 arrays.  Demodulation: D = A > 1e-3f ? A : 1e-3f (a NaN albedo gives 1e-3f), c0 = C / D.
template <bool RENDER>
__global__ __launch_bounds__(WG) void k_dn_prepare(DenoiseBufs b, DenoiseFilmSrc f, const float *C, const float *N, const float *P, const float *A, float *pprev, int w, int h, int demod) {
    const size_t i = (size_t) blockIdx.x * WG + threadIdx.x;
    if (i >= (size_t) w * h) return;
    float c[3], n[3], p[3], a[3] = {0.0f, 0.0f, 0.0f};
    if (RENDER) {
        const int x = (int) (i % w), y = (int) (i / w);
        const size_t plane = (size_t) f.W * f.H, src = (size_t) (y + f.border) * f.W + (x + f.border);
        const float wgt = f.film[4 * plane + src] + f.spill[4 * plane + src], inv = wgt != 0 ? 1.0f / wgt : 0.0f;
        const float fw = f.ffilm[f.nv * plane + src] + f.fspill[f.nv * plane + src], finv = fw != 0 ? 1.0f / fw : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = (f.film[k * plane + src] + f.spill[k * plane + src]) * inv;
            const size_t kn = (size_t) (3 * f.fN + k) * plane + src, kp = (size_t) (3 * f.fP + k) * plane + src;
            n[k] = (f.ffilm[kn] + f.fspill[kn]) * finv;
            p[k] = (f.ffilm[kp] + f.fspill[kp]) * finv;
            if (demod) { const size_t ka = (size_t) (3 * f.fA + k) * plane + src; a[k] = (f.ffilm[ka] + f.fspill[ka]) * finv; }
            if (pprev) { const size_t kq = (size_t) (3 * f.fQ + k) * plane + src; pprev[i * 3 + k] = (f.ffilm[kq] + f.fspill[kq]) * finv; }      // the temporal stage's Pprev: the prevPosition field, developed like the guides
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { c[k] = C[i * 3 + k]; n[k] = N[i * 3 + k]; p[k] = P[i * 3 + k]; if (demod) a[k] = A[i * 3 + k]; }
    }
    if (demod) {
        float d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { d[k] = a[k] > 1e-3f ? a[k] : 1e-3f; c[k] = c[k] / d[k]; }
        b.dem[i] = make_float4(d[0], d[1], d[2], 0.0f);
    }
    b.col[0][i] = make_float4(c[0], c[1], c[2], 0.0f);
    b.gA[i] = make_float4(n[0], n[1], n[2], p[0]);
    b.gB[i] = make_float2(p[1], p[2]);
}

// ---------------------------------------------------------------------------------------------- bounds (automatic position width)
// The box of the pixels whose three position components are all finite.  Min and max do not depend on the order, so any reduction shape gives the same bits: stage 1
// leaves one box per block, stage 2 reduces them and resolves the width.  No float atomics.
struct DnBox { float lo[3], hi[3]; };
DEV void dnBoxJoin(DnBox &a, const DnBox &o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.lo[k] = o.lo[k] < a.lo[k] ? o.lo[k] : a.lo[k]; a.hi[k] = o.hi[k] > a.hi[k] ? o.hi[k] : a.hi[k]; }
}
DEV DnBox dnBoxReduce(DnBox mine, DnBox *sm) {
    sm[threadIdx.x] = mine; __syncthreads();
    for (int d = WG / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) { DnBox a = sm[threadIdx.x]; dnBoxJoin(a, sm[threadIdx.x + d]); sm[threadIdx.x] = a; }
        __syncthreads();
    }
    return sm[0];
}
__global__ __launch_bounds__(WG) void k_dn_bounds1(DenoiseBufs b, size_t n) {
    __shared__ DnBox sm[WG];
    const float inf = __uint_as_float(0x7f800000u);
    DnBox m; for (int k = 0; k < 3; ++k) { m.lo[k] = inf; m.hi[k] = -inf; }
    for (size_t i = (size_t) blockIdx.x * WG + threadIdx.x; i < n; i += (size_t) gridDim.x * WG) {
        const float4 ga = b.gA[i]; const float2 gb = b.gB[i];
        if (isfinite(ga.w) && isfinite(gb.x) && isfinite(gb.y)) { DnBox o; o.lo[0] = o.hi[0] = ga.w; o.lo[1] = o.hi[1] = gb.x; o.lo[2] = o.hi[2] = gb.y; dnBoxJoin(m, o); }
    }
    m = dnBoxReduce(m, sm);
    if (threadIdx.x == 0) { for (int k = 0; k < 3; ++k) { b.partial[blockIdx.x * 6 + k] = m.lo[k]; b.partial[blockIdx.x * 6 + 3 + k] = m.hi[k]; } }
}
// resolved width = |sigma_position| x sqrtf((d.x d.x + d.y d.y) + d.z d.z); no finite position, or a diagonal of 0: the position term is off (width 0, kp 0)
__global__ __launch_bounds__(WG) void k_dn_bounds2(DenoiseBufs b, uint32_t nBlocks, float absSigma) {
    __shared__ DnBox sm[WG];
    const float inf = __uint_as_float(0x7f800000u);
    DnBox m; for (int k = 0; k < 3; ++k) { m.lo[k] = inf; m.hi[k] = -inf; }
    if (threadIdx.x < nBlocks) for (int k = 0; k < 3; ++k) { m.lo[k] = b.partial[threadIdx.x * 6 + k]; m.hi[k] = b.partial[threadIdx.x * 6 + 3 + k]; }
    m = dnBoxReduce(m, sm);
    if (threadIdx.x == 0) {
        float sigma = 0.0f, kp = 0.0f;
        if (m.lo[0] <= m.hi[0]) {
            const float dx = m.hi[0] - m.lo[0], dy = m.hi[1] - m.lo[1], dz = m.hi[2] - m.lo[2];
            const float diag = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (diag != 0.0f) { sigma = absSigma * diag; kp = 1.0f / (sigma * sigma); }
        }
        b.res[0] = sigma; b.res[1] = kp;
    }
}

// ---------------------------------------------------------------------------------------------- one level
// One thread per pixel, 32 x 8 tiles.  LDS (steps 1 and 2): neighbouring pixels share most of their taps, the tile and its halo of 2 step pixels are staged once --
// (32 + 4 step) x (8 + 4 step) records of 40 B, 25 KB at step 2.  From step 4 on the taps of neighbouring pixels are disjoint: the records are read directly (they stay
// in L2).  Taps outside the image are skipped by their coordinates; halo cells outside the image are never written and never read.
#define MI_DN_LDS_W (MI_DN_TILE_W + 4 * MI_DN_MAX_LDS_STEP)
#define MI_DN_LDS_H (MI_DN_TILE_H + 4 * MI_DN_MAX_LDS_STEP)
template <bool LDS, bool LAST>
__global__ __launch_bounds__(MI_DN_TILE_W * MI_DN_TILE_H) void k_dn_level(const float4 *__restrict__ cin, float4 *__restrict__ cout, const float4 *__restrict__ gA,
                                                                            const float2 *__restrict__ gB, const float4 *__restrict__ dem, float *__restrict__ out, DenoiseLevel L) {
    __shared__ float4 sC[LDS ? MI_DN_LDS_W * MI_DN_LDS_H : 1], sA[LDS ? MI_DN_LDS_W * MI_DN_LDS_H : 1];
    __shared__ float2 sB[LDS ? MI_DN_LDS_W * MI_DN_LDS_H : 1];
    const int s = L.step, w = L.w, h = L.h;
    const int px = (int) blockIdx.x * MI_DN_TILE_W + (int) threadIdx.x, py = (int) blockIdx.y * MI_DN_TILE_H + (int) threadIdx.y;
    const int tw = MI_DN_TILE_W + 4 * s;
    if (LDS) {
        const int th = MI_DN_TILE_H + 4 * s, ox = (int) blockIdx.x * MI_DN_TILE_W - 2 * s, oy = (int) blockIdx.y * MI_DN_TILE_H - 2 * s;
        for (int i = (int) (threadIdx.y * MI_DN_TILE_W + threadIdx.x); i < tw * th; i += MI_DN_TILE_W * MI_DN_TILE_H) {
            const int gx = ox + i % tw, gy = oy + i / tw;
            if (gx >= 0 && gy >= 0 && gx < w && gy < h) { const size_t g = (size_t) gy * w + gx; sC[i] = cin[g]; sA[i] = gA[g]; sB[i] = gB[g]; }
        }
        __syncthreads();
    }
    if (px >= w || py >= h) return;
    const size_t p = (size_t) py * w + px;
    const int lp = ((int) threadIdx.y + 2 * s) * tw + (int) threadIdx.x + 2 * s;
    const float4 cp = LDS ? sC[lp] : cin[p], ap = LDS ? sA[lp] : gA[p]; const float2 bp = LDS ? sB[lp] : gB[p];
    const float kc = L.kc, kn = L.kn, kp = L.res ? L.res[1] : L.kp;
    const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int y = py + s * dy;
        if (y < 0 || y >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int x = px + s * dx;
            if (x < 0 || x >= w) continue;
            float4 cq, aq; float2 bq;
            if (LDS) { const int lq = lp + (s * dy) * tw + s * dx; cq = sC[lq]; aq = sA[lq]; bq = sB[lq]; }
            else { const size_t q = (size_t) y * w + x; cq = cin[q]; aq = gA[q]; bq = gB[q]; }
            const float cx = cp.x - cq.x, cy = cp.y - cq.y, cz = cp.z - cq.z;
            const float nx = ap.x - aq.x, ny = ap.y - aq.y, nz = ap.z - aq.z;
            const float qx = ap.w - aq.w, qy = bp.x - bq.x, qz = bp.y - bq.y;
            const float d2c = (cx * cx + cy * cy) + cz * cz, d2n = (nx * nx + ny * ny) + nz * nz, d2p = (qx * qx + qy * qy) + qz * qz;
            const float e = -((d2c * kc + d2n * kn) + d2p * kp);
            if (!(e >= -80.0f)) continue;              // a NaN fails the comparison: this drops every non-finite colour or guide
            const float wt = (hk[dy + 2] * hk[dx + 2]) * mi_expf(e);
            if (wt == 0.0f) continue;
            sw += wt; sr += wt * cq.x; sg += wt * cq.y; sb += wt * cq.z;
        }
    }
    float r = cp.x, g = cp.y, bl = cp.z;
    if (sw > 0.0f) { r = sr / sw; g = sg / sw; bl = sb / sw; }
    if (LAST) {
        if (L.demod) { const float4 d = dem[p]; r = r * d.x; g = g * d.y; bl = bl * d.z; }
        out[p * 3] = r; out[p * 3 + 1] = g; out[p * 3 + 2] = bl;
    } else cout[p] = make_float4(r, g, bl, 0.0f);
}

extern "C" {
// pprev (H x W x 3, may be null): receives field f.fQ of the field film, developed
void mi_launch_dn_prepare_render(const DenoiseBufs &b, const DenoiseFilmSrc &f, float *pprev, int w, int h, int demod, hipStream_t st) {
    const size_t n = (size_t) w * h;
    hipLaunchKernelGGL(k_dn_prepare<true>, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, b, f, nullptr, nullptr, nullptr, nullptr, pprev, w, h, demod);
}
void mi_launch_dn_prepare_image(const DenoiseBufs &b, const float *C, const float *N, const float *P, const float *A, int w, int h, int demod, hipStream_t st) {
    const size_t n = (size_t) w * h;
    hipLaunchKernelGGL(k_dn_prepare<false>, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, b, DenoiseFilmSrc{}, C, N, P, A, nullptr, w, h, demod);
}
// leaves res[0] = the resolved width (0: position term off) and res[1] = kp
void mi_launch_dn_bounds(const DenoiseBufs &b, size_t n, float absSigma, hipStream_t st) {
    const uint32_t nb = (uint32_t) std::min<size_t>(MI_DN_BOUNDS_BLOCKS, (n + WG - 1) / WG);
    hipLaunchKernelGGL(k_dn_bounds1, dim3(nb), dim3(WG), 0, st, b, n);
    hipLaunchKernelGGL(k_dn_bounds2, dim3(1), dim3(WG), 0, st, b, nb, absSigma);
}
// level with colour buffer `from` -> the other one, or -> out (H x W x 3) when `last`
void mi_launch_dn_level(const DenoiseBufs &b, int from, const DenoiseLevel &L, bool last, float *out, hipStream_t st) {
    const dim3 grid((unsigned) ((L.w + MI_DN_TILE_W - 1) / MI_DN_TILE_W), (unsigned) ((L.h + MI_DN_TILE_H - 1) / MI_DN_TILE_H)), block(MI_DN_TILE_W, MI_DN_TILE_H);
    const bool lds = L.step <= MI_DN_MAX_LDS_STEP;
    const float4 *cin = b.col[from]; float4 *cout = b.col[from ^ 1];
    if (lds && last) hipLaunchKernelGGL((k_dn_level<true, true>), grid, block, 0, st, cin, cout, b.gA, b.gB, b.dem, out, L);
    else if (lds) hipLaunchKernelGGL((k_dn_level<true, false>), grid, block, 0, st, cin, cout, b.gA, b.gB, b.dem, out, L);
    else if (last) hipLaunchKernelGGL((k_dn_level<false, true>), grid, block, 0, st, cin, cout, b.gA, b.gB, b.dem, out, L);
    else hipLaunchKernelGGL((k_dn_level<false, false>), grid, block, 0, st, cin, cout, b.gA, b.gB, b.dem, out, L);
}
}
