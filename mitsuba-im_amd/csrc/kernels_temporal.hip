// kernels_temporal.hip -- temporal accumulation by reprojecting the previous frame (temporal.h; the definition is mi_denoise_image_temporal's comment in
// include/mi355pt.h).  Every float operation below is one rounding, in the order of the definition (-ffp-contract=off, IEEE divide): tests/temporal_model.py
// computes the same bits.
#include "kernels_common.h"
#include "temporal.h"

// One thread per pixel.  The four taps are data dependent (no LDS staging, no atomics); a thread reads and writes only its own entry of col[0] and of the new
// history set, and only reads the old set.  Every tap address is formed after its bounds test; fx / fy become integers only after the range test, which a NaN fails.
__global__ __launch_bounds__(WG) void k_tp_accumulate(DenoiseBufs b, TemporalSet prev, TemporalSet next, TemporalFrame F) {
    const size_t i = (size_t) blockIdx.x * WG + threadIdx.x;
    const int w = F.w, h = F.h;
    if (i >= (size_t) w * h) return;
    const float tp = F.res ? F.res[0] : F.tp;
    if (i == 0) F.tpOut[0] = tp;
    const float4 c0 = b.col[0][i], ga = b.gA[i]; const float2 gb = b.gB[i];
    float qx = ga.w, qy = gb.x, qz = gb.y;
    if (F.pprev) { qx = F.pprev[i * 3]; qy = F.pprev[i * 3 + 1]; qz = F.pprev[i * 3 + 2]; }
    const bool finite = isfinite(c0.x) && isfinite(c0.y) && isfinite(c0.z) && isfinite(ga.x) && isfinite(ga.y) && isfinite(ga.z) && isfinite(ga.w) && isfinite(gb.x) &&
                        isfinite(gb.y) && isfinite(qx) && isfinite(qy) && isfinite(qz);
    float ar = c0.x, ag = c0.y, ab = c0.z, n = finite ? 1.0f : 0.0f;
    if (finite && F.hasHistory) {
        const float *M = F.Mh;
        const float X = ((M[0] * qx + M[1] * qy) + M[2] * qz) + M[3], Y = ((M[4] * qx + M[5] * qy) + M[6] * qz) + M[7], Wc = ((M[8] * qx + M[9] * qy) + M[10] * qz) + M[11];
        if (Wc > 0.0f) {
            const float fx = X / Wc - 0.5f, fy = Y / Wc - 0.5f;
            if (fx > -1.0f && fx < (float) w && fy > -1.0f && fy < (float) h) {
                const float xf = floorf(fx), yf = floorf(fy), tx = fx - xf, ty = fy - yf;
                const int x0 = (int) xf, y0 = (int) yf;      // -1 .. w - 1, -1 .. h - 1
                const float tp2 = tp * tp;
                float sw = 0.0f, sn = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int y = y0 + j;
                    if (y < 0 || y >= h) continue;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int x = x0 + k;
                        if (x < 0 || x >= w) continue;
                        const float bw = (k ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        if (!(bw > 0.0f)) continue;
                        const size_t t = (size_t) y * w + x;
                        const float4 hc = prev.c[t];
                        if (!(hc.w > 0.0f)) continue;
                        const float4 ha = prev.gA[t]; const float2 hb = prev.gB[t];
                        const float ex = qx - ha.w, ey = qy - hb.x, ez = qz - hb.y;
                        const float d2 = (ex * ex + ey * ey) + ez * ez;
                        if (!(d2 <= tp2)) continue;
                        const float dn = (ga.x * ha.x + ga.y * ha.y) + ga.z * ha.z;
                        if (!(dn >= F.minNormalDot)) continue;
                        sw += bw; sn += bw * hc.w; sr += bw * hc.x; sg += bw * hc.y; sb += bw * hc.z;
                    }
                }
                if (sw > 0.0f) {
                    const float hr = sr / sw, hg = sg / sw, hbl = sb / sw, nh = sn / sw;
                    const float n1 = nh + 1.0f, nn = n1 < F.maxHistory ? n1 : F.maxHistory, alpha = 1.0f / nn;
                    ar = hr + (c0.x - hr) * alpha; ag = hg + (c0.y - hg) * alpha; ab = hbl + (c0.z - hbl) * alpha; n = nn;
                }
            }
        }
    }
    b.col[0][i] = make_float4(ar, ag, ab, 0.0f);
    next.c[i] = make_float4(ar, ag, ab, n); next.gA[i] = ga; next.gB[i] = gb;
}

// iterations = 0: the accumulated colour, modulated again
__global__ __launch_bounds__(WG) void k_tp_output(DenoiseBufs b, float *out, size_t n, int demod) {
    const size_t i = (size_t) blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const float4 c = b.col[0][i];
    float r = c.x, g = c.y, bl = c.z;
    if (demod) { const float4 d = b.dem[i]; r = r * d.x; g = g * d.y; bl = bl * d.z; }
    out[i * 3] = r; out[i * 3 + 1] = g; out[i * 3 + 2] = bl;
}

extern "C" {
void mi_launch_tp_accumulate(const DenoiseBufs &b, const TemporalSet &prev, const TemporalSet &next, const TemporalFrame &F, hipStream_t st) {
    const size_t n = (size_t) F.w * F.h;
    hipLaunchKernelGGL(k_tp_accumulate, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, b, prev, next, F);
}
void mi_launch_tp_output(const DenoiseBufs &b, float *out, size_t n, int demod, hipStream_t st) {
    hipLaunchKernelGGL(k_tp_output, dim3((unsigned) ((n + WG - 1) / WG)), dim3(WG), 0, st, b, out, n, demod);
}
}
