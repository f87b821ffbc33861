// denoise.h -- edge-avoiding a-trous filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) with albedo demodulation, guided by the field channels; shared by api.cpp and
// kernels_denoise.hip.  The normative definition is the comment of mi_denoise_image in include/mi355pt.h: float32, one rounding per operation, so the device result equals
// a NumPy model bit for bit (tests/denoise_model.py).
//
//   k_dn_prepare   one thread per pixel: radiance and guides (render form: developed from the film planes in place, as layout 2 develops them; image form: interleaved
//                  arrays), demodulation, and the packed records below
//   k_dn_bounds1/2 two-stage min / max of the finite positions -> resolved position width and kp (automatic width only)
//   k_dn_level     one thread per pixel, 32 x 8 tiles; steps 1 and 2 stage tile + halo in LDS, steps >= 4 read the records directly; the last level multiplies by D and
//                  writes H x W x 3
//
// Records (SoA, one entry per pixel, row-major over the crop window): colour float4 (r, g, b, -) in two buffers that ping-pong between the levels; guides float4
// (N.x, N.y, N.z, P.x) + float2 (P.y, P.z), written once; float4 (D.x, D.y, D.z, -), read by the last level only.  A tap costs one dwordx4 + one dwordx4 + one dwordx2.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define MI_DN_TILE_W 32
#define MI_DN_TILE_H 8
#define MI_DN_MAX_LDS_STEP 2                 // steps 1 and 2 go through LDS
#define MI_DN_BOUNDS_BLOCKS 256u             // partial boxes of stage 1 (at the most)
#define MI_DN_BYTES_PER_PIXEL 72u            // 2 x 16 colour + 16 + 8 guides + 16 divisor
#define MI_DN_TAIL_FLOATS (MI_DN_BOUNDS_BLOCKS * 6u + 2u)

struct DenoiseBufs {
    float4 *col[2];
    float4 *gA; float2 *gB;
    float4 *dem;
    float *partial;     // stage 1: block b's box at [6 b .. 6 b + 5] = min.xyz, max.xyz (min > max: no finite position in the block)
    float *res;         // stage 2: res[0] = resolved position width (0 = term off), res[1] = kp
};
// render form: where prepare finds radiance and guides.  Planes are (H + 2 border) x (W + 2 border); field f's values are planes 3 f .. 3 f + 2 of the field film, its weight plane nv
struct DenoiseFilmSrc {
    const float *film, *spill, *ffilm, *fspill;
    int W, H, border, nv;
    int fN, fP, fA;     // field list indices of shNormal, position, albedo (fA < 0: none)
    int fQ;             // ... of prevPosition (< 0: none): the temporal stage's Pprev, developed into a buffer of its own when prepare is given one
};
struct DenoiseLevel { int w, h, step; float kc, kn, kp; const float *res; int demod; };   // res != null: kp = res[1]
