// temporal.h -- temporal accumulation in front of the a-trous levels (denoise.h): the previous frame's accumulated colour is reprojected through the projection of
// the frame that wrote it and blended with the current colour; shared by api.cpp and kernels_temporal.hip.  The normative definition is the comment of
// mi_denoise_image_temporal in include/mi355pt.h: float32, one rounding per operation, so the device result equals a NumPy model bit for bit (tests/temporal_model.py).
//
//   k_tp_accumulate  one thread per pixel, after k_dn_prepare: reads col[0], gA, gB of DenoiseBufs, gathers up to four records of the old history, rewrites its own
//                    entry of col[0] and writes the new history record
//   k_tp_output      iterations = 0 only: H x W x 3 = col[0] x D
//
// History records use the packed layout of denoise.h: float4 (a.r, a.g, a.b, n) + float4 (N.x, N.y, N.z, P.x) + float2 (P.y, P.z), 40 B per pixel, in two sets that
// ping-pong between frames; one allocation holds both and a tail of MI_TP_TAIL_FLOATS floats (tail[0] = the temporal tolerance the last frame resolved).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "denoise.h"

#define MI_TP_BYTES_PER_PIXEL 80u            // 2 sets x (16 colour + count, 16 + 8 guides)
#define MI_TP_TAIL_FLOATS 4u

struct TemporalSet { float4 *c; float4 *gA; float2 *gB; };
struct TemporalFrame {
    int w, h;
    int hasHistory;             // 0: the history holds no frame, every pixel is alone
    float Mh[12];               // the projection of the frame that wrote `prev`
    float maxHistory, minNormalDot;
    float tp;                   // the tolerance when res == null
    const float *res;           // != null: tp = res[0] (mi_launch_dn_bounds ran with the temporal width)
    const float *pprev;         // H x W x 3, or null: Pprev = P
    float *tpOut;               // the tolerance used, for the host
};
