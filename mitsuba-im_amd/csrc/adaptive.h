// adaptive.h -- per-pixel error control over `path` / `volpath*` (the reference's `adaptive` integrator, src/integrators/misc/adaptive.cpp:202-319), shared by api.cpp
// and kernels_adaptive.hip.  The stages that trace a sample are untouched: a round of R consecutive sample indices of every ACTIVE pixel runs through the explicit
// (px, py, sampleIndex) list of k_generate, and the kernels here sit behind them.
//
//   k_adapt_list        the triple list of a batch: path = plane x nAct + a (plane-major, so that neighbouring threads of k_adapt_accumulate read neighbouring acc / pos)
//   k_adapt_accumulate  one thread per active pixel walks its samples of the batch IN SAMPLE ORDER: ImageBlock::put into the pixel's own footprint rows, Welford update,
//                       stopping rule; at the stop the footprint goes to the film scaled by 1.0f / n and n into the count map
//   k_adapt_count / k_adapt_compact   the next active list: a stable ballot compaction over wave-owned ranges (one uniform offset per wave, no global atomics)
//
// The independent sampler is a counter stream keyed by (pixel, sample index) and a pixel's state is owned by one thread in sample order, so the count map does not depend
// on the round length, the batch size or the pool shape, and equals a sequential float32 model bit for bit (-ffp-contract=off, IEEE divide and square root).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define MI_ADAPT_RANGES 1024u      // wave-owned ranges of the compaction (at the most)

struct AdaptArgs {
    float *fp;                  // footprints: value k of cell c of film pixel p at [(c * 5 + k) * n_pix + p], c = (dy + hb) * (2 hb + 1) + (dx + hb)
    float2 *ms;                 // per film pixel: mean, meanSqr of the sample luminances so far
    uint32_t *n;                // per film pixel: samples taken so far
    uint32_t *counts;           // per film pixel: samples of the FINISHED pixel (0 = not rendered / still active)
    uint32_t n_pix;             // film pixels (width x height, no border)
    int32_t hb;                 // half-width of a footprint in cells: floor(filter radius + 0.5)
    uint32_t spp;               // the stopping rule is first tested at this count
    uint32_t cap;               // a pixel stops at this count whatever its error
    float max_error, quantile;
    float lum_floor;            // averageLuminance * 0.01f
};
