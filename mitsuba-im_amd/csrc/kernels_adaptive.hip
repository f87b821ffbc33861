// kernels_adaptive.hip -- adaptive sampling behind the unchanged trace stages (adaptive.h; the reference's src/integrators/misc/adaptive.cpp:202-319)
#include "kernels_common.h"
#include "adaptive.h"

// round 0: the active list is the tile, row by row (film pixel index = py * width + px)
__global__ __launch_bounds__(WG) void k_adapt_tile(uint32_t *active, mi_tile tile, uint32_t width, uint32_t n) {
    const uint32_t a = blockIdx.x * WG + threadIdx.x;
    if (a >= n) return;
    const uint32_t tw = tile.x1 - tile.x0;
    active[a] = (tile.y0 + a / tw) * width + tile.x0 + a % tw;
}

// the (px, py, sampleIndex) triples of one batch for k_generate: path pid = plane x nAct + a draws sample `sampleBegin + plane` of active pixel a
__global__ __launch_bounds__(WG) void k_adapt_list(const uint32_t *active, uint32_t nAct, uint64_t nPaths, uint32_t sampleBegin, uint32_t width, uint32_t *list) {
    const uint64_t pid = (uint64_t) blockIdx.x * WG + threadIdx.x;
    if (pid >= nPaths) return;
    const uint32_t plane = (uint32_t) (pid / nAct), a = (uint32_t) (pid % nAct), p = active[a];
    list[pid * 3] = p % width; list[pid * 3 + 1] = p / width; list[pid * 3 + 2] = sampleBegin + plane;
}

// One thread per active pixel: its samples of the batch in sample order.  ImageBlock::put with k_film's rejection and k_film's footprint arithmetic, into the pixel's OWN
// footprint rows (plain loads and stores: nobody else touches them); then the online variance of adaptive.cpp:278-282 and the stopping rule of :284-304, one float32
// operation per line.  At the stop the footprint goes to the film scaled by 1.0f / n (the algebraic content of the snapshot blend at :307-317): the centre cell into
// `film` with a plain add, the others into `spill` with float atomics -- the split k_film makes.  The samples of the round that follow the stop are ignored.
// Bound by memory latency: every sample of a thread is a dependent read-modify-write chain over (2 hb + 1)^2 x 5 footprint words, strided by the film size.
__global__ __launch_bounds__(WG) void k_adapt_accumulate(DScene sc, Queues q, AdaptArgs ad, const uint32_t *active, uint32_t nAct, uint32_t nPlanes, float *film, float *spill) {
    const uint32_t a = blockIdx.x * WG + threadIdx.x;
    if (a >= nAct) return;
    const uint32_t p = active[a];
    if (ad.counts[p]) return;      // stopped in an earlier batch of this round
    const int px = (int) (p % sc.width), py = (int) (p / sc.width);
    const int W = (int) sc.width + 2 * sc.border, H = (int) sc.height + 2 * sc.border;
    const size_t plane = (size_t) W * H;
    const int ownX = px + sc.border, ownY = py + sc.border, hb = ad.hb, side = 2 * hb + 1;
    const float r = sc.filter_radius;
    float2 ms = ad.ms[p]; float mean = ms.x, meanSqr = ms.y; uint32_t n = ad.n[p];
    for (uint32_t s = 0; s < nPlanes; ++s) {
        const uint64_t pid = (uint64_t) s * nAct + a;
        const float4 li = q.acc[pid]; const float2 sp = q.pos[pid];
        const float vals[5] = {li.x, li.y, li.z, li.w, 1.0f};
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 5; ++k) bad |= (!isfinite(vals[k]) || vals[k] < 0);
        float lum = 0.0f;
        if (!bad) {
            lum = luminance(V(li.x, li.y, li.z));
            const float posx = sp.x - 0.5f - (float) (0 - sc.border), posy = sp.y - 0.5f - (float) (0 - sc.border);
            int minx = (int) ceilf(posx - r), miny = (int) ceilf(posy - r), maxx = (int) floorf(posx + r), maxy = (int) floorf(posy + r);
            minx = max(minx, 0); miny = max(miny, 0); maxx = min(maxx, W - 1); maxy = min(maxy, H - 1);
            // a sample of this pixel lies within half a pixel of its centre, so its footprint stays within hb = floor(radius + 0.5) cells of it; the clamp keeps the
            // index inside the pixel's rows whatever the position is
            minx = max(minx, ownX - hb); miny = max(miny, ownY - hb); maxx = min(maxx, ownX + hb); maxy = min(maxy, ownY + hb);
            for (int y = miny; y <= maxy; ++y) {
                const float wy = filterEvalDiscretized(sc, (float) y - posy);
                for (int x = minx; x <= maxx; ++x) {
                    const float w = filterEvalDiscretized(sc, (float) x - posx) * wy;
                    const size_t cell = (size_t) ((y - ownY + hb) * side + (x - ownX + hb)) * 5;
#pragma unroll
                    for (int k = 0; k < 5; ++k) { float *f = ad.fp + (cell + k) * ad.n_pix + p; *f = *f + w * vals[k]; }
                }
            }
        }
        ++n;
        const float delta = lum - mean;
        mean = mean + delta / (float) n;
        meanSqr = meanSqr + delta * (lum - mean);
        bool stop = n >= ad.cap;
        if (!stop && n >= ad.spp) {
            const float variance = meanSqr / (float) (n - 1u);
            const float stdError = sqrtf(variance / (float) n);
            const float ciWidth = stdError * ad.quantile;
            const float base = maxf(mean, ad.lum_floor);
            stop = ciWidth <= ad.max_error * base;
        }
        if (stop) {
            const float inv = 1.0f / (float) n;
            for (int dy = -hb; dy <= hb; ++dy) for (int dx = -hb; dx <= hb; ++dx) {
                const int x = ownX + dx, y = ownY + dy;
                if (x < 0 || y < 0 || x >= W || y >= H) continue;
                const size_t cell = (size_t) ((dy + hb) * side + (dx + hb)) * 5, at = (size_t) y * W + x;
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const float v = ad.fp[(cell + k) * ad.n_pix + p] * inv;
                    if (dx == 0 && dy == 0) film[k * plane + at] = film[k * plane + at] + v;
                    else if (v != 0.0f) atomicAdd(&spill[k * plane + at], v);
                }
            }
            ad.counts[p] = n;
            break;
        }
    }
    ad.ms[p] = make_float2(mean, meanSqr); ad.n[p] = n;
}

// The next active list: the pixels of `active` that have not stopped, in the same order.  Wave w owns the entries [w x rangeLen, (w + 1) x rangeLen): k_adapt_count
// leaves its number of survivors, k_adapt_compact sums the counts of the waves in front of it into one uniform offset and writes its survivors behind it by ballot rank.
// No atomics: the list's order, and with it every later batch's path numbering, does not depend on timing.
__global__ __launch_bounds__(WG) void k_adapt_count(const uint32_t *active, uint32_t nAct, const uint32_t *counts, uint32_t rangeLen, uint32_t nRanges, uint32_t *waveCount) {
    const uint32_t w = blockIdx.x * (WG / 64) + threadIdx.x / 64, lane = threadIdx.x & 63u;
    if (w >= nRanges) return;
    const uint64_t begin = (uint64_t) w * rangeLen, end = begin + rangeLen < (uint64_t) nAct ? begin + rangeLen : (uint64_t) nAct;
    uint32_t c = 0;
    for (uint64_t base = begin; base < end; base += 64) {
        const uint64_t i = base + lane;
        const bool alive = i < end && counts[active[i]] == 0u;
        c += (uint32_t) __popcll(__ballot(alive));
    }
    if (lane == 0) waveCount[w] = c;
}
__global__ __launch_bounds__(WG) void k_adapt_compact(const uint32_t *active, uint32_t nAct, const uint32_t *counts, uint32_t rangeLen, uint32_t nRanges, const uint32_t *waveCount,
                                                      uint32_t *next, uint32_t *nNext) {
    const uint32_t w = blockIdx.x * (WG / 64) + threadIdx.x / 64, lane = threadIdx.x & 63u;
    if (w >= nRanges) return;
    uint32_t off = 0;
    for (uint32_t j = lane; j < w; j += 64) off += waveCount[j];
    for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d);
    const uint64_t begin = (uint64_t) w * rangeLen, end = begin + rangeLen < (uint64_t) nAct ? begin + rangeLen : (uint64_t) nAct;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint64_t base = begin; base < end; base += 64) {
        const uint64_t i = base + lane;
        const uint32_t p = i < end ? active[i] : 0u;
        const bool alive = i < end && counts[p] == 0u;
        const unsigned long long m = __ballot(alive);
        if (alive) next[off + (uint32_t) __popcll(m & lt)] = p;
        off += (uint32_t) __popcll(m);
    }
    if (w == nRanges - 1u && lane == 0) *nNext = off;
}

extern "C" {
void mi_launch_adapt_tile(uint32_t *active, mi_tile tile, uint32_t width, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_adapt_tile, dim3((n + WG - 1) / WG), dim3(WG), 0, st, active, tile, width, n);
}
void mi_launch_adapt_list(const uint32_t *active, uint32_t nAct, uint64_t nPaths, uint32_t sampleBegin, uint32_t width, uint32_t *list, hipStream_t st) {
    hipLaunchKernelGGL(k_adapt_list, dim3((unsigned) ((nPaths + WG - 1) / WG)), dim3(WG), 0, st, active, nAct, nPaths, sampleBegin, width, list);
}
void mi_launch_adapt_accumulate(const DScene &sc, const Queues &q, const AdaptArgs &ad, const uint32_t *active, uint32_t nAct, uint32_t nPlanes, float *film, float *spill, hipStream_t st) {
    hipLaunchKernelGGL(k_adapt_accumulate, dim3((nAct + WG - 1) / WG), dim3(WG), 0, st, sc, q, ad, active, nAct, nPlanes, film, spill);
}
// active -> next, *nNext = entries of next.  nAct >= 1; waveCount holds MI_ADAPT_RANGES words
void mi_launch_adapt_compact(const uint32_t *active, uint32_t nAct, const uint32_t *counts, uint32_t *waveCount, uint32_t *next, uint32_t *nNext, hipStream_t st) {
    const uint32_t nRanges = std::min<uint32_t>(MI_ADAPT_RANGES, (nAct + 63u) / 64u);
    const uint32_t rangeLen = ((nAct + nRanges - 1u) / nRanges + 63u) / 64u * 64u;
    const uint32_t grid = (nRanges + WG / 64 - 1) / (WG / 64);
    hipLaunchKernelGGL(k_adapt_count, dim3(grid), dim3(WG), 0, st, active, nAct, counts, rangeLen, nRanges, waveCount);
    hipLaunchKernelGGL(k_adapt_compact, dim3(grid), dim3(WG), 0, st, active, nAct, counts, rangeLen, nRanges, waveCount, next, nNext);
}
}
