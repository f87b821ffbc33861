// record_width.hip -- streaming cost of one queue record per lane in the three forms a 3-float queue array can take on gfx950: the 16-byte record (xyz + a
// fourth lane), the 12-byte record (one 12-byte load / store per lane) and three dword planes.  Every kernel copies N records src -> dst the way the wavefront
// stages walk a segment (lane i takes record i, workgroups stride over the array), so bytes moved are known exactly: 2 x N x record size.
// Prints one JSON line per form (best and median of REPS launches).  Run under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (one counter per run, no
// tracing) the same launches calibrate the two counters for 12-byte lanes against the known byte counts (profiles/r04_record_width.json).
// Measurement tool (not part of libmi355pt.so): hipcc --offload-arch=gfx950 -O3 scripts/ubench/record_width.hip -o scripts/ubench/record_width
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define WG 256
#define REPS 9
struct Rec3 { float x, y, z; };

__global__ __launch_bounds__(WG) void k_copy16(const float4 *src, float4 *dst, uint32_t n) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) dst[i] = src[i];
}
__global__ __launch_bounds__(WG) void k_copy12(const Rec3 *src, Rec3 *dst, uint32_t n) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) dst[i] = src[i];
}
__global__ __launch_bounds__(WG) void k_copy3planes(const float *src, float *dst, uint32_t n) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        const float x = src[i], y = src[(size_t) n + i], z = src[2 * (size_t) n + i];
        dst[i] = x; dst[(size_t) n + i] = y; dst[2 * (size_t) n + i] = z;
    }
}
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    const uint32_t n = argc > 1 ? (uint32_t) atoll(argv[1]) : (32u << 20);      // records; fewer than 2^28, as in a path pool
    const uint32_t grid = argc > 2 ? (uint32_t) atoi(argv[2]) : 4096u;          // the traversal stages' grid
    if (n == 0 || n >= (1u << 28) || grid == 0 || grid > 65536u) { fprintf(stderr, "usage: record_width [records < 2^28] [grid <= 65536]\n"); return 2; }
    void *src = nullptr, *dst = nullptr;
    CHK(hipMalloc(&src, (size_t) n * 16)); CHK(hipMalloc(&dst, (size_t) n * 16));
    CHK(hipMemset(src, 0x3c, (size_t) n * 16)); CHK(hipMemset(dst, 0, (size_t) n * 16));
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    const char *names[3] = {"16B record", "12B record", "3 dword planes"}; const int bytes[3] = {16, 12, 12};
    for (int form = 0; form < 3; ++form) {
        std::vector<float> ms;
        for (int rep = 0; rep < REPS + 2; ++rep) {
            CHK(hipEventRecord(e0, nullptr));
            if (form == 0) hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(WG), 0, nullptr, (const float4 *) src, (float4 *) dst, n);
            else if (form == 1) hipLaunchKernelGGL(k_copy12, dim3(grid), dim3(WG), 0, nullptr, (const Rec3 *) src, (Rec3 *) dst, n);
            else hipLaunchKernelGGL(k_copy3planes, dim3(grid), dim3(WG), 0, nullptr, (const float *) src, (float *) dst, n);
            CHK(hipEventRecord(e1, nullptr)); CHK(hipEventSynchronize(e1)); CHK(hipGetLastError());
            float t = 0; CHK(hipEventElapsedTime(&t, e0, e1)); if (rep >= 2) ms.push_back(t);      // two warm-up launches
        }
        std::sort(ms.begin(), ms.end());
        const double moved = 2.0 * n * bytes[form], best = ms.front(), med = ms[ms.size() / 2];
        printf("{\"form\": \"%s\", \"records\": %u, \"grid\": %u, \"bytes_moved\": %.0f, \"ms_best\": %.4f, \"ms_median\": %.4f, \"GBps_best\": %.1f, \"GBps_median\": %.1f, \"us_per_Mrecords_median\": %.2f}\n",
               names[form], n, grid, moved, best, med, moved / best * 1e-6, moved / med * 1e-6, med * 1e3 / (n / 1e6));
    }
    CHK(hipFree(src)); CHK(hipFree(dst));
    return 0;
}
