// queues.h -- SoA wavefront queues in HBM (device pointers), shared by api.cpp and the kernel translation units (kernels_*.hip).
// Layout per path slot (algorithmic bytes, DESIGN.md §"bytes per segment"):
//   extension ray 24 B (rayO: o.xyz | rayD: d.xyz), hit 16 B (t,u,v,prim), path state 32 B
//   (st0: path id, sampler word a, sampler word b, dim|depth|flags; st1: throughput rgb; st2: bsdfPdf),
//   shadow record 44 B (shO: o.xyz,maxt | shD: d.xyz,path id | shC: contribution rgb), accumulator 16 B, film position 8 B.
// What is the same for every path of a launch is not stored: the interval (Epsilon, inf) of a bounce ray, eta = 1 where no BSDF of the shade variant changes it,
// the state (1,1,1), 1, 0 of a fresh path in front of k_shade.  The arrays that carry such a value where it does vary are allocated for those launches only:
//   rayT (mint, maxt) 8 B: camera rays (near / far clip) and the volumetric stages (medium vertices start at mint = 0);  eta 4 B: RC shade variants and the volumetric stages;
//   shCw 16 B instead of shC: the volumetric shadow records (contribution rgb | emitter-selection probability).
// The kernels reach rays, throughput, eta and shadow contributions through the accessors below only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mi355pt.h"

#define MI_TICKETS 1024
struct QVec3 { float x, y, z; };                // a 12-byte queue record: one 12-byte load / store per lane (profiles/r04_record_width.json)
struct Queues {
    QVec3 *rayO[2], *rayD[2];
    float2 *rayT[2];                            // (mint, maxt) where the interval differs from path to path (see above)
    uint4 *st0[2]; QVec3 *st1[2]; float *st2[2];
    float *eta[2];                              // only where a BSDF or a medium can change it (see above), else null
    float *st3[2];                              // only with a `constant` environment emitter: cos(wo, refN) of the vertex that spawned the ray (2 = no reference normal)
    float4 *hit;
    int32_t *hitInst;                           // only in scenes with instances: instance index of the hit (-1: a scene-level primitive)
    float4 *shO, *shD; QVec3 *shC;
    float4 *shCw;                               // volumetric integrators only: the wide form of shC (volume.h)
    float4 *shT, *shX;                          // volumetric integrators only: throughput and BSDF / phase value of a shadow record (the transmittance between the two enters before them, shade_vol.h)
    float4 *acc; float2 *pos;
    uint32_t *count[2]; uint32_t *shCount;      // per segment
    uint32_t *ticket;                           // [MI_TICKETS] segment tickets of the fused traversal launches of a batch (trace_fused.h), zeroed when the batch starts
    int32_t *stkSpill;                          // fused walk: stack entries beyond FZ_LDS_STACK, one column per lane of the persistent grid (entry e of lane l at [e * lanes + l])
    unsigned long long *counters;               // [0] closest-hit rays, [1] shadow rays, [2] sum of path depths
    uint32_t cap;                               // slots per segment (multiple of 64)
    uint32_t n_seg;                             // number of segments
};

// Element i of a queue array through a 32-bit BYTE offset: the address is base (a uniform pointer: SGPR pair) + a 32-bit vector offset, one shift instead of the
// 64-bit shift-and-add per access that `base[i]` costs with a 64-bit index -- integer vector operations issue at half the rate of fp32 multiply-adds on gfx950
// (scripts/ubench/valu_rates.hip), and the shade stage touches ~20 arrays per path.  Holds while a pool has fewer than 2^28 slots (allocPoolQ enforces it).
template <typename T> __device__ __forceinline__ T &qat(T *base, uint32_t i) { return *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + (uint32_t) (i * (uint32_t) sizeof(T))); }
template <typename T> __device__ __forceinline__ const T &qat(const T *base, uint32_t i) { return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (uint32_t) (i * (uint32_t) sizeof(T))); }

// ---- typed accessors: the one place that knows the element type of a ray, throughput, eta or shadow-contribution array.  12-byte offsets of fewer than 2^28 slots fit 32 bits.
#define MI_QDEV __device__ __forceinline__
MI_QDEV QVec3 qRayOrigin(const Queues &q, int buf, uint32_t i) { return qat(q.rayO[buf], i); }
MI_QDEV QVec3 qRayDirection(const Queues &q, int buf, uint32_t i) { return qat(q.rayD[buf], i); }
MI_QDEV void qSetRayOrigin(const Queues &q, int buf, uint32_t i, float x, float y, float z) { qat(q.rayO[buf], i) = QVec3{x, y, z}; }
MI_QDEV void qSetRayDirection(const Queues &q, int buf, uint32_t i, float x, float y, float z) { qat(q.rayD[buf], i) = QVec3{x, y, z}; }
MI_QDEV float2 qRayInterval(const Queues &q, int buf, uint32_t i) { return qat(q.rayT[buf], i); }
MI_QDEV void qSetRayInterval(const Queues &q, int buf, uint32_t i, float mint, float maxt) { qat(q.rayT[buf], i) = make_float2(mint, maxt); }
MI_QDEV QVec3 qThroughput(const Queues &q, int buf, uint32_t i) { return qat(q.st1[buf], i); }
MI_QDEV void qSetThroughput(const Queues &q, int buf, uint32_t i, float r, float g, float b) { qat(q.st1[buf], i) = QVec3{r, g, b}; }
MI_QDEV float qEta(const Queues &q, int buf, uint32_t i) { return qat(q.eta[buf], i); }
MI_QDEV void qSetEta(const Queues &q, int buf, uint32_t i, float eta) { qat(q.eta[buf], i) = eta; }
MI_QDEV QVec3 qShadowContribution(const Queues &q, uint32_t i) { return qat(q.shC, i); }
MI_QDEV void qSetShadowContribution(const Queues &q, uint32_t i, float r, float g, float b) { qat(q.shC, i) = QVec3{r, g, b}; }
MI_QDEV float4 qShadowContributionWide(const Queues &q, uint64_t i) { return q.shCw[i]; }      // (two records per path slot: the index may pass 2^28, no 32-bit byte offset)
MI_QDEV void qSetShadowContributionWide(const Queues &q, uint64_t i, float4 c) { q.shCw[i] = c; }

struct BatchDesc {
    mi_tile tile; uint32_t n_pix; uint32_t n_planes; uint32_t sample_begin; uint64_t n_paths;
    uint32_t row_stride;    // film rows of the tile: y0, y0 + row_stride, ... (1 = contiguous rectangle; N = rows interleaved over N ranks)
    const uint32_t *list;   // optional explicit (px, py, sampleIndex) triples, one per path (parity entry point mi_render_samples)
};
