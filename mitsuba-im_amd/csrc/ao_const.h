// ao_const.h -- per-render constants of the ambient-occlusion integrator's kernels (ao.h), shared with api.cpp
#pragma once
#include <stdint.h>

// Constants of one render (AoConst::pass changes per launch).  Sampler layout: DESIGN.md §4, the numbering `direct` gives its emitter side.
struct AoConst {
    uint32_t n;                           // shadingSamples (ao.cpp:40)
    float ray_length;                     // m_rayLength after preprocess (ao.cpp:77-80): the caller's, or half the radius of the scene's bounding sphere
    float recip;                          // 1.0f / (float) n: Spectrum::operator/= multiplies by the reciprocal (spectrum.h:447-456)
    uint32_t array;                       // n > 1 -- Sobol': first of the two dimensions of the 2-D array (5, sobol.cpp:171-198); independent: call counter of element 0 (element j: counter - j)
    uint32_t own_dim;                     // n == 1: dimension / call counter of nextSample2D on the sample's own index (the skip rule of sobol.cpp:233-235 already applied)
    uint32_t pass;                        // shading sample j of this launch
};
