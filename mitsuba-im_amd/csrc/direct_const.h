// direct_const.h -- per-render constants of the direct integrator's kernels (direct.h), shared with api.cpp
#pragma once
#include <stdint.h>

// Constants of one render (DirectConst::pass changes per launch).  Sampler layout: DESIGN.md §4.
struct DirectConst {
    uint32_t n_em, n_bs;                  // emitterSamples, bsdfSamples (direct.cpp:99-101)
    float weight_lum, weight_bsdf;        // 1 / N, 1 / M (direct.cpp:132-133)
    float frac_lum, frac_bsdf;            // N / (N + M), M / (N + M) (:134-135)
    uint32_t em_array, bs_array;          // a side with count > 1 -- Sobol': first of the two dimensions of its 2-D array (sobol.cpp:189-197); independent: call counter of element 0 (element j: counter - j)
    uint32_t em_dim, bs_dim;              // a side with count <= 1: dimension / call counter of its next2D on the sample's own index (the skip rules of sobol.cpp:233-235 already applied)
    uint32_t extra_dim;                   // running dimension / call counter after both requests: where the 1-D draws of EUsesSampler BSDFs start
    uint32_t array_end;                   // Sobol': m_arrayEndDim = 5 + 2 x (number of arrays) (sobol.cpp:176-178)
    uint32_t pass;                        // sub-sample j of this launch
};
