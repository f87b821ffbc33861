// kernels_ao.hip -- k_ao<SMALL, AN> and k_ao_resolve; see ao.h
#include "ao.h"
// variants by small_tables and sc.ext, the rule of launchDirectVariantSM (no texture variant: nothing is looked up)
extern "C" void mi_launch_ao(const DScene &sc, const RenderConst &rc, const AoConst &ac, const Queues &q, const BatchDesc &bd, uint32_t grid, size_t lds, hipStream_t st) {
    if (sc.small_tables != 0) { if (sc.ext) launchWithLds(k_ao<true, true>, grid, lds, st, sc, rc, ac, q, bd); else launchWithLds(k_ao<true, false>, grid, lds, st, sc, rc, ac, q, bd); }
    else if (sc.ext) launchWithLds(k_ao<false, true>, grid, lds, st, sc, rc, ac, q, bd);
    else launchWithLds(k_ao<false, false>, grid, lds, st, sc, rc, ac, q, bd);
}
extern "C" void mi_launch_ao_resolve(const Queues &q, float recip, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_ao_resolve, dim3(grid), dim3(WG), 0, st, q, recip);
}
