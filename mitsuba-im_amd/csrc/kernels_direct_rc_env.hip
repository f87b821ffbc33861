// kernels_direct_rc_env.hip -- k_direct<RC = true, ENV = true>; see direct.h
#include "direct.h"
extern "C" void mi_launch_direct_rc_env(const DScene &sc, const RenderConst &rc, const DirectConst &dc, const Queues &q, const BatchDesc &bd, int bsdfPass, uint32_t grid, size_t lds, hipStream_t st) {
    launchDirectVariant<true, true>(sc, rc, dc, q, bd, bsdfPass, grid, lds, st);
}
