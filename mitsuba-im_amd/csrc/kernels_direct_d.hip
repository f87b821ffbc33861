// kernels_direct_d.hip -- k_direct<RC = false, ENV = false>; see direct.h
#include "direct.h"
extern "C" void mi_launch_direct_d(const DScene &sc, const RenderConst &rc, const DirectConst &dc, const Queues &q, const BatchDesc &bd, int bsdfPass, uint32_t grid, size_t lds, hipStream_t st) {
    launchDirectVariant<false, false>(sc, rc, dc, q, bd, bsdfPass, grid, lds, st);
}
