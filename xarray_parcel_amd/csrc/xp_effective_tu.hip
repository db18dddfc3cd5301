// The translation unit of k_effective_inflow (xp_effective.hpp says why it has one of its own) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_effective.hpp"

namespace xp {

void launch_effective_inflow(const EffectiveArgs &a, bool f64, bool table, hipStream_t s) {
    if (a.ncol <= 0) return;
    const dim3 gr((unsigned)((a.ncol + 255) / 256)), bl(256);
    if (f64) {
        if (table) hipLaunchKernelGGL((k_effective_inflow<double, true>), gr, bl, 0, s, a);
        else hipLaunchKernelGGL((k_effective_inflow<double, false>), gr, bl, 0, s, a);
    } else {
        if (table) hipLaunchKernelGGL((k_effective_inflow<float, true>), gr, bl, 0, s, a);
        else hipLaunchKernelGGL((k_effective_inflow<float, false>), gr, bl, 0, s, a);
    }
}

}  // namespace xp
