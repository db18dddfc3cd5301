// The translation unit of k_cape_layers (xp_cape_layers.hpp says why it has one of its own) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_cape_layers.hpp"

namespace xp {

void launch_cape_layers(const CapeLayersArgs &a, bool f64, bool table, hipStream_t s) {
    if (a.base.ncol <= 0) return;
    const dim3 gr((unsigned)((a.base.ncol + 255) / 256)), bl(256);
    if (f64) {
        if (table) hipLaunchKernelGGL((k_cape_layers<double, true>), gr, bl, 0, s, a);
        else hipLaunchKernelGGL((k_cape_layers<double, false>), gr, bl, 0, s, a);
    } else {
        if (table) hipLaunchKernelGGL((k_cape_layers<float, true>), gr, bl, 0, s, a);
        else hipLaunchKernelGGL((k_cape_layers<float, false>), gr, bl, 0, s, a);
    }
}

}  // namespace xp
