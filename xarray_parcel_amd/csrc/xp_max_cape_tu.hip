// The translation unit of k_max_cape_select and k_rebase_from (xp_max_cape.hpp says why it has one of its own) and their launchers.
#include <hip/hip_runtime.h>

#include "xp_max_cape.hpp"

namespace xp {

void launch_max_cape_select(const MaxCapeArgs &a, bool f64, bool table, hipStream_t s) {
    if (a.e.ncol <= 0) return;
    const dim3 gr((unsigned)((a.e.ncol + 255) / 256)), bl(256);
    if (f64) {
        if (table) hipLaunchKernelGGL((k_max_cape_select<double, true>), gr, bl, 0, s, a);
        else hipLaunchKernelGGL((k_max_cape_select<double, false>), gr, bl, 0, s, a);
    } else {
        if (table) hipLaunchKernelGGL((k_max_cape_select<float, true>), gr, bl, 0, s, a);
        else hipLaunchKernelGGL((k_max_cape_select<float, false>), gr, bl, 0, s, a);
    }
}

void launch_rebase_from(const RebaseFromArgs &a, bool f64, hipStream_t s) {
    if (a.ncol <= 0) return;
    const dim3 gr((unsigned)((a.ncol + 255) / 256)), bl(256);
    if (f64) hipLaunchKernelGGL(k_rebase_from<double>, gr, bl, 0, s, a);
    else hipLaunchKernelGGL(k_rebase_from<float>, gr, bl, 0, s, a);
}

}  // namespace xp
