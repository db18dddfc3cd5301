// The translation unit of k_ncape (xp_ecape.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_ecape.hpp"

namespace xp {

void launch_ncape(const NcapeArgs &a, bool f64, hipStream_t s) {
    if (a.ncol <= 0) return;
    const dim3 gr((unsigned)((a.ncol + 255) / 256)), bl(256);
    if (f64) hipLaunchKernelGGL(k_ncape<double>, gr, bl, 0, s, a);
    else hipLaunchKernelGGL(k_ncape<float>, gr, bl, 0, s, a);
}

}  // namespace xp
