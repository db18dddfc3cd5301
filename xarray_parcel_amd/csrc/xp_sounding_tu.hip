// The translation unit of k_sounding (xp_sounding.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_sounding.hpp"

namespace xp {

namespace {
template <typename T, bool WIND> void launch_ccl(const SoundingArgs &a, int ccl, hipStream_t s) {
    const dim3 gr((unsigned)((a.ncol + 255) / 256)), bl(256);
    switch (ccl) {
        case CCL_NONE: hipLaunchKernelGGL((k_sounding<T, WIND, CCL_NONE>), gr, bl, 0, s, a); break;
        case CCL_SURFACE: hipLaunchKernelGGL((k_sounding<T, WIND, CCL_SURFACE>), gr, bl, 0, s, a); break;
        default: hipLaunchKernelGGL((k_sounding<T, WIND, CCL_MIXED>), gr, bl, 0, s, a); break;
    }
}
template <typename T> void launch_t(const SoundingArgs &a, bool wind, int ccl, hipStream_t s) {
    if (wind) launch_ccl<T, true>(a, ccl, s); else launch_ccl<T, false>(a, ccl, s);
}
}  // namespace

void launch_sounding(const SoundingArgs &a, bool f64, bool wind, int ccl, hipStream_t s) {
    if (a.ncol <= 0) return;
    if (f64) launch_t<double>(a, wind, ccl, s); else launch_t<float>(a, wind, ccl, s);
}

}  // namespace xp
