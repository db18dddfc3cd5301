// The translation unit of k_isentropic (xp_isentropic.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_isentropic.hpp"

namespace xp {

namespace {
template <typename T> void launch_t(const IsentropicArgs &a, const IsentropicLevels &lv, bool extras, hipStream_t s) {
    const dim3 gr((unsigned)((a.ncol + 255) / 256)), bl(256);
    if (extras) hipLaunchKernelGGL((k_isentropic<T, true>), gr, bl, 0, s, a, lv);
    else hipLaunchKernelGGL((k_isentropic<T, false>), gr, bl, 0, s, a, lv);
}
}  // namespace

void launch_isentropic(const IsentropicArgs &a, const IsentropicLevels &lv, bool f64, hipStream_t s) {
    if (a.ncol <= 0) return;
    bool extras = false;
    for (int q = 0; q < ISEN_MAX_VARS; ++q) extras = extras || a.vars[q] != nullptr;
    if (f64) launch_t<double>(a, lv, extras, s); else launch_t<float>(a, lv, extras, s);
}

}  // namespace xp
