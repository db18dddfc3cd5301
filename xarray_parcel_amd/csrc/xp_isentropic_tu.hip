// The translation unit of k_isentropic (xp_isentropic.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_isentropic.hpp"

namespace xp {

void launch_isentropic(const IsentropicArgs &a, const IsentropicLevels &lv, bool f64, hipStream_t s) {
    bool extras = false;
    for (int q = 0; q < ISEN_MAX_VARS; ++q) extras = extras || a.vars[q] != nullptr;
    with_type(f64, [&](auto z) { with_bool(extras, [&](auto EXTRAS) {
        launch_columns(k_isentropic<decltype(z), EXTRAS()>, a.ncol, s, a, lv);
    }); });
}

}  // namespace xp
