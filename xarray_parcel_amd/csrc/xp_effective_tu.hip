// The translation unit of k_effective_inflow (xp_effective.hpp says why it has one of its own) and its launcher.
#include "xp_launch.hpp"
#include "xp_effective.hpp"

namespace xp {

void launch_effective_inflow(const EffectiveArgs &a, bool f64, bool table, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(table, [&](auto TABLE) {
        launch_columns(k_effective_inflow<decltype(z), TABLE()>, a.ncol, s, a);
    }); });
}

}  // namespace xp
