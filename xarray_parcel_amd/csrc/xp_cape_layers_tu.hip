// The translation unit of k_cape_layers (xp_cape_layers.hpp says why it has one of its own) and its launcher.
#include "xp_launch.hpp"
#include "xp_cape_layers.hpp"

namespace xp {

void launch_cape_layers(const CapeLayersArgs &a, bool f64, bool table, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(table, [&](auto TABLE) {
        launch_columns(k_cape_layers<decltype(z), TABLE()>, a.base.ncol, s, a);
    }); });
}

}  // namespace xp
