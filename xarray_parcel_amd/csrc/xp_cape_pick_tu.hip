// The translation unit of k_cape_pick (xp_cape_pick.hpp says why it has one of its own) and its launcher.
#include "xp_launch.hpp"
#include "xp_cape_pick.hpp"

namespace xp {

void launch_cape_pick(const CapeArgs &a, int pmode, int which, bool f64, bool table, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(table, [&](auto TABLE) { with_bool(a.hum != 0, [&](auto HUM) {
        launch_columns(k_cape_pick<decltype(z), TABLE(), HUM()>, a.ncol, s, a, pmode, which);
    }); }); });
}

}  // namespace xp
