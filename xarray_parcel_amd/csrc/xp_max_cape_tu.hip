// The translation unit of k_max_cape_select and k_rebase_from (xp_max_cape.hpp says why it has one of its own) and their launchers.
#include "xp_launch.hpp"
#include "xp_max_cape.hpp"

namespace xp {

void launch_max_cape_select(const MaxCapeArgs &a, bool f64, bool table, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(table, [&](auto TABLE) {
        launch_columns(k_max_cape_select<decltype(z), TABLE()>, a.e.ncol, s, a);
    }); });
}

void launch_rebase_from(const RebaseFromArgs &a, bool f64, hipStream_t s) {
    with_type(f64, [&](auto z) { launch_columns(k_rebase_from<decltype(z)>, a.ncol, s, a); });
}

}  // namespace xp
