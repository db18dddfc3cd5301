// The translation unit of k_cape_f32 (xp_cape_f32.hpp): xp_cape_cin with xp_opts.compute == XP_F32.  Compiled with the
// family units' flags (xarray_parcel_amd/_lib.py): ONE 1024-thread workgroup per CU, whose LDS holds the e_s / ln tables
// (11.8 KB), the fp32 copy of the family table (22.8 KB) and the scan's slots (96 KB); an ordinary launch, or persistent
// wavefronts where the fp64 family kernel takes them (CapeArgs::persist).
#include "xp_launch.hpp"
#include "xp_cape_f32.hpp"

namespace xp {

static_assert(XP_CAPE_THREADS == 1024, "k_cape_f32 is launched as one 1024-thread workgroup per CU");
static_assert((LDS_TAB + SLOT_FIELDS * SLOT_STRIDE) * 8 + FAM_COEFS * 4 + 64 <= 160 * 1024, "LDS budget of one workgroup per CU");

void launch_cape_f32(const CapeArgs &a, hipStream_t s) {
    if (a.ncol == 0) return;
    const int b = XP_CAPE_THREADS;
    with_bool(a.persist, [&](auto PERSIST) {               // persistent wavefronts: one workgroup per CU (as xp_cape_tu.hip)
        const unsigned nblk = PERSIST() ? persistent_blocks(a.ncol, b) : blocks_for(a.ncol, b);
        hipLaunchKernelGGL((k_cape_f32<float, PERSIST()>), dim3(nblk), dim3(b), 0, s, a);
    });
}

}  // namespace xp
