// One translation unit of libxparcel per (XP_TU_T, XP_TU_MODE): the k_cape_cin instantiations of that data type and
// moist mode (4 parcel modes x profile on/off x dewpoint / specific-humidity input, + the default-options specialisation of
// the CAPE/CIN-only dewpoint-input kernels) and the launcher that picks one.
// Compiled six times by the build (xarray_parcel_amd/_lib.py), e.g. -DXP_TU_T=double -DXP_TU_MODE=0.
#include <cstdlib>

#include "xp_launch.hpp"
#include "xp_kernels.hpp"

#if !defined(XP_TU_T) || !defined(XP_TU_MODE)
#error "compile with -DXP_TU_T=<float|double> -DXP_TU_MODE=<0|1|2>"
#endif

namespace xp {
namespace {

int cape_block() {             // XP_CAPE_BLOCK: workgroup size for experiments (64 / 128 / 256; default 256)
    static int b = [] { const char *e = getenv("XP_CAPE_BLOCK"); int v = e ? atoi(e) : XP_CAPE_THREADS; return (v == 64 || v == 128 || v == 256 || v == XP_CAPE_THREADS) ? v : XP_CAPE_THREADS; }();
    return b;
}

// k_cape_cin<T, PM, PROFILE, MODE, HUM, DEF, LEAN, PERSIST> for one call.  Which of the DEF / LEAN / LAZY instantiations a
// moist mode has is stated here and nowhere else; tests/test_kernel_resources.py watches the numbers the rules rest on.
template <typename T, int PM, int MODE, bool PERSIST> void launch_p(const CapeArgs &a, bool profile, hipStream_t s) {
    const int b = cape_block();
    // persistent wavefronts: one 1024-thread workgroup's worth of waves per CU
    const unsigned nblk = PERSIST ? persistent_blocks(a.ncol, b, b >= 1024 ? 1 : 1024 / b) : blocks_for(a.ncol, b);
    auto go = [&](auto PROFILE, auto HUM, auto DEF, auto LEAN) {
        hipLaunchKernelGGL((k_cape_cin<T, PM, PROFILE(), MODE, HUM(), DEF(), LEAN(), PERSIST>), dim3(nblk), dim3(b), 0, s, a);
    };
    constexpr std::true_type yes;
    constexpr std::false_type no;
    if (a.hum) { with_bool(profile, [&](auto PROFILE) { go(PROFILE, yes, no, no); }); return; }
    const bool dflt = a.vtc && a.pos_neg && a.log_interp;                           // the reference's defaults (pf.py:1396, 1293)
    const bool lean = cape_cin_only(a);
    if (profile) {
        if constexpr (MODE == 2) {
            // the lifted index and nothing else of the profile, default options, CAPE / CIN only (the product bundle's
            // parcel passes): the LAZY instantiation (PROFILE + DEF + LEAN, see k_cape_cin)
            if (a.prof.nlev_out == 0 && a.prof.li && dflt && lean) { go(yes, no, yes, yes); return; }
        }
        go(yes, no, no, no);
        return;
    }
    // Default-options (DEF) and CAPE/CIN-only (LEAN) specialisations: the reference's default option set as compile-time
    // constants, and -- when the caller wants neither LFC / EL temperatures nor interval indices (the bench, a multi-GPU
    // gather, the product bundle) -- no tracking of them.  The RK4 and lookup-table modes take both; the family kernels
    // sit at the 128-VGPR cap of their 1024-thread workgroups and take only the combination DEF + LEAN, which comes out
    // of the register allocator without a spill for every parcel (121-128 VGPRs; round 2's code base spilled here and
    // always took the generic kernel) and runs 2.5-5 % faster than the generic one (same-box A/B); DEF
    // alone still spills for the searching parcels (40-55 VGPRs) and stays with the generic kernel.
    if (dflt && lean) { go(no, no, yes, yes); return; }
    if constexpr (MODE != 2) {
        if (dflt) { go(no, no, yes, no); return; }
    }
    go(no, no, no, no);
}

}  // namespace

template <> void launch_cape_mode<XP_TU_T, XP_TU_MODE>(const CapeArgs &a, int pm, bool profile, hipStream_t s) {
    with_one_of<PM_SURFACE, PM_MU, PM_ML, PM_EXPLICIT>(pm, [&](auto PM) {
        if constexpr (XP_TU_MODE == 2) {                   // persistent wavefronts are the family kernels' alone
            if (a.persist) { launch_p<XP_TU_T, PM(), XP_TU_MODE, true>(a, profile, s); return; }
        }
        launch_p<XP_TU_T, PM(), XP_TU_MODE, false>(a, profile, s);
    });
}

}  // namespace xp
