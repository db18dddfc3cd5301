"""Build-time guard on the operating points of the headline kernels (no GPU needed: hipcc cross-compiles and reports the
resource usage).

* RK4 kernels (moist mode 0, 256-thread workgroups): the surface-parcel CAPE/CIN instantiations must stay within 128
  VGPRs -- four wavefronts per SIMD -- without spilling, and the workgroup's LDS (tables + per-thread scan slots) within
  a quarter of a CU's 160 KB.
* Family kernels (moist mode 2, ONE 1024-thread workgroup per CU): 128 VGPRs is the hard cap that comes with 16
  wavefronts per CU, the LDS (e_s / ln tables + family coefficient table + scan slots) must fit the CU's 160 KB, and
  scratch must stay small -- without -disable-machine-licm the compiler hoists ~40 fp64 constants out of the level loop
  and spills them (200+ B / lane, reloaded every level: measured 1.33 ms instead of 0.93 on c2).
An innocent edit can cost 10-30 % here; this test says so."""
import itertools
import re

from tests.resource_report import needs_hipcc, resources
from xarray_parcel_amd import _lib


def _resources(tmp_path, mode):
    return resources(tmp_path, 'xp_cape_tu.hip', ['-DXP_TU_T=double', f'-DXP_TU_MODE={mode}'] + _lib.TU_FLAGS[mode])


def _pick(rec, pm, profile, mode, hum, deflt, lean=0, persist=0):
    # k_cape_cin<double, PMODE, PROFILE, MODE, HUM, DEF, LEAN, PERSIST>
    k = [n for n in rec if re.search(r'k_cape_cinIdLi%dELb%dELi%dELb%dELb%dELb%dELb%dE' % (pm, profile, mode, hum, deflt, lean, persist), n)]
    assert len(k) == 1, (pm, profile, mode, hum, deflt, lean, persist, list(rec))
    return rec[k[0]]


@needs_hipcc
def test_surface_kernel_keeps_four_waves_per_simd(tmp_path):
    rec = _resources(tmp_path, 0)
    for hum, deflt, lean in ((0, 1, 1), (0, 1, 0), (0, 0, 0), (1, 0, 0)):
        r = _pick(rec, 0, 0, 0, hum, deflt, lean)
        assert r['vgprs'] <= 128 and r['occupancy'] >= 4, r
        assert r['scratch'] <= 8, r                      # 8 B/lane is the call frame of the out-of-line slow paths
        assert r['lds'] <= 160 * 1024 // 4, r
    # the profile-output kernels (config c3) fit four waves too since the fixed polynomials take their coefficients
    # from scalar registers
    assert _pick(rec, 0, 1, 0, 0, 0)['vgprs'] <= 128


@needs_hipcc
def test_family_kernels_fit_one_workgroup_per_cu(tmp_path):
    rec = _resources(tmp_path, 2)
    # what xp_cape_tu.hip dispatches in family mode: the default-options + CAPE/CIN-only specialisation (DEF + LEAN) when
    # the caller asks for no more, the generic instantiation otherwise (DEF alone spills 40-55 VGPRs for the searching
    # parcels at the 128-VGPR cap) -- each as an ordinary launch and with persistent wavefronts
    for (pm, deflt, lean), persist in itertools.product(((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0),
                                                         (0, 1, 1), (1, 1, 1), (2, 1, 1), (3, 1, 1)), (0, 1)):
        r = _pick(rec, pm, 0, 2, 0, deflt, lean, persist)
        assert r['vgprs'] <= 128 and r['occupancy'] >= 4, r
        assert r['lds'] <= 160 * 1024, r
        assert r['spills'] == 0 and r['scratch'] <= 64, r    # no spill in the kernel; the scratch is the frames of the out-of-line slow paths


@needs_hipcc
def test_family_profile_kernels_spill_no_more_than_they_do(tmp_path):
    """The family kernels WITH profile output (BASELINE config 3 in family mode) do not fit the 128-VGPR cap of their 1024-thread
    workgroups without spilling: 12 VGPRs / 72 B of scratch for the surface and explicit parcels, 32-33 / 88-104 B for the
    searching ones.  That is measured and accepted -- but it is fragile: putting their LDS arrays into one object (as the
    other kernels have them) made it 18 VGPRs and cost c3 13 % (profiles/r03_ab.txt).  This bound says so when it moves."""
    rec = _resources(tmp_path, 2)
    for pm, cap in ((0, 80), (3, 80), (1, 112), (2, 104)):
        r = _pick(rec, pm, 1, 2, 0, 0, 0, 1)
        assert r['vgprs'] <= 128 and r['scratch'] <= cap, (pm, r)


@needs_hipcc
def test_fused_parcels_kernel_fits_one_workgroup_per_cu(tmp_path):
    """csrc/xp_multi.hpp, two parcels per thread: 512-thread workgroups (two wavefronts per SIMD, up to 256 VGPRs), LDS
    = tables + 2 x 12 slot fields x 512 threads within the CU's 160 KB, no VGPR spill."""
    rec = resources(tmp_path, 'xp_multi_tu.hip', ['-DXP_TU_T=float', '-DXP_MULTI_NP=2'] + _lib.MULTI_FLAGS[2])
    vg, lds, sp = ([r[k] for r in rec.values()] for k in ('vgprs', 'lds', 'vgpr_spill'))
    assert len(vg) == 2 and max(vg) <= 256 and max(lds) <= 160 * 1024 and max(sp) == 0, (vg, lds, sp)
