// xparcel.hip -- C ABI of libxparcel (include/xparcel.h): argument checking, host<->device staging,
// kernel dispatch.  Everything numerical lives in xp_device.hpp / xp_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/xparcel.h"
#include "xp_launch.hpp"
#include "xp_kernels.hpp"
#include "xp_cape_f32.hpp"
#include "xp_multi.hpp"
#include "xp_ground.hpp"
#include "xp_bundle.hpp"
#include "xp_dcape.hpp"
#include "xp_kinematics.hpp"
#include "xp_effective.hpp"
#include "xp_max_cape.hpp"
#include "xp_cape_layers.hpp"
#include "xp_cape_pick.hpp"
#include "xp_wind_layers.hpp"
#include "xp_thermo_layers.hpp"
#include "xp_sounding.hpp"
#include "xp_isentropic.hpp"
#include "xp_hydrostatic.hpp"
#include "xp_humidity.hpp"
#include "xp_ecape.hpp"
#include "xp_per_point.hpp"

static_assert(xp::ST_TOP_NAN == XP_ST_TOP_NAN && xp::ST_LCL_NOT_CONVERGED == XP_ST_LCL_NOT_CONVERGED &&
              xp::ST_NAN_PRESSURE == XP_ST_NAN_PRESSURE && xp::ST_BAD_PRESSURE == XP_ST_BAD_PRESSURE &&
              xp::ST_NO_LAYER == XP_ST_NO_LAYER && xp::ST_BAD_HEIGHT == XP_ST_BAD_HEIGHT &&
              xp::ST_LAYER_OPEN == XP_ST_LAYER_OPEN && xp::ST_NO_CCL == XP_ST_NO_CCL &&
              xp::ST_NOT_CONVERGED == XP_ST_NOT_CONVERGED, "the kernels' status bits are the ABI's");
static_assert(xp::ISEN_MAX_LEVELS == XP_ISEN_MAX_LEVELS && xp::ISEN_MAX_VARS == sizeof(xp_isentropic_out::vars) / sizeof(void *),
              "the isentropic kernel's limits are the ABI's");
static_assert(xp::HY_MAX_LAYERS == sizeof(xp_hydrostatic_out::thickness) / sizeof(void *) && xp::HY_DEWPOINT == XP_HUM_DEWPOINT + 1 &&
              xp::HY_SPECIFIC == XP_HUM_SPECIFIC + 1, "the hydrostatic kernel's limits and moisture kinds follow the ABI's");
static_assert(xp::HUM_RELATIVE == XP_HUM_RELATIVE && xp::HUM_MIXING_RATIO == XP_HUM_MIXING_RATIO, "the conversion kernel's moisture kinds are the ABI's");
static_assert(xp::PM_SURFACE == XP_PARCEL_SURFACE && xp::PM_MU == XP_PARCEL_MOST_UNSTABLE && xp::PM_ML == XP_PARCEL_MIXED_LAYER &&
              xp::PM_EXPLICIT == XP_PARCEL_EXPLICIT, "the kernels' parcel kinds are the ABI's");
static_assert(xp::PICK_LOWEST == XP_OPT_LAYER_LOWEST >> XP_OPT_LAYER_SHIFT && xp::PICK_HIGHEST == XP_OPT_LAYER_HIGHEST >> XP_OPT_LAYER_SHIFT &&
              xp::PICK_DEEPEST == XP_OPT_LAYER_DEEPEST >> XP_OPT_LAYER_SHIFT && xp::PICK_MOST_CAPE == XP_OPT_LAYER_MOST_CAPE >> XP_OPT_LAYER_SHIFT,
              "the positive-layer kernel's choices are the ABI's");
static_assert(xp::CCL_TOP == XP_CCL_TOP && xp::CCL_BOTTOM == XP_CCL_BOTTOM, "the kernel's CCL choices are the ABI's");
static_assert(xp::WL_PRESSURE == XP_LAYER_PRESSURE && xp::WL_PRESSURE_DEPTH == XP_LAYER_PRESSURE_DEPTH &&
              xp::WL_HEIGHT == XP_LAYER_HEIGHT, "the kernel's layer kinds are the ABI's");

namespace {

thread_local char g_err[512] = "";
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(XP_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

struct State {
    std::mutex mu;
    bool init = false;
    int device = -1;
    bool tables = false;
    xp::Tables tb{};
    void *tb_index = nullptr, *tb_adiabats = nullptr;
    double *es_tab = nullptr;   // device copy of the e_s(T) polynomial table
    double *fam_tab = nullptr;  // device copy of the adiabat-family table
    std::vector<double> fam_host;
} g;

size_t esize(int dtype) { return dtype == XP_F64 ? 8 : 4; }

// e_s(T) table for xp::es_tab: per 1 K interval the degree-ES_DEG interpolant of Bolton's formula at Chebyshev nodes,
// monomial coefficients in r = T - left edge (what v_fract_f64 delivers), built in long double; layout [coefficient][interval].
void build_es_table(double *out) {
    using LD = long double;
    const int n = xp::ES_DEG + 1;
    const LD pi = 3.14159265358979323846264338327950288L;
    for (int i = 0; i < xp::ES_N; ++i) {
        LD edge = (LD)xp::ES_T_LO + (LD)i;
        LD A[8][9];
        for (int k = 0; k < n; ++k) {
            LD r = 0.5L + 0.5L * cosl(pi * ((LD)k + 0.5L) / (LD)n);
            LD t = edge + r;
            LD v = 1.0L;
            for (int j = 0; j < n; ++j) { A[k][j] = v; v *= r; }
            A[k][n] = 6.112L * expl(17.67L * (t - 273.15L) / (t - 29.65L));
        }
        for (int col = 0; col < n; ++col) {                     // Gaussian elimination with partial pivoting
            int piv = col;
            for (int r = col + 1; r < n; ++r) if (fabsl(A[r][col]) > fabsl(A[piv][col])) piv = r;
            for (int j = 0; j <= n; ++j) { LD t_ = A[col][j]; A[col][j] = A[piv][j]; A[piv][j] = t_; }
            for (int r = 0; r < n; ++r) {
                if (r == col) continue;
                LD f = A[r][col] / A[col][col];
                for (int j = col; j <= n; ++j) A[r][j] -= f * A[col][j];
            }
        }
        for (int j = 0; j < n; ++j) out[j * xp::ES_STRIDE + i] = (double)(A[j][n] / A[j][j]);
    }
    // ln table for xp::log_tab: mantissa interval i of [0.5, 1) has centre c_i = (i + 64.5) / 128
    double *lt = out + xp::LOG_OFF;                    // spare columns of rows 0 (1/c_i) and 1 (ln c_i)
    for (int i = 0; i < xp::LOG_N; ++i) {
        LD c = ((LD)i + 64.5L) / 128.0L;
        lt[i] = (double)(1.0L / c);
        lt[xp::ES_STRIDE + i] = (double)logl(c);
    }
    // exp(i / 64) for xp::dry_factor: spare columns of row 2 (exp(0) = 1 exactly)
    for (int i = 0; i < xp::EXPT_N; ++i) out[xp::EXPT_OFF + i] = (double)expl((LD)(i + xp::EXPT_LO) / 64.0L);
}

// Stages host buffers through device scratch for one call; device buffers pass through.
struct Stager {
    hipStream_t s;
    struct Back { void *host; void *dev; size_t bytes; };
    std::vector<void *> scratch;
    std::vector<Back> back;
    bool any_host = false;
    explicit Stager(void *stream) : s((hipStream_t)stream) {}
    // stream-ordered allocations: a host-array call stages ~25 buffers, and hipMalloc / hipFree would each synchronise
    ~Stager() { for (void *p : scratch) (void)hipFreeAsync(p, s); }
    // device scratch for this call, released with the Stager
    template <typename P> int alloc(size_t bytes, P **d) {
        void *v = nullptr;
        HIP_TRY(hipMallocAsync(&v, bytes ? bytes : 1, s));
        scratch.push_back(v);
        *d = (P *)v;
        return 0;
    }
    int in(const void *p, size_t bytes, int mem, const void **out) {
        *out = p;
        if (p == nullptr || mem == XP_MEM_DEVICE) return 0;
        void *d;
        if (int rc = alloc(bytes, &d)) return rc;
        HIP_TRY(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, s));
        any_host = true;
        *out = d;
        return 0;
    }
    int out(void *p, size_t bytes, int mem, void **dev) {
        *dev = p;
        if (p == nullptr || mem == XP_MEM_DEVICE) return 0;
        void *d;
        if (int rc = alloc(bytes, &d)) return rc;
        back.push_back({p, d, bytes});
        any_host = true;
        *dev = d;
        return 0;
    }
    int out(int32_t *p, size_t bytes, int mem, int32_t **dev) {
        void *d;
        const int rc = out((void *)p, bytes, mem, &d);
        *dev = (int32_t *)d;
        return rc;
    }
    int finish() {
        HIP_TRY(hipGetLastError());
        for (const Back &b : back) HIP_TRY(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s));
        if (any_host) HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
};

// adiabat-family table (xp::Family; specification restated independently in oracle/family.py): the VIRTUAL temperature
// T (1 + 0.608 w_s(p, T)) of the parcel along the pseudo-adiabat through every psi-node (Chebyshev points of every psi-piece) is marched from 1000 hPa through the x-nodes (Chebyshev
// points of every x-piece, in order of distance) by classical RK4 with steps <= 1/80, and every (x-piece, psi-piece)
// block of 9 x 9 values is turned into the monomial coefficients of its interpolant (long double elimination).
double fam_dt_dlnp(double x, double t) {
    double p = std::exp(x), e = 6.112 * std::exp(17.67 * (t - 273.15) / (t - 29.65)), pe = p - e;
    double num = xp::RD * t * pe + xp::LV * xp::EPS * e;
    double den = xp::CP_D * xp::RD * t * t * pe + xp::LV * xp::LV * xp::EPS * xp::EPS * e;
    return xp::RD * t * t * num / den;
}
double fam_march(double x, double t, double x1) {
    int n = (int)std::ceil(std::fabs(x1 - x) / 0.0125 - 1e-12);
    if (n < 1) n = 1;
    const double h = (x1 - x) / n;
    for (int s = 0; s < n; ++s) {
        double k1 = fam_dt_dlnp(x, t);
        double k2 = fam_dt_dlnp(x + 0.5 * h, t + 0.5 * h * k1);
        double k3 = fam_dt_dlnp(x + 0.5 * h, t + 0.5 * h * k2);
        double k4 = fam_dt_dlnp(x + h, t + h * k3);
        t = t + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4);
        x = x + h;
    }
    return t;
}
// monomial coefficients of the polynomial through (u_k, y_k), k < n
void fam_interpolant(int n, const double *u, const double *y, double *c) {
    using LD = long double;
    std::vector<LD> A((size_t)n * (n + 1));
    auto at = [&](int r, int col) -> LD & { return A[(size_t)r * (n + 1) + col]; };
    for (int k = 0; k < n; ++k) {
        LD v = 1.0L;
        for (int i = 0; i < n; ++i) { at(k, i) = v; v *= (LD)u[k]; }
        at(k, n) = (LD)y[k];
    }
    for (int col = 0; col < n; ++col) {
        int piv = col;
        for (int r = col + 1; r < n; ++r) if (fabsl(at(r, col)) > fabsl(at(piv, col))) piv = r;
        for (int i = 0; i <= n; ++i) std::swap(at(col, i), at(piv, i));
        for (int r = 0; r < n; ++r) {
            if (r == col) continue;
            LD f = at(r, col) / at(col, col);
            for (int i = col; i <= n; ++i) at(r, i) -= f * at(col, i);
        }
    }
    for (int i = 0; i < n; ++i) c[i] = (double)(at(i, n) / at(i, i));
}
const double kFamEdges[xp::FAM_NPS + 1] = XP_FAM_EDGES;
// the psi-piece centres and reciprocal half-widths the device reads behind the coefficients
void fam_append_pieces(double *tab) {
    for (int q = 0; q < xp::FAM_NPS; ++q) {
        tab[xp::FAM_COEFS + q] = 0.5 * (kFamEdges[q] + kFamEdges[q + 1]);
        tab[xp::FAM_COEFS + xp::FAM_NPS + q] = 1.0 / (0.5 * (kFamEdges[q + 1] - kFamEdges[q]));
    }
}
// The device copy is laid out [power of s][power of z][x-piece][psi-piece] (+ the appended piece constants): the nine
// coefficients a lane multiplies through one Horner row are then 5184 B apart, beyond the reach of ds_read2_b64, so the
// compiler issues plain ds_read_b64 (2 LDS cycles each, banks mod 64) instead of pairing them (8 cycles per pair, banks mod
// 32) -- the same remedy as the e_s table's row stride (xp_device.hpp).  The ABI / oracle order stays [x-piece][z][s][psi].
std::vector<double> family_device_layout(const std::vector<double> &host) {
    const int NN = xp::FAM_ND + 1, MM = xp::FAM_MD + 1;
    std::vector<double> dev(host.size());
    for (int j = 0; j < xp::FAM_NPX; ++j)
        for (int n = 0; n < NN; ++n)
            for (int m = 0; m < MM; ++m)
                for (int q = 0; q < xp::FAM_NPS; ++q)
                    dev[(((size_t)m * NN + n) * xp::FAM_NPX + j) * xp::FAM_NPS + q] = host[(((size_t)j * NN + n) * MM + m) * xp::FAM_NPS + q];
    for (int i = xp::FAM_COEFS; i < xp::FAM_SIZE; ++i) dev[i] = host[i];
    return dev;
}
void build_family_table(double *tab) {
    const int NN = xp::FAM_ND + 1, MM = xp::FAM_MD + 1, NXN = xp::FAM_NPX * NN, NSN = xp::FAM_NPS * MM;
    const double pi = 3.14159265358979323846;
    std::vector<double> un(NN), um(MM), xs(NXN), ps(NSN), vals((size_t)NXN * NSN);
    for (int k = 0; k < NN; ++k) un[k] = std::cos(pi * (k + 0.5) / NN);
    for (int k = 0; k < MM; ++k) um[k] = std::cos(pi * (k + 0.5) / MM);
    for (int j = 0; j < xp::FAM_NPX; ++j)
        for (int k = 0; k < NN; ++k) xs[j * NN + k] = (xp::FAM_XHI - xp::FAM_WX * (j + 0.5)) + 0.5 * xp::FAM_WX * un[k];
    for (int q = 0; q < xp::FAM_NPS; ++q)
        for (int k = 0; k < MM; ++k)
            ps[q * MM + k] = 0.5 * (kFamEdges[q] + kFamEdges[q + 1]) + 0.5 * (kFamEdges[q + 1] - kFamEdges[q]) * um[k];
    for (int side = 0; side < 2; ++side) {
        std::vector<int> order;
        for (int i = 0; i < NXN; ++i) if ((side == 0) == (xs[i] <= xp::FAM_X1000)) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::fabs(xs[a] - xp::FAM_X1000) < std::fabs(xs[b] - xp::FAM_X1000); });
        for (int c = 0; c < NSN; ++c) {
            double x = xp::FAM_X1000, t = ps[c];
            for (int i : order) {
                if (xs[i] != x) { t = fam_march(x, t, xs[i]); x = xs[i]; }
                // the parcel's virtual temperature along the adiabat (pf.py:760 + 775), which is what the table holds
                const double pr = std::exp(xs[i]), e = 6.112 * std::exp(17.67 * (t - 273.15) / (t - 29.65));
                vals[(size_t)i * NSN + c] = t * (1.0 + xp::VT_EPS * (xp::EPS * e / (pr - e)));
            }
        }
    }
    std::vector<double> a((size_t)NN * MM), col(NN), cf(NN), row(MM), rf(MM);
    for (int j = 0; j < xp::FAM_NPX; ++j)
        for (int q = 0; q < xp::FAM_NPS; ++q) {
            for (int m = 0; m < MM; ++m) {
                for (int k = 0; k < NN; ++k) col[k] = vals[(size_t)(j * NN + k) * NSN + (q * MM + m)];
                fam_interpolant(NN, un.data(), col.data(), cf.data());
                for (int n = 0; n < NN; ++n) a[(size_t)n * MM + m] = cf[n];
            }
            for (int n = 0; n < NN; ++n) {
                for (int m = 0; m < MM; ++m) row[m] = a[(size_t)n * MM + m];
                fam_interpolant(MM, um.data(), row.data(), rf.data());
                for (int m = 0; m < MM; ++m) tab[(((size_t)j * NN + n) * MM + m) * xp::FAM_NPS + q] = rf[m];
            }
        }
    fam_append_pieces(tab);
}

int check_view(const xp_view *v, const char *name) {
    if (!v || !v->data) return fail(XP_E_ARG, "%s: null view", name);
    if (v->dtype != XP_F32 && v->dtype != XP_F64) return fail(XP_E_ARG, "%s: dtype must be XP_F32 or XP_F64", name);
    if (v->nlev < 1 || v->ncol < 0 || v->nlev >= (1ll << 30))
        return fail(XP_E_ARG, "%s: bad shape (%lld, %lld)", name, (long long)v->nlev, (long long)v->ncol);
    if (v->mem == XP_MEM_HOST && !(v->col_stride == 1 && v->lev_stride == v->ncol))
        return fail(XP_E_ARG, "%s: host views must be dense (nlev, ncol) C-order", name);
    return 0;
}
// the views of one call: each of them valid, all of them of the first one's shape and dtype
struct Arg { const xp_view *v; const char *name; };
int check_views(std::initializer_list<Arg> vs) {
    for (const Arg &x : vs)
        if (int rc = check_view(x.v, x.name)) return rc;
    const Arg &a = *vs.begin();
    for (const Arg &b : vs)
        if (b.v->nlev != a.v->nlev || b.v->ncol != a.v->ncol || b.v->dtype != a.v->dtype)
            return fail(XP_E_ARG, "%s/%s: views differ in shape or dtype", a.name, b.name);
    return 0;
}
int stage_view(Stager &st, const xp_view *v, xp::View *out) {
    const void *d;
    int rc = st.in(v->data, (size_t)v->nlev * (size_t)v->ncol * esize(v->dtype), v->mem, &d);
    if (rc) return rc;
    out->data = d; out->ls = v->lev_stride; out->cs = v->col_stride;
    return 0;
}
size_t rows_bytes(const xp_view *v, int64_t rows) { return (size_t)rows * (size_t)v->ncol * esize(v->dtype); }
// an output laid out like view v (a device output keeps its input's strides), or as dense (rows, ncol)
xp::OutView out_like(void *d, const xp_view *v) { return {d, v->lev_stride, v->col_stride}; }
xp::OutView dense_out(void *d, int64_t ncol) { return {d, ncol, 1}; }
// an output struct with a dtype and a mem of its own: present, and both equal to the views'
template <typename O> int check_out(const char *entry, const O *out, const xp_view *v) {
    if (!out) return fail(XP_E_ARG, "%s: out: null", entry);
    if (out->dtype != v->dtype || out->mem != v->mem) return fail(XP_E_ARG, "%s: out: dtype / mem differ from the views'", entry);
    return 0;
}

// every entry point switches to the library's device for its duration and leaves the calling thread's current device
// as it found it (the caller -- torch, say -- may be working on another one)
struct DevGuard {
    int prev = -1;
    DevGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
int ensure_init() {
    if (!g.init) return fail(XP_E_NOT_INIT, "xp_init() has not been called");
    hipError_t e = hipSetDevice(g.device);
    if (e != hipSuccess) return fail(XP_E_HIP, "hipSetDevice(%d): %s", g.device, hipGetErrorString(e));
    return 0;
}
// an entry point's prologue: the library's device, XP_E_NOT_INIT (rc) before any argument, the call's Stager
struct Entry : DevGuard, Stager {
    int rc;
    explicit Entry(void *stream) : Stager(stream), rc(ensure_init()) {}
};
// run-time values -> template arguments, and the launch geometry: xp_launch.hpp
using xp::launch_columns;
using xp::with_bool;
using xp::with_int;
using xp::with_one_of;
using xp::with_type;

// A per-point entry point (kernel and operations: xp_per_point.hpp): n points of dtype in mem.  The first n_required of
// `in` must be given, the rest may be null, and so may the outputs unless out_required.
template <typename Op> int per_point(const char *entry, int64_t n, int32_t dtype, int32_t mem, std::initializer_list<const void *> in,
                                     int n_required, std::initializer_list<void *> out, bool out_required, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    if (n < 0 || (dtype != XP_F32 && dtype != XP_F64)) return fail(XP_E_ARG, "%s: bad n / dtype", entry);
    bool null = false;
    for (int i = 0; i < n_required; ++i) null = null || !in.begin()[i];
    for (void *o : out) null = null || (out_required && !o);
    if (null) return fail(XP_E_ARG, "%s: null argument", entry);
    const size_t b = (size_t)n * esize(dtype);
    xp::PointArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    int rc, i = 0;
    for (const void *p : in) if ((rc = st.in(p, b, mem, &a.in[i++]))) return rc;
    i = 0;
    for (void *p : out) if ((rc = st.out(p, b, mem, &a.out[i++]))) return rc;
    with_type(dtype == XP_F64, [&](auto z) { launch_columns(xp::k_per_point<decltype(z), Op>, n, st.s, a); });
    return st.finish();
}

int stage_scalars(Stager &st, xp_scalars_out *s, int64_t ncol, xp::ScalarsOut *o) {
    memset(o, 0, sizeof(*o));
    if (!s) { o->f64 = 1; return 0; }
    if (s->dtype != XP_F32 && s->dtype != XP_F64) return fail(XP_E_ARG, "scalars: bad dtype");
    if (s->mem != XP_MEM_HOST && s->mem != XP_MEM_DEVICE) return fail(XP_E_ARG, "scalars: mem must be XP_MEM_HOST or XP_MEM_DEVICE");
    o->f64 = s->dtype == XP_F64;
    size_t fb = (size_t)ncol * esize(s->dtype), ib = (size_t)ncol * 4;
    int rc = 0;
#define F_(dst, src) if (!rc) rc = st.out(s->src, fb, s->mem, &o->dst)
#define I_(dst, src) if (!rc) rc = st.out(s->src, ib, s->mem, &o->dst)
    F_(cape, cape); F_(cin, cin); F_(lcl_p, lcl_pressure); F_(lcl_t, lcl_temperature); F_(lcl_tv, lcl_virtual_temperature);
    F_(lfc_p, lfc_pressure); F_(lfc_t, lfc_temperature); F_(el_p, el_pressure); F_(el_t, el_temperature);
    I_(lfc_idx, lfc_index); I_(el_idx, el_index); I_(status, status); I_(parcel_idx, parcel_index);
    F_(par_p, parcel_pressure); F_(par_t, parcel_temperature); F_(par_td, parcel_dewpoint);
#undef F_
#undef I_
    return rc;
}

// The library's tables for one call, read under the lock that xp_init / xp_set_tables / xp_set_family_table replace
// them under; table mode needs the reference-format tables loaded.
struct TableSet { xp::Tables tb; const double *es, *fam; };
int snapshot_tables(bool table_mode, TableSet *t) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (table_mode && !g.tables) return fail(XP_E_NO_TABLES, "Call load_moist_adiabat_lookups first.");
    *t = {g.tb, g.es_tab, g.fam_tab};
    return 0;
}

// Family mode runs persistent wavefronts (k_cape_cin / k_cape_cin_multi, PERSIST) on grids of at least this many
// columns; mode is the parcel's XP_PARCEL_*, or -1 for the fused several-parcels kernel.  Measured per grid size
// (profiles/r03_persist.txt, scripts/run_gpu_persist.py): equal to the ordinary launch up to two rounds of workgroups
// (512 Ki columns), 10-13 % faster from three rounds on (768 Ki ... 2 Mi columns of 64 f64 levels; c2: 0.64 -> 0.575 ms)
// -- a workgroup's sixteen wavefronts no longer wait for the slowest of them before the next sixteen tiles start.
// XP_PERSIST_MIN_COLS (A/B) overrides every threshold; bench.py's persist_min_cols mirrors the single-parcel ones.
bool persist(int mode, int64_t ncol) {
    static const long long env = [] { const char *e = getenv("XP_PERSIST_MIN_COLS"); return e ? atoll(e) : -1ll; }();
    const bool searching = mode < 0 || mode == XP_PARCEL_MOST_UNSTABLE || mode == XP_PARCEL_MIXED_LAYER;
    const long long min_cols = env >= 0 ? env : searching ? (1ll << 19) : (3ll << 18);
    return (long long)ncol >= min_cols && ncol < (1ll << 36);
}

// k_cape_cin's 96 instantiations are compiled in six translation units (xp_cape_tu.hip, one per dtype x moist mode) so
// that the build parallelises; this file only picks the unit.  pm: the parcel's XP_PARCEL_*, which is the units' PM_*
// (launch_cape_mode makes it a template argument; any other value is the explicit parcel there).
template <typename T> void launch_cape(const xp::CapeArgs &a, int pm, bool profile, hipStream_t s) {
    if (a.ncol == 0) return;
    if (a.table_mode) xp::launch_cape_mode<T, 1>(a, pm, profile, s);
    else if (a.flags) {                                      // family mode: fast pass, then RK4 for the flagged columns
        xp::launch_cape_mode<T, 2>(a, pm, profile, s);
        xp::CapeArgs b = a;
        b.only_flagged = 1;
        xp::launch_cape_mode<T, 0>(b, pm, profile, s);
    } else xp::launch_cape_mode<T, 0>(a, pm, profile, s);
}

// the options of a call that passes none (the reference's defaults)
xp_opts default_opts() {
    xp_opts o;
    memset(&o, 0, sizeof(o));
    o.virtual_temperature_correction = 1; o.lcl_interp = XP_LCL_INTERP_LOG; o.pos_cape_neg_cin = 1; o.compute = XP_F64;
    return o;
}
// the XP_OPT_LAYER_* field of xp_opts.flags as the kernel's PICK_* (0: the envelope, the default)
int layer_of(const xp_opts &o) { return (o.flags & XP_OPT_LAYER_MASK) >> XP_OPT_LAYER_SHIFT; }
// f32_ok: the caller implements xp_opts.compute == XP_F32 (xp_cape_cin alone, which then holds the call to check_compute32);
// layer_ok: it implements XP_OPT_LAYER_* (xp_cape_cin and xp_cape_cin_multi, without profile output)
int check_opts(const xp_opts &o, bool f32_ok = false, bool layer_ok = false) {
    if (layer_of(o)) {
        if (!layer_ok) return fail(XP_E_ARG, "xp_opts.flags: XP_OPT_LAYER_* is honoured by xp_cape_cin and xp_cape_cin_multi without profile output only");
        if (layer_of(o) > xp::PICK_MOST_CAPE) return fail(XP_E_ARG, "xp_opts.flags: bad XP_OPT_LAYER_* value %d", layer_of(o));
        if (!o.pos_cape_neg_cin) return fail(XP_E_ARG, "xp_opts.flags: XP_OPT_LAYER_* is defined for pos_cape_neg_cin only");
        if (o.compute == XP_F32) return fail(XP_E_ARG, "xp_opts.flags: XP_OPT_LAYER_* does not combine with xp_opts.compute = XP_F32");
    }
    if (o.lcl_interp != XP_LCL_INTERP_LINEAR && o.lcl_interp != XP_LCL_INTERP_LOG)
        return fail(XP_E_INTERP, "interpolator must be linear or log");
    if (o.moist_mode != XP_MOIST_EXACT && o.moist_mode != XP_MOIST_TABLE && o.moist_mode != XP_MOIST_FAMILY)
        return fail(XP_E_ARG, "bad moist_mode");
    if (o.compute != XP_F64 && !(f32_ok && o.compute == XP_F32))
        return fail(XP_E_ARG, o.compute == XP_F32 ? "xp_opts.compute: XP_F32 arithmetic is implemented by xp_cape_cin only" : "xp_opts.compute: XP_F32 or XP_F64");
    if (o.humidity < XP_HUM_DEWPOINT || o.humidity > XP_HUM_MIXING_RATIO) return fail(XP_E_ARG, "bad xp_opts.humidity");
    return 0;
}
// XP_PARCEL_OVER_GROUND: the flag on a surface / most-unstable / mixed-layer mode, and the parcel mode under it
bool over_ground(const xp_parcel &parcel) {
    return parcel.mode >= XP_PARCEL_OVER_GROUND && parcel.mode < (XP_PARCEL_OVER_GROUND | XP_PARCEL_EXPLICIT);
}
int parcel_mode(const xp_parcel &parcel) { return over_ground(parcel) ? parcel.mode & 3 : parcel.mode; }
// ground_ok: the caller implements XP_PARCEL_OVER_GROUND (xp_cape_cin, xp_cape_cin_multi, xp_select_parcel);
// max_cape_ok: it implements XP_PARCEL_MAX_CAPE (the same three)
int check_parcel(const xp_parcel *parcel, bool ground_ok = false, bool max_cape_ok = false) {
    if (!parcel) return fail(XP_E_ARG, "parcel: null");
    if (parcel->mode == (XP_PARCEL_OVER_GROUND | XP_PARCEL_EXPLICIT))
        return fail(XP_E_ARG, "parcel: XP_PARCEL_OVER_GROUND does not combine with XP_PARCEL_EXPLICIT");
    if (over_ground(*parcel)) {
        if (!ground_ok) return fail(XP_E_ARG, "parcel: XP_PARCEL_OVER_GROUND is honoured by xp_cape_cin, xp_cape_cin_multi and xp_select_parcel only");
        if (!parcel->pressure || !parcel->temperature || !parcel->dewpoint)
            return fail(XP_E_ARG, "parcel: XP_PARCEL_OVER_GROUND needs the surface pressure, temperature and dewpoint arrays");
        return 0;
    }
    if (max_cape_ok && parcel->mode == XP_PARCEL_MAX_CAPE) {
        if (!(std::isfinite(parcel->depth) && parcel->depth > 0.0)) return fail(XP_E_ARG, "parcel: XP_PARCEL_MAX_CAPE: depth must be finite and positive");
        return 0;
    }
    if (parcel->mode < XP_PARCEL_SURFACE || parcel->mode > XP_PARCEL_EXPLICIT) return fail(XP_E_ARG, "parcel: bad mode");
    if (parcel->mode == XP_PARCEL_EXPLICIT && (!parcel->pressure || !parcel->temperature || !parcel->dewpoint))
        return fail(XP_E_ARG, "explicit parcel: null arrays");
    return 0;
}
// the arguments of the CAPE family: p / T / Td, each of np parcels, the options
int check_cape(const xp_view *p, const xp_view *t, const xp_view *td, int np, const xp_parcel *parcels, const xp_opts &o, bool f32_ok = false,
               bool ground_ok = false, bool max_cape_ok = false, bool layer_ok = false) {
    if (int rc = check_views({{p, "pressure"}, {t, "temperature"}, {td, "dewpoint"}})) return rc;
    for (int i = 0; i < np; ++i) {
        if (int rc = check_parcel(parcels + i, ground_ok, max_cape_ok)) return rc;
        if (parcels[i].mode == XP_PARCEL_MAX_CAPE && o.humidity == XP_HUM_SPECIFIC)
            return fail(XP_E_ARG, "parcel: XP_PARCEL_MAX_CAPE: humidity must be XP_HUM_DEWPOINT");
    }
    // the parcels of one call share its grid: over the ground all of them, over the same surface fields, or none
    for (int i = 1; i < np; ++i) {
        const xp_parcel &a = parcels[0], &b = parcels[i];
        if (over_ground(a) != over_ground(b) || (over_ground(a) && (a.pressure != b.pressure || a.temperature != b.temperature || a.dewpoint != b.dewpoint)))
            return fail(XP_E_ARG, "parcels: XP_PARCEL_OVER_GROUND must be set on every parcel, with the same surface arrays, or on none");
    }
    return check_opts(o, f32_ok, layer_ok);
}

// XP_HUM_RELATIVE / XP_HUM_MIXING_RATIO (csrc/xp_humidity.hpp): the staged moisture view *m becomes the dewpoint D of the
// header, a dense (nlev, ncol) array in the call's scratch, written on the call's stream; the other kinds leave *m alone.
// What follows is the dewpoint-input call on D.
int dewpoint_front(Stager &st, const xp_view *p, const xp_opts &o, const xp::View &pv, const xp::View &tv, xp::View *m) {
    if (o.humidity != XP_HUM_RELATIVE && o.humidity != XP_HUM_MIXING_RATIO) return 0;
    xp::HumidityArgs h = {pv, tv, *m, p->nlev, p->ncol, nullptr};
    if (int rc = st.alloc(rows_bytes(p, p->nlev), &h.out)) return rc;
    xp::launch_dewpoint_from(h, p->dtype == XP_F64, o.humidity, st.s);
    *m = {h.out, p->ncol, 1};
    return 0;
}

// the CAPE family's p / T / Td, options and tables, staged once per call however many parcels it lifts; `ground`: a parcel
// with XP_PARCEL_OVER_GROUND, whose surface arrays re-base the grid (csrc/xp_ground.hpp) before anything else sees it
int stage_cape(Stager &st, const xp_view *p, const xp_view *t, const xp_view *td, const xp_opts &o, xp::CapeArgs *a,
               const xp_parcel *ground = nullptr) {
    int rc;
    TableSet ts;
    memset(a, 0, sizeof(*a));
    if ((rc = snapshot_tables(o.moist_mode == XP_MOIST_TABLE, &ts)) || (rc = stage_view(st, p, &a->p)) ||
        (rc = stage_view(st, t, &a->t)) || (rc = stage_view(st, td, &a->td)) ||
        (rc = dewpoint_front(st, p, o, a->p, a->t, &a->td))) return rc;       // (before the ground cut and the densify step)
    a->nlev = p->nlev; a->ncol = p->ncol;
    a->tb = ts.tb; a->es_tab = ts.es; a->fam_tab = ts.fam;
    // fast level addressing (xp_kernels.hpp load3): common strides, non-negative, column offsets below 4 GiB
    const bool same = a->p.ls == a->t.ls && a->p.ls == a->td.ls && a->p.cs == a->t.cs && a->p.cs == a->td.cs;
    const unsigned long long row = (unsigned long long)(p->ncol > 0 ? p->ncol : 1) * esize(p->dtype);
    a->off32 = 1;
    a->hum = o.humidity == XP_HUM_SPECIFIC;
    if (ground) {                                            // the views are read in place; this replaces the densify step
        if (row >= (1ull << 32)) return fail(XP_E_ARG, "more than 4 GiB per level row");
        xp::GroundArgs ga;
        ga.p = a->p; ga.t = a->t; ga.m = a->td; ga.nlev = p->nlev; ga.ncol = p->ncol;
        const size_t b = rows_bytes(p, 1);
        if ((rc = st.in(ground->pressure, b, p->mem, &ga.ps)) || (rc = st.in(ground->temperature, b, p->mem, &ga.ts)) ||
            (rc = st.in(ground->dewpoint, b, p->mem, &ga.tds)) || (rc = st.alloc(rows_bytes(p, p->nlev + 1), &ga.op)) ||
            (rc = st.alloc(rows_bytes(p, p->nlev + 1), &ga.ot)) || (rc = st.alloc(rows_bytes(p, p->nlev + 1), &ga.otd))) return rc;
        with_type(p->dtype == XP_F64, [&](auto z) { with_bool(a->hum, [&](auto HUM) {
            launch_columns(xp::k_ground_rebase<decltype(z), HUM()>, p->ncol, st.s, ga);
        }); });
        a->nlev = p->nlev + 1; a->hum = 0;
        a->p = {ga.op, p->ncol, 1}; a->t = {ga.ot, p->ncol, 1}; a->td = {ga.otd, p->ncol, 1};
    } else if (!(same && a->p.cs >= 0 && a->p.ls >= 0 && (unsigned long long)a->p.cs * row < (1ull << 32))) {
        if (row >= (1ull << 32)) return fail(XP_E_ARG, "more than 4 GiB per level row");
        const int64_t n = p->nlev * p->ncol;                 // rare: densify the three views on the device first
        for (xp::View *v : {&a->p, &a->t, &a->td}) {
            void *d;
            if (n == 0) break;
            if ((rc = st.alloc(rows_bytes(p, p->nlev), &d))) return rc;
            with_type(p->dtype == XP_F64, [&](auto z) { using T = decltype(z); launch_columns(xp::k_densify<T>, n, st.s, *v, p->nlev, p->ncol, (T *)d); });
            *v = {d, p->ncol, 1};
        }
    }
    a->vtc = o.virtual_temperature_correction; a->log_interp = o.lcl_interp == XP_LCL_INTERP_LOG;
    a->pos_neg = o.pos_cape_neg_cin; a->post_zero = o.post_zero_cin; a->table_mode = o.moist_mode == XP_MOIST_TABLE;
    return 0;
}
// one parcel's part of the arguments: its depth, and the arrays of an explicit parcel (in the views' dtype and mem)
int set_parcel(Stager &st, const xp_parcel &parcel, const xp_view *p, xp::CapeArgs *a) {
    a->depth = parcel.depth;
    a->ex_p = a->ex_t = a->ex_td = nullptr;
    if (parcel.mode != XP_PARCEL_EXPLICIT) return 0;         // (the surface arrays of XP_PARCEL_OVER_GROUND: stage_cape)
    const size_t b = rows_bytes(p, 1);
    int rc;
    if ((rc = st.in(parcel.pressure, b, p->mem, &a->ex_p)) || (rc = st.in(parcel.temperature, b, p->mem, &a->ex_t)) ||
        (rc = st.in(parcel.dewpoint, b, p->mem, &a->ex_td))) return rc;
    return 0;
}
int fill_common(Stager &st, const xp_view *p, const xp_view *t, const xp_view *td, const xp_parcel *parcel,
                const xp_opts &o, xp::CapeArgs *a, bool f32_ok = false, bool ground_ok = false, bool max_cape_ok = false, bool layer_ok = false) {
    int rc;
    if ((rc = check_cape(p, t, td, 1, parcel, o, f32_ok, ground_ok, max_cape_ok, layer_ok)) ||
        (rc = stage_cape(st, p, t, td, o, a, over_ground(*parcel) ? parcel : nullptr)) || (rc = set_parcel(st, *parcel, p, a)))
        return rc;
    return 0;
}
// one parcel's outputs: its scalars and, when asked for, its profile rows and lifted index
int stage_cape_out(Stager &st, int dtype, xp_scalars_out *scalars, xp_profile_out *profile, xp::CapeArgs *a) {
    int rc;
    if ((rc = stage_scalars(st, scalars, a->ncol, &a->s)) || !profile) return rc;
    if (profile->dtype != XP_F32 && profile->dtype != XP_F64) return fail(XP_E_ARG, "profile: bad dtype");
    if (profile->mem != XP_MEM_HOST && profile->mem != XP_MEM_DEVICE) return fail(XP_E_ARG, "profile: mem must be XP_MEM_HOST or XP_MEM_DEVICE");
    if (profile->nlev_out < a->nlev + 1) return fail(XP_E_ARG, "profile: nlev_out must be >= nlev + 1");
    if (profile->lev_stride < 0 || profile->col_stride < 0) return fail(XP_E_ARG, "profile: lev_stride and col_stride must not be negative");
    if (profile->mem == XP_MEM_HOST && !(profile->col_stride == 1 && profile->lev_stride == a->ncol))
        return fail(XP_E_ARG, "profile: host arrays must be dense (nlev_out, ncol)");
    void *src[6] = {profile->pressure, profile->temperature, profile->virtual_temperature,
                    profile->environment_temperature, profile->environment_virtual_temperature,
                    profile->environment_dewpoint};
    size_t b = (size_t)profile->nlev_out * (size_t)a->ncol * esize(profile->dtype);
    int rows = 0;                                            // how many of the six arrays are wanted
    for (int v = 0; v < 6; ++v) {
        if ((rc = st.out(src[v], b, profile->mem, &a->prof.v[v]))) return rc;
        rows += a->prof.v[v] != nullptr;
    }
    a->prof.nlev_out = rows ? profile->nlev_out : 0;         // lifted index only: the kernel's row loops see an empty profile
    a->prof.ls = profile->lev_stride; a->prof.cs = profile->col_stride;
    a->prof.f64 = profile->dtype == XP_F64;
    a->prof.native6 = rows == 6 && profile->dtype == dtype;
    if (profile->lifted_index) {
        if (!(profile->lifted_index_pressure > 0.0)) return fail(XP_E_ARG, "profile: lifted_index_pressure must be positive");
        if ((rc = st.out(profile->lifted_index, (size_t)a->ncol * esize(profile->dtype), profile->mem, &a->prof.li))) return rc;
        a->prof.li_x = log(profile->lifted_index_pressure);
    }
    return 0;
}
// family mode's scratch for cape_pass: which columns the RK4 pass redoes (null in the other modes)
int family_flags(Stager &st, const xp_opts &o, int64_t ncol, int32_t **flags) {
    *flags = nullptr;
    if (o.moist_mode != XP_MOIST_FAMILY || ncol == 0) return 0;
    return st.alloc(sizeof(int32_t) * (size_t)ncol, flags);
}
// one parcel's CAPE / CIN on staged arguments; the parcels of one call share the family flags (one stream orders them)
// layer: the call's XP_OPT_LAYER_* choice (layer_of) -- not the envelope: the positive-layer kernel (csrc/xp_cape_pick.hpp)
// in place of the CAPE kernels, XP_MOIST_FAMILY as exact, no flags and no redo pass
void cape_pass(const Stager &st, xp::CapeArgs a, int dtype, int mode, bool profile, int32_t *flags, int layer = 0) {
    if (layer) { xp::launch_cape_pick(a, mode, layer, dtype == XP_F64, a.table_mode != 0, st.s); return; }
    a.flags = flags;
    a.persist = flags && persist(mode, a.ncol);
    with_type(dtype == XP_F64, [&](auto z) { launch_cape<decltype(z)>(a, mode, profile, st.s); });
}

// XP_PARCEL_MAX_CAPE (csrc/xp_max_cape.hpp), the selection on a call's staged views: k* per column into scratch of the call
// (kstar), or, for xp_select_parcel, the parcel it names into `sel`.  Lifted with the call's four options, by the tables in
// table mode and by RK4 otherwise.
int max_cape_select(Stager &st, const xp_parcel &parcel, const xp::CapeArgs &a, const xp_view *p, const xp::ScalarsOut *sel, int32_t **kstar) {
    xp::MaxCapeArgs m;
    memset(&m, 0, sizeof(m));
    m.e.p = a.p; m.e.t = a.t; m.e.td = a.td;
    m.e.nlev = a.nlev; m.e.ncol = a.ncol; m.e.depth = parcel.depth;
    m.e.vtc = a.vtc; m.e.log_interp = a.log_interp; m.e.pos_neg = a.pos_neg; m.e.post_zero = a.post_zero;
    m.e.tb = a.tb; m.e.es_tab = a.es_tab;
    if (sel) m.s = *sel;
    else if (int rc = st.alloc(sizeof(int32_t) * (size_t)a.ncol, &m.kstar)) return rc;
    if (kstar) *kstar = m.kstar;
    xp::launch_max_cape_select(m, p->dtype == XP_F64, a.table_mode != 0, st.s);
    return 0;
}
// ... and the front of a CAPE / CIN call with that parcel: the selection, then the columns from k* on as three dense scratch
// arrays in place of the views.  What follows is the call with XP_PARCEL_SURFACE on those; copy_kstar ends it.
int max_cape_front(Stager &st, const xp_parcel &parcel, const xp_view *p, xp::CapeArgs *a, int32_t **kstar) {
    int rc;
    xp::RebaseFromArgs r;
    if ((rc = max_cape_select(st, parcel, *a, p, nullptr, kstar)) || (rc = st.alloc(rows_bytes(p, p->nlev), &r.op)) ||
        (rc = st.alloc(rows_bytes(p, p->nlev), &r.ot)) || (rc = st.alloc(rows_bytes(p, p->nlev), &r.otd))) return rc;
    r.p = a->p; r.t = a->t; r.td = a->td; r.kstar = *kstar; r.nlev = a->nlev; r.ncol = a->ncol;
    xp::launch_rebase_from(r, p->dtype == XP_F64, st.s);
    a->p = {r.op, a->ncol, 1}; a->t = {r.ot, a->ncol, 1}; a->td = {r.otd, a->ncol, 1};
    return 0;
}
// parcel_index = k*, the most-unstable parcel's convention, over the 0 the surface pass stored (same stream: after it)
int copy_kstar(const Stager &st, const int32_t *kstar, const xp::CapeArgs &a) {
    if (kstar && a.s.parcel_idx && a.ncol > 0)
        HIP_TRY(hipMemcpyAsync(a.s.parcel_idx, kstar, sizeof(int32_t) * (size_t)a.ncol, hipMemcpyDeviceToDevice, st.s));
    return 0;
}

// xp_opts.compute == XP_F32 is honoured in exactly one case (include/xparcel.h); every other one names what it is held to
int check_compute32(const xp_view *p, const xp_parcel *parcel, const xp_opts &o, const xp_scalars_out *s, const xp_profile_out *profile) {
    if (p->dtype != XP_F32) return fail(XP_E_ARG, "xp_opts.compute = XP_F32: the views must be XP_F32");
    if (parcel->mode != XP_PARCEL_SURFACE) return fail(XP_E_ARG, "xp_opts.compute = XP_F32: parcel->mode must be XP_PARCEL_SURFACE");
    if (o.moist_mode != XP_MOIST_FAMILY) return fail(XP_E_ARG, "xp_opts.compute = XP_F32: moist_mode must be XP_MOIST_FAMILY");
    if (o.humidity != XP_HUM_DEWPOINT) return fail(XP_E_ARG, "xp_opts.compute = XP_F32: humidity must be XP_HUM_DEWPOINT");
    if (!o.virtual_temperature_correction || o.lcl_interp != XP_LCL_INTERP_LOG || !o.pos_cape_neg_cin || o.post_zero_cin)
        return fail(XP_E_ARG, "xp_opts.compute = XP_F32: virtual_temperature_correction, lcl_interp, pos_cape_neg_cin and post_zero_cin must be at their defaults");
    if (profile) return fail(XP_E_ARG, "xp_opts.compute = XP_F32: profile must be NULL");
    if (s && (s->lfc_temperature || s->el_temperature || s->lfc_index || s->el_index || s->status))
        return fail(XP_E_ARG, "xp_opts.compute = XP_F32: scalars->lfc_temperature, el_temperature, lfc_index, el_index and status must be NULL");
    return 0;
}
// the fp32-arithmetic pass (csrc/xp_cape_f32.hpp), then RK4 for the columns the family table cannot serve, as cape_pass
void cape_pass32(const Stager &st, xp::CapeArgs a, int32_t *flags) {
    if (a.ncol == 0) return;
    a.flags = flags;
    a.persist = persist(XP_PARCEL_SURFACE, a.ncol);
    xp::launch_cape_f32(a, st.s);
    a.only_flagged = 1; a.persist = 0;
    xp::launch_cape_mode<float, 0>(a, xp::PM_SURFACE, false, st.s);
}

// xp_interp_levels on checked views (xp_conv_properties calls it on its staged winds)
int interp_levels(Stager &st, const xp_view *coords, int32_t nvar, const xp_view *const *variables, int32_t ntarget,
                  const double *at, int32_t log_coords, void *const *out) {
    xp::View cv;
    xp::InterpMany m;
    memset(&m, 0, sizeof(m));
    int rc;
    if ((rc = stage_view(st, coords, &cv))) return rc;
    for (int v = 0; v < nvar; ++v) {
        if ((rc = stage_view(st, variables[v], &m.x[v]))) return rc;
        for (int j = 0; j < ntarget; ++j)
            if ((rc = st.out(out[v * ntarget + j], rows_bytes(coords, 1), coords->mem, &m.out[v * ntarget + j]))) return rc;
    }
    for (int j = 0; j < ntarget; ++j) m.at[j] = at[j];
    with_type(coords->dtype == XP_F64, [&](auto z) { with_int<1, 4>(nvar, [&](auto NV) { with_int<1, 4>(ntarget, [&](auto NT) {
        launch_columns(xp::k_interp_levels<decltype(z), NV(), NT()>, coords->ncol, st.s, cv, m, coords->nlev, coords->ncol, (int)log_coords);
    }); }); });
    return 0;
}

// The body of xp_storm_relative_helicity and xp_storm_relative_helicity_layers (entry: which of them, for the messages).
// bounds(a) is the caller's part: it checks its own bounds arguments and puts them into a -- the LAYERS ones as the caller's
// pointers, staged here.
template <bool LAYERS, typename O, typename F>
int helicity(const char *entry, const xp_view *z, const xp_view *u, const xp_view *v, const void *surface_u,
             const void *surface_v, const void *storm_u, const void *storm_v, int n, O *out, void *stream, F &&bounds) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    xp::SrhArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = check_views({{z, "height"}, {u, "u"}, {v, "v"}})) || (rc = check_out(entry, out, z)) || (rc = bounds(a))) return rc;
    if (!surface_u != !surface_v) return fail(XP_E_ARG, "%s: surface wind: give both components or neither", entry);
    const size_t cb = rows_bytes(z, 1);
    if ((rc = stage_view(st, z, &a.z)) || (rc = stage_view(st, u, &a.u)) || (rc = stage_view(st, v, &a.v)) ||
        (rc = st.in(surface_u, cb, z->mem, &a.sfc_u)) || (rc = st.in(surface_v, cb, z->mem, &a.sfc_v)) ||
        (rc = st.in(storm_u, cb, z->mem, &a.storm_u)) || (rc = st.in(storm_v, cb, z->mem, &a.storm_v))) return rc;
    if constexpr (LAYERS)
        if ((rc = st.in(a.bottom_col, cb, z->mem, &a.bottom_col))) return rc;
    for (int i = 0; i < n; ++i) {
        if ((rc = st.out(out->positive[i], cb, out->mem, &a.pos[i])) || (rc = st.out(out->negative[i], cb, out->mem, &a.neg[i])) ||
            (rc = st.out(out->total[i], cb, out->mem, &a.tot[i]))) return rc;
        if constexpr (LAYERS)
            if ((rc = st.in(a.top_col[i], cb, z->mem, &a.top_col[i])) || (rc = st.out(out->shear_u[i], cb, out->mem, &a.shu[i])) ||
                (rc = st.out(out->shear_v[i], cb, out->mem, &a.shv[i]))) return rc;
    }
    if ((rc = st.out(out->status, (size_t)z->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = z->nlev; a.ncol = z->ncol; a.n = n;
    with_type(z->dtype == XP_F64, [&](auto t) {
        if constexpr (LAYERS) launch_columns(xp::k_helicity_layers<decltype(t)>, z->ncol, st.s, a);
        else launch_columns(xp::k_storm_relative_helicity<decltype(t)>, z->ncol, st.s, a);
    });
    return st.finish();
}

bool multi_fused_ok(int32_t np, const xp_parcel *parcels, const xp_opts &o, const xp_profile_out *profiles) {
    if (!(o.flags & XP_OPT_FUSE_PARCELS) || o.moist_mode != XP_MOIST_FAMILY || o.humidity == XP_HUM_SPECIFIC) return false;
    if (np != 2 || profiles) return false;                                   // instantiated parcel counts (xp_multi_tu.hip)
    for (int i = 0; i < np; ++i)
        if (parcel_mode(parcels[i]) == XP_PARCEL_EXPLICIT || parcel_mode(parcels[i]) == XP_PARCEL_MAX_CAPE) return false;
    return true;
}

}  // namespace

extern "C" {

int xp_version(void) { return XP_VERSION; }
const char *xp_last_error(void) { return g_err; }

int xp_init(int device) {
    std::lock_guard<std::mutex> lk(g.mu);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(XP_E_NO_DEVICE, "no HIP device: %s", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(XP_E_ARG, "device %d out of range (0..%d)", device, n - 1);
    DevGuard dg_;
    if (g.init && g.device != device) {                      // moving to another device: nothing queued on the old one may
        HIP_TRY(hipSetDevice(g.device));                     // still be reading the buffers freed below
        HIP_TRY(hipDeviceSynchronize());
    }
    HIP_TRY(hipSetDevice(device));
    if (g.init && g.device != device && g.tables) {
        // tables live on the old device; drop them, the caller reloads
        (void)hipFree(g.tb_index); (void)hipFree(g.tb_adiabats);
        g.tb_index = g.tb_adiabats = nullptr; g.tables = false;
    }
    if (g.init && g.device != device && g.es_tab) { (void)hipFree(g.es_tab); g.es_tab = nullptr; }
    if (!g.es_tab) {
        std::vector<double> tab(xp::LDS_TAB);
        build_es_table(tab.data());
        HIP_TRY(hipMalloc((void **)&g.es_tab, sizeof(double) * xp::LDS_TAB));
        HIP_TRY(hipMemcpy(g.es_tab, tab.data(), sizeof(double) * xp::LDS_TAB, hipMemcpyHostToDevice));
    }
    if (g.init && g.device != device && g.fam_tab) { (void)hipFree(g.fam_tab); g.fam_tab = nullptr; }
    if (!g.fam_tab) {
        if (g.fam_host.empty()) { g.fam_host.resize((size_t)xp::FAM_SIZE); build_family_table(g.fam_host.data()); }
        HIP_TRY(hipMalloc((void **)&g.fam_tab, sizeof(double) * g.fam_host.size()));
        HIP_TRY(hipMemcpy(g.fam_tab, family_device_layout(g.fam_host).data(), sizeof(double) * g.fam_host.size(), hipMemcpyHostToDevice));
    }
    g.device = device;
    g.init = true;
    return XP_OK;
}

int xp_set_tables(const xp_tables *t) {
    DevGuard dg_;
    int rc = ensure_init();
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g.mu);
    if (!t || !t->index || !t->adiabats || t->n_pressure < 2 || t->n_temperature < 2 || t->n_adiabat < 1)
        return fail(XP_E_ARG, "xp_set_tables: bad tables");
    if (g.tables) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(g.tb_index); (void)hipFree(g.tb_adiabats); g.tables = false; }
    {   // an index entry beyond n_adiabat would send Moist::start outside the adiabat array
        const uint16_t *ix = (const uint16_t *)t->index;
        size_t n_ix = (size_t)t->n_pressure * (size_t)t->n_temperature;
        for (size_t i = 0; i < n_ix; ++i)
            if ((int64_t)ix[i] > t->n_adiabat) return fail(XP_E_ARG, "xp_set_tables: index entry %u > n_adiabat %lld", (unsigned)ix[i], (long long)t->n_adiabat);
    }
    size_t ib = (size_t)t->n_pressure * (size_t)t->n_temperature * 2, ab = (size_t)t->n_adiabat * (size_t)t->n_pressure * 4;
    HIP_TRY(hipMalloc(&g.tb_index, ib));
    HIP_TRY(hipMalloc(&g.tb_adiabats, ab));
    HIP_TRY(hipMemcpy(g.tb_index, t->index, ib, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g.tb_adiabats, t->adiabats, ab, hipMemcpyHostToDevice));
    g.tb.index = (const uint16_t *)g.tb_index; g.tb.adiabats = (const float *)g.tb_adiabats;
    g.tb.n_p = t->n_pressure; g.tb.n_t = t->n_temperature;
    g.tb.p_max = t->p_max; g.tb.p_step = t->p_step; g.tb.t_min = t->t_min; g.tb.t_step = t->t_step;
    g.tables = true;
    return XP_OK;
}
int xp_tables_loaded(void) { return g.tables ? 1 : 0; }

int xp_family_table(double *out, int64_t *n_lnp, int64_t *n_label) {
    DevGuard dg_;
    int rc = ensure_init();
    if (rc) return rc;
    if (n_lnp) *n_lnp = xp::FAM_COEFS / xp::FAM_NPS;
    if (n_label) *n_label = xp::FAM_NPS;
    if (out) memcpy(out, g.fam_host.data(), sizeof(double) * xp::FAM_COEFS);
    return XP_OK;
}
int xp_set_family_table(const double *tab, int64_t n_lnp, int64_t n_label) {
    DevGuard dg_;
    int rc = ensure_init();
    if (rc) return rc;
    if (!tab || n_lnp != xp::FAM_COEFS / xp::FAM_NPS || n_label != xp::FAM_NPS) return fail(XP_E_ARG, "xp_set_family_table: wrong shape");
    std::lock_guard<std::mutex> lk(g.mu);
    HIP_TRY(hipDeviceSynchronize());                         // kernels in flight may still read the old table
    memcpy(g.fam_host.data(), tab, sizeof(double) * xp::FAM_COEFS);
    HIP_TRY(hipMemcpy(g.fam_tab, family_device_layout(g.fam_host).data(), sizeof(double) * g.fam_host.size(), hipMemcpyHostToDevice));
    return XP_OK;
}

int xp_cape_cin(const xp_view *p, const xp_view *t, const xp_view *td, const xp_parcel *parcel, const xp_opts *o,
                xp_scalars_out *scalars, xp_profile_out *profile, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    const xp_opts oo = o ? *o : default_opts();
    xp::CapeArgs a;
    int32_t *flags;
    int rc;
    const bool f32 = oo.compute == XP_F32;                   // (held to its contract before anything is staged or looked up)
    if (f32 && ((rc = check_cape(p, t, td, 1, parcel, oo, true, true, true, true)) || (rc = check_compute32(p, parcel, oo, scalars, profile)))) return rc;
    const int layer = layer_of(oo);
    if (layer && profile) return fail(XP_E_ARG, "xp_cape_cin: XP_OPT_LAYER_*: profile must be NULL (the profile does not depend on the choice)");
    if ((rc = fill_common(st, p, t, td, parcel, oo, &a, true, true, true, profile == nullptr)) || (rc = stage_cape_out(st, p->dtype, scalars, profile, &a)) ||
        (rc = family_flags(st, oo, a.ncol, &flags))) return rc;
    if (f32) cape_pass32(st, a, flags);
    else if (parcel->mode == XP_PARCEL_MAX_CAPE) {           // the surface call on the columns from k* on
        int32_t *kstar;
        if ((rc = max_cape_front(st, *parcel, p, &a, &kstar))) return rc;
        cape_pass(st, a, p->dtype, XP_PARCEL_SURFACE, profile != nullptr, flags, layer);
        if ((rc = copy_kstar(st, kstar, a))) return rc;
    } else cape_pass(st, a, p->dtype, parcel_mode(*parcel), profile != nullptr, flags, layer);
    return st.finish();
}

int xp_cape_cin_multi(const xp_view *p, const xp_view *t, const xp_view *td, int32_t np, const xp_parcel *parcels,
                      const xp_opts *o, xp_scalars_out *scalars, xp_profile_out *profiles, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    if (np < 1 || np > xp::MULTI_MAX) return fail(XP_E_ARG, "xp_cape_cin_multi: 1...%d parcels", xp::MULTI_MAX);
    if (!parcels || !scalars) return fail(XP_E_ARG, "xp_cape_cin_multi: null parcels / scalars");
    const xp_opts oo = o ? *o : default_opts();
    xp::CapeArgs a, pa[xp::MULTI_MAX];
    int rc;
    // every parcel is checked, and its outputs staged, before anything runs; p / T / Td are staged once
    const int layer = layer_of(oo);
    if (layer && profiles) return fail(XP_E_ARG, "xp_cape_cin_multi: XP_OPT_LAYER_*: profiles must be NULL (a profile does not depend on the choice)");
    if ((rc = check_cape(p, t, td, np, parcels, oo, false, true, true, profiles == nullptr)) ||
        (rc = stage_cape(st, p, t, td, oo, &a, over_ground(parcels[0]) ? parcels : nullptr))) return rc;   // re-based once per call
    for (int i = 0; i < np; ++i) {
        pa[i] = a;
        if ((rc = set_parcel(st, parcels[i], p, &pa[i])) ||
            (rc = stage_cape_out(st, p->dtype, &scalars[i], profiles ? &profiles[i] : nullptr, &pa[i]))) return rc;
    }
    const int64_t ncol = a.ncol;
    if (layer || !multi_fused_ok(np, parcels, oo, profiles)) {   // one pass per parcel
        int32_t *flags;
        if ((rc = family_flags(st, oo, ncol, &flags))) return rc;
        for (int i = 0; i < np; ++i) {
            const bool mc = parcels[i].mode == XP_PARCEL_MAX_CAPE;           // its own selection and re-based views of the shared grid
            int32_t *kstar = nullptr;
            if (mc && (rc = max_cape_front(st, parcels[i], p, &pa[i], &kstar))) return rc;
            cape_pass(st, pa[i], p->dtype, mc ? XP_PARCEL_SURFACE : parcel_mode(parcels[i]), profiles != nullptr, flags, layer);
            if ((rc = copy_kstar(st, kstar, pa[i]))) return rc;
        }
        return st.finish();
    }
    xp::MultiArgs m;
    memset(&m, 0, sizeof(m));
    m.base = a;
    m.np = np;
    for (int i = 0; i < np; ++i) {
        m.mode[i] = parcel_mode(parcels[i]);                                 // XP_PARCEL_* == xp::PM_*
        m.depth[i] = parcels[i].depth;
        m.s[i] = pa[i].s;
    }
    if (ncol == 0) return st.finish();
    int32_t *flags;
    if ((rc = st.alloc(sizeof(int32_t) * (size_t)ncol * (size_t)np, &flags))) return rc;
    for (int i = 0; i < np; ++i) m.flags[i] = flags + (size_t)i * (size_t)ncol;
    m.base.persist = persist(-1, ncol);
    with_type(p->dtype == XP_F64, [&](auto z) {
        using T = decltype(z);
        xp::launch_cape_multi<T, 2>(m, st.s);
        // columns a chain's family table could not serve: the single-parcel RK4 kernel redoes them, chain by chain
        for (int i = 0; i < np; ++i) {
            xp::CapeArgs b = pa[i];
            b.flags = m.flags[i]; b.only_flagged = 1;
            xp::launch_cape_mode<T, 0>(b, m.mode[i], false, st.s);
        }
    });
    return st.finish();
}

int xp_conv_properties(const xp_conv_in *in, const xp_opts *o, int32_t ignore_nans, xp_conv_out *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    if (!in || !out) return fail(XP_E_ARG, "xp_conv_properties: null argument");
    const xp_view *p = in->pressure, *t = in->temperature, *q = in->specific_humidity, *z = in->height_asl;
    const xp_view *wu = in->wind_u, *wv = in->wind_v, *wh = in->wind_height_above_surface;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {q, "specific_humidity"}, {z, "height_asl"}})) ||
        (rc = check_views({{wu, "wind_u"}, {wv, "wind_v"}, {wh, "wind_height_above_surface"}}))) return rc;
    if (wu->ncol != p->ncol || wu->dtype != p->dtype)
        return fail(XP_E_ARG, "xp_conv_properties: pressure/wind_u: views differ in columns or dtype");
    // all seven views are staged with pressure's mem: every one of them must live there
    for (const Arg &x : {Arg{t, "temperature"}, Arg{q, "specific_humidity"}, Arg{z, "height_asl"}, Arg{wu, "wind_u"}, Arg{wv, "wind_v"},
                         Arg{wh, "wind_height_above_surface"}})
        if (x.v->mem != p->mem) return fail(XP_E_ARG, "xp_conv_properties: pressure/%s: views differ in mem", x.name);
    if (!in->surface_wind_u || !in->surface_wind_v) return fail(XP_E_ARG, "xp_conv_properties: null surface wind");
    const int64_t nlev = p->nlev, ncol = p->ncol;
    const size_t cb = rows_bytes(p, 1);
    const int mem = p->mem;
    xp_opts oo = o ? *o : default_opts();
    oo.humidity = XP_HUM_DEWPOINT;
    if ((rc = check_opts(oo))) return rc;
    if (ncol == 0) return XP_OK;
    // inputs on the device (host views are dense by contract: staged as they are)
    xp_view dv[7];
    const xp_view *src[7] = {p, t, q, z, wu, wv, wh};
    for (int i = 0; i < 7; ++i) {
        dv[i] = *src[i];
        const void *d;
        if ((rc = st.in(src[i]->data, rows_bytes(src[i], src[i]->nlev), mem, &d))) return rc;
        dv[i].data = d; dv[i].mem = XP_MEM_DEVICE;
    }
    const void *sfu, *sfv;
    if ((rc = st.in(in->surface_wind_u, cb, mem, &sfu)) || (rc = st.in(in->surface_wind_v, cb, mem, &sfv))) return rc;
    // scratch: the dewpoint grid and per-point temporaries
    void *td, *tmp;
    int32_t *valid;
    enum { T850, T700, T500, TD850, Z700, Z500, HIU, HIV, MUP, MUTD, NTMP };
    if ((rc = st.alloc((size_t)nlev * cb, &td)) || (rc = st.alloc((size_t)NTMP * cb, &tmp)) || (rc = st.alloc((size_t)ncol * 4, &valid))) return rc;
    auto tp = [&](int i) { return (void *)((char *)tmp + (size_t)i * cb); };
    // outputs: the caller's buffers when they live on the device, staged otherwise; results that are also inputs of the
    // per-point kernel need a buffer even when the caller does not want them
    void *o_[21];
    void *const want[21] = {out->mu_cape, out->mu_cin, out->mu_mixing_ratio, out->mu_lifted_index, out->mu_dci,
                            out->mixed_100_cape, out->mixed_100_cin, out->mixed_100_lifted_index, out->mixed_100_dci,
                            out->mixed_50_cape, out->mixed_50_cin, out->mixed_50_lifted_index, out->mixed_50_dci,
                            out->lapse_rate_700_500, out->temp_500, out->freezing_level, out->melting_level,
                            out->shear_u, out->shear_v, out->shear_magnitude, (void *)out->positive_shear};
    for (int i = 0; i < 21; ++i) {
        const size_t b = i == 20 ? (size_t)ncol * 4 : cb;
        if ((rc = want[i] ? st.out(want[i], b, mem, &o_[i]) : st.alloc(b, &o_[i]))) return rc;
    }
    enum { O_MU_CAPE, O_MU_CIN, O_MU_W, O_MU_LI, O_MU_DCI, O_M1_CAPE, O_M1_CIN, O_M1_LI, O_M1_DCI, O_M5_CAPE, O_M5_CIN, O_M5_LI, O_M5_DCI,
           O_LAPSE, O_T500, O_FRZ, O_MLT, O_SHU, O_SHV, O_SHM, O_POS };
    // 1. one pass over the four grids
    xp::ConvColumnsArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.p = {dv[0].data, dv[0].lev_stride, dv[0].col_stride}; ca.t = {dv[1].data, dv[1].lev_stride, dv[1].col_stride};
    ca.q = {dv[2].data, dv[2].lev_stride, dv[2].col_stride}; ca.z = {dv[3].data, dv[3].lev_stride, dv[3].col_stride};
    ca.nlev = nlev; ca.ncol = ncol; ca.td = td;
    ca.t850 = tp(T850); ca.t700 = tp(T700); ca.t500 = tp(T500); ca.td850 = tp(TD850); ca.z700 = tp(Z700); ca.z500 = tp(Z500);
    ca.freezing = o_[O_FRZ]; ca.melting = o_[O_MLT]; ca.valid = valid;
    with_type(p->dtype == XP_F64, [&](auto z_) { launch_columns(xp::k_conv_columns<decltype(z_)>, ncol, st.s, ca); });
    // 2. the three parcels (pf.py:1984-2006), lifted index out of the same passes
    xp_view tdv = dv[0];
    tdv.data = td; tdv.lev_stride = ncol; tdv.col_stride = 1;
    xp::CapeArgs a;
    int32_t *flags;
    if ((rc = stage_cape(st, &dv[0], &dv[1], &tdv, oo, &a)) || (rc = family_flags(st, oo, ncol, &flags))) return rc;
    const struct { int mode; double depth; int cape, cin, li; } pc[3] = {{XP_PARCEL_MOST_UNSTABLE, 250.0, O_MU_CAPE, O_MU_CIN, O_MU_LI},
                                                                        {XP_PARCEL_MIXED_LAYER, 100.0, O_M1_CAPE, O_M1_CIN, O_M1_LI},
                                                                        {XP_PARCEL_MIXED_LAYER, 50.0, O_M5_CAPE, O_M5_CIN, O_M5_LI}};
    for (int i = 0; i < 3; ++i) {
        xp_scalars_out so;
        memset(&so, 0, sizeof(so));
        so.dtype = p->dtype; so.mem = XP_MEM_DEVICE; so.cape = o_[pc[i].cape]; so.cin = o_[pc[i].cin];
        if (i == 0) { so.parcel_pressure = tp(MUP); so.parcel_dewpoint = tp(MUTD); }
        xp_profile_out po;
        memset(&po, 0, sizeof(po));
        po.dtype = p->dtype; po.mem = XP_MEM_DEVICE; po.nlev_out = nlev + 1; po.lev_stride = ncol; po.col_stride = 1;
        po.lifted_index = o_[pc[i].li]; po.lifted_index_pressure = 500.0;
        xp::CapeArgs b = a;
        b.depth = pc[i].depth;
        if ((rc = stage_cape_out(st, p->dtype, &so, &po, &b))) return rc;
        cape_pass(st, b, p->dtype, pc[i].mode, true, flags);
    }
    // 3. wind at 6000 m above the surface (pf.py:2240-2243: linear interpolation in height)
    {
        const xp_view *vars[2] = {&dv[4], &dv[5]};
        const double at6 = 6000.0;
        void *outs[2] = {tp(HIU), tp(HIV)};
        if ((rc = interp_levels(st, &dv[6], 2, vars, 1, &at6, 0, outs))) return rc;
    }
    // 4. per point
    xp::ConvFinishArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.ncol = ncol; fa.ignore_nans = ignore_nans != 0;
    fa.mu_p = tp(MUP); fa.mu_td = tp(MUTD);
    fa.li[0] = o_[O_MU_LI]; fa.li[1] = o_[O_M1_LI]; fa.li[2] = o_[O_M5_LI];
    fa.t850 = tp(T850); fa.t700 = tp(T700); fa.t500 = tp(T500); fa.td850 = tp(TD850); fa.z700 = tp(Z700); fa.z500 = tp(Z500);
    fa.hi_u = tp(HIU); fa.hi_v = tp(HIV); fa.sfc_u = sfu; fa.sfc_v = sfv; fa.valid = valid;
    fa.cape[0] = o_[O_MU_CAPE]; fa.cape[1] = o_[O_M1_CAPE]; fa.cape[2] = o_[O_M5_CAPE];
    fa.cin[0] = o_[O_MU_CIN]; fa.cin[1] = o_[O_M1_CIN]; fa.cin[2] = o_[O_M5_CIN];
    fa.li_out[0] = o_[O_MU_LI]; fa.li_out[1] = o_[O_M1_LI]; fa.li_out[2] = o_[O_M5_LI];
    fa.freezing = o_[O_FRZ]; fa.melting = o_[O_MLT];
    fa.mu_mixing_ratio = o_[O_MU_W]; fa.dci[0] = o_[O_MU_DCI]; fa.dci[1] = o_[O_M1_DCI]; fa.dci[2] = o_[O_M5_DCI];
    fa.lapse = o_[O_LAPSE]; fa.temp_500 = o_[O_T500]; fa.shear_u = o_[O_SHU]; fa.shear_v = o_[O_SHV]; fa.shear_mag = o_[O_SHM];
    fa.positive_shear = (int32_t *)o_[O_POS];
    with_type(p->dtype == XP_F64, [&](auto z_) { launch_columns(xp::k_conv_finish<decltype(z_)>, ncol, st.s, fa); });
    return st.finish();
}

int xp_select_parcel(const xp_view *p, const xp_view *t, const xp_view *td, const xp_parcel *parcel,
                     xp_scalars_out *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    xp::CapeArgs a;
    int rc;
    if ((rc = fill_common(st, p, t, td, parcel, default_opts(), &a, false, true, true))) return rc;
    if (parcel->mode == XP_PARCEL_MAX_CAPE) {                // the selection alone, with the default options and RK4
        if ((rc = stage_scalars(st, out, a.ncol, &a.s)) || (rc = max_cape_select(st, *parcel, a, p, &a.s, nullptr))) return rc;
        return st.finish();
    }
    if (parcel_mode(*parcel) != XP_PARCEL_MOST_UNSTABLE && parcel_mode(*parcel) != XP_PARCEL_MIXED_LAYER)
        return fail(XP_E_ARG, "xp_select_parcel: mode must be most-unstable or mixed-layer");
    if ((rc = stage_scalars(st, out, a.ncol, &a.s))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) { with_one_of<xp::PM_MU, xp::PM_ML>(parcel_mode(*parcel), [&](auto PM) {
        launch_columns(xp::k_select_parcel<decltype(z), PM()>, a.ncol, st.s, a);
    }); });
    return st.finish();
}

int xp_mixed_layer(const xp_view *p, const xp_view *v, double depth, void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {v, "variable"}}))) return rc;
    if (!out) return fail(XP_E_ARG, "xp_mixed_layer: null output");
    xp::View pv, vv;
    void *od;
    if ((rc = stage_view(st, p, &pv)) || (rc = stage_view(st, v, &vv)) || (rc = st.out(out, rows_bytes(p, 1), p->mem, &od))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_mixed_layer<decltype(z)>, p->ncol, st.s, pv, vv, p->nlev, p->ncol, depth, od, (int)(p->dtype == XP_F64)); });
    return st.finish();
}

int xp_lcl(int64_t n, int32_t dtype, int32_t mem, const void *pp, const void *pt, const void *ptd, void *lp, void *lt,
           void *ltv, int32_t *status, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    if (n < 0 || !pp || !pt || !ptd) return fail(XP_E_ARG, "xp_lcl: null input");
    if (dtype != XP_F32 && dtype != XP_F64) return fail(XP_E_ARG, "xp_lcl: bad dtype");
    size_t b = (size_t)n * esize(dtype);
    const void *dp, *dt, *dtd;
    void *op, *ot, *otv;
    int32_t *os;
    int rc;
    if ((rc = st.in(pp, b, mem, &dp)) || (rc = st.in(pt, b, mem, &dt)) || (rc = st.in(ptd, b, mem, &dtd)) ||
        (rc = st.out(lp, b, mem, &op)) || (rc = st.out(lt, b, mem, &ot)) || (rc = st.out(ltv, b, mem, &otv)) ||
        (rc = st.out(status, (size_t)n * 4, mem, &os))) return rc;
    with_type(dtype == XP_F64, [&](auto z) { launch_columns(xp::k_lcl<decltype(z)>, n, st.s, n, dp, dt, dtd, op, ot, otv, os); });
    return st.finish();
}

int xp_dry_lapse(const xp_view *p, const void *pt, const void *pp, void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_view(p, "pressure"))) return rc;
    if (!pt || !out) return fail(XP_E_ARG, "xp_dry_lapse: null argument");
    xp::View pv;
    const void *dt, *dp;
    void *od;
    if ((rc = stage_view(st, p, &pv)) || (rc = st.in(pt, rows_bytes(p, 1), p->mem, &dt)) || (rc = st.in(pp, rows_bytes(p, 1), p->mem, &dp)) ||
        (rc = st.out(out, rows_bytes(p, p->nlev), p->mem, &od))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_dry_lapse<decltype(z)>, p->ncol, st.s, pv, p->nlev, p->ncol, dt, dp, out_like(od, p)); });
    return st.finish();
}

// component entry points: XP_MOIST_FAMILY is served by the RK4 stepper of their kernels
int xp_moist_lapse(const xp_view *p, const void *pt, const void *pp, int32_t moist_mode, void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_view(p, "pressure"))) return rc;
    if (!pt || !out) return fail(XP_E_ARG, "xp_moist_lapse: null argument");
    const int tm = moist_mode == XP_MOIST_TABLE;
    TableSet ts;
    xp::View pv;
    const void *dt, *dp;
    void *od;
    if ((rc = snapshot_tables(tm, &ts)) || (rc = stage_view(st, p, &pv)) || (rc = st.in(pt, rows_bytes(p, 1), p->mem, &dt)) ||
        (rc = st.in(pp, rows_bytes(p, 1), p->mem, &dp)) || (rc = st.out(out, rows_bytes(p, p->nlev), p->mem, &od))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) {
        launch_columns(xp::k_moist_lapse<decltype(z)>, p->ncol, st.s, pv, p->nlev, p->ncol, dt, dp, tm, ts.tb, ts.es, out_like(od, p));
    });
    return st.finish();
}

int xp_parcel_profile(const xp_view *p, const void *pp, const void *pt, const void *ptd, int32_t moist_mode,
                      void *t_out, void *tv_out, void *lp, void *lt, void *ltv, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_view(p, "pressure"))) return rc;
    if (!pp || !pt || !ptd) return fail(XP_E_ARG, "xp_parcel_profile: null parcel");
    const int tm = moist_mode == XP_MOIST_TABLE;
    TableSet ts;
    xp::View pv;
    const size_t cb = rows_bytes(p, 1), fb = rows_bytes(p, p->nlev);
    const void *dpp, *dpt, *dptd;
    void *d1, *d2, *d3, *d4, *d5;
    if ((rc = snapshot_tables(tm, &ts)) || (rc = stage_view(st, p, &pv)) || (rc = st.in(pp, cb, p->mem, &dpp)) ||
        (rc = st.in(pt, cb, p->mem, &dpt)) || (rc = st.in(ptd, cb, p->mem, &dptd)) || (rc = st.out(t_out, fb, p->mem, &d1)) ||
        (rc = st.out(tv_out, fb, p->mem, &d2)) || (rc = st.out(lp, cb, p->mem, &d3)) || (rc = st.out(lt, cb, p->mem, &d4)) ||
        (rc = st.out(ltv, cb, p->mem, &d5))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) {
        launch_columns(xp::k_parcel_profile<decltype(z)>, p->ncol, st.s, pv, p->nlev, p->ncol, dpp, dpt, dptd, tm, ts.tb, ts.es,
               out_like(d1, p), out_like(d2, p), d3, d4, d5);
    });
    return st.finish();
}

int xp_lfc_el(const xp_view *p, const xp_view *par, const xp_view *env, const void *lcl_p, const void *lcl_t,
              xp_scalars_out *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {par, "parcel_temperature"}, {env, "temperature"}}))) return rc;
    if (!lcl_p || !lcl_t || !out) return fail(XP_E_ARG, "xp_lfc_el: null argument");
    xp::View pv, pav, ev;
    xp::ScalarsOut so;
    const void *dlp, *dlt;
    if ((rc = stage_view(st, p, &pv)) || (rc = stage_view(st, par, &pav)) || (rc = stage_view(st, env, &ev)) ||
        (rc = st.in(lcl_p, rows_bytes(p, 1), p->mem, &dlp)) || (rc = st.in(lcl_t, rows_bytes(p, 1), p->mem, &dlt)) ||
        (rc = stage_scalars(st, out, p->ncol, &so))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_lfc_el<decltype(z)>, p->ncol, st.s, pv, pav, ev, p->nlev, p->ncol, dlp, dlt, so); });
    return st.finish();
}

int xp_cape_cin_base(const xp_view *p, const xp_view *env, const xp_view *par, const void *lfc_p, const void *el_p,
                     const xp_opts *o, void *cape, void *cin, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {par, "parcel_temperature"}, {env, "temperature"}}))) return rc;
    if (!lfc_p || !el_p) return fail(XP_E_ARG, "xp_cape_cin_base: null argument");
    if (o && layer_of(*o)) return fail(XP_E_ARG, "xp_cape_cin_base: xp_opts.flags: XP_OPT_LAYER_* is honoured by xp_cape_cin and xp_cape_cin_multi only");
    xp::View pv, pav, ev;
    const size_t cb = rows_bytes(p, 1);
    const void *dl, *de;
    void *dc, *dn;
    if ((rc = stage_view(st, p, &pv)) || (rc = stage_view(st, par, &pav)) || (rc = stage_view(st, env, &ev)) ||
        (rc = st.in(lfc_p, cb, p->mem, &dl)) || (rc = st.in(el_p, cb, p->mem, &de)) || (rc = st.out(cape, cb, p->mem, &dc)) ||
        (rc = st.out(cin, cb, p->mem, &dn))) return rc;
    const xp_opts oo = o ? *o : default_opts();
    with_type(p->dtype == XP_F64, [&](auto z) {
        launch_columns(xp::k_cape_cin_base<decltype(z)>, p->ncol, st.s, pv, ev, pav, p->nlev, p->ncol, dl, de, oo.pos_cape_neg_cin, oo.post_zero_cin, dc, dn);
    });
    return st.finish();
}

int xp_wet_bulb_temperature(const xp_view *p, const xp_view *t, const xp_view *td, int32_t moist_mode, void *out,
                            void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {td, "dewpoint"}}))) return rc;
    if (!out) return fail(XP_E_ARG, "xp_wet_bulb_temperature: null output");
    const int tm = moist_mode == XP_MOIST_TABLE;
    TableSet ts;
    xp::View pv, tv, tdv;
    void *od;
    if ((rc = snapshot_tables(tm, &ts)) || (rc = stage_view(st, p, &pv)) || (rc = stage_view(st, t, &tv)) ||
        (rc = stage_view(st, td, &tdv)) || (rc = st.out(out, rows_bytes(p, p->nlev), p->mem, &od))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) {
        launch_columns(xp::k_wet_bulb<decltype(z)>, p->nlev * p->ncol, st.s, pv, tv, tdv, p->nlev, p->ncol, tm, ts.tb, ts.es, out_like(od, p));
    });
    return st.finish();
}

int xp_downdraft_cape(const xp_view *p, const xp_view *t, const xp_view *td, double layer_bottom, double layer_depth,
                      int32_t moist_mode, xp_dcape_out *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {td, "dewpoint"}}))) return rc;
    if ((rc = check_out("xp_downdraft_cape", out, p))) return rc;
    if (!(std::isfinite(layer_bottom) && layer_bottom > 0.0))
        return fail(XP_E_ARG, "xp_downdraft_cape: layer_bottom must be finite and positive");
    if (!(layer_depth > 0.0 && layer_depth < layer_bottom))
        return fail(XP_E_ARG, "xp_downdraft_cape: layer_depth must lie in (0, layer_bottom)");
    if (moist_mode != XP_MOIST_EXACT && moist_mode != XP_MOIST_TABLE && moist_mode != XP_MOIST_FAMILY)
        return fail(XP_E_ARG, "xp_downdraft_cape: moist_mode: unknown mode %d", (int)moist_mode);
    const int tm = moist_mode == XP_MOIST_TABLE;
    const size_t cb = rows_bytes(p, 1);
    TableSet ts;
    xp::DcapeArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = snapshot_tables(tm, &ts)) || (rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, t, &a.t)) ||
        (rc = stage_view(st, td, &a.td)) || (rc = st.out(out->dcape, cb, out->mem, &a.dcape)) ||
        (rc = st.out(out->start_pressure, cb, out->mem, &a.p0)) || (rc = st.out(out->start_temperature, cb, out->mem, &a.t0)) ||
        (rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status)) ||
        (rc = st.out(out->parcel_temperature, rows_bytes(p, p->nlev), out->mem, &a.prof))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol;
    a.bottom = layer_bottom; a.top = layer_bottom - layer_depth;
    a.table_mode = tm; a.tb = ts.tb; a.es_tab = ts.es;
    with_type(p->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_downdraft_cape<decltype(z)>, p->ncol, st.s, a); });
    return st.finish();
}

int xp_effective_inflow_layer(const xp_view *p, const xp_view *t, const xp_view *td, const xp_view *z, double cape_min,
                              double cin_min, double search_depth, const xp_opts *o, xp_effective_layer_out *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    const xp_opts opts = o ? *o : default_opts();
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {td, "dewpoint"}})) || (rc = check_opts(opts))) return rc;
    if (z && (rc = check_views({{p, "pressure"}, {z, "height"}}))) return rc;
    if ((rc = check_out("xp_effective_inflow_layer", out, p))) return rc;
    if (opts.humidity == XP_HUM_SPECIFIC) return fail(XP_E_ARG, "xp_effective_inflow_layer: humidity must be XP_HUM_DEWPOINT");
    if (!(std::isfinite(cape_min) && std::isfinite(cin_min))) return fail(XP_E_ARG, "xp_effective_inflow_layer: cape_min and cin_min must be finite");
    if (!(std::isfinite(search_depth) && search_depth > 0.0)) return fail(XP_E_ARG, "xp_effective_inflow_layer: search_depth must be finite and positive");
    const int tm = opts.moist_mode == XP_MOIST_TABLE;
    const size_t cb = rows_bytes(p, 1), ib = (size_t)p->ncol * 4;
    TableSet ts;
    xp::EffectiveArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = snapshot_tables(tm, &ts)) || (rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, t, &a.t)) ||
        (rc = stage_view(st, td, &a.td)) || (rc = dewpoint_front(st, p, opts, a.p, a.t, &a.td)) || (z && (rc = stage_view(st, z, &a.z))) ||
        (rc = st.out(out->base_pressure, cb, out->mem, &a.base_p)) || (rc = st.out(out->top_pressure, cb, out->mem, &a.top_p)) ||
        (rc = st.out(out->base_height, cb, out->mem, &a.base_z)) || (rc = st.out(out->top_height, cb, out->mem, &a.top_z)) ||
        (rc = st.out(out->base_index, ib, out->mem, &a.base_idx)) || (rc = st.out(out->top_index, ib, out->mem, &a.top_idx)) ||
        (rc = st.out(out->status, ib, out->mem, &a.status)) ||
        (rc = st.out(out->candidate_cape, rows_bytes(p, p->nlev), out->mem, &a.cand_cape)) ||
        (rc = st.out(out->candidate_cin, rows_bytes(p, p->nlev), out->mem, &a.cand_cin))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol;
    a.cape_min = cape_min; a.cin_min = cin_min; a.depth = search_depth;
    a.vtc = opts.virtual_temperature_correction; a.log_interp = opts.lcl_interp == XP_LCL_INTERP_LOG;
    a.pos_neg = opts.pos_cape_neg_cin; a.post_zero = opts.post_zero_cin;
    a.tb = ts.tb; a.es_tab = ts.es;
    xp::launch_effective_inflow(a, p->dtype == XP_F64, tm != 0, st.s);
    return st.finish();
}

int xp_cape_cin_layers(const xp_view *p, const xp_view *t, const xp_view *td, const xp_parcel *parcel, const xp_opts *o,
                       int32_t nlayer, const void *const *bottom, const void *const *top, xp_cape_layers_out *out, void *stream) {
    const char *const entry = "xp_cape_cin_layers";
    Entry st(stream);
    if (st.rc) return st.rc;
    const xp_opts opts = o ? *o : default_opts();
    int rc;
    xp::CapeLayersArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = check_cape(p, t, td, 1, parcel, opts)) || (rc = check_out(entry, out, p))) return rc;
    if (opts.humidity == XP_HUM_SPECIFIC) return fail(XP_E_ARG, "%s: humidity must be XP_HUM_DEWPOINT", entry);
    if (!opts.pos_cape_neg_cin) return fail(XP_E_ARG, "%s: layers are defined for pos_cape_neg_cin only", entry);
    if (nlayer < 1 || nlayer > xp::CL_MAX_LAYERS) return fail(XP_E_ARG, "%s: nlayer must lie in 1 ... 4, got %d", entry, (int)nlayer);
    if (!top) return fail(XP_E_ARG, "%s: top: null", entry);
    for (int i = 0; i < nlayer; ++i)
        if (!top[i]) return fail(XP_E_ARG, "%s: top[%d]: null", entry, i);
    if ((rc = stage_cape(st, p, t, td, opts, &a.base)) || (rc = set_parcel(st, *parcel, p, &a.base))) return rc;
    const size_t cb = rows_bytes(p, 1);
    for (int i = 0; i < nlayer; ++i)
        if ((rc = st.in(bottom ? bottom[i] : nullptr, cb, p->mem, &a.bottom[i])) || (rc = st.in(top[i], cb, p->mem, &a.top[i])) ||
            (rc = st.out(out->cape[i], cb, out->mem, &a.cape[i])) || (rc = st.out(out->cin[i], cb, out->mem, &a.cin[i]))) return rc;
    if ((rc = st.out(out->total_cape, cb, out->mem, &a.total_cape)) || (rc = st.out(out->total_cin, cb, out->mem, &a.total_cin)) ||
        (rc = st.out(out->lfc_pressure, cb, out->mem, &a.lfc_p)) || (rc = st.out(out->el_pressure, cb, out->mem, &a.el_p)) ||
        (rc = st.out(out->lcl_pressure, cb, out->mem, &a.lcl_p)) ||
        (rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.pmode = parcel->mode == XP_PARCEL_SURFACE ? xp::PM_SURFACE : parcel->mode == XP_PARCEL_MOST_UNSTABLE ? xp::PM_MU
            : parcel->mode == XP_PARCEL_MIXED_LAYER ? xp::PM_ML : xp::PM_EXPLICIT;
    a.nlayer = nlayer;
    xp::launch_cape_layers(a, p->dtype == XP_F64, a.base.table_mode != 0, st.s);
    return st.finish();
}

int xp_bunkers_storm_motion(const xp_view *p, const xp_view *u, const xp_view *v, const xp_view *z, xp_storm_motion_out *out,
                            void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {u, "u"}, {v, "v"}, {z, "height"}}))) return rc;
    if ((rc = check_out("xp_bunkers_storm_motion", out, p))) return rc;
    const size_t cb = rows_bytes(p, 1);
    xp::StormMotionArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, u, &a.u)) || (rc = stage_view(st, v, &a.v)) ||
        (rc = stage_view(st, z, &a.z)) || (rc = st.out(out->right_u, cb, out->mem, &a.right_u)) ||
        (rc = st.out(out->right_v, cb, out->mem, &a.right_v)) || (rc = st.out(out->left_u, cb, out->mem, &a.left_u)) ||
        (rc = st.out(out->left_v, cb, out->mem, &a.left_v)) || (rc = st.out(out->mean_u, cb, out->mem, &a.mean_u)) ||
        (rc = st.out(out->mean_v, cb, out->mem, &a.mean_v)) ||
        (rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol;
    with_type(p->dtype == XP_F64, [&](auto t) { launch_columns(xp::k_bunkers_storm_motion<decltype(t)>, p->ncol, st.s, a); });
    return st.finish();
}

int xp_storm_relative_helicity(const xp_view *z, const xp_view *u, const xp_view *v, const void *surface_u,
                               const void *surface_v, const void *storm_u, const void *storm_v, double bottom,
                               int32_t ndepth, const double *depth, xp_srh_out *out, void *stream) {
    const char *const entry = "xp_storm_relative_helicity";
    return helicity<false>(entry, z, u, v, surface_u, surface_v, storm_u, storm_v, ndepth, out, stream, [&](xp::SrhArgs &a) {
        if (ndepth < 1 || ndepth > xp::SRH_MAX_DEPTHS) return fail(XP_E_ARG, "%s: ndepth must lie in 1 ... 4, got %d", entry, (int)ndepth);
        if (!depth) return fail(XP_E_ARG, "%s: depth: null", entry);
        for (int i = 0; i < ndepth; ++i)
            if (!(std::isfinite(depth[i]) && depth[i] > 0.0)) return fail(XP_E_ARG, "%s: depth[%d] must be finite and positive", entry, i);
        if (!(std::isfinite(bottom) && bottom >= 0.0)) return fail(XP_E_ARG, "%s: bottom must be finite and >= 0", entry);
        a.bottom = bottom;
        for (int i = 0; i < ndepth; ++i) a.top[i] = bottom + depth[i];
        return 0;
    });
}

int xp_storm_relative_helicity_layers(const xp_view *z, const xp_view *u, const xp_view *v, const void *surface_u,
                                      const void *surface_v, const void *storm_u, const void *storm_v, const void *bottom,
                                      int32_t nlayer, const void *const *top, xp_srh_layers_out *out, void *stream) {
    const char *const entry = "xp_storm_relative_helicity_layers";
    return helicity<true>(entry, z, u, v, surface_u, surface_v, storm_u, storm_v, nlayer, out, stream, [&](xp::SrhArgs &a) {
        if (nlayer < 1 || nlayer > xp::SRH_MAX_DEPTHS) return fail(XP_E_ARG, "%s: nlayer must lie in 1 ... 4, got %d", entry, (int)nlayer);
        if (!bottom || !top) return fail(XP_E_ARG, "%s: bottom / top: null", entry);
        for (int i = 0; i < nlayer; ++i)
            if (!top[i]) return fail(XP_E_ARG, "%s: top[%d]: null", entry, i);
        a.bottom_col = bottom;
        for (int i = 0; i < nlayer; ++i) a.top_col[i] = top[i];
        return 0;
    });
}

int xp_significant_tornado(int64_t n, int32_t dtype, int32_t mem, const void *sbcape, const void *lcl_height, const void *srh,
                           const void *shear, void *out, void *stream) {
    return per_point<xp::StpOp>("xp_significant_tornado", n, dtype, mem, {sbcape, lcl_height, srh, shear}, 4, {out}, true, stream);
}

int xp_supercell_composite(int64_t n, int32_t dtype, int32_t mem, const void *mucape, const void *srh, const void *shear,
                           void *out, void *stream) {
    return per_point<xp::ScpOp>("xp_supercell_composite", n, dtype, mem, {mucape, srh, shear}, 3, {out}, true, stream);
}

// One layer of an xp_wind_layers / xp_thermo_layers request, checked; *bottom_out, *top_out: its bounds as the kernels take them
// (NaN where bottom_col / top_col replaces the scalar; a NaN bottom height: 0).  allow_open: a NaN top by pressure is the open one.
static int check_layer(const char *entry, int i, const xp_wind_layer &l, bool have_z, const void *bottom_col, const void *top_col,
                       bool allow_open, double *bottom_out, double *top_out) {
    double bottom = bottom_col ? (double)NAN : l.bottom;
    const double top = top_col ? (double)NAN : l.top;
    if (l.kind != XP_LAYER_PRESSURE && l.kind != XP_LAYER_PRESSURE_DEPTH && l.kind != XP_LAYER_HEIGHT)
        return fail(XP_E_ARG, "%s: layers[%d]: unknown kind %d", entry, i, (int)l.kind);
    if ((bottom_col || top_col) && l.kind != XP_LAYER_PRESSURE)
        return fail(XP_E_ARG, "%s: layers[%d]: per-column bounds need kind XP_LAYER_PRESSURE", entry, i);
    // a top that an array replaces is not looked at
    if (!top_col && !std::isfinite(top) && !(allow_open && l.kind == XP_LAYER_PRESSURE && std::isnan(top)))
        return fail(XP_E_ARG, allow_open ? "%s: layers[%d]: top must be finite (or, by pressure, NaN: to the highest valid level)"
                                         : "%s: layers[%d]: top must be finite", entry, i);
    if (std::isinf(bottom)) return fail(XP_E_ARG, "%s: layers[%d]: bottom must be finite or NaN", entry, i);
    if (l.kind == XP_LAYER_PRESSURE_DEPTH && !(top > 0.0)) return fail(XP_E_ARG, "%s: layers[%d]: depth must be positive", entry, i);
    if (l.kind == XP_LAYER_HEIGHT) {
        if (!have_z) return fail(XP_E_ARG, "%s: layers[%d]: a layer by height needs height", entry, i);
        if (std::isnan(bottom)) bottom = 0.0;
        if (bottom < 0.0) return fail(XP_E_ARG, "%s: layers[%d]: bottom height must be >= 0", entry, i);
        if (!(top > bottom)) return fail(XP_E_ARG, "%s: layers[%d]: depth must be positive (top above bottom)", entry, i);
    }
    *bottom_out = bottom; *top_out = top;
    return 0;
}

int xp_wind_layers(const xp_view *p, const xp_view *u, const xp_view *v, const xp_view *z, int32_t nlayer,
                   const xp_wind_layer *layers, xp_wind_layers_out *out, void *stream) {
    const char *const entry = "xp_wind_layers";
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {u, "u"}, {v, "v"}}))) return rc;
    if (z && (rc = check_views({{p, "pressure"}, {z, "height"}}))) return rc;
    if ((rc = check_out(entry, out, p))) return rc;
    if (nlayer < 1 || nlayer > xp::WL_MAX_LAYERS) return fail(XP_E_ARG, "%s: nlayer must lie in 1 ... 4, got %d", entry, (int)nlayer);
    if (!layers) return fail(XP_E_ARG, "%s: layers: null", entry);
    xp::WindLayersArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nlayer; ++i) {
        if ((rc = check_layer(entry, i, layers[i], z != nullptr, nullptr, nullptr, false, &a.bottom[i], &a.top[i]))) return rc;
        a.kind[i] = layers[i].kind;
    }
    const size_t cb = rows_bytes(p, 1);
    if ((rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, u, &a.u)) || (rc = stage_view(st, v, &a.v)) ||
        (z && (rc = stage_view(st, z, &a.z)))) return rc;
    bool want_max = false;
    for (int i = 0; i < nlayer; ++i) {
        if ((rc = st.out(out->mean_u[i], cb, out->mem, &a.mean_u[i])) || (rc = st.out(out->mean_v[i], cb, out->mem, &a.mean_v[i])) ||
            (rc = st.out(out->shear_u[i], cb, out->mem, &a.shear_u[i])) || (rc = st.out(out->shear_v[i], cb, out->mem, &a.shear_v[i])) ||
            (rc = st.out(out->bottom_u[i], cb, out->mem, &a.bottom_u[i])) || (rc = st.out(out->bottom_v[i], cb, out->mem, &a.bottom_v[i])) ||
            (rc = st.out(out->max_u[i], cb, out->mem, &a.max_u[i])) || (rc = st.out(out->max_v[i], cb, out->mem, &a.max_v[i])) ||
            (rc = st.out(out->max_pressure[i], cb, out->mem, &a.max_p[i]))) return rc;
        want_max = want_max || a.max_u[i] || a.max_v[i] || a.max_p[i];
    }
    if ((rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol; a.n = nlayer;
    xp::launch_wind_layers(a, p->dtype == XP_F64, want_max, st.s);
    return st.finish();
}

int xp_thermo_layers(const xp_view *p, const xp_view *t, const xp_view *td, const xp_view *z, int32_t nlayer,
                     const xp_wind_layer *layers, const void *const *bottom_columns, const void *const *top_columns,
                     xp_thermo_layers_out *out, void *stream) {
    const char *const entry = "xp_thermo_layers";
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_view(p, "pressure"))) return rc;
    if (t && (rc = check_views({{p, "pressure"}, {t, "temperature"}}))) return rc;
    if (td && (rc = check_views({{p, "pressure"}, {td, "dewpoint"}}))) return rc;
    if (z && (rc = check_views({{p, "pressure"}, {z, "height"}}))) return rc;
    if ((rc = check_out(entry, out, p))) return rc;
    if (nlayer < 1 || nlayer > xp::TL_MAX_LAYERS) return fail(XP_E_ARG, "%s: nlayer must lie in 1 ... 4, got %d", entry, (int)nlayer);
    if (!layers) return fail(XP_E_ARG, "%s: layers: null", entry);
    xp::ThermoLayersArgs a;
    memset(&a, 0, sizeof(a));
    bool colb = false, moist = false, theta = false;
    for (int i = 0; i < nlayer; ++i) {
        const xp_wind_layer &l = layers[i];
        const void *const bc = bottom_columns ? bottom_columns[i] : nullptr, *const tc = top_columns ? top_columns[i] : nullptr;
        if ((rc = check_layer(entry, i, l, z != nullptr, bc, tc, true, &a.bottom[i], &a.top[i]))) return rc;
        a.kind[i] = l.kind; a.open[i] = l.kind == XP_LAYER_PRESSURE && !tc && std::isnan(a.top[i]);
        colb = colb || bc || tc;
        // what each wanted output reads
        const bool rh = out->mean_relative_humidity[i] != nullptr, lapse = out->lapse_rate[i] != nullptr;
        const bool th = out->theta_e_min[i] || out->theta_e_min_pressure[i] || out->theta_e_max[i] || out->theta_e_max_pressure[i];
        const bool sums = out->precipitable_water[i] || out->mean_mixing_ratio[i] || rh;
        if (!t && (rh || lapse || th))
            return fail(XP_E_ARG, "%s: layers[%d]: mean_relative_humidity, lapse_rate and theta_e_* need temperature", entry, i);
        if (!td && (sums || th))
            return fail(XP_E_ARG, "%s: layers[%d]: every output except thickness and lapse_rate needs dewpoint", entry, i);
        if (!z && (out->thickness[i] || lapse)) return fail(XP_E_ARG, "%s: layers[%d]: thickness and lapse_rate need height", entry, i);
        moist = moist || sums; theta = theta || th;
        a.want_rh = a.want_rh || rh;
    }
    const size_t cb = rows_bytes(p, 1);
    if ((rc = stage_view(st, p, &a.p)) || (t && (rc = stage_view(st, t, &a.t))) || (td && (rc = stage_view(st, td, &a.td))) ||
        (z && (rc = stage_view(st, z, &a.z)))) return rc;
    for (int i = 0; i < nlayer; ++i) {
        if ((rc = st.in(bottom_columns ? bottom_columns[i] : nullptr, cb, p->mem, &a.bottom_col[i])) ||
            (rc = st.in(top_columns ? top_columns[i] : nullptr, cb, p->mem, &a.top_col[i])) ||
            (rc = st.out(out->precipitable_water[i], cb, out->mem, &a.pw[i])) ||
            (rc = st.out(out->mean_mixing_ratio[i], cb, out->mem, &a.mean_w[i])) ||
            (rc = st.out(out->mean_relative_humidity[i], cb, out->mem, &a.mean_rh[i])) ||
            (rc = st.out(out->thickness[i], cb, out->mem, &a.thickness[i])) || (rc = st.out(out->lapse_rate[i], cb, out->mem, &a.lapse[i])) ||
            (rc = st.out(out->theta_e_min[i], cb, out->mem, &a.th_min[i])) ||
            (rc = st.out(out->theta_e_min_pressure[i], cb, out->mem, &a.th_min_p[i])) ||
            (rc = st.out(out->theta_e_max[i], cb, out->mem, &a.th_max[i])) ||
            (rc = st.out(out->theta_e_max_pressure[i], cb, out->mem, &a.th_max_p[i]))) return rc;
    }
    if ((rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol; a.n = nlayer;
    xp::launch_thermo_layers(a, p->dtype == XP_F64, moist, theta, colb, st.s);
    return st.finish();
}

int xp_sounding_indices(const xp_view *p, const xp_view *t, const xp_view *td, const xp_view *u, const xp_view *v,
                        const xp_sounding_opts *o, xp_sounding_out *out, void *stream) {
    const char *const entry = "xp_sounding_indices";
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {td, "dewpoint"}}))) return rc;
    if ((u != nullptr) != (v != nullptr)) return fail(XP_E_ARG, "%s: u and v must be given together (%s is null)", entry, u ? "v" : "u");
    if (u && (rc = check_views({{p, "pressure"}, {u, "u"}, {v, "v"}}))) return rc;
    if ((rc = check_out(entry, out, p))) return rc;
    if (out->sweat_index && !u) return fail(XP_E_ARG, "%s: sweat_index needs u and v", entry);
    xp_sounding_opts opts;
    memset(&opts, 0, sizeof(opts));
    if (o) opts = *o;
    if (opts.moist_mode != XP_MOIST_EXACT && opts.moist_mode != XP_MOIST_TABLE && opts.moist_mode != XP_MOIST_FAMILY)
        return fail(XP_E_ARG, "%s: moist_mode: unknown mode %d", entry, (int)opts.moist_mode);
    if (opts.ccl_which != XP_CCL_TOP && opts.ccl_which != XP_CCL_BOTTOM)
        return fail(XP_E_ARG, "%s: ccl_which: unknown choice %d", entry, (int)opts.ccl_which);
    if (!(std::isfinite(opts.ccl_mixed_layer_depth) && opts.ccl_mixed_layer_depth >= 0.0))
        return fail(XP_E_ARG, "%s: ccl_mixed_layer_depth must be 0 or finite and positive", entry);
    const bool want_ccl = out->ccl_pressure || out->ccl_temperature || out->convective_temperature;
    const bool wind = out->sweat_index != nullptr;
    const int tm = opts.moist_mode == XP_MOIST_TABLE;
    const size_t cb = rows_bytes(p, 1);
    TableSet ts;
    xp::SoundingArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = snapshot_tables(tm, &ts)) || (rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, t, &a.t)) ||
        (rc = stage_view(st, td, &a.td)) || (wind && ((rc = stage_view(st, u, &a.u)) || (rc = stage_view(st, v, &a.v)))) ||
        (rc = st.out(out->k_index, cb, out->mem, &a.k_index)) || (rc = st.out(out->total_totals, cb, out->mem, &a.total_totals)) ||
        (rc = st.out(out->cross_totals, cb, out->mem, &a.cross_totals)) ||
        (rc = st.out(out->vertical_totals, cb, out->mem, &a.vertical_totals)) ||
        (rc = st.out(out->showalter_index, cb, out->mem, &a.showalter)) || (rc = st.out(out->sweat_index, cb, out->mem, &a.sweat)) ||
        (rc = st.out(out->ccl_pressure, cb, out->mem, &a.ccl_p)) || (rc = st.out(out->ccl_temperature, cb, out->mem, &a.ccl_t)) ||
        (rc = st.out(out->convective_temperature, cb, out->mem, &a.conv_t)) ||
        (rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol;
    a.table_mode = tm; a.which = opts.ccl_which; a.ml_depth = opts.ccl_mixed_layer_depth;
    a.want_index = a.k_index || a.total_totals || a.cross_totals || a.vertical_totals || a.showalter || a.sweat;
    a.tb = ts.tb; a.es_tab = ts.es;
    const int ccl = !want_ccl ? xp::CCL_NONE : opts.ccl_mixed_layer_depth > 0.0 ? xp::CCL_MIXED : xp::CCL_SURFACE;
    xp::launch_sounding(a, p->dtype == XP_F64, wind, ccl, st.s);
    return st.finish();
}

int xp_isentropic_interpolation(const xp_view *p, const xp_view *t, int32_t nvar, const xp_view *const *variables, int32_t nlevel,
                                const double *levels, const xp_isentropic_opts *o, xp_isentropic_out *out, void *stream) {
    const char *const entry = "xp_isentropic_interpolation";
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}}))) return rc;
    if (nvar < 0 || nvar > xp::ISEN_MAX_VARS) return fail(XP_E_ARG, "%s: nvar must lie in 0 ... 4, got %d", entry, (int)nvar);
    if (nvar > 0 && !variables) return fail(XP_E_ARG, "%s: variables: null", entry);
    for (int i = 0; i < nvar; ++i) {
        char name[32];
        snprintf(name, sizeof(name), "variables[%d]", i);
        if ((rc = check_views({{p, "pressure"}, {variables[i], name}}))) return rc;
        if (variables[i]->mem != p->mem) return fail(XP_E_ARG, "%s: %s: mem differs from pressure's", entry, name);
    }
    if (t->mem != p->mem) return fail(XP_E_ARG, "%s: temperature: mem differs from pressure's", entry);
    if ((rc = check_out(entry, out, p))) return rc;
    for (int i = nvar; i < xp::ISEN_MAX_VARS; ++i)
        if (out->vars[i]) return fail(XP_E_ARG, "%s: out: vars[%d] is set, but nvar is %d", entry, i, (int)nvar);
    if (nlevel < 1 || nlevel > xp::ISEN_MAX_LEVELS)
        return fail(XP_E_ARG, "%s: nlevel must lie in 1 ... %d, got %d", entry, xp::ISEN_MAX_LEVELS, (int)nlevel);
    if (!levels) return fail(XP_E_ARG, "%s: levels: null", entry);
    xp::IsentropicLevels lv;
    memset(&lv, 0, sizeof(lv));
    for (int j = 0; j < nlevel; ++j) {
        if (!std::isfinite(levels[j])) return fail(XP_E_ARG, "%s: levels[%d] is not finite", entry, j);
        if (j > 0 && !(levels[j] > levels[j - 1])) return fail(XP_E_ARG, "%s: levels must increase strictly (levels[%d])", entry, j);
        lv.v[j] = levels[j];
    }
    xp_isentropic_opts opts = {1, 50, 1e-6};
    if (o) opts = *o;
    if (opts.max_iters < 1) return fail(XP_E_ARG, "%s: max_iters must be >= 1, got %d", entry, (int)opts.max_iters);
    if (!(std::isfinite(opts.eps) && opts.eps > 0.0)) return fail(XP_E_ARG, "%s: eps must be finite and positive", entry);
    const size_t lb = rows_bytes(p, nlevel);
    xp::IsentropicArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, t, &a.t))) return rc;
    for (int i = 0; i < nvar; ++i)
        if ((rc = stage_view(st, variables[i], &a.v[i])) || (rc = st.out(out->vars[i], lb, out->mem, &a.vars[i]))) return rc;
    if ((rc = st.out(out->pressure, lb, out->mem, &a.pressure)) || (rc = st.out(out->temperature, lb, out->mem, &a.temperature)) ||
        (rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol; a.nlevel = nlevel;
    a.from_below = opts.from_below != 0; a.max_iters = opts.max_iters; a.eps = opts.eps;
    xp::launch_isentropic(a, lv, p->dtype == XP_F64, st.s);
    return st.finish();
}

int xp_hydrostatic_height(const xp_view *p, const xp_view *t, const xp_view *m, const void *base_height, int32_t nlayer,
                          const xp_wind_layer *layers, const xp_hydrostatic_opts *o, xp_hydrostatic_out *out, void *stream) {
    const char *const entry = "xp_hydrostatic_height";
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}}))) return rc;
    if (t->mem != p->mem) return fail(XP_E_ARG, "%s: temperature: mem differs from pressure's", entry);
    if (m && (rc = check_views({{p, "pressure"}, {m, "moisture"}}))) return rc;
    if (m && m->mem != p->mem) return fail(XP_E_ARG, "%s: moisture: mem differs from pressure's", entry);
    xp_hydrostatic_opts opts = {XP_HUM_DEWPOINT, 0};
    if (o) opts = *o;
    if (opts.humidity != XP_HUM_DEWPOINT && opts.humidity != XP_HUM_SPECIFIC)
        return fail(XP_E_ARG, "%s: humidity must be XP_HUM_DEWPOINT or XP_HUM_SPECIFIC, got %d", entry, (int)opts.humidity);
    if ((rc = check_out(entry, out, p))) return rc;
    if (nlayer < 0 || nlayer > xp::HY_MAX_LAYERS) return fail(XP_E_ARG, "%s: nlayer must lie in 0 ... 4, got %d", entry, (int)nlayer);
    if (nlayer > 0 && !layers) return fail(XP_E_ARG, "%s: layers: null", entry);
    for (int i = nlayer; i < xp::HY_MAX_LAYERS; ++i)
        if (out->thickness[i]) return fail(XP_E_ARG, "%s: out: thickness[%d] is set, but nlayer is %d", entry, i, (int)nlayer);
    xp::HydrostaticArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < nlayer; ++i) {
        const xp_wind_layer &l = layers[i];
        if (l.kind == XP_LAYER_HEIGHT) return fail(XP_E_ARG, "%s: layers[%d]: a layer by height is not served here", entry, i);
        if ((rc = check_layer(entry, i, l, false, nullptr, nullptr, true, &a.bottom[i], &a.top[i]))) return rc;
        a.kind[i] = l.kind; a.open[i] = l.kind == XP_LAYER_PRESSURE && std::isnan(a.top[i]);
    }
    const size_t cb = rows_bytes(p, 1);
    if ((rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, t, &a.t)) || (m && (rc = stage_view(st, m, &a.m))) ||
        (rc = st.in(base_height, cb, p->mem, &a.base)) || (rc = st.out(out->height, rows_bytes(p, p->nlev), out->mem, &a.height))) return rc;
    for (int i = 0; i < nlayer; ++i)
        if ((rc = st.out(out->thickness[i], cb, out->mem, &a.thickness[i]))) return rc;
    if ((rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol; a.n = nlayer;
    xp::launch_hydrostatic(a, p->dtype == XP_F64, m ? opts.humidity + 1 : xp::HY_DRY, st.s);
    return st.finish();
}

int xp_geopotential_to_height(int64_t n, int32_t dtype, int32_t mem, const void *geopotential, void *out, void *stream) {
    return per_point<xp::GeopotentialToHeightOp>("xp_geopotential_to_height", n, dtype, mem, {geopotential}, 1, {out}, true, stream);
}

int xp_height_to_geopotential(int64_t n, int32_t dtype, int32_t mem, const void *height, void *out, void *stream) {
    return per_point<xp::HeightToGeopotentialOp>("xp_height_to_geopotential", n, dtype, mem, {height}, 1, {out}, true, stream);
}

int xp_critical_angle(int64_t n, int32_t dtype, int32_t mem, const void *shear_u, const void *shear_v, const void *surface_u,
                      const void *surface_v, const void *storm_u, const void *storm_v, void *out, void *stream) {
    return per_point<xp::CriticalAngleOp>("xp_critical_angle", n, dtype, mem, {shear_u, shear_v, surface_u, surface_v, storm_u, storm_v}, 6,
                                          {out}, true, stream);
}

int xp_corfidi_storm_motion(int64_t n, int32_t dtype, int32_t mem, const void *mean_u, const void *mean_v, const void *llj_u,
                            const void *llj_v, void *upwind_u, void *upwind_v, void *downwind_u, void *downwind_v,
                            void *stream) {
    return per_point<xp::CorfidiOp>("xp_corfidi_storm_motion", n, dtype, mem, {mean_u, mean_v, llj_u, llj_v}, 4,
                                    {upwind_u, upwind_v, downwind_u, downwind_v}, false, stream);
}

int xp_significant_tornado_effective(int64_t n, int32_t dtype, int32_t mem, const void *mlcape, const void *mlcin,
                                     const void *lcl_height, const void *esrh, const void *ebwd, const void *base_height,
                                     void *out, void *stream) {
    return per_point<xp::StpEffectiveOp>("xp_significant_tornado_effective", n, dtype, mem,
                                         {mlcape, mlcin, lcl_height, esrh, ebwd, base_height}, 5, {out}, true, stream);
}

int xp_ncape(const xp_view *p, const xp_view *t, const xp_view *td, const xp_view *z, const void *lfc_pressure,
             const void *el_pressure, xp_ncape_out *out, void *stream) {
    const char *const entry = "xp_ncape";
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {td, "dewpoint"}, {z, "height"}}))) return rc;
    if (!lfc_pressure) return fail(XP_E_ARG, "%s: lfc_pressure: null", entry);
    if (!el_pressure) return fail(XP_E_ARG, "%s: el_pressure: null", entry);
    if ((rc = check_out(entry, out, p))) return rc;
    const size_t cb = rows_bytes(p, 1);
    xp::NcapeArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = stage_view(st, p, &a.p)) || (rc = stage_view(st, t, &a.t)) || (rc = stage_view(st, td, &a.td)) ||
        (rc = stage_view(st, z, &a.z)) || (rc = st.in(lfc_pressure, cb, p->mem, &a.lfc_p)) ||
        (rc = st.in(el_pressure, cb, p->mem, &a.el_p)) || (rc = st.out(out->ncape, cb, out->mem, &a.ncape)) ||
        (rc = st.out(out->lfc_height, cb, out->mem, &a.lfc_z)) || (rc = st.out(out->el_height, cb, out->mem, &a.el_z)) ||
        (rc = st.out(out->status, (size_t)p->ncol * 4, out->mem, &a.status))) return rc;
    a.nlev = p->nlev; a.ncol = p->ncol;
    xp::launch_ncape(a, p->dtype == XP_F64, st.s);
    return st.finish();
}

int xp_ecape(int64_t n, int32_t dtype, int32_t mem, const void *cape, const void *ncape, const void *el_height,
             const void *sr_u, const void *sr_v, void *ecape, void *ecape_a, void *psi, void *stream) {
    const void *const in[5] = {cape, ncape, el_height, sr_u, sr_v};
    const char *const name[5] = {"cape", "ncape", "el_height", "sr_u", "sr_v"};
    for (int i = 0; i < 5 && g.init; ++i)                // (not initialised: per_point's XP_E_NOT_INIT comes first)
        if (!in[i]) return fail(XP_E_ARG, "xp_ecape: %s: null", name[i]);
    return per_point<xp::EcapeOp>("xp_ecape", n, dtype, mem, {cape, ncape, el_height, sr_u, sr_v}, 5, {ecape, ecape_a, psi}, false,
                                  stream);
}

int xp_interp_level(const xp_view *coords, const xp_view *x, const void *at, int32_t at_is_scalar, int32_t log_coords,
                    void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{coords, "coords"}, {x, "variable"}}))) return rc;
    if (!at || !out) return fail(XP_E_ARG, "xp_interp_level: null argument");
    xp::View cv, xv;
    const void *da;
    void *od;
    if ((rc = stage_view(st, coords, &cv)) || (rc = stage_view(st, x, &xv)) ||
        (rc = st.in(at, at_is_scalar ? esize(coords->dtype) : rows_bytes(coords, 1), coords->mem, &da)) ||
        (rc = st.out(out, rows_bytes(coords, 1), coords->mem, &od))) return rc;
    with_type(coords->dtype == XP_F64, [&](auto z) {
        launch_columns(xp::k_interp_level<decltype(z)>, coords->ncol, st.s, cv, xv, coords->nlev, coords->ncol, da, (int)at_is_scalar, (int)log_coords, od);
    });
    return st.finish();
}

int xp_interp_levels(const xp_view *coords, int32_t nvar, const xp_view *const *variables, int32_t ntarget, const double *at,
                     int32_t log_coords, void *const *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    if (nvar < 1 || nvar > 4 || ntarget < 1 || ntarget > 4) return fail(XP_E_ARG, "xp_interp_levels: 1..4 variables and 1..4 coordinates");
    if (!variables || !at || !out) return fail(XP_E_ARG, "xp_interp_levels: null argument");
    int rc;
    for (int v = 0; v < nvar; ++v)
        if ((rc = check_views({{coords, "coords"}, {variables[v], "variable"}}))) return rc;
    if ((rc = interp_levels(st, coords, nvar, variables, ntarget, at, log_coords, out))) return rc;
    return st.finish();
}

int xp_dewpoint_from_specific_humidity(const xp_view *p, const xp_view *t, const xp_view *q, void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{p, "pressure"}, {t, "temperature"}, {q, "specific_humidity"}}))) return rc;
    if (!out) return fail(XP_E_ARG, "xp_dewpoint_from_specific_humidity: null output");
    xp::View pv, tv, qv;
    void *od;
    if ((rc = stage_view(st, p, &pv)) || (rc = stage_view(st, t, &tv)) || (rc = stage_view(st, q, &qv)) ||
        (rc = st.out(out, rows_bytes(p, p->nlev), p->mem, &od))) return rc;
    with_type(p->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_dewpoint_from_q<decltype(z)>, p->nlev * p->ncol, st.s, pv, tv, qv, p->nlev, p->ncol, out_like(od, p)); });
    return st.finish();
}

int xp_crossing_level(const xp_view *x, const xp_view *a, double value, void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{x, "x"}, {a, "a"}}))) return rc;
    if (!out) return fail(XP_E_ARG, "xp_crossing_level: null output");
    xp::View xv, av;
    void *od;
    if ((rc = stage_view(st, x, &xv)) || (rc = stage_view(st, a, &av)) || (rc = st.out(out, rows_bytes(x, 1), x->mem, &od))) return rc;
    with_type(x->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_crossing_level<decltype(z)>, x->ncol, st.s, xv, av, x->nlev, x->ncol, value, od); });
    return st.finish();
}

int xp_mixing_ratio(const xp_view *t, const xp_view *td, const xp_view *p, void *out, void *stream) {
    Entry st(stream);
    if (st.rc) return st.rc;
    int rc;
    if ((rc = check_views({{t, "temperature"}, {td, "dewpoint"}, {p, "pressure"}}))) return rc;
    if (!out) return fail(XP_E_ARG, "xp_mixing_ratio: null output");
    xp::View tv, tdv, pv;
    void *od;
    if ((rc = stage_view(st, t, &tv)) || (rc = stage_view(st, td, &tdv)) || (rc = stage_view(st, p, &pv)) ||
        (rc = st.out(out, rows_bytes(t, t->nlev), t->mem, &od))) return rc;
    with_type(t->dtype == XP_F64, [&](auto z) { launch_columns(xp::k_mixing_ratio<decltype(z)>, t->nlev * t->ncol, st.s, tv, tdv, pv, t->nlev, t->ncol, out_like(od, t)); });
    return st.finish();
}

}  // extern "C"

// the reference's array primitives (insert_level, find_intersections, trapz, ...): kernels + entry points
#include "xp_primitives_abi.hpp"
