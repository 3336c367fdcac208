// varpro_posterior_args_stub.cpp -- the host-side argument checks, the prior's normaliser, the centres, the amplitude bound A and
// the LDS slab sizing of pnx_curvefit_varpro_posterior_f64 (pyneapple_amd/csrc/pnx_varpro_posterior_args.hpp, free of HIP types) as
// a stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_varpro_posterior_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read past n_nl * n_atoms atom values, n_atoms prior entries or n_free
// bounds is an AddressSanitizer report.
// With arguments "n_b k" it prints the slab width of that shape (the test compares api.varpro_posterior_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_varpro_posterior_args.hpp"

namespace pnx {
static char g_err[512];
int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace pnx

using namespace pnx;

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_err); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static const int kAll[7] = {2, 3, 4, 4, 5, 6, 6};   // parameters per model
static const int kLin[7] = {1, 1, 2, 2, 2, 3, 3};   // linear parameters

struct Call {
    pnx_curvefit_opts o;
    int n_atoms = 0, n_nl = 0, marg = 1;
    double noise_sd = 0.0;
    std::vector<double> nl, lo, hi, fixed, lp;
    bool with_mean = true, with_lp = false;
    VarproLayout L;
    VarproPosteriorHost H;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(o.n_free, 0.0);
        g_err[0] = 0;
        return varpro_posterior_check_args(&o, 1, b.data(), y.data(), n_atoms, nl.data(), fixed.empty() ? nullptr : fixed.data(), lo.data(),
                                           hi.data(), with_lp ? lp.data() : nullptr, noise_sd, marg, with_mean ? out.data() : nullptr,
                                           PNX_MEM_HOST, &L, &H);
    }
};

// every parameter free but those in `fixed_pos`; atom g holds the rates 0.5 / (j + 1) - g * 1e-5 (distinct within an atom)
static Call make(int model, int n_b, int n_atoms, std::vector<int> fixed_pos = {}, int t1 = 0) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    c.o.t1_mode = t1;
    const int n_all = kAll[model] + (t1 ? 1 : 0);
    for (int i = 0; i < n_all; ++i) {
        bool fx = false;
        for (int f : fixed_pos) fx = fx || f == i;
        if (fx)
            c.o.fixed_idx[c.o.n_fixed++] = i;
        else
            c.o.free_idx[c.o.n_free++] = i;
    }
    c.n_atoms = n_atoms;
    c.n_nl = c.o.n_free - kLin[model];
    const int na = n_atoms > 0 ? n_atoms : 1;
    c.nl.assign((size_t)(c.n_nl > 0 ? c.n_nl : 1) * na, 0.0);
    for (int r = 0; r < c.n_nl; ++r)
        for (int g = 0; g < na; ++g) c.nl[(size_t)r * na + g] = 0.5 / (r + 1) - g * 1e-5;
    c.lo.assign(c.o.n_free, 0.0);
    c.hi.assign(c.o.n_free, 1.0);
    c.lp.assign(na, 0.0);
    for (size_t f = 0; f < fixed_pos.size(); ++f) c.fixed.push_back(0.9 - 0.01 * f);
    return c;
}

int main(int argc, char **argv) {
    if (argc == 3) {
        printf("%d\n", varpro_posterior_slab(atoi(argv[1]), atoi(argv[2])).width);
        return 0;
    }
    for (int model = 0; model < 7; ++model)  // valid edges, exact-size arrays, with and without a prior, both noise modes
        for (int n_atoms : {1, 15, 16, 17, 4096}) {
            Call c = make(model, 32, n_atoms);
            EXPECT(c.run() == PNX_OK && fabs(c.H.log_prior_norm - log((double)n_atoms)) < 1e-12);
            c.with_lp = true;
            c.noise_sd = 0.5;
            c.marg = 0;
            EXPECT(c.run() == PNX_OK && fabs(c.H.log_prior_norm - log((double)n_atoms)) < 1e-9);
            Call t = make(model, 32, n_atoms, {}, 1);  // T1 free: one more non-linear row
            EXPECT(t.run() == PNX_OK && t.L.n_nl == kAll[model] - kLin[model] + 1);
        }
    {   // the centres: mid-range of the admissible atoms of a non-linear row, 0 for a linear row
        Call c = make(PNX_MODEL_TRI_S0, 32, 4);
        c.with_lp = true;
        c.lp = {-HUGE_VAL, 0.5, -1.0, -HUGE_VAL};
        EXPECT(c.run() == PNX_OK);
        EXPECT(c.H.centre[0] == 0.0 && c.H.centre[2] == 0.0 && c.H.centre[5] == 0.0);
        EXPECT(fabs(c.H.centre[1] - 0.5 * (c.nl[1] + c.nl[2])) < 1e-15 && fabs(c.H.centre[3] - 0.5 * (c.nl[4 + 1] + c.nl[4 + 2])) < 1e-15);
        EXPECT(fabs(c.H.log_prior_norm - log(exp(0.5) + exp(-1.0))) < 1e-12);
        c.lp = {-HUGE_VAL, -HUGE_VAL, 2.0, -HUGE_VAL};  // all but one excluded: the centre is that atom's value, exactly
        EXPECT(c.run() == PNX_OK && c.H.centre[1] == c.nl[2] && c.H.log_prior_norm == 2.0);
    }
    {   // A per class
        Call c = make(PNX_MODEL_TRI_S0, 32, 4);
        c.hi[5] = 10.0;
        EXPECT(c.run() == PNX_OK && c.H.amp_l1 == 10.0 * (1.0 + 1.0 + 1.0));
        c.lo[0] = 0.3, c.hi[0] = 0.35, c.lo[2] = 0.3, c.hi[2] = 0.35, c.lo[5] = 0.9, c.hi[5] = 0.95;
        EXPECT(c.run() == PNX_OK && fabs(c.H.amp_l1 - 0.95 * (0.35 + 0.35 + 0.4)) < 1e-15);
        c = make(PNX_MODEL_TRI_REDUCED, 32, 4);
        EXPECT(c.run() == PNX_OK && c.H.amp_l1 == 3.0);
        c = make(PNX_MODEL_BI_FULL, 32, 4);
        c.lo[0] = -2.0;
        EXPECT(c.run() == PNX_OK && c.H.amp_l1 == 3.0);
        c = make(PNX_MODEL_MONO, 2, 4);
        c.hi[0] = 7.0;
        EXPECT(c.run() == PNX_OK && c.H.amp_l1 == 7.0);
    }
    {   // the new arguments, by name
        Call c = make(PNX_MODEL_TRI_S0, 32, 4);
        c.with_mean = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "mean"));
        c.with_mean = true;
        for (double bad : {-1.0, (double)NAN, (double)INFINITY, -(double)INFINITY}) {
            c.noise_sd = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        }
        c.noise_sd = 0.0;
        for (int bad : {-1, 2, 7}) {
            c.marg = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "marginal_amplitudes"));
        }
        c.marg = 1;
        c.with_lp = true;
        for (double bad : {(double)NAN, (double)INFINITY}) {
            c.lp[2] = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior[2]"));
        }
        c.lp.assign(4, -HUGE_VAL);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior excludes every atom"));
        c.lp[3] = -700.0;
        EXPECT(c.run() == PNX_OK);
        c.lo[3] = 0.7, c.hi[3] = 0.6;  // a non-linear row: named as a bound, not as the stand-in fallback
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "parameter 3") && strstr(g_err, "lo=0.7") && !strstr(g_err, "fallback"));
    }
    {   // the variable projection's refusals come through unchanged
        Call c = make(PNX_MODEL_TRI_S0, 32, 4);
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        const int32_t order[1] = {0};
        c.o.queue_order = order;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "queue_order"));
        c.o.queue_order = nullptr;
        for (int n_atoms : {0, -1, 4097}) {  // refused before the atoms and the prior are read
            c.n_atoms = n_atoms;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        }
        c.n_atoms = 4;
        c.o.n_b = 3;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_b=3"));
        c.o.n_b = 4;
        EXPECT(c.run() == PNX_OK);
        c.nl[4 + 2] = c.nl[2];  // D2 = D1 of atom 2
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 2") && strstr(g_err, "equal rates"));
        c.nl[4 + 2] = 1.5;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 2") && strstr(g_err, "outside its bounds"));
        c.nl[4 + 2] = 0.2;
        c.lo[5] = -1e-300;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "lo_S0"));
        c = make(PNX_MODEL_TRI_S0, 32, 4, {2});
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "parameter 2") && strstr(g_err, "fixed"));
        c = make(PNX_MODEL_BI_S0, 32, 4, {3});
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "parameter 3"));
        c = make(PNX_MODEL_BI_S0, 32, 4, {1});
        c.o.fixed_per_voxel = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "fixed_per_voxel"));
        c = make(PNX_MODEL_TRI_S0, 32, 4, {4, 6}, 1);  // fixed rates and a fixed T1 are served
        EXPECT(c.run() == PNX_OK && c.L.n_nl == 2);
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: whole tiles, inside 64 KB, the half-waves on opposite bank halves
        for (int k = 1; k <= 3; ++k) {
            const GridSlab s = varpro_posterior_slab(n_b, k);
            const int rows = varpro_const_rows(k) + varpro_posterior_extra_rows(k);
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.kpad - n_b < 4);
            EXPECT(s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.width <= varpro_slab(n_b, k).width);
            EXPECT(s.stride >= s.width && s.stride % 32 == 16);
            EXPECT(s.lds_doubles == k * s.kpad * s.stride + rows * s.width && s.lds_doubles * 8 <= 64 * 1024);
        }
    EXPECT(varpro_posterior_slab(128, 3).width == 16 && varpro_posterior_extra_rows(3) == 5);
    if (failures) return 1;
    printf("varpro posterior args stub ok\n");
    return 0;
}
