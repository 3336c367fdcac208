// varpro_prior_args_stub.cpp -- the host-side argument checks, the normalised start prior, the stopping rule, the report of a call
// and the LDS slab sizing of pnx_curvefit_varpro_prior_em_f64 (pyneapple_amd/csrc/pnx_varpro_prior_args.hpp, free of HIP types) as a
// stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_varpro_prior_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read or write past n_nl * n_atoms atom values, n_atoms prior entries
// or n_iter + 1 trace entries is an AddressSanitizer report.  With arguments "n_b k" it prints the slab width of that shape (the
// test compares api.varpro_prior_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_varpro_prior_args.hpp"

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
    int n_atoms = 0, n_nl = 0, marg = 1, n_iter = 20;
    double noise_sd = 0.0, pseudo_count = 0.0, rel_tol = 1e-6;
    std::vector<double> nl, lo, hi, fixed, lp;
    bool with_out = true, with_lp = false;
    VarproLayout L;
    VarproPosteriorHost H;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(n_atoms > 0 ? n_atoms : 1, 0.0);
        g_err[0] = 0;
        return varpro_prior_check_args(&o, 1, b.data(), y.data(), n_atoms, nl.data(), fixed.empty() ? nullptr : fixed.data(), lo.data(),
                                       hi.data(), with_lp ? lp.data() : nullptr, noise_sd, marg, n_iter, pseudo_count, rel_tol,
                                       with_out ? out.data() : nullptr, PNX_MEM_HOST, &L, &H);
    }
};

// every parameter free but those in `fixed_pos`; atom g holds the rates 0.5 / (j + 1) - g * 1e-5 (distinct within an atom)
static Call make(int model, int n_b, int n_atoms, std::vector<int> fixed_pos = {}) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    for (int i = 0; i < kAll[model]; ++i) {
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
        printf("%d\n", varpro_prior_slab(atoi(argv[1]), atoi(argv[2])).width);
        return 0;
    }
    const double inf = HUGE_VAL;
    for (int model = 0; model < 7; ++model)  // valid edges, exact-size arrays, with and without a start, both noise modes
        for (int n_atoms : {1, 15, 16, 17, 4096}) {
            Call c = make(model, 32, n_atoms);
            EXPECT(c.run() == PNX_OK && fabs(c.H.log_prior_norm - log((double)n_atoms)) < 1e-12);
            c.with_lp = true;
            c.noise_sd = 0.5;
            c.marg = 0;
            EXPECT(c.run() == PNX_OK);
        }
    {   // the four arguments of the EM, each refused by name and with this call's own prefix; the edges accepted
        Call c = make(PNX_MODEL_TRI_S0, 32, 5);
        for (int bad : {0, -1, 1001, 1 << 30}) {
            c.n_iter = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_iter") && strstr(g_err, "varpro prior"));
        }
        for (int good : {1, 1000}) {
            c.n_iter = good;
            EXPECT(c.run() == PNX_OK);
        }
        for (double bad : {-1e-300, -1.0, (double)NAN, inf, -inf}) {
            c.pseudo_count = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "pseudo_count"));
            c.pseudo_count = 0.0;
            c.rel_tol = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "rel_tol"));
            c.rel_tol = 0.0;
        }
        c.pseudo_count = 1e300;
        c.rel_tol = 1.0;
        EXPECT(c.run() == PNX_OK);
        c.with_out = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior_out"));
        c.with_out = true;
        // the posterior's refusals, inherited through its own check
        for (int bad : {-1, 2, 7}) {
            c.marg = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "marginal_amplitudes"));
        }
        c.marg = 1;
        c.noise_sd = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.with_lp = true;
        c.lp.assign(5, -inf);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior excludes every atom"));
        c.lp[3] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.with_lp = false;
        for (int n_atoms : {0, -1, 4097}) {
            c.n_atoms = n_atoms;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        }
        c.n_atoms = 5;
        c.lo[5] = -1e-300;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "lo_S0"));
        c.lo[5] = 0.0;
        c.nl[5 + 2] = c.nl[2];  // D2 = D1 of atom 2
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 2") && strstr(g_err, "equal rates"));
        c = make(PNX_MODEL_TRI_S0, 32, 4, {2});
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "parameter 2") && strstr(g_err, "fixed"));
        c = make(PNX_MODEL_BI_S0, 32, 4, {3});
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "parameter 3"));
        c = make(PNX_MODEL_BI_S0, 32, 4);
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
    }
    for (int n_atoms : {1, 15, 16, 17, 4096}) {  // the start (the grid EM's function, called): normalised, -inf kept
        std::vector<double> start(n_atoms, 7.0), prior(n_atoms, -inf);
        EXPECT(grid_prior_start(n_atoms, nullptr, log((double)n_atoms), start.data()) == n_atoms && start[n_atoms - 1] == -log((double)n_atoms));
        prior[n_atoms - 1] = 2.0;
        prior[0] = 2.0 + log(3.0);
        double norm = 0.0;
        EXPECT(posterior_check_log_prior("stub", n_atoms, prior.data(), &norm) == PNX_OK);
        EXPECT(grid_prior_start(n_atoms, prior.data(), norm, start.data()) == (n_atoms == 1 ? 1 : 2));
        if (n_atoms > 1) EXPECT(fabs(start[0] - log(0.75)) < 1e-12 && fabs(start[n_atoms - 1] - log(0.25)) < 1e-12 && start[n_atoms / 2] == (n_atoms > 2 ? -inf : start[n_atoms / 2]));
    }
    {   // the stopping rule and the report (the grid EM's functions, called)
        const double trace[4] = {-100.0, -90.0, -89.9999, -89.9999};
        EXPECT(!grid_prior_converged(trace, 0, 1.0) && grid_prior_converged(trace, 1, 1.0) && !grid_prior_converged(trace, 1, 1e-6));
        EXPECT(grid_prior_converged(trace, 2, 1e-5) && !grid_prior_converged(trace, 3, 0.0));
        for (int n_iter : {1, 5}) {
            std::vector<double> loglik(n_iter + 1, 3.0);
            int done = -1;
            int64_t n_eff = -1;
            grid_prior_report(n_iter, 1, 42, loglik.data(), &done, &n_eff);
            EXPECT(done == 1 && n_eff == 42 && loglik[0] == 3.0 && loglik[1] == 3.0);
            for (int t = 2; t <= n_iter; ++t) EXPECT(std::isnan(loglik[t]));
        }
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: whole tiles, inside 64 KB, room for the block's reduction
        for (int k = 1; k <= 3; ++k) {
            const GridSlab s = varpro_prior_slab(n_b, k);
            const int rows = varpro_const_rows(k) + 1 + kVarproPriorWaves;
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.kpad - n_b < 4);
            EXPECT(s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.width <= varpro_posterior_slab(n_b, k).width);
            EXPECT(s.stride >= s.width && s.stride % 32 == 16);
            EXPECT(s.lds_doubles == k * s.kpad * s.stride + rows * s.width && s.lds_doubles * 8 <= 64 * 1024 && s.lds_doubles >= 32);
            if (k == 3) EXPECT(s.width == varpro_posterior_slab(n_b, k).width);
        }
    EXPECT(varpro_prior_slab(128, 3).width == 16 && varpro_prior_slab(32, 2).width == 80 && varpro_posterior_slab(32, 2).width == 96);
    if (failures) return 1;
    printf("varpro prior args stub ok\n");
    return 0;
}
