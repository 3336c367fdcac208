// grid_prior_args_stub.cpp -- the host-side argument checks, the normalised start prior, the stopping rule, the report of a call
// and the LDS slab sizing of pnx_curvefit_grid_prior_em_f64 (pyneapple_amd/csrc/pnx_grid_prior_args.hpp, free of HIP types) as a
// stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_grid_prior_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read or write past n_atoms prior entries or n_iter + 1 trace entries
// is an AddressSanitizer report.  With the argument "n_b" it prints the slab width of that shape (the test compares
// api.grid_prior_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_grid_prior_args.hpp"

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

struct Call {
    pnx_curvefit_opts o;
    int n_atoms, n_iter = 20, project = 0;
    std::vector<double> atoms, lo, hi, prior;
    bool with_prior = false, with_out = true;
    double noise_sd = 0.0, pseudo_count = 0.0, rel_tol = 1e-6;
    GridPosteriorHost H;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(n_atoms > 0 ? n_atoms : 1, 0.0);
        g_err[0] = 0;
        return grid_prior_check_args(&o, 1, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), project,
                                     with_prior ? prior.data() : nullptr, noise_sd, n_iter, pseudo_count, rel_tol,
                                     with_out ? out.data() : nullptr, PNX_MEM_HOST, &H);
    }
};

static Call make(int model, int n_all, int n_b, int n_atoms) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    for (int i = 0; i < n_all; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.n_atoms = n_atoms;
    c.atoms.assign((size_t)n_all * (n_atoms > 0 ? n_atoms : 1), 0.5);
    c.lo.assign(n_all, 0.0);
    c.hi.assign(n_all, 1.0);
    c.prior.assign(n_atoms > 0 ? n_atoms : 1, 0.0);
    return c;
}

int main(int argc, char **argv) {
    if (argc == 2) {
        printf("%d\n", grid_prior_slab(atoi(argv[1])).width);
        return 0;
    }
    const double inf = HUGE_VAL;
    {   // the four arguments of the EM, each refused by name; the edges accepted
        Call c = make(PNX_MODEL_BI_S0, 4, 16, 5);
        EXPECT(c.run() == PNX_OK);
        for (int bad : {0, -1, 1001, 1 << 30}) {
            c.n_iter = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_iter"));
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
        c.noise_sd = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.with_prior = true;
        c.prior.assign(5, -inf);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.prior[3] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.with_prior = false;
        c.n_atoms = 0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        c.n_atoms = 4097;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        c.n_atoms = 5;
        c.project = 1;
        EXPECT(c.run() == PNX_OK && c.H.s0_row == 3);
        c.o.model = PNX_MODEL_BI_FULL;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "S0"));
        c.o.model = PNX_MODEL_BI_S0;
        c.project = 0;
        c.atoms[7] = 1.5;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 2") && strstr(g_err, "parameter 1"));
        c.atoms[7] = 0.5;
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        const int32_t order[1] = {0};
        c.o.queue_order = order;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "queue_order"));
        c.o.queue_order = nullptr;
        c.o.n_fixed = 1;
        c.o.fixed_per_voxel = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "fixed_per_voxel"));
    }
    for (int n_atoms : {1, 15, 16, 17, 4096}) {  // the start: normalised, -inf kept, the admissible atoms counted
        std::vector<double> start(n_atoms, 7.0);
        EXPECT(grid_prior_start(n_atoms, nullptr, log((double)n_atoms), start.data()) == n_atoms);
        double sum = 0.0;
        for (double s : start) sum += exp(s);
        EXPECT(fabs(sum - 1.0) < 1e-12 && start[0] == -log((double)n_atoms) && start[n_atoms - 1] == start[0]);
        std::vector<double> prior(n_atoms, -inf);
        prior[n_atoms - 1] = 2.0;
        prior[0] = 2.0 + log(3.0);
        double norm = 0.0;
        EXPECT(posterior_check_log_prior("stub", n_atoms, prior.data(), &norm) == PNX_OK);
        const int adm = grid_prior_start(n_atoms, prior.data(), norm, start.data());
        EXPECT(adm == (n_atoms == 1 ? 1 : 2));
        if (n_atoms > 1) {
            EXPECT(fabs(start[0] - log(0.75)) < 1e-12 && fabs(start[n_atoms - 1] - log(0.25)) < 1e-12);
            for (int g = 1; g < n_atoms - 1; ++g) EXPECT(start[g] == -inf);
        } else {
            EXPECT(fabs(start[0]) < 1e-15);
        }
    }
    {   // the stopping rule and the report
        const double trace[4] = {-100.0, -90.0, -89.9999, -89.9999};
        EXPECT(!grid_prior_converged(trace, 0, 1.0));         // never before the first update
        EXPECT(grid_prior_converged(trace, 1, 1.0));          // 10 <= 1 x 90
        EXPECT(!grid_prior_converged(trace, 1, 1e-6));
        EXPECT(grid_prior_converged(trace, 2, 1e-5) && !grid_prior_converged(trace, 2, 1e-7));
        EXPECT(!grid_prior_converged(trace, 3, 0.0));         // rel_tol = 0 runs every update, a gain of exactly 0 included
        for (int n_iter : {1, 5}) {
            std::vector<double> loglik(n_iter + 1, 3.0);
            int done = -1;
            int64_t n_eff = -1;
            grid_prior_report(n_iter, 1, 42, loglik.data(), &done, &n_eff);
            EXPECT(done == 1 && n_eff == 42 && loglik[0] == 3.0 && loglik[1] == 3.0);
            for (int t = 2; t <= n_iter; ++t) EXPECT(std::isnan(loglik[t]));
            grid_prior_report(n_iter, 0, 0, loglik.data(), nullptr, nullptr);
            EXPECT(loglik[0] == 3.0 && std::isnan(loglik[1]));
            grid_prior_report(n_iter, n_iter, 7, nullptr, nullptr, nullptr);  // every output optional
        }
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b) {  // the slab: the dictionary rows, three values per atom and four wave rows in 64 KB
        const GridSlab s = grid_prior_slab(n_b);
        EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.kpad - n_b < 4);
        EXPECT(s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.stride >= s.width && s.stride % 32 == 16);
        EXPECT(s.lds_doubles == s.kpad * s.stride + 7 * s.width && s.lds_doubles * 8 <= 64 * 1024 && s.lds_doubles >= 32);
        for (int n_free = 4; n_free <= PNX_MAX_PARAMS; ++n_free) EXPECT(s.width >= grid_posterior_slab(n_b, n_free).width);
    }
    if (failures) return 1;
    printf("grid prior args stub ok\n");
    return 0;
}
