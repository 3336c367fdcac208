// grid_posterior_args_stub.cpp -- the host-side argument checks, the prior's normaliser, the row centres and the LDS slab sizing
// of pnx_curvefit_grid_posterior_f64 (pyneapple_amd/csrc/pnx_grid_posterior_args.hpp, free of HIP types) as a stand-alone CPU
// program, built with -fsanitize=address,undefined by tests/test_grid_posterior_host.py.  Every array is heap-allocated at exactly
// the size the ABI documents, so a read past n_atoms prior entries or n_free * n_atoms atoms is an AddressSanitizer report.
// With arguments "n_b n_free" it prints the slab width of that shape (the test compares api.grid_posterior_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_grid_posterior_args.hpp"

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

static pnx_curvefit_opts opts(int model, int n_all, int n_b) {
    pnx_curvefit_opts o;
    memset(&o, 0, sizeof(o));
    o.model = model;
    o.n_b = n_b;
    for (int i = 0; i < n_all; ++i) o.free_idx[o.n_free++] = i;
    return o;
}

struct Call {
    pnx_curvefit_opts o;
    int n_atoms;
    std::vector<double> atoms, lo, hi, prior;
    bool with_prior = false, with_mean = true;
    double noise_sd = 0.0;
    int project = 0;
    GridPosteriorHost H;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), mean(o.n_free, 0.0);
        g_err[0] = 0;
        return grid_posterior_check_args(&o, 1, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), project,
                                         with_prior ? prior.data() : nullptr, noise_sd, with_mean ? mean.data() : nullptr, PNX_MEM_HOST, &H);
    }
};

static Call make(int model, int n_all, int n_b, int n_atoms) {
    Call c;
    c.o = opts(model, n_all, n_b);
    c.n_atoms = n_atoms;
    c.atoms.assign((size_t)n_all * (n_atoms > 0 ? n_atoms : 1), 0.5);
    c.lo.assign(n_all, 0.0);
    c.hi.assign(n_all, 1.0);
    c.prior.assign(n_atoms > 0 ? n_atoms : 1, 0.0);
    return c;
}

int main(int argc, char **argv) {
    if (argc == 3) {
        printf("%d\n", grid_posterior_slab(atoi(argv[1]), atoi(argv[2])).width);
        return 0;
    }
    const double inf = HUGE_VAL;
    for (int n_atoms : {1, 15, 16, 17, 4096}) {  // valid edges, exact-size arrays
        Call c = make(PNX_MODEL_TRI_S0, 6, 32, n_atoms);
        EXPECT(c.run() == PNX_OK && c.H.s0_row == -1 && fabs(c.H.log_prior_norm - log((double)n_atoms)) < 1e-15);
        c.project = 1;
        EXPECT(c.run() == PNX_OK && c.H.s0_row == 5 && c.H.centre[5] == 0.0 && c.H.centre[0] == 0.5);
        c.project = 0;
        c.with_prior = true;  // all but the last atom excluded: the normaliser and the centres are the last atom's
        for (int g = 0; g < n_atoms - 1; ++g) c.prior[g] = -inf;
        c.prior[n_atoms - 1] = -3.0;
        for (int k = 0; k < 6; ++k) c.atoms[(size_t)k * n_atoms + n_atoms - 1] = 0.25;
        EXPECT(c.run() == PNX_OK && c.H.log_prior_norm == -3.0 && c.H.centre[2] == 0.25);
        c.noise_sd = 0.02;
        EXPECT(c.run() == PNX_OK);
        c.prior[n_atoms - 1] = -inf;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.prior[n_atoms - 1] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.prior[n_atoms - 1] = inf;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
    }
    {
        Call c = make(PNX_MODEL_BI_REDUCED, 3, 16, 4);
        for (double bad : {-1.0, -0.0 - 1e-300, (double)NAN, inf, -inf}) {
            c.noise_sd = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        }
        c.noise_sd = 0.0;
        EXPECT(c.run() == PNX_OK);
        c.with_mean = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "mean"));
        c.with_mean = true;
        // grid start's refusals, unchanged
        c.n_atoms = 0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        c.n_atoms = 4097;  // refused before atoms or log_prior are read
        c.with_prior = true;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        c.n_atoms = 4;
        c.project = 1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "S0"));
        c.project = 0;
        c.atoms[5] = 1.5;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 1") && strstr(g_err, "parameter 1"));
        c.atoms[5] = 0.5;
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
    {   // a finite prior: the normaliser is the log-sum-exp, whatever the offset
        Call c = make(PNX_MODEL_MONO, 2, 8, 3);
        c.with_prior = true;
        c.prior = {1000.0, 1000.0 + log(2.0), 1000.0 + log(3.0)};
        c.atoms = {0.1, 0.2, 0.9, 0.5, 0.5, 0.5};
        EXPECT(c.run() == PNX_OK && fabs(c.H.log_prior_norm - (1000.0 + log(6.0))) < 1e-12);
        EXPECT(c.H.centre[0] == 0.1 + 0.5 * (0.9 - 0.1) && c.H.centre[1] == 0.5);
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: whole tiles, inside 64 KB, the half-waves on opposite bank halves
        for (int n_free = 1; n_free <= PNX_MAX_PARAMS; ++n_free) {
            const GridSlab s = grid_posterior_slab(n_b, n_free);
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.kpad - n_b < 4);
            EXPECT(s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.width <= grid_slab(n_b).width);
            EXPECT(s.stride >= s.width && s.stride % 32 == 16);
            EXPECT(s.lds_doubles == s.kpad * s.stride + (3 + n_free) * s.width && s.lds_doubles * 8 <= 64 * 1024);
        }
    if (failures) return 1;
    printf("grid posterior args stub ok\n");
    return 0;
}
