// varpro_class_args_stub.cpp -- the host-side checks of n_classes, labels and the (n_classes, n_atoms) table, the per-row starts, the
// centres, the report of an EM call and the LDS slab sizing of pnx_curvefit_varpro_posterior_classes_f64 /
// pnx_curvefit_varpro_prior_em_classes_f64 (pyneapple_amd/csrc/pnx_varpro_class_args.hpp, free of HIP types) as a stand-alone CPU
// program, built with -fsanitize=address,undefined by tests/test_varpro_class_prior_host.py.  Every array is heap-allocated at
// exactly the size the ABI documents, so a read or write past n_classes rows is an AddressSanitizer report.  With the arguments
// "n_b k n_classes extra" it prints the slab width of that shape (the test compares api.varpro_class_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_varpro_class_args.hpp"

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

// bi_s0, every parameter free (f1, D1, D2, S0): two non-linear rows
struct Call {
    pnx_curvefit_opts o;
    int n_atoms, n_classes = 3, n_iter = 20, marg = 1;
    std::vector<double> nl, lo, hi, prior;
    bool with_prior = false, with_labels = true, with_out = true;
    double noise_sd = 0.0;
    VarproLayout L;
    VarproPosteriorHost H;
    GridClassHost K;
    int run(bool em) {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out((size_t)(n_classes > 0 && n_classes <= kGridMaxClasses ? n_classes : 1) * n_atoms, 0.0);  // a refused count sizes nothing
        std::vector<int32_t> lab(1, 0);
        g_err[0] = 0;
        const double *p = with_prior ? prior.data() : nullptr, *res = with_out ? out.data() : nullptr;
        const int32_t *l = with_labels ? lab.data() : nullptr;
        if (em)
            return varpro_class_prior_check_args(&o, 1, b.data(), y.data(), n_atoms, nl.data(), nullptr, lo.data(), hi.data(), n_classes, l, p,
                                                 noise_sd, marg, n_iter, 0.0, 0.0, res, PNX_MEM_HOST, &L, &H, &K);
        return varpro_class_posterior_check_args(&o, 1, b.data(), y.data(), n_atoms, nl.data(), nullptr, lo.data(), hi.data(), n_classes, l, p,
                                                 noise_sd, marg, res, PNX_MEM_HOST, &L, &H, &K);
    }
};

static Call make(int n_atoms, int n_classes) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = PNX_MODEL_BI_S0;
    c.o.n_b = 16;
    for (int i = 0; i < 4; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.n_atoms = n_atoms;
    c.n_classes = n_classes;
    c.nl.assign((size_t)2 * n_atoms, 0.0);
    for (int g = 0; g < n_atoms; ++g) {
        c.nl[g] = 0.1 + 0.2 * g / (n_atoms > 1 ? n_atoms - 1 : 1);  // D1: 0.1 .. 0.3
        c.nl[(size_t)n_atoms + g] = 0.01;                           // D2
    }
    c.lo.assign(4, 0.0);
    c.hi.assign(4, 1.0);
    c.prior.assign((size_t)(n_classes > 0 ? n_classes : 1) * n_atoms, 0.0);
    return c;
}

int main(int argc, char **argv) {
    if (argc == 5) {
        printf("%d\n", varpro_class_slab(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4])).width);
        return 0;
    }
    const double inf = HUGE_VAL;
    for (int em = 0; em < 2; ++em) {
        Call c = make(5, 3);
        EXPECT(c.run(em) == PNX_OK);
        for (int good : {1, 16}) {
            Call d = make(5, good);
            EXPECT(d.run(em) == PNX_OK);
            d.with_prior = true;
            EXPECT(d.run(em) == PNX_OK);
        }
        for (int bad : {0, -1, 17, 1 << 30}) {  // refused before the table is looked at
            c.n_classes = bad;
            EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "n_classes") && strstr(g_err, em ? "varpro prior" : "varpro posterior"));
        }
        c.n_classes = 3;
        c.with_labels = false;
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "labels"));
        c.with_labels = true;
        c.with_prior = true;
        for (int g = 0; g < 5; ++g) c.prior[2 * 5 + g] = -inf;  // the last row excludes every atom
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "row 2") && strstr(g_err, "excludes every atom"));
        c.prior[2 * 5 + 4] = -3.0;
        EXPECT(c.run(em) == PNX_OK && c.K.n_adm[0] == 5 && c.K.n_adm[1] == 5 && c.K.n_adm[2] == 1 && c.K.norm[2] == -3.0);
        EXPECT(fabs(c.K.norm[0] - log(5.0)) < 1e-15);
        c.prior[1 * 5 + 3] = NAN;
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "log_prior[1, 3]"));
        c.prior[1 * 5 + 3] = inf;
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "log_prior[1, 3]"));
        c.prior[1 * 5 + 3] = 0.0;
        // the refusals of the unlabelled calls, inherited
        c.noise_sd = -1.0;
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.marg = 2;
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "marginal_amplitudes"));
        c.marg = 1;
        c.with_out = false;
        EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, em ? "log_prior_out" : "mean"));
        c.with_out = true;
        if (em) {
            c.n_iter = 0;
            EXPECT(c.run(em) == PNX_ERR_INVALID && strstr(g_err, "n_iter"));
            c.n_iter = 20;
        }
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run(em) != PNX_OK && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        // the centres: mid-range of the atoms any row admits -- rows 0 and 1 admit atoms 3 and 4 only, row 2 atom 4; D1 is free
        // row 1 (0.25, 0.3 -> 0.275), D2 row 2 (one value), the linear rows f1 and S0 stay 0
        for (int r = 0; r < 2; ++r)
            for (int g = 0; g < 3; ++g) c.prior[r * 5 + g] = -inf;
        EXPECT(c.run(em) == PNX_OK && fabs(c.H.centre[1] - 0.275) < 1e-15 && c.H.centre[2] == 0.01 && c.H.centre[0] == 0.0 && c.H.centre[3] == 0.0);
        c.with_prior = false;
        EXPECT(c.run(em) == PNX_OK && fabs(c.H.centre[1] - 0.2) < 1e-15);
    }
    {   // one row: the unlabelled call's normaliser, centres and start, byte for byte
        Call c = make(7, 1);
        c.with_prior = true;
        for (int g = 0; g < 7; ++g) c.prior[g] = g == 2 ? -inf : 0.3 * g - 1.0;
        EXPECT(c.run(0) == PNX_OK);
        VarproLayout L;
        VarproPosteriorHost H;
        std::vector<double> b(16, 0.0), y(16, 1.0), out(7);
        EXPECT(varpro_posterior_check_args(&c.o, 1, b.data(), y.data(), 7, c.nl.data(), nullptr, c.lo.data(), c.hi.data(), c.prior.data(), 0.0, 1,
                                           out.data(), PNX_MEM_HOST, &L, &H) == PNX_OK);
        EXPECT(H.log_prior_norm == c.K.norm[0] && memcmp(H.centre, c.H.centre, sizeof(H.centre)) == 0 && c.K.n_adm[0] == 6);
        EXPECT(H.amp_l1 == c.H.amp_l1 && L.k == c.L.k && L.cls == c.L.cls);
        std::vector<double> s1(7), s2(7);
        grid_prior_start(7, c.prior.data(), H.log_prior_norm, s1.data());
        grid_class_start(1, 7, c.prior.data(), c.K, s2.data());
        EXPECT(memcmp(s1.data(), s2.data(), 7 * sizeof(double)) == 0);
    }
    for (int C : {1, 3, 16}) {  // the starts, row by row, and the report
        const int G = 17;
        std::vector<double> prior((size_t)C * G), start((size_t)C * G, 7.0);
        for (int c = 0; c < C; ++c)
            for (int g = 0; g < G; ++g) prior[(size_t)c * G + g] = (g + c) % 5 == 0 ? -inf : 0.1 * g - c;
        GridClassHost K;
        std::vector<int32_t> lab(1, 0);
        EXPECT(grid_class_check_table("varpro prior", C, lab.data(), 1, G, prior.data(), &K) == PNX_OK);
        grid_class_start(C, G, prior.data(), K, start.data());
        for (int c = 0; c < C; ++c) {
            double sum = 0.0;
            int adm = 0;
            for (int g = 0; g < G; ++g) {
                sum += exp(start[(size_t)c * G + g]);
                adm += start[(size_t)c * G + g] > -inf;
                EXPECT((start[(size_t)c * G + g] == -inf) == ((g + c) % 5 == 0));
            }
            EXPECT(fabs(sum - 1.0) < 1e-12 && adm == K.n_adm[c]);
        }
        for (int n_iter : {1, 5}) {
            std::vector<double> loglik(n_iter + 1, 3.0), per((size_t)(n_iter + 1) * C, 3.0);
            std::vector<int64_t> n_eff(C, -1), finite(C, 42);
            int done = -1;
            grid_class_report(n_iter, 1, C, finite.data(), loglik.data(), per.data(), &done, n_eff.data());
            EXPECT(done == 1 && n_eff[C - 1] == 42 && loglik[1] == 3.0 && per[(size_t)2 * C - 1] == 3.0);
            for (int t = 2; t <= n_iter; ++t) EXPECT(std::isnan(loglik[t]) && std::isnan(per[(size_t)t * C]) && std::isnan(per[(size_t)(t + 1) * C - 1]));
            grid_class_report(n_iter, 0, C, nullptr, loglik.data(), per.data(), nullptr, n_eff.data());
            EXPECT(n_eff[0] == 0 && std::isnan(loglik[1]) && per[C - 1] == 3.0);
        }
    }
    // the slab: at least 16 atoms, a multiple of 16, inside 64 KB for every class count, k and n_b; one class is the unlabelled slab
    for (int C = 1; C <= kGridMaxClasses; ++C)
        for (int k = 1; k <= 3; ++k)
            for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b) {
                const GridSlab e = varpro_class_prior_slab(n_b, k, C), p = varpro_class_posterior_slab(n_b, k, C);
                for (const GridSlab &s : {e, p}) {
                    EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.stride >= s.width &&
                           s.stride % 32 == 16 && s.lds_doubles * 8 <= 64 * 1024);
                }
                EXPECT(e.lds_doubles == k * e.kpad * e.stride + (varpro_const_rows(k) + 5 * C) * e.width);
                EXPECT(p.lds_doubles == k * p.kpad * p.stride + (varpro_const_rows(k) + C + k + 1) * p.width);
                if (C > 1) EXPECT(e.width <= varpro_class_prior_slab(n_b, k, C - 1).width && p.width <= varpro_class_posterior_slab(n_b, k, C - 1).width);
                if (C == 1) {
                    const GridSlab ue = varpro_prior_slab(n_b, k), up = varpro_posterior_slab(n_b, k);
                    EXPECT(e.width == ue.width && e.stride == ue.stride && e.lds_doubles == ue.lds_doubles);
                    EXPECT(p.width == up.width && p.stride == up.stride && p.lds_doubles == up.lds_doubles);
                }
            }
    EXPECT(varpro_class_prior_slab(128, 3, 16).lds_doubles == 7616);  // the worst case: 384 16 + 92 16
    EXPECT(varpro_class_prior_slab(32, 3, 1).width == 48 && varpro_class_prior_slab(32, 3, 16).width == 32);
    if (failures) return 1;
    printf("varpro class args stub ok\n");
    return 0;
}
