// grid_refine_stub.cpp -- the host-side argument checks, the axis construction, the admissibility rule and the LDS sizing of
// pnx_curvefit_grid_refine_f64 (pyneapple_amd/csrc/pnx_grid_refine_args.hpp, free of HIP types) as a stand-alone CPU program, built
// with -fsanitize=address,undefined by tests/test_grid_refine_host.py.  Every array is heap-allocated at exactly the size the ABI
// documents, so a read past n_free entries is an AddressSanitizer report.
// With arguments "axis lo hi c hw m" it prints the axis values (the test compares the numpy reference's construction with them).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_grid_refine_args.hpp"

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
    std::vector<double> lo, hi;
    std::vector<int32_t> npts;
    bool with_mean = true, with_centre = true;
    double noise_sd = 0.0;
    int project = 0;
    GridRefineHost H;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), mean(o.n_free, 0.0), centre(o.n_free, 0.5), hw(o.n_free, 0.1), fixed(1, 0.5);
        g_err[0] = 0;
        return grid_refine_check_args(&o, 1, b.data(), y.data(), fixed.data(), lo.data(), hi.data(), project, noise_sd, npts.data(),
                                      with_centre ? centre.data() : nullptr, hw.data(), with_mean ? mean.data() : nullptr, PNX_MEM_HOST, &H);
    }
};

static Call make(int model, int n_all, int n_b, int points) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    for (int i = 0; i < n_all; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.lo.assign(n_all, 0.0);
    c.hi.assign(n_all, 1.0);
    c.npts.assign(n_all, points);
    return c;
}

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "axis")) {
        const RefineAxis r = grid_refine_axis(atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), atoi(argv[6]));
        for (int j = 0; j < r.m; ++j) printf("%.17g\n", grid_refine_value(r, j));
        return 0;
    }
    {
        Call c = make(PNX_MODEL_TRI_REDUCED, 5, 32, 5);  // 5^5 = 3125 atoms
        EXPECT(c.run() == PNX_OK && c.H.n_atoms == 3125 && c.H.mmax == 5 && c.H.s0_row == -1);
        c.npts = {9, 9, 9, 5, 1};  // 3645
        EXPECT(c.run() == PNX_OK && c.H.n_atoms == 3645 && c.H.mmax == 9);
        c.npts = {9, 9, 9, 6, 1};  // 4374 > 4096
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "4374 atoms"));
        c.npts = {8, 8, 8, 8, 1};  // exactly 4096
        EXPECT(c.run() == PNX_OK && c.H.n_atoms == 4096);
        c.npts = {5, 0, 5, 5, 5};
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_points[1]=0"));
        c.npts = {5, 5, 10, 5, 5};
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_points[2]=10"));
        c.npts.assign(5, 2);
        for (double bad : {(double)NAN, (double)HUGE_VAL, -(double)HUGE_VAL}) {
            c.noise_sd = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        }
        c.noise_sd = -1.0;  // <= 0: marginalised
        EXPECT(c.run() == PNX_OK);
        c.noise_sd = 0.02;
        EXPECT(c.run() == PNX_OK);
        c.with_mean = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "mean"));
        c.with_mean = true;
        c.with_centre = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "NULL"));
        c.with_centre = true;
        c.lo[3] = 2.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "free parameter 3"));
        c.lo[3] = -HUGE_VAL;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "free parameter 3"));
        c.lo[3] = 0.0;
        c.project = 1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "S0"));
        c.project = 0;
        const double sig[32] = {1.0};
        c.o.sigma = sig;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "sigma is not built"));
        c.o.sigma = nullptr;
        c.o.t1_mode = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "t1_mode=1 is not built"));
        c.o.t1_mode = 0;
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        const int32_t order[1] = {0};
        c.o.queue_order = order;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "queue_order"));
        c.o.queue_order = nullptr;
        EXPECT(c.run() == PNX_OK);
    }
    {   // projection: the S0 row is found and must hold one point
        Call c = make(PNX_MODEL_BI_S0, 4, 16, 3);
        c.project = 1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "projected S0"));
        c.npts[3] = 1;
        EXPECT(c.run() == PNX_OK && c.H.s0_row == 3 && c.H.n_atoms == 27);
    }
    {   // the axis: clipping at a bound, one point, b <= a, the last value is the bound itself
        RefineAxis r = grid_refine_axis(0.0, 1.0, 0.9, 0.3, 5);
        EXPECT(r.m == 5 && r.a == 0.9 - 0.3 && r.b == 1.0 && grid_refine_value(r, 4) == 1.0 && grid_refine_value(r, 0) == r.a);
        r = grid_refine_axis(0.0, 1.0, 0.05, 0.3, 4);
        EXPECT(r.m == 4 && r.a == 0.0 && r.b == 0.05 + 0.3);
        r = grid_refine_axis(0.0, 1.0, 0.5, 0.3, 1);
        EXPECT(r.m == 1 && grid_refine_value(r, 0) == 0.5 && r.step == 0.0);
        r = grid_refine_axis(0.0, 1.0, 1.7, 0.3, 9);  // the box lies beyond the bound: b = 1 <= a = 1.4
        EXPECT(r.m == 1 && grid_refine_value(r, 0) == 1.0);
        r = grid_refine_axis(0.0, 1.0, 0.4, 0.0, 9);
        EXPECT(r.m == 1 && grid_refine_value(r, 0) == 0.4);
        r = grid_refine_axis(0.0, 1.0, -3.0, 0.0, 1);
        EXPECT(r.m == 1 && grid_refine_value(r, 0) == 0.0);
        for (int m = 2; m <= kRefineMaxPoints; ++m) {  // every value inside the bounds, ascending
            r = grid_refine_axis(0.1, 0.7, 0.55, 0.333, m);
            for (int j = 0; j < m; ++j) {
                const double x = grid_refine_value(r, j);
                EXPECT(x >= 0.1 && x <= 0.7 && (j == 0 || x > grid_refine_value(r, j - 1)));
            }
        }
    }
    {   // the fraction-sum rule
        const double in[6] = {0.6, 0.01, 0.4, 0.001, 0.0001, 1.0}, out[6] = {0.6, 0.01, 0.41, 0.001, 0.0001, 1.0};
        EXPECT(grid_refine_admissible(PNX_MODEL_TRI_REDUCED, in) && !grid_refine_admissible(PNX_MODEL_TRI_REDUCED, out));
        EXPECT(grid_refine_admissible(PNX_MODEL_TRI_S0, in) && !grid_refine_admissible(PNX_MODEL_TRI_S0, out));
        EXPECT(grid_refine_admissible(PNX_MODEL_TRI_FULL, out) && grid_refine_admissible(PNX_MODEL_BI_FULL, out) && grid_refine_admissible(PNX_MODEL_MONO, out));
        const double one[4] = {1.0, 0.01, 0.001, 1.0}, more[4] = {1.0000000000000002, 0.01, 0.001, 1.0};
        EXPECT(grid_refine_admissible(PNX_MODEL_BI_REDUCED, one) && !grid_refine_admissible(PNX_MODEL_BI_REDUCED, more));
        EXPECT(grid_refine_admissible(PNX_MODEL_BI_S0, one) && !grid_refine_admissible(PNX_MODEL_BI_S0, more));
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the block: at least two waves inside 64 KB, an odd pitch
        for (int m = 1; m <= kRefineMaxPoints; ++m) {
            const GridRefineBlock B = grid_refine_block(n_b, m);
            EXPECT(B.pitch >= n_b && (B.pitch & 1) && B.waves >= 2 && B.waves <= 4);
            EXPECT(B.per_wave == n_b + PNX_MAX_PARAMS * kRefineMaxPoints + 3 * m * B.pitch && B.waves * B.per_wave * 8 <= 64 * 1024);
        }
    if (failures) return 1;
    printf("grid refine stub ok\n");
    return 0;
}
