// varpro_mrf_args_stub.cpp -- the host-side checks of the neighbourhood (MRF) prior over the variable projection's dictionary,
// the per-atom row r_g, the ranges and the LDS slab sizing (pyneapple_amd/csrc/pnx_varpro_mrf_args.hpp, free of HIP types) as a
// stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_varpro_mrf_host.py.  Every array is heap-allocated
// at exactly the size the ABI documents, so a read or write past it is an AddressSanitizer report.  With the arguments "n_b k" it
// prints the slab width of that shape and the posterior's (the test compares api.varpro_mrf_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_varpro_mrf_args.hpp"

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

// bi_s0: free parameters f1, D1, D2, S0; the rows of nl_atoms are D1, D2
struct Call {
    pnx_curvefit_opts o;
    int n_atoms = 5, n_nb = 4, n_colours = 2, n_sweeps = 4, marginal = 1, mem = PNX_MEM_HOST;
    int64_t n_vox = 6;
    double tol = 0.0, noise_sd = 0.0;
    std::vector<double> nl, lo, hi, prior, precision;
    std::vector<int64_t> start;
    bool with_prior = false, with_nb = true, with_start = true, with_precision = true, with_out = true;
    VarproLayout L;
    VarproPosteriorHost H;
    VarproMrfHost M;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y((size_t)n_vox * o.n_b, 1.0), out((size_t)o.n_free * n_vox, 0.0);
        for (int i = 0; i < o.n_b; ++i) b[i] = 50.0 * i;
        std::vector<int32_t> nb((size_t)n_vox * (n_nb > 0 && n_nb <= kGridMrfMaxNeighbours ? n_nb : 1), -1);  // a refused count sizes nothing
        g_err[0] = 0;
        return varpro_mrf_check_args(&o, n_vox, b.data(), y.data(), n_atoms, nl.data(), nullptr, lo.data(), hi.data(),
                                     with_prior ? prior.data() : nullptr, noise_sd, marginal, n_nb, with_nb ? nb.data() : nullptr, n_colours,
                                     with_start ? start.data() : nullptr, with_precision ? precision.data() : nullptr, n_sweeps, tol,
                                     with_out ? out.data() : nullptr, mem, &L, &H, &M);
    }
    int run_field(int64_t first, int64_t count) {
        std::vector<double> b(o.n_b, 0.0), y((size_t)n_vox * o.n_b, 1.0), out((size_t)o.n_free * n_vox, 0.0), q((size_t)o.n_free * n_vox, 0.0);
        for (int i = 0; i < o.n_b; ++i) b[i] = 50.0 * i;
        std::vector<int32_t> n((size_t)n_vox, 0);
        g_err[0] = 0;
        return varpro_mrf_posterior_field_check_args(&o, n_vox, b.data(), y.data(), n_atoms, nl.data(), nullptr, lo.data(), hi.data(),
                                                     with_prior ? prior.data() : nullptr, noise_sd, marginal, first, count, q.data(), n.data(),
                                                     with_precision ? precision.data() : nullptr, with_out ? out.data() : nullptr, mem, &L, &H,
                                                     &M);
    }
};

static Call make() {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = PNX_MODEL_BI_S0;
    c.o.n_b = 16;
    for (int i = 0; i < 4; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.nl.assign((size_t)2 * c.n_atoms, 0.0);
    for (int g = 0; g < c.n_atoms; ++g) {
        c.nl[g] = 0.02 + 0.02 * g;                    // D1: 0.02 .. 0.10
        c.nl[c.n_atoms + g] = 0.001 + 0.0005 * g;     // D2: 0.001 .. 0.003
    }
    c.lo = {0.0, 1e-4, 1e-4, 0.0};
    c.hi = {1.0, 1.0, 1.0, 10.0};
    c.prior.assign(c.n_atoms, 0.0);
    c.precision = {0.0, 2.0, 0.5, 0.0};
    c.start = {0, 3, 6};
    return c;
}

int main(int argc, char **argv) {
    if (argc == 3) {
        printf("%d %d\n", varpro_mrf_slab(atoi(argv[1]), atoi(argv[2])).width, varpro_posterior_slab(atoi(argv[1]), atoi(argv[2])).width);
        return 0;
    }
    const double inf = HUGE_VAL;
    {   // the driver's refusals, each by its message, behind the posterior's own
        Call c = make();
        EXPECT(c.run() == PNX_OK);
        EXPECT(c.M.range[0] == 0.0 && fabs(c.M.range[1] - 0.08) < 1e-15 && fabs(c.M.range[2] - 0.002) < 1e-15 && c.M.range[3] == 0.0);
        EXPECT(c.H.centre[0] == 0.0 && fabs(c.H.centre[1] - 0.06) < 1e-15 && c.H.centre[3] == 0.0);
        c.noise_sd = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.marginal = 2;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "marginal_amplitudes"));
        c.marginal = 1;
        c.with_out = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "mean"));
        c.with_out = true;
        for (int bad : {0, -1, 9, 1 << 30}) {
            c.n_nb = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_nb"));
        }
        c.n_nb = 8;
        EXPECT(c.run() == PNX_OK);
        for (int bad : {0, 9}) {
            c.n_colours = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_colours"));  // refused before colour_start is read
        }
        c.n_colours = 2;
        for (int bad : {-1, 101}) {
            c.n_sweeps = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_sweeps"));
        }
        c.n_sweeps = 0;
        EXPECT(c.run() == PNX_OK);
        c.n_sweeps = 100;
        for (double bad : {-1.0, (double)NAN, inf}) {
            c.tol = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "tol"));
        }
        c.tol = 0.0;
        c.with_nb = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "neighbours"));
        c.with_nb = true;
        c.with_start = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "colour_start is NULL"));
        c.with_start = true;
        c.start = {1, 3, 6};
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "from 0 to n_vox"));
        c.start = {0, 3, 5};
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "from 0 to n_vox"));
        c.n_colours = 3;
        c.start = {0, 4, 3, 6};
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "not ascending at colour 1"));
        c.start = {0, 3, 3, 6};  // an empty colour is fine
        EXPECT(c.run() == PNX_OK);
        c.with_precision = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "precision is NULL"));
        c.with_precision = true;
        for (double bad : {-1.0, (double)NAN, inf}) {
            c.precision[2] = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "precision[2]"));
        }
        c.precision[2] = 0.5;
        for (int row : {0, 3}) {  // the fraction and S0: no grid value
            c.precision[row] = 1.0;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "fraction / S0 row") && strstr(g_err, row ? "precision[3]" : "precision[0]"));
            c.precision[row] = 0.0;
        }
        EXPECT(c.run() == PNX_OK);
        // ranges and centres over the admissible atoms only
        c.with_prior = true;
        c.prior[0] = c.prior[1] = -inf;
        EXPECT(c.run() == PNX_OK && fabs(c.M.range[1] - 0.04) < 1e-15 && fabs(c.H.centre[1] - 0.08) < 1e-15);
    }
    {   // one colour update: device memory only, the range inside the voxels
        Call c = make();
        c.mem = PNX_MEM_DEVICE;
        EXPECT(c.run_field(0, 6) == PNX_OK && c.run_field(6, 0) == PNX_OK && c.run_field(2, 4) == PNX_OK);
        for (auto r : {std::pair<int64_t, int64_t>{-1, 2}, {0, 7}, {5, 2}, {7, 0}, {0, -1}, {INT64_MAX, 2}, {2, INT64_MAX}}) {
            EXPECT(c.run_field(r.first, r.second) == PNX_ERR_INVALID && strstr(g_err, "range"));
        }
        c.mem = PNX_MEM_HOST;
        EXPECT(c.run_field(0, 6) == PNX_ERR_INVALID && strstr(g_err, "PNX_MEM_DEVICE"));
        c.mem = PNX_MEM_DEVICE;
        c.precision[1] = -2.0;
        EXPECT(c.run_field(0, 6) == PNX_ERR_INVALID && strstr(g_err, "precision[1]"));
        c.precision[1] = 2.0;
        c.precision[0] = 0.25;
        EXPECT(c.run_field(0, 6) == PNX_ERR_INVALID && strstr(g_err, "fraction / S0 row"));
    }
    {   // r_g: the non-linear rows only, k ascending, about the centres, 0 for padded atoms
        Call c = make();
        EXPECT(c.run() == PNX_OK);
        const int gp = 16;
        std::vector<double> r(gp, 7.0);
        varpro_mrf_r(c.o.n_free, c.L, c.n_atoms, gp, c.nl.data(), c.H.centre, c.precision.data(), r.data());
        for (int g = 0; g < gp; ++g) {
            const double t1 = c.nl[g < c.n_atoms ? g : 0] - c.H.centre[1], t2 = c.nl[c.n_atoms + (g < c.n_atoms ? g : 0)] - c.H.centre[2];
            double s = 0.0;
            s += 2.0 * (t1 * t1);
            s += 0.5 * (t2 * t2);
            EXPECT(r[g] == (g < c.n_atoms ? s : 0.0));
        }
        GridMrfHost G;
        for (int k = 0; k < PNX_MAX_PARAMS; ++k) G.range[k] = c.M.range[k];
        double scale[PNX_MAX_PARAMS];
        grid_mrf_delta_scale(c.o.n_free, c.precision.data(), G, scale);
        EXPECT(scale[0] == 0.0 && scale[1] == c.M.range[1] && scale[2] == c.M.range[2] && scale[3] == 0.0);
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: inside 64 KB for every n_b x k, never wider than the posterior's
        for (int k = 1; k <= 3; ++k) {
            const GridSlab s = varpro_mrf_slab(n_b, k);
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.stride >= s.width && s.stride % 32 == 16);
            EXPECT(s.lds_doubles == k * s.kpad * s.stride + (varpro_const_rows(k) + k + 3) * s.width + kGridMrfReduceDoubles);
            EXPECT(s.lds_doubles <= 8192 && s.width <= varpro_posterior_slab(n_b, k).width);
        }
    if (failures) return 1;
    printf("varpro mrf args stub ok\n");
    return 0;
}
