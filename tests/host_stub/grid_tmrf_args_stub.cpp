// grid_tmrf_args_stub.cpp -- the host-side checks of the edge-preserving (Student-t) neighbourhood prior's three calls
// (pyneapple_amd/csrc/pnx_grid_tmrf_args.hpp, free of HIP types) as a stand-alone CPU program, built with
// -fsanitize=address,undefined by tests/test_grid_tmrf_host.py.  Every array is heap-allocated at exactly the size the ABI
// documents, so a read or write past it is an AddressSanitizer report.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_grid_tmrf_args.hpp"

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
    int n_atoms = 5, n_nb = 4, n_colours = 2, n_sweeps = 4, mem = PNX_MEM_HOST;
    int64_t n_vox = 6;
    double dof = 4.0, tol = 0.0;
    std::vector<double> atoms, lo, hi, precision;
    std::vector<int64_t> start;
    bool with_sd = true, with_w = true;
    GridPosteriorHost H;
    GridMrfHost M;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y((size_t)n_vox * o.n_b, 1.0), out((size_t)o.n_free * n_vox, 0.0), sd((size_t)o.n_free * n_vox, 0.0);
        std::vector<int32_t> nb((size_t)n_vox * (n_nb > 0 && n_nb <= kGridMrfMaxNeighbours ? n_nb : 1), -1);
        g_err[0] = 0;
        return grid_tmrf_check_args(&o, n_vox, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), 0, nullptr, 0.0, n_nb,
                                    nb.data(), n_colours, start.data(), precision.data(), dof, n_sweeps, tol, out.data(),
                                    with_sd ? sd.data() : nullptr, mem, &H, &M);
    }
    int run_field(int64_t first, int64_t count) {
        std::vector<double> b(o.n_b, 0.0), y((size_t)n_vox * o.n_b, 1.0), out((size_t)o.n_free * n_vox, 0.0), q((size_t)o.n_free * n_vox, 0.0);
        std::vector<double> w((size_t)n_vox, 0.0);
        g_err[0] = 0;
        return grid_tmrf_posterior_field_check_args(&o, n_vox, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), 0, nullptr,
                                                    0.0, first, count, q.data(), with_w ? w.data() : nullptr, precision.data(), out.data(), mem,
                                                    &H, &M);
    }
};

static Call make() {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = PNX_MODEL_BI_S0;
    c.o.n_b = 16;
    for (int i = 0; i < 4; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.atoms.assign((size_t)4 * c.n_atoms, 0.5);
    for (int g = 0; g < c.n_atoms; ++g) c.atoms[g] = 0.1 + 0.8 * g / (c.n_atoms - 1);
    c.lo.assign(4, 0.0);
    c.hi.assign(4, 1.0);
    c.precision.assign(4, 0.0);
    c.precision[0] = 2.0;
    c.start = {0, 3, 6};
    return c;
}

int main() {
    const double inf = HUGE_VAL;
    {   // the driver: dof and sd in front of everything the Gaussian driver refuses
        Call c = make();
        EXPECT(c.run() == PNX_OK && fabs(c.M.range[0] - 0.8) < 1e-15);
        for (double bad : {0.0, -1.0, (double)NAN, inf, -inf}) {
            c.dof = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "dof"));
        }
        c.dof = 1e300;
        EXPECT(c.run() == PNX_OK);
        c.dof = 5e-324;
        EXPECT(c.run() == PNX_OK);
        c.dof = 4.0;
        c.with_sd = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "sd is NULL"));
        c.with_sd = true;
        c.n_nb = 9;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_nb"));
        c.n_nb = 4;
        c.n_sweeps = 101;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_sweeps"));
        c.n_sweeps = 4;
        c.start = {0, 3, 5};
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "from 0 to n_vox"));
        c.start = {0, 3, 6};
        c.precision[1] = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "precision[1]"));
    }
    {   // one weighted colour update: the Gaussian one's checks, field_w required
        Call c = make();
        c.mem = PNX_MEM_DEVICE;
        EXPECT(c.run_field(0, 6) == PNX_OK && c.run_field(6, 0) == PNX_OK && c.run_field(2, 4) == PNX_OK);
        EXPECT(c.run_field(5, 2) == PNX_ERR_INVALID && strstr(g_err, "range"));
        c.with_w = false;
        EXPECT(c.run_field(0, 6) == PNX_ERR_INVALID && strstr(g_err, "field_w is NULL"));
        c.with_w = true;
        c.mem = PNX_MEM_HOST;
        EXPECT(c.run_field(0, 6) == PNX_ERR_INVALID && strstr(g_err, "PNX_MEM_DEVICE"));
    }
    {   // the weighted gather, and K
        std::vector<int32_t> nb(6 * 4, -1), n(6);
        std::vector<double> mean(3 * 6, 0.0), sd(3 * 6, 0.0), q(3 * 6), w(6), centre(3, 0.5), prec(3, 1.0);
        auto run = [&](int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb, double dof, bool with_sd, bool with_w) {
            g_err[0] = 0;
            return grid_tmrf_field_check_args(n_vox, first, count, n_free, n_nb, nb.data(), mean.data(), with_sd ? sd.data() : nullptr, centre.data(),
                                              prec.data(), dof, q.data(), with_w ? w.data() : nullptr, n.data(), PNX_MEM_HOST);
        };
        EXPECT(run(6, 0, 6, 3, 4, 4.0, true, true) == PNX_OK && run(6, 5, 1, 3, 1, 0.25, true, true) == PNX_OK);
        EXPECT(run(6, 0, 6, 3, 4, 0.0, true, true) == PNX_ERR_INVALID && strstr(g_err, "dof"));
        EXPECT(run(6, 0, 6, 3, 4, NAN, true, true) == PNX_ERR_INVALID && strstr(g_err, "dof"));
        EXPECT(run(6, 0, 6, 3, 4, 4.0, false, true) == PNX_ERR_INVALID && strstr(g_err, "sd and field_w"));
        EXPECT(run(6, 0, 6, 3, 4, 4.0, true, false) == PNX_ERR_INVALID && strstr(g_err, "sd and field_w"));
        EXPECT(run(6, 0, 6, 9, 4, 4.0, true, true) == PNX_ERR_INVALID && strstr(g_err, "n_free"));
        EXPECT(run(6, 4, 3, 3, 4, 4.0, true, true) == PNX_ERR_INVALID && strstr(g_err, "range"));
        EXPECT(grid_tmrf_rows(3, prec.data()) == 3);
        prec = {0.0, 2.0, 0.0};
        EXPECT(grid_tmrf_rows(3, prec.data()) == 1 && grid_tmrf_rows(1, prec.data()) == 0);
    }
    if (failures) return 1;
    printf("grid tmrf args stub ok\n");
    return 0;
}
