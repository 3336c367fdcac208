// grid_mrf_args_stub.cpp -- the host-side checks of the neighbourhood (MRF) prior's three calls, the per-atom row r_g, the
// centres and ranges, the report of a driver call and the LDS slab sizing (pyneapple_amd/csrc/pnx_grid_mrf_args.hpp, free of HIP
// types) as a stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_grid_mrf_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read or write past it is an AddressSanitizer report.  With the
// arguments "n_b n_free" it prints the slab width of that shape (the test compares api.grid_mrf_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_grid_mrf_args.hpp"

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
    int n_atoms = 5, n_nb = 4, n_colours = 2, n_sweeps = 4, project = 0, mem = PNX_MEM_HOST;
    int64_t n_vox = 6;
    double tol = 0.0, noise_sd = 0.0;
    std::vector<double> atoms, lo, hi, prior, precision;
    std::vector<int64_t> start;
    bool with_prior = false, with_nb = true, with_start = true, with_precision = true, with_out = true;
    GridPosteriorHost H;
    GridMrfHost M;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y((size_t)n_vox * o.n_b, 1.0), out((size_t)o.n_free * n_vox, 0.0);
        std::vector<int32_t> nb((size_t)n_vox * (n_nb > 0 && n_nb <= kGridMrfMaxNeighbours ? n_nb : 1), -1);  // a refused count sizes nothing
        g_err[0] = 0;
        return grid_mrf_check_args(&o, n_vox, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), project,
                                   with_prior ? prior.data() : nullptr, noise_sd, n_nb, with_nb ? nb.data() : nullptr, n_colours,
                                   with_start ? start.data() : nullptr, with_precision ? precision.data() : nullptr, n_sweeps, tol,
                                   with_out ? out.data() : nullptr, mem, &H, &M);
    }
    int run_field(int64_t first, int64_t count) {
        std::vector<double> b(o.n_b, 0.0), y((size_t)n_vox * o.n_b, 1.0), out((size_t)o.n_free * n_vox, 0.0), q((size_t)o.n_free * n_vox, 0.0);
        std::vector<int32_t> n((size_t)n_vox, 0);
        g_err[0] = 0;
        return grid_mrf_posterior_field_check_args(&o, n_vox, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), project,
                                                   with_prior ? prior.data() : nullptr, noise_sd, first, count, q.data(), n.data(),
                                                   with_precision ? precision.data() : nullptr, with_out ? out.data() : nullptr, mem, &H, &M);
    }
};

static Call make() {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = PNX_MODEL_BI_S0;
    c.o.n_b = 16;
    for (int i = 0; i < 4; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.atoms.assign((size_t)4 * c.n_atoms, 0.5);
    for (int g = 0; g < c.n_atoms; ++g) c.atoms[g] = 0.1 + 0.8 * g / (c.n_atoms - 1);  // row 0: 0.1 .. 0.9
    c.lo.assign(4, 0.0);
    c.hi.assign(4, 1.0);
    c.prior.assign(c.n_atoms, 0.0);
    c.precision.assign(4, 0.0);
    c.precision[0] = 2.0;
    c.start = {0, 3, 6};
    return c;
}

int main(int argc, char **argv) {
    if (argc == 3) {
        printf("%d\n", grid_mrf_slab(atoi(argv[1]), atoi(argv[2])).width);
        return 0;
    }
    const double inf = HUGE_VAL;
    {   // the driver's refusals, each by its message, behind the posterior's own
        Call c = make();
        EXPECT(c.run() == PNX_OK && fabs(c.M.range[0] - 0.8) < 1e-15 && c.M.range[1] == 0.0 && fabs(c.H.centre[0] - 0.5) < 1e-15);
        c.noise_sd = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.with_out = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "mean"));
        c.with_out = true;
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
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
        c.precision[2] = 0.0;
        c.project = 1;  // S0 is free parameter 3 of bi_s0
        EXPECT(c.run() == PNX_OK && c.H.s0_row == 3 && c.M.range[3] == 0.0);
        c.precision[3] = 1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "projected S0"));
        c.project = 0;
        EXPECT(c.run() == PNX_OK);  // unprojected, the S0 row is a grid row like any other
        c.precision[3] = 0.0;
        // ranges and centres over the admissible atoms only
        c.with_prior = true;
        c.prior[0] = c.prior[1] = -inf;
        EXPECT(c.run() == PNX_OK && fabs(c.M.range[0] - 0.4) < 1e-15 && fabs(c.H.centre[0] - 0.7) < 1e-15);
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
    }
    {   // the gather
        std::vector<int32_t> nb(6 * 4, -1), n(6);
        std::vector<double> mean(3 * 6, 0.0), q(3 * 6), centre(3, 0.5), prec(3, 1.0);
        auto run = [&](int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb) {
            g_err[0] = 0;
            return grid_mrf_field_check_args(n_vox, first, count, n_free, n_nb, nb.data(), mean.data(), centre.data(), prec.data(), q.data(), n.data(),
                                             PNX_MEM_HOST);
        };
        EXPECT(run(6, 0, 6, 3, 4) == PNX_OK && run(6, 5, 1, 3, 1) == PNX_OK);
        EXPECT(run(6, 0, 6, 0, 4) == PNX_ERR_INVALID && strstr(g_err, "n_free"));
        EXPECT(run(6, 0, 6, 9, 4) == PNX_ERR_INVALID && strstr(g_err, "n_free"));
        EXPECT(run(6, 0, 6, 3, 0) == PNX_ERR_INVALID && strstr(g_err, "n_nb"));
        EXPECT(run(6, 0, 6, 3, 9) == PNX_ERR_INVALID && strstr(g_err, "n_nb"));
        EXPECT(run(6, 4, 3, 3, 4) == PNX_ERR_INVALID && strstr(g_err, "range"));
        EXPECT(run((int64_t)INT32_MAX + 1, 0, 1, 3, 4) == PNX_ERR_INVALID && strstr(g_err, "n_vox"));
        prec[1] = -1.0;
        EXPECT(run(6, 0, 6, 3, 4) == PNX_ERR_INVALID && strstr(g_err, "precision[1]"));
        prec[1] = 1.0;
        centre[2] = NAN;
        EXPECT(run(6, 0, 6, 3, 4) == PNX_ERR_INVALID && strstr(g_err, "centre[2]"));
    }
    {   // r_g: k ascending, about the centres, 0 for padded atoms; the delta scales; the report
        const int n_free = 3, G = 5, gp = 16;
        std::vector<double> atoms((size_t)n_free * G), centre(n_free), prec = {2.0, 0.0, 0.5}, r(gp, 7.0);
        for (int k = 0; k < n_free; ++k) {
            centre[k] = 1000.0 * k + 0.5;
            for (int g = 0; g < G; ++g) atoms[(size_t)k * G + g] = 1000.0 * k + 0.25 * g;
        }
        grid_mrf_r(n_free, G, gp, atoms.data(), centre.data(), prec.data(), r.data());
        for (int g = 0; g < gp; ++g) {
            const double t = 0.25 * g - 0.5;
            EXPECT(r[g] == (g < G ? 2.0 * (t * t) + 0.0 + 0.5 * (t * t) : 0.0));
        }
        GridMrfHost M;
        grid_mrf_ranges(n_free, G, atoms.data(), nullptr, 1, &M);
        EXPECT(M.range[0] == 1.0 && M.range[1] == 0.0 && M.range[2] == 1.0);
        double scale[PNX_MAX_PARAMS];
        grid_mrf_delta_scale(n_free, prec.data(), M, scale);
        EXPECT(scale[0] == 1.0 && scale[1] == 0.0 && scale[2] == 1.0 && scale[3] == 0.0 && scale[PNX_MAX_PARAMS - 1] == 0.0);
        EXPECT(grid_mrf_any_precision(n_free, prec.data()));
        prec = {0.0, 0.0, 0.0};
        EXPECT(!grid_mrf_any_precision(n_free, prec.data()));
        for (int n_sweeps : {0, 1, 5}) {
            std::vector<double> trace((size_t)n_sweeps + 1, 0.25), delta((size_t)n_sweeps, 3.0);
            int done = -1;
            grid_mrf_report(n_sweeps, n_sweeps ? 1 : 0, trace.data(), delta.data(), &done);
            EXPECT(done == (n_sweeps ? 1 : 0));
            for (int s = 0; s < n_sweeps; ++s) EXPECT(s < 1 ? delta[s] == 0.25 : std::isnan(delta[s]));
            grid_mrf_report(n_sweeps, 0, trace.data(), nullptr, nullptr);  // both outputs optional
        }
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: inside 64 KB for every n_b x n_free, never wider than the posterior's
        for (int n_free = 1; n_free <= PNX_MAX_PARAMS; ++n_free) {
            const GridSlab s = grid_mrf_slab(n_b, n_free);
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.stride >= s.width && s.stride % 32 == 16);
            EXPECT(s.lds_doubles == s.kpad * s.stride + (4 + n_free) * s.width + kGridMrfReduceDoubles && s.lds_doubles * 8 <= 64 * 1024);
            EXPECT(s.width <= grid_posterior_slab(n_b, n_free).width);
        }
    if (failures) return 1;
    printf("grid mrf args stub ok\n");
    return 0;
}
