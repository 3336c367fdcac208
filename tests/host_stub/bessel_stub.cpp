// bessel_stub.cpp -- log_i0e of pyneapple_amd/csrc/pnx_bessel.hpp and the argument checks of the Rician grid posterior
// (pnx_grid_rician_args.hpp, free of HIP types) as a stand-alone CPU program.  tests/test_grid_rician_host.py builds it twice with
// g++: plainly (the bytes the device kernel is compared with) and with -fsanitize=address,undefined.
//   bessel_stub IN OUT   reads the doubles of file IN, writes log_i0e of each to file OUT
//   bessel_stub slab N_B N_FREE   prints the kernel's slab width, waves per block and LDS bytes of that shape
//   bessel_stub          runs the argument checks on exact-size heap arrays and prints "grid rician stub ok"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_bessel.hpp"
#include "pnx_grid_rician_args.hpp"

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

static int evaluate(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<double> z((size_t)bytes / 8), h((size_t)bytes / 8);
    const size_t got = fread(z.data(), 8, z.size(), f);
    fclose(f);
    if (got != z.size()) return 2;
    for (size_t i = 0; i < z.size(); ++i) h[i] = log_i0e(z[i]);
    f = fopen(out, "wb");
    if (!f) return 2;
    const size_t put = fwrite(h.data(), 8, h.size(), f);
    fclose(f);
    return put == h.size() ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc == 3) return evaluate(argv[1], argv[2]);
    if (argc == 4) {  // "slab n_b n_free": the kernel's slab width, waves and LDS bytes of that shape
        const GridRicianSlab r = grid_rician_slab(atoi(argv[2]), atoi(argv[3]));
        printf("%d %d %d\n", r.slab.width, r.waves, r.lds_doubles * 8);
        return 0;
    }
    const double inf = HUGE_VAL;
    EXPECT(log_i0e(0.0) == 0.0 && std::isnan(log_i0e(-1.0)) && std::isnan(log_i0e(NAN)) && std::isnan(log_i0e(-0x1p-1074)));
    EXPECT(std::isfinite(log_i0e(1e300)) && std::isfinite(log_i0e(0x1p-1074)) && log_i0e(inf) == -inf);
    for (int n_atoms : {1, 17, 4096}) {
        pnx_curvefit_opts o;
        memset(&o, 0, sizeof(o));
        o.model = PNX_MODEL_BI_REDUCED;
        o.n_b = 16;
        for (int i = 0; i < 3; ++i) o.free_idx[o.n_free++] = i;
        std::vector<double> atoms((size_t)3 * n_atoms, 0.5), lo(3, 0.0), hi(3, 1.0), prior(n_atoms, 0.0), b(16, 0.0), y(16, 1.0), mean(3, 0.0);
        GridPosteriorHost H;
        auto run = [&](double noise_sd) {
            g_err[0] = 0;
            return grid_rician_check_args(&o, 1, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), prior.data(), noise_sd,
                                          mean.data(), PNX_MEM_HOST, &H);
        };
        EXPECT(run(0.05) == PNX_OK && H.s0_row == -1);
        for (double bad : {0.0, -0.05, (double)NAN, inf, -inf}) EXPECT(run(bad) == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        std::vector<double> sigma(16, 1.0);
        o.sigma = sigma.data();
        EXPECT(run(0.05) == PNX_ERR_UNSUPPORTED && strstr(g_err, "sigma"));
        o.sigma = nullptr;
        atoms[(size_t)n_atoms + n_atoms - 1] = 1.5;  // grid start's refusal, unchanged
        EXPECT(run(0.05) == PNX_ERR_INVALID && strstr(g_err, "parameter 1"));
        atoms[(size_t)n_atoms + n_atoms - 1] = 0.5;
        prior[n_atoms - 1] = inf;
        EXPECT(run(0.05) == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: whole tiles and the signal rows inside 64 KB
        for (int n_free = 1; n_free <= PNX_MAX_PARAMS; ++n_free) {
            const GridRicianSlab r = grid_rician_slab(n_b, n_free);
            const GridSlab &s = r.slab;
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.width >= 16 && s.width % 16 == 0 && s.stride >= s.width && s.stride % 32 == 16);
            EXPECT((r.waves == 4 || r.waves == 2) && r.ypitch >= s.kpad);
            EXPECT(r.lds_doubles == s.kpad * s.stride + (3 + n_free) * s.width + r.waves * 16 * r.ypitch && r.lds_doubles * 8 <= 64 * 1024);
        }
    double one = 1.0;
    EXPECT(log_i0e_check_args(0, nullptr, nullptr, PNX_MEM_HOST) == PNX_OK && log_i0e_check_args(1, &one, &one, PNX_MEM_DEVICE) == PNX_OK);
    EXPECT(log_i0e_check_args(-1, &one, &one, PNX_MEM_HOST) == PNX_ERR_INVALID && log_i0e_check_args(1, nullptr, &one, PNX_MEM_HOST) == PNX_ERR_INVALID);
    EXPECT(log_i0e_check_args(1, &one, &one, 7) == PNX_ERR_INVALID);
    if (failures) return 1;
    printf("grid rician stub ok\n");
    return 0;
}
