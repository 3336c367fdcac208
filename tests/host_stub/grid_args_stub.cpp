// grid_args_stub.cpp -- the host-side argument checks and the LDS slab sizing of pnx_curvefit_grid_start_f64
// (pyneapple_amd/csrc/pnx_grid_args.hpp, free of HIP types) as a stand-alone CPU program, built with
// -fsanitize=address,undefined by tests/test_grid_start_host.py.  Every array is heap-allocated at exactly the size the ABI
// documents, so a read past n_free * n_atoms atoms or past the n_free bounds is an AddressSanitizer report.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pnx_grid_args.hpp"

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

static pnx_curvefit_opts opts(int model, int n_all, int n_b, int fixed_pos = -1) {
    pnx_curvefit_opts o;
    memset(&o, 0, sizeof(o));
    o.model = model;
    o.n_b = n_b;
    for (int i = 0; i < n_all; ++i) {
        if (i == fixed_pos)
            o.fixed_idx[o.n_fixed++] = i;
        else
            o.free_idx[o.n_free++] = i;
    }
    return o;
}

static int check(const pnx_curvefit_opts &o, int n_atoms, const std::vector<double> &atoms, const std::vector<double> &lo,
                 const std::vector<double> &hi, int project, int *s0_row, bool with_out = true, const double *fixed = nullptr) {
    std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(o.n_free, 0.0);
    return grid_check_args(&o, 1, b.data(), y.data(), n_atoms, atoms.data(), fixed, lo.data(), hi.data(), project, with_out ? out.data() : nullptr,
                           PNX_MEM_HOST, s0_row);
}

int main() {
    int row = 0;
    for (int n_atoms : {1, 15, 16, 17, 4096}) {  // exact-size arrays: the scan stops at n_free * n_atoms
        pnx_curvefit_opts o = opts(PNX_MODEL_TRI_S0, 6, 32);
        std::vector<double> atoms((size_t)6 * n_atoms, 0.5), lo(6, 0.0), hi(6, 1.0);
        EXPECT(check(o, n_atoms, atoms, lo, hi, 0, &row) == PNX_OK && row == -1);
        EXPECT(check(o, n_atoms, atoms, lo, hi, 1, &row) == PNX_OK && row == 5);
        atoms.back() = 1.5;  // the last atom of the last parameter
        EXPECT(check(o, n_atoms, atoms, lo, hi, 0, &row) == PNX_ERR_INVALID && strstr(g_err, "parameter 5"));
        atoms.back() = NAN;
        EXPECT(check(o, n_atoms, atoms, lo, hi, 0, &row) == PNX_ERR_INVALID);
        atoms.back() = 1.0;  // on the bound: inside
        EXPECT(check(o, n_atoms, atoms, lo, hi, 0, &row) == PNX_OK);
    }
    {
        pnx_curvefit_opts o = opts(PNX_MODEL_BI_REDUCED, 3, 16);
        std::vector<double> atoms(3 * 4, 0.5), lo(3, 0.0), hi(3, 1.0);
        EXPECT(check(o, 0, atoms, lo, hi, 0, &row) == PNX_ERR_INVALID);
        EXPECT(check(o, 4097, atoms, lo, hi, 0, &row) == PNX_ERR_INVALID);  // refused before the atoms are read
        EXPECT(check(o, 4, atoms, lo, hi, 1, &row) == PNX_ERR_INVALID && strstr(g_err, "S0"));
        EXPECT(check(o, 4, atoms, lo, hi, 0, &row, false) == PNX_ERR_INVALID);
        o.per_voxel_p0_bounds = 1;
        EXPECT(check(o, 4, atoms, lo, hi, 0, &row) == PNX_ERR_UNSUPPORTED);
        o.per_voxel_p0_bounds = 0;
        const int32_t order[1] = {0};
        o.queue_order = order;
        EXPECT(check(o, 4, atoms, lo, hi, 0, &row) == PNX_ERR_UNSUPPORTED);
    }
    {   // S0 of the mono-exponential model is parameter 0; fixed, there is nothing to project
        pnx_curvefit_opts o = opts(PNX_MODEL_MONO, 2, 8);
        std::vector<double> atoms(2 * 3, 0.5), lo(2, 0.0), hi(2, 1.0);
        EXPECT(check(o, 3, atoms, lo, hi, 1, &row) == PNX_OK && row == 0);
        pnx_curvefit_opts f = opts(PNX_MODEL_MONO, 2, 8, 0);
        std::vector<double> a1(1 * 3, 0.5), l1(1, 0.0), h1(1, 1.0);
        const double fixed[1] = {1.0};
        EXPECT(check(f, 3, a1, l1, h1, 1, &row, true, fixed) == PNX_ERR_INVALID);
        EXPECT(check(f, 3, a1, l1, h1, 0, &row, true, fixed) == PNX_OK);
        EXPECT(check(f, 3, a1, l1, h1, 0, &row, true, nullptr) == PNX_ERR_INVALID);
        f.fixed_per_voxel = 1;
        EXPECT(check(f, 3, a1, l1, h1, 0, &row, true, fixed) == PNX_ERR_UNSUPPORTED);
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b) {  // the slab: whole tiles, inside 64 KB, the two half-waves on opposite bank halves
        const GridSlab s = grid_slab(n_b);
        EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.kpad - n_b < 4);
        EXPECT(s.width >= 16 && s.width <= 256 && s.width % 16 == 0);
        EXPECT(s.stride >= s.width && s.stride % 32 == 16);
        EXPECT(s.lds_doubles == s.kpad * s.stride + 2 * s.width && s.lds_doubles * 8 <= 64 * 1024);
    }
    if (failures) return 1;
    printf("grid args stub ok\n");
    return 0;
}
