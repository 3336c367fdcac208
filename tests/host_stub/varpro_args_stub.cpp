// varpro_args_stub.cpp -- the host-side argument checks, the layout tables and the LDS slab sizing of pnx_curvefit_varpro_f64
// (pyneapple_amd/csrc/pnx_varpro_args.hpp, free of HIP types) as a stand-alone CPU program, built with -fsanitize=address,undefined
// by tests/test_varpro_host.py.  Every array is heap-allocated at exactly the size the ABI documents, so a read past
// n_nl * n_atoms atom values or n_free bounds is an AddressSanitizer report.
// With arguments "n_b k" it prints the slab width of that shape (the test compares api.varpro_slab_atoms with it).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_varpro_args.hpp"

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

static const int kAll[7] = {2, 3, 4, 4, 5, 6, 6};    // parameters per model
static const int kComp[7] = {1, 2, 2, 2, 3, 3, 3};   // compartments
static const int kLin[7] = {1, 1, 2, 2, 2, 3, 3};    // linear parameters

struct Call {
    pnx_curvefit_opts o;
    int n_atoms = 0, n_nl = 0;
    std::vector<double> nl, lo, hi, fb, fixed;
    bool with_out = true;
    VarproLayout L;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(o.n_free, 0.0);
        g_err[0] = 0;
        return varpro_check_args(&o, 1, b.data(), y.data(), n_atoms, nl.data(), fixed.empty() ? nullptr : fixed.data(), lo.data(), hi.data(),
                                 fb.data(), with_out ? out.data() : nullptr, PNX_MEM_HOST, &L);
    }
};

// every parameter free but those in `fixed_pos`; atom g holds the rates 0.5 / (j + 1) - g * 1e-5 (distinct within an atom)
static Call make(int model, int n_b, int n_atoms, std::vector<int> fixed_pos = {}, int t1 = 0) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    c.o.t1_mode = t1;
    const int n_all = kAll[model] + (t1 ? 1 : 0);
    for (int i = 0; i < n_all; ++i) {
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
    c.fb.assign(c.o.n_free, 0.25);
    for (size_t f = 0; f < fixed_pos.size(); ++f) c.fixed.push_back(0.9 - 0.01 * f);
    return c;
}

int main(int argc, char **argv) {
    if (argc == 3) {
        printf("%d\n", varpro_slab(atoi(argv[1]), atoi(argv[2])).width);
        return 0;
    }
    for (int model = 0; model < 7; ++model)  // valid edges, exact-size arrays, the layout tables
        for (int n_atoms : {1, 15, 16, 17, 4096}) {
            Call c = make(model, 32, n_atoms);
            EXPECT(c.run() == PNX_OK && c.L.k == kComp[model] && c.L.n_nl == kAll[model] - kLin[model]);
            EXPECT(c.L.n_lin == kLin[model]);
            int lin = 0, nl = 0;
            for (int r = 0; r < c.o.n_free; ++r) {
                if (c.L.row_src[r] < 0) {
                    EXPECT(c.L.lin_row[-1 - c.L.row_src[r]] == r);
                    ++lin;
                } else {
                    EXPECT(c.L.row_src[r] == nl);
                    ++nl;
                }
            }
            EXPECT(lin == kLin[model] && nl == c.L.n_nl);
            Call t = make(model, 32, n_atoms, {}, 1);  // T1 free: one more non-linear row
            EXPECT(t.run() == PNX_OK && t.L.n_nl == kAll[model] - kLin[model] + 1);
        }
    {   // S0 is the last linear slot of the S0 class; the classes
        Call c = make(PNX_MODEL_TRI_S0, 32, 4);
        EXPECT(c.run() == PNX_OK && c.L.cls == kVarproS0 && c.L.lin_row[2] == 5 && c.L.lin_row[0] == 0 && c.L.lin_row[1] == 2);
        c = make(PNX_MODEL_TRI_REDUCED, 32, 4);
        EXPECT(c.run() == PNX_OK && c.L.cls == kVarproReduced && c.L.n_lin == 2);
        c = make(PNX_MODEL_MONO, 2, 4);
        EXPECT(c.run() == PNX_OK && c.L.cls == kVarproFree && c.L.row_src[0] == -1 && c.L.row_src[1] == 0);
    }
    {   // fixed rates and a fixed T1 are served; the fixed rate takes part in the comparison of the rates
        Call c = make(PNX_MODEL_TRI_S0, 32, 4, {4, 6}, 1);
        EXPECT(c.run() == PNX_OK && c.L.n_nl == 2);
        c.fixed[0] = c.nl[1];  // D3 = D1 of atom 1
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 1") && strstr(g_err, "equal rates"));
        Call a = make(PNX_MODEL_BI_REDUCED, 8, 4, {1, 2});  // every rate fixed: no non-linear row is read
        EXPECT(a.run() == PNX_OK && a.L.n_nl == 0);
    }
    {
        Call c = make(PNX_MODEL_TRI_S0, 32, 4);
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        const int32_t order[1] = {0};
        c.o.queue_order = order;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "queue_order"));
        c.o.queue_order = nullptr;
        for (int n_atoms : {0, -1, 4097}) {  // refused before the atoms are read
            c.n_atoms = n_atoms;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_atoms"));
        }
        c.n_atoms = 4;
        for (int n_b : {1, 2, 3}) {
            c.o.n_b = n_b;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_b="));
        }
        c.o.n_b = 4;
        EXPECT(c.run() == PNX_OK);
        c.with_out = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "NULL"));
        c.with_out = true;
        c.nl[4 + 2] = c.nl[2];  // D2 = D1 of atom 2
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 2") && strstr(g_err, "D1 = D2"));
        c.nl[4 + 2] = 1.5;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 2") && strstr(g_err, "outside its bounds"));
        c.nl[4 + 2] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "outside its bounds"));
        c.nl[4 + 2] = 0.2;
        EXPECT(c.run() == PNX_OK);
        c.lo[5] = -1e-300;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "lo_S0"));
        c.lo[5] = 0.0;
        c.lo[0] = 2.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "lo=2"));
        c.lo[0] = 0.0;
        for (double bad : {-0.1, 1.1, (double)NAN}) {
            c.fb[3] = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "fallback[3]"));
        }
        c.fb[3] = 1.0;  // on the bound
        EXPECT(c.run() == PNX_OK);
    }
    {   // a fixed fraction, a fixed S0, per-voxel fixed values
        Call c = make(PNX_MODEL_TRI_S0, 32, 4, {2});
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "parameter 2") && strstr(g_err, "fixed"));
        c = make(PNX_MODEL_BI_S0, 32, 4, {3});
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "parameter 3"));
        c = make(PNX_MODEL_BI_S0, 32, 4, {1});
        c.o.fixed_per_voxel = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "fixed_per_voxel"));
        VarproLayout L;
        EXPECT(varpro_layout(7, &L) == PNX_ERR_INVALID && varpro_layout(-1, &L) == PNX_ERR_INVALID);
    }
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b)  // the slab: whole tiles, inside 64 KB, the half-waves on opposite bank halves
        for (int k = 1; k <= 3; ++k) {
            const GridSlab s = varpro_slab(n_b, k);
            EXPECT(s.kpad >= n_b && s.kpad % 4 == 0 && s.kpad - n_b < 4);
            EXPECT(s.width >= 16 && s.width <= 256 && s.width % 16 == 0 && s.width <= grid_slab(n_b).width);
            EXPECT(s.stride >= s.width && s.stride % 32 == 16);
            EXPECT(s.lds_doubles == k * s.kpad * s.stride + varpro_const_rows(k) * s.width && s.lds_doubles * 8 <= 64 * 1024);
        }
    EXPECT(varpro_slab(128, 3).width == 16 && varpro_const_rows(3) == 12 && varpro_const_rows(1) == 2);
    if (failures) return 1;
    printf("varpro args stub ok\n");
    return 0;
}
