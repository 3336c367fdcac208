// grid_marginal_args_stub.cpp -- the host-side argument checks, the table of global bin indices and the choice of the
// instantiation of pnx_curvefit_grid_marginals_f64 (pyneapple_amd/csrc/pnx_grid_marginal_args.hpp, free of HIP types) as a
// stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_grid_marginals_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read past n_free bin counts, n_free x n_atoms bins, B bin values or
// n_q levels is an AddressSanitizer report.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_grid_marginal_args.hpp"

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

// A call over a complete Cartesian grid: parameter k takes the values (j + 1) / (n_bins[k] + 1), the last parameter fastest.
struct Call {
    pnx_curvefit_opts o;
    int n_atoms = 1, project = 0, n_q = 0;
    std::vector<int32_t> n_bins, bin_of;
    std::vector<double> atoms, lo, hi, bin_value, probs;
    bool with_marginal = true, with_quantile = true, with_probs = true, with_bins = true;
    double noise_sd = 0.0;
    GridPosteriorHost H;
    GridMarginalHost M;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(1, 0.0);
        g_err[0] = 0;
        return grid_marginal_check_args(&o, 1, b.data(), y.data(), n_atoms, atoms.data(), nullptr, lo.data(), hi.data(), project, nullptr,
                                        noise_sd, with_bins ? n_bins.data() : nullptr, bin_of.data(), bin_value.data(), n_q,
                                        with_probs ? probs.data() : nullptr, with_marginal ? out.data() : nullptr,
                                        with_quantile ? out.data() : nullptr, PNX_MEM_HOST, &H, &M);
    }
};

static Call make(int model, int n_b, std::vector<int32_t> bins, std::vector<double> probs = {}) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    const int n = (int)bins.size();
    for (int i = 0; i < n; ++i) c.o.free_idx[c.o.n_free++] = i;
    c.n_bins = bins;
    c.n_atoms = 1;
    for (int nb : bins) c.n_atoms *= nb > 0 ? nb : 1;
    c.atoms.assign((size_t)n * c.n_atoms, 0.5);
    c.bin_of.assign((size_t)n * c.n_atoms, 0);
    c.lo.assign(n, 0.0);
    c.hi.assign(n, 1.0);
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < bins[k]; ++j) c.bin_value.push_back((j + 1.0) / (bins[k] + 1.0));
    int rep = c.n_atoms, off = 0;
    for (int k = 0; k < n; ++k) {
        const int nb = bins[k] > 0 ? bins[k] : 1;
        rep /= nb;
        for (int g = 0; g < c.n_atoms && bins[k] > 0; ++g) {
            const int j = (g / rep) % nb;
            c.bin_of[(size_t)k * c.n_atoms + g] = j;
            c.atoms[(size_t)k * c.n_atoms + g] = c.bin_value[off + j];
        }
        off += bins[k];
    }
    c.probs = probs;
    c.n_q = (int)probs.size();
    if (c.bin_value.empty()) c.bin_value.push_back(0.5);  // B = 0: the array may not be NULL, nothing of it is read
    if (c.probs.empty()) c.probs.push_back(0.5);
    return c;
}

int main() {
    const double inf = HUGE_VAL;
    {   // a valid call: the offsets, the rows, the total
        Call c = make(PNX_MODEL_BI_S0, 16, {3, 0, 4, 2}, {0.025, 0.5, 0.975});
        EXPECT(c.run() == PNX_OK);
        EXPECT(c.M.n_bins_total == 9 && c.M.n_rows == 3 && c.M.off[0] == 0 && c.M.off[1] == 3 && c.M.off[2] == 3 && c.M.off[3] == 7);
        EXPECT(c.M.n_bins[1] == 0 && c.M.n_bins[3] == 2);
        // the table: one row per parameter with a marginal, global bin indices, -1 for the padded atoms
        const int gp = (c.n_atoms + 15) & ~15;
        std::vector<int32_t> table((size_t)c.M.n_rows * gp, 77);
        grid_marginal_table(c.o.n_free, c.n_atoms, gp, c.M, c.bin_of.data(), table.data());
        for (int g = 0; g < gp; ++g) {
            if (g < c.n_atoms) {
                EXPECT(table[g] == c.bin_of[g] && table[gp + g] == 3 + c.bin_of[2 * c.n_atoms + g] && table[2 * gp + g] == 7 + c.bin_of[3 * c.n_atoms + g]);
            } else {
                EXPECT(table[g] == -1 && table[gp + g] == -1 && table[2 * gp + g] == -1);
            }
        }
        // NULL outputs and arrays
        c.with_marginal = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "marginal is NULL"));
        c.with_marginal = true;
        c.with_quantile = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "quantile is NULL"));
        c.n_q = 0;  // no levels: quantile may be NULL, and so may probs
        c.with_probs = false;
        EXPECT(c.run() == PNX_OK);
        c.n_q = 3;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "probs is NULL"));
        c.with_probs = c.with_quantile = true;
        c.with_bins = false;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_bins"));
        c.with_bins = true;
        // the levels
        for (int bad : {-1, 9, 1 << 30}) {
            c.n_q = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_q"));
        }
        c.n_q = 3;
        for (double bad : {0.0, 1.0, -0.5, 1.5, (double)NAN, inf}) {
            c.probs[1] = bad;
            EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "probs[1]"));
        }
        c.probs[1] = 0x1p-1074;
        EXPECT(c.run() == PNX_OK);
        c.probs.assign(8, 0.5);  // the most levels
        c.n_q = 8;
        EXPECT(c.run() == PNX_OK);
        // a bin out of range, an atom off its bin's value, values that do not ascend
        c.bin_of[2 * c.n_atoms + 5] = 4;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_of[2, 5]=4"));
        c.bin_of[2 * c.n_atoms + 5] = -1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_of[2, 5]=-1"));
        const int keep = (5 / 2) % 4;
        c.bin_of[2 * c.n_atoms + 5] = (keep + 1) % 4;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 5, free parameter 2"));
        c.bin_of[2 * c.n_atoms + 5] = keep;
        EXPECT(c.run() == PNX_OK);
        c.bin_of[1 * c.n_atoms + 5] = 99;  // a row with n_bins == 0 is not read
        EXPECT(c.run() == PNX_OK);
        const double v = c.bin_value[4];
        c.bin_value[4] = std::nextafter(v, 1.0);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom") && strstr(g_err, "bin_value[4]"));
        c.bin_value[4] = c.bin_value[3];
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_value[4]") && strstr(g_err, "ascending"));
        c.bin_value[4] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_value[4]"));
        c.bin_value[4] = v;
        c.n_bins[0] = -1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_bins[0]=-1"));
        c.n_bins[0] = 3;
        // the posterior's refusals, inherited through its own check
        c.noise_sd = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.atoms[3] = 1.5;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 3") && strstr(g_err, "bounds"));
        c.atoms[3] = c.bin_value[c.bin_of[3]];
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        // projection: the S0 row must hold no bins
        c.project = 1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "S0") && strstr(g_err, "n_bins[3]=2"));
        EXPECT(c.H.s0_row == 3);
    }
    {   // projection with the S0 row at 0 bins; projection without a free S0
        Call c = make(PNX_MODEL_BI_S0, 16, {3, 2, 4, 0});
        c.project = 1;
        EXPECT(c.run() == PNX_OK && c.M.n_rows == 3 && c.M.n_bins_total == 9);
        c.o.model = PNX_MODEL_BI_FULL;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "S0"));
    }
    {   // B = 0, B = 1, B = 128, B = 129
        Call c = make(PNX_MODEL_TRI_REDUCED, 16, {0, 0, 0, 0, 0});
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "B = sum n_bins = 0"));
        c = make(PNX_MODEL_TRI_REDUCED, 16, {0, 0, 1, 0, 0});
        EXPECT(c.run() == PNX_OK && c.M.n_bins_total == 1 && c.M.n_rows == 1 && c.M.off[2] == 0 && c.M.off[3] == 1);
        c = make(PNX_MODEL_BI_REDUCED, 16, {64, 0, 64});
        EXPECT(c.n_atoms == 4096 && c.run() == PNX_OK && c.M.n_bins_total == 128);
        c = make(PNX_MODEL_BI_REDUCED, 16, {65, 0, 64});
        c.n_atoms = 4096;  // the bins are counted before the atoms are looked at
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "B = sum n_bins = 129"));
        c = make(PNX_MODEL_BI_REDUCED, 16, {128, 0, 0});
        EXPECT(c.run() == PNX_OK && c.M.n_bins_total == 128);
        c = make(PNX_MODEL_BI_REDUCED, 16, {129, 0, 0});
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "129"));
    }
    // the instantiation and the slab: 2 / 4 / 8 chunks; the table fits the EM's slab for every n_b
    EXPECT(grid_marginal_chunks(1) == 2 && grid_marginal_chunks(32) == 2 && grid_marginal_chunks(33) == 4 && grid_marginal_chunks(64) == 4);
    EXPECT(grid_marginal_chunks(65) == 8 && grid_marginal_chunks(128) == 8);
    for (int n_b = 1; n_b <= PNX_MAX_BVALUES; ++n_b) {
        const GridSlab s = grid_marginal_slab(n_b);
        const size_t used = (size_t)(s.kpad * s.stride + 3 * s.width) * sizeof(double) + (size_t)PNX_MAX_PARAMS * s.width * sizeof(int32_t);
        EXPECT(used <= (size_t)s.lds_doubles * sizeof(double) && s.lds_doubles * 8 <= 64 * 1024 && s.width % 16 == 0);
    }
    if (failures) return 1;
    printf("grid marginal args stub ok\n");
    return 0;
}
