// varpro_marginal_args_stub.cpp -- the host-side argument checks, the table of global bin indices and the choice of the
// instantiation of pnx_curvefit_varpro_marginals_f64 (pyneapple_amd/csrc/pnx_varpro_marginal_args.hpp, free of HIP types) as a
// stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_varpro_marginals_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read past n_free bin counts, n_free x n_atoms bins, B bin values,
// n_nl x n_atoms atoms or n_q levels is an AddressSanitizer report.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnx_varpro_marginal_args.hpp"

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

// A call of a layout with every parameter free over a complete Cartesian grid of its K rates: rate j takes the values
// (200 j + i + 1) / 1000, i < per[j] (no two rates of an atom equal), the last rate fastest.
struct Call {
    pnx_curvefit_opts o;
    VarproLayout lay;
    int n_atoms = 1, n_q = 0, marginal_amplitudes = 1;
    std::vector<int32_t> n_bins, bin_of;
    std::vector<double> nl, lo, hi, bin_value, probs, log_prior;
    bool with_marginal = true, with_quantile = true, with_probs = true, with_bins = true, with_prior = false;
    double noise_sd = 0.0;
    VarproLayout L;
    VarproPosteriorHost H;
    GridMarginalHost M;
    int run() {
        std::vector<double> b(o.n_b, 0.0), y(o.n_b, 1.0), out(1, 0.0);
        g_err[0] = 0;
        return varpro_marginal_check_args(&o, 1, b.data(), y.data(), n_atoms, nl.data(), nullptr, lo.data(), hi.data(),
                                          with_prior ? log_prior.data() : nullptr, noise_sd, marginal_amplitudes,
                                          with_bins ? n_bins.data() : nullptr, bin_of.data(), bin_value.data(), n_q,
                                          with_probs ? probs.data() : nullptr, with_marginal ? out.data() : nullptr,
                                          with_quantile ? out.data() : nullptr, PNX_MEM_HOST, &L, &H, &M);
    }
};

static int n_params(int model) {
    switch (model) {
    case PNX_MODEL_MONO: return 2;
    case PNX_MODEL_BI_REDUCED: return 3;
    case PNX_MODEL_BI_S0: case PNX_MODEL_BI_FULL: return 4;
    case PNX_MODEL_TRI_REDUCED: return 5;
    }
    return 6;
}

static Call make(int model, int n_b, std::vector<int> per, std::vector<double> probs = {}) {
    Call c;
    memset(&c.o, 0, sizeof(c.o));
    c.o.model = model;
    c.o.n_b = n_b;
    const int n = n_params(model);
    for (int i = 0; i < n; ++i) c.o.free_idx[c.o.n_free++] = i;
    varpro_layout(model, &c.lay);
    const int K = c.lay.k;
    c.n_atoms = 1;
    for (int j = 0; j < K; ++j) c.n_atoms *= per[j];
    c.n_bins.assign(n, 0);
    c.bin_of.assign((size_t)n * c.n_atoms, 0);
    c.nl.assign((size_t)K * c.n_atoms, 0.0);
    c.lo.assign(n, 0.0);
    c.hi.assign(n, 1.0);
    int rep = c.n_atoms, off = 0;
    for (int j = 0; j < K; ++j) {  // rate j is free parameter rate_pos[j] (every parameter is free) and row j of nl_atoms
        const int k = c.lay.rate_pos[j];
        c.n_bins[k] = per[j];
        for (int i = 0; i < per[j]; ++i) c.bin_value.push_back((200.0 * j + i + 1.0) / 1000.0);
        rep /= per[j];
        for (int g = 0; g < c.n_atoms; ++g) {
            const int i = (g / rep) % per[j];
            c.bin_of[(size_t)k * c.n_atoms + g] = i;
            c.nl[(size_t)j * c.n_atoms + g] = c.bin_value[off + i];
        }
        off += per[j];
    }
    c.probs = probs;
    c.n_q = (int)probs.size();
    if (c.probs.empty()) c.probs.push_back(0.5);
    c.log_prior.assign(c.n_atoms, 0.0);
    return c;
}

int main() {
    const double inf = HUGE_VAL;
    {   // a valid call: tri S0 = (f1, D1, f2, D2, D3, S0); the offsets, the rows, the total
        Call c = make(PNX_MODEL_TRI_S0, 16, {3, 4, 2}, {0.025, 0.5, 0.975});
        EXPECT(c.run() == PNX_OK);
        EXPECT(c.M.n_bins_total == 9 && c.M.n_rows == 3 && c.M.off[1] == 0 && c.M.off[3] == 3 && c.M.off[4] == 7 && c.M.off[5] == 9);
        EXPECT(c.M.n_bins[0] == 0 && c.M.n_bins[1] == 3 && c.M.n_bins[2] == 0 && c.M.n_bins[3] == 4 && c.M.n_bins[4] == 2 && c.M.n_bins[5] == 0);
        EXPECT(c.L.k == 3 && c.L.n_nl == 3 && c.L.row_src[1] == 0 && c.L.row_src[3] == 1 && c.L.row_src[4] == 2 && c.L.row_src[0] < 0);
        // the table: one row per parameter with a marginal, global bin indices, -1 for the padded atoms
        const int gp = (c.n_atoms + 15) & ~15;
        EXPECT(c.n_atoms == 24 && gp == 32);
        std::vector<int32_t> table((size_t)c.M.n_rows * gp, 77);
        grid_marginal_table(c.o.n_free, c.n_atoms, gp, c.M, c.bin_of.data(), table.data());
        for (int g = 0; g < gp; ++g) {
            if (g < c.n_atoms) {
                EXPECT(table[g] == c.bin_of[1 * c.n_atoms + g] && table[gp + g] == 3 + c.bin_of[3 * c.n_atoms + g] &&
                       table[2 * gp + g] == 7 + c.bin_of[4 * c.n_atoms + g]);
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
        // bins on a linear row: a fraction, S0
        c.n_bins[0] = 2;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_bins[0]=2") && strstr(g_err, "linear row"));
        c.n_bins[0] = 0;
        c.n_bins[5] = 1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_bins[5]=1") && strstr(g_err, "linear row"));
        c.n_bins[5] = 0;
        c.bin_of[0 * c.n_atoms + 5] = 99;  // a row with n_bins == 0 is not read
        EXPECT(c.run() == PNX_OK);
        // a bin out of range, an atom off its bin's value, values that do not ascend
        c.bin_of[3 * c.n_atoms + 5] = 4;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_of[3, 5]=4"));
        c.bin_of[3 * c.n_atoms + 5] = -1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_of[3, 5]=-1"));
        const int keep = (5 / 2) % 4;
        c.bin_of[3 * c.n_atoms + 5] = (keep + 1) % 4;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 5, free parameter 3"));
        c.bin_of[3 * c.n_atoms + 5] = keep;
        EXPECT(c.run() == PNX_OK);
        const double v = c.bin_value[4];
        c.bin_value[4] = std::nextafter(v, 1.0);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom") && strstr(g_err, "bin_value[4]"));
        c.bin_value[4] = c.bin_value[3];
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_value[4]") && strstr(g_err, "ascending"));
        c.bin_value[4] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "bin_value[4]"));
        c.bin_value[4] = v;
        c.n_bins[1] = -1;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_bins[1]=-1"));
        c.n_bins[1] = 3;
        // a non-linear row may go without bins
        c.n_bins[4] = 0;
        c.bin_value.resize(7);
        EXPECT(c.run() == PNX_OK && c.M.n_rows == 2 && c.M.n_bins_total == 7);
        c.n_bins[4] = 2;
        c.bin_value.push_back(0.401);
        c.bin_value.push_back(0.402);
        EXPECT(c.run() == PNX_OK);
        // the posterior's refusals, inherited through its own check, and the variable projection's through the posterior's
        c.noise_sd = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "noise_sd"));
        c.noise_sd = 0.0;
        c.marginal_amplitudes = 2;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "marginal_amplitudes=2"));
        c.marginal_amplitudes = 0;
        EXPECT(c.run() == PNX_OK);
        c.with_prior = true;
        c.log_prior[3] = NAN;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.log_prior.assign(c.n_atoms, -inf);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "log_prior"));
        c.log_prior[7] = -2.0;  // one admissible atom
        EXPECT(c.run() == PNX_OK);
        c.with_prior = false;
        const double a3 = c.nl[3];
        c.nl[3] = 1.5;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "atom 3") && strstr(g_err, "bounds"));
        c.nl[3] = a3;
        c.lo[5] = -1.0;
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "lo_S0"));
        c.lo[5] = 0.0;
        c.o.per_voxel_p0_bounds = 1;
        EXPECT(c.run() == PNX_ERR_UNSUPPORTED && strstr(g_err, "per_voxel_p0_bounds"));
        c.o.per_voxel_p0_bounds = 0;
        c.o.n_b = 3;  // n_b must exceed the K amplitudes
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "n_b=3"));
        c.o.n_b = 4;
        EXPECT(c.run() == PNX_OK);
    }
    {   // every layout accepts its rates
        const int models[7] = {PNX_MODEL_MONO, PNX_MODEL_BI_REDUCED, PNX_MODEL_BI_S0, PNX_MODEL_BI_FULL, PNX_MODEL_TRI_REDUCED, PNX_MODEL_TRI_S0,
                               PNX_MODEL_TRI_FULL};
        for (int model : models) {
            Call c = make(model, 8, {3, 2, 2});
            EXPECT(c.run() == PNX_OK && c.M.n_rows == c.L.k && c.M.n_bins_total == (c.L.k == 1 ? 3 : c.L.k == 2 ? 5 : 7));
        }
    }
    {   // B = 0, B = 1, B = 128, B = 129
        Call c = make(PNX_MODEL_BI_REDUCED, 16, {2, 2});
        c.n_bins.assign(3, 0);
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "B = sum n_bins = 0"));
        c = make(PNX_MODEL_MONO, 16, {1});
        EXPECT(c.run() == PNX_OK && c.M.n_bins_total == 1 && c.M.n_rows == 1 && c.M.off[1] == 0);
        c = make(PNX_MODEL_BI_REDUCED, 16, {64, 64});
        EXPECT(c.n_atoms == 4096 && c.run() == PNX_OK && c.M.n_bins_total == 128);
        c = make(PNX_MODEL_BI_REDUCED, 16, {64, 64});
        c.n_bins[1] = 65;  // the bins are counted before the atoms are looked at
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "B = sum n_bins = 129"));
        c = make(PNX_MODEL_MONO, 16, {128});
        EXPECT(c.run() == PNX_OK && c.M.n_bins_total == 128);
        c = make(PNX_MODEL_MONO, 16, {129});
        EXPECT(c.run() == PNX_ERR_INVALID && strstr(g_err, "129"));
    }
    // the instantiation and the slab: 4 / 8 chunks; the table sits inside the posterior's slab, behind lw, for every n_b and k
    EXPECT(varpro_marginal_chunks(1) == 4 && varpro_marginal_chunks(57) == 4 && varpro_marginal_chunks(64) == 4);
    EXPECT(varpro_marginal_chunks(65) == 8 && varpro_marginal_chunks(128) == 8);
    for (int k = 1; k <= 3; ++k)
        for (int n_b = k + 1; n_b <= PNX_MAX_BVALUES; ++n_b) {
            const GridSlab s = varpro_marginal_slab(n_b, k), p = varpro_posterior_slab(n_b, k);
            EXPECT(s.width == p.width && s.stride == p.stride && s.lds_doubles == p.lds_doubles && s.kpad == p.kpad);
            const size_t used = (size_t)(k * s.kpad * s.stride + (varpro_const_rows(k) + 1) * s.width) * sizeof(double) +
                                (size_t)(k + 1) * s.width * sizeof(int32_t);  // at most k + 1 non-linear rows hold bins
            EXPECT(used <= (size_t)s.lds_doubles * sizeof(double) && s.lds_doubles * 8 <= 64 * 1024 && s.width % 16 == 0 && s.stride >= s.width);
        }
    if (failures) return 1;
    printf("varpro marginal args stub ok\n");
    return 0;
}
