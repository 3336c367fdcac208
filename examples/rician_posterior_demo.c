/* examples/rician_posterior_demo.c -- the grid posterior under a Rician likelihood from plain C: pnx_log_i0e_f64 and
 * pnx_curvefit_grid_posterior_rician_f64 beside pnx_curvefit_grid_posterior_f64 on the same magnitude data.
 *   gcc -std=c99 -Iinclude examples/rician_posterior_demo.c -Lpyneapple_amd -lpnx_hip -Wl,-rpath,$PWD/pyneapple_amd -lm -o rician_demo
 * 512 reduced bi-exponential voxels, 32 b-values up to 2500, noise sd 0.10: at the high b-values the signal sits on the noise
 * floor, which the Gaussian likelihood reads as a slower D2.  Prints the mean signed error of D2 under both likelihoods. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pnx.h"

enum { NV = 512, NB = 32, NF1 = 5, ND1 = 5, ND2 = 12, NA = NF1 * ND1 * ND2 };

static unsigned long long rng_state = 88172645463325252ull;
static double urand(void) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
static double nrand(void) { return sqrt(-2.0 * log(1.0 - urand())) * cos(6.283185307179586 * urand()); }

static int fail(const char *what) {
    char msg[512];
    pnx_last_error(msg, (int)sizeof(msg));
    fprintf(stderr, "%s failed: %s\n", what, msg);
    return 1;
}

int main(void) {
    if (pnx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 1;
    }
    const double z[4] = {0.0, 1.0, 10.0, 1e300};
    double h[4];
    if (pnx_log_i0e_f64(4, z, h, PNX_MEM_HOST, 0, NULL)) return fail("pnx_log_i0e_f64");
    printf("log I0e(0, 1, 10, 1e300) = %.17g %.17g %.17g %.17g\n", h[0], h[1], h[2], h[3]);
    if (h[0] != 0.0 || fabs(h[1] - -0.7640856414928214) > 1e-13) return 2;

    const double sd = 0.10;
    double b[NB], f1v[NF1], d1v[ND1], d2v[ND2];
    for (int i = 0; i < NB; ++i) b[i] = 2500.0 * i / (NB - 1);
    for (int i = 0; i < NF1; ++i) f1v[i] = 0.05 + 0.1 * i;
    for (int i = 0; i < ND1; ++i) d1v[i] = 0.01 * pow(10.0, i / (double)(ND1 - 1));
    for (int i = 0; i < ND2; ++i) d2v[i] = 2e-4 + (3e-3 - 2e-4) * i / (ND2 - 1);
    double *atoms = malloc(sizeof(double) * 3 * NA);
    for (int i = 0, g = 0; i < NF1; ++i)
        for (int j = 0; j < ND1; ++j)
            for (int k = 0; k < ND2; ++k, ++g) {
                atoms[g] = f1v[i];
                atoms[NA + g] = d1v[j];
                atoms[2 * NA + g] = d2v[k];
            }
    double *y = malloc(sizeof(double) * NV * NB), *truth = malloc(sizeof(double) * NV);
    for (int v = 0; v < NV; ++v) {
        const int g = (int)(urand() * NA) % NA;
        truth[v] = atoms[2 * NA + g];
        for (int i = 0; i < NB; ++i) {
            const double m = atoms[g] * exp(-b[i] * atoms[NA + g]) + (1 - atoms[g]) * exp(-b[i] * atoms[2 * NA + g]);
            const double re = m + sd * nrand(), im = sd * nrand();
            y[v * NB + i] = sqrt(re * re + im * im); /* a magnitude: Rice(m, sd) */
        }
    }
    pnx_curvefit_opts o;
    memset(&o, 0, sizeof(o));
    o.model = PNX_MODEL_BI_REDUCED;
    o.n_b = NB;
    o.n_free = pnx_model_n_params(PNX_MODEL_BI_REDUCED);
    for (int k = 0; k < o.n_free; ++k) o.free_idx[k] = k;
    o.jac_mode = PNX_JAC_ANALYTIC;
    const double lo[3] = {0.0, 1e-3, 1e-5}, hi[3] = {1.0, 0.5, 5e-3};
    double *mean_g = malloc(sizeof(double) * 3 * NV), *mean_r = malloc(sizeof(double) * 3 * NV), *ev = malloc(sizeof(double) * NV);
    if (pnx_curvefit_grid_posterior_f64(&o, NV, b, y, NA, atoms, NULL, lo, hi, 0, NULL, sd, mean_g, NULL, NULL, NULL, NULL, NULL, PNX_MEM_HOST, 0, NULL))
        return fail("pnx_curvefit_grid_posterior_f64");
    if (pnx_curvefit_grid_posterior_rician_f64(&o, NV, b, y, NA, atoms, NULL, lo, hi, NULL, sd, mean_r, NULL, NULL, NULL, ev, NULL, PNX_MEM_HOST, 0, NULL))
        return fail("pnx_curvefit_grid_posterior_rician_f64");
    double bias_g = 0, bias_r = 0;
    for (int v = 0; v < NV; ++v) {
        bias_g += (mean_g[2 * NV + v] - truth[v]) / NV;
        bias_r += (mean_r[2 * NV + v] - truth[v]) / NV;
    }
    printf("mean signed error of D2: Gaussian likelihood %.3e, Rician likelihood %.3e\n", bias_g, bias_r);
    /* a marginalised noise scale and per-b-value weights are refused by name, before any device work */
    if (pnx_curvefit_grid_posterior_rician_f64(&o, NV, b, y, NA, atoms, NULL, lo, hi, NULL, 0.0, mean_r, NULL, NULL, NULL, NULL, NULL, PNX_MEM_HOST, 0, NULL) !=
        PNX_ERR_INVALID)
        return 3;
    if (!(fabs(bias_r) < fabs(bias_g))) return 4;
    printf("Rician posterior demo ok\n");
    free(atoms); free(y); free(truth); free(mean_g); free(mean_r); free(ev);
    return 0;
}
