// peel_args_stub.cpp -- the host-side argument checks of pnx_peel_f64 / _f32 (pyneapple_amd/csrc/pnx_peel_args.hpp, free of HIP
// types) as a stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_peel_host.py.  Every array is
// heap-allocated at exactly the size the ABI documents, so a read past n_b b-values, K * n_b mask bytes or n_params bounds is an
// AddressSanitizer report; a refusal that comes before an array may be read gets that array as NULL.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pnx_peel_args.hpp"

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

static const int kExp[7] = {1, 2, 2, 2, 3, 3, 3}, kPar[7] = {2, 3, 4, 4, 5, 6, 6};

// A valid call of `model` on n b-values 0, 50, 100, ...: stage k takes every K-th b-value starting at k.
template <typename T> struct Call {
    int model, n_b, weighting = 1, clip = 0, mem = PNX_MEM_HOST;
    int64_t n_vox = 1;
    std::vector<T> b, lo, hi, fb;
    std::vector<uint8_t> use;
    bool with_b = true, with_use = true, with_bounds = false, with_fb = false, with_y = true, with_params = true;
    Call(int m, int n) : model(m), n_b(n) {
        const int K = m >= 0 && m < 7 ? kExp[m] : 1, np = m >= 0 && m < 7 ? kPar[m] : 0;
        for (int i = 0; i < n; ++i) b.push_back((T)(50 * i));
        use.assign((size_t)K * (n > 0 ? n : 0), 0);
        for (int i = 0; i < n; ++i) use[(size_t)(i % K) * n + i] = 1;
        for (int j = 0; j < np; ++j) {
            lo.push_back((T)(j + 1));
            hi.push_back((T)(10 * (j + 1)));
            fb.push_back((T)(2 * j + 3));
        }
    }
    int run(PeelOpts *o) {
        static T y[1], p[6];
        return peel_check_args<T>(model, n_vox, n_b, with_b ? b.data() : nullptr, with_use ? use.data() : nullptr, weighting, clip,
                                  with_bounds ? lo.data() : nullptr, with_bounds ? hi.data() : nullptr, with_fb ? fb.data() : nullptr,
                                  with_y ? y : nullptr, with_params ? p : nullptr, mem, o);
    }
};

static int bits(const PeelOpts &o, int k) {
    int n = 0;
    for (int i = 0; i < PNX_MAX_BVALUES; ++i) n += (int)((o.use[k][i >> 6] >> (i & 63)) & 1);
    return n;
}

template <typename T> static void walk() {
    PeelOpts o;
    for (int model = 0; model < 7; ++model) {  // the accepted case of every layout at every size around the mask words
        const int K = kExp[model], np = kPar[model];
        EXPECT(peel_n_exp(model) == K && peel_n_params(model) == np);
        for (int n_b : {2 * K, 2 * K + 1, 63, 64, 65, 127, 128}) {
            Call<T> c(model, n_b);
            c.clip = 1;
            c.with_bounds = c.with_fb = true;
            EXPECT(c.run(&o) == PNX_OK && o.model == model && o.n_stage == K && o.n_params == np && o.n_b == n_b && o.weighting == 1);
            EXPECT(o.clip == 1 && o.has_fallback == 1 && o.lo[np - 1] == (double)np && o.hi[0] == 10.0 && o.fallback[np - 1] == 2.0 * np + 1);
            int total = 0;
            for (int k = 0; k < kPeelMaxStages; ++k) {
                total += bits(o, k);
                EXPECT(k < K ? ((o.use[k][0] >> k) & 1) == 1 : bits(o, k) == 0);
            }
            EXPECT(total == n_b && o.b[n_b - 1] == (double)c.b[n_b - 1]);
            for (int j = np; j < kPeelMaxParams; ++j) EXPECT(o.lo[j] == 0.0 && o.hi[j] == 0.0 && o.fallback[j] == 0.0);
            c.clip = 0;  // bounds and fallback are optional
            c.with_bounds = c.with_fb = false;
            c.weighting = 0;
            c.mem = PNX_MEM_DEVICE;
            EXPECT(c.run(&o) == PNX_OK && o.clip == 0 && o.has_fallback == 0 && o.weighting == 0);
        }
        for (int n_b : {-1, 0, 2 * K - 1, 129}) {  // refused before b and use are read: both are NULL here
            Call<T> c(model, 0);
            c.n_b = n_b;
            c.with_b = c.with_use = false;
            EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "n_b"));
        }
    }
    for (int model : {-1, 7, 100}) {  // refused before anything is read
        Call<T> c(model, 0);
        c.n_b = 8;
        c.with_b = c.with_use = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "model"));
    }
    const int M = PNX_MODEL_TRI_S0;
    {
        Call<T> c(M, 8);
        c.with_b = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "b is NULL"));
    }
    {
        Call<T> c(M, 8);
        c.with_use = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "use is NULL"));
    }
    {
        Call<T> c(M, 8);
        c.with_y = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "y is NULL"));
        c.n_vox = 0;  // nothing to read: no array needed
        c.with_params = false;
        EXPECT(c.run(&o) == PNX_OK);
        c.n_vox = -1;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "n_vox"));
    }
    {
        Call<T> c(M, 8);
        c.with_params = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "params is NULL"));
    }
    for (T bad : {(T)NAN, (T)INFINITY, (T)-INFINITY}) {
        Call<T> c(M, 8);
        c.b[7] = bad;  // the last one
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "b[7]"));
    }
    for (int w : {-1, 2}) {
        Call<T> c(M, 8);
        c.weighting = w;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "weighting"));
    }
    for (int k = 0; k < 3; ++k) {  // masks, every row: none left, one left, two left with the same b, two distinct left
        Call<T> c(M, 8);
        uint8_t *row = c.use.data() + (size_t)k * 8;
        memset(row, 0, 8);
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "use row") && strchr(g_err, '0' + k));
        row[7] = 1;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "use row"));
        row[3] = 1;
        c.b[3] = c.b[7];
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "distinct"));
        c.b[3] = (T)10;
        EXPECT(c.run(&o) == PNX_OK && o.use[k][0] == ((1ull << 3) | (1ull << 7)) && o.use[k][1] == 0);
    }
    {   // clip: the bounds are read only with clip, and every one of the n_params
        Call<T> c(M, 8);
        c.clip = 1;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "lo"));
        c.with_bounds = true;
        EXPECT(c.run(&o) == PNX_OK && o.clip == 1);
        c.hi[5] = c.lo[5];
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "lo[5]"));
        c.hi[5] = (T)NAN;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "lo[5]"));
        c.clip = 0;  // not looked at
        EXPECT(c.run(&o) == PNX_OK);
    }
    for (int mem : {-1, 2}) {
        Call<T> c(M, 8);
        c.mem = mem;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "mem"));
    }
}

int main() {
    walk<double>();
    walk<float>();
    for (int n_b = 2; n_b <= PNX_MAX_BVALUES; ++n_b)  // both tiles inside a workgroup's 160 KB, rows of an odd number of doubles
        EXPECT(peel_lds_bytes(n_b) == (size_t)2 * 64 * 8 * (n_b | 1) && peel_lds_bytes(n_b) <= 160 * 1024);
    EXPECT(sizeof(PeelOpts) <= 2048);  // travels by value in the kernel arguments (4 KB with the pointers)
    if (failures) return 1;
    printf("peel args stub ok\n");
    return 0;
}
