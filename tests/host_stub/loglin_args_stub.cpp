// loglin_args_stub.cpp -- the host-side argument checks of pnx_loglinear_f64 / _f32 (pyneapple_amd/csrc/pnx_loglin_args.hpp, free
// of HIP types) as a stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_loglinear_host.py.  Every array
// is heap-allocated at exactly the size the ABI documents, so a read past n_b b-values or mask bytes, or past the two bounds, is
// an AddressSanitizer report; a refusal that comes before an array may be read gets that array as NULL.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pnx_loglin_args.hpp"

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

template <typename T> struct Call {
    int n_b = 8, weighting = 1, n_reweight = 0, clip = 0, mem = PNX_MEM_HOST;
    int64_t n_vox = 1;
    std::vector<T> b, lo, hi;
    std::vector<uint8_t> use;
    bool with_b = true, with_use = false, with_bounds = false, with_y = true, with_params = true;
    explicit Call(int n) : n_b(n) {
        for (int i = 0; i < n; ++i) b.push_back((T)(50 * i));
        use.assign(n > 0 ? n : 0, 1);
        lo = {(T)1, (T)1e-5};
        hi = {(T)5000, (T)0.1};
    }
    int run(LogLinOpts *o) {
        static T y[1], p[2];
        return loglin_check_args<T>(n_vox, n_b, with_b ? b.data() : nullptr, with_use ? use.data() : nullptr, weighting, n_reweight, clip,
                                    with_bounds ? lo.data() : nullptr, with_bounds ? hi.data() : nullptr, with_y ? y : nullptr,
                                    with_params ? p : nullptr, mem, o);
    }
};

template <typename T> static void walk() {
    LogLinOpts o;
    for (int n_b : {2, 3, 63, 64, 65, 127, 128}) {  // a valid set at every size around the mask words: exact-size arrays
        Call<T> c(n_b);
        EXPECT(c.run(&o) == PNX_OK && o.n_b == n_b && o.weighting == 1 && o.n_reweight == 0 && o.clip == 0);
        int bits = 0;
        for (int i = 0; i < PNX_MAX_BVALUES; ++i) bits += (int)((o.use[i >> 6] >> (i & 63)) & 1);
        EXPECT(bits == n_b && o.b[n_b - 1] == (double)c.b[n_b - 1]);
        c.with_use = true;
        c.use[0] = 0;
        if (n_b > 2) {
            EXPECT(c.run(&o) == PNX_OK && !(o.use[0] & 1) && ((o.use[(n_b - 1) >> 6] >> ((n_b - 1) & 63)) & 1));
        } else {
            EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "use"));
        }
    }
    for (int n_b : {-1, 0, 1, 129}) {  // refused before b is read: b is NULL here
        Call<T> c(0);
        c.n_b = n_b;
        c.with_b = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "n_b"));
    }
    {
        Call<T> c(8);
        c.with_b = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "b is NULL"));
    }
    {
        Call<T> c(8);
        c.with_y = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "y is NULL"));
        c.n_vox = 0;  // nothing to read: no array needed
        c.with_params = false;
        EXPECT(c.run(&o) == PNX_OK);
        c.n_vox = -1;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "n_vox"));
    }
    {
        Call<T> c(8);
        c.with_params = false;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "params is NULL"));
    }
    for (T bad : {(T)NAN, (T)INFINITY, (T)-INFINITY}) {
        Call<T> c(8);
        c.b[7] = bad;  // the last one
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "b[7]"));
    }
    for (int w : {-1, 2}) {
        Call<T> c(8);
        c.weighting = w;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "weighting"));
    }
    for (int r : {-1, 9}) {
        Call<T> c(8);
        c.n_reweight = r;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "n_reweight"));
    }
    {
        Call<T> c(8);
        c.n_reweight = 8;
        c.weighting = 0;
        EXPECT(c.run(&o) == PNX_OK && o.n_reweight == 8 && o.weighting == 0);
    }
    {   // masks: one b-value left, none left, two left with the same b, two distinct left
        Call<T> c(8);
        c.with_use = true;
        c.use.assign(8, 0);
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "use"));
        c.use[7] = 1;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "use"));
        c.use[3] = 1;
        c.b[3] = c.b[7];
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "distinct"));
        c.b[3] = (T)10;
        EXPECT(c.run(&o) == PNX_OK && o.use[0] == ((1ull << 3) | (1ull << 7)) && o.use[1] == 0);
    }
    {   // without a mask all b-values equal leave no line either
        Call<T> c(4);
        c.b.assign(4, (T)100);
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "distinct"));
    }
    {   // clip: the bounds are read only with clip
        Call<T> c(8);
        c.clip = 1;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "lo"));
        c.with_bounds = true;
        EXPECT(c.run(&o) == PNX_OK && o.clip == 1 && o.lo[1] == (double)c.lo[1] && o.hi[0] == 5000.0);
        c.hi[1] = c.lo[1];
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "lo[1]"));
        c.hi[1] = (T)NAN;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "lo[1]"));
        c.clip = 0;  // not looked at
        EXPECT(c.run(&o) == PNX_OK);
    }
    for (int mem : {-1, 2}) {
        Call<T> c(8);
        c.mem = mem;
        EXPECT(c.run(&o) == PNX_ERR_INVALID && strstr(g_err, "mem"));
    }
}

int main() {
    walk<double>();
    walk<float>();
    for (int n_b = 2; n_b <= PNX_MAX_BVALUES; ++n_b)  // both tiles inside a workgroup's 160 KB, rows of an odd number of doubles
        EXPECT(loglin_lds_bytes(n_b) == (size_t)2 * 64 * 8 * (n_b | 1) && loglin_lds_bytes(n_b) <= 160 * 1024);
    if (failures) return 1;
    printf("loglin args stub ok\n");
    return 0;
}
