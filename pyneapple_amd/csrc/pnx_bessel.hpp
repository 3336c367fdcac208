// pnx_bessel.hpp -- log of the exponentially scaled modified Bessel function of order zero, h(z) = log I0e(z) = log(e^-z I0(z)),
// for the Rician likelihood of magnitude data (pnx_grid_rician.hip).  Plain C++: a host program compiles it with
// g++ (tests/host_stub/bessel_stub.cpp), HIP compiles the same text for the device.
//
// h(0) = 0, h <= 0, h(z) ~ -1/2 log(2 pi z) for large z.  Four pieces, each a polynomial by Horner's rule in one chain of fma in a
// variable t in [-1, 1] (coefficients: Chebyshev interpolants of the exact function at 60 digits, converted to the power basis in
// t and rounded to double; the power basis in t is well conditioned because every piece is analytic well beyond its interval):
//
//   0 <= z < 2    h = w A(t) - z,  w = z^2, t = w / 2 - 1, A(w) = log I0(sqrt w) / w: log I0 is even, its series in w has the
//                 radius 5.78 (the first zero of J0, squared), so degree 17 reaches 0.07 * 2^-52 on w in [0, 4].  A denormal z gives
//                 w = 0 and h = -z, which is h to 2^-52 relative.
//   2 <= z < 4    h = B1(t), t = z - 3 (exact);  4 <= z < 8: h = B2(t), t = z / 2 - 3.  Degree 19 each.
//   8 <= z        h = C(t) - (log z + log 2 pi) / 2, t = 16 / z - 1, C = log(sqrt(2 pi z) I0e(z)) = 1 / (8 z) + ... as a function of
//                 8 / z in (0, 1]: smooth down to 0 although its series in 1 / z only is asymptotic; degree 23.  log z is the one
//                 library call; nothing can overflow: z = 1e300 gives t = -1 and log z = 690.8, z = inf gives -inf.
//
// Error, in units of 2^-52 max(|h|, 1): approximation 0.06 / 0.27 / 0.13 / 0.12 per piece, Horner (the running bound
// 2^-53 sum_k |p_k| |t|^k over the partial sums p_k) 0.39 / 0.63 / 0.59 / 0.01; with the roundings of w, t, log z (1 ulp), the sum
// and the last fma: 1.5 / 0.9 / 1.0 / 2.1.  E_h = 4.5 is that bound with a margin of 2 (tests/test_grid_rician_host.py asserts SciPy
// inside it; DESIGN.md 4.1t holds the derivation and the observed maximum).
//
// A negative or NaN argument returns NaN.  Every multiply-add is an explicit fma, so a compiler's contraction setting changes
// nothing: the three polynomial pieces give the same bytes on the host and on the device, the last piece differs by what the two
// `log` differ by.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PNX_BESSEL_HD __host__ __device__
#else
#define PNX_BESSEL_HD
#endif

namespace pnx {

constexpr double kLogI0eBound = 4.5;  // E_h: |log_i0e(z) - h(z)| <= E_h 2^-52 max(|h(z)|, 1) for every z in [0, 1e300]

template <int N> PNX_BESSEL_HD inline double bessel_horner(const double (&c)[N], double t) {
    double p = c[0];
#pragma unroll
    for (int k = 1; k < N; ++k) p = fma(p, t, c[k]);
    return p;
}

PNX_BESSEL_HD inline double log_i0e_small(double z) {  // 0 <= z < 2
    constexpr double c[18] = {                         // highest power first
        -0x1.4496c4d1b34eap-40, 0x1.4d8767798a451p-38, -0x1.f90988466d538p-37, 0x1.05dfe229a75ddp-34, -0x1.1b75c383c1d69p-32,
        0x1.288417ef0def2p-30,  -0x1.3744f639323d7p-28, 0x1.49ae37dead088p-26, -0x1.5ffca8d41d387p-24, 0x1.7b64557f88701p-22,
        -0x1.9dc900ae24734p-20, 0x1.ca146d0d824b3p-18, -0x1.028d5d934f2a5p-15, 0x1.2bc937568a705p-13, -0x1.69a992baeddd4p-11,
        0x1.d2a6c2a508dd9p-9,   -0x1.5ca0ab69b6c8cp-6, 0x1.cb57e9f857e1ap-3};
    const double w = z * z;
    return fma(w, bessel_horner(c, fma(w, 0.5, -1.0)), -z);
}

PNX_BESSEL_HD inline double log_i0e_mid1(double z) {  // 2 <= z < 4
    constexpr double c[20] = {                        // highest power first
        0x1.975f68d3c4dcbp-41,  -0x1.e97a48af94039p-39, 0x1.c8ca38652475dp-38, 0x1.7eb53ad311b61p-37, -0x1.772fa14a77732p-33,
        0x1.fc8cbb9bcc350p-31,  -0x1.a64ac2eb3a757p-29, 0x1.119deebc73902p-28, 0x1.da11c1ff8df2bp-26, -0x1.0e1474e154ab1p-22,
        0x1.3a7a20b663aa3p-20,  -0x1.b72dff5361320p-19, 0x1.46388dba3156dp-21, 0x1.e2a591ca5a91ap-15, -0x1.c286261cd7274p-12,
        0x1.1abe80a5b07d6p-9,   -0x1.29225d4cb4896p-7, 0x1.2ecfe32a36df3p-5, -0x1.85266e21ba184p-3, -0x1.6a29479a3639ep+0};
    return bessel_horner(c, z - 3.0);
}

PNX_BESSEL_HD inline double log_i0e_mid2(double z) {  // 4 <= z < 8
    constexpr double c[20] = {                        // highest power first
        0x1.32d0892ba535cp-37,  -0x1.1d8944b04c4a2p-34, 0x1.256e2f6cfd55bp-32, -0x1.e6c89d3e46f3dp-31, 0x1.6100bdca4cf80p-29,
        -0x1.978c53167ae5ap-28, 0x1.ebe5e72226206p-28, 0x1.a2ab26ec8e554p-26, -0x1.fba14b5b34e94p-23, 0x1.4444fece179b8p-20,
        -0x1.4b91b4787c346p-18, 0x1.2b1370dad9c4ep-16, -0x1.f3a028a7dff2ap-15, 0x1.91ac98064d4e5p-13, -0x1.4303704d5b82dp-11,
        0x1.0e3747c9cbaf7p-9,   -0x1.e9b03c83d07dcp-8, 0x1.fd3c22197d1bap-6, -0x1.66f9ee19a58dep-3, -0x1.cab4613048f65p+0};
    return bessel_horner(c, fma(z, 0.5, -3.0));
}

PNX_BESSEL_HD inline double log_i0e_large(double z) {  // 8 <= z
    constexpr double c[24] = {                         // highest power first
        -0x1.1375ef6adb684p-34, 0x1.f124a526d2cdcp-33, 0x1.f2d1b34ee518cp-32, -0x1.ba9ce75c6b459p-30, -0x1.bd00d36109ca9p-30,
        0x1.705a8bb55bc58p-28,  0x1.196dbaeeffa5ap-28, -0x1.81043bb507879p-27, -0x1.37343e5728fbep-27, 0x1.1414c1c2afc4bp-26,
        0x1.469c4f373c95cp-26,  -0x1.a30c59730c000p-27, -0x1.1da080f66d0dbp-25, -0x1.27e081bd5c829p-26, 0x1.3aa439c75da64p-26,
        0x1.c4f1d1a991782p-25,  0x1.9ade41b4ebda4p-24, 0x1.c9d200159e4a8p-23, 0x1.78cfcdc8d681fp-21, 0x1.cb70cac87be7fp-19,
        0x1.a49fde13a05c9p-16,  0x1.3e8b182536409p-12, 0x1.11ce7ada3f9bap-7, 0x1.0894584107934p-7};
    const double q = bessel_horner(c, fma(8.0 / z, 2.0, -1.0));
    const double s = log(z) + 0x1.d67f1c864beb5p+0;  // log(2 pi)
    return fma(-0.5, s, q);
}

// h(z) = log(exp(-z) I0(z)) for z >= 0; NaN for z < 0 or NaN
PNX_BESSEL_HD inline double log_i0e(double z) {
    if (!(z >= 0.0)) return __builtin_nan("");
    if (z < 2.0) return log_i0e_small(z);
    if (z < 4.0) return log_i0e_mid1(z);
    if (z < 8.0) return log_i0e_mid2(z);
    return log_i0e_large(z);
}
}  // namespace pnx
