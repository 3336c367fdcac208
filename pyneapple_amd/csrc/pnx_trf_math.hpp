// pnx_trf_math.hpp -- the per-voxel algebra of the Trust-Region-Reflective iteration, once for both curve-fit kernels: the small
// dense helpers, the Householder merge, the one-sided Jacobi SVD and SciPy's strictly-feasible / step-to-bound / trust-region
// step functions (scipy/optimize/_lsq/common.py, trf.py), as templates on the scalar type T.  T = double is the fp64 kernel
// (pnx_curvefit_kernel.hpp) and the covariance epilogue of both, T = float the fp32 kernel (pnx_curvefit_f32_kernel.hpp).
// What differs between the two precisions is in TrfTraits<T> and in one line of solve_lsq_trust_region; everything else is the
// same text.  Constants that are not exactly representable are given per type (a double literal cast to float can round
// differently from the float literal), and no unadorned double literal takes part in T arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace pnx {

template <typename T> struct TrfTraits;

template <> struct TrfTraits<double> {
    static constexpr double eps = 2.220446049250313e-16;
    // jacobi_svd: a pair is skipped when g^2 <= skip * a b (|cos| <= 1e-15).  A sweep whose largest |cos(angle)| was below 1e-8
    // is the last one: Jacobi converges quadratically, so the rotations of that sweep already leave the off-diagonal at the
    // 1e-16 level.
    static constexpr double jacobi_skip = 1.0e-30, jacobi_rotated = 1.0e-16;
    static constexpr double rstep = 1e-10;  // least_squares.py:827-828
    // solve_lsq_trust_region (common.py:148-165): floor of the safeguarded alpha, relative tolerance of the root find
    static constexpr double alpha_floor = 0.001, phi_rtol = 0.01;
    // Reciprocal / reciprocal square root to ~1 ulp from the hardware seeds (v_rcp_f64 / v_rsq_f64) and two
    // Newton steps: 5-6 VALU ops instead of the 11 (fdiv) / 18 (sqrt) of the IEEE-exact expansions.  Used only
    // inside orthogonal transformations (Householder, Givens/Jacobi), where a last-bit error perturbs
    // orthogonality at the 1e-16 level and nothing else.  Arguments are finite and > 0.
    __device__ static inline double rcp(double x) {
        double r = __builtin_amdgcn_rcp(x);
        r = fma(fma(-x, r, 1.0), r, r);
        r = fma(fma(-x, r, 1.0), r, r);
        return r;
    }
    // returns sqrt(x), *rs = 1/sqrt(x)
    __device__ static inline double sqrt_rsqrt(double x, double *rs) {
        double y = __builtin_amdgcn_rsq(x);
        double g = x * y, h = 0.5 * y;
        double r = fma(-h, g, 0.5);
        g = fma(g, r, g);
        h = fma(h, r, h);
        r = fma(-h, g, 0.5);
        g = fma(g, r, g);
        h = fma(h, r, h);
        *rs = h + h;
        return g;
    }
};

template <> struct TrfTraits<float> {
    static constexpr float eps = 1.1920929e-07f;  // FLT_EPSILON
    // jacobi_svd: a pair is skipped when g^2 <= skip * a b (|cos| <= 3e-7).  A sweep whose largest |cos(angle)| was below 3e-4
    // (the square root of the fp32 resolution) is the last one: Jacobi converges quadratically, so the rotations of that sweep
    // already leave the off-diagonal at the 1e-7 level.
    static constexpr float jacobi_skip = 1.0e-13f, jacobi_rotated = 1.0e-7f;
    // least_squares.py:827-828 with rstep = 8 FLT_EPSILON: SciPy's 1e-10 is below fp32 resolution (lb + 1e-10 |lb| == lb), and a
    // start value that stays ON a bound has a zero Coleman-Li scale
    static constexpr float rstep = 8.0f * eps;
    static constexpr float alpha_floor = 0.001f, phi_rtol = 0.01f;
    // Reciprocal / square root with reciprocal square root from the hardware seeds (v_rcp_f32 / v_rsq_f32, 1 ulp) and one Newton
    // step.  Used only inside orthogonal transformations, as in fp64.  Arguments are finite and > 0.
    __device__ static inline float rcp(float x) {
        float r = __builtin_amdgcn_rcpf(x);
        return fmaf(fmaf(-x, r, 1.0f), r, r);
    }
    // returns sqrt(x), *rs = 1/sqrt(x)
    __device__ static inline float sqrt_rsqrt(float x, float *rs) {
        const float y = __builtin_amdgcn_rsqf(x);
        float g = x * y, h = 0.5f * y;
        const float r = fmaf(-h, g, 0.5f);
        g = fmaf(g, r, g);
        h = fmaf(h, r, h);
        *rs = h + h;
        return g;
    }
};

template <typename T> __device__ inline T fast_rcp(T x) { return TrfTraits<T>::rcp(x); }
template <typename T> __device__ inline T fast_sqrt_rsqrt(T x, T *rs) { return TrfTraits<T>::sqrt_rsqrt(x, rs); }

// ---------------------------------------------------------------------------------------------
// Small dense helpers, everything statically indexed (register resident).
// ---------------------------------------------------------------------------------------------
template <int N, typename T> __device__ inline T dotn(const T *a, const T *b) {
    T s = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) s += a[i] * b[i];
    return s;
}
template <int N, typename T> __device__ inline T normn(const T *a) { return sqrt(dotn<N>(a, a)); }

// Merge RB rows (J part in blk[r][0..N), rhs in blk[r][N]) into the upper-triangular factor R | q
// by Householder reflections acting on [R[k][k]; blk[:,k]].  Afterwards blk is garbage.
template <int N, int RB, typename T> __device__ inline void qr_merge(T (&R)[N][N], T (&q)[N], T (&blk)[RB][N + 1]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        T sig = 0;
#pragma unroll
        for (int r = 0; r < RB; ++r) sig += blk[r][k] * blk[r][k];
        if (sig > 0) {
            const T alpha = R[k][k];
            T rs;
            const T nrm = fast_sqrt_rsqrt(alpha * alpha + sig, &rs);
            const T beta = alpha <= 0 ? nrm : -nrm;
            const T v0 = alpha - beta;            // |v0| >= nrm > 0
            const T inv_v0 = copysign(fast_rcp(fabs(v0)), v0);
            const T tau = -v0 * (alpha <= 0 ? rs : -rs);  // -v0 / beta
#pragma unroll
            for (int r = 0; r < RB; ++r) blk[r][k] *= inv_v0;
            R[k][k] = beta;
#pragma unroll
            for (int j = k + 1; j <= N; ++j) {
                T w = (j < N) ? R[k][j] : q[k];
#pragma unroll
                for (int r = 0; r < RB; ++r) w += blk[r][k] * blk[r][j];
                w *= tau;
                if (j < N)
                    R[k][j] -= w;
                else
                    q[k] -= w;
#pragma unroll
                for (int r = 0; r < RB; ++r) blk[r][j] -= w * blk[r][k];
            }
        }
    }
}

// One-sided Jacobi SVD of the N x N matrix W (in place: W <- U*diag(s)), V accumulates the right
// singular vectors (columns).  Callers pass the TRANSPOSE of a triangular factor (lower triangular W):
// row-cyclic Jacobi converges in ~1 sweep less on R^T than on R (Drmac-Veselic), see DESIGN.md.
// The two thresholds (which pair is rotated, which sweep is the last) are TrfTraits<T>::jacobi_*.
template <int N, typename T> __device__ inline void jacobi_svd(T (&W)[N][N], T (&V)[N][N]) {
    using Tr = TrfTraits<T>;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i][j] = (i == j) ? T(1) : T(0);
    if (N == 1) return;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;  // some pair of this sweep had g^2 / (a b) >= jacobi_rotated (tested as a product: no division)
#pragma unroll
        for (int p = 0; p < N - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                T a = 0, b = 0, g = 0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    a += W[i][p] * W[i][p];
                    b += W[i][q] * W[i][q];
                    g += W[i][p] * W[i][q];
                }
                const T g2 = g * g, ab = a * b;
                if (g2 > Tr::jacobi_skip * ab) {
                    rotated = rotated || (g2 >= Tr::jacobi_rotated * ab);
                    // t = tan(theta) = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)),  zeta = (b - a) / (2 g)
                    const T num = b - a, den = T(2) * g;
                    T rs;
                    const T hyp = fast_sqrt_rsqrt(num * num + den * den, &rs);
                    T t = fabs(den) * fast_rcp(fabs(num) + hyp);
                    t = ((num < 0) != (den < 0)) ? -t : t;
                    T c;
                    (void)fast_sqrt_rsqrt(T(1) + t * t, &c);
                    const T s = c * t;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        const T wp = W[i][p], wq = W[i][q];
                        W[i][p] = c * wp - s * wq;
                        W[i][q] = s * wp + c * wq;
                        const T vp = V[i][p], vq = V[i][q];
                        V[i][p] = c * vp - s * vq;
                        V[i][q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
}

// scipy/optimize/_lsq/common.py:400-464 with rstep = 0 (np.nextafter form)
template <typename T> __device__ inline T strictly_feasible0(T x, T lb, T ub) {
    if (x <= lb) x = nextafter(lb, ub);
    if (x >= ub) x = nextafter(ub, lb);  // numpy applies the lower mask first, then the upper one
    if (x < lb || x > ub) x = T(0.5) * (lb + ub);
    return x;
}
// same with rstep = TrfTraits<T>::rstep (least_squares.py:827-828)
template <typename T> __device__ inline T strictly_feasible_r(T x, T lb, T ub) {
    const T rstep = TrfTraits<T>::rstep;
    const T lower_dist = x - lb, upper_dist = ub - x;
    const T lt = rstep * fmax(T(1), fabs(lb)), ut = rstep * fmax(T(1), fabs(ub));
    int active = 0;
    if (isfinite(lb) && lower_dist <= fmin(upper_dist, lt)) active = -1;
    if (isfinite(ub) && upper_dist <= fmin(lower_dist, ut)) active = 1;
    if (active == -1) x = lb + lt;
    if (active == 1) x = ub - ut;
    if (x < lb || x > ub) x = T(0.5) * (lb + ub);
    return x;
}

// scipy/optimize/_lsq/common.py:367-397
template <int N, typename T>
__device__ inline T step_size_to_bound(const T *x, const T *s, const T *lb, const T *ub, int *hits) {
    T steps[N];
    T mn = T(INFINITY);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        // max((lb - x) / s, (ub - x) / s) is the quotient with the larger numerator for s > 0 and with the smaller one for
        // s < 0 (lb <= ub): one IEEE division instead of two, the same value bit for bit
        const T num = (s[i] > 0) ? (ub[i] - x[i]) : (lb[i] - x[i]);
        steps[i] = (s[i] != 0) ? num / s[i] : T(INFINITY);
        mn = fmin(mn, steps[i]);
    }
    if (hits) {
#pragma unroll
        for (int i = 0; i < N; ++i) hits[i] = (steps[i] == mn) ? ((s[i] > 0) - (s[i] < 0)) : 0;
    }
    return mn;
}

// 0.5*||R2 s||^2 + g_h.s  ==  evaluate_quadratic(J_h, g_h, s, diag=diag_h) (common.py:325-362), because
// R2^T R2 = J_h^T J_h + diag(diag_h).
template <int N, typename T> __device__ inline void rmul(const T (&R)[N][N], const T *s, T *out) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T a = 0;
#pragma unroll
        for (int j = i; j < N; ++j) a += R[i][j] * s[j];
        out[i] = a;
    }
}

// common.py:303-322
template <typename T> __device__ inline T minimize_quadratic_1d(T a, T b, T lb, T ub, T c, T &y) {
    T tb = lb, yb = lb * (a * lb + b) + c;
    const T yu = ub * (a * ub + b) + c;
    if (yu < yb) {
        yb = yu;
        tb = ub;
    }
    if (a != 0) {
        const T ext = T(-0.5) * b / a;
        if (lb < ext && ext < ub) {
            const T ye = ext * (a * ext + b) + c;
            if (ye < yb) {
                yb = ye;
                tb = ext;
            }
        }
    }
    y = yb;
    return tb;
}

// common.py:57-168
template <int N, typename T>
__device__ inline T solve_lsq_trust_region(int m, const T *uf, const T *s, const T (&V)[N][N], T smax, T smin, T Delta,
                                           T initial_alpha, T *p) {
    using Tr = TrfTraits<T>;
    T suf[N], t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) suf[i] = s[i] * uf[i];
    const bool full_rank = (m >= N) && (smin > Tr::eps * m * smax);
    if (full_rank) {
#pragma unroll
        for (int i = 0; i < N; ++i) t[i] = uf[i] / s[i];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            T a = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) a += V[i][k] * t[k];
            p[i] = -a;
        }
        if (normn<N>(p) <= Delta) return T(0);
    }
    T alpha_upper = normn<N>(suf) / Delta;
    T alpha_lower = 0;
    auto phi_and_derivative = [&] __device__(T alpha, T &phi, T &phi_prime) {
        T pn2 = 0, sp = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const T denom = s[i] * s[i] + alpha;
            const T q = suf[i] / denom;
            pn2 += q * q;
            if constexpr (std::is_same_v<T, double>)
                sp += suf[i] * suf[i] / (denom * denom * denom);
            else
                sp += q * q / denom;  // suf^2 / denom^3 without the cube: denom^3 leaves the fp32 range for signals of amplitude 1e3
        }
        const T p_norm = sqrt(pn2);
        phi = p_norm - Delta;
        phi_prime = -sp / p_norm;
    };
    T phi, phi_prime;
    if (full_rank) {
        phi_and_derivative(T(0), phi, phi_prime);
        alpha_lower = -phi / phi_prime;
    }
    T alpha;
    if (!full_rank && initial_alpha == 0)
        alpha = fmax(Tr::alpha_floor * alpha_upper, sqrt(alpha_lower * alpha_upper));
    else
        alpha = initial_alpha;
    for (int it = 0; it < 10; ++it) {
        if (alpha < alpha_lower || alpha > alpha_upper)
            alpha = fmax(Tr::alpha_floor * alpha_upper, sqrt(alpha_lower * alpha_upper));
        phi_and_derivative(alpha, phi, phi_prime);
        if (phi < 0) alpha_upper = alpha;
        const T ratio = phi / phi_prime;
        alpha_lower = fmax(alpha_lower, alpha - ratio);
        alpha -= (phi + Delta) * ratio / Delta;
        if (fabs(phi) < Tr::phi_rtol * Delta) break;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = suf[i] / (s[i] * s[i] + alpha);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T a = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) a += V[i][k] * t[k];
        p[i] = -a;
    }
    const T sc = Delta / normn<N>(p);
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] *= sc;
    return alpha;
}

// trf.py:128-202.  Returns predicted reduction; writes step / step_h.
template <int N, typename T>
__device__ inline T select_step(const T *x, const T (&R2)[N][N], const T *g_h, T *p, T *p_h, const T *d, T Delta, const T *lb,
                                const T *ub, T theta, T *step, T *step_h) {
    bool inb = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const T xp = x[i] + p[i];
        inb = inb && (xp >= lb[i]) && (xp <= ub[i]);
    }
    T t1[N], t2[N];
    if (inb) {
        rmul<N>(R2, p_h, t1);
        const T p_value = T(0.5) * dotn<N>(t1, t1) + dotn<N>(p_h, g_h);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            step[i] = p[i];
            step_h[i] = p_h[i];
        }
        return -p_value;
    }
    int hits[N];
    const T p_stride = step_size_to_bound<N>(x, p, lb, ub, hits);
    T r_h[N], r[N], xb[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        r_h[i] = hits[i] ? -p_h[i] : p_h[i];
        r[i] = d[i] * r_h[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        p[i] *= p_stride;
        p_h[i] *= p_stride;
        xb[i] = x[i] + p[i];
    }
    // intersect_trust_region(p_h, r_h, Delta) (common.py:18-54), positive root
    T to_tr;
    {
        const T a = dotn<N>(r_h, r_h), b = dotn<N>(p_h, r_h), c = dotn<N>(p_h, p_h) - Delta * Delta;
        const T dd = sqrt(b * b - a * c);
        const T q = -(b + copysign(dd, b));
        const T ta = q / a, tb = c / q;
        to_tr = fmax(ta, tb);
    }
    T to_bound = step_size_to_bound<N>(xb, r, lb, ub, nullptr);
    T r_stride = fmin(to_bound, to_tr);
    T r_stride_l, r_stride_u;
    if (r_stride > 0) {
        r_stride_l = (1 - theta) * p_stride / r_stride;
        r_stride_u = (r_stride == to_bound) ? theta * to_bound : to_tr;
    } else {
        r_stride_l = 0;
        r_stride_u = -1;
    }
    T r_value;
    if (r_stride_l <= r_stride_u) {
        // build_quadratic_1d(J_h, g_h, r_h, s0=p_h, diag=diag_h) (common.py:250-300)
        rmul<N>(R2, r_h, t1);   // v
        rmul<N>(R2, p_h, t2);   // u
        const T a = T(0.5) * dotn<N>(t1, t1);
        const T b = dotn<N>(g_h, r_h) + dotn<N>(t2, t1);
        const T c = T(0.5) * dotn<N>(t2, t2) + dotn<N>(g_h, p_h);
        r_stride = minimize_quadratic_1d(a, b, r_stride_l, r_stride_u, c, r_value);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            r_h[i] = r_h[i] * r_stride + p_h[i];
            r[i] = r_h[i] * d[i];
        }
    } else
        r_value = T(INFINITY);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        p[i] *= theta;
        p_h[i] *= theta;
    }
    rmul<N>(R2, p_h, t1);
    const T p_value = T(0.5) * dotn<N>(t1, t1) + dotn<N>(p_h, g_h);

    T ag_h[N], ag[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ag_h[i] = -g_h[i];
        ag[i] = d[i] * ag_h[i];
    }
    to_tr = Delta / normn<N>(ag_h);
    to_bound = step_size_to_bound<N>(x, ag, lb, ub, nullptr);
    T ag_stride = (to_bound < to_tr) ? theta * to_bound : to_tr;
    T ag_value;
    {
        rmul<N>(R2, ag_h, t1);
        const T a = T(0.5) * dotn<N>(t1, t1);
        const T b = dotn<N>(g_h, ag_h);
        ag_stride = minimize_quadratic_1d(a, b, T(0), ag_stride, T(0), ag_value);
    }
    if (p_value < r_value && p_value < ag_value) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            step[i] = p[i];
            step_h[i] = p_h[i];
        }
        return -p_value;
    } else if (r_value < p_value && r_value < ag_value) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            step[i] = r[i];
            step_h[i] = r_h[i];
        }
        return -r_value;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            step[i] = ag[i] * ag_stride;
            step_h[i] = ag_h[i] * ag_stride;
        }
        return -ag_value;
    }
}

}  // namespace pnx
