// pnx_model_t.hpp -- the seven forward models and their analytic Jacobian rows for a scalar type T (float or double):
// signal and Jacobian row of one measurement from the parameter vector, formulas and operation order of Model<MODEL>
// (pnx_curvefit_kernel.hpp; model_functions/multiexp.py:35-202, models/{monoexp,biexp,triexp}.py jacobian()).
// Used by the residual sweep (pnx_sweep.hip, T = float and double) and by the fp32-arithmetic curve fit
// (pnx_curvefit_f32_kernel.hpp, T = float).
#pragma once
#include <hip/hip_runtime.h>

#include "pnx_curvefit_kernel.hpp"

namespace pnx {

template <typename T> __device__ inline T fast_exp(T x);
template <> __device__ inline float fast_exp<float>(float x) { return __expf(x); }  // v_exp_f32 (native 2^x)
template <> __device__ inline double fast_exp<double>(double x) { return exp(x); }

// Model<MODEL> works on doubles; a thin generic restatement of signal/jac for T (same formulas)
template <int MODEL, typename T> struct ModelT {
    using M = Model<MODEL>;
    static constexpr int NALL = M::NALL, NC = M::NC;
    __device__ static void eval(const T *p, T bb, T &sig, T *ja) {
        T E[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) E[c] = fast_exp<T>(-bb * p[M::dpos(c)]);
        if constexpr (MODEL == 0) {
            sig = p[0] * E[0];
            ja[0] = E[0];
            ja[1] = -bb * p[0] * E[0];
        } else if constexpr (MODEL == 1) {
            sig = p[0] * E[0] + (1 - p[0]) * E[1];
            ja[0] = E[0] - E[1];
            ja[1] = -bb * p[0] * E[0];
            ja[2] = -bb * (1 - p[0]) * E[1];
        } else if constexpr (MODEL == 2) {
            const T inner = p[0] * E[0] + (1 - p[0]) * E[1];
            sig = p[3] * inner;
            ja[0] = p[3] * (E[0] - E[1]);
            ja[1] = -bb * p[3] * p[0] * E[0];
            ja[2] = -bb * p[3] * (1 - p[0]) * E[1];
            ja[3] = inner;
        } else if constexpr (MODEL == 3) {
            sig = p[0] * E[0] + p[2] * E[1];
            ja[0] = E[0];
            ja[1] = -bb * p[0] * E[0];
            ja[2] = E[1];
            ja[3] = -bb * p[2] * E[1];
        } else if constexpr (MODEL == 4) {
            const T f3 = 1 - p[0] - p[2];
            sig = p[0] * E[0] + p[2] * E[1] + f3 * E[2];
            ja[0] = E[0] - E[2];
            ja[1] = -bb * p[0] * E[0];
            ja[2] = E[1] - E[2];
            ja[3] = -bb * p[2] * E[1];
            ja[4] = -bb * f3 * E[2];
        } else if constexpr (MODEL == 5) {
            const T f3 = 1 - p[0] - p[2];
            const T inner = p[0] * E[0] + p[2] * E[1] + f3 * E[2];
            sig = p[5] * inner;
            ja[0] = p[5] * (E[0] - E[2]);
            ja[1] = -bb * p[5] * p[0] * E[0];
            ja[2] = p[5] * (E[1] - E[2]);
            ja[3] = -bb * p[5] * p[2] * E[1];
            ja[4] = -bb * p[5] * f3 * E[2];
            ja[5] = inner;
        } else {
            sig = p[0] * E[0] + p[2] * E[1] + p[4] * E[2];
            ja[0] = E[0];
            ja[1] = -bb * p[0] * E[0];
            ja[2] = E[1];
            ja[3] = -bb * p[2] * E[1];
            ja[4] = E[2];
            ja[5] = -bb * p[4] * E[2];
        }
    }
};

}  // namespace pnx
