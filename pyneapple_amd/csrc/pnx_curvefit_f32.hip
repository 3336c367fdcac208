// pnx_curvefit_f32.hip -- instantiations and launch of the fp32-arithmetic TRF kernel (pnx_curvefit_f32_kernel.hpp): the
// seven models, all parameters free, shared or per-voxel start values and bounds.
#include <cstdio>

#include "pnx_curvefit_f32_kernel.hpp"
#include "pnx_launch.hpp"

namespace pnx {
namespace f32 {

template <int N> static int launch_pcov(const CurvefitF32Args &args, const ColPerm &cp, hipStream_t stream) {
    const int pb = 256;
    hipLaunchKernelGGL(pcov_f32_kernel<N>, dim3((unsigned)((args.n_vox + pb - 1) / pb)), dim3(pb), 0, stream, args.pcov,
                       (const int8_t *)args.status, (const float *)args.cost, args.n_vox, args.n_b, cp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PNX_ERR_HIP, "pcov (fp32 fit) launch: %s", hipGetErrorString(e));
    return PNX_OK;
}

template <int MODEL, bool PV> static int launch_one(const CurvefitF32Args &args, int device_cus, hipStream_t stream) {
    constexpr int N = Model<MODEL>::NALL;
    ColPerm cp;
    for (int k = 0; k < kMaxP; ++k) cp.p[k] = k < N ? colperm<MODEL>(k) : k;
    auto kern = curvefit_f32_kernel<MODEL, PV>;
    // LDS per block: b-value table + per wave the signal tile, the parked R factor and singular vectors.  Up to 4 waves per
    // block; fewer when two blocks per CU (two waves per SIMD) would not fit 160 KiB, or one block would not.
    int waves = 4;
    auto bytes = [&](int w) { return sizeof(float) * (kMaxB + (size_t)w * Park<N>::per_wave(args.n_b)); };
    while (waves > 1 && 2 * bytes(waves) > 160 * 1024) --waves;
    if (bytes(waves) > 160 * 1024) return set_error(PNX_ERR_UNSUPPORTED, "n_b=%d does not fit the LDS tile", args.n_b);
    const int block = waves * kWave;
    const size_t shmem = bytes(waves);
    if (hipError_t ea = allow_big_lds<curvefit_f32_kernel<MODEL, PV>>(); ea != hipSuccess)
        return set_error(PNX_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(ea));
    int occ = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, block, shmem);
    if (e != hipSuccess || occ < 1) return set_error(PNX_ERR_HIP, "occupancy query failed (shmem=%zu): %s", shmem, hipGetErrorString(e));
    long long want = (args.n_vox + block - 1) / block;
    long long cap = (long long)occ * device_cus;
    int grid = (int)(want < cap ? want : cap);
    if (grid < 1) grid = 1;
    if (dev_getenv("PNX_LAUNCH_TRACE"))
        fprintf(stderr, "[pnx launch] curvefit f32 model=%d N=%d PV=%d n_b=%d waves=%d lds=%zu occ=%d grid=%d\n", MODEL, N, (int)PV,
                args.n_b, waves, shmem, occ, grid);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), shmem, stream, args);
    e = hipGetLastError();
    if (e != hipSuccess) return set_error(PNX_ERR_HIP, "curvefit (fp32) launch: %s", hipGetErrorString(e));
    if (args.pcov) return launch_pcov<N>(args, cp, stream);
    return PNX_OK;
}

template <int MODEL> static int launch_model(const CurvefitF32Args &args, int cus, hipStream_t st) {
    return args.per_voxel ? launch_one<MODEL, true>(args, cus, st) : launch_one<MODEL, false>(args, cus, st);
}

}  // namespace f32
}  // namespace pnx

extern "C" int pnx_launch_curvefit_f32(int model, const pnx::f32::CurvefitF32Args *args, int cus, void *stream) {
    using namespace pnx::f32;
    hipStream_t st = (hipStream_t)stream;
    switch (model) {
    case 0: return launch_model<0>(*args, cus, st);
    case 1: return launch_model<1>(*args, cus, st);
    case 2: return launch_model<2>(*args, cus, st);
    case 3: return launch_model<3>(*args, cus, st);
    case 4: return launch_model<4>(*args, cus, st);
    case 5: return launch_model<5>(*args, cus, st);
    case 6: return launch_model<6>(*args, cus, st);
    }
    return pnx::set_error(PNX_ERR_INVALID, "unknown model %d", model);
}
