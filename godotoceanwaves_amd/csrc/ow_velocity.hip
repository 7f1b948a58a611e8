// ow_velocity.hip -- launchers of the velocity layers (kernels and layout in ow_velocity_kernels.h).
#include "ow_kernels.h"

namespace ow {
namespace {

// tw[m] = exp(2 pi i m / n), evaluated in FP64 and rounded once
__global__ __launch_bounds__(256) void k_velocity_twiddles(int n, cplx *tw) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    double s, c;
    sincospi(2.0 * (double)m / (double)n, &s, &c);
    tw[m] = cplx{(float)c, (float)s};
}

template <int N>
hipError_t launch_n(const VelocityArgs &args, const DeviceBuffers &buf, const cplx *tw, cplx *scratch, u16x4 *vel, hipStream_t s) {
    using P = VelPlan<N>;
    const dim3 grid(N / P::W, args.count);
    hipLaunchKernelGGL(k_velocity_pass1<N>, grid, dim3(P::THREADS), 0, s, args, buf.h0, buf.omega, tw, scratch);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_velocity_pass2<N>, grid, dim3(P::THREADS), 0, s, args, scratch, tw, vel);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_velocity_twiddles(int n, cplx *tw, hipStream_t s) {
    hipLaunchKernelGGL(k_velocity_twiddles, dim3((n + 255) / 256), dim3(256), 0, s, n, tw);
    return hipGetLastError();
}

hipError_t launch_velocity(int n, const VelocityArgs &args, const DeviceBuffers &buf, const cplx *tw, cplx *scratch, u16x4 *vel, hipStream_t s) {
    if (args.count < 1 || args.count > vel_batch(n)) return hipErrorInvalidValue;
    switch (n) {
        case 128: return launch_n<128>(args, buf, tw, scratch, vel, s);
        case 256: return launch_n<256>(args, buf, tw, scratch, vel, s);
        case 512: return launch_n<512>(args, buf, tw, scratch, vel, s);
        case 1024: return launch_n<1024>(args, buf, tw, scratch, vel, s);
        case 2048: return launch_n<2048>(args, buf, tw, scratch, vel, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ow
