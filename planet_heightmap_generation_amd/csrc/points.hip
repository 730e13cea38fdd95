// The Fibonacci sphere's points on the device: generateFibonacciSphere(N, jitter, makeRng(seed)) (js/sphere-mesh.js:9-37) plus the pole
// buildSphere appends (:179-181).  The arithmetic is points_ops.h's, the same bodies the test emulator (tests/emu_points) compiles.
//
// The host makes what the points share (fib_setup: the seed's state, s, dz and the two chain tables, a few dozen entries each) and one
// launch makes the points:
//   k_fib_points   one lane per point, grid-stride over k in [0, N]; k == N is the pole (0, 0, 1).  Every workgroup copies the two
//                  tables into LDS (CHAIN_CAP entries each, 12 KB) and its lanes search them there.
// Bounds: k <= N guards the stores to xyz[3k .. 3k + 2] of 3 (N + 1) floats; the table copies are clamped to CHAIN_CAP, and the binary
// search stays inside [0, n - 1].  Loops: the grid stride, 32 multiplications of the jump-ahead, 9 search steps, and inside the large
// reduction fixed trip counts over 20-entry work arrays (jz < 18, 16 recompute rounds at the most).
// Memory (device_mem.h): everything is a temporary of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "device.h"
#include "points_ops.h"

namespace P = wo::points;

namespace wo {

__global__ __launch_bounds__(WO_BLOCK) void k_fib_points(P::FibParams F, float* __restrict__ xyz) {
    __shared__ P::ChainEntry sLng[P::CHAIN_CAP], sZ[P::CHAIN_CAP];
    const int32_t nL = F.nLng < P::CHAIN_CAP ? F.nLng : P::CHAIN_CAP, nZ = F.nZ < P::CHAIN_CAP ? F.nZ : P::CHAIN_CAP;
    for (int32_t i = threadIdx.x; i < nL; i += WO_BLOCK) sLng[i] = F.lng[i];
    for (int32_t i = threadIdx.x; i < nZ; i += WO_BLOCK) sZ[i] = F.z[i];
    __syncthreads();
    F.lng = sLng; F.z = sZ; F.nLng = nL; F.nZ = nZ;
    const int64_t stride = (int64_t)gridDim.x * WO_BLOCK;
    for (int64_t k = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x; k <= (int64_t)F.N; k += stride) {
        float p[3] = {0.f, 0.f, 1.f};
        if (k < F.N) P::fib_point((int32_t)k, F, p);
        xyz[3 * k] = p[0]; xyz[3 * k + 1] = p[1]; xyz[3 * k + 2] = p[2];
    }
}

// N points and the pole into d_xyz (3 (N + 1) floats on the device), on stream s; the tables live in A.  false: a table overflowed
WO_LOCAL bool fib_points_to_device(hipStream_t s, DeviceArena& A, int32_t N, double jitter, double seed, float* d_xyz) {
    std::vector<P::ChainEntry> lng(P::CHAIN_CAP), z(P::CHAIN_CAP);
    P::FibParams F{};
    if (P::fib_setup(N, jitter, seed, lng.data(), z.data(), F)) return false;
    P::ChainEntry* h = A.pinned<P::ChainEntry>((size_t)F.nLng + F.nZ);       // pinned: the async copy below reads it after we return
    std::copy(lng.begin(), lng.begin() + F.nLng, h);
    std::copy(z.begin(), z.begin() + F.nZ, h + F.nLng);
    P::ChainEntry* d = A.dev<P::ChainEntry>((size_t)F.nLng + F.nZ);
    WO_HIP(hipMemcpyAsync(d, h, ((size_t)F.nLng + F.nZ) * sizeof(P::ChainEntry), hipMemcpyHostToDevice, s));
    F.lng = d; F.z = d + F.nLng;
    hipLaunchKernelGGL(k_fib_points, dim3((unsigned)blocks_for((int64_t)N + 1, 4096)), dim3(WO_BLOCK), 0, s, F, d_xyz);
    WO_HIP(hipGetLastError());
    return true;
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_fib_sphere_points_device(wo_ctx* ctx, int32_t N, double jitter, double seed, float* r_xyz) {
    if (!ctx) { set_error("wo_fib_sphere_points_device: null context"); return 1; }
    if (!r_xyz) { set_error("wo_fib_sphere_points_device: null pointer"); return 1; }
    if (N < 1 || N > P::FIB_MAX_N) { set_error("wo_fib_sphere_points_device: N out of range"); return 1; }
    WO_TRY
        WO_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DeviceArena A;                                        // the temporaries of this call
        const size_t n = 3 * ((size_t)N + 1);
        float* d_xyz = A.dev<float>(n);
        if (!fib_points_to_device(s, A, N, jitter, seed, d_xyz)) { set_error("wo_fib_sphere_points_device: chain table overflow"); return 1; }
        WO_HIP(hipMemcpyAsync(r_xyz, d_xyz, n * sizeof(float), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before A frees the temporaries
        return 0;
    WO_CATCH("wo_fib_sphere_points_device")
}

}  // extern "C"
