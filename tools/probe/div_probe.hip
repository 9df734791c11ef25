// div_probe.hip -- csrc/div_shared.h on the hardware seed (v_rcp_f64), over arrays.
//
// k_div_probe<K>: thread g divides group g -- x[g K + i] / y[g K + i], i < K -- with div_shared<K>,
// as k_bp's short path does, and stores the K quotients.  tests/test_gpu_bp_division.py compares
// them bit for bit with float64 division on the host.  Built with -ffp-contract=off like bp.hip.
#include <hip/hip_runtime.h>

#include "../../ft8_demodulator_amd/csrc/div_shared.h"

namespace {

struct RcpHw {
  __device__ __forceinline__ double operator()(double v) const { return __builtin_amdgcn_rcp(v); }
};

template <int K>
__global__ __launch_bounds__(256) void k_div_probe(const double* x, const double* y, double* q, int groups) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= groups) return;
  double xs[K], ys[K], qs[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    xs[i] = x[(size_t)g * K + i];
    ys[i] = y[(size_t)g * K + i];
  }
  ft8::div_shared<K, (K % 3 == 0 ? 3 : K)>(qs, xs, ys, RcpHw());
#pragma unroll
  for (int i = 0; i < K; ++i) q[(size_t)g * K + i] = qs[i];
}

}  // namespace

// x, y, q: host arrays of groups * K doubles.  -> 0, a HIP error code, or -1 for a bad argument
extern "C" int ft8probe_div_shared(int K, const double* x, const double* y, double* q, int groups) {
  if ((K != 3 && K != 6 && K != 9) || groups <= 0 || groups > (1 << 24) || !x || !y || !q) return -1;
  const size_t bytes = (size_t)groups * K * sizeof(double);
  double *dx = nullptr, *dy = nullptr, *dq = nullptr;
  hipError_t e = hipMalloc(&dx, bytes);
  if (e == hipSuccess) e = hipMalloc(&dy, bytes);
  if (e == hipSuccess) e = hipMalloc(&dq, bytes);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dq, 0, bytes);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    if (K == 3) hipLaunchKernelGGL(k_div_probe<3>, grid, block, 0, 0, dx, dy, dq, groups);
    else if (K == 6) hipLaunchKernelGGL(k_div_probe<6>, grid, block, 0, 0, dx, dy, dq, groups);
    else hipLaunchKernelGGL(k_div_probe<9>, grid, block, 0, 0, dx, dy, dq, groups);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(q, dq, bytes, hipMemcpyDeviceToHost);
  if (dx) (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  if (dq) (void)hipFree(dq);
  return (int)e;
}
