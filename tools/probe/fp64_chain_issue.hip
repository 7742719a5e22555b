// Developer probe (GPU box): at what rate does a SIMD issue v_fma_f64 when a wave offers it C independent
// dependency chains, with 1, 2 or 4 waves resident on the SIMD?  (Value by value, the fast sine of
// csrc/tfem_source.hpp is ONE chain; would interleaving several values pay?  On MI355X: no -- one chain
// issues as fast as eight, and what sets the rate is the number of waves, profiles/fused_chain_interleave.log.)
//   hipcc --offload-arch=gfx950 -O2 -o /tmp/fp64_chain_issue tools/probe/fp64_chain_issue.hip && /tmp/fp64_chain_issue
// Workgroups of 256 lanes (one wave per SIMD); the grid is (compute units) x R workgroups, each padded with
// so much LDS that exactly R fit on a compute unit, so R waves share every SIMD.  Every lane runs kIters x
// kBody fused multiply-adds, dealt round-robin to C accumulators; wave 0 of a workgroup stamps the loop
// with s_memtime.  Printed: shader cycles per instruction PER SIMD = ticks / (instructions x R), median
// over the workgroups (and the slowest workgroup's, which shows an uneven placement).
//   "vgpr":    acc = fma(acc, x, y), all operands in vector registers
//   "literal": acc = fma(acc, x, K_j), K_j 64-bit constants in scalar registers -- the Horner steps of the sine
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                   \
  do {                                                                                \
    const hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess) {                                                           \
      std::printf("%s failed: %s\n", #call, hipGetErrorString(e_));                   \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

constexpr int kBody = 48;  // a multiple of every C
constexpr int kIters = 2000;

template <int C, bool LIT>
__global__ __launch_bounds__(256) void chain(double *out, long long *ticks, int iters, double x0, double y0) {
  extern __shared__ char pad[];
  double acc[C];
#pragma unroll
  for (int j = 0; j < C; ++j) acc[j] = 1e-3 * threadIdx.x + j;
  const double x = x0 + 1e-9 * threadIdx.x, y = y0 + 1e-9 * threadIdx.x;
  constexpr double lit[8] = {-7.64397029616579265e-13, 1.60589773124442683e-10, -2.50521076169958777e-08,
                             2.75573192191632300e-06,  -1.98412698412549741e-04, 8.33333333333331587e-03,
                             -1.66666666666666657e-01, 2.73144475909634011e-15};
  const long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int j = 0; j < kBody; ++j) {
      if constexpr (LIT) acc[j % C] = __builtin_fma(acc[j % C], x, lit[(j / C) % 8]);
      else acc[j % C] = __builtin_fma(acc[j % C], x, y);
    }
#pragma unroll
    for (int j = 0; j < C; ++j) asm volatile("" : "+v"(acc[j]));  // the loop stays a loop of kBody instructions
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < C; ++j) s += acc[j];
  out[size_t(blockIdx.x) * blockDim.x + threadIdx.x] = s;
  if (threadIdx.x == 0) ticks[blockIdx.x] = t1 - t0;
}

template <int C, bool LIT>
void run(int cus, int resident, double *out, long long *ticks) {
  // LDS per workgroup: `resident` fit into the 160 KiB of a compute unit, `resident` + 1 do not
  const int lds = resident == 1 ? 100 * 1024 : resident == 2 ? 60 * 1024 : 36 * 1024;
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&chain<C, LIT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            lds));
  const int grid = cus * resident;
  std::vector<long long> t(grid);
  for (int rep = 0; rep < 3; ++rep) {  // the last launch counts (clocks up, code cached)
    chain<C, LIT><<<grid, 256, lds>>>(out, ticks, kIters, 0.5, 0.25);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
  }
  CHECK(hipMemcpy(t.data(), ticks, grid * sizeof(long long), hipMemcpyDeviceToHost));
  std::sort(t.begin(), t.end());
  const double per = double(kIters) * kBody * resident;
  std::printf("  %-7s C %d  waves/SIMD %d   median %6.3f   slowest %6.3f  cycles / instruction / SIMD\n",
              LIT ? "literal" : "vgpr", C, resident, t[grid / 2] / per, t[grid - 1] / per);
}

template <int C>
void both(int cus, double *out, long long *ticks) {
  for (int r : {1, 2, 4}) run<C, false>(cus, r, out, ticks);
  for (int r : {1, 2, 4}) run<C, true>(cus, r, out, ticks);
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  std::printf("%s, %d compute units; %d x %d v_fma_f64 per lane and launch\n", prop.name, cus, kIters, kBody);
  double *out;
  long long *ticks;
  CHECK(hipMalloc(&out, size_t(cus) * 4 * 256 * sizeof(double)));
  CHECK(hipMalloc(&ticks, size_t(cus) * 4 * sizeof(long long)));
  both<1>(cus, out, ticks);
  both<2>(cus, out, ticks);
  both<3>(cus, out, ticks);
  both<4>(cus, out, ticks);
  both<8>(cus, out, ticks);
  CHECK(hipFree(out));
  CHECK(hipFree(ticks));
  return 0;
}
