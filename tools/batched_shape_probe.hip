// A/B of k_solve_batched's workgroup shapes (waves per matrix x rows per
// wave) on B = 4096 seeded random matrices, fp64 and fp32, n = 16 ... 256:
// device-event time of the one launch, best of 5 after a warm-up, and whether
// every shape leaves the same eigenvectors bit for bit (it must: which wave
// holds a row changes no sum).  The shapes the launcher ships are the first
// row of each n (st_kernels.hip launch_solve_batched; DESIGN.md, Batched
// solve; profiles/batched_shape_probe.log).
//
//   make -C tools batched_shape_probe && tools/batched_shape_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstring>
#include "st_device.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

using namespace st::dev;

template <typename T, int WAVES, int RPW>
void run(const char* tname, uint32_t n, uint32_t B, T* master, T* work, T* v, st_state* st,
         std::vector<unsigned char>* ref)
{
  if (n > (uint32_t)(WAVES * RPW) || n > 64u * WAVES) { printf("bad shape\n"); exit(3); }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const size_t bytes = sizeof(T) * (size_t)B * n * n;
  float best = 1e30f;
  for (int rep = 0; rep < 6; rep++) {
    CK(hipMemcpy(work, master, bytes, hipMemcpyDeviceToDevice));
    CK(hipMemset(st, 0, sizeof(st_state) * B));
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL((k_solve_batched<T, 0, WAVES, RPW>), dim3(B), dim3(64 * WAVES), 0, 0,
                       work, v, n, (T)1e-3, 1000u, 0u, st, 1u);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep && ms < best) best = ms;
  }
  std::vector<unsigned char> got(sizeof(T) * (size_t)B * n);
  CK(hipMemcpy(got.data(), v, got.size(), hipMemcpyDeviceToHost));
  bool same = true;
  if (ref->empty()) *ref = got; else same = memcmp(ref->data(), got.data(), got.size()) == 0;
  std::vector<st_state> hs(B);
  CK(hipMemcpy(hs.data(), st, sizeof(st_state) * B, hipMemcpyDeviceToHost));
  uint32_t rmax = 0; for (auto& s : hs) rmax = s.end > rmax ? s.end : rmax;
  printf("%s n=%3u B=%u waves=%2d rpw=%2d : %8.4f ms  %10.0f matrices/s  %7.1f GB/s  rounds<=%u  v_same=%d\n",
         tname, n, B, WAVES, RPW, best, B / (best * 1e-3), 2.0 * bytes / (best * 1e-3) * 1e-9, rmax, (int)same);
  fflush(stdout);
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

template <typename T>
void all(const char* tname)
{
  const uint32_t B = 4096, NMAX = small_solve_max_n<T>();
  T *master, *work, *v; st_state* st;
  CK(hipMalloc(&master, sizeof(T) * (size_t)B * NMAX * NMAX));
  CK(hipMalloc(&work, sizeof(T) * (size_t)B * NMAX * NMAX));
  CK(hipMalloc(&v, sizeof(T) * (size_t)B * NMAX));
  CK(hipMalloc(&st, sizeof(st_state) * B));
  auto gen = [&](uint32_t n) {
    hipLaunchKernelGGL((k_generate<T, kRandom>), dim3(65536), dim3(kBlock), 0, 0, master, B * n, n, 0u, (uint64_t)11);
    CK(hipDeviceSynchronize());
  };
  std::vector<unsigned char> ref;
  gen(16); ref.clear();
  run<T, 4, 4>(tname, 16, B, master, work, v, st, &ref);
  run<T, 2, 8>(tname, 16, B, master, work, v, st, &ref);
  run<T, 1, 16>(tname, 16, B, master, work, v, st, &ref);
  gen(32); ref.clear();
  run<T, 4, 8>(tname, 32, B, master, work, v, st, &ref);
  run<T, 8, 4>(tname, 32, B, master, work, v, st, &ref);
  run<T, 2, 16>(tname, 32, B, master, work, v, st, &ref);
  gen(64); ref.clear();
  run<T, 4, 16>(tname, 64, B, master, work, v, st, &ref);
  run<T, 8, 8>(tname, 64, B, master, work, v, st, &ref);
  run<T, 16, 4>(tname, 64, B, master, work, v, st, &ref);
  gen(128); ref.clear();
  run<T, 8, 16>(tname, 128, B, master, work, v, st, &ref);
  run<T, 16, 8>(tname, 128, B, master, work, v, st, &ref);
  if constexpr (sizeof(T) == 4) {
    gen(256); ref.clear();
    run<T, 16, 16>(tname, 256, B, master, work, v, st, &ref);
  }
  CK(hipFree(master)); CK(hipFree(work)); CK(hipFree(v)); CK(hipFree(st));
}

int main()
{
  all<double>("f64");
  all<float>("f32");
  return 0;
}
