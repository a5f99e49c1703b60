// The host "launch" of the tile emulators (tests/ssim_emulate.cpp, msssim_emulate.cpp, vif_emulate.cpp): one set of nt threads per
// launch, the workgroups of a (gx, gy) grid run one after the other on it, g_smem is the workgroup's LDS.  Test scaffolding only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
static unsigned char* g_smem;
template <class F> void launch(int gx, int gy, int nt, size_t smem, F body) {
  gridDim.x = gx; gridDim.y = gy; gridDim.z = 1;
  unsigned char* buf = (unsigned char*)aligned_alloc(64, (smem + 63) / 64 * 64);
  g_smem = buf;
  std::barrier<> bar(nt); g_bar = &bar;
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) th.emplace_back([&, t] {
    threadIdx.x = t;
    for (int b = 0; b < gx * gy; ++b) {
      if (t == 0) { blockIdx.x = b % gx; blockIdx.y = b / gx; blockIdx.z = 0; }
      bar.arrive_and_wait();
      body();
      bar.arrive_and_wait();
    }
  });
  for (auto& t : th) t.join();
  free(buf);
}
