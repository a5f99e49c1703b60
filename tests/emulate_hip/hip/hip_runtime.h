// A stand-in for <hip/hip_runtime.h> that lets tests/*_emulate.cpp run the device text of csrc/m2t_moment_tile.h and the tile headers
// on it on the host (tests/emulate_hip/launch.h is the launch):
// a workgroup is a set of real threads, __syncthreads a barrier, a wave shuffle an exchange through memory.  Test scaffolding only.
#pragma once
#include <barrier>
#include <cmath>
#include <cstddef>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
struct dim3 { unsigned x = 1, y = 1, z = 1; };
inline thread_local dim3 threadIdx;
inline dim3 blockIdx, gridDim;
inline std::barrier<>* g_bar = nullptr;
inline double g_sh[1024];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline double __shfl_xor(double v, int o) {
  g_sh[threadIdx.x] = v; __syncthreads();
  double r = g_sh[threadIdx.x ^ o]; __syncthreads();
  return r;
}
using std::fma; using std::fmin; using std::fmax;
