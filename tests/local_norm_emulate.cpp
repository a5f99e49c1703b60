// Host emulation of k_local_norm.hip for tests/test_local_norm_emulate_cpu.py: the per-thread text the device runs
// (csrc/m2t_local_norm_tile.h: hsum_segment, vapply_segment) over the thread decomposition of the two kernels, restated here as loops.
// A stand-alone program with its own main; built with clang (the header uses ext_vector_type and __bf16), also under ASan / UBSan:
// X, hs and Xn are heap blocks of exactly the plan's sizes, so an access outside a region is an error there.
//   local_norm_emulate in.bin out.bin
// in:  int32 dt (0 fp32, 1 bf16), B, H, W, T; float X[4][B*H*W][16] (values representable in the element type)
// out: float Xn[4][B*H*W][16]
#include "m2t_local_norm_tile.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace ln_tile;

template <typename T> T* block(size_t n) { return (T*)aligned_alloc(64, (n * sizeof(T) + 63) / 64 * 64); }

template <typename T> static void run(int B, int H, int W, int Tw, const float* xin, float* out) {
  const size_t n = (size_t)4 * B * H * W * 16;
  T* X = block<T>(n);
  T* Xn = block<T>(n);
  double* hs = block<double>(2 * n);
  for (size_t i = 0; i < n; ++i) { X[i] = (T)xin[i]; Xn[i] = (T)NAN; }
  for (size_t i = 0; i < 2 * n; ++i) hs[i] = NAN;                       // (the result does not depend on the scratch)
  const int kh = Tw < H ? Tw : H, kw = Tw < W ? Tw : W;
  const int nsx = (W + SEGX - 1) / SEGX, nsy = (H + SEGY - 1) / SEGY;
  const long long rows = (long long)B * H;
  // local_norm_hsum_kernel: thread = (quarter, column segment, row, chunk)
  for (long long chunk = 0; chunk < 4; ++chunk)
    for (long long row = 0; row < rows; ++row)
      for (int seg = 0; seg < nsx; ++seg)
        for (int q = 0; q < 4; ++q) {
          const size_t e = ((size_t)(chunk * rows + row) * W) * 16 + q * CPL;
          const int x0 = seg * SEGX;
          hsum_segment<T>(X + e, hs + 2 * e, x0, x0 + SEGX < W ? x0 + SEGX : W, W, kw);
        }
  // local_norm_vapply_kernel: thread = (quarter, column, row segment, image, chunk)
  const double cnt = (double)kh * (double)kw;
  for (long long chunk = 0; chunk < 4; ++chunk)
    for (long long b = 0; b < B; ++b)
      for (int seg = 0; seg < nsy; ++seg)
        for (int x = 0; x < W; ++x)
          for (int q = 0; q < 4; ++q) {
            const size_t e = (((size_t)(chunk * B + b) * H) * W + x) * 16 + q * CPL;
            const int y0 = seg * SEGY;
            vapply_segment<T>(hs + 2 * e, X + e, Xn + e, y0, y0 + SEGY < H ? y0 + SEGY : H, H, W, kh, cnt);
          }
  for (size_t i = 0; i < n; ++i) out[i] = (float)Xn[i];
  free(X); free(Xn); free(hs);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[5];
  if (fread(h, sizeof(int32_t), 5, f) != 5) return 2;
  const int dt = h[0], B = h[1], H = h[2], W = h[3], T = h[4];
  if (B < 1 || H < 1 || W < 1 || T < 1 || (dt != 0 && dt != 1)) return 2;
  const size_t n = (size_t)4 * B * H * W * 16;
  std::vector<float> x(n), y(n);
  if (fread(x.data(), sizeof(float), n, f) != n) return 2;
  fclose(f);
  if (dt == 0) run<float>(B, H, W, T, x.data(), y.data());
  else run<__bf16>(B, H, W, T, x.data(), y.data());
  f = fopen(argv[2], "wb");
  if (!f || fwrite(y.data(), sizeof(float), n, f) != n) return 2;
  fclose(f);
  return 0;
}
