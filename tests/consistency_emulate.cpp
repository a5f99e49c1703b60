// Host emulation of k_consistency.hip for tests/test_consistency_cpu.py: the tile text the device runs (csrc/m2t_consistency_tile.h:
// down_tile, finish_tile, adjoint_tile, update_tile) on real threads with a barrier for __syncthreads (tests/emulate_hip), driven by
// the launch sequences of k_consistency.hip restated here.  Built as plain C++ (no device code), also under ASan / UBSan.
//   consistency_emulate in.bin out.bin
// in:  int32 mode (0 loss, 1 back-projection, 2 adjoint alone), S, H, W (LR), row stride of x, planes, clamp, accumulate;
//      float R; double eps, scale (mode 1: beta); float x[planes][H S][rs], y[planes][H][W], gx[planes][H S][rs]
//      (mode 1: rs = W S, x is sr and is updated in place, gx is unused; mode 2: y is g, x is unused, gx is the destination)
// out: float loss; double stats[3]; float gx[planes][H S][rs]  (mode 1: the updated sr)
#include "m2t_consistency_tile.h"
#include "launch.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace cons_tile;
template <class T> T* aligned(size_t n) { return (T*)aligned_alloc(64, (n * sizeof(T) + 63) / 64 * 64); }

template <int S>
void run(int mode, int H, int W, int rs, int planes, int clamp, int accumulate, float R, double eps, double scale, float* x, const float* y,
         float* gx, float* loss, double* stats) {
  const int Hs = H * S, Ws = W * S;
  const int ty = (H + Down<S>::TQH - 1) / Down<S>::TQH, tx = (W + Down<S>::TQW - 1) / Down<S>::TQW;
  const size_t hw = (size_t)H * W, img = (size_t)Hs * rs;
  double* const plane = aligned<double>((size_t)planes * hw);
  double* const part = aligned<double>((size_t)planes * ty * tx * 4);
  for (size_t i = 0; i < (size_t)planes * hw; ++i) plane[i] = NAN;               // (the result does not depend on the scratch)
  for (size_t i = 0; i < (size_t)planes * ty * tx * 4; ++i) part[i] = NAN;
  const Taps down = make_taps(S, false), up = make_taps(S, true);
  if (mode != 2) {
    for (int z = 0; z < planes; ++z)
      launch(tx, ty, NT, Down<S>::SMEM, [&] {
        double sums[4];
        down_tile<S>(g_smem, x + z * img, rs, y + z * hw, H, W, blockIdx.y * Down<S>::TQH, blockIdx.x * Down<S>::TQW, R, clamp,
                     1.0 / (double)R, eps, mode == 1, down, plane + z * hw, sums);
        if (threadIdx.x == 0) {
          double* p = part + (((size_t)z * ty + blockIdx.y) * tx + blockIdx.x) * 4;
          for (int k = 0; k < 4; ++k) p[k] = sums[k];
        } });
    launch(1, 1, NT, 64, [&] {
      finish_tile((double*)g_smem, part, (long long)planes * ty * tx, (double)planes * (double)hw, mode == 0 ? scale : 0.0, accumulate,
                  mode == 0 ? loss : nullptr, stats); });
  }
  if (mode == 0 || mode == 2) {
    const int ay = (Hs + Adj<S>::TH - 1) / Adj<S>::TH, ax = (Ws + Adj<S>::TW - 1) / Adj<S>::TW;
    for (int z = 0; z < planes; ++z)
      launch(ax, ay, NT, Adj<S>::SMEM, [&] {
        if (mode == 0)
          adjoint_tile<S, double>(g_smem, plane + z * hw, H, W, blockIdx.y * Adj<S>::TH, blockIdx.x * Adj<S>::TW, x + z * img, rs, R, clamp,
                                  scale / (double)R, down, gx + z * img, rs, 1);
        else
          adjoint_tile<S, float>(g_smem, y + z * hw, H, W, blockIdx.y * Adj<S>::TH, blockIdx.x * Adj<S>::TW, nullptr, rs, 1.f, 0, 1.0, down,
                                 gx + z * img, rs, accumulate); });
  } else {
    const int uy = (H + Up::TQ - 1) / Up::TQ, ux = (W + Up::TQ - 1) / Up::TQ;
    const int vec = ((uintptr_t)x & 15) == 0 && Ws % 4 == 0;
    for (int z = 0; z < planes; ++z)
      launch(ux, uy, NT, Upd<S>::SMEM, [&] {
        update_tile<S>(g_smem, plane + z * hw, x + z * img, H, W, blockIdx.y * Up::TQ, blockIdx.x * Up::TQ, R, scale * (double)R, vec, up); });
  }
  free(plane); free(part);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[8]; float R; double eps, scale;
  if (fread(hdr, 4, 8, f) != 8 || fread(&R, 4, 1, f) != 1 || fread(&eps, 8, 1, f) != 1 || fread(&scale, 8, 1, f) != 1) return 2;
  const int mode = hdr[0], S = hdr[1], H = hdr[2], W = hdr[3], rs = hdr[4], planes = hdr[5], clamp = hdr[6], accumulate = hdr[7];
  if (S < 2 || S > 4 || H < 1 || W < 1 || rs < W * S || planes < 1 || (mode == 1 && rs != W * S)) return 2;
  const size_t nx = (size_t)planes * H * S * rs, ny = (size_t)planes * H * W;
  float* const x = aligned<float>(nx); float* const y = aligned<float>(ny); float* const gx = aligned<float>(nx);
  if (fread(x, 4, nx, f) != nx || fread(y, 4, ny, f) != ny || fread(gx, 4, nx, f) != nx) return 2;
  fclose(f);
  float loss = 0.25f;                                          // (accumulate adds to this)
  double stats[3] = {0.0, 0.0, 0.0};
  if (S == 2) run<2>(mode, H, W, rs, planes, clamp, accumulate, R, eps, scale, x, y, gx, &loss, stats);
  else if (S == 3) run<3>(mode, H, W, rs, planes, clamp, accumulate, R, eps, scale, x, y, gx, &loss, stats);
  else run<4>(mode, H, W, rs, planes, clamp, accumulate, R, eps, scale, x, y, gx, &loss, stats);
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(&loss, 4, 1, f); fwrite(stats, 8, 3, f); fwrite(mode == 1 ? x : gx, 4, nx, f);
  fclose(f);
  printf("loss %.9g stats %.17g %.17g %.17g\n", loss, stats[0], stats[1], stats[2]);
  free(x); free(y); free(gx);
  return 0;
}
