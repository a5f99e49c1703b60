// Host emulation of k_ssim_loss.hip for tests/test_ssim_loss_cpu.py, one (image, channel): the tile text the device runs
// (csrc/m2t_ssim_tile.h on csrc/m2t_moment_tile.h: Tile<float, 32, 512>, the 1 - SSIM map, value then gradient in one workgroup) on
// real threads with a barrier for __syncthreads (tests/emulate_hip), driven by the launch sequence of launch_ssim_loss restated
// here: the tile kernel, then the fold of the tiles' partial sums.  Built as plain C++ (no device code), also under ASan / UBSan.
//   ssim_emulate in.bin out.bin
// in:  int32 H, W, row stride, clamp; float R; double scale; float x[H][rs], y[H][W], gx[H][rs]
// out: float loss; float gx[H][rs] (after the add)
#include "m2t_ssim_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace ssim_tile;
using SsimTile = Tile<float, 32, 512>;
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[4]; float R; double scale;
  if (fread(hdr, 4, 4, f) != 4 || fread(&R, 4, 1, f) != 1 || fread(&scale, 8, 1, f) != 1) return 2;
  const int H = hdr[0], W = hdr[1], rs = hdr[2], clamp = hdr[3];
  std::vector<float> x((size_t)H * rs), y((size_t)H * W), gx((size_t)H * rs);
  if (fread(x.data(), 4, x.size(), f) != x.size() || fread(y.data(), 4, y.size(), f) != y.size() || fread(gx.data(), 4, gx.size(), f) != gx.size()) return 2;
  fclose(f);
  Taps win; { static const float k[6] = {0.0010283803567290306f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f, 0.21300552785396576f, 0.26601171493530273f};
    for (int i = 0; i < WIN; ++i) win.g[i] = (double)k[i <= 5 ? i : 10 - i]; }
  const int tx = (W + 31) / 32, ty = (H + 31) / 32;
  std::vector<double> part((size_t)tx * ty, 0.0);
  double* P = part.data(); float* gp = gx.data(); const double gcoef = -scale / (double)R;
  launch(tx, ty, SsimTile::NT, SsimTile::SMEM, [&] {
    const int y0 = blockIdx.y * 32, x0 = blockIdx.x * 32;
    const double tsum = SsimTile::maps<MAP_SSIM_LOSS, true>(g_smem, x.data(), rs, y.data(), W, H, W, y0, x0, R, clamp, win);
    if (threadIdx.x == 0) P[blockIdx.y * gridDim.x + blockIdx.x] = tsum;
    SsimTile::grad(g_smem, H, W, y0, x0, R, clamp, win, [=](int gy, int gxx, double d, float) {
      const long long o = (long long)gy * rs + gxx; gp[o] = gp[o] + (float)(gcoef * d); }); });
  double t = 0; for (double p : part) t += p;
  const float loss = (float)(scale * t);
  f = fopen(argv[2], "wb");
  fwrite(&loss, 4, 1, f); fwrite(gx.data(), 4, gx.size(), f);
  fclose(f);
  printf("loss %.9g\n", loss);
  return 0;
}
