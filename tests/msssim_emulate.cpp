// Host emulation of k_msssim_loss.hip for tests/test_msssim_loss_cpu.py, one (image, channel): the tile text the device runs
// (csrc/m2t_ssim_tile.h: both instantiations, the cs and the SSIM map, value and gradient phases) on real threads with a barrier for
// __syncthreads (tests/emulate_hip), driven by the launch sequence of launch_msssim_loss restated here: pyramid, phase 1, record,
// phase 2 from the coarsest level down.  Built as plain C++ (no device code), also under ASan / UBSan.
//   msssim_emulate in.bin out.bin
// in:  int32 H, W, row stride, clamp; float R; double scale; float x[H][rs], y[H][W], gx[H][rs]
// out: float loss; double M; float gx[H][rs] (after the add); double x pyramid levels 1 .. 4
#include "m2t_ssim_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace ssim_tile;
using Tile0 = Tile<float, 32, 512>;
using TileP = Tile<double, 16, 256>;
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int hdr[4]; float R; double scale;
  fread(hdr, 4, 4, f); fread(&R, 4, 1, f); fread(&scale, 8, 1, f);
  const int H = hdr[0], W = hdr[1], rs = hdr[2], clamp = hdr[3];
  std::vector<float> x((size_t)H * rs), y((size_t)H * W), gx((size_t)H * rs);
  fread(x.data(), 4, x.size(), f); fread(y.data(), 4, y.size(), f); fread(gx.data(), 4, gx.size(), f); fclose(f);
  Taps win; { static const float k[6] = {0.0010283803567290306f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f, 0.21300552785396576f, 0.26601171493530273f};
    for (int i = 0; i < 11; ++i) win.g[i] = (double)k[i <= 5 ? i : 10 - i]; }
  int h[5], w[5]; h[0] = H; w[0] = W;
  for (int l = 1; l < 5; ++l) { h[l] = h[l-1] / 2 + h[l-1] % 2; w[l] = w[l-1] / 2 + w[l-1] % 2; }
  std::vector<double> xp[5], yp[5], g[5], part[5];
  for (int l = 1; l < 5; ++l) { xp[l].resize((size_t)h[l] * w[l]); yp[l].resize(xp[l].size()); g[l].resize(xp[l].size()); }
  // pyramid (sequential: no LDS, no barriers in the device kernel)
  for (int l = 1; l < 5; ++l) for (int oy = 0; oy < h[l]; ++oy) for (int ox = 0; ox < w[l]; ++ox) {
    const int Hi = h[l-1], Wi = w[l-1], iy0 = 2 * oy - (Hi & 1), ix0 = 2 * ox - (Wi & 1);
    double u[4], v[4];
    for (int k = 0; k < 4; ++k) {
      const int gy = iy0 + (k >> 1), gxx = ix0 + (k & 1); const bool in = gy >= 0 && gy < Hi && gxx >= 0 && gxx < Wi;
      if (l == 1) { float a = in ? x[(size_t)gy * rs + gxx] : 0.f; if (clamp) a = clamp_to(a, R); u[k] = a; v[k] = in ? (double)y[(size_t)gy * W + gxx] : 0.0; }
      else { u[k] = in ? xp[l-1][(size_t)gy * Wi + gxx] : 0.0; v[k] = in ? yp[l-1][(size_t)gy * Wi + gxx] : 0.0; }
    }
    xp[l][(size_t)oy * w[l] + ox] = (((u[0] + u[1]) + u[2]) + u[3]) * 0.25; yp[l][(size_t)oy * w[l] + ox] = (((v[0] + v[1]) + v[2]) + v[3]) * 0.25;
  }
  double v[5], n[5];
  for (int l = 0; l < 5; ++l) {
    const int ts = l ? 16 : 32, tx = (w[l] + ts - 1) / ts, ty = (h[l] + ts - 1) / ts;
    part[l].assign((size_t)tx * ty, 0.0);
    double* P = part[l].data();
    if (l == 0) launch(tx, ty, 512, Tile0::SMEM, [&] { double s = Tile0::maps<MAP_CS, true>(g_smem, x.data(), rs, y.data(), W, H, W, blockIdx.y * 32, blockIdx.x * 32, R, clamp, win); if (threadIdx.x == 0) P[blockIdx.y * gridDim.x + blockIdx.x] = s; });
    else if (l < 4) launch(tx, ty, 256, TileP::SMEM, [&] { double s = TileP::maps<MAP_CS, true>(g_smem, xp[l].data(), w[l], yp[l].data(), w[l], h[l], w[l], blockIdx.y * 16, blockIdx.x * 16, (double)R, 0, win); if (threadIdx.x == 0) P[blockIdx.y * gridDim.x + blockIdx.x] = s; });
    else launch(tx, ty, 256, TileP::SMEM, [&] { double s = TileP::maps<MAP_SSIM, true>(g_smem, xp[l].data(), w[l], yp[l].data(), w[l], h[l], w[l], blockIdx.y * 16, blockIdx.x * 16, (double)R, 0, win); if (threadIdx.x == 0) P[blockIdx.y * gridDim.x + blockIdx.x] = s; });
    n[l] = (double)(h[l] - 10) * (double)(w[l] - 10);
    double a = 0; for (double p : part[l]) a += p; v[l] = a / n[l];
  }
  const double wt[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  bool alive = true; double M = 1.0, c[5];
  for (int l = 0; l < 5; ++l) { alive = alive && v[l] > 0; M *= pow(fmax(v[l], 0.0), wt[l]); }
  if (!alive) M = 0;
  for (int l = 0; l < 5; ++l) c[l] = alive ? wt[l] * M / (v[l] * n[l]) : 0.0;
  if (alive) {
    for (int l = 4; l >= 1; --l) {
      const int tx = (w[l] + 15) / 16, ty = (h[l] + 15) / 16;
      const double* gp = l == 4 ? nullptr : g[l+1].data(); const int Wp = l == 4 ? 0 : w[l+1];
      double* go = g[l].data(); const double cl = c[l]; const int py = h[l] & 1, px = w[l] & 1, Wl = w[l];
      auto epi = [=](int gy, int gxx, double d, double) { double q = cl * d; if (gp) q += 0.25 * gp[(long long)((gy + py) >> 1) * Wp + ((gxx + px) >> 1)]; go[(long long)gy * Wl + gxx] = q; };
      if (l == 4) launch(tx, ty, 256, TileP::SMEM, [&] { TileP::maps<MAP_SSIM, false>(g_smem, xp[l].data(), w[l], yp[l].data(), w[l], h[l], w[l], blockIdx.y * 16, blockIdx.x * 16, (double)R, 0, win); TileP::grad(g_smem, h[l], w[l], blockIdx.y * 16, blockIdx.x * 16, (double)R, 0, win, epi); });
      else launch(tx, ty, 256, TileP::SMEM, [&] { TileP::maps<MAP_CS, false>(g_smem, xp[l].data(), w[l], yp[l].data(), w[l], h[l], w[l], blockIdx.y * 16, blockIdx.x * 16, (double)R, 0, win); TileP::grad(g_smem, h[l], w[l], blockIdx.y * 16, blockIdx.x * 16, (double)R, 0, win, epi); });
    }
    const double* gp = g[1].data(); const int Wp = w[1], py = H & 1, px = W & 1; const double cl = c[0], gcoef = -scale / (double)R; float* gxp = gx.data();
    launch((W + 31) / 32, (H + 31) / 32, 512, Tile0::SMEM, [&] {
      Tile0::maps<MAP_CS, false>(g_smem, x.data(), rs, y.data(), W, H, W, blockIdx.y * 32, blockIdx.x * 32, R, clamp, win);
      Tile0::grad(g_smem, H, W, blockIdx.y * 32, blockIdx.x * 32, R, clamp, win, [=](int gy, int gxx, double d, float) {
        double q = cl * d + 0.25 * gp[(long long)((gy + py) >> 1) * Wp + ((gxx + px) >> 1)];
        const long long o = (long long)gy * rs + gxx; gxp[o] = gxp[o] + (float)(gcoef * q); }); });
  }
  f = fopen(argv[2], "wb");
  float loss = (float)(scale * (1.0 - M)); fwrite(&loss, 4, 1, f); fwrite(&M, 8, 1, f); fwrite(gx.data(), 4, gx.size(), f);
  for (int l = 1; l < 5; ++l) fwrite(xp[l].data(), 8, xp[l].size(), f);
  fclose(f);
  printf("M %.17g loss %.9g\n", M, loss);
  return 0;
}
