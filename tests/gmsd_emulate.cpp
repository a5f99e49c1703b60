// Host emulation of k_gmsd_loss.hip for tests/test_gmsd_loss_cpu.py, one image: the tile text the device runs (csrc/m2t_gmsd_tile.h:
// the staging of the pooled planes, phase 1, phase 2 with the transposed Prewitt pair and the scatter) on real threads with a barrier
// for __syncthreads (tests/emulate_hip), driven by the launch sequence of launch_gmsd_loss restated here: phase 1, record, phase 2.
// Built as plain C++ (no device code), also under ASan / UBSan.
//   gmsd_emulate in.bin out.bin
// in:  int32 H, W, row stride, C, clamp, vec; float R; double scale; float x[C][H][rs], y[C][H][W], gx[C][H][rs]
//      (vec != 0: take the 16-byte pieces where the strides allow; the buffers here are 16-byte aligned)
// out: float loss; double GMSD; float gx[C][H][rs] (after the add)
#include "m2t_gmsd_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace gmsd_tile;
template <class T> T* aligned(size_t n) { return (T*)aligned_alloc(64, (n * sizeof(T) + 63) / 64 * 64); }
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[6]; float R; double scale;
  if (fread(hdr, 4, 6, f) != 6 || fread(&R, 4, 1, f) != 1 || fread(&scale, 8, 1, f) != 1) return 2;
  const int H = hdr[0], W = hdr[1], rs = hdr[2], C = hdr[3], clamp = hdr[4], vec = hdr[5];
  const size_t nx = (size_t)C * H * rs, ny = (size_t)C * H * W;
  float* const x = aligned<float>(nx); float* const y = aligned<float>(ny); float* const gx = aligned<float>(nx);
  if (fread(x, 4, nx, f) != nx || fread(y, 4, ny, f) != ny || fread(gx, 4, nx, f) != nx) return 2;
  fclose(f);
  Src s;
  s.x = x; s.y = y; s.xs_ch = (long long)H * rs; s.xs_row = rs; s.ys_ch = (long long)H * W; s.ys_row = W; s.C = C; s.R = R; s.clamp = clamp;
  s.vec_x = vec && rs % 4 == 0 && s.xs_ch % 4 == 0; s.vec_y = vec && W % 4 == 0; s.iR = 1.0 / (double)R;
  const int hp = (H + 1) / 2, wp = (W + 1) / 2, ty = (hp + TP - 1) / TP, tx = (wp + TP - 1) / TP;
  std::vector<double> part((size_t)ty * tx * 2, 0.0);
  double* const P = part.data();
  launch(tx, ty, NT, SMEM_VALUE, [&] {
    double sd, sd2;
    value_tile(g_smem, s, H, W, hp, wp, blockIdx.y * TP, blockIdx.x * TP, sd, sd2);
    if (threadIdx.x == 0) { double* p = P + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2; p[0] = sd; p[1] = sd2; } });
  double sd = 0, sd2 = 0;
  for (size_t i = 0; i < part.size() / 2; ++i) { sd += part[2 * i]; sd2 += part[2 * i + 1]; }
  const double n = (double)hp * (double)wp, mean = sd / n;
  const double g = sqrt(fmax(sd2 / n - mean * mean, 0.0));
  const double coef = g > 0.0 ? scale / (n * g) : 0.0;
  if (coef != 0.0)
    launch(tx, ty, NT, SMEM_GRAD, [&] { grad_tile(g_smem, s, H, W, hp, wp, blockIdx.y * TP, blockIdx.x * TP, coef, mean, gx); });
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  const float loss = (float)(scale * g);
  fwrite(&loss, 4, 1, f); fwrite(&g, 8, 1, f); fwrite(gx, 4, nx, f);
  fclose(f);
  printf("GMSD %.17g loss %.9g\n", g, loss);
  free(x); free(y); free(gx);
  return 0;
}
