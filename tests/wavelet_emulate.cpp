// Host emulation of k_wavelet_loss.hip for tests/test_wavelet_loss_cpu.py, one image: the tile text the device runs
// (csrc/m2t_wavelet_tile.h: the wrapped staging, the forward level with its band sums and psi planes, the adjoint level with the
// scatter through the clamp mask) on real threads with a barrier for __syncthreads (tests/emulate_hip), driven by the launch sequence
// of launch_wavelet_loss restated here: the forward levels, the fold of the partial sums, the backward levels; then the transform
// alone of x.  Built as plain C++ (no device code), also under ASan / UBSan.
//   wavelet_emulate in.bin out.bin
// in:  int32 H, W, row stride, C, clamp, vec, taps, levels; float R; double scale, eps, lo[8], hi[8], w[10];
//      float x[C][H][rs], y[C][H][W], gx[C][H][rs]      (vec != 0: take the 16-byte pieces where the strides allow)
// out: float loss; double S[10]; float gx[C][H][rs] (after the add); float swt[C][3 levels + 1][H][W] (of x itself)
#include "m2t_wavelet_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace wavelet_tile;
template <class T> T* aligned(size_t n) { return (T*)aligned_alloc(64, (n * sizeof(T) + 63) / 64 * 64); }
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) return 2;
  int hdr[8]; float R; double scale, eps, w[MAXB];
  Filt f;
  if (fread(hdr, 4, 8, fp) != 8 || fread(&R, 4, 1, fp) != 1 || fread(&scale, 8, 1, fp) != 1 || fread(&eps, 8, 1, fp) != 1 ||
      fread(f.lo, 8, MAXL, fp) != MAXL || fread(f.hi, 8, MAXL, fp) != MAXL || fread(w, 8, MAXB, fp) != MAXB) return 2;
  const int H = hdr[0], W = hdr[1], rs = hdr[2], C = hdr[3], clamp = hdr[4], vec = hdr[5], taps = hdr[6], J = hdr[7];
  if (taps < 2 || taps > MAXL || J < 1 || J > MAXJ || H < ((taps - 1) << (J - 1)) + 1 || W < ((taps - 1) << (J - 1)) + 1 || rs < W) return 2;
  f.taps = taps;
  const int nb = 3 * J + 1;
  const size_t hw = (size_t)H * W, nx = (size_t)C * H * rs, ny = C * hw;
  float* const x = aligned<float>(nx); float* const y = aligned<float>(ny); float* const gx = aligned<float>(nx);
  float* const swt = aligned<float>(ny * nb);
  if (fread(x, 4, nx, fp) != nx || fread(y, 4, ny, fp) != ny || fread(gx, 4, nx, fp) != nx) return 2;
  fclose(fp);
  const int ty = (H + TH - 1) / TH, tx = (W + TW - 1) / TW;
  const size_t items = (size_t)C * ty * tx;
  double* const A[2] = {aligned<double>(ny), aligned<double>(ny)};
  double* const PSI = aligned<double>(ny * nb);
  double* const PART = aligned<double>(items * nb);
  memset(A[0], 0xFF, ny * 8); memset(A[1], 0xFF, ny * 8); memset(PSI, 0xFF, ny * nb * 8); memset(PART, 0xFF, items * nb * 8);
  const int vec_d = W % 2 == 0, vec_x = vec && rs % 4 == 0 && ((size_t)H * rs) % 4 == 0;
  int jmax = J;
  while (jmax > 1 && !(w[3 * (jmax - 1)] > 0 || w[3 * (jmax - 1) + 1] > 0 || w[3 * (jmax - 1) + 2] > 0 || (jmax == J && w[3 * J] > 0))) --jmax;
  for (int pass = 0; pass < 2; ++pass) {                       // 0: the loss, 1: the transform alone
    const int top = pass ? J : jmax;
    for (int j = 1; j <= top; ++j)
      for (int z = 0; z < C; ++z) {
        FwdOut o;
        for (int k = 0; k < 4; ++k) {
          const int gb = k < 3 ? 3 * (j - 1) + k : j == J ? 3 * J : -1;
          o.band[k] = pass && gb >= 0 ? swt + ((size_t)z * nb + gb) * hw : nullptr;
          o.w[k] = !pass && gb >= 0 ? w[gb] : 0.0;
          o.psi[k] = o.w[k] > 0.0 ? PSI + gb * ny + z * hw : nullptr;
        }
        o.a_out = j < top ? A[j & 1] + z * hw : nullptr;
        o.eps = eps; o.vec_f = vec && W % 4 == 0; o.vec_d = vec && vec_d;
        DiffSource ds;
        ds.W = W;
        ds.s.x = x + (size_t)z * H * rs; ds.s.y = pass ? nullptr : y + z * hw; ds.s.xs_ch = (long long)H * rs; ds.s.xs_row = rs;
        ds.s.R = R; ds.s.clamp = clamp; ds.s.vec_x = vec_x; ds.s.vec_y = vec && W % 4 == 0; ds.s.iR = 1.0 / (double)R;
        const PlaneSource ps{A[(j - 1) & 1] + z * hw, W, vec && vec_d};
        const bool small = small_reach(taps, 1 << (j - 1));      // (the variant launch_wavelet_loss picks for this level)
        launch(tx, ty, NT, small ? Geo<HM_SMALL>::SMEM : Geo<HM_BIG>::SMEM, [&] {
          double sum[4];
          const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, dil = 1 << (j - 1);
          if (j == 1 && small) fwd_tile<HM_SMALL>(g_smem, ds, H, W, y0, x0, dil, f, o, sum);
          else if (j == 1) fwd_tile<HM_BIG>(g_smem, ds, H, W, y0, x0, dil, f, o, sum);
          else if (small) fwd_tile<HM_SMALL>(g_smem, ps, H, W, y0, x0, dil, f, o, sum);
          else fwd_tile<HM_BIG>(g_smem, ps, H, W, y0, x0, dil, f, o, sum);
          if (threadIdx.x == 0)
            for (int k = 0; k < 4; ++k)
              if (o.w[k] > 0.0)
                PART[(k < 3 ? 3 * (j - 1) + k : 3 * J) * items + ((size_t)z * ty + blockIdx.y) * tx + blockIdx.x] = sum[k];
        });
      }
  }
  double S[MAXB] = {0}, total = 0.0;
  for (int b = 0; b < nb; ++b) {
    if (!(w[b] > 0.0)) continue;
    for (size_t i = 0; i < items; ++i) S[b] += PART[b * items + i];
    total = total + w[b] * S[b];
  }
  for (int j = jmax; j >= 1; --j)
    for (int z = 0; z < C; ++z) {
      const auto psi = [&](int b) -> const double* { return w[b] > 0.0 ? PSI + b * ny + z * hw : nullptr; };
      BwdIn in;
      in.abar = j == J ? psi(3 * J) : j == jmax ? nullptr : A[j & 1] + z * hw;
      in.lh = psi(3 * (j - 1)); in.hl = psi(3 * (j - 1) + 1); in.hh = psi(3 * (j - 1) + 2);
      in.vec = vec && vec_d;
      GradDst g;
      g.x = x + (size_t)z * H * rs; g.gx = gx + (size_t)z * H * rs; g.xs_row = rs; g.R = R; g.clamp = clamp; g.vec = vec_x;
      g.coef = scale * (1.0 / (double)R);
      double* const a_out = A[(j - 1) & 1] + z * hw;
      const bool small = small_reach(taps, 1 << (j - 1));
      launch(tx, ty, NT, small ? Geo<HM_SMALL>::SMEM : Geo<HM_BIG>::SMEM, [&] {
        const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, dil = 1 << (j - 1);
        if (j == 1 && small) bwd_tile<true, HM_SMALL>(g_smem, in, H, W, y0, x0, dil, f, nullptr, in.vec, g);
        else if (j == 1) bwd_tile<true, HM_BIG>(g_smem, in, H, W, y0, x0, dil, f, nullptr, in.vec, g);
        else if (small) bwd_tile<false, HM_SMALL>(g_smem, in, H, W, y0, x0, dil, f, a_out, in.vec, g);
        else bwd_tile<false, HM_BIG>(g_smem, in, H, W, y0, x0, dil, f, a_out, in.vec, g);
      });
    }
  fp = fopen(argv[2], "wb");
  if (!fp) return 2;
  const float loss = (float)(scale * total);
  fwrite(&loss, 4, 1, fp); fwrite(S, 8, MAXB, fp); fwrite(gx, 4, nx, fp); fwrite(swt, 4, ny * nb, fp);
  fclose(fp);
  printf("total %.17g loss %.9g\n", total, loss);
  free(x); free(y); free(gx); free(swt); free(A[0]); free(A[1]); free(PSI); free(PART);
  return 0;
}
