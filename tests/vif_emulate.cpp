// Host emulation of k_vif_loss.hip for tests/test_vif_loss_cpu.py, one image: the tile text the device runs (csrc/m2t_vif_tile.h: the
// pyramid tile, the four window instantiations of the moment tile, value and gradient phases, the gathered adjoint) on real threads
// with a barrier for __syncthreads (tests/emulate_hip), driven by the launch sequence of launch_vif_loss restated here: pyramid,
// phase 1, record, phase 2 from the coarsest scale down.  Built as plain C++ (no device code), also under ASan / UBSan.
//   vif_emulate in.bin out.bin
// in:  int32 H, W, row stride, C, clamp; float R; double scale, sigma_n_sq; float x[C][H][rs], y[C][H][W], gx[C][H][rs]
// out: float loss; double VIF; float gx[C][H][rs] (after the add); double u pyramid levels 1 .. 3
#include "m2t_vif_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace vif_tile;
template <int N> using TileN = Tile<N, 16, 256>;
struct Ctx {
  int h[SCALES], w[SCALES]; Src src0; Taps win[SCALES]; double nn;
  std::vector<double> up[SCALES], vp[SCALES], g[SCALES], part[SCALES];
  Src plane(int s) { Src p = src0; p.u = up[s].data(); p.v = vp[s].data(); p.row = w[s]; return p; }
};
template <int S> void pyramid(Ctx& c) {
  constexpr int N = win_len(S);
  const Src s = S == 1 ? c.src0 : c.plane(S - 1);
  launch((c.w[S] + PT - 1) / PT, (c.h[S] + PT - 1) / PT, 256, Pyr<N>::SMEM, [&] {
    pyr_tile<N, S == 1>(g_smem, s, c.h[S - 1], c.w[S - 1], c.h[S], c.w[S], c.win[S], c.up[S].data(), c.vp[S].data()); });
}
template <int S> void value(Ctx& c) {
  constexpr int N = win_len(S);
  const Src s = S == 0 ? c.src0 : c.plane(S);
  const int tx = (c.w[S] + 15) / 16, ty = (c.h[S] + 15) / 16;
  c.part[S].assign((size_t)tx * ty * 2, 0.0);
  double* P = c.part[S].data();
  launch(tx, ty, 256, TileN<N>::SMEM, [&] {
    double st = 0, sd = 0;
    TileN<N>::template maps<S == 0, true>(g_smem, s, c.h[S], c.w[S], blockIdx.y * 16, blockIdx.x * 16, c.nn, c.win[S], st, sd);
    if (threadIdx.x == 0) { double* p = P + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2; p[0] = st; p[1] = sd; } });
}
template <int S> void grad(Ctx& c, double coef_scale, float* gx) {
  constexpr int N = win_len(S), NP = S < SCALES - 1 ? win_len(S + 1) : 1;
  const Src s = S == 0 ? c.src0 : c.plane(S);
  const bool top = S == SCALES - 1;
  const double* gp = top ? nullptr : c.g[S + 1].data();
  const int Hp = top ? 0 : c.h[S + 1], Wp = top ? 0 : c.w[S + 1], Wl = c.w[S];
  const double* pg = c.win[top ? S : S + 1].g;
  double* go = S == 0 ? nullptr : c.g[S].data();
  const double coef = S == 0 ? -coef_scale * s.k255 : 0.0;
  launch((c.w[S] + 15) / 16, (c.h[S] + 15) / 16, 256, TileN<N>::SMEM, [&] {
    double st, sd;
    TileN<N>::template maps<S == 0, false>(g_smem, s, c.h[S], c.w[S], blockIdx.y * 16, blockIdx.x * 16, c.nn, c.win[S], st, sd);
    TileN<N>::grad(g_smem, c.h[S], c.w[S], blockIdx.y * 16, blockIdx.x * 16, c.win[S], [=](int gy, int gxx, double d) {
      double g = d;
      if (gp) g += parent_gather<NP>(gp, Hp, Wp, pg, gy, gxx);
      if (S == 0) {
        for (int ch = 0; ch < s.C; ++ch) {
          const long long o = (long long)ch * s.xs_ch + (long long)gy * s.xs_row + gxx;
          const float xv = s.x[o];
          if (s.clamp && !(xv >= 0.f && xv <= s.R)) continue;
          const double wch = s.C == 3 ? (ch == 0 ? 0.299 : ch == 1 ? 0.587 : 0.114) : 1.0;
          gx[o] = gx[o] + (float)(coef * wch * g);
        }
      } else {
        go[(long long)gy * Wl + gxx] = g;
      }
    }); });
}
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[5]; float R; double sc[2];
  if (fread(hdr, 4, 5, f) != 5 || fread(&R, 4, 1, f) != 1 || fread(sc, 8, 2, f) != 2) return 2;
  const int H = hdr[0], W = hdr[1], rs = hdr[2], C = hdr[3], clamp = hdr[4];
  const double scale = sc[0];
  std::vector<float> x((size_t)C * H * rs), y((size_t)C * H * W), gx((size_t)C * H * rs);
  if (fread(x.data(), 4, x.size(), f) != x.size() || fread(y.data(), 4, y.size(), f) != y.size() || fread(gx.data(), 4, gx.size(), f) != gx.size()) return 2;
  fclose(f);
  Ctx c;
  c.nn = sc[1];
  c.src0 = Src{x.data(), y.data(), (long long)H * rs, rs, (long long)H * W, W, C, R, clamp, 255.0 / (double)R, nullptr, nullptr, 0};
  for (int s = 0; s < SCALES; ++s) {
    c.h[s] = s ? decimated_side(c.h[s - 1], win_len(s)) : H;
    c.w[s] = s ? decimated_side(c.w[s - 1], win_len(s)) : W;
    for (int k = 0; k < MAXWIN; ++k) c.win[s].g[k] = 0.0;
    make_taps(win_len(s), c.win[s].g);
    if (s) { c.up[s].resize((size_t)c.h[s] * c.w[s]); c.vp[s].resize(c.up[s].size()); c.g[s].resize(c.up[s].size()); }
  }
  pyramid<1>(c); pyramid<2>(c); pyramid<3>(c);
  value<0>(c); value<1>(c); value<2>(c); value<3>(c);
  double tt = 0, dd = 0;
  for (int s = 0; s < SCALES; ++s) {
    double a = 0, b = 0;
    for (size_t i = 0; i < c.part[s].size() / 2; ++i) { a += c.part[s][2 * i]; b += c.part[s][2 * i + 1]; }
    tt += a; dd += b;
  }
  const double vif = (tt + EPS) / (dd + EPS), coef = scale / (dd + EPS);
  grad<3>(c, coef, gx.data()); grad<2>(c, coef, gx.data()); grad<1>(c, coef, gx.data()); grad<0>(c, coef, gx.data());
  f = fopen(argv[2], "wb");
  float loss = (float)(scale * (1.0 - vif)); fwrite(&loss, 4, 1, f); fwrite(&vif, 8, 1, f); fwrite(gx.data(), 4, gx.size(), f);
  for (int s = 1; s < SCALES; ++s) fwrite(c.up[s].data(), 8, c.up[s].size(), f);
  fclose(f);
  printf("VIF %.17g loss %.9g\n", vif, loss);
  return 0;
}
