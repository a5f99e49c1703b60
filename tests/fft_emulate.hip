// Host emulation of k_fft_loss.hip for tests/test_fft_loss_cpu.py: the three kernels' phases (csrc/m2t_fft.h, the text the device
// runs) with a loop over the thread index in place of a workgroup and a sequential fp64 sum in place of the fold of the partials.
//   fft_emulate in.bin out.bin
// in:  int32 B, C, H, W, rows, row stride, clamp, norm; double scale; float x[B][C][rows][rs], y[B][C][H][W], gx[B][C][rows][rs]
// out: float loss; float gx[B][C][rows][rs] (after the add); float spectrum[B*C][H][W/2+1][2] = the plain transform of y
#include "../m2trans_amd/csrc/m2t_fft.h"
#include <cmath>
#include <cstdio>
#include <vector>
using namespace m2t_fft;
static const int NT = 256;

static std::vector<float2> table(int N) {          // as twiddles() of k_fft_loss.hip
  std::vector<float2> t(N);
  for (int j = 0; j < N; ++j) {
    const double ang = -2.0 * M_PI * (double)j / (double)N;
    double c = cos(ang), s = sin(ang);
    if ((4 * j) % N == 0) { const int qd = 4 * j / N; c = qd == 0 ? 1.0 : (qd == 2 ? -1.0 : 0.0); s = qd == 1 ? -1.0 : (qd == 3 ? 1.0 : 0.0); }
    t[j] = make_float2((float)c, (float)s);
  }
  return t;
}

static float2* run(float2* a, float2* b, int N, int ld, int nseq, const float2* tw, int inv) {
  int n = N, s = 1;
  while (n > 1) {
    const int r = next_radix(n);
    for (int t = 0; t < NT; ++t) stage_any(r, a, b, N, ld, nseq, s, tw, inv, t, NT);
    float2* x = a; a = b; b = x; n /= r; s *= r;
  }
  return a;
}

static void rows_fwd(const Image& im, const float2* tw, float2* spec) {
  const int nseq = rows_nseq(im.W);
  std::vector<float2> a((size_t)nseq * im.W), b((size_t)nseq * im.W);
  for (long long blk = 0; blk < (im.npairs + nseq - 1) / nseq; ++blk) {
    for (int t = 0; t < NT; ++t) rows_load(im, a.data(), nseq, blk, t, NT);
    const float2* z = run(a.data(), b.data(), im.W, im.W, nseq, tw, 0);
    for (int t = 0; t < NT; ++t) rows_write(im, z, spec, nseq, blk, t, NT);
  }
}

// mode 0: the plain transform; 2: value and the adjoint of the signs.  Returns sum |Re| + |Im|.
static double cols(float2* spec, int planes, int H, int W, const float2* tw, int mode, float scale) {
  const int Wh = W / 2 + 1, sw = cols_strip(H), ld = cols_ld(H, sw), strips = (Wh + sw - 1) / sw;
  std::vector<float2> a((size_t)sw * ld), b((size_t)sw * ld);
  double sum = 0.0;
  for (int p = 0; p < planes; ++p)
    for (int st = 0; st < strips; ++st) {
      for (int t = 0; t < NT; ++t) cols_load(spec, a.data(), p, H, Wh, st * sw, sw, ld, t, NT);
      float2* z = run(a.data(), b.data(), H, ld, sw, tw, 0);
      for (int t = 0; t < NT; ++t) sum += cols_mid(z, H, W, st * sw, sw, ld, mode != 0, scale, t, NT);
      if (mode == 2) z = run(z, z == a.data() ? b.data() : a.data(), H, ld, sw, tw, 1);
      for (int t = 0; t < NT; ++t) cols_write(spec, z, p, H, Wh, st * sw, sw, ld, t, NT);
    }
  return sum;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int h[8];
  double scale;
  if (fread(h, 4, 8, f) != 8 || fread(&scale, 8, 1, f) != 1) return 4;
  const int B = h[0], C = h[1], H = h[2], W = h[3], rows = h[4], rs = h[5], clamp = h[6], norm = h[7];
  if (!size_supported(H) || !size_supported(W) || rows < H || rs < W || B < 1 || C < 1) return 5;
  const int planes = B * C, Wh = W / 2 + 1;
  const size_t nbuf = (size_t)planes * rows * rs, nimg = (size_t)planes * H * W;
  std::vector<float> x(nbuf), y(nimg), gx(nbuf);
  if (fread(x.data(), 4, nbuf, f) != nbuf || fread(y.data(), 4, nimg, f) != nimg || fread(gx.data(), 4, nbuf, f) != nbuf) return 6;
  fclose(f);
  const std::vector<float2> twW = table(W), twH = table(H);
  const double s = norm == 1 ? 1.0 / sqrt((double)H * (double)W) : 1.0;
  // the loss: launch_fft_loss
  std::vector<float2> spec((size_t)planes * H * Wh);
  const Image im{x.data(), y.data(), gx.data(), C, H, W, (long long)C * rows * rs, (long long)rows * rs, rs, 1.f, clamp, (long long)planes * (H / 2)};
  rows_fwd(im, twW.data(), spec.data());
  const double sum = cols(spec.data(), planes, H, W, twH.data(), 2, 1.f);
  {
    const int nseq = rows_nseq(W);
    std::vector<float2> a((size_t)nseq * W), b((size_t)nseq * W);
    for (long long blk = 0; blk < (im.npairs + nseq - 1) / nseq; ++blk) {
      for (int t = 0; t < NT; ++t) rowsadj_load(im, spec.data(), a.data(), nseq, blk, t, NT);
      const float2* z = run(a.data(), b.data(), W, W, nseq, twW.data(), 1);
      for (int t = 0; t < NT; ++t) rowsadj_add(im, z, scale * s / 1.0, nseq, blk, t, NT);
    }
  }
  const float loss = (float)(scale * s * sum);
  // the plain transform of y: m2t_rfft2
  std::vector<float2> out((size_t)planes * H * Wh);
  const Image plain{y.data(), nullptr, nullptr, 1, H, W, (long long)H * W, (long long)H * W, W, 1.f, 0, (long long)planes * (H / 2)};
  rows_fwd(plain, twW.data(), out.data());
  cols(out.data(), planes, H, W, twH.data(), 0, norm == 1 ? (float)s : 1.f);
  f = fopen(argv[2], "wb");
  if (!f) return 7;
  fwrite(&loss, 4, 1, f);
  fwrite(gx.data(), 4, nbuf, f);
  fwrite(out.data(), 8, out.size(), f);
  fclose(f);
  return 0;
}
