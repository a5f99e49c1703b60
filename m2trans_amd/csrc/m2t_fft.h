// m2t_fft.h -- the arithmetic of k_fft_loss.hip: mixed-radix (4 / 2 / 3) Stockham stages on sequences held in LDS, and the
// per-workgroup phases of the three kernels (rows forward, columns forward + signs + adjoint, rows adjoint).
//
// Everything here is a function of (workgroup index, thread index, thread count) on plain pointers, so that the same text runs
// as the body of a kernel (phases separated by __syncthreads()) and on the host with a loop over the thread index in place of
// the workgroup (how the arithmetic was checked against fp64 before it ran on a device).
//
// Stockham, decimation in frequency, any order of radices: with n the length still to transform, s = N / n the stride reached,
// m = n / R, butterfly t = p * s + q (p < m, q < s) reads x[t + j * N / R] (j < R: consecutive t, conflict-free) and writes
//   y[q + s * (R * p + k)] = w_N^(p * s * k) * sum_j x[t + j * N / R] * w_R^(j * k)            (k < R),
// so every twiddle is an entry of ONE table of the N-th roots of unity (fp64 values rounded once to fp32 on the host), indexed
// without a recurrence.  Butterflies are fp32; inv != 0 conjugates the roots (the inverse-direction transform, unnormalised).
#pragma once
#include <hip/hip_runtime.h>

#define M2T_FFT_HD __host__ __device__ __forceinline__

namespace m2t_fft {

constexpr int MIN_N = 8, MAX_N = 2048;
constexpr int LDS_COMPLEX = 4096;          // complex values per ping-pong buffer a workgroup aims at (32 KB; two buffers)

// even, 8 .. 2048, 2^a * 3^b
M2T_FFT_HD bool size_supported(int n) {
  if (n < MIN_N || n > MAX_N || (n & 1)) return false;
  while (n % 2 == 0) n /= 2;
  while (n % 3 == 0) n /= 3;
  return n == 1;
}
M2T_FFT_HD int next_radix(int n) { return n % 4 == 0 ? 4 : (n % 2 == 0 ? 2 : 3); }

// row pairs per workgroup of the row kernels (a pair of real rows is ONE complex sequence of length W)
M2T_FFT_HD int rows_nseq(int W) { const int n = LDS_COMPLEX / W; return n < 1 ? 1 : (n > 8 ? 8 : n); }
// strip width of the column kernel: a power of two in 2 .. 16, chosen from H so that 2048 rows still fit
M2T_FFT_HD int cols_strip(int H) { int sw = 16; while (sw > 2 && sw * H > LDS_COMPLEX) sw >>= 1; return sw; }
// LDS stride (complex values) between the columns of a strip: the strip is read and written transposed (thread i: column i % SW,
// row i / SW), so a 32-lane group of ds_read_b64 covers SW columns x 32 / SW rows; ld = 32 / SW (mod 32) puts them on 32 distinct
// 8-byte bank pairs, where ld = H (a multiple of 32 at every training size) would put a whole group on 32 / SW of them.
M2T_FFT_HD int cols_ld(int H, int sw) { const int want = 32 / sw; return H + ((want - H % 32) + 32) % 32; }

// a / b and a % b for 0 <= a < 2^24 through the reciprocal (gfx950 has no integer divide; the indices of a stage are runtime values)
M2T_FFT_HD void divmod(int a, int b, float rb, int& q, int& r) {
  q = (int)((float)a * rb);
  r = a - q * b;
  if (r < 0) { --q; r += b; } else if (r >= b) { ++q; r -= b; }
}

M2T_FFT_HD float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
M2T_FFT_HD float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
M2T_FFT_HD float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// -i * a (forward) or +i * a (inverse direction)
M2T_FFT_HD float2 crot(float2 a, int inv) { return inv ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }
M2T_FFT_HD float2 root(const float2* tw, int idx, int inv) { float2 w = tw[idx]; if (inv) w.y = -w.y; return w; }

// one stage of radix R on nseq sequences of length N (sequence q at x + q * ld), x -> y
template <int R>
M2T_FFT_HD void stage(const float2* x, float2* y, int N, int ld, int nseq, int s, const float2* tw, int inv, int tid, int nth) {
  const int per = N / R, total = nseq * per;
  const float rper = 1.0f / (float)per, rs = 1.0f / (float)s;
  for (int i = tid; i < total; i += nth) {
    int seq, t, p, q;
    divmod(i, per, rper, seq, t);
    divmod(t, s, rs, p, q);
    const float2* xs = x + seq * ld + t;
    float2* ys = y + seq * ld + q + s * R * p;
    const int ti = p * s;
    if (R == 2) {
      const float2 a = xs[0], b = xs[per];
      ys[0] = cadd(a, b);
      ys[s] = cmul(csub(a, b), root(tw, ti, inv));
    } else if (R == 4) {
      const float2 a0 = xs[0], a1 = xs[per], a2 = xs[2 * per], a3 = xs[3 * per];
      const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = crot(csub(a1, a3), inv);
      ys[0] = cadd(t0, t2);
      ys[s] = cmul(cadd(t1, t3), root(tw, ti, inv));
      ys[2 * s] = cmul(csub(t0, t2), root(tw, 2 * ti, inv));
      ys[3 * s] = cmul(csub(t1, t3), root(tw, 3 * ti, inv));
    } else {
      const float2 a0 = xs[0], a1 = xs[per], a2 = xs[2 * per];
      const float2 u = cadd(a1, a2), d = csub(a1, a2);
      const float2 t2 = make_float2(a0.x - 0.5f * u.x, a0.y - 0.5f * u.y);
      const float2 t3 = crot(make_float2(0.8660254037844386f * d.x, 0.8660254037844386f * d.y), inv);     // sqrt(3) / 2
      ys[0] = cadd(a0, u);
      ys[s] = cmul(cadd(t2, t3), root(tw, ti, inv));
      ys[2 * s] = cmul(csub(t2, t3), root(tw, 2 * ti, inv));
    }
  }
}

M2T_FFT_HD void stage_any(int r, const float2* x, float2* y, int N, int ld, int nseq, int s, const float2* tw, int inv, int tid, int nth) {
  if (r == 4) stage<4>(x, y, N, ld, nseq, s, tw, inv, tid, nth);
  else if (r == 2) stage<2>(x, y, N, ld, nseq, s, tw, inv, tid, nth);
  else stage<3>(x, y, N, ld, nseq, s, tw, inv, tid, nth);
}

// ---- the image the loss works on -------------------------------------------------------------------------------------------------
// x [B][C][H][W] with strides (xs_img, xs_ch, xs_row, 1), y contiguous or NULL (the plain transform: d = x); gx has x's strides.
struct Image {
  const float* x; const float* y; float* gx;
  int C, H, W; long long xs_img, xs_ch; int xs_row; float R; int clamp;
  long long npairs;           // planes * H / 2
};

M2T_FFT_HD long long x_offset(const Image& im, long long plane, int row) {
  const long long b = plane / im.C, c = plane - b * im.C;
  return b * im.xs_img + c * im.xs_ch + (long long)row * im.xs_row;
}
// d = clamp(pre, 0, R) / R - hr / R as ONE fp32 value: (clamp(pre) - hr) / R
M2T_FFT_HD float diff_at(const Image& im, long long plane, int row, int w) {
  float xv = im.x[x_offset(im, plane, row) + w];
  if (!im.y) return xv;
  if (im.clamp) xv = fminf(fmaxf(xv, 0.f), im.R);
  return (xv - im.y[(plane * im.H + row) * im.W + w]) / im.R;
}

// ---- rows, forward: two real rows r0, r0 + 1 of one plane are the real and imaginary part of one complex sequence ----------------
M2T_FFT_HD void rows_load(const Image& im, float2* a, int nseq, long long blk, int tid, int nth) {
  const int W = im.W, hp = im.H / 2;
  const float rW = 1.0f / (float)W;
  for (int i = tid; i < nseq * W; i += nth) {
    int seq, w;
    divmod(i, W, rW, seq, w);
    const long long pair = blk * nseq + seq;
    float2 v = make_float2(0.f, 0.f);
    if (pair < im.npairs) {
      const long long plane = pair / hp;
      const int r0 = 2 * (int)(pair - plane * hp);
      v = make_float2(diff_at(im, plane, r0, w), diff_at(im, plane, r0 + 1, w));
    }
    a[i] = v;
  }
}
// Z = A + i B with A, B the spectra of the two real rows: A[k] = (Z[k] + conj Z[W-k]) / 2, B[k] = (Z[k] - conj Z[W-k]) / (2 i);
// the half spectrum k <= W / 2 goes to spec [planes][H][W / 2 + 1].  At k = 0 and W / 2 the imaginary parts are exactly 0.
M2T_FFT_HD void rows_write(const Image& im, const float2* z, float2* spec, int nseq, long long blk, int tid, int nth) {
  const int W = im.W, hp = im.H / 2, Wh = W / 2 + 1;
  const float rWh = 1.0f / (float)Wh;
  for (int i = tid; i < nseq * Wh; i += nth) {
    int seq, k;
    divmod(i, Wh, rWh, seq, k);
    const long long pair = blk * nseq + seq;
    if (pair >= im.npairs) continue;
    const float2 u = z[seq * W + k], v = z[seq * W + (k == 0 ? 0 : W - k)];
    const long long o = pair * 2 * Wh + k;                 // row r0 of the plane: (plane * H + r0) * Wh with plane * H + r0 = 2 * pair
    spec[o] = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));
    spec[o + Wh] = make_float2(0.5f * (u.y + v.y), 0.5f * (v.x - u.x));
  }
}

// ---- columns: a strip of sw adjacent kx over all H, column j of the strip at a + j * ld ---------------------------------------------
M2T_FFT_HD void cols_load(const float2* spec, float2* a, long long plane, int H, int Wh, int kx0, int sw, int ld, int tid, int nth) {
  const float rsw = 1.0f / (float)sw;
  for (int i = tid; i < H * sw; i += nth) {
    int h, j;
    divmod(i, sw, rsw, h, j);
    a[j * ld + h] = kx0 + j < Wh ? spec[(plane * H + h) * Wh + kx0 + j] : make_float2(0.f, 0.f);
  }
}
M2T_FFT_HD void cols_write(float2* spec, const float2* a, long long plane, int H, int Wh, int kx0, int sw, int ld, int tid, int nth) {
  const float rsw = 1.0f / (float)sw;
  for (int i = tid; i < H * sw; i += nth) {
    int h, j;
    divmod(i, sw, rsw, h, j);
    if (kx0 + j < Wh) spec[(plane * H + h) * Wh + kx0 + j] = a[j * ld + h];
  }
}
M2T_FFT_HD float sign0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }          // sign(0) = 0 (and a NaN gives 0)
// After the column transform: the imaginary part of the four self-conjugate bins is forced to exactly 0.  signs == 0: the values
// times `scale` stay (the plain transform).  signs != 0: returns this thread's share of sum |Re| + |Im| in fp64 and replaces the
// values by their signs.
M2T_FFT_HD double cols_mid(float2* a, int H, int W, int kx0, int sw, int ld, int signs, float scale, int tid, int nth) {
  const float rH = 1.0f / (float)H;
  double acc = 0.0;
  for (int i = tid; i < H * sw; i += nth) {
    int j, ky;
    divmod(i, H, rH, j, ky);
    float2 v = a[j * ld + ky];
    const int kx = kx0 + j;
    if ((ky == 0 || ky == H / 2) && (kx == 0 || kx == W / 2)) v.y = 0.f;
    if (signs) {
      acc += (double)fabsf(v.x) + (double)fabsf(v.y);
      v = make_float2(sign0(v.x), sign0(v.y));
    } else {
      v = make_float2(v.x * scale, v.y * scale);
    }
    a[j * ld + ky] = v;
  }
  return acc;
}

// ---- rows, adjoint: g[w] = Re sum_{k <= W/2} G[k] e^{+2 pi i k w / W} (no Hermitian doubling) is the inverse-direction transform of
// the Hermitian part S[k] = (G^[k] + conj G^[W-k]) / 2 of the zero-extended half spectrum G^; two rows again share one sequence,
// Z = S_a + i S_b, whose transform is g_a + i g_b.
M2T_FFT_HD void rowsadj_load(const Image& im, const float2* spec, float2* a, int nseq, long long blk, int tid, int nth) {
  const int W = im.W, Wh = W / 2 + 1;
  const float rW = 1.0f / (float)W;
  for (int i = tid; i < nseq * W; i += nth) {
    int seq, k;
    divmod(i, W, rW, seq, k);
    const long long pair = blk * nseq + seq;
    float2 v = make_float2(0.f, 0.f);
    if (pair < im.npairs) {
      const int kk = k <= W / 2 ? k : W - k;
      const float2 ga = spec[pair * 2 * Wh + kk], gb = spec[pair * 2 * Wh + Wh + kk];
      float2 sa, sb;
      if (k == 0 || k == W / 2) { sa = make_float2(ga.x, 0.f); sb = make_float2(gb.x, 0.f); }
      else if (k < W / 2) { sa = make_float2(0.5f * ga.x, 0.5f * ga.y); sb = make_float2(0.5f * gb.x, 0.5f * gb.y); }
      else { sa = make_float2(0.5f * ga.x, -0.5f * ga.y); sb = make_float2(0.5f * gb.x, -0.5f * gb.y); }
      v = make_float2(sa.x - sb.y, sa.y + sb.x);
    }
    a[i] = v;
  }
}
// gx += (float)(gcoef * g) where the clamp passes (ends of [0, R] included): one fp32 rounding per gradient value, one fp32 add
M2T_FFT_HD void rowsadj_add(const Image& im, const float2* z, double gcoef, int nseq, long long blk, int tid, int nth) {
  const int W = im.W, hp = im.H / 2;
  const float rW = 1.0f / (float)W;
  for (int i = tid; i < nseq * W; i += nth) {
    int seq, w;
    divmod(i, W, rW, seq, w);
    const long long pair = blk * nseq + seq;
    if (pair >= im.npairs) continue;
    const long long plane = pair / hp;
    const int r0 = 2 * (int)(pair - plane * hp);
    const float2 g = z[i];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const long long o = x_offset(im, plane, r0 + e) + w;
      const float xv = im.x[o];
      if (im.clamp && !(xv >= 0.f && xv <= im.R)) continue;
      im.gx[o] = im.gx[o] + (float)(gcoef * (double)(e ? g.y : g.x));
    }
  }
}

}  // namespace m2t_fft
