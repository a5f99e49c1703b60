// Host emulation of k_jpeg.hip for tests/test_jpeg_cpu.py, one item: the tile text the device runs (csrc/m2t_jpeg_tile.h on
// csrc/m2t_degrade_tile.h: run_tile with the store into LDS, the colour transform, the four passes with their barriers, the skipped
// blocks of a partial tile, the flip of the store position) on real threads with a barrier for __syncthreads (tests/emulate_hip),
// over the tile grid the launches use.  Built as plain C++ (no device code) with -ffp-contract=off, also under ASan / UBSan: the
// buffers are exact-size heap blocks, so a read or a store outside them is reported.
//   jpeg_emulate in.bin out.bin
// in:  int32 mode (0 = degraded patch, 1 = degraded whole image, 2 = the stage alone on hr), H, W, s, K, ly, lx, lh, lw, flags, gray,
//      quality; uint64 noise_id, seed; double sigma_add, sigma_speckle; double consts[320]; double w[K][K]; uint8 hr[H][W][3]
// out: uint8 [lh][lw][3]: mode 0 at the flipped position (lh == lw), modes 1 and 2 in place
#include "m2t_jpeg_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace degrade_tile;
using namespace jpeg_tile;
struct StoreU8 {
  unsigned char* out; int lw, flags, mode;
  void operator()(int y, int x, const int (&q)[CH]) const {
    int oy = y, ox = x;
    if (mode == 0) flipped(flags, lw, y, x, oy, ox);
    for (int c = 0; c < CH; ++c) out[((size_t)oy * lw + ox) * CH + c] = (unsigned char)q[c];
  }
};
struct Lds { Smem sm; JSmem js; double work[WORK_DOUBLES]; };
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int h[12]; unsigned long long id[2]; double lev[2];
  if (fread(h, 4, 12, f) != 12 || fread(id, 8, 2, f) != 2 || fread(lev, 8, 2, f) != 2) return 2;
  const int mode = h[0], H = h[1], W = h[2], s = h[3], K = h[4], lh = h[7], lw = h[8], flags = h[9], quality = h[11];
  if (K < 1 || K > KMAX || ((K ^ s) & 1) || s < 2 || s > 4 || H < 1 || W < 1 || lh < 1 || lw < 1 || quality < 0 || quality > 100) return 2;
  if (mode == 2 && (lh != H || lw != W || quality < 1)) return 2;
  double* const consts = (double*)malloc(sizeof(double) * N_CONSTS);
  double* const w = (double*)malloc(sizeof(double) * K * K);
  unsigned char* const hr = (unsigned char*)malloc((size_t)H * W * CH);
  unsigned char* const out = (unsigned char*)malloc((size_t)lh * lw * CH);
  if (fread(consts, 8, N_CONSTS, f) != (size_t)N_CONSTS || fread(w, 8, (size_t)K * K, f) != (size_t)K * K ||
      fread(hr, 1, (size_t)H * W * CH, f) != (size_t)H * W * CH) return 2;
  fclose(f);
  memset(out, 0xAB, (size_t)lh * lw * CH);
  Item it;
  it.hr = hr; it.w = w; it.H = H; it.W = W; it.ly = h[5]; it.lx = h[6]; it.lh = lh; it.lw = lw; it.K = K; it.s = s;
  it.sigma_add = lev[0]; it.sigma_speckle = lev[1]; it.noise_id = id[0];
  it.seed_lo = (unsigned int)id[1]; it.seed_hi = (unsigned int)(id[1] >> 32); it.gray = h[10];
  const int gx = (lw + TL - 1) / TL, gy = (lh + TL - 1) / TL;
  launch(gx, gy, NT, sizeof(Lds), [&] {
    Lds& l = *(Lds*)g_smem;
    const StoreU8 store{out, lw, flags, mode};
    if (mode == 2) run_image_tile(l.js, l.work, hr, lh, lw, consts, quality, blockIdx.y * TL, blockIdx.x * TL, store);
    else run_degrade_jpeg_tile(l.sm, l.js, it, consts, quality, blockIdx.y * TL, blockIdx.x * TL, mode == 0 && (flags & 4) != 0, store);
  });
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out, 1, (size_t)lh * lw * CH, f);
  fclose(f);
  free(consts); free(w); free(hr); free(out);
  return 0;
}
