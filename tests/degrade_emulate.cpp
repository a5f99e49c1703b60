// Host emulation of k_degrade.hip for tests/test_degrade_cpu.py, one item: the tile text the device runs (csrc/m2t_degrade_tile.h: the
// staging of the folded HR halo tile and of the weights, the tap walk, the generator, the quantisation, the flip of the store position)
// on real threads with a barrier for __syncthreads (tests/emulate_hip), over the tile grid the launches use.  Built as plain C++ (no
// device code) with -ffp-contract=off, also under ASan / UBSan: the buffers are exact-size heap blocks, so a tap or a store outside
// them is reported.
//   degrade_emulate in.bin out.bin
// in:  int32 mode (0 = patch, 1 = whole image), H, W, s, K, ly, lx, lh, lw, flags, gray; uint64 noise_id, seed; double sigma_add,
//      sigma_speckle; double w[K][K]; uint8 hr[H][W][3]
// out: uint8 [lh][lw][3]: mode 0 at the flipped position (lh == lw), mode 1 in place
#include "m2t_degrade_tile.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace degrade_tile;
struct StoreU8 {
  unsigned char* out; int lw, flags, mode;
  void operator()(int y, int x, const int (&q)[CH]) const {
    int oy = y, ox = x;
    if (mode == 0) flipped(flags, lw, y, x, oy, ox);
    for (int c = 0; c < CH; ++c) out[((size_t)oy * lw + ox) * CH + c] = (unsigned char)q[c];
  }
};
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int h[11]; unsigned long long id[2]; double lev[2];
  if (fread(h, 4, 11, f) != 11 || fread(id, 8, 2, f) != 2 || fread(lev, 8, 2, f) != 2) return 2;
  const int mode = h[0], H = h[1], W = h[2], s = h[3], K = h[4], lh = h[7], lw = h[8], flags = h[9];
  if (K < 1 || K > KMAX || ((K ^ s) & 1) || s < 2 || s > 4 || H < 1 || W < 1 || lh < 1 || lw < 1) return 2;
  double* const w = (double*)malloc(sizeof(double) * K * K);
  unsigned char* const hr = (unsigned char*)malloc((size_t)H * W * CH);
  unsigned char* const out = (unsigned char*)malloc((size_t)lh * lw * CH);
  if (fread(w, 8, (size_t)K * K, f) != (size_t)K * K || fread(hr, 1, (size_t)H * W * CH, f) != (size_t)H * W * CH) return 2;
  fclose(f);
  memset(out, 0xAB, (size_t)lh * lw * CH);
  Item it;
  it.hr = hr; it.w = w; it.H = H; it.W = W; it.ly = h[5]; it.lx = h[6]; it.lh = lh; it.lw = lw; it.K = K; it.s = s;
  it.sigma_add = lev[0]; it.sigma_speckle = lev[1]; it.noise_id = id[0];
  it.seed_lo = (unsigned int)id[1]; it.seed_hi = (unsigned int)(id[1] >> 32); it.gray = h[10];
  const int gx = (lw + TL - 1) / TL, gy = (lh + TL - 1) / TL;
  launch(gx, gy, NT, sizeof(Smem), [&] {
    run_tile(*(Smem*)g_smem, it, blockIdx.y * TL, blockIdx.x * TL, mode == 0 && (flags & 4) != 0, StoreU8{out, lw, flags, mode}); });
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out, 1, (size_t)lh * lw * CH, f);
  fclose(f);
  free(w); free(hr); free(out);
  return 0;
}
