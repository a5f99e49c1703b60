// k_jpeg.hip -- JPEG compression artefacts (include/m2t_jpeg.h): the LR synthesis of k_degrade.hip with a simulated baseline JPEG round
// trip of a per-sample quality between the quantisation and the flips, and the stage alone on a uint8 image.
//
// MI355X-first, as k_degrade.hip: pool, bank and the 320 constants stay resident, the draws arrive in the kernel arguments, one launch
// per 32 samples.  A workgroup owns one 16 x 16 LR tile = 2 x 2 JPEG blocks (csrc/m2t_jpeg_tile.h): run_tile leaves the tile's 8-bit
// values in LDS as Y / Cb / Cr, four passes of eight fp64 multiply-adds per thread and plane take them through the DCT, the quantiser
// and back, and the store is the one of k_degrade.hip.  An item of quality 0 takes run_tile's own path: the bytes and the work of
// k_degrade.hip.  Static LDS, no scratch, no atomics; bit-reproducible.
#include "m2t_common.h"
#include "m2t_jpeg_tile.h"
#include "../../include/m2t_degrade.h"
#include "../../include/m2t_jpeg.h"
#include <cmath>
#include <cstring>

namespace {

using namespace degrade_tile;
using jpeg_tile::JSmem;

constexpr int DESC_PER_LAUNCH = 32;
static_assert(jpeg_tile::N_CONSTS == M2T_JPEG_CONSTS, "header and tile text agree on the constants");

struct JpegDesc {                     // DegradeDesc of k_degrade.hip with the quality in its padding
  long long hr_off;
  unsigned long long noise_id;
  double sigma_add, sigma_speckle;
  int H, W;
  int lx, ly;
  int flags, bank;
  int gray, quality;
};
struct JpegTable { JpegDesc d[DESC_PER_LAUNCH]; };   // 32 x 64 B of kernel arguments

struct StorePatch {                   // float32 CHW with the flips (k_degrade.hip)
  float* out; int lp, flags;
  __device__ __forceinline__ void operator()(int y, int x, const int (&q)[CH]) const {
    int oy, ox;
    flipped(flags, lp, y, x, oy, ox);
    float* dst = out + (long long)oy * lp + ox;
    for (int c = 0; c < CH; ++c) dst[(long long)c * lp * lp] = __fdiv_rn((float)q[c], 255.f);
  }
};
struct StoreImage {                   // uint8 HWC
  unsigned char* out; int lw;
  __device__ __forceinline__ void operator()(int y, int x, const int (&q)[CH]) const {
    unsigned char* dst = out + ((long long)y * lw + x) * CH;
    for (int c = 0; c < CH; ++c) dst[c] = (unsigned char)q[c];
  }
};

// grid (samples of this launch, tiles * tiles + ceil(hp^2 / 256)), as degrade_patches_kernel: the LR tiles first, then the HR half.
__global__ __launch_bounds__(NT) void degrade_jpeg_patches_kernel(const uint8_t* __restrict__ hr_pool, const double* __restrict__ bank,
                                                                  const double* __restrict__ consts, JpegTable tab, int first, int K, int lp,
                                                                  int scale, unsigned int seed_lo, unsigned int seed_hi,
                                                                  float* __restrict__ lr_out, float* __restrict__ hr_out) {
  __shared__ Smem sm;
  __shared__ JSmem js;
  const JpegDesc d = tab.d[blockIdx.x];
  const int tiles = (lp + TL - 1) / TL;
  const int hp = lp * scale;
  if ((int)blockIdx.y < tiles * tiles) {
    Item it;
    it.hr = hr_pool + d.hr_off; it.w = bank + (long long)d.bank * K * K;
    it.H = d.H; it.W = d.W; it.ly = d.ly; it.lx = d.lx; it.lh = lp; it.lw = lp; it.K = K; it.s = scale;
    it.sigma_add = d.sigma_add; it.sigma_speckle = d.sigma_speckle; it.noise_id = d.noise_id;
    it.seed_lo = seed_lo; it.seed_hi = seed_hi; it.gray = d.gray;
    const int ty = blockIdx.y / tiles, tx = blockIdx.y - ty * tiles;
    jpeg_tile::run_degrade_jpeg_tile(sm, js, it, consts, d.quality, ty * TL, tx * TL, (d.flags & 4) != 0,
                                     StorePatch{lr_out + (long long)(first + blockIdx.x) * CH * lp * lp, lp, d.flags});
    return;
  }
  // the HR half: crop_patches_kernel's index walk (k_datas.hip)
  const int nh = hp * hp;
  int i = (blockIdx.y - tiles * tiles) * NT + threadIdx.x;
  if (i >= nh) return;
  int y = i / hp, x = i - y * hp;
  if (d.flags & 4) { const int t = y; y = x; x = t; }
  if (d.flags & 2) y = hp - 1 - y;
  if (d.flags & 1) x = hp - 1 - x;
  const uint8_t* src = hr_pool + d.hr_off + ((long long)(d.ly * scale + y) * d.W + d.lx * scale + x) * CH;
  float* dst = hr_out + (long long)(first + blockIdx.x) * CH * nh + i;
  for (int c = 0; c < CH; ++c) dst[(long long)c * nh] = __fdiv_rn((float)src[c], 255.f);
}

// grid (ceil(lw / 16), ceil(lh / 16)): one workgroup per LR tile of the whole image
__global__ __launch_bounds__(NT) void degrade_jpeg_image_kernel(Item it, const double* __restrict__ consts, int quality,
                                                                unsigned char* __restrict__ out) {
  __shared__ Smem sm;
  __shared__ JSmem js;
  jpeg_tile::run_degrade_jpeg_tile(sm, js, it, consts, quality, blockIdx.y * TL, blockIdx.x * TL, false, StoreImage{out, it.lw});
}

// grid (ceil(W / 16), ceil(H / 16)): the stage alone
__global__ __launch_bounds__(NT) void jpeg_image_kernel(const uint8_t* __restrict__ img, int H, int W, const double* __restrict__ consts,
                                                        int quality, unsigned char* __restrict__ out) {
  __shared__ JSmem js;
  __shared__ double work[jpeg_tile::WORK_DOUBLES];
  jpeg_tile::run_image_tile(js, work, img, H, W, consts, quality, blockIdx.y * TL, blockIdx.x * TL, StoreImage{out, W});
}

const char* bank_error(int M, int K, int scale) {
  if (scale < 2 || scale > 4) return "scale must be 2, 3 or 4";
  if (M < 1) return "the bank is empty";
  if (K < 1 || K > KMAX || ((K ^ scale) & 1)) return "K must have the parity of scale: 1, 3 .. 21 (scale 3) or 2, 4 .. 20 (scale 2, 4)";
  return nullptr;
}
bool bad_level(double v) { return !(v >= 0.0) || std::isinf(v); }

}  // namespace

extern "C" int m2t_jpeg_quant_tables(int quality, int luma[64], int chroma[64]) {
  const char* who = "m2t_jpeg_quant_tables";
  if (!luma || !chroma) return m2t_set_error_at(M2T_ERR_ARG, who, "bad argument");
  if (quality < 1 || quality > 100) return m2t_set_error_at(M2T_ERR_ARG, who, "quality must be 1 .. 100");
  const int S = jpeg_tile::quant_scale(quality);
  for (int k = 0; k < 64; ++k) {
    luma[k] = jpeg_tile::quant_entry(0, k, S);
    chroma[k] = jpeg_tile::quant_entry(1, k, S);
  }
  return 0;
}

extern "C" int m2t_jpeg_image_u8(const unsigned char* img, int H, int W, int channels, const double* consts_dev, int quality,
                                 unsigned char* out, void* stream) {
  const char* who = "m2t_jpeg_image_u8";
  if (!img || !consts_dev || !out) return m2t_set_error_at(M2T_ERR_ARG, who, "bad argument");
  if (channels != CH) return m2t_set_error_at(M2T_ERR_ARG, who, "only 3 channels are built");
  if (H < 1 || W < 1 || H > (1 << 28) || W > (1 << 28)) return m2t_set_error_at(M2T_ERR_ARG, who, "H and W must be 1 .. 2^28");
  if (quality < 1 || quality > 100) return m2t_set_error_at(M2T_ERR_ARG, who, "quality must be 1 .. 100");
  const int gy = (H + TL - 1) / TL, gx = (W + TL - 1) / TL;
  if (gy > 65535) return m2t_set_error_at(M2T_ERR_ARG, who, "the image is taller than 1048560 rows");
  jpeg_image_kernel<<<dim3(gx, gy), NT, 0, (hipStream_t)stream>>>(img, H, W, consts_dev, quality, out);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" int m2t_degrade_jpeg_patches(const unsigned char* hr_pool, const double* bank_dev, int M, int K, const double* consts_dev,
                                        const long long* desc_host, int n, int channels, int patch_size, int scale,
                                        unsigned long long seed, float* lr_out, float* hr_out, void* stream) {
  const char* who = "m2t_degrade_jpeg_patches";
  if (!hr_pool || !bank_dev || !consts_dev || !desc_host || !lr_out || !hr_out || n < 1) return m2t_set_error_at(M2T_ERR_ARG, who, "bad argument");
  if (channels != CH) return m2t_set_error_at(M2T_ERR_ARG, who, "only 3 channels are built");
  if (const char* e = bank_error(M, K, scale)) return m2t_set_error_at(M2T_ERR_ARG, who, e);
  if (patch_size < scale || patch_size % scale) return m2t_set_error_at(M2T_ERR_ARG, who, "patch_size must be a positive multiple of scale");
  const int lp = patch_size / scale;
  if (lp > 16384) return m2t_set_error_at(M2T_ERR_ARG, who, "patch_size too large");
  for (int i = 0; i < n; ++i) {
    const long long* q = desc_host + (long long)M2T_DEGRADE_JPEG_DESC_COLS * i;
    double sa, ss;
    std::memcpy(&sa, q + 8, 8);
    std::memcpy(&ss, q + 9, 8);
    if (q[0] < 0 || q[1] < 1 || q[2] < 1 || q[1] > (1 << 28) || q[2] > (1 << 28) || q[3] < 0 || q[4] < 0)
      return m2t_set_error_at(M2T_ERR_ARG, who, "descriptor out of range");
    if ((q[3] + lp) * scale > q[2] || (q[4] + lp) * scale > q[1]) return m2t_set_error_at(M2T_ERR_ARG, who, "patch outside the image");
    if (q[5] & ~7LL) return m2t_set_error_at(M2T_ERR_ARG, who, "flags > 7");
    if (q[6] < 0 || q[6] >= M) return m2t_set_error_at(M2T_ERR_ARG, who, "bank index outside the bank");
    if (bad_level(sa) || bad_level(ss)) return m2t_set_error_at(M2T_ERR_ARG, who, "a noise level must be a finite number >= 0");
    if (q[10] != 0 && q[10] != 1) return m2t_set_error_at(M2T_ERR_ARG, who, "gray must be 0 or 1");
    if (q[11] < 0 || q[11] > 100) return m2t_set_error_at(M2T_ERR_ARG, who, "quality must be 0 (skipped) or 1 .. 100");
  }
  const int tiles = (lp + TL - 1) / TL;
  const long long blocks = (long long)tiles * tiles + ((long long)patch_size * patch_size + NT - 1) / NT;
  if (blocks > 65535) return m2t_set_error_at(M2T_ERR_ARG, who, "patch_size too large (more than 65535 workgroups per sample)");
  for (int first = 0; first < n; first += DESC_PER_LAUNCH) {
    const int m = n - first < DESC_PER_LAUNCH ? n - first : DESC_PER_LAUNCH;
    JpegTable tab;
    for (int i = 0; i < m; ++i) {
      const long long* q = desc_host + (long long)M2T_DEGRADE_JPEG_DESC_COLS * (first + i);
      JpegDesc& d = tab.d[i];
      d.hr_off = q[0]; d.noise_id = (unsigned long long)q[7];
      std::memcpy(&d.sigma_add, q + 8, 8);
      std::memcpy(&d.sigma_speckle, q + 9, 8);
      d.H = (int)q[1]; d.W = (int)q[2]; d.lx = (int)q[3]; d.ly = (int)q[4]; d.flags = (int)q[5]; d.bank = (int)q[6];
      d.gray = (int)q[10]; d.quality = (int)q[11];
    }
    for (int i = m; i < DESC_PER_LAUNCH; ++i) tab.d[i] = tab.d[0];
    degrade_jpeg_patches_kernel<<<dim3(m, (unsigned)blocks), NT, 0, (hipStream_t)stream>>>(
        hr_pool, bank_dev, consts_dev, tab, first, K, lp, scale, (unsigned int)seed, (unsigned int)(seed >> 32), lr_out, hr_out);
    M2T_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int m2t_degrade_jpeg_image_u8(const unsigned char* hr_img, int H, int W, int channels, const double* bank_dev, int M, int K,
                                         int index, int scale, unsigned long long seed, unsigned long long noise_id, double sigma_add,
                                         double sigma_speckle, int gray, const double* consts_dev, int quality, unsigned char* lr_u8_out,
                                         void* stream) {
  const char* who = "m2t_degrade_jpeg_image_u8";
  if (!hr_img || !bank_dev || !consts_dev || !lr_u8_out) return m2t_set_error_at(M2T_ERR_ARG, who, "bad argument");
  if (channels != CH) return m2t_set_error_at(M2T_ERR_ARG, who, "only 3 channels are built");
  if (const char* e = bank_error(M, K, scale)) return m2t_set_error_at(M2T_ERR_ARG, who, e);
  if (H < scale || W < scale || H > (1 << 28) || W > (1 << 28)) return m2t_set_error_at(M2T_ERR_ARG, who, "the image is smaller than one LR pixel (or too large)");
  if (index < 0 || index >= M) return m2t_set_error_at(M2T_ERR_ARG, who, "bank index outside the bank");
  if (bad_level(sigma_add) || bad_level(sigma_speckle)) return m2t_set_error_at(M2T_ERR_ARG, who, "a noise level must be a finite number >= 0");
  if (gray != 0 && gray != 1) return m2t_set_error_at(M2T_ERR_ARG, who, "gray must be 0 or 1");
  if (quality < 0 || quality > 100) return m2t_set_error_at(M2T_ERR_ARG, who, "quality must be 0 (skipped) or 1 .. 100");
  Item it;
  it.hr = hr_img; it.w = bank_dev + (long long)index * K * K;
  it.H = H; it.W = W; it.ly = 0; it.lx = 0; it.lh = H / scale; it.lw = W / scale; it.K = K; it.s = scale;
  it.sigma_add = sigma_add; it.sigma_speckle = sigma_speckle; it.noise_id = noise_id;
  it.seed_lo = (unsigned int)seed; it.seed_hi = (unsigned int)(seed >> 32); it.gray = gray;
  if ((long long)it.lh * it.lw > 0xffffffffLL) return m2t_set_error_at(M2T_ERR_ARG, who, "more than 2^32 LR pixels");
  const int gy = (it.lh + TL - 1) / TL, gx = (it.lw + TL - 1) / TL;
  if (gy > 65535) return m2t_set_error_at(M2T_ERR_ARG, who, "the LR image is taller than 1048560 rows");
  degrade_jpeg_image_kernel<<<dim3(gx, gy), NT, 0, (hipStream_t)stream>>>(it, consts_dev, quality, lr_u8_out);
  M2T_LAUNCH_CHECK();
  return 0;
}
