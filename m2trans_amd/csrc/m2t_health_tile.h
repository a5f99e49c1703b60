// m2t_health_tile.h -- the per-lane text of the step health record (option "health" of include/m2t.h, which has the definition of a
// row; k_health.hip launches it).  Plain host + device functions without LDS or barriers, so that tests/health_emulate.cpp runs the
// same text on the host.
//
// A row's elements [0, n) are cut into chunks of CHUNK elements; one workgroup of LANES lanes takes a chunk.  Inside a chunk the
// elements go in groups of GROUP: group g of the chunk belongs to lane g % LANES, a lane visits its groups in ascending order and
// the elements of a group in ascending order, so every lane's fp64 sums are folded in an order the element index alone decides.
// The lanes are then folded by the tree  for s = LANES / 2 .. 1: lane[t] += lane[t + s]  (lane_merge), the chunks of a row by one
// thread per slot in ascending chunk order (fold_slot).  Nothing depends on the grid; nothing is atomic.
//
// A group is one 16-byte load (bf16) or two (fp32) where the row's base is 16-byte aligned and the group is whole; a plain loop over
// the same elements otherwise (an unaligned base, the tail of a row).  CHUNK is a multiple of GROUP, so alignment follows the base.
// Per lane the histogram is LANE_ELEMS <= 255 one-byte counters per bin, private to the lane: hist[bin * hstride], the lane's own
// byte at lane_slot(lane) of every bin's LANES bytes -- the 64 lanes of a wave 4 bytes apart, so that a wave's 64 counters of one
// visit lie in 64 different LDS banks whatever their bins are (bin * LANES is a multiple of the 256-byte bank period).
#ifndef M2T_HEALTH_TILE_H
#define M2T_HEALTH_TILE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace health_tile {

constexpr int CHUNK = 32768;                 // elements per chunk: the constant the fold order hangs on
constexpr int LANES = 256;                   // lanes (threads) per chunk
constexpr int GROUP = 8;                     // elements per visit of a lane
constexpr int LANE_ELEMS = CHUNK / LANES;    // 128: what one lane can count into one bin
constexpr int BINS = 64;
constexpr int SLOTS = 8 + BINS;              // doubles per row and per chunk partial
constexpr int BIN_LO = -41, BIN_HI = 20;     // floor(log2 |x|) is clamped to this range
static_assert(LANE_ELEMS <= 255 && CHUNK % (LANES * GROUP) == 0, "one-byte counters, whole groups per lane");

typedef float hf32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 hbf16x8 __attribute__((ext_vector_type(8)));

struct Lane {
  double s1, s2;        // sum and sum of squares over finite elements
  float mx, mn;         // max |x| over finite elements (0: none), min |x| over finite non-zero elements (+Inf: none)
  unsigned nan;         // NaNs
};
__host__ __device__ inline int lane_slot(int lane) { return (lane & 63) * 4 + (lane >> 6); }
__host__ __device__ inline void lane_clear(Lane& a) { a.s1 = 0.0; a.s2 = 0.0; a.mx = 0.f; a.mn = INFINITY; a.nan = 0u; }
__host__ __device__ inline void lane_merge(Lane& a, const Lane& b) {
  a.s1 += b.s1; a.s2 += b.s2;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.nan += b.nan;
}

// bin of an fp32 bit pattern: 0 zeros, 1 .. 62 = clamp(floor(log2 |x|), BIN_LO, BIN_HI) + 42 (subnormals: 1), 63 non-finite
__host__ __device__ inline int bin_of(uint32_t bits) {
  const int e = (int)((bits >> 23) & 0xffu);
  if (e == 255) return BINS - 1;
  if (e == 0) return (bits & 0x7fffffu) ? 1 : 0;
  int f = e - 127;
  f = f < BIN_LO ? BIN_LO : (f > BIN_HI ? BIN_HI : f);
  return f - BIN_LO + 1;
}

__host__ __device__ inline void visit(float v, Lane& a, unsigned char* hist, int hstride) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  const int b = bin_of(bits);
  hist[b * hstride] = (unsigned char)(hist[b * hstride] + 1);
  const bool bad = b == BINS - 1, body = !bad && b != 0;      // (+-0 is counted and adds nothing: the max of "finite elements" starts at 0)
  a.nan += (bad && (bits & 0x7fffffu)) ? 1u : 0u;
  const float m = fabsf(v);
  a.mx = (body && m > a.mx) ? m : a.mx;
  a.mn = (body && m < a.mn) ? m : a.mn;
  const double d = body ? (double)v : 0.0;                    // (adding +0.0 leaves a sum as it is; a sum is never -0.0)
  a.s1 += d;
  a.s2 += d * d;                                              // (the product of two fp32 values is exact in fp64)
}

template <typename T> __host__ __device__ inline void load_group(const T* p, float (&v)[GROUP]);
template <> __host__ __device__ inline void load_group<float>(const float* p, float (&v)[GROUP]) {
  const hf32x4 a = *reinterpret_cast<const hf32x4*>(p), b = *reinterpret_cast<const hf32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}
template <> __host__ __device__ inline void load_group<__bf16>(const __bf16* p, float (&v)[GROUP]) {
  const hbf16x8 a = *reinterpret_cast<const hbf16x8*>(p);
#pragma unroll
  for (int i = 0; i < GROUP; ++i) v[i] = (float)a[i];      // (bf16 -> fp32 is exact)
}

// lane `lane` of chunk `chunk` of a row of n elements at `base`; hist: the lane's BINS counters, cleared by the caller.
// Reads elements of [chunk * CHUNK, min(n, (chunk + 1) * CHUNK)) only.
template <typename T>
__host__ __device__ inline void lane_chunk(const T* base, long long n, long long chunk, int lane, Lane& a, unsigned char* hist, int hstride) {
  const long long lo = chunk * CHUNK;
  const long long hi = n - lo < CHUNK ? n : lo + CHUNK;
  const bool vec = (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
  for (long long g = lo + (long long)lane * GROUP; g < hi; g += (long long)LANES * GROUP) {
    if (vec && g + GROUP <= hi) {
      float v[GROUP];
      load_group<T>(base + g, v);
#pragma unroll
      for (int i = 0; i < GROUP; ++i) visit(v[i], a, hist, hstride);
    } else {
      const long long e = g + GROUP < hi ? g + GROUP : hi;
      for (long long i = g; i < e; ++i) visit((float)base[i], a, hist, hstride);
    }
  }
}

// the chunk's partial from the folded lanes and the summed counters (cnt[BINS]); n_chunk = elements of the chunk
__host__ __device__ inline void chunk_slot(const Lane& a, const unsigned* cnt, long long n_chunk, int slot, double* out) {
  double v;
  switch (slot) {
    case 0: v = (double)n_chunk; break;
    case 1: v = (double)cnt[BINS - 1]; break;
    case 2: v = (double)a.nan; break;
    case 3: v = (double)a.mx; break;
    case 4: v = a.s1; break;
    case 5: v = a.s2; break;
    case 6: v = (double)cnt[0]; break;
    case 7: v = (double)a.mn; break;
    default: v = (double)cnt[slot - 8]; break;
  }
  out[slot] = v;
}

// slot `slot` of a row from its chunks' partials, in ascending chunk order: max for [3], min for [7], a sum otherwise
__host__ __device__ inline double fold_slot(const double* parts, int nchunks, int slot) {
  double r = slot == 7 ? (double)INFINITY : 0.0;
  for (int c = 0; c < nchunks; ++c) {
    const double v = parts[(size_t)c * SLOTS + slot];
    if (slot == 3) r = v > r ? v : r;
    else if (slot == 7) r = v < r ? v : r;
    else r += v;
  }
  return r;
}

}  // namespace health_tile
#endif
