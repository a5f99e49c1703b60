// m2t_window.h -- geometry of the 8x8-query / 10x10-key halo windows (models/M2Trans_network.py:310-317),
// shared by the attention kernels and the fused branch kernel.
#pragma once
#include "m2t_common.h"

#define WA_NK 100
#define WA_KT 7          // key tiles that can hold real keys (112)
#define WA_KR 128        // key rows staged (4 contraction chunks of 32)
#define WA_QP 72         // 64 queries + 8 pad

// A key coordinate clamped into an image axis of n pixels: where the kernels whose loads are unconditional read for a key
// outside the image (the value is then zeroed by a select).
__device__ __forceinline__ int clamp_px(int v, int n) { return min(max(v, 0), n - 1); }
// Raster key order: key = 10 kr + kc, (kr, kc) the position in the 10x10 neighbourhood (0 and 9: the ring).
// (dkv_row and three kernel sites keep the division written out: hipcc folds their range tests on kr into the division
// before it inlines anything, and through a call it generates other code.)
__device__ __forceinline__ void key_rc(int key, int& kr, int& kc) {
  kr = key / 10;
  kc = key - kr * 10;
}
// The same for key < 1024 (205 / 2^11 = 1 / 9.99..: exact up to 1023) with a 24-bit multiply.  On purpose: the kernels that use it
// compute one address per lane and load from it, a 32-bit multiply or a 64-bit pixel index per lane costs v_mul_lo_u32 /
// v_mad_u64_u32, quarter-rate instructions, and phase 0 of those kernels is bound by exactly that integer work
// (profiles/r06_attn_phase0_integer_work.txt).
__device__ __forceinline__ void key_rc_fast(int key, int& kr, int& kc) {
  kr = (int)(__umul24((unsigned)key, 205u) >> 11);
  kc = key - 10 * kr;
}
// Own-pixels-first key order of the fused forward kernels: 0..63 the window's own pixels (= query order, so the first four 16-row
// tiles serve the q projection too), 64..99 the ring, where key 64 + r is the ring key with ring_index(kr, kc) == r (below).
// Branch-free (selects): the callers issue loads whose addresses depend on the result.
__device__ __forceinline__ void own_first_key_rc(int k, int& kr, int& kc) {
  const int r = k - 64;
  const int kr_ring = (r < 10) ? 0 : ((r < 20) ? 9 : ((r < 28) ? r - 19 : r - 27));
  const int kc_ring = (r < 10) ? r : ((r < 20) ? r - 10 : ((r < 28) ? 0 : 9));
  kr = (k < 64) ? (k >> 3) + 1 : kr_ring;
  kc = (k < 64) ? (k & 7) + 1 : kc_ring;
}

struct WinGeom {
  int h, w, nw, nh;
  int b, wy, wx;
  int wi;                 // logical window index (XCD-aware, see xcd_block_index)
  // pixel of raster key `key`; false: outside the image (ring keys of border windows: zero padding)
  __device__ __forceinline__ bool key_pixel(int key, long long& pix) const {
    int kr, kc;
    key_rc(key, kr, kc);
    const int y = 8 * wy + kr - 1, x = 8 * wx + kc - 1;
    pix = ((long long)b * h + y) * w + x;
    return (y >= 0 && y < h && x >= 0 && x < w);
  }
  __device__ __forceinline__ long long query_pixel(int q) const {
    return ((long long)b * h + 8 * wy + (q >> 3)) * w + 8 * wx + (q & 7);
  }
};
// dK|dV rows of a window's backward: the 64 keys that are the window's OWN pixels (kr, kc in 1..8) go straight to
// their row of gqkv ([pixel][3C], columns C..3C); the 36 ring keys go to the per-window scratch `win`
// [window][36][2C] and are added by halo_gather to the border pixels of the neighbouring windows.
#define WA_RING 36
__device__ __forceinline__ int ring_index(int kr, int kc) {      // kr or kc in {0, 9}
  return (kr == 0) ? kc : ((kr == 9) ? 10 + kc : ((kc == 0) ? 19 + kr : 27 + kr));
}
// destination row (element offset of its dK|dV part) of key (kr,kc) of window (b,wy,wx); false: phantom key outside
// the image whose dK|dV is dropped (the gradient of zero padding) -- only possible for ring keys
template <typename T>
__device__ __forceinline__ T* dkv_row(T* gqkv, T* win, long long wi, int b, int wy, int wx, int h, int w, int C, int key) {
  const int kr = key / 10, kc = key - kr * 10;
  if (kr >= 1 && kr <= 8 && kc >= 1 && kc <= 8)
    return gqkv + (((long long)b * h + 8 * wy + kr - 1) * w + 8 * wx + kc - 1) * (3 * C) + C;
  return win + (wi * WA_RING + ring_index(kr, kc)) * (2 * C);
}

// The (<= 3) neighbouring windows whose 10x10 neighbourhood covers pixel (y, x) of image b, as element offsets of their
// ring rows in a [window][36][rw] scratch (same order as halo_gather_kernel adds them: row-neighbour column first).
__device__ __forceinline__ int halo_sources(int b, int y, int x, int nh, int nw, int rw, long long (&off)[3]) {
  // branch-free: the three candidates -- A = the column neighbour of the pixel's own window row, B = the row neighbour, C = the diagonal one --
  // are all computed (their indices are valid whether they exist or not) and packed by selects.  As two nested loops with data-dependent
  // trip counts this cost the attention backward's prep role 4.7 k cycles per workgroup (profiles/r06_attn_phase0_integer_work.txt)
  const int wy0 = y >> 3, wx0 = x >> 3, py = y & 7, px = x & 7;
  const bool up = py == 0 && wy0 > 0, dn = py == 7 && wy0 < nh - 1;
  const bool lf = px == 0 && wx0 > 0, rt = px == 7 && wx0 < nw - 1;
  const bool hasy = up || dn, hasx = lf || rt;
  const int wy1 = wy0 + (dn ? 1 : 0) - (up ? 1 : 0), kr1 = up ? 9 : 0;
  const int wx1 = wx0 + (rt ? 1 : 0) - (lf ? 1 : 0), kc1 = lf ? 9 : 0;
  const int kr0 = py + 1, kc0 = px + 1;
  const int row0 = (b * nh + wy0) * nw, row1 = (b * nh + wy1) * nw;          // window counts stay far below 2^31 / 36
  const int eA = (row0 + wx1) * WA_RING + ((kc1 == 0) ? 19 + kr0 : 27 + kr0); // ring_index(kr0 in 1..8, kc1 in {0, 9})
  const int eB = (row1 + wx0) * WA_RING + ((kr1 == 0) ? kc0 : 10 + kc0);      // ring_index(kr1 in {0, 9}, kc0)
  const int eC = (row1 + wx1) * WA_RING + ((kr1 == 0) ? kc1 : 10 + kc1);
  off[0] = (long long)(hasx ? eA : eB) * rw;
  off[1] = (long long)eB * rw;                                               // (read only when both neighbours exist)
  off[2] = (long long)eC * rw;
  return (hasx ? 1 : 0) + (hasy ? 1 : 0) + ((hasx && hasy) ? 1 : 0);
}

// window `wi` (logical index) of an h x w map
__device__ __forceinline__ WinGeom make_geom(int h, int w, int wi) {
  WinGeom g;
  g.h = h; g.w = w; g.nw = w / 8; g.nh = h / 8;
  g.wi = wi;
  g.wx = wi % g.nw;
  const int q = wi / g.nw;
  g.wy = q % g.nh;
  g.b = q / g.nh;
  return g;
}
// the workgroup's own window (one workgroup per window)
__device__ __forceinline__ WinGeom make_geom(int h, int w) {
#ifdef M2T_WIN_HOT       // scratch/bench_*.hip knock-out (results WRONG): every workgroup works on one of M2T_WIN_HOT windows -- the kernel's
  const int wi = xcd_block_index() % (M2T_WIN_HOT);      // loads and stores hit L2, its HBM traffic all but disappears, its instruction stream stays
#else
  const int wi = xcd_block_index();
#endif
  return make_geom(h, w, wi);
}

// Key `key` (0..99) of the window as a 32-bit element offset of its pixel row in a [pixel][row_elems] tensor, relative to the first key
// row of the window (key_row0), clamped into the image (the loads are unconditional), and whether the key lies inside the image.
// 24-bit multiplies throughout, for the reason given at key_rc_fast.
struct KeyAddr { unsigned off; bool ok; int kr, kc; };
__device__ __forceinline__ int key_row0(const WinGeom& gm) { return max(8 * gm.wy - 1, 0); }
__device__ __forceinline__ KeyAddr key_addr(const WinGeom& gm, int h, int w, int key, int row_elems) {
  KeyAddr a;
  key_rc_fast(key, a.kr, a.kc);
  const int yy = 8 * gm.wy + a.kr - 1, xx = 8 * gm.wx + a.kc - 1;
  a.ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
  const unsigned pix = __umul24((unsigned)(clamp_px(yy, h) - key_row0(gm)), (unsigned)w) + (unsigned)clamp_px(xx, w);
  a.off = __umul24(pix, (unsigned)row_elems);
  return a;
}
