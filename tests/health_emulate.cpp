// Host emulation of k_health.hip for tests/test_health_cpu.py: the per-lane text the device runs (csrc/m2t_health_tile.h: lane_chunk,
// lane_merge, chunk_slot, fold_slot) over the thread decomposition of the two kernels, restated here as loops.  A stand-alone program
// with its own main; built with clang (the header uses ext_vector_type and __bf16), also under ASan / UBSan: the row is a heap block
// of exactly its size behind `shift` elements, so a read past the row's end is an error there.
//   health_emulate in.bin out.bin
// in:  int32 dt (0 fp32, 1 bf16), int32 shift (elements the base is moved off its 64-byte alignment), int64 n; float x[n] (values
//      representable in the element type)
// out: double row[72]
#include "m2t_health_tile.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace health_tile;

template <typename T> static void run(long long n, int shift, const float* xin, double* out) {
  // malloc's block is 16-byte aligned and ends where the row ends; the row starts `shift` elements into it
  T* raw = (T*)malloc((size_t)(n + shift) * sizeof(T) + (n + shift == 0 ? 1 : 0));
  if (!raw || (reinterpret_cast<uintptr_t>(raw) & 15u)) exit(3);
  T* base = raw + shift;
  for (long long i = 0; i < n; ++i) base[i] = (T)xin[i];
  const int nchunks = (int)((n + CHUNK - 1) / CHUNK > 0 ? (n + CHUNK - 1) / CHUNK : 1);
  std::vector<double> parts((size_t)nchunks * SLOTS);
  std::vector<unsigned char> hist((size_t)BINS * LANES);
  std::vector<Lane> lanes(LANES);
  for (int c = 0; c < nchunks; ++c) {
    // health_stream_kernel: one workgroup = one chunk, thread = lane
    std::fill(hist.begin(), hist.end(), 0);
    for (int t = 0; t < LANES; ++t) {
      lane_clear(lanes[t]);
      lane_chunk<T>(base, n, c, t, lanes[t], hist.data() + lane_slot(t), LANES);
    }
    unsigned cnt[BINS];
    for (int b = 0; b < BINS; ++b) {
      unsigned s = 0;
      for (int t = 0; t < LANES; ++t) s += hist[(size_t)b * LANES + t];
      cnt[b] = s;
    }
    for (int s = LANES / 2; s >= 1; s >>= 1)
      for (int t = 0; t < s; ++t) lane_merge(lanes[t], lanes[t + s]);
    long long nc = n - (long long)c * CHUNK;
    nc = nc < 0 ? 0 : (nc > CHUNK ? CHUNK : nc);
    for (int t = 0; t < SLOTS; ++t) chunk_slot(lanes[0], cnt, nc, t, parts.data() + (size_t)c * SLOTS);
  }
  // health_finish_kernel: one thread per slot
  for (int t = 0; t < SLOTS; ++t) out[t] = fold_slot(parts.data(), nchunks, t);
  free(raw);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[2];
  int64_t n;
  if (fread(h, sizeof(int32_t), 2, f) != 2 || fread(&n, sizeof(int64_t), 1, f) != 1) return 2;
  const int dt = h[0], shift = h[1];
  if (n < 0 || shift < 0 || shift > 64 || (dt != 0 && dt != 1)) return 2;
  std::vector<float> x((size_t)n);
  if (n && fread(x.data(), sizeof(float), (size_t)n, f) != (size_t)n) return 2;
  fclose(f);
  double out[SLOTS];
  if (dt == 0) run<float>(n, shift, x.data(), out);
  else run<__bf16>(n, shift, x.data(), out);
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out, sizeof(double), SLOTS, f) != SLOTS) return 2;
  fclose(f);
  return 0;
}
