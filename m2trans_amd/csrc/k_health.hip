// k_health.hip -- the step health record (option "health" of include/m2t.h, which defines a row): per stored tensor the element
// count, non-finite and NaN counts, max / min |x|, fp64 sum and sum of squares, zeros and a 64-bin exponent histogram.  Two launches
// per phase (forward rows behind m2t_forward's last kernel, backward rows behind the join at the end of the backward pass); the
// per-lane text and the fold order are in m2t_health_tile.h.
//   stream  one workgroup per (row, chunk) of the phase's work list -> one 72-double partial per chunk ("ws:health_part")
//   finish  workgroup 0: the header row (pass counter, first row with a non-finite element); workgroup 1 + k: row k of the phase,
//           one thread per slot folding the row's chunks in ascending order -> "ws:health"
// The kernels read the tensors and write those two regions only.  No atomics: a lane counts into LDS bytes of its own.
#include "m2t_kernels.h"
#include "m2t_health_tile.h"

using namespace health_tile;

__global__ void __launch_bounds__(LANES) health_stream_kernel(const char* __restrict__ ws, const void* __restrict__ ext,
                                                              const m2t_health_desc* __restrict__ descs, const int* __restrict__ work,
                                                              double* __restrict__ parts, int item0) {
  __shared__ unsigned char hist[BINS * LANES];     // [bin][lane_slot(lane)]: one byte per lane and bin, private to the lane
  __shared__ Lane lanes[LANES];
  __shared__ unsigned cnt[BINS];
  const int t = threadIdx.x;
  const long long item = (long long)item0 + blockIdx.x;
  const int row = work[2 * item], chunk = work[2 * item + 1];
  const m2t_health_desc d = descs[row];
  const void* base = d.off >= 0 ? (const void*)(ws + d.off) : ext;
  const long long n = base ? d.n : 0;              // a pass without the caller's buffer (sr == NULL) records an empty row
  unsigned* h32 = reinterpret_cast<unsigned*>(hist);
#pragma unroll
  for (int i = 0; i < BINS * LANES / 4 / LANES; ++i) h32[i * LANES + t] = 0u;
  __syncthreads();
  Lane a;
  lane_clear(a);
  if (d.dtype == M2T_F32) lane_chunk<float>((const float*)base, n, chunk, t, a, hist + lane_slot(t), LANES);
  else lane_chunk<bf16_t>((const bf16_t*)base, n, chunk, t, a, hist + lane_slot(t), LANES);
  lanes[t] = a;
  __syncthreads();
  if (t < BINS) {                                  // bin t over the lanes
    unsigned s = 0;
    for (int i = 0; i < LANES / 4; ++i) {
      const unsigned w = h32[t * (LANES / 4) + i];
      s += (w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24);
    }
    cnt[t] = s;
  }
  for (int s = LANES / 2; s >= 1; s >>= 1) {
    if (t < s) lane_merge(lanes[t], lanes[t + s]);
    __syncthreads();
  }
  if (t < SLOTS) {
    const long long lo = (long long)chunk * CHUNK;
    long long nc = n - lo;
    nc = nc < 0 ? 0 : (nc > CHUNK ? CHUNK : nc);
    chunk_slot(lanes[0], cnt, nc, t, parts + (size_t)item * SLOTS);
  }
}

__global__ void __launch_bounds__(128) health_finish_kernel(const m2t_health_desc* __restrict__ descs, const int* __restrict__ work,
                                                            const double* __restrict__ parts, double* __restrict__ rec, int phase,
                                                            int row0, int item0, int nitems) {
  const int t = threadIdx.x;
  if (blockIdx.x > 0) {
    const int row = row0 + (int)blockIdx.x - 1;
    const m2t_health_desc d = descs[row];
    if (t < SLOTS) rec[(size_t)(1 + row) * SLOTS + t] = fold_slot(parts + (size_t)d.item0 * SLOTS, d.nitems, t);
    return;
  }
  // header: the first row of this phase, in row order, with a non-finite element (the work list is sorted by row)
  __shared__ int first[128];
  int f = 0x7fffffff;
  for (int i = t; i < nitems; i += 128)
    if (parts[(size_t)(item0 + i) * SLOTS + 1] > 0.0) { const int r = work[2 * (item0 + i)]; f = r < f ? r : f; }
  first[t] = f;
  __syncthreads();
  for (int s = 64; s >= 1; s >>= 1) {
    if (t < s) first[t] = first[t + s] < first[t] ? first[t + s] : first[t];
    __syncthreads();
  }
  if (t == 0) {
    rec[phase] = rec[phase] + 1.0;                 // passes recorded
    rec[2 + phase] = first[0] == 0x7fffffff ? -1.0 : (double)first[0];
  }
}

int launch_health_record(const void* ws, const void* ext, const m2t_health_desc* descs, const int* work, double* parts, double* rec,
                         int phase, int row0, int nrows, int item0, int nitems, hipStream_t st) {
  if (!ws || !descs || !work || !parts || !rec || nrows < 1 || nitems < 1) return m2t_set_error(-2, "health: bad argument");
  hipLaunchKernelGGL(health_stream_kernel, dim3((unsigned)nitems), dim3(LANES), 0, st, (const char*)ws, ext, descs, work, parts, item0);
  M2T_LAUNCH_CHECK();
  hipLaunchKernelGGL(health_finish_kernel, dim3((unsigned)(1 + nrows)), dim3(128), 0, st, descs, work, (const double*)parts, rec, phase, row0,
                     item0, nitems);
  M2T_LAUNCH_CHECK();
  return 0;
}
