// m2t_prof.hip -- optional per-kernel timing with HIP events on the launch stream (m2t_profile_enable / m2t_profile_read /
// m2t_profile_sample_every of include/m2t.h; the launchers' side is M2TProfScope / M2T_LAUNCH_TIMED of m2t_kernels.h), and the
// armed fork event of m2t_backward's option "fork_on_kernel", which rides on a dispatch the same way.  Host code only.
// The enable mask and the event pool are process-wide (an atomic and a mutex-protected pool): the C ABI is entered from
// the caller's thread for m2t_forward and from the autograd engine's worker thread for m2t_backward (model(x);
// loss.backward()), and both must land in the same table.  Only the "a dispatch-timed scope is open" state is per thread.
#include <atomic>
#include <mutex>
#include <vector>
#include "m2t_kernels.h"
#include "../../include/m2t.h"

namespace {
struct ProfRec { hipEvent_t a, b; int cat; };
struct ProfState {
  std::atomic<unsigned long long> mask{0};
  std::atomic<int> every{1};              // dispatch-timed categories: events ride on one launch in `every` (m2t_profile_sample_every)
  std::mutex mu;
  std::vector<ProfRec> pool;
  size_t used = 0;
  long long seen[64] = {0};               // launches of each category since m2t_profile_enable (under mu)
};
ProfState g_prof;
struct ProfOpen { long long slot = -1; bool taken = false; };
thread_local ProfOpen g_open;             // the record of the scope this thread has open
long long prof_claim(int cat) {           // next free record, or -1 (mask off / not a sampled launch / pool exhausted)
  if (!((g_prof.mask.load(std::memory_order_relaxed) >> cat) & 1ull)) return -1;
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if ((M2T_PROF_DISPATCH_CATS >> cat) & 1ull) {
    // an event-carrying dispatch costs ~10 us of launch path (measured: 16 timed launches per step = +2.3 % on the step);
    // timing a uniform 1-in-N sample of a category's launches keeps the average and most of the step
    const int n = g_prof.every.load(std::memory_order_relaxed);
    if (n > 1 && (g_prof.seen[cat]++ % n) != 0) return -1;
  }
  if (g_prof.used >= g_prof.pool.size()) return -1;
  g_prof.pool[g_prof.used].cat = -1;      // becomes `cat` once both events are on a stream
  return (long long)g_prof.used++;
}
}
void m2t_prof_begin(int cat, hipStream_t st) {
  g_open.slot = prof_claim(cat);
  g_open.taken = false;
  if (g_open.slot < 0) return;
  if ((M2T_PROF_DISPATCH_CATS >> cat) & 1ull) return;           // the launcher takes the events (m2t_prof_take)
  (void)hipEventRecord(g_prof.pool[(size_t)g_open.slot].a, st);
}
thread_local hipEvent_t g_m2t_fork_armed = nullptr;      // armed by m2t_backward in front of the launch the fork follows
hipEvent_t m2t_fork_take() {
  if (!g_m2t_fork_armed || (g_open.slot >= 0 && !g_open.taken)) return nullptr;     // a timing pair goes first; the fork then falls back to a record
  hipEvent_t e = g_m2t_fork_armed;
  g_m2t_fork_armed = nullptr;
  return e;
}
bool m2t_prof_take(hipEvent_t* a, hipEvent_t* b) {
  if (g_open.slot < 0 || g_open.taken) return false;
  g_open.taken = true;
  *a = g_prof.pool[(size_t)g_open.slot].a; *b = g_prof.pool[(size_t)g_open.slot].b;
  return true;
}
void m2t_prof_end(int cat, hipStream_t st) {
  if (g_open.slot < 0) return;
  ProfRec& r = g_prof.pool[(size_t)g_open.slot];
  if ((M2T_PROF_DISPATCH_CATS >> cat) & 1ull) {
    if (g_open.taken) r.cat = cat;         // a scope whose launcher did not take the events stays unlabelled (dropped)
  } else {
    (void)hipEventRecord(r.b, st);
    r.cat = cat;
  }
  g_open.slot = -1;
  g_open.taken = false;
}
extern "C" int m2t_profile_enable(unsigned long long category_mask) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (category_mask && g_prof.pool.empty()) {
    g_prof.pool.resize(16384);
    for (auto& r : g_prof.pool) {
      // timing-only events: without the system-scope fence a default event carries, whose L2 write-back lengthens the
      // measured kernel and the one behind it (rocprofv3 of the same step: 46 vs 31 us for a sampled C = 256 attention backward
      // launch, 54 vs 44 us for its successor).  m2t_profile_read is only called after the streams were synchronised.
      if (hipEventCreateWithFlags(&r.a, hipEventDisableSystemFence) != hipSuccess ||
          hipEventCreateWithFlags(&r.b, hipEventDisableSystemFence) != hipSuccess)
        return m2t_set_error(M2T_ERR_STATE, "m2t_profile_enable: hipEventCreate failed");
      r.cat = -1;
    }
  }
  g_prof.mask.store(category_mask, std::memory_order_relaxed);
  g_prof.used = 0;
  for (auto& v : g_prof.seen) v = 0;
  return 0;
}
extern "C" int m2t_profile_sample_every(int n) {
  if (n < 1) return m2t_set_error(M2T_ERR_ARG, "m2t_profile_sample_every: n >= 1");
  g_prof.every.store(n, std::memory_order_relaxed);
  return 0;
}
// total milliseconds and launch count of one category since m2t_profile_enable, over every thread that launched; the
// caller must have synchronised the streams
extern "C" int m2t_profile_read(int cat, double* total_ms, long long* count) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  double t = 0.0; long long n = 0;
  for (size_t i = 0; i < g_prof.used; ++i) {
    if (g_prof.pool[i].cat != cat) continue;
    float ms = 0.f;
    hipError_t e = hipEventElapsedTime(&ms, g_prof.pool[i].a, g_prof.pool[i].b);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
    t += ms; ++n;
  }
  if (total_ms) *total_ms = t;
  if (count) *count = n;
  return 0;
}
