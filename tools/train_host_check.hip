// train_host_check.hip -- a stand-alone host program around the launchers of k_train.hip, for a sanitizer run of their HOST code (the
// argument checks and the packing of the meter's pointer table into the kernel's argument block) on a machine without a device:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/train_host_check.hip m2trans_amd/csrc/k_train.hip -o train_host_check
//   ./train_host_check
//
// It links none of the library: the three error hooks the launchers call are defined here.  The host arrays are heap blocks of
// exactly n_cols entries, so a launcher that reads one entry too many is caught.  Without a device the launches of the valid calls
// fail with a HIP error, which the launchers must return, not crash on; with one they run and 0 comes back.  Exit status 0 = every
// expectation held.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/m2t_train.h"

static char g_last[256];
int m2t_set_error_at(int code, const char* who, const char* what) {
  snprintf(g_last, sizeof g_last, "%s: %s", who, what);
  return code;
}
int m2t_set_error(int code, const char* msg) {
  snprintf(g_last, sizeof g_last, "%s", msg);
  return code;
}
int m2t_set_hip_error(hipError_t e, const char* file, int line) {
  snprintf(g_last, sizeof g_last, "%s:%d: %s", file, line, hipGetErrorString(e));
  return (int)e;
}

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ++failures;                                                           \
      fprintf(stderr, "line %d: expectation failed: %s (last error: %s)\n", __LINE__, #cond, g_last); \
    }                                                                       \
  } while (0)

int main() {
  int devices = 0;
  const bool have_device = hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
  (void)hipGetLastError();
  double* record = nullptr;
  float *ring = nullptr, *img = nullptr;
  unsigned char* dst = nullptr;
  float* scalar = nullptr;
  if (have_device) {
    EXPECT(hipMalloc(&record, 16 * 8 * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc(&ring, 4 * 17 * sizeof(float)) == hipSuccess);
    EXPECT(hipMalloc(&img, 3 * 16 * 16 * sizeof(float)) == hipSuccess);
    EXPECT(hipMemset(img, 0, 3 * 16 * 16 * sizeof(float)) == hipSuccess);
    EXPECT(hipMalloc(&dst, 16 * 48 * 3) == hipSuccess);
    EXPECT(hipMalloc(&scalar, sizeof(float)) == hipSuccess);
    EXPECT(hipMemset(scalar, 0, sizeof(float)) == hipSuccess);
  } else {                                      // never dereferenced on the host: the checks come first, the launch fails
    record = reinterpret_cast<double*>(0x1000);
    ring = reinterpret_cast<float*>(0x2000);
    img = reinterpret_cast<float*>(0x3000);
    dst = reinterpret_cast<unsigned char*>(0x4000);
    scalar = reinterpret_cast<float*>(0x5000);
  }

  // ---- argument errors, decided before any launch
  EXPECT(m2t_meter_reset(nullptr, ring, 3, 4, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_meter_reset(record, nullptr, 3, 4, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_meter_reset(record, ring, 0, 4, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_meter_reset(record, ring, M2T_METER_MAX_COLS + 1, 4, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_meter_reset(record, ring, 3, 0, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_meter_reset(record, ring, 3, (1 << 24) + 1, nullptr) == M2T_ERR_ARG);
  for (int n = 1; n <= M2T_METER_MAX_COLS; ++n) {
    // heap blocks of exactly n entries: reading entry n is a heap-buffer-overflow
    std::vector<const void*> values(n, scalar);
    std::vector<int> kinds(n, 0);
    values[n / 2] = nullptr;                    // an absent column
    EXPECT(m2t_meter_update(nullptr, kinds.data(), n, record, ring, 4, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(m2t_meter_update(values.data(), nullptr, n, record, ring, 4, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(m2t_meter_update(values.data(), kinds.data(), n, nullptr, ring, 4, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(m2t_meter_update(values.data(), kinds.data(), n, record, nullptr, 4, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(m2t_meter_update(values.data(), kinds.data(), n, record, ring, 0, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(m2t_meter_update(values.data(), kinds.data(), n, record, ring, 4, -1, nullptr) == M2T_ERR_ARG);
    kinds[n - 1] = 2;
    EXPECT(m2t_meter_update(values.data(), kinds.data(), n, record, ring, 4, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(strstr(g_last, "m2t_meter_update") != nullptr);
    kinds[n - 1] = 1;
    // a valid call packs the table and launches: 0 with a device, the launch's HIP error without one
    const int rc = m2t_meter_update(values.data(), kinds.data(), n, record, ring, 4, (1LL << 40) + n, nullptr);
    EXPECT(have_device ? rc == 0 : (rc != 0 && rc != M2T_ERR_ARG));
  }
  {
    std::vector<const void*> values(M2T_METER_MAX_COLS, scalar);
    std::vector<int> kinds(M2T_METER_MAX_COLS, 0);
    EXPECT(m2t_meter_update(values.data(), kinds.data(), 0, record, ring, 4, 0, nullptr) == M2T_ERR_ARG);
    EXPECT(m2t_meter_update(values.data(), kinds.data(), M2T_METER_MAX_COLS + 1, record, ring, 4, 0, nullptr) == M2T_ERR_ARG);
  }
  const int scales[] = {-1, 0, 1, 5, 1 << 30};
  for (int s : scales) EXPECT(m2t_preview_strip(img, img, img, 4, 4, s, 1.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(nullptr, img, img, 4, 4, 2, 1.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 4, 4, 2, 1.0f, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 0, 4, 2, 1.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 4, -7, 2, 1.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 0x7fffffff, 4, 4, 1.0f, dst, nullptr) == M2T_ERR_ARG);     // h * scale would overflow an int
  EXPECT(m2t_preview_strip(img, img, img, 4, 4097, 4, 1.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 4, 4, 2, 0.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 4, 4, 2, -1.0f, dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 4, 4, 2, __builtin_nanf(""), dst, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_preview_strip(img, img, img, 4, 4, 2, __builtin_inff(), dst, nullptr) == M2T_ERR_ARG);
  EXPECT(strstr(g_last, "m2t_preview_strip") != nullptr);
  // ---- valid calls
  int rc = m2t_meter_reset(record, ring, M2T_METER_MAX_COLS, 4, nullptr);
  EXPECT(have_device ? rc == 0 : (rc != 0 && rc != M2T_ERR_ARG));
  rc = m2t_preview_strip(img, img, img, 4, 4, 4, 1.0f, dst, nullptr);
  EXPECT(have_device ? rc == 0 : (rc != 0 && rc != M2T_ERR_ARG));
  if (have_device) EXPECT(hipDeviceSynchronize() == hipSuccess);
  printf("train_host_check: %s (%s device), %d failed expectation(s)\n", failures ? "FAILED" : "ok", have_device ? "with a" : "no", failures);
  return failures ? 1 : 0;
}
