// adapter_sum_order_driver.cpp -- TEST INFRASTRUCTURE: lsm2d_srrg::HipContext (adapters/srrg/lsm2d_srrg_common.h) and its sum_order PARAM, compiled
// against the stand-in headers of tests/cpp/adapter_shim and linked with the real liblsm2d_hip.so.  Prints one JSON object
// (tests/test_gpu_sum_order_latency.py::test_adapter_hip_context_follows_its_sum_order_param):
//   * the context follows a change of the PARAM made after its first handle() (lsm2d_get_option reads it back), both ways;
//   * when applying the option fails, handle() throws and leaves no context behind: the next handle() creates a fresh one with the PARAM's order.
// The failure is injected here: this executable defines lsm2d_set_option, which the adapter's call binds to, and forwards to the library's unless told to fail.
#include <lsm2d_srrg_common.h>

#include <dlfcn.h>

#include <cstdio>

static bool g_fail_set_option = false;
extern "C" int lsm2d_set_option(lsm2d_context* ctx, const char* key, int64_t value) {
  using Fn = int (*)(lsm2d_context*, const char*, int64_t);
  static Fn real = (Fn) dlsym(RTLD_NEXT, "lsm2d_set_option");
  if (g_fail_set_option) {
    return LSM2D_BAD_ARGUMENT;
  }
  return real ? real(ctx, key, value) : LSM2D_BAD_ARGUMENT;
}

static int64_t sumOrder(lsm2d_context* ctx_) {
  int64_t v = -1;
  if (lsm2d_get_option(ctx_, "sum_order", &v) != LSM2D_SUCCESS) {
    return -2;
  }
  return v;
}

int main() {
  lsm2d_srrg::HipContext hc;
  lsm2d_context* c0 = hc.handle("driver");
  const int64_t first = sumOrder(c0);
  hc.param_sum_order.setValue(1);
  lsm2d_context* c1 = hc.handle("driver");
  const int64_t after_on = sumOrder(c1);
  hc.param_sum_order.setValue(0);
  lsm2d_context* c2 = hc.handle("driver");
  const int64_t after_off = sumOrder(c2);
  const int same_context = c0 == c1 && c1 == c2;
  // a failed apply: handle() throws, and the context it had is gone
  hc.param_sum_order.setValue(1);
  g_fail_set_option = true;
  int threw = 0;
  try {
    hc.handle("driver");
  } catch (const std::runtime_error&) {
    threw = 1;
  }
  g_fail_set_option = false;
  lsm2d_context* c3 = hc.handle("driver");
  const int64_t after_failure = sumOrder(c3);
  printf("{\"first\": %lld, \"after_on\": %lld, \"after_off\": %lld, \"same_context\": %d, \"threw\": %d, \"after_failure\": %lld}\n", (long long) first,
         (long long) after_on, (long long) after_off, same_context, threw, (long long) after_failure);
  return 0;
}
