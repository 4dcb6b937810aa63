// process_setup.cpp -- rsi_hot_process_setup (include/rsi_hot.h): the one place that decides how many hardware queues the
// process asks the HIP runtime for.  Host code only and no HIP call: the runtime reads GPU_MAX_HW_QUEUES when it initialises,
// so this has to be able to run before anything touches the GPU.  rsicnv_amd/api.py applies the same policy at import
// (_process_setup there; tests/test_process_setup.py holds the two together).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "process_setup.h"
#include "../../include/rsi_hot.h"

namespace rsip {

int parse_queue_count(const char* s) {
  if (!s) return -1;
  const size_t len = strlen(s);
  if (len < 1 || len > 9) return -1;
  int v = 0;
  for (size_t i = 0; i < len; ++i) {
    if (s[i] < '0' || s[i] > '9') return -1;
    v = v * 10 + (s[i] - '0');
  }
  return v;
}

int env_hw_queues() { return std::max(0, parse_queue_count(getenv("GPU_MAX_HW_QUEUES"))); }

}  // namespace rsip

extern "C" int rsi_hot_process_setup(void) {
  using namespace rsip;
  const char* user = getenv("RSI_HOT_HW_QUEUES");
  if (user && strcmp(user, "keep") == 0) return env_hw_queues();
  int want = parse_queue_count(user);
  if (want >= 0) {
    want = std::min(kPoolHwQueues, std::max(kMinHwQueues, want));
  } else {
    if (parse_queue_count(getenv("GPU_MAX_HW_QUEUES")) >= kPoolHwQueues) return env_hw_queues();   // enough already: not ours to lower
    want = kPoolHwQueues;
  }
  char text[16];
  snprintf(text, sizeof text, "%d", want);
  setenv("GPU_MAX_HW_QUEUES", text, 1);
  return env_hw_queues();
}
