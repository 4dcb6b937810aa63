// process_setup.h -- the hardware-queue policy of process_setup.cpp, for the pool.  Plain C++ (no HIP).
#pragma once

namespace rsip {

constexpr int kPoolHwQueues = 32;      // what a pool wants, and the most the library ever writes
constexpr int kMinHwQueues = 4;        // the least it writes: the runtime's own default
constexpr int kRuntimeHwQueues = 4;    // what the runtime uses when GPU_MAX_HW_QUEUES holds no number
constexpr int kQueuesNotWorkers = 2;   // queues the pool's workers do not get: the copy stream's and the host framework's own

// One to nine decimal digits and nothing else -> the number; anything else (NULL included) -> -1.
int parse_queue_count(const char* s);
// GPU_MAX_HW_QUEUES as the environment holds it now, or 0 when it holds no number.
int env_hw_queues();

}  // namespace rsip
