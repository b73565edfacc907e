// dispatch.h -- per-process counters of which kernel family a call was served by (sprintz_mi355x_dispatch_counts, SPRINTZ_KF_*).
// Every kernel family is bit-exact with every other, so equal bytes cannot tell a test which one ran: the launch sites say it here.
// Host only: one relaxed add behind a launch that returned hipSuccess, nothing inside a kernel.  The counters live in api.hip.
#pragma once

#include "../../include/sprintz_mi355x.h"

#include <atomic>
#include <cstdint>

namespace sprintz {

extern std::atomic<uint64_t> g_dispatch_counts[SPRINTZ_KF_COUNT];

inline void dispatched(int family) { g_dispatch_counts[family].fetch_add(1, std::memory_order_relaxed); }

}  // namespace sprintz
