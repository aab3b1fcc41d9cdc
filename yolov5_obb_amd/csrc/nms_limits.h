// The limits that the NMS drivers' path decisions (nms_plan.h) share with the kernels they choose between.  Host only, nothing of
// HIP in here: each constant is defined once, here, and its owner (named beside it) includes this header.
#pragma once
#include <stdint.h>

#include "obb_hip.h"

namespace obb {

// ---- persistent kernel (nms_driver.h, nms_core.h)
// Chunk capacities: the first chunk has 2048 boxes, later chunks double up to 8192 for a single list, 2048 per segment for
// batches of up to 64 segments and 1024 beyond.  (The edge list of a team is sized for the worst case cap*(cap-1)/2 of one
// chunk: 134 MB at 8192, 8.4 MB at 2048, 2 MB at 1024 -- times the number of teams.)
constexpr int kCapFirst = 2048;     // clipped to cap_max in the kernel
static inline int cap_max(int64_t nseg) { return nseg == 1 ? 8192 : (nseg <= 64 ? 2048 : 1024); }
constexpr int64_t kGridMinN = 8192;    // below this the exhaustive cross phase is cheaper than building the index

// ---- phase kernels of a long single list (nms_mk.h)
constexpr int64_t kMkMinN = 16384;
constexpr int kMkMinKept = 256;    // below this many kept boxes (a handful of dense clusters: huge conflict lists per chunk) the phase kernels are not even tried
constexpr int kMkXRows = 3072;            // kept rows of a pass
constexpr int kMkPend1 = 1 << 21;         // pending-list capacity (pairs); an overflow hands the call to the persistent kernel

// ---- small-segment kernel (nms_small.h)
constexpr int kSmallMax = OBB_NMS_SMALL_SEG;        // boxes per segment (include/obb_hip.h)
constexpr int kSmallWords = kSmallMax / 64;         // bit-matrix words per row
constexpr int kSmallHelpMax = 256;

// ---- fused driver (nmsobb_impl.h, nmsobb_front.h, psrs_sort.h)
constexpr int64_t kSortLdsHint = OBB_NMS_SORT_LDS_HINT;   // use the in-LDS path when the previous call's largest image was at most this
constexpr int kPsMaxN = 131072;       // kPsRun * kPsMaxRuns (psrs_sort.h asserts it)
constexpr int kDecThreads = 512;      // 8 waves: a workgroup whose share of rows is three times the median still needs one pass

}  // namespace obb
