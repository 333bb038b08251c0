// Host side of a persistent launch -- one whose workgroups wait for each other (handoff.h) -- shared by every kernel file that has
// one (persist.hip, persist_split.hip, train_persist*.hip) and by the hosts that plan and launch them (decode.hip, encoder.hip,
// train.hip): how many workgroups are resident at once, where the hand-off counters keep the launch's give-up word, and the order
// and the back-off of the decode path's launches within the process.
#pragma once
#include "common.h"
#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <tuple>

namespace casv {

// ---- residency ----
// Workgroups of `kernel` (256 threads, `lds` bytes of dynamic LDS) that one CU holds at once, as the runtime reports it for the
// code object that is actually loaded -- asked once per (device, kernel, LDS size) -- and never more than `cap`, the figure the
// kernel's launch bounds promise or its host plans for.  The query counts registers and LDS; a workgroup's static LDS is part of
// the kernel's own figure.  0 = the query failed: no persistent launch.  Above 48 KB a kernel has to be allowed its dynamic LDS
// before it can be asked about, as before it can be launched.  Ask for exactly the (kernel, LDS size) pair of the launch: a grid
// planned from another pair's figure may not be resident as a whole, and then waits for workgroups that never start.
inline int persist_blocks_per_cu(const void* kernel, size_t lds, int cap) {
    static std::mutex mu;
    static std::map<std::tuple<int, const void*, size_t>, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({dev, kernel, lds});
    if (it == cache.end()) {
        int n = 0;
        if (lds > 48 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) n = 0;
        else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, lds) != hipSuccess) n = 0;
        it = cache.emplace(std::make_tuple(dev, kernel, lds), std::max(n, 0)).first;
    }
    return std::min(it->second, cap);
}
template <class K> inline int persist_blocks_per_cu(K* kernel, size_t lds, int cap) {
    return persist_blocks_per_cu(reinterpret_cast<const void*>(kernel), lds, cap);
}

// ---- hand-off counters ----
// `n` counters of 32 words each (a counter has its 128-byte line to itself), then 32 words of padding, the first of which is the
// launch's give-up word (the kernels' abort_w, handoff.h).  Zeroed ahead of the launch.
inline size_t persist_counters_bytes(size_t n) { return (n * 32 + 32) * sizeof(unsigned); }
inline unsigned* persist_give_up_word(unsigned* counters, size_t counter_bytes) { return counters + counter_bytes / sizeof(unsigned) - 32; }

// ---- order and back-off of the decode path's launches (decode.hip, encoder.hip) ----
// These launches are serialised inside the process: two of them together can want more workgroup slots than the chip has, and
// workgroups that spin on peers which are not resident never make room for them.  (Across processes the bounded spins catch that
// case: the launch gives up and the caller falls back to the per-step kernels.)  On the host the mutex orders the ENQUEUEING of
// such launches (no call waits for its kernel inside it) ...
inline std::mutex g_persist_mutex;
// ... and on the DEVICE: a persistent launch of any handle starts behind the previous one of the process on the same device (an
// event wait on the launching handle's stream -- the host does not wait).  Call both with g_persist_mutex held.
inline hipEvent_t g_persist_event[64];
inline bool g_persist_event_made[64] = {false}, g_persist_event_set[64] = {false};
inline void persist_order_before(int device, hipStream_t stream) {
    if (device >= 0 && device < 64 && g_persist_event_set[device]) (void)hipStreamWaitEvent(stream, g_persist_event[device], 0);
}
inline void persist_order_after(int device, hipStream_t stream) {
    const int d = device;
    if (d < 0 || d >= 64) return;
    if (!g_persist_event_made[d]) {
        if (hipEventCreateWithFlags(&g_persist_event[d], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
        g_persist_event_made[d] = true;
    }
    if (hipEventRecord(g_persist_event[d], stream) == hipSuccess) g_persist_event_set[d] = true;
}
// A persistent launch that gave up waiting (its workgroups were not all resident: the GPU is shared with another process's
// persistent kernel, or partitioned) costs one bounded wait.  The handle then leaves the persistent path alone for a number
// of calls that doubles with every further give-up, instead of paying that wait on every call.
struct PersistBackoff { int skip = 0, penalty = 0; bool told = false; };
inline bool persist_backed_off(PersistBackoff& b) {
    if (b.skip > 0) { --b.skip; return true; }
    return false;
}
inline void persist_note_abort(PersistBackoff& b, const char* what) {
    b.penalty = std::min(b.penalty ? 2 * b.penalty : 16, 1 << 16);
    b.skip = b.penalty;
    if (!b.told) {
        fprintf(stderr, "cor_asv_ann_hip: persistent %s gave up waiting (GPU shared with another persistent kernel?); using the per-step kernels for the next %d calls\n", what, b.skip);
        b.told = true;
    }
}

}  // namespace casv
