// Workspace layout of the C ABI (include/obb_hip.h: "size from the matching query, 256-byte aligned, refused before any device
// call").  Every entry that takes (ws, ws_bytes) has ONE layout function over a WsCursor; its *_workspace_bytes query runs it
// on a NULL base, the entry on `ws`, so a size and its pointers cannot drift apart.  Host only: nothing of HIP in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace obb {

constexpr size_t kWsAlign = 256;
static inline size_t align_up(size_t v, size_t a = kWsAlign) { return (v + a - 1) / a * a; }

// the refusal rule: a workspace is there, 256-byte aligned and at least as large as the layout
static inline bool ws_ok(const void* ws, size_t ws_bytes, size_t need) { return ws && !((uintptr_t)ws & (kWsAlign - 1)) && ws_bytes >= need; }

// Hands out consecutive 256-byte-aligned blocks of a workspace.  base == NULL is a sizing pass: every pointer is NULL (no
// arithmetic on the null base), total() is what a placing pass of the same takes needs.  An empty take is still one block.
class WsCursor {
  char* base_;
  size_t off_ = 0;
  void* at(size_t bytes) { void* p = base_ ? base_ + off_ : nullptr; off_ += align_up(bytes); return p; }
 public:
  explicit WsCursor(void* base) : base_(static_cast<char*>(base)) {}
  void* bytes(size_t n) { return at(n ? n : 1); }
  template <class T> T* take(size_t count) { return static_cast<T*>(bytes(count * sizeof(T))); }
  // a nested layout: lay(base) lays out from `base` (NULL on a sizing pass) and returns the bytes it used
  template <class F> void nest(F&& lay) { void* here = at(0); at(lay(here)); }
  size_t total() const { return off_; }
};

}  // namespace obb
