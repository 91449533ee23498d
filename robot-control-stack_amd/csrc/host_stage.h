// Layout of one host-pointer call over a device buffer that grows on demand (rcs_hip.hip: d_query, d_image; staged_call is the
// device part).  A host form declares each of its arrays once -- pointer, element type, count, direction -- and gets a ticket back;
// the slices lie in declaration order, each on an 8-byte boundary (hipMalloc's base alignment does the rest), and do not overlap.  An
// absent array (null pointer, or no elements) takes no room and has a null device view.  No HIP in here: a host compiler builds it alone.
#pragma once
#include <cassert>
#include <cstddef>

namespace rcsh {
// the ticket of one declared array; staged_call turns it into a typed device pointer once the buffer has grown
template <class T> struct StageRef { int slot; };

struct StageLayout {
  static constexpr int kMaxSlices = 16;
  struct Slice {
    size_t at, bytes;  // bytes == 0: absent
    const void* src;   // an input's host source, uploaded
    void* dst;         // an output's host destination, downloaded (null: not asked for)
    const void* from;  // non-null: the download comes from this device array outside the staging; the slice takes no room
  };
  Slice slice[kMaxSlices] = {};
  int count = 0;
  size_t total = 0;  // known before anything is allocated

  template <class T> StageRef<const T> in(const T* host, size_t n) { return {take(host ? sizeof(T) * n : 0, host, nullptr)}; }
  template <class T> StageRef<T> out(T* host, size_t n) { return {take(host ? sizeof(T) * n : 0, nullptr, host)}; }
  // an output the kernel is handed whatever the caller asked for: staged even when `host` is null, downloaded only when it is not
  template <class T> StageRef<T> out_always(T* host, size_t n) { return {take(sizeof(T) * n, nullptr, host)}; }
  // an output that lies elsewhere on the device already (the guard's records): downloaded with the others, nothing staged, no view
  template <class T> void out_from(T* host, const T* dev, size_t n) { take(host ? sizeof(T) * n : 0, nullptr, host, dev); }
  // a slice as a typed pointer into the allocation at `base`, null for an absent array (in the library only staged_call has a base)
  template <class T> T* view(void* base, StageRef<T> r) const {
    const Slice& e = slice[r.slot];
    return e.bytes && !e.from ? reinterpret_cast<T*>(static_cast<char*>(base) + e.at) : nullptr;
  }

 private:
  int take(size_t bytes, const void* src, void* dst, const void* from = nullptr) {
    assert(count < kMaxSlices);
    slice[count] = bytes ? Slice{total, bytes, src, dst, from} : Slice{total, 0, nullptr, nullptr, nullptr};
    if (!from) total += (bytes + 7) & ~(size_t)7;
    return count++;
  }
};
}  // namespace rcsh
