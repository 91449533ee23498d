// owned.h -- the one owner of one resource: a device buffer, a page-locked buffer, a stream, an event.  Move-only; the resource is
// released exactly once -- by the destructor, by reset() or when another owner is moved in.  Nothing else: no allocator, no counting,
// no size.  What a kernel or a device-visible struct gets is get(): a raw view that does not outlive the owner.
// Compiles without HIP (tests/host/owned_main.cpp instantiates it with a counting release function).
#pragma once

namespace rcsh {

template <class T, auto Release>
class Owned {
 public:
  Owned() = default;
  explicit Owned(T r) : r_(r) {}
  Owned(Owned&& o) noexcept : r_(o.release()) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }

  T get() const { return r_; }
  explicit operator bool() const { return r_ != T{}; }
  // hands the resource out: the caller owns it now
  T release() {
    T r = r_;
    r_ = T{};
    return r;
  }
  void reset(T r = T{}) {
    if (r_ != T{}) Release(r_);
    r_ = r;
  }
  // for the creating call's out-parameter, hipMalloc(buf.out(), bytes): releases what was held; stays empty if the call fails
  T* out() {
    reset();
    return &r_;
  }

 private:
  T r_{};
};

#ifdef __HIPCC__
template <class T> using DevBuf = Owned<T*, hipFree>;      // hipMalloc, hipExtMallocWithFlags
template <class T> using PinBuf = Owned<T*, hipHostFree>;  // hipHostMalloc
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
#endif

}  // namespace rcsh
