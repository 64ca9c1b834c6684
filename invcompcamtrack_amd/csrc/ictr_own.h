// ictr_own.h -- who releases what on the host side: move-only holders of device memory, pinned host memory and HIP events.
// A holder owns; a raw pointer next to it borrows. An object that carves one block up itself (a pyramid's planes, the flow
// grid's arena) holds that block with ONE holder. Host only; included through ictr_launch.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

#include "../../include/ictr.h"

namespace ictr {

int fail(int code, const char *fmt, ...);  // ictr_launch.h

// `bytes` of device memory (hipMalloc / hipFree) or, Pinned, of page-locked host memory (hipHostMalloc / hipHostFree)
template <class T, bool Pinned>
class Block {
 public:
  Block() = default;
  Block(Block &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  Block &operator=(Block &&o) noexcept {
    if (this != &o) adopt(std::exchange(o.p_, nullptr));
    return *this;
  }
  ~Block() { reset(); }
  T *get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { adopt(nullptr); }
  // takes over memory that hipFree / hipHostFree releases (hipExtMallocWithFlags); what was held before is released
  void adopt(T *p) {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = p;
  }
  // Releases what is held, THEN allocates (a block that grows never holds old and new at once), zero-filled on request.
  // On failure the holder is empty and the ictr status is returned through fail().
  int alloc(size_t bytes, bool zero = false) {
    reset();
    hipError_t e = Pinned ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    if (e == hipSuccess && zero) e = hipMemset(p_, 0, bytes);
    if (e == hipSuccess) return ICTR_OK;
    reset();
    return fail(ICTR_ERR_HIP, "%s(%zu) failed: %s", Pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
  }

 private:
  T *p_ = nullptr;
};
template <class T>
using DevBuf = Block<T, false>;
template <class T>
using PinBuf = Block<T, true>;

// a HIP event, destroyed only if it was created
class Event {
 public:
  Event() = default;
  Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event &operator=(Event &&o) noexcept {
    std::swap(e_, o.e_);
    return *this;
  }
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  int create(unsigned flags = hipEventDefault) {
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    return e == hipSuccess ? ICTR_OK : fail(ICTR_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
  }
  hipEvent_t get() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace ictr
