// ictr_own.h -- who releases what on the host side: move-only holders of device memory, pinned host memory and HIP events,
// and the run / wait state of an object that is run now and waited for later: with its result block and pinned mirror
// (Readback), or around a dense field that stays on the device (DenseResult).
// A holder owns; a raw pointer next to it borrows. An object that carves one block up itself (a pyramid's planes, the flow
// grid's arena) holds that block with ONE holder. Host only; included through ictr_launch.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

#include "../../include/ictr.h"

namespace ictr {

int fail(int code, const char *fmt, ...);  // ictr_launch.h
#define HIPCHK(expr)                                                                                  \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) return fail(ICTR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));   \
  } while (0)

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

// One array of a carved block, and the carving: take() rounds the end up to `align`, places `bytes` there and moves on. A
// result layout is ONE function that fills a struct of Parts; the kernel arguments and the copy-out both read that struct.
struct Part {
  size_t at = 0, bytes = 0;
};
struct Carve {
  size_t end = 0;
  Part take(size_t bytes, size_t align = 1) {
    const Part p{(end + align - 1) / align * align, bytes};
    end = p.at + bytes;
    return p;
  }
};

// The result block of an object that runs now and is waited for later: the device block its kernels write, the pinned
// mirror, the event behind the copy, and whether a run is in flight / was ever enqueued. Declare it LAST in its object:
// members go in reverse order, so the wait in this destructor comes before any buffer of a run in flight is released.
class Readback {
 public:
  ~Readback() {
    if (pending_) (void)hipEventSynchronize(done_.get());
  }
  // only grows, and releases both blocks before it allocates; the device block zero-filled on request
  int reserve(size_t bytes, bool zero) {
    if (int rc = done_ ? ICTR_OK : done_.create(hipEventDisableTiming)) return rc;
    if (bytes <= cap_) return ICTR_OK;
    cap_ = 0;
    dev_.reset();
    host_.reset();
    if (int rc = dev_.alloc(bytes, zero)) return rc;
    if (int rc = host_.alloc(bytes)) return rc;
    cap_ = bytes;
    return ICTR_OK;
  }
  char *dev() const { return dev_.get(); }
  char *host() const { return host_.get(); }
  bool pending() const { return pending_; }
  bool ran() const { return ran_; }
  int refuse(const char *what, const char *object) const {
    // the inputs of a run stay fixed until its wait
    return pending_ ? fail(ICTR_ERR_STATE, "%s: a run is in flight; call ictr_%s_wait first", what, object) : ICTR_OK;
  }
  // the tail of every run: the block's first `bytes` to the mirror, behind everything enqueued on s
  int post(size_t bytes, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(host_.get(), dev_.get(), bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(done_.get(), s));
    pending_ = ran_ = true;
    return ICTR_OK;
  }
  int wait() {  // the head of every wait (the caller has checked pending())
    HIPCHK(hipEventSynchronize(done_.get()));
    pending_ = false;
    return ICTR_OK;
  }

 private:
  DevBuf<char> dev_;
  PinBuf<char> host_;
  size_t cap_ = 0;
  Event done_;
  bool pending_ = false, ran_ = false;
};

// The dense field [h][w][2] f32 that a run fills on the caller's stream and a later call waits for (the flow refiner, the
// flow densifier). No Readback: there is no pinned mirror, the array is BORROWED from the object's arena. The holder owns
// the event behind the last run and whether one was ever enqueued. Declare it LAST in its object, as a Readback.
class DenseResult {
 public:
  ~DenseResult() { (void)settle(); }
  int bind(float *out, int w, int h) {
    out_ = out;
    bytes_ = sizeof(float) * 2 * (size_t)w * h;
    return done_.create(hipEventDisableTiming);
  }
  float *get() const { return out_; }
  // the tail of every run: behind everything enqueued on s
  int record(hipStream_t s) {
    HIPCHK(hipEventRecord(done_.get(), s));
    ran_ = true;
    return ICTR_OK;
  }
  // waits if a run was enqueued: before the host reads or overwrites what that run reads or writes
  int settle() {
    if (ran_) HIPCHK(hipEventSynchronize(done_.get()));
    return ICTR_OK;
  }
  // waits for the last run, or refuses when there was none
  int wait(const char *what) { return ran_ ? settle() : fail(ICTR_ERR_STATE, "%s: no run yet", what); }
  // wait(what), then the field to `out` in host or device memory
  int copy_out(const char *what, float *out, int on_device) {
    if (int rc = wait(what)) return rc;
    if (!out) return fail(ICTR_ERR_INVALID, "%s: out is NULL", what);
    HIPCHK(hipMemcpy(out, out_, bytes_, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return ICTR_OK;
  }

 private:
  float *out_ = nullptr;
  size_t bytes_ = 0;
  Event done_;
  bool ran_ = false;
};

}  // namespace ictr
