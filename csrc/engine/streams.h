// Stream ordering: the vocabulary for handing data from one HIP stream to
// another (the out-of-core layer's side-stream copies). The rules:
//  1. A stream that reads what another stream wrote waits for that stream
//     first: Event::record + wait_on, or order_after if nobody keeps the event.
//  2. A device block that is freed while another stream may still use it is
//     marked with use_on: the allocator keeps it until that stream has passed.
//  3. A pinned host block read by an asynchronous copy is held until that
//     copy's event has passed. This is the CALLER's job (a `hold` list next to
//     the copy's Event): hostarena blocks have no stream tracking.
// Host tensors and an Event never recorded are no-ops, so code shared with the
// CPU engine needs no branch. A null hipStream_t is no no-op: it is the
// device's default stream, the current one unless a guard says otherwise.
#pragma once
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPCachingAllocator.h>

#include <stdexcept>
#include <string>
#include <utility>

#include "kv.h"

namespace mrh {

// a hipEvent without timing, created by its first record(); errors throw
// std::runtime_error("<what>: <HIP error>")
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    std::swap(e_, o.e_);
    return *this;
  }
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  explicit operator bool() const { return e_ != nullptr; }  // recorded at least once

  void record(hipStream_t s, const char* what = "mrhip: event record failed") {
    if (!e_) check(hipEventCreateWithFlags(&e_, hipEventDisableTiming), what);
    check(hipEventRecord(e_, s), what);
  }
  // stream s waits for the work the last record() covered
  void wait_on(hipStream_t s, const char* what = "mrhip: stream wait failed") const {
    if (e_) check(hipStreamWaitEvent(s, e_, 0), what);
  }
  // the host waits for it
  void sync(const char* what = "mrhip: event wait failed") const {
    if (e_) check(hipEventSynchronize(e_), what);
  }
  // has that work finished? (hipErrorNotReady -> false, other errors throw)
  bool done(const char* what = "mrhip: device error") const {
    const hipError_t r = e_ ? hipEventQuery(e_) : hipSuccess;
    if (r != hipErrorNotReady) check(r, what);
    return r == hipSuccess;
  }

 private:
  static void check(hipError_t r, const char* what) {
    if (r != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(r));
  }
  hipEvent_t e_ = nullptr;
};

// `consumer` waits for everything queued on `producer` so far
inline void order_after(hipStream_t consumer, hipStream_t producer, const char* what = "mrhip: stream fence failed") {
  Event e;
  e.record(producer, what);
  e.wait_on(consumer, what);
}
inline void order_after(hipStream_t consumer) { order_after(consumer, at::hip::getCurrentHIPStream().stream()); }

// the device tensor / every device column of the KV is also used on stream s
inline void use_on(const at::Tensor& t, hipStream_t s) {
  if (t.defined() && t.is_cuda())
    c10::hip::HIPCachingAllocator::recordStream(t.storage().data_ptr(),
                                               c10::hip::getStreamFromExternal(s, t.device().index()));
}
inline void use_on(const KV& kv, hipStream_t s) {
  for (const at::Tensor* t : {&kv.kdata, &kv.vdata, &kv.koff, &kv.voff}) use_on(*t, s);
}

}  // namespace mrh
