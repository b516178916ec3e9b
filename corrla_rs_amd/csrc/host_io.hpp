// The copies around a stage whose entry takes host pointers or device pointers (cov, the fitted PCA model, RBF, polynomial
// surfaces, KDE, the gradient stage).  The stage asks for every array of the call through one of the operations below
// and calls finish() at its end.  Device-pointer call: every operation returns the caller's pointer, nothing is allocated,
// and finish() does nothing -- the call enqueues and returns without end_call (end_call is the synchronise).  Host-pointer
// call: the inputs go to workspace of the call's arena, the outputs are built there, and finish() copies them back in the
// order they were asked for and ends the call.
// Which operation an array takes is part of the stage's behaviour: kernels branch on 16-byte alignment, so an array that is
// staged "as it lies" takes, from a host pointer, the route a device pointer of the same layout takes.
// Dev provides alloc_bytes, h2d_bytes (complete when it returns), h2d_2d_enqueue and d2h_2d (enqueue only: pageable host memory
// is read before the call returns to the stage, and every host-pointer call ends with end_call) and end_call.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "call_spans.hpp"

namespace corrla {

template <class Dev>
class HostIo {
 public:
  HostIo(Dev& dev, bool host_ptrs) : dev_(dev), host_(host_ptrs) {}

  // input as it lies: the whole span, at the offset the host array has from a 16-byte boundary
  template <class T>
  const T* in_as_lies(const Span& s) {
    if (!staged(s)) return (const T*)s.p;
    T* d = (T*)room_like(s);
    dev_.h2d_bytes(d, s.p, s.bytes());
    return d;
  }
  // input at arena alignment: the whole span, without the offset
  template <class T>
  const T* in_aligned(const Span& s) {
    if (!staged(s)) return (const T*)s.p;
    T* d = (T*)dev_.alloc_bytes(s.bytes());
    dev_.h2d_bytes(d, s.p, s.bytes());
    return d;
  }
  // input packed: the rows x cols elements as a dense image; *ld: its row stride (the caller's in a device-pointer call).
  // Enqueued: the stage's next synchronising copy, or the end of the call, covers it.
  template <class T>
  const T* in_packed(const Span& s, int64_t* ld) {
    *ld = s.ld;
    if (!staged(s)) return (const T*)s.p;
    T* d = (T*)dev_.alloc_bytes((size_t)s.rows * (size_t)s.cols * s.esz);
    dev_.h2d_2d_enqueue(d, (size_t)s.cols * s.esz, s.p, (size_t)s.ld * s.esz, (size_t)s.cols * s.esz, (size_t)s.rows);
    *ld = s.cols;
    return d;
  }
  // output as it lies: workspace at the host's offset and row stride
  template <class T>
  T* out_as_lies(const Span& s) {
    if (!staged(s)) return (T*)s.p;
    T* d = (T*)room_like(s);
    copy_back(s, d, s.ld);
    return d;
  }
  // output packed: a dense rows x cols image; *ld (optional): its row stride (the caller's in a device-pointer call)
  template <class T>
  T* out_packed(const Span& s, int64_t* ld = nullptr) {
    if (ld) *ld = staged(s) ? s.cols : s.ld;
    if (!staged(s)) return (T*)s.p;
    T* d = (T*)dev_.alloc_bytes((size_t)s.rows * (size_t)s.cols * s.esz);
    copy_back(s, d, s.cols);
    return d;
  }
  // output from a dense rows x cols image the stage already has on the device.  Host-pointer call: the image is what
  // finish() copies back, nothing is allocated, null is returned.  Device-pointer call: the caller's pointer, for the stage's
  // own device-to-device copy.
  template <class T>
  T* out_from(const Span& s, const T* image) {
    if (!staged(s)) return (T*)s.p;
    copy_back(s, image, s.cols);
    return nullptr;
  }
  // Host-pointer call: the rows x cols elements of every output to the host at the host's pitch -- the elements between them
  // are never written -- then end_call.  Device-pointer call: enqueued on the context's stream, the workspace is reused by
  // later calls in stream order.
  void finish() {
    enqueue_back();
    if (host_) dev_.end_call();
  }
  // the copies of finish() alone, for a stage that ends the call itself (grad_stage: its event behind them, then end_call
  // in both kinds of call)
  void enqueue_back() {
    for (const Back& b : back_) dev_.d2h_2d(b.host, b.host_pitch, b.dev, b.dev_pitch, b.width, b.rows);
    back_.clear();
  }

 private:
  struct Back {
    void* host;
    size_t host_pitch;
    const void* dev;
    size_t dev_pitch, width, rows;  // bytes, bytes, rows
  };
  bool staged(const Span& s) const { return host_ && s.p; }
  // One row has no pitch: a row stride below the width (legal for one row) never reaches a 2-D copy.  A contiguous vector
  // given as a column (KDE with inco = 1) is one row too.  A matrix stays a 2-D copy even where its rows touch.
  void copy_back(const Span& s, const void* d, int64_t dev_ld) {
    const size_t width = (size_t)s.cols * s.esz;
    if (s.rows == 1)
      back_.push_back({(void*)s.p, width, d, width, width, 1});
    else if (s.cols == 1 && s.ld == 1 && dev_ld == 1)
      back_.push_back({(void*)s.p, width * (size_t)s.rows, d, width * (size_t)s.rows, width * (size_t)s.rows, 1});
    else
      back_.push_back({(void*)s.p, (size_t)s.ld * s.esz, d, (size_t)dev_ld * s.esz, width, (size_t)s.rows});
  }
  void* room_like(const Span& s) { return (char*)dev_.alloc_bytes(s.bytes() + 16) + (uintptr_t)s.p % 16; }
  Dev& dev_;
  bool host_;
  std::vector<Back> back_;
};

}  // namespace corrla
