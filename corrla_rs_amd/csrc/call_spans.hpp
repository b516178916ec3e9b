// What an entry of the C ABI knows about the caller's arrays before anything is staged: the span of each (first to last
// element, gaps included), the overlap check over those spans, and the guard in front of a stage the backend may not carry.
// Host code without a HIP include: compiled into the emulation backend as capi_impl.hpp is.  A call record (capi_impl.hpp)
// returns the spans of its arrays; its *_entry passes them to no_overlap and its stage passes the same spans to HostIo
// (host_io.hpp), so the range that is checked is the range that is copied.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "driver.hpp"  // Error

namespace corrla {

// One array of a call.  The two constructors are the only places where the extent of an array is computed; for a null pointer
// they compute none (an absent jac or dnll comes with dimensions nobody checked) and the span is empty.
struct Span {
  const void* p = nullptr;
  size_t count = 0;  // elements from the first to the last, gaps included
  size_t esz = 0;
  const char* name = "";
  int64_t rows = 0, cols = 0, ld = 0;  // the row-strided shape (the packed copies of HostIo)
  Span() = default;
  // rows x cols, the rows ld elements apart.  A vector of n elements `inc` apart is (n, 1, inc); r slabs of m rows are r * m rows.
  template <class T>
  Span(const T* p_, int64_t rows_, int64_t cols_, int64_t ld_, const char* name_)
      : p(p_), count(p_ ? (size_t)((rows_ - 1) * ld_ + cols_) : 0), esz(sizeof(T)), name(name_), rows(rows_), cols(cols_), ld(ld_) {}
  // the dense operand with two strides: m x n, element (i, j) at i * rs + j * cs.  Copied whole, as one row.
  template <class T>
  Span(const T* p_, int64_t m, int64_t n, int64_t rs, int64_t cs, const char* name_)
      : p(p_), count(p_ ? (size_t)((m - 1) * rs + (n - 1) * cs + 1) : 0), esz(sizeof(T)), name(name_), rows(1), cols((int64_t)count), ld((int64_t)count) {}
  size_t bytes() const { return count * esz; }
  bool overlaps(const Span& o) const {
    if (!p || !o.p) return false;
    const uintptr_t a0 = (uintptr_t)p, b0 = (uintptr_t)o.p;
    return a0 < b0 + o.bytes() && b0 < a0 + bytes();
  }
};

// every output against every input and every later output; null spans are skipped
inline void no_overlap(const char* who, const Span* in, int n_in, const Span* out, int n_out) {
  auto check = [&](const Span& o, const Span& other) {
    if (o.overlaps(other)) throw Error(ST_EINVAL, std::string(who) + ": " + o.name + " overlaps " + other.name);
  };
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i) check(out[o], in[i]);
    for (int q = o + 1; q < n_out; ++q) check(out[o], out[q]);
  }
}

// `run` on a backend that carries the kernels (Has: one of the dev_has_* traits of driver.hpp); any other backend ends the
// call with EINVAL, never with another way of computing the result.
template <class Has, class Run>
inline void on_backend_with(Run&& run, const char* kernels, const char* entries) {
  if constexpr (Has::value)
    run();
  else
    throw Error(ST_EINVAL, std::string("this backend has no ") + kernels + ": " + entries + " is not supported");
}

}  // namespace corrla
