// Where the arrays of corrla_eigh_* live during a call (host code, no HIP include: tests/test_eigh_host.py compiles it over a
// fake device).  Device-pointer call: the caller's arrays, nothing is staged -- a is only read, the working copy W lives in
// workspace.  Host-pointer call: a is staged as it lies (the host's row stride and offset from a 16-byte boundary) and never
// written; w is built as a dense vector and v in an image at the host's row stride and offset.  finish copies the n elements
// of w and the n x n elements of v back -- the gaps of v keep what they held -- and a call that ends early copies nothing.
#pragma once
#include "capi_impl.hpp"
#include "host_io.hpp"

namespace corrla {
namespace eigh_stage {

struct Arrays {
  const double* a;  // n x n, row stride lda: its lower triangle is read
  int64_t lda;
  double* w;        // n
  double* v;        // n x n, row stride ldv
  int64_t ldv;
};

template <class Dev>
Arrays stage(HostIo<Dev>& io, const EighCall& c) {
  Arrays on;
  on.a = io.template in_as_lies<double>(c.a_span());
  on.lda = c.lda;
  on.w = io.template out_packed<double>(c.w_span());
  on.v = io.template out_as_lies<double>(c.v_span());
  on.ldv = c.ldv;
  return on;
}

}  // namespace eigh_stage
}  // namespace corrla
