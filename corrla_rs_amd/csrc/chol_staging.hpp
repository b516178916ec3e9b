// Where the arrays of corrla_chol_factor_* live during a call (host code, no HIP include: tests/test_chol_host.py compiles it
// over a fake device).  corrla_chol_solve_* stages exactly as corrla_lu_solve_* does -- A factored in its staged copy, B copied
// into the image of X -- so it takes lu_stage::stage_solve (lu_staging.hpp) over the same call record, without an ipiv.
// Device-pointer factor: the caller's array, nothing is allocated.  Host-pointer factor: A is staged as it lies and copied into
// the image of L (the host's row stride and offset from a 16-byte boundary), which is factored in place; the host's A is never
// written.  finish_factor copies the n x n elements of L back -- the gaps of l keep what they held -- and clears the strict upper
// triangle on the host: the kernels never touch it, so the image still holds A's there.
#pragma once
#include <cstring>

#include "capi_impl.hpp"
#include "host_io.hpp"
#include "lu_staging.hpp"

namespace corrla {
namespace chol_stage {

struct FactorArrays {
  double* l;  // n x n, row stride ldl: its lower triangle becomes L
  int64_t ldl;
};

template <class Dev>
FactorArrays stage_factor(Dev& dev, HostIo<Dev>& io, bool host_ptrs, const CholFactorCall& c) {
  if (!host_ptrs) return FactorArrays{c.a_rw, c.lda};
  const double* a = io.template in_as_lies<double>(c.a_span());
  double* l = io.template out_as_lies<double>(c.l_span());
  dev.d2d_2d(l, (size_t)c.ldl * sizeof(double), a, (size_t)c.lda * sizeof(double), (size_t)c.n * sizeof(double), (size_t)c.n);
  return FactorArrays{l, c.ldl};
}

template <class Dev>
void finish_factor(HostIo<Dev>& io, bool host_ptrs, const CholFactorCall& c) {
  io.finish();
  if (!host_ptrs) return;
  for (int64_t i = 0; i + 1 < c.n; ++i) std::memset(c.l + i * c.ldl + i + 1, 0, (size_t)(c.n - 1 - i) * sizeof(double));
}

}  // namespace chol_stage
}  // namespace corrla
