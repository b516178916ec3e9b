// Where the arrays of corrla_lu_solve_* and corrla_rbffit_* live during a call (host code, no HIP include: tests/test_lu_host.py
// compiles it over a fake device).  Device-pointer call: the caller's arrays, nothing is allocated.  Host-pointer call: A is
// factored in its staged copy and B is copied into the image of X, so the host's A and B are never written; the coefficients
// of a fit are built in the image of the caller's array -- all of them as they lie (the same row strides, the same offset
// from a 16-byte boundary), so the kernels see the layout a device pointer of that shape would give them, and finish() copies
// back the n x n_rhs elements alone.  Dev provides what HostIo needs and d2d_2d (enqueue only).
#pragma once
#include "capi_impl.hpp"
#include "host_io.hpp"

namespace corrla {
namespace lu_stage {

struct SolveArrays {
  double* a;  // n x n, row stride lda: becomes LU
  double* b;  // n x n_rhs, row stride ldb: becomes X
  int64_t ldb;
};

template <class Dev>
SolveArrays stage_solve(Dev& dev, HostIo<Dev>& io, bool host_ptrs, const LuSolveCall& c) {
  if (!host_ptrs) return SolveArrays{c.a_rw, c.b_rw, c.ldb};
  double* a = const_cast<double*>(io.template in_as_lies<double>(c.a_span()));
  const double* b_in = io.template in_as_lies<double>(c.b_span());
  double* x = io.template out_as_lies<double>(c.x_span());
  dev.d2d_2d(x, (size_t)c.ldx * sizeof(double), b_in, (size_t)c.ldb * sizeof(double), (size_t)c.n_rhs * sizeof(double), (size_t)c.n);
  return SolveArrays{a, x, c.ldx};
}

struct FitArrays {
  const double* xs;
  const double* y;
  double* coeffs;  // row stride ldw in both kinds of call
};

template <class Dev>
FitArrays stage_fit(HostIo<Dev>& io, const RbfFitCall& c) {
  FitArrays f;
  f.xs = io.template in_as_lies<double>(c.xs_span());
  f.y = io.template in_as_lies<double>(c.y_span());
  f.coeffs = io.template out_as_lies<double>(c.coeffs_span());
  return f;
}

}  // namespace lu_stage
}  // namespace corrla
