"""The host-pointer staging and the argument checks of the dense-solve entries (corrla_rs_amd/csrc/lu_staging.hpp and the
lu_solve_entry / rbf_fit_entry of capi_impl.hpp), pinned on the CPU: both are host code, compiled here into a stand-alone
program with its own main over a fake device -- heap blocks for alloc_bytes, memcpy for the copies, a counter for end_call.
The program is built twice, under AddressSanitizer + UBSan and plain, as tests/test_host_io.py is: a copy that leaves its
span fails the first build, and the test does not depend on the sanitizer runtime being installed.

Checked at offsets 0 and 8 from a 16-byte boundary: a solve leaves the host's A and B untouched, factors the staged copy of A,
starts X as a copy of B and writes back the n x n_rhs elements alone -- every gap of x and the elements behind its last keep
their sentinel; the coefficients of a fit likewise.  The device images sit at the host's offset with the host's row strides.
no_overlap rejects every pair of an output with an input or another output, and names both."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lu_staging.hpp"
using namespace corrla;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __func__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

struct FakeDev {
  static constexpr bool kHasLu = true;
  std::vector<void*> blocks;
  std::vector<size_t> asked;
  int ends = 0, d2d = 0;
  void* alloc_bytes(size_t bytes) {
    void* p = nullptr;
    if (posix_memalign(&p, 256, (bytes + 255) / 256 * 256 + 256) != 0) std::exit(3);
    std::memset(p, 0x5C, (bytes + 255) / 256 * 256);
    blocks.push_back(p);
    asked.push_back(bytes);
    return p;
  }
  void h2d_bytes(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); }
  static void copy_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    CHECK(rows == 1 || (dpitch >= width && spitch >= width));
    for (size_t r = 0; r < rows; ++r) std::memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
  }
  void h2d_2d_enqueue(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) { copy_2d(dst, dpitch, src, spitch, width, rows); }
  void d2h_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) { copy_2d(dst, dpitch, src, spitch, width, rows); }
  void d2d_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    ++d2d;
    copy_2d(dst, dpitch, src, spitch, width, rows);
  }
  void end_call() { ++ends; }
  bool owns(const void* p, size_t bytes) const {
    for (size_t i = 0; i < blocks.size(); ++i)
      if ((const char*)p >= (const char*)blocks[i] && (const char*)p + bytes <= (const char*)blocks[i] + asked[i]) return true;
    return false;
  }
  ~FakeDev() {
    for (void* p : blocks) std::free(p);
  }
};

constexpr double kSentinel = -7.25e300;

// rows x cols doubles, ld apart, the first `off` bytes behind a 16-byte boundary, `tail` elements behind the last; everything
// that is not an element of the matrix holds the sentinel
struct HostMat {
  std::vector<unsigned char> mem;
  double* p;
  int64_t rows, cols, ld;
  size_t count, tail;
  HostMat(int64_t r, int64_t c, int64_t ld_, size_t off, size_t tail_ = 6)
      : mem(((size_t)((r - 1) * ld_ + c) + tail_) * 8 + 32), rows(r), cols(c), ld(ld_), count((size_t)((r - 1) * ld_ + c)), tail(tail_) {
    p = (double*)(((uintptr_t)mem.data() + 15) / 16 * 16 + off);
    CHECK((uintptr_t)p % 16 == off);
    for (size_t e = 0; e < count + tail; ++e) p[e] = kSentinel;
  }
  void fill(double base) {
    for (int64_t i = 0; i < rows; ++i)
      for (int64_t j = 0; j < cols; ++j) p[i * ld + j] = base + 100.0 * i + j;
  }
  bool holds(double base, double add) const {  // the elements base + 100 i + j + add, every other slot the sentinel
    for (size_t e = 0; e < count + tail; ++e) {
      const int64_t i = (int64_t)e / ld, j = (int64_t)e % ld;
      const bool elem = e < count && i < rows && j < cols;
      if (p[e] != (elem ? base + 100.0 * i + j + add : kSentinel)) return false;
    }
    return true;
  }
};

void solve_case(size_t off, int64_t n, int64_t n_rhs, int64_t lda, int64_t ldb, int64_t ldx) {
  HostMat a(n, n, lda, off), b(n, n_rhs, ldb, off), x(n, n_rhs, ldx, off);
  a.fill(1.0), b.fill(5000.0);
  const LuSolveCall c{a.p, n, lda, b.p, n_rhs, ldb, x.p, ldx, nullptr, nullptr, nullptr};
  bool ran = false;
  FakeDev dev;
  lu_solve_entry<FakeDev>(dev, true, c, [&] { ran = true; });
  CHECK(ran);
  HostIo<FakeDev> io(dev, true);
  const lu_stage::SolveArrays on = lu_stage::stage_solve(dev, io, true, c);
  // staged copies at the host's offset, inside their blocks, never the host arrays
  CHECK(on.a != a.p && on.b != x.p && on.b != b.p && on.ldb == ldx && dev.d2d == 1);
  CHECK((uintptr_t)on.a % 16 == off && (uintptr_t)on.b % 16 == off);
  CHECK(dev.owns(on.a, ((size_t)(n - 1) * lda + n) * 8) && dev.owns(on.b, ((size_t)(n - 1) * ldx + n_rhs) * 8));
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < n; ++j) CHECK(on.a[i * lda + j] == a.p[i * lda + j]);
    for (int64_t j = 0; j < n_rhs; ++j) CHECK(on.b[i * ldx + j] == b.p[i * ldb + j]);  // X starts as B
  }
  // what the kernels do: LU over the copy of A, X over the copy of B, junk in the gaps of the images
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < n; ++j) on.a[i * lda + j] = -1.0;
    for (int64_t j = 0; j < (i + 1 < n ? ldx : n_rhs); ++j) on.b[i * ldx + j] = j < n_rhs ? on.b[i * ldx + j] + 0.25 : 77.0;
  }
  CHECK(dev.ends == 0 && x.holds(0.0, 0.0) == false && x.p[0] == kSentinel);
  io.finish();
  CHECK(dev.ends == 1);
  CHECK(x.holds(5000.0, 0.25));                       // the elements, and a sentinel in every gap and behind the last
  CHECK(a.holds(1.0, 0.0) && b.holds(5000.0, 0.0));   // A and B untouched
  // the device entry: the caller's arrays, nothing staged
  FakeDev dev2;
  HostIo<FakeDev> io2(dev2, false);
  int64_t ipiv[8];
  const LuSolveCall d{a.p, n, lda, b.p, n_rhs, ldb, nullptr, 0, a.p, b.p, ipiv};
  const lu_stage::SolveArrays on2 = lu_stage::stage_solve(dev2, io2, false, d);
  CHECK(on2.a == a.p && on2.b == b.p && on2.ldb == ldb && dev2.blocks.empty() && dev2.d2d == 0);
  io2.finish();
  CHECK(dev2.ends == 0);
}

void fit_case(size_t off, int64_t n_s, int64_t dim, int64_t n_rhs, int degree, int64_t ldxs, int64_t ldy, int64_t ldw) {
  const int64_t n = n_s + rbf_poly_terms(dim, degree);
  HostMat xs(n_s, dim, ldxs, off), y(n_s, n_rhs, ldy, off), w(n, n_rhs, ldw, off);
  xs.fill(1.0), y.fill(3000.0);
  const RbfFitCall c{xs.p, n_s, ldxs, dim, y.p, n_rhs, ldy, 1, 0.0, degree, w.p, ldw, nullptr, 0};
  CHECK(c.order() == n);
  bool ran = false;
  FakeDev dev;
  rbf_fit_entry<FakeDev>(dev, c, true, [&] { ran = true; });
  CHECK(ran);
  HostIo<FakeDev> io(dev, true);
  const lu_stage::FitArrays on = lu_stage::stage_fit(io, c);
  CHECK(on.xs != xs.p && on.y != y.p && on.coeffs != w.p);
  CHECK((uintptr_t)on.xs % 16 == off && (uintptr_t)on.y % 16 == off && (uintptr_t)on.coeffs % 16 == off);
  CHECK(dev.owns(on.coeffs, ((size_t)(n - 1) * ldw + n_rhs) * 8));
  for (int64_t i = 0; i < n_s; ++i) {
    for (int64_t j = 0; j < dim; ++j) CHECK(on.xs[i * ldxs + j] == xs.p[i * ldxs + j]);
    for (int64_t j = 0; j < n_rhs; ++j) CHECK(on.y[i * ldy + j] == y.p[i * ldy + j]);
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < (i + 1 < n ? ldw : n_rhs); ++j) on.coeffs[i * ldw + j] = j < n_rhs ? 9000.0 + 100.0 * i + j : 77.0;
  io.finish();
  CHECK(dev.ends == 1 && w.holds(9000.0, 0.0) && xs.holds(1.0, 0.0) && y.holds(3000.0, 0.0));
}

template <class F>
void rejected(F&& f, const char* text) {
  bool ran = false;
  try {
    f(ran);
  } catch (const Error& e) {
    CHECK(!ran && e.code == ST_EINVAL);
    if (std::string(e.what()).find(text) == std::string::npos) {
      std::printf("FAILED: '%s' does not carry '%s'\n", e.what(), text);
      std::exit(1);
    }
    return;
  }
  std::printf("FAILED: no rejection carrying '%s'\n", text);
  std::exit(1);
}

void overlap_cases() {
  FakeDev dev;
  std::vector<double> buf(4096, 0.0);
  double *p0 = buf.data(), *p1 = p0 + 1000, *p2 = p0 + 2000;
  int64_t* ip = (int64_t*)(p0 + 3000);
  const int64_t n = 5, r = 3;
  auto solve_host = [&](const double* a, const double* b, double* x) {
    return [=, &dev](bool& ran) { lu_solve_entry<FakeDev>(dev, true, LuSolveCall{a, n, n, b, r, r, x, r, nullptr, nullptr, nullptr}, [&] { ran = true; }); };
  };
  rejected(solve_host(p0, p1, p0 + 24), "lu_solve: x overlaps a");   // the last element of a
  rejected(solve_host(p0, p1, p1 + 14), "lu_solve: x overlaps b");   // the last element of b
  rejected(solve_host(p0 + 14, p1, p0), "lu_solve: x overlaps a");   // the last element of x
  bool ran = false;
  solve_host(p0, p0 + 25, p0 + 40)(ran);                             // back to back: no overlap
  CHECK(ran);
  auto solve_dev = [&](double* a, double* b, int64_t* ipiv) {
    return [=, &dev](bool& ran_) { lu_solve_entry<FakeDev>(dev, false, LuSolveCall{a, n, n, b, r, r, nullptr, 0, a, b, ipiv}, [&] { ran_ = true; }); };
  };
  rejected(solve_dev(p0, p0 + 24, ip), "lu_solve: a overlaps b");
  rejected(solve_dev(p0, p1, (int64_t*)(p0 + 24)), "lu_solve: a overlaps ipiv");
  rejected(solve_dev(p0, p1, (int64_t*)(p1 + 14)), "lu_solve: b overlaps ipiv");
  rejected(solve_dev(p0, p1, (int64_t*)(p1 - 4)), "lu_solve: b overlaps ipiv");  // the last element of ipiv
  ran = false;
  solve_dev(p0, p1, nullptr)(ran);                                   // ipiv is optional
  CHECK(ran);
  const int64_t n_s = 6, dim = 2;  // degree 1: N = 9
  auto fit = [&](const double* xs, const double* y, double* w) {
    return [=, &dev](bool& ran_) { rbf_fit_entry<FakeDev>(dev, RbfFitCall{xs, n_s, dim, dim, y, r, r, 1, 0.0, 1, w, r, nullptr, 0}, true, [&] { ran_ = true; }); };
  };
  rejected(fit(p0, p1, p0 + 11), "rbf_fit: coeffs overlaps xs");
  rejected(fit(p0, p1, p1 + 17), "rbf_fit: coeffs overlaps y");
  rejected(fit(p0, p1 + 26, p1), "rbf_fit: coeffs overlaps y");      // the tail rows of the coefficients count: 9 x 3
  ran = false;
  fit(p0, p1 + 27, p1)(ran);
  CHECK(ran);
  auto sys = [&](const double* xs, double* m) {
    return [=, &dev](bool& ran_) { rbf_fit_entry<FakeDev>(dev, RbfFitCall{xs, n_s, dim, dim, nullptr, 0, 0, 1, 0.0, 1, nullptr, 0, m, 9}, false, [&] { ran_ = true; }); };
  };
  rejected(sys(p0, p0 + 11), "rbf_system: m overlaps xs");
  rejected(sys(p0 + 80, p0), "rbf_system: m overlaps xs");           // the last element of the 9 x 9 system
  ran = false;
  sys(p0 + 81, p0)(ran);
  CHECK(ran);
  // the limits are the plan's, and name their argument
  rejected([&](bool& ran_) { lu_solve_entry<FakeDev>(dev, true, LuSolveCall{p0, 0, 1, p1, r, r, p2, r, nullptr, nullptr, nullptr}, [&] { ran_ = true; }); },
           "lu: n must be >= 1");
  rejected([&](bool& ran_) { lu_solve_entry<FakeDev>(dev, true, LuSolveCall{p0, n, n - 1, p1, r, r, p2, r, nullptr, nullptr, nullptr}, [&] { ran_ = true; }); },
           "lu_solve: lda < n");
}

// a backend without the kernels ends the call after the argument checks
struct BareDev {};
void guard_case() {
  BareDev dev;
  double a[4] = {1, 2, 3, 4}, b[2] = {1, 1}, x[2];
  rejected([&](bool& ran) { lu_solve_entry<BareDev>(dev, true, LuSolveCall{a, 2, 2, b, 1, 1, x, 1, nullptr, nullptr, nullptr}, [&] { ran = true; }); },
           "this backend has no LU kernels");
  rejected([&](bool& ran) { rbf_fit_entry<BareDev>(dev, RbfFitCall{a, 2, 2, 2, b, 1, 1, 1, 0.0, -1, x, 1, nullptr, 0}, true, [&] { ran = true; }); },
           "this backend has no LU kernels");
}

int main() {
  for (size_t off : {(size_t)0, (size_t)8}) {
    solve_case(off, 5, 3, 5, 3, 3);    // dense
    solve_case(off, 5, 3, 7, 4, 6);    // gaps in all three
    solve_case(off, 1, 1, 1, 1, 1);
    solve_case(off, 4, 1, 4, 2, 3);    // a column of X with a stride
    fit_case(off, 6, 2, 3, 1, 2, 3, 3);
    fit_case(off, 6, 2, 3, 2, 5, 4, 7);
    fit_case(off, 4, 1, 1, -1, 1, 1, 2);
  }
  overlap_cases();
  guard_case();
  std::printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def src(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lu_host")
    path = tmp / "lu_host_driver.cpp"
    path.write_text(DRIVER)
    return tmp, path


@pytest.mark.parametrize("flags", [("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"), ()], ids=["asan_ubsan", "plain"])
def test_staging_and_overlap_checks(src, flags):
    tmp, path = src
    exe = tmp / ("driver_" + ("san" if flags else "plain"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           str(path), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr
