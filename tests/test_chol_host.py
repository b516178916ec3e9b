"""The host-pointer staging and the argument checks of the Cholesky entries (corrla_rs_amd/csrc/chol_staging.hpp, the shared
lu_stage::stage_solve, and chol_factor_entry / chol_solve_entry of capi_impl.hpp), pinned on the CPU: all of it is host code,
compiled here into a stand-alone program with its own main over a fake device -- heap blocks for alloc_bytes, memcpy for the
copies, a counter for end_call.  The program is built twice, under AddressSanitizer + UBSan and plain, as tests/test_lu_host.py
is: a copy that leaves its span fails the first build, and the test does not depend on the sanitizer runtime being installed.

Checked at offsets 0 and 8 from a 16-byte boundary: a factor leaves the host's A untouched, factors a copy of it in the image of
l (the host's row stride and offset), writes back the n x n elements alone -- every gap of l and the elements behind its last
keep their sentinel -- and l's strict upper triangle comes back as exact zeros whatever A held there; a solve leaves A and B
untouched, starts X as a copy of B and writes back the n x n_rhs elements alone.  no_overlap rejects every pair of an output
with an input or another output, and names both; every other rejection names its argument."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "chol_staging.hpp"
using namespace corrla;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __func__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

struct FakeDev {
  static constexpr bool kHasChol = true;
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


void factor_case(size_t off, int64_t n, int64_t lda, int64_t ldl) {
  HostMat a(n, n, lda, off), l(n, n, ldl, off);
  a.fill(1.0);
  const CholFactorCall c{a.p, n, lda, l.p, ldl, nullptr};
  bool ran = false;
  FakeDev dev;
  chol_factor_entry<FakeDev>(dev, true, c, [&] { ran = true; });
  CHECK(ran);
  HostIo<FakeDev> io(dev, true);
  const chol_stage::FactorArrays on = chol_stage::stage_factor(dev, io, true, c);
  // the image of l at the host's offset and stride, inside its block, never a host array; it starts as a copy of A
  CHECK(on.l != a.p && on.l != l.p && on.ldl == ldl && dev.d2d == 1);
  CHECK((uintptr_t)on.l % 16 == off && dev.owns(on.l, ((size_t)(n - 1) * ldl + n) * 8));
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) CHECK(on.l[i * ldl + j] == a.p[i * lda + j]);
  // what the kernels do: L over the lower triangle of the image, the upper triangle as it was, junk in the gaps
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < (i + 1 < n ? ldl : n); ++j) on.l[i * ldl + j] = j <= i ? on.l[i * ldl + j] + 0.5 : (j < n ? on.l[i * ldl + j] : 77.0);
  CHECK(dev.ends == 0 && l.p[0] == kSentinel);
  chol_stage::finish_factor(io, true, c);
  CHECK(dev.ends == 1);
  for (size_t e = 0; e < l.count + l.tail; ++e) {  // L below and on the diagonal, exact zeros above, the sentinel everywhere else
    const int64_t i = (int64_t)e / ldl, j = (int64_t)e % ldl;
    const bool elem = e < l.count && i < n && j < n;
    const double want = !elem ? kSentinel : (j <= i ? 1.0 + 100.0 * i + j + 0.5 : 0.0);
    CHECK(l.p[e] == want && (want != 0.0 || !std::signbit(l.p[e])));
  }
  CHECK(a.holds(1.0, 0.0));  // A untouched
  // the device entry: the caller's array, nothing staged, nothing cleared
  FakeDev dev2;
  HostIo<FakeDev> io2(dev2, false);
  const CholFactorCall d{a.p, n, lda, nullptr, 0, a.p};
  const chol_stage::FactorArrays on2 = chol_stage::stage_factor(dev2, io2, false, d);
  CHECK(on2.l == a.p && on2.ldl == lda && dev2.blocks.empty() && dev2.d2d == 0);
  chol_stage::finish_factor(io2, false, d);
  CHECK(dev2.ends == 0 && a.holds(1.0, 0.0));
}

void solve_case(size_t off, int64_t n, int64_t n_rhs, int64_t lda, int64_t ldb, int64_t ldx) {
  HostMat a(n, n, lda, off), b(n, n_rhs, ldb, off), x(n, n_rhs, ldx, off);
  a.fill(1.0), b.fill(5000.0);
  const LuSolveCall c{a.p, n, lda, b.p, n_rhs, ldb, x.p, ldx, nullptr, nullptr, nullptr};
  bool ran = false;
  FakeDev dev;
  chol_solve_entry<FakeDev>(dev, true, c, [&] { ran = true; });
  CHECK(ran);
  HostIo<FakeDev> io(dev, true);
  const lu_stage::SolveArrays on = lu_stage::stage_solve(dev, io, true, c);
  CHECK(on.a != a.p && on.b != x.p && on.b != b.p && on.ldb == ldx && dev.d2d == 1);
  CHECK((uintptr_t)on.a % 16 == off && (uintptr_t)on.b % 16 == off);
  CHECK(dev.owns(on.a, ((size_t)(n - 1) * lda + n) * 8) && dev.owns(on.b, ((size_t)(n - 1) * ldx + n_rhs) * 8));
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < n; ++j) CHECK(on.a[i * lda + j] == a.p[i * lda + j]);
    for (int64_t j = 0; j < n_rhs; ++j) CHECK(on.b[i * ldx + j] == b.p[i * ldb + j]);  // X starts as B
  }
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j <= i; ++j) on.a[i * lda + j] = -1.0;
    for (int64_t j = 0; j < (i + 1 < n ? ldx : n_rhs); ++j) on.b[i * ldx + j] = j < n_rhs ? on.b[i * ldx + j] + 0.25 : 77.0;
  }
  CHECK(dev.ends == 0 && x.p[0] == kSentinel);
  io.finish();
  CHECK(dev.ends == 1);
  CHECK(x.holds(5000.0, 0.25));                       // the elements, and a sentinel in every gap and behind the last
  CHECK(a.holds(1.0, 0.0) && b.holds(5000.0, 0.0));   // A and B untouched
  FakeDev dev2;
  HostIo<FakeDev> io2(dev2, false);
  const LuSolveCall d{a.p, n, lda, b.p, n_rhs, ldb, nullptr, 0, a.p, b.p, nullptr};
  const lu_stage::SolveArrays on2 = lu_stage::stage_solve(dev2, io2, false, d);
  CHECK(on2.a == a.p && on2.b == b.p && on2.ldb == ldb && dev2.blocks.empty() && dev2.d2d == 0);
  io2.finish();
  CHECK(dev2.ends == 0);
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

void overlap_and_argument_cases() {
  FakeDev dev;
  std::vector<double> buf(4096, 0.0);
  double *p0 = buf.data(), *p1 = p0 + 1000, *p2 = p0 + 2000;
  const int64_t n = 5, r = 3;
  auto factor_host = [&](const double* a, int64_t n_, int64_t lda, double* l, int64_t ldl) {
    return [=, &dev](bool& ran) { chol_factor_entry<FakeDev>(dev, true, CholFactorCall{a, n_, lda, l, ldl, nullptr}, [&] { ran = true; }); };
  };
  rejected(factor_host(p0, n, n, p0 + 24, n), "chol_factor: l overlaps a");  // the last element of a
  rejected(factor_host(p0 + 24, n, n, p0, n), "chol_factor: l overlaps a");  // the last element of l
  rejected(factor_host(p0, n, n, p0, n), "chol_factor: l overlaps a");
  bool ran = false;
  factor_host(p0, n, n, p0 + 25, n)(ran);                                    // back to back: no overlap
  CHECK(ran);
  rejected(factor_host(nullptr, n, n, p1, n), "chol_factor: a is NULL");
  rejected(factor_host(p0, n, n, nullptr, n), "chol_factor: l is NULL");
  rejected(factor_host(p0, 0, n, p1, n), "chol: n must be >= 1");
  rejected(factor_host(p0, ((int64_t)1 << 17) + 1, (int64_t)1 << 18, p1, (int64_t)1 << 18), "chol: n must be <= 131072");
  rejected(factor_host(p0, n, n - 1, p1, n), "chol_factor: lda < n");
  rejected(factor_host(p0, n, n, p1, n - 1), "chol_factor: ldl < n");
  auto factor_dev = [&](double* a, int64_t n_, int64_t lda) {
    return [=, &dev](bool& ran_) { chol_factor_entry<FakeDev>(dev, false, CholFactorCall{a, n_, lda, nullptr, 0, a}, [&] { ran_ = true; }); };
  };
  rejected(factor_dev(nullptr, n, n), "chol_factor: a is NULL");
  rejected(factor_dev(p0, n, n - 1), "chol_factor: lda < n");
  ran = false;
  factor_dev(p0, n, n)(ran);
  CHECK(ran);
  auto solve_host = [&](const double* a, int64_t n_, int64_t lda, const double* b, int64_t r_, int64_t ldb, double* x, int64_t ldx) {
    return [=, &dev](bool& ran_) {
      chol_solve_entry<FakeDev>(dev, true, LuSolveCall{a, n_, lda, b, r_, ldb, x, ldx, nullptr, nullptr, nullptr}, [&] { ran_ = true; });
    };
  };
  rejected(solve_host(p0, n, n, p1, r, r, p0 + 24, r), "chol_solve: x overlaps a");   // the last element of a
  rejected(solve_host(p0, n, n, p1, r, r, p1 + 14, r), "chol_solve: x overlaps b");   // the last element of b
  rejected(solve_host(p0 + 14, n, n, p1, r, r, p0, r), "chol_solve: x overlaps a");   // the last element of x
  ran = false;
  solve_host(p0, n, n, p0 + 25, r, r, p0 + 40, r)(ran);                               // back to back: no overlap
  CHECK(ran);
  rejected(solve_host(nullptr, n, n, p1, r, r, p2, r), "chol_solve: a is NULL");
  rejected(solve_host(p0, n, n, nullptr, r, r, p2, r), "chol_solve: b is NULL");
  rejected(solve_host(p0, n, n, p1, r, r, nullptr, r), "chol_solve: x is NULL");
  rejected(solve_host(p0, 0, n, p1, r, r, p2, r), "chol: n must be >= 1");
  rejected(solve_host(p0, n, n, p1, 0, r, p2, r), "chol_solve: n_rhs must be >= 1");
  rejected(solve_host(p0, n, n, p1, ((int64_t)1 << 20) + 1, (int64_t)1 << 21, p2, (int64_t)1 << 21), "chol: n_rhs must be <= 1048576");
  rejected(solve_host(p0, n, n - 1, p1, r, r, p2, r), "chol_solve: lda < n");
  rejected(solve_host(p0, n, n, p1, r, r - 1, p2, r), "chol_solve: ldb < n_rhs");
  rejected(solve_host(p0, n, n, p1, r, r, p2, r - 1), "chol_solve: ldx < n_rhs");
  auto solve_dev = [&](double* a, double* b) {
    return [=, &dev](bool& ran_) { chol_solve_entry<FakeDev>(dev, false, LuSolveCall{a, n, n, b, r, r, nullptr, 0, a, b, nullptr}, [&] { ran_ = true; }); };
  };
  rejected(solve_dev(p0, p0 + 24), "chol_solve: a overlaps b");
  rejected(solve_dev(p0 + 14, p0), "chol_solve: a overlaps b");
  ran = false;
  solve_dev(p0, p0 + 25)(ran);
  CHECK(ran);
}

// a backend without the kernels ends the call after the argument checks
struct BareDev {};
void guard_case() {
  BareDev dev;
  double a[4] = {1, 2, 3, 4}, b[2] = {1, 1}, x[2], l[4];
  rejected([&](bool& ran) { chol_solve_entry<BareDev>(dev, true, LuSolveCall{a, 2, 2, b, 1, 1, x, 1, nullptr, nullptr, nullptr}, [&] { ran = true; }); },
           "this backend has no Cholesky kernels");
  rejected([&](bool& ran) { chol_factor_entry<BareDev>(dev, true, CholFactorCall{a, 2, 2, l, 2, nullptr}, [&] { ran = true; }); },
           "this backend has no Cholesky kernels");
}

int main() {
  for (size_t off : {(size_t)0, (size_t)8}) {
    factor_case(off, 5, 5, 5);     // dense
    factor_case(off, 5, 7, 6);     // gaps in both
    factor_case(off, 1, 1, 1);
    factor_case(off, 4, 4, 9);
    solve_case(off, 5, 3, 5, 3, 3);
    solve_case(off, 5, 3, 7, 4, 6);
    solve_case(off, 1, 1, 1, 1, 1);
    solve_case(off, 4, 1, 4, 2, 3);
  }
  overlap_and_argument_cases();
  guard_case();
  std::printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def src(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("chol_host")
    path = tmp / "chol_host_driver.cpp"
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
