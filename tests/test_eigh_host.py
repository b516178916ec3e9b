"""The host-pointer staging and the argument checks of the eigensolver entries (corrla_rs_amd/csrc/eigh_staging.hpp and
eigh_entry of capi_impl.hpp), pinned on the CPU: all of it is host code, compiled here into a stand-alone program with its own
main over a fake device -- heap blocks for alloc_bytes, memcpy for the copies, a counter for end_call.  The program is built
twice, under AddressSanitizer + UBSan and plain, as tests/test_chol_host.py is: a copy that leaves its span fails the first
build, and the test does not depend on the sanitizer runtime being installed.

Checked at offsets 0 and 8 from a 16-byte boundary: a is staged as it lies (the host's row stride and offset) and never
written; w is built dense and v in an image at the host's row stride and offset; finish writes back the n elements of w and the
n x n elements of v alone -- every gap of v and the elements behind the last of either keep their sentinel -- and a call that
ends before finish writes nothing.  A device-pointer call stages nothing.  no_overlap rejects either output over the input
and v over w, and names both; every other rejection names its argument."""
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
#include "eigh_staging.hpp"
using namespace corrla;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __func__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

struct FakeDev {
  static constexpr bool kHasEigh = true;
  std::vector<void*> blocks;
  std::vector<size_t> asked;
  int ends = 0;
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
  bool holds(double base) const {  // the elements base + 100 i + j, every other slot the sentinel
    for (size_t e = 0; e < count + tail; ++e) {
      const int64_t i = (int64_t)e / ld, j = (int64_t)e % ld;
      const bool elem = e < count && i < rows && j < cols;
      if (p[e] != (elem ? base + 100.0 * i + j : kSentinel)) return false;
    }
    return true;
  }
  bool untouched() const {
    for (size_t e = 0; e < count + tail; ++e)
      if (p[e] != kSentinel) return false;
    return true;
  }
};

void eigh_case(size_t off, int64_t n, int64_t lda, int64_t ldv, bool fails) {
  HostMat a(n, n, lda, off), v(n, n, ldv, off), w(1, n, n, off);
  a.fill(1.0);
  const EighCall c{a.p, n, lda, w.p, v.p, ldv};
  bool ran = false;
  FakeDev dev;
  eigh_entry<FakeDev>(dev, c, [&] { ran = true; });
  CHECK(ran);
  {
    HostIo<FakeDev> io(dev, true);
    const eigh_stage::Arrays on = eigh_stage::stage(io, c);
    // a as it lies, inside its block, never the host array; the images of w and v are workspace too
    CHECK(on.a != a.p && on.lda == lda && (uintptr_t)on.a % 16 == off && dev.owns(on.a, ((size_t)(n - 1) * lda + n) * 8));
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < n; ++j) CHECK(on.a[i * lda + j] == a.p[i * lda + j]);
    CHECK(on.w != w.p && dev.owns(on.w, (size_t)n * 8));
    CHECK(on.v != v.p && on.ldv == ldv && (uintptr_t)on.v % 16 == off && dev.owns(on.v, ((size_t)(n - 1) * ldv + n) * 8));
    // what the kernels do: the elements, and junk in the gaps of the image of v
    for (int64_t j = 0; j < n; ++j) on.w[j] = 7.0 + j;
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < (i + 1 < n ? ldv : n); ++j) on.v[i * ldv + j] = j < n ? 3.0 + 100.0 * i + j : 77.0;
    CHECK(dev.ends == 0 && v.untouched() && w.untouched());
    if (!fails) {
      io.finish();
      CHECK(dev.ends == 1);
      CHECK(v.holds(3.0));  // the elements, and a sentinel in every gap and behind the last
      for (int64_t j = 0; j < n; ++j) CHECK(w.p[j] == 7.0 + j);
      for (size_t e = (size_t)n; e < w.count + w.tail; ++e) CHECK(w.p[e] == kSentinel);
    }
  }
  if (fails) CHECK(dev.ends == 0 && v.untouched() && w.untouched());  // a call that throws before finish copies nothing back
  CHECK(a.holds(1.0));                                                // a untouched
  // the device entry: the caller's arrays, nothing staged
  FakeDev dev2;
  HostIo<FakeDev> io2(dev2, false);
  const eigh_stage::Arrays on2 = eigh_stage::stage(io2, c);
  CHECK(on2.a == a.p && on2.w == w.p && on2.v == v.p && on2.lda == lda && on2.ldv == ldv && dev2.blocks.empty());
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
  const int64_t n = 5;
  auto call = [&](const double* a, int64_t n_, int64_t lda, double* w, double* v, int64_t ldv) {
    return [=, &dev](bool& ran) { eigh_entry<FakeDev>(dev, EighCall{a, n_, lda, w, v, ldv}, [&] { ran = true; }); };
  };
  rejected(call(p0, n, n, p1, p0 + 24, n), "eigh: v overlaps a");  // the last element of a
  rejected(call(p0 + 24, n, n, p1, p0, n), "eigh: v overlaps a");  // the last element of v
  rejected(call(p0, n, n, p0 + 24, p2, n), "eigh: w overlaps a");
  rejected(call(p0, n, n, p1, p1 + 4, n), "eigh: w overlaps v");   // the last element of w
  bool ran = false;
  call(p0, n, n, p0 + 25, p0 + 30, n)(ran);                         // back to back: no overlap
  CHECK(ran);
  rejected(call(nullptr, n, n, p1, p2, n), "eigh: a is NULL");
  rejected(call(p0, n, n, nullptr, p2, n), "eigh: w is NULL");
  rejected(call(p0, n, n, p1, nullptr, n), "eigh: v is NULL");
  rejected(call(p0, 0, n, p1, p2, n), "eigh: n must be >= 1");
  rejected(call(p0, 32769, 32769, p1, p2, 32769), "eigh: n must be <= 32768");
  rejected(call(p0, n, n - 1, p1, p2, n), "eigh: lda < n");
  rejected(call(p0, n, n, p1, p2, n - 1), "eigh: ldv < n");
}

// a backend without the kernels ends the call after the argument checks
struct BareDev {};
void guard_case() {
  BareDev dev;
  double a[4] = {1, 2, 2, 1}, w[2], v[4];
  rejected([&](bool& ran) { eigh_entry<BareDev>(dev, EighCall{a, 2, 2, w, v, 2}, [&] { ran = true; }); },
           "this backend has no symmetric eigensolver kernels");
}

int main() {
  for (size_t off : {(size_t)0, (size_t)8})
    for (bool fails : {false, true}) {
      eigh_case(off, 5, 5, 5, fails);  // dense
      eigh_case(off, 5, 7, 6, fails);  // gaps in both
      eigh_case(off, 1, 1, 1, fails);
      eigh_case(off, 4, 4, 9, fails);
    }
  overlap_and_argument_cases();
  guard_case();
  std::printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def src(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eigh_host")
    path = tmp / "eigh_host_driver.cpp"
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
