"""The host-pointer staging of the C ABI (corrla_rs_amd/csrc/call_spans.hpp, host_io.hpp), pinned on the CPU: both headers are
host code, compiled here with the host compiler into a stand-alone program that instantiates HostIo over a fake device --
256-byte-aligned heap blocks for alloc_bytes, memcpy for the copies (logged), a counter for end_call.  The program runs every
case itself and names the first one that fails; it is built twice, under AddressSanitizer + UBSan and plain, so a copy that
leaves its span fails the first build and the test does not depend on the sanitizer runtime being installed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#include "host_io.hpp"
using namespace corrla;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __func__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

struct FakeDev {
  struct Copy {
    const void* dst;
    const void* src;
    size_t bytes;  // what the copy moved
    size_t dpitch = 0, spitch = 0, width = 0, rows = 0;  // of a 2-D copy, as asked for
  };
  std::vector<void*> blocks;
  std::vector<size_t> asked;  // the sizes alloc_bytes was asked for
  std::vector<Copy> h2d, d2h;
  int ends = 0;
  void* alloc_bytes(size_t bytes) {
    void* p = nullptr;
    if (posix_memalign(&p, 256, (bytes + 255) / 256 * 256 + 256) != 0) std::exit(3);
    blocks.push_back(p);
    asked.push_back(bytes);
    return p;
  }
  void h2d_bytes(void* dst, const void* src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    h2d.push_back({dst, src, bytes});
  }
  // a real 2-D copy rejects a pitch below the width, so this one does
  static void copy_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if (dpitch < width || spitch < width) {
      std::printf("FAILED: a 2-D copy with a pitch below its width\n");
      std::exit(1);
    }
    for (size_t r = 0; r < rows; ++r) std::memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
  }
  void h2d_2d_enqueue(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    copy_2d(dst, dpitch, src, spitch, width, rows);
    h2d.push_back({dst, src, width * rows, dpitch, spitch, width, rows});
  }
  void d2h_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    copy_2d(dst, dpitch, src, spitch, width, rows);
    d2h.push_back({dst, src, width * rows, dpitch, spitch, width, rows});
  }
  void end_call() { ++ends; }
  ~FakeDev() {
    for (void* p : blocks) std::free(p);
  }
};

constexpr unsigned char kSentinel = 0xA5;

// `count` elements of T whose first lies `off` bytes behind a 16-byte boundary, plus `tail` elements behind them
template <class T>
struct HostBuf {
  std::vector<unsigned char> mem;
  T* p;
  size_t count, tail;
  HostBuf(size_t count_, size_t off, size_t tail_ = 0) : mem((count_ + tail_) * sizeof(T) + 32, kSentinel), count(count_), tail(tail_) {
    uintptr_t a = ((uintptr_t)mem.data() + 15) / 16 * 16 + off;
    p = (T*)a;
    CHECK((uintptr_t)p % 16 == off);
  }
  bool sentinel_at(size_t elem) const {
    const unsigned char* b = (const unsigned char*)(p + elem);
    for (size_t i = 0; i < sizeof(T); ++i)
      if (b[i] != kSentinel) return false;
    return true;
  }
};

template <class T>
T value(int64_t i, int64_t j) { return (T)(1000 * (i + 1) + j + 0.5); }

// ---- input as it lies: the same offset mod 16, exactly bytes() copied, bytes() + 16 allocated ----
template <class T>
void in_as_lies_case(const Span& s, size_t off) {
  FakeDev dev;
  HostIo<FakeDev> io(dev, true);
  const T* d = io.in_as_lies<T>(s);
  CHECK(d != (const T*)s.p);
  CHECK((uintptr_t)d % 16 == off && (uintptr_t)s.p % 16 == off);
  CHECK(dev.asked.size() == 1 && dev.asked[0] == s.bytes() + 16);
  CHECK(dev.h2d.size() == 1 && dev.h2d[0].bytes == s.bytes() && dev.h2d[0].src == s.p && dev.h2d[0].dst == (const void*)d);
  CHECK((const char*)d >= (const char*)dev.blocks[0] && (const char*)d + s.bytes() <= (const char*)dev.blocks[0] + dev.asked[0]);
  CHECK(std::memcmp(d, s.p, s.bytes()) == 0);
  io.finish();
  CHECK(dev.d2h.empty() && dev.ends == 1);
}
template <class T>
void test_in_as_lies() {
  // (every offset for f64 too: a base 4 bytes off an 8-byte boundary is still a byte range to copy; nothing here reads it as T)
  for (size_t off = 0; off < 16; off += 4) {
    {  // row-strided: 5 rows of 3, 7 apart
      HostBuf<T> h((5 - 1) * 7 + 3, off);
      for (size_t b = 0; b < h.count * sizeof(T); ++b) ((unsigned char*)h.p)[b] = (unsigned char)(7 * b + 1);
      const Span s((const T*)h.p, 5, 3, 7, "x");
      CHECK(s.count == 31 && s.esz == sizeof(T) && s.bytes() == 31 * sizeof(T));
      in_as_lies_case<T>(s, off);
    }
    {  // the KDE form: 7 elements 3 apart
      HostBuf<T> h((7 - 1) * 3 + 1, off);
      const Span s((const T*)h.p, 7, 1, 3, "s");
      CHECK(s.count == 19);
      in_as_lies_case<T>(s, off);
    }
    {  // two strides: 4 x 3, element (i, j) at 2 i + 9 j
      HostBuf<T> h((4 - 1) * 2 + (3 - 1) * 9 + 1, off);
      const Span s((const T*)h.p, 4, 3, 2, 9, "x");
      CHECK(s.count == 25 && s.bytes() == 25 * sizeof(T));
      in_as_lies_case<T>(s, off);
    }
  }
}

// ---- the other two inputs ----
template <class T>
void test_in_aligned_and_packed() {
  HostBuf<T> h((4 - 1) * 6 + 2, sizeof(T));
  for (int64_t i = 0; i < 4; ++i)
    for (int64_t j = 0; j < 2; ++j) h.p[i * 6 + j] = value<T>(i, j);
  const Span s((const T*)h.p, 4, 2, 6, "scores");
  FakeDev dev;
  HostIo<FakeDev> io(dev, true);
  const T* a = io.in_aligned<T>(s);
  CHECK((uintptr_t)a % 256 == 0 && dev.asked.back() == s.bytes() && dev.h2d.back().bytes == s.bytes());
  CHECK(std::memcmp(a, h.p, s.bytes()) == 0);
  int64_t ld = -1;
  const T* d = io.in_packed<T>(s, &ld);
  CHECK(ld == 2 && (uintptr_t)d % 256 == 0 && dev.asked.back() == 4 * 2 * sizeof(T) && dev.h2d.back().bytes == 4 * 2 * sizeof(T));
  CHECK(dev.h2d.back().spitch == 6 * sizeof(T) && dev.h2d.back().dpitch == 2 * sizeof(T) && dev.h2d.back().rows == 4);
  for (int64_t i = 0; i < 4; ++i)
    for (int64_t j = 0; j < 2; ++j) CHECK(d[i * 2 + j] == value<T>(i, j));
  io.finish();
  CHECK(dev.d2h.empty() && dev.ends == 1);
}

// ---- outputs: after finish() the rows x cols elements carry the device image, every other byte the sentinel ----
template <class T>
void check_host_image(const HostBuf<T>& h, int64_t rows, int64_t cols, int64_t ld) {
  for (size_t e = 0; e < h.count + h.tail; ++e) {
    const int64_t i = (int64_t)e / ld, j = (int64_t)e % ld;
    if (i < rows && j < cols)
      CHECK(h.p[e] == value<T>(i, j));
    else
      CHECK(h.sentinel_at(e));
  }
}
template <class T>
void out_as_lies_case(int64_t rows, int64_t cols, int64_t ld, size_t off) {
  HostBuf<T> h((size_t)((rows - 1) * ld + cols), off, /*tail=*/8);
  const Span s((const T*)h.p, rows, cols, ld, "out");
  FakeDev dev;
  HostIo<FakeDev> io(dev, true);
  T* d = io.out_as_lies<T>(s);
  CHECK((uintptr_t)d % 16 == off && dev.asked.size() == 1 && dev.asked[0] == s.bytes() + 16 && dev.h2d.empty());
  for (size_t e = 0; e < s.count; ++e) d[e] = (T)-1;  // what a kernel leaves in the gaps stays on the device
  for (int64_t i = 0; i < rows; ++i)
    for (int64_t j = 0; j < cols; ++j) d[i * ld + j] = value<T>(i, j);
  CHECK(dev.d2h.empty() && dev.ends == 0);
  io.finish();
  CHECK(dev.d2h.size() == 1 && dev.d2h[0].bytes == (size_t)(rows * cols) * sizeof(T) && dev.d2h[0].dst == (const void*)h.p && dev.ends == 1);
  check_host_image(h, rows, cols, ld);
}
template <class T>
void test_out_packed() {
  const int64_t rows = 5, cols = 3, ld = 7;
  HostBuf<T> h((size_t)((rows - 1) * ld + cols), 8, /*tail=*/8);
  HostBuf<T> v(4, 0, /*tail=*/2);  // a small vector behind it: the copies back run in the order the outputs were asked for
  FakeDev dev;
  HostIo<FakeDev> io(dev, true);
  int64_t ldd = -1;
  T* d = io.out_packed<T>(Span((const T*)h.p, rows, cols, ld, "c"), &ldd);
  T* dv = io.out_packed<T>(Span((const T*)v.p, 1, 4, 4, "means_out"));
  CHECK(ldd == cols && (uintptr_t)d % 256 == 0 && dev.asked.size() == 2 && dev.asked[0] == (size_t)(rows * cols) * sizeof(T) &&
        dev.asked[1] == 4 * sizeof(T) && dev.h2d.empty());
  for (int64_t i = 0; i < rows; ++i)
    for (int64_t j = 0; j < cols; ++j) d[i * cols + j] = value<T>(i, j);
  for (int64_t j = 0; j < 4; ++j) dv[j] = value<T>(0, j);
  io.finish();
  CHECK(dev.d2h.size() == 2 && dev.d2h[0].dst == (const void*)h.p && dev.d2h[1].dst == (const void*)v.p && dev.ends == 1);
  CHECK(dev.d2h[0].bytes == (size_t)(rows * cols) * sizeof(T) && dev.d2h[1].bytes == 4 * sizeof(T));
  check_host_image(h, rows, cols, ld);
  check_host_image(v, 1, 4, 4);
}

// one row whose stride is below its width (legal: pca_inverse with m = 1): the copy back is one row without a pitch
template <class T>
void test_one_row_below_its_width() {
  HostBuf<T> h(5, 0, /*tail=*/4);
  FakeDev dev;
  HostIo<FakeDev> io(dev, true);
  T* d = io.out_as_lies<T>(Span((const T*)h.p, 1, 5, 3, "out"));
  CHECK(dev.asked.size() == 1 && dev.asked[0] == 5 * sizeof(T) + 16);
  for (int64_t j = 0; j < 5; ++j) d[j] = value<T>(0, j);
  io.finish();
  CHECK(dev.d2h.size() == 1 && dev.d2h[0].rows == 1 && dev.d2h[0].width == 5 * sizeof(T));
  CHECK(dev.d2h[0].dpitch == dev.d2h[0].width && dev.d2h[0].spitch == dev.d2h[0].width && dev.ends == 1);
  check_host_image(h, 1, 5, 5);
}

// an output the stage already holds as a dense device image: copied back from there in a host-pointer call, nothing
// allocated; in a device-pointer call the caller's pointer comes back for the stage's own copy.  enqueue_back() is finish()
// without end_call.
void test_out_from_and_enqueue_back() {
  double image[4] = {value<double>(0, 0), value<double>(0, 1), value<double>(0, 2), value<double>(0, 3)};
  HostBuf<double> v(4, 0, /*tail=*/2);
  const Span s((const double*)v.p, 1, 4, 4, "means");
  {
    FakeDev dev;
    HostIo<FakeDev> io(dev, true);
    CHECK(io.out_from<double>(s, image) == nullptr && io.out_from<double>(Span(), image) == nullptr);
    CHECK(dev.asked.empty() && dev.d2h.empty());
    io.enqueue_back();
    CHECK(dev.d2h.size() == 1 && dev.d2h[0].src == (const void*)image && dev.d2h[0].dst == (const void*)v.p && dev.ends == 0);
    check_host_image(v, 1, 4, 4);
    io.finish();  // nothing left to copy
    CHECK(dev.d2h.size() == 1 && dev.ends == 1);
  }
  {
    FakeDev dev;
    HostIo<FakeDev> io(dev, false);
    CHECK(io.out_from<double>(s, image) == v.p && io.out_from<double>(Span(), image) == nullptr);
    io.enqueue_back();
    io.finish();
    CHECK(dev.asked.empty() && dev.d2h.empty() && dev.ends == 0);
  }
}

// ---- null spans: null in, null out, nothing allocated, nothing copied ----
void test_null_spans() {
  FakeDev dev;
  HostIo<FakeDev> io(dev, true);
  const Span none, null_rows((const double*)nullptr, 3, 2, 5, "jac");
  CHECK(none.bytes() == 0 && null_rows.bytes() == 0);
  for (const Span& s : {none, null_rows}) {
    int64_t ld = 0;
    CHECK(io.in_as_lies<double>(s) == nullptr && io.in_aligned<double>(s) == nullptr && io.in_packed<double>(s, &ld) == nullptr);
    CHECK(io.out_as_lies<double>(s) == nullptr && io.out_packed<double>(s) == nullptr && io.out_packed<double>(s, &ld) == nullptr);
  }
  io.finish();
  CHECK(dev.asked.empty() && dev.h2d.empty() && dev.d2h.empty() && dev.ends == 1);
}

// ---- device-pointer call: the caller's pointers and strides, and nothing else ----
void test_device_pointers() {
  FakeDev dev;
  HostIo<FakeDev> io(dev, false);
  HostBuf<float> h((5 - 1) * 7 + 3, 4);
  const Span s((const float*)h.p, 5, 3, 7, "x"), two((const float*)h.p, 4, 3, 2, 9, "x");
  int64_t ld = -1;
  CHECK(io.in_as_lies<float>(s) == h.p && io.in_as_lies<float>(two) == h.p && io.in_aligned<float>(s) == h.p);
  CHECK(io.in_packed<float>(s, &ld) == h.p && ld == 7);
  ld = -1;
  CHECK(io.out_as_lies<float>(s) == h.p && io.out_packed<float>(s) == h.p && io.out_packed<float>(s, &ld) == h.p && ld == 7);
  io.finish();
  CHECK(dev.asked.empty() && dev.h2d.empty() && dev.d2h.empty() && dev.ends == 0);
  for (size_t e = 0; e < h.count; ++e) CHECK(h.sentinel_at(e));
}

// ---- no_overlap ----
template <class F>
std::string thrown(F&& f) {
  try {
    f();
  } catch (const Error& e) {
    CHECK(e.code == ST_EINVAL);
    return e.what();
  }
  return "";
}
void test_no_overlap() {
  char bytes[32] = {};
  const Span a((const char*)bytes, 1, 10, 10, "a");
  {  // adjacent ranges pass, in either order
    const Span b((const char*)bytes + 10, 1, 6, 6, "b");
    CHECK(thrown([&] { no_overlap("who", &a, 1, &b, 1); }).empty() && thrown([&] { no_overlap("who", &b, 1, &a, 1); }).empty());
  }
  {  // one byte of overlap throws with both names, the output first
    const Span b((const char*)bytes + 9, 1, 6, 6, "b");
    CHECK(thrown([&] { no_overlap("who", &a, 1, &b, 1); }) == "who: b overlaps a");
    CHECK(thrown([&] { no_overlap("who", &b, 1, &a, 1); }) == "who: a overlaps b");
  }
  {  // every output against every later output; null spans are skipped wherever they stand
    const Span outs[3] = {Span((const char*)bytes + 12, 1, 4, 4, "c"), Span(), Span((const char*)bytes + 15, 1, 4, 4, "d")};
    const Span ins[2] = {Span((const char*)nullptr, 1, 32, 32, "n"), a};
    CHECK(thrown([&] { no_overlap("who", ins, 2, outs, 3); }) == "who: c overlaps d");
    CHECK(thrown([&] { no_overlap("who", ins, 2, outs, 2); }).empty());
  }
  {  // a strided span counts to its last element: 9 elements 3 apart end at element 24
    double buf[40] = {};
    const Span x((const double*)buf, 9, 1, 3, "x");
    const Span behind((const double*)buf + 25, 9, 1, 1, "out"), on((const double*)buf + 24, 9, 1, 1, "out");
    CHECK(thrown([&] { no_overlap("kde_eval", &x, 1, &behind, 1); }).empty());
    CHECK(thrown([&] { no_overlap("kde_eval", &x, 1, &on, 1); }) == "kde_eval: out overlaps x");
  }
}

// ---- the backend guard ----
void test_backend_guard() {
  bool ran = false;
  on_backend_with<std::true_type>([&] { ran = true; }, "symmetric rank-k kernel", "corrla_cov_*");
  CHECK(ran);
  ran = false;
  const std::string msg = thrown([&] { on_backend_with<std::false_type>([&] { ran = true; }, "symmetric rank-k kernel", "corrla_cov_*"); });
  CHECK(!ran && msg == "this backend has no symmetric rank-k kernel: corrla_cov_* is not supported");
}

int main() {
  test_in_as_lies<float>();
  test_in_as_lies<double>();
  test_in_aligned_and_packed<float>();
  test_in_aligned_and_packed<double>();
  for (size_t off = 0; off < 16; off += 4) {
    out_as_lies_case<float>(5, 3, 7, off);
    out_as_lies_case<float>(7, 1, 3, off);  // the KDE form
    out_as_lies_case<double>(5, 3, 7, off & 8);
    out_as_lies_case<double>(7, 1, 3, off & 8);
  }
  test_out_packed<float>();
  test_out_packed<double>();
  test_one_row_below_its_width<float>();
  test_one_row_below_its_width<double>();
  test_out_from_and_enqueue_back();
  test_null_spans();
  test_device_pointers();
  test_no_overlap();
  test_backend_guard();
  std::printf("ok\n");
  return 0;
}
"""

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(tmp, name, extra):
    src = os.path.join(tmp, "host_io_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC, src, "-o", exe]
    return exe, subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout


def test_every_case_passes_without_the_sanitizers(tmp_path):
    exe, built = _build(str(tmp_path), "host_io_plain", [])
    assert built.returncode == 0, built.stdout
    _run(exe)


def _sanitizers_link(tmp):
    """an empty program links against the sanitizer runtimes: asked before the driver is built, so that an error in the driver
    is never read as a missing runtime"""
    src = os.path.join(tmp, "empty.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    return subprocess.run(["g++", *SANITIZE, src, "-o", os.path.join(tmp, "empty")], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT).returncode == 0


def test_every_case_passes_under_asan_and_ubsan(tmp_path):
    if not _sanitizers_link(str(tmp_path)):
        pytest.skip("the sanitizer runtimes are not installed: only the plain build ran")
    exe, built = _build(str(tmp_path), "host_io_san", SANITIZE)
    assert built.returncode == 0, built.stdout
    _run(exe)
