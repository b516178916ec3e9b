// HIP backend of the RSVD driver: one device, one stream, one cached workspace arena and
// (optionally) one RCCL communicator per context.  Implements the `Dev` interface that
// driver.hpp / capi_impl.hpp are written against.  Every operation is enqueued on the context's
// stream; the only host synchronisations are the small l x l downloads the host factorizations need.
// The compute stages are planned in their *_plan.hpp and launched from their *_stage.hpp, which define the members declared
// here (tall products: tall_stage.hpp, core SVD: core_svd_stage.hpp, thin-Q: thinq_stage.hpp, column passes:
// colstat_stage.hpp); this file keeps the device
// services -- memory, transfers, collectives, events -- the state of a context and the small elementwise launches.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "core_svd_plan.hpp"
#include "driver.hpp"
#include "hip_kernels.hpp"
#include "thinq_plan.hpp"
#include "jacobi_mc_kernels.hpp"
#include "ata_kernels.hpp"
#include "tall_kernels.hpp"
#include "mixed_kernels.hpp"
#include "bf16in_kernels.hpp"
#include "grad_kernels.hpp"
#include "knn2_kernels.hpp"
#include "grad_wide_kernels.hpp"
#include "spmm_kernels.hpp"
#include "syrk_kernels.hpp"
#include "pca_apply_kernels.hpp"
#include "rbf_kernels.hpp"
#include "polyfit_kernels.hpp"
#include "kde_kernels.hpp"
#include "dirichlet_kernels.hpp"
#include "mvn_kernels.hpp"

namespace corrla {

#define CORRLA_HIP(call)                                                                                       \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess)                                                                                      \
      throw Error(ST_EHIP, std::string(#call) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" +       \
                               std::to_string(__LINE__) + ")");                                                \
  } while (0)
#define CORRLA_NCCL(call)                                                                                      \
  do {                                                                                                         \
    ncclResult_t r_ = (call);                                                                                  \
    if (r_ != ncclSuccess) throw Error(ST_ECOMM, std::string(#call) + " failed: " + ncclGetErrorString(r_));   \
  } while (0)

inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v && *v ? std::atoi(v) : dflt;
}

template <class T>
struct NcclType;
template <>
struct NcclType<float> {
  static constexpr ncclDataType_t v = ncclFloat;
};
template <>
struct NcclType<double> {
  static constexpr ncclDataType_t v = ncclDouble;
};

// the instantiations of a kernel over its column tiles (or planes, waves, ...): with_nt calls
// f(std::integral_constant<int, n>) for one n in [N, MAX], with_one_of for one n of the listed values, for_each_nt for
// every n in [N, MAX], for_each_of for every listed value (a list named once, as a std::integer_sequence, serves both
// the launch and the LDS limits).  A value without an instantiation is an error, never another kernel.
template <int MAX, int N = 1, class F>
inline void with_nt(int n, const F& f) {
  if constexpr (N < MAX) {
    if (n > N) return with_nt<MAX, N + 1>(n, f);
  }
  if (n != N) throw Error(ST_EINVAL, "internal: no kernel instantiation for " + std::to_string(n));
  f(std::integral_constant<int, N>{});
}
template <int... Vs, class F>
inline void with_one_of(int n, const F& f) {
  if (!((n == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...))
    throw Error(ST_EINVAL, "internal: no kernel instantiation for " + std::to_string(n));
}
template <int... Vs, class F>
inline void with_one_of(std::integer_sequence<int, Vs...>, int n, const F& f) {
  with_one_of<Vs...>(n, f);
}
template <int MAX, int N = 1, class F>
inline void for_each_nt(const F& f) {
  f(std::integral_constant<int, N>{});
  if constexpr (N < MAX) for_each_nt<MAX, N + 1>(f);
}
template <int... Vs, class F>
inline void for_each_of(std::integer_sequence<int, Vs...>, const F& f) {
  (f(std::integral_constant<int, Vs>{}), ...);
}

// Every kernel launched with more dynamic LDS than the default gets its limit once per device: a function attribute
// applies to the device that is current when it is set (the HipDev constructor has made its own current).
inline void lds_limit(const void* fn, size_t bytes) {
  CORRLA_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}
namespace core_svd_stage {
template <class T>
void set_lds_limits();  // core_svd_stage.hpp: the core SVD's kernels
}
namespace tall_stage {
struct Call;            // tall_stage.hpp: what a launcher of the tall products needs of a context
template <class T>
void set_lds_limits();  // the tall products' kernels of element type T ...
inline void set_lds_limits();  // ... and the f32-only ones (bf16 split, bf16 stored, one-sweep)
}
namespace rbf_stage {
template <class T>
void set_lds_limits();  // rbf_stage.hpp: the radial-basis-function kernels
}
namespace polyfit_stage {
inline void set_lds_limits();  // polyfit_stage.hpp: the polynomial response-surface kernels
}
namespace thinq_stage {
template <class T>
void set_lds_limits();  // thinq_stage.hpp: the Householder panels
}
namespace mvn_stage {
template <class T>
void set_lds_limits();  // mvn_stage.hpp: the multivariate normal and sandwich kernels
}
namespace lu_stage {
inline void set_lds_limits();  // lu_stage.hpp: the LU kernels
}
namespace chol_stage {
inline void set_lds_limits();  // chol_stage.hpp: the Cholesky kernels
}
namespace eigh_stage {
inline void set_lds_limits();  // eigh_stage.hpp: the symmetric eigensolver's kernels
}

class HipDev {
 public:
  int device = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_size = 1;
  int n_collectives = 0;        // since begin_call
  double collective_bytes = 0;

  explicit HipDev(int dev_ordinal) : device(dev_ordinal) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
      throw Error(ST_ENODEV, "no HIP device visible (libcorrla_rsvd has no CPU fallback)");
    if (dev_ordinal < 0 || dev_ordinal >= count) throw Error(ST_EINVAL, "device ordinal out of range");
    CORRLA_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    CORRLA_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      throw Error(ST_ENODEV, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    num_cus = prop.multiProcessorCount;
    CORRLA_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CORRLA_HIP(hipMalloc(&zero_page_, 256));
    CORRLA_HIP(hipHostMalloc(&pinned_, kPinnedBytes, hipHostMallocDefault));
    for (auto& e : events_) CORRLA_HIP(hipEventCreate(&e));
    CORRLA_HIP(hipMemsetAsync(zero_page_, 0, 256, stream));
    set_lds_limits();
    {
      std::random_device rd;
      entropy_ = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    }
    // the thin-Q's knobs (thinq_plan.hpp)
    thinq_knobs_.host_chol = env_int("CORRLA_HOST_CHOL", 0) != 0;
    thinq_knobs_.robust_qr = env_int("CORRLA_DEVICE_ROBUST_QR", 1) != 0;  // 0: the round-1 optimistic CholeskyQR2 + host-controlled repeat
    if (const char* e = std::getenv("CORRLA_HH_BLOCK")) thinq_knobs_.hh_block = std::atoll(e);
    robust_passes_ = std::max(2, env_int("CORRLA_ROBUST_PASSES", 2));
    gemm_debug_flags_ = env_int("CORRLA_GEMM_DEBUG", 0);  // timing-only ablations, results are wrong
    // the tall products' geometry knobs (gemm_plan.hpp)
    gemm_knobs_.split_nn = env_int("CORRLA_SPLIT_NN", 0);
    gemm_knobs_.split_tn = env_int("CORRLA_SPLIT_TN", 0);
    gemm_knobs_.mw = env_int("CORRLA_MW", 0);
    gemm_knobs_.xcd_remap = env_int("CORRLA_GEMM_XCD", 1);
    gemm_knobs_.tall_min_rows = env_int("CORRLA_TALL_MIN_ROWS", 65536);  // 0: the general kernels everywhere
    gemm_knobs_.persist_max_tiles = env_int("CORRLA_GEMM_PERSIST_TILES", 16);  // 0: one workgroup per outer tile everywhere
    gemm_knobs_.f64_waves = env_int("CORRLA_F64_WAVES", 8);
    if (const char* e = std::getenv("CORRLA_MIXED_MIN_WORK")) gemm_knobs_.mixed_min_work = std::atof(e);
    gemm_knobs_.even_blocks = env_int("CORRLA_EVEN_BLOCKS", 0) != 0;
    gemm_knobs_.no_gram_alias = env_int("CORRLA_NO_GRAM_ALIAS", 0) != 0;
    gemm_knobs_.no_rotate = env_int("CORRLA_GEMM_NO_ROTATE", 0) != 0;
    gemm_knobs_.mixed_split = env_int("CORRLA_MIXED_SPLIT", 0);
    syrk_knobs_.slab_rows = env_int("CORRLA_SYRK_SLAB_ROWS", 0);  // syrk_plan.hpp
    poly_knobs_.slab_rows = env_int("CORRLA_POLYFIT_SLAB_ROWS", 0);  // polyfit_plan.hpp
  }
  ~HipDev() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (comm) (void)ncclCommDestroy(comm);
    for (auto& c : chunks_) (void)hipFree(c.p);
    for (auto& c : zchunks_) (void)hipFree(c.p);
    if (zero_page_) (void)hipFree(zero_page_);
    if (poly_table_) (void)hipFree(poly_table_);
    if (pinned_) (void)hipHostFree(pinned_);
    for (auto& e : events_)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_pool_) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
  HipDev(const HipDev&) = delete;
  HipDev& operator=(const HipDev&) = delete;

  int nranks() const { return comm_size; }

  // Seed of a call that names none: the reference draws every sketch from an unseeded thread_rng
  // (mat_utils.rs:161-175), so repeated calls must not share one Omega.  Per-context entropy (taken once, at
  // creation) mixed with a call counter; rank_invariant (row-sharded calls: every rank must draw the SAME Omega)
  // leaves the entropy out, so ranks that make the same sequence of calls agree.
  uint64_t fresh_seed(bool rank_invariant) {
    uint64_t z = (rank_invariant ? 0x5eedull : entropy_) + 0x9e3779b97f4a7c15ull * (uint64_t)(++(rank_invariant ? calls_sharded_ : calls_));
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;   // splitmix64 finaliser
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z ? z : 0x5eedull;
  }

  void comm_init(const void* id128, int rank, int nranks_) {
    CORRLA_HIP(hipSetDevice(device));
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) <= CORRLA_UNIQUE_ID_BYTES, "unique id size");
    std::memcpy(&id, id128, sizeof(id));
    if (comm) {
      (void)ncclCommDestroy(comm);
      comm = nullptr;
    }
    CORRLA_NCCL(ncclCommInitRank(&comm, nranks_, id, rank));
    comm_rank = rank;
    comm_size = nranks_;
  }
  // what RCCL itself reports for the communicator (not what the caller asked for)
  void comm_info(int* rank_out, int* nranks_out) {
    if (!comm) {
      *rank_out = 0;
      *nranks_out = 0;
      return;
    }
    CORRLA_NCCL(ncclCommUserRank(comm, rank_out));
    CORRLA_NCCL(ncclCommCount(comm, nranks_out));
  }

  // ---- memory ----------------------------------------------------------------------------
  void begin_call() {
    CORRLA_HIP(hipSetDevice(device));
    events_set_[0] = events_set_[1] = events_set_[2] = false;
    n_collectives = 0;
    collective_bytes = 0;
    marks_.clear();
    ev_used_ = 0;
    phase_mark(nullptr);  // start of the call
    for (auto& c : chunks_) c.used = 0;
    sp_scratch_ = nullptr;
    sp_scratch_bytes_ = 0;
    // zero pool: the part the previous call used is cleared by ONE memset per chunk (capped), instead of one
    // small memset per workspace allocation
    for (auto& c : zchunks_) {
      c.zeroed = std::min<size_t>(c.used, (size_t)256 << 20);
      c.used = 0;
      if (c.zeroed) CORRLA_HIP(hipMemsetAsync(c.p, 0, c.zeroed, stream));
    }
  }
  void end_call() { sync(); }
  void sync() { CORRLA_HIP(hipStreamSynchronize(stream)); }

  void* alloc_bytes(size_t bytes) {
    bytes = (bytes + 255) / 256 * 256;
    if (bytes == 0) bytes = 256;
    for (auto& c : chunks_)
      if (c.size - c.used >= bytes) {
        void* p = (char*)c.p + c.used;
        c.used += bytes;
        return p;
      }
    Chunk c;
    c.size = std::max<size_t>(bytes, (size_t)64 << 20);
    if (hipMalloc(&c.p, c.size) != hipSuccess) {
      (void)hipGetLastError();
      throw Error(ST_ENOMEM, "device allocation of " + std::to_string(c.size) + " bytes failed");
    }
    c.used = bytes;
    chunks_.push_back(c);
    return c.p;
  }
  void memset_zero(void* p, size_t bytes) { CORRLA_HIP(hipMemsetAsync(p, 0, bytes, stream)); }
  // zero-filled workspace from the zero pool
  void* alloc_zeroed(size_t bytes) {
    bytes = (bytes + 255) / 256 * 256;
    if (bytes == 0) bytes = 256;
    Chunk* hit = nullptr;
    for (auto& c : zchunks_)
      if (c.size - c.used >= bytes) {
        hit = &c;
        break;
      }
    if (!hit) {
      Chunk c;
      c.size = std::max<size_t>(bytes, (size_t)128 << 20);
      if (hipMalloc(&c.p, c.size) != hipSuccess) {
        (void)hipGetLastError();
        throw Error(ST_ENOMEM, "device allocation of " + std::to_string(c.size) + " bytes failed");
      }
      zchunks_.push_back(c);
      hit = &zchunks_.back();
    }
    char* p = (char*)hit->p + hit->used;
    const size_t end = hit->used + bytes;
    if (end > hit->zeroed) {  // beyond what begin_call cleared
      const size_t from = std::max(hit->used, hit->zeroed);
      CORRLA_HIP(hipMemsetAsync((char*)hit->p + from, 0, end - from, stream));
    }
    hit->used = end;
    return p;
  }

  // rows x cols in the padded layout (gemm_plan.hpp: skinny_layout), not yet backed by memory
  template <class T>
  static Skinny<T> skinny_of(int64_t rows, int64_t cols) {
    const SkinnyLayout lay = skinny_layout(rows, cols);
    Skinny<T> s;
    s.rows = rows;
    s.cols = cols;
    s.ld = lay.ld;
    s.cols_alloc = lay.cols_alloc;
    return s;
  }
  template <class T>
  Skinny<T> alloc_skinny(int64_t rows, int64_t cols) {
    Skinny<T> s = skinny_of<T>(rows, cols);
    const size_t bytes = (size_t)s.ld * (size_t)s.cols_alloc * sizeof(T);
    s.p = (T*)alloc_zeroed(bytes);
    return s;
  }
  // a skinny matrix that a product is about to overwrite completely (every allocated column, rows [0, rows)): only
  // the padding rows [rows, ld) are cleared instead of the whole buffer (four m x l work matrices of a 10^7-row call
  // are 12.8 GB of memset otherwise)
  template <class T>
  Skinny<T> alloc_skinny_out(int64_t rows, int64_t cols) {
    Skinny<T> s = skinny_of<T>(rows, cols);
    const size_t bytes = (size_t)s.ld * (size_t)s.cols_alloc * sizeof(T);
    if (bytes < ((size_t)4 << 20)) {
      s.p = (T*)alloc_zeroed(bytes);
      return s;
    }
    s.p = (T*)alloc_bytes(bytes);
    if (s.ld > rows)
      CORRLA_HIP(hipMemset2DAsync(s.p + rows, (size_t)s.ld * sizeof(T), 0, (size_t)(s.ld - rows) * sizeof(T), (size_t)s.cols_alloc,
                                  stream));
    // the padding columns too: an uneven column blocking does not write its all-zero tail tile
    if (s.cols_alloc > cols) memset_zero(s.p + cols * s.ld, (size_t)(s.cols_alloc - cols) * s.ld * sizeof(T));
    return s;
  }
  double* alloc_f64(int64_t n) {
    return (double*)alloc_zeroed(sizeof(double) * (size_t)n);
  }
  template <class T>
  T* alloc_scalar(int n) {
    return (T*)alloc_zeroed(sizeof(T) * n);
  }

  void h2d_2d(void* dst, int64_t dpitch_e, const void* src, int64_t spitch_e, int64_t width_e, int64_t rows, size_t esz) {
    CORRLA_HIP(hipMemcpy2DAsync(dst, (size_t)dpitch_e * esz, src, (size_t)spitch_e * esz, (size_t)width_e * esz,
                                (size_t)rows, hipMemcpyHostToDevice, stream));
    sync();
  }
  template <class T>
  void h2d_2d(T* dst, int64_t dpitch_e, const T* src, int64_t spitch_e, int64_t width_e, int64_t rows) {
    h2d_2d((void*)dst, dpitch_e, (const void*)src, spitch_e, width_e, rows, sizeof(T));
  }
  // HostIo (host_io.hpp): `rows` rows of `width` bytes, pitches in bytes; both enqueue only (HostIo::finish ends the call)
  void h2d_2d_enqueue(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    CORRLA_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyHostToDevice, stream));
  }
  // lu_staging.hpp: B into the image of X
  void d2d_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    CORRLA_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, stream));
  }
  void d2h_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if (rows == 1)  // HostIo decides what is one row; a matrix whose rows touch measured slower as one large copy
      CORRLA_HIP(hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, stream));
    else
      CORRLA_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToHost, stream));
  }

  // ---- tall products: gemm_plan.hpp decides, tall_stage.hpp launches what it says and defines these members -----------
  template <class T>
  void gemm_nn(const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev);
  template <class T>
  void gemm_tn(const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev);

  // ---- CSR sparse operand (spmm_kernels.hpp) ---------------------------------------------------------------------
  static constexpr bool kHasSpmm = true;  // driver.hpp: dev_has_spmm
  // Validates row_ptr (and, check_idx, every column index) of `v` on the device, ends the call with ST_EINVAL on a
  // violation -- before anything is gathered through these arrays -- and builds the lists of long rows and their chunks.
  // One host synchronisation (the verdict and the two list sizes come back in one 40-byte copy).
  template <class T>
  void csr_plan(CsrView<T>& v, bool check_idx);
  // CSR of the transpose of a VALIDATED matrix, in arena memory (released with the call).  Entries of a row of the
  // transpose keep the order (original row, original position): a stable radix sort by column index.
  template <class T>
  CsrView<T> csr_transpose(const CsrView<T>& a);
  // y (s.rows x L) = scale * S * x (s.cols x L); writes rows [0, s.rows) x columns [0, x.cols) of y and nothing else
  template <class T>
  void spmm(const CsrView<T>& s, const Skinny<T>& x, Skinny<T>& y, const T* scale_dev);
  // XT + long-row partial sums of the SpMM: one scratch per call, grown on demand (the arena is released at end_call)
  void* spmm_scratch(size_t bytes) {
    if (bytes > sp_scratch_bytes_) {
      sp_scratch_ = alloc_bytes(bytes);
      sp_scratch_bytes_ = bytes;
    }
    return sp_scratch_;
  }
  void h2d_bytes(void* dst, const void* src, size_t bytes) {
    CORRLA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    sync();
  }

  // bf16-split tall products (mixed_kernels.hpp): f32 operands, bf16 MFMA, f32 accumulate.  np = 2
  // ("bf16x3": hi hi + hi lo + lo hi) or 3 ("bf16x6").  The caller asks mixed_fits first and keeps the exact kernels
  // for everything outside the split kernels' domain (gemm_mixed_domain).
  template <class T>
  bool mixed_fits(bool tn, const Big<T>& r, const Skinny<T>& x, const Skinny<T>& out) const;
  template <class T>
  void gemm_mixed(bool tn, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev, int np);

  // ---- dense bf16 input (bf16in_kernels.hpp): R stored in bfloat16, f32 skinny operands, f32 accumulate ---------------
  static constexpr bool kHasBf16In = true;  // driver.hpp: dev_has_bf16in
  // both products of a call with this operand and an l-column sketch are in the kernel's domain (gemm_bf16a_call_domain):
  // asked ONCE per call by the entry layer, which widens the matrix otherwise
  bool bf16a_fits(const Big<uint16_t>& r, int64_t l) const;
  // out = scale * op(R) * X on gemm_bf16a_kernel; a product outside its domain is an error (no fallback here)
  void gemm_bf16a(bool tn, const Big<uint16_t>& r, const Skinny<float>& x, Skinny<float>& out, const float* scale_dev);
  // strided bf16 view -> zero-padded row-major f32 (dst already cleared): the widened route of the entry layer
  void widen_bf16(const uint16_t* src, int64_t rows, int64_t cols, int64_t rs, int64_t cs, float* dst, int64_t ldd) {
    const int64_t tiles_c = (cols + 31) / 32, tiles_r = (rows + 31) / 32;
    if (tiles_c * tiles_r > 0x7fffffff) throw Error(ST_EINVAL, "problem too large for the launch grid");
    hipLaunchKernelGGL(k::widen_bf16_kernel, dim3((unsigned)(tiles_c * tiles_r)), dim3(256), 0, stream, src, rows, cols, rs, cs, dst, ldd,
                       tiles_c);
    CORRLA_HIP(hipGetLastError());
  }

  // ---- one-sweep Z' = A^T (A Z) (ata_kernels.hpp): row-major f32 A with n <= 512, l <= 80 (ata_plan) -----
  template <class T>
  bool ata_fused_fits(const Big<T>& a, int64_t l) const;
  template <class T>
  void ata_fused(const Big<T>& a, const Skinny<T>& x, Skinny<T>& z);

  // ---- collectives (RCCL over xGMI, on the compute stream) ---------------------------------
  template <class T>
  void allreduce(T* p, size_t count) {
    // CORRLA_FORCE_ALLREDUCE=1: issue the collective on a one-rank communicator too (an identity), so that a 1-GPU
    // box exercises the very RCCL calls -- datatype, count, in-place buffer, stream -- the N > 1 ranks make
    if (comm_size <= 1 && !(comm && env_int("CORRLA_FORCE_ALLREDUCE", 0))) return;
    if (!comm) throw Error(ST_ECOMM, "communicator not initialised");
    CORRLA_NCCL(ncclAllReduce(p, p, count, NcclType<T>::v, ncclSum, comm, stream));
    ++n_collectives;
    collective_bytes += (double)count * sizeof(T);
  }
  void allreduce_f64(double* p, size_t count) { allreduce<double>(p, count); }
  // sum of one host integer over the ranks (exact in f64 up to 2^53); synchronises.  Used for rank-invariant
  // decisions that need the global row count of a sharded matrix.
  int64_t allreduce_sum_host(int64_t v) {
    if (comm_size <= 1) return v;
    if (!comm) throw Error(ST_ECOMM, "communicator not initialised");
    double* d = alloc_f64(1);
    double h = (double)v;
    CORRLA_HIP(hipMemcpyAsync(d, &h, sizeof(double), hipMemcpyHostToDevice, stream));
    CORRLA_NCCL(ncclAllReduce(d, d, 1, ncclDouble, ncclSum, comm, stream));
    ++n_collectives;
    collective_bytes += sizeof(double);
    CORRLA_HIP(hipMemcpyAsync(&h, d, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    return (int64_t)(h + 0.5);
  }

  // ---- small transfers -------------------------------------------------------------------
  // device skinny (rows x cols leading block) -> host f64 column-major (ld = rows); synchronises
  template <class T>
  void download_skinny(const Skinny<T>& s, int64_t rows, int64_t cols, double* host) {
    const size_t n = (size_t)rows * cols;
    std::vector<T> heap;
    T* tmp = (T*)pinned_;
    if (n * sizeof(T) > kPinnedBytes) {
      heap.resize(n);
      tmp = heap.data();
    }
    CORRLA_HIP(hipMemcpy2DAsync(tmp, (size_t)rows * sizeof(T), s.p, (size_t)s.ld * sizeof(T), (size_t)rows * sizeof(T),
                                (size_t)cols, hipMemcpyDeviceToHost, stream));
    sync();
    for (size_t i = 0; i < n; ++i) host[i] = (double)tmp[i];
  }
  // host f64 column-major (rows x cols, ld_host) -> device skinny; the whole allocation is
  // rewritten so padding stays zero
  template <class T>
  void upload_skinny(const double* host, int64_t rows, int64_t cols, int64_t ld_host, Skinny<T>& dst) {
    const size_t n = (size_t)dst.ld * dst.cols_alloc;
    std::vector<T> heap;
    T* tmp = (T*)pinned_;
    if (n * sizeof(T) > kPinnedBytes) {
      heap.resize(n);
      tmp = heap.data();
    }
    sync();  // the staging buffer may still feed an earlier copy
    std::memset(tmp, 0, n * sizeof(T));
    for (int64_t j = 0; j < cols; ++j)
      for (int64_t i = 0; i < rows; ++i) tmp[(size_t)j * dst.ld + i] = (T)host[(size_t)j * ld_host + i];
    CORRLA_HIP(hipMemcpyAsync(dst.p, tmp, n * sizeof(T), hipMemcpyHostToDevice, stream));
    if (!heap.empty()) sync();
  }
  template <class T>
  void upload_skinny_native(const T* host, int64_t ld_host, Skinny<T>& dst) {
    h2d_2d(dst.p, dst.ld, host, ld_host, dst.rows, dst.cols);
  }
  template <class T>
  void copy_in_skinny(const T* src_dev, int64_t ld_src, Skinny<T>& dst) {
    CORRLA_HIP(hipMemcpy2DAsync(dst.p, (size_t)dst.ld * sizeof(T), src_dev, (size_t)ld_src * sizeof(T),
                                (size_t)dst.rows * sizeof(T), (size_t)dst.cols, hipMemcpyDeviceToDevice, stream));
  }
  template <class T>
  void copy_skinny(const Skinny<T>& src, Skinny<T>& dst) {
    CORRLA_HIP(hipMemcpyAsync(dst.p, src.p, (size_t)src.ld * src.cols_alloc * sizeof(T), hipMemcpyDeviceToDevice, stream));
  }
  // dst columns [c0, c0 + n) <- src columns [0, n)  (same row count, hence the same leading dimension)
  template <class T>
  void copy_cols(const Skinny<T>& src, Skinny<T>& dst, int64_t c0, int64_t n) {
    if (src.ld != dst.ld) throw Error(ST_EINVAL, "internal: copy_cols needs equal leading dimensions");
    if (n > 0)
      CORRLA_HIP(hipMemcpyAsync(dst.p + c0 * dst.ld, src.p, (size_t)n * src.ld * sizeof(T), hipMemcpyDeviceToDevice, stream));
  }
  // y -= p over the whole (padded) allocation
  template <class T>
  void sub_inplace(Skinny<T>& y, const Skinny<T>& p) {
    const int64_t n = y.ld * std::min(y.cols_alloc, p.cols_alloc);
    const int blocks = (int)std::min<int64_t>(4096, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL((k::sub_kernel<T>), dim3(blocks), dim3(256), 0, stream, y.p, (const T*)p.p, n);
    CORRLA_HIP(hipGetLastError());
  }
  template <class T>
  void zero_cols(Skinny<T>& s, int64_t c0, int64_t c1) {
    if (c1 > c0) memset_zero(s.p + c0 * s.ld, (size_t)(c1 - c0) * s.ld * sizeof(T));
  }
  template <class T>
  void store_values(const T* host_src, int64_t n, T* dst, bool dst_is_host) {
    if (dst_is_host) {
      std::memcpy(dst, host_src, sizeof(T) * n);
    } else {
      CORRLA_HIP(hipMemcpyAsync(dst, host_src, sizeof(T) * n, hipMemcpyHostToDevice, stream));
      sync();
    }
  }
  template <class T>
  void copy_values_out(const T* src_dev, int64_t n, T* dst, bool dst_is_host) {
    CORRLA_HIP(hipMemcpyAsync(dst, src_dev, sizeof(T) * n, dst_is_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                              stream));
    if (dst_is_host) sync();
  }
  // ---- thin-Q orthonormalisation: thinq_plan.hpp routes and sizes, thinq_stage.hpp launches what it says and defines the
  // members declared here ----
  template <class T>
  bool device_chol_fits(int64_t l) const { return thinq_route(sizeof(T), l, thinq_knobs_).factor == ThinQFactor::kSingle; }
  template <class T>
  bool device_chol_blocked_fits(int64_t l) const { return thinq_route(sizeof(T), l, thinq_knobs_).factor == ThinQFactor::kBlocked2x2; }
  template <class T>
  bool device_qr_robust_fits(int64_t l) const { return thinq_route(sizeof(T), l, thinq_knobs_).robust; }
  // one column block: the products of a pass may run in place (see apply_inplace)
  bool qr_inplace_fits(int64_t l) const { return thinq_route(sizeof(float), l, thinq_knobs_).inplace; }
  // dst(dr0 + i, dc0 + j) <- src(r0 + i, c0 + j), i < rows, j < cols
  template <class T>
  void copy_block(const Skinny<T>& src, int64_t r0, int64_t c0, int64_t rows, int64_t cols, Skinny<T>& dst, int64_t dr0,
                  int64_t dc0) {
    if (rows <= 0 || cols <= 0) return;
    CORRLA_HIP(hipMemcpy2DAsync(dst.p + dc0 * dst.ld + dr0, (size_t)dst.ld * sizeof(T), src.p + c0 * src.ld + r0,
                                (size_t)src.ld * sizeof(T), (size_t)rows * sizeof(T), (size_t)cols, hipMemcpyDeviceToDevice,
                                stream));
  }
  // optimistic CholeskyQR2: factor-and-invert of the r x r Gram g into m_out, status record `slot` of st_dev
  template <class T>
  void chol_inv(const Skinny<T>& g, int64_t r, T piv_rel, Skinny<T>& m_out, void* st_dev, int slot);
  // ---- device-robust Cholesky-QR (driver.hpp: orthonormalize_device) ----
  // every launch enqueued while a run_if word is set does nothing when that device word is 0
  void set_run_if(const int* p) { run_if_ = p; }
  // passes a device-robust thin-Q enqueues on this context (driver.hpp: orthonormalize_device); grows on demand
  int robust_passes() const { return robust_passes_; }
  void set_robust_passes(int n) { robust_passes_ = n; }
  // the core SVD of a call did not converge within the sweeps enqueued: enqueue 8 more from now on (false: at the cap)
  bool svd_more_sweeps() {
    if (svd_state_.extra_sweeps >= 24) return false;
    svd_state_.extra_sweeps += 8;
    svd_state_.sweeps_hint = 0;
    return true;
  }
  // the W-only shortcut of the block Jacobi failed its verification: accumulate V from now on (false: already does)
  bool svd_force_v() {
    if (svd_state_.force_v) return false;
    svd_state_.force_v = true;
    return true;
  }
  // sweeps the last converged core SVD of this context used: the next call enqueues two more than that instead of the
  // default (the sweeps enqueued beyond convergence are launches that only test a flag: 15 x 4.6 us at C2)
  void svd_sweeps_used(int n) { svd_state_.sweeps_hint = std::max(svd_state_.sweeps_hint - 1, n); }
  int* alloc_flags(int n) { return (int*)alloc_zeroed(sizeof(int) * (size_t)std::max(n, 1)); }
  void* alloc_zeroed_bytes(size_t bytes) { return alloc_zeroed(bytes); }
  void read_bytes(const void* dev_p, size_t bytes, void* host) {
    CORRLA_HIP(hipMemcpyAsync(host, dev_p, bytes, hipMemcpyDeviceToHost, stream));
    sync();
  }
  // TEST HOOK (CORRLA_TEST_POISON_CORE): entry (i, j) of a skinny matrix <- NaN (kind 1) / +inf (kind 2)
  template <class T>
  void poison_entry(Skinny<T>& s, int64_t i, int64_t j, int kind) {
    hipLaunchKernelGGL((k::poison_entry_kernel<T>), dim3(1), dim3(1), 0, stream, s.p + j * s.ld + i, kind);
    CORRLA_HIP(hipGetLastError());
  }
  // ---- workspace marks: a repeated attempt of a call (driver.hpp: random_svd_tall) reuses the workspace of the
  // abandoned one instead of growing the arena (an ill-conditioned 10^7 x 80 call held four 3.2 GB buffers per attempt)
  struct ArenaMark {
    std::vector<size_t> used, zused;
  };
  ArenaMark arena_mark() const {
    ArenaMark mk;
    for (const auto& c : chunks_) mk.used.push_back(c.used);
    for (const auto& c : zchunks_) mk.zused.push_back(c.used);
    return mk;
  }
  void arena_rewind(const ArenaMark& mk) {
    sp_scratch_ = nullptr;  // may lie behind the mark
    sp_scratch_bytes_ = 0;
    for (size_t i = 0; i < chunks_.size(); ++i) chunks_[i].used = i < mk.used.size() ? mk.used[i] : 0;
    for (size_t i = 0; i < zchunks_.size(); ++i) {
      Chunk& c = zchunks_[i];
      const size_t keep = i < mk.zused.size() ? mk.zused[i] : 0;
      // what the abandoned attempt dirtied goes back to the pool as zeros (stream order: after its kernels)
      if (c.used > keep) CORRLA_HIP(hipMemsetAsync((char*)c.p + keep, 0, c.used - keep, stream));
      c.zeroed = std::max(c.zeroed, c.used);
      c.used = keep;
    }
  }
  // ---- start of a sharded call: ONE small all-reduce (max) carries (a) this rank's validation / staging status, so that
  // a rank-local failure ends the call on EVERY rank instead of leaving the peers blocked in the first collective, and
  // (b) the adaptive schedule state of the context (thin-Q passes enqueued, extra Jacobi sweeps, sweep hint, V mode),
  // which decides how many collectives a call enqueues and so must not differ between ranks with different histories.
  // Returns the largest status over the ranks.  Synchronises (the stream is idle at this point of a call).
  int sharded_handshake(int local_status) {
    if (comm_size <= 1 && !(comm && env_int("CORRLA_FORCE_ALLREDUCE", 0))) return local_status;
    if (!comm) throw Error(ST_ECOMM, "communicator not initialised");
    double h[8] = {(double)local_status, (double)robust_passes_, (double)svd_state_.extra_sweeps, (double)svd_state_.sweeps_hint,
                   svd_state_.force_v ? 1.0 : 0.0, 0.0, 0.0, 0.0};
    double* d = (double*)alloc_bytes(sizeof(h));
    CORRLA_HIP(hipMemcpyAsync(d, h, sizeof(h), hipMemcpyHostToDevice, stream));
    CORRLA_NCCL(ncclAllReduce(d, d, 8, ncclDouble, ncclMax, comm, stream));
    ++n_collectives;
    collective_bytes += sizeof(h);
    CORRLA_HIP(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, stream));
    sync();
    robust_passes_ = (int)h[1];
    svd_state_.extra_sweeps = (int)h[2];
    svd_state_.sweeps_hint = (int)h[3];
    svd_state_.force_v = h[4] != 0.0;
    return (int)h[0];
  }
  void read_flags(const int* dev_p, int n, int* host) {
    CORRLA_HIP(hipMemcpyAsync(host, dev_p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, stream));
    sync();
  }
  // 2 x 2 blocked robust factorisation (l > 176 / 152): the whole Gram is inspected (shift decision, ||G - I||) and shifted
  // once, the two diagonal-block factorisations take the shift from the record, combine_need forms the pass verdict
  template <class T>
  void* alloc_inspect();
  template <class T>
  const void* inspect_shift_ptr(const void* insp) const;
  template <class T>
  void gram_inspect(Skinny<T>& g, int64_t l, float shift_rel, int shift_mode, void* insp);
  template <class T>
  void combine_need(int* need, const void* insp, const int* na, const int* nb);
  template <class T>
  void chol_inv_robust(const Skinny<T>& g, int64_t r, T piv_rel, float shift_rel, int shift_mode, float null_excess,
                       Skinny<T>& m_out, void* st_dev, int slot, int* need_next, int* null_mask,
                       const void* abs_shift = nullptr, float need_ratio = 0.f);
  // y <- y * m (m: l x l): in place -- a workgroup / wave of the product kernels reads exactly the rows it writes,
  // all of them before its first store (one column block only: device_qr_robust_fits)
  template <class T>
  void apply_inplace(Skinny<T>& y, int64_t l, const Skinny<T>& m) {
    Skinny<T> out = y.view_cols(l);
    Skinny<T> mv = m.view_cols(l);
    mv.rows = l;
    launch_gemm<T>(true, as_rowmajor_transposed(y, l), mv, out, (const T*)nullptr);
  }
  // columns of y marked in null_mask <- random columns (refill_null_kernel)
  template <class T>
  void refill_null(Skinny<T>& y, int64_t l, const int* null_mask, uint64_t seed);

  void read_chol_status(const void* st_dev, int n, int* fail, float* min_ratio, float* dev_i) {
    static_assert(sizeof(k::CholStatus) == 32, "driver.hpp assumes 32-byte status records");
    static_assert(k::kNeedNonFinite == kFlagNonFinite && k::kNeedNullCols == kFlagNullCols, "need_next bits: kernels vs driver");
    std::vector<k::CholStatus> h((size_t)std::max(n, 1));
    CORRLA_HIP(hipMemcpyAsync(h.data(), st_dev, sizeof(k::CholStatus) * n, hipMemcpyDeviceToHost, stream));
    sync();
    for (int i = 0; i < n; ++i) {
      fail[i] = h[i].fail;
      min_ratio[i] = h[i].min_ratio;
      dev_i[i] = h[i].dev_i;
      if (env_int("CORRLA_DEBUG", 0) >= 2)
        std::fprintf(stderr, "[corrla] chol_inv[%d]: fail %d min_ratio %.3g dev_i %.3g clk %lld wall %lld (%.0f MHz)\n", i,
                     h[i].fail, h[i].min_ratio, h[i].dev_i, h[i].clk, h[i].wall,
                     h[i].wall > 0 ? 100.0 * (double)h[i].clk / (double)h[i].wall : 0.0);
    }
  }

  // m_out (r x r) = (I + E)^(-1/2) with G = I + E given in g (overwritten by E); everything on the device
  template <class T>
  void inv_sqrt_series(Skinny<T>& g, int64_t r, Skinny<T>& m_out);

  // ---- Householder TSQR with explicit thin Q (tsqr_kernels.hpp) -------------------------------------------
  // one 2 l x l panel (plus the 16 x 16 T and Gram blocks of the compact-WY form) must fit in LDS: l <= 142 (f32) / 99 (f64)
  template <class T>
  bool householder_fits(int64_t l) const { return hh_fits(sizeof(T), l); }
  // widest column block of a Householder thin-Q: the widest panel one workgroup can hold, under the CORRLA_HH_BLOCK cap
  template <class T>
  int householder_max_width() const { return (int)hh_capped_width(hh_max_width(sizeof(T)), thinq_knobs_.hh_block); }
  // Up sweep of the TSQR of y (m x l, m >= l): leaf reflectors -> tmp (same shape as y), tree reflectors and the root's
  // R factor (l x l, column-major, ld = l) stay in call-lifetime device buffers named by the returned state.
  template <class T>
  struct HhState {
    int64_t m = 0;
    int l = 0;
    HhTreePlan plan;  // the panel tree, the buffer sizes and the LDS of both sweeps
    std::vector<T*> rbuf, cbuf, taub, vbuf, tbuf;  // per level; tbuf: the T factors of the 16-column blocks
    T* r_root() const { return rbuf[plan.levels]; }
  };
  template <class T>
  HhState<T> householder_up(Skinny<T>& y, Skinny<T>& tmp);
  // Down sweep: y <- Q [C; 0] with Q the orthogonal factor of the up sweep and C = root_coef (l x l, column-major,
  // ld = l; nullptr = the identity, i.e. y <- the explicit thin Q).  A cross-rank TSQR passes its block of the top-level
  // Q here (driver.hpp householder_panel).
  template <class T>
  void householder_down(HhState<T>& h, Skinny<T>& y, Skinny<T>& tmp, const T* root_coef = nullptr);
  // y (m x l, m >= l) <- thin Q of its Householder QR; tmp (same shape) receives the leaf reflectors
  template <class T>
  void householder_thin_q(Skinny<T>& y, Skinny<T>& tmp) {
    HhState<T> h = householder_up(y, tmp);
    householder_down(h, y, tmp);
  }
  int rank() const { return comm_rank; }

  // SVD of the l x l core (random_svd.rs:89), defined in core_svd_stage.hpp with the launchers it switches into
  template <class T>
  void small_svd(const Skinny<T>& c, int64_t l, int64_t k, Skinny<T>& m1, Skinny<T>& m2, T* s_dev, void* conv_status);
  // skinny (rows x ncols) -> column-major destination, optionally transposed (ncols x rows)
  template <class T>
  void copy_out(const Skinny<T>& src, int64_t ncols, T* dst, int64_t ldd, bool transpose, bool to_host) {
    const int64_t rows = src.rows;
    if (!to_host) {
      launch_copy_out(src.p, src.ld, rows, ncols, dst, ldd, transpose);
      return;
    }
    if (!transpose) {
      CORRLA_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(T), src.p, (size_t)src.ld * sizeof(T),
                                  (size_t)rows * sizeof(T), (size_t)ncols, hipMemcpyDeviceToHost, stream));
    } else {
      T* tmp = (T*)alloc_bytes((size_t)rows * ncols * sizeof(T));
      launch_copy_out(src.p, src.ld, rows, ncols, tmp, ncols, true);
      CORRLA_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(T), tmp, (size_t)ncols * sizeof(T),
                                  (size_t)ncols * sizeof(T), (size_t)rows, hipMemcpyDeviceToHost, stream));
    }
    sync();
  }
  template <class T>
  void pack_strided(const T* src, int64_t rows, int64_t cols, int64_t rs, int64_t cs, T* dst, int64_t ldd) {
    const int64_t tiles_c = (cols + 31) / 32, tiles_r = (rows + 31) / 32;
    if (tiles_c * tiles_r > 0x7fffffff) throw Error(ST_EINVAL, "problem too large for the launch grid");
    dim3 grid((unsigned)(tiles_c * tiles_r));
    hipLaunchKernelGGL((k::pack_strided_kernel<T>), grid, dim3(256), 0, stream, src, rows, cols, rs, cs, dst, ldd, tiles_c);
    CORRLA_HIP(hipGetLastError());
  }

  // ---- implicit centring ---------------------------------------------------------
  template <class T>
  void weighted_colsum(const Skinny<T>& x, int64_t rows, const T* w, T* v);  // colstat_stage.hpp
  template <class T>
  void rank1_sub(Skinny<T>& out, int64_t rows, const T* u, const T* v, const T* scale) {
    dim3 grid((unsigned)((rows + 255) / 256), (unsigned)out.cols_alloc);
    check_grid(grid);
    hipLaunchKernelGGL((k::rank1_sub_kernel<T>), grid, dim3(256), 0, stream, out.p, out.ld, rows, u, v, scale);
    CORRLA_HIP(hipGetLastError());
  }

  // sign convention: flip (u_i, v_i) so the largest-magnitude entry of v_i is positive
  template <class T>
  void fix_signs(Skinny<T>& v_ref, Skinny<T>& other, int64_t k) {
    hipLaunchKernelGGL((k::column_sign_apply_kernel<T>), dim3((unsigned)k), dim3(256), 0, stream, v_ref.p, v_ref.ld, v_ref.rows,
                       other.p, other.ld, other.rows);
    CORRLA_HIP(hipGetLastError());
  }
  template <class T>
  void fill_const(T* p, int64_t n, T v) {
    const int blocks = (int)std::min<int64_t>(2048, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL((k::fill_const_kernel<T>), dim3(blocks), dim3(256), 0, stream, p, n, v);
    CORRLA_HIP(hipGetLastError());
  }
  // inv_sd (optional, indexed like mu): the copy is standardised as well as centred
  template <class T>
  void center_rows_cols(const T* in, int64_t rows, int64_t cols, int64_t ldi, const T* mu, bool along_cols, T* out,
                        int64_t ldo, const T* inv_sd = nullptr) {
    dim3 grid((unsigned)((cols + 255) / 256), (unsigned)std::min<int64_t>(rows, 4096));
    hipLaunchKernelGGL((k::center_kernel<T>), grid, dim3(256), 0, stream, in, rows, cols, ldi, mu, along_cols ? 1 : 0, out,
                       ldo, inv_sd);
    CORRLA_HIP(hipGetLastError());
  }

  // ---- PCA on standardised columns: colstat_plan.hpp plans, colstat_stage.hpp launches colvar_kernels.hpp and defines
  // the members declared here ----
  static constexpr bool kHasColVar = true;  // driver.hpp: dev_has_colvar
  // ss[j] (f64) = sum_i (x_ij - mu_j)^2 per data column j of the staged operand `a` (f32, f64 or bf16 bit patterns, read
  // in place).  along_cols: the data columns run along the memory columns (reduce down the rows), else they are the
  // memory rows (reduce along them).  Per-slab partial sums, then a final sum in index order.
  template <class TI, class T>
  void col_ss(const Big<TI>& a, bool along_cols, const T* mu, double* ss);
  // the same over a CSR whose ROWS are the data columns (a transpose built by csr_transpose)
  template <class T>
  void col_ss_csr(const CsrView<T>& s, const T* mu, int64_t n_samples, double* ss);
  // sd[j] = sqrt(ss[j] / (m - 1)) -- 1 for a constant column -- and its reciprocal, on the device
  template <class T>
  void sd_from_ss(const double* ss, const T* mu, int64_t n, int64_t m_samples, T* sd, T* inv_sd);
  // ---- covariance / correlation matrices: syrk_plan.hpp plans, cov_stage.hpp launches syrk_kernels.hpp ---------------------
  static constexpr bool kHasSyrk = true;  // driver.hpp: dev_has_syrk
  const SyrkKnobs& syrk_knobs() const { return syrk_knobs_; }
  // ---- fitted PCA model on the device: pca_apply_plan.hpp plans, pca_apply_stage.hpp launches pca_apply_kernels.hpp ---------
  static constexpr bool kHasPcaApply = true;  // driver.hpp: dev_has_pca_apply
  // ---- radial-basis-function kernel matrices: rbf_plan.hpp plans, rbf_stage.hpp launches rbf_kernels.hpp ---------------------
  static constexpr bool kHasRbf = true;  // driver.hpp: dev_has_rbf
  // ---- polynomial response surfaces: polyfit_plan.hpp plans, polyfit_stage.hpp launches polyfit_kernels.hpp ------------------
  static constexpr bool kHasPolyfit = true;  // driver.hpp: dev_has_polyfit
  // ---- kernel density estimates: kde_plan.hpp plans, kde_stage.hpp launches kde_kernels.hpp -----------------------------------
  static constexpr bool kHasKde = true;  // driver.hpp: dev_has_kde
  // ---- constrained Dirichlet sampling: dirichlet_plan.hpp plans, dirichlet_stage.hpp launches dirichlet_kernels.hpp ---------
  static constexpr bool kHasDirichlet = true;  // driver.hpp: dev_has_dirichlet
  // ---- multivariate normal rows and sandwich variances: mvn_plan.hpp plans, mvn_stage.hpp launches mvn_kernels.hpp ----------
  static constexpr bool kHasMvn = true;  // driver.hpp: dev_has_mvn
  // ---- dense LU solve and the RBF fit on it: lu_plan.hpp plans, lu_stage.hpp launches lu_kernels.hpp --------------------------
  static constexpr bool kHasLu = true;  // driver.hpp: dev_has_lu
  // ---- dense Cholesky factor and SPD solve: chol_plan.hpp plans, chol_stage.hpp launches chol_kernels.hpp ---------------------
  static constexpr bool kHasChol = true;  // driver.hpp: dev_has_chol
  // ---- symmetric eigensolver: eigh_plan.hpp plans, eigh_stage.hpp launches eigh_kernels.hpp ------------------------------------
  static constexpr bool kHasEigh = true;  // driver.hpp: dev_has_eigh
  const PolyKnobs& poly_knobs() const { return poly_knobs_; }
  // The plan's pair table on the device.  It depends on (k, r, degree) alone, so it is uploaded when those change and kept
  // between calls: a repeated fit enqueues without a synchronising copy.
  const int32_t* poly_table(int64_t kf, int64_t r, int degree) {
    const int64_t key = (kf * 128 + r) * 4 + degree;
    if (key != poly_table_key_) {
      constexpr size_t kMaxBytes = ((size_t)poly_terms(k::kPolyMaxK, 2) + k::kPolyMaxRhs + k::kPolyBT) * sizeof(int32_t);
      if (!poly_table_) CORRLA_HIP(hipMalloc((void**)&poly_table_, kMaxBytes));
      const std::vector<int32_t> t = poly_pair_table(kf, r, degree);
      sync();  // a queued launch may still read the previous table
      h2d_bytes(poly_table_, t.data(), t.size() * sizeof(int32_t));
      poly_table_key_ = key;
    }
    return poly_table_;
  }
  // out(i, c) = d[i] * in(i, c) over every allocated column (the padding columns are zero and stay zero); out may be in
  template <class T>
  void row_scale(const Skinny<T>& in, Skinny<T>& out, int64_t rows, const T* d) {
    if (in.ld != out.ld || in.cols_alloc > out.cols_alloc) throw Error(ST_EINVAL, "internal: row_scale operands must share the padded layout");
    dim3 grid((unsigned)((rows + 255) / 256), (unsigned)in.cols_alloc);
    check_grid(grid);
    hipLaunchKernelGGL((k::row_scale_kernel<T>), grid, dim3(256), 0, stream, (const T*)in.p, out.p, in.ld, rows, d);
    CORRLA_HIP(hipGetLastError());
  }

  // ---- elementwise / reductions ------------------------------------------------------------
  template <class T>
  void sumsq(const Skinny<T>& y, double* out_dev) {
    const int64_t n = y.ld * y.cols_alloc;  // padding is zero
    const int blocks = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n + 255) / 256));
    double* partial = (double*)alloc_bytes(sizeof(double) * blocks);
    hipLaunchKernelGGL((k::sumsq_partial_kernel<T>), dim3(blocks), dim3(256), 0, stream, y.p, n, partial);
    hipLaunchKernelGGL(k::sum_partials_kernel, dim3(1), dim3(64), 0, stream, partial, blocks, out_dev);
    CORRLA_HIP(hipGetLastError());
  }
  // ss_dev <- sum of squares of y, inv_dev <- 1 / sqrt(ss): the partial sums and ONE finishing launch
  template <class T>
  void inv_norm(const Skinny<T>& y, double* ss_dev, T* inv_dev) {
    const int64_t n = y.ld * y.cols_alloc;  // padding is zero
    const int blocks = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n + 255) / 256));
    double* partial = (double*)alloc_bytes(sizeof(double) * blocks);
    hipLaunchKernelGGL((k::sumsq_partial_kernel<T>), dim3(blocks), dim3(256), 0, stream, y.p, n, partial);
    hipLaunchKernelGGL((k::sum_partials_rsqrt_kernel<T>), dim3(1), dim3(64), 0, stream, (const double*)partial, blocks, ss_dev, inv_dev);
    CORRLA_HIP(hipGetLastError());
  }
  template <class T>
  void rsqrt_scalar(const double* ss_dev, T* out_dev) {
    hipLaunchKernelGGL((k::rsqrt_scalar_kernel<T>), dim3(1), dim3(1), 0, stream, ss_dev, out_dev);
    CORRLA_HIP(hipGetLastError());
  }
  template <class T>
  void scale_inplace(Skinny<T>& y, const T* scale_dev) {
    const int64_t n = y.ld * y.cols_alloc;
    const int blocks = (int)std::min<int64_t>(2048, std::max<int64_t>(1, (n + 255) / 256));
    hipLaunchKernelGGL((k::scale_kernel<T>), dim3(blocks), dim3(256), 0, stream, y.p, n, scale_dev);
    CORRLA_HIP(hipGetLastError());
  }
  template <class T>
  void fill_normal(T* p, int64_t rows, int64_t cols, int64_t rs, int64_t cs, uint64_t seed, int64_t row0,
                   int64_t global_cols) {
    const int64_t n = rows * cols;
    if (n <= 0) return;
    const int blocks = (int)std::min<int64_t>(8192, (n + 255) / 256);
    hipLaunchKernelGGL((k::fill_normal_kernel<T>), dim3(blocks), dim3(256), 0, stream, p, rows, cols, rs, cs, seed, row0,
                       global_cols, cs <= rs ? 1 : 0);
    CORRLA_HIP(hipGetLastError());
  }

  // ---- per-phase device times (corrla_timings) ------------------------------------------------------------
  // An event is recorded on the compute stream at every phase boundary; after the call has completed,
  // phase_resolve() adds the elapsed device time between consecutive events to the slot named at the later one.
  // phase_events_ off (corrla_ctx_set_phase_timings): only the first and the last event of a call are recorded --
  // total_ms stays, the per-phase slots stay zero -- because every event record is ~5 us of idle GPU between kernels
  // (9 of them per call: 1 % of a 5 ms step).  The two events around the sketch launch are always recorded.
  void set_phase_events(bool on) { phase_events_ = on; }
  void phase_end() {
    if (!phase_events_) phase_mark_impl(nullptr);
  }
  void phase_mark(double* slot) {
    if (!phase_events_ && slot != nullptr) return;
    phase_mark_impl(slot);
  }
  void phase_mark_impl(double* slot) {
    if (ev_used_ == ev_pool_.size()) {
      hipEvent_t e;
      CORRLA_HIP(hipEventCreate(&e));
      ev_pool_.push_back(e);
    }
    hipEvent_t e = ev_pool_[ev_used_++];
    CORRLA_HIP(hipEventRecord(e, stream));
    marks_.push_back({e, slot});
  }
  void phase_forget() {
    for (auto& m_ : marks_) m_.slot = nullptr;
  }
  // call after end_call(); *total (optional) receives first-mark -> last-mark
  void phase_resolve(double* total) {
    for (size_t i = 1; i < marks_.size(); ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, marks_[i - 1].ev, marks_[i].ev) != hipSuccess) {
        (void)hipGetLastError();
        continue;
      }
      if (marks_[i].slot) *marks_[i].slot += (double)ms;
    }
    if (total && marks_.size() >= 2) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, marks_.front().ev, marks_.back().ev) == hipSuccess)
        *total = (double)ms;
      else
        (void)hipGetLastError();
    }
    marks_.clear();
  }

  // hipEvents on the compute stream around a kernel sequence of the current call (read after end_call)
  void event_mark(int i) {
    CORRLA_HIP(hipEventRecord(events_[i], stream));
    events_set_[i] = true;
  }
  double event_elapsed_ms(int i, int j) {
    if (!events_set_[i] || !events_set_[j]) return 0.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, events_[i], events_[j]) != hipSuccess) {
      (void)hipGetLastError();
      return 0.0;
    }
    return (double)ms;
  }

  // hipEvent timing of `reps` back-to-back sketch products on this stream
  template <class F>
  double time_on_stream(int reps, F&& f) {
    hipEvent_t e0, e1;
    CORRLA_HIP(hipEventCreate(&e0));
    CORRLA_HIP(hipEventCreate(&e1));
    f();  // warm-up (also pages in the code object)
    CORRLA_HIP(hipEventRecord(e0, stream));
    for (int i = 0; i < reps; ++i) f();
    CORRLA_HIP(hipEventRecord(e1, stream));
    CORRLA_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    CORRLA_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return (double)ms / reps;
  }

 private:
  struct Chunk {
    void* p = nullptr;
    size_t size = 0, used = 0;
    size_t zeroed = 0;  // zero pool only: bytes cleared by begin_call
  };
  std::vector<Chunk> chunks_;
  std::vector<Chunk> zchunks_;  // zero pool (alloc_zeroed)
  void* sp_scratch_ = nullptr;  // XT + long-row partial sums of the SpMM (spmm), valid within one call
  size_t sp_scratch_bytes_ = 0;
  void* zero_page_ = nullptr;
  void* pinned_ = nullptr;  // staging for the small l x l transfers
  hipEvent_t events_[3] = {nullptr, nullptr, nullptr};
  bool events_set_[3] = {false, false, false};
  struct PhaseMark {
    hipEvent_t ev;
    double* slot;
  };
  std::vector<hipEvent_t> ev_pool_;
  size_t ev_used_ = 0;
  std::vector<PhaseMark> marks_;
  static constexpr size_t kPinnedBytes = (size_t)8 << 20;
  int gemm_debug_flags_ = 0;
  GemmKnobs gemm_knobs_;
  SyrkKnobs syrk_knobs_;
  PolyKnobs poly_knobs_;
  int32_t* poly_table_ = nullptr;
  int64_t poly_table_key_ = -1;
  uint64_t entropy_ = 0, calls_ = 0, calls_sharded_ = 0;
  ThinQKnobs thinq_knobs_;  // thinq_plan.hpp
  const int* run_if_ = nullptr;
  bool phase_events_ = true;
  int robust_passes_ = 2;
  CoreSvdState svd_state_;  // core_svd_plan.hpp

  static void check_grid(const dim3& g) {
    if (g.y > 65535u || g.z > 65535u) throw Error(ST_EINVAL, "problem too large for the launch grid");
  }

  // ---- dynamic-LDS limits (lds_limit) ----
  static void set_lds_limits() {
    constexpr size_t kMax = k::kLdsMaxBytes;
    set_lds_limits_typed<float>();
    set_lds_limits_typed<double>();
    core_svd_stage::set_lds_limits<float>();
    core_svd_stage::set_lds_limits<double>();
    tall_stage::set_lds_limits();
    lu_stage::set_lds_limits();
    chol_stage::set_lds_limits();
    eigh_stage::set_lds_limits();
    // nearest neighbours and local fits of the gradient stage (grad_stage.hpp)
    lds_limit((const void*)k::knn_kernel, kMax);
    lds_limit((const void*)k::knn_mfma_kernel<4, 4>, kMax);
    lds_limit((const void*)k::knn_mfma_kernel<4, 8>, kMax);
    lds_limit((const void*)k::knn_mfma_kernel<4, 16>, kMax);
    lds_limit((const void*)k::knn_mfma_kernel<2, 4>, kMax);
    lds_limit((const void*)k::knn_mfma_kernel<2, 8>, kMax);
    lds_limit((const void*)k::knn_mfma_kernel<2, 16>, kMax);
    lds_limit((const void*)k::knn2_kernel<1>, k::k2_lds_bytes(1));
    lds_limit((const void*)k::knn2_kernel<2>, k::k2_lds_bytes(2));
    lds_limit((const void*)k::grad_fit_kernel, kMax);
    lds_limit((const void*)k::grad_fit_lin_kernel<1>, kMax);
    lds_limit((const void*)k::grad_fit_lin_kernel<2>, kMax);
    lds_limit((const void*)k::grad_fit_lin_kernel<3>, kMax);
    lds_limit((const void*)k::grad_fit_lin_kernel<4>, kMax);
    lds_limit((const void*)k::grad_fit_lin_kernel<5>, kMax);
    lds_limit((const void*)k::knn_wide_kernel, k::ws_lds_bytes());
    lds_limit((const void*)k::grad_fit_wide_kernel, k::wf_lds_bytes());
  }
  template <class T>
  static void set_lds_limits_typed() {
    tall_stage::set_lds_limits<T>();
    rbf_stage::set_lds_limits<T>();
    if (sizeof(T) == 8) polyfit_stage::set_lds_limits();
    lds_limit((const void*)k::syrk_kernel<T, true>, (size_t)k::syrk_lds_bytes((int)sizeof(T)));
    lds_limit((const void*)k::syrk_kernel<T, false>, (size_t)k::syrk_lds_bytes((int)sizeof(T)));
    thinq_stage::set_lds_limits<T>();
    mvn_stage::set_lds_limits<T>();
  }
  // ---- the tall products' launch (tall_stage.hpp) ----
  // what a launcher of the stage needs of this context beyond the plan
  tall_stage::Call tall_call();
  // out (outer_n x L) = scale * op(R) * X: op(R) = R (tn false, outer_n = R's rows) or R^T (outer_n = R's columns)
  template <class T>
  void launch_gemm(bool tn, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev);

  template <class T>
  void launch_copy_out(const T* src, int64_t lds_, int64_t rows, int64_t cols, T* dst, int64_t ldd, bool transpose) {
    const int64_t tiles_c = (cols + 31) / 32, tiles_r = (rows + 31) / 32;
    if (tiles_c * tiles_r > 0x7fffffff) throw Error(ST_EINVAL, "problem too large for the launch grid");
    dim3 grid((unsigned)(tiles_c * tiles_r));
    hipLaunchKernelGGL((k::copy_out_kernel<T>), grid, dim3(256), 0, stream, src, lds_, rows, cols, dst, ldd,
                       transpose ? 1 : 0, tiles_c);
    CORRLA_HIP(hipGetLastError());
  }
};

}  // namespace corrla
