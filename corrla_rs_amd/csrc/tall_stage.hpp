// The tall products on the device -- A X, A^T X, the Gram and apply products of the thin-Q, the bf16-split and bf16-stored
// products, the one-sweep A^T (A Z), the CSR product and the CSR preparation: one launcher per kernel family.  gemm_plan.hpp
// has decided the family and instantiation, every grid, workgroup size, LDS and workspace size, or the rejection; a launcher
// allocates what the plan sized, fills the kernel's arguments and launches.  The HipDev members the driver and the entry
// layer call are defined at the end: shape, plan, throw on `error`, launcher.
#pragma once
#include "gemm_plan.hpp"
#include "hip_backend.hpp"

namespace corrla {
namespace tall_stage {

// what a launcher needs of the context beyond the plan (HipDev::tall_call)
struct Call {
  HipDev& dev;            // the allocator: arena, zero pool, SpMM scratch
  hipStream_t stream;
  const void* zero_page;  // 256 bytes of zeros
  const int* run_if;      // optional device word: launches enqueued while it is set do nothing when it is 0
  int debug_flags;        // CORRLA_GEMM_DEBUG: timing-only ablations
};

// ---- shapes: the operands of a product without their pointers ----
template <class T>
inline GemmOperand operand(const Big<T>& r) {
  return {r.rows, r.cols, r.ld, r.cols_readable, 0, false, (uintptr_t)r.p % 16 == 0};
}
template <class T>
inline GemmOperand operand(const Skinny<T>& x) {
  return {x.rows, x.cols, x.ld, 0, x.cols_alloc, x.external, (uintptr_t)x.p % 16 == 0};
}
// R holds T, or bfloat16 bit patterns (the plan then reads r.ld and r.cols_readable in 2-byte elements)
template <class R, class T>
inline GemmShape shape(bool tn, const Big<R>& r, const Skinny<T>& x, const Skinny<T>& out, int np, int num_cus) {
  GemmShape s;
  s.tn = tn;
  s.esz = (int)sizeof(T);
  s.r = operand(r);
  s.x = operand(x);
  s.out = operand(out);
  s.same = (const void*)r.p == (const void*)x.p;
  s.np = np;
  s.num_cus = num_cus;
  s.r_bf16 = !std::is_same<R, T>::value;
  return s;
}
template <class Plan>
inline Plan checked(const Plan& p) {
  if (p.error) throw Error(ST_EINVAL, p.error);
  return p;
}

// ---- the instantiations of each family are the lists of gemm_plan.hpp: a launcher picks the one a plan names (with_nt /
// with_one_of over a list), set_lds_limits registers all of them (for_each_nt / for_each_of over the same list).  A value
// without an instantiation is an error, never another kernel.  The general kernels' list is a predicate over three
// arguments: each_general calls f(MW, NT, NW) once per instantiation, with_general for the one named. ----
template <class T, class F>
inline void each_general(const F& f) {  // f(MW, NT, NW)
  for_each_nt<2>([&](auto mw) {
    for_each_of(GeneralNWs{}, [&](auto nw) {
      for_each_nt<kMaxColTiles>([&](auto nt) {
        if constexpr (gemm_general_exists((int)sizeof(T), decltype(mw)::value, decltype(nt)::value, decltype(nw)::value)) f(mw, nt, nw);
      });
    });
  });
}
template <class T, class F>
inline void with_general(int mw_, int nt_, int nw_, const F& f) {
  with_nt<2>(mw_, [&](auto mw) {
    with_one_of(GeneralNWs{}, nw_, [&](auto nw) {
      with_nt<kMaxColTiles>(nt_, [&](auto nt) {
        if constexpr (gemm_general_exists((int)sizeof(T), decltype(mw)::value, decltype(nt)::value, decltype(nw)::value))
          f(mw, nt, nw);
        else
          throw Error(ST_EINVAL, "internal: no kernel instantiation for " + std::to_string(nw_));
      });
    });
  });
}
// the two families on bf16 planes: R = float is the bf16 split (gemm_bf16s_kernel<NT, NP, TN>, planes in MFMA fragment
// order), R = uint16_t the bf16-stored operand (gemm_bf16a_kernel<NT, TN>, three planes in memory order, no ablations)
template <class R>
struct Planes;
template <>
struct Planes<float> {
  static constexpr int kMinPlanes = kMxMinPlanes, kMaxPlanes = kMxMaxPlanes;
  static constexpr bool kKmap = true;
  static constexpr int lds_bytes(int nt, int np) { return k::mx_lds_bytes(nt, np); }
  template <int NT, int NP, bool TN>
  static auto kernel() { return k::gemm_bf16s_kernel<NT, NP, TN>; }
  static int debug_flags(const Call& c) { return c.debug_flags; }
};
template <>
struct Planes<uint16_t> {
  static constexpr int kMinPlanes = k::kBaPlanes, kMaxPlanes = k::kBaPlanes;
  static constexpr bool kKmap = false;
  static constexpr int lds_bytes(int nt, int) { return k::ba_lds_bytes(nt); }
  template <int NT, int NP, bool TN>
  static auto kernel() { return k::gemm_bf16a_kernel<NT, TN>; }
  static int debug_flags(const Call&) { return 0; }
};

// every kernel of the stage launched with more dynamic LDS than the default (HipDev::set_lds_limits); tall_apply_kernel
// takes none
template <class T>
inline void set_lds_limits() {
  each_general<T>([](auto mw, auto nt, auto nw) {
    constexpr int MW = decltype(mw)::value, NT = decltype(nt)::value, NW = decltype(nw)::value;
    constexpr int kBytes = k::gemm_lds_bytes(MW * NW / 4, NT);  // the ring of the 64 * MW * NW / 4 outer tile
    lds_limit((const void*)k::gemm_nn_kernel<T, MW, NT, false, NW>, kBytes);
    lds_limit((const void*)k::gemm_tn_kernel<T, MW, NT, NW>, kBytes);
  });
  for_each_nt<kAliasMaxTiles>([](auto nt) { lds_limit((const void*)k::gemm_nn_kernel<T, 2, decltype(nt)::value, true>, 3 * k::big_tile_bytes(2)); });
  for_each_nt<tall_max_tiles((int)sizeof(T))>([](auto nct) {
    lds_limit((const void*)k::tall_gram_kernel<T, decltype(nct)::value>, k::gram_lds_bytes(nct, (int)sizeof(T)));
  });
}
template <class R>
inline void set_planes_limits() {
  using P = Planes<R>;
  for_each_nt<kMaxColTiles>([](auto nt) {
    for_each_nt<P::kMaxPlanes, P::kMinPlanes>([&](auto np) {
      constexpr int NT = decltype(nt)::value, NP = decltype(np)::value;
      lds_limit((const void*)P::template kernel<NT, NP, false>(), P::lds_bytes(NT, NP));
      lds_limit((const void*)P::template kernel<NT, NP, true>(), P::lds_bytes(NT, NP));
    });
  });
}
inline void set_lds_limits() {
  set_planes_limits<float>();
  set_planes_limits<uint16_t>();
  for_each_of(AtaNKs{}, [](auto nk) {
    for_each_nt<kAtaMaxColTiles>([&](auto nct) {
      lds_limit((const void*)k::ata_fused_kernel<decltype(nk)::value, decltype(nct)::value>, k::ata_lds_bytes(nk, nct));
    });
  });
}

// ---- the partial results of a split reduction: their workspace, and their sum (slab_reduce_kernel / slab_reduce_deep_kernel) ----
template <class T>
inline T* alloc_slab(const Call& c, const GemmPlan& p) {
  return p.reduce.kind != SlabReduce::none ? (T*)c.dev.alloc_bytes(p.slab_bytes) : nullptr;
}
template <class T>
inline void slab_reduce(const Call& c, const SlabReducePlan& rp, const T* slab, int64_t stride, T* out, int64_t ld, const T* scale,
                        const int* run_if) {
  if (rp.kind == SlabReduce::none) return;
  const dim3 grid(rp.grid[0], rp.grid[1]);
  if (rp.kind == SlabReduce::deep)
    hipLaunchKernelGGL((k::slab_reduce_deep_kernel<T>), grid, dim3(256), 0, c.stream, slab, stride, rp.slabs, out, ld, rp.rows, rp.cols,
                       scale, run_if);
  else
    hipLaunchKernelGGL((k::slab_reduce_kernel<T>), grid, dim3(256), 0, c.stream, slab, stride, rp.slabs, out, ld, rp.rows, rp.cols, scale,
                       run_if);
  CORRLA_HIP(hipGetLastError());
}

// ---- gemm_nn_kernel / gemm_tn_kernel<T, MW, NT, NW>, the aliased gemm_nn_kernel<T, 2, NT, true> of a Gram matrix; one
// launch, or the wide and the narrow column blocks of an uneven blocking ----
template <class T>
inline void general(const Call& c, const GemmPlan& p, bool tn, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev) {
  T* slab = alloc_slab<T>(c, p);
  k::GemmArgs<T> a{r.p, r.rows, r.cols, r.ld, r.cols_readable,  // big operand
                   x.p, x.ld,                                     // skinny operand
                   out.p, out.ld, p.out_cols, 0,                  // output; col_base per launch
                   slab, p.slab_stride, scale_dev, (const T*)c.zero_page,
                   p.tiles_total, p.tiles_per_split, p.nsplit, c.debug_flags, c.run_if,
                   p.vec_store, p.rotate, p.outer_blocks, 0};     // xcd_remap per launch
  for (int i = 0; i < p.nlaunch; ++i) {
    const GemmLaunch& L = p.launch[i];
    const dim3 grid(L.grid[0], L.grid[1], L.grid[2]), block(p.block);
    a.col_base = L.col_base;
    a.xcd_remap = L.xcd_remap;
    if (p.family == GemmFamily::gram_alias)
      with_nt<kAliasMaxTiles>(L.nt, [&](auto nt) {
        hipLaunchKernelGGL((k::gemm_nn_kernel<T, 2, decltype(nt)::value, true>), grid, block, L.lds, c.stream, a);
      });
    else
      with_general<T>(p.mw, L.nt, p.nw, [&](auto mw, auto nt, auto nw) {
        constexpr int MW = decltype(mw)::value, NT = decltype(nt)::value, NW = decltype(nw)::value;
        if (tn)
          hipLaunchKernelGGL((k::gemm_tn_kernel<T, MW, NT, NW>), grid, block, L.lds, c.stream, a);
        else
          hipLaunchKernelGGL((k::gemm_nn_kernel<T, MW, NT, false, NW>), grid, block, L.lds, c.stream, a);
      });
  }
  CORRLA_HIP(hipGetLastError());
  slab_reduce<T>(c, p.reduce, slab, p.slab_stride, out.p, out.ld, scale_dev, c.run_if);
}

// ---- tall_kernels.hpp: out (m x n2) = Y M with Y^T stored row-major kdim x m ----
template <class T>
inline void tall_apply(const Call& c, const GemmPlan& p, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev) {
  const GemmLaunch& L = p.launch[0];
  const k::TallApplyArgs<T> g{r.p, r.cols, r.ld, (int)r.rows, x.p, x.ld, (int)x.cols, out.p, out.ld, (int)p.out_cols,
                              scale_dev, p.vec_store, c.run_if};
  with_nt<tall_max_tiles((int)sizeof(T))>(L.nt, [&](auto kt) {
    constexpr int K = decltype(kt)::value;
    hipLaunchKernelGGL((k::tall_apply_kernel<T, K, K>), dim3(L.grid[0]), dim3(p.block), L.lds, c.stream, g);
  });
  CORRLA_HIP(hipGetLastError());
}

// ---- tall_kernels.hpp: G (l x l) = Y^T Y, both operands the same m x l memory; one partial Gram per row group ----
template <class T>
inline void tall_gram(const Call& c, const GemmPlan& p, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev) {
  const GemmLaunch& L = p.launch[0];
  T* slab = alloc_slab<T>(c, p);
  const k::TallGramArgs<T> g{x.p, r.cols, x.ld, (int)out.rows, slab, p.slab_stride, out.ld, p.rows_per_group,
                             (const T*)c.zero_page, c.run_if};
  with_nt<tall_max_tiles((int)sizeof(T))>(L.nt, [&](auto nct) {
    hipLaunchKernelGGL((k::tall_gram_kernel<T, decltype(nct)::value>), dim3(L.grid[0]), dim3(p.block), L.lds, c.stream, g);
  });
  CORRLA_HIP(hipGetLastError());
  slab_reduce<T>(c, p.reduce, slab, p.slab_stride, out.p, out.ld, scale_dev, c.run_if);
}

// ---- mixed_kernels.hpp / bf16in_kernels.hpp: the skinny operand split into the plan's bf16 planes, then the product ----
template <class R>
inline void planes(const Call& c, const GemmPlan& p, bool tn, const Big<R>& r, const Skinny<float>& x, Skinny<float>& out,
                   const float* scale_dev) {
  using P = Planes<R>;
  __bf16* pl = (__bf16*)c.dev.alloc_bytes(p.plane_bytes);
  with_nt<P::kMaxPlanes, P::kMinPlanes>(p.np, [&](auto np) {
    hipLaunchKernelGGL((k::split_planes_kernel<decltype(np)::value, P::kKmap>), dim3(p.split_grid), dim3(256), 0, c.stream,
                       (const float*)x.p, x.ld, p.plane_cols, pl, p.plane_stride, c.run_if);
  });
  CORRLA_HIP(hipGetLastError());
  float* slab = alloc_slab<float>(c, p);
  const k::MxArgsT<R> a{r.p, r.rows, r.cols, r.ld, r.cols_readable,  // big operand
                        pl, x.ld, p.plane_stride,                    // skinny operand
                        out.p, out.ld, p.out_cols,                   // output
                        slab, p.slab_stride, scale_dev, (const float*)c.zero_page,
                        p.tiles_total, p.tiles_per_split, p.nsplit, c.run_if, p.vec_store, P::debug_flags(c)};
  const GemmLaunch& L = p.launch[0];
  with_nt<kMaxColTiles>(L.nt, [&](auto nt) {
    with_nt<P::kMaxPlanes, P::kMinPlanes>(p.np, [&](auto np) {
      constexpr int NT = decltype(nt)::value, NP = decltype(np)::value;
      auto kernel = tn ? P::template kernel<NT, NP, true>() : P::template kernel<NT, NP, false>();
      hipLaunchKernelGGL(kernel, dim3(L.grid[0], L.grid[1], L.grid[2]), dim3(p.block), L.lds, c.stream, a);
    });
  });
  CORRLA_HIP(hipGetLastError());
  slab_reduce<float>(c, p.reduce, slab, p.slab_stride, out.p, out.ld, scale_dev, c.run_if);
}

// ---- ata_kernels.hpp: Z' = A^T (A Z), one partial Z' per row group (empty groups contribute zeros) ----
inline void ata(const Call& c, const AtaPlan& p, const Big<float>& a, const Skinny<float>& x, Skinny<float>& z) {
  float* slab = (float*)c.dev.alloc_zeroed(p.slab_bytes);
  const k::AtaArgs g{a.p, a.rows, a.cols, a.ld, a.cols_readable, x.p, x.ld, slab, p.slab_stride, z.ld, p.rows_per_group, p.nrg,
                     (const float*)c.zero_page};
  with_one_of(AtaNKs{}, p.nk, [&](auto nk) {
    with_nt<kAtaMaxColTiles>(p.nct, [&](auto nct) {
      hipLaunchKernelGGL((k::ata_fused_kernel<decltype(nk)::value, decltype(nct)::value>), dim3((unsigned)p.nrg), dim3(p.block), p.lds,
                         c.stream, g);
    });
  });
  CORRLA_HIP(hipGetLastError());
  slab_reduce<float>(c, p.reduce, slab, p.slab_stride, z.p, z.ld, nullptr, nullptr);
}

// ---- spmm_kernels.hpp: X into the row-major scratch, the row gather, then the long rows chunk by chunk ----
template <class T>
inline void spmm(const Call& c, const SpmmPlan& p, const CsrView<T>& s, const Skinny<T>& x, Skinny<T>& y, const T* scale_dev) {
  const int64_t L = x.cols;
  char* scratch = (char*)c.dev.spmm_scratch(p.scratch_bytes);
  T* xt = (T*)scratch;
  T* part = (T*)(scratch + p.xt_bytes);
  auto grid = [](const unsigned (&g)[2]) { return dim3(g[0], g[1]); };
  hipLaunchKernelGGL((k::spmm_xt_kernel<T>), grid(p.grid_xt), dim3(256), 0, c.stream, (const T*)x.p, x.ld, s.cols, L, xt, p.Lp);
  hipLaunchKernelGGL((k::spmm_rows_kernel<T>), grid(p.grid_rows), dim3(256), 0, c.stream, s.rp, s.ci, s.val, (const T*)xt, p.Lp, s.rows,
                     L, y.p, y.ld, scale_dev);
  if (s.n_long > 0) {
    hipLaunchKernelGGL((k::spmm_long_partial_kernel<T>), grid(p.grid_long_partial), dim3(256), 0, c.stream, s.rp, s.ci, s.val,
                       (const T*)xt, p.Lp, L, s.long_row, s.long_base, s.chunk_long, part, p.Lpart);
    hipLaunchKernelGGL((k::spmm_long_reduce_kernel<T>), grid(p.grid_long_reduce), dim3(64), 0, c.stream, s.rp, s.long_row, s.long_base,
                       (const T*)part, p.Lpart, L, y.p, y.ld, scale_dev);
  }
  CORRLA_HIP(hipGetLastError());
}

// ---- spmm_kernels.hpp: validation of a caller's CSR arrays and the lists of long rows and their chunks ----
template <class T>
inline void csr_validate(const Call& c, CsrView<T>& v, bool check_idx) {
  HipDev& dev = c.dev;
  k::CsrCounts* cnt = (k::CsrCounts*)dev.alloc_zeroed(sizeof(k::CsrCounts));
  const int64_t top = std::max(v.rows, v.nnz);
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((top + 255) / 256, (int64_t)dev.num_cus * 16));
  hipLaunchKernelGGL(k::csr_validate_kernel, dim3(blocks), dim3(256), 0, c.stream, v.rp, v.ci, v.rows, v.cols, v.nnz, check_idx ? 1 : 0, cnt);
  CORRLA_HIP(hipGetLastError());
  k::CsrCounts h;
  dev.read_bytes(cnt, sizeof(h), &h);
  if (h.bad) {
    std::string why;
    if (h.bad & 1) why += " row_ptr[0] != 0;";
    if (h.bad & 2) why += " row_ptr is not monotone within [0, nnz];";
    if (h.bad & 4) why += " row_ptr[m] != nnz;";
    if (h.bad & 8) why += " a column index lies outside [0, n);";
    throw Error(ST_EINVAL, "invalid CSR matrix:" + why);
  }
  v.n_long = (int64_t)h.n_long;
  v.n_chunks = (int64_t)h.n_chunks;
  if (v.n_long == 0) return;
  if (v.n_chunks > 0x7fffffff) throw Error(ST_EINVAL, "problem too large for the launch grid");
  int64_t* lr = (int64_t*)dev.alloc_bytes(sizeof(int64_t) * (size_t)v.n_long);
  int64_t* lb = (int64_t*)dev.alloc_bytes(sizeof(int64_t) * (size_t)v.n_long);
  int32_t* cl = (int32_t*)dev.alloc_bytes(sizeof(int32_t) * (size_t)v.n_chunks);
  const unsigned b2 = (unsigned)std::max<int64_t>(1, std::min<int64_t>((v.rows + 255) / 256, (int64_t)dev.num_cus * 16));
  hipLaunchKernelGGL(k::csr_long_build_kernel, dim3(b2), dim3(256), 0, c.stream, v.rp, v.rows, cnt, lr, lb, cl);
  CORRLA_HIP(hipGetLastError());
  v.long_row = lr;
  v.long_base = lb;
  v.chunk_long = cl;
}

// ---- spmm_kernels.hpp: a stable radix sort of the nonzero positions by column index, then the transposed arrays ----
template <class T>
inline CsrView<T> csr_transpose(const Call& c, const CsrView<T>& a) {
  HipDev& dev = c.dev;
  const int64_t nnz = a.nnz;
  if (nnz < 1 || nnz > 0x7fffffff) throw Error(ST_EINVAL, "csr_transpose: nnz must be in [1, 2^31)");
  const int64_t nb = (nnz + k::kSortTile - 1) / k::kSortTile;
  uint32_t* key[2] = {(uint32_t*)dev.alloc_bytes(sizeof(uint32_t) * (size_t)nnz), (uint32_t*)dev.alloc_bytes(sizeof(uint32_t) * (size_t)nnz)};
  uint32_t* pay[2] = {(uint32_t*)dev.alloc_bytes(sizeof(uint32_t) * (size_t)nnz), (uint32_t*)dev.alloc_bytes(sizeof(uint32_t) * (size_t)nnz)};
  uint32_t* hist = (uint32_t*)dev.alloc_bytes(sizeof(uint32_t) * (size_t)nb * 256);
  int bits = 1;
  while (((int64_t)1 << bits) < a.cols) ++bits;
  const int passes = (bits + 7) / 8;
  const uint32_t* kin = (const uint32_t*)a.ci;  // validated: every index is in [0, cols), so the bit patterns agree
  const uint32_t* pin = nullptr;
  for (int ps = 0; ps < passes; ++ps) {
    uint32_t* kout = key[ps & 1];
    uint32_t* pout = pay[ps & 1];
    hipLaunchKernelGGL(k::csr_radix_hist_kernel, dim3((unsigned)nb), dim3(64), 0, c.stream, kin, nnz, 8 * ps, hist, nb);
    hipLaunchKernelGGL(k::csr_scan_kernel, dim3(1), dim3(1024), 0, c.stream, hist, nb * 256);
    hipLaunchKernelGGL(k::csr_radix_scatter_kernel, dim3((unsigned)nb), dim3(64), 0, c.stream, kin, pin, nnz, 8 * ps, (const uint32_t*)hist, nb,
                       kout, pout);
    CORRLA_HIP(hipGetLastError());
    kin = kout;
    pin = pout;
  }
  CsrView<T> t;
  t.rows = a.cols;
  t.cols = a.rows;
  t.nnz = nnz;
  int64_t* trp = (int64_t*)dev.alloc_bytes(sizeof(int64_t) * (size_t)(a.cols + 1));
  int32_t* tci = (int32_t*)dev.alloc_bytes(sizeof(int32_t) * (size_t)nnz);
  T* tval = (T*)dev.alloc_bytes(sizeof(T) * (size_t)nnz);
  hipLaunchKernelGGL((k::csr_transpose_finish_kernel<T>), dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, c.stream, kin, pin, a.rp, a.rows,
                     a.val, nnz, a.cols, trp, tci, tval);
  CORRLA_HIP(hipGetLastError());
  t.rp = trp;
  t.ci = tci;
  t.val = tval;
  return t;
}

}  // namespace tall_stage

// ---- the HipDev members of the stage: shape, plan, throw on `error`, launcher ----
inline tall_stage::Call HipDev::tall_call() { return {*this, stream, zero_page_, run_if_, gemm_debug_flags_}; }

template <class T>
void HipDev::launch_gemm(bool tn, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev) {
  const GemmPlan p = tall_stage::checked(gemm_plan(tall_stage::shape(tn, r, x, out, 0, num_cus), gemm_knobs_));
  if (p.family == GemmFamily::tall_apply)
    tall_stage::tall_apply(tall_call(), p, r, x, out, scale_dev);
  else if (p.family == GemmFamily::tall_gram)
    tall_stage::tall_gram(tall_call(), p, r, x, out, scale_dev);
  else
    tall_stage::general(tall_call(), p, tn, r, x, out, scale_dev);
}
template <class T>
void HipDev::gemm_nn(const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev) {
  if (x.rows != r.cols) throw Error(ST_EINVAL, "gemm_nn: inner dimensions differ");
  launch_gemm<T>(false, r, x, out, scale_dev);
}
template <class T>
void HipDev::gemm_tn(const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev) {
  if (x.rows != r.rows) throw Error(ST_EINVAL, "gemm_tn: inner dimensions differ");
  launch_gemm<T>(true, r, x, out, scale_dev);
}

template <class T>
bool HipDev::mixed_fits(bool tn, const Big<T>& r, const Skinny<T>& x, const Skinny<T>& out) const {
  return gemm_mixed_domain(tall_stage::shape(tn, r, x, out, 2, num_cus), gemm_knobs_);
}
template <class T>
void HipDev::gemm_mixed(bool tn, const Big<T>& r, const Skinny<T>& x, Skinny<T>& out, const T* scale_dev, int np) {
  if constexpr (std::is_same<T, float>::value) {
    const GemmPlan p = tall_stage::checked(gemm_plan(tall_stage::shape(tn, r, x, out, np, num_cus), gemm_knobs_));
    tall_stage::planes<float>(tall_call(), p, tn, r, x, out, scale_dev);
  } else {
    throw Error(ST_EINVAL, "internal: the bf16-split products are f32 only");
  }
}

inline bool HipDev::bf16a_fits(const Big<uint16_t>& r, int64_t l) const {
  return gemm_bf16a_call_domain(tall_stage::operand(r), l, num_cus);
}
inline void HipDev::gemm_bf16a(bool tn, const Big<uint16_t>& r, const Skinny<float>& x, Skinny<float>& out, const float* scale_dev) {
  if (x.rows != (tn ? r.rows : r.cols)) throw Error(ST_EINVAL, "gemm_bf16a: inner dimensions differ");
  const GemmPlan p = tall_stage::checked(gemm_plan(tall_stage::shape(tn, r, x, out, 0, num_cus), gemm_knobs_));
  tall_stage::planes<uint16_t>(tall_call(), p, tn, r, x, out, scale_dev);
}

template <class T>
bool HipDev::ata_fused_fits(const Big<T>& a, int64_t l) const {
  return ata_domain((int)sizeof(T), a.rows, a.cols, l);
}
template <class T>
void HipDev::ata_fused(const Big<T>& a, const Skinny<T>& x, Skinny<T>& z) {
  const AtaPlan p =
      tall_stage::checked(ata_plan((int)sizeof(T), tall_stage::operand(a), tall_stage::operand(x), tall_stage::operand(z), num_cus));
  if constexpr (std::is_same<T, float>::value) tall_stage::ata(tall_call(), p, a, x, z);  // any other type was rejected
}

template <class T>
void HipDev::spmm(const CsrView<T>& s, const Skinny<T>& x, Skinny<T>& y, const T* scale_dev) {
  if (x.rows != s.cols || y.rows != s.rows) throw Error(ST_EINVAL, "spmm: dimensions differ");
  if (x.cols < 1 || y.cols < x.cols) throw Error(ST_EINVAL, "spmm: destination has fewer columns than the operand");
  const SpmmPlan p = tall_stage::checked(spmm_plan((int)sizeof(T), s.rows, s.cols, x.cols, s.n_long, s.n_chunks));
  tall_stage::spmm(tall_call(), p, s, x, y, scale_dev);
}
template <class T>
void HipDev::csr_plan(CsrView<T>& v, bool check_idx) {
  tall_stage::csr_validate(tall_call(), v, check_idx);
}
template <class T>
CsrView<T> HipDev::csr_transpose(const CsrView<T>& a) {
  return tall_stage::csr_transpose(tall_call(), a);
}

}  // namespace corrla
