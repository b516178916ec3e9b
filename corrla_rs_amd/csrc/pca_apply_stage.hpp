// The fitted-model stage of the C ABI (corrla_pca_transform_* / corrla_pca_inverse_*, pca_rsvd.rs:43-52): the forward product
// on the tall kernels as pca_body drives them (RsvdDriver::a_times over a TallA with mu_short / inv_sd_short, or over a centred
// and scaled copy), the back-projection kernel by the plan of pca_apply_plan.hpp, and for host pointers the copies around
// them.  The arguments were checked by pca_transform_entry / pca_inverse_entry (capi_impl.hpp).
// The device path enqueues and returns, as cov_stage does: begin_call has no end_call there, every constant goes to the
// device through a kernel (fill_const), never through a synchronising copy, and a throw after begin_call is drained by the
// entry's locked_call.  What can still synchronise: hipMalloc inside alloc_bytes the first time a call needs more workspace
// than the arena holds, and the validation of a CSR operand (csr_plan), as in every CSR entry.  The host path is the same
// code behind HostIo (host_io.hpp): the whole strided SPAN of x and the output of the inverse are staged as they lie, so
// the device path's routes serve them unchanged; the model goes in at arena alignment, the scores are a packed input of the
// inverse and a packed output of the transform.
#pragma once
#include "capi_impl.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace pca_apply_stage {

// how the context's last call ran (corrla_ctx_last_pca_apply)
struct Ran {
  int centring = 0;  // 0 none, 1 fused, 2 copy
  int route = 0;     // PcaApplyRoute of the back-projection kernel, 0: none ran
};

// One launch of pca_back_kernel<T, MODE> (and, RESID, of the finishing kernel).  t: m x k column-major (ldt); v: k rows of n
// contiguous features (ldv); big: out (STORE) or x (RESID) with the plan's row stride.
template <class T>
void back(HipDev& dev, const PcaApplyPlan& p, PcaApplyMode mode, const T* t, int64_t ldt, const T* v, int64_t ldv, const T* mu,
          const T* sd, int64_t m, int64_t n, int64_t k, T* big, T* q) {
  k::PcaBackArgs<T> a{t, ldt, v, ldv, mu, sd, m, n, k, p.nbn, big, p.ld, p.wide, nullptr};
  const dim3 grid(p.grid_x);  // one-dimensional: the plan keeps it below 2^31
  if (mode == PcaApplyMode::kStore) {
    hipLaunchKernelGGL((k::pca_back_kernel<T, k::kPcaStore>), grid, dim3(p.block), p.lds_bytes, dev.stream, a);
    CORRLA_HIP(hipGetLastError());
    return;
  }
  a.ws = (T*)dev.alloc_bytes(p.ws_bytes);
  hipLaunchKernelGGL((k::pca_back_kernel<T, k::kPcaResid>), grid, dim3(p.block), p.lds_bytes, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
  hipLaunchKernelGGL((k::pca_resid_finish_kernel<T>), dim3(p.finish_grid_x), dim3(p.finish_block), 0, dev.stream, (const T*)a.ws, p.nbn, m,
                     q);
  CORRLA_HIP(hipGetLastError());
}

// The dense target as the caller describes it (device memory by now).
template <class T>
struct DenseX {
  const T* x = nullptr;
  int64_t rs = 0, cs = 0;
};

// The transform on the device.  `call`: the arrays as the caller gave them; x, rs, cs: the dense target as the caller gave it
// (an empty span: a CSR target); `stage`: the target, on the device by then, as the tall operand (never transposed).
template <class T, class Stage>
void transform(HipDev& dev, HostIo<HipDev>& io, const PcaTransformCall<T>& call, const Span& x, int64_t rs, int64_t cs, Stage&& stage,
               Ran* ran) {
  const int64_t m = call.m, n = call.n, k = call.k;
  const bool sparse = x.p == nullptr;
  PcaTransformCall<T> c = call;  // every array on the device
  c.means = io.in_aligned<T>(call.means_span());
  c.scales = io.in_aligned<T>(call.scales_span());
  c.comps = io.in_aligned<T>(call.comps_span());
  c.scores = io.out_packed<T>(call.scores_span(), &c.ld_scores);
  c.resid_out = io.out_packed<T>(call.resid_span());
  c.means_out = io.out_packed<T>(call.means_out_span());
  // x as it lies, so the device path's routes serve a host pointer unchanged
  const DenseX<T> dx{io.in_as_lies<T>(x), rs, cs};
  PcaApplyPlan rp;
  if (c.resid_out) {
    PcaApplyShape s;
    s.m = m, s.n = n, s.k = k;
    s.row_stride = dx.rs, s.col_stride = dx.cs;
    s.esz = (int)sizeof(T);
    s.base_aligned = (uintptr_t)dx.x % 16 == 0;
    s.mode = PcaApplyMode::kResid;
    rp = pca_apply_plan(s);
    if (rp.route == PcaApplyRoute::kReject) throw Error(ST_EINVAL, rp.error);
  }
  TallA<T> ta = stage(dx);
  RsvdDriver<HipDev, T> drv(dev, false);
  // V^T as the n x k skinny operand of the forward product; read row-wise it is V with unit stride along the features, which
  // is how the back-projection kernel stages it
  Skinny<T> vt = dev.template alloc_skinny<T>(n, k);
  dev.pack_strided(c.comps, k, n, (int64_t)1, c.ldc, vt.p, vt.ld);
  const T* mu = c.means;
  if (c.own_means()) {
    // the target's own column means, by the routine pca_body uses (the operand is never transposed here)
    const Skinny<T> mus = drv.column_means(ta, /*fat=*/false, m, /*sharded=*/false);
    mu = mus.p;
    if (c.means_out) dev.copy_values_out(mus.p, n, c.means_out, /*dst_is_host=*/false);
  }
  const T* inv_sd = nullptr;
  if (c.scales) {
    T* inv = (T*)dev.alloc_bytes((size_t)n * sizeof(T));
    hipLaunchKernelGGL((k::pca_reciprocal_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dev.stream, c.scales, n, inv);
    CORRLA_HIP(hipGetLastError());
    inv_sd = inv;
    if (!mu) mu = dev.template alloc_scalar<T>((int)n);  // scaling without centring: zero means
  }
  TallA<T> tc = ta;
  const int centring = !mu ? 0 : (sparse ? 1 : c.centring());
  if (centring == 1) {
    tc.mu_short = mu, tc.inv_sd_short = inv_sd;
    if (inv_sd) drv.set_scale_workspace(dev.template alloc_skinny<T>(n, k));
  } else if (centring == 2) {
    // centred and scaled copy of the staged operand (its memory rows are the samples iff it is row-major)
    const int64_t ldp = round_up(ta.mem.cols, kLdPad);
    T* cbuf = (T*)dev.alloc_bytes((size_t)ta.mem.rows * (size_t)ldp * sizeof(T));
    // only the padding columns need zeros (the copy kernel writes every other element): no pass over m x n for them
    if (ldp > ta.mem.cols)
      CORRLA_HIP(hipMemset2DAsync(cbuf + ta.mem.cols, (size_t)ldp * sizeof(T), 0, (size_t)(ldp - ta.mem.cols) * sizeof(T),
                                  (size_t)ta.mem.rows, dev.stream));
    dev.center_rows_cols(ta.mem.p, ta.mem.rows, ta.mem.cols, ta.mem.ld, mu, ta.row_major, cbuf, ldp, inv_sd);
    tc.mem.p = cbuf;
    tc.mem.ld = ldp;
    tc.mem.cols_readable = ldp;
  }
  Skinny<T> y = caller_skinny(c.scores, m, k, c.ld_scores);  // the scores land in the caller's buffer (or its image)
  drv.a_times(tc, vt, y, nullptr);
  ran->centring = centring;
  ran->route = 0;
  if (c.resid_out) {
    const T* xr = dx.x;
    if (rp.route == PcaApplyRoute::kRepacked) {
      T* packed = (T*)dev.alloc_bytes(rp.repack_bytes);
      dev.pack_strided(dx.x, m, n, dx.rs, dx.cs, packed, rp.ld);
      xr = packed;
    }
    back<T>(dev, rp, PcaApplyMode::kResid, c.scores, c.ld_scores, vt.p, vt.ld, mu, c.scales, m, n, k, const_cast<T*>(xr), c.resid_out);
    ran->route = (int)rp.route;
  }
  io.finish();
}

template <class T>
void run_dense(HipDev& dev, bool host_ptrs, const T* x, int64_t rs, int64_t cs, const PcaTransformCall<T>& c, Ran* ran) {
  validate_matrix(x, c.m, c.n, rs, cs);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  transform<T>(dev, io, c, Span(x, c.m, c.n, rs, cs, "x"), rs, cs, [&](const DenseX<T>& dx) {
    return stage_input<HipDev, T>(dev, false, dx.x, c.m, c.n, rs, cs, /*force_tall=*/true);
  }, ran);
}

template <class T>
void run_csr(HipDev& dev, bool host_ptrs, const T* values, const int32_t* ci, const int64_t* rp, int64_t nnz,
             const PcaTransformCall<T>& c, Ran* ran) {
  validate_csr_args(values, ci, rp, c.m, c.n, nnz);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  transform<T>(dev, io, c, Span(), 0, 0, [&](const DenseX<T>&) {
    return stage_csr<HipDev, T>(dev, host_ptrs, values, ci, rp, c.m, c.n, nnz, /*keep_orientation=*/true);
  }, ran);
}

template <class T>
void run_inverse(HipDev& dev, bool host_ptrs, const PcaInverseCall<T>& c, Ran* ran) {
  const int64_t m = c.m, n = c.n, k = c.k;
  PcaApplyShape s;
  s.m = m, s.n = n, s.k = k;
  s.row_stride = c.row_stride_out;
  s.col_stride = 1;
  s.esz = (int)sizeof(T);
  s.base_aligned = (uintptr_t)c.out % 16 == 0;
  s.mode = PcaApplyMode::kStore;
  const PcaApplyPlan p = pca_apply_plan(s);
  if (p.route == PcaApplyRoute::kReject) throw Error(ST_EINVAL, p.error);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  int64_t ldt;
  const T* td = io.in_packed<T>(c.scores_span(), &ldt);
  const T* md = io.in_aligned<T>(c.means_span());
  const T* sd = io.in_aligned<T>(c.scales_span());
  const T* cd = io.in_aligned<T>(c.comps_span());
  T* od = io.out_as_lies<T>(c.out_span());  // so the route is the one a device pointer of this layout takes
  // V with unit stride along the features (k rows, padded row stride): one small transposing copy
  const int64_t ldv = round_up(n, kLdPad);
  T* v = (T*)dev.alloc_bytes((size_t)k * (size_t)ldv * sizeof(T));
  dev.pack_strided(cd, k, n, (int64_t)1, c.ldc, v, ldv);
  back<T>(dev, p, PcaApplyMode::kStore, td, ldt, (const T*)v, ldv, md, sd, m, n, k, od, (T*)nullptr);
  ran->centring = 0;
  ran->route = (int)p.route;
  io.finish();
}

}  // namespace pca_apply_stage
}  // namespace corrla
