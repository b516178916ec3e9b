// The thin-Q orthonormalisation on the device (random_svd.rs:38,57): one launcher per kernel family of cholqr_kernels.hpp
// (plain and robust factor-and-invert, gram_inspect, combine_need, refill_null, the inverse-square-root series) and of
// tsqr_kernels.hpp (the Householder up sweep and down sweep).  thinq_plan.hpp has decided the route of every width, the
// threads and LDS of each launch, the panel tree and its buffer sizes; a launcher allocates what the plan sized, fills the
// kernel's arguments and launches.  The HipDev members driver.hpp calls are defined at the end.
#pragma once
#include "cholqr_kernels.hpp"
#include "hip_backend.hpp"
#include "thinq_plan.hpp"
#include "tsqr_kernels.hpp"

namespace corrla {
namespace thinq_stage {

// every kernel of the stage launched with more dynamic LDS than the default (HipDev::set_lds_limits_typed)
template <class T>
inline void set_lds_limits() {
  lds_limit((const void*)k::hh_leaf_factor_kernel<T>, k::kLdsMaxBytes);
  lds_limit((const void*)k::hh_tree_factor_kernel<T>, k::kLdsMaxBytes);
  lds_limit((const void*)k::hh_tree_apply_kernel<T>, k::kLdsMaxBytes);
  lds_limit((const void*)k::hh_leaf_apply_kernel<T>, k::kLdsMaxBytes);
}

// ---- factor-and-invert of one r x r (diagonal block of a) Gram: plain, or robust with rq.need_next set ----
// m_out comes zero-filled from alloc_skinny and only its upper triangle is ever written
template <class T>
inline void chol_inv(HipDev& dev, const Skinny<T>& g, int64_t r, T piv_rel, Skinny<T>& m_out, k::CholStatus* st) {
  const CholInvLaunch p = chol_inv_launch((int)r, sizeof(T));
  hipLaunchKernelGGL((k::chol_inv_kernel<T>), dim3(1), dim3(p.threads), p.lds, dev.stream, (const T*)g.p, g.ld, p.n, piv_rel, m_out.p,
                     m_out.ld, st);
  CORRLA_HIP(hipGetLastError());
}
template <class T>
inline void chol_inv_robust(HipDev& dev, const Skinny<T>& g, int64_t r, T piv_rel, Skinny<T>& m_out, k::CholStatus* st,
                            const k::CholRobust& rb) {
  const CholInvLaunch p = chol_inv_launch((int)r, sizeof(T));
  hipLaunchKernelGGL((k::chol_inv_kernel<T>), dim3(1), dim3(p.threads), p.lds, dev.stream, (const T*)g.p, g.ld, p.n, piv_rel, m_out.p,
                     m_out.ld, st, rb);
  CORRLA_HIP(hipGetLastError());
}
// 2 x 2 blocked robust factorisation: the whole Gram is inspected (shift decision, ||G - I||) and shifted once, the two
// diagonal-block factorisations take the shift from the record, combine_need forms the pass verdict
template <class T>
inline void gram_inspect(HipDev& dev, const int* run_if, Skinny<T>& g, int64_t l, float shift_rel, int shift_mode, k::GramInspect<T>* insp) {
  hipLaunchKernelGGL((k::gram_inspect_kernel<T>), dim3(1), dim3(1024), 0, dev.stream, g.p, g.ld, (int)l, shift_rel, shift_mode, insp,
                     run_if);
  CORRLA_HIP(hipGetLastError());
}
template <class T>
inline void combine_need(HipDev& dev, const int* run_if, int* need, const k::GramInspect<T>* insp, const int* na, const int* nb) {
  hipLaunchKernelGGL((k::combine_need_kernel<T>), dim3(1), dim3(1), 0, dev.stream, need, insp, na, nb, run_if);
  CORRLA_HIP(hipGetLastError());
}
template <class T>
inline void refill_null(HipDev& dev, const int* run_if, Skinny<T>& y, int64_t l, const int* null_mask, uint64_t seed) {
  const Grid2 g = refill_null_grid(y.rows, l);
  hipLaunchKernelGGL((k::refill_null_kernel<T>), dim3(g.x, g.y), dim3(g.block), 0, dev.stream, y.p, y.ld, y.rows, (int)l, null_mask, seed,
                     run_if);
  CORRLA_HIP(hipGetLastError());
}

// m_out (r x r) = (I + E)^(-1/2) with G = I + E given in g (overwritten by E); everything on the device
template <class T>
inline void inv_sqrt_series(HipDev& dev, Skinny<T>& g, int64_t r, Skinny<T>& m_out) {
  Skinny<T> e2 = dev.alloc_skinny<T>(r, r), e3 = dev.alloc_skinny<T>(r, r);
  if (e2.ld != g.ld || m_out.ld != g.ld) throw Error(ST_EINVAL, "internal: series operands must share a leading dimension");
  const Grid2 gr = series_grid(r);
  hipLaunchKernelGGL((k::series_prep_kernel<T>), dim3(gr.x, gr.y), dim3(gr.block), 0, dev.stream, g.p, g.ld, (int)r);
  Big<T> eb;  // E is symmetric: its column-major image is also its row-major image
  eb.p = g.p;
  eb.rows = r;
  eb.cols = r;
  eb.ld = g.ld;
  eb.cols_readable = g.ld;
  Skinny<T> gv = g.view_cols(r);
  gv.rows = r;
  dev.gemm_nn(eb, gv, e2, (const T*)nullptr);
  dev.gemm_nn(eb, e2, e3, (const T*)nullptr);
  dev.memset_zero(m_out.p, (size_t)m_out.ld * m_out.cols_alloc * sizeof(T));
  hipLaunchKernelGGL((k::series_combine_kernel<T>), dim3(gr.x, gr.y), dim3(gr.block), 0, dev.stream, (const T*)g.p, (const T*)e2.p,
                     (const T*)e3.p, g.ld, (int)r, m_out.p, m_out.ld);
  CORRLA_HIP(hipGetLastError());
}

// ---- Householder TSQR with explicit thin Q (tsqr_kernels.hpp) ----
// Up sweep of the TSQR of y (m x l, m >= l): leaf reflectors -> tmp (same shape as y), tree reflectors and the root's
// R factor (l x l, column-major, ld = l) stay in call-lifetime device buffers named by the returned state.
template <class T>
inline HipDev::HhState<T> householder_up(HipDev& dev, Skinny<T>& y, Skinny<T>& tmp) {
  HipDev::HhState<T> h;
  const HhTreePlan p = hh_tree_plan(sizeof(T), y.rows, y.cols);
  if (p.error) throw Error(ST_EINVAL, p.error);
  const int l = (int)y.cols;
  h.m = y.rows;
  h.l = l;
  h.plan = p;
  h.rbuf.resize(p.levels + 1);
  h.cbuf.resize(p.levels + 1);
  h.taub.resize(p.levels + 1);
  h.vbuf.assign(p.levels + 1, nullptr);
  h.tbuf.resize(p.levels + 1);
  for (int k_ = 0; k_ <= p.levels; ++k_) {
    h.tbuf[k_] = (T*)dev.alloc_bytes(p.t_elems[k_] * sizeof(T));
    h.rbuf[k_] = (T*)dev.alloc_bytes(p.r_elems[k_] * sizeof(T));
    h.cbuf[k_] = (T*)dev.alloc_bytes(p.c_elems[k_] * sizeof(T));
    h.taub[k_] = (T*)dev.alloc_bytes(p.tau_elems[k_] * sizeof(T));
    if (k_ >= 1) h.vbuf[k_] = (T*)dev.alloc_bytes(p.v_elems[k_] * sizeof(T));
  }
  hipLaunchKernelGGL((k::hh_leaf_factor_kernel<T>), dim3((unsigned)p.nleaf), dim3(k::kHhThreads), p.lds_up_leaf, dev.stream, (const T*)y.p,
                     y.ld, h.m, l, p.nleaf, tmp.p, tmp.ld, h.taub[0], h.rbuf[0], h.tbuf[0]);
  for (int k_ = 1; k_ <= p.levels; ++k_)
    hipLaunchKernelGGL((k::hh_tree_factor_kernel<T>), dim3((unsigned)p.n_at[k_]), dim3(k::kHhThreads), p.lds_up_tree, dev.stream,
                       (const T*)h.rbuf[k_ - 1], p.n_at[k_ - 1], l, h.vbuf[k_], h.taub[k_], h.rbuf[k_], h.tbuf[k_]);
  CORRLA_HIP(hipGetLastError());
  return h;
}
// Down sweep: y <- Q [C; 0] with Q the orthogonal factor of the up sweep and C = root_coef (l x l, column-major,
// ld = l; nullptr = the identity, i.e. y <- the explicit thin Q).
template <class T>
inline void householder_down(HipDev& dev, HipDev::HhState<T>& h, Skinny<T>& y, Skinny<T>& tmp, const T* root_coef) {
  const HhTreePlan& p = h.plan;
  const int l = h.l;
  for (int k_ = p.levels; k_ >= 1; --k_)
    hipLaunchKernelGGL((k::hh_tree_apply_kernel<T>), dim3((unsigned)p.n_at[k_]), dim3(k::kHhThreads), p.lds_down_tree, dev.stream,
                       (const T*)(k_ == p.levels ? root_coef : h.cbuf[k_]), (const T*)h.vbuf[k_], (const T*)h.taub[k_],
                       p.n_at[k_ - 1], l, h.cbuf[k_ - 1], (const T*)h.tbuf[k_]);
  hipLaunchKernelGGL((k::hh_leaf_apply_kernel<T>), dim3((unsigned)p.nleaf), dim3(k::kHhThreads), p.lds_down_leaf, dev.stream,
                     (const T*)(p.levels == 0 ? root_coef : h.cbuf[0]), (const T*)tmp.p, tmp.ld, (const T*)h.taub[0], h.m, l,
                     p.nleaf, y.p, y.ld, (const T*)h.tbuf[0]);
  CORRLA_HIP(hipGetLastError());
}

}  // namespace thinq_stage

// ---- the members of the Dev interface (driver.hpp) ----
template <class T>
void HipDev::chol_inv(const Skinny<T>& g, int64_t r, T piv_rel, Skinny<T>& m_out, void* st_dev, int slot) {
  thinq_stage::chol_inv(*this, g, r, piv_rel, m_out, (k::CholStatus*)st_dev + slot);
}
template <class T>
void HipDev::chol_inv_robust(const Skinny<T>& g, int64_t r, T piv_rel, float shift_rel, int shift_mode, float null_excess,
                             Skinny<T>& m_out, void* st_dev, int slot, int* need_next, int* null_mask, const void* abs_shift,
                             float need_ratio) {
  const k::CholRobust rb{shift_rel, shift_mode, null_excess, need_next, null_mask, run_if_, need_ratio, abs_shift};
  thinq_stage::chol_inv_robust(*this, g, r, piv_rel, m_out, (k::CholStatus*)st_dev + slot, rb);
}
template <class T>
void* HipDev::alloc_inspect() {
  return alloc_zeroed(sizeof(k::GramInspect<T>));
}
template <class T>
const void* HipDev::inspect_shift_ptr(const void* insp) const {
  return &((const k::GramInspect<T>*)insp)->shift;
}
template <class T>
void HipDev::gram_inspect(Skinny<T>& g, int64_t l, float shift_rel, int shift_mode, void* insp) {
  thinq_stage::gram_inspect(*this, run_if_, g, l, shift_rel, shift_mode, (k::GramInspect<T>*)insp);
}
template <class T>
void HipDev::combine_need(int* need, const void* insp, const int* na, const int* nb) {
  thinq_stage::combine_need<T>(*this, run_if_, need, (const k::GramInspect<T>*)insp, na, nb);
}
template <class T>
void HipDev::refill_null(Skinny<T>& y, int64_t l, const int* null_mask, uint64_t seed) {
  thinq_stage::refill_null(*this, run_if_, y, l, null_mask, seed);
}
template <class T>
void HipDev::inv_sqrt_series(Skinny<T>& g, int64_t r, Skinny<T>& m_out) {
  thinq_stage::inv_sqrt_series(*this, g, r, m_out);
}
template <class T>
HipDev::HhState<T> HipDev::householder_up(Skinny<T>& y, Skinny<T>& tmp) {
  return thinq_stage::householder_up(*this, y, tmp);
}
template <class T>
void HipDev::householder_down(HhState<T>& h, Skinny<T>& y, Skinny<T>& tmp, const T* root_coef) {
  thinq_stage::householder_down(*this, h, y, tmp, root_coef);
}

}  // namespace corrla
