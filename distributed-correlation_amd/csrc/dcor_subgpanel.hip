// dcor_subgpanel.hip -- the sub-G simulation estimators (correlation_NI_subG + ci_INT_subG,
// ver-cor-subG.R:25-108) on a shared (X, Y) panel with every noise draw made inside the kernel
// (dcor_subg_panel_launch).
//
// Two launches per call.  k_subg_panel_prep packs the panel as (x, y) pairs and, for every distinct
// batch size m of the call, writes the k batch means of the clipped samples: the clips l1 / l2 do
// not depend on the data and the batches are contiguous, so a batch's two means are the same in
// every replicate (subg_fused_core's arithmetic: the clipped samples added in index order, then
// sum * inv_md for m a power of two and sum / md otherwise).  Every value has one writer and no
// sum crosses threads: no atomics, nothing depends on the grid.
// k_subg_panel runs the replicates: a persistent grid over the call's (segment, replicate) items,
// the replicate's segment (eps pair, key, replicate range) found by binary search in a device
// table.  A replicate is one workgroup for n > SUBG_W_NMAX and one wave otherwise -- a function of
// n alone, as in the fused engine, so a replicate's bits depend on nothing else.  The draws are the
// fused sub-G engine's (include/dcor.h, "Draw-site contract") with the DGP samples replaced by the
// panel; the NI result and the INT tail are the fused engine's own code (ni_subg_result,
// subg_int_finish).
//
// Work split inside a replicate.  INT: the threads stride over the packed panel two samples (one
// 32-byte read) at a time, one DCOR_SITE_DGP_B block and one table-driven log per sample.  NI: the
// threads stride over the k prepared batch means, one DCOR_SITE_NI_LAP block per batch.  The log
// table is read from LDS: a gather from global memory would wait behind the panel loads.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dcor_common.h"
#include "dcor_segtab.h"

namespace dcor {

#define SGP_PREP_NT 256
#define SGP_PREP_MAXGRID 1024

__global__ __launch_bounds__(SGP_PREP_NT) void k_subg_panel_prep(const double* __restrict__ X,
                                                                 const double* __restrict__ Y, int64_t n,
                                                                 int64_t npad, double l1, double l2,
                                                                 const SubgMeanSlot* __restrict__ slots_g,
                                                                 int nslots, double2* __restrict__ xy,
                                                                 double2* __restrict__ means) {
  const int64_t gt = (int64_t)blockIdx.x * SGP_PREP_NT + threadIdx.x;
  const int64_t gs = (int64_t)gridDim.x * SGP_PREP_NT;
  for (int64_t i = gt; i < npad; i += gs)   // i >= n: the zero padding of the last pair
    xy[i] = i < n ? make_double2(X[i], Y[i]) : make_double2(0.0, 0.0);
  const SegTab<SubgMeanSlot> slots = (SegTab<SubgMeanSlot>)slots_g;
  for (int d = 0; d < nslots; ++d) {
    const int64_t k = slots[d].k, off = slots[d].off;
    const int32_t m = slots[d].m, pow2 = slots[d].md_pow2;
    const double md = slots[d].md, inv_md = slots[d].inv_md;
    for (int64_t j = gt; j < k; j += gs) {   // batch j: samples j m .. j m + m - 1 < k m <= n
      double sx = 0.0, sy = 0.0;
      const int64_t i0 = j * m;
      for (int32_t r = 0; r < m; ++r) {
        sx += rclip(X[i0 + r], l1);                                      // ver-cor-subG.R:33
        sy += rclip(Y[i0 + r], l2);                                      // :34
      }
      means[off + j] = make_double2(pow2 ? sx * inv_md : sx / md, pow2 ? sy * inv_md : sy / md);
    }
  }
}

// The sample loader of the packed panel: samples 2 q and 2 q + 1 in one 32-byte read (the pack is
// padded with (0, 0) to a multiple of 4 samples and starts 256-B aligned).
struct SubgPackedLoad {
  const double2* __restrict__ xy;
  __device__ __forceinline__ void pair(uint32_t q, double2& a, double2& b) const {
    const double4 v = reinterpret_cast<const double4*>(xy)[q];
    a = make_double2(v.x, v.y);
    b = make_double2(v.z, v.w);
  }
};

// The segment's fields over the call-wide ones in c (scalar loads: the address is uniform).
__device__ __forceinline__ void sgp_seg_load(SegTab<SubgSegConst> tab, int s, SubgConst& c) {
  c.k = tab[s].k; c.m = tab[s].m; c.md_pow2 = tab[s].md_pow2; c.sender_is_X = tab[s].sender_is_X;
  c.md = tab[s].md; c.kd = tab[s].kd; c.inv_md = tab[s].inv_md;
  c.bx = tab[s].bx; c.by = tab[s].by; c.m_over_k = tab[s].m_over_k; c.sqrt_k = tab[s].sqrt_k;
  c.ls = tab[s].ls; c.lr = tab[s].lr; c.bs = tab[s].bs; c.s_central = tab[s].s_central;
  c.sn2x2 = tab[s].sn2x2; c.eps_r = tab[s].eps_r;
  c.k0 = tab[s].k0; c.k1 = tab[s].k1; c.rep_begin = tab[s].rep_begin;
}

// The LDS of one workgroup: the log table, and the epilogue's of a wave or workgroup replicate.
template <bool WAVE, int VPL> struct SgpLds;
template <int VPL> struct SgpLds<true, VPL> {
  double2 lt[256];
  WaveMix<VPL> ws[DCOR_WAVES];
};
template <int VPL> struct SgpLds<false, VPL> {
  double2 lt[256];
  double red[16 * DCOR_WAVES];
  SelScratch sel;
};

// Replicate `rep` of the segment with constants c.  load.pair(q, a, b) gives samples 2 q, 2 q + 1
// as (x, y) (zeros past n); bm: the k batch means of the segment's m; lt: the log table in LDS.
// A NaN sample is seen by the unordered compare, not by the clips (v_min / v_max drop it), and
// reaches the INT sums once, before the reduction; the NI side's NaN is in the prepared means.
template <bool WAVE, int VPL, class Load>
__device__ __forceinline__ void subg_panel_item(const SubgConst& c, uint32_t rep, Load load,
                                                const double2* __restrict__ bm, const double2* lt,
                                                SgpLds<WAVE, VPL>& lds, dcor_rep_out* dst) {
  constexpr uint32_t NT = WAVE ? 64 : DCOR_BLOCK;
  const uint32_t tid = WAVE ? (threadIdx.x & 63u) : threadIdx.x;
  const uint32_t npairs = ((uint32_t)c.n + 1u) >> 1, k = (uint32_t)c.k;
  DD sP{0, 0}, sT{0, 0}, sT2{0, 0}, sU{0, 0}, sU2{0, 0};
  bool bad = false;
  // INT: Uc = clip((clip(S, ls) + bs L) O, lr) (ver-cor-subG.R:88-90); two samples' terms added
  // plainly and the pair sum compensated (subg_fused_core's int_term2).  SX: the sender is X.
  auto int_stream = [&](auto SX) {
    for (uint32_t q = tid; q < npairs; q += NT) {
      double2 a, b;
      load.pair(q, a, b);
      const U4 w0 = draw(2u * q, rep, DCOR_SITE_DGP_B, c.k0, c.k1);
      const U4 w1 = draw(2u * q + 1u, rep, DCOR_SITE_DGP_B, c.k0, c.k1);
      const double l0 = unit_laplace_t(u53(w0.w2, w0.w3), lt);
      const double l1 = unit_laplace_t(u53(w1.w2, w1.w3), lt);
      bad |= __builtin_isunordered(a.x, a.y) | __builtin_isunordered(b.x, b.y);
      const double S0 = decltype(SX)::value ? a.x : a.y, O0 = decltype(SX)::value ? a.y : a.x;
      const double S1 = decltype(SX)::value ? b.x : b.y, O1 = decltype(SX)::value ? b.y : b.x;
      const double U0 = rclip_fin((rclip_fin(S0, c.ls) + c.bs * l0) * O0, c.lr);
      const double U1 = rclip_fin((rclip_fin(S1, c.ls) + c.bs * l1) * O1, c.lr);
      ks_acc(sU, U0 + U1);
      ks_acc(sU2, U0 * U0 + U1 * U1);
    }
  };
  if (c.sender_is_X) int_stream(std::true_type{}); else int_stream(std::false_type{});
  // NI: batch j's prepared means meet its Laplace pair (:48-55)
  for (uint32_t j = tid; j < k; j += NT) {
    const double2 mb = bm[j];
    const U4 w = draw(j, rep, DCOR_SITE_NI_LAP, c.k0, c.k1);
    const double xt = mb.x + c.bx * unit_laplace_t(u53(w.w0, w.w1), lt);   // :48
    const double yt = mb.y + c.by * unit_laplace_t(u53(w.w2, w.w3), lt);   // :49
    ks_acc(sP, xt * yt);
    const double T = c.md * xt * yt;                                      // :55
    ks_acc(sT, T);
    ks_acc(sT2, T * T);
  }
  if (bad) sU.hi = dnan();   // a NaN anywhere: the INT columns are NaN
  DD d5[5] = {sP, sT, sT2, sU, sU2};
  if constexpr (WAVE) {
#pragma unroll
    for (int q = 0; q < 5; ++q) d5[q] = wave_sum_dd(d5[q]);
  } else {
    block_sum_dd<5>(d5, lds.red);
  }
  double o[6];
  ni_subg_result(c, d5[0], d5[1], d5[2], o);
  const U4 wz = draw(4u, rep, DCOR_SITE_SCALAR, c.k0, c.k1);   // uniform: every thread draws it
  const double lapz = unit_laplace(u53(wz.w0, wz.w1));
  if constexpr (WAVE)
    subg_int_finish<true, VPL>(c, rep, d5[3], d5[4], lapz, nullptr, &lds.ws[threadIdx.x >> 6], o);
  else
    subg_int_finish<false, VPL>(c, rep, d5[3], d5[4], lapz, &lds.sel, (WaveMix<VPL>*)nullptr, o);
  if (tid == 0) *dst = dcor_rep_out{o[0], o[1], o[2], o[3], o[4], o[5]};
}

// Work unit u of the launch (a workgroup, or a wave with WAVE) takes items u, u + units, ...: its
// items ascend, so the table is re-read once per segment entered.
template <bool WAVE, int VPL>
__global__ __launch_bounds__(DCOR_BLOCK) void k_subg_panel(SubgConst c,
                                                           const SubgSegConst* __restrict__ tab_g, int nseg,
                                                           int64_t items, const double2* __restrict__ xy,
                                                           const double2* __restrict__ means,
                                                           dcor_rep_out* __restrict__ out) {
  __shared__ SgpLds<WAVE, VPL> lds;
  const SegTab<SubgSegConst> tab = (SegTab<SubgSegConst>)tab_g;
  log_tab_to_lds(lds.lt, DCOR_BLOCK);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t unit = WAVE ? (int64_t)blockIdx.x * DCOR_WAVES + wv : (int64_t)blockIdx.x;
  const int64_t units = WAVE ? (int64_t)gridDim.x * DCOR_WAVES : (int64_t)gridDim.x;
  const SubgPackedLoad load{xy};
  const double2* bm = means;
  SegCursor cur;
  int64_t out_row = 0;
  for (int64_t it = unit; it < items; it += units) {
    cur.seek(tab, nseg, items, it, [&](int s) {
      sgp_seg_load(tab, s, c);
      bm = means + tab[s].mean_off;
      out_row = tab[s].out_row;
    });
    // the previous item's readers of the epilogue's LDS are done
    if constexpr (WAVE) wave_sync(); else __syncthreads();
    const uint32_t rep = (uint32_t)c.rep_begin + (uint32_t)(it - cur.first);
    subg_panel_item<WAVE, VPL>(c, rep, load, bm, lds.lt, lds, out + out_row + (it - cur.first));
  }
}

int launch_subg_panel(const SubgConst& c, const double* X, const double* Y, const SubgMeanSlot* slots,
                      int nslots, double2* means, double2* xy, int64_t npad, const SubgSegConst* tab,
                      int nseg, int64_t items, dcor_rep_out* out, void* stream) {
  if (items <= 0 || nseg <= 0 || nslots <= 0) return 0;
  const bool wave = c.n <= SUBG_W_NMAX;   // a function of n alone (as launch_subg_fused)
  const void* kern = wave ? (c.mix.nsim > 1024 ? (const void*)k_subg_panel<true, 32>
                                               : (const void*)k_subg_panel<true, 16>)
                          : (const void*)k_subg_panel<false, 16>;
  int64_t grid = 0;
  const int64_t units = wave ? (items + DCOR_WAVES - 1) / DCOR_WAVES : items;
  if (int e = persistent_grid(kern, DCOR_BLOCK, 0, units, &grid)) return e;
  int64_t pg = (npad + SGP_PREP_NT - 1) / SGP_PREP_NT;
  if (pg > SGP_PREP_MAXGRID) pg = SGP_PREP_MAXGRID;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_subg_panel_prep, dim3((unsigned)pg), dim3(SGP_PREP_NT), 0, st, X, Y, c.n, npad, c.l1,
                     c.l2, slots, nslots, xy, means);
  const dim3 g((unsigned)grid), b(DCOR_BLOCK);
  if (!wave)
    hipLaunchKernelGGL((k_subg_panel<false, 16>), g, b, 0, st, c, tab, nseg, items, (const double2*)xy,
                       (const double2*)means, out);
  else if (c.mix.nsim > 1024)
    hipLaunchKernelGGL((k_subg_panel<true, 32>), g, b, 0, st, c, tab, nseg, items, (const double2*)xy,
                       (const double2*)means, out);
  else
    hipLaunchKernelGGL((k_subg_panel<true, 16>), g, b, 0, st, c, tab, nseg, items, (const double2*)xy,
                       (const double2*)means, out);
  return (int)hipGetLastError();
}

}  // namespace dcor
