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
//
// The table form (dcor_subg_table_launch): k_subg_table_prep copies every column of a shared table
// to a 32-B aligned pitch and writes, for every column and every distinct m, the k batch means of
// the column clipped at its own lambda_n -- once per (column, m), not once per pair -- with
// k_subg_panel_prep's arithmetic (sgp_batch_means is the one loop); k_subg_table is k_subg_panel's
// shell with the segment's two columns and two mean rows taken from the segment table.  A
// replicate is subg_panel_item in both, templated on where a sample pair and a batch's two means
// come from, so its operation order is one piece of code.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dcor_common.h"
#include "dcor_segtab.h"

namespace dcor {

#define SGP_PREP_NT 256
#define SGP_PREP_MAXGRID 1024

// Batch j's means of NC columns, column c clipped at l[c]: the clipped samples added in index
// order, then sum * inv_md for m a power of two and sum / md otherwise (subg_fused_core's
// arithmetic).  A column's mean depends on that column alone.
template <int NC>
__device__ __forceinline__ void sgp_batch_means(const double* const (&col)[NC], const double (&l)[NC], int64_t j,
                                                int32_t m, int32_t pow2, double md, double inv_md,
                                                double (&mean)[NC]) {
  double s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  const int64_t i0 = j * m;   // samples j m .. j m + m - 1 < k m <= n
  for (int32_t r = 0; r < m; ++r) {
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] += rclip(col[c][i0 + r], l[c]);    // ver-cor-subG.R:33-34
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) mean[c] = pow2 ? s[c] * inv_md : s[c] / md;
}

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
    const double* const col[2] = {X, Y};
    const double l[2] = {l1, l2};
    for (int64_t j = gt; j < k; j += gs) {
      double mean[2];
      sgp_batch_means<2>(col, l, j, m, pow2, md, inv_md, mean);
      means[off + j] = make_double2(mean[0], mean[1]);
    }
  }
}

// The table's preparation, in tiles of SGP_PREP_NT consecutive values of one column taken at a
// stride of the grid (p is not a grid dimension).  The copy: column c of D (at D + c ld) to
// cols + c npad, zeros from n on.  The means: for every slot d, batch j of column c clipped at
// clips[c] to means[c mpitch + off_d + j] -- one thread owns a batch, the bits k_subg_panel_prep
// writes for that column on either side.  Every value has one writer; nothing depends on the grid.
__global__ __launch_bounds__(SGP_PREP_NT) void k_subg_table_prep(const double* __restrict__ D, int64_t ld,
                                                                 int64_t n, int64_t npad, int64_t p,
                                                                 const double* __restrict__ clips,
                                                                 const SubgMeanSlot* __restrict__ slots_g,
                                                                 int nslots, double* __restrict__ cols,
                                                                 double* __restrict__ means, int64_t mpitch) {
  const int64_t ct = (npad + SGP_PREP_NT - 1) / SGP_PREP_NT;
  for (int64_t t = blockIdx.x; t < p * ct; t += gridDim.x) {
    const int64_t c = t / ct, i = (t - c * ct) * SGP_PREP_NT + threadIdx.x;
    if (i < npad) cols[c * npad + i] = i < n ? D[c * ld + i] : 0.0;
  }
  const SegTab<SubgMeanSlot> slots = (SegTab<SubgMeanSlot>)slots_g;
  for (int d = 0; d < nslots; ++d) {
    const int64_t k = slots[d].k, off = slots[d].off;
    const int32_t m = slots[d].m, pow2 = slots[d].md_pow2;
    const double md = slots[d].md, inv_md = slots[d].inv_md;
    const int64_t kt = (k + SGP_PREP_NT - 1) / SGP_PREP_NT;
    for (int64_t t = blockIdx.x; t < p * kt; t += gridDim.x) {
      const int64_t c = t / kt, j = (t - c * kt) * SGP_PREP_NT + threadIdx.x;
      if (j >= k) continue;
      const double* const col[1] = {D + c * ld};
      const double l[1] = {clips[c]};
      double mean[1];
      sgp_batch_means<1>(col, l, j, m, pow2, md, inv_md, mean);
      means[c * mpitch + off + j] = mean[0];
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

// The batch means of the packed panel's entry: (X-bar_j, Y-bar_j) in one 16-byte read.
struct SubgPackedMeans {
  const double2* __restrict__ bm;
  __device__ __forceinline__ double2 at(uint32_t j) const { return bm[j]; }
};

// The table's loader: samples 2 q and 2 q + 1 as one 16-byte read from each of the pair's two
// columns (coalesced, 1 KB per wave-instruction and column; a column is padded with zeros to a
// multiple of 4 samples and starts 32-B aligned), and its means: batch j of the two columns' rows.
struct SubgColumnLoad {
  const double2* __restrict__ xa;
  const double2* __restrict__ yb;
  __device__ __forceinline__ void pair(uint32_t q, double2& a, double2& b) const {
    const double2 x = xa[q], y = yb[q];
    a = make_double2(x.x, y.x);
    b = make_double2(x.y, y.y);
  }
};
struct SubgColumnMeans {
  const double* __restrict__ mx;
  const double* __restrict__ my;
  __device__ __forceinline__ double2 at(uint32_t j) const { return make_double2(mx[j], my[j]); }
};

// The segment's fields over the call-wide ones in c (scalar loads: the address is uniform).
template <class Seg>
__device__ __forceinline__ void sgp_seg_load(SegTab<Seg> tab, int s, SubgConst& c) {
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
// as (x, y) (zeros past n); bm.at(j): batch j's two means at the segment's m; lt: the log table in
// LDS.
// A NaN sample is seen by the unordered compare, not by the clips (v_min / v_max drop it), and
// reaches the INT sums once, before the reduction; the NI side's NaN is in the prepared means.
template <bool WAVE, int VPL, class Load, class Means>
__device__ __forceinline__ void subg_panel_item(const SubgConst& c, uint32_t rep, Load load, Means bm,
                                                const double2* lt,
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
    const double2 mb = bm.at(j);
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
    subg_panel_item<WAVE, VPL>(c, rep, load, SubgPackedMeans{bm}, lds.lt, lds, out + out_row + (it - cur.first));
  }
}

// The same shell over a table's column pairs: the segment's columns (pitch doubles apart in cols)
// and their rows of batch means (mpitch doubles apart in means) change with the segment, read at
// wave-uniform addresses.  c holds n, nd, sqrt_n, crit and mix; everything else is the segment's.
// The waves per SIMD asked for are the panel kernels' (LDS-bound 2 and 3 in the wave forms): the
// four pointers of a pair must not cost the workgroup form its fourth wave.
template <bool WAVE, int VPL>
__global__ __launch_bounds__(DCOR_BLOCK, WAVE ? (VPL == 32 ? 2 : 3) : 4) void k_subg_table(SubgConst c,
                                                           const SubgPairSegConst* __restrict__ tab_g, int nseg,
                                                           int64_t items, const double* __restrict__ cols,
                                                           int64_t pitch, const double* __restrict__ means,
                                                           int64_t mpitch, dcor_rep_out* __restrict__ out) {
  __shared__ SgpLds<WAVE, VPL> lds;
  const SegTab<SubgPairSegConst> tab = (SegTab<SubgPairSegConst>)tab_g;
  log_tab_to_lds(lds.lt, DCOR_BLOCK);
  __syncthreads();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t unit = WAVE ? (int64_t)blockIdx.x * DCOR_WAVES + wv : (int64_t)blockIdx.x;
  const int64_t units = WAVE ? (int64_t)gridDim.x * DCOR_WAVES : (int64_t)gridDim.x;
  SubgColumnLoad load{nullptr, nullptr};
  SubgColumnMeans bm{nullptr, nullptr};
  SegCursor cur;
  int64_t out_row = 0;
  for (int64_t it = unit; it < items; it += units) {
    cur.seek(tab, nseg, items, it, [&](int s) {
      sgp_seg_load(tab, s, c);
      const int64_t a = tab[s].col_x, b = tab[s].col_y, off = tab[s].mean_off;
      load.xa = (const double2*)(cols + a * pitch);
      load.yb = (const double2*)(cols + b * pitch);
      bm.mx = means + a * mpitch + off;
      bm.my = means + b * mpitch + off;
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

int launch_subg_table(const SubgConst& c, const double* D, int64_t p, int64_t ld, const double* clips,
                      const SubgMeanSlot* slots, int nslots, double* means, int64_t mpitch, double* cols,
                      int64_t npad, const SubgPairSegConst* tab, int nseg, int64_t items, dcor_rep_out* out,
                      void* stream) {
  if (items <= 0 || nseg <= 0 || nslots <= 0 || p <= 0) return 0;
  const bool wave = c.n <= SUBG_W_NMAX;   // a function of n alone (as launch_subg_panel)
  const void* kern = wave ? (c.mix.nsim > 1024 ? (const void*)k_subg_table<true, 32>
                                               : (const void*)k_subg_table<true, 16>)
                          : (const void*)k_subg_table<false, 16>;
  int64_t grid = 0;
  const int64_t units = wave ? (items + DCOR_WAVES - 1) / DCOR_WAVES : items;
  if (int e = persistent_grid(kern, DCOR_BLOCK, 0, units, &grid)) return e;
  // the copy has the most tiles of the preparation's phases (k <= n)
  int64_t pg = p * ((npad + SGP_PREP_NT - 1) / SGP_PREP_NT);
  if (pg > SGP_PREP_MAXGRID) pg = SGP_PREP_MAXGRID;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_subg_table_prep, dim3((unsigned)pg), dim3(SGP_PREP_NT), 0, st, D, ld, c.n, npad, p, clips,
                     slots, nslots, cols, means, mpitch);
  const dim3 g((unsigned)grid), b(DCOR_BLOCK);
  const double *cc = cols, *cm = means;
  if (!wave)
    hipLaunchKernelGGL((k_subg_table<false, 16>), g, b, 0, st, c, tab, nseg, items, cc, npad, cm, mpitch, out);
  else if (c.mix.nsim > 1024)
    hipLaunchKernelGGL((k_subg_table<true, 32>), g, b, 0, st, c, tab, nseg, items, cc, npad, cm, mpitch, out);
  else
    hipLaunchKernelGGL((k_subg_table<true, 16>), g, b, 0, st, c, tab, nseg, items, cc, npad, cm, mpitch, out);
  return (int)hipGetLastError();
}

}  // namespace dcor
