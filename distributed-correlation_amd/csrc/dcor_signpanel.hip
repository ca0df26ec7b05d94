// dcor_signpanel.hip -- the sign family (ci_NI_signbatch + ci_INT_signflip, vert-cor.R:204-317) on
// a shared (X, Y) panel with every noise draw made inside the kernel (dcor_sign_panel_launch).
//
// Two launches per call.  k_sign_panel_prep (one workgroup, a fixed summation order) clips the
// panel at L = sqrt(2 log n), forms the four double-double sums of priv_standardize
// (vert-cor.R:328-340) and their means, and packs (xc, yc) as 16-byte pairs -- all of it the same
// for every replicate.  k_sign_panel runs the replicates: persistent workgroups of DCOR_BLOCK
// threads, one replicate per work item, the replicate's segment (eps pair, key, replicate range)
// found by binary search in a device table.  The draws are the fused engine's (include/dcor.h,
// "Draw-site contract") with the DGP samples replaced by the panel.
//
// Work split inside a replicate.  A thread takes whole flip blocks -- 4 consecutive samples, one
// 64-byte read of the packed panel, one Philox block of DCOR_SITE_FLIP -- at a stride of the
// workgroup, so the lanes are busy whatever the batch geometry (m = 2 .. 200 and beyond, k from 1)
// and every flip block is drawn once.  The samples' NI signs are summed per batch in LDS
// counters: a thread adds its run of consecutive samples of one batch with one LDS atomic (at
// most two per flip block for m >= 4; the adds are integers, so their order does not matter).
// Batches are taken SP_CAP at a time (the counters' LDS), then each batch's counts meet its
// DCOR_SITE_NI_LAP draw in one thread.  The INT flip sum is an integer per thread over all n.
//
// The table form (dcor_sign_table_launch): k_sign_table_prep is the same preparation with one
// workgroup per column of a shared table (sp_prep_columns is the one loop), the columns kept as
// plain doubles at a 32-B aligned pitch; k_sign_table is k_sign_panel's shell with the segment's
// two columns and four means taken from the segment table, a flip block read as two 32-byte loads.
// A replicate is sign_panel_item in both, so its operation order is one piece of code.
#include <hip/hip_runtime.h>

#include "dcor_common.h"
#include "dcor_segtab.h"

namespace dcor {

#define SP_PREP_NT 512
#define SP_PREP_UNR 4

// The preparation's loop over NC columns of n samples: a thread takes samples tid, tid + SP_PREP_NT,
// ... (SP_PREP_UNR loads in flight per column), clips them at L when normalise, adds xc and xc^2 of
// column c to v[2 c], v[2 c + 1] and hands the NC values of sample i < npad (zeros from n on) to
// store(i, xc).  A column's two sums depend on that column alone.
template <int NC, class Store>
__device__ __forceinline__ void sp_prep_columns(const double* const (&col)[NC], int64_t n, int64_t npad,
                                                int normalise, double L, DD (&v)[2 * NC], Store store) {
  const int tid = threadIdx.x;
  for (int64_t i0 = tid; i0 < npad; i0 += (int64_t)SP_PREP_NT * SP_PREP_UNR) {
    double x[NC][SP_PREP_UNR];
#pragma unroll
    for (int u = 0; u < SP_PREP_UNR; ++u) {   // every load of the trip first
      const int64_t i = i0 + (int64_t)u * SP_PREP_NT;
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c][u] = i < n ? col[c][i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < SP_PREP_UNR; ++u) {
      const int64_t i = i0 + (int64_t)u * SP_PREP_NT;
      if (i >= npad) break;
      double xc[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        xc[c] = x[c][u];
        if (normalise && i < n) {
          xc[c] = rclip(xc[c], L);
          dd_acc(v[2 * c], xc[c]); dd_acc(v[2 * c + 1], xc[c] * xc[c]);
        }
      }
      store(i, xc);   // i >= n: the zero padding of the last flip block
    }
  }
}

// means[q] = v[q] / n in double-double, rounded once (R: long-double mean); thread 0 only.
template <int NV>
__device__ __forceinline__ void sp_prep_means(const DD (&v)[NV], double nd, double* __restrict__ means) {
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const DD m = dd_div_d(v[q], nd);
    means[q] = m.hi + m.lo;
  }
}

__global__ __launch_bounds__(SP_PREP_NT) void k_sign_panel_prep(const double* __restrict__ X,
                                                                const double* __restrict__ Y,
                                                                int64_t n, int64_t npad, int normalise,
                                                                double L, double nd,
                                                                double2* __restrict__ xyc,
                                                                double* __restrict__ means) {
  __shared__ double red[8 * (SP_PREP_NT / 64)];
  DD v[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  const double* const col[2] = {X, Y};
  sp_prep_columns<2>(col, n, npad, normalise, L, v,
                     [&](int64_t i, const double (&xc)[2]) { xyc[i] = make_double2(xc[0], xc[1]); });
  block_sum_dd<4, SP_PREP_NT / 64>(v, red);
  if (threadIdx.x == 0) sp_prep_means<4>(v, nd, means);
}

// One workgroup per column c of the table D (column c at D + c ld): the column clipped (or raw,
// normalise = 0) to cols + c npad, its two means to means[2 c], means[2 c + 1] -- the bits
// k_sign_panel_prep writes for that column on either side (the same striding, unroll and
// block_sum_dd order; block_sum_dd folds each sum on its own).
__global__ __launch_bounds__(SP_PREP_NT) void k_sign_table_prep(const double* __restrict__ D, int64_t ld,
                                                                int64_t n, int64_t npad, int normalise,
                                                                double L, double nd,
                                                                double* __restrict__ cols,
                                                                double* __restrict__ means) {
  __shared__ double red[4 * (SP_PREP_NT / 64)];
  const int64_t c = blockIdx.x;
  DD v[2] = {{0, 0}, {0, 0}};
  const double* const col[1] = {D + c * ld};
  double* const dst = cols + c * npad;
  sp_prep_columns<1>(col, n, npad, normalise, L, v,
                     [&](int64_t i, const double (&xc)[1]) { dst[i] = xc[0]; });
  block_sum_dd<2, SP_PREP_NT / 64>(v, red);
  if (threadIdx.x == 0) sp_prep_means<2>(v, nd, means + 2 * c);
}

#define SP_CAP 4096   // LDS batch counters per pass (16 KB)
#define SP_PACK_M 32767  // up to this m a batch's two counts share one counter: cx + 65536 cy

// The fields of segment s the replicate uses (scalar loads: the address is workgroup-uniform).
template <class Seg>
__device__ __forceinline__ void sp_seg_load(SegTab<Seg> tab, int s, SignConst& c) {
  c.n = tab[s].s.n; c.k = tab[s].s.k; c.rep_begin = tab[s].s.rep_begin;
  c.k0 = tab[s].s.k0; c.k1 = tab[s].s.k1;
  c.m = tab[s].s.m; c.normalise = tab[s].s.normalise; c.mode_normal = tab[s].s.mode_normal;
  c.mix.nsim = tab[s].s.mix.nsim; c.mix.pos = tab[s].s.mix.pos; c.mix.P = tab[s].s.mix.P;
  c.nd = tab[s].s.nd; c.md = tab[s].s.md; c.kd = tab[s].s.kd;
  c.s_mu_x = tab[s].s.s_mu_x; c.s_m2_x = tab[s].s.s_m2_x;
  c.s_mu_y = tab[s].s.s_mu_y; c.s_m2_y = tab[s].s.s_m2_y;
  c.bx = tab[s].s.bx; c.by = tab[s].s.by;
  c.inv_k = tab[s].s.inv_k; c.crit = tab[s].s.crit; c.sqrt_k = tab[s].s.sqrt_k;
  c.flipT = tab[s].s.flipT;
  c.scale_Z = tab[s].s.scale_Z; c.coefZ = tab[s].s.coefZ; c.q2 = tab[s].s.q2;
  c.ratio = tab[s].s.ratio; c.eps_r = tab[s].s.eps_r; c.w_laplace = tab[s].s.w_laplace;
}

// The LDS of one workgroup of the replicate kernels.
struct SpLds {
  double red[16 * DCOR_WAVES];
  long long redi[DCOR_WAVES];
  double lap[10];
  SelScratch sel;
  int cnt[SP_CAP];   // all zero between items
};

// Replicate `rep` of the segment with constants c on the pair whose clipped means are mean0 .. 3
// (mean(xc), mean(xc^2), mean(yc), mean(yc^2)); load(g, v) gives flip block g's four (xc, yc).
template <class Load>
__device__ __forceinline__ void sign_panel_item(const SignConst& c, uint32_t rep, double mean0, double mean1,
                                                double mean2, double mean3, Load load, SpLds& lds,
                                                dcor_rep_out* dst) {
  const uint32_t tid = threadIdx.x;
  __syncthreads();   // the previous item's readers of lap and sel are done; cnt is all zero
  scalar_laplace(rep, c.k0, c.k1, lds.lap);
  __syncthreads();
  SignStd s;
  {
    double l8[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) l8[q] = lds.lap[q];
    priv_std_from_means(c, mean0, mean1, mean2, mean3, l8, s);   // vert-cor.R:335-344
  }
  const uint32_t n = (uint32_t)c.n, m = (uint32_t)c.m, k = (uint32_t)c.k;
  const uint32_t km = k * m;                     // <= n < 2^31
  const bool wide = m > SP_PACK_M;
  const uint32_t cap = wide ? SP_CAP / 2 : SP_CAP;
  // a thread's next flip block is 4 DCOR_BLOCK samples on: its batch and offset move by these
  const uint32_t dq = (4u * DCOR_BLOCK) / m, dr = (4u * DCOR_BLOCK) % m;
  bool bad_ni = false, bad_int = false;          // NaN seen by NI (first k*m) / INT (all n)
  DD sT{0, 0}, sT2{0, 0};
  int core = 0;                                  // |core| <= n / DCOR_BLOCK + 4 per thread
  auto flush = [&](uint32_t b, int cx, int cy) {
    if (wide) {
      atomicAdd(&lds.cnt[2 * b], cx);
      atomicAdd(&lds.cnt[2 * b + 1], cy);
    } else {
      atomicAdd(&lds.cnt[b], cx + 65536 * cy);
    }
  };
  for (uint32_t jb = 0; jb < k; jb += cap) {
    // batches [jb, je): samples [lo, hi); the last pass also takes the tail i >= k m (INT only)
    const uint32_t je = k - jb < cap ? k : jb + cap;
    const uint32_t lo = jb * m, hi = je == k ? n : je * m;
    const uint32_t gend = (hi + 3) >> 2;
    uint32_t g = (lo >> 2) + tid;
    uint32_t j = (4 * g) / m, r = 4 * g - j * m;  // batch and offset of sample 4 g
    for (; g < gend; g += DCOR_BLOCK) {
      const uint32_t i0 = 4 * g;
      double2 v[4];
      load(g, v);   // samples 4 g .. 4 g + 3: the panel is padded to whole blocks
      const U4 fw = draw(g, rep, DCOR_SITE_FLIP, c.k0, c.k1);
      int cx = 0, cy = 0;
      bool had = false;
      uint32_t jj = j, rr = r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t i = i0 + q;
        if (i >= lo && i < hi) {
          int nx, ny, ix, iy;
          bool b = false;
          if (c.normalise) {
            nx = sgn_std(v[q].x, s.muNx, s.sdNx, b);
            ny = sgn_std(v[q].y, s.muNy, s.sdNy, b);
            ix = sgn_std(v[q].x, s.muIx, s.sdIx, bad_int);
            iy = sgn_std(v[q].y, s.muIy, s.sdIy, bad_int);
          } else {
            nx = ix = sgn_raw(v[q].x, b);
            ny = iy = sgn_raw(v[q].y, b);
            bad_int |= b;
          }
          if (i < km) {
            cx += nx; cy += ny;
            bad_ni |= b;
            had = true;
          }
          core += FlipGen::of(fw, i, c.flipT) * ix * iy;
        }
        if (++rr == m) {   // sample i closes batch jj
          if (had) flush(jj - jb, cx, cy);
          cx = cy = 0;
          had = false;
          rr = 0;
          ++jj;
        }
      }
      if (had) flush(jj - jb, cx, cy);
      j += dq;
      r += dr;
      if (r >= m) { r -= m; ++j; }
    }
    __syncthreads();
    for (uint32_t t = tid; t < je - jb; t += DCOR_BLOCK) {
      int cx, cy;
      if (wide) {
        cx = lds.cnt[2 * t]; cy = lds.cnt[2 * t + 1];
        lds.cnt[2 * t] = 0; lds.cnt[2 * t + 1] = 0;
      } else {
        const int w = lds.cnt[t];
        lds.cnt[t] = 0;
        cx = (int)(int16_t)(w & 0xffff);
        cy = (w - cx) / 65536;
      }
      const U4 w4 = draw(jb + t, rep, DCOR_SITE_NI_LAP, c.k0, c.k1);
      const double xt = (double)cx / c.md + c.bx * unit_laplace(u53(w4.w0, w4.w1));
      const double yt = (double)cy / c.md + c.by * unit_laplace(u53(w4.w2, w4.w3));
      const double T = c.md * xt * yt;
      dd_acc(sT, T);
      dd_acc(sT2, T * T);
    }
    __syncthreads();
  }
  DD d2[2] = {sT, sT2};
  block_sum_dd<2>(d2, lds.red);
  const long long csum = block_sum_i((long long)core, lds.redi);
  const long long nbad = block_sum_i((bad_ni ? 1LL : 0LL) + (bad_int ? (1LL << 20) : 0LL), lds.redi);
  sign_finish(c, rep, d2[0], d2[1], csum, (nbad & 0xFFFFF) != 0, (nbad >> 20) != 0, lds.lap, &lds.sel, dst);
}

__global__ __launch_bounds__(DCOR_BLOCK) void k_sign_panel(const SignSegConst* __restrict__ tab_g,
                                                           int nseg, int64_t items,
                                                           const double2* __restrict__ xyc,
                                                           const double* __restrict__ means,
                                                           dcor_rep_out* __restrict__ out) {
  __shared__ SpLds lds;
  const SegTab<SignSegConst> tab = (SegTab<SignSegConst>)tab_g;
  for (uint32_t t = threadIdx.x; t < SP_CAP; t += DCOR_BLOCK) lds.cnt[t] = 0;
  const double mean0 = means[0], mean1 = means[1], mean2 = means[2], mean3 = means[3];
  SignConst c{};
  SegCursor cur;
  int64_t out_row = 0;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    cur.seek(tab, nseg, items, it, [&](int s) {
      sp_seg_load(tab, s, c);
      out_row = tab[s].out_row;
    });
    const uint32_t rep = (uint32_t)c.rep_begin + (uint32_t)(it - cur.first);
    sign_panel_item(c, rep, mean0, mean1, mean2, mean3,
                    [&](uint32_t g, double2 (&v)[4]) {   // one 64-byte read of the packed pairs
#pragma unroll
                      for (int q = 0; q < 4; ++q) v[q] = xyc[4 * g + q];
                    },
                    lds, out + out_row + (it - cur.first));
  }
}

// The same shell over a table's column pairs: the segment's columns (pitch doubles apart in cols)
// and their means change with the segment, read at workgroup-uniform addresses.
__global__ __launch_bounds__(DCOR_BLOCK) void k_sign_table(const SignPairSegConst* __restrict__ tab_g,
                                                           int nseg, int64_t items,
                                                           const double* __restrict__ cols, int64_t pitch,
                                                           const double* __restrict__ means,
                                                           dcor_rep_out* __restrict__ out) {
  __shared__ SpLds lds;
  const SegTab<SignPairSegConst> tab = (SegTab<SignPairSegConst>)tab_g;
  for (uint32_t t = threadIdx.x; t < SP_CAP; t += DCOR_BLOCK) lds.cnt[t] = 0;
  double mean0 = 0, mean1 = 0, mean2 = 0, mean3 = 0;
  const double4 *xa = nullptr, *yb = nullptr;   // the pair's columns, a flip block per element
  SignConst c{};
  SegCursor cur;
  int64_t out_row = 0;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    cur.seek(tab, nseg, items, it, [&](int s) {
      sp_seg_load(tab, s, c);
      out_row = tab[s].out_row;
      const int64_t a = tab[s].col_x, b = tab[s].col_y;
      xa = (const double4*)(cols + a * pitch);
      yb = (const double4*)(cols + b * pitch);
      mean0 = means[2 * a]; mean1 = means[2 * a + 1];
      mean2 = means[2 * b]; mean3 = means[2 * b + 1];
    });
    const uint32_t rep = (uint32_t)c.rep_begin + (uint32_t)(it - cur.first);
    sign_panel_item(c, rep, mean0, mean1, mean2, mean3,
                    [&](uint32_t g, double2 (&v)[4]) {   // two 32-byte reads, one per column
                      const double4 x = xa[g], y = yb[g];
                      v[0] = make_double2(x.x, y.x); v[1] = make_double2(x.y, y.y);
                      v[2] = make_double2(x.z, y.z); v[3] = make_double2(x.w, y.w);
                    },
                    lds, out + out_row + (it - cur.first));
  }
}

int launch_sign_panel(const SignConst& c, const double* X, const double* Y, double* means, void* xyc,
                      const SignSegConst* tab, int nseg, int64_t items, dcor_rep_out* out,
                      void* stream) {
  if (items <= 0 || nseg <= 0) return 0;
  const int64_t npad = (c.n + 3) & ~(int64_t)3;
  int64_t grid = 0;
  if (int e = persistent_grid((const void*)k_sign_panel, DCOR_BLOCK, 0, items, &grid)) return e;
  hipLaunchKernelGGL(k_sign_panel_prep, dim3(1), dim3(SP_PREP_NT), 0, (hipStream_t)stream, X, Y, c.n,
                     npad, c.normalise, c.L, c.nd, (double2*)xyc, means);
  hipLaunchKernelGGL(k_sign_panel, dim3((unsigned)grid), dim3(DCOR_BLOCK), 0, (hipStream_t)stream, tab,
                     nseg, items, (const double2*)xyc, (const double*)means, out);
  return (int)hipGetLastError();
}

int launch_sign_table(const SignConst& c, const double* D, int64_t p, int64_t ld, double* means,
                      double* cols, const SignPairSegConst* tab, int nseg, int64_t items,
                      dcor_rep_out* out, void* stream) {
  if (items <= 0 || nseg <= 0 || p <= 0) return 0;
  const int64_t npad = (c.n + 3) & ~(int64_t)3;
  int64_t grid = 0;
  if (int e = persistent_grid((const void*)k_sign_table, DCOR_BLOCK, 0, items, &grid)) return e;
  hipLaunchKernelGGL(k_sign_table_prep, dim3((unsigned)p), dim3(SP_PREP_NT), 0, (hipStream_t)stream, D, ld,
                     c.n, npad, c.normalise, c.L, c.nd, cols, means);
  hipLaunchKernelGGL(k_sign_table, dim3((unsigned)grid), dim3(DCOR_BLOCK), 0, (hipStream_t)stream, tab,
                     nseg, items, (const double*)cols, npad, (const double*)means, out);
  return (int)hipGetLastError();
}

}  // namespace dcor
