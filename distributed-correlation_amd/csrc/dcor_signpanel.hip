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
#include <hip/hip_runtime.h>

#include "dcor_common.h"

namespace dcor {

#define SP_PREP_NT 512
#define SP_PREP_UNR 4

__global__ __launch_bounds__(SP_PREP_NT) void k_sign_panel_prep(const double* __restrict__ X,
                                                                const double* __restrict__ Y,
                                                                int64_t n, int64_t npad, int normalise,
                                                                double L, double nd,
                                                                double2* __restrict__ xyc,
                                                                double* __restrict__ means) {
  __shared__ double red[8 * (SP_PREP_NT / 64)];
  const int tid = threadIdx.x;
  DD v[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  for (int64_t i0 = tid; i0 < npad; i0 += (int64_t)SP_PREP_NT * SP_PREP_UNR) {
    double x[SP_PREP_UNR], y[SP_PREP_UNR];
#pragma unroll
    for (int u = 0; u < SP_PREP_UNR; ++u) {   // every load of the trip first
      const int64_t i = i0 + (int64_t)u * SP_PREP_NT;
      x[u] = i < n ? X[i] : 0.0;
      y[u] = i < n ? Y[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < SP_PREP_UNR; ++u) {
      const int64_t i = i0 + (int64_t)u * SP_PREP_NT;
      if (i >= npad) break;
      double xc = x[u], yc = y[u];
      if (normalise && i < n) {
        xc = rclip(xc, L); yc = rclip(yc, L);
        dd_acc(v[0], xc); dd_acc(v[1], xc * xc); dd_acc(v[2], yc); dd_acc(v[3], yc * yc);
      }
      xyc[i] = make_double2(xc, yc);   // i >= n: the zero padding of the last flip block
    }
  }
  block_sum_dd<4, SP_PREP_NT / 64>(v, red);
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // R: long-double mean
      const DD m = dd_div_d(v[q], nd);
      means[q] = m.hi + m.lo;
    }
  }
}

#define SP_CAP 4096   // LDS batch counters per pass (16 KB)
#define SP_PACK_M 32767  // up to this m a batch's two counts share one counter: cx + 65536 cy

typedef const __attribute__((address_space(4))) SignSegConst* SignSegTab;

// The last segment whose first item is <= it (`first` is strictly increasing, tab[0].first = 0).
__device__ __forceinline__ int sp_seg_find(SignSegTab tab, int nseg, int64_t it) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= it) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The fields of segment s the replicate uses (scalar loads: the address is workgroup-uniform).
__device__ __forceinline__ void sp_seg_load(SignSegTab tab, int s, SignConst& c) {
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

__global__ __launch_bounds__(DCOR_BLOCK) void k_sign_panel(const SignSegConst* __restrict__ tab_g,
                                                           int nseg, int64_t items,
                                                           const double2* __restrict__ xyc,
                                                           const double* __restrict__ means,
                                                           dcor_rep_out* __restrict__ out) {
  __shared__ double red[16 * DCOR_WAVES];
  __shared__ long long redi[DCOR_WAVES];
  __shared__ double lap[10];
  __shared__ SelScratch sel;
  __shared__ int cnt[SP_CAP];
  const SignSegTab tab = (SignSegTab)tab_g;
  const uint32_t tid = threadIdx.x;
  for (uint32_t t = tid; t < SP_CAP; t += DCOR_BLOCK) cnt[t] = 0;
  const double mean0 = means[0], mean1 = means[1], mean2 = means[2], mean3 = means[3];
  SignConst c{};
  int64_t first = 0, end = 0, out_row = 0;   // items [first, end) belong to the loaded segment
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    if (it >= end) {   // a workgroup's items ascend: the table is re-read once per segment entered
      const int s = __builtin_amdgcn_readfirstlane(sp_seg_find(tab, nseg, it));
      sp_seg_load(tab, s, c);
      first = tab[s].first;
      out_row = tab[s].out_row;
      end = s + 1 < nseg ? tab[s + 1].first : items;
    }
    const uint32_t rep = (uint32_t)c.rep_begin + (uint32_t)(it - first);
    __syncthreads();   // the previous item's readers of lap and sel are done; cnt is all zero
    scalar_laplace(rep, c.k0, c.k1, lap);
    __syncthreads();
    SignStd s;
    {
      double l8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) l8[q] = lap[q];
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
        atomicAdd(&cnt[2 * b], cx);
        atomicAdd(&cnt[2 * b + 1], cy);
      } else {
        atomicAdd(&cnt[b], cx + 65536 * cy);
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
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xyc[i0 + q];   // the panel is padded to whole blocks
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
          cx = cnt[2 * t]; cy = cnt[2 * t + 1];
          cnt[2 * t] = 0; cnt[2 * t + 1] = 0;
        } else {
          const int w = cnt[t];
          cnt[t] = 0;
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
    block_sum_dd<2>(d2, red);
    const long long csum = block_sum_i((long long)core, redi);
    const long long nbad = block_sum_i((bad_ni ? 1LL : 0LL) + (bad_int ? (1LL << 20) : 0LL), redi);
    sign_finish(c, rep, d2[0], d2[1], csum, (nbad & 0xFFFFF) != 0, (nbad >> 20) != 0, lap, &sel,
                out + out_row + (it - first));
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

}  // namespace dcor
