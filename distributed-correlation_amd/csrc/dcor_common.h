// dcor_common.h -- device helpers shared by the fused and pre-materialised kernels:
// R-exact sign of a standardised value, mixquant order statistic from loaded draws, and
// the NI / INT epilogues of both estimator families (cited R lines inline).
#pragma once
#include "dcor_device.h"
#include "dcor_engine.h"

namespace dcor {

// sign((a - mu)/sd) exactly as R computes it (sd > 0): the quotient has the sign of
// the numerator unless it underflows, which needs |a - mu| < sd * 2^-1000.
__device__ __forceinline__ int sgn_std(double a, double mu, double sd, bool& bad) {
  const double d = a - mu;
  if (fabs(d) >= sd * 0x1p-1000) return (d > 0) - (d < 0);
  const double q = d / sd;
  bad |= (q != q);
  return (q > 0) - (q < 0);
}
__device__ __forceinline__ int sgn_raw(double a, bool& bad) {
  bad |= (a != a);
  return (a > 0) - (a < 0);
}

// mixquant over keys already in registers: zv[s], lv[s] = z[i], l[i] for i = tid + s*DCOR_BLOCK
// (a caller can issue these loads before c is known).
__device__ __forceinline__ double mixquant_regs(const MixConst& mx, double c,
                                                const double (&zv)[SEL_VPT],
                                                const double (&lv)[SEL_VPT], SelScratch* sc) {
  if (threadIdx.x == 0) sc->nan_cnt = 0;
  __syncthreads();
  double val[SEL_VPT];
  int nn = 0;
#pragma unroll
  for (int s = 0; s < SEL_VPT; ++s) {
    const int i = threadIdx.x + s * DCOR_BLOCK;
    val[s] = dnan();
    if (i < mx.nsim) {
      val[s] = zv[s] + c * lv[s];
      nn += (val[s] != val[s]);
    }
  }
  if (nn) atomicAdd(&sc->nan_cnt, nn);
  __syncthreads();
  return value_select(val, mx.pos, mx.nsim - sc->nan_cnt, sc);
}

__device__ __forceinline__ void mixquant_prefetch(const MixConst& mx, const double* z,
                                                  const double* l, double (&zv)[SEL_VPT],
                                                  double (&lv)[SEL_VPT]) {
#pragma unroll
  for (int s = 0; s < SEL_VPT; ++s) {
    const int i = threadIdx.x + s * DCOR_BLOCK;
    zv[s] = i < mx.nsim ? z[i] : 0.0;
    lv[s] = i < mx.nsim ? l[i] : 0.0;
  }
}

__device__ __forceinline__ double mixquant_loaded(const MixConst& mx, double c, const double* z,
                                                  const double* l, SelScratch* sc) {
  if (threadIdx.x == 0) sc->nan_cnt = 0;
  __syncthreads();
  double val[SEL_VPT];
  int nn = 0;
#pragma unroll
  for (int s = 0; s < SEL_VPT; ++s) {
    const int i = threadIdx.x + s * DCOR_BLOCK;
    val[s] = dnan();
    if (i < mx.nsim) {
      val[s] = z[i] + c * l[i];
      nn += (val[s] != val[s]);
    }
  }
  if (nn) atomicAdd(&sc->nan_cnt, nn);
  __syncthreads();
  return value_select(val, mx.pos, mx.nsim - sc->nan_cnt, sc);
}

#define MIX_MAX 2048

// ------------------------------------------------- sign-family epilogues
struct SignStd { double muNx, sdNx, muNy, sdNy, muIx, sdIx, muIy, sdIy; };

// vert-cor.R:335-344 from mean(xc), mean(xc^2), mean(yc), mean(yc^2): NI thresholds with
// draws lap[0..3], INT thresholds (fresh noise, :271-272) with lap[4..7].
__device__ __forceinline__ void priv_std_from_means(const SignConst& c, double mx, double m2x,
                                                    double my, double m2y, const double lap[8],
                                                    SignStd& s) {
  s.muNx = mx + c.s_mu_x * lap[0];
  s.sdNx = sqrt(rmax((m2x + c.s_m2_x * lap[1]) - s.muNx * s.muNx, 1e-12));
  s.muNy = my + c.s_mu_y * lap[2];
  s.sdNy = sqrt(rmax((m2y + c.s_m2_y * lap[3]) - s.muNy * s.muNy, 1e-12));
  s.muIx = mx + c.s_mu_x * lap[4];
  s.sdIx = sqrt(rmax((m2x + c.s_m2_x * lap[5]) - s.muIx * s.muIx, 1e-12));
  s.muIy = my + c.s_mu_y * lap[6];
  s.sdIy = sqrt(rmax((m2y + c.s_m2_y * lap[7]) - s.muIy * s.muIy, 1e-12));
}

__device__ __forceinline__ void priv_std_from_sums(const SignConst& c, const double v[4],
                                                   const double lap[8], SignStd& s) {
  // mean(xc) = sum/n (R: LD mean, agrees to rounding)
  priv_std_from_means(c, v[0] / c.nd, v[1] / c.nd, v[2] / c.nd, v[3] / c.nd, lap, s);
}

__device__ __forceinline__ void ni_sign_result(const SignConst& c, DD sT, DD sT2, bool bad,
                                               double* o) {
  // vert-cor.R:233-254
  const double sumT = sT.hi + sT.lo;
  const double eta = c.inv_k * sumT;
  const double S = sqrt(dd_var(sT, sT2, c.kd));
  o[0] = sin(M_PI * eta / 2.0);
  o[1] = sin(M_PI / 2.0 * rmax(eta - c.crit * S / c.sqrt_k, -1.0));
  o[2] = sin(M_PI / 2.0 * rmin(eta + c.crit * S / c.sqrt_k, 1.0));
  if (bad) o[0] = o[1] = o[2] = dnan();
}

// vert-cor.R:186-194, 281-313.  Returns (rho, eta, se_eta) and the mixquant c*.
__device__ __forceinline__ void int_sign_point(const SignConst& c, long long core, double lapz,
                                               double& rho, double& eta, double& se,
                                               double& cstar) {
  const double Z = c.scale_Z * lapz;
  const double eta0 = c.coefZ * (double)core + Z;
  rho = sin(M_PI * eta0 / 2.0);
  eta = 1.0 - acos(rho) * 2.0 / M_PI;
  const double h = 1.0 - acos(rho) * 2.0 / M_PI;
  const double s2 = 1.0 - c.q2 * (h * h);
  se = 1.0 / sqrt(c.nd) * sqrt(s2) * c.ratio;
  cstar = 2.0 / (sqrt(c.nd * s2) * c.eps_r);
}

// ------------------------------------------------- in-kernel draws of the sign family
__device__ __forceinline__ uint32_t word(const U4& w, uint32_t q) {
  return q == 0 ? w.w0 : (q == 1 ? w.w1 : (q == 2 ? w.w2 : w.w3));
}

struct FlipGen {  // sign-family INT flips, 4 per Philox block (SITE_FLIP), cached per block
  uint32_t cidx;
  U4 cw;
  // the flip of sample i from its block's words: 2*S - 1 (vert-cor.R:175-179)
  static __device__ __forceinline__ int of(const U4& w, uint32_t i, uint64_t p) {
    return ((uint64_t)word(w, i & 3) < p) ? 1 : -1;
  }
  __device__ __forceinline__ int get(uint32_t i, uint32_t rep, uint32_t k0, uint32_t k1,
                                     uint64_t p) {
    const uint32_t bi = i >> 2;
    if (bi != cidx) { cw = draw(bi, rep, DCOR_SITE_FLIP, k0, k1); cidx = bi; }
    return of(cw, i, p);
  }
};

// mixquant inside the workgroup: keys = z + c*l from Philox, then the order statistic.
__device__ __forceinline__ double mixquant_fused(const MixConst& mx, double c, uint32_t rep,
                                                 uint32_t k0, uint32_t k1, SelScratch* sc) {
  if (threadIdx.x == 0) sc->nan_cnt = 0;
  __syncthreads();
  double val[SEL_VPT];
  int nn = 0;
#pragma unroll
  for (int s = 0; s < SEL_VPT / 2; ++s) {
    const int b = threadIdx.x + s * DCOR_BLOCK;  // Philox block b -> elements 2b, 2b+1
    val[2 * s] = val[2 * s + 1] = dnan();
    if (2 * b < mx.nsim) {
      const U4 wz = draw((uint32_t)b, rep, DCOR_SITE_MIX_Z, k0, k1);
      const U4 wl = draw((uint32_t)b, rep, DCOR_SITE_MIX_L, k0, k1);
      double z0, z1;
      normal_pair(wz, &z0, &z1);
      val[2 * s] = z0 + c * unit_laplace(u53(wl.w0, wl.w1));
      nn += (val[2 * s] != val[2 * s]);
      if (2 * b + 1 < mx.nsim) {
        val[2 * s + 1] = z1 + c * unit_laplace(u53(wl.w2, wl.w3));
        nn += (val[2 * s + 1] != val[2 * s + 1]);
      }
    }
  }
  if (nn) atomicAdd(&sc->nan_cnt, nn);
  __syncthreads();
  return value_select(val, mx.pos, mx.nsim - sc->nan_cnt, sc);
}

__device__ __forceinline__ void scalar_laplace(uint32_t rep, uint32_t k0, uint32_t k1, double* lap) {
  if (threadIdx.x < 5) {  // SITE_SCALAR blocks 0..4: NI mu/m2 X, NI mu/m2 Y, INT ..., Z
    const U4 w = draw((uint32_t)threadIdx.x, rep, DCOR_SITE_SCALAR, k0, k1);
    lap[2 * threadIdx.x] = unit_laplace(u53(w.w0, w.w1));
    lap[2 * threadIdx.x + 1] = unit_laplace(u53(w.w2, w.w3));
  }
}

// INT epilogue + CI write shared by the sign kernels (vert-cor.R:281-313).
__device__ __forceinline__ void sign_finish(const SignConst& c, uint32_t rep, DD sT, DD sT2,
                                            long long core, bool any_ni, bool any_int,
                                            const double* lap, SelScratch* sel,
                                            dcor_rep_out* dst) {
  double o[6];
  ni_sign_result(c, sT, sT2, any_ni, o);
  double rho, eta, se, cstar;
  int_sign_point(c, core, lap[8], rho, eta, se, cstar);
  double w;
  if (c.mode_normal)
    w = mixquant_fused(c.mix, cstar, rep, c.k0, c.k1, sel) * se;
  else
    w = c.w_laplace;
  o[3] = rho;
  o[4] = sin(M_PI / 2.0 * rmax(eta - w, -1.0));
  o[5] = sin(M_PI / 2.0 * rmin(eta + w, 1.0));
  if (any_int) o[3] = o[4] = o[5] = dnan();
  if (threadIdx.x == 0) *dst = dcor_rep_out{o[0], o[1], o[2], o[3], o[4], o[5]};
}

__device__ __forceinline__ void ni_subg_result(const SubgConst& c, DD sP, DD sT, DD sT2,
                                               double* o) {
  // ver-cor-subG.R:51-59
  const double rho = c.m_over_k * (sP.hi + sP.lo);
  const double se = sqrt(dd_var(sT, sT2, c.kd)) / c.sqrt_k;
  o[0] = rho;
  o[1] = rmax(rho - c.crit * se, -1.0);
  o[2] = rmin(rho + c.crit * se, 1.0);
}

// Wave-level mixquant from Philox (one replicate per wave): the same elements as
// mixquant_fused, VPL keys per lane, written to the wave's LDS and selected there.
template <int VPL>
struct WaveMix {
  double keys[64 * VPL];
  WaveSelL sel;
};

template <int VPL>
__device__ __forceinline__ double wave_mixquant_fused(const MixConst& mx, double c, uint32_t rep,
                                                      uint32_t k0, uint32_t k1, WaveMix<VPL>* ws) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < VPL / 2; ++s) {
    const int b = lane + 64 * s;  // Philox block b -> elements 2b, 2b+1
    double v0 = dnan(), v1 = dnan();
    if (2 * b < mx.nsim) {
      const U4 wz = draw((uint32_t)b, rep, DCOR_SITE_MIX_Z, k0, k1);
      const U4 wl = draw((uint32_t)b, rep, DCOR_SITE_MIX_L, k0, k1);
      double z0, z1;
      normal_pair(wz, &z0, &z1);
      v0 = z0 + c * unit_laplace(u53(wl.w0, wl.w1));
      if (2 * b + 1 < mx.nsim) v1 = z1 + c * unit_laplace(u53(wl.w2, wl.w3));
    }
    ws->keys[lane + 64 * (2 * s)] = v0;
    ws->keys[lane + 64 * (2 * s + 1)] = v1;
  }
  wave_sync();
  return wave_select_lds<VPL>(ws->keys, mx.pos, &ws->sel);
}

// The INT tail of a sub-G replicate (ver-cor-subG.R:91-103) from the sums of Uc and Uc^2 over all
// n samples and the central unit Laplace lapz: o[3..5] = the estimate and its CI.  The tail of the
// fused engine's subg_fused_core, operation for operation, for the panel kernel
// (dcor_subgpanel.hip).  WAVE: one wave per replicate (ws), else one workgroup (sel); every thread
// of it calls.
template <bool WAVE, int VPL>
__device__ __forceinline__ void subg_int_finish(const SubgConst& c, uint32_t rep, const DD& sU,
                                                const DD& sU2, double lapz, SelScratch* sel,
                                                WaveMix<VPL>* ws, double* o) {
  const DD mU = dd_div_d(sU, c.nd);
  const double rho = (mU.hi + mU.lo) + c.s_central * lapz;             // :91
  const double sd = sqrt(dd_var(sU, sU2, c.nd));
  const double se_norm = sqrt(sd * sd + c.sn2x2);                      // :99
  const double cstar = 2.0 / (c.sqrt_n * sd * c.eps_r);                // :100
  double q;
  if constexpr (WAVE) q = wave_mixquant_fused<VPL>(c.mix, cstar, rep, c.k0, c.k1, ws);
  else q = mixquant_fused(c.mix, cstar, rep, c.k0, c.k1, sel);
  const double width = q * se_norm / c.sqrt_n;                         // :101
  o[3] = rho;
  o[4] = rmax(rho - width, -1.0);
  o[5] = rmin(rho + width, 1.0);
}


}  // namespace dcor
