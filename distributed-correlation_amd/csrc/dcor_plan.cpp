// dcor_plan.cpp -- the device-free half of the host side (dcor_plan.h): the error reporter, the
// argument checks of the reference's stopifnot() calls, every data-independent scalar of the
// estimators (R operation order, cited), and the segment planners of the ten segment-list
// entries.  No HIP: this file and the headers it includes compile with a host compiler alone.
#include "dcor_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>

namespace dcor {
namespace host {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

double r_min(double a, double b) { return (std::isnan(a) || std::isnan(b)) ? NAN : (a < b ? a : b); }
double r_max(double a, double b) { return (std::isnan(a) || std::isnan(b)) ? NAN : (a > b ? a : b); }

// T with (double)w * 2^-32 < p  <=>  w < T for every uint32 w: T = ceil(p * 2^32) clamped
// to [0, 2^32] (p * 2^32 is exact).
uint64_t u32_threshold(double p) {
  if (!(p > 0)) return 0;
  const double t = std::ceil(p * 4294967296.0);
  return t >= 4294967296.0 ? (uint64_t)4294967296ull : (uint64_t)t;
}

// MixConst for sort(x)[ceiling(p*nsim)], p = 1 - alpha/2.
int make_mix(int64_t nsim, double alpha, MixConst& mx) {
  if (nsim < 1 || nsim > 2048) return fail(DCOR_EINVAL, "nsim must be in [1, 2048] (got %lld)", (long long)nsim);
  const double pos = std::ceil((1.0 - alpha / 2.0) * (double)nsim);
  mx.nsim = (int32_t)nsim;
  mx.pos = (pos >= 1 && pos <= (double)nsim) ? (int32_t)pos - 1 : -1;
  mx.P = 1;
  while (mx.P < mx.nsim) mx.P <<= 1;
  mx.pad = 0;
  return DCOR_OK;
}

int check_common(int64_t n, double eps1, double eps2, double alpha) {
  if (n < 1 || n > 0x7fffffffLL) return fail(DCOR_EINVAL, "n must be in [1, 2^31) (got %lld)", (long long)n);
  if (!(eps1 > 0) || !(eps2 > 0) || !std::isfinite(eps1) || !std::isfinite(eps2))
    return fail(DCOR_EINVAL, "eps1 > 0 and eps2 > 0 required (vert-cor.R:264)");
  // The reference never checks alpha: qnorm(1 - alpha/2) and mixquant's
  // sort(x)[ceiling((1 - alpha/2) nsim)] are evaluated as they come (alpha = 1: a zero-width
  // CI; alpha < 0: NaN).  alpha >= 2 makes the mixquant index < 1, where R's x[0] is
  // numeric(0) and run_sim_one's detail assignment fails, so it is refused here.
  if (std::isnan(alpha) || !(alpha < 2))
    return fail(DCOR_EINVAL, "alpha must be < 2 (R's mixquant index ceiling((1-alpha/2)*nsim) >= 1)");
  return DCOR_OK;
}

// ci_NI_signbatch + ci_INT_signflip scalars (vert-cor.R:204-317).
// allow_k0: INT-only single calls (ci_INT_signflip has no batch requirement).
int make_sign(int64_t n, double eps1, double eps2, double alpha, int normalise, int mode,
              int64_t nsim, bool allow_k0, SignConst& c) {
  std::memset(&c, 0, sizeof(c));
  if (int st = check_common(n, eps1, eps2, alpha)) return st;
  const double nd = (double)n;
  const double md = std::ceil(8.0 / (eps1 * eps2));                     // :207
  const double kd = std::floor(nd / md);                                 // :208
  if (!(kd >= 1) && !allow_k0)
    return fail(DCOR_EKLT1, "ci_NI_signbatch: k = floor(n/m) = %g < 1 (n=%lld, m=%g; vert-cor.R:209)", kd, (long long)n, md);
  if (md > 0x7fffffff) return fail(DCOR_EINVAL, "batch size m too large");
  c.n = n; c.m = (int32_t)md; c.k = kd >= 1 ? (int64_t)kd : 0;
  c.nd = nd; c.md = md; c.kd = kd;
  c.pieces = sign_pieces(c.m);
  {
    int e = 0;
    c.md_pow2 = (std::frexp(md, &e) == 0.5) ? 1 : 0;  // md = 2^(e-1): count / md == count * 2^(1-e)
    c.inv_md = c.md_pow2 ? std::ldexp(1.0, 1 - e) : 0.0;
  }
  c.normalise = normalise ? 1 : 0;
  const double L = std::sqrt(2.0 * std::log(nd));                        // :212
  c.L = L;
  c.s_mu_x = 2.0 * L / (nd * (eps1 / 2));                                // :335-336
  c.s_m2_x = 2.0 * (L * L) / (nd * (eps1 / 2));                          // :339-340
  c.s_mu_y = 2.0 * L / (nd * (eps2 / 2));
  c.s_m2_y = 2.0 * (L * L) / (nd * (eps2 / 2));
  c.bx = 2.0 / (md * eps1);                                              // :230
  c.by = 2.0 / (md * eps2);                                              // :231
  c.inv_k = 1.0 / kd;                                                    // :234
  c.crit = dcor_qnorm(1.0 - alpha / 2.0);                                // :242
  c.sqrt_k = std::sqrt(kd);
  c.sender_is_X = (eps1 >= eps2) ? 1 : 0;                                // :275
  const double eps_s = c.sender_is_X ? eps1 : eps2, eps_r = c.sender_is_X ? eps2 : eps1;
  const double es = std::exp(eps_s);
  c.pflip = es / (es + 1.0);                                             // :174
  c.flipT = u32_threshold(c.pflip);
  {
    const double t = std::ceil(c.pflip * 16777216.0);  // exact scaling
    c.flipT24 = t >= 16777216.0 ? 16777216u : (t > 0 ? (uint32_t)t : 0u);
  }
  c.scale_Z = 2.0 * (es + 1.0) / (nd * (es - 1.0) * eps_r);              // :186-187
  c.coefZ = (es + 1.0) / (nd * (es - 1.0));                              // :190-191
  const double q = (es - 1.0) / (es + 1.0);
  c.q2 = q * q;                                                          // :284
  c.ratio = (es + 1.0) / (es - 1.0);                                     // :289
  c.inv_sqrt_n = 1.0 / std::sqrt(nd);
  c.eps_r = eps_r;
  c.w_laplace = (2.0 / (nd * eps_r)) * c.ratio * std::log(1.0 / alpha);  // :305-308
  int md_ = mode;
  if (md_ == DCOR_MODE_AUTO) md_ = (std::sqrt(nd) * eps_r > 0.5) ? DCOR_MODE_NORMAL : DCOR_MODE_LAPLACE;  // :294-296
  else if (md_ != DCOR_MODE_NORMAL && md_ != DCOR_MODE_LAPLACE) return fail(DCOR_EINVAL, "ci_mode must be auto/normal/laplace");
  c.mode_normal = (md_ == DCOR_MODE_NORMAL) ? 1 : 0;
  if (int st = make_mix(nsim, alpha, c.mix)) return st;
  return DCOR_OK;
}

// correlation_NI_subG + ci_INT_subG scalars (ver-cor-subG.R:25-108; HRS variant
// real-data-sims.R:115-147,176-252 when hrs).
int make_subg(int64_t n, double eps1, double eps2, double eta1, double eta2, double alpha,
              int hrs, double lam_x, double lam_y, double lam_s, double lam_o, double lam_r,
              double delta, int64_t nsim, SubgConst& c, double* lo_out, double* crit_sqrt2_s) {
  std::memset(&c, 0, sizeof(c));
  if (int st = check_common(n, eps1, eps2, alpha)) return st;
  if (hrs && n < 2) return fail(DCOR_EINVAL, "n >= 2 required (real-data-sims.R:121)");
  const double nd = (double)n;
  c.n = n; c.nd = nd;
  c.l1 = (hrs && !std::isnan(lam_x)) ? lam_x : dcor_lambda_n(nd, eta1);  // :30 / rds:123
  c.l2 = (hrs && !std::isnan(lam_y)) ? lam_y : dcor_lambda_n(nd, eta2);
  double md = std::ceil(8.0 / (eps1 * eps2));                            // :37
  if (md > nd) md = nd;
  double kd = std::floor(nd / md);                                       // :38
  if (hrs) {
    if (kd < 2) { kd = 2; md = std::floor(nd / kd); }                    // rds:130
  } else if (!(kd >= 1)) {
    return fail(DCOR_EKLT1, "correlation_NI_subG: k < 1 (ver-cor-subG.R:38)");
  }
  c.m = (int32_t)md; c.k = (int64_t)kd; c.md = md; c.kd = kd;
  {
    int e = 0;
    c.md_pow2 = (std::frexp(md, &e) == 0.5) ? 1 : 0;
    c.inv_md = c.md_pow2 ? std::ldexp(1.0, 1 - e) : 0.0;
  }
  c.bx = 2.0 * c.l1 / (md * eps1);                                       // :48
  c.by = 2.0 * c.l2 / (md * eps2);                                       // :49
  c.m_over_k = md / kd;                                                  // :51
  c.crit = dcor_qnorm(1.0 - alpha / 2.0);                                // :57
  c.sqrt_k = std::sqrt(kd);
  c.sender_is_X = (eps1 >= eps2) ? 1 : 0;                                // :76
  const double eps_s = c.sender_is_X ? eps1 : eps2, eps_r = c.sender_is_X ? eps2 : eps1;
  const double eta_s = c.sender_is_X ? eta1 : eta2, eta_r = c.sender_is_X ? eta2 : eta1;
  double lo_ = NAN;
  if (!hrs) {
    double lam[2];
    dcor_lambda_int_n(nd, eta_s, eta_r, eps_s, lam);                     // :83-85
    c.ls = lam[0]; c.lr = lam[1];
  } else {
    const double dl = std::isnan(delta) ? 1.0 / nd : delta;              // rds:199
    double ls = lam_s;
    lo_ = lam_o;
    if (std::isnan(ls) || std::isnan(lo_)) {                             // rds:202-208
      double lam[2];
      dcor_lambda_int_n(nd, eta_s, eta_r, eps_s, lam);
      if (std::isnan(ls)) ls = lam[0];
      if (std::isnan(lo_)) lo_ = dcor_lambda_n(nd, c.sender_is_X ? eta2 : eta1);
    }
    double lr = lam_r;
    if (std::isnan(lr)) lr = dcor_lambda_receiver_from_noise(ls, lo_, eps_s, dl);  // rds:211-218
    c.ls = ls; c.lr = lr;
  }
  c.bs = 2.0 * c.ls / (eps_s);                                           // :89
  c.s_central = 2.0 * c.lr / (nd * eps_r);                               // :91
  c.sn2x2 = 2.0 * (c.s_central * c.s_central);                           // :99
  c.sqrt_n = std::sqrt(nd);
  c.eps_r = eps_r;
  if (lo_out) *lo_out = lo_;
  if (crit_sqrt2_s) *crit_sqrt2_s = c.crit * std::sqrt(2.0) * (2.0 * c.lr / (nd * eps_r));  // rds:238
  if (int st = make_mix(nsim, alpha, c.mix)) return st;
  return DCOR_OK;
}

int premat_subg_const(const dcor_premat_subg* d, PrematSubgConst& p) {
  std::memset(&p, 0, sizeof(p));
  if (int st = make_subg(d->n, d->eps1, d->eps2, d->eta1, d->eta2, d->alpha, d->hrs, d->lam_x,
                         d->lam_y, d->lam_s, d->lam_o, d->lam_r, d->delta, d->nsim, p.s, &p.lo_,
                         &p.crit_sqrt2_s)) return st;
  p.hrs = d->hrs ? 1 : 0;
  // element-aligned arrays (the streaming kernels read 16 B at a time from the first 16-B
  // boundary of each row)
  const uintptr_t mis8 = ((uintptr_t)d->X | (uintptr_t)d->Y | (uintptr_t)d->lap_ni_x |
                          (uintptr_t)d->lap_ni_y | (uintptr_t)d->lap_local |
                          (uintptr_t)d->lap_central | (uintptr_t)d->mix_z | (uintptr_t)d->mix_l) & 7;
  if (mis8 || ((uintptr_t)d->perm & 3))
    return fail(DCOR_EINVAL, "premat_subg: arrays must be aligned to their element size");
  p.X = d->X; p.Y = d->Y; p.xy_stride = d->xy_stride; p.perm = d->perm;
  p.lap_ni_x = d->lap_ni_x; p.lap_ni_y = d->lap_ni_y; p.lap_local = d->lap_local;
  p.lap_central = d->lap_central; p.mix_z = d->mix_z; p.mix_l = d->mix_l;
  return DCOR_OK;
}

int hrs_noise_geometry(const dcor_premat_subg* d, int64_t* k, int64_t* m, size_t* per) {
  int64_t km[2];
  if (int st = dcor_batch_geometry(d->n, d->eps1, d->eps2, DCOR_FAMILY_SUBG, 1, km)) return st;
  *k = km[0]; *m = km[1];
  *per = HrsNoiseLayout(d->n, km[0], km[1], d->nsim, 1).bytes;
  return DCOR_OK;
}

int64_t hrs_chunk(size_t per, int64_t reps, size_t budget, int64_t cap) {
  int64_t cr = (int64_t)(budget / per);
  if (cr < 1) cr = 1;
  if (cr > cap) cr = cap;
  return cr > reps ? reps : cr;
}

// ------------------------------------------------------------------ segment planners
namespace {

// What the segment types differ in, one trait each: the test of its eps field(s), their wording in
// the message, and whether the segment names two columns of a table.
struct OneEps {
  template <class Seg> static bool eps_ok(const Seg& g) { return g.eps > 0.0; }
  static constexpr const char* eps_names = "eps";
};
struct TwoEps {
  template <class Seg> static bool eps_ok(const Seg& g) { return g.eps1 > 0.0 && g.eps2 > 0.0; }
  static constexpr const char* eps_names = "eps1, eps2";
};
struct TwoFiniteEps {
  template <class Seg> static bool eps_ok(const Seg& g) {
    return TwoEps::eps_ok(g) && std::isfinite(g.eps1) && std::isfinite(g.eps2);
  }
  static constexpr const char* eps_names = "finite eps1, eps2";
};
template <class Seg> struct SegTrait;
template <> struct SegTrait<dcor_hrs_segment> : OneEps { static constexpr bool columns = false; };
template <> struct SegTrait<dcor_hrs_pair_segment> : OneEps { static constexpr bool columns = true; };
template <> struct SegTrait<dcor_sign_segment> : TwoEps { static constexpr bool columns = false; };
template <> struct SegTrait<dcor_sign_pair_segment> : TwoEps { static constexpr bool columns = true; };
template <> struct SegTrait<dcor_subg_segment> : TwoFiniteEps { static constexpr bool columns = false; };
template <> struct SegTrait<dcor_subg_pair_segment> : TwoFiniteEps { static constexpr bool columns = true; };

// Segment i's own fields (they need nothing but the segment; p: the table's column count), its
// replicates added to `items`; cap: at most 2^31 - 1 replicates in one call.
template <class Seg>
int segment_head(const char* entry, const Seg& g, int64_t i, int64_t p, bool cap, int64_t& items) {
  using Tr = SegTrait<Seg>;
  if (g.reps < 0 || g.rep_begin < 0 || g.out_row < 0 || !Tr::eps_ok(g))
    return fail(DCOR_EINVAL, "%s: segment %lld: need %s > 0, reps, rep_begin, out_row >= 0", entry,
                (long long)i, Tr::eps_names);
  if constexpr (Tr::columns) {
    if (g.col_x < 0 || g.col_x >= p || g.col_y < 0 || g.col_y >= p)
      return fail(DCOR_EINVAL, "%s: segment %lld: columns (%d, %d) outside [0, %lld)", entry, (long long)i,
                  (int)g.col_x, (int)g.col_y, (long long)p);
  }
  if (rep_range_exceeds(g.rep_begin, g.reps))
    return fail(DCOR_EINVAL, "%s: segment %lld: replicate range exceeds 2^32", entry, (long long)i);
  items += g.reps;   // reps <= 2^32 each: no overflow below 2^31 segments
  if (cap && items > 0x7fffffffLL)
    return fail(DCOR_EINVAL, "%s: more than 2^31 - 1 replicates in one call", entry);
  return DCOR_OK;
}

template <class Seg>
int segment_heads(const char* entry, const Seg* segs, int64_t nseg, int64_t p, int64_t* items) {
  *items = 0;
  for (int64_t i = 0; i < nseg; ++i)
    if (int st = segment_head(entry, segs[i], i, p, true, *items)) return st;
  return DCOR_OK;
}

// Every segment's launch constants (n, eps, alpha, ci_mode, nsim, k >= 1: make_sign; a segment
// without replicates is checked too), the kept ones into `tab`.
template <class Desc, class Seg, class SegConst>
int sign_segment_table(const Desc& d, const Seg* segs, int64_t nseg, std::vector<SegConst>& tab) {
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const Seg& g = segs[i];
    SegConst t;
    std::memset(&t, 0, sizeof(t));
    if (int st = make_sign(d.n, g.eps1, g.eps2, d.alpha, d.normalise, d.ci_mode, d.nsim, false, t.s))
      return st;
    if (g.reps == 0) continue;
    t.s.k0 = (uint32_t)g.seed; t.s.k1 = (uint32_t)(g.seed >> 32);
    t.s.rep_begin = g.rep_begin;
    t.first = first; t.out_row = g.out_row;
    if constexpr (SegTrait<Seg>::columns) { t.col_x = g.col_x; t.col_y = g.col_y; }
    first += g.reps;
    tab.push_back(t);
  }
  return DCOR_OK;
}

// The panel and base checks of the two HRS sweeps.
int check_hrs_base(const char* entry, const dcor_premat_subg* base, const dcor_panel* panel) {
  if (base->X != panel->X || base->Y != panel->Y || base->xy_stride != 0 || base->n != panel->n)
    return fail(DCOR_EINVAL, "%s: X, Y, n must be the panel's and xy_stride 0", entry);
  if (!base->hrs) return fail(DCOR_EINVAL, "%s: the HRS variant only (hrs = 1)", entry);
  if (!(base->delta > 0.0)) return fail(DCOR_EINVAL, "%s: delta must be positive", entry);
  return DCOR_OK;
}

// The device-table record of a fused HRS segment from its launch constants pc (make_subg's values,
// unchanged), its keys and its place in the call.
template <class Seg>
void hrs_segment_record(const PrematSubgConst& pc, const Seg& g, int64_t first, HrsSegConst& t) {
  const SubgConst& a = pc.s;
  t.k = a.k; t.m = a.m; t.md_pow2 = a.md_pow2;
  t.md = a.md; t.kd = a.kd; t.inv_md = a.inv_md;
  t.bx = a.bx; t.by = a.by; t.m_over_k = a.m_over_k; t.sqrt_k = a.sqrt_k;
  t.lr = a.lr; t.bs = a.bs; t.s_central = a.s_central; t.sn2x2 = a.sn2x2; t.eps_r = a.eps_r;
  t.crit_sqrt2_s = pc.crit_sqrt2_s;
  t.ni0 = (uint32_t)g.seed_ni; t.ni1 = (uint32_t)(g.seed_ni >> 32);
  t.in0 = (uint32_t)g.seed_int; t.in1 = (uint32_t)(g.seed_int >> 32);
  t.rep_begin = (uint32_t)g.rep_begin;
  t.first = first; t.out_row = g.out_row;
}

// The device-table record of a sub-G panel segment from its launch constants a (make_subg's values,
// unchanged), its key and its place in the call; its batch size m joins `slots` when it is new (the
// slots are the distinct m in order of first use, off the sum of the k before).
template <class Seg>
void subg_segment_record(const SubgConst& a, const Seg& g, int64_t first, std::vector<SubgMeanSlot>& slots,
                         SubgSegConst& t) {
  size_t d = 0;
  while (d < slots.size() && slots[d].m != a.m) ++d;
  if (d == slots.size()) {   // a batch size not seen before: its k means follow the others'
    SubgMeanSlot sl;
    std::memset(&sl, 0, sizeof(sl));
    sl.k = a.k; sl.off = slots.empty() ? 0 : slots.back().off + slots.back().k;
    sl.m = a.m; sl.md_pow2 = a.md_pow2; sl.md = a.md; sl.inv_md = a.inv_md;
    slots.push_back(sl);
  }
  std::memset(&t, 0, sizeof(t));
  t.k = a.k; t.m = a.m; t.md_pow2 = a.md_pow2; t.sender_is_X = a.sender_is_X;
  t.m_slot = (int32_t)d;
  t.md = a.md; t.kd = a.kd; t.inv_md = a.inv_md;
  t.bx = a.bx; t.by = a.by; t.m_over_k = a.m_over_k; t.sqrt_k = a.sqrt_k;
  t.ls = a.ls; t.lr = a.lr; t.bs = a.bs; t.s_central = a.s_central; t.sn2x2 = a.sn2x2; t.eps_r = a.eps_r;
  t.k0 = (uint32_t)g.seed; t.k1 = (uint32_t)(g.seed >> 32);
  t.rep_begin = (uint32_t)g.rep_begin;
  t.mean_off = slots[d].off;
  t.first = first; t.out_row = g.out_row;
}
int64_t mean_count(const std::vector<SubgMeanSlot>& slots) {   // the batch means of a call
  return slots.empty() ? 0 : slots.back().off + slots.back().k;
}

// The checks table entries share, in the entries' order: p and ld (every table descriptor); D's
// alignment and every lam[c] (T: dcor_hrs_table_desc or dcor_hrs_table_na_desc).
template <class T> int table_shape(const char* entry, const T& t) {
  if (t.p < 1 || t.p > 0x7fffffffLL)
    return fail(DCOR_EINVAL, "%s: p must be in [1, 2^31) (got %lld)", entry, (long long)t.p);
  if (t.ld < t.n)
    return fail(DCOR_EINVAL, "%s: ld = %lld < n = %lld", entry, (long long)t.ld, (long long)t.n);
  return DCOR_OK;
}
template <class T> int hrs_table_clips(const char* entry, const T& t) {
  if ((uintptr_t)t.D & 7) return fail(DCOR_EINVAL, "%s: D must be aligned to 8 bytes", entry);
  for (int64_t c = 0; c < t.p; ++c)
    if (!std::isfinite(t.lam[c]) || !(t.lam[c] > 0.0))
      return fail(DCOR_EINVAL, "%s: column %lld: lam must be finite and > 0 (got %g)", entry, (long long)c,
                  t.lam[c]);
  return DCOR_OK;
}
// alpha and nsim of a sub-G or HRS call, as every segment's make_subg would refuse them
int check_alpha_nsim(int64_t n, double alpha, int64_t nsim) {
  MixConst mx;
  if (int st = check_common(n, 1.0, 1.0, alpha)) return st;
  return make_mix(nsim, alpha, mx);
}

// The standardisation's part of the two private descriptors (T: dcor_hrs_private_desc or
// dcor_hrs_private_na_desc), in the entries' order: D's alignment, every interval, the budgets.
template <class T> int private_release_args(const char* entry, const T& t) {
  if ((uintptr_t)t.D & 7) return fail(DCOR_EINVAL, "%s: D must be aligned to 8 bytes", entry);
  for (int64_t c = 0; c < t.p; ++c)
    if (!std::isfinite(t.lo[c]) || !std::isfinite(t.hi[c]) || !(t.lo[c] < t.hi[c]))
      return fail(DCOR_EINVAL, "%s: column %lld: need finite lo < hi (got %g, %g)", entry, (long long)c,
                  t.lo[c], t.hi[c]);
  if (!std::isfinite(t.eps_mean) || !std::isfinite(t.eps_m2) || !(t.eps_mean > 0.0) || !(t.eps_m2 > 0.0))
    return fail(DCOR_EINVAL, "%s: eps_mean, eps_m2 must be finite and > 0 (got %g, %g)", entry, t.eps_mean,
                t.eps_m2);
  return DCOR_OK;
}
// What the two private plans carry of their descriptor: the intervals as (lo, hi) pairs, the budgets
// and the key of DCOR_SITE_STD.
template <class T> void private_release_plan(const T& t, std::vector<double>& lohi, HrsPrivCall& pv) {
  lohi.resize(2 * (size_t)t.p);
  for (int64_t c = 0; c < t.p; ++c) { lohi[2 * (size_t)c] = t.lo[c]; lohi[2 * (size_t)c + 1] = t.hi[c]; }
  pv.eps_mean = t.eps_mean; pv.eps_m2 = t.eps_m2;
  pv.k0 = (uint32_t)t.seed_std; pv.k1 = (uint32_t)(t.seed_std >> 32);
}
// A private segment's constants and record at sample count n and clip delta: make_subg's checks and
// everything of it that no clip bound enters (the bounds are placeholders), the lambda-dependent
// fields zero (every replicate derives its own), the two host factors of that derivation.
int private_segment_record(int64_t n, double delta, double alpha, int64_t nsim, const dcor_hrs_pair_segment& g,
                           int64_t first, PrematSubgConst& pc, HrsPrivSegConst& r) {
  std::memset(&pc, 0, sizeof(pc));
  if (int st = make_subg(n, g.eps, g.eps, 1.0, 1.0, alpha, 1, 1.0, 1.0, 1.0, 1.0, 1.0, delta, nsim, pc.s, &pc.lo_,
                         &pc.crit_sqrt2_s))
    return st;
  hrs_segment_record(pc, g, first, r);
  r.bx = r.by = r.bs = r.lr = r.s_central = r.sn2x2 = r.crit_sqrt2_s = 0.0;   // per replicate
  r.col_x = g.col_x; r.col_y = g.col_y;
  r.log_inv_delta = std::log(1.0 / delta);   // lambda_receiver_from_noise's, rds:172
  r.crit_sqrt2 = pc.s.crit * std::sqrt(2.0);
  return DCOR_OK;
}
// The call-wide constants of a private call from any segment's (n, nd, sqrt_n: the pairwise entry's
// records carry their own).
void private_call_consts(const PrematSubgConst& pc, PrematSubgConst& c0) {
  c0.s.n = pc.s.n; c0.s.nd = pc.s.nd; c0.s.sqrt_n = pc.s.sqrt_n; c0.s.crit = pc.s.crit; c0.s.mix = pc.s.mix;
  c0.s.sender_is_X = 1;
  c0.hrs = 1;
}

// The pairs of a pairwise call: every segment's n_ab (a pair is counted once), and the distinct
// ordered pairs of the segments with replicates as slots in order of first use, each panel behind the
// one before.
struct PairSlots {
  struct Pair { int64_t n_ab, slot; };   // slot: -1 until a segment with replicates names the pair
  std::map<std::pair<int32_t, int32_t>, Pair> seen;
  Pair& pair(const uint64_t* valid, int64_t n, const dcor_hrs_pair_segment& g) {
    const auto at = seen.emplace(std::make_pair(g.col_x, g.col_y), Pair{0, -1});
    if (at.second) at.first->second.n_ab = hrs_pair_count(valid, n, g.col_x, g.col_y);
    return at.first->second;
  }
  // segment i's pair, refused unless 2 <= n_ab <= DCOR_DICT_NMAX
  int checked(const char* entry, const uint64_t* valid, int64_t n, const dcor_hrs_pair_segment& g, int64_t i,
              Pair** out) {
    Pair& pr = pair(valid, n, g);
    *out = &pr;
    if (pr.n_ab < 2 || pr.n_ab > DCOR_DICT_NMAX)
      return fail(DCOR_EINVAL, "%s: segment %lld: columns (%d, %d) have n_ab = %lld pairwise-complete rows, "
                  "must be in [2, %d]: a replicate keeps u16 indices of the compacted rows in LDS", entry,
                  (long long)i, (int)g.col_x, (int)g.col_y, (long long)pr.n_ab, DCOR_DICT_NMAX);
    return DCOR_OK;
  }
  // the pair's slot, a new one when no segment has run the pair before
  const HrsPairSlot& slot(Pair& pr, const dcor_hrs_pair_segment& g, std::vector<HrsPairSlot>& slots,
                          int64_t& panel_elems) {
    if (pr.slot < 0) {
      HrsPairSlot sl;
      std::memset(&sl, 0, sizeof(sl));
      sl.n_ab = pr.n_ab; sl.panel = panel_elems;
      sl.col_x = g.col_x; sl.col_y = g.col_y;
      panel_elems += hrs_pair_panel_elems(pr.n_ab);
      pr.slot = (int64_t)slots.size();
      slots.push_back(sl);
    }
    return slots[(size_t)pr.slot];
  }
};

}  // namespace

dcor_premat_subg hrs_segment_desc(const dcor_premat_subg& base, const dcor_hrs_segment& g) {
  dcor_premat_subg q = base;
  q.reps = g.reps;
  q.eps1 = q.eps2 = g.eps;
  q.eta1 = q.eta2 = 1.0;
  q.lam_r = dcor_lambda_receiver_from_noise(base.lam_s, base.lam_o, g.eps, base.delta);
  return q;
}

int plan_hrs_sweep(const dcor_premat_subg* base, const dcor_panel* panel,
                   const dcor_hrs_segment* segs, int64_t nseg, HrsSweepPlan& plan) {
  if (int st = check_hrs_base("hrs_sweep", base, panel)) return st;
  // every segment's constants and geometry first: nothing is enqueued for an invalid sweep
  plan.segs = std::vector<HrsSweepSeg>((size_t)nseg);
  // noise of up to 8192 replicates per launch chain (C5's 8192 x 420 KB: 3.4 GB), at most 4 GB
  const size_t budget = (size_t)4 << 30;
  int64_t items = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_hrs_segment& g = segs[i];
    if (int st = segment_head("hrs_sweep", g, i, 0, false, items)) return st;
    HrsSweepSeg& sp = plan.segs[(size_t)i];
    sp.q = hrs_segment_desc(*base, g);
    PrematSubgConst pc;   // the launch constants' own checks, here rather than mid-sweep
    if (int st = premat_subg_const(&sp.q, pc)) return st;
    size_t per;
    if (int st = hrs_noise_geometry(&sp.q, &sp.k, &sp.m, &per)) return st;
    sp.cr = hrs_chunk(per, g.reps, budget, 8192);
    plan.need = std::max(plan.need, per * (size_t)sp.cr);
    plan.cap = std::max(plan.cap, sp.cr);
  }
  return DCOR_OK;
}

int plan_hrs_fused_sweep(const dcor_premat_subg* base, const dcor_panel* panel,
                         const dcor_hrs_segment* segs, int64_t nseg, HrsFusedSweepPlan& plan) {
  // the segments' own fields first (they need nothing but segs), then the panel and base, then
  // every segment's launch constants: nothing is enqueued for an invalid sweep
  if (int st = segment_heads("hrs_fused_sweep", segs, nseg, 0, &plan.items)) return st;
  if (int st = check_hrs_base("hrs_fused_sweep", base, panel)) return st;
  plan.qs = std::vector<dcor_premat_subg>((size_t)nseg);
  std::vector<HrsSegConst>& tab = plan.tab;
  PrematSubgConst& p0 = plan.p0;
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_hrs_segment& g = segs[i];
    dcor_premat_subg& q = plan.qs[(size_t)i];
    q = hrs_segment_desc(*base, g);
    PrematSubgConst pc;
    if (int st = premat_subg_const(&q, pc)) return st;
    if (g.reps == 0) continue;
    if (tab.empty()) p0 = pc;
    const SubgConst &a = pc.s, &b = p0.s;
    // bitwise: a NaN clip (lam_s / lam_o unset with an out-of-range eta) differs from itself in
    // value but not as a constant
    const double wa[] = {a.l1, a.l2, a.ls, pc.lo_, a.nd, a.sqrt_n, a.crit};
    const double wb[] = {b.l1, b.l2, b.ls, p0.lo_, b.nd, b.sqrt_n, b.crit};
    plan.wide = plan.wide && std::memcmp(wa, wb, sizeof(wa)) == 0 && a.sender_is_X == b.sender_is_X &&
                std::memcmp(&a.mix, &b.mix, sizeof(a.mix)) == 0;
    HrsSegConst t;
    std::memset(&t, 0, sizeof(t));
    hrs_segment_record(pc, g, first, t);
    first += g.reps;
    tab.push_back(t);
    plan.max_km = std::max(plan.max_km, a.k * (int64_t)a.m);
  }
  return DCOR_OK;
}

int plan_sign_panel(const dcor_sign_panel_desc* p, const dcor_sign_segment* segs, int64_t nseg,
                    SignPanelPlan& plan) {
  plan = SignPanelPlan();
  if (!p->X || !p->Y) return fail(DCOR_EINVAL, "sign_panel: null argument (X, Y)");
  if (int st = segment_heads("sign_panel", segs, nseg, 0, &plan.items)) return st;
  if (int st = sign_segment_table(*p, segs, nseg, plan.tab)) return st;
  plan.lay = SignPanelLayout((int64_t)plan.tab.size(), p->n);
  return DCOR_OK;
}

int plan_sign_table(const dcor_sign_table_desc* t, const dcor_sign_pair_segment* segs, int64_t nseg,
                    SignTablePlan& plan) {
  plan = SignTablePlan();
  if (!t->D) return fail(DCOR_EINVAL, "sign_table: null argument (D)");
  if (int st = table_shape("sign_table", *t)) return st;
  if (int st = segment_heads("sign_table", segs, nseg, t->p, &plan.items)) return st;
  if (int st = sign_segment_table(*t, segs, nseg, plan.tab)) return st;
  plan.lay = SignTableLayout((int64_t)plan.tab.size(), t->n, t->p);
  if (!plan.lay.ok)
    return fail(DCOR_EINVAL, "sign_table: p * npad * 8 scratch bytes overflow (p = %lld, n = %lld)",
                (long long)t->p, (long long)t->n);
  return DCOR_OK;
}

dcor_premat_subg hrs_pair_desc(const dcor_hrs_table_desc& t, const dcor_hrs_pair_segment& g) {
  dcor_premat_subg q;
  std::memset(&q, 0, sizeof(q));
  q.n = t.n; q.reps = g.reps;
  q.eps1 = q.eps2 = g.eps;
  q.eta1 = q.eta2 = 1.0;
  q.alpha = t.alpha; q.hrs = 1;
  q.lam_x = q.lam_s = t.lam[g.col_x];
  q.lam_y = q.lam_o = t.lam[g.col_y];
  q.delta = t.delta;
  q.lam_r = dcor_lambda_receiver_from_noise(q.lam_s, q.lam_o, g.eps, t.delta);
  q.nsim = t.nsim;
  q.X = (const double*)((uintptr_t)t.D + (uintptr_t)g.col_x * (uintptr_t)t.ld * sizeof(double));
  q.Y = (const double*)((uintptr_t)t.D + (uintptr_t)g.col_y * (uintptr_t)t.ld * sizeof(double));
  return q;
}

int plan_hrs_table(const dcor_hrs_table_desc* t, const dcor_hrs_pair_segment* segs, int64_t nseg,
                   HrsTablePlan& plan) {
  plan = HrsTablePlan();
  if (!t->D || !t->lam) return fail(DCOR_EINVAL, "hrs_table: null argument (D, lam)");
  if (t->n < 2 || t->n > DCOR_DICT_NMAX)
    return fail(DCOR_EINVAL, "hrs_table: n must be in [2, %d] (got %lld): the kernel keeps a replicate's "
                "u16 batch indices in LDS and there is no fallback for a larger table", DCOR_DICT_NMAX,
                (long long)t->n);
  if (int st = table_shape("hrs_table", *t)) return st;
  if (!HrsTableLayout::columns(t->n, t->p).ok)
    return fail(DCOR_EINVAL, "hrs_table: p * npad * 8 scratch bytes overflow (p = %lld, n = %lld)",
                (long long)t->p, (long long)t->n);
  if (int st = hrs_table_clips("hrs_table", *t)) return st;
  if (!(t->delta > 0.0)) return fail(DCOR_EINVAL, "hrs_table: delta must be positive");
  if (int st = check_alpha_nsim(t->n, t->alpha, t->nsim)) return st;
  if (int st = segment_heads("hrs_table", segs, nseg, t->p, &plan.items)) return st;
  // every segment's launch constants: those of the reference call on its pair, lam and eps
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_hrs_pair_segment& g = segs[i];
    const dcor_premat_subg q = hrs_pair_desc(*t, g);
    PrematSubgConst pc;
    if (int st = premat_subg_const(&q, pc)) return st;
    if (g.reps == 0) continue;
    if (plan.tab.empty()) { plan.c0 = pc; plan.c0.X = plan.c0.Y = nullptr; }
    HrsPairSegConst r;
    std::memset(&r, 0, sizeof(r));
    hrs_segment_record(pc, g, first, r);
    r.col_x = g.col_x; r.col_y = g.col_y;
    first += g.reps;
    plan.tab.push_back(r);
    plan.max_km = std::max(plan.max_km, pc.s.k * (int64_t)pc.s.m);
  }
  plan.lay = HrsTableLayout(plan.items, (int64_t)plan.tab.size(), t->n, t->p);
  if (!plan.lay.ok)
    return fail(DCOR_EINVAL, "hrs_table: scratch bytes overflow (p = %lld, n = %lld)", (long long)t->p,
                (long long)t->n);
  return DCOR_OK;
}

int plan_hrs_private(const dcor_hrs_private_desc* t, const dcor_hrs_pair_segment* segs, int64_t nseg,
                     HrsPrivatePlan& plan) {
  const char* const entry = "hrs_private_table";
  plan = HrsPrivatePlan();
  if (!t->D || !t->lo || !t->hi) return fail(DCOR_EINVAL, "%s: null argument (D, lo, hi)", entry);
  if (t->n < 2 || t->n > DCOR_DICT_NMAX)
    return fail(DCOR_EINVAL, "%s: n must be in [2, %d] (got %lld): the kernel keeps a replicate's "
                "u16 batch indices in LDS and there is no fallback for a larger table", entry, DCOR_DICT_NMAX,
                (long long)t->n);
  if (int st = table_shape(entry, *t)) return st;
  if (!HrsPrivateLayout::columns(t->n, t->p).ok)
    return fail(DCOR_EINVAL, "%s: p * npad * 8 scratch bytes overflow (p = %lld, n = %lld)", entry,
                (long long)t->p, (long long)t->n);
  if (int st = private_release_args(entry, *t)) return st;
  if (!(t->delta > 0.0)) return fail(DCOR_EINVAL, "%s: delta must be positive", entry);
  if (int st = check_alpha_nsim(t->n, t->alpha, t->nsim)) return st;
  if (int st = segment_heads(entry, segs, nseg, t->p, &plan.items)) return st;
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_hrs_pair_segment& g = segs[i];
    PrematSubgConst pc;
    HrsPrivSegConst r;
    std::memset(&r, 0, sizeof(r));
    if (int st = private_segment_record(t->n, t->delta, t->alpha, t->nsim, g, first, pc, r)) return st;
    if (g.reps == 0) continue;
    if (plan.tab.empty()) private_call_consts(pc, plan.c0);
    first += g.reps;
    plan.tab.push_back(r);
    plan.max_km = std::max(plan.max_km, pc.s.k * (int64_t)pc.s.m);
  }
  plan.lay = HrsPrivateLayout(plan.items, (int64_t)plan.tab.size(), t->n, t->p);
  if (!plan.lay.ok)
    return fail(DCOR_EINVAL, "%s: scratch bytes overflow (p = %lld, n = %lld)", entry, (long long)t->p,
                (long long)t->n);
  private_release_plan(*t, plan.lohi, plan.pv);
  return DCOR_OK;
}

int64_t hrs_pair_count(const uint64_t* valid, int64_t n, int64_t col_x, int64_t col_y) {
  const int64_t nw = (n + 63) >> 6;
  const uint64_t* a = valid + col_x * nw;
  const uint64_t* b = valid + col_y * nw;
  int64_t c = 0;
  for (int64_t w = 0; w + 1 < nw; ++w) c += __builtin_popcountll(a[w] & b[w]);
  const uint64_t tail = (n & 63) ? (~0ull >> (64 - (n & 63))) : ~0ull;   // the rows of the last word
  return c + __builtin_popcountll(a[nw - 1] & b[nw - 1] & tail);
}

int plan_hrs_table_pairwise(const dcor_hrs_table_na_desc* t, const dcor_hrs_pair_segment* segs,
                            int64_t nseg, HrsPairTablePlan& plan) {
  const char* const entry = "hrs_table_pairwise";
  plan = HrsPairTablePlan();
  auto &tab = plan.tab; auto &slots = plan.slots;
  if (!t->D || !t->lam || !t->valid) return fail(DCOR_EINVAL, "%s: null argument (D, lam, valid)", entry);
  if (t->n < 2 || t->n > 0x7fffffffLL)
    return fail(DCOR_EINVAL, "%s: n must be in [2, 2^31) (got %lld)", entry, (long long)t->n);
  if (int st = table_shape(entry, *t)) return st;
  if (!HrsPairTableLayout::columns(t->n, t->p).ok)
    return fail(DCOR_EINVAL, "%s: p * ceil(n / 64) * 8 scratch bytes overflow (p = %lld, n = %lld)", entry,
                (long long)t->p, (long long)t->n);
  if (int st = hrs_table_clips(entry, *t)) return st;
  if (!(t->delta > 0.0) && !std::isnan(t->delta))
    return fail(DCOR_EINVAL, "%s: delta must be positive, or NaN for 1 / n_ab per pair", entry);
  if (int st = check_alpha_nsim(t->n, t->alpha, t->nsim)) return st;
  if (int st = segment_heads(entry, segs, nseg, t->p, &plan.items)) return st;
  // every segment's pair, then its launch constants: those of the reference call on the pair's
  // n_ab compacted rows, lam and eps
  PairSlots pairs;
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_hrs_pair_segment& g = segs[i];
    PairSlots::Pair* prp;
    if (int st = pairs.checked(entry, t->valid, t->n, g, i, &prp)) return st;
    PairSlots::Pair& pr = *prp;
    dcor_hrs_table_desc u;   // the reference call's table: the pair's own count and delta (rds:199)
    std::memset(&u, 0, sizeof(u));
    u.n = pr.n_ab; u.p = t->p; u.ld = t->ld; u.D = t->D; u.lam = t->lam;
    u.alpha = t->alpha; u.delta = std::isnan(t->delta) ? 1.0 / (double)pr.n_ab : t->delta; u.nsim = t->nsim;
    const dcor_premat_subg q = hrs_pair_desc(u, g);
    PrematSubgConst pc;
    if (int st = premat_subg_const(&q, pc)) return st;
    if (g.reps == 0) continue;
    if (tab.empty()) { plan.c0 = pc; plan.c0.X = plan.c0.Y = nullptr; }
    const HrsPairSlot& sl = pairs.slot(pr, g, slots, plan.panel_elems);
    HrsPairNaSegConst r;
    std::memset(&r, 0, sizeof(r));
    hrs_segment_record(pc, g, first, r);
    r.col_x = g.col_x; r.col_y = g.col_y;
    r.n = pc.s.n; r.nd = pc.s.nd; r.sqrt_n = pc.s.sqrt_n;
    hrs_feistel_split(pc.s.n, &r.pa, &r.pc);
    r.panel = sl.panel;
    first += g.reps;
    tab.push_back(r);
    plan.max_km = std::max(plan.max_km, pc.s.k * (int64_t)pc.s.m);
  }
  plan.lay = HrsPairTableLayout(plan.items, (int64_t)tab.size(), (int64_t)slots.size(), t->n, t->p, plan.panel_elems);
  if (!plan.lay.ok)
    return fail(DCOR_EINVAL, "%s: scratch bytes overflow (p = %lld, n = %lld)", entry, (long long)t->p,
                (long long)t->n);
  return DCOR_OK;
}

int plan_hrs_private_pairwise(const dcor_hrs_private_na_desc* t, const dcor_hrs_pair_segment* segs,
                              int64_t nseg, HrsPrivPairPlan& plan) {
  const char* const entry = "hrs_private_pairwise";
  plan = HrsPrivPairPlan();
  auto &tab = plan.tab; auto &slots = plan.slots;
  if (!t->D || !t->lo || !t->hi || !t->valid)
    return fail(DCOR_EINVAL, "%s: null argument (D, lo, hi, valid)", entry);
  if (t->n < 2 || t->n > 0x7fffffffLL)
    return fail(DCOR_EINVAL, "%s: n must be in [2, 2^31) (got %lld)", entry, (long long)t->n);
  if (int st = table_shape(entry, *t)) return st;
  if (!HrsPrivPairLayout::columns(t->n, t->p).ok)
    return fail(DCOR_EINVAL, "%s: p * ceil(n / 64) * 8 scratch bytes overflow (p = %lld, n = %lld)", entry,
                (long long)t->p, (long long)t->n);
  if (int st = private_release_args(entry, *t)) return st;
  if (!(t->delta > 0.0) && !std::isnan(t->delta))
    return fail(DCOR_EINVAL, "%s: delta must be positive, or NaN for 1 / n_ab per pair", entry);
  if (int st = check_alpha_nsim(t->n, t->alpha, t->nsim)) return st;
  if (int st = segment_heads(entry, segs, nseg, t->p, &plan.items)) return st;
  // every segment's pair, then its record: the private entry's at the pair's n_ab and delta
  PairSlots pairs;
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_hrs_pair_segment& g = segs[i];
    PairSlots::Pair* pr;
    if (int st = pairs.checked(entry, t->valid, t->n, g, i, &pr)) return st;
    const double delta = std::isnan(t->delta) ? 1.0 / (double)pr->n_ab : t->delta;   // rds:199
    PrematSubgConst pc;
    HrsPrivNaSegConst r;
    std::memset(&r, 0, sizeof(r));
    if (int st = private_segment_record(pr->n_ab, delta, t->alpha, t->nsim, g, first, pc, r)) return st;
    if (g.reps == 0) continue;
    if (tab.empty()) private_call_consts(pc, plan.c0);
    r.n = pc.s.n; r.nd = pc.s.nd; r.sqrt_n = pc.s.sqrt_n;
    hrs_feistel_split(pc.s.n, &r.pa, &r.pc);
    r.panel = pairs.slot(*pr, g, slots, plan.panel_elems).panel;
    r.n_x = (double)hrs_pair_count(t->valid, t->n, g.col_x, g.col_x);   // dp_sd's own n (rds:74)
    r.n_y = (double)hrs_pair_count(t->valid, t->n, g.col_y, g.col_y);
    first += g.reps;
    tab.push_back(r);
    plan.max_km = std::max(plan.max_km, pc.s.k * (int64_t)pc.s.m);
  }
  if (!tab.empty()) {   // every column's count and the place of its compacted copy
    plan.cols.resize((size_t)t->p);
    for (int64_t c = 0; c < t->p; ++c) {
      HrsPrivCol& q = plan.cols[(size_t)c];
      q.n_c = hrs_pair_count(t->valid, t->n, c, c);
      q.off = plan.comp_elems;
      plan.comp_elems += hrs_priv_col_elems(q.n_c);
    }
  }
  plan.lay = HrsPrivPairLayout(plan.items, (int64_t)tab.size(), (int64_t)slots.size(), t->n, t->p,
                               plan.comp_elems, plan.panel_elems);
  if (!plan.lay.ok)
    return fail(DCOR_EINVAL, "%s: scratch bytes overflow (p = %lld, n = %lld)", entry, (long long)t->p,
                (long long)t->n);
  private_release_plan(*t, plan.lohi, plan.pv);
  return DCOR_OK;
}

int plan_subg_panel(const dcor_subg_panel_desc* p, const dcor_subg_segment* segs, int64_t nseg,
                    SubgPanelPlan& plan) {
  plan = SubgPanelPlan();
  auto &tab = plan.tab; auto &slots = plan.slots;
  if (!p->X || !p->Y) return fail(DCOR_EINVAL, "subg_panel: null argument (X, Y)");
  if (((uintptr_t)p->X | (uintptr_t)p->Y) & 7)
    return fail(DCOR_EINVAL, "subg_panel: X and Y must be aligned to 8 bytes");
  if (p->n < 1 || p->n > 0x7fffffffLL)
    return fail(DCOR_EINVAL, "subg_panel: n must be in [1, 2^31) (got %lld)", (long long)p->n);
  if (!(p->eta1 > 0.0) || !(p->eta2 > 0.0) || !std::isfinite(p->eta1) || !std::isfinite(p->eta2))
    return fail(DCOR_EINVAL, "subg_panel: eta1, eta2 must be finite and > 0 (got %g, %g)", p->eta1, p->eta2);
  if (int st = check_alpha_nsim(p->n, p->alpha, p->nsim)) return st;
  if (int st = segment_heads("subg_panel", segs, nseg, 0, &plan.items)) return st;
  // every segment's launch constants: make_subg's own, the simulation variant (hrs = 0, no override)
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_subg_segment& g = segs[i];
    SubgConst a;
    if (int st = make_subg(p->n, g.eps1, g.eps2, p->eta1, p->eta2, p->alpha, 0, NAN, NAN, NAN, NAN, NAN,
                           NAN, p->nsim, a, nullptr, nullptr))
      return st;
    if (g.reps == 0) continue;
    if (tab.empty()) plan.c0 = a;
    SubgSegConst t;
    subg_segment_record(a, g, first, slots, t);
    first += g.reps;
    tab.push_back(t);
  }
  plan.lay = SubgPanelLayout((int64_t)tab.size(), (int64_t)slots.size(), mean_count(slots), p->n);
  return DCOR_OK;
}

int plan_subg_table(const dcor_subg_table_desc* t, const dcor_subg_pair_segment* segs, int64_t nseg,
                    SubgTablePlan& plan) {
  plan = SubgTablePlan();
  auto &tab = plan.tab; auto &slots = plan.slots;
  if (!t->D || !t->eta) return fail(DCOR_EINVAL, "subg_table: null argument (D, eta)");
  if ((uintptr_t)t->D & 7) return fail(DCOR_EINVAL, "subg_table: D must be aligned to 8 bytes");
  if (t->n < 1 || t->n > 0x7fffffffLL)
    return fail(DCOR_EINVAL, "subg_table: n must be in [1, 2^31) (got %lld)", (long long)t->n);
  if (int st = table_shape("subg_table", *t)) return st;
  if (!SubgTableLayout::columns(t->n, t->p).ok)
    return fail(DCOR_EINVAL, "subg_table: p * npad * 8 scratch bytes overflow (p = %lld, n = %lld)",
                (long long)t->p, (long long)t->n);
  for (int64_t c = 0; c < t->p; ++c)
    if (!std::isfinite(t->eta[c]) || !(t->eta[c] > 0.0))
      return fail(DCOR_EINVAL, "subg_table: column %lld: eta must be finite and > 0 (got %g)", (long long)c,
                  t->eta[c]);
  if (int st = check_alpha_nsim(t->n, t->alpha, t->nsim)) return st;
  if (int st = segment_heads("subg_table", segs, nseg, t->p, &plan.items)) return st;
  // every segment's launch constants: those of the reference call on its pair, eta and eps
  int64_t first = 0;
  for (int64_t i = 0; i < nseg; ++i) {
    const dcor_subg_pair_segment& g = segs[i];
    SubgConst a;
    if (int st = make_subg(t->n, g.eps1, g.eps2, t->eta[g.col_x], t->eta[g.col_y], t->alpha, 0, NAN, NAN, NAN,
                           NAN, NAN, NAN, t->nsim, a, nullptr, nullptr))
      return st;
    if (g.reps == 0) continue;
    if (tab.empty()) {   // the call-wide constants alone: nothing of eta, eps or the key
      SubgConst& c0 = plan.c0;
      std::memset(&c0, 0, sizeof(c0));
      c0.n = a.n; c0.nd = a.nd; c0.sqrt_n = a.sqrt_n; c0.crit = a.crit; c0.mix = a.mix;
    }
    SubgPairSegConst r;
    std::memset(&r, 0, sizeof(r));
    subg_segment_record(a, g, first, slots, r);
    r.col_x = g.col_x; r.col_y = g.col_y;
    first += g.reps;
    tab.push_back(r);
  }
  const int64_t nmeans = mean_count(slots);
  plan.lay = SubgTableLayout((int64_t)tab.size(), (int64_t)slots.size(), nmeans, t->n, t->p);
  if (!plan.lay.ok)
    return fail(DCOR_EINVAL, "subg_table: scratch bytes overflow (p = %lld, n = %lld, %lld batch means per column)",
                (long long)t->p, (long long)t->n, (long long)nmeans);
  if (!tab.empty()) {   // make_subg's own expression for l1 / l2, so the reference call's clips are these bits
    plan.clips.resize((size_t)t->p);
    for (int64_t c = 0; c < t->p; ++c) plan.clips[(size_t)c] = dcor_lambda_n((double)t->n, t->eta[c]);
  }
  return DCOR_OK;
}

}  // namespace host
}  // namespace dcor

// ===================================================================== ABI
using namespace dcor::host;

extern "C" {

int dcor_last_error(char* buf, size_t len) {
  if (buf && len) {
    std::strncpy(buf, g_err, len - 1);
    buf[len - 1] = 0;
  }
  return (int)std::strlen(g_err);
}

double dcor_lambda_n(double n, double eta) {  // ver-cor-subG.R:1
  return r_min(2.0 * eta * std::sqrt(std::log(n)), 2.0 * std::sqrt(3.0));
}

void dcor_lambda_int_n(double n, double eta_s, double eta_r, double eps_s, double out[2]) {
  out[0] = r_min(2.0 * eta_s * std::sqrt(std::log(n)), 2.0 * std::sqrt(3.0));  // ver-cor-subG.R:4
  out[1] = 5.0 * r_max(eta_r, 1.0) * r_min(std::log(n), 6.0) / (r_min(eps_s, 1.0));  // :5
}

double dcor_lambda_receiver_from_noise(double lam_s, double lam_o, double eps_s, double delta) {
  return dcor::hrs_lambda_receiver(lam_s, lam_o, eps_s, std::log(1.0 / delta));  // real-data-sims.R:172
}

double dcor_qnorm(double p) {
  // R's qnorm(p, 0, 1) (qnorm.c: Wichura's AS241, lower tail, log.p = FALSE), same operation
  // order, so crit = qnorm(1 - alpha/2) is R's double.
  if (std::isnan(p) || p < 0 || p > 1) return NAN;
  if (p == 0) return -INFINITY;
  if (p == 1) return INFINITY;
  const double q = p - 0.5;
  double r, val;
  if (std::fabs(q) <= .425) {
    r = .180625 - q * q;
    return q * (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r +
                     67265.770927008700853) * r + 45921.953931549871457) * r +
                   13731.693765509461125) * r + 1971.5909503065514427) * r +
                 133.14166789178437745) * r + 3.387132872796366608) /
           (((((((r * 5226.495278852545925 + 28729.085735721942674) * r +
                 39307.89580009271061) * r + 21213.794301586595867) * r +
               5394.1960214247511077) * r + 687.1870074920579083) * r +
             42.313330701600911252) * r + 1.);
  }
  r = std::sqrt(-std::log((q > 0) ? (0.5 - p + 0.5) : p));
  if (r <= 5.) {
    r += -1.6;
    val = (((((((r * 7.7454501427834140764e-4 + .0227238449892691845833) * r +
                .24178072517745061177) * r + 1.27045825245236838258) * r +
              3.64784832476320460504) * r + 5.7694972214606914055) * r +
            4.6303378461565452959) * r + 1.42343711074968357734) /
          (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r +
                .0151986665636164571966) * r + .14810397642748007459) * r +
              .68976733498510000455) * r + 1.6763848301838038494) * r +
            2.05319162663775882187) * r + 1.);
  } else {
    r += -5.;
    val = (((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r +
                .0012426609473880784386) * r + .026532189526576123093) * r +
              .29656057182850489123) * r + 1.7848265399172913358) * r +
            5.4637849111641143699) * r + 6.6579046435011037772) /
          (((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r +
                1.8463183175100546818e-5) * r + 7.868691311456132591e-4) * r +
              .0148753612908506148525) * r + .13692988092273580531) * r +
            .59983220655588793769) * r + 1.);
  }
  return (q < 0.0) ? -val : val;
}

int dcor_batch_geometry(int64_t n, double eps1, double eps2, int family, int hrs, int64_t km[2]) {
  const double nd = (double)n;
  double md = std::ceil(8.0 / (eps1 * eps2));
  if (family == DCOR_FAMILY_SUBG && md > nd) md = nd;
  double kd = std::floor(nd / md);
  if (family == DCOR_FAMILY_SUBG && hrs && kd < 2) { kd = 2; md = std::floor(nd / kd); }
  km[0] = (int64_t)kd; km[1] = (int64_t)md;
  if (!(kd >= 1)) return fail(DCOR_EKLT1, "k = floor(n/m) < 1");
  return DCOR_OK;
}

}  // extern "C"
