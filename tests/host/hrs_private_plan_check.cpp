// hrs_private_plan_check.cpp -- stand-alone check of plan_hrs_private and of the derivations
// dcor_hrs_private_table_launch makes per replicate on the device (hrs_lambda_consts,
// hrs_private_release: csrc/dcor_engine.h), built from this file and dcor_plan.cpp alone with a host
// compiler: no HIP, no device.  The shared derivation must give, field by field with ==, what
// plan_hrs_table writes for the same clip bounds; the release must give dcor_lambda_from_priv's
// expression; the planner's records, scratch carve and rejections are checked as in
// hrs_table_plan_check.cpp.  Harness: check.h.
#include "check.h"

static const double* const kD = (const double*)4096;   // never dereferenced
// every eps of the GPU test: the k < 2 guard, m = 8, the m == 2 path twice
static const double kEps[4] = {0.1, 1.0, 2.0, 2.45};
// clip bounds: tiny, the usual size, and 1e9 (sd = 0 -> den = 1e-8)
static const double kLam[6] = {1e-3, 0.75, 2.2, 3.0625, 4.5e4, 1e9};
static const int64_t kN[4] = {2, 1000, 1001, 65536};
static const double kLo[4] = {45.0, 15.0, -3.0, 0.25};
static const double kHi[4] = {90.0, 35.0, 3.0, 0.75};

static dcor_hrs_private_desc desc_of(int64_t n, int64_t ld) {
  dcor_hrs_private_desc t;
  std::memset(&t, 0, sizeof(t));
  t.n = n; t.p = 4; t.ld = ld; t.D = kD; t.lo = kLo; t.hi = kHi;
  t.eps_mean = 0.1; t.eps_m2 = 0.2; t.seed_std = 0x0123456789abcdefull;
  t.alpha = 0.05; t.delta = 1.0 / (double)n; t.nsim = 2000;
  return t;
}

static dcor_hrs_pair_segment segment_of(double eps, int64_t reps) {
  dcor_hrs_pair_segment g;
  std::memset(&g, 0, sizeof(g));
  g.eps = eps; g.seed_ni = 0x1234567800000011ull; g.seed_int = 0x0fedcba900000022ull;
  g.rep_begin = 0xffffffffLL - reps; g.reps = reps; g.out_row = 7; g.col_x = 0; g.col_y = 1;
  return g;
}

// hrs_lambda_consts from the private record's two host factors against plan_hrs_table's record for
// lam = {lx, ly}, and the record's lambda-independent fields against the same record.
static void check_constants() {
  for (int64_t n : kN)
    for (double eps : kEps)
      for (double lx : kLam)
        for (double ly : kLam) {
          const double lam[4] = {lx, ly, 1.0, 1.0};
          dcor_hrs_table_desc u;
          std::memset(&u, 0, sizeof(u));
          u.n = n; u.p = 4; u.ld = n; u.D = kD; u.lam = lam;
          u.alpha = 0.05; u.delta = 1.0 / (double)n; u.nsim = 2000;
          const dcor_hrs_pair_segment g = segment_of(eps, 3);
          HrsTablePlan want;
          CHECK(plan_hrs_table(&u, &g, 1, want) == DCOR_OK);
          CHECK(want.tab.size() == 1);
          const HrsPairSegConst& w = want.tab[0];

          const dcor_hrs_private_desc t = desc_of(n, n);
          HrsPrivatePlan pl;
          CHECK(plan_hrs_private(&t, &g, 1, pl) == DCOR_OK);
          CHECK(pl.tab.size() == 1 && pl.items == 3);
          const HrsPrivSegConst& r = pl.tab[0];
          CHECK(r.log_inv_delta == std::log(1.0 / t.delta));
          CHECK(r.crit_sqrt2 == want.c0.s.crit * std::sqrt(2.0));

          const HrsLamConst c = hrs_lambda_consts(lx, ly, r.eps_r, r.md, pl.c0.s.nd, r.log_inv_delta, r.crit_sqrt2);
          CHECK(c.bx == w.bx);
          CHECK(c.by == w.by);
          CHECK(c.bs == w.bs);
          CHECK(c.lr == w.lr);
          CHECK(c.s_central == w.s_central);
          CHECK(c.sn2x2 == w.sn2x2);
          CHECK(c.crit_sqrt2_s == w.crit_sqrt2_s);
          CHECK(std::isfinite(c.lr) && c.lr > 0.0 && std::isfinite(c.crit_sqrt2_s));

          // the record: plan_hrs_table's with the lambda-dependent fields zeroed
          HrsPairSegConst z = w;
          z.bx = z.by = z.bs = z.lr = z.s_central = z.sn2x2 = z.crit_sqrt2_s = 0.0;
          const HrsPairSegConst& got = r;
          CHECK(std::memcmp(&got, &z, sizeof(HrsPairSegConst)) == 0);
          CHECK(pl.max_km == want.max_km);
          // the call-wide constants the kernels read
          CHECK(pl.c0.s.n == want.c0.s.n && pl.c0.s.nd == want.c0.s.nd && pl.c0.s.sqrt_n == want.c0.s.sqrt_n);
          CHECK(pl.c0.s.crit == want.c0.s.crit && pl.c0.hrs == 1);
          CHECK(std::memcmp(&pl.c0.s.mix, &want.c0.s.mix, sizeof(MixConst)) == 0);
        }
}

// hrs_private_release against the host helpers' expressions (dcor_dp_sd's scales and k_dp_sd's
// lines, dcor_standardize_dp's denominator, dcor_lambda_from_priv), the degenerate sd included.
static void check_release() {
  const double m1s[3] = {67.25, 45.0, 90.0}, laps[4] = {0.0, -1.75, 2.5, 40.0};
  for (int64_t n : kN)
    for (double m1 : m1s)
      for (double l0 : laps)
        for (double l1 : laps) {
          const double lo = 45.0, hi = 90.0, e1 = 0.1, e2 = 0.3, nd = (double)n;
          const double m2 = m1 * m1 + (m1 == 67.25 ? 30.0 : 0.0);   // a constant column: m2 = m1^2
          const HrsPriv r = hrs_private_release(m1, m2, lo, hi, nd, e1, e2, l0, l1);
          const double s_mu = (hi - lo) / (nd * e1), s_m2 = (hi * hi - lo * lo) / (nd * e2);
          const double mu = m1 + s_mu * l0, m2p = m2 + s_m2 * l1;
          const double sd = std::sqrt(r_max(m2p - mu * mu, 0.0));
          const double sig = r_max(sd, 1e-8);
          CHECK(r.mean == mu && r.sd == sd && r.den == sig);
          CHECK(r.lam == r_max(std::fabs((lo - mu) / sig), std::fabs((hi - mu) / sig)));
          CHECK(std::isfinite(r.lam) && r.lam > 0.0 && r.den >= 1e-8);
        }
  // a NaN mean reaches every field
  const HrsPriv q = hrs_private_release(NAN, 1.0, 0.0, 1.0, 10.0, 0.1, 0.1, 0.5, 0.5);
  CHECK(std::isnan(q.mean) && std::isnan(q.sd) && std::isnan(q.den) && std::isnan(q.lam));
  CHECK(hrs_lambda_receiver(2.0, 3.0, 0.5, std::log(1.0 / 0.01)) ==
        dcor_lambda_receiver_from_noise(2.0, 3.0, 0.5, 0.01));
}

// Several segments: exactly the reps > 0 ones in call order, firsts, columns, and the scratch carve.
static void check_table_and_carve() {
  for (int64_t n : {1000, 1001, 65536}) {
    const dcor_hrs_private_desc t = desc_of(n, n + 3);
    std::vector<dcor_hrs_pair_segment> segs;
    const int64_t reps[6] = {3, 0, 2, 5, 0, 1};
    for (int i = 0; i < 6; ++i) {
      dcor_hrs_pair_segment g = segment_of(kEps[i % 4], reps[i]);
      g.col_x = i % 4; g.col_y = (i + 1) % 4; g.out_row = 100 * i; g.rep_begin = 11 * i;
      segs.push_back(g);
    }
    const auto hs = heap(segs);
    HrsPrivatePlan pl;
    CHECK(plan_hrs_private(&t, hs.get(), (int64_t)segs.size(), pl) == DCOR_OK);
    CHECK(pl.tab.size() == 4 && pl.items == 11);
    size_t j = 0;
    int64_t first = 0;
    for (int i = 0; i < 6; ++i) {
      if (reps[i] == 0) continue;
      const HrsPrivSegConst& r = pl.tab[j++];
      CHECK(r.first == first && r.out_row == 100 * i && r.col_x == i % 4 && r.col_y == (i + 1) % 4);
      CHECK(r.rep_begin == (uint32_t)(11 * i) && r.eps_r == kEps[i % 4]);
      CHECK(r.ni0 == 0x00000011u && r.ni1 == 0x12345678u && r.in0 == 0x00000022u && r.in1 == 0x0fedcba9u);
      first += reps[i];
    }
    CHECK(pl.pv.eps_mean == 0.1 && pl.pv.eps_m2 == 0.2 && pl.pv.k0 == 0x89abcdefu && pl.pv.k1 == 0x01234567u);
    CHECK(pl.lohi.size() == 8);
    for (int c = 0; c < 4; ++c) CHECK(pl.lohi[2 * c] == kLo[c] && pl.lohi[2 * c + 1] == kHi[c]);
    // the carve: 80 B per replicate | the table | 16 B per column (lo, hi) | 16 B per column (m1, m2)
    // | 8 B per sample and column at pitch npad; every region 256-B aligned, none overlapping
    const HrsPrivateLayout& lay = pl.lay;
    const int64_t npad = (n + 3) & ~(int64_t)3;
    CHECK(lay.ok && lay.npad == npad);
    CHECK(lay.tab_off == al256(11 * sizeof(SubgPartial)));
    CHECK(lay.lohi_off == al256(lay.tab_off + 4 * sizeof(HrsPrivSegConst)));
    CHECK(lay.m12_off == al256(lay.lohi_off + 4 * 16));
    CHECK(lay.cols_off == al256(lay.m12_off + 4 * 16));
    CHECK(lay.bytes == lay.cols_off + (size_t)(4 * npad) * sizeof(double));
    CHECK(lay.bytes == HrsPrivateLayout(11, 4, n, 4).bytes);
    CHECK(sizeof(SubgPartial) == 80 && sizeof(HrsPrivSegConst) == 184);
  }
  // columns that cannot be held are refused by the carver, not wrapped
  CHECK(!HrsPrivateLayout::columns(65536, (int64_t)1 << 62).ok);
}

static void check_rejections() {
  HrsPrivatePlan pl;
  const dcor_hrs_pair_segment g = segment_of(1.0, 1);
  auto plan = [&](const dcor_hrs_private_desc& t, const dcor_hrs_pair_segment& s) {
    return plan_hrs_private(&t, &s, 1, pl);
  };
  dcor_hrs_private_desc t = desc_of(100, 100);
  CHECK(plan(t, g) == DCOR_OK);
  t.D = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = desc_of(100, 100); t.lo = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = desc_of(100, 100); t.hi = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  CHECK_FAILS(plan(desc_of(1, 1), g), DCOR_EINVAL, "n must be in [2, 65536]");
  CHECK_FAILS(plan(desc_of(65537, 65537), g), DCOR_EINVAL, "n must be in [2, 65536]");
  CHECK(plan(desc_of(2, 2), g) == DCOR_OK);
  CHECK(plan(desc_of(65536, 65536), g) == DCOR_OK);
  t = desc_of(100, 100); t.p = 0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "p must be in [1, 2^31)");
  CHECK_FAILS(plan(desc_of(100, 99), g), DCOR_EINVAL, "ld = 99 < n = 100");
  t = desc_of(100, 100); t.D = (const double*)4100;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "D must be aligned to 8 bytes");
  for (int c = 0; c < 4; ++c) {
    const std::string want = "column " + std::to_string(c) + ": need finite lo < hi";
    const double bad_lo[4] = {NAN, -INFINITY, kHi[c], kHi[c] + 1.0};
    for (double b : bad_lo) {
      double lo[4] = {kLo[0], kLo[1], kLo[2], kLo[3]};
      lo[c] = b;
      t = desc_of(100, 100); t.lo = lo;
      CHECK_FAILS(plan(t, g), DCOR_EINVAL, want);
    }
    const double bad_hi[3] = {NAN, INFINITY, kLo[c]};
    for (double b : bad_hi) {
      double hi[4] = {kHi[0], kHi[1], kHi[2], kHi[3]};
      hi[c] = b;
      t = desc_of(100, 100); t.hi = hi;
      CHECK_FAILS(plan(t, g), DCOR_EINVAL, want);
    }
  }
  const double bad_eps[4] = {0.0, -0.1, INFINITY, NAN};
  for (double b : bad_eps) {
    t = desc_of(100, 100); t.eps_mean = b;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "eps_mean, eps_m2 must be finite and > 0");
    t = desc_of(100, 100); t.eps_m2 = b;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "eps_mean, eps_m2 must be finite and > 0");
  }
  const double bad_delta[3] = {0.0, -0.5, NAN};
  for (double b : bad_delta) {
    t = desc_of(100, 100); t.delta = b;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "delta must be positive");
  }
  t = desc_of(100, 100); t.alpha = 2.0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "alpha must be < 2");
  t = desc_of(100, 100); t.nsim = 2049;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "nsim must be in [1, 2048]");
  t = desc_of(100, 100);
  dcor_hrs_pair_segment h = g;
  h.col_y = 4;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (0, 4) outside [0, 4)");
  h = g; h.col_x = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (-1, 1) outside [0, 4)");
  const double bad_seg_eps[3] = {0.0, -1.0, NAN};
  for (double b : bad_seg_eps) {
    h = g; h.eps = b;
    CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need eps > 0");
  }
  h = g; h.eps = INFINITY;
  CHECK(plan(t, h) == DCOR_EINVAL);
  h = g; h.reps = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need eps > 0, reps, rep_begin, out_row >= 0");
  h = g; h.rep_begin = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0");
  h = g; h.out_row = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0");
  h = g; h.rep_begin = 0xffffffffLL; h.reps = 1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: replicate range exceeds 2^32");
  h = g; h.rep_begin = 0xfffffffeLL; h.reps = 1;
  CHECK(plan(t, h) == DCOR_OK);
  // a bad segment without replicates is refused too; the table's own fields come before any segment's
  h = g; h.reps = 0; h.col_x = 9;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns");
  CHECK_FAILS(plan(desc_of(1, 1), h), DCOR_EINVAL, "n must be in [2, 65536]");
  // a failed call reports nothing to run; a call without replicates plans nothing
  CHECK(pl.items == 0 && pl.max_km == 0 && pl.tab.empty());
  h = g; h.reps = 0;
  CHECK(plan(t, h) == DCOR_OK && pl.items == 0 && pl.tab.empty());
}

int main() {
  check_constants();
  check_release();
  check_table_and_carve();
  check_rejections();
  std::printf("hrs_private_plan_check: ok\n");
  return 0;
}
