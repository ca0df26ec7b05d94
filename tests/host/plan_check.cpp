// plan_check.cpp -- stand-alone check of the planning unit (csrc/dcor_plan.cpp): the sign and HRS
// sweep planners' tables against direct calls of the constant builders (harness: check.h).
#include "check.h"

static const double* const kX = (const double*)64;   // never dereferenced
static const double* const kY = (const double*)128;

static dcor_panel panel_of(const double* X, const double* Y, int64_t n) {
  dcor_panel pn{};
  pn.X = X; pn.Y = Y; pn.n = n;
  return pn;
}

// replicate counts with reps == 0 at the front, in the middle, at the end, everywhere, nowhere
static const std::vector<std::vector<int64_t>> kReps = {
    {0, 3, 2}, {3, 0, 2}, {3, 2, 0}, {0, 0, 0}, {0, 4, 0, 1, 0}, {2}, {0}, {1, 2, 3, 4, 5}, {0, 0, 7, 0, 0}};

struct Eps { double e1, e2; };
// n = 100: m = 8, 2, 11, 6, 64; n = 4: m = 2, 4, 3, 3, 4
static const Eps kEps100[5] = {{1.0, 1.0}, {2.0, 2.0}, {0.5, 1.5}, {2.0, 0.7}, {0.25, 0.5}};
static const Eps kEps4[5] = {{2.0, 2.0}, {1.5, 1.5}, {3.0, 1.0}, {2.0, 1.5}, {4.0, 0.5}};

static SignConst direct_sign(int64_t n, const dcor_sign_segment& g) {
  SignConst c;
  CHECK(make_sign(n, g.eps1, g.eps2, 0.05, 1, DCOR_MODE_AUTO, 1000, false, c) == DCOR_OK);
  c.k0 = (uint32_t)g.seed; c.k1 = (uint32_t)(g.seed >> 32);
  c.rep_begin = g.rep_begin;
  return c;
}

static void check_sign(int64_t n, int64_t p) {
  const Eps* eps = n == 100 ? kEps100 : kEps4;
  for (const auto& reps : kReps) {
    std::vector<dcor_sign_segment> a;
    std::vector<dcor_sign_pair_segment> b;
    for (size_t i = 0; i < reps.size(); ++i) {
      dcor_sign_segment g;
      std::memset(&g, 0, sizeof(g));
      g.eps1 = eps[i].e1; g.eps2 = eps[i].e2;
      g.seed = 0x1234567800000000ull + 77 * i;
      g.rep_begin = i % 2 ? 0xffffffffLL - reps[i] : (int64_t)(5 * i);   // odd: the last legal range
      g.reps = reps[i];
      g.out_row = (int64_t)(1000 * i + 3);
      a.push_back(g);
      dcor_sign_pair_segment h;
      std::memset(&h, 0, sizeof(h));
      h.eps1 = g.eps1; h.eps2 = g.eps2; h.seed = g.seed; h.rep_begin = g.rep_begin; h.reps = g.reps;
      h.out_row = g.out_row;
      h.col_x = (int32_t)(i % p); h.col_y = (int32_t)((i + 1) % p);
      b.push_back(h);
    }
    dcor_sign_panel_desc pd;
    std::memset(&pd, 0, sizeof(pd));
    pd.n = n; pd.X = kX; pd.Y = kY; pd.alpha = 0.05; pd.normalise = 1; pd.ci_mode = DCOR_MODE_AUTO; pd.nsim = 1000;
    dcor_sign_table_desc td;
    std::memset(&td, 0, sizeof(td));
    td.n = n; td.p = p; td.ld = n + 1; td.D = kX; td.alpha = 0.05; td.normalise = 1; td.ci_mode = DCOR_MODE_AUTO;
    td.nsim = 1000;
    const auto ha = heap(a);
    const auto hb = heap(b);
    SignPanelPlan pa;
    SignTablePlan pb;
    pa.items = pb.items = -1;
    CHECK(plan_sign_panel(&pd, ha.get(), (int64_t)a.size(), pa) == DCOR_OK);
    CHECK(plan_sign_table(&td, hb.get(), (int64_t)b.size(), pb) == DCOR_OK);
    const std::vector<SignSegConst>& ta = pa.tab;
    const std::vector<SignPairSegConst>& tb = pb.tab;
    const int64_t ia = pa.items, ib = pb.items;
    size_t j = 0;
    int64_t first = 0;
    for (size_t i = 0; i < reps.size(); ++i) {
      if (reps[i] == 0) continue;          // exactly the reps > 0 segments, in call order
      CHECK(j < ta.size() && j < tb.size());
      const SignConst want = direct_sign(n, a[i]);
      CHECK(std::memcmp(&ta[j].s, &want, sizeof(want)) == 0);
      CHECK(std::memcmp(&tb[j].s, &want, sizeof(want)) == 0);
      CHECK(ta[j].first == first && tb[j].first == first);
      CHECK(ta[j].out_row == a[i].out_row && tb[j].out_row == a[i].out_row);
      CHECK(tb[j].col_x == b[i].col_x && tb[j].col_y == b[i].col_y);
      first += reps[i];
      ++j;
    }
    CHECK(j == ta.size() && j == tb.size());
    CHECK(ia == first && ib == first);
    // the scratch is the plan's own: built once, for the kept segments
    CHECK(pa.lay.ok && pa.lay.bytes == SignPanelLayout((int64_t)ta.size(), n).bytes);
    CHECK(pb.lay.ok && pb.lay.bytes == SignTableLayout((int64_t)tb.size(), n, p).bytes);
  }
}

static dcor_premat_subg hrs_base(int64_t n, bool lam_set) {
  dcor_premat_subg d;
  std::memset(&d, 0, sizeof(d));
  d.n = n; d.eta1 = d.eta2 = 1.0; d.alpha = 0.05; d.hrs = 1;
  d.lam_x = d.lam_y = 2.0;
  d.lam_s = d.lam_o = lam_set ? 2.0 : NAN;
  d.lam_r = NAN; d.delta = 0.1; d.nsim = 10;
  d.X = kX; d.Y = kY;
  return d;
}

static void check_hrs(int64_t n, bool lam_set) {
  // eps from 0.05 to 8: m from n / 2 (k raised to 2) down to 1
  const double eps[5] = {1.0, 0.05, 8.0, 2.0, 0.5};
  const dcor_premat_subg base = hrs_base(n, lam_set);
  for (const auto& reps : kReps) {
    std::vector<dcor_hrs_segment> s;
    for (size_t i = 0; i < reps.size(); ++i) {
      dcor_hrs_segment g;
      std::memset(&g, 0, sizeof(g));
      g.eps = eps[i];
      g.seed_ni = 0xabcdef0100000000ull + i; g.seed_int = 0x1020304050607080ull - i;
      g.rep_begin = i % 2 ? 0xffffffffLL - reps[i] : (int64_t)(9 * i);
      g.reps = reps[i];
      g.out_row = (int64_t)(100 * i);
      s.push_back(g);
    }
    const auto hs = heap(s);
    const dcor_panel pn = panel_of(kX, kY, n);
    HrsFusedSweepPlan f;
    CHECK(plan_hrs_fused_sweep(&base, &pn, hs.get(), (int64_t)s.size(), f) == DCOR_OK);
    HrsSweepPlan m;
    CHECK(plan_hrs_sweep(&base, &pn, hs.get(), (int64_t)s.size(), m) == DCOR_OK);
    CHECK(f.qs.size() == s.size() && m.segs.size() == s.size());
    size_t j = 0, need = 0;
    int64_t first = 0, max_km = 0, cap = 0;
    for (size_t i = 0; i < s.size(); ++i) {
      const dcor_hrs_segment& g = s[i];
      const dcor_premat_subg q = hrs_segment_desc(base, g);
      CHECK(q.reps == g.reps && q.eps1 == g.eps && q.eps2 == g.eps && q.eta1 == 1.0 && q.eta2 == 1.0);
      CHECK(q.lam_r == dcor_lambda_receiver_from_noise(base.lam_s, base.lam_o, g.eps, base.delta) ||
            (std::isnan(q.lam_r) && !lam_set));
      CHECK(q.n == n && q.X == kX && q.Y == kY && q.hrs == 1 && q.nsim == 10);
      for (const dcor_premat_subg* got : {&f.qs[i], &m.segs[i].q})
        CHECK(got->reps == q.reps && got->eps1 == q.eps1 && got->eps2 == q.eps2 && got->eta1 == q.eta1 &&
              std::memcmp(&got->lam_r, &q.lam_r, sizeof(double)) == 0 && got->n == q.n && got->X == q.X);
      PrematSubgConst pc;
      CHECK(premat_subg_const(&q, pc) == DCOR_OK);
      // the materialised sweep's geometry and chunk
      int64_t km[2];
      CHECK(dcor_batch_geometry(n, g.eps, g.eps, DCOR_FAMILY_SUBG, 1, km) == DCOR_OK);
      CHECK(m.segs[i].k == km[0] && m.segs[i].m == km[1] && km[0] == pc.s.k && km[1] == pc.s.m);
      const size_t per = HrsNoiseLayout(n, km[0], km[1], 10, 1).bytes;
      CHECK(m.segs[i].cr == hrs_chunk(per, g.reps, (size_t)4 << 30, 8192) && m.segs[i].cr == g.reps);
      if (per * (size_t)g.reps > need) need = per * (size_t)g.reps;
      if (g.reps > cap) cap = g.reps;
      if (g.reps == 0) continue;
      CHECK(j < f.tab.size());
      const HrsSegConst& t = f.tab[j];
      const SubgConst& a = pc.s;
      if (j == 0) CHECK(std::memcmp(&f.p0, &pc, sizeof(pc)) == 0);
      CHECK(t.k == a.k && t.m == a.m && t.md_pow2 == a.md_pow2 && t.md == a.md && t.kd == a.kd &&
            t.inv_md == a.inv_md && t.bx == a.bx && t.by == a.by && t.m_over_k == a.m_over_k &&
            t.sqrt_k == a.sqrt_k && t.bs == a.bs && t.eps_r == a.eps_r && t.pad == 0);
      const double got[] = {t.lr, t.s_central, t.sn2x2, t.crit_sqrt2_s};
      const double want[] = {a.lr, a.s_central, a.sn2x2, pc.crit_sqrt2_s};
      CHECK(std::memcmp(got, want, sizeof(got)) == 0);
      CHECK(t.ni0 == (uint32_t)g.seed_ni && t.ni1 == (uint32_t)(g.seed_ni >> 32));
      CHECK(t.in0 == (uint32_t)g.seed_int && t.in1 == (uint32_t)(g.seed_int >> 32));
      CHECK(t.rep_begin == (uint32_t)g.rep_begin && t.first == first && t.out_row == g.out_row);
      if (a.k * (int64_t)a.m > max_km) max_km = a.k * (int64_t)a.m;
      first += g.reps;
      ++j;
    }
    CHECK(j == f.tab.size() && f.items == first && f.max_km == max_km);
    CHECK(m.need == need && m.cap == cap && (need == 0) == (first == 0));
    // the sweep-wide constants (the clips l1, l2, ls, lo_, nd, sqrt_n, crit, the sender, mix) do
    // not depend on a segment's eps, set or unset (NaN compares as a constant): one dictionary
    CHECK(f.wide);
  }
}

static void check_rejections() {
  // the table's scratch size: (2^31 - 1) columns of 2^31 padded samples do not fit
  {
    const int64_t big = 0x7fffffffLL;
    dcor_sign_table_desc td;
    std::memset(&td, 0, sizeof(td));
    td.n = big; td.p = big; td.ld = big; td.D = kX; td.alpha = 0.05; td.normalise = 1; td.nsim = 1000;
    std::vector<dcor_sign_pair_segment> b(1);
    std::memset(&b[0], 0, sizeof(b[0]));
    b[0].eps1 = b[0].eps2 = 1.0; b[0].reps = 1;
    const auto hb = heap(b);
    SignTablePlan tb;
    CHECK_FAILS_EXACT(plan_sign_table(&td, hb.get(), 1, tb), DCOR_EINVAL,
                "sign_table: p * npad * 8 scratch bytes overflow (p = 2147483647, n = 2147483647)");
    td.n = 100; td.p = 3; td.ld = 99;
    CHECK_FAILS_EXACT(plan_sign_table(&td, hb.get(), 1, tb), DCOR_EINVAL, "sign_table: ld = 99 < n = 100");
    td.ld = 100; b[0].col_y = 3;
    const auto hc = heap(b);
    CHECK_FAILS_EXACT(plan_sign_table(&td, hc.get(), 1, tb), DCOR_EINVAL,
                "sign_table: segment 0: columns (0, 3) outside [0, 3)");
  }
  // the HRS sweeps' panel and base checks, and their place among the segment checks
  const dcor_premat_subg base = hrs_base(100, true);
  std::vector<dcor_hrs_segment> s(2);
  std::memset(s.data(), 0, 2 * sizeof(s[0]));
  s[0].eps = 1.0; s[0].reps = 2; s[1].eps = 2.0; s[1].reps = 1;
  const auto ok = heap(s);
  s[1].reps = -1;
  const auto bad = heap(s);
  struct Case { const double* X; const double* Y; int64_t n; int hrs; double delta; const char* msg; };
  const Case cases[] = {
      {kY, kY, 100, 1, 0.1, "X, Y, n must be the panel's and xy_stride 0"},
      {kX, kX, 100, 1, 0.1, "X, Y, n must be the panel's and xy_stride 0"},
      {kX, kY, 101, 1, 0.1, "X, Y, n must be the panel's and xy_stride 0"},
      {kX, kY, 100, 0, 0.1, "the HRS variant only (hrs = 1)"},
      {kX, kY, 100, 1, 0.0, "delta must be positive"},
      {kX, kY, 100, 1, -1.0, "delta must be positive"},
      {kX, kY, 100, 1, NAN, "delta must be positive"},
  };
  for (const Case& c : cases) {
    dcor_premat_subg d = base;
    d.hrs = c.hrs; d.delta = c.delta;
    const dcor_panel pn = panel_of(c.X, c.Y, c.n);
    HrsFusedSweepPlan f;
    HrsSweepPlan m;
    CHECK_FAILS_EXACT(plan_hrs_fused_sweep(&d, &pn, ok.get(), 2, f), DCOR_EINVAL,
                std::string("hrs_fused_sweep: ") + c.msg);
    CHECK_FAILS_EXACT(plan_hrs_sweep(&d, &pn, ok.get(), 2, m), DCOR_EINVAL, std::string("hrs_sweep: ") + c.msg);
    // with a bad segment too: the fused sweep reports the segment, the materialised one the panel
    HrsFusedSweepPlan f2;
    HrsSweepPlan m2;
    CHECK_FAILS_EXACT(plan_hrs_fused_sweep(&d, &pn, bad.get(), 2, f2), DCOR_EINVAL,
                "hrs_fused_sweep: segment 1: need eps > 0, reps, rep_begin, out_row >= 0");
    CHECK_FAILS_EXACT(plan_hrs_sweep(&d, &pn, bad.get(), 2, m2), DCOR_EINVAL, std::string("hrs_sweep: ") + c.msg);
  }
  dcor_premat_subg d = base;
  d.xy_stride = 100;
  const dcor_panel pn = panel_of(kX, kY, 100);
  HrsFusedSweepPlan f;
  CHECK_FAILS_EXACT(plan_hrs_fused_sweep(&d, &pn, ok.get(), 2, f), DCOR_EINVAL,
              "hrs_fused_sweep: X, Y, n must be the panel's and xy_stride 0");
  // a bad segment is reported before the panel is read: no panel needed
  HrsFusedSweepPlan f2;
  CHECK_FAILS_EXACT(plan_hrs_fused_sweep(&base, (const dcor_panel*)8, bad.get(), 2, f2), DCOR_EINVAL,
              "hrs_fused_sweep: segment 1: need eps > 0, reps, rep_begin, out_row >= 0");
}

int main() {
  for (int64_t n : {100, 4}) {
    for (int64_t p : {1, 3}) check_sign(n, p);
    for (bool lam_set : {true, false}) check_hrs(n, lam_set);
  }
  check_rejections();
  std::printf("plan_check: ok\n");
  return 0;
}
