// hrs_table_plan_check.cpp -- stand-alone check of plan_hrs_table (csrc/dcor_plan.cpp), built from
// this file and dcor_plan.cpp alone with a host compiler: no HIP, no device.  A 4-column table
// with four distinct clip bounds; every record of the table planner must equal, as bytes over the
// fields the two records share, the record plan_hrs_fused_sweep builds for the reference call of
// the segment's pair (a panel on the two columns, lam_x = lam_s = lam[col_x], lam_y = lam_o =
// lam[col_y]).  Harness: check.h.
#include "check.h"

static const double* const kD = (const double*)4096;   // never dereferenced
static const double kLam[4] = {1.75, 2.5, 3.0625, 0.9};
static const double kEps[5] = {0.1, 0.25, 1.0, 2.0, 2.45};
static const int kPairs[4][2] = {{0, 1}, {1, 0}, {2, 2}, {3, 0}};

static dcor_hrs_table_desc table_of(int64_t n, int64_t ld) {
  dcor_hrs_table_desc t;
  std::memset(&t, 0, sizeof(t));
  t.n = n; t.p = 4; t.ld = ld; t.D = kD; t.lam = kLam;
  t.alpha = 0.05; t.delta = 1.0 / (double)n; t.nsim = 2000;
  return t;
}

// Segment i of the list: pair i % 4, eps i % 5, keys above 2^32, the last legal replicate range on
// odd i, and reps[i] replicates.
static std::vector<dcor_hrs_pair_segment> segments(const std::vector<int64_t>& reps) {
  std::vector<dcor_hrs_pair_segment> v;
  for (size_t i = 0; i < reps.size(); ++i) {
    dcor_hrs_pair_segment g;
    std::memset(&g, 0, sizeof(g));
    g.eps = kEps[i % 5];
    g.seed_ni = 0x1234567800000000ull + 77 * i;
    g.seed_int = 0x0fedcba900000000ull + 91 * i;
    g.rep_begin = i % 2 ? 0xffffffffLL - reps[i] : (int64_t)(5 * i);
    g.reps = reps[i];
    g.out_row = (int64_t)(1000 * i + 3);
    g.col_x = kPairs[i % 4][0]; g.col_y = kPairs[i % 4][1];
    v.push_back(g);
  }
  return v;
}

// The reference record: plan_hrs_fused_sweep on a panel of the pair's two columns, one segment.
static HrsSegConst reference_record(const dcor_hrs_table_desc& t, const dcor_hrs_pair_segment& g,
                                    int64_t* km) {
  const double* X = t.D + g.col_x * t.ld;
  const double* Y = t.D + g.col_y * t.ld;
  dcor_panel pn{};
  pn.X = X; pn.Y = Y; pn.n = t.n;
  dcor_premat_subg base;
  std::memset(&base, 0, sizeof(base));
  base.n = t.n; base.eps1 = base.eps2 = 1.0; base.eta1 = base.eta2 = 1.0; base.alpha = t.alpha;
  base.hrs = 1;
  base.lam_x = base.lam_s = t.lam[g.col_x];
  base.lam_y = base.lam_o = t.lam[g.col_y];
  base.lam_r = NAN; base.delta = t.delta; base.nsim = t.nsim;
  base.X = X; base.Y = Y; base.xy_stride = 0;
  dcor_hrs_segment s;
  std::memset(&s, 0, sizeof(s));
  s.eps = g.eps; s.seed_ni = g.seed_ni; s.seed_int = g.seed_int;
  s.rep_begin = g.rep_begin; s.reps = g.reps; s.out_row = g.out_row;
  HrsFusedSweepPlan plan;
  CHECK(plan_hrs_fused_sweep(&base, &pn, &s, 1, plan) == DCOR_OK);
  CHECK(plan.tab.size() == 1 && plan.items == g.reps);
  *km = plan.max_km;
  return plan.tab[0];
}

static void check_records(int64_t n) {
  const std::vector<std::vector<int64_t>> kReps = {
      {3, 2, 1, 4, 5}, {0, 3, 2}, {3, 0, 2}, {3, 2, 0}, {0, 0, 0}, {0, 4, 0, 1, 0}, {2}, {0},
      // every pair at every eps: 20 segments
      {1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2}};
  const dcor_hrs_table_desc t = table_of(n, n + 3);
  for (const auto& reps : kReps) {
    const std::vector<dcor_hrs_pair_segment> segs = segments(reps);
    const auto hs = heap(segs);
    HrsTablePlan pl;
    pl.items = pl.max_km = -1;
    CHECK(plan_hrs_table(&t, hs.get(), (int64_t)segs.size(), pl) == DCOR_OK);
    const std::vector<HrsPairSegConst>& tab = pl.tab;
    const int64_t items = pl.items, max_km = pl.max_km;
    size_t j = 0;
    int64_t first = 0, want_km = 0;
    for (size_t i = 0; i < reps.size(); ++i) {
      if (reps[i] == 0) continue;          // exactly the reps > 0 segments, in call order
      CHECK(j < tab.size());
      int64_t km = 0;
      HrsSegConst want = reference_record(t, segs[i], &km);
      CHECK(want.first == 0);
      want.first = first;                  // its place in this call
      const HrsSegConst& got = tab[j];     // the shared fields: the record's HrsSegConst part
      CHECK(std::memcmp(&got, &want, sizeof(HrsSegConst)) == 0);
      CHECK(tab[j].out_row == segs[i].out_row);
      CHECK(tab[j].col_x == segs[i].col_x && tab[j].col_y == segs[i].col_y);
      CHECK((int64_t)got.k * got.m == km && km <= n);
      want_km = km > want_km ? km : want_km;
      first += reps[i];
      ++j;
    }
    CHECK(j == tab.size());
    CHECK(items == first && max_km == want_km);
    CHECK(pl.lay.ok && pl.lay.bytes == HrsTableLayout(items, (int64_t)tab.size(), t.n, t.p).bytes);
    // the call-wide constants: the first kept segment's reference call, no columns' addresses
    for (size_t i = 0; i < reps.size(); ++i) {
      if (reps[i] == 0) continue;
      const dcor_premat_subg q = hrs_pair_desc(t, segs[i]);
      PrematSubgConst want;
      CHECK(premat_subg_const(&q, want) == DCOR_OK);
      want.X = want.Y = nullptr;
      CHECK(std::memcmp(&pl.c0, &want, sizeof(want)) == 0);
      break;
    }
  }
}

// The geometry the GPU tests rely on (n = 1000): the k < 2 guard, m = 128, 8 and the m == 2 path.
static void check_geometry() {
  const dcor_hrs_table_desc t = table_of(1000, 1000);
  const int64_t want_m[5] = {500, 128, 8, 2, 2}, want_k[5] = {2, 7, 125, 500, 500};
  for (int e = 0; e < 5; ++e) {
    dcor_hrs_pair_segment g;
    std::memset(&g, 0, sizeof(g));
    g.eps = kEps[e]; g.reps = 1; g.col_x = 3; g.col_y = 1;
    HrsTablePlan pl;
    CHECK(plan_hrs_table(&t, &g, 1, pl) == DCOR_OK);
    const std::vector<HrsPairSegConst>& tab = pl.tab;
    CHECK(tab.size() == 1 && tab[0].m == want_m[e] && tab[0].k == want_k[e]);
    // the constants that depend on lambda come from the segment's own columns
    const double ls = kLam[3], lo = kLam[1];
    CHECK(tab[0].bx == 2.0 * ls / ((double)want_m[e] * g.eps));
    CHECK(tab[0].by == 2.0 * lo / ((double)want_m[e] * g.eps));
    CHECK(tab[0].bs == 2.0 * ls / g.eps);
    CHECK(tab[0].lr == dcor_lambda_receiver_from_noise(ls, lo, g.eps, t.delta));
  }
}

static void check_rejections() {
  HrsTablePlan pl;
  dcor_hrs_pair_segment g;
  std::memset(&g, 0, sizeof(g));
  g.eps = 1.0; g.reps = 1; g.col_x = 0; g.col_y = 1;
  auto plan = [&](const dcor_hrs_table_desc& t, const dcor_hrs_pair_segment& s) {
    return plan_hrs_table(&t, &s, 1, pl);
  };
  dcor_hrs_table_desc t = table_of(100, 100);
  t.D = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = table_of(100, 100); t.lam = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  CHECK_FAILS(plan(table_of(1, 1), g), DCOR_EINVAL, "n must be in [2, 65536]");
  CHECK_FAILS(plan(table_of(65537, 65537), g), DCOR_EINVAL, "n must be in [2, 65536]");
  CHECK(plan(table_of(2, 2), g) == DCOR_OK);
  CHECK(plan(table_of(65536, 65536), g) == DCOR_OK);
  t = table_of(100, 100); t.p = 0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "p must be in [1, 2^31)");
  CHECK_FAILS(plan(table_of(100, 99), g), DCOR_EINVAL, "ld = 99 < n = 100");
  const double bad[4] = {0.0, -1.0, INFINITY, NAN};
  for (double b : bad)
    for (int c = 0; c < 4; ++c) {
      double lam[4] = {kLam[0], kLam[1], kLam[2], kLam[3]};
      lam[c] = b;
      t = table_of(100, 100); t.lam = lam;
      const std::string want = "column " + std::to_string(c) + ": lam must be finite and > 0";
      CHECK_FAILS(plan(t, g), DCOR_EINVAL, want);
    }
  t = table_of(100, 100); t.delta = 0.0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "delta must be positive");
  t = table_of(100, 100); t.alpha = 2.0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "alpha must be < 2");
  t = table_of(100, 100); t.nsim = 2049;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "nsim must be in [1, 2048]");
  t = table_of(100, 100);
  dcor_hrs_pair_segment h = g;
  h.col_y = 4;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (0, 4) outside [0, 4)");
  h = g; h.eps = 0.0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need eps > 0");
  h = g; h.rep_begin = 0xffffffffLL; h.reps = 1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: replicate range exceeds 2^32");
  h = g; h.rep_begin = 0xfffffffeLL; h.reps = 1;
  CHECK(plan(t, h) == DCOR_OK);
  // the order: the table's own fields before any segment's
  h = g; h.col_x = 9;
  t = table_of(1, 1);
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "n must be in [2, 65536]");
  // a failed call reports no items
  CHECK(pl.items == 0 && pl.max_km == 0);
}

int main() {
  check_records(1001);
  check_records(1000);
  check_records(257);
  check_geometry();
  check_rejections();
  std::printf("hrs_table_plan_check: ok\n");
  return 0;
}
