// hrs_private_pairwise_plan_check.cpp -- stand-alone check of plan_hrs_private_pairwise
// (csrc/dcor_plan.cpp), built from this file and dcor_plan.cpp alone with a host compiler: no HIP, no
// device.  Every record field against what plan_hrs_private gives at n = n_ab and the pair's delta,
// plus the pair's slot from plan_hrs_table_pairwise; the column counts against the single-mask
// popcounts (they differ from n_ab in the fixture); log_inv_delta following n_ab when delta is NaN;
// hrs_lambda_consts at the record's n_ab against plan_hrs_table_pairwise's record; the scratch carve;
// every rejection's code and message.  Harness: check.h.
#include "check.h"

static const double* const kD = (const double*)4096;   // never dereferenced
static const double kEps[4] = {0.1, 1.0, 2.0, 2.45};
static const double kLo[4] = {45.0, 15.0, -3.0, 0.25};
static const double kHi[4] = {90.0, 35.0, 3.0, 0.75};
static const double kLam[4] = {1.75, 2.5, 3.0625, 0.9};
static const int kPairs[6][2] = {{0, 1}, {1, 0}, {2, 2}, {3, 0}, {1, 2}, {0, 1}};

// Column c keeps row i unless (i + c) % (4 + c) == 0, and column 3 also drops a whole mask word: every
// column has gaps of its own, so n_c > n_ab for every pair of different columns.  junk: the last
// word's bits at i >= n set, which must never count.
static bool present(int64_t c, int64_t i) { return (i + c) % (4 + c) != 0 && !(c == 3 && i >= 64 && i < 128); }
static std::vector<uint64_t> masks_of(int64_t n, bool full) {
  const int64_t nw = (n + 63) / 64;
  std::vector<uint64_t> v((size_t)(4 * nw), 0);
  for (int64_t c = 0; c < 4; ++c) {
    for (int64_t i = 0; i < n; ++i)
      if (full || present(c, i)) v[(size_t)(c * nw + (i >> 6))] |= 1ull << (i & 63);
    if (n & 63) v[(size_t)(c * nw + nw - 1)] |= ~0ull << (n & 63);
  }
  return v;
}
static int64_t naive_count(int64_t n, int64_t a, int64_t b) {
  int64_t k = 0;
  for (int64_t i = 0; i < n; ++i) k += present(a, i) && present(b, i);
  return k;
}

static dcor_hrs_private_na_desc desc_of(int64_t n, int64_t ld, const uint64_t* valid, double delta) {
  dcor_hrs_private_na_desc t;
  std::memset(&t, 0, sizeof(t));
  t.n = n; t.p = 4; t.ld = ld; t.D = kD; t.lo = kLo; t.hi = kHi; t.valid = valid;
  t.eps_mean = 0.1; t.eps_m2 = 0.2; t.seed_std = 0x0123456789abcdefull;
  t.alpha = 0.05; t.delta = delta; t.nsim = 2000;
  return t;
}

static std::vector<dcor_hrs_pair_segment> segments(const std::vector<int64_t>& reps) {
  std::vector<dcor_hrs_pair_segment> v;
  for (size_t i = 0; i < reps.size(); ++i) {
    dcor_hrs_pair_segment g;
    std::memset(&g, 0, sizeof(g));
    g.eps = kEps[i % 4];
    g.seed_ni = 0x1234567800000000ull + 77 * i;
    g.seed_int = 0x0fedcba900000000ull + 91 * i;
    g.rep_begin = i % 2 ? 0xffffffffLL - reps[i] : (int64_t)(5 * i);
    g.reps = reps[i];
    g.out_row = (int64_t)(1000 * i + 3);
    g.col_x = kPairs[i % 6][0]; g.col_y = kPairs[i % 6][1];
    v.push_back(g);
  }
  return v;
}

static void check_records(int64_t n, double delta) {
  const std::vector<std::vector<int64_t>> kReps = {{3, 2, 1, 4, 5, 2}, {0, 3, 2}, {3, 0, 2}, {0, 0, 0}, {2},
                                                   {1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3}};
  const std::vector<uint64_t> v = masks_of(n, false);
  const auto hv = heap(v);
  const dcor_hrs_private_na_desc t = desc_of(n, n + 3, hv.get(), delta);
  dcor_hrs_table_na_desc u;   // the pairwise entry on the same masks: the slots and the lambda constants
  std::memset(&u, 0, sizeof(u));
  u.n = n; u.p = 4; u.ld = n + 3; u.D = kD; u.lam = kLam; u.valid = hv.get();
  u.alpha = 0.05; u.delta = delta; u.nsim = 2000;
  for (const auto& reps : kReps) {
    const auto segs = segments(reps);
    const auto hs = heap(segs);
    HrsPrivPairPlan pl;
    CHECK(plan_hrs_private_pairwise(&t, hs.get(), (int64_t)segs.size(), pl) == DCOR_OK);
    HrsPairTablePlan pw;
    CHECK(plan_hrs_table_pairwise(&u, hs.get(), (int64_t)segs.size(), pw) == DCOR_OK);
    // the slot table is plan_hrs_table_pairwise's
    CHECK(pl.slots.size() == pw.slots.size() && pl.panel_elems == pw.panel_elems);
    CHECK(pl.slots.empty() ||
          std::memcmp(pl.slots.data(), pw.slots.data(), pl.slots.size() * sizeof(HrsPairSlot)) == 0);
    CHECK(pl.tab.size() == pw.tab.size() && pl.items == pw.items && pl.max_km == pw.max_km);
    size_t j = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
      if (reps[i] == 0) continue;
      const dcor_hrs_pair_segment& g = segs[i];
      const HrsPrivNaSegConst& r = pl.tab[j];
      const HrsPairNaSegConst& w = pw.tab[j];
      ++j;
      const int64_t n_ab = naive_count(n, g.col_x, g.col_y);
      // the private entry's record at n = n_ab and the pair's delta
      dcor_hrs_private_desc q;
      std::memset(&q, 0, sizeof(q));
      q.n = n_ab; q.p = 4; q.ld = n_ab; q.D = kD; q.lo = kLo; q.hi = kHi;
      q.eps_mean = 0.1; q.eps_m2 = 0.2; q.seed_std = t.seed_std;
      q.alpha = 0.05; q.delta = std::isnan(delta) ? 1.0 / (double)n_ab : delta; q.nsim = 2000;
      HrsPrivatePlan one;
      CHECK(plan_hrs_private(&q, &g, 1, one) == DCOR_OK && one.tab.size() == 1);
      HrsPrivSegConst z = one.tab[0];
      z.first = r.first;   // its place in this call
      const HrsPrivSegConst& got = r;
      CHECK(std::memcmp(&got, &z, sizeof(HrsPrivSegConst)) == 0);
      CHECK(r.log_inv_delta == std::log(1.0 / q.delta));
      if (std::isnan(delta)) CHECK(r.log_inv_delta == std::log(1.0 / (1.0 / (double)n_ab)));
      // what the pairwise record adds, and its place
      CHECK(r.n == n_ab && r.n == w.n && r.nd == w.nd && r.sqrt_n == w.sqrt_n);
      CHECK(r.pa == w.pa && r.pc == w.pc && r.panel == w.panel && r.first == w.first && r.out_row == w.out_row);
      CHECK(r.nd == one.c0.s.nd && r.sqrt_n == one.c0.s.sqrt_n);
      // the columns' own counts: the single-mask popcounts, larger than n_ab for two different columns
      CHECK(r.n_x == (double)naive_count(n, g.col_x, g.col_x) && r.n_y == (double)naive_count(n, g.col_y, g.col_y));
      if (g.col_x != g.col_y) CHECK(r.n_x > r.nd && r.n_y > r.nd);
      else CHECK(r.n_x == r.nd && r.n_y == r.nd);
      // the device derivation at the record's n_ab gives the pairwise entry's constants for lam = kLam
      const HrsLamConst c = hrs_lambda_consts(kLam[g.col_x], kLam[g.col_y], r.eps_r, r.md, r.nd, r.log_inv_delta,
                                              r.crit_sqrt2);
      CHECK(c.bx == w.bx && c.by == w.by && c.bs == w.bs && c.lr == w.lr);
      CHECK(c.s_central == w.s_central && c.sn2x2 == w.sn2x2 && c.crit_sqrt2_s == w.crit_sqrt2_s);
    }
    CHECK(j == pl.tab.size());
    if (pl.tab.empty()) {
      CHECK(pl.cols.empty() && pl.comp_elems == 0 && pl.items == 0);
      continue;
    }
    CHECK(pl.c0.s.crit == pw.c0.s.crit && pl.c0.hrs == 1 && pl.c0.s.sender_is_X == 1);
    CHECK(std::memcmp(&pl.c0.s.mix, &pw.c0.s.mix, sizeof(MixConst)) == 0);
    CHECK(pl.pv.eps_mean == 0.1 && pl.pv.eps_m2 == 0.2 && pl.pv.k0 == 0x89abcdefu && pl.pv.k1 == 0x01234567u);
    CHECK(pl.lohi.size() == 8);
    for (int c = 0; c < 4; ++c) CHECK(pl.lohi[2 * c] == kLo[c] && pl.lohi[2 * c + 1] == kHi[c]);
    // the column table: every column's count, the copies 256-B aligned, disjoint and in order
    CHECK(pl.cols.size() == 4);
    int64_t off = 0;
    for (int c = 0; c < 4; ++c) {
      CHECK(pl.cols[(size_t)c].n_c == naive_count(n, c, c) && pl.cols[(size_t)c].off == off);
      CHECK(off % 32 == 0);
      off += (pl.cols[(size_t)c].n_c + 31) / 32 * 32;
    }
    CHECK(pl.comp_elems == off);
    // the carve: 80 B per replicate | the three tables | lo, hi | m1, m2 | the masks | 8 B per present
    // row | 16 B per panel element; every region 256-B aligned, none overlapping
    const HrsPrivPairLayout& lay = pl.lay;
    const int64_t nw = (n + 63) / 64;
    CHECK(lay.ok && lay.nw == nw);
    CHECK(lay.tab_off == al256((size_t)pl.items * sizeof(SubgPartial)));
    CHECK(lay.slot_off == al256(lay.tab_off + pl.tab.size() * sizeof(HrsPrivNaSegConst)));
    CHECK(lay.col_off == al256(lay.slot_off + pl.slots.size() * sizeof(HrsPairSlot)));
    CHECK(lay.lohi_off == al256(lay.col_off + 4 * sizeof(HrsPrivCol)));
    CHECK(lay.m12_off == al256(lay.lohi_off + 4 * 16));
    CHECK(lay.mask_off == al256(lay.m12_off + 4 * 16));
    CHECK(lay.comp_off == al256(lay.mask_off + (size_t)(4 * nw) * sizeof(uint64_t)));
    CHECK(lay.panel_off == al256(lay.comp_off + (size_t)pl.comp_elems * sizeof(double)));
    CHECK(lay.bytes == lay.panel_off + (size_t)pl.panel_elems * sizeof(double2));
    CHECK(sizeof(HrsPrivNaSegConst) == 240 && sizeof(HrsPrivCol) == 16);
  }
}

// Every mask bit set and delta = 1 / n: the records are the private entry's, the counts all n.
static void check_full_masks(int64_t n) {
  const std::vector<uint64_t> v = masks_of(n, true);
  const auto hv = heap(v);
  const dcor_hrs_private_na_desc t = desc_of(n, n, hv.get(), 1.0 / (double)n);
  dcor_hrs_private_desc q;
  std::memset(&q, 0, sizeof(q));
  q.n = n; q.p = 4; q.ld = n; q.D = kD; q.lo = kLo; q.hi = kHi;
  q.eps_mean = 0.1; q.eps_m2 = 0.2; q.seed_std = t.seed_std; q.alpha = 0.05; q.delta = 1.0 / (double)n; q.nsim = 2000;
  const auto segs = segments({3, 0, 2, 1, 4});
  const auto hs = heap(segs);
  HrsPrivPairPlan pl;
  HrsPrivatePlan pr;
  CHECK(plan_hrs_private_pairwise(&t, hs.get(), (int64_t)segs.size(), pl) == DCOR_OK);
  CHECK(plan_hrs_private(&q, hs.get(), (int64_t)segs.size(), pr) == DCOR_OK);
  CHECK(pl.tab.size() == pr.tab.size() && pl.items == pr.items && pl.max_km == pr.max_km);
  for (size_t j = 0; j < pl.tab.size(); ++j) {
    const HrsPrivSegConst& got = pl.tab[j];
    CHECK(std::memcmp(&got, &pr.tab[j], sizeof(HrsPrivSegConst)) == 0);
    CHECK(pl.tab[j].n == n && pl.tab[j].nd == pr.c0.s.nd && pl.tab[j].sqrt_n == pr.c0.s.sqrt_n);
    CHECK(pl.tab[j].n_x == (double)n && pl.tab[j].n_y == (double)n);
    int pa, pc;
    hrs_feistel_split(n, &pa, &pc);
    CHECK(pl.tab[j].pa == pa && pl.tab[j].pc == pc);
  }
}

static void check_rejections() {
  HrsPrivPairPlan pl;
  const int64_t n = 200;
  const std::vector<uint64_t> v = masks_of(n, false);
  const auto hv = heap(v);
  dcor_hrs_pair_segment g = segments({1})[0];
  auto plan = [&](const dcor_hrs_private_na_desc& t, const dcor_hrs_pair_segment& s) {
    return plan_hrs_private_pairwise(&t, &s, 1, pl);
  };
  auto ok_desc = [&]() { return desc_of(n, n, hv.get(), NAN); };
  dcor_hrs_private_na_desc t = ok_desc();
  CHECK(plan(t, g) == DCOR_OK);
  t.delta = 0.01;
  CHECK(plan(t, g) == DCOR_OK);
  for (int which = 0; which < 4; ++which) {
    t = ok_desc();
    if (which == 0) t.D = nullptr;
    if (which == 1) t.lo = nullptr;
    if (which == 2) t.hi = nullptr;
    if (which == 3) t.valid = nullptr;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument (D, lo, hi, valid)");
  }
  t = ok_desc(); t.n = 1;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "n must be in [2, 2^31)");
  t = ok_desc(); t.n = (int64_t)1 << 31; t.ld = t.n;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "n must be in [2, 2^31)");
  t = ok_desc(); t.p = 0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "p must be in [1, 2^31)");
  t = ok_desc(); t.ld = n - 1;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "ld = 199 < n = 200");
  t = ok_desc(); t.D = (const double*)4100;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "D must be aligned to 8 bytes");
  for (int c = 0; c < 4; ++c) {
    const std::string want = "column " + std::to_string(c) + ": need finite lo < hi";
    const double bad_lo[4] = {NAN, -INFINITY, kHi[c], kHi[c] + 1.0};
    for (double b : bad_lo) {
      double lo[4] = {kLo[0], kLo[1], kLo[2], kLo[3]};
      lo[c] = b;
      t = ok_desc(); t.lo = lo;
      CHECK_FAILS(plan(t, g), DCOR_EINVAL, want);
    }
    const double bad_hi[2] = {NAN, INFINITY};
    for (double b : bad_hi) {
      double hi[4] = {kHi[0], kHi[1], kHi[2], kHi[3]};
      hi[c] = b;
      t = ok_desc(); t.hi = hi;
      CHECK_FAILS(plan(t, g), DCOR_EINVAL, want);
    }
  }
  const double bad_eps[4] = {0.0, -0.1, INFINITY, NAN};
  for (double b : bad_eps) {
    t = ok_desc(); t.eps_mean = b;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "eps_mean, eps_m2 must be finite and > 0");
    t = ok_desc(); t.eps_m2 = b;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "eps_mean, eps_m2 must be finite and > 0");
  }
  const double bad_delta[2] = {0.0, -0.5};
  for (double b : bad_delta) {
    t = ok_desc(); t.delta = b;
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "delta must be positive, or NaN");
  }
  t = ok_desc(); t.alpha = 2.0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "alpha must be < 2");
  t = ok_desc(); t.nsim = 2049;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "nsim must be in [1, 2048]");
  t = ok_desc();
  dcor_hrs_pair_segment h = g;
  h.col_y = 4;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (0, 4) outside [0, 4)");
  h = g; h.eps = 0.0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need eps > 0");
  h = g; h.reps = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need eps > 0, reps, rep_begin, out_row >= 0");
  h = g; h.rep_begin = 0xffffffffLL; h.reps = 1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: replicate range exceeds 2^32");
  h = g; h.rep_begin = 0xfffffffeLL; h.reps = 1;
  CHECK(plan(t, h) == DCOR_OK);
  // a pair with one pairwise-complete row, and one with none, with and without replicates
  {
    const int64_t nw = (n + 63) / 64;
    std::vector<uint64_t> m((size_t)(4 * nw), ~0ull);
    for (int64_t w = 0; w < nw; ++w) m[(size_t)(nw + w)] = 0;
    m[(size_t)nw + 1] = 1ull << 5;   // column 1: row 69 only
    for (int64_t w = 0; w < nw; ++w) m[(size_t)(2 * nw + w)] = 0;   // column 2: nothing
    const auto hm = heap(m);
    t = desc_of(n, n, hm.get(), NAN);
    const dcor_hrs_pair_segment two[2] = {segments({1})[0], segments({1, 1, 1, 1})[3]};   // (0, 1), (3, 0)
    dcor_hrs_pair_segment s2[2] = {two[1], two[0]};
    CHECK_FAILS(plan_hrs_private_pairwise(&t, s2, 2, pl), DCOR_EINVAL, "segment 1: columns (0, 1) have n_ab = 1 ");
    s2[1].reps = 0;
    CHECK_FAILS(plan_hrs_private_pairwise(&t, s2, 2, pl), DCOR_EINVAL, "segment 1: columns (0, 1) have n_ab = 1 ");
    s2[1].col_x = 2; s2[1].col_y = 2;
    CHECK_FAILS(plan_hrs_private_pairwise(&t, s2, 2, pl), DCOR_EINVAL, "segment 1: columns (2, 2) have n_ab = 0 ");
    CHECK(plan_hrs_private_pairwise(&t, s2, 1, pl) == DCOR_OK && pl.tab.size() == 1 && pl.tab[0].n == n);
    CHECK(pl.cols[1].n_c == 1 && pl.cols[2].n_c == 0 && pl.cols[3].n_c == n);
  }
  // n = 70000 with full masks: n_ab > 65536
  {
    const int64_t big = 70000;
    const std::vector<uint64_t> m = masks_of(big, true);
    const auto hm = heap(m);
    t = desc_of(big, big, hm.get(), NAN);
    CHECK_FAILS(plan(t, g), DCOR_EINVAL, "segment 0: columns (0, 1) have n_ab = 70000 ");
    CHECK(last_error().find("must be in [2, 65536]") != std::string::npos);
  }
  // a call refused for its pairs plans no record, slot or column; one refused before its segments
  // reports nothing to run; a call without replicates plans nothing
  CHECK(pl.max_km == 0 && pl.tab.empty() && pl.slots.empty() && pl.cols.empty());
  t = ok_desc(); t.alpha = 2.0;
  CHECK(plan(t, g) == DCOR_EINVAL && pl.items == 0 && pl.tab.empty());
  t = ok_desc();
  h = g; h.reps = 0;
  CHECK(plan(t, h) == DCOR_OK && pl.items == 0 && pl.tab.empty() && pl.cols.empty());
  // scratch that cannot be held is refused by the carver, not wrapped
  CHECK(!HrsPrivPairLayout(1, 1, 1, 1000, 4, (int64_t)1 << 62, 16).ok);
  CHECK(!HrsPrivPairLayout::columns((int64_t)1 << 40, (int64_t)1 << 30).ok);
}

int main() {
  for (int64_t n : {200, 1000, 1001}) {
    check_records(n, NAN);
    check_records(n, 0.004);
    check_full_masks(n);
  }
  check_rejections();
  std::printf("hrs_private_pairwise_plan_check: ok\n");
  return 0;
}
