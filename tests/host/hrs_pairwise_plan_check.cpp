// hrs_pairwise_plan_check.cpp -- stand-alone check of plan_hrs_table_pairwise (csrc/dcor_plan.cpp),
// built from this file and dcor_plan.cpp alone with a host compiler: no HIP, no device.  The masks'
// counts n_ab against a per-row loop (the compaction-edge masks, the tail of the last word
// included); the slots (the distinct ordered pairs, their panels 256-B aligned and disjoint); every
// segment record against the record plan_hrs_fused_sweep builds for a panel of n_ab samples with
// the pair's delta, as bytes over the fields the two share; every rejection's code and message.
// Harness: check.h.
#include <utility>

#include "check.h"

static const double* const kD = (const double*)4096;   // never dereferenced
static const double kLam[4] = {1.75, 2.5, 3.0625, 0.9};
static const double kEps[5] = {0.1, 0.25, 1.0, 2.0, 2.45};

// The masks of p columns as rows of booleans, packed as the entry takes them; junk: set the last
// word's bits at i >= n, which must never count.
static std::vector<uint64_t> pack(const std::vector<std::vector<bool>>& rows, bool junk) {
  const int64_t n = (int64_t)rows[0].size(), nw = (n + 63) / 64;
  std::vector<uint64_t> v(rows.size() * (size_t)nw, 0);
  for (size_t c = 0; c < rows.size(); ++c) {
    for (int64_t i = 0; i < n; ++i)
      if (rows[c][(size_t)i]) v[c * (size_t)nw + (size_t)(i >> 6)] |= 1ull << (i & 63);
    if (junk && (n & 63)) v[c * (size_t)nw + (size_t)nw - 1] |= ~0ull << (n & 63);
  }
  return v;
}

static int64_t naive_count(const std::vector<bool>& a, const std::vector<bool>& b) {
  int64_t c = 0;
  for (size_t i = 0; i < a.size(); ++i) c += a[i] && b[i];
  return c;
}

// The compaction-edge masks at n rows: full, alternate bits, first row missing, last row missing,
// one whole word missing (rows 64 .. 127 where there are that many, else rows 0 .. 63 of what is
// there), only rows {0, n - 1}, and rows {0, n / 2, n - 1} (three present).
static std::vector<std::vector<bool>> edge_masks(int64_t n) {
  std::vector<std::vector<bool>> m(7, std::vector<bool>((size_t)n, true));
  for (int64_t i = 0; i < n; ++i) {
    m[1][(size_t)i] = (i & 1) == 0;
    m[4][(size_t)i] = n > 128 ? !(i >= 64 && i < 128) : !(i < 64 && i < n - 2);
    m[5][(size_t)i] = i == 0 || i == n - 1;
    m[6][(size_t)i] = i == 0 || i == n / 2 || i == n - 1;
  }
  m[2][0] = false;
  m[3][(size_t)n - 1] = false;
  return m;
}

static void check_counts() {
  const int64_t ns[] = {2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1001};
  for (int64_t n : ns) {
    const auto rows = edge_masks(n);
    for (int junk = 0; junk < 2; ++junk) {
      const std::vector<uint64_t> v = pack(rows, junk != 0);
      const auto hv = heap(v);
      for (size_t a = 0; a < rows.size(); ++a)
        for (size_t b = 0; b < rows.size(); ++b)
          CHECK(hrs_pair_count(hv.get(), n, (int64_t)a, (int64_t)b) == naive_count(rows[a], rows[b]));
    }
  }
}

static dcor_hrs_table_na_desc table_of(int64_t n, int64_t ld, const uint64_t* valid, double delta) {
  dcor_hrs_table_na_desc t;
  std::memset(&t, 0, sizeof(t));
  t.n = n; t.p = 4; t.ld = ld; t.D = kD; t.lam = kLam; t.valid = valid;
  t.alpha = 0.05; t.delta = delta; t.nsim = 2000;
  return t;
}

static const int kPairs[6][2] = {{0, 1}, {1, 0}, {2, 2}, {3, 0}, {1, 2}, {0, 1}};

// Segment i of the list: pair i % 6 ((0, 1) twice: one slot), eps i % 5, keys above 2^32, the last
// legal replicate range on odd i, and reps[i] replicates.
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
    g.col_x = kPairs[i % 6][0]; g.col_y = kPairs[i % 6][1];
    v.push_back(g);
  }
  return v;
}

// The reference record: plan_hrs_fused_sweep on a panel of n_ab samples, one segment.
static HrsSegConst reference_record(int64_t n_ab, double delta, double alpha, int64_t nsim,
                                    const dcor_hrs_pair_segment& g, int64_t* km, PrematSubgConst* p0) {
  dcor_panel pn{};
  pn.X = kD; pn.Y = kD + 8; pn.n = n_ab;
  dcor_premat_subg base;
  std::memset(&base, 0, sizeof(base));
  base.n = n_ab; base.eps1 = base.eps2 = 1.0; base.eta1 = base.eta2 = 1.0; base.alpha = alpha;
  base.hrs = 1;
  base.lam_x = base.lam_s = kLam[g.col_x];
  base.lam_y = base.lam_o = kLam[g.col_y];
  base.lam_r = NAN; base.delta = delta; base.nsim = nsim;
  base.X = pn.X; base.Y = pn.Y; base.xy_stride = 0;
  dcor_hrs_segment s;
  std::memset(&s, 0, sizeof(s));
  s.eps = g.eps; s.seed_ni = g.seed_ni; s.seed_int = g.seed_int;
  s.rep_begin = g.rep_begin; s.reps = g.reps; s.out_row = g.out_row;
  HrsFusedSweepPlan plan;
  CHECK(plan_hrs_fused_sweep(&base, &pn, &s, 1, plan) == DCOR_OK);
  CHECK(plan.tab.size() == 1 && plan.items == g.reps);
  *km = plan.max_km;
  *p0 = plan.p0;
  return plan.tab[0];
}

// Columns 0 .. 3 of the record checks: full, alternate rows, one word missing, every third row and
// the two ends missing.
static std::vector<std::vector<bool>> record_masks(int64_t n) {
  std::vector<std::vector<bool>> m(4, std::vector<bool>((size_t)n, true));
  for (int64_t i = 0; i < n; ++i) {
    m[1][(size_t)i] = (i & 1) == 0;
    m[2][(size_t)i] = !(i >= 128 && i < 192);
    m[3][(size_t)i] = !(i == 0 || i == n - 1 || i % 3 == 0);
  }
  return m;
}

static void check_records(int64_t n, double delta) {
  const std::vector<std::vector<int64_t>> kReps = {
      {3, 2, 1, 4, 5, 2}, {0, 3, 2}, {3, 0, 2}, {3, 2, 0}, {0, 0, 0}, {0, 4, 0, 1, 0}, {2}, {0},
      // every pair at every eps: 30 segments
      {1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3}};
  const auto rows = record_masks(n);
  const std::vector<uint64_t> v = pack(rows, true);
  const auto hv = heap(v);
  const dcor_hrs_table_na_desc t = table_of(n, n + 3, hv.get(), delta);
  for (const auto& reps : kReps) {
    const std::vector<dcor_hrs_pair_segment> segs = segments(reps);
    const auto hs = heap(segs);
    HrsPairTablePlan pl;
    pl.items = pl.max_km = pl.panel_elems = -1;
    CHECK(plan_hrs_table_pairwise(&t, hs.get(), (int64_t)segs.size(), pl) == DCOR_OK);
    const std::vector<HrsPairNaSegConst>& tab = pl.tab;
    const std::vector<HrsPairSlot>& slots = pl.slots;
    const PrematSubgConst& c0 = pl.c0;
    const int64_t items = pl.items, max_km = pl.max_km, panel_elems = pl.panel_elems;
    // the slots: the distinct ordered pairs of the kept segments in order of first use
    std::vector<std::pair<int, int>> want_slots;
    for (size_t i = 0; i < reps.size(); ++i) {
      if (reps[i] == 0) continue;
      const std::pair<int, int> pr(segs[i].col_x, segs[i].col_y);
      bool seen = false;
      for (const auto& w : want_slots) seen = seen || w == pr;
      if (!seen) want_slots.push_back(pr);
    }
    CHECK(slots.size() == want_slots.size());
    int64_t off = 0;
    for (size_t d = 0; d < slots.size(); ++d) {
      CHECK(slots[d].col_x == want_slots[d].first && slots[d].col_y == want_slots[d].second);
      CHECK(slots[d].n_ab == naive_count(rows[(size_t)slots[d].col_x], rows[(size_t)slots[d].col_y]));
      // 256-B aligned, disjoint, room for n_ab samples and the zero pad of an odd count
      CHECK(slots[d].panel == off && (slots[d].panel * (int64_t)sizeof(double2)) % 256 == 0);
      CHECK(hrs_pair_panel_elems(slots[d].n_ab) >= slots[d].n_ab + (slots[d].n_ab & 1));
      off += hrs_pair_panel_elems(slots[d].n_ab);
    }
    CHECK(panel_elems == off);
    size_t j = 0;
    int64_t first = 0, want_km = 0;
    for (size_t i = 0; i < reps.size(); ++i) {
      if (reps[i] == 0) continue;          // exactly the reps > 0 segments, in call order
      CHECK(j < tab.size());
      const int64_t n_ab = naive_count(rows[(size_t)segs[i].col_x], rows[(size_t)segs[i].col_y]);
      const double dl = std::isnan(delta) ? 1.0 / (double)n_ab : delta;
      int64_t km = 0;
      PrematSubgConst p0;
      HrsSegConst want = reference_record(n_ab, dl, t.alpha, t.nsim, segs[i], &km, &p0);
      CHECK(want.first == 0);
      want.first = first;                  // its place in this call
      const HrsSegConst& got = tab[j];     // the shared fields: the record's HrsSegConst part
      CHECK(std::memcmp(&got, &want, sizeof(HrsSegConst)) == 0);
      CHECK(tab[j].col_x == segs[i].col_x && tab[j].col_y == segs[i].col_y);
      // what the panel entry keeps call-wide: its n, nd, sqrt_n and the split of ceil(log2 n_ab) bits
      CHECK(tab[j].n == n_ab && tab[j].n == p0.s.n);
      CHECK(std::memcmp(&tab[j].nd, &p0.s.nd, sizeof(double)) == 0);
      CHECK(std::memcmp(&tab[j].sqrt_n, &p0.s.sqrt_n, sizeof(double)) == 0);
      int bits = 1;
      while ((1ll << bits) < n_ab) ++bits;
      CHECK(tab[j].pa == bits / 2 && tab[j].pc == bits - bits / 2);
      bool found = false;
      for (const auto& sl : slots)
        if (sl.col_x == segs[i].col_x && sl.col_y == segs[i].col_y) {
          CHECK(tab[j].panel == sl.panel);
          found = true;
        }
      CHECK(found);
      if (j == 0) {   // the call-wide constants: those of the first kept segment
        CHECK(std::memcmp(&c0.s.crit, &p0.s.crit, sizeof(double)) == 0 && c0.hrs == 1);
        CHECK(std::memcmp(&c0.s.mix, &p0.s.mix, sizeof(p0.s.mix)) == 0);
      }
      CHECK((int64_t)got.k * got.m == km && km <= n_ab);
      want_km = km > want_km ? km : want_km;
      first += reps[i];
      ++j;
    }
    CHECK(j == tab.size());
    CHECK(items == first && max_km == want_km);
    CHECK(pl.lay.ok && pl.lay.bytes == HrsPairTableLayout(items, (int64_t)tab.size(), (int64_t)slots.size(), t.n,
                                                         t.p, panel_elems).bytes);
  }
}

// The k < 2 guard at the smallest counts: n_ab = 2 and 3 give k = 2, m = 1.
static void check_tiny_pairs() {
  for (int64_t n : {63, 64, 65, 257}) {
    const auto rows = edge_masks(n);
    const std::vector<uint64_t> v = pack({rows[0], rows[5], rows[6], rows[0]}, true);
    const auto hv = heap(v);
    const dcor_hrs_table_na_desc t = table_of(n, n, hv.get(), NAN);
    for (int c = 1; c <= 2; ++c) {
      dcor_hrs_pair_segment g;
      std::memset(&g, 0, sizeof(g));
      g.eps = 2.0; g.reps = 1; g.col_x = 0; g.col_y = c;
      HrsPairTablePlan pl;
      CHECK(plan_hrs_table_pairwise(&t, &g, 1, pl) == DCOR_OK);
      const std::vector<HrsPairNaSegConst>& tab = pl.tab;
      const std::vector<HrsPairSlot>& slots = pl.slots;
      const int64_t max_km = pl.max_km, panel_elems = pl.panel_elems;
      CHECK(tab.size() == 1 && tab[0].n == c + 1 && tab[0].k == 2 && tab[0].m == 1 && max_km == 2);
      CHECK(tab[0].lr == dcor_lambda_receiver_from_noise(kLam[0], kLam[c], 2.0, 1.0 / (double)(c + 1)));
      CHECK(slots.size() == 1 && slots[0].n_ab == c + 1 && panel_elems == 16);
    }
  }
}

static void check_rejections() {
  HrsPairTablePlan pl;
  const std::vector<HrsPairNaSegConst>& tab = pl.tab;
  dcor_hrs_pair_segment g;
  std::memset(&g, 0, sizeof(g));
  g.eps = 1.0; g.reps = 1; g.col_x = 0; g.col_y = 1;
  auto plan_n = [&](const dcor_hrs_table_na_desc& t, const dcor_hrs_pair_segment* s, int64_t ns) {
    return plan_hrs_table_pairwise(&t, s, ns, pl);
  };
  auto plan = [&](const dcor_hrs_table_na_desc& t, const dcor_hrs_pair_segment& s) { return plan_n(t, &s, 1); };
  const std::vector<uint64_t> full100(4 * 2, ~0ull);
  const auto h100 = heap(full100);
  dcor_hrs_table_na_desc t = table_of(100, 100, h100.get(), NAN);
  CHECK(plan(t, g) == DCOR_OK);   // delta = NaN is the per-pair default
  CHECK(tab.size() == 1 && tab[0].n == 100);
  t.D = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = table_of(100, 100, h100.get(), NAN); t.lam = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = table_of(100, 100, nullptr, NAN);
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument (D, lam, valid)");
  CHECK_FAILS(plan(table_of(1, 1, h100.get(), NAN), g), DCOR_EINVAL, "n must be in [2, 2^31)");
  CHECK_FAILS(plan(table_of(1ll << 31, 1ll << 31, h100.get(), NAN), g), DCOR_EINVAL, "n must be in [2, 2^31)");
  t = table_of(100, 100, h100.get(), NAN); t.p = 0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "p must be in [1, 2^31)");
  CHECK_FAILS(plan(table_of(100, 99, h100.get(), NAN), g), DCOR_EINVAL, "ld = 99 < n = 100");
  const double bad[4] = {0.0, -1.0, INFINITY, NAN};
  for (double b : bad)
    for (int c = 0; c < 4; ++c) {
      double lam[4] = {kLam[0], kLam[1], kLam[2], kLam[3]};
      lam[c] = b;
      t = table_of(100, 100, h100.get(), NAN); t.lam = lam;
      const std::string want = "column " + std::to_string(c) + ": lam must be finite and > 0";
      CHECK_FAILS(plan(t, g), DCOR_EINVAL, want);
    }
  for (double d : {0.0, -0.5, -(double)INFINITY})
    CHECK_FAILS(plan(table_of(100, 100, h100.get(), d), g), DCOR_EINVAL, "delta must be positive");
  CHECK(plan(table_of(100, 100, h100.get(), 0.01), g) == DCOR_OK);
  t = table_of(100, 100, h100.get(), NAN); t.alpha = 2.0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "alpha must be < 2");
  t = table_of(100, 100, h100.get(), NAN); t.nsim = 2049;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "nsim must be in [1, 2048]");
  t = table_of(100, 100, h100.get(), NAN);
  dcor_hrs_pair_segment h = g;
  h.col_y = 4;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (0, 4) outside [0, 4)");
  h = g; h.eps = 0.0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need eps > 0");
  h = g; h.rep_begin = 0xffffffffLL; h.reps = 1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: replicate range exceeds 2^32");
  // n_ab = 0 and 1: the message names the segment and the count, also for a segment without replicates
  {
    const int64_t n = 65;
    std::vector<std::vector<bool>> rows(4, std::vector<bool>((size_t)n, true));
    for (int64_t i = 0; i < n; ++i) {
      rows[1][(size_t)i] = i == 64;            // with column 0: one row; junk bits must not lift it
      rows[2][(size_t)i] = i < 64;             // with column 1: none
    }
    const std::vector<uint64_t> v = pack(rows, true);
    const auto hv = heap(v);
    t = table_of(n, n, hv.get(), NAN);
    dcor_hrs_pair_segment two[2] = {g, g};
    two[0].col_x = 0; two[0].col_y = 2;        // n_ab = 64: fine
    two[1].col_x = 0; two[1].col_y = 1;
    CHECK_FAILS(plan_n(t, two, 2), DCOR_EINVAL, "segment 1: columns (0, 1) have n_ab = 1 ");
    two[1].col_x = 2; two[1].col_y = 1; two[1].reps = 0;
    CHECK_FAILS(plan_n(t, two, 2), DCOR_EINVAL, "segment 1: columns (2, 1) have n_ab = 0 ");
    CHECK(plan_n(t, two, 1) == DCOR_OK);
  }
  // n_ab = 65537 (n = 70000 itself is legal), and 65536 passes
  {
    const int64_t n = 70000;
    std::vector<std::vector<bool>> rows(4, std::vector<bool>((size_t)n, true));
    for (int64_t i = 0; i < n; ++i) {
      rows[1][(size_t)i] = i < 65537;
      rows[2][(size_t)i] = i >= n - 65536;
    }
    const std::vector<uint64_t> v = pack(rows, true);
    const auto hv = heap(v);
    t = table_of(n, n, hv.get(), NAN);
    h = g; h.col_x = 0; h.col_y = 3;
    CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (0, 3) have n_ab = 70000 ");
    h.col_y = 1;
    CHECK_FAILS(plan(t, h), DCOR_EINVAL, "n_ab = 65537 ");
    h.col_y = 2;
    CHECK(plan(t, h) == DCOR_OK);
    CHECK(tab.size() == 1 && tab[0].n == 65536 && tab[0].pa == 8 && tab[0].pc == 8);
  }
  // the order: the table's own fields before any segment's
  h = g; h.col_x = 9;
  CHECK_FAILS(plan(table_of(1, 1, h100.get(), NAN), h), DCOR_EINVAL, "n must be in [2, 2^31)");
}

int main() {
  check_counts();
  for (double delta : {(double)NAN, 0.003}) {
    check_records(1001, delta);
    check_records(1000, delta);
    check_records(257, delta);
  }
  check_tiny_pairs();
  check_rejections();
  std::printf("hrs_pairwise_plan_check: ok\n");
  return 0;
}
