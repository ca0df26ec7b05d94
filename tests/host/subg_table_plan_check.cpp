// subg_table_plan_check.cpp -- stand-alone check of plan_subg_table and SubgTableLayout
// (csrc/dcor_plan.cpp, csrc/dcor_layout.h), built from this file and dcor_plan.cpp alone with a host
// compiler: no HIP, no device.  Every kept record of the planner must equal, as bytes over its
// SubgSegConst part, the record plan_subg_panel builds for the segment's reference call (X = column
// col_x, Y = column col_y, eta1 = eta[col_x], eta2 = eta[col_y]) once the place fields (first,
// out_row, m_slot, mean_off) are set alike; the slot list must be the segments' distinct m in order
// of first use; the clips must be the reference calls' l1 / l2 bits; the layout's regions must not
// overlap.  Harness: check.h.
#include "check.h"

static const double* const kD = (const double*)4096;   // never dereferenced

static dcor_subg_table_desc table_of(int64_t n, int64_t p, int64_t ld, const double* eta) {
  dcor_subg_table_desc t;
  std::memset(&t, 0, sizeof(t));
  t.n = n; t.p = p; t.ld = ld; t.D = kD; t.eta = eta; t.alpha = 0.05; t.nsim = 2000;
  return t;
}

static dcor_subg_pair_segment seg_of(int32_t a, int32_t b, double e1, double e2, int64_t reps, size_t i) {
  dcor_subg_pair_segment g;
  std::memset(&g, 0, sizeof(g));
  g.eps1 = e1; g.eps2 = e2;
  g.seed = 0x1234567800000000ull + 77 * i;
  g.rep_begin = i % 2 ? 0xffffffffLL - reps : (int64_t)(5 * i);
  g.reps = reps;
  g.out_row = (int64_t)(1000 * i + 3);
  g.col_x = a; g.col_y = b;
  return g;
}

// The record plan_subg_panel builds for g's reference call, alone in its call.
static SubgSegConst reference_record(const dcor_subg_table_desc& t, const dcor_subg_pair_segment& g,
                                     SubgConst* c0) {
  dcor_subg_panel_desc p;
  std::memset(&p, 0, sizeof(p));
  p.n = t.n;
  p.X = t.D + g.col_x;   // any aligned non-null addresses: never read
  p.Y = t.D + g.col_y;
  p.eta1 = t.eta[g.col_x]; p.eta2 = t.eta[g.col_y]; p.alpha = t.alpha; p.nsim = t.nsim;
  dcor_subg_segment s;
  std::memset(&s, 0, sizeof(s));
  s.eps1 = g.eps1; s.eps2 = g.eps2; s.seed = g.seed; s.rep_begin = g.rep_begin; s.reps = g.reps;
  s.out_row = g.out_row;
  SubgPanelPlan pl;
  CHECK(plan_subg_panel(&p, &s, 1, pl) == DCOR_OK);
  CHECK(pl.tab.size() == 1 && pl.slots.size() == 1 && pl.items == g.reps);
  *c0 = pl.c0;
  return pl.tab[0];
}

// Pairs, (a, a), (b, a), a zero-rep segment, per-column eta; m = 8 shared by two segments on
// different columns, m = 11 with either sender.
static void check_list(int64_t n, const std::vector<int64_t>& want_m) {
  const std::vector<double> eta_v = {1.0, 0.5, 0.8, 1.3};
  const auto eta = heap(eta_v);
  const int64_t p = 4;
  const dcor_subg_table_desc t = table_of(n, p, n + 1, eta.get());
  const int32_t col[8][2] = {{0, 1}, {1, 0}, {2, 2}, {3, 1}, {0, 3}, {1, 3}, {3, 0}, {2, 1}};
  const double e[8][2] = {{1, 1}, {2, .5}, {.2, .2}, {.5, 1.5}, {1.5, .5}, {3, 3}, {2, 2}, {1, 1}};
  const int64_t reps[8] = {3, 2, 1, 4, 5, 0, 2, 2};
  std::vector<dcor_subg_pair_segment> segs;
  for (size_t i = 0; i < 8; ++i) segs.push_back(seg_of(col[i][0], col[i][1], e[i][0], e[i][1], reps[i], i));
  const auto hs = heap(segs);
  SubgTablePlan pl;
  pl.items = -1;
  CHECK(plan_subg_table(&t, hs.get(), 8, pl) == DCOR_OK);
  const std::vector<SubgPairSegConst>& tab = pl.tab;
  const std::vector<SubgMeanSlot>& slots = pl.slots;
  const std::vector<double>& clips = pl.clips;
  const SubgConst& c0 = pl.c0;
  const int64_t items = pl.items;
  CHECK(tab.size() == 7 && items == 19);
  CHECK(slots.size() == want_m.size());
  int64_t off = 0;
  for (size_t d = 0; d < slots.size(); ++d) {   // order of first use; off: the k before
    CHECK(slots[d].m == want_m[d] && slots[d].k == n / want_m[d] && slots[d].off == off);
    CHECK(slots[d].md == (double)want_m[d]);
    off += slots[d].k;
  }
  int64_t first = 0;
  size_t r = 0;
  for (size_t i = 0; i < 8; ++i) {
    if (reps[i] == 0) continue;
    SubgConst a;
    SubgSegConst want = reference_record(t, segs[i], &a);
    size_t d = 0;
    while (d < slots.size() && slots[d].m != want.m) ++d;
    CHECK(d < slots.size());
    want.first = first; want.out_row = segs[i].out_row; want.m_slot = (int32_t)d; want.mean_off = slots[d].off;
    const SubgSegConst& got = tab[r];   // the SubgSegConst part of the pair record
    CHECK(std::memcmp(&got, &want, sizeof(SubgSegConst)) == 0);
    CHECK(tab[r].col_x == col[i][0] && tab[r].col_y == col[i][1]);
    CHECK(slots[d].md_pow2 == a.md_pow2 && slots[d].inv_md == a.inv_md);
    // the prepared clips are the reference call's l1 / l2, bit for bit
    CHECK(std::memcmp(&clips[(size_t)col[i][0]], &a.l1, sizeof(double)) == 0);
    CHECK(std::memcmp(&clips[(size_t)col[i][1]], &a.l2, sizeof(double)) == 0);
    // the call-wide constants are the reference call's, and nothing else is set
    SubgConst w;
    std::memset(&w, 0, sizeof(w));
    w.n = a.n; w.nd = a.nd; w.sqrt_n = a.sqrt_n; w.crit = a.crit; w.mix = a.mix;
    CHECK(std::memcmp(&c0, &w, sizeof(SubgConst)) == 0);
    first += reps[i];
    ++r;
  }
  CHECK(clips.size() == (size_t)p);
  // (0,1) at (1,1) and (1,0) at (2,.5) share m = 8's slot on different columns; (3,1) at (.5,1.5)
  // and (0,3) at (1.5,.5) share m = 11 (or n) and differ in sender; eta follows the pair
  CHECK(tab[0].m_slot == tab[1].m_slot && tab[0].mean_off == tab[1].mean_off);
  CHECK(tab[3].m_slot == tab[4].m_slot && tab[3].sender_is_X == 0 && tab[4].sender_is_X == 1);
  CHECK(tab[0].m_slot == tab[6].m_slot);
  CHECK(tab[0].ls != tab[1].ls);   // the sender's eta: column 0's 1.0 against column 1's 0.5
  // the layout: regions in order, disjoint, aligned as stated
  const int64_t nmeans = off;
  const SubgTableLayout lay((int64_t)tab.size(), (int64_t)slots.size(), nmeans, n, p);
  CHECK(pl.lay.ok && pl.lay.cols_off == lay.cols_off && pl.lay.bytes == lay.bytes);   // the plan's own scratch
  CHECK(lay.ok && lay.npad % 4 == 0 && lay.npad >= n && lay.npad < n + 4);
  CHECK(lay.mpitch % 2 == 0 && lay.mpitch >= nmeans && lay.mpitch < nmeans + 2);
  CHECK(lay.tab_off == 0);
  CHECK(lay.slot_off >= lay.tab_off + tab.size() * sizeof(SubgPairSegConst));
  CHECK(lay.clip_off >= lay.slot_off + slots.size() * sizeof(SubgMeanSlot));
  CHECK(lay.means_off >= lay.clip_off + (size_t)p * sizeof(double));
  CHECK(lay.cols_off >= lay.means_off + (size_t)p * (size_t)lay.mpitch * sizeof(double));
  CHECK(lay.bytes == lay.cols_off + (size_t)p * (size_t)lay.npad * sizeof(double));
  const size_t offs[5] = {lay.tab_off, lay.slot_off, lay.clip_off, lay.means_off, lay.cols_off};
  for (size_t o : offs) CHECK(o % 256 == 0);
  CHECK((size_t)lay.mpitch * sizeof(double) % 16 == 0 && (size_t)lay.npad * sizeof(double) % 32 == 0);
  char* const base = (char*)65536;
  CHECK((char*)lay.tab(base) == base && (char*)lay.slots(base) == base + lay.slot_off);
  CHECK((char*)lay.clips(base) == base + lay.clip_off && (char*)lay.means(base) == base + lay.means_off);
  CHECK((char*)lay.cols(base) == base + lay.cols_off);
}

static void check_layout_overflow() {
  const int64_t big = 0x7fffffffLL;
  CHECK(!SubgTableLayout(0, 0, 0, big, big).ok);          // p * npad * 8 = 2^65
  CHECK(!SubgTableLayout(1, 1, 1, big, (int64_t)1 << 29).ok);
  CHECK(SubgTableLayout(1, 1, 1, big, 1 << 20).ok);       // 2^54 bytes: representable
  CHECK(!SubgTableLayout(1, 1, (int64_t)1 << 40, 1000, big).ok);   // p * mpitch * 8 = 2^74
  CHECK(!SubgTableLayout(1, 1, (int64_t)1 << 61, 1000, 4).ok);
  CHECK(!SubgTableLayout(-1, 1, 1, 1000, 4).ok && !SubgTableLayout(1, 1, 1, 0, 4).ok);
  CHECK(!SubgTableLayout(1, 1, 1, 1000, 0).ok);
  CHECK(SubgTableLayout(0, 0, 0, 1, 1).ok);
  // the planner refuses it before eta (one entry here) is read
  const std::vector<double> one = {1.0};
  const auto eta = heap(one);
  const dcor_subg_table_desc t = table_of(big, big, big, eta.get());
  const dcor_subg_pair_segment g = seg_of(0, 0, 1, 1, 1, 0);
  SubgTablePlan pl;
  CHECK_FAILS(plan_subg_table(&t, &g, 1, pl), DCOR_EINVAL, "scratch bytes overflow");
}

static void check_rejections() {
  SubgTablePlan pl;
  const std::vector<SubgPairSegConst>& tab = pl.tab;
  const std::vector<SubgMeanSlot>& slots = pl.slots;
  const std::vector<double>& clips = pl.clips;
  const std::vector<double> good_v = {1.0, 0.5, 0.8};
  const auto good = heap(good_v);
  const dcor_subg_pair_segment g = seg_of(0, 1, 1.0, 1.0, 1, 0);
  auto plan = [&](const dcor_subg_table_desc& t, const dcor_subg_pair_segment& s) {
    return plan_subg_table(&t, &s, 1, pl);
  };
  auto T = [&](const double* eta = nullptr) { return table_of(100, 3, 100, eta ? eta : good.get()); };
  dcor_subg_table_desc t = T();
  CHECK(plan(t, g) == DCOR_OK && tab.size() == 1 && clips.size() == 3);
  t.D = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = T(); t.eta = nullptr;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "null argument");
  t = T(); t.D = (const double*)4100;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "aligned to 8 bytes");
  t = T(); t.n = 0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "n must be in [1, 2^31)");
  t = T(); t.n = t.ld = 0x80000000LL;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "n must be in [1, 2^31)");
  t = T(); t.p = 0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "p must be in [1, 2^31)");
  t = T(); t.p = 0x80000000LL;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "p must be in [1, 2^31)");
  t = T(); t.ld = 99;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "ld = 99 < n = 100");
  const double bad[4] = {0.0, -1.0, INFINITY, NAN};
  for (double b : bad) {
    const std::vector<double> ev = {1.0, 0.5, b};
    const auto e = heap(ev);
    CHECK_FAILS(plan(T(e.get()), g), DCOR_EINVAL, "column 2: eta must be finite and > 0");
  }
  t = T(); t.alpha = 2.0;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "alpha must be < 2");
  t = T(); t.nsim = 2049;
  CHECK_FAILS(plan(t, g), DCOR_EINVAL, "nsim must be in [1, 2048]");
  t = T();
  dcor_subg_pair_segment h = g;
  for (double b : bad) {
    h = g; h.eps1 = b;
    CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need finite eps1, eps2 > 0");
    h = g; h.eps2 = b;
    CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: need finite eps1, eps2 > 0");
  }
  h = g; h.out_row = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0:");
  h = g; h.col_y = 3;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (0, 3) outside [0, 3)");
  h = g; h.col_x = -1;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: columns (-1, 1)");
  h = g; h.rep_begin = 0xffffffffLL - 5; h.reps = 7;   // rep_begin + reps = 2^32 + 1
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "segment 0: replicate range exceeds 2^32");
  h = g; h.rep_begin = 0xfffffffeLL; h.reps = 1;
  CHECK(plan(t, h) == DCOR_OK);
  // the order: D and eta, D's alignment, n, p, ld, eta[c], alpha, nsim, then the segments (fields,
  // columns, range)
  const std::vector<double> ev = {1.0, 0.0, 1.0};
  const auto e = heap(ev);
  h = g; h.eps1 = 0.0; h.col_x = 7; h.rep_begin = 0xffffffffLL; h.reps = 5;
  t = T();
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "need finite eps1, eps2 > 0");
  h.eps1 = 1.0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "columns (7, 1)");
  h.col_x = 0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "replicate range");
  h.eps1 = 0.0;
  t.nsim = 0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "nsim must be in [1, 2048]");
  t.alpha = 3.0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "alpha must be < 2");
  t.eta = e.get();
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "column 1: eta");
  t.ld = 50;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "ld = 50");
  t.p = 0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "p must be");
  t.n = 0;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "n must be");
  t.D = (const double*)4100;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "aligned");
  t.eta = nullptr;
  CHECK_FAILS(plan(t, h), DCOR_EINVAL, "null argument");
  // a bad last segment among good ones is named; the cap on a call's replicates; a call without
  // replicates keeps nothing
  {
    std::vector<dcor_subg_pair_segment> v = {g, g, g};
    v[2].col_y = 3;
    const auto hv = heap(v);
    t = T();
    CHECK_FAILS(plan_subg_table(&t, hv.get(), 3, pl), DCOR_EINVAL, "segment 2: columns");
    v[2].col_y = 1; v[2].reps = 0x40000000LL; v[1].reps = 0x40000000LL;
    const auto hw = heap(v);
    CHECK_FAILS(plan_subg_table(&t, hw.get(), 3, pl), DCOR_EINVAL, "2^31 - 1");
    v[0].reps = v[1].reps = v[2].reps = 0;
    const auto hz = heap(v);
    CHECK(plan_subg_table(&t, hz.get(), 3, pl) == DCOR_OK);
    CHECK(tab.empty() && slots.empty() && clips.empty() && pl.items == 0);
  }
}

int main() {
  // m = 8, 200, 11, 2 at n >= 200 in order of first use; at n = 5 the m > n guard makes every m but
  // 2 equal to 5
  check_list(1001, {8, 200, 11, 2});
  check_list(401, {8, 200, 11, 2});
  check_list(70001, {8, 200, 11, 2});
  check_list(5, {5, 2});
  check_list(12, {8, 12, 11, 2});
  check_layout_overflow();
  check_rejections();
  std::printf("subg_table_plan_check: ok\n");
  return 0;
}
