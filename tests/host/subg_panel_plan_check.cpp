// subg_panel_plan_check.cpp -- stand-alone check of plan_subg_panel (csrc/dcor_plan.cpp), built
// from this file and dcor_plan.cpp alone with a host compiler: no HIP, no device.  Every record of
// the planner must equal, as bytes, the fields make_subg yields for the segment's (n, eta1, eta2,
// eps1, eps2) with hrs = 0 and no override, and the list of distinct batch sizes must be the
// segments'.  Harness: check.h.
#include "check.h"

static const double* const kX = (const double*)4096;   // never dereferenced
static const double* const kY = (const double*)8192;

static dcor_subg_panel_desc panel_of(int64_t n, double eta1, double eta2) {
  dcor_subg_panel_desc p;
  std::memset(&p, 0, sizeof(p));
  p.n = n; p.X = kX; p.Y = kY; p.eta1 = eta1; p.eta2 = eta2; p.alpha = 0.05; p.nsim = 2000;
  return p;
}

static dcor_subg_segment seg_of(double e1, double e2, int64_t reps, size_t i) {
  dcor_subg_segment g;
  std::memset(&g, 0, sizeof(g));
  g.eps1 = e1; g.eps2 = e2;
  g.seed = 0x1234567800000000ull + 77 * i;
  g.rep_begin = i % 2 ? 0xffffffffLL - reps : (int64_t)(5 * i);
  g.reps = reps;
  g.out_row = (int64_t)(1000 * i + 3);
  return g;
}

// The record make_subg's constants give for segment g at its place in the call.
static SubgSegConst reference_record(const dcor_subg_panel_desc& p, const dcor_subg_segment& g,
                                     int64_t first, int32_t slot, int64_t mean_off, SubgConst* full) {
  SubgConst a;
  CHECK(make_subg(p.n, g.eps1, g.eps2, p.eta1, p.eta2, p.alpha, 0, NAN, NAN, NAN, NAN, NAN, NAN, p.nsim,
                  a, nullptr, nullptr) == DCOR_OK);
  SubgSegConst t;
  std::memset(&t, 0, sizeof(t));
  t.k = a.k; t.m = a.m; t.md_pow2 = a.md_pow2; t.sender_is_X = a.sender_is_X; t.m_slot = slot;
  t.md = a.md; t.kd = a.kd; t.inv_md = a.inv_md;
  t.bx = a.bx; t.by = a.by; t.m_over_k = a.m_over_k; t.sqrt_k = a.sqrt_k;
  t.ls = a.ls; t.lr = a.lr; t.bs = a.bs; t.s_central = a.s_central; t.sn2x2 = a.sn2x2; t.eps_r = a.eps_r;
  t.k0 = (uint32_t)g.seed; t.k1 = (uint32_t)(g.seed >> 32);
  t.rep_begin = (uint32_t)g.rep_begin;
  t.mean_off = mean_off; t.first = first; t.out_row = g.out_row;
  if (full) *full = a;
  return t;
}

// The issue's list: (1,1), (2,2), (.2,.2), (1.5,.5), (.5,1.5), (1,1) again, one with reps == 0.
static void check_list(int64_t n, double eta1, double eta2, const std::vector<int64_t>& want_m) {
  const dcor_subg_panel_desc p = panel_of(n, eta1, eta2);
  const double e[7][2] = {{1, 1}, {2, 2}, {.2, .2}, {1.5, .5}, {.5, 1.5}, {1, 1}, {3, 3}};
  const int64_t reps[7] = {3, 2, 1, 4, 5, 2, 0};
  std::vector<dcor_subg_segment> segs;
  for (size_t i = 0; i < 7; ++i) segs.push_back(seg_of(e[i][0], e[i][1], reps[i], i));
  const auto hs = heap(segs);
  SubgPanelPlan pl;
  pl.items = -1;
  CHECK(plan_subg_panel(&p, hs.get(), 7, pl) == DCOR_OK);
  const std::vector<SubgSegConst>& tab = pl.tab;
  const std::vector<SubgMeanSlot>& slots = pl.slots;
  const SubgConst& c0 = pl.c0;
  const int64_t items = pl.items;
  CHECK(tab.size() == 6 && items == 17);
  CHECK(slots.size() == want_m.size());
  int64_t off = 0;
  for (size_t d = 0; d < slots.size(); ++d) {   // order of first use; off: the k before
    CHECK(slots[d].m == want_m[d] && slots[d].k == n / want_m[d] && slots[d].off == off);
    CHECK(slots[d].md == (double)want_m[d]);
    off += slots[d].k;
  }
  int64_t first = 0;
  for (size_t i = 0; i < 6; ++i) {
    SubgConst a;
    const SubgSegConst probe = reference_record(p, segs[i], 0, 0, 0, &a);
    size_t d = 0;
    while (d < slots.size() && slots[d].m != probe.m) ++d;
    CHECK(d < slots.size());
    const SubgSegConst want = reference_record(p, segs[i], first, (int32_t)d, slots[d].off, nullptr);
    CHECK(std::memcmp(&tab[i], &want, sizeof(SubgSegConst)) == 0);
    CHECK(slots[d].md_pow2 == a.md_pow2 && slots[d].inv_md == a.inv_md);
    CHECK(tab[i].sender_is_X == (segs[i].eps1 >= segs[i].eps2 ? 1 : 0));
    first += reps[i];
  }
  // segments 0 and 5 share (1, 1)'s slot; (1.5, .5) and (.5, 1.5) share m = 11 and differ in sender
  CHECK(tab[0].m_slot == tab[5].m_slot && tab[0].mean_off == tab[5].mean_off);
  CHECK(tab[3].m_slot == tab[4].m_slot && tab[3].sender_is_X == 1 && tab[4].sender_is_X == 0);
  // the call-wide constants are the first kept segment's
  SubgConst a0;
  reference_record(p, segs[0], 0, 0, 0, &a0);
  CHECK(std::memcmp(&c0, &a0, sizeof(SubgConst)) == 0);
  CHECK(c0.l1 == dcor_lambda_n((double)n, eta1) && c0.l2 == dcor_lambda_n((double)n, eta2));
  CHECK(pl.lay.ok && pl.lay.bytes == SubgPanelLayout((int64_t)tab.size(), (int64_t)slots.size(), off, n).bytes);
}

static void check_rejections() {
  SubgPanelPlan pl;
  const dcor_subg_segment g = seg_of(1.0, 1.0, 1, 0);
  auto plan = [&](const dcor_subg_panel_desc& p, const dcor_subg_segment& s) {
    return plan_subg_panel(&p, &s, 1, pl);
  };
  dcor_subg_panel_desc p = panel_of(100, 1, 1);
  p.X = nullptr;
  CHECK_FAILS(plan(p, g), DCOR_EINVAL, "null argument");
  p = panel_of(100, 1, 1); p.Y = (const double*)4100;
  CHECK_FAILS(plan(p, g), DCOR_EINVAL, "aligned to 8 bytes");
  CHECK_FAILS(plan(panel_of(0, 1, 1), g), DCOR_EINVAL, "n must be in [1, 2^31)");
  CHECK_FAILS(plan(panel_of(0x80000000LL, 1, 1), g), DCOR_EINVAL, "n must be in [1, 2^31)");
  CHECK(plan(panel_of(0x7fffffffLL, 1, 1), g) == DCOR_OK);
  const double bad[4] = {0.0, -1.0, INFINITY, NAN};
  for (double b : bad) {
    CHECK_FAILS(plan(panel_of(100, b, 1), g), DCOR_EINVAL, "eta1, eta2 must be finite and > 0");
    CHECK_FAILS(plan(panel_of(100, 1, b), g), DCOR_EINVAL, "eta1, eta2 must be finite and > 0");
  }
  p = panel_of(100, 1, 1); p.alpha = 2.0;
  CHECK_FAILS(plan(p, g), DCOR_EINVAL, "alpha must be < 2");
  p = panel_of(100, 1, 1); p.nsim = 2049;
  CHECK_FAILS(plan(p, g), DCOR_EINVAL, "nsim must be in [1, 2048]");
  p = panel_of(100, 1, 1);
  dcor_subg_segment h = g;
  for (double b : bad) {
    h = g; h.eps1 = b;
    CHECK_FAILS(plan(p, h), DCOR_EINVAL, "segment 0: need finite eps1, eps2 > 0");
    h = g; h.eps2 = b;
    CHECK_FAILS(plan(p, h), DCOR_EINVAL, "segment 0: need finite eps1, eps2 > 0");
  }
  h = g; h.out_row = -1;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "segment 0:");
  h = g; h.rep_begin = 0xffffffffLL; h.reps = 1;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "segment 0: replicate range exceeds 2^32");
  h = g; h.rep_begin = 0xfffffffeLL; h.reps = 1;
  CHECK(plan(p, h) == DCOR_OK);
  // the order: X and Y, n, eta, alpha, nsim, then the segments
  h = g; h.eps1 = 0.0;
  p = panel_of(100, 1, 1); p.nsim = 0;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "nsim must be in [1, 2048]");
  p.alpha = 3.0;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "alpha must be < 2");
  p.eta2 = 0.0;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "eta1, eta2");
  p.n = 0;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "n must be in [1, 2^31)");
  p.X = nullptr;
  CHECK_FAILS(plan(p, h), DCOR_EINVAL, "null argument");
  // a bad last segment among good ones is named; the cap on a call's replicates
  {
    std::vector<dcor_subg_segment> v = {g, g, g};
    v[2].reps = -1;
    const auto hv = heap(v);
    p = panel_of(100, 1, 1);
    CHECK_FAILS(plan_subg_panel(&p, hv.get(), 3, pl), DCOR_EINVAL, "segment 2:");
    v[2].reps = 0x40000000LL; v[1].reps = 0x40000000LL;
    const auto hw = heap(v);
    CHECK_FAILS(plan_subg_panel(&p, hw.get(), 3, pl), DCOR_EINVAL, "2^31 - 1");
  }
}

int main() {
  // m = 8, 2, 200, 11 at n >= 200; at n = 5 the m > n guard makes every m but 2 equal to 5
  check_list(1001, 1.0, 1.0, {8, 2, 200, 11});
  check_list(401, 0.5, 0.8, {8, 2, 200, 11});
  check_list(70001, 1.0, 1.0, {8, 2, 200, 11});
  check_list(5, 1.0, 1.0, {5, 2});
  check_list(12, 1.0, 1.0, {8, 2, 12, 11});
  check_rejections();
  std::printf("subg_panel_plan_check: ok\n");
  return 0;
}
