// layout_check.cpp -- stand-alone check of the ten scratch layouts (csrc/dcor_layout.h), built from
// this file and dcor_plan.cpp alone with a host compiler: no HIP, no device.  Each layout's offset
// formulas are written out here in plain form, as the sums of al256 terms they were before the
// layouts shared a carver, in 128-bit arithmetic so that nothing wraps; over a grid of arguments every
// field, pitch, accessor and the total must equal them, and ok must be true exactly when every
// argument is in its domain (n >= 1, p >= 1, no negative count; the grid has 0 and -1 of each) and
// the total is at most SIZE_MAX / 2.  Exit status 0: every check held.
#include "check.h"

typedef unsigned __int128 u128;
static const u128 kLim = SIZE_MAX / 2;
static u128 al256w(u128 b) { return (b + 255) & ~(u128)255; }
static u128 w(int64_t v) { return (u128)(v < 0 ? 0 : v); }

static const int64_t kBig = 0x7fffffffLL;
static const int64_t kN[] = {-1, 0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 65535, 65536, kBig};
static const int64_t kP[] = {-1, 0, 1, 2, 8, 1 << 20};
static const int64_t kCount[] = {-1, 0, 1, 7, kBig};
static const int64_t kMeans[] = {-1, 0, 1, 2, 501};
static const bool kBool[] = {false, true};

static char* const kBase = (char*)65536;
static long g_cases = 0;

// ok is as wanted; where it is true, every offset named is the plain formula's
#define FIELDS(lay, want_ok, total, ...)                                            \
  do {                                                                              \
    ++g_cases;                                                                      \
    const bool ok_ = (want_ok) && (total) <= kLim;                                  \
    CHECK((lay).ok == ok_);                                                         \
    if (ok_) {                                                                      \
      const u128 want_[] = {__VA_ARGS__, (total)};                                  \
      const size_t got_[] = {LAYOUT_FIELDS, (lay).bytes};                           \
      static_assert(sizeof(want_) / sizeof(want_[0]) == sizeof(got_) / sizeof(got_[0]), "one formula per field"); \
      for (size_t i_ = 0; i_ < sizeof(got_) / sizeof(got_[0]); ++i_) CHECK((u128)got_[i_] == want_[i_]); \
    }                                                                               \
  } while (0)

static void check_coded(int64_t n) {
  const CodedPanelLayout lay(n);
  const u128 dict_off = al256w(w(n) * 2), ok_off = dict_off + 2 * 256 * sizeof(double), bytes = ok_off + 256;
#define LAYOUT_FIELDS lay.dict_off, lay.ok_off
  FIELDS(lay, n >= 1, bytes, dict_off, ok_off);
#undef LAYOUT_FIELDS
  if (!lay.ok) return;
  CHECK((char*)lay.codes(kBase) == kBase && (char*)lay.dict(kBase) == kBase + lay.dict_off);
  CHECK((char*)lay.ok_flag(kBase) == kBase + lay.ok_off);
}

static void check_premat(int64_t reps, int64_t slices, int64_t n, bool pack, bool dict) {
  const PrematScratchLayout lay(reps, slices, n, pack, dict);
  const u128 pack_off = al256w(w(reps) * sizeof(SubgPartial) * w(slices));
  const u128 coded_off = pack_off + (pack ? w(n) * 2 * sizeof(double2) : 0);
  const u128 coded_bytes = dict ? al256w(w(n) * 2) + 2 * 256 * sizeof(double) + 256 : 0;
#define LAYOUT_FIELDS lay.pack_off, lay.coded_off, lay.coded.bytes
  FIELDS(lay, n >= 1 && reps >= 0 && slices >= 0, coded_off + coded_bytes, pack_off, coded_off, coded_bytes);
#undef LAYOUT_FIELDS
  if (!lay.ok) return;
  CHECK(lay.n == n && lay.coded.ok == dict);
  CHECK((char*)lay.partials(kBase) == kBase && (char*)lay.partials(kBase, 3) == kBase + 3 * sizeof(SubgPartial));
  CHECK((char*)lay.xyc(kBase) == kBase + lay.pack_off);
  CHECK((char*)lay.soc(kBase) == kBase + lay.pack_off + (size_t)n * sizeof(double2));
  CHECK((char*)lay.coded_base(kBase) == kBase + lay.coded_off);
  if (dict) CHECK(lay.coded.dict_off == CodedPanelLayout(n).dict_off && lay.coded.ok_off == CodedPanelLayout(n).ok_off);
}

static void check_noise(int64_t n, int64_t k, int64_t m, int64_t nsim, int64_t cr) {
  const HrsNoiseLayout lay(n, k, m, nsim, cr);
  const u128 b[7] = {w(cr) * w(k) * w(m) * 4, w(cr) * w(k) * 8, w(cr) * w(k) * 8, w(cr) * w(n) * 8,
                     w(cr) * 8,               w(cr) * w(nsim) * 8, w(cr) * w(nsim) * 8};
  u128 off[7], bytes = 0;
  for (int i = 0; i < 7; ++i) { off[i] = bytes; bytes += al256w(b[i]); }
#define LAYOUT_FIELDS lay.off[0], lay.off[1], lay.off[2], lay.off[3], lay.off[4], lay.off[5], lay.off[6]
  FIELDS(lay, n >= 1 && k >= 0 && m >= 0 && nsim >= 0 && cr >= 0, bytes, off[0], off[1], off[2], off[3], off[4],
         off[5], off[6]);
#undef LAYOUT_FIELDS
  if (!lay.ok) return;
  CHECK(lay.bytes % 256 == 0);   // the last array is rounded up too: chunks are sized by this
  HrsNoise j{};
  lay.point(kBase, j);
  CHECK((char*)j.perm == kBase + lay.off[0] && (char*)j.lap_x == kBase + lay.off[1]);
  CHECK((char*)j.lap_y == kBase + lay.off[2] && (char*)j.lap_local == kBase + lay.off[3]);
  CHECK((char*)j.lap_central == kBase + lay.off[4] && (char*)j.mix_z == kBase + lay.off[5]);
  CHECK((char*)j.mix_l == kBase + lay.off[6]);
}

static void check_fused_sweep(int64_t items, int64_t nseg, int64_t n, bool pack) {
  const FusedSweepLayout lay(items, nseg, n, pack);
  const u128 tab_off = al256w(w(items) * sizeof(SubgPartial));
  const u128 pack_off = tab_off + al256w(w(nseg) * sizeof(HrsSegConst));
  const u128 bytes = pack_off + (pack ? w(n) * 2 * sizeof(double2) : 0);
#define LAYOUT_FIELDS lay.tab_off, lay.pack_off
  FIELDS(lay, n >= 1 && items >= 0 && nseg >= 0, bytes, tab_off, pack_off);
#undef LAYOUT_FIELDS
  if (!lay.ok) return;
  CHECK(lay.n == n && (char*)lay.tab(kBase) == kBase + lay.tab_off && (char*)lay.xyc(kBase) == kBase + lay.pack_off);
  CHECK((char*)lay.soc(kBase) == kBase + lay.pack_off + (size_t)n * sizeof(double2));
}

static void check_hrs_table(int64_t items, int64_t nseg, int64_t n, int64_t p) {
  const HrsTableLayout lay(items, nseg, n, p);
  const int64_t npad = (n + 3) & ~(int64_t)3;
  const u128 tab_off = al256w(w(items) * sizeof(SubgPartial));
  const u128 lam_off = tab_off + al256w(w(nseg) * sizeof(HrsPairSegConst));
  const u128 cols_off = lam_off + al256w(w(p) * sizeof(double));
  const u128 bytes = cols_off + w(p) * (w(npad) * sizeof(double));
#define LAYOUT_FIELDS lay.tab_off, lay.lam_off, lay.cols_off
  FIELDS(lay, n >= 1 && p >= 1 && items >= 0 && nseg >= 0, bytes, tab_off, lam_off, cols_off);
#undef LAYOUT_FIELDS
  CHECK(lay.npad == npad);
  if (!lay.ok) return;
  CHECK((char*)lay.tab(kBase) == kBase + lay.tab_off && (char*)lay.lam(kBase) == kBase + lay.lam_off);
  CHECK((char*)lay.cols(kBase) == kBase + lay.cols_off);
  if (items == 0 && nseg == 0) CHECK(HrsTableLayout::columns(n, p).ok && HrsTableLayout::columns(n, p).bytes == lay.bytes);
}

static void check_hrs_pair_table(int64_t items, int64_t nseg, int64_t nslot, int64_t n, int64_t p, int64_t elems) {
  const HrsPairTableLayout lay(items, nseg, nslot, n, p, elems);
  const int64_t nw = (n + 63) >> 6;
  const u128 tab_off = al256w(w(items) * sizeof(SubgPartial));
  const u128 slot_off = tab_off + al256w(w(nseg) * sizeof(HrsPairNaSegConst));
  const u128 lam_off = slot_off + al256w(w(nslot) * sizeof(HrsPairSlot));
  const u128 mask_off = lam_off + al256w(w(p) * sizeof(double));
  const u128 panel_off = mask_off + al256w(w(p) * (w(nw) * sizeof(uint64_t)));
  const u128 bytes = panel_off + w(elems) * sizeof(double2);
#define LAYOUT_FIELDS lay.tab_off, lay.slot_off, lay.lam_off, lay.mask_off, lay.panel_off
  FIELDS(lay, n >= 1 && p >= 1 && items >= 0 && nseg >= 0 && nslot >= 0 && elems >= 0, bytes, tab_off, slot_off,
         lam_off, mask_off, panel_off);
#undef LAYOUT_FIELDS
  CHECK(lay.nw == nw);
  if (!lay.ok) return;
  CHECK((char*)lay.tab(kBase) == kBase + lay.tab_off && (char*)lay.slots(kBase) == kBase + lay.slot_off);
  CHECK((char*)lay.lam(kBase) == kBase + lay.lam_off && (char*)lay.masks(kBase) == kBase + lay.mask_off);
  CHECK((char*)lay.panels(kBase) == kBase + lay.panel_off);
}

static void check_subg_panel(int64_t nseg, int64_t nslots, int64_t nmeans, int64_t n) {
  const SubgPanelLayout lay(nseg, nslots, nmeans, n);
  const int64_t npad = (n + 3) & ~(int64_t)3;
  const u128 slot_off = al256w(w(nseg) * sizeof(SubgSegConst));
  const u128 means_off = slot_off + al256w(w(nslots) * sizeof(SubgMeanSlot));
  const u128 pack_off = means_off + al256w(w(nmeans) * sizeof(double2));
  const u128 bytes = pack_off + w(npad) * sizeof(double2);
#define LAYOUT_FIELDS lay.tab_off, lay.slot_off, lay.means_off, lay.pack_off
  FIELDS(lay, n >= 1 && nseg >= 0 && nslots >= 0 && nmeans >= 0, bytes, 0, slot_off, means_off, pack_off);
#undef LAYOUT_FIELDS
  CHECK(lay.npad == npad);
  if (!lay.ok) return;
  CHECK((char*)lay.tab(kBase) == kBase && (char*)lay.slots(kBase) == kBase + lay.slot_off);
  CHECK((char*)lay.means(kBase) == kBase + lay.means_off && (char*)lay.xy(kBase) == kBase + lay.pack_off);
}

static void check_subg_table(int64_t nseg, int64_t nslots, int64_t nmeans, int64_t n, int64_t p) {
  const SubgTableLayout lay(nseg, nslots, nmeans, n, p);
  const int64_t npad = (n + 3) & ~(int64_t)3, mpitch = (nmeans + 1) & ~(int64_t)1;
  const u128 slot_off = al256w(w(nseg) * sizeof(SubgPairSegConst));
  const u128 clip_off = slot_off + al256w(w(nslots) * sizeof(SubgMeanSlot));
  const u128 means_off = clip_off + al256w(w(p) * sizeof(double));
  const u128 cols_off = means_off + al256w(w(p) * (w(mpitch) * sizeof(double)));
  const u128 bytes = cols_off + w(p) * (w(npad) * sizeof(double));
#define LAYOUT_FIELDS lay.tab_off, lay.slot_off, lay.clip_off, lay.means_off, lay.cols_off
  FIELDS(lay, n >= 1 && p >= 1 && nseg >= 0 && nslots >= 0 && nmeans >= 0, bytes, 0, slot_off, clip_off, means_off,
         cols_off);
#undef LAYOUT_FIELDS
  CHECK(lay.npad == npad && lay.mpitch == mpitch);
  if (!lay.ok) return;
  CHECK((char*)lay.tab(kBase) == kBase && (char*)lay.slots(kBase) == kBase + lay.slot_off);
  CHECK((char*)lay.clips(kBase) == kBase + lay.clip_off && (char*)lay.means(kBase) == kBase + lay.means_off);
  CHECK((char*)lay.cols(kBase) == kBase + lay.cols_off);
}

static void check_sign_panel(int64_t nseg, int64_t n) {
  const SignPanelLayout lay(nseg, n);
  const int64_t npad = (n + 3) & ~(int64_t)3;
  const u128 tab_off = 256;
  const u128 pack_off = tab_off + al256w(w(nseg) * sizeof(SignSegConst));
  const u128 bytes = pack_off + w(npad) * 2 * sizeof(double);
#define LAYOUT_FIELDS lay.tab_off, lay.pack_off
  FIELDS(lay, n >= 1 && nseg >= 0, bytes, tab_off, pack_off);
#undef LAYOUT_FIELDS
  CHECK(lay.npad == npad);
  if (!lay.ok) return;
  CHECK((char*)lay.means(kBase) == kBase && (char*)lay.tab(kBase) == kBase + lay.tab_off);
  CHECK((char*)lay.xyc(kBase) == kBase + lay.pack_off);
}

static void check_sign_table(int64_t nseg, int64_t n, int64_t p) {
  const SignTableLayout lay(nseg, n, p);
  const int64_t npad = (n + 3) & ~(int64_t)3;
  const u128 tab_off = al256w(w(p) * 2 * sizeof(double));
  const u128 cols_off = tab_off + al256w(w(nseg) * sizeof(SignPairSegConst));
  const u128 bytes = cols_off + w(p) * (w(npad) * sizeof(double));
#define LAYOUT_FIELDS lay.tab_off, lay.cols_off
  FIELDS(lay, n >= 1 && p >= 1 && nseg >= 0, bytes, tab_off, cols_off);
#undef LAYOUT_FIELDS
  CHECK(lay.npad == npad);
  if (!lay.ok) return;
  CHECK((char*)lay.means(kBase) == kBase && (char*)lay.tab(kBase) == kBase + lay.tab_off);
  CHECK((char*)lay.cols(kBase) == kBase + lay.cols_off);
}

static void check_grid() {
  for (int64_t n : kN) {
    check_coded(n);
    for (int64_t a : kCount) {
      check_sign_panel(a, n);
      for (int64_t p : kP) check_sign_table(a, n, p);
      for (int64_t b : kCount) {
        for (bool pack : kBool) {
          check_fused_sweep(a, b, n, pack);
          for (bool dict : kBool) check_premat(a, b, n, pack, dict);   // b slices per replicate
        }
        for (int64_t p : kP) check_hrs_table(a, b, n, p);
        for (int64_t nmeans : kMeans) {
          check_subg_panel(a, b, nmeans, n);
          for (int64_t p : kP) check_subg_table(a, b, nmeans, n, p);
        }
        for (int64_t c : kCount)
          for (int64_t p : kP)
            for (int64_t elems : kCount) check_hrs_pair_table(a, b, c, n, p, elems);
        // k = a, m = b; nsim and the chunk from the counts too
        for (int64_t nsim : kCount)
          for (int64_t cr : kCount) check_noise(n, a, b, nsim, cr);
      }
    }
  }
}

// Far outside the domain (the grid has 0 and -1 of every argument).
static void check_domain() {
  const int64_t lo = INT64_MIN;
  check_coded(lo);
  check_premat(lo, lo, lo, true, true);
  check_noise(lo, lo, lo, lo, lo);
  check_fused_sweep(lo, lo, lo, true);
  check_hrs_table(lo, lo, lo, lo);
  check_hrs_pair_table(lo, lo, lo, lo, lo, lo);
  check_subg_panel(lo, lo, lo, lo);
  check_subg_table(lo, lo, lo, lo, lo);
  check_subg_table(1, 1, lo, 8, 1);   // mpitch alone would hide a negative nmeans
  check_sign_panel(lo, lo);
  check_sign_table(lo, lo, lo);
}

// The totals around SIZE_MAX / 2 = 2^63 - 1, for layouts that had no guard and for one that had.
static void check_limit() {
  // coded panel: al256(2 n) + 4096 + 256, so 2 n = 2^63 - 4608 gives 2^63 - 256 and one sample more 2^63
  const int64_t n_fit = ((int64_t)1 << 62) - 2304;
  CHECK(CodedPanelLayout(n_fit).ok && CodedPanelLayout(n_fit).bytes == ((size_t)1 << 63) - 256);
  CHECK(!CodedPanelLayout(n_fit + 1).ok);
  check_coded(INT64_MAX);
  // sub-G panel: nmeans * 16 bytes of means before a 4-sample panel of 64 bytes
  const int64_t means_fit = ((int64_t)1 << 59) - 16;     // 2^63 - 256 bytes of means: the total is 2^63 - 192
  CHECK(SubgPanelLayout(0, 0, means_fit, 4).ok && SubgPanelLayout(0, 0, means_fit, 4).bytes == ((size_t)1 << 63) - 192);
  CHECK(!SubgPanelLayout(0, 0, means_fit + 1, 4).ok);    // the panel would start at 2^63
  check_subg_panel(0, 0, means_fit + 1, 4);
  check_subg_panel(INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX - 3);
  // sign panel: 256 + nseg records + the panel
  const int64_t seg_fit = (int64_t)((((size_t)1 << 63) - 256 - 256 - 64) / sizeof(SignSegConst));
  for (int64_t d = 0; d < 3; ++d) check_sign_panel(seg_fit + d, 4);
  CHECK(SignPanelLayout(seg_fit, 4).ok && !SignPanelLayout(seg_fit + 2, 4).ok);
  // fused sweep and premat partials: 80 bytes per replicate
  const int64_t items_fit = (int64_t)((((size_t)1 << 63) - 512) / sizeof(SubgPartial));
  for (int64_t d : {0, 4}) {
    check_fused_sweep(items_fit + d, 1, 4, true);
    check_premat(items_fit + d, 1, 4, true, d != 0);
  }
  check_premat(kBig, (int64_t)1 << 32, 4, false, false);   // 80 * 2^63: the product alone
  CHECK(FusedSweepLayout(items_fit, 1, 4, true).ok && !FusedSweepLayout(items_fit + 4, 1, 4, true).ok);
  // noise: a zero factor makes an array empty whatever the others are
  check_noise(8, INT64_MAX, INT64_MAX, 0, 0);
  check_noise(8, INT64_MAX, 0, INT64_MAX, 1);
  check_noise(8, kBig, kBig, 1, 2);     // 2^65 bytes of perm
  check_noise(8, kBig, kBig, 1, 1);     // 2^64 - 2^34 + 4: above the limit, below SIZE_MAX
  // a guarded layout, as its planner's check programs pin it: p * npad * 8 = 2^63 and one column less
  check_subg_table(1, 1, 1, kBig, (int64_t)1 << 29);
  check_subg_table(1, 1, 1, kBig, ((int64_t)1 << 29) - 1);
  check_hrs_table(1, 1, kBig, (int64_t)1 << 29);
  check_sign_table(1, kBig, (int64_t)1 << 29);
  check_hrs_pair_table(1, 1, 1, kBig, kBig, ((int64_t)1 << 59));   // the panels alone: 2^63 bytes
  CHECK(!SubgTableLayout(1, 1, 1, kBig, (int64_t)1 << 29).ok && SubgTableLayout(1, 1, 1, kBig, ((int64_t)1 << 29) - 1).ok);
}

// The carver itself: 256-B starts, an empty region moves the end to its start, and ok is sticky.
static void check_carver() {
  Carver c(true);
  CHECK(c.add(3, 7) == 0 && c.bytes == 21);
  CHECK(c.add(0, 8) == 256 && c.bytes == 256);
  CHECK(c.add(1, 1) == 256 && c.bytes == 257);
  CHECK(c.add(2, 16, 16) == 272 && c.bytes == 304 && c.ok);
  CHECK(c.add({3, 5}, 2) == 512 && c.bytes == 542 && c.ok);
  CHECK(c.add({0, INT64_MAX, INT64_MAX}, 8) == 768 && c.bytes == 768 && c.ok);
  Carver d = c;
  d.add(-1, 1);
  d.add(1, 1);
  CHECK(!d.ok && d.bytes <= 769);
  Carver e = c;
  e.add({INT64_MAX, 2}, 1);
  CHECK(!e.ok && e.bytes <= Carver::kLim);
  Carver f(true);
  CHECK(f.add((int64_t)(Carver::kLim), 1) == 0 && f.ok && f.bytes == Carver::kLim);
  f.add(0, 1);   // the rounded end is past the limit
  CHECK(!f.ok && f.bytes == Carver::kLim);
}

int main() {
  check_carver();
  check_grid();
  check_domain();
  check_limit();
  CHECK(g_cases > 70000);   // the grid ran
  std::printf("layout_check: ok\n");
  return 0;
}
