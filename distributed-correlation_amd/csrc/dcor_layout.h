// dcor_layout.h -- the host's scratch layouts, each the single definition of its buffer: offsets and
// the total from the geometry, pointers over a base address.  HIP-free (no kernel names a layout);
// read through dcor_plan.h, which supplies double2 where the HIP headers are absent.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "dcor_engine.h"

namespace dcor {

// Every scratch region on the panel / HRS path starts on a 256-B boundary.
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Consecutive regions of one buffer: the base of every layout and their only overflow arithmetic.
// ok: the arguments are in their domain (the constructor's test), no count is negative and no
// product or sum exceeds SIZE_MAX / 2; nothing wraps on the way, and the offsets of a layout that is
// not ok mean nothing.  The table planners refuse a call whose layout is not ok; the sign-panel,
// sub-G panel, fused-sweep, premat and noise layouts are built where n < 2^31 and at most 2^31 - 1
// replicates are already checked, which keeps them ok, and are not asked.  A layout constructed from
// no arguments is the layout of nothing (n = 0: not ok).
struct Carver {
  static constexpr size_t kLim = SIZE_MAX / 2;
  size_t bytes = 0;
  bool ok;
  explicit Carver(bool in_domain = false) : ok(in_domain) {}
  // count * elem_bytes (0 when it is not representable)
  size_t mul(int64_t count, size_t elem_bytes) {
    if (count < 0 || (elem_bytes && (size_t)count > kLim / elem_bytes)) { ok = false; return 0; }
    return (size_t)count * elem_bytes;
  }
  // The offset of a region of counts[0] x counts[1] x ... elements: the end rounded up to `align`, a
  // power of two (an empty region too: it moves the end to its own start).
  size_t add(std::initializer_list<int64_t> counts, size_t elem_bytes, size_t align = 256) {
    size_t size = 1;
    for (int64_t n : counts) size = mul(n, size);
    size = mul((int64_t)size, elem_bytes);
    const size_t start = (bytes + align - 1) & ~(align - 1);
    if (start > kLim || size > kLim - start) { ok = false; return bytes; }
    bytes = start + size;
    return start;
  }
  size_t add(int64_t count, size_t elem_bytes, size_t align = 256) { return add({count}, elem_bytes, align); }
};

// Coded panel: codes (n u16) | dict (2 columns x 256 doubles) | ok (one int in a 256-B tail).
struct CodedPanelLayout : Carver {
  size_t dict_off = 0, ok_off = 0;
  CodedPanelLayout() = default;
  explicit CodedPanelLayout(int64_t n) : Carver(n >= 1) {
    add(n, sizeof(uint16_t));
    dict_off = add(2 * 256, sizeof(double));
    ok_off = add(256, 1);
  }
  uint16_t* codes(void* base) const { return (uint16_t*)base; }
  double* dict(void* base) const { return (double*)((char*)base + dict_off); }
  int* ok_flag(void* base) const { return (int*)((char*)base + ok_off); }
};

// The rest is internal to the library (dcor_panel, a type of the ABI, holds a CodedPanelLayout).
#pragma GCC visibility push(hidden)
// Premat sub-G scratch: partials (one SubgPartial per replicate slice) | pack (xyc | soc: two double2
// per sample, uncoded shared panel) | a coded panel built per launch (dict), directly behind the pack.
struct PrematScratchLayout : Carver {
  int64_t n = 0;
  size_t pack_off = 0, coded_off = 0;
  CodedPanelLayout coded;
  PrematScratchLayout(int64_t reps, int64_t slices, int64_t n_, bool pack, bool dict) : Carver(n_ >= 1), n(n_) {
    add({reps, slices}, sizeof(SubgPartial));
    pack_off = add(pack ? n_ : 0, 2 * sizeof(double2));
    if (dict) coded = CodedPanelLayout(n_);
    coded_off = add((int64_t)coded.bytes, 1, 1);
    ok = ok && (!dict || coded.ok);
  }
  // the partials from replicate slice `item` on
  void* partials(void* base, int64_t item = 0) const { return (SubgPartial*)base + item; }
  double2* xyc(void* base) const { return (double2*)((char*)base + pack_off); }
  double2* soc(void* base) const { return xyc(base) + n; }
  void* coded_base(void* base) const { return (char*)base + coded_off; }
};

// The seven noise arrays of cr HRS replicates: perm [cr][k m] i32 | lap_x, lap_y [cr][k] | lap_local
// [cr][n] | lap_central [cr] | mix_z, mix_l [cr][nsim], each rounded up to 256 B (the last too).
// cr = 1 gives the bytes per replicate a buffer is sized by; a chunk's layout fits cr times that.
struct HrsNoiseLayout : Carver {
  size_t off[7] = {};
  HrsNoiseLayout(int64_t n, int64_t k, int64_t m, int64_t nsim, int64_t cr) : Carver(n >= 1) {
    const int64_t row[7] = {k, k, k, n, 1, nsim, nsim};
    for (int i = 0; i < 7; ++i) off[i] = add({cr, row[i], i ? 1 : m}, i ? sizeof(double) : sizeof(int32_t));
    add(0, 1);   // the end rounded up
  }
  void point(char* base, HrsNoise& j) const {   // j's seven pointers over `base`
    j.perm = (int32_t*)(base + off[0]);
    double** const d[6] = {&j.lap_x, &j.lap_y, &j.lap_local, &j.lap_central, &j.mix_z, &j.mix_l};
    for (int i = 0; i < 6; ++i) *d[i] = (double*)(base + off[i + 1]);
  }
};

// Fused sweep scratch: partials (one SubgPartial per replicate of the call) | the segment table |
// pack (xyc | soc, uncoded panel).
struct FusedSweepLayout : Carver {
  int64_t n = 0;
  size_t tab_off = 0, pack_off = 0;
  FusedSweepLayout(int64_t items, int64_t nseg, int64_t n_, bool pack) : Carver(n_ >= 1), n(n_) {
    add(items, sizeof(SubgPartial));
    tab_off = add(nseg, sizeof(HrsSegConst));
    pack_off = add(pack ? n_ : 0, 2 * sizeof(double2));
  }
  HrsSegConst* tab(void* base) const { return (HrsSegConst*)((char*)base + tab_off); }
  double2* xyc(void* base) const { return (double2*)((char*)base + pack_off); }
  double2* soc(void* base) const { return xyc(base) + n; }
};

// HRS-table scratch: partials (one SubgPartial per replicate of the call) | the segment table | the
// p clip bounds | the p clipped columns as plain doubles, each zero-padded to npad = n rounded up to
// 4: every column starts 32-B aligned.  columns(n, p), here and below: can the columns alone be held?
struct HrsTableLayout : Carver {
  int64_t npad = 0;
  size_t tab_off = 0, lam_off = 0, cols_off = 0;
  HrsTableLayout(int64_t items = 0, int64_t nseg = 0, int64_t n = 0, int64_t p = 0)
      : Carver(n >= 1 && p >= 1), npad((n + 3) & ~(int64_t)3) {
    add(items, sizeof(SubgPartial));
    tab_off = add(nseg, sizeof(HrsPairSegConst));
    lam_off = add(p, sizeof(double));
    cols_off = add({p, npad}, sizeof(double));
  }
  static HrsTableLayout columns(int64_t n, int64_t p) { return HrsTableLayout(0, 0, n, p); }
  HrsPairSegConst* tab(void* base) const { return (HrsPairSegConst*)((char*)base + tab_off); }
  double* lam(void* base) const { return (double*)((char*)base + lam_off); }
  double* cols(void* base) const { return (double*)((char*)base + cols_off); }
};

// Private HRS-table scratch: partials (one SubgPartial per replicate of the call) | the segment table
// | the p clip intervals (lo, hi) | the p pairs (m1, m2) the preparation writes | the p raw columns
// clipped to their intervals, laid out as HrsTableLayout's.
struct HrsPrivateLayout : Carver {
  int64_t npad = 0;
  size_t tab_off = 0, lohi_off = 0, m12_off = 0, cols_off = 0;
  HrsPrivateLayout(int64_t items = 0, int64_t nseg = 0, int64_t n = 0, int64_t p = 0)
      : Carver(n >= 1 && p >= 1), npad((n + 3) & ~(int64_t)3) {
    add(items, sizeof(SubgPartial));
    tab_off = add(nseg, sizeof(HrsPrivSegConst));
    lohi_off = add(p, 2 * sizeof(double));
    m12_off = add(p, 2 * sizeof(double));
    cols_off = add({p, npad}, sizeof(double));
  }
  static HrsPrivateLayout columns(int64_t n, int64_t p) { return HrsPrivateLayout(0, 0, n, p); }
  HrsPrivSegConst* tab(void* base) const { return (HrsPrivSegConst*)((char*)base + tab_off); }
  double* lohi(void* base) const { return (double*)((char*)base + lohi_off); }
  double* m12(void* base) const { return (double*)((char*)base + m12_off); }
  double* cols(void* base) const { return (double*)((char*)base + cols_off); }
};

// Pairwise HRS-table scratch: partials (one SubgPartial per replicate of the call) | the segment
// table, then the slot table | the p clip bounds | the p masks of nw = ceil(n / 64) words | the
// slots' packed panels (panel_elems double2 in all).
struct HrsPairTableLayout : Carver {
  int64_t nw = 0;
  size_t tab_off = 0, slot_off = 0, lam_off = 0, mask_off = 0, panel_off = 0;
  HrsPairTableLayout(int64_t items = 0, int64_t nseg = 0, int64_t nslot = 0, int64_t n = 0, int64_t p = 0,
                     int64_t panel_elems = 0)
      : Carver(n >= 1 && p >= 1), nw((n + 63) >> 6) {
    add(items, sizeof(SubgPartial));
    tab_off = add(nseg, sizeof(HrsPairNaSegConst));
    slot_off = add(nslot, sizeof(HrsPairSlot));
    lam_off = add(p, sizeof(double));
    mask_off = add({p, nw}, sizeof(uint64_t));
    panel_off = add(panel_elems, sizeof(double2));
  }
  static HrsPairTableLayout columns(int64_t n, int64_t p) { return HrsPairTableLayout(0, 0, 0, n, p, 0); }
  HrsPairNaSegConst* tab(void* base) const { return (HrsPairNaSegConst*)((char*)base + tab_off); }
  HrsPairSlot* slots(void* base) const { return (HrsPairSlot*)((char*)base + slot_off); }
  double* lam(void* base) const { return (double*)((char*)base + lam_off); }
  uint64_t* masks(void* base) const { return (uint64_t*)((char*)base + mask_off); }
  double2* panels(void* base) const { return (double2*)((char*)base + panel_off); }
};

// Private pairwise HRS-table scratch: partials (one SubgPartial per replicate of the call) | the
// segment table, the slot table, the column table | the p clip intervals (lo, hi) | the p pairs
// (m1, m2) the preparation writes | the p masks of nw = ceil(n / 64) words | the columns' compacted
// copies (comp_elems doubles in all: 8 B per present row) | the slots' packed panels (panel_elems
// double2 in all).
struct HrsPrivPairLayout : Carver {
  int64_t nw = 0;
  size_t tab_off = 0, slot_off = 0, col_off = 0, lohi_off = 0, m12_off = 0, mask_off = 0, comp_off = 0,
         panel_off = 0;
  HrsPrivPairLayout(int64_t items = 0, int64_t nseg = 0, int64_t nslot = 0, int64_t n = 0, int64_t p = 0,
                    int64_t comp_elems = 0, int64_t panel_elems = 0)
      : Carver(n >= 1 && p >= 1), nw((n + 63) >> 6) {
    add(items, sizeof(SubgPartial));
    tab_off = add(nseg, sizeof(HrsPrivNaSegConst));
    slot_off = add(nslot, sizeof(HrsPairSlot));
    col_off = add(p, sizeof(HrsPrivCol));
    lohi_off = add(p, 2 * sizeof(double));
    m12_off = add(p, 2 * sizeof(double));
    mask_off = add({p, nw}, sizeof(uint64_t));
    comp_off = add(comp_elems, sizeof(double));
    panel_off = add(panel_elems, sizeof(double2));
  }
  static HrsPrivPairLayout columns(int64_t n, int64_t p) { return HrsPrivPairLayout(0, 0, 0, n, p, 0, 0); }
  HrsPrivNaSegConst* tab(void* base) const { return (HrsPrivNaSegConst*)((char*)base + tab_off); }
  HrsPairSlot* slots(void* base) const { return (HrsPairSlot*)((char*)base + slot_off); }
  HrsPrivCol* cols(void* base) const { return (HrsPrivCol*)((char*)base + col_off); }
  double* lohi(void* base) const { return (double*)((char*)base + lohi_off); }
  double* m12(void* base) const { return (double*)((char*)base + m12_off); }
  uint64_t* masks(void* base) const { return (uint64_t*)((char*)base + mask_off); }
  double* comp(void* base) const { return (double*)((char*)base + comp_off); }
  double2* panels(void* base) const { return (double2*)((char*)base + panel_off); }
};

// Sub-G panel scratch: the segment table | the slot table | the batch means of every slot (16 B
// per batch) | the packed panel (x, y) of n rounded up to npad (a multiple of 4; zeros from n on).
// nmeans: the sum of the slots' k.
struct SubgPanelLayout : Carver {
  int64_t npad = 0;
  size_t tab_off = 0, slot_off = 0, means_off = 0, pack_off = 0;
  SubgPanelLayout(int64_t nseg = 0, int64_t nslots = 0, int64_t nmeans = 0, int64_t n = 0)
      : Carver(n >= 1), npad((n + 3) & ~(int64_t)3) {
    tab_off = add(nseg, sizeof(SubgSegConst));
    slot_off = add(nslots, sizeof(SubgMeanSlot));
    means_off = add(nmeans, sizeof(double2));
    pack_off = add(npad, sizeof(double2));
  }
  SubgSegConst* tab(void* base) const { return (SubgSegConst*)((char*)base + tab_off); }
  SubgMeanSlot* slots(void* base) const { return (SubgMeanSlot*)((char*)base + slot_off); }
  double2* means(void* base) const { return (double2*)((char*)base + means_off); }
  double2* xy(void* base) const { return (double2*)((char*)base + pack_off); }
};

// Sub-G table scratch: the segment table | the slot table | the p NI clips lambda_n(n, eta[c]) | the
// batch means, per column a row of every slot's k means (doubles, [p][nmeans] at pitch mpitch = nmeans
// rounded up to 2, so each row starts 16-B aligned; a slot's means start at its off) | the p columns
// as plain doubles, each zero-padded to npad = n rounded up to 4: every column starts 32-B aligned.
struct SubgTableLayout : Carver {
  int64_t npad = 0, mpitch = 0;
  size_t tab_off = 0, slot_off = 0, clip_off = 0, means_off = 0, cols_off = 0;
  SubgTableLayout(int64_t nseg = 0, int64_t nslots = 0, int64_t nmeans = 0, int64_t n = 0, int64_t p = 0)
      : Carver(n >= 1 && p >= 1 && nmeans >= 0), npad((n + 3) & ~(int64_t)3), mpitch((nmeans + 1) & ~(int64_t)1) {
    tab_off = add(nseg, sizeof(SubgPairSegConst));
    slot_off = add(nslots, sizeof(SubgMeanSlot));
    clip_off = add(p, sizeof(double));
    means_off = add({p, mpitch}, sizeof(double));
    cols_off = add({p, npad}, sizeof(double));
  }
  static SubgTableLayout columns(int64_t n, int64_t p) { return SubgTableLayout(0, 0, 0, n, p); }
  SubgPairSegConst* tab(void* base) const { return (SubgPairSegConst*)((char*)base + tab_off); }
  SubgMeanSlot* slots(void* base) const { return (SubgMeanSlot*)((char*)base + slot_off); }
  double* clips(void* base) const { return (double*)((char*)base + clip_off); }
  double* means(void* base) const { return (double*)((char*)base + means_off); }
  double* cols(void* base) const { return (double*)((char*)base + cols_off); }
};

// Sign-panel scratch: head (the four clipped means, 256 B) | the segment table | the packed panel
// (xc, yc) of n rounded up to a whole 4-sample flip block.
struct SignPanelLayout : Carver {
  int64_t npad = 0;
  size_t tab_off = 0, pack_off = 0;
  SignPanelLayout(int64_t nseg = 0, int64_t n = 0) : Carver(n >= 1), npad((n + 3) & ~(int64_t)3) {
    add(4, sizeof(double));
    tab_off = add(nseg, sizeof(SignSegConst));
    pack_off = add(npad, 2 * sizeof(double));
  }
  double* means(void* base) const { return (double*)base; }
  SignSegConst* tab(void* base) const { return (SignSegConst*)((char*)base + tab_off); }
  void* xyc(void* base) const { return (char*)base + pack_off; }
};

// Sign-table scratch: the per-column means (mean(xc), mean(xc^2) of column c at means[2 c],
// means[2 c + 1]) | the segment table | the p clipped columns as plain doubles, each zero-padded
// to npad = n rounded up to a whole 4-sample flip block, so every column starts 32-B aligned.
struct SignTableLayout : Carver {
  int64_t npad = 0;
  size_t tab_off = 0, cols_off = 0;
  SignTableLayout(int64_t nseg = 0, int64_t n = 0, int64_t p = 0) : Carver(n >= 1 && p >= 1), npad((n + 3) & ~(int64_t)3) {
    add(p, 2 * sizeof(double));
    tab_off = add(nseg, sizeof(SignPairSegConst));
    cols_off = add({p, npad}, sizeof(double));
  }
  double* means(void* base) const { return (double*)base; }
  SignPairSegConst* tab(void* base) const { return (SignPairSegConst*)((char*)base + tab_off); }
  double* cols(void* base) const { return (double*)((char*)base + cols_off); }
};

#pragma GCC visibility pop

}  // namespace dcor
