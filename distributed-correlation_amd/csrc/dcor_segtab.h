// dcor_segtab.h -- the device side of a segment-table launch (dcor_hrs_fused_sweep_launch,
// dcor_sign_panel_launch, dcor_sign_table_launch, dcor_hrs_table_launch,
// dcor_hrs_table_pairwise_launch, dcor_hrs_private_table_launch, dcor_hrs_private_pairwise_launch,
// dcor_subg_panel_launch, dcor_subg_table_launch): a persistent grid whose work unit u takes items u,
// u + units, ... and reads the constants of the segment an item belongs to from a device table the
// host planner built (dcor_plan.cpp).
//
// The table contract, for every record type Seg: `first` (the segment's first item) is strictly
// increasing with tab[0].first == 0, so only segments with reps > 0 are present and segment s holds
// the items [tab[s].first, tab[s + 1].first), the last one up to the launch's item count.  The
// table is read through the constant address space at wave-uniform addresses: scalar loads into
// SGPRs, never per lane.  Which fields of a record are per-segment is the family's own loader's
// business (sp_seg_load, sgp_seg_load, hrs_seg_load).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcor {

template <class Seg> using SegTab = const __attribute__((address_space(4))) Seg*;

// The last segment whose first item is <= it.
template <class Seg>
__device__ __forceinline__ int seg_find(SegTab<Seg> tab, int nseg, int64_t it) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= it) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// A work unit's items ascend, so it re-reads the table only when an item passes the end of the
// segment it holds.  seek(it) on entering a segment calls enter(s) with the wave-uniform index s --
// the kernel's field loader and whatever else changes with the segment (out_row, columns, means) --
// and returns s; it returns -1 when the held segment still covers `it`.
struct SegCursor {
  int64_t first = 0, end = 0;   // items [first, end) belong to the held segment
  template <class Seg, class Enter>
  __device__ __forceinline__ int seek(SegTab<Seg> tab, int nseg, int64_t items, int64_t it, Enter enter) {
    if (it < end) return -1;
    const int s = __builtin_amdgcn_readfirstlane(seg_find(tab, nseg, it));
    enter(s);
    first = tab[s].first;
    end = s + 1 < nseg ? tab[s + 1].first : items;
    return s;
  }
};

}  // namespace dcor
