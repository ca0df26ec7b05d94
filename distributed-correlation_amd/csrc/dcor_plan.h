// dcor_plan.h -- the host decisions that need no device: the error reporter, the argument checks,
// every launch constant (R operation order, cited), the scratch layouts (dcor_layout.h) and the
// segment planners of the ten segment-list entries, one plan struct each.  Plain C++: neither
// this header nor dcor_plan.cpp includes the HIP runtime, so the unit compiles, runs and is
// sanitized with a host compiler alone (tests/host/*.cpp over tests/host/check.h).  Not part of
// the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// dcor_engine.h names two things of the HIP headers: double2 (by pointer, and by size in the
// scratch layouts) and the __host__ __device__ markers.  Where the HIP headers have not been read
// (this unit, the stand-alone test program) they are stand-ins of HIP's size and alignment.
#ifndef HIP_INCLUDE_HIP_HIP_VECTOR_TYPES_H
struct alignas(16) double2 { double x, y; };
#endif
#ifndef __host__
#define __host__
#define __device__
#endif

#include "../../include/dcor.h"
#include "dcor_engine.h"
#include "dcor_layout.h"

static_assert(sizeof(double2) == 16 && alignof(double2) == 16, "the scratch layouts' pack stride");

// A prepared HRS panel (dcor_panel_create): plain data, defined here so the HRS planners can check
// a sweep against its panel without reading the panel before the segments' own fields.
struct dcor_panel {
  const double* X;
  const double* Y;
  int64_t n;
  void* buf;          // CodedPanelLayout(n)
  dcor::CodedPanelLayout lay;
  void* stream;
  int coded;          // host copy of the device flag (read once at create)
  uint16_t* codes() const { return lay.codes(buf); }
  double* dict() const { return lay.dict(buf); }
  int* ok() const { return lay.ok_flag(buf); }
};

namespace dcor {
namespace host {

// Record the message of a failure for dcor_last_error() (thread-local) and return `code`.
int fail(int code, const char* fmt, ...);
// Replicate indices are 32-bit Philox counters: for rep_begin >= 0 and reps >= 0 (the caller
// checks), true when rep_begin + reps > 2^32 - 1 -- without forming the sum, which overflows for
// a huge rep_begin.
inline bool rep_range_exceeds(int64_t rep_begin, int64_t reps) { return rep_begin > 0xffffffffLL - reps; }
double r_min(double a, double b);
double r_max(double a, double b);
// T with (double)w * 2^-32 < p  <=>  w < T for every uint32 w
uint64_t u32_threshold(double p);

// The launch constants of the estimators; each returns the status the reference raises.
int check_common(int64_t n, double eps1, double eps2, double alpha);
int make_mix(int64_t nsim, double alpha, MixConst& mx);
int make_sign(int64_t n, double eps1, double eps2, double alpha, int normalise, int mode,
              int64_t nsim, bool allow_k0, SignConst& c);
int make_subg(int64_t n, double eps1, double eps2, double eta1, double eta2, double alpha,
              int hrs, double lam_x, double lam_y, double lam_s, double lam_o, double lam_r,
              double delta, int64_t nsim, SubgConst& c, double* lo_out, double* crit_sqrt2_s);

// What follows is new with the planning unit and stays out of the library's dynamic symbols.
#pragma GCC visibility push(hidden)

int premat_subg_const(const dcor_premat_subg* d, PrematSubgConst& p);
// per: bytes of one HRS replicate's materialised noise; hrs_chunk: the replicates whose noise
// fits `budget` bytes, capped at `cap`
int hrs_noise_geometry(const dcor_premat_subg* d, int64_t* k, int64_t* m, size_t* per);
int64_t hrs_chunk(size_t per, int64_t reps, size_t budget, int64_t cap);

// ---- the segment planners: every check of an entry after its null checks, in the entry's order,
// then its table of the segments with reps > 0 in call order.  None touches a device. ----

// The sweep's descriptor at one segment's eps (both HRS sweeps).
dcor_premat_subg hrs_segment_desc(const dcor_premat_subg& base, const dcor_hrs_segment& g);

// dcor_hrs_sweep_launch: per segment (reps == 0 included) its descriptor, batch geometry and
// chunk; need: the largest chunk's noise bytes (0: nothing to run), cap: the largest chunk.
struct HrsSweepSeg {
  dcor_premat_subg q;
  int64_t k, m, cr;
};
struct HrsSweepPlan {
  std::vector<HrsSweepSeg> segs;
  size_t need = 0;
  int64_t cap = 0;
};
int plan_hrs_sweep(const dcor_premat_subg* base, const dcor_panel* panel,
                   const dcor_hrs_segment* segs, int64_t nseg, HrsSweepPlan& plan);

// dcor_hrs_fused_sweep_launch: qs, every segment's descriptor (the per-segment fallback's);
// p0, the first kept segment's constants (the sweep-wide ones are read from it); wide, whether the
// sweep-wide constants are the same in every kept segment; max_km, the largest k m.
struct HrsFusedSweepPlan {
  std::vector<dcor_premat_subg> qs;
  std::vector<HrsSegConst> tab;
  PrematSubgConst p0;
  bool wide = true;
  int64_t max_km = 0, items = 0;
};
int plan_hrs_fused_sweep(const dcor_premat_subg* base, const dcor_panel* panel,
                         const dcor_hrs_segment* segs, int64_t nseg, HrsFusedSweepPlan& plan);

// ---- the eight table entries: int plan_X(desc, segs, nseg, XPlan&).  A planner resets its plan and
// makes every check of its entry after the null checks of the descriptor, segs and d_out, in the
// order include/dcor.h documents; a segment without replicates is checked too.  On DCOR_OK the plan
// is all the entry needs: tab, the records of the segments with reps > 0 in call order; items, the
// call's replicates; c0, the call-wide constants; lay, the call's scratch, built once. ----
template <class Record, class Layout> struct TablePlan {
  std::vector<Record> tab;
  int64_t items = 0;
  Layout lay;
};

// dcor_sign_panel_launch, dcor_sign_table_launch: a record is make_sign's constants with the
// segment's key, first replicate and place (and columns); the call-wide ones are tab[0].s's.
using SignPanelPlan = TablePlan<SignSegConst, SignPanelLayout>;
using SignTablePlan = TablePlan<SignPairSegConst, SignTableLayout>;
int plan_sign_panel(const dcor_sign_panel_desc* p, const dcor_sign_segment* segs, int64_t nseg,
                    SignPanelPlan& plan);

// dcor_hrs_table_launch.  The reference call of a segment (include/dcor.h): the descriptor
// dcor_hrs_fused_launch takes for the pair's columns, clip bounds and eps (lam_x = lam_s = lam[col_x],
// lam_y = lam_o = lam[col_y], eta = 1, lam_r = lambda_receiver_from_noise; X, Y the columns'
// addresses, never read here).  g's columns must be in [0, t.p).
dcor_premat_subg hrs_pair_desc(const dcor_hrs_table_desc& t, const dcor_hrs_pair_segment& g);
// A record holds, field for field, what plan_hrs_fused_sweep builds for hrs_pair_desc.  c0: the
// first kept segment's constants with X and Y null; max_km: the largest k m of the kept segments.
struct HrsTablePlan : TablePlan<HrsPairSegConst, HrsTableLayout> {
  PrematSubgConst c0{};
  int64_t max_km = 0;
};
int plan_hrs_table(const dcor_hrs_table_desc* t, const dcor_hrs_pair_segment* segs, int64_t nseg,
                   HrsTablePlan& plan);

// dcor_hrs_private_table_launch.  A record holds plan_hrs_table's fields that do not depend on a
// clip bound (the geometry, m_over_k, sqrt_k, eps_r, the keys, the place) and zeros in those that do:
// every replicate derives them on the device with hrs_lambda_consts from its own release, out of
// log_inv_delta = log(1 / delta) and crit_sqrt2 = crit * sqrt(2.0), both computed here.  lohi: the p
// intervals as (lo, hi) pairs, the block the entry uploads; pv: the budgets and the key of
// DCOR_SITE_STD; c0: n, nd, sqrt_n, crit, mix, hrs of any segment's make_subg, else zero.
struct HrsPrivatePlan : TablePlan<HrsPrivSegConst, HrsPrivateLayout> {
  std::vector<double> lohi;
  HrsPrivCall pv{};
  PrematSubgConst c0{};
  int64_t max_km = 0;
};
int plan_hrs_private(const dcor_hrs_private_desc* t, const dcor_hrs_pair_segment* segs, int64_t nseg,
                     HrsPrivatePlan& plan);

// dcor_hrs_table_pairwise_launch.  The rows present in both columns: popcount of the ANDed mask words
// (column c's nw = ceil(n / 64) words at valid + c * nw), the last word's bits at i >= n masked off.
int64_t hrs_pair_count(const uint64_t* valid, int64_t n, int64_t col_x, int64_t col_y);
// slots: the distinct ordered pairs of the kept segments in order of first use, each with its n_ab
// and its panel's first element (hrs_pair_panel_elems apart); panel_elems: the panels' double2
// elements in all.  A record is plan_hrs_table's at n = n_ab (2 <= n_ab <= DCOR_DICT_NMAX) and delta =
// t->delta or 1 / n_ab, with n_ab, nd, sqrt_n (make_subg's), the Feistel split of ceil(log2 n_ab)
// bits and its slot's panel.
struct HrsPairTablePlan : TablePlan<HrsPairNaSegConst, HrsPairTableLayout> {
  std::vector<HrsPairSlot> slots;
  PrematSubgConst c0{};
  int64_t max_km = 0, panel_elems = 0;
};
int plan_hrs_table_pairwise(const dcor_hrs_table_na_desc* t, const dcor_hrs_pair_segment* segs,
                            int64_t nseg, HrsPairTablePlan& plan);

// dcor_hrs_private_pairwise_launch.  slots, panel_elems: plan_hrs_table_pairwise's slot table (the
// distinct ordered pairs, n_ab, the panel's first element).  A record is plan_hrs_private's at n =
// n_ab and delta = t->delta or 1 / n_ab (log_inv_delta follows), with n_ab, nd, sqrt_n, the Feistel
// split and the slot's panel as plan_hrs_table_pairwise's record, and the two columns' own counts n_x,
// n_y = popcount(valid[c]) as the doubles the release divides by.  cols: every column's count and the
// first element of its compacted copy (hrs_priv_col_elems apart; comp_elems in all); lohi, pv: as
// plan_hrs_private's; c0: crit, mix, hrs (n, nd, sqrt_n are the first kept segment's: the records
// carry their own).
struct HrsPrivPairPlan : TablePlan<HrsPrivNaSegConst, HrsPrivPairLayout> {
  std::vector<HrsPairSlot> slots;
  std::vector<HrsPrivCol> cols;
  std::vector<double> lohi;
  HrsPrivCall pv{};
  PrematSubgConst c0{};
  int64_t max_km = 0, panel_elems = 0, comp_elems = 0;
};
int plan_hrs_private_pairwise(const dcor_hrs_private_na_desc* t, const dcor_hrs_pair_segment* segs,
                              int64_t nseg, HrsPrivPairPlan& plan);

// dcor_subg_panel_launch.  A record holds, field for field, what make_subg yields for (n, eps1, eps2,
// eta1, eta2, alpha, hrs = 0, nsim).  slots: the distinct batch sizes m of the kept segments in order
// of first use (m_slot names a record's entry, mean_off that entry's off); c0: the first kept's.
struct SubgPanelPlan : TablePlan<SubgSegConst, SubgPanelLayout> {
  std::vector<SubgMeanSlot> slots;
  SubgConst c0{};
};
int plan_subg_panel(const dcor_subg_panel_desc* p, const dcor_subg_segment* segs, int64_t nseg,
                    SubgPanelPlan& plan);

// dcor_subg_table_launch.  A record is plan_subg_panel's for the segment's reference call (X = column
// col_x, Y = column col_y, eta1 = eta[col_x], eta2 = eta[col_y]), and its columns.  clips: the p NI
// clips lambda_n(n, eta[c]) (empty when nothing is kept); c0: n, nd, sqrt_n, crit, mix, else zero.
struct SubgTablePlan : TablePlan<SubgPairSegConst, SubgTableLayout> {
  std::vector<SubgMeanSlot> slots;
  std::vector<double> clips;
  SubgConst c0{};
};
int plan_subg_table(const dcor_subg_table_desc* t, const dcor_subg_pair_segment* segs, int64_t nseg,
                    SubgTablePlan& plan);

#pragma GCC visibility pop

// C linkage and exported: the one planner among the library's dynamic symbols.
extern "C" int plan_sign_table(const dcor_sign_table_desc* t, const dcor_sign_pair_segment* segs,
                               int64_t nseg, SignTablePlan& plan);

}  // namespace host
}  // namespace dcor
