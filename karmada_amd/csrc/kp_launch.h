// kp_launch.h — arguments shared by the kernels and their launchers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kp_layout.h"
#include "kp_paths.h"

namespace kp {

struct KArgs {
  SnapView s;
  BatchView bv;
  const int32_t* list;    // binding ids handled by this launch
  int32_t n;
  const uint64_t* fmask;  // [B][W]
  // calAvailableReplicas rows: [B][Cp] merged per binding (bcls == nullptr), or
  // [n_classes][Cp] raw GeneralEstimator rows of the estimator classes, binding b
  // reading row bcls[b] (row 0: non-workload bindings, MaxInt32).
  const int32_t* est;
  const int32_t* bcls;
  Sink sink;
  int32_t* slow;          // [B] SLOW_* reason the binding needs k_slow for (0: none)
  int32_t* slow_ids;      // bindings flagged for k_slow, [0, stats[KS_SLOW_TOTAL]) (append order)
  uint32_t* stats;        // the batch's counters, [kStatSlots] (KS_* below)
  unsigned long long* dbg;  // diagnostic build only: phase cycle sums (nullptr otherwise)
  // set: the launch covers list[0, *n_dev) with a grid-stride loop (a list another
  // kernel appended to, e.g. k_select_top's fallback list); n is its capacity
  const uint32_t* n_dev = nullptr;
  // k_class_order's per-class orders and walkability (bits mode; nullptr when the
  // batch did not compute them): the spread kernels' class-order shortcut
  const uint64_t* ord = nullptr;
  const int32_t* cok = nullptr;
  uint32_t* n_order = nullptr;  // count of the bindings that took it
  // set (with n_dev): loop index j stands for list position sub[j] (a device-appended
  // fallback list of positions, so per-position arrays such as rsel stay aligned)
  const int32_t* sub = nullptr;
  // set: the estimator class of list[i] (k_select_top loads it with the list entry, so the
  // class order and class flags load one dependent global load earlier)
  const int32_t* lcls = nullptr;
};

// The batch's device counters (KArgs::stats; kp_batch::h_stats is their host copy after a
// schedule call). The kernels index [KS_SLOW_TOTAL], [SLOW_* reason] and [KS_TIE_BLOCK]
// themselves; the host hands the others out as pointers (TopArgs, OrderArgs, n_dev, n_order).
enum : int {
  KS_SLOW_TOTAL = 0,  // bindings flagged for the serial path; [1..6]: by SLOW_* reason (kp_paths.h)
  KS_TIE_BLOCK = 7,         // of the SLOW_TIE ones, resolved block-parallel
  // (slot 8 is unused: the component-set overflow is reported per class, kp_batch::d_sets_ovf)
  KS_TOP_FALLBACK = 9,      // k_select_top's fallback list length
  KS_CLUSTER_ORDER = 10,    // cluster-spread bindings selected over the class order
  KS_REGION_ORDER = 11,     // region-spread bindings selected over the class order
  KS_FB_CLUSTER = 12,       // k_spread_order's fallback list length, cluster positions
  KS_FB_REGION = 13,        // ... region positions
  KS_FB_REGION_A = 14,      // k_region_a_order's fallback list length
  KS_CHECK = 15,            // diagnostic builds' check counter
  KS_TOP_OVERFLOW = 16,     // k_select_top's capacity overflows (the top_cap_mid launch)
  KS_REGION_WIDE_DONE = 17  // bindings k_region_wide scheduled or errored
};
constexpr int kStatSlots = 20;
static_assert((int)SLOW_CLUSTER < (int)KS_TIE_BLOCK, "the SLOW_* reasons index the counters below KS_TIE_BLOCK");

enum : int {
  SEL_LAUNCH_ALL = 0,
  SEL_LAUNCH_CLUSTER,
  SEL_LAUNCH_REGION_A,
  SEL_LAUNCH_REGION_B,
  SEL_LAUNCH_SLOW,
  SEL_LAUNCH_ALL_STREAM  // SEL_ALL over streamed candidates (bits mode)
};

struct SelectExtra {
  RegionOut* rout = nullptr;         // region A output [n][n_regions]
  int32_t* rstat = nullptr;          // region A status [n]
  const int32_t* rsel = nullptr;     // region B input [n][n_regions]
  const int32_t* rnsel = nullptr;    // region B input [n]
  unsigned char* scratch = nullptr;  // slow path global scratch
  size_t slot_bytes = 0;
  int grid = 0;                      // slow path persistent grid
  int list_grid = 0;                 // > 0: caps the grid of a launch over a device-appended list
                                     // (its count read back by the host: no idle workgroups)
  int lds_area = 0;                  // slow path: LDS bytes for the small serial problems
  int lds_sort = 0;                  // slow path: LDS bytes for the candidate sorts (0: global slot)
  // the launch's KArgs in device memory: the kernels whose bodies keep pointers into
  // their arguments (SelCtx: &a.s, &a.bv) across calls take them by pointer, since a
  // by-value kernel argument would be copied to scratch by every wave (~34 KB per wave)
  const KArgs* dargs = nullptr;
};
// A binding of kp_batch_create_filters that has a row of the out-of-tree filter plugins'
// verdicts: (binding index, row id), the list sorted by binding index.
struct FltPair {
  int32_t b, r;
};

// device KArgs slots per batch (one per such launch in a schedule call)
constexpr int kArgSlots = 16;

constexpr int kBlock = 256;
constexpr int kSlowBlock = 512;  // k_slow: wider for the LDS bitonic sort
// waves per workgroup of the one-wave-per-binding kernels (each wave its own LDS slice)
// Waves per workgroup of the one-wave-per-binding kernels. LDS is granted per workgroup and
// held until its last wave ends, so a finished binding's slice waits for its neighbours':
// k_select_top at 1 / 2 / 4 waves per workgroup 0.751 / 0.819 / 0.935 ms (same box,
// profiles/r06_ab/waves_*.json).
#ifndef KP_TOP_WAVES
#define KP_TOP_WAVES 1
#endif
#ifndef KP_STATIC_WAVES
#define KP_STATIC_WAVES 4
#endif
#ifndef KP_ORDER_WAVES
#define KP_ORDER_WAVES 4
#endif
constexpr int kTopWaves = KP_TOP_WAVES;        // k_select_top
constexpr int kStaticWaves = KP_STATIC_WAVES;  // k_select_static
constexpr int kOrderWaves = KP_ORDER_WAVES;    // k_spread_order, k_region_a_order
constexpr int kPairStage = 4096;  // bytes of per-binding predicate data staged in LDS
constexpr int kTsetMax = 4096;    // distinct taint lists answered once per binding (LDS bits)


constexpr int kOffThreads = 256, kOffChunk = 4 * kOffThreads;  // CSR offsets scan (body_offsets_a/b)
constexpr int kSwRules = 4;  // StaticWeight rules kept as LDS bitsets (more: per-cluster static_vote)
// Dynamic LDS of k_select_all_stream (kp_kernels.h body_select_all_stream).
KP_HD inline size_t sel_stream_lds_bytes(int Cp) {
  const int words = (Cp + 31) >> 5, W = Cp / 64;
  return kRedBytes + 4 * (size_t)((words + 3) & ~3) + 8 * (size_t)kSwRules * W + 3072 + 8 * (size_t)sel_all_ecap(Cp) +
         64;
}
// Dynamic LDS of the other kernels that carve it by cluster count: the one size both device
// builds launch with (kernels.hip; dev_cpu.cpp, whose workgroups get exactly these bytes and
// a guard band behind them) and batch_lds_check holds against the device's limit. Each
// follows its body's carve in kp_kernels.h: [red | ...], 8 B per cluster of gathered
// candidates (rank, votes) and 2 B more of region ids in the region stages.
// k_pair* (pair_lds_carve): target and eviction bits, MaxDivided table, predicate stage, taint bits.
KP_HD inline size_t pair_lds_bytes(int Cp, int md_cap) {
  const int words = (Cp + 31) >> 5;
  return kRedBytes + 8 * (size_t)words + 4 * (size_t)((md_cap + 3) & ~3) + kPairStage + kTsetMax / 8 + 64;
}
// k_select_all / _wide (body_select_all): target bits, candidates, SelScratch.
KP_HD inline size_t sel_all_lds_bytes(int Cp) {
  const int words = (Cp + 31) >> 5;
  return kRedBytes + 4 * (size_t)((words + 3) & ~3) + 8 * (size_t)Cp + 3072 + 8 * (size_t)sel_all_ecap(Cp) + 64;
}
// k_select_cluster (body_select_cluster): cap = entries of its serial scratch.
KP_HD inline size_t sel_cluster_lds_bytes(int Cp, int cap) {
  const int words = (Cp + 31) >> 5;
  const size_t cand = 8 * (size_t)Cp, ser = serial_scratch_bytes(cap);
  return kRedBytes + 1024 + sizeof(Item) * 2 * kSmallMax + 16 * kSmallMax + 4 * (size_t)((words + 3) & ~3) +
         (cand > ser ? cand : ser) + 64;
}
// k_region_a (body_region_a), R regions.
KP_HD inline size_t region_a_lds_bytes(int Cp, int R) {
  const int words = (Cp + 31) >> 5;
  return kRedBytes + 80 * (size_t)R + 4 * (size_t)((words + 3) & ~3) + 10 * (size_t)Cp + 64;
}
// k_region_b (body_region_b): cand r/v/g, then the serial scratch in their place.
KP_HD inline size_t region_b_lds_bytes(int Cp, int R, int cap) {
  const int words = (Cp + 31) >> 5;
  const size_t cand = 10 * (size_t)Cp, ser = serial_scratch_bytes(cap);
  return kRedBytes + 1024 + sizeof(Item) * 2 * kSmallMax + 16 * kSmallMax + 8 * (size_t)R + 4 * (size_t)((R + 3) & ~3) +
         4 * (size_t)((words + 3) & ~3) + (cand > ser ? cand : ser) + 64;
}
// k_est_class* (body_est_class): the MaxDivided table; feasible: and the representative's
// feasible clusters compacted behind it (at most Cp).
KP_HD inline size_t est_class_lds_bytes(int Cp, bool feasible) {
  return kRedBytes + 4 * (size_t)kTmplDense + (feasible ? 4 * (size_t)Cp : 0);
}
// k_class_order (body_class_order): the bitonic sort's P = class_order_pad(C) keys.
KP_HD inline int class_order_pad(int C) {
  int P = 1;
  while (P < C) P <<= 1;
  return P;
}
KP_HD inline size_t class_order_lds_bytes(int P) { return kRedBytes + 8 * (size_t)P; }
// k_fit_hist (body_fit_hist): per wave, the histogram bin of each distinct taint list.
constexpr int kFitHistWaves = 4;  // one wave per diagnosed binding, as k_filter
KP_HD inline size_t fit_hist_lds_bytes() { return 4 * (size_t)kTsetRowsMax; }
// k_changed_long (body_changed_long): the result's replicas by cluster rank and a presence
// bit per cluster (77 848 bytes at the 18 624-cluster ceiling).
KP_HD inline size_t changed_lds_bytes(int Cp) { return kRedBytes + 4 * (size_t)Cp + 4 * (size_t)((Cp + 31) >> 5); }
// k_assume_cluster / k_est_assumed (kp_assume.h): one wave per item, the runs in global
// scratch; the waves' reduction slots only.
constexpr int kEstAssumedWaves = 4;  // (row, assumed cluster) items per workgroup
KP_HD inline size_t assume_cluster_lds_bytes() { return 16; }
KP_HD inline size_t est_assumed_lds_bytes() { return 16 * (size_t)kEstAssumedWaves; }
// k_slow (body_slow): target bits, lds_area bytes for the small serial problems, lds_sort
// for the candidate sorts.
KP_HD inline size_t slow_lds_bytes(int Cp, int lds_area, int lds_sort) {
  return kRedBytes + 512 + 4 * (size_t)(((Cp + 31) >> 5) + 4) + (size_t)lds_area + (size_t)lds_sort;
}
}  // namespace kp
