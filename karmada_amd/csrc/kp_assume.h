// kp_assume.h — the scheduler's assumed workloads (SchedulingOvercommitProtection)
// deducted from a batch's estimator rows.
//
//   k_assume_cluster  once per kp_assumptions_create, one wave per cluster that has
//                     entries: deductAssumedWorkloadsFromSummary's sums (estimator/client/
//                     general.go:110-151) and, for a model cluster, the model nodes left
//                     after every workload's SimulateScheduling(components, 1)
//                     (general.go:531-546), as runs of identical nodes (kp_sets.h).
//   k_est_assumed     every schedule call of an assumed batch, one wave per (estimate
//                     row, assumed cluster): GeneralEstimator.maxAvailableReplicas
//                     (general.go:66-108) over the deducted state, written over the
//                     row's entry.
#pragma once
#include "kp_algo.h"
#include "kp_nodes.h"  // kp_fence_wg

namespace kp {

// One request entry of an assumed component. The summary path's demand and the model
// node's requiredPerReplica use the same unit (MilliValue for cpu, Value otherwise), so
// one value serves both; `kind` says which paths read it.
enum : int32_t {
  AQ_NODE = 1,  // util.NewResource keeps it (cpu, memory, ephemeral-storage, scalar resources)
  AQ_PODS = 2,  // the request names "pods": the summary's Allocating pods grow by it too
};
struct AssumedReq {
  int32_t rid;   // snapshot resource id, -1: no cluster's summary or model names it
  int32_t kind;  // AQ_*
  int64_t val;   // >= 0
};
enum : int32_t {
  AS_OK = 0,
  AS_SUM_OVERFLOW = 1,  // a per-resource (or pod) sum left int64
  AS_RUN_CAPACITY = 2,  // the residual nodes needed more runs than the cluster's scratch holds
};

struct AssumedView {
  int32_t n = 0;      // clusters with entries
  int32_t n_res = 0;  // the snapshot's resource dictionary at creation
  int32_t rid_pods = -1;  // the dictionary's "pods" (the summary path divides by it for a request that names pods)
  const int32_t* rank = nullptr;      // [n] ascending
  const int32_t* wl_off = nullptr;    // [n + 1] workloads of cluster a, in the caller's order
  const int32_t* comp_off = nullptr;  // [workloads + 1] components of a workload
  const int32_t* c_rep = nullptr;     // [components] Replicas (>= 0)
  const int32_t* c_rr = nullptr;      // [components] ReplicaRequirements != nil
  const int32_t* req_off = nullptr;   // [components + 1]
  const AssumedReq* req = nullptr;
  int64_t* pods = nullptr;            // [n] pods added to Allocating
  int64_t* sums = nullptr;            // [n][n_res] demand added to Allocating
  const int64_t* run_off = nullptr;   // [n + 1] the clusters' run scratch (units of runs)
  int64_t* runs = nullptr;            // run = [count | capacity[n_res] | pods]
  int32_t* n_runs = nullptr;          // [n] residual runs (0 for a cluster off the model path)
  int32_t* status = nullptr;          // [n] AS_*
};

// Resource.MaxDivided (util/resource.go:221-248) of one run's node for component k:
// AllowedPodNumber (request 1), then every positive entry NewResource keeps.
KP_HD inline int64_t assume_maxdiv(const AssumedView& A, const int64_t* run, int k) {
  int64_t res = run[1 + A.n_res];
  for (int q = A.req_off[k]; q < A.req_off[k + 1]; q++) {
    const AssumedReq r = A.req[q];
    if (!(r.kind & AQ_NODE) || r.val <= 0) continue;
    const int64_t d = r.rid < 0 ? 0 : run[1 + r.rid] / r.val;
    res = d < res ? d : res;
  }
  return res;
}
// Component k's requiredPerReplica entry of run slot j (0 = count, 1 + rid, 1 + n_res = pods).
KP_HD inline int64_t assume_req_of(const AssumedView& A, int k, int j) {
  if (j == 1 + A.n_res) return 1;
  for (int q = A.req_off[k]; q < A.req_off[k + 1]; q++)
    if ((A.req[q].kind & AQ_NODE) && A.req[q].rid == j - 1) return A.req[q].val;
  return 0;
}
// SubResource(requiredPerReplica.Clone().Multiply(f)) on slot j >= 1: Go's wrapping product
// and difference, clamped at 0 (util/resource.go:77-115).
KP_HD inline int64_t assume_sub(int64_t cap, int64_t req, int64_t f) {
  const int64_t v = (int64_t)((uint64_t)cap - (uint64_t)req * (uint64_t)f);
  return v > 0 ? v : 0;
}

// Moves runs [from, nr) to start at run `to` (to != from), the lanes over the flat
// elements: a step reads 64 elements, then writes them, and the steps walk away from the
// overlap, so nothing is overwritten before it is read.
template <class Blk>
KP_HD inline void assume_move(const Blk& b, int64_t* runs, int stride, int from, int to, int nr) {
  const int64_t n = (int64_t)(nr - from) * stride, W = b.wwidth();
  const int64_t src = (int64_t)from * stride, dst = (int64_t)to * stride;
  if (n <= 0) return;
  const int64_t steps = (n + W - 1) / W;
  for (int64_t t = 0; t < steps; t++) {
    const int64_t i = (to < from ? t : steps - 1 - t) * W + b.lane();
    int64_t v = 0;
    if (i < n) v = runs[src + i];
    kp_fence_wg();
    if (i < n) runs[dst + i] = v;
    kp_fence_wg();
  }
}

// Cluster a of the assumptions: sums, pods, and the residual model nodes. One wave64 on
// the device (a "wave" of one lane on the host build); every branch is wave-uniform.
template <class Blk>
KP_HD inline void body_assume_cluster(const Blk& b, const SnapView& s, const AssumedView& A, int a) {
  const int lane = b.lane(), W = b.wwidth(), R = A.n_res, stride = R + 2;
  const int c = A.rank[a];
  const int w0 = A.wl_off[a], w1 = A.wl_off[a + 1];
  // deductAssumedWorkloadsFromSummary: pods of every component with replicas > 0, demand
  // of those with requirements; lane l owns resources l, l + W, ...
  bool ovf = false;
  __int128 pods = 0;
  for (int w = w0; w < w1; w++)
    for (int k = A.comp_off[w]; k < A.comp_off[w + 1]; k++) {
      if (A.c_rep[k] <= 0) continue;
      pods += A.c_rep[k];
      if (!A.c_rr[k]) continue;
      for (int q = A.req_off[k]; q < A.req_off[k + 1]; q++)
        if (A.req[q].kind & AQ_PODS) pods += (__int128)A.req[q].val * A.c_rep[k];
    }
  if (pods > (__int128)INT64_MAX) ovf = true;
  for (int r0 = 0; r0 < R; r0 += W) {
    const int r = r0 + lane;
    __int128 acc = 0;
    if (r < R)
      for (int w = w0; w < w1; w++)
        for (int k = A.comp_off[w]; k < A.comp_off[w + 1]; k++) {
          if (A.c_rep[k] <= 0) continue;
          if (r == A.rid_pods) acc += A.c_rep[k];  // Allocating["pods"] takes the replicas themselves (general.go:124-125)
          if (!A.c_rr[k]) continue;
          for (int q = A.req_off[k]; q < A.req_off[k + 1]; q++)
            if (A.req[q].rid == r) acc += (__int128)A.req[q].val * A.c_rep[k];
        }
    if (acc > (__int128)INT64_MAX) ovf = true;
    if (r < R) A.sums[(size_t)a * R + r] = ovf ? 0 : (int64_t)acc;
  }
  const bool any_ovf = b.wballot(ovf) != 0;
  int32_t st = any_ovf ? AS_SUM_OVERFLOW : AS_OK;
  int nr = 0;
  // The model path is decided by the undeducted cluster (general.go:89): CF_MODEL_OK.
  const bool model = !any_ovf && (s.flags[c] & CF_MODEL_OK) != 0;
  int64_t* runs = A.runs + (size_t)A.run_off[a] * stride;
  const int rcap = (int)(A.run_off[a + 1] - A.run_off[a]);
  if (model) {
    for (int k = 0; k < s.kmax && st == AS_OK; k++) {  // buildModelNodes: grades ascending
      const int32_t cnt = s.mg_cnt[(size_t)k * s.Cp + c];
      if (cnt <= 0) continue;
      if (nr == rcap) {
        st = AS_RUN_CAPACITY;
        break;
      }
      const int32_t tid = s.mg_tid[(size_t)k * s.Cp + c];
      for (int j = lane; j < stride; j += W)
        runs[(size_t)nr * stride + j] = j == 0 ? cnt : (j == stride - 1 ? kMaxPodsPerNode : s.tmpl[(size_t)tid * s.n_res + (j - 1)]);
      nr++;
    }
    kp_fence_wg();
  }
  // run i merged into i - 1 when their capacities are equal; returns whether it was
  auto merge_left = [&](int i) -> bool {
    if (i <= 0 || i >= nr) return false;
    bool diff = false;
    for (int j = 1 + lane; j < stride; j += W)
      diff = diff || runs[(size_t)(i - 1) * stride + j] != runs[(size_t)i * stride + j];
    if (b.wballot(diff) != 0) return false;
    if (lane == 0) runs[(size_t)(i - 1) * stride] += runs[(size_t)i * stride];
    kp_fence_wg();
    assume_move(b, runs, stride, i + 1, i, nr);
    nr--;
    return true;
  };
  for (int w = w0; w < w1 && model && st == AS_OK; w++) {
    // one SimulateScheduling(components, 1); a workload without components is skipped
    // (general.go:536), one that stops fitting leaves what it placed
    bool ok = true;
    for (int k = A.comp_off[w]; k < A.comp_off[w + 1] && ok && st == AS_OK; k++) {
      int64_t rem = A.c_rep[k];
      int i = 0;
      while (rem > 0) {  // scheduleComponent: first fit over the runs from i on
        int found = -1;
        int64_t m = 0;
        for (int base = i; base < nr; base += W) {
          const int r = base + lane;
          int64_t mm = 0;
          if (r < nr) mm = assume_maxdiv(A, runs + (size_t)r * stride, k);
          const uint64_t bal = b.wballot(mm > 0);
          if (bal) {
            const int f = ctz64(bal);
            found = base + f;
            m = b.wread(mm, f);
            break;
          }
        }
        if (found < 0) break;
        int64_t* r = runs + (size_t)found * stride;
        const int64_t cnt = r[0];
        const __int128 all = (__int128)m * cnt;
        if ((__int128)rem >= all) {  // every node of the run takes m
          for (int j = 1 + lane; j < stride; j += W) r[j] = assume_sub(r[j], assume_req_of(A, k, j), m);
          kp_fence_wg();
          rem -= (int64_t)all;
          i = merge_left(found) ? found : found + 1;
          continue;
        }
        // partial: q nodes take m, one takes rem % m, the rest keep their capacity
        const int64_t q = rem / m, rr = rem % m, rest = cnt - q - (rr > 0 ? 1 : 0);
        const int parts = (q > 0) + (rr > 0) + (rest > 0);
        if (nr + parts - 1 > rcap) {
          st = AS_RUN_CAPACITY;
          break;
        }
        if (parts > 1) assume_move(b, runs, stride, found + 1, found + parts, nr);
        // written last part first: the first part lies over the run the others copy from
        const int64_t pc[3] = {q, rr > 0 ? 1 : 0, rest}, pt[3] = {m, rr, 0};
        int at = found + parts - 1;
        for (int p = 2; p >= 0; p--) {
          if (pc[p] <= 0) continue;
          for (int j = lane; j < stride; j += W)
            runs[(size_t)at * stride + j] = j == 0 ? pc[p] : assume_sub(r[j], assume_req_of(A, k, j), pt[p]);
          kp_fence_wg();
          at--;
        }
        nr += parts - 1;
        (void)merge_left(found);
        rem = 0;
      }
      if (rem > 0) ok = false;
    }
  }
  if (lane == 0) {
    A.pods[a] = any_ovf ? 0 : (int64_t)pods;
    A.n_runs[a] = st == AS_OK ? nr : 0;
    A.status[a] = st;
  }
}

// GeneralEstimator.maxAvailableReplicas (general.go:66-108) for binding header h on
// assumed cluster a over the deducted state; the lanes share the residual runs.
template <class Blk>
KP_HD inline int32_t assumed_estimate(const Blk& b, const SnapView& s, const BatchView& bv, const BindHdr& h,
                                      const AssumedView& A, int a) {
  const int c = A.rank[a];
  const uint32_t f = s.flags[c];
  if (!(f & CF_HAS_SUMMARY)) return 0;
  // (the column is clamped at 0 and the pods only grow, so the clamp commutes)
  const int64_t allowed = s.allowed[c] - A.pods[a];
  if (allowed <= 0) return 0;
  if (!(h.flags & BF_HAS_RR)) return (int32_t)allowed;
  int64_t m = allowed;
  if (f & CF_MODEL_OK) {
    // the one-pod component over the residual nodes: each absorbs its MaxDivided
    const int stride = A.n_res + 2, nr = A.n_runs[a];
    const int64_t* runs = A.runs + (size_t)A.run_off[a] * stride;
    int64_t part = 0;
    for (int i = b.lane(); i < nr; i += b.wwidth()) {
      const int64_t* r = runs + (size_t)i * stride;
      int64_t d = r[stride - 1];
      for (int j = 0; j < h.mreq_cnt; j++) {
        const int32_t rid = bv.ipool[h.mreq_off + j];
        const int64_t x = rid < 0 ? 0 : r[1 + rid] / bv.lpool[h.mreq_q_off + j];
        d = x < d ? x : d;
      }
      part += d * r[0];  // d <= 110, count <= MaxInt32, at most kSetsRunsMax runs: below 2^51
    }
    int64_t total = b.sum64(part);
    if (total >= kInt32Max) total = kInt32Max;  // SimulateScheduling's upper bound
    if (total < m) m = total;
    return (int32_t)m;
  }
  // getMaximumReplicasBasedOnClusterSummary over Allocating + the sums
  int64_t num = INT64_MAX;
  for (int j = 0; j < h.sreq_cnt; j++) {
    const int32_t rid = bv.ipool[h.sreq_off + j];
    if (rid < 0) return 0;
    int64_t av = s.avail[(size_t)rid * s.Cp + c];
    if (av <= 0) return 0;
    av -= A.sums[(size_t)a * A.n_res + rid];
    if (av <= 0) return 0;
    const int64_t d = av / bv.lpool[h.sreq_q_off + j];
    if (d < num) num = d;
  }
  if (num < m) m = num;
  return (int32_t)m;
}

// Item (row, a) of k_est_assumed. mode EA_CLASS: row k of the class rows, header of the
// class's representative rep[k] (row 0 and the rows without one are left alone);
// EA_RAW: row b of the per-binding rows, the raw answer (kp_max_available_replicas);
// EA_MERGED: row b of the pair kernel's rows, as pair_eval writes them: cal_merge on the
// binding's feasible clusters, 0 elsewhere, non-workload bindings left alone.
enum : int32_t { EA_CLASS = 0, EA_RAW = 1, EA_MERGED = 2 };
template <class Blk>
KP_HD inline void body_est_assumed(const Blk& b, const SnapView& s, const BatchView& bv, const AssumedView& A,
                                   int mode, const int32_t* rep, const uint64_t* fmask, int row0, int row, int a,
                                   int32_t* rows) {
  const int d = row0 + row;
  const int hb = mode == EA_CLASS ? (d == 0 ? -1 : rep[d]) : d;
  if (hb < 0) return;
  const BindHdr& h = bv.hdr[hb];
  if (mode == EA_MERGED && (h.flags & BF_NONWORKLOAD_EST)) return;
  const int c = A.rank[a];
  int32_t v = assumed_estimate(b, s, bv, h, A, a);
  if (mode == EA_MERGED) v = mask_test(fmask + (size_t)d * s.W, c) ? cal_merge(h, v) : 0;
  if (b.lane() == 0) rows[(size_t)d * s.Cp + c] = v;
}

}  // namespace kp
