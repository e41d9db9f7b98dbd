// assumed.cpp — kp_assumptions_* and kp_batch_create_assumed: the scheduler's assumed
// workloads (SchedulingOvercommitProtection; AssigningResourceBindingCache.GetAssumedWorkloads,
// pkg/scheduler/cache/cache.go:287, handed to the estimators by buildAssumedWorkloadsByCluster,
// core/estimation.go:115-139) deducted from a batch's GeneralEstimator answers. The host
// resolves names and quantities and groups the entries by cluster, keeping their order;
// k_assume_cluster (kp_assume.h) deducts once per cluster; an assumed batch's schedule calls
// correct their estimate rows with k_est_assumed (engine.cpp).
#include "kp_env.h"
#include "kp_host.h"

namespace {

struct Packed {
  std::vector<int32_t> rank, wl_off, comp_off, c_rep, c_rr, req_off;
  std::vector<AssumedReq> req;
  std::vector<int64_t> run_off;
};

// One component's ResourceRequest as AssumedReq entries (one per distinct name).
int pack_component(kp_engine* e, const kp_snapshot* s, const kp_component& c, uint64_t entry, uint32_t k, Packed* p) {
  const std::string at = "kp_assumptions_create: entry " + std::to_string(entry) + " component " + std::to_string(k);
  if (c.replicas < 0) {
    e->err = at + " has negative replicas";
    return KP_EINVAL;
  }
  p->c_rep.push_back(c.replicas);
  p->c_rr.push_back(c.has_replica_requirements ? 1 : 0);
  if (c.has_replica_requirements) {
    QtyMap rq;
    if (c.n_resource_request && !c.resource_request) {
      e->err = at + " has a null resource_request with n_resource_request > 0";
      return KP_EINVAL;
    }
    if (!qmap(c.resource_request, c.n_resource_request, &rq)) {
      e->err = at + " has an unparsable quantity";
      return KP_EINVAL;
    }
    for (auto& kv : rq) {
      const std::string& nm = kv.first;
      if (kv.second.nano < 0) {  // (the clamped availability columns cannot take a demand below zero)
        e->err = at + " requests a negative quantity of " + nm;
        return KP_ENOTSUP;
      }
      AssumedReq r;
      r.rid = s->res.get(nm);
      r.val = nm == "cpu" ? k8s::milli(kv.second) : k8s::value(kv.second);  // MilliValue for cpu, Value otherwise
      r.kind = nm == "pods" ? AQ_PODS
                            : (nm == "cpu" || nm == "memory" || nm == "ephemeral-storage" || k8s::scalar_resource(nm) ? AQ_NODE : 0);
      p->req.push_back(r);
    }
    if (p->req.size() > (size_t)INT32_MAX) {
      e->err = "kp_assumptions_create: more than 2^31 - 1 request entries";
      return KP_ENOTSUP;
    }
  }
  p->req_off.push_back((int32_t)p->req.size());
  return KP_OK;
}

}  // namespace

extern "C" {

int kp_assumptions_create(kp_engine* e, const kp_snapshot* s, const kp_assumed_entry* entries, uint64_t n,
                          kp_assumptions** out) {
  if (!e || !s || !out || (n && !entries)) return KP_EINVAL;
  // (the device arrays are indexed in 32 bits: workloads, 16 components each, and their request entries)
  constexpr uint64_t kMaxEntries = (uint64_t)INT32_MAX / (2 * kSetsComp);
  if (n > kMaxEntries) {
    e->err = "kp_assumptions_create: " + std::to_string(n) + " entries, more than " + std::to_string(kMaxEntries);
    return KP_ENOTSUP;
  }
  (void)dev::set_device(e->device);
  auto a = std::make_unique<kp_assumptions>();
  a->e = e;
  if (n == 0) {
    *out = a.release();
    return KP_OK;
  }
  // entries by cluster rank, each cluster's in the order given
  std::vector<std::vector<uint64_t>> by_rank((size_t)s->C);
  for (uint64_t i = 0; i < n; i++) {
    const kp_assumed_entry& en = entries[i];
    if (en.cluster >= (uint32_t)s->C) {
      e->err = "kp_assumptions_create: entry " + std::to_string(i) + " names cluster index " + std::to_string(en.cluster) +
               ", the snapshot has " + std::to_string(s->C) + " clusters";
      return KP_EINVAL;
    }
    if (en.n_components > (uint32_t)kSetsComp) {
      e->err = "kp_assumptions_create: entry " + std::to_string(i) + " has " + std::to_string(en.n_components) +
               " components, more than " + std::to_string(kSetsComp) + " in one workload";
      return KP_ENOTSUP;
    }
    if (en.n_components && !en.components) {
      e->err = "kp_assumptions_create: entry " + std::to_string(i) + " has null components with n_components > 0";
      return KP_EINVAL;
    }
    by_rank[(size_t)s->inv[en.cluster]].push_back(i);
  }
  // run scratch per cluster: min(model node count, capacity); KP_ASSUME_RUNS_CAP lowers it (tests)
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kSetsRunsMax, kp_env_int("KP_ASSUME_RUNS_CAP", kSetsRunsMax)));
  Packed p;
  p.wl_off.push_back(0);
  p.comp_off.push_back(0);
  p.req_off.push_back(0);
  p.run_off.push_back(0);
  for (int r = 0; r < s->C; r++) {
    if (by_rank[r].empty()) continue;
    p.rank.push_back(r);
    for (uint64_t i : by_rank[r]) {
      for (uint32_t k = 0; k < entries[i].n_components; k++)
        if (int rc = pack_component(e, s, entries[i].components[k], i, k, &p)) return rc;
      p.comp_off.push_back((int32_t)p.c_rep.size());
    }
    p.wl_off.push_back((int32_t)p.comp_off.size() - 1);
    int64_t nodes = 0;
    if (s->flags[r] & CF_MODEL_OK)
      for (int g = s->mgrp_off[r]; g < s->mgrp_off[r + 1]; g++) nodes = std::min<int64_t>(cap, nodes + s->mgrp_cnt[g]);
    p.run_off.push_back(p.run_off.back() + std::max<int64_t>(1, std::min(nodes, cap)));
  }
  const size_t A = p.rank.size(), R = s->res.names.size(), stride = R + 2;
  auto st = std::make_shared<AssumedState>();
  st->snap = s;
  st->epoch = s->epoch;
  st->updates = s->updates;
  st->dev.pool_dev = e->device;
  AssumedView& v = st->view;
  v.n = (int32_t)A;
  v.n_res = (int32_t)R;
  v.rid_pods = s->res.get("pods");
  Arena& d = st->dev;
  d.add(const_cast<int32_t**>(&v.rank), p.rank.data(), A);
  d.add(const_cast<int32_t**>(&v.wl_off), p.wl_off.data(), p.wl_off.size());
  d.add(const_cast<int32_t**>(&v.comp_off), p.comp_off.data(), p.comp_off.size());
  d.add(const_cast<int32_t**>(&v.c_rep), p.c_rep.data(), p.c_rep.size(), 1);
  d.add(const_cast<int32_t**>(&v.c_rr), p.c_rr.data(), p.c_rr.size(), 1);
  d.add(const_cast<int32_t**>(&v.req_off), p.req_off.data(), p.req_off.size());
  d.add(const_cast<AssumedReq**>(&v.req), p.req.data(), p.req.size(), 1);
  d.add(const_cast<int64_t**>(&v.run_off), p.run_off.data(), p.run_off.size());
  d.add(&v.pods, A);
  d.add(&v.sums, A * std::max<size_t>(R, 1));
  d.add(&v.runs, (size_t)p.run_off.back() * stride);
  d.add(&v.n_runs, A);
  d.add(&v.status, A);
  HIPCHK(d.alloc());
  std::vector<int32_t> status(A);
  int rc = d.upload(e->stream) || dev::assume_cluster(e->stream, s->view, v) ||
           dev::d2h(status.data(), v.status, 4 * A, e->stream);
  rc = dev::sync(e->stream) || rc;  // (the packed arrays and the arena outlive what was queued)
  if (rc) {
    e->err = std::string("kp_assumptions_create: ") + dev::last_error();
    return KP_EDEVICE;
  }
  for (size_t i = 0; i < A; i++) {
    if (status[i] == AS_OK) continue;
    const std::string who = "kp_assumptions_create: cluster " + s->names[p.rank[i]] + " (index " +
                            std::to_string(s->perm[p.rank[i]]) + ")";
    e->err = status[i] == AS_SUM_OVERFLOW
                 ? who + ": the assumed workloads' summed demand of a resource leaves int64"
                 : who + ": the model nodes left after the assumed workloads need more than " +
                       std::to_string(p.run_off[i + 1] - p.run_off[i]) + " node runs";
    return KP_ENOTSUP;
  }
  a->st = std::move(st);
  *out = a.release();
  return KP_OK;
}

void kp_assumptions_destroy(kp_assumptions* a) {
  if (!a) return;
  // (the batches made over it keep the state; the last holder returns it to the pool)
  delete a;
}

int kp_batch_create_assumed(kp_engine* e, const kp_snapshot* s, const kp_assumptions* a, const kp_binding* bindings,
                            uint64_t n, kp_batch** out) {
  if (!e || !s || !out) return KP_EINVAL;
  if (a && a->st) {
    const AssumedState& st = *a->st;
    if (st.snap != s || a->e != e) {
      e->err = "kp_batch_create_assumed: the assumptions were made over another engine or snapshot";
      return KP_ESTATE;
    }
    if (st.epoch != s->epoch || st.updates != s->updates) {
      e->err = "kp_batch_create_assumed: the snapshot was updated after kp_assumptions_create deducted from it";
      return KP_ESTATE;
    }
  }
  kp_batch* bt = nullptr;
  if (int rc = kp_batch_create(e, s, bindings, n, &bt)) return rc;
  if (a && a->st) {
    for (int b = 0; b < bt->B; b++)
      if (bt->hdr[b].flags & BF_SETS) {
        e->err = "kp_batch_create_assumed: binding " + std::to_string(b) +
                 " takes MaxAvailableComponentSets, which is not deducted (assumed workloads serve the "
                 "single-template path only)";
        kp_batch_destroy(bt);
        return KP_ENOTSUP;
      }
    bt->assumed = a->st;
  }
  *out = bt;
  return KP_OK;
}

}  // extern "C"
