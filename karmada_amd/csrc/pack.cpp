// pack.cpp — the binding packer and batch creation: kp_batch_create and its keyed, estimates
// and filters forms, kp_batch_digest, kp_batch_destroy and kp_pack_cache_*. The Packer, the
// worker threads it runs on, the per-binding routes, the cached records, and the stages of
// kp_batch_create. Defines valid_req (kp_host.h). The Packer compiles affinities through the
// SelectorCompiler it derives from (kp_selc.h, shared with watch.cpp).
//
// pack_parallel packs a batch in stages that share a PackCtx: prepare_cache, pack_chunks,
// unify_classes, merge_chunks, fill_cache, pick_representatives, and report_timing under
// KP_PACK_TIMING. Within pack_chunks a ChunkPacker (one per thread) takes each binding through
// look_ahead, then take_hit or pack_fresh, class_key and, for a keyed miss, make_record.
// shift_binding is the one routine that knows which fields are offsets into which pool;
// records and the chunk merge both rebase through it.
#include "kp_host.h"
#include "kp_selc.h"
#include "kp_pdq.h"
#include "kp_top.h"

// ============================================================================
// Binding packing
// ============================================================================
namespace {
// Diagnostic build (-DKP_PACK_PROF): cycles per section of Packer::pack, summed over
// the process and printed by pack_parallel under KP_PACK_TIMING.
#ifdef KP_PACK_PROF
#include <x86intrin.h>
std::atomic<uint64_t> g_pack_cyc[8];
#define KP_PACK_MARK_INIT uint64_t kp_c0 = __rdtsc()
#define KP_PACK_MARK(i)                                                  \
  do {                                                                   \
    const uint64_t kp_c1 = __rdtsc();                                    \
    g_pack_cyc[i].fetch_add(kp_c1 - kp_c0, std::memory_order_relaxed); \
    kp_c0 = kp_c1;                                                       \
  } while (0)
#else
#define KP_PACK_MARK_INIT
#define KP_PACK_MARK(i)
#endif
}  // namespace

namespace kp::host {

// labels.NewRequirement validation (labels/selector.go:150-230)
bool valid_req(std::string_view key, std::string_view op, const kp_str* v, uint32_t n) {
  bool ok = k8s::label_key(key);
  if (op == "In" || op == "NotIn") ok = ok && n > 0;
  else if (op == "=") ok = ok && n == 1;
  else if (op == "Exists" || op == "DoesNotExist") ok = ok && n == 0;
  else if (op == "Gt" || op == "Lt") {
    ok = ok && n == 1;
    for (uint32_t i = 0; i < n; i++) {
      int64_t x;
      if (!k8s::parse_int64(SV(v[i]), &x)) ok = false;
    }
  } else {
    ok = false;
  }
  for (uint32_t i = 0; i < n; i++)
    if (!k8s::label_value(SV(v[i]))) ok = false;
  return ok;
}

}  // namespace kp::host

namespace {

// (s, this packer's pools bt and the selector compiler come from SelectorCompiler, kp_selc.h)
struct Packer : SelectorCompiler {
  // per-packer caches: the last (apiVersion, kind) and its GVK id, parsed quantity
  // strings, and scratch lists reused across bindings (no per-binding allocation)
  std::string gvkey;
  SvMap<std::pair<bool, k8s::Qty>> qcache;
  SvMap<int32_t> gvk_cache;  // apiVersion + '\0' + kind -> GVK id
  SvMap<bool> scalar_cache;  // resource name -> IsScalarResourceName
  std::vector<int32_t> tmp_t, tmp_rk, tmp_sr, tmp_mr;
  std::vector<int64_t> tmp_sq, tmp_mq;
  std::vector<std::pair<std::string_view, k8s::Qty>> tmp_rq;
  std::vector<int32_t> tmp_filt, tmp_ovf, tmp_ov, tmp_ids, tmp_ev;
  std::vector<int64_t> tmp_ws;
  // ResourceRequest lists memoized by content (their names and quantity strings): a batch
  // repeats a few request specs, so most bindings skip the parse, sort and name lookups
  struct ReqMemo {
    bool bad;
    std::vector<int32_t> sr, mr;
    std::vector<int64_t> sq, mq;
  };
  SvMap<int32_t> rmemo;
  std::vector<ReqMemo> rlist;
  std::string rkey;

  bool scalar(std::string_view nm) {
    auto it = scalar_cache.find(nm);
    if (it != scalar_cache.end()) return it->second;
    const bool v = k8s::scalar_resource(std::string(nm));
    if (scalar_cache.size() < 4096) scalar_cache.emplace(std::string(nm), v);
    return v;
  }

  bool qty(std::string_view str, k8s::Qty* q) {
    auto it = qcache.find(str);
    if (it != qcache.end()) {
      *q = it->second.second;
      return it->second.first;
    }
    k8s::Qty v;
    const bool ok = k8s::parse_quantity(str, &v);
    if (qcache.size() < 4096) qcache.emplace(std::string(str), std::make_pair(ok, v));
    *q = v;
    return ok;
  }

  void pack(const kp_binding& b, BindHdr& h) {
    KP_PACK_MARK_INIT;
    memset(&h, 0, sizeof(h));
    h.ip_beg = (int32_t)bt->ipool.size();
    h.pr_beg = (int32_t)bt->progs.size();
    h.in_beg = (int32_t)bt->instrs.size();
    const kp_options& o = s->opts;
    h.replicas = b.replicas;
    h.enabled = (int32_t)o.enabled_plugins;
    uint32_t f = 0;
    if (b.has_replica_requirements) f |= BF_HAS_RR;
    if (b.replicas == 0 && b.n_components == 0) f |= BF_NONWORKLOAD_EST;
    if ((b.replicas > 0 || b.has_replica_requirements) && b.n_components <= 1) f |= BF_WORKLOAD_ASSIGN;
    if (b.has_reschedule_triggered_at && b.has_last_scheduled_time &&
        b.reschedule_triggered_at_ns > b.last_scheduled_time_ns)
      f |= BF_FRESH;
    if (b.uid.len && (k8s::fnv32a(b.uid.ptr, b.uid.len) & 1)) f |= BF_UID_DESC;
    if (o.enable_empty_workload_propagation) f |= BF_EMPTY_PROP;
    if (b.has_weight_preference) f |= BF_HAS_WP;
    // APIEnablement GVK (group_version.go:211-226,300-305)
    {
      gvkey.assign(SV(b.api_version));
      gvkey.push_back('\0');
      gvkey.append(SV(b.kind));
      auto it = gvk_cache.find(std::string_view(gvkey));
      if (it != gvk_cache.end()) {
        h.gvk = it->second;  // (a batch repeats a few kinds)
      } else {
        std::string av = S(b.api_version), g, ver;
        size_t slashes = std::count(av.begin(), av.end(), '/');
        if (!(av.empty() || av == "/")) {
          if (slashes == 0) ver = av;
          else if (slashes == 1) {
            g = av.substr(0, av.find('/'));
            ver = av.substr(av.find('/') + 1);
          }
        }
        std::string gv = g.empty() ? ver : g + "/" + ver;
        h.gvk = s->gvk.get(gv + '\0' + S(b.kind));
        if (gvk_cache.size() < 4096) gvk_cache.emplace(gvkey, h.gvk);
      }
    }
    KP_PACK_MARK(0);
    // spec.Clusters
    h.n_targets_all = (int32_t)b.n_clusters;
    {
      std::vector<int32_t>& t = tmp_t;
      std::vector<int32_t>& rk = tmp_rk;
      t.clear();
      rk.clear();
      for (uint32_t i = 0; i < b.n_clusters; i++) {
        auto it = s->rank_of.find(SV(b.clusters[i].name));
        if (it == s->rank_of.end()) continue;
        rk.push_back(it->second);
        t.push_back(it->second);
        t.push_back(b.clusters[i].replicas);
      }
      std::sort(rk.begin(), rk.end());
      if (std::adjacent_find(rk.begin(), rk.end()) != rk.end()) f |= BF_DUP_TARGETS;
      h.tgt_off = list(t);
      h.tgt_cnt = (int32_t)t.size() / 2;
      if (b.n_clusters > 0 && (o.enabled_plugins & KP_PLUGIN_CLUSTER_LOCALITY)) f |= BF_SCORE_LOCALITY;
    }
    {
      auto& r = tmp_ev;
      r.clear();
      for (uint32_t i = 0; i < b.n_eviction_from; i++) {
        auto it = s->rank_of.find(SV(b.eviction_from[i]));
        if (it != s->rank_of.end()) r.push_back(it->second);
      }
      h.evict_off = list(r);
      h.evict_cnt = (int32_t)r.size();
    }
    KP_PACK_MARK(1);
    // tolerations
    h.tol_off = (int32_t)bt->tols.size();
    for (uint32_t i = 0; i < b.n_tolerations; i++) {
      const kp_toleration& t = b.tolerations[i];
      const std::string_view eff = SV(t.effect), key = SV(t.key), op = SV(t.op);
      Tol x;
      if (eff.empty()) x.eff = EFF_ANY;
      else if (eff == "NoSchedule") x.eff = EFF_NOSCHEDULE;
      else if (eff == "NoExecute") x.eff = EFF_NOEXECUTE;
      else continue;
      if (key.empty()) x.key = -1;
      else if ((x.key = s->str.get(key)) < 0) continue;
      if (op.empty() || op == "Equal") {
        x.op = TOL_EQUAL;
        if ((x.val = s->str.get(SV(t.value))) < 0) continue;
      } else if (op == "Exists") {
        x.op = TOL_EXISTS;
        x.val = -1;
      } else {
        continue;  // Lt/Gt disabled, unknown operators never tolerate
      }
      bt->tols.push_back(x);
    }
    h.tol_cnt = (int32_t)bt->tols.size() - h.tol_off;
    KP_PACK_MARK(2);
    // ClusterAffinity filter list + overflow order programs
    {
      auto &filt = tmp_filt, &ovf = tmp_ovf;
      filt.clear();
      ovf.clear();
      bool have = false;
      const kp_affinity_term* term = nullptr;
      if (b.has_cluster_affinity) {
        filt.push_back(compile(b.cluster_affinity));
        have = true;
      } else {
        const std::string_view obs = SV(b.observed_affinity_name);
        for (uint32_t i = 0; i < b.n_cluster_affinities; i++)
          if (SV(b.cluster_affinities[i].affinity_name) == obs) {
            term = &b.cluster_affinities[i];
            break;
          }
        if (term) {
          have = true;
          ovf.push_back(compile(term->affinity));
          filt.push_back(ovf[0]);
          auto& ov = tmp_ov;
          ov.clear();
          for (uint32_t j = 0; j < term->n_overflow; j++) ov.push_back(compile(term->overflow[j]));
          ovf.insert(ovf.end(), ov.begin(), ov.end());
          bool workload = b.replicas > 0 || b.has_replica_requirements || b.n_components >= 1;
          if (workload) filt.insert(filt.end(), ov.begin(), ov.end());
        }
      }
      if (!have) f |= BF_AFF_ALL;
      h.filt_off = list(filt);
      h.filt_cnt = (int32_t)filt.size();
      if (b.has_cluster_affinity || b.n_cluster_affinities == 0) h.ovf_mode = OVF_ZERO;
      else if (!term) h.ovf_mode = OVF_1000;
      else h.ovf_mode = OVF_PROGS;
      h.ovf_off = list(ovf);
      h.ovf_cnt = (int32_t)ovf.size();
      // engine limit: the sortClusters key orders kMaxOvfTerms overflow orders (kp_algo.h)
      // (reported as KP_ERR_OVERFLOW_TERMS, not as a malformed request)
      if (h.ovf_mode == OVF_PROGS && h.ovf_cnt > kMaxOvfTerms) f |= BF_BAD | BF_LIMIT_OVF;
      // enableOverflow (common.go:156-170)
      if (!b.has_cluster_affinity && b.n_cluster_affinities > 0 && b.observed_affinity_name.len > 0 && term &&
          term->n_overflow > 0)
        f |= BF_OVERFLOW;
    }
    KP_PACK_MARK(3);
    // static weights
    {
      auto& ids = tmp_ids;
      auto& ws = tmp_ws;
      ids.clear();
      ws.clear();
      for (uint32_t i = 0; i < b.n_static_weights; i++) {
        ids.push_back(compile(b.static_weights[i].target));
        ws.push_back(b.static_weights[i].weight);
      }
      h.sw_off = list(ids);
      h.sw_cnt = (int32_t)ids.size();
      h.sw_w_off = (int32_t)bt->lpool.size();
      bt->lpool.insert(bt->lpool.end(), ws.begin(), ws.end());
    }
    KP_PACK_MARK(4);
    // requests
    rkey.clear();
    for (uint32_t i = 0; i < b.n_resource_request; i++) {
      rkey.append(SV(b.resource_request[i].name));
      rkey.push_back('\0');
      rkey.append(SV(b.resource_request[i].quantity));
      rkey.push_back('\0');
    }
    if (auto* m = rmemo.find(std::string_view(rkey))) {
      const ReqMemo& q = rlist[m->second];
      if (q.bad) f |= BF_BAD;
      h.sreq_off = list(q.sr);
      h.sreq_cnt = (int32_t)q.sr.size();
      h.sreq_q_off = (int32_t)bt->lpool.size();
      bt->lpool.insert(bt->lpool.end(), q.sq.begin(), q.sq.end());
      h.mreq_off = list(q.mr);
      h.mreq_cnt = (int32_t)q.mr.size();
      h.mreq_q_off = (int32_t)bt->lpool.size();
      bt->lpool.insert(bt->lpool.end(), q.mq.begin(), q.mq.end());
    } else {
      bool bad = false;
      // the ResourceList as (name, quantity) in name order, a repeated name's last
      // entry winning (the map the reference decodes), without per-entry allocation
      auto& rq = tmp_rq;
      rq.clear();
      for (uint32_t i = 0; i < b.n_resource_request; i++) {
        k8s::Qty q;
        if (!qty(SV(b.resource_request[i].quantity), &q)) bad = true;
        const std::string_view nm = SV(b.resource_request[i].name);
        bool dup = false;
        for (auto& kv : rq)
          if (kv.first == nm) {
            kv.second = q;
            dup = true;
          }
        if (!dup) rq.push_back({nm, q});
      }
      std::sort(rq.begin(), rq.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
      auto &sr = tmp_sr, &mr = tmp_mr;
      auto &sq = tmp_sq, &mq = tmp_mq;
      sr.clear(), mr.clear(), sq.clear(), mq.clear();
      for (auto& kv : rq) {
        const std::string_view nm = kv.first;
        const bool cpu = nm == "cpu", mem = nm == "memory";
        const int32_t rid = cpu ? s->rid_cpu : (mem ? s->rid_mem : s->res.get(nm));
        int64_t v = k8s::value(kv.second);
        if (v > 0) {  // summary path: every resource name (general.go:467-471)
          sr.push_back(rid);
          sq.push_back(cpu ? k8s::milli(kv.second) : v);
        }
        // model path: util.NewResource classes (resource.go:46-75)
        if (cpu) {
          int64_t m = k8s::milli(kv.second);
          if (m > 0) {
            mr.push_back(rid);
            mq.push_back(m);
          }
        } else if (mem || nm == "ephemeral-storage" || (nm != "pods" && scalar(nm))) {
          if (v > 0) {
            mr.push_back(rid);
            mq.push_back(v);
          }
        }
      }
      h.sreq_off = list(sr);
      h.sreq_cnt = (int32_t)sr.size();
      h.sreq_q_off = (int32_t)bt->lpool.size();
      bt->lpool.insert(bt->lpool.end(), sq.begin(), sq.end());
      h.mreq_off = list(mr);
      h.mreq_cnt = (int32_t)mr.size();
      h.mreq_q_off = (int32_t)bt->lpool.size();
      bt->lpool.insert(bt->lpool.end(), mq.begin(), mq.end());
      if (bad) f |= BF_BAD;
      if (rlist.size() < 4096) {
        rmemo.emplace(rkey, (int32_t)rlist.size());
        rlist.push_back(ReqMemo{bad, sr, mr, sq, mq});
      }
    }
    KP_PACK_MARK(5);
    // spread constraints: filter presence + selection kind (select_clusters.go:28-80)
    const std::string_view rst = b.has_replica_scheduling ? SV(b.replica_scheduling_type) : std::string_view("Duplicated");
    const std::string_view div = SV(b.replica_division_preference);
    bool hasRegion = false, hasCluster = false;
    int n_order = 0;
    for (uint32_t i = 0; i < b.n_spread_constraints; i++) {
      const kp_spread_constraint& sc = b.spread_constraints[i];
      const std::string_view fld = SV(sc.spread_by_field);
      const int code = fld == "provider" ? 1 : fld == "region" ? 2 : fld == "zone" ? 3 : 0;
      bool seen = false;
      for (int k = 0; k < n_order; k++) seen = seen || ((h.spread_order >> (2 * k)) & 3) == code;
      if (code && !seen) h.spread_order |= code << (2 * n_order++);
      if (fld == "provider") f |= BF_NEED_PROVIDER;
      if (fld == "region") {
        f |= BF_NEED_REGION;
        hasRegion = true;
        h.region_min = sc.min_groups;
        h.region_max = sc.max_groups;
      }
      if (fld == "zone") f |= BF_NEED_ZONES;
      if (fld == "cluster") {
        hasCluster = true;
        h.cluster_min = sc.min_groups;
        h.cluster_max = sc.max_groups;
      }
    }
    bool ignoreSpread = b.has_replica_scheduling && SV(b.replica_scheduling_type) == "Divided" && div == "Weighted" &&
                        (!b.has_weight_preference || (b.n_static_weights != 0 && b.dynamic_weight.len == 0));
    if (b.n_spread_constraints == 0 || ignoreSpread) h.sel = SEL_ALL;
    else if (hasRegion) h.sel = SEL_REGION;
    else if (hasCluster) h.sel = SEL_CLUSTER;
    else h.sel = SEL_ERR_UNSUPPORTED;
    h.need_replicas = (!b.has_replica_scheduling || SV(b.replica_scheduling_type) == "Duplicated") ? -1 : b.replicas;
    // runReplicaEstimator / SelectClusters with the MultiplePodTemplatesScheduling gate:
    // isMultiTemplateSchedulingApplicable (core/estimation.go:43-65) = components and a
    // cluster spread constraint with MinGroups == MaxGroups == 1. Such a binding's
    // estimator row is MaxAvailableComponentSets (core/util.go:113-118) and it needs one
    // available replica (one set) in SelectBestClusters (common.go:42-46).
    if (o.multiple_pod_templates_scheduling && b.n_components > 0) {
      bool one = false;
      for (uint32_t i = 0; i < b.n_spread_constraints; i++)
        one = one || (SV(b.spread_constraints[i].spread_by_field) == "cluster" &&
                      b.spread_constraints[i].min_groups == 1 && b.spread_constraints[i].max_groups == 1);
      if (one) {
        f |= BF_SETS;
        if (h.need_replicas != -1) h.need_replicas = 1;
      }
    }
    if (rst == "Duplicated") f |= BF_GROUP_DUP;
    // strategy (assignment.go:95-123)
    if (rst == "Duplicated") h.strategy = ST_DUPLICATED;
    else if (rst == "Divided") {
      if (div == "Aggregated") h.strategy = ST_AGGREGATED;
      else if (div == "Weighted")
        h.strategy = (b.has_weight_preference && b.dynamic_weight.len) ? ST_DYNAMIC : ST_STATIC;
      else h.strategy = ST_NONE;
    } else {
      h.strategy = ST_NONE;
    }
    h.flags = f;
    uint64_t C = (uint64_t)s->C;
    bool big = !(f & BF_WORKLOAD_ASSIGN) || h.strategy == ST_DUPLICATED || (f & BF_EMPTY_PROP);
    uint64_t rep = b.replicas > 0 ? (uint64_t)b.replicas : 0;
    h.out_cap = (big ? C : std::min<uint64_t>(C, rep)) + (uint64_t)h.tgt_cnt;
    h.ip_end = (int32_t)bt->ipool.size();
    h.pr_end = (int32_t)bt->progs.size();
    h.in_end = (int32_t)bt->instrs.size();
    KP_PACK_MARK(6);
  }
};

// Hardware threads, capped by the cgroup v2 CPU quota (cpu.max "quota period") when set.
int host_cpus() {
  int n = (int)std::max(1u, std::thread::hardware_concurrency());
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
      const long long quota = atoll(q);
      n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
    }
    fclose(f);
  }
  return n;
}

// Process-wide worker threads for the packer's per-thread phases (pack, merge, cache
// inserts): each phase of each batch used to start and join its own threads (three rounds
// of 16 per batch with kp_pack_cache), and two engines packing at once started 32 at a time.
// run(T, fn) calls fn(t) once for every t in [0, T), the caller taking tasks too; jobs of
// concurrent callers interleave task by task. Workers are started lazily, never joined.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool* p = new HostPool();  // (never destroyed: workers may be blocked in wait)
    return *p;
  }
  void run(int T, const std::function<void(int)>& fn) {
    if (T <= 1) {
      if (T == 1) fn(0);
      return;
    }
    ensure(T - 1);
    Job j;
    j.fn = &fn;
    j.T = T;
    j.left = T;
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_back(&j);
    }
    cv_.notify_all();
    for (;;) {  // the caller takes tasks of its own job until none is left to start
      int t;
      {
        std::lock_guard<std::mutex> g(mu_);
        if (j.next >= j.T) break;
        t = j.next++;
        if (j.next >= j.T) q_.erase(std::find(q_.begin(), q_.end(), &j));
      }
      fn(t);
      std::lock_guard<std::mutex> g(mu_);
      j.left--;
    }
    std::unique_lock<std::mutex> g(mu_);
    done_.wait(g, [&] { return j.left == 0; });
  }

 private:
  struct Job {
    const std::function<void(int)>* fn = nullptr;
    int T = 0, next = 0, left = 0;
  };
  std::mutex mu_;
  std::condition_variable cv_, done_;
  std::vector<Job*> q_;
  int n_workers_ = 0;
  void ensure(int n) {
    std::lock_guard<std::mutex> g(mu_);
    for (; n_workers_ < n; n_workers_++) std::thread([this] { loop(); }).detach();
  }
  void loop() {
    std::unique_lock<std::mutex> g(mu_);
    for (;;) {
      cv_.wait(g, [&] { return !q_.empty(); });
      Job* j = q_.front();
      const int t = j->next++;
      if (j->next >= j->T) q_.erase(q_.begin());
      g.unlock();
      (*j->fn)(t);
      g.lock();
      if (--j->left == 0) done_.notify_all();
    }
  }
};

// Whether the specialised pair kernel (est_compute<true>) covers every binding of
// the batch: MaxDivided and taint-set tables fit in LDS, the dense node-count
// matrix exists (or no cluster has models), at most kReqUnroll resource requests
// per binding, divisors <= 2^60.
// The snapshot half (its clusters' estimator paths and table sizes), kept in
// kp_snapshot::est_kind and refreshed by every upload; the batch half
// (request counts and divisors) in kp_batch::fast_ok. The launch takes
// est_kind when fast_ok, else EST_GENERIC.
bool batch_fast_ok(const kp_batch* bt) {
  for (const BindHdr& h : bt->hdr) {
    if (h.sreq_cnt > kReqUnroll) return false;
    for (int j = 0; j < h.sreq_cnt; j++)
      if (bt->lpool[h.sreq_q_off + j] > ((int64_t)1 << 60)) return false;
  }
  return true;
}

// Estimator class key of a packed binding: everything the GeneralEstimator reads
// from it (est_load / est_compute_bf / template_md, kp_algo.h): whether it has
// ReplicaRequirements and its summary and model requests (resource id, divisor).
void est_key(const BindHdr& h, const Pools& p, std::string* k) {
  k->clear();
  auto put = [&](const void* v, size_t n) { k->append((const char*)v, n); };
  const uint32_t rr = h.flags & BF_HAS_RR;
  put(&rr, 4);
  put(&h.sreq_cnt, 4);
  for (int j = 0; j < h.sreq_cnt; j++) {
    put(&p.ipool[h.sreq_off + j], 4);
    put(&p.lpool[h.sreq_q_off + j], 8);
  }
  put(&h.mreq_cnt, 4);
  for (int j = 0; j < h.mreq_cnt; j++) {
    put(&p.ipool[h.mreq_off + j], 4);
    put(&p.lpool[h.mreq_q_off + j], 8);
  }
}

// A binding's route through kp_schedule_batch, recorded while packing so that the
// batch's lists come from one pass over n bytes instead of passes over the headers.
enum : uint8_t { RT_CLUSTER = 1, RT_REGION = 2, RT_DYN = 4, RT_SMALL = 8, RT_STATIC_OK = 16 };
KP_HD inline bool route_static_ok(const SnapView& v, const BindHdr& h, const int64_t* lpool) {
  if (h.sel != SEL_ALL || h.strategy != ST_STATIC || h.replicas < 0 || (int64_t)h.replicas >= kSeatWrap) return false;
  if (!(h.flags & BF_WORKLOAD_ASSIGN) || (h.flags & (BF_OVERFLOW | BF_DUP_TARGETS | BF_BAD))) return false;
  if (v.C >= 65536) return false;  // packed class counts
  if (h.flags & BF_HAS_WP) {
    if (h.sw_cnt > kSwRules || v.n_bits <= 0) return false;
    for (int j = 0; j < h.sw_cnt; j++)
      if (lpool[h.sw_w_off + j] >= (int64_t)kInt32Max) return false;  // saturated votes: SLOW_WEIGHT
  }
  return true;
}
// Replicas + len(spec.Clusters) up to which a binding takes k_select_top's small slice
// (KP_TOP_SMALL_NEED overrides kTopSmallNeed, for measurement).
inline int64_t top_small_need() {
  static const int64_t v = std::max<int64_t>(0, kp_env_int("KP_TOP_SMALL_NEED", kTopSmallNeed));
  return v;
}
inline uint8_t route_of(const SnapView& v, const BindHdr& h, const int64_t* lpool) {
  uint8_t r = h.sel == SEL_CLUSTER ? RT_CLUSTER : h.sel == SEL_REGION ? RT_REGION : 0;
  if (!r) {
    if (h.strategy != ST_STATIC) r |= RT_DYN;
    if ((int64_t)h.replicas + h.tgt_cnt <= top_small_need()) r |= RT_SMALL;
    if (route_static_ok(v, h, lpool)) r |= RT_STATIC_OK;
  }
  return r;
}

// Packing reads each binding's struct and the strings and arrays it points to once,
// scattered over the caller's memory: cache misses, not the parsing, bound it (about
// 3k cycles per config-3 binding, spread evenly over the struct's sections). So the
// loop prefetches three levels ahead of the binding it packs: the struct of i + 3,
// the arrays and strings i + 2 points to, the strings inside i + 1's arrays.
inline void pf(const void* p) {
  if (p) __builtin_prefetch(p, 0, 3);
}
inline void pf_struct(const kp_binding* b) {
  for (size_t o = 0; o < sizeof(kp_binding); o += 64) pf((const char*)b + o);
}
inline void pf_affinity(const kp_cluster_affinity& a) {
  pf(a.match_labels);
  pf(a.match_expressions);
  pf(a.field_expressions);
  pf(a.cluster_names);
  pf(a.exclude_clusters);
}
inline void pf_arrays(const kp_binding& b) {
  pf(b.uid.ptr);
  pf(b.api_version.ptr);
  pf(b.kind.ptr);
  pf(b.resource_request);
  pf(b.clusters);
  pf(b.eviction_from);
  pf(b.tolerations);
  pf(b.spread_constraints);
  pf(b.static_weights);
  pf(b.cluster_affinities);
  if (b.has_cluster_affinity) pf_affinity(b.cluster_affinity);
}
inline void pf_strings(const kp_binding& b) {
  for (uint32_t j = 0; j < b.n_resource_request && j < 4; j++) {
    pf(b.resource_request[j].name.ptr);
    pf(b.resource_request[j].quantity.ptr);
  }
  for (uint32_t j = 0; j < b.n_clusters && j < 4; j++) pf(b.clusters[j].name.ptr);
  for (uint32_t j = 0; j < b.n_tolerations && j < 2; j++) {
    pf(b.tolerations[j].key.ptr);
    pf(b.tolerations[j].value.ptr);
  }
  if (b.has_cluster_affinity)
    for (uint32_t j = 0; j < b.cluster_affinity.n_match_expressions && j < 2; j++) {
      pf(b.cluster_affinity.match_expressions[j].key.ptr);
      pf(b.cluster_affinity.match_expressions[j].values);
    }
}

// The pool-reference map, the one copy of it beside Packer::pack, which writes the
// references: shifts a packed binding's references by (di, dl, dt, dp, dn) (ipool, lpool,
// tols, progs, instrs). Its header, the program ids in its ipool lists, its programs'
// instruction offsets and its instructions' list offsets. ip, pr and in point at the
// binding's own slices [ip_beg, ip_end), [pr_beg, pr_end) and [in_beg, in_end), wherever they
// lie (a chunk's pools, a record), located before the shift. A cached record's hit, a new
// record and the chunk merge all rebase through here.
inline void shift_binding(BindHdr& h, int32_t* ip, Prog* pr, Instr* in, int32_t di, int32_t dl, int32_t dt,
                          int32_t dp, int32_t dn) {
  const int n_pr = h.pr_end - h.pr_beg, n_in = h.in_end - h.in_beg;
  for (int j = 0; j < h.filt_cnt; j++) ip[h.filt_off - h.ip_beg + j] += dp;
  for (int j = 0; j < h.ovf_cnt; j++) ip[h.ovf_off - h.ip_beg + j] += dp;
  for (int j = 0; j < h.sw_cnt; j++) ip[h.sw_off - h.ip_beg + j] += dp;
  h.tgt_off += di, h.evict_off += di, h.filt_off += di, h.ovf_off += di, h.sw_off += di;
  h.sreq_off += di, h.mreq_off += di, h.ip_beg += di, h.ip_end += di;
  h.sw_w_off += dl, h.sreq_q_off += dl, h.mreq_q_off += dl;
  h.tol_off += dt;
  h.pr_beg += dp, h.pr_end += dp;
  h.in_beg += dn, h.in_end += dn;
  for (int j = 0; j < n_pr; j++) pr[j].ins_off += dn;
  for (int j = 0; j < n_in; j++) {
    Instr& x = in[j];
    if (Packer::list_ref_a(x.op)) x.a += di;
    else if (Packer::list_ref_b(x.op)) x.b += di;
  }
}

// One binding's packed record (kp_pack_cache), one allocation: this struct (the header
// with every pool reference relative to the record's own slices, the key and the status
// fields it was packed with), then its slices (lpool, instrs, tols, progs, ipool) and the
// uid, observed-affinity-name and estimator-class-key bytes.
struct PackRec {
  uint64_t key;
  int64_t gen, rt_ns, lst_ns;
  uint8_t has_rt, has_lst, nonworkload;  // nonworkload: bcls -1 (the estimator skipped)
  int32_t n_ip, n_lp, n_tol, n_pr, n_in;
  uint32_t uid_len, aff_len, cls_len;
  BindHdr h;
  unsigned char* tail() const { return (unsigned char*)(this + 1); }
  int64_t* lp() const { return (int64_t*)tail(); }
  Instr* in() const { return (Instr*)(lp() + n_lp); }
  Tol* tol() const { return (Tol*)(in() + n_in); }
  Prog* pr() const { return (Prog*)(tol() + n_tol); }
  int32_t* ip() const { return (int32_t*)(pr() + n_pr); }
  const char* uid() const { return (const char*)(ip() + n_ip); }
  const char* aff() const { return uid() + uid_len; }
  const char* cls() const { return aff() + aff_len; }
  static PackRec* make(int n_ip, int n_lp, int n_tol, int n_pr, int n_in, size_t n_str) {
    const size_t bytes = sizeof(PackRec) + 8 * (size_t)n_lp + sizeof(Instr) * (size_t)n_in +
                         sizeof(Tol) * (size_t)n_tol + sizeof(Prog) * (size_t)n_pr + 4 * (size_t)n_ip + n_str;
    auto* r = (PackRec*)::operator new(bytes, std::align_val_t(alignof(PackRec)));
    r->n_ip = n_ip, r->n_lp = n_lp, r->n_tol = n_tol, r->n_pr = n_pr, r->n_in = n_in;
    return r;
  }
  static void free(PackRec* r) { ::operator delete((void*)r, std::align_val_t(alignof(PackRec))); }
  bool same(const kp_binding_key& k, const kp_binding& b) const {
    return gen == k.generation && uid_len == k.uid.len && memcmp(uid(), k.uid.ptr, uid_len) == 0 &&
           has_rt == b.has_reschedule_triggered_at && has_lst == b.has_last_scheduled_time &&
           (!has_rt || rt_ns == b.reschedule_triggered_at_ns) && (!has_lst || lst_ns == b.last_scheduled_time_ns) &&
           std::string_view(aff(), aff_len) == SV(b.observed_affinity_name);
  }
};

// The records by key hash: kCacheShards open-addressed tables (linear probing, load <= 1/2;
// each slot holds the key beside the pointer, so a probe touches the table only), read-only
// while the packing threads look records up, filled shard by shard after.
constexpr int kCacheShards = 64;
struct PackTable {
  struct Slot {
    uint64_t key;  // 0: empty
    PackRec* r;
  };
  std::vector<Slot> slot;
  uint64_t n = 0;
  static size_t home(uint64_t key, size_t cap) { return (size_t)((key >> 6) * 0x9e3779b97f4a7c15ull >> 20) & (cap - 1); }
  const Slot* home_slot(uint64_t key) const { return slot.empty() ? nullptr : &slot[home(key, slot.size())]; }
  const PackRec* find(uint64_t key) const {
    if (slot.empty()) return nullptr;
    const size_t cap = slot.size();
    for (size_t i = home(key, cap);; i = (i + 1) & (cap - 1)) {
      if (slot[i].key == key) return slot[i].r;
      if (!slot[i].key) return nullptr;
    }
  }
  void put(PackRec* r) {  // (replaces a record of the same key)
    if (2 * (n + 1) > slot.size()) {
      std::vector<Slot> old(std::max<size_t>(64, 2 * slot.size()), Slot{0, nullptr});
      old.swap(slot);
      n = 0;
      for (const Slot& x : old)
        if (x.key) put(x.r);
    }
    const size_t cap = slot.size();
    for (size_t i = home(r->key, cap);; i = (i + 1) & (cap - 1)) {
      if (!slot[i].key) {
        slot[i] = Slot{r->key, r};
        n++;
        return;
      }
      if (slot[i].key == r->key) {
        PackRec::free(slot[i].r);
        slot[i].r = r;
        return;
      }
    }
  }
  void clear() {
    for (Slot& x : slot)
      if (x.key) PackRec::free(x.r), x = Slot{0, nullptr};
    n = 0;
  }
  ~PackTable() { clear(); }
};
}  // namespace

struct kp_pack_cache {
  uint64_t epoch = 0;  // the snapshot epoch the records resolved against (0: none yet)
  uint64_t max_entries = (uint64_t)4 << 20;
  uint64_t hits = 0, misses = 0, last_hits = 0;
  PackTable shard[kCacheShards];
  uint64_t entries() const {
    uint64_t e = 0;
    for (const auto& t : shard) e += t.n;
    return e;
  }
  void clear() {
    for (auto& t : shard) t.clear();
  }
};

namespace {
inline uint64_t cache_key(const kp_binding_key& k) {
  uint64_t h = 1469598103934665603ull;  // FNV-1a over the uid bytes, then the generation
  for (uint32_t i = 0; i < k.uid.len; i++) h = (h ^ (uint8_t)k.uid.ptr[i]) * 1099511628211ull;
  h ^= (uint64_t)k.generation * 0x9e3779b97f4a7c15ull;
  h ^= h >> 29;
  return h ? h : 1;
}

// pack_parallel packs bindings [0, n) into bt->hdr and bt's pools on T host threads. Chunks of
// kPackChunk bindings are taken from a shared counter (a thread that meets heavy bindings
// takes fewer chunks); each chunk packs into its own Pools (the Packer only reads the
// snapshot's dictionaries), then the chunks are concatenated in chunk order and every pool
// reference is rebased (shift_binding). The result equals a sequential pack (test_abi).
// Threads: KP_PACK_THREADS, else the CPUs this process may use (hardware threads, capped by a
// cgroup CPU quota), one per 4096 bindings at most. Packer caches and class-id maps are per
// thread. PackCtx is what the stages share.
constexpr int kPackChunk = 1024;
using PackClock = std::chrono::steady_clock;

struct PackCtx {
  kp_snapshot* s;
  const kp_binding* bindings;
  const int n;
  kp_batch* bt;
  const kp_binding_key* keys;
  kp_pack_cache* cache;
  // (kp_estimates, or null) each binding's row of the other estimators' answers; a workload
  // binding's estimator class is then (request key, row), the row appended to the class key
  // after the record lookup, so a cached record keeps the request key alone
  const int32_t* row_of;
  const int T, K;
  std::vector<int> lo, owner;       // chunk k: bindings [lo[k], lo[k + 1]), and the thread that packed it
  std::vector<Pools> pl;            // per chunk: its own pools,
  std::vector<size_t> bi, bl, bo, bp, bn;  // where each of the five goes in the batch's (merge_chunks),
  std::vector<uint64_t> chunk_cap;  // and its result slots at [k + 1], prefix-summed for out_off
  // per thread: the estimator class keys by thread-local id (bt->bcls holds those until the
  // merge) and their global ids, the first error, the headers' maxima and the cache hits
  // (each written once per chunk: adjacent slots share a line)
  std::vector<std::vector<std::string>> tkeys;
  std::vector<std::vector<int32_t>> remaps;
  std::vector<std::string> terr;
  std::vector<int> tmax_tgt, tmax_tiers;
  std::vector<uint64_t> thits;
  // kp_pack_cache: the new records per (chunk, shard), put into the shards after the merge
  std::vector<std::vector<PackRec*>> newrecs;
  // KP_PACK_TIMING: each thread's packing time and start; the pack stage's begin and end
  std::vector<double> tms, tstart;
  PackClock::time_point tpack0 = PackClock::now(), tq0, tq1;

  PackCtx(kp_snapshot* s_, const kp_binding* bindings_, int n_, kp_batch* bt_, const kp_binding_key* keys_,
          kp_pack_cache* cache_, const int32_t* row_of_, int T_)
      : s(s_), bindings(bindings_), n(n_), bt(bt_), keys(keys_), cache(cache_), row_of(row_of_), T(T_),
        K(std::max(1, (n_ + kPackChunk - 1) / kPackChunk)), lo(K + 1), owner(K, 0), pl(K), bi(K + 1, 0),
        bl(K + 1, 0), bo(K + 1, 0), bp(K + 1, 0), bn(K + 1, 0), chunk_cap(K + 1, 0), tkeys(T), remaps(T), terr(T), tmax_tgt(T, 0), tmax_tiers(T, 1), thits(T, 0),
        tms(T, 0.0), tstart(T, 0.0) {
    for (int k = 0; k <= K; k++) lo[k] = std::min(n, k * kPackChunk);
  }
  ~PackCtx() {  // records not handed to the cache (a failed batch) are freed
    for (auto& x : newrecs)
      for (PackRec* r : x)
        if (r) PackRec::free(r);
  }
  template <class F>
  void on_threads(F fn) {
    HostPool::get().run(T, std::function<void(int)>(fn));
  }
};

// Stage 1: records of another snapshot epoch, or past the size cap, are dropped before any
// lookup.
void prepare_cache(PackCtx& c) {
  kp_pack_cache* cache = c.cache;
  if (!cache) return;
  if (cache->epoch != c.s->epoch || cache->entries() > cache->max_entries) {
    cache->clear();
    cache->epoch = c.s->epoch;
  }
  c.newrecs.resize((size_t)c.K * kCacheShards);
}

// Stage 2's worker, one per packing thread: its Packer, its estimator-class ids, and the
// chunk it is packing. A binding goes through look_ahead, then take_hit or pack_fresh, then
// class_key, make_record for a keyed miss, and local_class.
struct ChunkPacker {
  static constexpr int kRing = 16;
  PackCtx& c;
  const int t;
  Packer pk;
  SvMap<int32_t> ids;  // class key -> thread-local class id
  std::string key;     // the class key of the binding in hand
  SetsArgs A;
  int hi = 0;          // the chunk's end, its pools, and the lookups in flight
  Pools* P = nullptr;
  size_t ip0 = 0, lp0 = 0, to0 = 0, pr0 = 0, in0 = 0;  // where the binding in hand starts in them
  uint64_t ck_ring[kRing];
  const PackRec* rec_ring[kRing];

  ChunkPacker(PackCtx& c_, int t_) : c(c_), t(t_), pk{{c_.s, nullptr}} {}

  // kp_pack_cache lookups run ahead of the packing in stages, each prefetching what the
  // next one reads: the uid bytes (8 ahead), the key hash and its table slot (4 ahead), the
  // record (2 ahead); bindings without a record get the packer's own prefetches instead
  bool keyed_at(int j) const { return c.cache && j < hi && c.keys[j].uid.len > 0; }
  void stage_hash(int j) {
    if (!keyed_at(j)) return;
    const uint64_t ck = cache_key(c.keys[j]);
    ck_ring[j % kRing] = ck;
    pf(c.cache->shard[ck % kCacheShards].home_slot(ck));
  }
  void stage_rec(int j) {
    const PackRec* r = nullptr;
    if (keyed_at(j)) {
      const uint64_t ck = ck_ring[j % kRing];
      r = c.cache->shard[ck % kCacheShards].find(ck);
      if (r)
        for (int o = 0; o < 8; o++) pf((const char*)r + 64 * o);
    }
    rec_ring[j % kRing] = r;
    if (!r && j < hi) pf_arrays(c.bindings[j]);
  }
  void look_ahead_open(int lo) {  // what look_ahead would have done before the chunk's first binding
    for (int q = lo; q < std::min(hi, lo + 3); q++) pf_struct(&c.bindings[q]);
    if (c.cache) {
      for (int q = lo; q < std::min(hi, lo + 8); q++)
        if (keyed_at(q)) pf(c.keys[q].uid.ptr);
      for (int q = lo; q < lo + 4; q++) stage_hash(q);
      for (int q = lo; q < lo + 2; q++) stage_rec(q);
    } else if (lo + 1 < hi) {
      pf_arrays(c.bindings[lo + 1]);
    }
  }
  void look_ahead(int i) {
    const kp_binding* bindings = c.bindings;
    if (i + 3 < hi) pf_struct(&bindings[i + 3]);
    if (c.cache) {
      if (keyed_at(i + 8)) pf(c.keys[i + 8].uid.ptr);
      stage_hash(i + 4);
      stage_rec(i + 2);
      if (i + 1 < hi && !rec_ring[(i + 1) % kRing]) pf_strings(bindings[i + 1]);
    } else {
      if (i + 2 < hi) pf_arrays(bindings[i + 2]);
      if (i + 1 < hi) pf_strings(bindings[i + 1]);
    }
  }

  // A cached record (kp_pack_cache): its slices appended at the pools' ends, and its
  // references shifted onto them.
  void take_hit(const PackRec& hit, BindHdr& h) {
    h = hit.h;
    P->ipool.insert(P->ipool.end(), hit.ip(), hit.ip() + hit.n_ip);
    P->lpool.insert(P->lpool.end(), hit.lp(), hit.lp() + hit.n_lp);
    P->tols.insert(P->tols.end(), hit.tol(), hit.tol() + hit.n_tol);
    P->progs.insert(P->progs.end(), hit.pr(), hit.pr() + hit.n_pr);
    P->instrs.insert(P->instrs.end(), hit.in(), hit.in() + hit.n_in);
    shift_binding(h, P->ipool.data() + ip0, P->progs.data() + pr0, P->instrs.data() + in0, (int32_t)ip0,
                  (int32_t)lp0, (int32_t)to0, (int32_t)pr0, (int32_t)in0);
  }
  void pack_fresh(int i) { pk.pack(c.bindings[i], c.bt->hdr[i]); }

  // The binding's estimator class key into `key`; false for one that calls no estimator
  // (bcls -1: its row of the other estimators' answers, if any, is ignored).
  bool class_key(int i, const PackRec* hit) {
    BindHdr& h = c.bt->hdr[i];
    if (hit) {
      if (!hit->nonworkload) key.assign(hit->cls(), hit->cls_len);
      return !hit->nonworkload;
    }
    if (h.flags & BF_NONWORKLOAD_EST) return false;
    if (h.flags & BF_SETS) {
      // a component-set class: key 'S' + the resolved SetsArgs (est_key's keys
      // start with the 0/1 ReplicaRequirements word, never 'S')
      std::string err;
      const int rc = build_sets_args(c.s, c.bindings[i].components, c.bindings[i].n_components, &A, &err);
      if (rc == KP_EINVAL) {
        h.flags = (h.flags & ~(uint32_t)BF_SETS) | BF_BAD;  // status ERROR, as a bad request
      } else if (rc != KP_OK) {
        if (c.terr[t].empty()) c.terr[t] = err;
        h.flags &= ~(uint32_t)BF_SETS;
      }
      c.bt->route[i] = route_of(c.s->view, h, P->lpool.data());  // (flags changed)
    }
    if (h.flags & BF_SETS) {
      key.assign(1, 'S');
      key.append((const char*)&A, sizeof(A));
    } else {
      est_key(h, *P, &key);
    }
    return true;
  }

  // A new record of a keyed binding packed fresh: what the pools hold since the binding's
  // start, the header with its references relative to those slices, and the fields
  // PackRec::same compares.
  void make_record(int i, uint64_t ck, bool workload, std::vector<PackRec*>* shards) {
    const kp_binding& bb = c.bindings[i];
    const kp_binding_key& bk = c.keys[i];
    const uint32_t ul = bk.uid.len, al = bb.observed_affinity_name.len, cl = workload ? (uint32_t)key.size() : 0u;
    PackRec* r = PackRec::make((int)(P->ipool.size() - ip0), (int)(P->lpool.size() - lp0), (int)(P->tols.size() - to0),
                               (int)(P->progs.size() - pr0), (int)(P->instrs.size() - in0), (size_t)ul + al + cl);
    r->key = ck;
    r->gen = bk.generation;
    r->has_rt = bb.has_reschedule_triggered_at;
    r->has_lst = bb.has_last_scheduled_time;
    r->rt_ns = r->has_rt ? bb.reschedule_triggered_at_ns : 0;
    r->lst_ns = r->has_lst ? bb.last_scheduled_time_ns : 0;
    r->nonworkload = workload ? 0 : 1;
    r->uid_len = ul, r->aff_len = al, r->cls_len = cl;
    r->h = c.bt->hdr[i];
    std::copy(P->ipool.begin() + (long)ip0, P->ipool.end(), r->ip());
    std::copy(P->lpool.begin() + (long)lp0, P->lpool.end(), r->lp());
    std::copy(P->tols.begin() + (long)to0, P->tols.end(), r->tol());
    std::copy(P->progs.begin() + (long)pr0, P->progs.end(), r->pr());
    std::copy(P->instrs.begin() + (long)in0, P->instrs.end(), r->in());
    if (ul) memcpy((char*)r->uid(), bk.uid.ptr, ul);
    if (al) memcpy((char*)r->aff(), bb.observed_affinity_name.ptr, al);
    if (cl) memcpy((char*)r->cls(), key.data(), cl);
    shift_binding(r->h, r->ip(), r->pr(), r->in(), -(int32_t)ip0, -(int32_t)lp0, -(int32_t)to0, -(int32_t)pr0,
                  -(int32_t)in0);
    shards[ck % kCacheShards].push_back(r);
  }

  // The thread-local id of the class `key` names (with the binding's row, if rows there are).
  int32_t local_class(int i) {
    if (c.row_of) key.append((const char*)&c.row_of[i], 4);
    auto it = ids.find(key);
    if (it == ids.end()) {
      it = ids.emplace(key, (int32_t)c.tkeys[t].size()).first;
      c.tkeys[t].push_back(key);
    }
    return it->second;
  }

  void pack_chunk(int k) {
    kp_batch* bt = c.bt;
    const int lo = c.lo[k];
    hi = c.lo[k + 1];
    P = pk.bt = &c.pl[k];
    c.owner[k] = t;
    std::vector<PackRec*>* shards = c.cache ? &c.newrecs[(size_t)k * kCacheShards] : nullptr;
    uint64_t cap = 0, hits = 0;      // (chunk and thread totals kept in registers: the shared
    int max_tgt = 0, max_tiers = 1;  // arrays are written once per chunk, not once per binding)
    look_ahead_open(lo);
    for (int i = lo; i < hi; i++) {
      look_ahead(i);
      // a cached record counts with the same key, generation and status fields
      const bool keyed = keyed_at(i);
      const uint64_t ck = keyed ? ck_ring[i % kRing] : 0;
      const PackRec* hit = keyed ? rec_ring[i % kRing] : nullptr;
      if (hit && !hit->same(c.keys[i], c.bindings[i])) hit = nullptr;
      BindHdr& h = bt->hdr[i];
      ip0 = P->ipool.size(), lp0 = P->lpool.size(), to0 = P->tols.size(), pr0 = P->progs.size(),
      in0 = P->instrs.size();
      if (hit) take_hit(*hit, h), hits++;
      else pack_fresh(i);
      cap += h.out_cap;
      bt->route[i] = route_of(c.s->view, h, P->lpool.data());  // (chunk-relative pool offsets)
      max_tgt = std::max(max_tgt, (int)h.tgt_cnt);
      max_tiers = std::max(max_tiers, (int)h.ovf_cnt + 2);  // primary, each overflow term, unmatched
      const bool workload = class_key(i, hit);
      if (keyed && !hit) make_record(i, ck, workload, shards);
      bt->bcls[i] = workload ? local_class(i) : -1;
    }
    c.chunk_cap[k + 1] = cap;
    c.thits[t] += hits;
    c.tmax_tgt[t] = std::max(c.tmax_tgt[t], max_tgt);
    c.tmax_tiers[t] = std::max(c.tmax_tiers[t], max_tiers);
  }
};

// Stage 2: every chunk packed into its own pools, with the headers, the routes and the
// thread-local classes in the batch's arrays. False, with bt->err, when a thread met an error.
bool pack_chunks(PackCtx& c) {
  c.bt->bcls.resize(c.n);
  c.bt->route.resize(c.n);
  std::atomic<int> next_chunk(0);
  c.tq0 = PackClock::now();
  c.on_threads([&](int t) {
    struct Stamp {  // (the thread's time, written however it leaves)
      PackClock::time_point t0;
      double* out;
      ~Stamp() { *out = std::chrono::duration<double, std::milli>(PackClock::now() - t0).count(); }
    } stamp{PackClock::now(), &c.tms[t]};
    c.tstart[t] = std::chrono::duration<double, std::milli>(stamp.t0 - c.tpack0).count();
    ChunkPacker w(c, t);
    for (int k; (k = next_chunk.fetch_add(1)) < c.K;) w.pack_chunk(k);
  });
  c.tq1 = PackClock::now();
  for (auto& x : c.terr)
    if (!x.empty()) {
      c.bt->err = x;
      return false;
    }
  return true;
}

// Stage 3: global class ids (1-based; 0 = non-workload) from the threads' keys in thread
// order, with what a class's key says of it: its row of the other estimators' answers, and
// the component list of a component-set class.
void unify_classes(PackCtx& c) {
  kp_batch* bt = c.bt;
  SvMap<int32_t> gid;
  bt->crep.assign(1, 0);
  if (c.row_of) bt->cls_est.assign(1, -1);
  for (int t = 0; t < c.T; t++) {
    std::vector<int32_t>& remap = c.remaps[t];
    remap.resize(c.tkeys[t].size());
    for (size_t j = 0; j < c.tkeys[t].size(); j++) {
      const std::string& key = c.tkeys[t][j];
      auto it = gid.emplace(key, (int32_t)gid.size() + 1).first;
      remap[j] = it->second;
      if ((size_t)it->second != bt->crep.size()) continue;  // (a class an earlier thread met)
      bt->crep.push_back(-1);
      if (c.row_of) {  // the key's last four bytes
        int32_t r;
        memcpy(&r, key.data() + key.size() - 4, 4);
        bt->cls_est.push_back(r);
        if (r >= 0) bt->l_est_cls.push_back(it->second);
      }
      if (!key.empty() && key[0] == 'S') {  // component-set class: its rows come from k_sets_rows
        SetsArgs A;
        memcpy(&A, key.data() + 1, sizeof(A));
        bt->sets_cls.push_back(it->second);
        bt->sets_args.push_back(A);
      }
    }
  }
}

// Stage 4: the pools concatenated in chunk order. Each chunk's bases are the prefix sums of
// the pool sizes before it; the threads, chunk by chunk from a shared counter, give the
// chunk's bindings their global class and result slots, rebase them and copy the chunk's
// pools into place. False when the pools outgrow int32 offsets.
// The rebasing relies on the bindings' slices [ip_beg, ip_end), [pr_beg, pr_end) and
// [in_beg, in_end) being contiguous and partitioning the chunk's ipool, progs and instrs:
// Packer::pack opens them at the pools' ends and closes them at its end, and a record's hit
// appends at the ends. So shift_binding, per binding, touches every program and instruction
// of the chunk exactly once. (-DKP_PACK_CHECK, the sanitizer builds, verifies it here.)
void merge_chunk(PackCtx& c, int k) {
  kp_batch* bt = c.bt;
  Pools& q = c.pl[k];
  const int32_t oi = (int32_t)c.bi[k], ol = (int32_t)c.bl[k], oo = (int32_t)c.bo[k], op = (int32_t)c.bp[k],
                on = (int32_t)c.bn[k];
  const std::vector<int32_t>& remap = c.remaps[c.owner[k]];
  uint64_t off = c.chunk_cap[k];
#ifdef KP_PACK_CHECK
  int32_t ip_end = 0, pr_end = 0, in_end = 0;
#endif
  for (int i = c.lo[k]; i < c.lo[k + 1]; i++) {
    BindHdr& h = bt->hdr[i];
    bt->bcls[i] = bt->bcls[i] < 0 ? 0 : remap[bt->bcls[i]];
    h.out_off = off;  // private result slots: no atomic on the emit path
    off += h.out_cap;
#ifdef KP_PACK_CHECK
    if (h.ip_beg != ip_end || h.pr_beg != pr_end || h.in_beg != in_end) abort();
    ip_end = h.ip_end, pr_end = h.pr_end, in_end = h.in_end;
#endif
    if (k == 0) continue;  // (its bases are zero)
    shift_binding(h, q.ipool.data() + h.ip_beg, q.progs.data() + h.pr_beg, q.instrs.data() + h.in_beg, oi, ol, oo,
                  op, on);
  }
#ifdef KP_PACK_CHECK
  if ((size_t)ip_end != q.ipool.size() || (size_t)pr_end != q.progs.size() || (size_t)in_end != q.instrs.size()) abort();
#endif
  std::copy(q.ipool.begin(), q.ipool.end(), bt->ipool.begin() + (long)c.bi[k]);
  std::copy(q.lpool.begin(), q.lpool.end(), bt->lpool.begin() + (long)c.bl[k]);
  std::copy(q.tols.begin(), q.tols.end(), bt->tols.begin() + (long)c.bo[k]);
  std::copy(q.progs.begin(), q.progs.end(), bt->progs.begin() + (long)c.bp[k]);
  std::copy(q.instrs.begin(), q.instrs.end(), bt->instrs.begin() + (long)c.bn[k]);
  q = Pools();
}
bool merge_chunks(PackCtx& c) {
  kp_batch* bt = c.bt;
  const int K = c.K;
  for (int k = 0; k < K; k++) {
    c.bi[k + 1] = c.bi[k] + c.pl[k].ipool.size();
    c.bl[k + 1] = c.bl[k] + c.pl[k].lpool.size();
    c.bo[k + 1] = c.bo[k] + c.pl[k].tols.size();
    c.bp[k + 1] = c.bp[k] + c.pl[k].progs.size();
    c.bn[k + 1] = c.bn[k] + c.pl[k].instrs.size();
    c.chunk_cap[k + 1] += c.chunk_cap[k];
  }
  if (c.bi[K] > (size_t)INT32_MAX || c.bl[K] > (size_t)INT32_MAX || c.bo[K] > (size_t)INT32_MAX ||
      c.bp[K] > (size_t)INT32_MAX || c.bn[K] > (size_t)INT32_MAX)
    return false;  // pool offsets are int32
  bt->ipool.resize(c.bi[K]);
  bt->lpool.resize(c.bl[K]);
  bt->tols.resize(c.bo[K]);
  bt->progs.resize(c.bp[K]);
  bt->instrs.resize(c.bn[K]);
  bt->out_cap = c.chunk_cap[K];
  bt->max_tgt = *std::max_element(c.tmax_tgt.begin(), c.tmax_tgt.end());
  bt->max_tiers = *std::max_element(c.tmax_tiers.begin(), c.tmax_tiers.end());
  std::atomic<int> next_merge(0);
  c.on_threads([&](int) {
    for (int k; (k = next_merge.fetch_add(1)) < K;) merge_chunk(c, k);
  });
  return true;
}

// Stage 5: the new records into the shards (thread t fills shards t, t + T, ...), and the
// cache's counts.
void fill_cache(PackCtx& c) {
  kp_pack_cache* cache = c.cache;
  if (!cache) return;
  c.on_threads([&](int t) {
    for (int sh = t; sh < kCacheShards; sh += c.T) {
      PackTable& tab = cache->shard[sh];
      for (int k = 0; k < c.K; k++)
        for (PackRec*& r : c.newrecs[(size_t)k * kCacheShards + sh]) {
          tab.put(r);
          r = nullptr;
        }
    }
  });
  uint64_t h = 0;
  for (uint64_t x : c.thits) h += x;
  cache->hits += h;
  cache->misses += (uint64_t)c.n - h;
  cache->last_hits = h;
}

// Stage 6: a class's representative, its first binding.
void pick_representatives(PackCtx& c) {
  kp_batch* bt = c.bt;
  size_t left = bt->crep.size() - 1;
  for (int i = 0; i < c.n && left; i++) {
    const int32_t g = bt->bcls[i];
    if (g && bt->crep[g] < 0) {
      bt->crep[g] = i;
      left--;
    }
  }
}

// KP_PACK_TIMING: the pack stage, and everything after it up to this call.
void report_timing(const PackCtx& c) {
  auto ms = [](auto x, auto y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
  fprintf(stderr, "pack_parallel: %d threads, %d chunks, pack %.1f ms, merge+classes %.1f ms; per thread", c.T, c.K,
          ms(c.tq0, c.tq1), ms(c.tq1, PackClock::now()));
  for (double x : c.tms) fprintf(stderr, " %.1f", x);
  fprintf(stderr, "; started at");
  for (double x : c.tstart) fprintf(stderr, " %.1f", x);
  fprintf(stderr, "\n");
#ifdef KP_PACK_PROF
  fprintf(stderr, "pack sections (Mcycles, cumulative): gvk %.1f targets %.1f tolerations %.1f affinity %.1f "
          "static %.1f requests %.1f rest %.1f\n", g_pack_cyc[0] / 1e6, g_pack_cyc[1] / 1e6, g_pack_cyc[2] / 1e6,
          g_pack_cyc[3] / 1e6, g_pack_cyc[4] / 1e6, g_pack_cyc[5] / 1e6, g_pack_cyc[6] / 1e6);
#endif
}

bool pack_parallel(kp_snapshot* s, const kp_binding* bindings, int n, kp_batch* bt, const kp_binding_key* keys,
                   kp_pack_cache* cache, const int32_t* row_of) {
  const int T = std::max(1, std::min((int)kp_env_int("KP_PACK_THREADS", host_cpus()), n / 4096));
  PackCtx c(s, bindings, n, bt, keys, cache, row_of, T);
  prepare_cache(c);
  if (!pack_chunks(c)) return false;
  unify_classes(c);
  if (!merge_chunks(c)) return false;
  fill_cache(c);
  pick_representatives(c);
  if (kp_env_flag("KP_PACK_TIMING")) report_timing(c);
  return true;
}
}  // namespace

// Bindings per estimator class below which a batch skips the class orders.
static int64_t order_amort() {  // (read per batch: tests switch it)
  return std::max<int64_t>(0, kp_env_int("KP_ORDER_AMORT", 4));
}

extern "C" {

int kp_batch_create_filters(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, const kp_binding_key* keys,
                            uint64_t n, kp_pack_cache* cache, const kp_estimates* est, const kp_filter_answers* flt,
                            kp_batch** out) {
  if (cache && n && !keys) return KP_EINVAL;  // (as kp_batch_create_keyed)
  BatchAnswers a;
  a.est = est;
  a.flt = flt;
  return batch_create_with(e, sc, bindings, n, cache ? keys : nullptr, cache, &a, out);
}
int kp_batch_create_estimates(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, const kp_binding_key* keys,
                              uint64_t n, kp_pack_cache* cache, const kp_estimates* est, kp_batch** out) {
  return kp_batch_create_filters(e, sc, bindings, keys, n, cache, est, nullptr, out);
}
int kp_batch_create(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, uint64_t n, kp_batch** out) {
  return kp_batch_create_filters(e, sc, bindings, nullptr, n, nullptr, nullptr, nullptr, out);
}
int kp_batch_create_keyed(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, const kp_binding_key* keys,
                          uint64_t n, kp_pack_cache* cache, kp_batch** out) {
  if (!cache || (n && !keys)) return KP_EINVAL;
  return kp_batch_create_filters(e, sc, bindings, keys, n, cache, nullptr, nullptr, out);
}
int kp_batch_digest(const kp_batch* b, uint64_t* out) {
  if (!b || !out) return KP_EINVAL;
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ c[i]) * 1099511628211ull;
  };
  mix(b->hdr.data(), sizeof(BindHdr) * b->hdr.size());
  mix(b->ipool.data(), 4 * b->ipool.size());
  mix(b->lpool.data(), 8 * b->lpool.size());
  mix(b->tols.data(), sizeof(Tol) * b->tols.size());
  mix(b->progs.data(), sizeof(Prog) * b->progs.size());
  mix(b->instrs.data(), sizeof(Instr) * b->instrs.size());
  mix(b->route.data(), b->route.size());
  for (size_t i = 0; i < b->bcls.size(); i++) {  // the class by its first binding (ids follow thread order)
    const int32_t g = b->bcls[i];
    const int32_t rep = g > 0 && (size_t)g < b->crep.size() ? b->crep[g] : -1;
    mix(&rep, 4);
  }
  *out = h;
  return KP_OK;
}
int kp_pack_cache_create(uint64_t max_entries, kp_pack_cache** out) {
  if (!out) return KP_EINVAL;
  auto* c = new kp_pack_cache();
  if (max_entries) c->max_entries = max_entries;
  *out = c;
  return KP_OK;
}
void kp_pack_cache_destroy(kp_pack_cache* c) { delete c; }
int kp_pack_cache_get_stats(const kp_pack_cache* c, kp_pack_cache_stats* out) {
  if (!c || !out) return KP_EINVAL;
  out->hits = c->hits;
  out->misses = c->misses;
  out->entries = c->entries();
  out->last_hits = c->last_hits;
  return KP_OK;
}
void kp_batch_destroy(kp_batch* b) { delete b; }

}  // extern "C"

// batch_create_with runs in stages (take_answers ... upload, in that order); CreateCtx is
// what they share. Every host array the arena uploads from and no kp_batch member keeps
// lives here, with the rows' staging copy, so it outlives the upload's sync by construction.
namespace {
struct CreateCtx {
  kp_engine* e;
  kp_snapshot* s;
  const kp_binding* bindings;
  uint64_t n;
  BatchAnswers& ans;               // est / flt null once found empty or unused
  kp_batch* bt = nullptr;
  Arena staging;                   // the caller-order rows make_answer_rows ranks on the device
  std::vector<int32_t> rep;        // d_crep's source: crep, -1 in the component-set classes
  std::vector<int64_t> sets_off;   // per cluster rank, its node-run scratch offset
  bool with_orders = false;
  std::chrono::steady_clock::time_point tp0, tp1, tp2;
};
}  // namespace

// Stage 1: a kp_batch_create* call's own inputs (BatchAnswers::est / flt) checked before
// anything is packed, the estimates first, and the batch's part taken from them; an input
// without rows, or verdicts no binding has a row of, counts as none from here on.
static int take_answers(CreateCtx& c) {
  BatchAnswers& a = c.ans;
  if (int rc = check_estimates(c.e, c.s, "kp_batch_create_estimates", "", a.est, c.n)) return rc;
  if (a.est && a.est->n_rows == 0) a.est = nullptr;
  if (a.est) a.est_row_of = a.est->row_of;
  if (!a.flt) return KP_OK;
  const char* who = "kp_batch_create_filters";
  a.flt_plugins = a.flt->n_plugins;
  if (int rc = check_filters(c.e, c.s, who, "", a.flt, c.n)) return rc;
  if (a.flt->n_rows == 0) a.flt = nullptr;
  if (!a.flt) return KP_OK;
  if (int rc = check_row_of(c.e, who, "", a.flt->row_of, 0, c.n, a.flt->n_rows)) return rc;
  for (uint64_t i = 0; i < c.n; i++)
    if (a.flt->row_of[i] >= 0) a.flt_list.push_back(FltPair{(int32_t)i, a.flt->row_of[i]});
  if (a.flt_list.empty()) a.flt = nullptr;
  return KP_OK;
}

// Stage 2: the selection lists from the routes (binding order within each kind), and the
// 256-region refusal. SEL_ALL:
// [non-StaticWeight | StaticWeight]; the non-StaticWeight ones split by the subset
// they likely need (k_select_top's small LDS slice first: a DynamicWeight /
// Aggregated subset holds the scheduled clusters and about as many walked parties
// as the target replicas), each part grouped by estimator class (counting sort,
// stable: the workgroups resident at any moment then cover a short run of the list,
// i.e. few classes, whose orders and rows stay in every XCD's L2; k_select_top
// 1.23 -> 1.10 ms at config 3, mapping each XCD to one contiguous run of the list
// instead was slower, 1.33 ms); StaticWeight bindings the class-level kernel covers
// (bits mode) before the others.
static int route_lists(CreateCtx& c) {
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const uint64_t n = c.n;
  {
    const std::vector<uint8_t>& rt = bt->route;
    const size_t ncls = std::max<size_t>(1, bt->crep.size());
    std::vector<int32_t> cnt(2 * ncls + 1, 0);
    int n_dyn = 0, n_small = 0, n_stat = 0, n_stat_ok = 0, n_cl = 0, n_rg = 0;
    for (uint64_t i = 0; i < n; i++) {
      const uint8_t r = rt[i];
      if (r & RT_CLUSTER) n_cl++;
      else if (r & RT_REGION) n_rg++;
      else if (r & RT_DYN) {
        n_dyn++;
        const bool sm = (r & RT_SMALL) != 0;
        n_small += sm;
        cnt[(sm ? 0 : ncls) + (size_t)std::max(0, bt->bcls[i]) + 1]++;
      } else {
        n_stat++;
        n_stat_ok += (r & RT_STATIC_OK) ? 1 : 0;
      }
    }
    for (size_t k = 1; k <= 2 * ncls; k++) cnt[k] += cnt[k - 1];
    bt->l_all.resize((size_t)n_dyn + n_stat);
    bt->l_cluster.resize(n_cl);
    bt->l_region.resize(n_rg);
    bt->l_cs.resize((size_t)n_cl + n_rg);
    int pc = 0, pr = 0, ps = n_dyn, pso = n_dyn + n_stat_ok, pcs = 0;
    for (uint64_t i = 0; i < n; i++) {
      const uint8_t r = rt[i];
      const int32_t b = (int32_t)i;
      if (r & (RT_CLUSTER | RT_REGION)) {
        bt->l_cs[pcs++] = b;
        if (r & RT_CLUSTER) bt->l_cluster[pc++] = b;
        else bt->l_region[pr++] = b;
      } else if (r & RT_DYN) {
        bt->l_all[cnt[((r & RT_SMALL) ? 0 : ncls) + (size_t)std::max(0, bt->bcls[i])]++] = b;
      } else if (r & RT_STATIC_OK) {
        bt->l_all[ps++] = b;
      } else {
        bt->l_all[pso++] = b;
      }
    }
    bt->n_all_dyn = n_dyn;
    bt->n_top_small = n_small;
    bt->n_static = n_stat_ok;
  }
  bt->l_all_cls.resize(bt->l_all.size());
  for (size_t i = 0; i < bt->l_all.size(); i++) bt->l_all_cls[i] = bt->bcls[bt->l_all[i]];
  bt->l_slow = bt->l_all;
  bt->l_slow.insert(bt->l_slow.end(), bt->l_cluster.begin(), bt->l_cluster.end());
  if (s->view.n_regions > kRegionMax && !bt->l_region.empty()) {
    c.e->err = "region spread over more than 256 regions is not supported";
    return KP_ENOTSUP;
  }
  // the region bindings that can need k_region_wide, by their row in l_region (rsel, rnsel
  // and rout are indexed by it)
  for (size_t j = 0; j < bt->l_region.size(); j++) {
    const BindHdr& h = bt->hdr[bt->l_region[j]];
    if (h.cluster_max > kSmallMax || ((h.flags & BF_DUP_TARGETS) && h.tgt_cnt > kTgtSmallMax))
      bt->l_region_wide.push_back((int32_t)j);
  }
  return KP_OK;
}

// Stage 3: the serial kernels' sizes (k_slow, k_region_wide): result capacity, LDS areas,
// scratch slots and grids, with their env knobs; and the batch's LDS check, which reads
// k_region_wide's sort area.
static int size_serial(CreateCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  int P = 1;
  while (P < s->Cp) P <<= 1;
  // k_region_wide's candidate sort in LDS when the keys fit beside the rest (KP_WIDE_LDS=0,
  // a diagnostic, keeps them in the global slot), as k_slow's
  if (!bt->l_region_wide.empty() && kp_env_int("KP_WIDE_LDS", 1) != 0 &&
      region_wide_lds_bytes(s->Cp, s->view.n_regions, 8 * P) <= e->max_lds)
    bt->wide_sort = 8 * P;
  if (batch_lds_check(e, s, bt)) return KP_ENOTSUP;
  bt->n_regions = s->view.n_regions;
  const int max_tgt = bt->max_tgt, max_tiers = bt->max_tiers;
  // SerialAssign's result list: every candidate once, plus, per overflow tier, the
  // spec.Clusters entries MergeTargetClusters appends (common.go:97-139; util/binding.go:91-115).
  bt->slow_cap = s->Cp + max_tiers * max_tgt + 64;
  {  // LDS for the targets-only serial problems (scale-down), if small
    size_t b = sizeof(Item) * (size_t)max_tgt + serial_scratch_bytes(2 * max_tgt + 16) + 64;
    bt->slow_lds = b <= 32768 ? (int)((b + 15) & ~(size_t)15) : 0;
  }
  {  // LDS for the candidate sorts (bitonic keys, then the sort.Sort emulation)
    const size_t base = slow_lds_bytes(s->Cp, bt->slow_lds, 0);
    const size_t sel = 3072 + 8 * (size_t)sel_all_ecap(s->Cp) + 64;  // SelScratch of the tie route
    const size_t pdq = (std::max(pdq_wave_bytes(s->Cp), sel) + 15) & ~(size_t)15;
    const size_t both = std::max(8 * (size_t)P, pdq);
    bt->slow_sort = base + both <= e->max_lds ? (int)both : (base + pdq <= e->max_lds ? (int)pdq : 0);
  }
  bt->slow_slot = (size_t)s->Cp * 8 + (size_t)P * 8 + sizeof(Item) * s->Cp + 4 * (size_t)s->Cp +
                  serial_scratch_bytes(bt->slow_cap) + 1024;
  bt->slow_slot = (bt->slow_slot + 255) & ~(size_t)255;
  // k_slow: one workgroup per CU pass over the flagged bindings (appended on device)
  bt->slow_grid = (int)std::max<size_t>(1, std::min<size_t>(256, bt->l_slow.size()));
  // diagnostics: KP_SLOW_GRID=<g> caps k_slow's grid, KP_SLOW_LDS=0 keeps its sort
  // keys and scale-down scratch in the global slot (no LDS sort, no wave sort.Sort)
  bt->slow_grid = std::max(1, std::min(bt->slow_grid, (int)kp_env_int("KP_SLOW_GRID", bt->slow_grid)));
  if (kp_env_int("KP_SLOW_LDS", 1) == 0) bt->slow_sort = bt->slow_lds = 0;
  if (!bt->l_region_wide.empty()) {
    // one slot per workgroup; the grid capped so the slots stay within 256 MB (a slot is
    // ~37 MB at Cp = 262144, ~0.8 MB at C = 5000)
    bt->wide_slot = region_wide_slot_bytes(s->Cp, bt->slow_cap);
    const size_t fit = std::max<size_t>(1, ((size_t)256 << 20) / bt->wide_slot);
    bt->wide_grid = (int)std::min<size_t>({(size_t)64, bt->l_region_wide.size(), fit});
  }
  bt->fast_ok = batch_fast_ok(bt);
  return KP_OK;
}

// Stage 4: what the estimator classes get. Class orders or not (with_orders), the
// singleton classes that keep feasible entries only (est_single), the representatives'
// upload form, and the component-set classes' scratch offsets.
static void plan_classes(CreateCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int B = bt->B ? bt->B : 1;
  // k_select_top (bits mode): class orders, fallback list. k_class_order sorts a class
  // row in LDS (kRedBytes + 8 * nextpow2(C)): a device with less LDS per workgroup
  // keeps the full-candidate kernels instead of failing the launch.
  // Class orders pay off when each order serves several bindings: a batch of nearly
  // one class per binding (per-binding requests) sorts a Cp row per binding instead,
  // so it keeps the full-candidate kernels (KP_ORDER_AMORT: bindings per class needed)
  const bool orders_pay = (int64_t)bt->crep.size() * order_amort() <= (int64_t)B;
  c.with_orders = s->C <= 16384 && !bt->crep.empty() && orders_pay &&
                  class_order_lds_bytes(class_order_pad(s->C)) <= e->max_lds;
  // singleton classes: feasible entries only, when every reader gathers feasible candidates
  // (no class orders, which sort whole rows; no spread lists; no component-set classes)
  static const bool est_single_on = kp_env_int("KP_EST_SINGLE", 1) != 0;
  if (est_single_on && !c.with_orders && bt->crep.size() > 1 && bt->l_cluster.empty() && bt->l_region.empty() &&
      bt->sets_cls.empty()) {
    std::vector<int32_t> cnt(bt->crep.size(), 0);
    for (uint64_t i = 0; i < c.n; i++) cnt[(size_t)std::max(0, bt->bcls[i])]++;
    // (a class with a row of the other estimators' answers keeps its whole row: k_est_extra
    // merges it before EV_CLASS_ROWS, the feasible-only rows are written after)
    auto has_est = [&](size_t g) { return !bt->cls_est.empty() && bt->cls_est[g] >= 0; };
    for (size_t g = 0; g < bt->crep.size(); g++)
      (g > 0 && cnt[g] == 1 && !has_est(g) ? bt->l_cls_single : bt->l_cls_full).push_back((int32_t)g);
    bt->est_single = !bt->l_cls_single.empty();
  }
  // representatives of the k_est_class rows; -1 for the component-set classes (k_sets_rows)
  c.rep = bt->crep;
  for (int32_t g : bt->sets_cls) c.rep[g] = -1;
  // component-set classes: per cluster rank its node-run scratch (one run per model
  // node at most, capped at kSetsRunsMax) for k_sets_rows, reused class after class
  if (!bt->sets_cls.empty()) {
    for (uint64_t i = 0; i < c.n; i++)
      if (bt->hdr[i].flags & BF_SETS) bt->l_sets.push_back((int32_t)i);
    c.sets_off.assign((size_t)s->C + 1, 0);
    // (KP_SETS_RUNS_CAP lowers it: tests of the overflow report)
    const int64_t runs_cap = std::max<int64_t>(1, std::min<int64_t>(kp_env_int("KP_SETS_RUNS_CAP", kSetsRunsMax), kSetsRunsMax));
    for (int r = 0; r < s->C; r++) {
      int64_t nodes = 0;
      for (int g = s->mgrp_off[r]; g < s->mgrp_off[r + 1]; g++) nodes += s->mgrp_cnt[g];
      c.sets_off[r + 1] = c.sets_off[r] + std::max<int64_t>(1, std::min<int64_t>(nodes, runs_cap));
    }
  }
}

// Stage 5: every device buffer of the batch registered in one pass (the order fixes the
// sub-buffer offsets, so it does not change), the arena and the page-locked
// launch-argument slots.
static int plan_arena(CreateCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  auto pad1 = [](auto& v) {
    if (v.empty()) v.resize(1);
  };
  pad1(bt->ipool);
  pad1(bt->lpool);
  pad1(bt->tols);
  pad1(bt->progs);
  pad1(bt->instrs);
  const int B = bt->B ? bt->B : 1;
  const int nr = (int)bt->l_region.size(), R = std::max(1, s->view.n_regions);
  const size_t n_cls = bt->crep.size();
  const uint64_t out2 = std::max<uint64_t>(1, 2 * bt->out_cap);
  Arena& a = bt->dev;
  a.pool_dev = e->device;
  BatchView& v = bt->view;
  v.B = bt->B;
  a.add(&v.hdr, bt->hdr.data(), bt->hdr.size(), 1);
  a.add(&v.ipool, bt->ipool.data(), bt->ipool.size());
  a.add(&v.lpool, bt->lpool.data(), bt->lpool.size());
  a.add(&v.tols, bt->tols.data(), bt->tols.size());
  a.add(&v.progs, bt->progs.data(), bt->progs.size());
  a.add(&v.instrs, bt->instrs.data(), bt->instrs.size());
  a.add(&bt->fmask, (size_t)B * s->W);
  a.add(&bt->d_bcls, bt->bcls.data(), bt->bcls.size(), 1);
  a.add(&bt->d_crep, c.rep.data(), c.rep.size());
  a.add(&bt->cls_rows, n_cls * (size_t)s->Cp);
  a.add(&bt->d_all, bt->l_all.data(), bt->l_all.size(), 1);
  a.add(&bt->d_all_cls, bt->l_all_cls.data(), bt->l_all_cls.size(), 1);
  a.add(&bt->d_cluster, bt->l_cluster.data(), bt->l_cluster.size(), 1);
  a.add(&bt->d_region, bt->l_region.data(), bt->l_region.size(), 1);
  a.add(&bt->d_slowlist, std::max<size_t>(1, bt->l_slow.size()));  // (appended on the device)
  a.add(&bt->d_cs, bt->l_cs.data(), bt->l_cs.size(), 1);
  a.add(&bt->status, B);
  a.add(&bt->errc, B);
  a.add(&bt->slow, B);
  a.add(&bt->arg, B);
  a.add(&bt->start, B);
  a.add(&bt->count, B);
  a.add(&bt->counter, 1);
  a.add(&bt->stats, kStatSlots);
  a.add(&bt->d_kargs, kArgSlots);
#if defined(KP_STAMPS) || defined(KP_SLOW_CHECK)
  a.add(&bt->dbg, kDbgSlots * kDbgSpread);
#endif
  // [0, out_cap): per-binding slots; [out_cap, 2 out_cap): serial results past their slot
  a.add(&bt->out_idx, out2);
  a.add(&bt->out_rep, out2);
  a.add(&bt->offsets_d, B + 1);
  a.add(&bt->off_part, (size_t)(B + kOffChunk - 1) / kOffChunk);
  a.add(&bt->cidx_d, out2);
  a.add(&bt->crep_d, out2);
  a.add(&bt->rout, (size_t)std::max(1, nr) * R);
  a.add(&bt->rstat, std::max(1, nr));
  a.add(&bt->rsel, (size_t)std::max(1, nr) * R);
  a.add(&bt->rnsel, std::max(1, nr));
  a.add(&bt->nhost, 1);
  a.add(&bt->slow_scratch, bt->slow_slot * bt->slow_grid);
  if (!bt->l_region_wide.empty()) {
    a.add(&bt->d_region_wide, bt->l_region_wide.data(), bt->l_region_wide.size());
    a.add(&bt->wide_scratch, bt->wide_slot * bt->wide_grid);
  }
  // Without class orders k_select_top thresholds each binding's votes by a histogram instead
  // of walking an order (kp_top.h), so its fallback list exists either way.
  if (n_cls) {
    a.add(&bt->d_fb, std::max(1, bt->n_all_dyn));
    a.add(&bt->d_ofb, std::max(1, bt->n_all_dyn));
  }
  if (bt->est_single) {
    a.add(&bt->d_cls_full, bt->l_cls_full.data(), bt->l_cls_full.size());
    a.add(&bt->d_cls_single, bt->l_cls_single.data(), bt->l_cls_single.size());
  }
  if (c.with_orders) {
    a.add(&bt->d_ord, n_cls * (size_t)s->Cp);
    a.add(&bt->d_ctot, n_cls);
    a.add(&bt->d_cok, n_cls);
    a.add(&bt->d_fbc, std::max<size_t>(1, bt->l_cluster.size()));
    a.add(&bt->d_fbr, std::max(1, nr));
    a.add(&bt->d_fba, std::max(1, nr));
  }
  if (!bt->sets_cls.empty()) {
    a.add(&bt->d_sets_args, bt->sets_args.data(), bt->sets_args.size());
    a.add(&bt->d_sets_off, c.sets_off.data(), c.sets_off.size());
    a.add(&bt->d_sets_scratch, (size_t)c.sets_off.back() * (1 + kSetsSlots));
    a.add(&bt->d_sets_ovf, bt->sets_cls.size());
    a.add(&bt->d_sets_list, bt->l_sets.data(), bt->l_sets.size());
  }
  if (!bt->l_est_cls.empty()) {
    a.add(&bt->d_cls_est, bt->cls_est.data(), bt->cls_est.size());
    a.add(&bt->d_est_cls, bt->l_est_cls.data(), bt->l_est_cls.size());
  }
  if (!bt->l_flt.empty()) a.add(&bt->d_flt_list, bt->l_flt.data(), bt->l_flt.size());
  c.tp1 = std::chrono::steady_clock::now();
  HIPCHK(a.alloc());
  bt->h_kargs = (KArgs*)pinned_get(sizeof(KArgs) * kArgSlots, &bt->h_kargs_bytes);
  if (!bt->h_kargs) {
    e->err = "kp_batch_create: page-locked launch-argument slots";
    return KP_EDEVICE;
  }
  return KP_OK;
}

// Stage 6: the copies, the rows of a kp_batch_create* call's own inputs when a class or a
// binding has one (ranked on the device, unprofiled), k_slow's flags cleared, the sync, and
// the KP_PACK_TIMING lines. create_stream is set while work may be queued: an early return
// waits for it in ~kp_batch before the arena and the rows go back to the pool.
static int upload(CreateCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int B = bt->B ? bt->B : 1;
  bt->create_stream = e->stream;
  c.tp2 = std::chrono::steady_clock::now();
  HIPCHK(bt->dev.upload(e->stream));
  const kp_estimates* est = bt->l_est_cls.empty() ? nullptr : c.ans.est;
  const kp_filter_answers* flt = bt->l_flt.empty() ? nullptr : c.ans.flt;
  if (est || flt)
    if (int rc = make_answer_rows(e, s, est, flt, e->stream, &c.staging, nullptr, &bt->rows)) return rc;
  if (bt->rows) bt->d_est_rows = bt->rows->d_est, bt->d_flt_rows = bt->rows->d_flt;
  HIPCHK(dev::fill(bt->slow, 0, 4 * (size_t)B, e->stream));
  HIPCHK(dev::sync(e->stream));
  c.staging.reset();
  if (kp_env_flag("KP_PACK_TIMING")) {
    if (!bt->l_est_cls.empty())
      fprintf(stderr, "kp_batch_create_estimates: %zu classes with a row, %zu bytes uploaded for them\n",
              bt->l_est_cls.size(),
              4 * (bt->cls_est.size() + bt->l_est_cls.size() + (est ? (size_t)est->n_rows * s->C : 0)));
    if (!bt->l_flt.empty())
      fprintf(stderr, "kp_batch_create_filters: %zu bindings with a row, %zu bytes uploaded for them\n",
              bt->l_flt.size(),
              sizeof(FltPair) * bt->l_flt.size() + (flt ? 8 * (size_t)flt->n_rows * (((size_t)s->C + 63) / 64) : 0));
    const auto tp3 = std::chrono::steady_clock::now();
    auto ms = [](auto x, auto y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
    fprintf(stderr, "kp_batch_create: pack %.1f ms, alloc %.1f ms, upload %.1f ms\n", ms(c.tp0, c.tp1),
            ms(c.tp1, c.tp2), ms(c.tp2, tp3));
  }
  bt->create_stream = nullptr;
  return KP_OK;
}

// The validations come in this order, which decides the error a call wrong in two ways
// sees: estimates, filters, the components check, then the packer.
int batch_create_with(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, uint64_t n,
                      const kp_binding_key* keys, kp_pack_cache* cache, BatchAnswers* ans, kp_batch** out) {
  if (!e || !sc || !out || (n && !bindings)) return KP_EINVAL;
  if (n > (uint64_t)INT32_MAX) return KP_ENOTSUP;
  (void)dev::set_device(e->device);
  CreateCtx c{e, const_cast<kp_snapshot*>(sc), bindings, n, *ans};
  kp_snapshot* s = c.s;
  if (int rc = take_answers(c)) return rc;
  auto* bt = new kp_batch();
  std::unique_ptr<kp_batch> guard(bt);
  c.bt = bt;
  bt->snap = s;
  bt->B = (int)n;
  bt->hdr.resize(n);
  bt->rows = ans->rows;
  bt->flt_plugins = ans->flt_plugins;
  bt->l_flt = std::move(ans->flt_list);
  const int32_t* est_row_of = ans->est_row_of;
  c.tp0 = std::chrono::steady_clock::now();
  if (s->opts.multiple_pod_templates_scheduling)
    for (uint64_t i = 0; i < n; i++)
      if (bindings[i].n_components > 0 && !bindings[i].components) {
        e->err = "kp_batch_create: binding " + std::to_string(i) +
                 " has n_components > 0 but no components (the MultiplePodTemplatesScheduling gate reads them)";
        return KP_EINVAL;
      }
  if (!pack_parallel(s, bindings, (int)n, bt, keys, cache, est_row_of)) {
    e->err = bt->err.empty() ? "batch pools exceed 2^31 entries" : bt->err;
    return KP_ENOTSUP;
  }
  if (int rc = route_lists(c)) return rc;
  if (int rc = size_serial(c)) return rc;
  plan_classes(c);
  if (int rc = plan_arena(c)) return rc;
  if (int rc = upload(c)) return rc;
  *out = guard.release();
  return KP_OK;
}
