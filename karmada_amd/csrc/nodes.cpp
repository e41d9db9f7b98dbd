// nodes.cpp — the node estimator: a member cluster's nodes and claims compiled for the
// device, kp_model_grades, kp_node_max_replicas and kp_node_max_component_sets. Needs
// qmap (snapshot.cpp) and valid_req (pack.cpp).
#include "kp_host.h"
#include "kp_nodes.h"

// ---------------------------------------------------------------------------
// Member-cluster nodes
// ---------------------------------------------------------------------------
namespace {
// util.Resource (util/resource.go:28-93): cpu in milli, the rest in units; scalar
// resources only under IsScalarResourceName.
struct NodeRes {
  int64_t cpu = 0, mem = 0, eph = 0, pods = 0;
  std::map<std::string, int64_t> sc;
};
void res_add(NodeRes& r, const QtyMap& rl) {
  for (auto& kv : rl) {
    const std::string& n = kv.first;
    if (n == "cpu") r.cpu += k8s::milli(kv.second);
    else if (n == "memory") r.mem += k8s::value(kv.second);
    else if (n == "pods") r.pods += k8s::value(kv.second);
    else if (n == "ephemeral-storage") r.eph += k8s::value(kv.second);
    else if (k8s::scalar_resource(n)) r.sc[n] += k8s::value(kv.second);
  }
}
k8s::Qty qty_of(int64_t v, int64_t unit_nano, int fmt) {
  k8s::Qty q;
  q.nano = (k8s::i128)v * unit_nano;
  q.fmt = fmt;
  return q;
}
// getNodeAvailable (cluster_status_controller.go:613-639); false: no pod room
// (the caller's walk stops there).
bool node_available(const kp_node& nd, QtyMap* out) {
  QtyMap alloc;
  if (!qmap(nd.allocatable, nd.n_allocatable, &alloc)) return false;
  if (nd.n_pods == 0) {  // no pods on the node: nodePodResourcesMap has no entry
    *out = alloc;
    return true;
  }
  QtyMap req;
  qmap(nd.requested, nd.n_requested, &req);
  NodeRes pr;
  res_add(pr, req);
  pr.pods += nd.n_pods;  // AddResourcePods
  QtyMap al;  // Resource.ResourceList(): the positive fields
  if (pr.cpu > 0) al["cpu"] = qty_of(pr.cpu, 1000000, 0);
  if (pr.mem > 0) al["memory"] = qty_of(pr.mem, 1000000000, 1);
  if (pr.eph > 0) al["ephemeral-storage"] = qty_of(pr.eph, 1000000000, 1);
  if (pr.pods > 0) al["pods"] = qty_of(pr.pods, 1000000000, 0);
  for (auto& kv : pr.sc)
    if (kv.second > 0) al[kv.first] = qty_of(kv.second, 1000000000, kv.first.rfind("hugepages-", 0) == 0 ? 1 : 0);
  auto pods_of = [](const QtyMap& m) {
    auto it = m.find("pods");
    return it == m.end() ? (int64_t)0 : k8s::value(it->second);
  };
  if (pods_of(alloc) - pods_of(al) <= 0) return false;
  for (auto& kv : al) {
    auto it = alloc.find(kv.first);
    if (it != alloc.end()) k8s::qsub(it->second, kv.second);
  }
  *out = alloc;
  return true;
}
// A member cluster's nodes in one call's dictionary (NodeView's host arrays).
struct HostNodes {
  std::vector<uint32_t> flags;
  std::vector<int32_t> name, lbl_off{0}, tnt_off{0}, tnt;
  std::vector<int64_t> lbl, lbl_int;
  std::vector<uint8_t> lbl_int_ok;
};
void pack_nodes(const kp_node* nodes, uint64_t n, Dict& d, HostNodes& h) {
  for (uint64_t i = 0; i < n; i++) {
    const kp_node& nd = nodes[i];
    h.flags.push_back(nd.unschedulable ? 1u : 0u);
    const std::string nm = S(nd.name);
    h.name.push_back(nm.empty() ? -1 : d.add(nm));
    std::map<std::string, std::string> lm;  // node.Labels is a map
    for (uint32_t j = 0; j < nd.n_labels; j++) lm[S(nd.labels[j].key)] = S(nd.labels[j].value);
    for (auto& kv : lm) {
      h.lbl.push_back(((int64_t)d.add(kv.first) << 32) | (int64_t)(uint32_t)d.add(kv.second));
      int64_t x = 0;
      const bool ok = k8s::parse_int64(kv.second, &x);
      h.lbl_int.push_back(ok ? x : 0);
      h.lbl_int_ok.push_back(ok ? 1 : 0);
    }
    h.lbl_off.push_back((int32_t)h.lbl.size());
    for (uint32_t j = 0; j < nd.n_taints; j++) {
      const std::string ef = S(nd.taints[j].effect);
      if (ef != "NoSchedule" && ef != "NoExecute") continue;  // DoNotScheduleTaintsFilterFunc
      h.tnt.push_back(d.add(S(nd.taints[j].key)));
      h.tnt.push_back(d.add(S(nd.taints[j].value)));
      h.tnt.push_back(ef == "NoSchedule" ? EFF_NOSCHEDULE : EFF_NOEXECUTE);
    }
    h.tnt_off.push_back((int32_t)(h.tnt.size() / 3));
  }
}
// pb.NodeClaim -> ClaimProg's host arrays (offsets relative to this claim).
struct HostClaim {
  std::vector<int64_t> sel;
  std::vector<Tol> tols;
  int32_t tol_unsched = 0, has_aff = 0;
  std::vector<int32_t> term_off{0};
  std::vector<NodeReq> reqs;
  std::vector<int32_t> vals;
};
void compile_claim(const kp_node_claim* c, Dict& d, HostClaim& h) {
  if (!c) return;
  std::map<std::string, std::string> sm;  // labels.SelectorFromSet: one requirement per key
  for (uint32_t j = 0; j < c->n_node_selector; j++) sm[S(c->node_selector[j].key)] = S(c->node_selector[j].value);
  for (auto& kv : sm) h.sel.push_back(((int64_t)d.add(kv.first) << 32) | (int64_t)(uint32_t)d.add(kv.second));
  for (uint32_t j = 0; j < c->n_tolerations; j++) {
    const kp_toleration& t = c->tolerations[j];
    const std::string ef = S(t.effect), key = S(t.key), op = S(t.op), val = S(t.value);
    // TolerationsTolerateTaint for {node.kubernetes.io/unschedulable, NoSchedule}
    if ((ef.empty() || ef == "NoSchedule") && (key.empty() || key == "node.kubernetes.io/unschedulable") &&
        (op == "Exists" || ((op.empty() || op == "Equal") && val.empty())))
      h.tol_unsched = 1;
    Tol x;
    if (ef.empty()) x.eff = EFF_ANY;
    else if (ef == "NoSchedule") x.eff = EFF_NOSCHEDULE;
    else if (ef == "NoExecute") x.eff = EFF_NOEXECUTE;
    else continue;
    x.key = key.empty() ? -1 : d.add(key);
    if (op.empty() || op == "Equal") {
      x.op = TOL_EQUAL;
      x.val = d.add(val);
    } else if (op == "Exists") {
      x.op = TOL_EXISTS;
      x.val = -1;
    } else {
      continue;  // Lt/Gt disabled, unknown operators never tolerate
    }
    h.tols.push_back(x);
  }
  // nodeaffinity.NewLazyErrorNodeSelector (nodeaffinity.go:50-67, 155-263): empty
  // terms select nothing and are dropped; a term with a parse error never matches.
  h.has_aff = c->has_node_affinity ? 1 : 0;
  if (!h.has_aff) return;
  for (uint32_t t = 0; t < c->n_node_affinity_terms; t++) {
    const kp_node_selector_term& term = c->node_affinity_terms[t];
    if (term.n_match_expressions == 0 && term.n_match_fields == 0) continue;
    std::vector<NodeReq> rq;
    std::vector<int32_t> vl;
    bool ok = true;
    for (uint32_t q = 0; q < term.n_match_expressions && ok; q++) {  // nodeSelectorRequirementsAsSelector
      const kp_requirement& r = term.match_expressions[q];
      const std::string key = S(r.key), op = S(r.op);
      if (!(op == "In" || op == "NotIn" || op == "Exists" || op == "DoesNotExist" || op == "Gt" || op == "Lt") ||
          !valid_req(key, op, r.values, r.n_values)) {
        ok = false;
        break;
      }
      NodeReq x{};
      x.key = d.add(key);
      if (op == "In" || op == "NotIn") {
        x.op = op == "In" ? NA_IN : NA_NOTIN;
        x.voff = (int32_t)(h.vals.size() + vl.size());
        for (uint32_t j = 0; j < r.n_values; j++) vl.push_back(d.add(S(r.values[j])));
        x.nv = (int32_t)r.n_values;
      } else if (op == "Exists" || op == "DoesNotExist") {
        x.op = op == "Exists" ? NA_EXISTS : NA_DNE;
      } else {
        x.op = op == "Gt" ? NA_GT : NA_LT;
        k8s::parse_int64(S(r.values[0]), &x.x);
      }
      rq.push_back(x);
    }
    for (uint32_t q = 0; q < term.n_match_fields && ok; q++) {  // nodeSelectorRequirementsAsFieldSelector
      const kp_requirement& r = term.match_fields[q];
      const std::string key = S(r.key), op = S(r.op);
      if (!(op == "In" || op == "NotIn") || r.n_values != 1) {
        ok = false;
        break;
      }
      const std::string v = S(r.values[0]);
      NodeReq x{};
      if (key == "metadata.name") {  // extractNodeFields: the only field a node carries
        x.op = op == "In" ? NA_NAME_IN : NA_NAME_NOTIN;
        x.voff = d.add(v);
      } else {  // fields.Set.Get of an absent field is ""
        x.op = ((op == "In") == v.empty()) ? NA_FIELD_TRUE : NA_FIELD_FALSE;
      }
      rq.push_back(x);
    }
    if (!ok) continue;
    h.reqs.insert(h.reqs.end(), rq.begin(), rq.end());
    h.vals.insert(h.vals.end(), vl.begin(), vl.end());
    h.term_off.push_back((int32_t)h.reqs.size());
  }
}
// Device copies of HostNodes and of several claims (one ClaimProg each).
struct DevNodes {
  NodeView v{};
  std::vector<ClaimProg> progs;
  uint32_t *d_flags = nullptr;
  int32_t *d_name = nullptr, *d_loff = nullptr, *d_toff = nullptr, *d_tnt = nullptr, *d_toffs = nullptr,
          *d_vals = nullptr;
  int64_t *d_lbl = nullptr, *d_lint = nullptr, *d_sel = nullptr;
  uint8_t* d_lok = nullptr;
  Tol* d_tols = nullptr;
  NodeReq* d_reqs = nullptr;
  std::vector<int64_t> sel;
  std::vector<Tol> tols;
  std::vector<int32_t> toffs, vals;
  std::vector<NodeReq> reqs;
  std::vector<size_t> o_sel, o_tol, o_toff, o_req, o_val;
  void plan(Arena& ar, const HostNodes& h, const std::vector<HostClaim>& cl) {
    for (auto& c : cl) {
      o_sel.push_back(sel.size());
      o_tol.push_back(tols.size());
      o_toff.push_back(toffs.size());
      o_req.push_back(reqs.size());
      o_val.push_back(vals.size());
      sel.insert(sel.end(), c.sel.begin(), c.sel.end());
      tols.insert(tols.end(), c.tols.begin(), c.tols.end());
      toffs.insert(toffs.end(), c.term_off.begin(), c.term_off.end());
      reqs.insert(reqs.end(), c.reqs.begin(), c.reqs.end());
      vals.insert(vals.end(), c.vals.begin(), c.vals.end());
    }
    ar.add(&d_flags, h.flags.data(), h.flags.size(), 1);
    ar.add(&d_name, h.name.data(), h.name.size(), 1);
    ar.add(&d_loff, h.lbl_off.data(), h.lbl_off.size());
    ar.add(&d_lbl, h.lbl.data(), h.lbl.size(), 1);
    ar.add(&d_lint, h.lbl_int.data(), h.lbl_int.size(), 1);
    ar.add(&d_lok, h.lbl_int_ok.data(), h.lbl_int_ok.size(), 1);
    ar.add(&d_toff, h.tnt_off.data(), h.tnt_off.size());
    ar.add(&d_tnt, h.tnt.data(), h.tnt.size(), 1);
    ar.add(&d_sel, sel.data(), sel.size(), 1);
    ar.add(&d_tols, tols.data(), tols.size(), 1);
    ar.add(&d_toffs, toffs.data(), toffs.size(), 1);
    ar.add(&d_reqs, reqs.data(), reqs.size(), 1);
    ar.add(&d_vals, vals.data(), vals.size(), 1);
  }
  // (after the arena's alloc()) the node view and each claim's program over the sub-buffers
  void views(const std::vector<HostClaim>& cl, uint64_t n) {
    v = NodeView{n, d_flags, d_name, d_loff, d_lbl, d_lint, d_lok, d_toff, d_tnt};
    for (size_t k = 0; k < cl.size(); k++) {
      ClaimProg p{};
      p.sel = d_sel + o_sel[k];
      p.n_sel = (int32_t)cl[k].sel.size();
      p.tols = d_tols + o_tol[k];
      p.n_tols = (int32_t)cl[k].tols.size();
      p.tol_unsched = cl[k].tol_unsched;
      p.has_aff = cl[k].has_aff;
      p.n_terms = (int32_t)cl[k].term_off.size() - 1;
      p.term_off = d_toffs + o_toff[k];
      p.reqs = d_reqs + o_req[k];
      p.vals = d_vals + o_val[k];
      progs.push_back(p);
    }
  }
};
void split128(k8s::i128 v, int64_t* hi, uint64_t* lo) {
  *hi = (int64_t)(v >> 64);
  *lo = (uint64_t)v;
}
}  // namespace

extern "C" {

int kp_model_grades(kp_engine* e, const kp_resource_model* models, uint32_t n_models, const kp_node* nodes,
                    uint64_t n_nodes, int64_t* out_counts) {
  if (!e || (n_models && !models) || (n_nodes && !nodes) || (n_models && !out_counts)) return KP_EINVAL;
  (void)dev::set_device(e->device);
  if (n_models == 0) return KP_OK;  // getAllocatableModelings returns nil
  // modeling.InitSummary (modeling.go:75-102)
  std::vector<std::string> rs_name;
  std::vector<QtyMap> rs_list;
  for (uint32_t g = 0; g < n_models; g++) {
    QtyMap tmp;
    for (uint32_t j = 0; j < models[g].n_ranges; j++) {
      const kp_model_range& it = models[g].ranges[j];
      if (rs_name.size() != models[g].n_ranges) rs_name.push_back(S(it.name));
      k8s::Qty q;
      if (!k8s::parse_quantity(S(it.min), &q)) {
        e->err = "kp_model_grades: unparsable range minimum";
        return KP_EINVAL;
      }
      tmp[S(it.name)] = q;
    }
    rs_list.push_back(tmp);
  }
  if (!rs_name.empty() && rs_name.size() != rs_list[0].size()) {
    e->err = "the number of resourceName is not equal the number of resourceList";
    return KP_EINVAL;
  }
  if (rs_name.empty()) {  // getIndex would index RMs[MaxInt]
    e->err = "kp_model_grades: resource models without ranges";
    return KP_EINVAL;
  }
  const int K = (int)n_models, NR = (int)rs_name.size();
  std::vector<int64_t> mh((size_t)NR * K), vh;
  std::vector<uint64_t> ml((size_t)NR * K), vl;
  for (int r = 0; r < NR; r++)
    for (int g = 0; g < K; g++) {
      auto it = rs_list[g].find(rs_name[r]);
      split128(it == rs_list[g].end() ? (k8s::i128)0 : it->second.nano, &mh[(size_t)r * K + g], &ml[(size_t)r * K + g]);
    }
  // the nodes' available resources, up to the first without pod room
  uint64_t n = 0;
  vh.reserve((size_t)n_nodes * NR);
  vl.reserve((size_t)n_nodes * NR);
  for (; n < n_nodes; n++) {
    QtyMap av;
    if (!node_available(nodes[n], &av)) break;
    for (int r = 0; r < NR; r++) {
      auto it = av.find(rs_name[r]);
      int64_t h;
      uint64_t l;
      split128(it == av.end() ? (k8s::i128)0 : it->second.nano, &h, &l);
      vh.push_back(h);
      vl.push_back(l);
    }
  }
  Arena a;
  int64_t *d_mh, *d_vh;
  uint64_t *d_ml, *d_vl;
  unsigned long long* d_cnt;
  a.add(&d_mh, mh.data(), mh.size());
  a.add(&d_ml, ml.data(), ml.size());
  a.add(&d_vh, vh.data(), vh.size(), 1);
  a.add(&d_vl, vl.data(), vl.size(), 1);
  a.add(&d_cnt, K);
  HIPCHK(a.alloc());
  dev::stream_t st = e->stream;
  HIPCHK(a.upload(st));
  HIPCHK(dev::fill(d_cnt, 0, 8 * (size_t)K, st));
  GradesArgs A{K, NR, d_mh, d_ml, d_vh, d_vl, n, d_cnt};
  HIPCHK(dev::grades(st, A));
  std::vector<unsigned long long> c(K);
  HIPCHK(dev::d2h(c.data(), d_cnt, 8 * (size_t)K, st));
  HIPCHK(dev::sync(st));
  for (int g = 0; g < K; g++) out_counts[g] = (int64_t)c[g];
  return KP_OK;
}

}  // extern "C"

namespace {
// One estimator-server call over a member cluster's nodes: the slots of every
// resource the components (and the Estimate request) name, the nodes' available
// resources in those slots, and a ClaimProg per component (+ the request's claim).
struct NodeJob {
  std::vector<std::string> slot{"pods"};
  NodeSetsArgs A{};
  std::vector<int64_t> avail;
  std::vector<uint32_t> present;
  Dict d;
  HostNodes hn;
  std::vector<HostClaim> cl;
  std::string err;
  int rc = KP_OK;
  static bool divides(const std::string& nm) {
    return nm == "cpu" || nm == "memory" || nm == "ephemeral-storage" || k8s::scalar_resource(nm);
  }
  static int64_t field(const NodeRes& r, const std::string& nm, bool* present) {
    *present = true;
    if (nm == "pods") return r.pods;
    if (nm == "cpu") return r.cpu;
    if (nm == "memory") return r.mem;
    if (nm == "ephemeral-storage") return r.eph;
    auto it = r.sc.find(nm);
    *present = it != r.sc.end();
    return *present ? it->second : 0;
  }
  int fail(int code, const char* m) {
    rc = code;
    err = m;
    return code;
  }
  // phases: the assumed workloads (empty ones skipped), then `main` (may be empty).
  int build(const kp_node* nodes, uint64_t n, const kp_assumed_workload* assumed, uint32_t n_assumed,
            const kp_node_component* main, uint32_t K, const QtyMap* extra) {
    std::vector<const kp_node_component*> comps;
    A.n = n;
    A.mono = 1;
    A.n_phase = 0;
    for (uint32_t w = 0; w < n_assumed; w++) {
      if (assumed[w].n_components == 0) continue;  // noderesource.go:168-170
      if (assumed[w].n_components > (uint32_t)kNodeComp || A.n_phase + 1 >= kNodePhase)
        return fail(KP_ENOTSUP, "more than 16 assumed workloads or 16 components in one");
      A.ph_k0[A.n_phase++] = (int32_t)comps.size();
      for (uint32_t k = 0; k < assumed[w].n_components; k++) comps.push_back(&assumed[w].components[k]);
    }
    if (K) {
      A.ph_k0[A.n_phase++] = (int32_t)comps.size();
      for (uint32_t k = 0; k < K; k++) comps.push_back(&main[k]);
    }
    A.ph_k0[A.n_phase] = (int32_t)comps.size();
    A.last_upper = K ? INT32_MAX : 1;
    if (comps.size() > (size_t)kNodeCompAll) return fail(KP_ENOTSUP, "more than 64 components in all");
    std::vector<NodeRes> creq(comps.size());
    for (size_t k = 0; k < comps.size(); k++) {
      const kp_node_component& c = *comps[k];
      if (!c.has_replica_requirements) continue;
      QtyMap q;
      if (!qmap(c.resource_request, c.n_resource_request, &q)) return fail(KP_EINVAL, "unparsable resource request");
      res_add(creq[k], q);
      for (auto& kv : q)
        if (divides(kv.first) && std::find(slot.begin(), slot.end(), kv.first) == slot.end()) slot.push_back(kv.first);
    }
    if (extra)
      for (auto& kv : *extra)
        if (divides(kv.first) && std::find(slot.begin(), slot.end(), kv.first) == slot.end()) slot.push_back(kv.first);
    if (slot.size() > (size_t)kNodeRes) return fail(KP_ENOTSUP, "more than 7 distinct requested resources");
    A.NU = (int32_t)slot.size();
    for (size_t k = 0; k < comps.size(); k++) {
      A.replicas[k] = comps[k]->replicas;
      if (comps[k]->replicas < 0) A.mono = 0;
      for (int u = 0; u < A.NU; u++) {
        bool pr;
        const int64_t v = u == 0 ? 1 : field(creq[k], slot[u], &pr);
        A.req[k][u] = v;
        A.pos[k][u] = v > 0 ? v : 0;
        if (v < 0) A.mono = 0;
      }
    }
    // getNodesAvailableResources / getNodeAvailableResource (noderesource.go:135-144,205-220)
    avail.assign((size_t)n * A.NU, 0);
    present.assign(n, 0);
    for (uint64_t i = 0; i < n; i++) {
      const kp_node& nd = nodes[i];
      QtyMap al, rqd;
      if (!qmap(nd.allocatable, nd.n_allocatable, &al) || !qmap(nd.requested, nd.n_requested, &rqd))
        return fail(KP_EINVAL, "unparsable node quantity");
      NodeRes a, r;
      res_add(a, al);
      res_add(r, rqd);
      uint32_t pm = 0;
      for (int u = 0; u < A.NU; u++) {
        bool pa, prq;
        const int64_t va = field(a, slot[u], &pa), vr = field(r, slot[u], &prq);
        int64_t x = 0;
        if (u == 0) x = std::max<int64_t>(std::max<int64_t>(va - vr, 0) - (int64_t)nd.n_pods, 0);
        else if (pa) x = prq ? std::max<int64_t>(va - vr, 0) : va;  // SubResource: absent scalars stay absent
        avail[(size_t)i * A.NU + u] = x;
        if (pa) pm |= 1u << u;
      }
      present[i] = pm;
    }
    A.max_steps = A.mono ? 4 * (int64_t)comps.size() * ((int64_t)n + 2) + 64 : (int64_t)1 << 20;
    pack_nodes(nodes, n, d, hn);
    cl.resize(comps.size());
    for (size_t k = 0; k < comps.size(); k++)
      if (comps[k]->has_replica_requirements) compile_claim(comps[k]->node_claim, d, cl[k]);
    return KP_OK;
  }
};
}  // namespace

extern "C" {

// Runs the job's set phases on the device; *sets = the last phase's count. On
// return the job's node state (d_avail) holds the deducted resources.
static int node_job_run(kp_engine* e, NodeJob& J, const kp_node_claim* est_claim, NodeEstArgs* est, int32_t* sets) {
  Arena ar;
  DevNodes dn;
  if (est) J.cl.emplace_back(), compile_claim(est_claim, J.d, J.cl.back());
  dn.plan(ar, J.hn, J.cl);
  const size_t NP = J.cl.size();
  const int KS = J.A.ph_k0[J.A.n_phase];
  ClaimProg* d_progs;
  NodeSetsArgs* d_args;
  int64_t* d_avail;
  uint32_t *d_present, *d_ovf, *d_sum;
  uint8_t* d_match;
  int32_t* d_out;
  ar.add(&d_progs, std::max<size_t>(1, NP));
  ar.add(&d_args, 1);
  ar.add(&d_avail, J.avail.data(), J.avail.size(), 1);
  ar.add(&d_present, J.present.data(), J.present.size(), 1);
  ar.add(&d_match, std::max<size_t>(1, (size_t)KS * J.A.n));
  ar.add(&d_out, 1);
  ar.add(&d_ovf, 1);
  ar.add(&d_sum, 1);
  HIPCHK(ar.alloc());
  dev::stream_t st = e->stream;
  HIPCHK(ar.upload(st));
  dn.views(J.cl, J.A.n);
  J.A.avail = d_avail;
  J.A.present = d_present;
  J.A.match = d_match;
  J.A.out = d_out;
  J.A.ovf = d_ovf;
  // (the claim programs and the arguments hold device pointers, known after alloc(): direct copies)
  if (NP) HIPCHK(dev::h2d(d_progs, dn.progs.data(), sizeof(ClaimProg) * NP, st));
  HIPCHK(dev::h2d(d_args, &J.A, sizeof(J.A), st));
  HIPCHK(dev::fill(d_out, 0, 4, st));
  HIPCHK(dev::fill(d_ovf, 0, 4, st));
  if (KS > 0 && J.A.n > 0) {
    HIPCHK(dev::node_match(st, dn.v, d_progs, KS, d_match));
    HIPCHK(dev::node_sets(st, d_args));
  }
  if (est) {
    HIPCHK(dev::fill(d_sum, 0, 4, st));
    est->v = dn.v;
    est->p = dn.progs.back();
    est->NU = J.A.NU;
    est->avail = d_avail;
    est->sum = d_sum;
    HIPCHK(dev::node_est(st, *est));
  }
  int32_t res = 0;
  uint32_t ovf = 0, sum = 0;
  HIPCHK(dev::d2h(&res, d_out, 4, st));
  HIPCHK(dev::d2h(&ovf, d_ovf, 4, st));
  if (est) HIPCHK(dev::d2h(&sum, d_sum, 4, st));
  HIPCHK(dev::sync(st));
  if (ovf) {
    e->err = "the first-fit simulation exceeded its step bound";
    return KP_ENOTSUP;
  }
  *sets = est ? (int32_t)sum : res;
  return KP_OK;
}

int kp_node_max_replicas(kp_engine* e, const kp_node* nodes, uint64_t n_nodes, const kp_resource* request,
                         uint32_t n_request, const kp_node_claim* claim, const kp_assumed_workload* assumed,
                         uint32_t n_assumed, int32_t* out) {
  if (!e || !out || (n_nodes && !nodes) || (n_request && !request) || (n_assumed && !assumed)) return KP_EINVAL;
  (void)dev::set_device(e->device);
  *out = 0;
  QtyMap rq;
  if (!qmap(request, n_request, &rq)) {
    e->err = "kp_node_max_replicas: unparsable resource request";
    return KP_EINVAL;
  }
  if (n_nodes == 0) return KP_OK;  // estimate.go:43-45
  NodeJob J;
  if (J.build(nodes, n_nodes, assumed, n_assumed, nullptr, 0, &rq) != KP_OK) {
    e->err = "kp_node_max_replicas: " + J.err;
    return J.rc;
  }
  // MaxDivided's dividing entries (resource.go:221-248): cpu milli, memory,
  // ephemeral-storage, scalar resources, each > 0
  NodeEstArgs E{};
  for (auto& kv : rq) {
    const std::string& nm = kv.first;
    if (!NodeJob::divides(nm)) continue;
    const int64_t v = nm == "cpu" ? k8s::milli(kv.second) : k8s::value(kv.second);
    const int u = (int)(std::find(J.slot.begin(), J.slot.end(), nm) - J.slot.begin());
    if (v > 0) E.q[u] = v;
  }
  int32_t sum = 0;
  const int rc = node_job_run(e, J, claim, &E, &sum);
  if (rc != KP_OK) return rc;
  *out = sum;
  return KP_OK;
}

int kp_node_max_component_sets(kp_engine* e, const kp_node* nodes, uint64_t n_nodes,
                               const kp_node_component* comps, uint32_t K, const kp_assumed_workload* assumed,
                               uint32_t n_assumed, int32_t* out) {
  if (!e || !out || (n_nodes && !nodes) || (K && !comps) || (n_assumed && !assumed)) return KP_EINVAL;
  (void)dev::set_device(e->device);
  *out = 0;
  if (K == 0) {  // noNodeConstraint (noderesource.go:155-158)
    *out = INT32_MAX;
    return KP_OK;
  }
  if (K > (uint32_t)kNodeComp) {
    e->err = "kp_node_max_component_sets: more than 16 components";
    return KP_ENOTSUP;
  }
  NodeJob J;
  if (J.build(nodes, n_nodes, assumed, n_assumed, comps, K, nullptr) != KP_OK) {
    e->err = "kp_node_max_component_sets: " + J.err;
    return J.rc;
  }
  if (n_nodes == 0) return KP_OK;  // no node holds a set
  int32_t sets = 0;
  const int rc = node_job_run(e, J, nullptr, nullptr, &sets);
  if (rc != KP_OK) return rc;
  *out = sets;
  return KP_OK;
}

}  // extern "C"
