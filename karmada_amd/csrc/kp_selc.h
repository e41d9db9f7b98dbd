// kp_selc.h — the selector compiler the host units share: util.ClusterMatches of a
// kp_cluster_affinity compiled into a conjunction program (Prog / Instr, kp_layout.h) over a
// snapshot's dictionaries and ranks. The binding packer (pack.cpp, Packer) compiles a
// binding's filter, overflow and static-weight affinities with it; a watch (watch.cpp)
// compiles the one affinity enqueueAffectedBindings reads.
#pragma once
#include "kp_host.h"

namespace kp::host {

// Host-side pools of packed bindings (one packing chunk's; kp_batch has the same five).
// (aligned to two cache lines: the packing threads fill adjacent chunks' pools at once, and
// every push_back writes its vector's end pointer; packed 120-B structs shared lines, and
// 16 threads packed at about a third of the single-thread rate per binding)
struct alignas(128) Pools {
  std::vector<int32_t> ipool;
  std::vector<int64_t> lpool;
  std::vector<Tol> tols;
  std::vector<Prog> progs;
  std::vector<Instr> instrs;
};

struct SelectorCompiler {
  kp_snapshot* s;
  Pools* bt;  // the pools the programs go to (one per packing thread, merged by kp_batch_create)
  // scratch lists reused across affinities (no per-affinity allocation)
  std::vector<Instr> tmp_out;
  std::vector<int32_t> tmp_vals;
  std::vector<std::pair<std::string_view, std::string_view>> tmp_ml;
  // compiled programs by affinity content (a batch repeats a policy's placement across
  // its bindings): the instructions with their list references relative to the lists
  // they own, re-emitted into the pools on a hit
  struct CProg {
    std::vector<Instr> ins;
    std::vector<int32_t> lists;
  };
  SvMap<int32_t> cmemo;
  std::vector<CProg> cprogs;
  std::string ckey;

  int32_t list(const std::vector<int32_t>& v) {
    int32_t off = (int32_t)bt->ipool.size();
    bt->ipool.insert(bt->ipool.end(), v.begin(), v.end());
    return off;
  }
  std::vector<int32_t> ranks(const kp_str* names, uint32_t n) {
    std::vector<int32_t> r;
    for (uint32_t i = 0; i < n; i++) {
      auto it = s->rank_of.find(SV(names[i]));
      if (it != s->rank_of.end()) r.push_back(it->second);
    }
    return r;
  }
  // (the list lives until the next call: callers hand it to list() at once)
  const std::vector<int32_t>& vals(const kp_str* v, uint32_t n) {
    std::vector<int32_t>& r = tmp_vals;
    r.clear();
    for (uint32_t i = 0; i < n; i++) {
      int32_t id = s->str.get(SV(v[i]));
      if (id >= 0) r.push_back(id);
    }
    return r;
  }
  void ins(std::vector<Instr>& out, int32_t op, int32_t a = 0, int32_t b = 0, int32_t c = 0, int64_t v = 0) {
    Instr i;
    i.op = op;
    i.a = a;
    i.b = b;
    i.c = c;
    i.v = v;
    out.push_back(i);
  }
  static bool list_ref_a(int32_t op) { return op == OP_EXCLUDE || op == OP_NAMES; }
  static bool list_ref_b(int32_t op) {
    return op == OP_LBL_IN || op == OP_LBL_NOTIN || op == OP_FLD_IN || op == OP_FLD_NOTIN || op == OP_ZONE_IN ||
           op == OP_ZONE_NOTIN;
  }
  // The affinity's content as a key: every field, strings length-prefixed.
  void affinity_key(const kp_cluster_affinity& a) {
    std::string& k = ckey;
    k.clear();
    auto u32 = [&](uint32_t v) { k.append((const char*)&v, 4); };
    auto str = [&](const kp_str& x) {
      u32(x.len);
      if (x.len) k.append(x.ptr, x.len);
    };
    auto strs = [&](const kp_str* v, uint32_t n) {
      u32(n);
      for (uint32_t i = 0; i < n; i++) str(v[i]);
    };
    auto reqs = [&](const kp_requirement* r, uint32_t n) {
      u32(n);
      for (uint32_t i = 0; i < n; i++) {
        str(r[i].key);
        str(r[i].op);
        strs(r[i].values, r[i].n_values);
      }
    };
    u32(a.has_label_selector);
    u32(a.n_match_labels);
    for (uint32_t i = 0; i < a.n_match_labels; i++) {
      str(a.match_labels[i].key);
      str(a.match_labels[i].value);
    }
    reqs(a.match_expressions, a.n_match_expressions);
    u32(a.has_field_selector);
    reqs(a.field_expressions, a.n_field_expressions);
    strs(a.cluster_names, a.n_cluster_names);
    strs(a.exclude_clusters, a.n_exclude_clusters);
  }
  // util.ClusterMatches compiled to a conjunction program (selector.go:97-155),
  // memoized by content
  int32_t compile(const kp_cluster_affinity& a) {
    affinity_key(a);
    auto it = cmemo.find(std::string_view(ckey));
    if (it != cmemo.end()) {
      const CProg& c = cprogs[it->second];
      const int32_t base = (int32_t)bt->ipool.size();
      bt->ipool.insert(bt->ipool.end(), c.lists.begin(), c.lists.end());
      Prog p;
      p.ins_off = (int32_t)bt->instrs.size();
      p.ins_cnt = (int32_t)c.ins.size();
      for (Instr x : c.ins) {
        if (list_ref_a(x.op)) x.a += base;
        else if (list_ref_b(x.op)) x.b += base;
        bt->instrs.push_back(x);
      }
      bt->progs.push_back(p);
      return (int32_t)bt->progs.size() - 1;
    }
    const int32_t ip0 = (int32_t)bt->ipool.size();
    const int32_t id = compile_new(a);
    if (cprogs.size() < 4096) {
      CProg c;
      const Prog& p = bt->progs[id];
      c.lists.assign(bt->ipool.begin() + ip0, bt->ipool.end());
      c.ins.assign(bt->instrs.begin() + p.ins_off, bt->instrs.begin() + p.ins_off + p.ins_cnt);
      for (Instr& x : c.ins) {
        if (list_ref_a(x.op)) x.a -= ip0;
        else if (list_ref_b(x.op)) x.b -= ip0;
      }
      cmemo.emplace(ckey, (int32_t)cprogs.size());
      cprogs.push_back(std::move(c));
    }
    return id;
  }
  int32_t compile_new(const kp_cluster_affinity& a) {
    std::vector<Instr>& out = tmp_out;
    out.clear();
    bool never = false;
    if (a.n_exclude_clusters) {
      auto r = ranks(a.exclude_clusters, a.n_exclude_clusters);
      if (!r.empty()) ins(out, OP_EXCLUDE, list(r), (int32_t)r.size());
    }
    if (a.has_label_selector) {  // metav1.LabelSelectorAsSelector (helpers.go:36-74)
      // matchLabels as a map: key order, a repeated key's last value
      auto& ml = tmp_ml;
      ml.clear();
      for (uint32_t i = 0; i < a.n_match_labels; i++) {
        const std::string_view k = SV(a.match_labels[i].key), v = SV(a.match_labels[i].value);
        bool dup = false;
        for (auto& kv : ml)
          if (kv.first == k) {
            kv.second = v;
            dup = true;
          }
        if (!dup) ml.push_back({k, v});
      }
      std::sort(ml.begin(), ml.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
      for (auto& kv : ml) {
        kp_str v{kv.second.data(), (uint32_t)kv.second.size()};
        if (!valid_req(kv.first, "=", &v, 1)) never = true;
        int32_t slot = s->keys.get(kv.first);
        int32_t id = s->str.get(kv.second);
        if (slot < 0 || id < 0) never = never || true;
        else {
          tmp_vals.assign(1, id);
          ins(out, OP_LBL_IN, slot, list(tmp_vals), 1);
        }
      }
      for (uint32_t i = 0; i < a.n_match_expressions; i++) {
        const kp_requirement& r = a.match_expressions[i];
        const std::string_view key = SV(r.key), op = SV(r.op);
        if (!(op == "In" || op == "NotIn" || op == "Exists" || op == "DoesNotExist") ||
            !valid_req(key, op, r.values, r.n_values)) {
          never = true;
          continue;
        }
        int32_t slot = s->keys.get(key);
        if (op == "In") {
          const auto& v = vals(r.values, r.n_values);
          if (slot < 0 || v.empty()) never = true;
          else ins(out, OP_LBL_IN, slot, list(v), (int32_t)v.size());
        } else if (op == "NotIn") {
          const auto& v = vals(r.values, r.n_values);
          if (slot >= 0) ins(out, OP_LBL_NOTIN, slot, list(v), (int32_t)v.size());
        } else if (op == "Exists") {
          if (slot < 0) never = true;
          else ins(out, OP_LBL_EXISTS, slot);
        } else if (slot >= 0) {
          ins(out, OP_LBL_DNE, slot);
        }
      }
    }
    if (a.has_field_selector) {
      bool any_other = false;
      bool others_ok = true;
      for (uint32_t i = 0; i < a.n_field_expressions; i++) {
        const kp_requirement& r = a.field_expressions[i];
        const std::string_view key = SV(r.key), op = SV(r.op);
        if (key == "zone") {  // matchZones (selector.go:208-235)
          const auto& v = vals(r.values, r.n_values);
          if (op == "In") ins(out, OP_ZONE_IN, 0, list(v), (int32_t)v.size());
          else if (op == "NotIn") ins(out, OP_ZONE_NOTIN, 0, list(v), (int32_t)v.size());
          else if (op == "Exists") ins(out, OP_ZONE_EXISTS);
          else if (op == "DoesNotExist") ins(out, OP_ZONE_DNE);
          else never = true;
          continue;
        }
        any_other = true;
        // lifted.NodeSelectorRequirementsAsSelector (nodeaffinity.go:36-71)
        if (!(op == "In" || op == "NotIn" || op == "Exists" || op == "DoesNotExist" || op == "Gt" || op == "Lt") ||
            !valid_req(key, op, r.values, r.n_values)) {
          others_ok = false;
          continue;
        }
        int field = key == "provider" ? 0 : (key == "region" ? 1 : 2);  // extractClusterFields
        if (op == "In") {
          const auto& v = vals(r.values, r.n_values);
          if (field == 2 || v.empty()) never = true;
          else ins(out, OP_FLD_IN, field, list(v), (int32_t)v.size());
        } else if (op == "NotIn") {
          const auto& v = vals(r.values, r.n_values);
          if (field != 2) ins(out, OP_FLD_NOTIN, field, list(v), (int32_t)v.size());
        } else if (op == "Exists") {
          if (field == 2) never = true;
          else ins(out, OP_FLD_EXISTS, field);
        } else if (op == "DoesNotExist") {
          if (field != 2) ins(out, OP_FLD_DNE, field);
        } else {
          int64_t x = 0;
          k8s::parse_int64(S(r.values[0]), &x);
          if (field == 2) never = true;
          else ins(out, op == "Gt" ? OP_FLD_GT : OP_FLD_LT, field, 0, 0, x);
        }
      }
      if (any_other && !others_ok) never = true;
    }
    if (a.n_cluster_names) {
      auto r = ranks(a.cluster_names, a.n_cluster_names);
      if (r.empty()) never = true;
      else ins(out, OP_NAMES, list(r), (int32_t)r.size());
    }
    if (never) {
      out.clear();
      ins(out, OP_FALSE);
    }
    Prog p;
    p.ins_off = (int32_t)bt->instrs.size();
    p.ins_cnt = (int32_t)out.size();
    bt->instrs.insert(bt->instrs.end(), out.begin(), out.end());
    bt->progs.push_back(p);
    return (int32_t)bt->progs.size() - 1;
  }
};

}  // namespace kp::host
