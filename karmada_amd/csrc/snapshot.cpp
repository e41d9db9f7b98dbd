// snapshot.cpp — the cluster snapshot: kp_snapshot_create, update, export, import and
// replicate. A member cluster packed into its row, the rows laid out in the snapshot's columns
// and uploaded, and the export bytes' writer and reader. Defines qmap (kp_host.h).
#include "kp_host.h"

// ============================================================================
// Snapshot packing (cache.Snapshot, cache.go:124-139, packed once)
// ============================================================================
namespace kp::host {

bool qmap(const kp_resource* r, uint32_t n, QtyMap* m) {
  bool ok = true;
  for (uint32_t i = 0; i < n; i++) {
    k8s::Qty q;
    if (!k8s::parse_quantity(S(r[i].quantity), &q)) ok = false;
    (*m)[S(r[i].name)] = q;
  }
  return ok;
}

}  // namespace kp::host

namespace {

int upload_snapshot(kp_engine* e, kp_snapshot* s);
int snapshot_est_kind(const kp_snapshot* s);

// One cluster's packed row before it is laid out in the snapshot columns
// (shared by kp_snapshot_create and kp_snapshot_update). Dictionary ids are
// taken with Dict::add: create has filled the dictionaries already (pass 1),
// an update may append to them.
struct ClusterRow {
  uint32_t flags = 0;
  int32_t provider = -1, region = -1;
  int64_t provider_int = 0, region_int = 0;
  std::vector<int32_t> zones;
  std::vector<std::pair<int32_t, int32_t>> labels;  // (key id, value id), later entries win
  std::vector<std::array<int32_t, 3>> taints;       // (key, value, effect), NoSchedule/NoExecute only
  std::vector<int32_t> gvks;
  int64_t allowed = 0;
  std::vector<std::pair<int32_t, int64_t>> avail;   // (resource id, available)
  std::vector<std::pair<int32_t, int64_t>> qa;      // (resource id, quantityAsInt64 availability)
  std::vector<std::pair<int32_t, int64_t>> groups;  // (template id, node count), grades ascending
};

int pack_row(kp_engine* e, kp_snapshot* s, const kp_cluster& c, std::map<std::vector<int64_t>, int32_t>& tmpl_ids,
             ClusterRow* out) {
  ClusterRow& w = *out;
  w = ClusterRow();
  uint32_t f = 0;
  if (c.deleting) f |= CF_DELETING;
  std::string prov = S(c.provider), reg = S(c.region);
  if (!prov.empty()) {
    f |= CF_HAS_PROVIDER;
    w.provider = s->str.add(prov);
    int64_t v;
    if (k8s::parse_int64(prov, &v)) {
      f |= CF_PROVIDER_INT;
      w.provider_int = v;
    }
  }
  if (!reg.empty()) {
    f |= CF_HAS_REGION;
    w.region = s->str.add(reg);
    int64_t v;
    if (k8s::parse_int64(reg, &v)) {
      f |= CF_REGION_INT;
      w.region_int = v;
    }
  }
  if (c.n_zones) f |= CF_HAS_ZONES;
  for (uint32_t i = 0; i < c.n_zones; i++) w.zones.push_back(s->str.add(S(c.zones[i])));
  for (uint32_t i = 0; i < c.n_labels; i++)
    w.labels.push_back({s->keys.add(S(c.labels[i].key)), s->str.add(S(c.labels[i].value))});
  for (uint32_t i = 0; i < c.n_taints; i++) {
    std::string eff = S(c.taints[i].effect);
    int32_t ef = eff == "NoSchedule" ? EFF_NOSCHEDULE : (eff == "NoExecute" ? EFF_NOEXECUTE : 0);
    if (!ef) continue;  // only NoSchedule/NoExecute are filtered (taint_toleration.go:65-67)
    w.taints.push_back({s->str.add(S(c.taints[i].key)), s->str.add(S(c.taints[i].value)), ef});
  }
  for (uint32_t i = 0; i < c.n_api_enablements; i++)
    w.gvks.push_back(s->gvk.add(S(c.api_enablements[i].group_version) + '\0' + S(c.api_enablements[i].kind)));
  if (c.has_resource_summary) {
    f |= CF_HAS_SUMMARY;
    QtyMap al, ad, ag;
    bool ok = qmap(c.allocatable, c.n_allocatable, &al) & qmap(c.allocated, c.n_allocated, &ad) &
              qmap(c.allocating, c.n_allocating, &ag);
    if (!ok) {
      e->err = "unparsable quantity in cluster " + S(c.name);
      return KP_EINVAL;
    }
    auto pods = [](const QtyMap& m) {
      auto it = m.find("pods");
      return it == m.end() ? 0 : k8s::value(it->second);
    };
    int64_t allowed = pods(al) - pods(ad) - pods(ag);  // getAllowedPodNumber (general.go:445-463)
    w.allowed = allowed > 0 ? allowed : 0;
    for (auto& kv : al) {  // getMaximumReplicasBasedOnClusterSummary operands (general.go:465-505)
      k8s::Qty q = kv.second;
      auto x = ad.find(kv.first);
      if (x != ad.end()) q.nano -= x->second.nano;
      x = ag.find(kv.first);
      if (x != ag.end()) q.nano -= x->second.nano;
      int64_t v = k8s::value(q);
      int64_t d = v <= 0 ? 0 : (kv.first == "cpu" ? k8s::milli(q) : v);
      w.avail.push_back({s->res.add(kv.first), d});
      // availableResourceMap (general.go:403-415): Sub keeps the allocatable's format
      k8s::Qty a = kv.second;
      if ((x = ad.find(kv.first)) != ad.end()) k8s::qsub(a, x->second);
      if ((x = ag.find(kv.first)) != ag.end()) k8s::qsub(a, x->second);
      w.qa.push_back({s->res.add(kv.first), k8s::as_int64(a)});
    }
    // buildModelNodes (general.go:296-361)
    if (s->opts.customized_cluster_resource_modeling && c.n_allocatable_modelings > 0 && c.n_resource_models > 0) {
      bool neg = false;
      std::map<uint32_t, int64_t> cnt;
      for (uint32_t i = 0; i < c.n_allocatable_modelings; i++) {
        if (c.allocatable_modelings[i].count < 0) neg = true;
        cnt[c.allocatable_modelings[i].grade] += c.allocatable_modelings[i].count;
      }
      if (!neg) {
        std::map<uint32_t, std::map<int32_t, int64_t>> caps;  // grade -> (resource id -> min)
        for (uint32_t m = 0; m < c.n_resource_models; m++) {
          QtyMap rl;
          for (uint32_t j = 0; j < c.resource_models[m].n_ranges; j++) {
            k8s::Qty q;
            if (!k8s::parse_quantity(S(c.resource_models[m].ranges[j].min), &q)) {
              e->err = "unparsable resource model quantity";
              return KP_EINVAL;
            }
            rl[S(c.resource_models[m].ranges[j].name)] = q;
          }
          std::map<int32_t, int64_t> t;
          for (auto& kv : rl) {  // util.NewResource (resource.go:46-75); pods forced to 110
            const std::string& nm = kv.first;
            int32_t rid = s->res.add(nm);
            if (nm == "cpu") t[rid] += k8s::milli(kv.second);
            else if (nm == "memory" || nm == "ephemeral-storage") t[rid] += k8s::value(kv.second);
            else if (nm == "pods") continue;
            else if (k8s::scalar_resource(nm)) t[rid] += k8s::value(kv.second);
          }
          caps[c.resource_models[m].grade] = t;
        }
        const int R = (int)s->res.names.size();
        for (auto& kv : caps) {  // grades ascending
          auto it = cnt.find(kv.first);
          int64_t k = it == cnt.end() ? 0 : it->second;
          if (k == 0) continue;
          std::vector<int64_t> t(R, 0);
          for (auto& rv : kv.second) t[rv.first] = rv.second;
          while (!t.empty() && t.back() == 0) t.pop_back();  // key independent of the resource count
          auto ti = tmpl_ids.find(t);
          int32_t tid;
          if (ti == tmpl_ids.end()) {
            tid = (int32_t)tmpl_ids.size();
            tmpl_ids.emplace(t, tid);
          } else {
            tid = ti->second;
          }
          w.groups.push_back({tid, k});
        }
        f |= CF_MODEL_OK;
      }
    }
  }
  w.flags = f;
  return KP_OK;
}

// Lays rows[0..C) (rank order) out in the snapshot's columns and derived arrays.
void apply_rows(kp_snapshot* s, const std::vector<ClusterRow>& rows,
                const std::map<std::vector<int64_t>, int32_t>& tmpl_ids) {
  const int C = s->C, Cp = s->Cp;
  const int K = (int)s->keys.names.size(), AW = ((int)s->gvk.names.size() + 63) / 64, R = (int)s->res.names.size();
  // regions in name order (region_idx); an update may have added names
  std::vector<std::string> regs;
  for (int r = 0; r < C; r++)
    if (rows[r].region >= 0) regs.push_back(s->str.names[rows[r].region]);
  std::sort(regs.begin(), regs.end());
  regs.erase(std::unique(regs.begin(), regs.end()), regs.end());
  s->regions = Dict();
  for (auto& r : regs) s->regions.add(r);
  s->flags.assign(Cp, 0);
  s->provider.assign(Cp, -1);
  s->region.assign(Cp, -1);
  s->region_idx.assign(Cp, -1);
  s->provider_int.assign(Cp, 0);
  s->region_int.assign(Cp, 0);
  s->label_val.assign((size_t)std::max(K, 1) * Cp, -1);
  s->api_bits.assign((size_t)std::max(AW, 1) * Cp, 0);
  s->allowed.assign(Cp, 0);
  s->avail.assign((size_t)std::max(R, 1) * Cp, 0);
  s->qa.assign((size_t)std::max(R, 1) * Cp, kQaAbsent);
  s->zone_off.assign(C + 1, 0);
  s->taint_off.assign(C + 1, 0);
  s->mgrp_off.assign(C + 1, 0);
  s->zone_ids.clear();
  s->taint_key.clear();
  s->taint_val.clear();
  s->taint_eff.clear();
  s->mgrp_tid.clear();
  s->mgrp_cnt.clear();
  for (int r = 0; r < C; r++) {
    const ClusterRow& w = rows[r];
    s->flags[r] = w.flags;
    s->provider[r] = w.provider;
    s->provider_int[r] = w.provider_int;
    s->region[r] = w.region;
    s->region_int[r] = w.region_int;
    if (w.region >= 0) s->region_idx[r] = s->regions.get(s->str.names[w.region]);
    for (int32_t z : w.zones) s->zone_ids.push_back(z);
    s->zone_off[r + 1] = (int32_t)s->zone_ids.size();
    for (auto& kv : w.labels) s->label_val[(size_t)kv.first * Cp + r] = kv.second;  // map semantics: later wins
    for (auto& t : w.taints) {
      s->taint_key.push_back(t[0]);
      s->taint_val.push_back(t[1]);
      s->taint_eff.push_back(t[2]);
    }
    s->taint_off[r + 1] = (int32_t)s->taint_key.size();
    for (int32_t g : w.gvks) s->api_bits[(size_t)(g >> 6) * Cp + r] |= 1ull << (g & 63);
    s->allowed[r] = w.allowed;
    for (auto& kv : w.avail) s->avail[(size_t)kv.first * Cp + r] = kv.second;
    for (auto& kv : w.qa) s->qa[(size_t)kv.first * Cp + r] = kv.second;
    for (auto& g : w.groups) {
      s->mgrp_tid.push_back(g.first);
      s->mgrp_cnt.push_back(g.second);
    }
    s->mgrp_off[r + 1] = (int32_t)s->mgrp_tid.size();
  }
  s->n_tmpl = (int)tmpl_ids.size();
  s->tmpl.assign((size_t)std::max(s->n_tmpl, 1) * std::max(R, 1), 0);
  for (auto& kv : tmpl_ids)  // (vectors of an earlier, shorter resource list read as zero-padded)
    for (int j = 0; j < R && j < (int)kv.first.size(); j++) s->tmpl[(size_t)kv.second * R + j] = kv.first[j];
  auto pad1 = [](auto& v) {
    if (v.empty()) v.resize(1);
  };
  pad1(s->zone_ids);
  pad1(s->taint_key);
  pad1(s->taint_val);
  pad1(s->taint_eff);
  // model groups transposed to [kmax][Cp] so a wave reads 64 clusters' k-th group coalesced
  int& kmax = s->kmax;
  kmax = 0;
  for (int r = 0; r < C; r++) kmax = std::max(kmax, s->mgrp_off[r + 1] - s->mgrp_off[r]);
  s->mg_tid.assign((size_t)std::max(kmax, 1) * Cp, 0);
  s->mg_cnt.assign((size_t)std::max(kmax, 1) * Cp, 0);
  for (int r = 0; r < C; r++)
    for (int g = s->mgrp_off[r]; g < s->mgrp_off[r + 1]; g++) {
      size_t k = (size_t)(g - s->mgrp_off[r]);
      s->mg_tid[k * Cp + r] = s->mgrp_tid[g];
      s->mg_cnt[k * Cp + r] = (int32_t)std::min<int64_t>(s->mgrp_cnt[g], kInt32Max);
    }
}

int build_snapshot(kp_engine* e, const kp_cluster* cl, uint64_t n, const kp_options* o, kp_snapshot* s) {
  s->opts = o ? *o : kp_options{0, 1, 0, KP_PLUGIN_ALL};
  if (n > (uint64_t)kMaxClusters) {
    e->err = "too many clusters";
    return KP_ENOTSUP;
  }
  const int C = (int)n;
  s->C = C;
  s->Cp = ((C + 63) / 64) * 64;
  if (s->Cp == 0) s->Cp = 64;
  s->W = s->Cp / 64;
  std::vector<uint32_t> order(C);
  std::vector<std::string> names(C);
  for (int i = 0; i < C; i++) {
    order[i] = i;
    names[i] = S(cl[i].name);
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
  s->perm = order;
  s->inv.assign(C, -1);
  for (int r = 0; r < C; r++) {
    s->inv[order[r]] = r;
    if (!s->rank_of.emplace(names[order[r]], r).second) {
      e->err = "duplicate cluster name " + names[order[r]];
      return KP_EINVAL;
    }
  }
  // pass 1: dictionaries
  for (int r = 0; r < C; r++) {
    const kp_cluster& c = cl[order[r]];
    for (uint32_t i = 0; i < c.n_labels; i++) {
      s->keys.add(S(c.labels[i].key));
      s->str.add(S(c.labels[i].value));
    }
    s->str.add(S(c.provider));
    s->str.add(S(c.region));
    for (uint32_t i = 0; i < c.n_zones; i++) s->str.add(S(c.zones[i]));
    for (uint32_t i = 0; i < c.n_taints; i++) {
      s->str.add(S(c.taints[i].key));
      s->str.add(S(c.taints[i].value));
    }
    for (uint32_t i = 0; i < c.n_api_enablements; i++)
      s->gvk.add(S(c.api_enablements[i].group_version) + '\0' + S(c.api_enablements[i].kind));
    for (uint32_t i = 0; i < c.n_allocatable; i++) s->res.add(S(c.allocatable[i].name));
    for (uint32_t m = 0; m < c.n_resource_models; m++)
      for (uint32_t j = 0; j < c.resource_models[m].n_ranges; j++) s->res.add(S(c.resource_models[m].ranges[j].name));
  }
  s->rid_cpu = s->res.add("cpu");
  s->rid_mem = s->res.add("memory");
  s->rid_eph = s->res.add("ephemeral-storage");
  std::map<std::vector<int64_t>, int32_t> tmpl_ids;
  std::vector<ClusterRow> rows(C);
  for (int r = 0; r < C; r++) {
    int rc = pack_row(e, s, cl[order[r]], tmpl_ids, &rows[r]);
    if (rc) return rc;
  }
  apply_rows(s, rows, tmpl_ids);
  s->names.resize(C);
  for (int r = 0; r < C; r++) s->names[r] = names[order[r]];
  return upload_snapshot(e, s);
}

// Device copy of a packed snapshot (kp_snapshot_create and kp_snapshot_import).
int upload_snapshot(kp_engine* e, kp_snapshot* s) {
  const int C = s->C, Cp = s->Cp, kmax = s->kmax;
  const int K = (int)s->keys.names.size(), AW = ((int)s->gvk.names.size() + 63) / 64,
            R = (int)s->res.names.size();
  SnapView& v = s->view;
  v = SnapView{};  // (an update uploads again: the optional tables start out null)
  v.C = C;
  v.Cp = Cp;
  v.W = s->W;
  v.n_label_keys = K;
  v.api_words = AW;
  v.n_res = R;
  v.n_tmpl = s->n_tmpl;
  v.n_regions = (int)s->regions.names.size();
  Arena& a = s->dev;
  // taint lists deduplicated: one TaintToleration answer per distinct list and binding
  std::vector<int32_t> tset(Cp, 0), trep;
  {
    std::map<std::vector<int32_t>, int32_t> ids;
    std::vector<int32_t> key;
    for (int r = 0; r < C; r++) {
      key.clear();
      for (int t = s->taint_off[r]; t < s->taint_off[r + 1]; t++) {
        key.push_back(s->taint_key[t]);
        key.push_back(s->taint_val[t]);
        key.push_back(s->taint_eff[t]);
      }
      auto it = ids.find(key);
      if (it == ids.end()) {
        it = ids.emplace(key, (int32_t)trep.size()).first;
        trep.push_back(r);
      }
      tset[r] = it->second;
    }
    if (trep.empty()) trep.push_back(0);
  }
  // FitError diagnosis: one id per distinct (key, value, effect) triple, i.e. per distinct
  // taint text, and the taint_ref that names it: the lowest caller cluster index that carries
  // the triple with its first position there. Ids are numbered in taint_ref order, so a
  // binding's taint bins come out of the dense histogram rows already sorted.
  std::vector<int32_t> tuid(s->taint_key.size(), 0);
  std::vector<uint32_t> uref;
  if (!tuid.empty()) {
    std::map<std::array<int32_t, 3>, uint32_t> ref_of;
    auto triple = [&](int t) { return std::array<int32_t, 3>{s->taint_key[t], s->taint_val[t], s->taint_eff[t]}; };
    for (int i = 0; i < C; i++) {
      const int r = s->inv[i];
      for (int t = s->taint_off[r]; t < s->taint_off[r + 1]; t++)
        ref_of.emplace(triple(t), (uint32_t)i | (uint32_t)(t - s->taint_off[r]) << kTaintRefShift);
    }
    for (auto& kv : ref_of) uref.push_back(kv.second);
    std::sort(uref.begin(), uref.end());
    for (size_t t = 0; t < tuid.size(); t++)
      tuid[t] = (int32_t)(std::lower_bound(uref.begin(), uref.end(), ref_of[triple((int)t)]) - uref.begin());
  }
  // Cluster bitsets of the filter predicates (kp_filter.h; SnapView::bits).
  std::vector<uint64_t> bits, bkey;
  std::vector<int32_t> bval;
  int32_t n_bits = 0, br_api = 0, br_tset = 0, br_lex = 0;
  const int W = s->W;
  if (W > 0 && (int)trep.size() <= kTsetRowsMax) {
    const int G = (int)s->gvk.names.size();
    std::unordered_map<uint64_t, int32_t> row_of;
    std::vector<std::pair<uint64_t, int32_t>> order;  // (key, cluster) in row-assignment order
    br_api = BR_FIXED;
    br_tset = br_api + G;
    br_lex = br_tset + (int)trep.size();
    int32_t next = br_lex + K;
    auto key_row = [&](uint64_t key) {
      auto it = row_of.find(key);
      if (it != row_of.end()) return it->second;
      row_of.emplace(key, next);
      return next++;
    };
    std::vector<std::pair<int32_t, int>> sets;  // (row, cluster) of the hashed rows
    for (int k = 0; k < K; k++)
      for (int r = 0; r < C; r++) {
        const int32_t v = s->label_val[(size_t)k * Cp + r];
        if (v >= 0) sets.push_back({key_row(bits_key(BK_LABEL, (uint32_t)k, v)), r});
      }
    for (int r = 0; r < C; r++) {
      if (s->provider[r] >= 0) sets.push_back({key_row(bits_key(BK_PROVIDER, 0, s->provider[r])), r});
      if (s->region[r] >= 0) sets.push_back({key_row(bits_key(BK_REGION, 0, s->region[r])), r});
      for (int z = s->zone_off[r]; z < s->zone_off[r + 1]; z++)
        sets.push_back({key_row(bits_key(BK_ZONE, 0, s->zone_ids[z])), r});
    }
    // within budget: the rows stay a small fraction of HBM even at large C
    if ((uint64_t)next * (uint64_t)W * 8 <= ((uint64_t)256 << 20)) {
      n_bits = next;
      bits.assign((size_t)n_bits * W, 0);
      auto set = [&](int32_t row, int r) { bits[(size_t)row * W + (r >> 6)] |= 1ull << (r & 63); };
      for (int r = 0; r < C; r++) {
        const uint32_t f = s->flags[r];
        if (!(f & CF_DELETING)) set(BR_BASE, r);
        if (f & CF_HAS_PROVIDER) set(BR_HAS_PROVIDER, r);
        if (f & CF_HAS_REGION) set(BR_HAS_REGION, r);
        if (f & CF_HAS_ZONES) set(BR_HAS_ZONES, r);
        if (s->provider[r] >= 0) set(BR_PROV_SET, r);
        if (s->region[r] >= 0) set(BR_REG_SET, r);
        if (s->zone_off[r + 1] > s->zone_off[r]) set(BR_ZONE_ANY, r);
        for (int g = 0; g < G; g++)
          if ((s->api_bits[(size_t)(g >> 6) * Cp + r] >> (g & 63)) & 1ull) set(br_api + g, r);
        set(br_tset + tset[r], r);
        for (int k = 0; k < K; k++)
          if (s->label_val[(size_t)k * Cp + r] >= 0) set(br_lex + k, r);
      }
      for (auto& x : sets) set(x.first, x.second);
      size_t tsz = 16;
      while (tsz < 2 * row_of.size()) tsz <<= 1;
      bkey.assign(tsz, kBitsEmpty);
      bval.assign(tsz, -1);
      for (auto& kv : row_of) {
        uint32_t i = bits_hash(kv.first) & (uint32_t)(tsz - 1);
        while (bkey[i] != kBitsEmpty) i = (i + 1) & (uint32_t)(tsz - 1);
        bkey[i] = kv.first;
        bval[i] = kv.second;
      }
    }
  }
  // model node counts per (template, cluster): the fast estimator's dense form
  std::vector<int32_t> mt;
  {
    bool dense = s->n_tmpl > 0 && s->n_tmpl <= kTmplDense;
    for (int64_t x : s->tmpl) dense = dense && x >= 0;
    if (dense) {
      std::vector<int64_t> acc((size_t)kTmplDense * Cp, 0);  // rows past n_tmpl stay zero
      for (int k = 0; k < kmax; k++)
        for (int r = 0; r < C; r++) {
          const int32_t cnt = s->mg_cnt[(size_t)k * Cp + r];
          if (cnt) acc[(size_t)s->mg_tid[(size_t)k * Cp + r] * Cp + r] += cnt;
        }
      mt.resize(acc.size());
      for (size_t i = 0; i < acc.size(); i++) mt[i] = (int32_t)std::min<int64_t>(acc[i], kInt32Max);
    }
  }
  std::vector<uint32_t> permp(Cp, 0);
  for (int r = 0; r < C; r++) permp[r] = s->perm[r];
  a.add(&v.flags, s->flags.data(), Cp);
  a.add(&v.taint_set, tset.data(), Cp);
  a.add(&v.tset_rep, trep.data(), trep.size());
  if (!mt.empty()) a.add(&v.mt_cnt, mt.data(), mt.size());
  a.add(&v.perm, permp.data(), Cp);
  a.add(&v.provider, s->provider.data(), Cp);
  a.add(&v.region, s->region.data(), Cp);
  a.add(&v.region_idx, s->region_idx.data(), Cp);
  a.add(&v.zone_off, s->zone_off.data(), C + 1);
  a.add(&v.zone_ids, s->zone_ids.data(), s->zone_ids.size());
  a.add(&v.label_val, s->label_val.data(), s->label_val.size());
  a.add(&v.taint_off, s->taint_off.data(), C + 1);
  a.add(&v.taint_key, s->taint_key.data(), s->taint_key.size());
  a.add(&v.taint_val, s->taint_val.data(), s->taint_val.size());
  a.add(&v.taint_eff, s->taint_eff.data(), s->taint_eff.size());
  if (!tuid.empty()) {
    a.add(&v.taint_uid, tuid.data(), tuid.size());
    a.add(&v.uid_ref, uref.data(), uref.size());
  }
  a.add(&v.mg_tid, s->mg_tid.data(), s->mg_tid.size());
  a.add(&v.mg_cnt, s->mg_cnt.data(), s->mg_cnt.size());
  a.add(&v.provider_int, s->provider_int.data(), Cp);
  a.add(&v.region_int, s->region_int.data(), Cp);
  a.add(&v.allowed, s->allowed.data(), Cp);
  a.add(&v.avail, s->avail.data(), s->avail.size());
  a.add(&v.qa, s->qa.data(), s->qa.size());
  a.add(&v.tmpl, s->tmpl.data(), s->tmpl.size());
  a.add(&v.api_bits, s->api_bits.data(), s->api_bits.size());
  if (n_bits) {
    a.add(&v.bits, bits.data(), bits.size());
    a.add(&v.bkey, bkey.data(), bkey.size());
    a.add(&v.bval, bval.data(), bval.size());
  }
  HIPCHK(a.alloc());
  HIPCHK(a.upload(e->stream));
  HIPCHK(dev::sync(e->stream));
  v.n_tsets = (int32_t)trep.size();
  v.n_taint_uid = (int32_t)uref.size();
  v.kmax = kmax;
  v.n_bits = n_bits;
  v.br_api = br_api;
  v.br_tset = br_tset;
  v.br_lex = br_lex;
  v.bmask = n_bits ? (uint32_t)(bkey.size() - 1) : 0u;
  s->est_kind = snapshot_est_kind(s);
  return KP_OK;
}

int snapshot_est_kind(const kp_snapshot* s) {
  if (md_cap_of(s) == 0 || s->view.n_tsets > kTsetMax || (s->n_tmpl > 0 && !s->view.mt_cnt)) return EST_GENERIC;
  // which estimator paths the snapshot's clusters can take
  bool any_model = false, any_summary_only = false;
  for (int r = 0; r < s->C; r++) {
    const uint32_t f = s->flags[r];
    if (f & CF_MODEL_OK) any_model = true;
    else if (f & CF_HAS_SUMMARY) any_summary_only = true;
  }
  if (!any_model) return EST_SUMMARY;
  if (!any_summary_only) return s->n_tmpl <= 8 ? EST_MODEL8 : EST_MODEL16;
  return EST_MIXED;
}

}  // namespace

// Packed-snapshot bytes: pack once on one rank, broadcast the bytes, import on
// the others. Host-endian; same engine build on every rank.
namespace {
const char kSnapMagic[8] = {'K', 'P', 'S', 'N', 'A', 'P', '0', '4'};
struct Wr {
  std::vector<unsigned char>& b;
  void raw(const void* p, size_t n) { b.insert(b.end(), (const unsigned char*)p, (const unsigned char*)p + n); }
  void u64(uint64_t x) { raw(&x, 8); }
  void str(const std::string& x) {
    u64(x.size());
    raw(x.data(), x.size());
  }
  void strs(const std::vector<std::string>& v) {
    u64(v.size());
    for (auto& x : v) str(x);
  }
  template <class T>
  void vec(const std::vector<T>& v) {
    u64(v.size());
    raw(v.data(), v.size() * sizeof(T));
  }
};
struct Rd {
  const unsigned char* p;
  const unsigned char* end;
  bool ok = true;
  bool raw(void* d, size_t n) {
    if ((size_t)(end - p) < n) return ok = false;
    memcpy(d, p, n);
    p += n;
    return true;
  }
  uint64_t u64() {
    uint64_t x = 0;
    raw(&x, 8);
    return x;
  }
  std::string str() {
    uint64_t n = u64();
    if (!ok || (size_t)(end - p) < n) {
      ok = false;
      return {};
    }
    std::string x((const char*)p, n);
    p += n;
    return x;
  }
  std::vector<std::string> strs() {
    uint64_t n = u64();
    std::vector<std::string> v;
    for (uint64_t i = 0; ok && i < n; i++) v.push_back(str());
    return v;
  }
  template <class T>
  std::vector<T> vec() {
    uint64_t n = u64();
    std::vector<T> v;
    if (!ok || n > (uint64_t)(end - p) / sizeof(T)) {
      ok = false;
      return v;
    }
    v.resize(n);
    raw(v.data(), n * sizeof(T));
    return v;
  }
};
void dict_from(Dict& d, const std::vector<std::string>& names) {
  for (auto& n : names) d.add(n);
}

// Every column of an imported snapshot against the sizes and id ranges the
// kernels and kp_snapshot_update index with (a foreign or corrupt image must
// fail here, not fault in a kernel).
bool snapshot_consistent(const kp_snapshot* s) {
  const int C = s->C;
  if (C < 0 || C > kMaxClusters) return false;
  const size_t Cp = (size_t)s->Cp, C1 = (size_t)C + 1;
  const int K = (int)s->keys.names.size(), AW = ((int)s->gvk.names.size() + 63) / 64, R = (int)s->res.names.size();
  const int NS = (int)s->str.names.size(), NR = (int)s->regions.names.size(), T = s->n_tmpl, km = s->kmax;
  if ((int)s->names.size() != C || s->perm.size() != (size_t)C || T < 0 || km < 0) return false;
  if (s->str.names.size() != s->str.m.size() || s->keys.names.size() != s->keys.m.size() ||
      s->gvk.names.size() != s->gvk.m.size() || s->res.names.size() != s->res.m.size() ||
      s->regions.names.size() != s->regions.m.size())
    return false;  // duplicate dictionary entries
  for (int r = 1; r < C; r++)
    if (!(s->names[r - 1] < s->names[r])) return false;  // ranks are name order, names unique
  std::vector<char> seen(C, 0);
  for (uint32_t p : s->perm) {
    if (p >= (uint32_t)C || seen[p]) return false;
    seen[p] = 1;
  }
  for (size_t n : {s->flags.size(), s->provider.size(), s->region.size(), s->region_idx.size(),
                   s->provider_int.size(), s->region_int.size(), s->allowed.size()})
    if (n != Cp) return false;
  if (s->label_val.size() != (size_t)std::max(K, 1) * Cp || s->api_bits.size() != (size_t)std::max(AW, 1) * Cp ||
      s->avail.size() != (size_t)std::max(R, 1) * Cp || s->qa.size() != (size_t)std::max(R, 1) * Cp || s->tmpl.size() != (size_t)std::max(T, 1) * std::max(R, 1) ||
      s->mg_tid.size() != (size_t)std::max(km, 1) * Cp || s->mg_cnt.size() != s->mg_tid.size())
    return false;
  if (s->taint_val.size() != s->taint_key.size() || s->taint_eff.size() != s->taint_key.size() ||
      s->mgrp_cnt.size() != s->mgrp_tid.size())
    return false;
  auto offsets_ok = [&](const std::vector<int32_t>& off, size_t pool) {
    if (off.size() != C1 || off[0] != 0 || (size_t)off[C] > pool) return false;
    for (int r = 0; r < C; r++)
      if (off[r + 1] < off[r]) return false;
    return true;
  };
  if (!offsets_ok(s->zone_off, s->zone_ids.size()) || !offsets_ok(s->taint_off, s->taint_key.size()) ||
      !offsets_ok(s->mgrp_off, s->mgrp_tid.size()))
    return false;
  int kmax = 0;
  for (int r = 0; r < C; r++) kmax = std::max(kmax, s->mgrp_off[r + 1] - s->mgrp_off[r]);
  if (kmax != km) return false;
  auto ids_ok = [](const std::vector<int32_t>& v, int lo, int hi) {
    for (int32_t x : v)
      if (x < lo || x >= hi) return false;
    return true;
  };
  if (!ids_ok(s->provider, -1, NS) || !ids_ok(s->region, -1, NS) || !ids_ok(s->region_idx, -1, std::max(NR, 1)) ||
      !ids_ok(s->label_val, -1, NS) || !ids_ok(s->zone_ids, 0, std::max(NS, 1)) ||
      !ids_ok(s->taint_key, 0, std::max(NS, 1)) || !ids_ok(s->taint_val, 0, std::max(NS, 1)) ||
      !ids_ok(s->taint_eff, 0, 4) || !ids_ok(s->mgrp_tid, 0, std::max(T, 1)) || !ids_ok(s->mg_tid, 0, std::max(T, 1)))
    return false;
  for (int32_t x : s->mg_cnt)
    if (x < 0) return false;
  for (int64_t x : s->mgrp_cnt)
    if (x < 0) return false;
  return s->rid_cpu >= 0 && s->rid_cpu < R && s->rid_mem >= 0 && s->rid_mem < R && s->rid_eph >= 0 && s->rid_eph < R;
}
}  // namespace

extern "C" {

int kp_snapshot_create(kp_engine* e, const kp_cluster* clusters, uint64_t n, const kp_options* opts,
                       kp_snapshot** out) {
  if (!e || !out || (n && !clusters)) return KP_EINVAL;
  (void)dev::set_device(e->device);
  auto* s = new kp_snapshot();
  s->e = e;
  int rc = build_snapshot(e, clusters, n, opts, s);
  if (rc != KP_OK) {
    delete s;
    return rc;
  }
  *out = s;
  return KP_OK;
}

void kp_snapshot_destroy(kp_snapshot* s) { delete s; }

namespace {
// Rank r's packed row read back from the snapshot's host columns (the inverse
// of apply_rows), for the clusters an update leaves as they are.
ClusterRow row_of(const kp_snapshot* s, int r) {
  ClusterRow w;
  const int Cp = s->Cp;
  const int K = (int)s->keys.names.size(), AW = ((int)s->gvk.names.size() + 63) / 64, R = (int)s->res.names.size();
  w.flags = s->flags[r];
  w.provider = s->provider[r];
  w.provider_int = s->provider_int[r];
  w.region = s->region[r];
  w.region_int = s->region_int[r];
  for (int z = s->zone_off[r]; z < s->zone_off[r + 1]; z++) w.zones.push_back(s->zone_ids[z]);
  for (int k = 0; k < K; k++) {
    const int32_t v = s->label_val[(size_t)k * Cp + r];
    if (v >= 0) w.labels.push_back({k, v});
  }
  for (int t = s->taint_off[r]; t < s->taint_off[r + 1]; t++)
    w.taints.push_back({s->taint_key[t], s->taint_val[t], s->taint_eff[t]});
  for (int wd = 0; wd < AW; wd++) {
    uint64_t bits = s->api_bits[(size_t)wd * Cp + r];
    while (bits) {
      const int b = __builtin_ctzll(bits);
      w.gvks.push_back(wd * 64 + b);
      bits &= bits - 1;
    }
  }
  w.allowed = s->allowed[r];
  for (int j = 0; j < R; j++) {
    const int64_t a = s->avail[(size_t)j * Cp + r];
    if (a != 0) w.avail.push_back({j, a});
    const int64_t q = s->qa[(size_t)j * Cp + r];
    if (q != kQaAbsent) w.qa.push_back({j, q});
  }
  for (int g = s->mgrp_off[r]; g < s->mgrp_off[r + 1]; g++) w.groups.push_back({s->mgrp_tid[g], s->mgrp_cnt[g]});
  return w;
}
}  // namespace

int kp_snapshot_update(kp_engine* e, kp_snapshot* s, const kp_cluster* clusters, uint64_t n, int* dict_grew) {
  if (!e || !s || (n && !clusters)) return KP_EINVAL;
  (void)dev::set_device(e->device);
  const int C = s->C;
  std::vector<int64_t> upd(C, -1);
  for (uint64_t i = 0; i < n; i++) {
    const std::string name = S(clusters[i].name);
    auto it = s->rank_of.find(name);
    if (it == s->rank_of.end()) {
      e->err = "kp_snapshot_update: no cluster named " + name + " in the snapshot (re-create it to add clusters)";
      return KP_EINVAL;
    }
    if (upd[it->second] >= 0) {
      e->err = "kp_snapshot_update: cluster " + name + " listed twice";
      return KP_EINVAL;
    }
    upd[it->second] = (int64_t)i;
  }
  const size_t n_str = s->str.names.size(), n_keys = s->keys.names.size(), n_gvk = s->gvk.names.size(),
               n_res = s->res.names.size();
  const std::vector<std::string> regions0 = s->regions.names;
  std::vector<ClusterRow> rows(C);
  for (int r = 0; r < C; r++)
    if (upd[r] < 0) rows[r] = row_of(s, r);
  // the snapshot's templates by value (trailing zeros dropped, as pack_row keys them)
  std::map<std::vector<int64_t>, int32_t> tmpl_ids;
  std::vector<std::vector<int64_t>> tv(s->n_tmpl);
  {
    const int R0 = (int)n_res;
    for (int t = 0; t < s->n_tmpl; t++) {
      std::vector<int64_t> v(s->tmpl.begin() + (size_t)t * R0, s->tmpl.begin() + (size_t)(t + 1) * R0);
      while (!v.empty() && v.back() == 0) v.pop_back();
      tmpl_ids.emplace(v, t);
      tv[t] = v;
    }
  }
  for (int r = 0; r < C; r++)
    if (upd[r] >= 0) {
      const int rc = pack_row(e, s, clusters[upd[r]], tmpl_ids, &rows[r]);
      if (rc) return rc;  // columns untouched (the dictionaries may hold unused entries)
    }
  // templates still in use, renumbered in first-use order
  tv.resize(tmpl_ids.size());
  for (auto& kv : tmpl_ids) tv[kv.second] = kv.first;
  std::vector<int32_t> remap(tv.size(), -1);
  std::map<std::vector<int64_t>, int32_t> used;
  for (auto& w : rows)
    for (auto& g : w.groups) {
      if (remap[g.first] < 0) {
        remap[g.first] = (int32_t)used.size();
        used.emplace(tv[g.first], remap[g.first]);
      }
      g.first = remap[g.first];
    }
  apply_rows(s, rows, used);
  s->blob.clear();
  // region ids index the batches' region buffers: a changed region set counts too
  const bool grew = s->str.names.size() != n_str || s->keys.names.size() != n_keys || s->gvk.names.size() != n_gvk ||
                    s->res.names.size() != n_res || s->regions.names != regions0;
  if (dict_grew) *dict_grew = grew ? 1 : 0;
  if (grew) s->epoch = next_snap_epoch();  // (packed records resolved against the old dictionaries)
  s->updates++;
  s->dev.reset();
  return upload_snapshot(e, s);
}

int kp_snapshot_export(const kp_snapshot* cs, const void** bytes, uint64_t* n_bytes) {
  if (!cs || !bytes || !n_bytes) return KP_EINVAL;
  kp_snapshot* s = const_cast<kp_snapshot*>(cs);
  s->blob.clear();
  Wr w{s->blob};
  w.raw(kSnapMagic, 8);
  w.u64((uint64_t)s->C);
  w.u64(s->opts.enable_empty_workload_propagation);
  w.u64(s->opts.customized_cluster_resource_modeling);
  w.u64(s->opts.enabled_plugins);
  w.u64(s->opts.multiple_pod_templates_scheduling);
  w.u64(s->opts.n_out_of_tree_plugins);
  w.u64((uint64_t)(int64_t)s->rid_cpu);
  w.u64((uint64_t)(int64_t)s->rid_mem);
  w.u64((uint64_t)(int64_t)s->rid_eph);
  w.u64((uint64_t)s->n_tmpl);
  w.u64((uint64_t)s->kmax);
  w.strs(s->str.names);
  w.strs(s->keys.names);
  w.strs(s->gvk.names);
  w.strs(s->res.names);
  w.strs(s->regions.names);
  w.strs(s->names);
  w.vec(s->perm);
  w.vec(s->flags);
  w.vec(s->provider);
  w.vec(s->region);
  w.vec(s->region_idx);
  w.vec(s->zone_off);
  w.vec(s->zone_ids);
  w.vec(s->label_val);
  w.vec(s->taint_off);
  w.vec(s->taint_key);
  w.vec(s->taint_val);
  w.vec(s->taint_eff);
  w.vec(s->mgrp_off);
  w.vec(s->mgrp_tid);
  w.vec(s->mgrp_cnt);
  w.vec(s->mg_tid);
  w.vec(s->mg_cnt);
  w.vec(s->provider_int);
  w.vec(s->region_int);
  w.vec(s->allowed);
  w.vec(s->avail);
  w.vec(s->qa);
  w.vec(s->tmpl);
  w.vec(s->api_bits);
  *bytes = s->blob.data();
  *n_bytes = s->blob.size();
  return KP_OK;
}

// The host half of kp_snapshot_import: every host column from the byte image
// (no device work).
static int import_host(kp_engine* e, const void* bytes, uint64_t n_bytes, kp_snapshot* s) {
  Rd r{(const unsigned char*)bytes, (const unsigned char*)bytes + n_bytes};
  char magic[8];
  if (!r.raw(magic, 8) || memcmp(magic, kSnapMagic, 8) != 0) {
    e->err = "not a kp snapshot";
    return KP_EINVAL;
  }
  s->e = e;
  s->C = (int)r.u64();
  s->Cp = s->C ? ((s->C + 63) / 64) * 64 : 64;
  s->W = s->Cp / 64;
  s->opts.enable_empty_workload_propagation = (uint8_t)r.u64();
  s->opts.customized_cluster_resource_modeling = (uint8_t)r.u64();
  s->opts.enabled_plugins = (uint32_t)r.u64();
  s->opts.multiple_pod_templates_scheduling = (uint8_t)r.u64();
  s->opts.n_out_of_tree_plugins = (uint32_t)r.u64();
  s->rid_cpu = (int32_t)(int64_t)r.u64();
  s->rid_mem = (int32_t)(int64_t)r.u64();
  s->rid_eph = (int32_t)(int64_t)r.u64();
  s->n_tmpl = (int)r.u64();
  s->kmax = (int)r.u64();
  dict_from(s->str, r.strs());
  dict_from(s->keys, r.strs());
  dict_from(s->gvk, r.strs());
  dict_from(s->res, r.strs());
  dict_from(s->regions, r.strs());
  s->names = r.strs();
  s->perm = r.vec<uint32_t>();
  s->flags = r.vec<uint32_t>();
  s->provider = r.vec<int32_t>();
  s->region = r.vec<int32_t>();
  s->region_idx = r.vec<int32_t>();
  s->zone_off = r.vec<int32_t>();
  s->zone_ids = r.vec<int32_t>();
  s->label_val = r.vec<int32_t>();
  s->taint_off = r.vec<int32_t>();
  s->taint_key = r.vec<int32_t>();
  s->taint_val = r.vec<int32_t>();
  s->taint_eff = r.vec<int32_t>();
  s->mgrp_off = r.vec<int32_t>();
  s->mgrp_tid = r.vec<int32_t>();
  s->mgrp_cnt = r.vec<int64_t>();
  s->mg_tid = r.vec<int32_t>();
  s->mg_cnt = r.vec<int32_t>();
  s->provider_int = r.vec<int64_t>();
  s->region_int = r.vec<int64_t>();
  s->allowed = r.vec<int64_t>();
  s->avail = r.vec<int64_t>();
  s->qa = r.vec<int64_t>();
  s->tmpl = r.vec<int64_t>();
  s->api_bits = r.vec<uint64_t>();
  if (!r.ok || r.p != r.end || !snapshot_consistent(s)) {
    e->err = "truncated or inconsistent snapshot bytes";
    return KP_EINVAL;
  }
  s->inv.assign(s->C, -1);
  for (int rk = 0; rk < s->C; rk++) {
    s->rank_of[s->names[rk]] = rk;
    if (s->perm[rk] < (uint32_t)s->C) s->inv[s->perm[rk]] = rk;
  }
  return KP_OK;
}

int kp_snapshot_import(kp_engine* e, const void* bytes, uint64_t n_bytes, kp_snapshot** out) {
  if (!e || !bytes || !out) return KP_EINVAL;
  (void)dev::set_device(e->device);
  auto* s = new kp_snapshot();
  std::unique_ptr<kp_snapshot> guard(s);
  int rc = import_host(e, bytes, n_bytes, s);
  if (rc != KP_OK) return rc;
  rc = upload_snapshot(e, s);
  if (rc != KP_OK) return rc;
  *out = guard.release();
  return KP_OK;
}

// A replica of `src` on engine e's device: the host columns from its byte image
// and the device arena copied device to device (hipMemcpyPeer: over xGMI between
// the GPUs of one node), its views rebased onto the copy. Nothing is re-derived.
int kp_snapshot_replicate(kp_engine* e, const kp_snapshot* src, kp_snapshot** out) {
  if (!e || !src || !out) return KP_EINVAL;
  const void* bytes = nullptr;
  uint64_t n_bytes = 0;
  int rc = kp_snapshot_export(src, &bytes, &n_bytes);
  if (rc != KP_OK) return rc;
  (void)dev::set_device(e->device);
  auto* s = new kp_snapshot();
  std::unique_ptr<kp_snapshot> guard(s);
  rc = import_host(e, bytes, n_bytes, s);
  if (rc != KP_OK) return rc;
  const size_t total = src->dev.total;
  HIPCHK(s->dev.alloc_raw(total));
  HIPCHK(dev::peer_copy(s->dev.base, e->device, src->dev.base, src->e->device, total, e->stream));
  HIPCHK(dev::sync(e->stream));
  s->view = src->view;
  const char* b0 = (const char*)src->dev.base;
  char* b1 = (char*)s->dev.base;
  auto rb = [&](auto& p) {
    if (p) p = (std::remove_reference_t<decltype(p)>)(b1 + ((const char*)p - b0));
  };
  SnapView& v = s->view;
  rb(v.flags), rb(v.perm), rb(v.provider), rb(v.region), rb(v.region_idx), rb(v.provider_int), rb(v.region_int);
  rb(v.zone_off), rb(v.zone_ids), rb(v.label_val), rb(v.taint_off), rb(v.taint_key), rb(v.taint_val);
  rb(v.taint_eff), rb(v.taint_set), rb(v.tset_rep), rb(v.api_bits), rb(v.allowed), rb(v.avail), rb(v.qa);
  rb(v.mg_tid), rb(v.mg_cnt), rb(v.tmpl), rb(v.mt_cnt), rb(v.bits), rb(v.bkey), rb(v.bval);
  rb(v.taint_uid), rb(v.uid_ref);
  s->est_kind = src->est_kind;
  *out = guard.release();
  return KP_OK;
}

}  // extern "C"
