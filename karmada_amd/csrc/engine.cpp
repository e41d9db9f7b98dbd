// engine.cpp — host side of the kp placement engine: the C-ABI of include/kp/kp_api.h except
// the node estimator (nodes.cpp). The snapshot/binding packer, kernel orchestration on one HIP
// stream, the host-kept selectGroups step, and the one definition of kp_host.h's shared state.
#include "kp_host.h"
#include "kp_paths.h"
#include "kp_pdq.h"
#include "kp_top.h"

namespace kp::host {

BufPool& buf_pool() {
  static BufPool* p = new BufPool();  // never destroyed: buffers may return during exit
  return *p;
}
void* pinned_get(size_t bytes, size_t* got) {
  if (void* p = buf_pool().get(-1, bytes, got)) return p;
  void* p = nullptr;
  if (dev::host_alloc(&p, bytes)) return nullptr;
  *got = bytes;
  return p;
}

// Snapshot epochs: unique per snapshot object and renewed when kp_snapshot_update grows
// its dictionaries, so packed records (kp_pack_cache) know which ids they resolved against.
uint64_t next_snap_epoch() {
  static std::atomic<uint64_t> n{0};
  return ++n;
}

}  // namespace kp::host

int build_sets_args(const kp_snapshot* s, const kp_component* comps, uint32_t K, SetsArgs* A, std::string* err);

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

// ============================================================================
// Binding packing
// ============================================================================
// Host-side pools of packed bindings (kp_batch's, or one packing thread's).
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

struct Packer {
  kp_snapshot* s;
  Pools* bt;  // this packer's pools (one per packing thread, merged by kp_batch_create)
  // per-packer caches: the last (apiVersion, kind) and its GVK id, parsed quantity
  // strings, and scratch lists reused across bindings (no per-binding allocation)
  std::string gvkey;
  SvMap<std::pair<bool, k8s::Qty>> qcache;
  SvMap<int32_t> gvk_cache;  // apiVersion + '\0' + kind -> GVK id
  SvMap<bool> scalar_cache;  // resource name -> IsScalarResourceName
  std::vector<int32_t> tmp_t, tmp_rk, tmp_sr, tmp_mr;
  std::vector<int64_t> tmp_sq, tmp_mq;
  std::vector<std::pair<std::string_view, k8s::Qty>> tmp_rq;
  std::vector<Instr> tmp_out;
  std::vector<int32_t> tmp_vals;
  std::vector<std::pair<std::string_view, std::string_view>> tmp_ml;
  std::vector<int32_t> tmp_filt, tmp_ovf, tmp_ov, tmp_ids, tmp_ev;
  std::vector<int64_t> tmp_ws;
  // compiled programs by affinity content (a batch repeats a policy's placement across
  // its bindings): the instructions with their list references relative to the lists
  // they own, re-emitted into the pools on a hit
  struct CProg {
    std::vector<Instr> ins;
    std::vector<int32_t> lists;
  };
  SvMap<int32_t> cmemo;
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
  std::vector<CProg> cprogs;
  std::string ckey;

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

// ---------------------------------------------------------------------------
// selectGroups (select_groups.go:102-224): the host-kept group combination.
// groups: (region id == name order, value = #clusters, weight = group score).
// ---------------------------------------------------------------------------
struct G {
  int id;
  int64_t value, weight;
};
std::vector<int> select_groups(std::vector<G> groups, int64_t minC, int64_t maxC, int64_t target) {
  if (groups.empty()) return {};
  if (groups.size() > 1)
    std::sort(groups.begin(), groups.end(), [](const G& a, const G& b) {
      if (a.value != b.value) return a.value < b.value;
      if (a.weight != b.weight) return a.weight > b.weight;
      return a.id < b.id;
    });
  struct Path {
    int id;
    int64_t weight, value;
    std::vector<int> g;  // indices into groups, sorted by (weight desc, id asc)
  };
  std::vector<Path> paths;
  std::vector<int> root;
  int pid = 0;
  const int n = (int)groups.size();
  std::function<void(int64_t, int)> dfs = [&](int64_t sum, int begin) {
    int64_t len = (int64_t)root.size();
    if (sum >= target && len >= minC && len <= maxC) {
      Path p;
      p.id = ++pid;
      p.weight = 0;
      p.value = 0;
      p.g = root;
      for (int i : p.g) {
        p.weight += groups[i].weight;
        p.value += groups[i].value;
      }
      std::sort(p.g.begin(), p.g.end(), [&](int a, int b) {
        if (groups[a].weight != groups[b].weight) return groups[a].weight > groups[b].weight;
        return groups[a].id < groups[b].id;
      });
      paths.push_back(std::move(p));
      return;
    }
    if (len >= maxC) return;
    for (int i = begin; i < n; i++) {
      sum += groups[i].value;
      root.push_back(i);
      dfs(sum, i + 1);
      if ((int64_t)n == minC) break;  // select_groups.go:179-182 (no backtracking)
      sum -= groups[i].value;
      root.pop_back();
    }
  };
  dfs(0, 0);
  if (paths.empty()) return {};
  const Path* fin = &paths[0];
  if (paths.size() > 1) {
    std::sort(paths.begin(), paths.end(), [](const Path& a, const Path& b) {
      if (a.weight != b.weight) return a.weight > b.weight;
      if (a.value != b.value) return a.value > b.value;
      return a.id < b.id;
    });
    fin = &paths[0];
    for (size_t i = 1; i < paths.size(); i++) {
      const Path& sp = paths[i];
      bool m = sp.g.size() < fin->g.size();
      for (size_t k = 0; m && k < sp.g.size(); k++) m = groups[fin->g[k]].id == groups[sp.g[k]].id;
      if (m) fin = &paths[i];
    }
  }
  std::vector<int> out;
  for (int i : fin->g) out.push_back(groups[i].id);
  return out;
}

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

template <class F>
void parallel_for(int n, int threads, F fn) {
  if (n <= 0) return;
  if (threads <= 1 || n < 64) {
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  std::atomic<int> next(0);
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([&]() {
      for (;;) {
        int i = next.fetch_add(16);
        if (i >= n) break;
        for (int k = i; k < std::min(n, i + 16); k++) fn(k);
      }
    });
  for (auto& t : th) t.join();
}

// The kernels' dynamic LDS for snapshot s (kp_launch.h: the sizes every launcher takes).
size_t smem_pair(const kp_snapshot* s, int md_cap) { return pair_lds_bytes(s->Cp, md_cap); }
size_t smem_all(const kp_snapshot* s) { return sel_all_lds_bytes(s->Cp); }
size_t smem_cluster(const kp_snapshot* s, int cap) { return sel_cluster_lds_bytes(s->Cp, cap); }
size_t smem_region_a(const kp_snapshot* s) { return region_a_lds_bytes(s->Cp, s->view.n_regions); }
size_t smem_region_b(const kp_snapshot* s, int cap) { return region_b_lds_bytes(s->Cp, s->view.n_regions, cap); }
const int kMdCap = 4096;
// MaxDivided table entries staged per workgroup: the snapshot's template count.
int md_cap_of(const kp_snapshot* s) { return s->n_tmpl <= kMdCap ? std::max(kTmplDense, s->n_tmpl) : 0; }
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
// The largest dynamic LDS any kernel of the batch takes must fit one workgroup.
// Checked at kp_batch_create and again at every kp_schedule_batch: an
// intervening kp_snapshot_update can change the region and template counts the
// sizes depend on.
int batch_lds_check(kp_engine* e, const kp_snapshot* s, const kp_batch* bt) {
  const int cap = kSmallMax + kTgtSmallMax + 16;
  size_t need = smem_pair(s, md_cap_of(s));
  if (!bt->l_all.empty()) need = std::max(need, smem_all(s));
  if (!bt->l_cluster.empty()) need = std::max(need, smem_cluster(s, cap));
  if (!bt->l_region.empty()) need = std::max({need, smem_region_a(s), smem_region_b(s, cap)});
  if (!bt->l_region_wide.empty())
    need = std::max(need, region_wide_lds_bytes(s->Cp, s->view.n_regions, bt->wide_sort));
  if (need > e->max_lds) {
    e->err = "snapshot too large for one workgroup's LDS (" + std::to_string(need) + " > " +
             std::to_string(e->max_lds) + " bytes)";
    return -1;
  }
  return 0;
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


// ============================================================================
// C ABI
// ============================================================================
extern "C" {

int kp_abi_version(void) { return KP_ABI_VERSION; }

int kp_engine_create(int device, kp_engine** out) {
  if (!out) return KP_EINVAL;
  if (device < 0 || dev::device_count() <= device) return KP_EDEVICE;
  auto* e = new kp_engine();
  e->device = device;
  // KP_STREAMS: distinct HIP streams per engine (default 3). HIP maps a process's streams
  // onto GPU_MAX_HW_QUEUES hardware queues (4 by default) round-robin, and streams that
  // share a queue run in order: several engines in one process (batches in flight) then
  // fit the default queues with fewer streams each. 2: the result/region stream and the
  // SEL_ALL stream are one (the class orders and the large select_top slice keep their
  // own); 1: every launch of the call in one stream.
  const int n_streams = (int)std::max(1ll, std::min(3ll, kp_env_int("KP_STREAMS", 3)));
  bool fail = dev::set_device(device) || dev::stream_create(&e->stream);
  if (!fail && n_streams >= 3) fail = dev::stream_create(&e->stream2) != 0;
  else e->stream2 = e->stream;
  if (!fail && n_streams >= 2) fail = dev::stream_create(&e->stream3) != 0;
  else e->stream3 = e->stream2;
  if (fail) {
    if (e->stream3 && e->stream3 != e->stream2 && e->stream3 != e->stream) dev::stream_destroy(e->stream3);
    if (e->stream2 && e->stream2 != e->stream) dev::stream_destroy(e->stream2);
    if (e->stream) dev::stream_destroy(e->stream);
    delete e;
    return KP_EDEVICE;
  }
  for (auto& ev : e->ev) (void)dev::event_create(&ev);
  e->max_lds = dev::max_lds_per_block(device);
  e->top_on = kp_env_int("KP_TOP", 1) != 0;
  e->top_split = kp_env_int("KP_TOP_SPLIT", 1) != 0;
  e->slow_order = kp_env_int("KP_SLOW_ORDER", 1) != 0;
  if (kp_env_flag("KP_TOP_CAP")) {  // (tests: one capacity for both slices)
    e->top_cap = std::max(64, std::min(1024, (int)kp_env_int("KP_TOP_CAP", 0) & ~63));
    e->top_cap_small = std::min(e->top_cap_small, e->top_cap);
  }
  e->top_cap_mid = std::max(0, std::min(1024, (int)kp_env_int("KP_TOP_CAP_MID", 0) & ~63));
  unsigned hc = std::thread::hardware_concurrency();
  e->n_threads = (int)std::max(1u, std::min(16u, hc));
  *out = e;
  return KP_OK;
}

void kp_engine_destroy(kp_engine* e) {
  if (!e) return;
  (void)dev::set_device(e->device);
  for (auto& ev : e->ev)
    if (ev) dev::event_destroy(ev);
  for (auto& ev : e->pev) dev::event_destroy(ev);
  // (aliases: KP_STREAMS < 3)
  if (e->stream3 && e->stream3 != e->stream2 && e->stream3 != e->stream) dev::stream_destroy(e->stream3);
  if (e->stream2 && e->stream2 != e->stream) dev::stream_destroy(e->stream2);
  if (e->stream) dev::stream_destroy(e->stream);
  delete e;
}

const char* kp_last_error(const kp_engine* e) { return e ? e->err.c_str() : "null engine"; }

int kp_engine_set_profile(kp_engine* e, int on) {
  if (!e) return KP_EINVAL;
  e->prof = on != 0;
  e->ktimes.clear();
  return KP_OK;
}

int kp_last_kernel_times(const kp_engine* e, kp_kernel_time* out, uint32_t cap, uint32_t* n_out) {
  if (!e || !n_out || (cap && !out)) return KP_EINVAL;
  *n_out = (uint32_t)e->ktimes.size();
  for (uint32_t i = 0; i < cap && i < e->ktimes.size(); i++) out[i] = e->ktimes[i];
  return KP_OK;
}

int kp_engine_set_threads(kp_engine* e, int n_threads) {
  if (!e || n_threads < 1) return KP_EINVAL;
  e->n_threads = std::min(n_threads, 256);
  return KP_OK;
}

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

// Packs bindings [0, n) into bt->hdr and bt's pools on T host threads: thread t
// packs a contiguous chunk into its own Pools (the Packer only reads the snapshot's
// dictionaries), then the chunks are concatenated and every pool reference is
// rebased: header offsets, program ids in the ipool lists, Prog::ins_off and the
// list offsets inside Instr. The result equals a sequential pack (test_abi).
// Threads: KP_PACK_THREADS, else the CPUs this process may use (hardware threads,
// capped by a cgroup CPU quota), one per 4096 bindings at most.
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

// Shifts a packed binding's pool references by (di, dl, dt, dp, dn) (ipool, lpool, tols,
// progs, instrs): its header, the program ids in its ipool lists, its programs'
// instruction offsets and its instructions' list offsets. ip: the binding's ipool slice
// (index = header offset - h.ip_beg, taken before the shift); pr / in: its program and
// instruction slices. pack_parallel's chunk merge applies the same shifts.
static void shift_binding(BindHdr& h, int32_t* ip, Prog* pr, int n_pr, Instr* in, int n_in, int32_t di, int32_t dl,
                          int32_t dt, int32_t dp, int32_t dn) {
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
    if (x.op == OP_EXCLUDE || x.op == OP_NAMES) x.a += di;
    else if (x.op == OP_LBL_IN || x.op == OP_LBL_NOTIN || x.op == OP_FLD_IN || x.op == OP_FLD_NOTIN ||
             x.op == OP_ZONE_IN || x.op == OP_ZONE_NOTIN)
      x.b += di;
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
}  // extern "C"

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

extern "C" {
static inline uint64_t cache_key(const kp_binding_key& k) {
  uint64_t h = 1469598103934665603ull;  // FNV-1a over the uid bytes, then the generation
  for (uint32_t i = 0; i < k.uid.len; i++) h = (h ^ (uint8_t)k.uid.ptr[i]) * 1099511628211ull;
  h ^= (uint64_t)k.generation * 0x9e3779b97f4a7c15ull;
  h ^= h >> 29;
  return h ? h : 1;
}

// row_of (kp_estimates, or null): each binding's row of the other estimators' answers; a
// workload binding's estimator class is then (request key, row), the row appended to the
// class key after the record lookup, so a cached record keeps the request key alone.
bool pack_parallel(kp_snapshot* s, const kp_binding* bindings, int n, kp_batch* bt, const kp_binding_key* keys = nullptr,
                   kp_pack_cache* cache = nullptr, const int32_t* row_of = nullptr) {
  int T = (int)kp_env_int("KP_PACK_THREADS", host_cpus());
  T = std::max(1, std::min(T, n / 4096));
  // Chunks of kPackChunk bindings taken from a shared counter (a thread that meets heavy
  // bindings takes fewer chunks); each chunk packs into its own pools, concatenated in
  // chunk order below. Packer caches and class-id maps are per thread.
  constexpr int kPackChunk = 1024;
  const int K = std::max(1, (n + kPackChunk - 1) / kPackChunk);
  std::vector<Pools> pl(K);
  std::vector<int> lo(K + 1), owner(K, 0);
  for (int k = 0; k <= K; k++) lo[k] = std::min(n, k * kPackChunk);
  // estimator classes: thread-local ids (bt->bcls) and keys, unified below
  bt->bcls.resize(n);
  std::vector<std::vector<std::string>> tkeys(T);
  std::vector<std::string> terr(T);
  std::vector<double> tms(T, 0.0), tstart(T, 0.0);
  const auto tpack0 = std::chrono::steady_clock::now();
  std::atomic<int> next_chunk(0);
  bt->route.resize(n);
  std::vector<uint64_t> chunk_cap(K + 1, 0);  // result slots per chunk (out_off prefix sums)
  std::vector<int> tmax_tgt(T, 0), tmax_tiers(T, 1);
  // kp_pack_cache: records of another snapshot epoch, or past the size cap, are dropped
  // first; new records collect per (chunk, shard) and go into the shards after the pack
  if (cache && (cache->epoch != s->epoch || cache->entries() > cache->max_entries)) {
    cache->clear();
    cache->epoch = s->epoch;
  }
  std::vector<std::vector<PackRec*>> newrecs(cache ? (size_t)K * kCacheShards : 0);
  struct RecGuard {  // records not handed to the cache (a failed batch) are freed
    std::vector<std::vector<PackRec*>>* v;
    ~RecGuard() {
      for (auto& x : *v)
        for (PackRec* r : x)
          if (r) PackRec::free(r);
    }
  } rec_guard{&newrecs};
  std::vector<uint64_t> thits(T, 0);  // (added once per chunk: adjacent slots share a line)
  auto run = [&](int t) {
    const auto tt0 = std::chrono::steady_clock::now();
    struct Stamp {
      std::chrono::steady_clock::time_point t0;
      double* out;
      ~Stamp() { *out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    } stamp{tt0, &tms[t]};
    tstart[t] = std::chrono::duration<double, std::milli>(tt0 - tpack0).count();
    Packer pk{s, nullptr};
    SvMap<int32_t> ids;
    std::string key;
    SetsArgs A;
    for (;;) {
      const int k = next_chunk.fetch_add(1);
      if (k >= K) break;
      owner[k] = t;
      pk.bt = &pl[k];
      uint64_t cap = 0, hits = 0;  // (chunk and thread totals kept in registers: the shared
      int max_tgt = 0, max_tiers = 1;  // arrays are written once per chunk, not once per binding)
      const int hi = lo[k + 1];
      // kp_pack_cache lookups run ahead of the packing in stages, each prefetching what the
      // next one reads: the uid bytes (8 ahead), the key hash and its table slot (4 ahead), the
      // record (2 ahead); bindings without a record get the packer's own prefetches instead
      constexpr int kRing = 16;
      uint64_t ck_ring[kRing];
      const PackRec* rec_ring[kRing];
      auto keyed_at = [&](int j) { return cache && j < hi && keys[j].uid.len > 0; };
      auto stage_hash = [&](int j) {
        if (!keyed_at(j)) return;
        const uint64_t c = cache_key(keys[j]);
        ck_ring[j % kRing] = c;
        pf(cache->shard[c % kCacheShards].home_slot(c));
      };
      auto stage_rec = [&](int j) {
        const PackRec* r = nullptr;
        if (keyed_at(j)) {
          const uint64_t c = ck_ring[j % kRing];
          r = cache->shard[c % kCacheShards].find(c);
          if (r)
            for (int o = 0; o < 8; o++) pf((const char*)r + 64 * o);
        }
        rec_ring[j % kRing] = r;
        if (!r && j < hi) pf_arrays(bindings[j]);
      };
      for (int q = lo[k]; q < std::min(hi, lo[k] + 3); q++) pf_struct(&bindings[q]);
      if (cache) {
        for (int q = lo[k]; q < std::min(hi, lo[k] + 8); q++)
          if (keyed_at(q)) pf(keys[q].uid.ptr);
        for (int q = lo[k]; q < lo[k] + 4; q++) stage_hash(q);
        for (int q = lo[k]; q < lo[k] + 2; q++) stage_rec(q);
      } else if (lo[k] + 1 < hi) {
        pf_arrays(bindings[lo[k] + 1]);
      }
      for (int i = lo[k]; i < hi; i++) {
        if (i + 3 < hi) pf_struct(&bindings[i + 3]);
        if (cache) {
          if (keyed_at(i + 8)) pf(keys[i + 8].uid.ptr);
          stage_hash(i + 4);
          stage_rec(i + 2);
          if (i + 1 < hi && !rec_ring[(i + 1) % kRing]) pf_strings(bindings[i + 1]);
        } else {
          if (i + 2 < hi) pf_arrays(bindings[i + 2]);
          if (i + 1 < hi) pf_strings(bindings[i + 1]);
        }
        // a cached record (kp_pack_cache): the same key, generation and status fields
        const bool keyed = keyed_at(i);
        const uint64_t ck = keyed ? ck_ring[i % kRing] : 0;
        const PackRec* hit = keyed ? rec_ring[i % kRing] : nullptr;
        if (hit && !hit->same(keys[i], bindings[i])) hit = nullptr;
        Pools& P = pl[k];
        const size_t ip0 = P.ipool.size(), lp0 = P.lpool.size(), to0 = P.tols.size(), pr0 = P.progs.size(),
                     in0 = P.instrs.size();
        if (hit) {  // the record's slices appended, its references shifted onto them
          BindHdr& h = bt->hdr[i];
          h = hit->h;
          P.ipool.insert(P.ipool.end(), hit->ip(), hit->ip() + hit->n_ip);
          P.lpool.insert(P.lpool.end(), hit->lp(), hit->lp() + hit->n_lp);
          P.tols.insert(P.tols.end(), hit->tol(), hit->tol() + hit->n_tol);
          P.progs.insert(P.progs.end(), hit->pr(), hit->pr() + hit->n_pr);
          P.instrs.insert(P.instrs.end(), hit->in(), hit->in() + hit->n_in);
          shift_binding(h, P.ipool.data() + ip0, P.progs.data() + pr0, hit->n_pr, P.instrs.data() + in0, hit->n_in,
                        (int32_t)ip0, (int32_t)lp0, (int32_t)to0, (int32_t)pr0, (int32_t)in0);
          hits++;
        } else {
          pk.pack(bindings[i], bt->hdr[i]);
        }
        {
          const BindHdr& h = bt->hdr[i];
          cap += h.out_cap;
          bt->route[i] = route_of(s->view, h, pl[k].lpool.data());  // (chunk-relative pool offsets)
          max_tgt = std::max(max_tgt, (int)h.tgt_cnt);
          max_tiers = std::max(max_tiers, (int)h.ovf_cnt + 2);  // primary, each overflow term, unmatched
        }
        bool nonworkload = false;
        if (hit) {
          nonworkload = hit->nonworkload;
          if (!nonworkload) key.assign(hit->cls(), hit->cls_len);
        } else if (bt->hdr[i].flags & BF_NONWORKLOAD_EST) {
          nonworkload = true;
        } else {
          if (bt->hdr[i].flags & BF_SETS) {
            // a component-set class: key 'S' + the resolved SetsArgs (est_key's keys
            // start with the 0/1 ReplicaRequirements word, never 'S')
            std::string err;
            const int rc = build_sets_args(s, bindings[i].components, bindings[i].n_components, &A, &err);
            if (rc == KP_EINVAL) {
              bt->hdr[i].flags = (bt->hdr[i].flags & ~(uint32_t)BF_SETS) | BF_BAD;  // status ERROR, as a bad request
            } else if (rc != KP_OK) {
              if (terr[t].empty()) terr[t] = err;
              bt->hdr[i].flags &= ~(uint32_t)BF_SETS;
            }
            bt->route[i] = route_of(s->view, bt->hdr[i], pl[k].lpool.data());  // (flags changed)
          }
          if (bt->hdr[i].flags & BF_SETS) {
            key.assign(1, 'S');
            key.append((const char*)&A, sizeof(A));
          } else {
            est_key(bt->hdr[i], pl[k], &key);
          }
        }
        if (keyed && !hit) {  // a new record: the binding's slices, references relative to them
          const kp_binding& bb = bindings[i];
          const uint32_t ul = keys[i].uid.len, al = bb.observed_affinity_name.len,
                         cl = nonworkload ? 0u : (uint32_t)key.size();
          PackRec* r = PackRec::make((int)(P.ipool.size() - ip0), (int)(P.lpool.size() - lp0),
                                     (int)(P.tols.size() - to0), (int)(P.progs.size() - pr0),
                                     (int)(P.instrs.size() - in0), (size_t)ul + al + cl);
          r->key = ck;
          r->gen = keys[i].generation;
          r->has_rt = bb.has_reschedule_triggered_at;
          r->has_lst = bb.has_last_scheduled_time;
          r->rt_ns = r->has_rt ? bb.reschedule_triggered_at_ns : 0;
          r->lst_ns = r->has_lst ? bb.last_scheduled_time_ns : 0;
          r->nonworkload = nonworkload ? 1 : 0;
          r->uid_len = ul, r->aff_len = al, r->cls_len = cl;
          r->h = bt->hdr[i];
          std::copy(P.ipool.begin() + (long)ip0, P.ipool.end(), r->ip());
          std::copy(P.lpool.begin() + (long)lp0, P.lpool.end(), r->lp());
          std::copy(P.tols.begin() + (long)to0, P.tols.end(), r->tol());
          std::copy(P.progs.begin() + (long)pr0, P.progs.end(), r->pr());
          std::copy(P.instrs.begin() + (long)in0, P.instrs.end(), r->in());
          if (ul) memcpy((char*)r->uid(), keys[i].uid.ptr, ul);
          if (al) memcpy((char*)r->aff(), bb.observed_affinity_name.ptr, al);
          if (cl) memcpy((char*)r->cls(), key.data(), cl);
          shift_binding(r->h, r->ip(), r->pr(), r->n_pr, r->in(), r->n_in, -(int32_t)ip0, -(int32_t)lp0,
                        -(int32_t)to0, -(int32_t)pr0, -(int32_t)in0);
          newrecs[(size_t)k * kCacheShards + ck % kCacheShards].push_back(r);
        }
        if (nonworkload) {  // (calls no estimator: its row, if any, is ignored)
          bt->bcls[i] = -1;
          continue;
        }
        if (row_of) key.append((const char*)&row_of[i], 4);
        auto it = ids.find(key);
        if (it == ids.end()) {
          it = ids.emplace(key, (int32_t)tkeys[t].size()).first;
          tkeys[t].push_back(key);
        }
        bt->bcls[i] = it->second;
      }
      chunk_cap[k + 1] = cap;
      thits[t] += hits;
      tmax_tgt[t] = std::max(tmax_tgt[t], max_tgt);
      tmax_tiers[t] = std::max(tmax_tiers[t], max_tiers);
    }
  };
  auto on_threads = [&](auto fn) { HostPool::get().run(T, std::function<void(int)>(fn)); };
  const auto tq0 = std::chrono::steady_clock::now();
  on_threads(run);
  const auto tq1 = std::chrono::steady_clock::now();
  for (auto& x : terr)
    if (!x.empty()) {
      bt->err = x;
      return false;
    }
  // pools concatenated in chunk order: each chunk's bases are the prefix sums of the
  // pool sizes before it; the threads rebase the chunks' headers and instructions
  // and copy their pools into place, chunk by chunk from a shared counter
  std::vector<size_t> bi(K + 1, 0), bl(K + 1, 0), bo(K + 1, 0), bp(K + 1, 0), bn(K + 1, 0);
  for (int k = 0; k < K; k++) {
    bi[k + 1] = bi[k] + pl[k].ipool.size();
    bl[k + 1] = bl[k] + pl[k].lpool.size();
    bo[k + 1] = bo[k] + pl[k].tols.size();
    bp[k + 1] = bp[k] + pl[k].progs.size();
    bn[k + 1] = bn[k] + pl[k].instrs.size();
  }
  if (bi[K] > (size_t)INT32_MAX || bl[K] > (size_t)INT32_MAX || bo[K] > (size_t)INT32_MAX ||
      bp[K] > (size_t)INT32_MAX || bn[K] > (size_t)INT32_MAX)
    return false;  // pool offsets are int32
  bt->ipool.resize(bi[K]);
  bt->lpool.resize(bl[K]);
  bt->tols.resize(bo[K]);
  bt->progs.resize(bp[K]);
  bt->instrs.resize(bn[K]);
  // global class ids (1-based; 0 = non-workload): the threads' keys in thread order
  SvMap<int32_t> gid;
  bt->crep.assign(1, 0);
  if (row_of) bt->cls_est.assign(1, -1);
  std::vector<std::vector<int32_t>> remaps(T);
  for (int t = 0; t < T; t++) {
    std::vector<int32_t>& remap = remaps[t];
    remap.resize(tkeys[t].size());
    for (size_t j = 0; j < tkeys[t].size(); j++) {
      auto it = gid.emplace(tkeys[t][j], (int32_t)gid.size() + 1).first;
      remap[j] = it->second;
      if ((size_t)it->second == bt->crep.size()) {
        bt->crep.push_back(-1);
        const std::string& key = tkeys[t][j];
        if (row_of) {  // the key's last four bytes
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
  for (int k = 0; k < K; k++) chunk_cap[k + 1] += chunk_cap[k];
  bt->out_cap = chunk_cap[K];
  bt->max_tgt = *std::max_element(tmax_tgt.begin(), tmax_tgt.end());
  bt->max_tiers = *std::max_element(tmax_tiers.begin(), tmax_tiers.end());
  std::atomic<int> next_merge(0);
  auto merge = [&](int) {
    for (;;) {
      const int k = next_merge.fetch_add(1);
      if (k >= K) break;
      Pools& q = pl[k];
      const int32_t oi = (int32_t)bi[k], ol = (int32_t)bl[k], oo = (int32_t)bo[k], op = (int32_t)bp[k],
                    on = (int32_t)bn[k];
      const std::vector<int32_t>& remap = remaps[owner[k]];
      uint64_t off = chunk_cap[k];
      for (int i = lo[k]; i < lo[k + 1]; i++) {
        BindHdr& h = bt->hdr[i];
        bt->bcls[i] = bt->bcls[i] < 0 ? 0 : remap[bt->bcls[i]];
        h.out_off = off;  // private result slots: no atomic on the emit path
        off += h.out_cap;
        if (k == 0) continue;
        for (int j = 0; j < h.filt_cnt; j++) q.ipool[h.filt_off + j] += op;
        for (int j = 0; j < h.ovf_cnt; j++) q.ipool[h.ovf_off + j] += op;
        for (int j = 0; j < h.sw_cnt; j++) q.ipool[h.sw_off + j] += op;
        h.tgt_off += oi, h.evict_off += oi, h.filt_off += oi, h.ovf_off += oi, h.sw_off += oi;
        h.sreq_off += oi, h.mreq_off += oi, h.ip_beg += oi, h.ip_end += oi;
        h.sw_w_off += ol, h.sreq_q_off += ol, h.mreq_q_off += ol;
        h.tol_off += oo;
        h.pr_beg += op, h.pr_end += op;
        h.in_beg += on, h.in_end += on;
      }
      if (k > 0) {
        for (Prog& p : q.progs) p.ins_off += on;
        for (Instr& x : q.instrs) {
          if (x.op == OP_EXCLUDE || x.op == OP_NAMES) x.a += oi;
          else if (x.op == OP_LBL_IN || x.op == OP_LBL_NOTIN || x.op == OP_FLD_IN || x.op == OP_FLD_NOTIN ||
                   x.op == OP_ZONE_IN || x.op == OP_ZONE_NOTIN)
            x.b += oi;
        }
      }
      std::copy(q.ipool.begin(), q.ipool.end(), bt->ipool.begin() + (long)bi[k]);
      std::copy(q.lpool.begin(), q.lpool.end(), bt->lpool.begin() + (long)bl[k]);
      std::copy(q.tols.begin(), q.tols.end(), bt->tols.begin() + (long)bo[k]);
      std::copy(q.progs.begin(), q.progs.end(), bt->progs.begin() + (long)bp[k]);
      std::copy(q.instrs.begin(), q.instrs.end(), bt->instrs.begin() + (long)bn[k]);
      q = Pools();
    }
  };
  on_threads(merge);
  if (cache) {  // the new records into the shards (thread t fills shards t, t + T, ...)
    on_threads([&](int t) {
      for (int sh = t; sh < kCacheShards; sh += T) {
        PackTable& tab = cache->shard[sh];
        for (int k = 0; k < K; k++)
          for (PackRec*& r : newrecs[(size_t)k * kCacheShards + sh]) {
            tab.put(r);
            r = nullptr;
          }
      }
    });
    uint64_t h = 0;
    for (uint64_t x : thits) h += x;
    cache->hits += h;
    cache->misses += (uint64_t)n - h;
    cache->last_hits = h;
  }
  // a class's representative: its first binding
  size_t left = bt->crep.size() - 1;
  for (int i = 0; i < n && left; i++) {
    const int32_t g = bt->bcls[i];
    if (g && bt->crep[g] < 0) {
      bt->crep[g] = i;
      left--;
    }
  }
  if (kp_env_flag("KP_PACK_TIMING")) {
    auto ms = [](auto x, auto y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
    fprintf(stderr, "pack_parallel: %d threads, %d chunks, pack %.1f ms, merge+classes %.1f ms; per thread", T, K,
            ms(tq0, tq1), ms(tq1, std::chrono::steady_clock::now()));
    for (double x : tms) fprintf(stderr, " %.1f", x);
    fprintf(stderr, "; started at");
    for (double x : tstart) fprintf(stderr, " %.1f", x);
    fprintf(stderr, "\n");
#ifdef KP_PACK_PROF
    fprintf(stderr, "pack sections (Mcycles, cumulative): gvk %.1f targets %.1f tolerations %.1f affinity %.1f "
            "static %.1f requests %.1f rest %.1f\n", g_pack_cyc[0] / 1e6, g_pack_cyc[1] / 1e6, g_pack_cyc[2] / 1e6,
            g_pack_cyc[3] / 1e6, g_pack_cyc[4] / 1e6, g_pack_cyc[5] / 1e6, g_pack_cyc[6] / 1e6);
#endif
  }
  return true;
}

// Bindings per estimator class below which a batch skips the class orders.
static int64_t order_amort() {  // (read per batch: tests switch it)
  return std::max<int64_t>(0, kp_env_int("KP_ORDER_AMORT", 4));
}

static int batch_create_impl(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, uint64_t n,
                             const kp_binding_key* keys, kp_pack_cache* cache, kp_batch** out,
                             const kp_estimates* est = nullptr, const kp_filter_answers* flt = nullptr);
int kp_batch_create_filters(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, const kp_binding_key* keys,
                            uint64_t n, kp_pack_cache* cache, const kp_estimates* est, const kp_filter_answers* flt,
                            kp_batch** out) {
  if (cache && n && !keys) return KP_EINVAL;  // (as kp_batch_create_keyed)
  return batch_create_impl(e, sc, bindings, n, cache ? keys : nullptr, cache, out, est, flt);
}
int kp_batch_create_estimates(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, const kp_binding_key* keys,
                              uint64_t n, kp_pack_cache* cache, const kp_estimates* est, kp_batch** out) {
  if (cache && n && !keys) return KP_EINVAL;  // (as kp_batch_create_keyed)
  return batch_create_impl(e, sc, bindings, n, cache ? keys : nullptr, cache, out, est);
}
int kp_batch_create(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, uint64_t n, kp_batch** out) {
  return batch_create_impl(e, sc, bindings, n, nullptr, nullptr, out);
}
int kp_batch_create_keyed(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, const kp_binding_key* keys,
                          uint64_t n, kp_pack_cache* cache, kp_batch** out) {
  if (!cache || (n && !keys)) return KP_EINVAL;
  return batch_create_impl(e, sc, bindings, n, keys, cache, out);
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
// kp_batch_create runs in stages (take_estimates ... upload, in that order); CreateCtx is
// what they share. Every host array the arena uploads from and no kp_batch member keeps
// lives here, so it outlives the upload's sync by construction.
namespace {
struct CreateCtx {
  kp_engine* e;
  kp_snapshot* s;
  const kp_binding* bindings;
  uint64_t n;
  const kp_estimates* est;         // null once found empty
  const kp_filter_answers* flt;    // null once found empty
  kp_batch* bt = nullptr;
  std::vector<int32_t> est_rows;   // kp_estimates rows by cluster rank, [n_rows][Cp]
  std::vector<uint64_t> flt_rows;  // kp_filter_answers rows by cluster rank, [n_rows][W]
  std::vector<FltPair> flt_list;   // the bindings that have a filter row
  uint32_t flt_plugins = 0;
  std::vector<int32_t> rep;        // d_crep's source: crep, -1 in the component-set classes
  std::vector<int64_t> sets_off;   // per cluster rank, its node-run scratch offset
  bool with_orders = false;
  std::chrono::steady_clock::time_point tp0, tp1, tp2;
};
}  // namespace

// What the two optional inputs' checks share: the n_clusters check that opens them and the
// n_rows bound and row_of range that close them; each input's own checks come between.
static int bad_answers(CreateCtx& c, const char* who, const std::string& why) {
  c.e->err = std::string(who) + ": " + why;
  return KP_EINVAL;
}
static int check_clusters(CreateCtx& c, const char* who, uint64_t n_clusters) {
  if (n_clusters == (uint64_t)c.s->C) return KP_OK;
  return bad_answers(c, who, "n_clusters is " + std::to_string(n_clusters) + ", the snapshot holds " +
                                 std::to_string(c.s->C) + " clusters");
}
static int check_row_of(CreateCtx& c, const char* who, uint32_t n_rows, const int32_t* row_of) {
  if (n_rows > (uint32_t)INT32_MAX) return bad_answers(c, who, "more than 2^31 - 1 rows");
  for (uint64_t i = 0; i < c.n; i++)
    if (row_of[i] < -1 || row_of[i] >= (int64_t)n_rows)
      return bad_answers(c, who, "row_of[" + std::to_string(i) + "] = " + std::to_string(row_of[i]) +
                                     " is outside -1.." + std::to_string((int64_t)n_rows - 1));
  return KP_OK;
}

// Stage 1a: the other estimators' rows (kp_estimates), checked and brought into rank order
// with the device rows' padding (-1: no answer) before anything is packed; none: est null.
static int take_estimates(CreateCtx& c) {
  const kp_estimates* est = c.est;
  kp_snapshot* s = c.s;
  if (est && est->n_rows == 0) est = c.est = nullptr;
  if (!est) return KP_OK;
  const char* who = "kp_batch_create_estimates";
  if (int rc = check_clusters(c, who, est->n_clusters)) return rc;
  if (!est->rows || (c.n && !est->row_of)) return bad_answers(c, who, "rows or row_of is null");
  if (int rc = check_row_of(c, who, est->n_rows, est->row_of)) return rc;
  c.est_rows.assign((size_t)est->n_rows * s->Cp, -1);
  for (uint32_t r = 0; r < est->n_rows; r++) {
    const int32_t* src = est->rows + (size_t)r * s->C;
    int32_t* dst = c.est_rows.data() + (size_t)r * s->Cp;
    for (int k = 0; k < s->C; k++) {
      const int32_t v = src[s->perm[k]];
      if (v < -1)
        return bad_answers(c, who, "rows[" + std::to_string(r) + "][" + std::to_string(s->perm[k]) + "] = " +
                                       std::to_string(v) + " is below -1 (UnauthenticReplica)");
      dst[k] = v;
    }
  }
  return KP_OK;
}

// Stage 1b: the out-of-tree filter verdicts (kp_filter_answers), checked and brought into
// rank order (dev_row bit rank = caller_row bit perm[rank]; W words a row, zero bits in the
// padding, caller bits at or above C never read), and the bindings that have a row.
static int take_filters(CreateCtx& c) {
  const kp_filter_answers* flt = c.flt;
  kp_snapshot* s = c.s;
  c.flt_plugins = flt ? flt->n_plugins : 0;
  if (flt && flt->n_rows == 0) flt = c.flt = nullptr;
  if (!flt) return KP_OK;
  const char* who = "kp_batch_create_filters";
  if (int rc = check_clusters(c, who, flt->n_clusters)) return rc;
  if (!flt->rows) return bad_answers(c, who, "rows is null");
  if (c.n && !flt->row_of) return bad_answers(c, who, "row_of is null");
  if (flt->n_plugins == 0)
    return bad_answers(c, who, "n_rows is " + std::to_string(flt->n_rows) + " with n_plugins == 0");
  if (int rc = check_row_of(c, who, flt->n_rows, flt->row_of)) return rc;
  for (uint64_t i = 0; i < c.n; i++)
    if (flt->row_of[i] >= 0) c.flt_list.push_back(FltPair{(int32_t)i, flt->row_of[i]});
  if (c.flt_list.empty()) return KP_OK;  // (rows that no binding uses: nothing to merge)
  const size_t Wc = ((size_t)s->C + 63) / 64;
  c.flt_rows.assign((size_t)flt->n_rows * s->W, 0);
  for (uint32_t r = 0; r < flt->n_rows; r++) {
    const uint64_t* src = flt->rows + (size_t)r * Wc;
    uint64_t* dst = c.flt_rows.data() + (size_t)r * s->W;
    for (int k = 0; k < s->C; k++) {
      const uint32_t cl = s->perm[k];
      dst[k >> 6] |= ((src[cl >> 6] >> (cl & 63)) & 1) << (k & 63);
    }
  }
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
    a.add(&bt->d_est_rows, c.est_rows.data(), c.est_rows.size());
  }
  if (!bt->l_flt.empty()) {
    a.add(&bt->d_flt_list, bt->l_flt.data(), bt->l_flt.size());
    a.add(&bt->d_flt_rows, c.flt_rows.data(), c.flt_rows.size());
  }
  c.tp1 = std::chrono::steady_clock::now();
  HIPCHK(a.alloc());
  bt->h_kargs = (KArgs*)pinned_get(sizeof(KArgs) * kArgSlots, &bt->h_kargs_bytes);
  if (!bt->h_kargs) {
    e->err = "kp_batch_create: page-locked launch-argument slots";
    return KP_EDEVICE;
  }
  return KP_OK;
}

// Stage 6: the copies, k_slow's flags cleared, the sync, and the KP_PACK_TIMING lines.
// create_stream is set while copies may be queued: an early return waits for them in
// ~kp_batch before the arena goes back to the pool.
static int upload(CreateCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  const int B = bt->B ? bt->B : 1;
  bt->create_stream = e->stream;
  c.tp2 = std::chrono::steady_clock::now();
  HIPCHK(bt->dev.upload(e->stream));
  HIPCHK(dev::fill(bt->slow, 0, 4 * (size_t)B, e->stream));
  HIPCHK(dev::sync(e->stream));
  if (kp_env_flag("KP_PACK_TIMING")) {
    if (!bt->l_est_cls.empty())
      fprintf(stderr, "kp_batch_create_estimates: %zu classes with a row, %zu bytes uploaded for them\n",
              bt->l_est_cls.size(), 4 * (bt->cls_est.size() + bt->l_est_cls.size() + c.est_rows.size()));
    if (!bt->l_flt.empty())
      fprintf(stderr, "kp_batch_create_filters: %zu bindings with a row, %zu bytes uploaded for them\n",
              bt->l_flt.size(), sizeof(FltPair) * bt->l_flt.size() + 8 * c.flt_rows.size());
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
static int batch_create_impl(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, uint64_t n,
                             const kp_binding_key* keys, kp_pack_cache* cache, kp_batch** out,
                             const kp_estimates* est, const kp_filter_answers* flt) {
  if (!e || !sc || !out || (n && !bindings)) return KP_EINVAL;
  if (n > (uint64_t)INT32_MAX) return KP_ENOTSUP;
  (void)dev::set_device(e->device);
  CreateCtx c{e, const_cast<kp_snapshot*>(sc), bindings, n, est, flt};
  kp_snapshot* s = c.s;
  if (int rc = take_estimates(c)) return rc;
  if (int rc = take_filters(c)) return rc;
  auto* bt = new kp_batch();
  std::unique_ptr<kp_batch> guard(bt);
  c.bt = bt;
  bt->snap = s;
  bt->B = (int)n;
  bt->hdr.resize(n);
  bt->flt_plugins = c.flt_plugins;
  bt->l_flt = std::move(c.flt_list);
  c.tp0 = std::chrono::steady_clock::now();
  if (s->opts.multiple_pod_templates_scheduling)
    for (uint64_t i = 0; i < n; i++)
      if (bindings[i].n_components > 0 && !bindings[i].components) {
        e->err = "kp_batch_create: binding " + std::to_string(i) +
                 " has n_components > 0 but no components (the MultiplePodTemplatesScheduling gate reads them)";
        return KP_EINVAL;
      }
  if (!pack_parallel(s, bindings, (int)n, bt, keys, cache, c.est ? c.est->row_of : nullptr)) {
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

void kp_batch_destroy(kp_batch* b) { delete b; }

// After a failed entry point: the work it queued on the engine's streams may still
// use the batch's buffers, so destruction must wait for it (kp_batch::quiesce).
static int batch_fence(kp_engine* e, kp_batch* bt, int rc) {
  if (rc == KP_OK || !e || !bt) return rc;
  const dev::stream_t ss[3] = {e->stream, e->stream2, e->stream3};
  for (int i = 0; i < 3; i++) {
    if (!bt->fence[i] && dev::event_create(&bt->fence[i])) {
      bt->fence[i] = nullptr;
      (void)dev::sync(ss[i]);  // no event: wait here instead
      continue;
    }
    if (dev::event_record(bt->fence[i], ss[i])) (void)dev::sync(ss[i]);
  }
  bt->fenced = true;
  return rc;
}

// The per-binding [B][Cp] calAvailableReplicas rows, allocated on first use (the
// pair-row mode and the diagnosis entry points; the default path never needs them).
static int ensure_rows(kp_engine* e, kp_batch* bt) {
  if (bt->est) return 0;
  void* p = nullptr;
  if (dev::alloc(&p, 4 * (size_t)std::max(1, bt->B) * (size_t)bt->snap->Cp)) {
    e->err = std::string("per-binding estimate rows: ") + dev::last_error();
    return -1;
  }
  bt->est = (int32_t*)p;
  return 0;
}

// The packed result form's buffers, allocated on the batch's first packed call (a batch
// only ever scheduled through kp_schedule_batch never needs them).
static int ensure_packed(kp_engine* e, kp_batch* bt) {
  const size_t B = (size_t)std::max(1, bt->B);
  if (!bt->wcount_d) {
    const size_t cnt = (4 * B + 255) & ~(size_t)255;  // the counts, then the 8-byte-aligned scan
    void* p = nullptr;
    if (dev::alloc(&p, cnt + 8 * (B + 1))) {
      e->err = std::string("packed results: ") + dev::last_error();
      return -1;
    }
    bt->wcount_d = (uint32_t*)p;
    bt->woff_d = (uint64_t*)((char*)p + cnt);
  }
  if (!bt->h_woff) {
    bt->h_woff = (uint64_t*)pinned_get(8 * (B + 1), &bt->h_woff_bytes);
    if (!bt->h_woff) {
      e->err = "packed results: page-locked wide_offsets";
      return -1;
    }
  }
  return 0;
}

// Per-kernel profiling (kp_engine_set_profile): prof_begin records the start event of
// launch i on its stream, prof_end its end event and what it covered.
static int prof_begin(kp_engine* e, dev::stream_t st) {
  if (!e->prof) return -1;
  const size_t i = e->pk.size();
  while (e->pev.size() < 2 * i + 2) {
    dev::event_t ev = nullptr;
    if (dev::event_create(&ev)) return -1;
    e->pev.push_back(ev);
  }
  if (dev::event_record(e->pev[2 * i], st)) return -1;
  e->pk.push_back({"", 0, -1});
  return (int)i;
}
static void prof_end(kp_engine* e, int i, dev::stream_t st, const char* name, uint64_t units, int units_stat = -1) {
  if (i < 0) return;
  (void)dev::event_record(e->pev[2 * (size_t)i + 1], st);
  e->pk[i] = {name, units, units_stat};
}
// After the batch's final sync: each kernel's launches folded by name.
static void prof_fold(kp_engine* e, const uint32_t* h_stats) {
  e->ktimes.clear();
  for (size_t i = 0; i < e->pk.size(); i++) {
    const auto& k = e->pk[i];
    const float ms = dev::event_ms(e->pev[2 * i], e->pev[2 * i + 1]);
    const uint64_t units = k.units_stat >= 0 ? h_stats[k.units_stat] : k.units;
    kp_kernel_time* t = nullptr;
    for (auto& x : e->ktimes)
      if (strncmp(x.name, k.name, sizeof(x.name)) == 0) t = &x;
    if (!t) {
      e->ktimes.push_back(kp_kernel_time{});
      t = &e->ktimes.back();
      snprintf(t->name, sizeof(t->name), "%s", k.name);
    }
    t->ms += ms > 0 ? ms : 0.f;
    t->launches++;
    t->units += units;
  }
  e->pk.clear();
}
#define KPROF(ST, NAME, UNITS, STAT, CALL)           \
  do {                                               \
    const int pi_ = prof_begin(e, ST);               \
    HIPCHK(CALL);                                    \
    prof_end(e, pi_, ST, NAME, (uint64_t)(UNITS), STAT); \
  } while (0)
// launch names of the select kernels (kernels.hip picks the wide instance past half
// the CU's LDS, as here)
static const char* sel_name(int which, size_t smem) {
  const bool wide = smem > 80 * 1024;
  switch (which) {
    case SEL_LAUNCH_ALL: return wide ? "k_select_all_wide" : "k_select_all";
    case SEL_LAUNCH_ALL_STREAM: return "k_select_all_stream";
    case SEL_LAUNCH_CLUSTER: return wide ? "k_select_cluster_wide" : "k_select_cluster";
    case SEL_LAUNCH_REGION_A: return wide ? "k_region_a_wide" : "k_region_a";
    case SEL_LAUNCH_REGION_B: return wide ? "k_region_b_wide" : "k_region_b";
    case SEL_LAUNCH_SLOW: return "k_slow";
  }
  return "k_select";
}
static const char* pair_name(int fast) {
  switch (fast) {
    case EST_MIXED: return "k_pair_fast";
    case EST_SUMMARY: return "k_pair_fast_summary";
    case EST_MODEL8: return "k_pair_fast_m8";
    case EST_MODEL16: return "k_pair_fast_m16";
  }
  return "k_pair";
}
static const char* est_class_feasible_name(int fast) {
  switch (fast) {
    case EST_SUMMARY: return "k_est_class_summary (feasible)";
    case EST_MODEL8: return "k_est_class_m8 (feasible)";
    case EST_MODEL16: return "k_est_class_m16 (feasible)";
    default: break;
  }
  return "k_est_class (feasible)";
}
static const char* est_class_name(int fast) {
  switch (fast) {
    case EST_SUMMARY: return "k_est_class_summary";
    case EST_MODEL8: return "k_est_class_m8";
    case EST_MODEL16: return "k_est_class_m16";
  }
  return "k_est_class";
}

// The batch path computes the in-tree plugin set (kp_options.n_out_of_tree_plugins) and takes
// the verdicts of out-of-tree filter plugins as rows (kp_batch_create_filters): a call runs
// when the answers fold in exactly the plugins the registry holds (answered: the batch's
// kp_filter_answers.n_plugins, 0 without answers and for the entry points that take none).
static int refuse_out_of_tree(kp_engine* e, const kp_snapshot* s, uint32_t answered = 0) {
  if (s->opts.n_out_of_tree_plugins == answered) return KP_OK;
  e->err = "the scheduler registry holds " + std::to_string(s->opts.n_out_of_tree_plugins) +
           " filter/score plugin(s) outside the in-tree set";
  if (answered)
    e->err += " and the batch's filter answers fold in " + std::to_string(answered) +
              " (kp_filter_answers.n_plugins must equal kp_options.n_out_of_tree_plugins)";
  else
    e->err += ": the batch path would ignore them (hand in filter-only plugins' verdicts with "
              "kp_batch_create_filters, or schedule through the framework with the per-pair entry points)";
  return KP_ENOTSUP;
}

// A schedule call in two halves: schedule_submit queues every launch and the per-binding
// read-backs of a batch (the region chain's host steps included) and records bt->pend.ev;
// schedule_finish waits for that event, copies the CSR back and fills the results.
// kp_schedule_batch runs both; kp_schedule_batch_submit / _collect let a caller keep the
// next batch's kernels queued on the engine's stream while it collects the previous one.
// packed: the results are gathered in the packed form (k_pack, the escape counts' scan,
// k_pack_wide) instead of the CSR (k_compact), for schedule_finish to return as
// kp_results_packed.
//
// schedule_submit queues the call in six stages (submit_rows ... submit_results, in that
// order) over the engine's three streams; SubmitCtx is what the stages share.
struct SubmitCtx {
  kp_engine* e;
  kp_batch* bt;
  kp_snapshot* s;
  bool packed;
  KArgs ka;       // the batch's launch arguments: a launch copies them and sets its list
  SelectExtra sx;
  int kslot = 0;  // device argument slots taken so far (with_args)
  int fast;       // the EST_* pair-kernel instance
  // Feasibility and calAvailableReplicas: by default (fast estimator instance and
  // the snapshot's bitset rows built) the filter runs as bitset algebra (k_filter)
  // and the estimator once per estimator class (k_est_class), kp_filter.h; else
  // (or KP_PAIR_ROWS=1) the pair kernel writes every binding's rows.
  bool bits;
  int top_cap, top_cap_small;  // k_select_top's subset capacities for this snapshot
  bool top;                    // SEL_ALL DynamicWeight / Aggregated over the deciding candidates (kp_top.h)
  // class orders: k_select_top's walk, and the spread selections over them
  // (k_spread_order, k_region_a_order), each where its LDS slices fit the device
  bool spread_orders, orders;
  // Fallback launches over device-appended lists, with a region chain: their counts are
  // read back where the host synchronises anyway (the region chain, k_slow's count), so a
  // list left empty launches nothing; the SEL_ALL and cluster-spread fallbacks move to
  // stream3 after that read, before k_slow (f_def / cl_def: their arguments until then).
  // A batch without a region chain queues every fallback, each workgroup reading the count.
  bool gate;
  bool defer_all = false, defer_all_stream = false, defer_cl = false;
  KArgs f_def{}, cl_def{};
  double th0 = 0, th1 = 0;  // the region chain's host step
  static constexpr int cap = kSmallMax + kTgtSmallMax + 16;

  SubmitCtx(kp_engine* e_, kp_batch* bt_, bool packed_) : e(e_), bt(bt_), s(bt_->snap), packed(packed_) {
    fast = kp_env_flag("KP_PAIR_GENERIC") || !bt->fast_ok ? EST_GENERIC : s->est_kind;
    bits = fast != EST_GENERIC && s->view.n_bits > 0 && !kp_env_flag("KP_PAIR_ROWS");
    ka.s = s->view;
    ka.bv = bt->view;
    ka.fmask = bt->fmask;
    ka.est = bits ? bt->cls_rows : bt->est;  // (rows mode: set again once ensure_rows has allocated them)
    ka.bcls = bits ? bt->d_bcls : nullptr;
    ka.sink.out_idx = bt->out_idx;
    ka.sink.out_rep = bt->out_rep;
    ka.sink.counter = bt->counter;
    ka.sink.status = bt->status;
    ka.sink.err = bt->errc;
    ka.sink.arg = bt->arg;
    ka.sink.start = bt->start;
    ka.sink.count = bt->count;
    ka.sink.cap_end = std::max<uint64_t>(1, 2 * bt->out_cap);
    ka.slow = bt->slow;
    ka.stats = bt->stats;
    ka.slow_ids = bt->d_slowlist;
    ka.dbg = bt->dbg;
    sx.rout = bt->rout;
    sx.rstat = bt->rstat;
    sx.rsel = bt->rsel;
    sx.rnsel = bt->rnsel;
    sx.scratch = bt->slow_scratch;
    sx.slot_bytes = bt->slow_slot;
    sx.grid = bt->slow_grid;
    sx.lds_area = bt->slow_lds;
    sx.lds_sort = bt->slow_sort;
    // the large slice's capacity, lowered until the slices fit the device's LDS
    top_cap = e->top_cap;
    while (top_cap > 64 && kTopWaves * ((top_lds_bytes(s->Cp, top_cap) + 15) & ~(size_t)15) > e->max_lds) top_cap /= 2;
    top_cap_small = std::min(e->top_cap_small, top_cap);
    // (without class orders, k_select_top thresholds the votes by a histogram: KP_TOPK=0 keeps
    // the full-candidate kernel there instead)
    static const bool topk_on = kp_env_int("KP_TOPK", 1) != 0;
    top = bits && e->top_on && s->Cp <= kTopMaxCp && (bt->d_ord != nullptr || (topk_on && bt->d_fb != nullptr)) &&
          bt->n_all_dyn > 0 && kTopWaves * ((top_lds_bytes(s->Cp, top_cap) + 15) & ~(size_t)15) <= e->max_lds;
    spread_orders = bits && e->top_on && bt->d_ord != nullptr && (!bt->l_cluster.empty() || !bt->l_region.empty()) &&
                    kOrderWaves * ((order_lds_bytes(s->view.W, s->view.n_regions) + 15) & ~(size_t)15) <= e->max_lds &&
                    kOrderWaves * ((region_a_order_lds_bytes(s->view.n_regions, s->view.W) + 15) & ~(size_t)15) <=
                        e->max_lds;
    orders = (top && bt->d_ord != nullptr) || spread_orders;
    gate = !bt->l_region.empty();
  }
  // A launch's KArgs copied to its own device slot (ordered before the launch on its
  // stream): the select kernels that keep pointers into their arguments read them there
  // (kp_launch.h SelectExtra::dargs). One slot per launch within this call.
  SelectExtra with_args(const KArgs& k, dev::stream_t sq) {
    SelectExtra r = sx;
    if (kslot >= kArgSlots) return r;  // (dargs stays null: the launch reports EINVAL)
    bt->h_kargs[kslot] = k;
    if (dev::h2d(bt->d_kargs + kslot, bt->h_kargs + kslot, sizeof(KArgs), sq) == 0) r.dargs = bt->d_kargs + kslot;
    kslot++;
    return r;
  }
};

// Stage 1, stream2: every row the selections read. The estimator classes' rows, the
// component-set classes' rows, the other estimators' answers, k_filter and the out-of-tree
// verdicts (or the pair kernel's per-binding rows instead), then the class orders; EV_ROWS_END
// marks them complete, and stream waits for it.
static int submit_rows(SubmitCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int B = bt->B, fast = c.fast;
  const bool bits = c.bits;
  dev::stream_t st = e->stream, sp = e->stream2;
  HIPCHK(dev::event_record(e->ev[EV_ROWS_BEGIN], sp));
  // component-set classes (BF_SETS bindings): their class rows (after the estimator
  // classes' rows, before k_class_order reads them all), and in the pair-row mode those
  // bindings' own rows rebuilt from them (feasible clusters only)
  auto sets_rows = [&]() -> int {
    for (size_t j = 0; j < bt->sets_cls.size(); j++)
      KPROF(sp, "k_sets_rows", 1, -1,
            dev::sets_rows(sp, s->view, bt->d_sets_args + j, bt->d_sets_off, bt->d_sets_scratch,
                           bt->cls_rows + (size_t)bt->sets_cls[j] * s->Cp, bt->d_sets_ovf + j));
    return KP_OK;
  };
  if (bits) {
    const bool single = bt->est_single;
    const int n_full = single ? (int)bt->l_cls_full.size() : (int)bt->crep.size();
    KPROF(sp, est_class_name(fast), n_full, -1,
          dev::est_class(sp, s->view, bt->view, bt->d_crep, n_full, bt->cls_rows, fast, single ? bt->d_cls_full : nullptr));
    if (int rc = sets_rows()) return rc;
    // the other estimators' answers merged into their classes' raw rows: every reader
    // below (class orders, the select kernels, k_slow) then sees merged rows
    if (!bt->l_est_cls.empty())
      KPROF(sp, "k_est_extra", bt->l_est_cls.size(), -1,
            dev::est_extra(sp, s->Cp, bt->d_est_cls, (int)bt->l_est_cls.size(), nullptr, bt->d_cls_est, bt->d_est_rows,
                           bt->cls_rows));
    HIPCHK(dev::event_record(e->ev[EV_CLASS_ROWS], sp));  // every class row is written (k_class_order's input)
    KPROF(sp, "k_filter", B, -1, dev::filter(sp, s->view, bt->view, bt->fmask));
    // the out-of-tree filter verdicts ANDed into their bindings' rows, ahead of every reader
    // of the feasibility rows (the feasible-only class rows next, then all behind EV_ROWS_END)
    if (!bt->l_flt.empty())
      KPROF(sp, "k_filter_extra", bt->l_flt.size(), -1,
            dev::filter_extra(sp, s->view, bt->d_flt_list, (int)bt->l_flt.size(), bt->d_flt_rows, bt->fmask, nullptr));
    if (single)  // the singleton classes' feasible entries, from the feasibility rows
      KPROF(sp, est_class_feasible_name(fast), bt->l_cls_single.size(), -1,
            dev::est_class(sp, s->view, bt->view, bt->d_crep, (int)bt->l_cls_single.size(), bt->cls_rows, fast,
                           bt->d_cls_single, bt->fmask));
  } else {
    const int md_cap = md_cap_of(s);
    KPROF(sp, pair_name(fast), B, -1,
          dev::pair(sp, s->view, bt->view, nullptr, 0, B, bt->fmask, bt->est, nullptr, 0, md_cap, smem_pair(s, md_cap),
                    fast));
    // pair-row mode: the same AND, and the estimate rows zeroed where the row rejects, as
    // the pair kernel leaves the clusters it found infeasible itself (k_rows_from_class and
    // k_est_extra below then keep them 0)
    if (!bt->l_flt.empty())
      KPROF(sp, "k_filter_extra", bt->l_flt.size(), -1,
            dev::filter_extra(sp, s->view, bt->d_flt_list, (int)bt->l_flt.size(), bt->d_flt_rows, bt->fmask, bt->est));
    if (int rc = sets_rows()) return rc;
    if (!bt->l_sets.empty())
      KPROF(sp, "k_rows_from_class", bt->l_sets.size(), -1,
            dev::rows_from_class(sp, s->view, bt->view, bt->d_sets_list, (int)bt->l_sets.size(), bt->d_bcls,
                                 bt->cls_rows, bt->fmask, bt->est));
    // the other estimators' answers merged over the rows of the bindings whose class has a
    // row; the entries are cal_merge'd already (0 on infeasible clusters), and a
    // GeneralEstimator answer is below MaxInt32, so the minimum is the reference's
    if (!bt->l_est_cls.empty())
      KPROF(sp, "k_est_extra", B, -1,
            dev::est_extra(sp, s->Cp, nullptr, B, bt->d_bcls, bt->d_cls_est, bt->d_est_rows, bt->est));
  }
  if (c.orders) {
    // k_class_order reads only the class rows (k_est_class), so it runs on stream3 beside
    // k_filter and stream2 waits for it (profiled runs keep it on stream2: each kernel's
    // event time is then its own)
    dev::stream_t so = e->prof ? sp : e->stream3;
    if (so != sp) HIPCHK(dev::stream_wait(so, e->ev[EV_CLASS_ROWS]));
    KPROF(so, "k_class_order", bt->crep.size(), -1,
          dev::class_order(so, s->view, bt->cls_rows, (int)bt->crep.size(), bt->d_ord, bt->d_ctot, bt->d_cok));
    if (so != sp) {
      HIPCHK(dev::event_record(e->ev[EV_CLASS_ORDER], so));
      HIPCHK(dev::stream_wait(sp, e->ev[EV_CLASS_ORDER]));
    }
  }
  HIPCHK(dev::event_record(e->ev[EV_ROWS_END], sp));
  HIPCHK(dev::stream_wait(st, e->ev[EV_ROWS_END]));  // every pair row precedes the rest
  HIPCHK(dev::event_record(e->ev[EV_SELECT_BEGIN], st));
  return KP_OK;
}

// Stage 2, stream2: the SEL_ALL bindings. k_select_top's slices over [0, n_all_dyn) and
// the full-candidate kernel over what they hand back, k_select_static, the streamed kernel
// over the rest. EV_SEL_ALL_BEGIN -> EV_SEL_ALL_END times it.
static int submit_sel_all(SubmitCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const bool bits = c.bits, top = c.top;
  const int cap = c.cap;
  dev::stream_t sp = e->stream2;
  HIPCHK(dev::event_record(e->ev[EV_SEL_ALL_BEGIN], sp));
  if (!bt->l_all.empty()) {
    KArgs k = c.ka;
    k.list = bt->d_all;
    k.n = (int)bt->l_all.size();
    // Candidates gathered into LDS (k_select_all), or, in bits mode, streamed from
    // the feasibility and class rows (k_select_all_stream): for the StaticWeight
    // bindings (votes from per-rule bitsets), and for all when the gathered
    // candidates would leave one workgroup per CU (C ~ 8.6k+).
    const bool stream_all = bits && smem_all(s) > 80 * 1024;
    const bool stream_w = bits;
    const int na = stream_all ? 0 : (stream_w ? bt->n_all_dyn : k.n);
    if (top) {
      // k_select_top over [0, n_all_dyn), small slices for [0, n_top_small); the
      // bindings it hands back (other strategies, subsets past capacity, ...) run with
      // every candidate from its fallback list
      HIPCHK(dev::event_record(e->ev[EV_TOP_BEGIN], sp));
      // the two slices' launches run concurrently, the large one on stream3 (which the
      // cluster-spread kernels use after it), so neither drains the CUs alone
      // (profiled steps keep both on one stream: each launch's HIP-event time is then its own)
      const bool split = e->top_split && !e->prof && bt->n_top_small > 0 && bt->n_all_dyn > bt->n_top_small;
      // the large slice in two capacities: top_cap_mid first (its smaller LDS slices
      // keep more waves per CU), then top_cap over the bindings whose subset outgrew it
      // (a device-appended list, grid-stride waves; the capacity only bounds the subset,
      // so both runs give the same answer)
      const bool mid = e->top_cap_mid >= 64 && e->top_cap_mid < c.top_cap;
      for (int part = 0; part < 2; part++) {
        KArgs g = k;
        const int cap_p = part == 0 ? c.top_cap_small : (mid ? e->top_cap_mid : c.top_cap);
        g.list = bt->d_all + (part == 0 ? 0 : bt->n_top_small);
        g.lcls = bt->d_all_cls + (part == 0 ? 0 : bt->n_top_small);
        g.n = part == 0 ? bt->n_top_small : bt->n_all_dyn - bt->n_top_small;
        if (g.n <= 0) continue;
        TopArgs ta{bt->d_ord, bt->d_ctot, bt->d_cok, bt->d_fb, bt->stats + KS_TOP_FALLBACK, cap_p};
        if (part == 1 && mid) {
          ta.ofb = bt->d_ofb;
          ta.ofb_n = bt->stats + KS_TOP_OVERFLOW;
        }
        const size_t slice = (top_lds_bytes(s->Cp, cap_p) + 15) & ~(size_t)15;
        dev::stream_t sx_ = split && part == 1 ? e->stream3 : sp;
        if (split && part == 1) HIPCHK(dev::stream_wait(sx_, e->ev[EV_ROWS_END]));
        KPROF(sx_, "k_select_top", g.n, -1, dev::select_top(sx_, g, ta, slice));
        if (part == 1 && mid) {
          KArgs o = k;
          o.list = bt->d_ofb;
          o.n = g.n;  // (the list's capacity; its length is stats[KS_TOP_OVERFLOW])
          o.n_dev = bt->stats + KS_TOP_OVERFLOW;
          TopArgs tb{bt->d_ord, bt->d_ctot, bt->d_cok, bt->d_fb, bt->stats + KS_TOP_FALLBACK, c.top_cap};
          const size_t slice_l = (top_lds_bytes(s->Cp, c.top_cap) + 15) & ~(size_t)15;
          // (units 0: the launch re-runs bindings the kernel's units already count)
          KPROF(sx_, "k_select_top", 0, -1, dev::select_top(sx_, o, tb, slice_l, kTopOverGrid));
        }
        if (split && part == 1) {
          HIPCHK(dev::event_record(e->ev[EV_TOP_LARGE], sx_));
          HIPCHK(dev::stream_wait(sp, e->ev[EV_TOP_LARGE]));  // both slices' fallbacks precede k_select_all
        }
      }
      HIPCHK(dev::event_record(e->ev[EV_TOP_END], sp));
      KArgs f = k;
      f.list = bt->d_fb;
      f.n = bt->n_all_dyn;
      f.n_dev = bt->stats + KS_TOP_FALLBACK;
      if (c.gate) {
        c.f_def = f;
        c.defer_all = true;
        c.defer_all_stream = stream_all;
      } else if (stream_all) {
        const SelectExtra sxa1 = c.with_args(f, sp);  // (the slot is copied before the launch is timed)
        KPROF(sp, "k_select_all_stream", 0, KS_TOP_FALLBACK,
              dev::select(sp, SEL_LAUNCH_ALL_STREAM, f, sel_stream_lds_bytes(s->Cp), cap, sxa1));
      } else {
        KPROF(sp, sel_name(SEL_LAUNCH_ALL, smem_all(s)), 0, KS_TOP_FALLBACK,
              dev::select(sp, SEL_LAUNCH_ALL, f, smem_all(s), cap, c.sx));
      }
    } else if (na > 0) {
      KArgs g = k;
      g.n = na;
      KPROF(sp, sel_name(SEL_LAUNCH_ALL, smem_all(s)), g.n, -1, dev::select(sp, SEL_LAUNCH_ALL, g, smem_all(s), cap, c.sx));
    }
    // the rest: StaticWeight at class level (k_select_static) where it applies, then
    // the streamed kernel
    int rest0 = top ? bt->n_all_dyn : na;
    if (bits && rest0 == bt->n_all_dyn && bt->n_static > 0 &&
        kStaticWaves * ((static_lds_bytes(s->view.W) + 15) & ~(size_t)15) <= e->max_lds) {
      KArgs g = k;
      g.list = bt->d_all + rest0;
      g.n = bt->n_static;
      KPROF(sp, "k_select_static", g.n, -1, dev::select_static(sp, g, (static_lds_bytes(s->view.W) + 15) & ~(size_t)15));
      rest0 += bt->n_static;
    }
    if (k.n - rest0 > 0) {
      KArgs g = k;
      g.list = bt->d_all + rest0;
      g.n = k.n - rest0;
      // (the argument slot is copied before the launch is timed)
      const SelectExtra sxa2 = c.with_args(g, sp);
      KPROF(sp, "k_select_all_stream", g.n, -1,
            dev::select(sp, SEL_LAUNCH_ALL_STREAM, g, sel_stream_lds_bytes(s->Cp), cap, sxa2));
    }
  }
  HIPCHK(dev::event_record(e->ev[EV_SEL_ALL_END], sp));  // k_select_all alone: EV_SEL_ALL_BEGIN -> EV_SEL_ALL_END
  return KP_OK;
}

// Stage 3, stream3 (behind the rows, EV_ROWS_END): the cluster-spread bindings, over the class
// orders first where the batch has them. EV_CLUSTER_BEGIN -> EV_CLUSTER_END times it.
static int submit_cluster_spread(SubmitCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int cap = c.cap;
  dev::stream_t s3 = e->stream3;
  HIPCHK(dev::stream_wait(s3, e->ev[EV_ROWS_END]));
  if (bt->l_cluster.empty()) return KP_OK;
  KArgs k = c.ka;
  k.list = bt->d_cluster;
  k.n = (int)bt->l_cluster.size();
  HIPCHK(dev::event_record(e->ev[EV_CLUSTER_BEGIN], s3));
  if (c.spread_orders) {
    // the class-order selection, one wave per binding; what it hands back runs below
    k.ord = bt->d_ord;
    k.cok = bt->d_cok;
    k.n_order = bt->stats + KS_CLUSTER_ORDER;
    OrderArgs oa{nullptr, nullptr, nullptr, bt->d_fbc, bt->stats + KS_FB_CLUSTER, 0};
    KPROF(s3, "k_spread_order", k.n, -1,
          dev::spread_order(s3, k, oa, (order_lds_bytes(s->view.W, s->view.n_regions) + 15) & ~(size_t)15));
    k.sub = bt->d_fbc;
    k.n_dev = bt->stats + KS_FB_CLUSTER;
  }
  if (c.gate && k.n_dev) {
    c.cl_def = k;
    c.defer_cl = true;
  } else {  // (the argument slot is copied before the launch is timed)
    const SelectExtra sxa3 = c.with_args(k, s3);
    KPROF(s3, sel_name(SEL_LAUNCH_CLUSTER, smem_cluster(s, cap)), k.n_dev ? 0 : k.n, k.n_dev ? KS_FB_CLUSTER : -1,
          dev::select(s3, SEL_LAUNCH_CLUSTER, k, smem_cluster(s, cap), cap, sxa3));
  }
  HIPCHK(dev::event_record(e->ev[EV_CLUSTER_END], s3));
  return KP_OK;
}

// Stage 4, stream: the region chain. Stage A (over the class orders, then the rest),
// selectGroups on the device with its host step, stage B the same two ways, k_region_wide.
// The two fallback launches over device-appended lists read their counts back first (the
// grid is then sized by the count: spread_grid), so an empty list launches nothing.
static int submit_region_chain(SubmitCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int cap = c.cap;
  dev::stream_t st = e->stream;
  if (bt->l_region.empty()) return KP_OK;
  const int nr = (int)bt->l_region.size(), R = s->view.n_regions;
  KArgs k = c.ka;
  k.list = bt->d_region;
  k.n = nr;
  if (c.spread_orders) {  // region_b_by_order
    k.ord = bt->d_ord;
    k.cok = bt->d_cok;
    k.n_order = bt->stats + KS_REGION_ORDER;
  }
  if (c.spread_orders) {  // stage A of the order-eligible bindings, one wave each; the rest below
    KArgs ko = k;
    ko.n_order = nullptr;
    KPROF(st, "k_region_a_order", ko.n, -1,
          dev::region_a_order(st, ko, bt->rout, bt->rstat, bt->d_fba, bt->stats + KS_FB_REGION_A,
                              (region_a_order_lds_bytes(R, s->view.W) + 15) & ~(size_t)15));
    KArgs kf = k;
    kf.sub = bt->d_fba;
    kf.n_dev = bt->stats + KS_FB_REGION_A;
    uint32_t nfa = 0;
    HIPCHK(dev::d2h(&nfa, bt->stats + KS_FB_REGION_A, 4, st));
    HIPCHK(dev::sync(st));
    if (nfa > 0) {  // (the argument slot is copied before the launch is timed)
      SelectExtra sxa4 = c.with_args(kf, st);
      sxa4.list_grid = (int)nfa;
      KPROF(st, sel_name(SEL_LAUNCH_REGION_A, smem_region_a(s)), 0, KS_FB_REGION_A,
            dev::select(st, SEL_LAUNCH_REGION_A, kf, smem_region_a(s), cap, sxa4));
    }
  } else {  // (the argument slot is copied before the launch is timed)
    const SelectExtra sxa5 = c.with_args(k, st);
    KPROF(st, sel_name(SEL_LAUNCH_REGION_A, smem_region_a(s)), k.n, -1,
          dev::select(st, SEL_LAUNCH_REGION_A, k, smem_region_a(s), cap, sxa5));
  }
  // selectGroups: on the device (one thread per binding) unless the snapshot
  // has more regions than its arrays hold; bindings whose DFS exceeds the node
  // budget, and every binding on the other route, take the host DFS.
  const bool dev_groups = R <= kGroupMax && !kp_env_flag("KP_REGION_HOST");
  uint32_t nh = 0;
  if (dev_groups) {
    HIPCHK(dev::fill(bt->nhost, 0, 4, st));
    KPROF(st, "k_region_groups", nr, -1, dev::region_groups(st, bt->rout, bt->rstat, bt->view.hdr, bt->d_region, nr, R, bt->rsel, bt->rnsel,
                              bt->nhost));
    HIPCHK(dev::d2h(&nh, bt->nhost, 4, st));
    HIPCHK(dev::sync(st));
  }
  if (!dev_groups || nh > 0) {
    bt->h_rout.resize((size_t)nr * std::max(R, 1));
    bt->h_rstat.resize(nr);
    HIPCHK(dev::d2h(bt->h_rout.data(), bt->rout, sizeof(RegionOut) * bt->h_rout.size(), st));
    HIPCHK(dev::d2h(bt->h_rstat.data(), bt->rstat, 4 * nr, st));
    bt->h_rsel.assign((size_t)nr * std::max(R, 1), -1);
    bt->h_rnsel.assign(nr, 0);
    if (dev_groups) {
      HIPCHK(dev::d2h(bt->h_rsel.data(), bt->rsel, 4 * bt->h_rsel.size(), st));
      HIPCHK(dev::d2h(bt->h_rnsel.data(), bt->rnsel, 4 * nr, st));
    }
    HIPCHK(dev::sync(st));
    c.th0 = now_ms();
    parallel_for(nr, e->n_threads, [&](int j) {
      if (dev_groups && bt->h_rnsel[j] != kGroupsHost) return;
      if (bt->h_rstat[j] != 0) {
        bt->h_rnsel[j] = -1000;
        return;
      }
      const BindHdr& h = bt->hdr[bt->l_region[j]];
      std::vector<G> groups;
      for (int r = 0; r < R; r++) {
        const RegionOut& ro = bt->h_rout[(size_t)j * R + r];
        if (ro.count > 0) groups.push_back({r, ro.count, ro.score});
      }
      // selectBestClustersByRegion (select_clusters_by_region.go:25-40)
      if ((int64_t)groups.size() < h.region_min) {
        bt->h_rnsel[j] = -KP_ERR_REGION_MIN_GROUPS;
        return;
      }
      auto sel = select_groups(groups, h.region_min, h.region_max, h.cluster_min);
      if (sel.empty()) {
        bt->h_rnsel[j] = -KP_ERR_REGION_CLUSTER_MIN;
        return;
      }
      for (int r = 0; r < R; r++) bt->h_rsel[(size_t)j * R + r] = -1;
      for (size_t q = 0; q < sel.size(); q++) bt->h_rsel[(size_t)j * R + q] = sel[q];
      bt->h_rnsel[j] = (int32_t)sel.size();
    });
    c.th1 = now_ms();
    HIPCHK(dev::h2d(bt->rsel, bt->h_rsel.data(), 4 * bt->h_rsel.size(), st));
    HIPCHK(dev::h2d(bt->rnsel, bt->h_rnsel.data(), 4 * nr, st));
  }
  uint32_t nfb = 1;
  if (c.spread_orders) {
    OrderArgs oa{bt->rout, bt->rsel, bt->rnsel, bt->d_fbr, bt->stats + KS_FB_REGION, 1};
    KPROF(st, "k_spread_order", k.n, -1, dev::spread_order(st, k, oa, (order_lds_bytes(s->view.W, R) + 15) & ~(size_t)15));
    k.sub = bt->d_fbr;
    k.n_dev = bt->stats + KS_FB_REGION;
    HIPCHK(dev::d2h(&nfb, bt->stats + KS_FB_REGION, 4, st));
    HIPCHK(dev::sync(st));
  }
  if (nfb > 0) {  // (the argument slot is copied before the launch is timed)
    SelectExtra sxa6 = c.with_args(k, st);
    if (k.n_dev) sxa6.list_grid = (int)nfb;
    KPROF(st, sel_name(SEL_LAUNCH_REGION_B, smem_region_b(s, cap)), k.n_dev ? 0 : k.n, k.n_dev ? KS_FB_REGION : -1,
          dev::select(st, SEL_LAUNCH_REGION_B, k, smem_region_b(s, cap), cap, sxa6));
  }
  // the selections past k_region_b's lists (marked there in a.slow), queued behind it: no
  // count is read back, a workgroup whose binding carries no mark returns at once
  if (!bt->l_region_wide.empty()) {
    KArgs kw = c.ka;
    kw.list = bt->d_region;
    kw.n = nr;
    const SelectExtra sxw = c.with_args(kw, st);
    KPROF(st, "k_region_wide", 0, KS_REGION_WIDE_DONE,
          dev::region_wide(st, kw, sxw, bt->d_region_wide, (int)bt->l_region_wide.size(), bt->wide_scratch,
                           bt->wide_slot, bt->wide_grid, bt->slow_cap, bt->wide_sort, bt->stats + KS_REGION_WIDE_DONE));
  }
  return KP_OK;
}

// Stage 5, stream3: k_slow after every kernel that flags bindings (SEL_ALL on stream2,
// cluster spread on stream3; the region chain, queued above, flags none), beside the region
// chain. With a region chain the flagged count is read back first (the host waits for the
// flagging kernels only): a batch that flags none launches nothing, and a few flagged take a
// small grid, instead of up to 256 workgroups whose LDS slices wait for CUs behind the
// region kernels (config 4: 3.87 -> 3.74 ms); the deferred SEL_ALL and cluster-spread
// fallbacks run at the same read. Without one the wait costs more than it saves (config 3:
// 2.00 -> 2.20 ms with four batches in flight), so k_slow is queued.
static int submit_slow(SubmitCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int cap = c.cap;
  dev::stream_t s3 = e->stream3;
  HIPCHK(dev::stream_wait(s3, e->ev[EV_SEL_ALL_END]));
  uint32_t nslow = (uint32_t)bt->slow_grid;
  if (c.gate) {
    uint32_t hs[KS_CHECK + 1];  // (KS_SLOW_TOTAL flagged, KS_TOP_FALLBACK / KS_FB_CLUSTER fallbacks among them)
    HIPCHK(dev::d2h(hs, bt->stats, sizeof(hs), s3));
    HIPCHK(dev::sync(s3));
    nslow = hs[KS_SLOW_TOTAL];
    bool more = false;  // a deferred fallback runs: it may flag bindings for k_slow
    if (c.defer_all && hs[KS_TOP_FALLBACK] > 0) {
      const KArgs& f = c.f_def;
      if (c.defer_all_stream) {
        SelectExtra sxa1 = c.with_args(f, s3);
        sxa1.list_grid = (int)hs[KS_TOP_FALLBACK];
        KPROF(s3, "k_select_all_stream", hs[KS_TOP_FALLBACK], -1,
              dev::select(s3, SEL_LAUNCH_ALL_STREAM, f, sel_stream_lds_bytes(s->Cp), cap, sxa1));
      } else {
        SelectExtra sxg = c.sx;
        sxg.list_grid = (int)hs[KS_TOP_FALLBACK];
        KPROF(s3, sel_name(SEL_LAUNCH_ALL, smem_all(s)), hs[KS_TOP_FALLBACK], -1,
              dev::select(s3, SEL_LAUNCH_ALL, f, smem_all(s), cap, sxg));
      }
      more = true;
    }
    if (c.defer_cl && hs[KS_FB_CLUSTER] > 0) {
      const KArgs& k = c.cl_def;
      SelectExtra sxa3 = c.with_args(k, s3);
      sxa3.list_grid = (int)hs[KS_FB_CLUSTER];
      KPROF(s3, sel_name(SEL_LAUNCH_CLUSTER, smem_cluster(s, cap)), hs[KS_FB_CLUSTER], -1,
            dev::select(s3, SEL_LAUNCH_CLUSTER, k, smem_cluster(s, cap), cap, sxa3));
      more = true;
    }
    if (more) nslow = (uint32_t)bt->slow_grid;  // (the kernel reads the final count itself)
  }
  if (!bt->l_slow.empty() && nslow > 0) {
    KArgs k = c.ka;
    k.list = bt->d_slowlist;
    k.n = (int)bt->l_slow.size();
    k.ord = c.orders ? bt->d_ord : nullptr;  // sortClusters order from the class orders (kp_kernels.h)
    k.cok = c.orders ? bt->d_cok : nullptr;
    if (!e->slow_order) k.ord = nullptr;
    SelectExtra sxs = c.with_args(k, s3);
    sxs.grid = (int)std::min<uint32_t>((uint32_t)bt->slow_grid, nslow);
    KPROF(s3, "k_slow", 0, KS_SLOW_TOTAL,
          dev::select(s3, SEL_LAUNCH_SLOW, k,
                      slow_lds_bytes(s->Cp, c.sx.lds_area, c.sx.lds_sort),
                      bt->slow_cap, sxs));
  }
  HIPCHK(dev::event_record(e->ev[EV_SLOW_END], s3));
  return KP_OK;
}

// Stage 6, stream (behind every select kernel and k_slow): results -> host. The offsets
// are scanned and the results compacted to CSR on the device (or packed: one word per
// target into cidx_d, the escape counts scanned into wide_offsets — the CSR scan's chunk
// totals are consumed by now, one stream — and the escaped replicas into crep_d); the
// per-binding arrays are read back here, the CSR by schedule_finish once it knows its size.
static int submit_results(SubmitCtx& c) {
  kp_engine* e = c.e;
  kp_batch* bt = c.bt;
  kp_snapshot* s = c.s;
  const int B = bt->B;
  dev::stream_t st = e->stream;
  HIPCHK(dev::stream_wait(st, e->ev[EV_SEL_ALL_END]));
  HIPCHK(dev::stream_wait(st, e->ev[EV_SLOW_END]));  // k_slow (stream3) and every select kernel precede the results
  HIPCHK(dev::event_record(e->ev[EV_SELECT_END], st));
  KPROF(st, "k_offsets", B, -1, dev::offsets(st, bt->status, bt->count, B, bt->offsets_d, bt->off_part));
  if (c.packed) {
    KPROF(st, "k_pack", B, -1,
          dev::pack(st, bt->start, bt->offsets_d, bt->out_idx, bt->out_rep, bt->cidx_d, bt->wcount_d, B, s->view.perm));
    KPROF(st, "k_offsets", B, -1, dev::offsets(st, bt->status, bt->wcount_d, B, bt->woff_d, bt->off_part));
    KPROF(st, "k_pack_wide", B, -1,
          dev::pack_wide(st, bt->start, bt->offsets_d, bt->woff_d, bt->out_rep, bt->crep_d, B));
    HIPCHK(dev::d2h(bt->h_woff, bt->woff_d, 8 * (size_t)(B + 1), st));
  } else {
    KPROF(st, "k_compact", B, -1,
          dev::compact(st, bt->start, bt->count, bt->offsets_d, bt->out_idx, bt->out_rep, bt->cidx_d, bt->crep_d, B,
                       s->view.perm));
  }
  bt->h_status.resize(B);
  bt->h_err.resize(B);
  bt->h_arg.resize(B);
  bt->h_offsets.resize(B + 1);
  HIPCHK(dev::d2h(bt->h_status.data(), bt->status, 4 * (size_t)B, st));
  HIPCHK(dev::d2h(bt->h_err.data(), bt->errc, 4 * (size_t)B, st));
  HIPCHK(dev::d2h(bt->h_arg.data(), bt->arg, 8 * (size_t)B, st));
  HIPCHK(dev::d2h(bt->h_offsets.data(), bt->offsets_d, 8 * (size_t)(B + 1), st));
  HIPCHK(dev::d2h(bt->h_stats, bt->stats, sizeof(bt->h_stats), st));
  SchedPend& pd = bt->pend;
  if (!pd.ev && dev::event_create(&pd.ev)) {
    pd.ev = nullptr;
    e->err = "kp_schedule_batch: event";
    return KP_EDEVICE;
  }
  HIPCHK(dev::event_record(pd.ev, st));
  return KP_OK;
}

static int schedule_submit(kp_engine* e, kp_batch* bt, bool packed) {
  if (!e || !bt) return KP_EINVAL;
  if (int rc = refuse_out_of_tree(e, bt->snap, bt->flt_plugins)) return rc;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  if (packed && s->C > 65536) {  // (kp_batch_create's LDS bound refuses such snapshots long before)
    e->err = "kp_schedule_batch_packed: a packed cluster index holds 16 bits (more than 65536 clusters)";
    return KP_ENOTSUP;
  }
  if (packed && ensure_packed(e, bt)) return KP_EDEVICE;
  SchedPend& pd = bt->pend;
  {
    const dev::event_t ev = pd.ev;  // (the event is kept across calls)
    pd = SchedPend{};
    pd.ev = ev;
  }
  bt->sched_done = false;
  pd.packed = packed;
  pd.t0 = now_ms();
  pd.seq = ++e->submit_seq;
  if (bt->B == 0) {
    pd.empty = true;
    pd.live = true;
    return KP_OK;
  }
  if (!bt->l_region.empty() && s->view.n_regions != bt->n_regions) {
    e->err = "kp_schedule_batch: the snapshot's region set changed since the batch was packed (re-create it)";
    return KP_ESTATE;
  }
  if (batch_lds_check(e, s, bt)) return KP_ENOTSUP;
  e->pk.clear();
  dev::stream_t st = e->stream;
  HIPCHK(dev::h2d(bt->counter, &bt->out_cap, sizeof(unsigned long long), st));  // the shared area's start
  HIPCHK(dev::fill(bt->stats, 0, sizeof(bt->h_stats), st));
  if (!bt->sets_cls.empty()) HIPCHK(dev::fill(bt->d_sets_ovf, 0, 4 * bt->sets_cls.size(), st));
#if defined(KP_STAMPS) || defined(KP_SLOW_CHECK)
  HIPCHK(dev::fill(bt->dbg, 0, kDbgSlots * kDbgSpread * 8, st));
#endif
  HIPCHK(dev::event_record(e->ev[EV_FILLS], st));
  HIPCHK(dev::stream_wait(e->stream2, e->ev[EV_FILLS]));  // the fills above precede every kernel
  SubmitCtx c(e, bt, packed);
  if (!c.bits) {
    if (ensure_rows(e, bt)) return KP_EDEVICE;
    c.ka.est = bt->est;
  }
  // The three selection kinds touch disjoint bindings: SEL_ALL on stream2 (after the
  // rows there), cluster spread on stream3, the region chain on stream, so a
  // latency-bound kernel shares the CUs with the others instead of running alone.
  if (int rc = submit_rows(c)) return rc;
  if (int rc = submit_sel_all(c)) return rc;
  if (int rc = submit_cluster_spread(c)) return rc;
  if (int rc = submit_region_chain(c)) return rc;
  if (int rc = submit_slow(c)) return rc;
  if (int rc = submit_results(c)) return rc;
  pd.bits = c.bits;
  pd.fast = c.fast;
  pd.top = c.top;
  pd.spread_orders = c.spread_orders;
  pd.th0 = c.th0;
  pd.th1 = c.th1;
  pd.live = true;
  return KP_OK;
}

// Exactly one of out / pout is given: the format the caller collects in, which must be
// the one the call was submitted in.
static int schedule_finish(kp_engine* e, kp_batch* bt, kp_results* out, kp_results_packed* pout) {
  if (!e || !bt || (!out && !pout)) return KP_EINVAL;
  SchedPend& pd = bt->pend;
  if (!pd.live) {
    e->err = "kp_schedule_batch_collect: the batch has no submitted call";
    return KP_ESTATE;
  }
  const bool packed = pout != nullptr;
  if (pd.packed != packed) {  // (the call stays submitted, for the right function to collect)
    e->err = pd.packed ? "kp_schedule_batch_collect: the submitted call is packed (kp_schedule_batch_collect_packed)"
                       : "kp_schedule_batch_collect_packed: the submitted call is not packed (kp_schedule_batch_collect)";
    return KP_ESTATE;
  }
  pd.live = false;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  const int B = bt->B;
  if (pd.empty) {
    bt->h_offsets.assign(1, 0);
    bt->h_status.clear();
    bt->sched_done = true;
    auto none = [&](auto* r) { memset(r, 0, sizeof(*r)), r->offsets = bt->h_offsets.data(); };
    packed ? none(pout) : none(out);
    return KP_OK;
  }
  dev::stream_t st = e->stream;
  const double t0 = pd.t0, th0 = pd.th0, th1 = pd.th1;
  const bool bits = pd.bits, top = pd.top, spread_orders = pd.spread_orders;
  const int fast = pd.fast;
  kp_stage_times tm{};
  HIPCHK(dev::event_sync(pd.ev));
  std::vector<uint32_t> sets_ovf(bt->sets_cls.size(), 0);
  if (!sets_ovf.empty()) {
    HIPCHK(dev::d2h(sets_ovf.data(), bt->d_sets_ovf, 4 * sets_ovf.size(), st));
    HIPCHK(dev::sync(st));
  }
  double tc0 = now_ms();
  const uint64_t tot = bt->h_offsets[B];
  if (tot > bt->h_res_cap || !bt->h_cidx) {
    buf_pool().put(-1, bt->h_cidx, bt->h_cidx_bytes);
    buf_pool().put(-1, bt->h_crep, bt->h_crep_bytes);
    bt->h_cidx = nullptr;
    bt->h_crep = nullptr;
    bt->h_res_cap = 0;
    const uint64_t cap = std::max<uint64_t>(1, tot + tot / 4);  // headroom for repeated calls
    bt->h_cidx = (uint32_t*)pinned_get(4 * cap, &bt->h_cidx_bytes);
    bt->h_crep = (int32_t*)pinned_get(4 * cap, &bt->h_crep_bytes);
    if (!bt->h_cidx || !bt->h_crep) {
      e->err = "kp_schedule_batch: page-locked result buffers";
      return KP_ENOMEM;
    }
    bt->h_res_cap = std::min(bt->h_cidx_bytes, bt->h_crep_bytes) / 4;
  }
  // (a packed call: tot packed words in cidx_d and the n_wide <= tot escaped replicas in
  // crep_d, 4 * (tot + n_wide) bytes instead of 8 * tot)
  uint64_t n_wide = packed ? bt->h_woff[B] : 0;
  if (packed) {
    if (tot) HIPCHK(dev::d2h(bt->h_cidx, bt->cidx_d, 4 * tot, st));
    if (n_wide) HIPCHK(dev::d2h(bt->h_crep, bt->crep_d, 4 * n_wide, st));
    if (tot) HIPCHK(dev::sync(st));
  } else if (tot) {
    HIPCHK(dev::d2h(bt->h_cidx, bt->cidx_d, 4 * tot, st));
    HIPCHK(dev::d2h(bt->h_crep, bt->crep_d, 4 * tot, st));
    HIPCHK(dev::sync(st));
  }
  // A component-set class whose simulation outgrew the device's node runs in some
  // cluster (kSetsRunsMax): its bindings report KP_ERR_SETS_CAPACITY, every other
  // binding keeps its result (the CSR is re-packed without their targets).
  for (size_t j = 0; j < sets_ovf.size(); j++) {
    if (!sets_ovf[j]) continue;
    const int32_t cls = bt->sets_cls[j];
    for (int32_t b : bt->l_sets)
      if (bt->bcls[b] == cls) {
        bt->h_status[b] = KP_STATUS_ERROR;
        bt->h_err[b] = KP_ERR_SETS_CAPACITY;
        bt->h_arg[b] = (int64_t)s->perm[sets_ovf[j] - 1];
      }
  }
  if (std::any_of(sets_ovf.begin(), sets_ovf.end(), [](uint32_t v) { return v != 0; })) {
    uint64_t w = 0, ww = 0;  // (packed: h_cidx holds the words, h_crep the escaped replicas)
    for (int b = 0; b < B; b++) {
      const uint64_t lo = bt->h_offsets[b], hi = bt->h_offsets[b + 1];
      bt->h_offsets[b] = w;
      if (packed) {
        const uint64_t wlo = bt->h_woff[b], whi = bt->h_woff[b + 1];
        bt->h_woff[b] = ww;
        if (bt->h_status[b] != KP_STATUS_OK) continue;
        for (uint64_t k = lo; k < hi; k++, w++) bt->h_cidx[w] = bt->h_cidx[k];
        for (uint64_t k = wlo; k < whi; k++, ww++) bt->h_crep[ww] = bt->h_crep[k];
        continue;
      }
      if (bt->h_status[b] != KP_STATUS_OK) continue;
      for (uint64_t k = lo; k < hi; k++, w++) {
        bt->h_cidx[w] = bt->h_cidx[k];
        bt->h_crep[w] = bt->h_crep[k];
      }
    }
    bt->h_offsets[B] = w;
    if (packed) bt->h_woff[B] = n_wide = ww;
  }
  const uint64_t tot_out = bt->h_offsets[B];
  double t1 = now_ms();
  if (e->prof) prof_fold(e, bt->h_stats);
  // pair: the pair launch, or k_est_class + k_filter (stream2; filter: k_filter
  // alone); select: from the point where they are complete to the end of the last
  // select kernel.
  // (the engine's events time this call unless a later submit has re-recorded them)
  const bool timed = pd.seq == e->submit_seq;
  auto ems = [&](int a, int b) { return timed ? dev::event_ms(e->ev[a], e->ev[b]) : 0.f; };
  const float ms_pair = ems(EV_ROWS_BEGIN, EV_ROWS_END);
  const float ms_filter = bits ? ems(EV_CLASS_ROWS, EV_ROWS_END) : 0.f;
  const float ms_sel = ems(EV_SELECT_BEGIN, EV_SELECT_END);
  tm.pair_launches = bits ? 2 : 1;
  tm.pair_kind = (uint32_t)fast;
  tm.pair_kernel_ms = ms_pair;
  tm.select_kernel_ms = ms_sel;
  tm.filter_kernel_ms = ms_filter;
  tm.sel_all_kernel_ms = ems(EV_SEL_ALL_BEGIN, EV_SEL_ALL_END);
  tm.n_sel_all = (uint32_t)bt->l_all.size();
  tm.bits = bits ? 1u : 0u;
  tm.n_classes = bits ? (uint32_t)bt->crep.size() : 0u;
  tm.n_slow = bt->h_stats[KS_SLOW_TOTAL];
  tm.n_top = top ? (uint32_t)bt->n_all_dyn : 0u;
  tm.n_top_fallback = top ? bt->h_stats[KS_TOP_FALLBACK] : 0u;
  tm.top_kernel_ms = top ? ems(EV_TOP_BEGIN, EV_TOP_END) : 0.f;
  tm.n_cluster = (uint32_t)bt->l_cluster.size();
  tm.n_cluster_order = spread_orders ? bt->h_stats[KS_CLUSTER_ORDER] : 0u;
  tm.cluster_kernel_ms = bt->l_cluster.empty() ? 0.f : ems(EV_CLUSTER_BEGIN, EV_CLUSTER_END);
  tm.n_region = (uint32_t)bt->l_region.size();
  tm.n_region_order = spread_orders ? bt->h_stats[KS_REGION_ORDER] : 0u;
  tm.n_region_wide = bt->l_region_wide.empty() ? 0u : bt->h_stats[KS_REGION_WIDE_DONE];
#if defined(KP_STAMPS) || defined(KP_SLOW_CHECK)
  {
    std::vector<unsigned long long> hv((size_t)kDbgSlots * kDbgSpread);
    HIPCHK(dev::d2h(hv.data(), bt->dbg, 8 * hv.size(), st));
    HIPCHK(dev::sync(st));
    unsigned long long h[kDbgSlots] = {};
    for (size_t q = 0; q < hv.size(); q++) h[q % kDbgSlots] += hv[q];
    fprintf(stderr, "kp stamps (s_memtime ticks, summed over workgroups):");
    for (int i = 0; i < kDbgSlots; i++)
      if (h[i]) fprintf(stderr, " [%d]=%llu", i, h[i]);
    fprintf(stderr, "\n");
  }
#endif
  if (kp_env_flag("KP_DEBUG_SLOW"))
    fprintf(stderr,
            "kp slow: total %u overflow/dup %u scale-down %u wrap %u tie %u weight %u cluster %u "
            "(ties resolved block-parallel %u); class-order spread fallbacks: cluster %u region %u (stage A %u)"
            " check %u\n",
            bt->h_stats[KS_SLOW_TOTAL], bt->h_stats[SLOW_OVERFLOW_DUP], bt->h_stats[SLOW_SCALE_DOWN],
            bt->h_stats[SLOW_WRAP], bt->h_stats[SLOW_TIE], bt->h_stats[SLOW_WEIGHT], bt->h_stats[SLOW_CLUSTER],
            bt->h_stats[KS_TIE_BLOCK], bt->h_stats[KS_FB_CLUSTER], bt->h_stats[KS_FB_REGION],
            bt->h_stats[KS_FB_REGION_A], bt->h_stats[KS_CHECK]);
  tm.pair_ms = ms_pair;
  tm.select_ms = ms_sel;
  tm.host_ms = th1 - th0;
  tm.copy_ms = t1 - tc0;
  tm.total_ms = t1 - t0;
  e->times = tm;
  bt->sched_done = true;
  auto common = [&](auto* r) {  // the fields the two result forms share
    r->n_bindings = (uint64_t)B;
    r->status = bt->h_status.data();
    r->err_code = bt->h_err.data();
    r->err_arg = bt->h_arg.data();
    r->offsets = bt->h_offsets.data();
    r->n_targets = tot_out;
  };
  if (packed) {
    common(pout);
    pout->targets = bt->h_cidx;
    pout->wide_replicas = bt->h_crep;
    pout->n_wide = n_wide;
    pout->wide_offsets = bt->h_woff;
  } else {
    common(out);
    out->cluster_idx = bt->h_cidx;
    out->replicas = bt->h_crep;
  }
  return KP_OK;
}

// The wide and the packed entry points share one body per call. The one-shot call: exactly
// one of out / pout is given, as for schedule_finish.
static int schedule_both(kp_engine* e, kp_batch* bt, kp_results* out, kp_results_packed* pout) {
  if (!out && !pout) return KP_EINVAL;
  if (int rc = schedule_submit(e, bt, pout != nullptr)) return rc;
  return schedule_finish(e, bt, out, pout);
}
// The submit call; `who` names the entry point in the error texts.
static int submit_call(kp_engine* e, kp_batch* bt, bool packed, const char* who) {
  if (e && e->prof) {
    e->err = std::string(who) + ": per-kernel profiling covers kp_schedule_batch only";
    return KP_EINVAL;
  }
  if (!e || !bt) return KP_EINVAL;
  if (bt->pend.live) {
    e->err = std::string(who) + ": the batch's previous call is not collected";
    return KP_ESTATE;
  }
  return batch_fence(e, bt, schedule_submit(e, bt, packed));
}
int kp_schedule_batch(kp_engine* e, kp_batch* bt, kp_results* out) { return batch_fence(e, bt, schedule_both(e, bt, out, nullptr)); }
int kp_schedule_batch_submit(kp_engine* e, kp_batch* bt) {
  return submit_call(e, bt, false, "kp_schedule_batch_submit");
}
int kp_schedule_batch_collect(kp_engine* e, kp_batch* bt, kp_results* out) {
  return batch_fence(e, bt, schedule_finish(e, bt, out, nullptr));
}
// The packed result form (kp_results_packed): the same calls with packed = true.
int kp_schedule_batch_packed(kp_engine* e, kp_batch* bt, kp_results_packed* out) {
  return batch_fence(e, bt, schedule_both(e, bt, nullptr, out));
}
int kp_schedule_batch_submit_packed(kp_engine* e, kp_batch* bt) {
  return submit_call(e, bt, true, "kp_schedule_batch_submit_packed");
}
int kp_schedule_batch_collect_packed(kp_engine* e, kp_batch* bt, kp_results_packed* out) {
  return batch_fence(e, bt, schedule_finish(e, bt, nullptr, out));
}
int kp_results_unpack(const kp_results_packed* in, uint32_t* cluster_idx, int32_t* replicas) {
  if (!in || (in->n_targets && (!in->targets || !cluster_idx || !replicas))) return KP_EINVAL;
  uint64_t k = 0;  // the escape cursor: the next entry of wide_replicas
  for (uint64_t i = 0; i < in->n_targets; i++) {
    const uint32_t w = in->targets[i];
    cluster_idx[i] = w & 0xFFFFu;
    if ((w >> 16) != 0xFFFFu) {
      replicas[i] = (int32_t)(w >> 16);
    } else {
      if (k >= in->n_wide || !in->wide_replicas) return KP_EINVAL;  // more escapes than wide entries
      replicas[i] = in->wide_replicas[k++];
    }
  }
  return k == in->n_wide ? KP_OK : KP_EINVAL;
}

// Runs the pair kernel and returns the rank-ordered device row pointers.
static int run_pair(kp_engine* e, kp_batch* bt, int64_t* score, int est_mode, int b0, int nb) {
  if (ensure_rows(e, bt)) return KP_EDEVICE;
  kp_snapshot* s = bt->snap;
  HIPCHK(dev::pair(e->stream, s->view, bt->view, nullptr, b0, nb, bt->fmask, bt->est, score, est_mode, md_cap_of(s),
                     smem_pair(s, md_cap_of(s))));
  HIPCHK(dev::sync(e->stream));
  return KP_OK;
}

static int filter_batch_impl(kp_engine* e, kp_batch* bt, uint64_t* out_mask) {
  if (!e || !bt || !out_mask) return KP_EINVAL;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  if (bt->B == 0) return KP_OK;
  if (s->view.n_bits > 0 && !kp_env_flag("KP_PAIR_ROWS")) {  // the schedule path's bitset filter
    HIPCHK(dev::filter(e->stream, s->view, bt->view, bt->fmask));
  } else {
    int rc = run_pair(e, bt, nullptr, 0, 0, bt->B);
    if (rc) return rc;
  }
  if (!bt->l_flt.empty())  // the merged mask: the out-of-tree verdicts ANDed in
    HIPCHK(dev::filter_extra(e->stream, s->view, bt->d_flt_list, (int)bt->l_flt.size(), bt->d_flt_rows, bt->fmask,
                             nullptr));
  std::vector<uint64_t> m((size_t)bt->B * s->W);
  HIPCHK(dev::d2h(m.data(), bt->fmask, 8 * m.size(), e->stream));
  HIPCHK(dev::sync(e->stream));
  const int Wc = (s->C + 63) / 64;
  memset(out_mask, 0, 8 * (size_t)bt->B * Wc);
  for (int b = 0; b < bt->B; b++)
    for (int r = 0; r < s->C; r++)
      if ((m[(size_t)b * s->W + (r >> 6)] >> (r & 63)) & 1) {
        uint32_t c = s->perm[r];
        out_mask[(size_t)b * Wc + (c >> 6)] |= 1ull << (c & 63);
      }
  return KP_OK;
}
int kp_filter_batch(kp_engine* e, kp_batch* bt, uint64_t* out_mask) { return batch_fence(e, bt, filter_batch_impl(e, bt, out_mask)); }

static int filter_reasons_impl(kp_engine* e, kp_batch* bt, uint32_t* out_reasons) {
  if (!e || !bt || !out_reasons) return KP_EINVAL;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  if (bt->B == 0 || s->C == 0) return KP_OK;
  // bindings in chunks of at most kChunkPairs pairs through one reused device
  // buffer (a 100k x 5k batch would otherwise take 2 GB on each side)
  const size_t chunk = std::max<size_t>(1, (size_t)kp_env_int("KP_REASONS_CHUNK", 1 << 24));  // (tests lower it)
  const int nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)bt->B, chunk / (size_t)s->C));
  const size_t pairs = (size_t)nb * s->C;
  uint32_t* d = nullptr;
  HIPCHK(dev::alloc((void**)&d, 4 * pairs));
  std::vector<uint32_t> h(pairs);
  int rc = KP_OK;
  for (int b0 = 0; b0 < bt->B && rc == KP_OK; b0 += nb) {
    const int m = std::min(nb, bt->B - b0);
    // the chunk's bindings that have a row of out-of-tree verdicts (l_flt is in binding
    // order): KP_REASON_OUT_OF_TREE substituted in the device buffer before the copy-back
    auto below = [](const FltPair& p, int b) { return p.b < b; };
    const size_t f0 = std::lower_bound(bt->l_flt.begin(), bt->l_flt.end(), b0, below) - bt->l_flt.begin();
    const size_t f1 = std::lower_bound(bt->l_flt.begin(), bt->l_flt.end(), b0 + m, below) - bt->l_flt.begin();
    if (dev::reasons(e->stream, s->view, bt->view, b0, m, d) ||
        dev::reasons_extra(e->stream, s->view, bt->d_flt_list + f0, (int)(f1 - f0), bt->d_flt_rows, b0, d) ||
        dev::d2h(h.data(), d, 4 * (size_t)m * s->C, e->stream) ||
        dev::sync(e->stream)) {
      e->err = std::string("kp_filter_reasons: ") + dev::last_error();
      rc = KP_EDEVICE;
      break;
    }
    for (int b = 0; b < m; b++)
      for (int r = 0; r < s->C; r++) out_reasons[(size_t)(b0 + b) * s->C + s->perm[r]] = h[(size_t)b * s->C + r];
  }
  dev::release(d);
  if (rc) return rc;
  return KP_OK;
}
int kp_filter_reasons(kp_engine* e, kp_batch* bt, uint32_t* out_reasons) { return batch_fence(e, bt, filter_reasons_impl(e, bt, out_reasons)); }

// One chunk of kp_fit_diagnosis_batch: the dense histogram rows of the bindings list[i0, i0 + m)
// (k_fit_hist over the snapshot's bitset rows; without them k_reasons / k_reasons_extra over
// each run of consecutive bindings, then k_reason_hist), compacted into the CSR on the device
// (count, k_offsets_a/b, write) and appended to the engine's result arrays. Only the chunk's
// offsets, its bins and n_fit / n_deleting are copied back.
struct DiagBufs {
  int32_t *list, *frow, *status0;
  uint32_t *dense, *words, *nbins, *n_fit, *n_del;
  uint64_t *off, *part;
};
static int fit_diagnosis_chunk(kp_engine* e, kp_batch* bt, const std::vector<int32_t>& list, const DiagBufs& d,
                               bool bits, int i0, int m) {
  kp_snapshot* s = bt->snap;
  const SnapView& v = s->view;
  const int U = v.n_taint_uid, S = hist_stride(U);
  auto& D = e->diag;
  dev::stream_t st = e->stream;
  HIPCHK(dev::fill(d.dense, 0, 4 * (size_t)m * S, st));
  if (bits) {
    HIPCHK(dev::fit_hist(st, v, bt->view, d.list + i0, d.frow + i0, m, bt->d_flt_rows, d.dense));
  } else {
    auto below = [](const FltPair& p, int b) { return p.b < b; };
    for (int j = 0; j < m;) {  // runs of consecutive binding indices: one k_reasons launch each
      int k = j + 1;
      while (k < m && list[i0 + k] == list[i0 + k - 1] + 1) k++;
      const int b0 = list[i0 + j], nb = k - j;
      uint32_t* w = d.words + (size_t)j * s->C;
      const size_t f0 = std::lower_bound(bt->l_flt.begin(), bt->l_flt.end(), b0, below) - bt->l_flt.begin();
      const size_t f1 = std::lower_bound(bt->l_flt.begin(), bt->l_flt.end(), b0 + nb, below) - bt->l_flt.begin();
      HIPCHK(dev::reasons(st, v, bt->view, b0, nb, w));
      HIPCHK(dev::reasons_extra(st, v, bt->d_flt_list + f0, (int)(f1 - f0), bt->d_flt_rows, b0, w));
      j = k;
    }
    HIPCHK(dev::reason_hist(st, v, d.words, m, d.dense));
  }
  HIPCHK(dev::hist_count(st, m, U, d.dense, d.nbins));
  HIPCHK(dev::offsets(st, d.status0, d.nbins, m, d.off, d.part));
  std::vector<uint64_t> off((size_t)m + 1);
  HIPCHK(dev::d2h(off.data(), d.off, 8 * off.size(), st));
  HIPCHK(dev::sync(st));  // (the chunk's bin total sizes the CSR arrays)
  const uint64_t tot = off[m], base = D.reason.size();
  Arena csr;
  uint32_t *reason, *tref, *count;
  csr.add(&reason, tot);
  csr.add(&tref, tot);
  csr.add(&count, tot);
  HIPCHK(csr.alloc());
  HIPCHK(dev::hist_write(st, m, U, v.uid_ref, d.dense, d.off, reason, tref, count, d.n_fit, d.n_del));
  D.reason.resize(base + tot);
  D.taint_ref.resize(base + tot);
  D.count.resize(base + tot);
  int rc = dev::d2h(D.reason.data() + base, reason, 4 * tot, st) || dev::d2h(D.taint_ref.data() + base, tref, 4 * tot, st) ||
           dev::d2h(D.count.data() + base, count, 4 * tot, st) ||
           dev::d2h(D.n_fit.data() + i0, d.n_fit, 4 * (size_t)m, st) ||
           dev::d2h(D.n_del.data() + i0, d.n_del, 4 * (size_t)m, st);
  rc = dev::sync(st) || rc;  // (csr is released below: nothing may still write it)
  if (rc) {
    e->err = std::string("kp_fit_diagnosis_batch: ") + dev::last_error();
    return KP_EDEVICE;
  }
  for (int j = 0; j < m; j++) D.offsets[(size_t)i0 + j + 1] = base + off[(size_t)j + 1];
  return KP_OK;
}

static int fit_diagnosis_impl(kp_engine* e, kp_batch* bt, const uint64_t* bindings, uint64_t n, kp_fit_diagnosis* out) {
  if (!e || !bt || !out) return KP_EINVAL;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  std::vector<int32_t> list;
  if (bindings) {
    for (uint64_t i = 0; i < n; i++) {
      if (bindings[i] >= (uint64_t)bt->B || (i > 0 && bindings[i] <= bindings[i - 1])) {
        e->err = "kp_fit_diagnosis_batch: the binding indices must be strictly ascending and below the batch size";
        return KP_EINVAL;
      }
      list.push_back((int32_t)bindings[i]);
    }
  } else {
    if (bt->pend.live || !bt->sched_done) {
      e->err = bt->pend.live ? "kp_fit_diagnosis_batch: the batch's submitted call is not collected"
                             : "kp_fit_diagnosis_batch: the batch has no completed schedule call";
      return KP_ESTATE;
    }
    for (int b = 0; b < (int)bt->h_status.size(); b++)
      if (bt->h_status[b] == KP_STATUS_FIT_ERROR) list.push_back(b);
  }
  const int N = (int)list.size();
  auto& D = e->diag;
  D.binding.assign(list.begin(), list.end());
  D.offsets.assign((size_t)N + 1, 0);
  D.reason.clear();
  D.taint_ref.clear();
  D.count.clear();
  D.n_fit.assign((size_t)N + 1, 0);  // (+ 1: data() of an empty list is still an array)
  D.n_del.assign((size_t)N + 1, 0);
  int rc = KP_OK;
  if (N > 0) {
    const bool bits = s->view.n_bits > 0 && !kp_env_flag("KP_PAIR_ROWS");
    std::vector<int32_t> frow((size_t)N, -1);  // the listed bindings' rows of out-of-tree verdicts
    for (size_t i = 0, f = 0; i < frow.size() && f < bt->l_flt.size(); i++) {
      while (f < bt->l_flt.size() && bt->l_flt[f].b < list[i]) f++;
      if (f < bt->l_flt.size() && bt->l_flt[f].b == list[i]) frow[i] = bt->l_flt[f].r;
    }
    // bindings per chunk: the dense rows, and without the bitset rows the reason words, of
    // one chunk stay within KP_REASONS_CHUNK words each (kp_filter_reasons' buffer bound)
    const size_t S = (size_t)hist_stride(s->view.n_taint_uid);
    const size_t chunk = std::max<size_t>(1, (size_t)kp_env_int("KP_REASONS_CHUNK", 1 << 24));
    const size_t per = bits ? S : std::max(S, (size_t)s->C);
    const int nbc = (int)std::max<size_t>(1, std::min<size_t>((size_t)N, chunk / per));
    Arena a;
    DiagBufs d{};
    a.add(&d.list, (size_t)N);
    a.add(&d.frow, (size_t)N);
    a.add(&d.status0, (size_t)nbc);
    a.add(&d.dense, (size_t)nbc * S);
    a.add(&d.words, bits ? 0 : (size_t)nbc * s->C);
    a.add(&d.nbins, (size_t)nbc);
    a.add(&d.n_fit, (size_t)nbc);
    a.add(&d.n_del, (size_t)nbc);
    a.add(&d.off, (size_t)nbc + 1);
    a.add(&d.part, (size_t)(nbc + kOffChunk - 1) / kOffChunk);
    HIPCHK(a.alloc());
    rc = dev::h2d(d.list, list.data(), 4 * (size_t)N, e->stream) || dev::h2d(d.frow, frow.data(), 4 * (size_t)N, e->stream) ||
                 dev::fill(d.status0, 0, 4 * (size_t)nbc, e->stream)  // (KP_STATUS_OK: k_offsets_a counts every row)
             ? KP_EDEVICE
             : KP_OK;
    if (rc) e->err = std::string("kp_fit_diagnosis_batch: ") + dev::last_error();
    for (int i0 = 0; i0 < N && rc == KP_OK; i0 += nbc) rc = fit_diagnosis_chunk(e, bt, list, d, bits, i0, std::min(nbc, N - i0));
    if (rc) (void)dev::sync(e->stream);  // (the arena is released here: nothing may still use it)
  }
  if (rc) return rc;
  out->n_bindings = (uint64_t)N;
  out->binding = D.binding.data();
  out->offsets = D.offsets.data();
  out->reason = D.reason.data();
  out->taint_ref = D.taint_ref.data();
  out->count = D.count.data();
  out->n_fit = D.n_fit.data();
  out->n_deleting = D.n_del.data();
  out->n_bins = (uint64_t)D.reason.size();
  return KP_OK;
}
int kp_fit_diagnosis_batch(kp_engine* e, kp_batch* bt, const uint64_t* bindings, uint64_t n, kp_fit_diagnosis* out) {
  return batch_fence(e, bt, fit_diagnosis_impl(e, bt, bindings, n, out));
}

}  // extern "C"

// One component list resolved against the snapshot's resource dictionary (SetsArgs,
// kp_sets.h): podsInSet, perSetRequirement (general.go:371-401, wrapping int64) and
// each component's util.NewResource request (resource.go:46-75). KP_EINVAL for an
// unparsable quantity, KP_ENOTSUP beyond the device limits.
int build_sets_args(const kp_snapshot* s, const kp_component* comps, uint32_t K, SetsArgs* A, std::string* err) {
  if (K > (uint32_t)kSetsComp) {
    *err = "MaxAvailableComponentSets: more than 16 components";
    return KP_ENOTSUP;
  }
  memset(A, 0, sizeof(*A));
  A->K = (int32_t)K;
  std::map<std::string, int64_t> per;       // perSetRequirement (general.go:389-401), wrapping int64
  std::vector<std::map<std::string, int64_t>> nr(K);  // util.NewResource of each request
  std::vector<std::string> slots;
  int64_t pps = 0;
  for (uint32_t k = 0; k < K; k++) {
    A->replicas[k] = comps[k].replicas;
    pps += comps[k].replicas;  // podsInSet
    if (!comps[k].has_replica_requirements) continue;
    QtyMap rq;
    if (!qmap(comps[k].resource_request, comps[k].n_resource_request, &rq)) {
      *err = "MaxAvailableComponentSets: unparsable quantity";
      return KP_EINVAL;
    }
    for (auto& kv : rq) {
      const std::string& nm = kv.first;
      per[nm] = (int64_t)((uint64_t)per[nm] + (uint64_t)k8s::as_int64(kv.second) * (uint64_t)(int64_t)comps[k].replicas);
      int64_t v;
      if (nm == "cpu") v = k8s::milli(kv.second);
      else if (nm == "memory" || nm == "ephemeral-storage" || (nm != "pods" && k8s::scalar_resource(nm)))
        v = k8s::value(kv.second);
      else continue;  // pods: requiredPerReplica.AllowedPodNumber = 1
      nr[k][nm] += v;
      if (std::find(slots.begin(), slots.end(), nm) == slots.end()) slots.push_back(nm);
    }
  }
  if (slots.size() + 1 > (size_t)kSetsSlots || per.size() > (size_t)kSetsPer) {
    *err = "MaxAvailableComponentSets: too many distinct resources";
    return KP_ENOTSUP;
  }
  A->NS = (int32_t)slots.size() + 1;
  for (size_t j = 0; j < slots.size(); j++) A->slot_rid[j] = s->res.get(slots[j]);
  A->slot_rid[slots.size()] = -2;  // pods
  for (uint32_t k = 0; k < K; k++) {
    for (size_t j = 0; j < slots.size(); j++) {
      auto it = nr[k].find(slots[j]);
      const int64_t v = it == nr[k].end() ? 0 : it->second;
      A->req[k][j] = v;
      A->pos[k][j] = v > 0 ? v : 0;
    }
    A->req[k][slots.size()] = 1;
    A->pos[k][slots.size()] = 1;
  }
  A->pods_per_set = pps;
  for (auto& kv : per) {
    A->per_rid[A->nper] = s->res.get(kv.first);
    A->per_req[A->nper] = kv.second;
    A->per_nonzero |= kv.second != 0 ? 1 : 0;
    A->nper++;
  }
  return KP_OK;
}

extern "C" {

int kp_max_available_component_sets(kp_engine* e, const kp_snapshot* sc, const kp_component* comps, uint32_t K,
                                    const uint32_t* cluster_idx, uint64_t n, int32_t* out) {
  if (!e || !sc || (K && !comps) || (n && (!cluster_idx || !out))) return KP_EINVAL;
  (void)dev::set_device(e->device);
  kp_snapshot* s = const_cast<kp_snapshot*>(sc);
  if (!s->opts.multiple_pod_templates_scheduling) {
    e->err = "MaxAvailableComponentSets: the MultiplePodTemplatesScheduling gate is off";
    return KP_ENOTSUP;
  }
  SetsArgs A;
  if (int rc = build_sets_args(s, comps, K, &A, &e->err)) return rc;
  std::vector<int32_t> ranks(n);
  std::vector<int64_t> off(n + 1, 0);  // runs per cluster: its model node count (a run holds >= 1 node)
  for (uint64_t i = 0; i < n; i++) {
    if (cluster_idx[i] >= (uint32_t)s->C) return KP_EINVAL;
    const int r = s->inv[cluster_idx[i]];
    ranks[i] = r;
    int64_t nodes = 0;
    for (int g = s->mgrp_off[r]; g < s->mgrp_off[r + 1]; g++) nodes += s->mgrp_cnt[g];
    off[i + 1] = off[i] + std::max<int64_t>(1, std::min<int64_t>(nodes, kSetsRunsMax));
  }
  if (n == 0) return KP_OK;
  Arena a;
  SetsArgs* dA;
  int32_t *dr, *dout;
  int64_t *doff, *scratch;
  a.add(&dA, 1);
  a.add(&dr, n);
  a.add(&doff, n + 1);
  a.add(&dout, n);
  a.add(&scratch, (size_t)off[n] * (1 + kSetsSlots));
  HIPCHK(a.alloc());
  HIPCHK(dev::h2d(dA, &A, sizeof(A), e->stream));
  HIPCHK(dev::h2d(dr, ranks.data(), 4 * n, e->stream));
  HIPCHK(dev::h2d(doff, off.data(), 8 * (n + 1), e->stream));
  HIPCHK(dev::component_sets(e->stream, s->view, dA, dr, doff, n, scratch, dout));
  HIPCHK(dev::d2h(out, dout, 4 * n, e->stream));
  HIPCHK(dev::sync(e->stream));
  for (uint64_t i = 0; i < n; i++)
    if (out[i] == kSetsOverflow) {
      e->err = "MaxAvailableComponentSets: cluster " + s->names[ranks[i]] + " needs more than " +
               std::to_string(kSetsRunsMax) + " node runs";
      return KP_ENOTSUP;
    }
  return KP_OK;
}

static int score_batch_impl(kp_engine* e, kp_batch* bt, int64_t* out_scores) {
  if (!e || !bt || !out_scores) return KP_EINVAL;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  if (bt->B == 0) return KP_OK;
  int64_t* d = nullptr;
  size_t n = (size_t)bt->B * std::max(1, s->C);
  HIPCHK(dev::alloc((void**)&d, 8 * n));
  int rc = run_pair(e, bt, d, 0, 0, bt->B);
  std::vector<int64_t> h(n);
  if (rc == KP_OK) rc = (dev::d2h(h.data(), d, 8 * n, e->stream) || dev::sync(e->stream)) ? KP_EDEVICE : KP_OK;
  dev::release(d);
  if (rc) return rc;
  for (int b = 0; b < bt->B; b++)
    for (int r = 0; r < s->C; r++) out_scores[(size_t)b * s->C + s->perm[r]] = h[(size_t)b * s->C + r];
  return KP_OK;
}
int kp_score_batch(kp_engine* e, kp_batch* bt, int64_t* out_scores) { return batch_fence(e, bt, score_batch_impl(e, bt, out_scores)); }

static int max_available_replicas_impl(kp_engine* e, kp_batch* bt, uint64_t binding, const uint32_t* cluster_idx, uint64_t n,
                                       int32_t* out) {
  if (!e || !bt || (n && (!cluster_idx || !out)) || binding >= (uint64_t)bt->B) return KP_EINVAL;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  int rc = run_pair(e, bt, nullptr, 1, (int)binding, 1);
  if (rc) return rc;
  std::vector<int32_t> row(s->Cp);
  HIPCHK(dev::d2h(row.data(), bt->est + (size_t)binding * s->Cp, 4 * (size_t)s->Cp, e->stream));
  HIPCHK(dev::sync(e->stream));
  for (uint64_t i = 0; i < n; i++) {
    if (cluster_idx[i] >= (uint32_t)s->C) return KP_EINVAL;
    out[i] = row[s->inv[cluster_idx[i]]];
  }
  return KP_OK;
}
int kp_max_available_replicas(kp_engine* e, kp_batch* bt, uint64_t binding, const uint32_t* cluster_idx, uint64_t n,
                              int32_t* out) {
  return batch_fence(e, bt, max_available_replicas_impl(e, bt, binding, cluster_idx, n, out));
}

int kp_last_stage_times(const kp_engine* e, kp_stage_times* out) {
  if (!e || !out) return KP_EINVAL;
  *out = e->times;
  return KP_OK;
}

}  // extern "C"

// getAffinityIndex (pkg/scheduler/helper.go:99-110).
static uint32_t affinity_index_of(const kp_binding& b) {
  if (!b.observed_affinity_name.ptr || b.observed_affinity_name.len == 0) return 0;
  const std::string obs(b.observed_affinity_name.ptr, b.observed_affinity_name.len);
  for (uint32_t i = 0; i < b.n_cluster_affinities; i++) {
    const kp_str& nm = b.cluster_affinities[i].affinity_name;
    if (nm.len == obs.size() && (nm.len == 0 || memcmp(nm.ptr, obs.data(), nm.len) == 0)) return i;
  }
  return 0;
}

int kp_schedule_affinities(kp_engine* e, const kp_snapshot* s, const kp_binding* bs, uint64_t n,
                           kp_affinity_results* out) {
  if (!e || !s || !out || (n && !bs)) return KP_EINVAL;
  if (int rc = refuse_out_of_tree(e, s)) return rc;
  auto& A = e->aff;
  A.status.assign(n, KP_STATUS_OK);
  A.err.assign(n, KP_ERR_NONE);
  A.arg.assign(n, 0);
  A.idx.assign(n, -1);
  A.attempts.assign(n, 0);
  // per binding: current term, first error seen, and its final (offset, count) in `pool`
  std::vector<uint32_t> cur(n, 0);
  std::vector<uint8_t> have_first(n, 0);
  std::vector<uint64_t> f_off(n, 0), f_cnt(n, 0);
  std::vector<uint32_t> pool_idx;
  std::vector<int32_t> pool_rep;
  std::vector<uint64_t> pending(n);
  for (uint64_t i = 0; i < n; i++) {
    pending[i] = i;
    const kp_binding& b = bs[i];
    if (b.n_cluster_affinities == 0) continue;
    cur[i] = affinity_index_of(b);
    if (b.has_reschedule_triggered_at && b.has_last_scheduled_time &&
        b.reschedule_triggered_at_ns > b.last_scheduled_time_ns)  // util.RescheduleRequired (binding.go:118-127)
      cur[i] = 0;
  }
  uint32_t rounds = 0;
  std::vector<kp_binding> sub;
  while (!pending.empty()) {
    rounds++;
    sub.resize(pending.size());
    for (size_t j = 0; j < pending.size(); j++) {
      sub[j] = bs[pending[j]];
      if (sub[j].n_cluster_affinities)  // updatedStatus.SchedulerObservedAffinityName (scheduler.go:640)
        sub[j].observed_affinity_name = sub[j].cluster_affinities[cur[pending[j]]].affinity_name;
    }
    kp_batch* bt = nullptr;
    int rc = kp_batch_create(e, s, sub.data(), sub.size(), &bt);
    if (rc) return rc;
    kp_results r{};
    rc = kp_schedule_batch(e, bt, &r);
    if (rc) {
      kp_batch_destroy(bt);
      return rc;
    }
    std::vector<uint64_t> next;
    for (size_t j = 0; j < pending.size(); j++) {
      const uint64_t i = pending[j];
      const kp_binding& b = bs[i];
      A.attempts[i]++;
      const bool ok = r.status[j] == KP_STATUS_OK;
      if (ok || b.n_cluster_affinities == 0) {
        A.status[i] = r.status[j];
        A.err[i] = r.err_code[j];
        A.arg[i] = r.err_arg[j];
        if (b.n_cluster_affinities && ok) A.idx[i] = (int32_t)cur[i];
        f_off[i] = pool_idx.size();
        f_cnt[i] = r.offsets[j + 1] - r.offsets[j];
        pool_idx.insert(pool_idx.end(), r.cluster_idx + r.offsets[j], r.cluster_idx + r.offsets[j + 1]);
        pool_rep.insert(pool_rep.end(), r.replicas + r.offsets[j], r.replicas + r.offsets[j + 1]);
        continue;
      }
      if (!have_first[i]) {  // firstErr (scheduler.go:646-649)
        have_first[i] = 1;
        A.status[i] = r.status[j];
        A.err[i] = r.err_code[j];
        A.arg[i] = r.err_arg[j];
      }
      if (++cur[i] < b.n_cluster_affinities) next.push_back(i);
    }
    kp_batch_destroy(bt);
    pending.swap(next);
  }
  A.offsets.assign(n + 1, 0);
  uint64_t tot = 0;
  for (uint64_t i = 0; i < n; i++) {
    A.offsets[i] = tot;
    tot += f_cnt[i];
  }
  A.offsets[n] = tot;
  A.cidx.resize(std::max<uint64_t>(1, tot));
  A.rep.resize(std::max<uint64_t>(1, tot));
  for (uint64_t i = 0; i < n; i++)
    for (uint64_t k = 0; k < f_cnt[i]; k++) {
      A.cidx[A.offsets[i] + k] = pool_idx[f_off[i] + k];
      A.rep[A.offsets[i] + k] = pool_rep[f_off[i] + k];
    }
  out->results.n_bindings = n;
  out->results.status = A.status.data();
  out->results.err_code = A.err.data();
  out->results.err_arg = A.arg.data();
  out->results.offsets = A.offsets.data();
  out->results.cluster_idx = A.cidx.data();
  out->results.replicas = A.rep.data();
  out->results.n_targets = tot;
  out->affinity_index = A.idx.data();
  out->attempts = A.attempts.data();
  out->rounds = rounds;
  return KP_OK;
}
