// driver.cpp — sanitizer run of the engine's host code (test infrastructure).
//
// Builds the host units + dev_cpu.cpp (the kernel bodies on host threads: the CPU-sim
// device layer), the synthetic universes (synth.cpp) and the oracle (oracle.cpp)
// into one program, instrumented with ThreadSanitizer or AddressSanitizer +
// UndefinedBehaviorSanitizer (tools/sanitize/Makefile). It schedules seeded
// universes of every workload with KP_CPUSIM_THREADS concurrent "workgroups" and
// checks each binding against the oracle (status, error, argument, multiset of
// targets). A hand-built batch (run_filter_shapes) adds the predicate shapes the
// synthetic universes lack (several affinity terms, a list of more than 64 values,
// more than four tolerations, spec.Clusters members with eviction tasks) through
// the bitset filter, every (binding, cluster) pair against the oracle's filter.
// run_affinity_answers runs kp_schedule_affinities_ex with both answers (rows shared by the
// rounds' batches), run_batch_answers one batch created with both and scheduled twice,
// run_pack_stages the packer on two threads with keyed creations and one that fails,
// run_watch one kp_watch and kp_affected_bindings in both modes.
// Exit code 0 = no mismatch (the sanitizers abort on their own findings).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/kp/kp_api.h"
#include "../../oracle/oracle.h"

struct kps_world;
extern "C" {
int kps_create(int config, uint64_t seed, uint32_t n_clusters, uint64_t b_lo, uint64_t b_hi, kps_world** out);
void kps_destroy(kps_world* w);
const kp_cluster* kps_clusters(const kps_world* w, uint64_t* n);
const kp_binding* kps_bindings(const kps_world* w, uint64_t* n);
}

typedef std::vector<std::pair<uint32_t, int32_t>> Targets;

static Targets targets_of(const uint64_t* off, const uint32_t* idx, const int32_t* rep, uint64_t i) {
  Targets t;
  for (uint64_t k = off[i]; k < off[i + 1]; k++) t.push_back({idx[k], rep[k]});
  std::sort(t.begin(), t.end());
  return t;
}

static int run_case(kp_engine* e, int config, uint64_t seed, uint32_t C, uint64_t B, bool multi) {
  kps_world* w = nullptr;
  if (kps_create(config, seed, C, 0, B, &w)) return 1;
  uint64_t nc = 0, nb = 0;
  const kp_cluster* cl = kps_clusters(w, &nc);
  const kp_binding* bs = kps_bindings(w, &nb);
  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.multiple_pod_templates_scheduling = multi ? 1 : 0;
  o.enabled_plugins = KP_PLUGIN_ALL;
  kp_snapshot* s = nullptr;
  kp_batch* b = nullptr;
  kp_results r{};
  int bad = 0;
  if (kp_snapshot_create(e, cl, nc, &o, &s) || kp_batch_create(e, s, bs, nb, &b) || kp_schedule_batch(e, b, &r)) {
    fprintf(stderr, "config %d: engine error: %s\n", config, kp_last_error(e));
    bad = 1;
  } else {
    kpo_world* ow = kpo_world_create(cl, nc, &o);
    kpo_results* want = nullptr;
    kpo_schedule(ow, bs, nb, KPO_FAST, 4, &want);
    for (uint64_t i = 0; i < nb; i++) {
      const bool same = r.status[i] == want->status[i] && r.err_code[i] == want->err_code[i] &&
                        r.err_arg[i] == want->err_arg[i] &&
                        targets_of(r.offsets, r.cluster_idx, r.replicas, i) ==
                            targets_of(want->offsets, want->cluster_idx, want->replicas, i);
      if (!same && bad++ < 3) fprintf(stderr, "config %d seed %llu binding %llu differs\n", config,
                                      (unsigned long long)seed, (unsigned long long)i);
    }
    // the same batch in the packed result form, decoded by kp_results_unpack (the wide
    // result's buffers are reused by this call, so it runs after the comparison above)
    kp_results_packed p{};
    if (kp_schedule_batch_packed(e, b, &p)) {
      fprintf(stderr, "config %d: packed: engine error: %s\n", config, kp_last_error(e));
      bad++;
    } else {
      std::vector<uint32_t> ci(p.n_targets + 1);
      std::vector<int32_t> rp(p.n_targets + 1);
      if (kp_results_unpack(&p, ci.data(), rp.data()) || p.n_bindings != nb) bad++;
      for (uint64_t i = 0; i < nb && p.n_bindings == nb; i++) {
        const bool same = p.status[i] == want->status[i] && p.err_code[i] == want->err_code[i] &&
                          p.err_arg[i] == want->err_arg[i] &&
                          targets_of(p.offsets, ci.data(), rp.data(), i) ==
                              targets_of(want->offsets, want->cluster_idx, want->replicas, i);
        if (!same && bad++ < 3) fprintf(stderr, "config %d seed %llu binding %llu differs (packed)\n", config,
                                        (unsigned long long)seed, (unsigned long long)i);
      }
    }
    // the same bindings through kp_batch_create_estimates with rows that change nothing
    // (MaxInt32: the general answer is the minimum; -1: no answer), every third binding
    // without a row: the class split, the row upload and k_est_extra run, the placements stay
    {
      std::vector<int32_t> rows(2 * nc, INT32_MAX), row_of(nb);
      std::fill(rows.begin() + (long)nc, rows.end(), -1);
      for (uint64_t i = 0; i < nb; i++) row_of[i] = (int32_t)(i % 3) - 1;
      const kp_estimates est{2, nc, rows.data(), row_of.data()};
      kp_batch* be = nullptr;
      kp_results re{};
      if (kp_batch_create_estimates(e, s, bs, nullptr, nb, nullptr, &est, &be) || kp_schedule_batch(e, be, &re)) {
        fprintf(stderr, "config %d: estimates: engine error: %s\n", config, kp_last_error(e));
        bad++;
      } else {
        for (uint64_t i = 0; i < nb; i++) {
          const bool same = re.status[i] == want->status[i] && re.err_code[i] == want->err_code[i] &&
                            re.err_arg[i] == want->err_arg[i] &&
                            targets_of(re.offsets, re.cluster_idx, re.replicas, i) ==
                                targets_of(want->offsets, want->cluster_idx, want->replicas, i);
          if (!same && bad++ < 3) fprintf(stderr, "config %d seed %llu binding %llu differs (estimates)\n", config,
                                          (unsigned long long)seed, (unsigned long long)i);
        }
      }
      if (be) kp_batch_destroy(be);
    }
    // the same bindings through kp_batch_create_filters against a registry holding one
    // out-of-tree filter plugin, with rows that reject nothing (all ones, stray bits above the
    // cluster count in the last word), every third binding without a row: the rank-order
    // upload, k_filter_extra, the merged mask and the reasons pass run, the placements stay
    {
      const uint64_t wc = (nc + 63) / 64;
      std::vector<uint64_t> rows(2 * wc, ~0ull);
      std::vector<int32_t> row_of(nb);
      for (uint64_t i = 0; i < nb; i++) row_of[i] = (int32_t)(i % 3) - 1;
      const kp_filter_answers flt{2, nc, rows.data(), row_of.data(), 1};
      kp_options o1 = o;
      o1.n_out_of_tree_plugins = 1;
      kp_snapshot* s1 = nullptr;
      kp_batch* bf = nullptr;
      kp_results rf{};
      std::vector<uint64_t> mask(nb * wc + 1);
      std::vector<uint32_t> reasons(nb * nc + 1);
      if (kp_snapshot_create(e, cl, nc, &o1, &s1) || kp_batch_create_filters(e, s1, bs, nullptr, nb, nullptr, nullptr, &flt, &bf) ||
          kp_filter_batch(e, bf, mask.data()) || kp_filter_reasons(e, bf, reasons.data()) || kp_schedule_batch(e, bf, &rf)) {
        fprintf(stderr, "config %d: filters: engine error: %s\n", config, kp_last_error(e));
        bad++;
      } else {
        for (uint64_t i = 0; i < nb; i++) {
          const bool same = rf.status[i] == want->status[i] && rf.err_code[i] == want->err_code[i] &&
                            rf.err_arg[i] == want->err_arg[i] &&
                            targets_of(rf.offsets, rf.cluster_idx, rf.replicas, i) ==
                                targets_of(want->offsets, want->cluster_idx, want->replicas, i);
          if (!same && bad++ < 3) fprintf(stderr, "config %d seed %llu binding %llu differs (filters)\n", config,
                                          (unsigned long long)seed, (unsigned long long)i);
        }
        for (uint64_t k = 0; k < nb * nc; k++)
          if ((reasons[k] & 0xff) == KP_REASON_OUT_OF_TREE && bad++ < 3)
            fprintf(stderr, "config %d: an all-ones row rejected pair %llu\n", config, (unsigned long long)k);
      }
      if (bf) kp_batch_destroy(bf);
      if (s1) kp_snapshot_destroy(s1);
    }
    kpo_results_free(want);
    kpo_world_destroy(ow);
  }
  if (b) kp_batch_destroy(b);
  if (s) kp_snapshot_destroy(s);
  kps_destroy(w);
  printf("config %d seed %llu: %llu bindings x %u clusters, %d mismatches\n", config, (unsigned long long)seed,
         (unsigned long long)nb, C, bad);
  return bad ? 1 : 0;
}

// ---- hand-built filter shapes ---------------------------------------------------
// Owns every string and array the kp_* views below point into.
struct Arena {
  std::deque<std::string> strs;
  std::deque<std::vector<kp_str>> lists;
  std::deque<std::vector<kp_requirement>> reqs;
  std::deque<std::vector<kp_cluster_affinity>> affs;
  std::deque<std::vector<kp_toleration>> tols;
  std::deque<std::vector<kp_label>> labels;
  std::deque<std::vector<kp_taint>> taints;
  std::deque<std::vector<kp_api_enablement>> apis;
  std::deque<std::vector<kp_target_cluster>> tgts;
  std::deque<std::vector<kp_affinity_term>> terms;
  kp_str s(const std::string& v) {
    strs.push_back(v);
    return kp_str{strs.back().data(), (uint32_t)strs.back().size()};
  }
  const kp_str* list(const std::vector<std::string>& v) {
    lists.emplace_back();
    for (auto& x : v) lists.back().push_back(s(x));
    return lists.back().data();
  }
  kp_requirement req(const std::string& key, const std::string& op, const std::vector<std::string>& v = {}) {
    return kp_requirement{s(key), s(op), v.empty() ? nullptr : list(v), (uint32_t)v.size()};
  }
  kp_cluster_affinity aff(const std::vector<kp_requirement>& lbl, const std::vector<kp_requirement>& fld,
                          const std::vector<std::string>& names = {}, const std::vector<std::string>& excl = {}) {
    kp_cluster_affinity a{};
    if (!lbl.empty()) {
      reqs.push_back(lbl);
      a.has_label_selector = 1;
      a.match_expressions = reqs.back().data();
      a.n_match_expressions = (uint32_t)lbl.size();
    }
    if (!fld.empty()) {
      reqs.push_back(fld);
      a.has_field_selector = 1;
      a.field_expressions = reqs.back().data();
      a.n_field_expressions = (uint32_t)fld.size();
    }
    if (!names.empty()) a.cluster_names = list(names), a.n_cluster_names = (uint32_t)names.size();
    if (!excl.empty()) a.exclude_clusters = list(excl), a.n_exclude_clusters = (uint32_t)excl.size();
    return a;
  }
};

static int run_filter_shapes(kp_engine* e) {
  Arena A;
  const int C = 131;  // three words, the last one partial
  auto sh = [](int i) { return "s" + std::to_string(i); };
  std::vector<std::string> names;
  std::vector<kp_cluster> cl(C);
  for (int i = 0; i < C; i++) {
    kp_cluster& c = cl[i];
    c = kp_cluster{};
    char nm[16];
    snprintf(nm, sizeof nm, "m-%04d", i);
    names.push_back(nm);
    c.name = A.s(nm);
    c.deleting = i % 37 == 36;
    A.labels.emplace_back();
    A.labels.back().push_back({A.s("shard"), A.s(sh(i % 97))});
    if (i % 5) A.labels.back().push_back({A.s("env"), A.s(std::string(1, (char)('a' + i % 4)))});
    c.labels = A.labels.back().data();
    c.n_labels = (uint32_t)A.labels.back().size();
    if (i % 7) c.provider = A.s(i % 2 ? "aws" : "12");
    if (i % 6) c.region = A.s(i % 3 ? "r1" : "100");
    if (i % 4) {
      c.zones = A.list({i % 2 ? "z1" : "z2", "z3"});
      c.n_zones = 2;
    }
    if (i < 40) {  // 40 taint lists of their own, plus the empty one
      A.taints.emplace_back();
      A.taints.back().push_back({A.s("k" + std::to_string(i)), A.s("v"), A.s("NoSchedule")});
      if (i % 3 == 0) A.taints.back().push_back({A.s("maint"), A.s("x"), A.s("NoExecute")});
      c.taints = A.taints.back().data();
      c.n_taints = (uint32_t)A.taints.back().size();
    }
    A.apis.emplace_back();
    if (i % 9) A.apis.back().push_back({A.s("apps/v1"), A.s("Deployment")});
    c.api_enablements = A.apis.back().data();
    c.n_api_enablements = (uint32_t)A.apis.back().size();
  }
  auto shards = [&](int lo, int hi) {
    std::vector<std::string> v;
    for (int i = lo; i < hi; i++) v.push_back(sh(i));
    return v;
  };
  auto tol = [&](const std::string& key, const std::string& op, const std::string& val, const std::string& eff) {
    return kp_toleration{A.s(key), A.s(op), A.s(val), A.s(eff)};
  };
  std::vector<kp_binding> bs;
  auto binding = [&]() -> kp_binding& {
    bs.emplace_back();
    kp_binding& b = bs.back();
    b = kp_binding{};
    b.uid = A.s("uid-" + std::to_string(bs.size()));
    b.api_version = A.s("apps/v1");
    b.kind = A.s("Deployment");
    b.namespace_ = A.s("ns");
    b.name = A.s("b" + std::to_string(bs.size()));
    b.replicas = 3;
    b.observed_affinity_name = A.s("t0");
    return b;
  };
  auto terms = [&](kp_binding& b, const std::vector<kp_cluster_affinity>& affs) {  // term t0 + overflow terms
    A.affs.emplace_back(affs.begin() + 1, affs.end());
    A.terms.emplace_back(1, kp_affinity_term{A.s("t0"), affs[0], A.affs.back().data(), (uint32_t)affs.size() - 1});
    b.cluster_affinities = A.terms.back().data();
    b.n_cluster_affinities = 1;
  };
  auto one = [&](kp_binding& b, const kp_cluster_affinity& a) {
    b.has_cluster_affinity = 1;
    b.cluster_affinity = a;
  };
  auto tols = [&](kp_binding& b, const std::vector<kp_toleration>& t) {
    A.tols.push_back(t);
    b.tolerations = A.tols.back().data();
    b.n_tolerations = (uint32_t)t.size();
  };
  const std::vector<kp_toleration> few = {tol("k1", "Exists", "", ""), tol("k2", "Equal", "v", "NoSchedule"),
                                          tol("maint", "Equal", "x", "")};
  // the matching tolerations behind more than four that match nothing (strings the snapshot knows)
  std::vector<kp_toleration> many;
  for (int j = 1; j <= 5; j++) many.push_back(tol(sh(j), "Exists", "", ""));
  many.push_back(tol("k0", "Equal", "v", ""));
  many.push_back(tol("maint", "Exists", "", ""));
  many.push_back(tol("k3", "Exists", "", "NoExecute"));
  std::vector<kp_toleration> lots;
  for (int j = 0; j < 40; j += 2) lots.push_back(tol("k" + std::to_string(j), "Exists", "", ""));

  binding();                                                          // no affinity, no toleration
  one(binding(), A.aff({A.req("env", "In", {"a"})}, {}));             // one term, one value
  one(binding(), A.aff({A.req("env", "NotIn", {"s5", "s6"})}, {}));   // values no cluster carries
  {                                                                   // several terms, several instructions
    kp_binding& b = binding();
    terms(b, {A.aff({A.req("env", "In", {"a", "b"}), A.req("shard", "NotIn", shards(0, 7))}, {A.req("provider", "In", {"aws"})}),
              A.aff({A.req("env", "DoesNotExist")}, {A.req("zone", "In", {"z1", "z3"}), A.req("region", "NotIn", {"r1"})}),
              A.aff({A.req("shard", "In", shards(3, 9))}, {A.req("zone", "DoesNotExist")}),
              A.aff({}, {A.req("region", "Exists"), A.req("provider", "Lt", {"50"})}, {}, {names[1], names[70], names[130]})});
    tols(b, few);
  }
  {                                                                   // more than 64 values, mixed with names and Gt
    kp_binding& b = binding();
    one(b, A.aff({A.req("shard", "In", shards(10, 80)), A.req("env", "Exists")}, {A.req("provider", "Gt", {"6"})},
                 std::vector<std::string>(names.begin(), names.begin() + 100)));
    tols(b, many);
  }
  one(binding(), A.aff({A.req("shard", "NotIn", shards(0, 66))}, {}));
  {                                                                   // 70 terms
    kp_binding& b = binding();
    std::vector<kp_cluster_affinity> t;
    for (int j = 0; j < 70; j++) t.push_back(A.aff({A.req("shard", "In", {sh(j)})}, {}));
    terms(b, t);
    tols(b, lots);
  }
  tols(binding(), many);
  tols(binding(), {tol("", "Exists", "", "NoSchedule")});
  for (int k = 0; k < 2; k++) {  // spec.Clusters members failing APIEnablement and TaintToleration, eviction tasks
    kp_binding& b = binding();
    b.api_version = A.s("nope/v9");
    b.kind = A.s("Thing");
    A.tgts.emplace_back();
    for (int i : {0, 1, 2, 9, 64, 130}) A.tgts.back().push_back({A.s(names[i]), 1});
    b.clusters = A.tgts.back().data();
    b.n_clusters = (uint32_t)A.tgts.back().size();
    b.eviction_from = A.list({names[0], names[64]});
    b.n_eviction_from = 2;
    if (k) one(b, A.aff({A.req("shard", "NotIn", {"s1"})}, {})), tols(b, few);
  }

  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.enabled_plugins = KP_PLUGIN_ALL;
  kp_snapshot* s = nullptr;
  kp_batch* b = nullptr;
  const uint64_t nb = bs.size(), W = (C + 63) / 64;
  std::vector<uint64_t> mask(nb * W);
  int bad = 0;
  uint64_t fit = 0;
  if (kp_snapshot_create(e, cl.data(), C, &o, &s) || kp_batch_create(e, s, bs.data(), nb, &b) ||
      kp_filter_batch(e, b, mask.data())) {
    fprintf(stderr, "filter shapes: engine error: %s\n", kp_last_error(e));
    bad = 1;
  } else {
    for (uint64_t i = 0; i < nb; i++)
      for (int c = 0; c < C; c++) {
        const bool got = (mask[i * W + (c >> 6)] >> (c & 63)) & 1;
        const bool want = !cl[c].deleting && kpo_filter(&cl[c], &bs[i], &o) == 0;
        fit += want;
        if (got != want && bad++ < 5) fprintf(stderr, "filter shapes: binding %llu cluster %d: got %d want %d\n",
                                              (unsigned long long)i, c, (int)got, (int)want);
      }
  }
  if (b) kp_batch_destroy(b);
  if (s) kp_snapshot_destroy(s);
  printf("filter shapes: %llu bindings x %d clusters, %llu fitting pairs, %d mismatches\n", (unsigned long long)nb, C,
         (unsigned long long)fit, bad);
  return bad ? 1 : 0;
}

// kp_schedule_affinities_ex with both answers over a universe with multi-term bindings: the
// rows go up once and every round's batch shares them, so the sanitizer sees them freed
// exactly once (a second free or a leak aborts the run). Three calls: rows that change
// nothing (the oracle's retry driver is the reference); rows that reject everything on each
// binding's first term and halve the estimates, so that later rounds run on the shared rows;
// and a call whose first round's batch creation fails (a binding with n_components > 0 and
// no components under the MultiplePodTemplatesScheduling gate) after the rows were made.
static int run_affinity_answers(kp_engine* e) {
  kps_world* w = nullptr;
  const uint32_t C = 150;
  if (kps_create(6, 6, C, 0, 600, &w)) return 1;
  uint64_t nc = 0, nb = 0;
  const kp_cluster* cl = kps_clusters(w, &nc);
  const kp_binding* bs = kps_bindings(w, &nb);
  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.enabled_plugins = KP_PLUGIN_ALL;
  o.n_out_of_tree_plugins = 1;
  const uint64_t wc = (nc + 63) / 64;
  std::vector<uint64_t> term_off(nb + 1, 0);
  for (uint64_t i = 0; i < nb; i++) term_off[i + 1] = term_off[i] + std::max<uint32_t>(1, bs[i].n_cluster_affinities);
  std::vector<int32_t> erows(2 * nc, INT32_MAX), erow_of(nb), frow_of(term_off[nb]);
  std::fill(erows.begin() + (long)nc, erows.end(), -1);
  for (uint64_t i = 0; i < nb; i++) erow_of[i] = (int32_t)(i % 3) - 1;
  std::vector<uint64_t> frows(2 * wc, ~0ull);  // row 0: all pass (stray bits above C); row 1: none passes
  std::fill(frows.begin() + (long)wc, frows.end(), 0ull);
  for (uint64_t k = 0; k < frow_of.size(); k++) frow_of[k] = (int32_t)(k % 2) - 1;  // -1 or the all-ones row
  const kp_estimates est{2, nc, erows.data(), erow_of.data()};
  const kp_filter_answers flt{2, nc, frows.data(), frow_of.data(), 1};
  const kp_affinity_answers ans{&est, &flt, term_off.data()};
  kp_snapshot* s = nullptr;
  kp_affinity_results r{};
  int bad = 0;
  uint64_t retried = 0;
  if (kp_snapshot_create(e, cl, nc, &o, &s) || kp_schedule_affinities_ex(e, s, bs, nb, &ans, &r)) {
    fprintf(stderr, "affinity answers: engine error: %s\n", kp_last_error(e));
    bad = 1;
  } else {
    kp_options o0 = o;
    o0.n_out_of_tree_plugins = 0;
    kpo_world* ow = kpo_world_create(cl, nc, &o0);
    kpo_results* want = nullptr;
    std::vector<int32_t> widx(nb), watt(nb);
    kpo_schedule_affinities(ow, bs, nb, KPO_FAST, 4, &want, widx.data(), watt.data());
    for (uint64_t i = 0; i < nb; i++) {
      const bool same = r.results.status[i] == want->status[i] && r.results.err_code[i] == want->err_code[i] &&
                        r.results.err_arg[i] == want->err_arg[i] && r.affinity_index[i] == widx[i] &&
                        r.attempts[i] == watt[i] &&
                        targets_of(r.results.offsets, r.results.cluster_idx, r.results.replicas, i) ==
                            targets_of(want->offsets, want->cluster_idx, want->replicas, i);
      if (!same && bad++ < 3) fprintf(stderr, "affinity answers: binding %llu differs\n", (unsigned long long)i);
    }
    kpo_results_free(want);
    kpo_world_destroy(ow);
    // every binding's first term rejected, the later ones not; small estimates
    std::fill(erows.begin(), erows.begin() + (long)nc, 1);
    for (uint64_t i = 0; i < nb; i++)
      for (uint64_t k = term_off[i]; k < term_off[i + 1]; k++) frow_of[k] = k == term_off[i] ? 1 : -1;
    if (kp_schedule_affinities_ex(e, s, bs, nb, &ans, &r)) {
      fprintf(stderr, "affinity answers: rejecting rows: engine error: %s\n", kp_last_error(e));
      bad++;
    } else {
      for (uint64_t i = 0; i < nb; i++) {
        // (a binding that resumes at a later term, or reschedules, starts where its rows allow)
        if (bs[i].n_cluster_affinities == 0 && r.results.status[i] != KP_STATUS_FIT_ERROR && bad++ < 3)
          fprintf(stderr, "affinity answers: binding %llu without terms passed an all-zero row\n", (unsigned long long)i);
        retried += r.attempts[i] >= 2;
      }
      if (r.rounds < 2 || retried == 0) bad++;
    }
  }
  if (s) kp_snapshot_destroy(s);
  // a round whose batch creation fails: the rows are up already and must go with the call
  {
    kp_options om = o;
    om.multiple_pod_templates_scheduling = 1;
    std::vector<kp_binding> broken(bs, bs + nb);
    broken[nb / 2].n_components = 1;
    broken[nb / 2].components = nullptr;
    kp_snapshot* sm = nullptr;
    if (kp_snapshot_create(e, cl, nc, &om, &sm)) {
      bad++;
    } else {
      const int rc = kp_schedule_affinities_ex(e, sm, broken.data(), nb, &ans, &r);
      if (rc != KP_EINVAL && bad++ < 3) fprintf(stderr, "affinity answers: the broken binding gave rc %d\n", rc);
      // the engine is usable afterwards, with the same rows
      if (kp_schedule_affinities_ex(e, sm, bs, nb, &ans, &r)) bad++;
    }
    if (sm) kp_snapshot_destroy(sm);
  }
  kps_destroy(w);
  printf("affinity answers: %llu bindings x %u clusters, %llu retried under rejecting rows, %d mismatches\n",
         (unsigned long long)nb, C, (unsigned long long)retried, bad);
  return bad ? 1 : 0;
}

// One batch created with both inputs (kp_batch_create_filters), scheduled twice and destroyed:
// the caller's rows go up in caller order, are ranked on the device into rows the batch
// holds, and the staging copy is let go inside the creation. The rows change nothing
// (MaxInt32 / -1 estimates, all-ones verdicts with stray bits above C), so both calls give
// the oracle's placements; the sanitizer sees the rows' block freed once, with the batch.
static int run_batch_answers(kp_engine* e) {
  kps_world* w = nullptr;
  const uint32_t C = 150;
  if (kps_create(6, 6, C, 0, 300, &w)) return 1;
  uint64_t nc = 0, nb = 0;
  const kp_cluster* cl = kps_clusters(w, &nc);
  const kp_binding* bs = kps_bindings(w, &nb);
  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.enabled_plugins = KP_PLUGIN_ALL;
  kpo_world* ow = kpo_world_create(cl, nc, &o);
  kpo_results* want = nullptr;
  kpo_schedule(ow, bs, nb, KPO_FAST, 4, &want);
  o.n_out_of_tree_plugins = 1;
  const uint64_t wc = (nc + 63) / 64;
  std::vector<int32_t> erows(2 * nc, INT32_MAX), erow_of(nb), frow_of(nb);
  std::fill(erows.begin() + (long)nc, erows.end(), -1);
  std::vector<uint64_t> frows(2 * wc, ~0ull);
  for (uint64_t i = 0; i < nb; i++) erow_of[i] = (int32_t)(i % 3) - 1, frow_of[i] = (int32_t)((i + 1) % 3) - 1;
  const kp_estimates est{2, nc, erows.data(), erow_of.data()};
  const kp_filter_answers flt{2, nc, frows.data(), frow_of.data(), 1};
  kp_snapshot* s = nullptr;
  kp_batch* b = nullptr;
  int bad = 0;
  if (kp_snapshot_create(e, cl, nc, &o, &s) || kp_batch_create_filters(e, s, bs, nullptr, nb, nullptr, &est, &flt, &b)) {
    fprintf(stderr, "batch answers: engine error: %s\n", kp_last_error(e));
    bad = 1;
  }
  for (int call = 0; call < 2 && !bad; call++) {
    kp_results r{};
    if (kp_schedule_batch(e, b, &r)) {
      fprintf(stderr, "batch answers: call %d: engine error: %s\n", call, kp_last_error(e));
      bad++;
      break;
    }
    for (uint64_t i = 0; i < nb; i++) {
      const bool same = r.status[i] == want->status[i] && r.err_code[i] == want->err_code[i] &&
                        r.err_arg[i] == want->err_arg[i] &&
                        targets_of(r.offsets, r.cluster_idx, r.replicas, i) ==
                            targets_of(want->offsets, want->cluster_idx, want->replicas, i);
      if (!same && bad++ < 3) fprintf(stderr, "batch answers: call %d binding %llu differs\n", call, (unsigned long long)i);
    }
  }
  if (b) kp_batch_destroy(b);
  if (s) kp_snapshot_destroy(s);
  kpo_results_free(want);
  kpo_world_destroy(ow);
  kps_destroy(w);
  printf("batch answers: %llu bindings x %u clusters, two calls, %d mismatches\n", (unsigned long long)nb, C, bad);
  return bad ? 1 : 0;
}

// The packer's stages on more than one thread (pack.cpp): 8 193 bindings are nine chunks on two
// packing threads (KP_PACK_THREADS=4, one per 4096 bindings at most). A keyed cold creation
// makes every record and the threads fill the cache's shards; a warm one with every tenth
// generation moved mixes hits and misses inside each chunk; both images must equal the unkeyed
// one (kp_batch_digest). Then a creation that fails after the chunks are packed (a component-set
// binding with 17 components): its new records were never handed to the cache and must be
// freed with the call (the leak check), the cache stays empty and usable.
static int run_pack_stages(kp_engine* e) {
  kps_world* w = nullptr;
  const uint32_t C = 130;
  if (kps_create(6, 21, C, 0, 8193, &w)) return 1;
  uint64_t nc = 0, nb = 0;
  const kp_cluster* cl = kps_clusters(w, &nc);
  const kp_binding* bs = kps_bindings(w, &nb);
  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.multiple_pod_templates_scheduling = 1;
  o.enabled_plugins = KP_PLUGIN_ALL;
  setenv("KP_PACK_THREADS", "4", 1);
  std::vector<kp_binding_key> cold(nb), warm(nb);
  for (uint64_t i = 0; i < nb; i++) {
    cold[i] = kp_binding_key{bs[i].uid, (int64_t)(1 + i % 5)};
    warm[i] = kp_binding_key{bs[i].uid, cold[i].generation + (i % 10 == 3)};
  }
  kp_snapshot* s = nullptr;
  kp_pack_cache* cache = nullptr;
  int bad = 0;
  uint64_t dig[3] = {0, 1, 2};
  kp_pack_cache_stats st{};
  if (kp_snapshot_create(e, cl, nc, &o, &s) || kp_pack_cache_create(0, &cache)) {
    fprintf(stderr, "pack stages: engine error: %s\n", kp_last_error(e));
    bad = 1;
  }
  for (int form = 0; form < 3 && !bad; form++) {
    kp_batch* b = nullptr;
    const int rc = form == 0 ? kp_batch_create(e, s, bs, nb, &b)
                             : kp_batch_create_keyed(e, s, bs, form == 1 ? cold.data() : warm.data(), nb, cache, &b);
    if (rc || kp_batch_digest(b, &dig[form])) {
      fprintf(stderr, "pack stages: form %d: engine error: %s\n", form, kp_last_error(e));
      bad++;
    }
    if (b) kp_batch_destroy(b);
    kp_pack_cache_get_stats(cache, &st);
    const uint64_t want_hits = form == 2 ? nb - (nb + 6) / 10 : 0;
    if (form && st.last_hits != want_hits && bad++ < 3)
      fprintf(stderr, "pack stages: form %d: %llu hits, expected %llu\n", form, (unsigned long long)st.last_hits,
              (unsigned long long)want_hits);
  }
  if (dig[1] != dig[0] || dig[2] != dig[0]) bad++;
  // the failing creation, against a cache of its own
  if (!bad) {
    std::vector<kp_binding> broken(bs, bs + nb);
    std::vector<kp_component> comps(17);
    for (auto& c : comps) c = kp_component{}, c.replicas = 1;
    kp_spread_constraint sc{};
    const std::string fld = "cluster";
    sc.spread_by_field = kp_str{fld.data(), (uint32_t)fld.size()};
    sc.min_groups = sc.max_groups = 1;
    kp_binding& x = broken[nb / 2];
    x.components = comps.data();
    x.n_components = (uint32_t)comps.size();
    x.spread_constraints = &sc;
    x.n_spread_constraints = 1;
    kp_pack_cache* c2 = nullptr;
    kp_batch* b = nullptr;
    if (kp_pack_cache_create(0, &c2)) bad++;
    const int rc = c2 ? kp_batch_create_keyed(e, s, broken.data(), cold.data(), nb, c2, &b) : 0;
    if (rc != KP_ENOTSUP && bad++ < 3) fprintf(stderr, "pack stages: the 17-component binding gave rc %d\n", rc);
    if (c2) kp_pack_cache_get_stats(c2, &st);
    if (st.entries != 0) bad++;
    if (b) kp_batch_destroy(b);
    b = nullptr;
    // the same cache takes the sound bindings afterwards
    if (c2 && (kp_batch_create_keyed(e, s, bs, cold.data(), nb, c2, &b) || kp_batch_digest(b, &dig[1]) || dig[1] != dig[0])) bad++;
    if (b) kp_batch_destroy(b);
    if (c2) kp_pack_cache_destroy(c2);
  }
  unsetenv("KP_PACK_THREADS");
  if (cache) kp_pack_cache_destroy(cache);
  if (s) kp_snapshot_destroy(s);
  kps_destroy(w);
  printf("pack stages: %llu bindings x %u clusters, unkeyed / cold / warm digests %s, %d mismatches\n",
         (unsigned long long)nb, C, dig[1] == dig[0] && dig[2] == dig[0] ? "equal" : "DIFFER", bad);
  return bad ? 1 : 0;
}

// kp_watch_create and kp_affected_bindings (watch.cpp) over a universe with multi-term
// bindings: one watch with all three modes, one call over the bitset rows and one under
// KP_PAIR_ROWS=1 with a changed set that repeats an index and ends in the partial last word,
// every binding against enqueueAffectedBindings restated over the oracle's ClusterMatches;
// then a watch made stale by another snapshot.
static int run_watch(kp_engine* e) {
  kps_world* w = nullptr;
  const uint32_t C = 130;
  if (kps_create(6, 31, C, 0, 500, &w)) return 1;
  uint64_t nc = 0, nb = 0;
  const kp_cluster* cl = kps_clusters(w, &nc);
  const kp_binding* bs = kps_bindings(w, &nb);
  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.enabled_plugins = KP_PLUGIN_ALL;
  std::vector<uint8_t> mode(nb);
  for (uint64_t i = 0; i < nb; i++) mode[i] = i % 11 == 3 ? KP_WATCH_SKIP : i % 11 == 7 ? KP_WATCH_ALWAYS : KP_WATCH_MATCH;
  const std::vector<uint32_t> changed = {0, 129, 64, 64, 5};
  std::vector<uint32_t> want;
  for (uint64_t i = 0; i < nb; i++) {
    const kp_binding& b = bs[i];
    if (mode[i] == KP_WATCH_SKIP) continue;
    const kp_cluster_affinity* a = nullptr;
    if (b.n_cluster_affinities > 0) {
      uint32_t t = 0;  // getAffinityIndex
      for (uint32_t k = 0; k < b.n_cluster_affinities && b.observed_affinity_name.len; k++) {
        const kp_str& nm = b.cluster_affinities[k].affinity_name;
        if (nm.len == b.observed_affinity_name.len &&
            std::string(nm.ptr, nm.len) == std::string(b.observed_affinity_name.ptr, nm.len)) {
          t = k;
          break;
        }
      }
      a = &b.cluster_affinities[t].affinity;
    } else if (b.has_cluster_affinity) {
      a = &b.cluster_affinity;
    }
    bool listed = mode[i] == KP_WATCH_ALWAYS || !a;
    for (uint32_t c : changed) listed = listed || kpo_cluster_matches(&cl[c], a);
    if (listed) want.push_back((uint32_t)i);
  }
  kp_snapshot *s = nullptr, *s2 = nullptr;
  kp_watch* wt = nullptr;
  int bad = 0;
  if (kp_snapshot_create(e, cl, nc, &o, &s) || kp_snapshot_create(e, cl, nc, &o, &s2) ||
      kp_watch_create(e, s, bs, nb, mode.data(), &wt)) {
    fprintf(stderr, "watch: engine error: %s\n", kp_last_error(e));
    bad = 1;
  }
  for (int rows = 0; rows < 2 && !bad; rows++) {
    if (rows) setenv("KP_PAIR_ROWS", "1", 1);
    kp_affected got{};
    if (kp_affected_bindings(e, wt, s, changed.data(), changed.size(), &got)) {
      fprintf(stderr, "watch: engine error: %s\n", kp_last_error(e));
      bad++;
    } else if (std::vector<uint32_t>(got.bindings, got.bindings + got.n) != want) {
      fprintf(stderr, "watch: rows=%d: %llu bindings listed, expected %llu\n", rows, (unsigned long long)got.n,
              (unsigned long long)want.size());
      bad++;
    }
    unsetenv("KP_PAIR_ROWS");
  }
  kp_affected none{};
  if (!bad && kp_affected_bindings(e, wt, s2, changed.data(), changed.size(), &none) != KP_ESTATE) bad++;
  if (wt) kp_watch_destroy(wt);
  if (s2) kp_snapshot_destroy(s2);
  if (s) kp_snapshot_destroy(s);
  kps_destroy(w);
  printf("watch: %llu bindings x %u clusters, %llu listed, %d mismatches\n", (unsigned long long)nb, C,
         (unsigned long long)want.size(), bad);
  return bad ? 1 : 0;
}

// kp_assumptions_create and kp_batch_create_assumed (assumed.cpp; kp_assume.h) over a universe
// with model clusters: entries on every third cluster, among them a long list, a workload
// that splits runs and one without components; the assumed batch scheduled on the class rows
// and under KP_PAIR_ROWS=1 (both must place alike), an n == 0 handle against the plain batch,
// then the run-capacity refusal.
static int run_assumed(kp_engine* e) {
  kps_world* w = nullptr;
  const uint32_t C = 130;
  if (kps_create(6, 13, C, 0, 400, &w)) return 1;
  uint64_t nc = 0, nb = 0;
  const kp_cluster* cl = kps_clusters(w, &nc);
  const kp_binding* bs = kps_bindings(w, &nb);
  kp_options o{};
  o.customized_cluster_resource_modeling = 1;
  o.enabled_plugins = KP_PLUGIN_ALL;
  const char *cpu = "cpu", *mem = "memory", *q1 = "750m", *q2 = "1Gi";
  kp_resource rq[2] = {{{cpu, 3}, {q1, 4}}, {{mem, 6}, {q2, 3}}};
  kp_component comps[3] = {};
  comps[0].replicas = 3;
  comps[0].has_replica_requirements = 1;
  comps[0].resource_request = rq;
  comps[0].n_resource_request = 2;
  comps[1].replicas = 2;
  comps[2].replicas = 0;
  std::vector<kp_assumed_entry> en;
  for (uint32_t c = 0; c < C; c += 3)
    for (int k = 0; k < (c == 63 ? 200 : 3); k++) en.push_back(kp_assumed_entry{c, comps, (uint32_t)(k % 4)});
  kp_snapshot* s = nullptr;
  kp_assumptions *a = nullptr, *a0 = nullptr, *a1 = nullptr;
  kp_batch *b = nullptr, *b0 = nullptr, *bp = nullptr;
  int bad = 0;
  if (kp_snapshot_create(e, cl, nc, &o, &s) || kp_assumptions_create(e, s, en.data(), en.size(), &a) ||
      kp_assumptions_create(e, s, nullptr, 0, &a0) || kp_batch_create_assumed(e, s, a, bs, nb, &b) ||
      kp_batch_create_assumed(e, s, a0, bs, nb, &b0) || kp_batch_create(e, s, bs, nb, &bp)) {
    fprintf(stderr, "assumed: engine error: %s\n", kp_last_error(e));
    bad = 1;
  }
  auto flat = [](const kp_results& r) {
    std::vector<int64_t> v(r.status, r.status + r.n_bindings);
    const size_t t0 = v.size();
    for (uint64_t i = 0; i < r.n_targets; i++) v.push_back(((int64_t)r.cluster_idx[i] << 32) | (uint32_t)r.replicas[i]);
    for (uint64_t b = 0; b < r.n_bindings; b++)  // (a binding's targets compare as a multiset)
      std::sort(v.begin() + t0 + r.offsets[b], v.begin() + t0 + r.offsets[b + 1]);
    return v;
  };
  if (!bad) {
    kp_results r{};
    std::vector<int64_t> rows, cls, plain, none;
    bad += kp_schedule_batch(e, b, &r) != 0;
    cls = flat(r);
    setenv("KP_PAIR_ROWS", "1", 1);
    bad += kp_schedule_batch(e, b, &r) != 0;
    rows = flat(r);
    unsetenv("KP_PAIR_ROWS");
    bad += kp_schedule_batch(e, bp, &r) != 0;
    plain = flat(r);
    bad += kp_schedule_batch(e, b0, &r) != 0;
    none = flat(r);
    if (cls != rows || plain != none || cls == plain) {
      fprintf(stderr, "assumed: class rows %s pair rows, n == 0 %s plain, assumed %s plain\n", cls == rows ? "==" : "!=",
              plain == none ? "==" : "!=", cls == plain ? "==" : "!=");
      bad++;
    }
    setenv("KP_ASSUME_RUNS_CAP", "1", 1);
    if (kp_assumptions_create(e, s, en.data(), en.size(), &a1) != KP_ENOTSUP) bad++;
    unsetenv("KP_ASSUME_RUNS_CAP");
  }
  for (kp_batch* x : {b, b0, bp})
    if (x) kp_batch_destroy(x);
  for (kp_assumptions* x : {a, a0, a1})
    if (x) kp_assumptions_destroy(x);
  if (s) kp_snapshot_destroy(s);
  kps_destroy(w);
  printf("assumed: %llu bindings x %u clusters, %zu entries, %d mismatches\n", (unsigned long long)nb, C, en.size(), bad);
  return bad ? 1 : 0;
}

// `driver ceiling`: the snapshots at which a workgroup's LDS is full (tests/test_lds_ceiling.py:
// 18 624 clusters without spread bindings, 14 336 with them, and the class-order switch at
// 16 384 / 16 385) instead of the small universes, so the sanitizer sees every global array
// at its largest supported size.
int main(int argc, char** argv) {
  kp_engine* e = nullptr;
  if (kp_engine_create(0, &e)) return 2;
  int fails = 0;
  const bool ceiling = argc > 1 && std::string(argv[1]) == "ceiling";
  std::vector<std::tuple<int, uint64_t, uint32_t, uint64_t, bool>> cases = {
      {3, 3, 120, 200, false}, {4, 4, 200, 300, false}, {6, 6, 150, 600, false}, {6, 9, 257, 300, true},
      {7, 17, 200, 300, false}, {8, 4, 64, 150, false}, {9, 1, 150, 300, true}, {2, 2, 200, 200, false},
  };
  if (ceiling)
    cases = {{3, 5, 18624, 100, false},  {7, 5, 18624, 100, false},  {10, 5, 18624, 100, false},
             {4, 5, 14336, 100, false},  {5, 5, 14336, 100, false},  {6, 5, 14336, 100, false},
             {3, 5, 16384, 100, false},  {10, 5, 16385, 100, false}, {7, 5, 16385, 100, false}};
  for (auto& c : cases) fails += run_case(e, std::get<0>(c), std::get<1>(c), std::get<2>(c), std::get<3>(c), std::get<4>(c));
  if (!ceiling) fails += run_filter_shapes(e);
  if (!ceiling) fails += run_affinity_answers(e);
  if (!ceiling) fails += run_batch_answers(e);
  if (!ceiling) fails += run_pack_stages(e);
  if (!ceiling) fails += run_watch(e);
  if (!ceiling) fails += run_assumed(e);
  kp_engine_destroy(e);
  printf("%s\n", fails ? "FAIL" : "ok");
  return fails ? 1 : 0;
}
