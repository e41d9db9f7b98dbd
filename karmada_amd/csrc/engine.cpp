// engine.cpp — host side of the kp placement engine: kp_engine_* and the schedule, filter,
// score, diagnosis and component-set entry points of include/kp/kp_api.h (the snapshots are in
// snapshot.cpp, the binding packer and batch creation in pack.cpp, the node estimator in
// nodes.cpp, the cluster-event watch in watch.cpp). Kernel orchestration on the engine's HIP streams, the host-kept selectGroups
// step, and the one definition of kp_host.h's shared state.
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

namespace {

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

}  // namespace

namespace kp::host {

// MaxDivided table entries staged per workgroup: the snapshot's template count.
int md_cap_of(const kp_snapshot* s) { return s->n_tmpl <= kMdCap ? std::max(kTmplDense, s->n_tmpl) : 0; }
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

}  // namespace kp::host

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
  buf_pool().put(-1, e->affected.h, e->affected.bytes);
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

// The delta result form's buffers, allocated on the batch's first delta call (kp_host.h; a
// batch never scheduled in this form allocates and uploads nothing for it). The list of
// long-list bindings is made here from the host headers and uploaded on the call's stream.
static int ensure_delta(kp_engine* e, kp_batch* bt) {
  const size_t B = (size_t)std::max(1, bt->B);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  if (!bt->dflag_d) {
    std::vector<int32_t> longs;
    for (int b = 0; b < bt->B; b++)
      if (changed_long(bt->hdr[b])) longs.push_back(b);
    if (!longs.empty() && changed_lds_bytes(bt->snap->Cp) > e->max_lds) {
      e->err = "delta results: snapshot too large for one workgroup's LDS (" +
               std::to_string(changed_lds_bytes(bt->snap->Cp)) + " > " + std::to_string(e->max_lds) + " bytes)";
      return KP_ENOTSUP;
    }
    const size_t o_cnt = up(4 * B), o_chg = o_cnt + up(4 * B), o_off = o_chg + up(4 * B),
                 o_moff = o_off + up(8 * (B + 1)), o_out = o_moff + up(8 * (B + 1)), o_long = o_out + up(8 * (B + 1));
    void* p = nullptr;
    if (dev::alloc(&p, o_long + 4 * std::max<size_t>(1, longs.size()))) {
      e->err = std::string("delta results: ") + dev::last_error();
      return KP_EDEVICE;
    }
    char* q = (char*)p;
    if (!longs.empty() && (dev::h2d(q + o_long, longs.data(), 4 * longs.size(), e->stream) || dev::sync(e->stream))) {
      e->err = std::string("delta results: ") + dev::last_error();
      dev::release(p);
      return KP_EDEVICE;
    }
    bt->dflag_d = (uint32_t*)q;
    bt->dcount_d = (uint32_t*)(q + o_cnt);
    bt->dchanged_d = (uint32_t*)(q + o_chg);
    bt->dchg_off_d = (uint64_t*)(q + o_off);
    bt->dmoff_d = (uint64_t*)(q + o_moff);
    bt->dout_off_d = (uint64_t*)(q + o_out);
    bt->dlong_d = (int32_t*)(q + o_long);
    bt->n_dlong = (int)longs.size();
  }
  if (!bt->h_delta) {
    bt->h_delta = (uint64_t*)pinned_get(32 + 8 * (B + 1) + 4 * B, &bt->h_delta_bytes);
    if (!bt->h_delta) {
      e->err = "delta results: page-locked buffers";
      return KP_ENOMEM;
    }
  }
  return KP_OK;
}

}  // extern "C"

// Per-kernel profiling (kp_engine_set_profile): prof_begin records the start event of
// launch i on its stream, prof_end its end event and what it covered (kp_host.h: watch.cpp
// records its launches through the same three).
int prof_begin(kp_engine* e, dev::stream_t st) {
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
void prof_end(kp_engine* e, int i, dev::stream_t st, const char* name, uint64_t units, int units_stat) {
  if (i < 0) return;
  (void)dev::event_record(e->pev[2 * (size_t)i + 1], st);
  e->pk[i] = {name, units, units_stat};
}
// After the batch's final sync: each kernel's launches folded by name.
void prof_fold(kp_engine* e, const uint32_t* h_stats) {
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

extern "C" {

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
// kp_results_packed. delta: k_changed compares every result with the binding's spec.Clusters,
// and only the changed bindings' results are compacted and copied back (kp_results_delta).
//
// schedule_submit queues the call in six stages (submit_rows ... submit_results, in that
// order) over the engine's three streams; SubmitCtx is what the stages share.
enum ResultForm : int { RF_WIDE = 0, RF_PACKED, RF_DELTA };
struct SubmitCtx {
  kp_engine* e;
  kp_batch* bt;
  kp_snapshot* s;
  ResultForm form;
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

  SubmitCtx(kp_engine* e_, kp_batch* bt_, ResultForm form_) : e(e_), bt(bt_), s(bt_->snap), form(form_) {
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
  if (bt->assumed && (bt->assumed->epoch != s->epoch || bt->assumed->updates != s->updates)) {
    e->err = "the snapshot was updated after the batch's assumed workloads were deducted from it";
    return KP_ESTATE;
  }
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
    // the assumed workloads deducted at their clusters, written over the rows' entries before
    // any reader (a batch with singleton classes has no class orders: its feasible-only rows
    // are written after k_filter, and the correction follows them there)
    if (bt->assumed && !single)
      KPROF(sp, "k_est_assumed", bt->crep.size(), -1,
            dev::est_assumed(sp, s->view, bt->view, bt->assumed->view, EA_CLASS, bt->d_crep, nullptr, 0,
                             (int)bt->crep.size(), bt->cls_rows));
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
    if (bt->assumed && single)
      KPROF(sp, "k_est_assumed", bt->crep.size(), -1,
            dev::est_assumed(sp, s->view, bt->view, bt->assumed->view, EA_CLASS, bt->d_crep, nullptr, 0,
                             (int)bt->crep.size(), bt->cls_rows));
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
    // pair-row mode: the bindings' own rows at the assumed clusters, as the pair kernel writes them
    if (bt->assumed)
      KPROF(sp, "k_est_assumed", B, -1,
            dev::est_assumed(sp, s->view, bt->view, bt->assumed->view, EA_MERGED, nullptr, bt->fmask, 0, B, bt->est));
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
// The delta form keeps the first scan for its total alone (n_targets_all), then k_changed /
// k_changed_long write each binding's flag and masked count, both are scanned (off_part
// again, as the packed form's second scan), k_compact gathers the changed bindings' results
// over the masked offsets and k_changed_list writes their indices and offsets; of the
// arrays sized by B only the three status arrays are read back.
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
  if (c.form == RF_DELTA) {
    KPROF(st, "k_changed", B, -1,
          dev::changed(st, bt->view, bt->status, bt->start, bt->count, bt->out_idx, bt->out_rep, bt->dflag_d,
                       bt->dcount_d));
    if (bt->n_dlong)
      KPROF(st, "k_changed_long", bt->n_dlong, -1,
            dev::changed_long(st, s->view, bt->view, bt->dlong_d, bt->n_dlong, bt->status, bt->start, bt->count,
                              bt->out_idx, bt->out_rep, bt->dflag_d, bt->dcount_d));
    HIPCHK(dev::d2h(bt->h_delta + 2, bt->offsets_d + B, 8, st));  // n_targets_all, before off_part is reused
    KPROF(st, "k_offsets", B, -1, dev::offsets(st, bt->status, bt->dcount_d, B, bt->dmoff_d, bt->off_part));
    KPROF(st, "k_offsets", B, -1, dev::offsets(st, bt->status, bt->dflag_d, B, bt->dchg_off_d, bt->off_part));
    KPROF(st, "k_compact", B, -1,
          dev::compact(st, bt->start, bt->dcount_d, bt->dmoff_d, bt->out_idx, bt->out_rep, bt->cidx_d, bt->crep_d, B,
                       s->view.perm));
    KPROF(st, "k_changed_list", B, -1,
          dev::changed_list(st, B, bt->dflag_d, bt->dchg_off_d, bt->dmoff_d, bt->dchanged_d, bt->dout_off_d));
    HIPCHK(dev::d2h(bt->h_delta, bt->dchg_off_d + B, 8, st));
    HIPCHK(dev::d2h(bt->h_delta + 1, bt->dmoff_d + B, 8, st));
  } else if (c.form == RF_PACKED) {
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
  if (c.form != RF_DELTA) bt->h_offsets.resize(B + 1);
  HIPCHK(dev::d2h(bt->h_status.data(), bt->status, 4 * (size_t)B, st));
  HIPCHK(dev::d2h(bt->h_err.data(), bt->errc, 4 * (size_t)B, st));
  HIPCHK(dev::d2h(bt->h_arg.data(), bt->arg, 8 * (size_t)B, st));
  if (c.form != RF_DELTA) HIPCHK(dev::d2h(bt->h_offsets.data(), bt->offsets_d, 8 * (size_t)(B + 1), st));
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

static int schedule_submit(kp_engine* e, kp_batch* bt, ResultForm form) {
  const bool packed = form == RF_PACKED;
  if (!e || !bt) return KP_EINVAL;
  if (int rc = refuse_out_of_tree(e, bt->snap, bt->flt_plugins)) return rc;
  (void)dev::set_device(e->device);
  kp_snapshot* s = bt->snap;
  if (packed && s->C > 65536) {  // (kp_batch_create's LDS bound refuses such snapshots long before)
    e->err = "kp_schedule_batch_packed: a packed cluster index holds 16 bits (more than 65536 clusters)";
    return KP_ENOTSUP;
  }
  if (packed && ensure_packed(e, bt)) return KP_EDEVICE;
  if (form == RF_DELTA)
    if (int rc = ensure_delta(e, bt)) return rc;
  SchedPend& pd = bt->pend;
  {
    const dev::event_t ev = pd.ev;  // (the event is kept across calls)
    pd = SchedPend{};
    pd.ev = ev;
  }
  bt->sched_done = false;
  pd.packed = packed;
  pd.delta = form == RF_DELTA;
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
  SubmitCtx c(e, bt, form);
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

// Exactly one of out / pout / dout is given: the format the caller collects in, which must
// be the one the call was submitted in.
static int schedule_finish(kp_engine* e, kp_batch* bt, kp_results* out, kp_results_packed* pout,
                           kp_results_delta* dout = nullptr) {
  if (!e || !bt || (!out && !pout && !dout)) return KP_EINVAL;
  SchedPend& pd = bt->pend;
  if (!pd.live) {
    e->err = "kp_schedule_batch_collect: the batch has no submitted call";
    return KP_ESTATE;
  }
  const bool packed = pout != nullptr, delta = dout != nullptr;
  if (pd.packed != packed || pd.delta != delta) {  // (the call stays submitted, for the right function to collect)
    static const char* const fn[3] = {"kp_schedule_batch_collect", "kp_schedule_batch_collect_packed",
                                      "kp_schedule_batch_collect_delta"};
    static const char* const is[3] = {"wide", "packed", "delta"};
    const int sub = pd.delta ? 2 : pd.packed ? 1 : 0;
    e->err = std::string(fn[delta ? 2 : packed ? 1 : 0]) + ": the submitted call is " + is[sub] + " (" + fn[sub] + ")";
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
    if (delta) {
      memset(dout, 0, sizeof(*dout));
      dout->offsets = bt->h_offsets.data();
    } else {
      packed ? none(pout) : none(out);
    }
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
  // (a delta call: the CSR of the changed bindings alone, h_delta[1] entries)
  const uint64_t tot = delta ? bt->h_delta[1] : bt->h_offsets[B];
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
  uint64_t n_changed = delta ? bt->h_delta[0] : 0, n_all = delta ? bt->h_delta[2] : 0;
  uint64_t* const d_off = bt->h_delta ? bt->h_delta + 4 : nullptr;
  uint32_t* const d_chg = bt->h_delta ? (uint32_t*)(bt->h_delta + 4 + (size_t)std::max(1, B) + 1) : nullptr;
  if (delta) {
    HIPCHK(dev::d2h(d_off, bt->dout_off_d, 8 * (n_changed + 1), st));
    HIPCHK(dev::d2h(d_chg, bt->dchanged_d, 4 * n_changed, st));
    if (tot) HIPCHK(dev::d2h(bt->h_cidx, bt->cidx_d, 4 * tot, st));
    if (tot) HIPCHK(dev::d2h(bt->h_crep, bt->crep_d, 4 * tot, st));
    HIPCHK(dev::sync(st));
  } else if (packed) {
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
  const bool any_ovf = std::any_of(sets_ovf.begin(), sets_ovf.end(), [](uint32_t v) { return v != 0; });
  if (any_ovf && delta) {
    // (the failed bindings leave the changed list, and n_targets_all loses their targets,
    // changed or not: the one case that reads the batch's full offsets back)
    bt->h_offsets.resize(B + 1);
    HIPCHK(dev::d2h(bt->h_offsets.data(), bt->offsets_d, 8 * (size_t)(B + 1), st));
    HIPCHK(dev::sync(st));
    for (int32_t b : bt->l_sets)
      if (bt->h_err[b] == KP_ERR_SETS_CAPACITY && bt->h_status[b] == KP_STATUS_ERROR)
        n_all -= bt->h_offsets[b + 1] - bt->h_offsets[b];
    uint64_t w = 0, nc = 0;
    for (uint64_t i = 0; i < n_changed; i++) {
      const uint64_t lo = d_off[i], hi = d_off[i + 1];
      const uint32_t b = d_chg[i];
      if (bt->h_status[b] != KP_STATUS_OK) continue;
      d_chg[nc] = b;
      d_off[nc++] = w;
      for (uint64_t k = lo; k < hi; k++, w++) {
        bt->h_cidx[w] = bt->h_cidx[k];
        bt->h_crep[w] = bt->h_crep[k];
      }
    }
    d_off[nc] = w;
    n_changed = nc;
  } else if (any_ovf) {
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
  const uint64_t tot_out = delta ? d_off[n_changed] : bt->h_offsets[B];
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
  if (delta) {
    dout->n_bindings = (uint64_t)B;
    dout->status = bt->h_status.data();
    dout->err_code = bt->h_err.data();
    dout->err_arg = bt->h_arg.data();
    dout->n_changed = n_changed;
    dout->changed = d_chg;
    dout->offsets = d_off;
    dout->cluster_idx = bt->h_cidx;
    dout->replicas = bt->h_crep;
    dout->n_targets = tot_out;
    dout->n_targets_all = n_all;
  } else if (packed) {
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

// The wide, the packed and the delta entry points share one body per call. The one-shot
// call: exactly one of out / pout / dout is given, as for schedule_finish.
static int schedule_both(kp_engine* e, kp_batch* bt, kp_results* out, kp_results_packed* pout,
                         kp_results_delta* dout = nullptr) {
  if (!out && !pout && !dout) return KP_EINVAL;
  if (int rc = schedule_submit(e, bt, dout ? RF_DELTA : pout ? RF_PACKED : RF_WIDE)) return rc;
  return schedule_finish(e, bt, out, pout, dout);
}
// The submit call; `who` names the entry point in the error texts.
static int submit_call(kp_engine* e, kp_batch* bt, ResultForm form, const char* who) {
  if (e && e->prof) {
    e->err = std::string(who) + ": per-kernel profiling covers kp_schedule_batch only";
    return KP_EINVAL;
  }
  if (!e || !bt) return KP_EINVAL;
  if (bt->pend.live) {
    e->err = std::string(who) + ": the batch's previous call is not collected";
    return KP_ESTATE;
  }
  return batch_fence(e, bt, schedule_submit(e, bt, form));
}
int kp_schedule_batch(kp_engine* e, kp_batch* bt, kp_results* out) { return batch_fence(e, bt, schedule_both(e, bt, out, nullptr)); }
int kp_schedule_batch_submit(kp_engine* e, kp_batch* bt) {
  return submit_call(e, bt, RF_WIDE, "kp_schedule_batch_submit");
}
int kp_schedule_batch_collect(kp_engine* e, kp_batch* bt, kp_results* out) {
  return batch_fence(e, bt, schedule_finish(e, bt, out, nullptr));
}
// The packed result form (kp_results_packed): the same calls with packed = true.
int kp_schedule_batch_packed(kp_engine* e, kp_batch* bt, kp_results_packed* out) {
  return batch_fence(e, bt, schedule_both(e, bt, nullptr, out));
}
int kp_schedule_batch_submit_packed(kp_engine* e, kp_batch* bt) {
  return submit_call(e, bt, RF_PACKED, "kp_schedule_batch_submit_packed");
}
int kp_schedule_batch_collect_packed(kp_engine* e, kp_batch* bt, kp_results_packed* out) {
  return batch_fence(e, bt, schedule_finish(e, bt, nullptr, out));
}
// The delta result form (kp_results_delta): the same calls with the changed bindings alone.
int kp_schedule_batch_delta(kp_engine* e, kp_batch* bt, kp_results_delta* out) {
  return batch_fence(e, bt, schedule_both(e, bt, nullptr, nullptr, out));
}
int kp_schedule_batch_submit_delta(kp_engine* e, kp_batch* bt) {
  return submit_call(e, bt, RF_DELTA, "kp_schedule_batch_submit_delta");
}
int kp_schedule_batch_collect_delta(kp_engine* e, kp_batch* bt, kp_results_delta* out) {
  if (e && e->prof) {  // (a call submitted before profiling was turned on stays collectable after it is off)
    e->err = "kp_schedule_batch_collect_delta: per-kernel profiling covers the one-call forms only";
    return KP_EINVAL;
  }
  return batch_fence(e, bt, schedule_finish(e, bt, nullptr, nullptr, out));
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

namespace kp::host {

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

}  // namespace kp::host

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
  if (bt->assumed)  // the answer over the deducted availability
    HIPCHK(dev::est_assumed(e->stream, s->view, bt->view, bt->assumed->view, EA_RAW, nullptr, nullptr, (int)binding, 1,
                            bt->est));
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

// kp_affinity_answers checked by the shared intake (kp_host.h), with the rules of term_off,
// which the verdicts' row_of is indexed through (one entry per binding and term), here.
static int check_affinity_answers(kp_engine* e, const kp_snapshot* s, const kp_binding* bs, uint64_t n,
                                  const kp_estimates* est, const kp_filter_answers* flt, const uint64_t* term_off) {
  const char* who = "kp_schedule_affinities_ex";
  auto bad = [&](const std::string& why) {
    e->err = std::string(who) + ": " + why;
    return KP_EINVAL;
  };
  if (int rc = check_estimates(e, s, who, "est->", est, n)) return rc;
  if (int rc = check_filters(e, s, who, "flt->", flt, n)) return rc;
  if (!flt || flt->n_rows == 0) return KP_OK;
  if (!term_off) return bad("term_off is null while flt has rows");
  for (uint64_t i = 0; i < n; i++)
    if (term_off[i + 1] < term_off[i])
      return bad("term_off is not non-decreasing: term_off[" + std::to_string(i + 1) + "] is below term_off[" +
                 std::to_string(i) + "]");
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t terms = std::max<uint32_t>(1, bs[i].n_cluster_affinities);
    if (term_off[i + 1] - term_off[i] != terms)
      return bad("term_off[" + std::to_string(i + 1) + "] - term_off[" + std::to_string(i) + "] is " +
                 std::to_string(term_off[i + 1] - term_off[i]) + ", binding " + std::to_string(i) + " has " +
                 std::to_string(terms) + " term(s) (max(1, n_cluster_affinities))");
    if (int rc = check_row_of(e, who, "flt->", flt->row_of, term_off[i], terms, flt->n_rows)) return rc;
  }
  return KP_OK;
}

int kp_schedule_affinities(kp_engine* e, const kp_snapshot* s, const kp_binding* bs, uint64_t n,
                           kp_affinity_results* out) {
  return kp_schedule_affinities_ex(e, s, bs, n, nullptr, out);
}

int kp_schedule_affinities_ex(kp_engine* e, const kp_snapshot* s, const kp_binding* bs, uint64_t n,
                              const kp_affinity_answers* ans, kp_affinity_results* out) {
  if (!e || !s || !out || (n && !bs)) return KP_EINVAL;
  const kp_estimates* est = ans ? ans->est : nullptr;
  const kp_filter_answers* flt = ans ? ans->flt : nullptr;
  const uint32_t flt_plugins = flt ? flt->n_plugins : 0;
  if (int rc = refuse_out_of_tree(e, s, flt_plugins)) return rc;
  if (int rc = check_affinity_answers(e, s, bs, n, est, flt, ans ? ans->term_off : nullptr)) return rc;
  const uint64_t* term_off = ans ? ans->term_off : nullptr;
  // rows that no binding uses merge nothing: the call then runs as without them
  auto used = [](const int32_t* row_of, uint64_t m) {
    for (uint64_t k = 0; k < m; k++)
      if (row_of[k] >= 0) return true;
    return false;
  };
  if (est && !(est->n_rows && used(est->row_of, n))) est = nullptr;
  if (flt && !(flt->n_rows && n && used(flt->row_of + term_off[0], term_off[n] - term_off[0]))) flt = nullptr;
  // The rows go up once and come into rank order on the device; every round's batch shares
  // them, and they go back to the pool with the last holder, whichever way the call returns.
  std::shared_ptr<const AnswerRows> rows;
  if (est || flt) {
    (void)dev::set_device(e->device);
    // (KP_PACK_TIMING: the two kernels' times between the engine's stage events, idle here)
    const dev::event_t tev[3] = {e->ev[EV_ROWS_BEGIN], e->ev[EV_ROWS_END], e->ev[EV_SELECT_BEGIN]};
    const bool timing = kp_env_flag("KP_PACK_TIMING");
    Arena staging;
    if (int rc = make_answer_rows(e, s, est, flt, e->stream, &staging, timing ? tev : nullptr, &rows)) {
      (void)dev::sync(e->stream);  // (what was queued uses the blocks that go back to the pool)
      return rc;
    }
    HIPCHK(dev::sync(e->stream));  // (the caller's rows are read; the batches' streams may start)
    if (timing)
      fprintf(stderr, "kp_schedule_affinities_ex: k_est_rows_rank %u rows %.1f us, k_flt_rows_rank %u rows %.1f us, %zu bytes uploaded\n",
              rows->n_est, 1e3 * dev::event_ms(tev[0], tev[1]), rows->n_flt, 1e3 * dev::event_ms(tev[1], tev[2]),
              4 * (size_t)rows->n_est * s->C + 8 * (size_t)rows->n_flt * (((size_t)s->C + 63) / 64));
  }
  std::vector<int32_t> sub_est;
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
    // this round's row_of and (binding, row) pairs from the pending list and each current term
    BatchAnswers a;
    a.rows = rows;
    a.flt_plugins = flt_plugins;
    if (est) {
      sub_est.resize(pending.size());
      for (size_t j = 0; j < pending.size(); j++) sub_est[j] = est->row_of[pending[j]];
      a.est_row_of = sub_est.data();
    }
    if (flt)
      for (size_t j = 0; j < pending.size(); j++) {
        const uint64_t i = pending[j];
        const int32_t r = flt->row_of[term_off[i] + (bs[i].n_cluster_affinities ? cur[i] : 0)];
        if (r >= 0) a.flt_list.push_back(FltPair{(int32_t)j, r});
      }
    int rc = batch_create_with(e, s, sub.data(), sub.size(), nullptr, nullptr, &a, &bt);
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
