// kp_host.h — what the host units of the kp placement engine share: the string map, the
// dictionaries, the buffer pool and the arena (namespace kp::host), the three ABI objects
// of include/kp/kp_api.h, and the declarations of the helpers that cross a unit boundary.
#pragma once

#include "kp_dev.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <tuple>
#include <type_traits>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/kp/kp_api.h"
#include "k8s.h"
#include "kp_env.h"
#include "kp_layout.h"
#include "kp_launch.h"
#include "kp_sets.h"  // (the one device-body header here: kp_batch holds SetsArgs by value)
#include "kp_assume.h"  // (AssumedView alone: kp_assumptions holds it by value)

using namespace kp;

namespace kp::host {

inline std::string S(const kp_str& s) { return (s.ptr && s.len) ? std::string(s.ptr, s.len) : std::string(); }
inline std::string_view SV(const kp_str& s) { return (s.ptr && s.len) ? std::string_view(s.ptr, s.len) : std::string_view(); }
inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// String-keyed hash table with string_view lookups for the packing hot path (names,
// dictionary strings, memo keys): open addressing with linear probing over a
// power-of-two slot array kept at most half full, one multiply-xorshift hash over
// 8-byte words per lookup, entries in a deque (stable addresses). find() returns the
// entry or nullptr (== end()); it->first / it->second as with std::unordered_map.
inline uint64_t sv_hash(std::string_view v) {
  const unsigned char* p = (const unsigned char*)v.data();
  size_t n = v.size();
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
  for (; n >= 8; n -= 8, p += 8) {
    uint64_t w;
    memcpy(&w, p, 8);
    h = (h ^ w) * 0xff51afd7ed558ccdull;
    h ^= h >> 32;
  }
  uint64_t w = 0;
  memcpy(&w, p, n);
  h = (h ^ w) * 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 29;
  return h | 1;  // 0 marks an empty slot
}
template <class V>
class SvMap {
 public:
  struct Entry {
    std::string first;
    V second;
  };
  Entry* find(std::string_view k) {
    if (slots_.empty()) return nullptr;
    const uint64_t h = sv_hash(k);
    for (size_t i = h & mask_;; i = (i + 1) & mask_) {
      const Slot& sl = slots_[i];
      if (sl.h == 0) return nullptr;
      if (sl.h == h && ent_[sl.i].first == k) return &ent_[sl.i];
    }
  }
  const Entry* find(std::string_view k) const { return const_cast<SvMap*>(this)->find(k); }
  Entry* end() const { return nullptr; }
  template <class K, class W>
  std::pair<Entry*, bool> emplace(K&& k, W&& v) {
    if (Entry* e = find(std::string_view(k))) return {e, false};
    if (2 * (ent_.size() + 1) > slots_.size()) grow();
    ent_.push_back(Entry{std::string(std::forward<K>(k)), V(std::forward<W>(v))});
    put(sv_hash(ent_.back().first), (uint32_t)(ent_.size() - 1));
    return {&ent_.back(), true};
  }
  V& operator[](std::string_view k) { return emplace(std::string(k), V()).first->second; }
  size_t size() const { return ent_.size(); }

 private:
  struct Slot {
    uint64_t h = 0;
    uint32_t i = 0;
  };
  std::vector<Slot> slots_;
  std::deque<Entry> ent_;
  size_t mask_ = 0;
  void put(uint64_t h, uint32_t i) {
    size_t j = h & mask_;
    while (slots_[j].h != 0) j = (j + 1) & mask_;
    slots_[j] = Slot{h, i};
  }
  void grow() {
    const size_t cap = std::max<size_t>(16, 2 * slots_.size());
    slots_.assign(cap, Slot{});
    mask_ = cap - 1;
    for (uint32_t i = 0; i < (uint32_t)ent_.size(); i++) put(sv_hash(ent_[i].first), i);
  }
};

struct Dict {
  SvMap<int32_t> m;
  std::vector<std::string> names;
  int32_t add(const std::string& s) {
    auto it = m.find(s);
    if (it != m.end()) return it->second;
    int32_t id = (int32_t)names.size();
    m.emplace(s, id);
    names.push_back(s);
    return id;
  }
  int32_t get(std::string_view s) const {
    auto it = m.find(s);
    return it == m.end() ? -1 : it->second;
  }
};

// Process-wide pools of freed batch buffers: a batch's device arena (per device)
// and its page-locked result buffers go back here on kp_batch_destroy and the next
// batch of a fitting size takes them, so a stream of batches pays hipMalloc /
// hipHostMalloc (and the frees) once. A block is reused for requests of at least
// half its size. Each pool (one per device, one for page-locked host memory) keeps
// at most kPoolKeep blocks and kPoolBytes (device) / kPoolHostBytes (host) bytes,
// oldest evicted first: several engines' batches in flight (bench lanes, kp_multi)
// each hold an arena and two host buffers.
struct BufPool {
  static constexpr size_t kPoolKeep = 32;
  static constexpr size_t kPoolBytes = (size_t)16 << 30;     // per device (288 GB of HBM)
  static constexpr size_t kPoolHostBytes = (size_t)4 << 30;  // page-locked host memory
  std::mutex mu;
  std::vector<std::tuple<int, void*, size_t>> free;  // (device or -1 for host, pointer, bytes), oldest first
  void* get(int dev_id, size_t bytes, size_t* got) {
    std::lock_guard<std::mutex> g(mu);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < free.size(); i++) {
      auto& [d, p, n] = free[i];
      if (d == dev_id && n >= bytes && n <= 2 * bytes + (1u << 20) && (best == (size_t)-1 || n < std::get<2>(free[best])))
        best = i;
    }
    if (best == (size_t)-1) return nullptr;
    void* p = std::get<1>(free[best]);
    *got = std::get<2>(free[best]);
    free.erase(free.begin() + (long)best);
    return p;
  }
  void put(int dev_id, void* p, size_t bytes) {
    if (!p) return;
    std::vector<std::tuple<int, void*, size_t>> drop;
    {
      std::lock_guard<std::mutex> g(mu);
      free.emplace_back(dev_id, p, bytes);
      size_t cnt = 0, tot = 0;
      for (auto& f : free)
        if (std::get<0>(f) == dev_id) cnt++, tot += std::get<2>(f);
      const size_t cap = dev_id < 0 ? kPoolHostBytes : kPoolBytes;
      for (size_t i = 0; i < free.size() && (cnt > kPoolKeep || tot > cap);) {  // the oldest of this pool go
        if (std::get<0>(free[i]) != dev_id) {
          i++;
          continue;
        }
        cnt--, tot -= std::get<2>(free[i]);
        drop.push_back(free[i]);
        free.erase(free.begin() + (long)i);
      }
    }
    for (auto& d : drop) {
      if (std::get<0>(d) < 0) dev::host_release(std::get<1>(d));
      else dev::release(std::get<1>(d));
    }
  }
};
// The process-wide state, each defined once (engine.cpp): the buffer pool, a page-locked
// block from it (or a fresh one), and the snapshot epoch counter.
BufPool& buf_pool();
void* pinned_get(size_t bytes, size_t* got);
uint64_t next_snap_epoch();

// One device allocation carved into aligned sub-buffers. pool_dev >= 0: the
// allocation comes from (and returns to) the batch-buffer pool of that device.
// A sub-buffer filled from host data is registered with its source (the second add):
// upload() then copies what was registered, so the bytes reserved and the bytes copied
// come from one count and the destination's element type.
struct Arena {
  struct Req {
    void** p;
    size_t bytes;     // reserved
    const void* src;  // host source, or null for a work buffer
    size_t src_bytes;
  };
  std::vector<Req> req;
  void* base = nullptr;
  size_t total = 0;
  int pool_dev = -1;
  size_t got = 0;
  template <class T>
  void add(T** p, size_t count) {
    req.push_back({(void**)p, count * sizeof(T), nullptr, 0});
  }
  // *p[0, count) = src[0, count) at upload(); max(count, min_count) elements are reserved
  // (a list that may be empty keeps a valid pointer). src must stay alive until the
  // stream upload() ran on is synchronised.
  template <class T>
  void add(T** p, const std::type_identity_t<T>* src, size_t count, size_t min_count = 0) {
    req.push_back({(void**)p, std::max(count, min_count) * sizeof(T), src, count * sizeof(T)});
  }
  static size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  int alloc() {
    total = 0;
    for (auto& r : req) total += pad(r.bytes);
    if (total == 0) total = 256;
    if (pool_dev >= 0) base = buf_pool().get(pool_dev, total, &got);
    if (!base) {
      if (dev::alloc(&base, total)) return -1;
      got = total;
    }
    char* p = (char*)base;
    for (auto& r : req) {
      *r.p = p;
      p += pad(r.bytes);
    }
    return 0;
  }
  // The registered host sources copied to their sub-buffers on `st` (after alloc()).
  int upload(dev::stream_t st) {
    for (auto& r : req) {
      if (r.src && dev::h2d(*r.p, r.src, r.src_bytes, st)) return -1;
      r.src = nullptr;  // (copied once: the source need not outlive the caller's sync)
    }
    return 0;
  }
  // One block of `bytes` with no sub-buffers (a replica's copy of another arena).
  int alloc_raw(size_t bytes) {
    req.clear();
    total = bytes ? bytes : 256;
    got = total;
    return dev::alloc(&base, total);
  }
  void drop() {
    if (!base) return;
    if (pool_dev >= 0) buf_pool().put(pool_dev, base, got);
    else dev::release(base);
    base = nullptr;
  }
  void reset() {
    drop();
    req.clear();
    total = 0;
  }
  ~Arena() { drop(); }
};

#define HIPCHK(x)                                                            \
  do {                                                                       \
    if ((x) != 0) {                                                          \
      e->err = std::string(#x) + ": " + dev::last_error();                   \
      return KP_EDEVICE;                                                     \
    }                                                                        \
  } while (0)

// std::allocator that leaves trivial elements uninitialized on resize: the packer
// writes every BindHdr itself (in parallel, so the pages are first touched there),
// and a value-initializing resize would zero 160 B per binding on one thread.
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = NoInitAlloc<U>;
  };
  NoInitAlloc() = default;
  template <class U>
  NoInitAlloc(const NoInitAlloc<U>&) {}
  template <class U>
  void construct(U* p) noexcept {
    ::new ((void*)p) U;
  }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    ::new ((void*)p) U(std::forward<A>(a)...);
  }
};

// The helpers that cross a unit boundary, each defined in one unit: a resource list as
// quantities (snapshot.cpp defines it; engine.cpp and nodes.cpp call it too), the
// labels.NewRequirement validation (pack.cpp; nodes.cpp), and from engine.cpp the MaxDivided
// table entries per workgroup (snapshot.cpp), the batch's LDS check and a component list
// resolved against the snapshot (pack.cpp).
typedef std::map<std::string, k8s::Qty> QtyMap;
bool qmap(const kp_resource* r, uint32_t n, QtyMap* m);
bool valid_req(std::string_view key, std::string_view op, const kp_str* v, uint32_t n);
int md_cap_of(const kp_snapshot* s);
int batch_lds_check(kp_engine* e, const kp_snapshot* s, const kp_batch* bt);
int build_sets_args(const kp_snapshot* s, const kp_component* comps, uint32_t K, SetsArgs* A, std::string* err);

// The one intake (answers.cpp) of kp_estimates and kp_filter_answers for kp_batch_create_estimates
// / _filters and kp_schedule_affinities_ex. The checks: `who` is the entry point's name, `pre`
// how it names the input's fields ("", or "est->" / "flt->" in the affinity call), n the call's
// bindings; an input that is null or without rows passes. check_estimates is every estimate
// check. check_filters ends with the n_rows bound; the verdicts' row_of range is check_row_of
// over [first, first + count): n entries, or one binding's between the term_off checks.
int check_estimates(kp_engine* e, const kp_snapshot* s, const char* who, const char* pre, const kp_estimates* est,
                    uint64_t n);
int check_filters(kp_engine* e, const kp_snapshot* s, const char* who, const char* pre, const kp_filter_answers* flt,
                  uint64_t n);
int check_row_of(kp_engine* e, const char* who, const char* pre, const int32_t* row_of, uint64_t first, uint64_t count,
                 uint32_t n_rows);
// Checked rows on the device in rank order: d_est [n_est][Cp], -1 in [C, Cp); d_flt [n_flt][W],
// zero bits at and above C. The batches made over them share it (kp_batch::rows); its block
// goes back to the engine device's buffer pool with the last holder.
struct AnswerRows {
  Arena dev;
  int32_t* d_est = nullptr;
  uint64_t* d_flt = nullptr;
  uint32_t n_est = 0, n_flt = 0;
};
// *out from checked est / flt (null: none), queued on `st`: the caller's arrays go up in caller
// order into `staging`, k_est_rows_rank / k_flt_rows_rank rank them. Nothing waits here: the
// caller synchronises `st` before it lets go of its arrays, of `staging` or, after an error, of
// *out. tev: three events recorded around the two kernels (KP_PACK_TIMING), or null.
int make_answer_rows(kp_engine* e, const kp_snapshot* s, const kp_estimates* est, const kp_filter_answers* flt,
                     dev::stream_t st, Arena* staging, const dev::event_t* tev, std::shared_ptr<const AnswerRows>* out);
// A batch's part of the answers. A kp_batch_create* call gives est / flt unchecked: creation
// checks them before it packs, fills the rest, and makes the rows once a class or a binding
// is known to have one. kp_schedule_affinities_ex gives its `rows` (or null), the bindings'
// estimate rows (null: none), the (binding, verdict row) pairs in binding order and the number
// of registered plugins the verdicts fold in.
struct BatchAnswers {
  const kp_estimates* est = nullptr;
  const kp_filter_answers* flt = nullptr;
  std::shared_ptr<const AnswerRows> rows;
  const int32_t* est_row_of = nullptr;
  std::vector<FltPair> flt_list;
  uint32_t flt_plugins = 0;
};

}  // namespace kp::host
using namespace kp::host;

// ============================================================================
// Engine / snapshot / batch objects
// ============================================================================
// The engine's events (kp_engine::ev), one per event a schedule call records; BEGIN / END
// pairs time a stage for kp_last_stage_times, the others order the three streams.
enum : int {
  EV_FILLS = 0,       // stream: the counters are cleared (every kernel waits for it)
  EV_SELECT_BEGIN,    // stream: the rows are complete ...
  EV_SELECT_END,      // ... to the end of the last select kernel and k_slow
  EV_ROWS_BEGIN,      // stream2: the estimator rows and the filter ...
  EV_ROWS_END,        // ... complete (stream and stream3 wait for it)
  EV_CLASS_ROWS,      // stream2: every class row is written (k_class_order's input)
  EV_CLASS_ORDER,     // stream3: k_class_order done (stream2 waits for it)
  EV_SEL_ALL_BEGIN,   // stream2: the SEL_ALL kernels ...
  EV_SEL_ALL_END,     // ... (k_slow and the results wait for it)
  EV_SLOW_END,        // stream3: k_slow done (the results wait for it)
  EV_TOP_LARGE,       // stream3: k_select_top's large slice done (its fallbacks follow on stream2)
  EV_TOP_BEGIN,       // stream2: k_select_top's launches ...
  EV_TOP_END,
  EV_CLUSTER_BEGIN,   // stream3: the cluster-spread kernels ...
  EV_CLUSTER_END,
  kEngineEvents
};

struct kp_engine {
  int device = 0;
  dev::stream_t stream = nullptr;   // select kernels, copies (the batch's result order)
  dev::stream_t stream2 = nullptr;  // pair kernel, then the SEL_ALL select kernel
  dev::stream_t stream3 = nullptr;  // the cluster-spread select kernel, beside the other selects
  dev::event_t ev[kEngineEvents] = {};
  std::string err;
  kp_stage_times times{};
  struct {  // kp_schedule_affinities results
    std::vector<int32_t> status, err, idx, attempts;
    std::vector<int64_t> arg;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> cidx;
    std::vector<int32_t> rep;
  } aff;
  struct {  // kp_fit_diagnosis_batch results
    std::vector<uint64_t> binding, offsets;
    std::vector<uint32_t> reason, taint_ref, count, n_fit, n_del;
  } diag;
  int n_threads = 8;
  size_t max_lds = 65536;
  // k_select_top (kp_top.h): on, and its subset capacity per binding (LDS entries);
  // KP_TOP=0 / KP_TOP_CAP=<n> at engine creation (tests, tuning)
  bool top_on = true;
  int top_cap = 832;       // subset capacity of the large slice (LDS: 8 workgroups of two waves per CU)
  int top_cap_small = 256;  // ... and of the small one (bindings needing <= kTopSmallNeed)
  // the large-slice bindings run at this capacity first (more waves per CU); those whose
  // subset outgrows it run again at top_cap (0 / >= top_cap: one launch at top_cap)
  int top_cap_mid = 0;
  bool top_split = true;    // the two slices' launches on two streams (KP_TOP_SPLIT=0: one)
  bool slow_order = true;   // k_slow orders candidates from the class orders (KP_SLOW_ORDER=0: sorts)
  // per-kernel timing of kp_schedule_batch (kp_engine_set_profile): an event pair
  // around every launch on its own stream, folded by kernel name after the batch
  struct KProf {
    const char* name;
    uint64_t units;  // bindings (or rows) the launch covered
    int units_stat;  // >= 0: the count is device-side, h_stats[units_stat] (KS_*)
  };
  bool prof = false;
  uint64_t submit_seq = 0;  // schedule calls submitted on this engine (stage timing validity)
  std::vector<dev::event_t> pev;
  std::vector<KProf> pk;
  std::vector<kp_kernel_time> ktimes;
  // kp_affected_bindings' result: one page-locked block from the host pool, the list's
  // length (8 bytes) and then the list, kept until the next call needs a larger one
  struct {
    uint64_t* h = nullptr;
    size_t bytes = 0;
  } affected;
};

// Per-kernel profiling (engine.cpp): prof_begin records the start event of a launch on its
// stream (-1: profiling off), prof_end its end event, name and units; prof_fold, after the
// call's final sync, folds the launches by name into kp_engine::ktimes (h_stats: the batch's
// counters for launches whose units are device-side, or null when none is). A call clears
// kp_engine::pk before its first launch.
int prof_begin(kp_engine* e, dev::stream_t st);
void prof_end(kp_engine* e, int i, dev::stream_t st, const char* name, uint64_t units, int units_stat = -1);
void prof_fold(kp_engine* e, const uint32_t* h_stats);
#define KPROF(ST, NAME, UNITS, STAT, CALL)               \
  do {                                                   \
    const int pi_ = prof_begin(e, ST);                   \
    HIPCHK(CALL);                                        \
    prof_end(e, pi_, ST, NAME, (uint64_t)(UNITS), STAT); \
  } while (0)

struct kp_snapshot {
  kp_engine* e = nullptr;
  uint64_t epoch = next_snap_epoch();
  uint64_t updates = 0;  // kp_snapshot_update calls applied (a kp_assumptions holds the state it deducted from)
  kp_options opts{};
  int C = 0, Cp = 0, W = 0;
  Dict str, keys, gvk, res, regions;
  SvMap<int32_t> rank_of;  // cluster name -> rank
  std::vector<uint32_t> perm;                        // rank -> caller index
  std::vector<int32_t> inv;                          // caller index -> rank
  int32_t rid_cpu = -1, rid_mem = -1, rid_eph = -1;
  int n_tmpl = 0, kmax = 0;
  int est_kind = 0;  // EST_* pair-kernel instance the clusters allow (snapshot_est_kind)
  std::vector<std::string> names;  // cluster names in rank order
  std::vector<unsigned char> blob;  // kp_snapshot_export buffer
  // host copies
  std::vector<uint32_t> flags;
  std::vector<int32_t> provider, region, region_idx, zone_off, zone_ids, label_val, taint_off, taint_key, taint_val,
      taint_eff, mgrp_off, mgrp_tid, mg_tid, mg_cnt;
  std::vector<int64_t> provider_int, region_int, allowed, avail, mgrp_cnt, tmpl;
  std::vector<int64_t> qa;  // [R][Cp] quantityAsInt64 availability, kQaAbsent where not allocatable
  std::vector<uint64_t> api_bits;
  Arena dev;
  SnapView view{};
};

// The assumed workloads deducted once per cluster (assumed.cpp; kp_assume.h): the device
// arrays of `view`, the snapshot state they were deducted from, and the clusters' caller
// indices for the error texts. A batch made over it shares it (kp_batch::assumed).
struct AssumedState {
  Arena dev;
  AssumedView view{};
  const kp_snapshot* snap = nullptr;
  uint64_t epoch = 0, updates = 0;
};
struct kp_assumptions {
  kp_engine* e = nullptr;
  std::shared_ptr<const AssumedState> st;  // null: no entries (the gate is off)
};

// diagnostic builds: phase stamps and counters, kDbgSlots x kDbgSpread (kp_select.h)
// The state schedule_submit leaves for schedule_finish (one submitted call per batch).
struct SchedPend {
  bool live = false, empty = false, bits = false, top = false, spread_orders = false;
  bool packed = false;  // the call returns kp_results_packed (kp_schedule_batch_submit_packed)
  bool delta = false;   // the call returns kp_results_delta (kp_schedule_batch_submit_delta)
  int fast = 0;
  double t0 = 0, th0 = 0, th1 = 0;
  uint64_t seq = 0;
  dev::event_t ev = nullptr;  // recorded after the call's last read-back (kept across calls)
};

struct kp_batch {
  kp_snapshot* snap = nullptr;
  int B = 0;
  std::vector<BindHdr, NoInitAlloc<BindHdr>> hdr;
  std::vector<int32_t> ipool;
  std::vector<int64_t> lpool;
  std::vector<Tol> tols;
  std::vector<Prog> progs;
  std::vector<Instr> instrs;
  std::vector<int32_t> l_all, l_cluster, l_region, l_slow, l_cs;  // l_cs: cluster + region bindings
  int n_all_dyn = 0;  // l_all = [other strategies | StaticWeight]: the first n_all_dyn are not StaticWeight
  int n_top_small = 0;  // of those, the first n_top_small take k_select_top's small slice
  int n_static = 0;   // of the StaticWeight ones, the first n_static take k_select_static (static_ok)
  uint64_t out_cap = 0;
  std::vector<uint8_t> route;     // RT_* per binding (pack_parallel)
  int max_tgt = 0, max_tiers = 1;  // over the batch's headers (pack_parallel)
  Arena dev;
  BatchView view{};
  // device work buffers
  uint64_t* fmask = nullptr;
  int32_t* est = nullptr;  // [B][Cp] per-binding rows (allocated on first use: rows mode, diagnosis entries)
  // estimator classes (kp_filter.h): class of each binding (0 = non-workload) and
  // a representative binding per class; their raw GeneralEstimator rows [n][Cp]
  std::vector<int32_t> bcls, crep;
  int32_t *d_bcls = nullptr, *d_crep = nullptr, *cls_rows = nullptr;
  int32_t* d_all_cls = nullptr;  // the estimator class of each l_all entry (KArgs::lcls)
  std::vector<int32_t> l_all_cls;
  // Estimator classes serving one binding, in a batch without class orders (est_single):
  // their rows hold only that binding's feasible clusters, written after k_filter
  // (k_est_class over l_cls_single with the feasibility rows); l_cls_full: the others.
  bool est_single = false;
  std::vector<int32_t> l_cls_full, l_cls_single;
  int32_t *d_cls_full = nullptr, *d_cls_single = nullptr;
  // The other estimators' answers (kp_batch_create_estimates; all empty / null for a batch
  // without them, which allocates, uploads and launches nothing for it): cls_est[class] =
  // the class's row of d_est_rows ([n_rows][Cp], by cluster rank, -1 in the padding), -1
  // for none; l_est_cls: the classes that have one (k_est_extra's list in bits mode).
  std::vector<int32_t> cls_est, l_est_cls;
  int32_t *d_cls_est = nullptr, *d_est_cls = nullptr, *d_est_rows = nullptr;
  // The out-of-tree filter plugins' verdicts (kp_batch_create_filters; empty / null for a
  // batch without rows, which allocates, uploads and launches nothing for them): l_flt =
  // the bindings that have a row, (binding, row id) in binding order (k_filter_extra's
  // list); d_flt_rows[n_rows][W] words by cluster rank, zero bits in the padding, fixed
  // for the batch's lifetime. flt_plugins: how many registered plugins the answers fold
  // in (the schedule calls' gate against kp_options.n_out_of_tree_plugins).
  std::vector<FltPair> l_flt;
  FltPair* d_flt_list = nullptr;
  uint64_t* d_flt_rows = nullptr;
  uint32_t flt_plugins = 0;
  // d_est_rows / d_flt_rows point into `rows` (answers.cpp), which this batch shares with
  // whoever else was created over the same answers (kp_schedule_affinities_ex: one batch a
  // round) and which goes back to the pool with the last of them; null for a batch without.
  std::shared_ptr<const AnswerRows> rows;
  // The assumed workloads' deducted state (kp_batch_create_assumed; null for every other
  // batch, which launches nothing for it): k_est_assumed rewrites the estimate rows at its
  // clusters in every schedule call.
  std::shared_ptr<const AssumedState> assumed;
  // component-set classes (BF_SETS): class id and resolved component list of each;
  // their rows are MaxAvailableComponentSets per cluster (k_sets_rows), and in the
  // pair-row mode the BF_SETS bindings' rows are rebuilt from them (k_rows_from_class)
  // k_select_top: per-class candidate orders, row sums and walkability; its fallback list
  uint64_t* d_ord = nullptr;
  int64_t* d_ctot = nullptr;
  int32_t *d_cok = nullptr, *d_fb = nullptr, *d_ofb = nullptr;
  int32_t *d_fbc = nullptr, *d_fbr = nullptr;  // k_spread_order's fallback lists (cluster / region positions)
  int32_t* d_fba = nullptr;                     // k_region_a_order's fallback list
  std::vector<int32_t> sets_cls, l_sets;
  std::vector<SetsArgs> sets_args;
  SetsArgs* d_sets_args = nullptr;
  int64_t *d_sets_off = nullptr, *d_sets_scratch = nullptr;
  uint32_t* d_sets_ovf = nullptr;  // [sets_cls] per component-set class: overflowing rank + 1, or 0
  int32_t* d_sets_list = nullptr;
  std::string err;  // packing error text
  int32_t *d_all = nullptr, *d_cluster = nullptr, *d_region = nullptr, *d_slowlist = nullptr, *d_cs = nullptr;
  int32_t *status = nullptr, *errc = nullptr, *slow = nullptr;
  int64_t* arg = nullptr;
  uint64_t* start = nullptr;
  uint32_t* count = nullptr;
  unsigned long long* counter = nullptr;
  uint32_t* stats = nullptr;
  unsigned long long* dbg = nullptr;
  // launch arguments of the kernels that read them through a pointer (kp_launch.h
  // SelectExtra::dargs): kArgSlots device slots and their page-locked host staging
  KArgs* d_kargs = nullptr;
  KArgs* h_kargs = nullptr;
  size_t h_kargs_bytes = 0;
  uint32_t h_stats[kStatSlots] = {};  // the counters after a schedule call (KS_*, kp_launch.h)
  uint32_t* out_idx = nullptr;
  int32_t* out_rep = nullptr;
  uint64_t* offsets_d = nullptr;
  uint64_t* off_part = nullptr;  // per-chunk totals of the offsets scan
  uint32_t* cidx_d = nullptr;
  int32_t* crep_d = nullptr;
  RegionOut* rout = nullptr;
  int32_t *rstat = nullptr, *rsel = nullptr, *rnsel = nullptr;
  uint32_t* nhost = nullptr;  // region bindings the device group search left to the host
  unsigned char* slow_scratch = nullptr;
  size_t slow_slot = 0;
  int slow_grid = 0, slow_cap = 0, slow_lds = 0, slow_sort = 0;
  // k_region_wide: the rows of l_region whose selection can outgrow k_region_b's lists
  // (cluster MaxGroups > kSmallMax, or a repeated spec.Clusters past kTgtSmallMax), its
  // own scratch slots (k_slow may run beside it) and LDS sort area; all empty / 0 for a
  // batch without such bindings, which then launches and allocates nothing for it
  std::vector<int32_t> l_region_wide;
  int32_t* d_region_wide = nullptr;
  unsigned char* wide_scratch = nullptr;
  size_t wide_slot = 0;
  int wide_grid = 0, wide_sort = 0;
  bool fast_ok = false;  // the batch half of the fast pair-kernel condition (batch_fast_ok)
  int n_regions = 0;     // the snapshot's region count the region buffers were sized for
  // host results
  std::vector<int32_t> h_status, h_err, h_rstat, h_rsel, h_rnsel;
  std::vector<int64_t> h_arg;
  std::vector<uint64_t> h_start, h_offsets;
  std::vector<uint32_t> h_count;
  // result CSR in page-locked host memory (h_res_cap entries each)
  uint32_t* h_cidx = nullptr;
  int32_t* h_crep = nullptr;
  uint64_t h_res_cap = 0;
  SchedPend pend;         // a submitted call (schedule_submit) awaiting schedule_finish
  bool sched_done = false;  // h_status holds a completed schedule call's statuses (kp_fit_diagnosis_batch)
  size_t h_cidx_bytes = 0, h_crep_bytes = 0;  // their pooled block sizes
  // The packed result form (kp_results_packed), allocated on the batch's first packed call
  // (ensure_packed): per-binding escape counts [B] and their scan [B + 1] on the device,
  // the scan's page-locked host copy. The packed words take cidx_d / h_cidx and the
  // escaped replicas crep_d / h_crep, which a packed call does not otherwise use.
  uint32_t* wcount_d = nullptr;
  uint64_t* woff_d = nullptr;
  uint64_t* h_woff = nullptr;
  size_t h_woff_bytes = 0;
  // The delta result form (kp_results_delta), allocated on the batch's first delta call
  // (ensure_delta), one device allocation behind dflag_d: per-binding flags and masked
  // counts [B], their scans [B + 1] each, the changed list [B], its CSR offsets [B + 1] and
  // the batch's long-list bindings (kp::changed_long, n_dlong of them). h_delta, page-locked:
  // [n_changed, n_targets, n_targets_all, pad | offsets [B + 1] | changed [B]], of which a
  // call copies the totals, n_changed + 1 offsets and n_changed indices. The delta CSR takes
  // cidx_d / crep_d and h_cidx / h_crep, as the wide one does.
  uint32_t *dflag_d = nullptr, *dcount_d = nullptr, *dchanged_d = nullptr;
  uint64_t *dchg_off_d = nullptr, *dmoff_d = nullptr, *dout_off_d = nullptr;
  int32_t* dlong_d = nullptr;
  int n_dlong = 0;
  uint64_t* h_delta = nullptr;
  size_t h_delta_bytes = 0;
  // The batch's device arena and page-locked buffers go back to the process-wide
  // pools on destruction, where another batch (of any engine) may take them at
  // once. An entry point that fails part-way leaves kernels queued that still
  // use them: it records these events on the engine's streams (batch_fence), and
  // destruction waits for them. kp_batch_create does the same through
  // create_stream while it runs.
  dev::event_t fence[3] = {};
  bool fenced = false;
  dev::stream_t create_stream = nullptr;
  void quiesce() {
    if (create_stream) (void)dev::sync(create_stream);
    create_stream = nullptr;
    for (auto& ev : fence)
      if (ev) {
        if (fenced) (void)dev::event_sync(ev);
        dev::event_destroy(ev);
        ev = nullptr;
      }
    fenced = false;
    if (pend.ev) {  // a submitted call never collected: its work uses the buffers
      if (pend.live) (void)dev::event_sync(pend.ev);
      dev::event_destroy(pend.ev);
      pend.ev = nullptr;
    }
    pend.live = false;
  }
  ~kp_batch() {
    quiesce();
    buf_pool().put(-1, h_cidx, h_cidx_bytes);
    buf_pool().put(-1, h_crep, h_crep_bytes);
    buf_pool().put(-1, h_kargs, h_kargs_bytes);
    buf_pool().put(-1, h_woff, h_woff_bytes);
    buf_pool().put(-1, h_delta, h_delta_bytes);
    if (est) dev::release(est);
    if (dflag_d) dev::release(dflag_d);  // (one allocation)
    if (wcount_d) dev::release(wcount_d);  // (one allocation: woff_d lies behind the counts)
  }
  std::vector<RegionOut> h_rout;
};

// The one creation function behind the four kp_batch_create* entry points and every round
// of kp_schedule_affinities_ex (pack.cpp); keys and cache may be null.
int batch_create_with(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings, uint64_t n,
                      const kp_binding_key* keys, kp_pack_cache* cache, BatchAnswers* ans, kp_batch** out);
