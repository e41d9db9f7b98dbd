// watch.cpp — kp_watch_* and kp_affected_bindings: which bindings a cluster event affects
// (enqueueAffectedBindings / enqueueAffectedCRBs, pkg/scheduler/event_handler.go:388-491),
// answered on the device. A watch holds, per binding, the compiled program of the one affinity
// the reference evaluates (kp_selc.h: the packer's selector compiler); a call turns the changed
// clusters into rank space once, marks the listed bindings (k_affected, or k_affected_rows
// without the snapshot's bitset rows), scans the marks (k_offsets_a / _b) and writes the
// ascending list (k_affected_write).
#include "kp_host.h"
#include "kp_selc.h"

struct kp_watch {
  kp_engine* e = nullptr;
  const kp_snapshot* snap = nullptr;
  uint64_t epoch = 0;  // the snapshot's dictionaries the programs resolved against
  int B = 0;
  Arena dev;
  BatchView view{};  // B and the program pools (progs / instrs / ipool); no headers
  int32_t* wprog = nullptr;    // [B] program id, kWatchAlways or kWatchNever
  int32_t* status0 = nullptr;  // [B] zeros (KP_STATUS_OK: k_offsets_a counts every binding)
  uint32_t* cnt = nullptr;     // [B] 1 = listed
  uint64_t* off = nullptr;     // [B + 1]
  uint64_t* part = nullptr;
  uint32_t* out = nullptr;     // [B] the list
  // a call's changed clusters: the distinct words (bits mode) or ranks (row mode), and the
  // words' masks
  int32_t* idx = nullptr;    // [max(C, 1)]
  uint64_t* mask = nullptr;  // [max(W, 1)]
};

namespace {

// getAffinityIndex (pkg/scheduler/helper.go:99-110)
uint32_t affinity_index(const kp_binding& b) {
  const std::string_view obs = SV(b.observed_affinity_name);
  if (obs.empty()) return 0;
  for (uint32_t i = 0; i < b.n_cluster_affinities; i++)
    if (SV(b.cluster_affinities[i].affinity_name) == obs) return i;
  return 0;
}

int watch_create(kp_engine* e, const kp_snapshot* sc, const kp_binding* bindings, uint64_t n, const uint8_t* mode,
                 kp_watch* w) {
  kp_snapshot* s = const_cast<kp_snapshot*>(sc);
  const int B = (int)n;
  w->e = e;
  w->snap = sc;
  w->epoch = sc->epoch;
  w->B = B;
  Pools pools;
  SelectorCompiler comp{s, &pools};
  SvMap<int32_t> ids;  // affinity content -> its program: bindings of one policy share it
  std::vector<int32_t> wprog((size_t)B);
  for (int i = 0; i < B; i++) {
    const kp_binding& b = bindings[i];
    const uint8_t m = mode ? mode[i] : (uint8_t)KP_WATCH_MATCH;
    if (m > KP_WATCH_SKIP) {
      e->err = "kp_watch_create: mode[" + std::to_string(i) + "] is not a KP_WATCH_* value";
      return KP_EINVAL;
    }
    if (m != KP_WATCH_MATCH) {
      wprog[i] = m == KP_WATCH_ALWAYS ? kWatchAlways : kWatchNever;
      continue;
    }
    // event_handler.go:417-431: ClusterAffinities first, then ClusterAffinity, else nil
    const kp_cluster_affinity* a = nullptr;
    if (b.n_cluster_affinities > 0) {
      if (!b.cluster_affinities) {
        e->err = "kp_watch_create: binding " + std::to_string(i) + " has n_cluster_affinities > 0 and no terms";
        return KP_EINVAL;
      }
      a = &b.cluster_affinities[affinity_index(b)].affinity;
    } else if (b.has_cluster_affinity) {
      a = &b.cluster_affinity;
    }
    if (!a) {
      wprog[i] = kWatchAlways;  // event_handler.go:434-436
      continue;
    }
    comp.affinity_key(*a);
    if (auto* hit = ids.find(std::string_view(comp.ckey))) {
      wprog[i] = hit->second;
      continue;
    }
    const std::string key = comp.ckey;  // (compile builds the key again)
    wprog[i] = comp.compile(*a);
    ids.emplace(key, wprog[i]);
  }
  w->dev.pool_dev = e->device;
  Arena& a = w->dev;
  BatchView& v = w->view;
  v = BatchView{};
  v.B = B;
  a.add(&v.progs, pools.progs.data(), pools.progs.size(), 1);
  a.add(&v.instrs, pools.instrs.data(), pools.instrs.size(), 1);
  a.add(&v.ipool, pools.ipool.data(), pools.ipool.size(), 1);
  a.add(&w->wprog, wprog.data(), wprog.size(), 1);
  a.add(&w->status0, (size_t)std::max(1, B));
  a.add(&w->cnt, (size_t)std::max(1, B));
  a.add(&w->off, (size_t)B + 1);
  a.add(&w->part, (size_t)std::max(1, (B + kOffChunk - 1) / kOffChunk));
  a.add(&w->out, (size_t)std::max(1, B));
  a.add(&w->idx, (size_t)std::max(1, sc->C));
  a.add(&w->mask, (size_t)std::max(1, sc->W));
  if (a.alloc()) {
    e->err = std::string("kp_watch_create: ") + dev::last_error();
    return KP_ENOMEM;
  }
  // (the host pools are locals: the stream is synchronised before they go)
  const int rc = a.upload(e->stream) || dev::fill(w->status0, 0, 4 * (size_t)std::max(1, B), e->stream);
  if (dev::sync(e->stream) || rc) {
    e->err = std::string("kp_watch_create: ") + dev::last_error();
    return KP_EDEVICE;
  }
  return KP_OK;
}

// The launches and read-backs of one call; on an error the caller synchronises the stream.
int affected_run(kp_engine* e, const kp_watch* w, const kp_snapshot* s, const uint32_t* cluster_idx, uint64_t n,
                 uint64_t* total) {
  const int B = w->B, W = s->W;
  dev::stream_t st = e->stream;
  const bool bits = s->view.n_bits > 0 && !kp_env_flag("KP_PAIR_ROWS");
  // the caller's indices in rank space, once: repeats fold here
  std::vector<uint64_t> mask((size_t)W, 0);
  for (uint64_t i = 0; i < n; i++) {
    const int32_t r = s->inv[cluster_idx[i]];
    mask[(size_t)(r >> 6)] |= 1ull << (r & 63);
  }
  std::vector<int32_t> idx;
  std::vector<uint64_t> cwm;
  for (int k = 0; k < W; k++) {
    if (!mask[k]) continue;
    if (bits) {
      idx.push_back(k);
      cwm.push_back(mask[k]);  // (bits of real clusters only: every rank is below C)
    } else {
      for (uint64_t m = mask[k]; m; m &= m - 1) idx.push_back(64 * k + __builtin_ctzll(m));
    }
  }
  e->pk.clear();
  HIPCHK(dev::h2d(w->idx, idx.data(), 4 * idx.size(), st));
  if (bits) {
    HIPCHK(dev::h2d(w->mask, cwm.data(), 8 * cwm.size(), st));
    KPROF(st, "k_affected", B, -1,
          dev::affected(st, s->view, w->view, w->wprog, w->idx, w->mask, (int)idx.size(), w->cnt));
  } else {
    KPROF(st, "k_affected_rows", B, -1,
          dev::affected_rows(st, s->view, w->view, w->wprog, w->idx, (int)idx.size(), w->cnt));
  }
  KPROF(st, "k_offsets", B, -1, dev::offsets(st, w->status0, w->cnt, B, w->off, w->part));
  KPROF(st, "k_affected_write", B, -1, dev::affected_write(st, B, w->cnt, w->off, w->out));
  // the total first, then the list's 4 * total bytes
  HIPCHK(dev::d2h(e->affected.h, w->off + B, 8, st));
  HIPCHK(dev::sync(st));
  *total = e->affected.h[0];
  if (*total > (uint64_t)B) {
    e->err = "kp_affected_bindings: the device list is longer than the watch";
    return KP_EDEVICE;
  }
  HIPCHK(dev::d2h(e->affected.h + 1, w->out, 4 * (size_t)*total, st));
  HIPCHK(dev::sync(st));
  if (e->prof) prof_fold(e, nullptr);
  return KP_OK;
}

}  // namespace

extern "C" {

int kp_watch_create(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings, uint64_t n, const uint8_t* mode,
                    kp_watch** out) {
  if (!e || !s || !out || (n && !bindings)) return KP_EINVAL;
  if (n >= (1ull << 31)) {
    e->err = "kp_watch_create: n_bindings must be below 2^31";
    return KP_EINVAL;
  }
  (void)dev::set_device(e->device);
  auto* w = new (std::nothrow) kp_watch();
  if (!w) return KP_ENOMEM;
  const int rc = watch_create(e, s, bindings, n, mode, w);
  if (rc) {
    delete w;
    return rc;
  }
  *out = w;
  return KP_OK;
}

void kp_watch_destroy(kp_watch* w) { delete w; }

int kp_affected_bindings(kp_engine* e, const kp_watch* w, const kp_snapshot* s, const uint32_t* cluster_idx,
                         uint64_t n_clusters, kp_affected* out) {
  if (!e || !w || !s || !out || (n_clusters && !cluster_idx)) {
    if (e) e->err = "kp_affected_bindings: null argument";
    return KP_EINVAL;
  }
  if (w->e != e) {
    e->err = "kp_affected_bindings: the watch belongs to another engine";
    return KP_EINVAL;
  }
  if (w->snap != s) {
    e->err = "kp_affected_bindings: the watch was made over another snapshot (make a new watch)";
    return KP_ESTATE;
  }
  if (w->epoch != s->epoch) {
    e->err = "kp_affected_bindings: the snapshot's dictionaries grew since the watch was made "
             "(kp_snapshot_update reported dict_grew = 1: make a new watch)";
    return KP_ESTATE;
  }
  for (uint64_t i = 0; i < n_clusters; i++)
    if (cluster_idx[i] >= (uint64_t)s->C) {
      e->err = "kp_affected_bindings: cluster_idx[" + std::to_string(i) + "] = " + std::to_string(cluster_idx[i]) +
               " is not below the snapshot's " + std::to_string(s->C) + " clusters";
      return KP_EINVAL;
    }
  static const uint32_t none[1] = {0};
  out->n = 0;
  out->bindings = none;
  if (n_clusters == 0 || w->B == 0) return KP_OK;  // (nothing launched)
  (void)dev::set_device(e->device);
  const size_t need = 8 + 4 * (size_t)w->B;
  if (e->affected.bytes < need) {
    buf_pool().put(-1, e->affected.h, e->affected.bytes);
    e->affected.bytes = 0;
    e->affected.h = (uint64_t*)pinned_get(need, &e->affected.bytes);
    if (!e->affected.h) {
      e->err = "kp_affected_bindings: page-locked result list";
      return KP_ENOMEM;
    }
  }
  uint64_t total = 0;
  const int rc = affected_run(e, w, s, cluster_idx, n_clusters, &total);
  if (rc) {
    (void)dev::sync(e->stream);  // (the watch may be destroyed next: nothing may still use its buffers)
    return rc;
  }
  out->n = total;
  out->bindings = (const uint32_t*)(e->affected.h + 1);
  return KP_OK;
}

}  // extern "C"
