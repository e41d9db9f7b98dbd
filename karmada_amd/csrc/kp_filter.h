// kp_filter.h — the filter stage as bitset algebra over cluster postings, and the
// GeneralEstimator evaluated once per estimator class.
//
// RunFilterPlugins (runtime/framework.go:93-122) is an AND of per-cluster
// predicates, and every predicate a binding can state is a union / intersection /
// complement of a few snapshot-wide cluster sets: the clusters carrying label k=v,
// provider p, region r or zone z, enabling GVK g, holding taint list t, not being
// deleted. upload_snapshot (snapshot.cpp) stores each of those sets once as a
// W-word bitset row (SnapView::bits); a binding's feasibility word w is then the
// same boolean expression over word w of the rows its selector names. One wave64
// per binding, one lane per word: a binding costs O(rows named x W / 64) word
// operations instead of C per-cluster evaluations, and the row it writes
// (fmask[b][W]) is the u64 feasibility layout the select kernels already read.
//
// The estimate (calAvailableReplicas' GeneralEstimator answer, general.go:57-108)
// depends on a binding only through its ReplicaRequirements (resource requests,
// in both the summary and the resource-model paths), so bindings with equal
// requests share one raw row per cluster; k_est_class computes each distinct
// class's row once, and the select kernels merge it with the binding's
// spec.Replicas as cal_merge_bf does (kp_select.h est_at).
#pragma once
#include "kp_algo.h"

namespace kp {

// Row of a hashed key (label, provider, region, zone value), -1 if no cluster has it.
// Uniform: every lane probes the same key.
KP_HD inline int32_t bits_find(const SnapView& s, uint64_t key) {
  uint32_t i = bits_hash(key) & s.bmask;
  for (;;) {
    const uint64_t k = kp_ldu(s.bkey + i);
    if (k == key) return kp_ldu(s.bval + i);
    if (k == kBitsEmpty) return -1;
    i = (i + 1) & s.bmask;
  }
}
KP_HD inline uint64_t bits_word(const SnapView& s, int row, int w) { return s.bits[(size_t)row * s.W + w]; }

// OR of the rows of the listed values (keys bits_key(kind, slot, value)).
KP_HD inline uint64_t bits_any(const SnapView& s, const int32_t* lst, int n, uint64_t kind, uint32_t slot, int w) {
  uint64_t m = 0;
  for (int k = 0; k < n; k++) {
    const int32_t row = bits_find(s, bits_key(kind, slot, kp_ldu(lst + k)));
    if (row >= 0) m |= bits_word(s, row, w);
  }
  return m;
}
// Bits of word w set for the listed cluster ranks.
KP_HD inline uint64_t rank_word(const int32_t* lst, int n, int w, int stride = 1) {
  uint64_t m = 0;
  for (int k = 0; k < n; k++) {
    const int32_t r = kp_ldu(lst + stride * k);
    if ((r >> 6) == w) m |= 1ull << (r & 63);
  }
  return m;
}

// Word w of one selector instruction (prog_eval_u's semantics, kp_algo.h; bits
// past C are cleared by BR_BASE).
KP_HD inline uint64_t instr_word(const SnapView& s, const BatchView& bv, const Instr& in, int w) {
  switch (in.op) {
    case OP_TRUE:
      return ~0ull;
    case OP_EXCLUDE:
      return ~rank_word(bv.ipool + in.a, in.b, w);
    case OP_NAMES:
      return rank_word(bv.ipool + in.a, in.b, w);
    case OP_LBL_IN:
      return bits_any(s, bv.ipool + in.b, in.c, BK_LABEL, (uint32_t)in.a, w);
    case OP_LBL_NOTIN:  // absent label, or a value outside the list
      return ~bits_any(s, bv.ipool + in.b, in.c, BK_LABEL, (uint32_t)in.a, w);
    case OP_LBL_EXISTS:
      return bits_word(s, s.br_lex + in.a, w);
    case OP_LBL_DNE:
      return ~bits_word(s, s.br_lex + in.a, w);
    case OP_FLD_IN:
      return bits_any(s, bv.ipool + in.b, in.c, in.a == 0 ? BK_PROVIDER : BK_REGION, 0, w);
    case OP_FLD_NOTIN:
      return ~bits_any(s, bv.ipool + in.b, in.c, in.a == 0 ? BK_PROVIDER : BK_REGION, 0, w);
    case OP_FLD_EXISTS:
      return bits_word(s, in.a == 0 ? BR_PROV_SET : BR_REG_SET, w);
    case OP_FLD_DNE:
      return ~bits_word(s, in.a == 0 ? BR_PROV_SET : BR_REG_SET, w);
    case OP_FLD_GT:
    case OP_FLD_LT: {  // integer compare: per cluster of the word
      uint64_t m = 0;
      for (int q = 0; q < 64; q++) {
        const int c = 64 * w + q;
        if (c >= s.C) break;
        const uint32_t f = s.flags[c];
        const bool has = (in.a == 0 ? (f & CF_PROVIDER_INT) : (f & CF_REGION_INT)) != 0;
        const int64_t x = in.a == 0 ? s.provider_int[c] : s.region_int[c];
        if (has && (in.op == OP_FLD_GT ? x > in.v : x < in.v)) m |= 1ull << q;
      }
      return m;
    }
    case OP_ZONE_IN:  // a listed zone implies a zone
      return bits_any(s, bv.ipool + in.b, in.c, BK_ZONE, 0, w);
    case OP_ZONE_NOTIN:
      return ~bits_any(s, bv.ipool + in.b, in.c, BK_ZONE, 0, w);
    case OP_ZONE_EXISTS:
      return bits_word(s, BR_ZONE_ANY, w);
    case OP_ZONE_DNE:
      return ~bits_word(s, BR_ZONE_ANY, w);
    default:  // OP_FALSE and unknown opcodes
      return 0;
  }
}
// A ClusterMatches program: the AND of its instructions.
KP_HD inline uint64_t prog_word(const SnapView& s, const BatchView& bv, int32_t prog_id, int w) {
  const Prog p = kp_ldu(bv.progs + prog_id);
  uint64_t m = ~0ull;
  for (int i = 0; i < p.ins_cnt; i++) m &= instr_word(s, bv, kp_ldu(bv.instrs + p.ins_off + i), w);
  return m;
}

// Word w of the sets a binding's filter stages are made of; filter_word ANDs the stages
// together, body_fit_hist counts what each one drops.
// spec.Clusters members, which pass APIEnablement and TaintToleration (TargetContains)
KP_HD inline uint64_t fw_targets(const BatchView& bv, const BindHdr& h, int w) {
  return h.tgt_cnt > 0 ? rank_word(bv.ipool + h.tgt_off, h.tgt_cnt, w, 2) : 0ull;
}
// clusters that enable the binding's GVK
KP_HD inline uint64_t fw_api(const SnapView& s, const BindHdr& h, int w) {
  return h.gvk >= 0 ? bits_word(s, s.br_api + h.gvk, w) : 0ull;
}
// clusters whose taint list the binding tolerates (tolm: bit t = it tolerates list t)
KP_HD inline uint64_t fw_tolerated(const SnapView& s, uint64_t tolm, int w) {
  uint64_t tl = 0;
  for (uint64_t t = tolm; t; t &= t - 1) tl |= bits_word(s, s.br_tset + ctz64(t), w);
  return tl;
}
// ClusterAffinity: any term matches
KP_HD inline uint64_t fw_affinity(const SnapView& s, const BatchView& bv, const BindHdr& h, int w) {
  uint64_t a = 0;
  for (int j = 0; j < h.filt_cnt; j++) a |= prog_word(s, bv, kp_ldu(bv.ipool + h.filt_off + j), w);
  return a;
}
// clusters the binding is being evicted from (only with h.evict_cnt > 0)
KP_HD inline uint64_t fw_evicting(const BatchView& bv, const BindHdr& h, int w) {
  return rank_word(bv.ipool + h.evict_off, h.evict_cnt, w);
}

// Feasibility word w of binding h: the same expression as pair_eval_fast's `ok`
// (kp_algo.h), over bitset rows. tolm: bit t = the binding tolerates taint list t.
KP_HD inline uint64_t filter_word(const SnapView& s, const BatchView& bv, const BindHdr& h, int w, uint64_t tolm) {
  const int en = h.enabled;
  uint64_t m = bits_word(s, BR_BASE, w);
  const uint64_t in_t = fw_targets(bv, h, w);
  if (en & 1) m &= in_t | fw_api(s, h, w);
  if (en & 2) m &= in_t | fw_tolerated(s, tolm, w);
  if ((en & 4) && !(h.flags & BF_AFF_ALL)) m &= fw_affinity(s, bv, h, w);
  if (en & 8) {  // SpreadConstraint presence checks
    if (h.flags & BF_NEED_PROVIDER) m &= bits_word(s, BR_HAS_PROVIDER, w);
    if (h.flags & BF_NEED_REGION) m &= bits_word(s, BR_HAS_REGION, w);
    if (h.flags & BF_NEED_ZONES) m &= bits_word(s, BR_HAS_ZONES, w);
  }
  if ((en & 32) && h.evict_cnt > 0) m &= ~fw_evicting(bv, h, w);  // ClusterEviction
  return m;
}

// taints_tolerated (kp_algo.h) of taints [t0, t1) with the binding's first kTolRegs
// tolerations in tr[] (loaded once per binding) and the rest read from the pool.
constexpr int kTolRegs = 4;
KP_FI bool taints_tolerated_regs(const SnapView& s, const BatchView& bv, const BindHdr& h, const Tol (&tr)[kTolRegs],
                                 int t0, int t1) {
  for (int t = t0; t < t1; t++) {
    const int32_t k = s.taint_key[t], v = s.taint_val[t], e = s.taint_eff[t];
    auto hit = [&](const Tol& tl) {
      return (tl.eff == EFF_ANY || tl.eff == e) && (tl.key < 0 || tl.key == k) && (tl.op == TOL_EXISTS || tl.val == v);
    };
    bool tol = false;
KP_UNROLL
    for (int j = 0; j < kTolRegs; j++) tol = tol | (j < h.tol_cnt && hit(tr[j]));
    for (int j = kTolRegs; j < h.tol_cnt && !tol; j++) tol = hit(kp_ldu(bv.tols + h.tol_off + j));
    if (!tol) return false;
  }
  return true;
}

// k_filter: binding b's feasibility row fmask[b][0, W), by the calling wave (one
// lane per word; on the host build one "lane" walks every word). b is wave-uniform
// (the kernel passes it through kp_uniform): the header and everything filter_word
// walks from it (program ids, Progs, Instrs, values, table probes, row ids) then go
// through scalar loads and scalar registers, and only the bits words are vector loads.
template <class BLK>
KP_FI void body_filter(const BLK& B, int b, const SnapView& s, const BatchView& bv, uint64_t* fmask) {
  const BindHdr h = kp_ldu(bv.hdr + b);
  const int ww = B.wwidth(), lane = B.lane() & (ww - 1);
  uint64_t tolm = 0;  // TaintToleration once per distinct taint list (n_tsets <= kTsetRowsMax)
  if (h.enabled & 2) {
    // the binding's tolerations once, ahead of the taint loop
    Tol tr[kTolRegs];
KP_UNROLL
    for (int j = 0; j < kTolRegs; j++)
      tr[j] = j < h.tol_cnt ? kp_ldu(bv.tols + h.tol_off + j) : Tol{0, 0, TOL_EQUAL, -1};
    for (int t0 = 0; t0 < s.n_tsets; t0 += ww) {
      const int t = t0 + lane;
      int tt0 = 0, tt1 = 0;
      if (t < s.n_tsets) {
        const int c = s.tset_rep[t];
        tt0 = s.taint_off[c], tt1 = s.taint_off[c + 1];
      }
      const bool ok = t < s.n_tsets && taints_tolerated_regs(s, bv, h, tr, tt0, tt1);
      tolm |= B.wballot(ok) << t0;
    }
  }
  uint64_t* row = fmask + (size_t)b * s.W;
  for (int w0 = 0; w0 < s.W; w0 += ww) {
    const int w = w0 + lane;
    if (w < s.W) row[w] = filter_word(s, bv, h, w, tolm);
  }
}

// FindMatchingUntoleratedTaint over taints [t0, t1): the position of the first one the
// binding does not tolerate, -1 when it tolerates them all (taints_tolerated_regs' walk,
// which only needs to know whether there is one).
KP_FI int first_untolerated_regs(const SnapView& s, const BatchView& bv, const BindHdr& h, const Tol (&tr)[kTolRegs],
                                 int t0, int t1) {
  for (int t = t0; t < t1; t++) {
    const int32_t k = s.taint_key[t], v = s.taint_val[t], e = s.taint_eff[t];
    auto hit = [&](const Tol& tl) {
      return (tl.eff == EFF_ANY || tl.eff == e) && (tl.key < 0 || tl.key == k) && (tl.op == TOL_EXISTS || tl.val == v);
    };
    bool tol = false;
KP_UNROLL
    for (int j = 0; j < kTolRegs; j++) tol = tol | (j < h.tol_cnt && hit(tr[j]));
    for (int j = kTolRegs; j < h.tol_cnt && !tol; j++) tol = hit(kp_ldu(bv.tols + h.tol_off + j));
    if (!tol) return t;
  }
  return -1;
}

// k_fit_hist: the FitError reason histogram of binding list[i] (kp_fit_diagnosis_batch),
// by the calling wave, into its dense row dense[i][hist_stride] (kp_launch.h; zeroed before
// the launch). A cluster's reason is the first stage of pair_reason's plugin order whose
// word drops it, so each stage counts popcount(alive & ~stage word) over the words
// filter_word ANDs together: one lane per word as body_filter, the per-lane counts summed
// across the wave once at the end. i is wave-uniform, so the list entry, the header and the
// predicate walk are scalar loads.
// TaintToleration has one bin per distinct (key, value, effect) triple: the list's first
// untolerated taint, answered once per distinct taint list (one lane per list, where
// body_filter computes tolm), names the bin through taint_uid; uidl (kTsetRowsMax words of
// the wave's LDS) hands each list's bin to the whole wave. A list's rejected clusters are
// those still alive before the stage, outside spec.Clusters, that hold the list. Several
// lists may share a bin, so lane 0 adds each list's wave sum to the row with an atomic.
// frow[i] >= 0: the binding's row of the out-of-tree verdicts flt_rows[..][W], the last stage.
template <class BLK>
KP_FI void body_fit_hist(const BLK& B, int i, int32_t* uidl, const SnapView& s, const BatchView& bv,
                         const int32_t* list, const int32_t* frow, const uint64_t* flt_rows, uint32_t* dense) {
  const int b = kp_ldu(list + i), fr = kp_ldu(frow + i);
  const BindHdr h = kp_ldu(bv.hdr + b);
  const int ww = B.wwidth(), lane = B.lane() & (ww - 1);
  const int en = h.enabled, U = s.n_taint_uid;
  uint32_t* row = dense + (size_t)i * hist_stride(U);
  uint64_t tolm = 0;
  if (en & 2) {
    Tol tr[kTolRegs];
KP_UNROLL
    for (int j = 0; j < kTolRegs; j++)
      tr[j] = j < h.tol_cnt ? kp_ldu(bv.tols + h.tol_off + j) : Tol{0, 0, TOL_EQUAL, -1};
    for (int t0 = 0; t0 < s.n_tsets; t0 += ww) {
      const int t = t0 + lane;
      int fu = -1;
      if (t < s.n_tsets) {
        const int c = s.tset_rep[t];
        fu = first_untolerated_regs(s, bv, h, tr, s.taint_off[c], s.taint_off[c + 1]);
        uidl[t] = fu >= 0 ? s.taint_uid[fu] : -1;
      }
      tolm |= B.wballot(t < s.n_tsets && fu < 0) << t0;
    }
    B.wsync();
  }
  // alive before TaintToleration (and the spec.Clusters members, which it passes)
  auto before_taint = [&](int w, uint64_t* in_t) {
    *in_t = fw_targets(bv, h, w);
    uint64_t m = bits_word(s, BR_BASE, w);
    if (en & 1) m &= *in_t | fw_api(s, h, w);
    return m;
  };
  uint32_t n_fit = 0, n_del = 0, c_api = 0, c_aff = 0, c_prov = 0, c_reg = 0, c_zone = 0, c_evict = 0, c_oot = 0;
  for (int w = lane; w < s.W; w += ww) {
    const int nv = s.C - 64 * w;  // clusters of this word (the last one's padding bits are no clusters)
    const uint64_t valid = nv >= 64 ? ~0ull : nv > 0 ? (1ull << nv) - 1 : 0ull;
    const uint64_t base = bits_word(s, BR_BASE, w);
    n_del += (uint32_t)popc64(valid & ~base);
    uint64_t in_t;
    uint64_t m = before_taint(w, &in_t);
    c_api += (uint32_t)popc64(base & ~m);
    if (en & 2) m &= in_t | fw_tolerated(s, tolm, w);  // (counted per list below)
    if ((en & 4) && !(h.flags & BF_AFF_ALL)) {
      const uint64_t a = fw_affinity(s, bv, h, w);
      c_aff += (uint32_t)popc64(m & ~a);
      m &= a;
    }
    if (en & 8) {  // SpreadConstraint: the constraints in spec order
      for (int k = 0; k < 3; k++) {
        const int fld = (h.spread_order >> (2 * k)) & 3;
        if (fld == 0) continue;
        const uint64_t p = bits_word(s, fld == 1 ? BR_HAS_PROVIDER : fld == 2 ? BR_HAS_REGION : BR_HAS_ZONES, w);
        const uint32_t d = (uint32_t)popc64(m & ~p);
        c_prov += fld == 1 ? d : 0u;
        c_reg += fld == 2 ? d : 0u;
        c_zone += fld == 3 ? d : 0u;
        m &= p;
      }
    }
    if ((en & 32) && h.evict_cnt > 0) {
      const uint64_t ev = fw_evicting(bv, h, w);
      c_evict += (uint32_t)popc64(m & ev);
      m &= ~ev;
    }
    if (fr >= 0) {
      const uint64_t x = flt_rows[(size_t)fr * s.W + w];
      c_oot += (uint32_t)popc64(m & ~x);
      m &= x;
    }
    n_fit += (uint32_t)popc64(m);
  }
  if (en & 2) {
    for (int t = 0; t < s.n_tsets; t++) {
      if ((tolm >> t) & 1) continue;  // wave-uniform
      uint32_t c = 0;
      for (int w = lane; w < s.W; w += ww) {
        uint64_t in_t;
        const uint64_t m = before_taint(w, &in_t);
        c += (uint32_t)popc64(m & ~in_t & bits_word(s, s.br_tset + t, w));
      }
      c = (uint32_t)B.wsum32((int32_t)c);
      if (lane == 0 && c) kp_atomic_add(row + hist_slot_uid(uidl[t]), c);
    }
  }
  n_fit = (uint32_t)B.wsum32((int32_t)n_fit);
  n_del = (uint32_t)B.wsum32((int32_t)n_del);
  c_api = (uint32_t)B.wsum32((int32_t)c_api);
  c_aff = (uint32_t)B.wsum32((int32_t)c_aff);
  c_prov = (uint32_t)B.wsum32((int32_t)c_prov);
  c_reg = (uint32_t)B.wsum32((int32_t)c_reg);
  c_zone = (uint32_t)B.wsum32((int32_t)c_zone);
  c_evict = (uint32_t)B.wsum32((int32_t)c_evict);
  c_oot = (uint32_t)B.wsum32((int32_t)c_oot);
  if (lane == 0) {
    row[0] = n_fit;
    row[1] = n_del;
    row[hist_slot(1, U)] = c_api;
    row[hist_slot(3, U)] = c_aff;
    row[hist_slot(4, U)] = c_prov;
    row[hist_slot(5, U)] = c_reg;
    row[hist_slot(6, U)] = c_zone;
    row[hist_slot(7, U)] = c_evict;
    row[hist_slot(8, U)] = c_oot;
  }
}

// k_affected (kp_affected_bindings): the transposed question of the filter, "does the one
// affinity enqueueAffectedBindings reads for binding b (event_handler.go:417-431) match any of
// a few changed clusters", by the calling wave. wprog[b] is that affinity's program in the
// watch's pools (bv holds progs / instrs / ipool only), kWatchAlways for a nil affinity or a
// binding listed on every event, kWatchNever for one never listed. b is wave-uniform, so
// wprog[b] and the program walk are scalar loads as in body_filter. cnt[b] = 1 when listed.
// util.ClusterMatches alone decides: BR_BASE (the not-deleting row of findClustersThatFit) is
// not ANDed, and cw_mask carries bits of real clusters only, which clears what the negated
// rows set past C.
// Over the snapshot's bitset rows: the changed clusters as n_cw distinct 64-cluster words
// (cw_word[j] < W, cw_mask[j] their bits), one lane per changed word; the loop leaves
// wave-uniformly at the first word that holds a match.
template <class BLK>
KP_FI void body_affected(const BLK& B, int b, const SnapView& s, const BatchView& bv, const int32_t* wprog,
                         const int32_t* cw_word, const uint64_t* cw_mask, int n_cw, uint32_t* cnt) {
  const int32_t p = kp_ldu(wprog + b);
  const int ww = B.wwidth(), lane = B.lane() & (ww - 1);
  bool hit = p == kWatchAlways;
  if (p >= 0) {
    for (int j0 = 0; j0 < n_cw && !hit; j0 += ww) {  // (wave-uniform trip count: the ballot)
      const int j = j0 + lane;
      uint64_t m = 0;
      if (j < n_cw) m = prog_word(s, bv, p, cw_word[j]) & cw_mask[j];
      hit = B.wballot(m != 0) != 0;
    }
  }
  if (lane == 0) cnt[b] = hit ? 1u : 0u;
}
// Without the bitset rows (or under KP_PAIR_ROWS=1): the changed clusters as n distinct ranks
// (each < C), one lane per changed cluster through the per-pair evaluator.
template <class BLK>
KP_FI void body_affected_rows(const BLK& B, int b, const SnapView& s, const BatchView& bv, const int32_t* wprog,
                              const int32_t* ranks, int n, uint32_t* cnt) {
  const int32_t p = kp_ldu(wprog + b);
  const int ww = B.wwidth(), lane = B.lane() & (ww - 1);
  bool hit = p == kWatchAlways;
  if (p >= 0) {
    for (int j0 = 0; j0 < n && !hit; j0 += ww) {  // (wave-uniform trip count: the ballot)
      const int j = j0 + lane;
      const bool m = j < n && prog_match(s, bv, p, ranks[j]);
      hit = B.wballot(m) != 0;
    }
  }
  if (lane == 0) cnt[b] = hit ? 1u : 0u;
}
// k_affected_write: after the offsets scan over cnt, a listed binding's index at its offset
// (one thread per binding), so the list is ascending and distinct by construction.
KP_HD inline void body_affected_write(int b, const uint32_t* cnt, const uint64_t* offsets, uint32_t* out) {
  if (cnt[b]) out[offsets[b]] = (uint32_t)b;
}

}  // namespace kp
