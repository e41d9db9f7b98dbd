// kp_dev.h — the device interface the host units (engine.cpp, snapshot.cpp, pack.cpp, nodes.cpp) run on.
//
// libkp.so implements it with HIP on gfx950 (kernels.hip). The test-only
// libkp_cpusim.so implements it on the host (dev_cpu.cpp) by running the same
// kernel bodies (kp_kernels.h) with a 1-thread block policy, so the engine's
// orchestration and kernel logic can be checked without a GPU. The CPU build
// is never linked into libkp.so.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kp_launch.h"

namespace kp {
struct SetsArgs;
struct TopArgs;
struct OrderArgs;
struct RegionOut;
struct GradesArgs;
struct NodeEstArgs;
struct NodeView;
struct ClaimProg;
struct NodeSetsArgs;
struct AssumedView;
namespace dev {

typedef void* stream_t;
typedef void* event_t;

int device_count();
int set_device(int device);
size_t max_lds_per_block(int device);
const char* last_error();  // text of the last failing call

int stream_create(stream_t* s);
void stream_destroy(stream_t s);
int sync(stream_t s);
int event_create(event_t* e);
void event_destroy(event_t e);
int event_record(event_t e, stream_t s);
int event_sync(event_t e);  // host waits for e
int stream_wait(stream_t s, event_t e);  // s waits for e (no host block)
float event_ms(event_t a, event_t b);

int alloc(void** p, size_t bytes);
void release(void* p);
// Page-locked host memory: the result copy-back DMAs straight into it.
int host_alloc(void** p, size_t bytes);
void host_release(void* p);
int h2d(void* dst, const void* src, size_t bytes, stream_t s);  // stream-ordered
int d2h(void* dst, const void* src, size_t bytes, stream_t s);
int fill(void* dst, int value, size_t bytes, stream_t s);
// Device-to-device copy between GPUs (xGMI peer copy; same device: a local copy).
int peer_copy(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, stream_t s);

// fast: the estimator instance (EST_*); other than EST_GENERIC only for batches
// that meet pair_fast_ok.
// Pair rows of bindings list[b0 + i] (or b0 + i when list is null), i < nb.
int pair(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* list, int b0, int nb, uint64_t* fmask,
         int32_t* est, int64_t* score, int est_mode, int md_cap, size_t smem, int fast = 0);
// Estimator-class rows: rows[k][Cp] for k = klist[i] (k = i when klist is null), i < n_rows
// (body_est_class; row 0 MaxInt32), class k's representative binding rep[k]; fast = EST_*
// kind (not EST_GENERIC). fmask set: only the entries of the representative's feasible
// clusters (the singleton classes of a batch without class orders, after k_filter).
int est_class(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* rep, int n_rows, int32_t* rows,
              int fast, const int32_t* klist = nullptr, const uint64_t* fmask = nullptr);
// Feasibility rows fmask[b][W] of every binding by bitset algebra (body_filter;
// requires s.n_bits > 0).
int filter(stream_t st, const SnapView& s, const BatchView& bv, uint64_t* fmask);
// kp_batch_create_filters: the out-of-tree filter plugins' verdicts ANDed into the feasibility
// rows of the n listed bindings (body_filter_extra): fmask[list[i].b] &= rows[list[i].r],
// rows [..][W] words by cluster rank. est (pair-row mode, else null): those bindings' estimate
// rows [..][Cp], zeroed where the row rejects.
int filter_extra(stream_t st, const SnapView& s, const FltPair* list, int n, const uint64_t* rows, uint64_t* fmask,
                 int32_t* est);
// kp_filter_reasons on such a batch: KP_REASON_OUT_OF_TREE into the reasons rows of the n
// listed bindings (all within the chunk that starts at binding b0) where the in-tree set
// fits and the row rejects (body_reasons_extra).
int reasons_extra(stream_t st, const SnapView& s, const FltPair* list, int n, const uint64_t* rows, int b0,
                  uint32_t* out);
int select(stream_t st, int which, const KArgs& a, size_t smem, int cap, const SelectExtra& x);
// Region stage B of the wide-listed bindings that k_region_b marked (body_region_wide):
// `grid` persistent workgroups, each with a slot of slot_bytes in scratch, over the rows
// wide[0, n_wide) of the region list a.list (x.rsel / x.rnsel by row; x.dargs: a on the
// device); lds_sort bytes of LDS for the candidate sort (0: in the slot); *n_done counts
// the bindings it scheduled or errored.
int region_wide(stream_t st, const KArgs& a, const SelectExtra& x, const int32_t* wide, int n_wide,
                unsigned char* scratch, size_t slot_bytes, int grid, int cap, int lds_sort, uint32_t* n_done);
// Estimator-class orders for k_select_top: ord[k][i] = (estimate << 32 | rank) of
// rows[k] sorted by estimate desc, rank asc; tot[k] its sum; ok[k] whether it can be
// walked (body_class_order). C <= 16384.
int class_order(stream_t st, const SnapView& s, const int32_t* rows, int n_rows, uint64_t* ord, int64_t* tot,
                int32_t* ok);
// SEL_ALL DynamicWeight / Aggregated bindings a.list[0, a.n) over their deciding
// candidates (body_select_top), `slice` bytes of LDS per binding; the others are
// appended to t.fb.
// (a.n_dev set: the list's length is on the device, a.n its capacity; max_grid > 0
// bounds the grid, whose waves then stride over the list)
int select_top(stream_t st, const KArgs& a, const TopArgs& t, size_t slice, int max_grid = 0);
// selectGroups for n region bindings (one thread each): rsel/rnsel as the host
// step writes them; *nhost counts the bindings left to the host (kGroupsHost).
int region_groups(stream_t st, const RegionOut* rout, const int32_t* rstat, const BindHdr* hdr, const int32_t* list,
                  int n, int R, int32_t* rsel, int32_t* rnsel, uint32_t* nhost);
// kp_max_available_component_sets: out[i] = sets_one for cluster rank ranks[i]
// (A, ranks and off in device memory; cluster i's runs at scratch[off[i], off[i+1])).
int component_sets(stream_t st, const SnapView& s, const SetsArgs* A, const int32_t* ranks, const int64_t* off,
                   uint64_t n, int64_t* scratch, int32_t* out);
// Component-set class row: row[r] = sets_one for every cluster rank r < C (cluster r's
// runs at scratch[off[r], off[r+1])); *ovf = 1 when a simulation outgrew its runs.
int sets_rows(stream_t st, const SnapView& s, const SetsArgs* A, const int64_t* off, int64_t* scratch, int32_t* row,
              uint32_t* ovf);
// Pair-row mode: est[b][c] of the n bindings list[i] rebuilt from their class rows
// (cal_merge_bf with spec.Replicas on feasible clusters, 0 elsewhere, as pair_eval writes).
int rows_from_class(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* list, int n,
                    const int32_t* bcls, const int32_t* cls_rows, const uint64_t* fmask, int32_t* est);
// kp_batch_create_estimates: the other estimators' answers merged into n estimate rows
// (body_est_extra): row d = list[i] (i when list is null) of rows[..][Cp], its class
// bcls[d] (d when bcls is null), that class's row cls_est[class] of extra[..][Cp] (rank
// order, -1 = no answer; negative cls_est: the row is left alone).
int est_extra(stream_t st, int Cp, const int32_t* list, int n, const int32_t* bcls, const int32_t* cls_est,
              const int32_t* extra, int32_t* rows);
// kp_assumptions_create: the n clusters of A (body_assume_cluster, one wave each): their
// Allocating sums, pods, residual model-node runs and status.
int assume_cluster(stream_t st, const SnapView& s, const AssumedView& A);
// An assumed batch's estimate rows corrected at A's clusters (body_est_assumed), one wave per
// (row, cluster): rows [row0, row0 + n_rows) of rows[..][Cp] in mode EA_* (kp_assume.h).
int est_assumed(stream_t st, const SnapView& s, const BatchView& bv, const AssumedView& A, int mode, const int32_t* rep,
                const uint64_t* fmask, int row0, int n_rows, int32_t* rows);
// kp_schedule_affinities_ex: a call's answer rows, uploaded in caller cluster order, into rank
// order (body_est_rows_rank, body_flt_rows_rank). src[n_rows][C] -> dst[n_rows][Cp] with -1
// in the padding; src[n_rows][ceil(C/64)] -> dst[n_rows][W] words with zero bits there.
int est_rows_rank(stream_t st, const SnapView& s, const int32_t* src, int n_rows, int32_t* dst);
int flt_rows_rank(stream_t st, const SnapView& s, const uint64_t* src, int n_rows, uint64_t* dst);
// kp_model_grades: A.counts[grade] += 1 per node (body_grades); A's arrays in device memory.
int grades(stream_t st, const GradesArgs& A);
// kp_node_max_replicas: *A.sum += int32 sum of node_replicas over the nodes (wrapping).
int node_est(stream_t st, const NodeEstArgs& A);
// StaticWeight SEL_ALL bindings a.list[0, a.n) at class level (body_select_static),
// one wave each with `slice` bytes of LDS.
int select_static(stream_t st, const KArgs& a, size_t slice);
// Spread selections over the estimator-class orders (body_spread_order), one wave
// per binding, `slice` bytes of LDS each; unfinished list positions go to o.fb.
int spread_order(stream_t st, const KArgs& a, const OrderArgs& o, size_t slice);
// Region stage A of the order-eligible bindings (body_region_a_order), one wave per
// binding; the other list positions go to fb.
int region_a_order(stream_t st, const KArgs& a, RegionOut* rout, int32_t* rstat, int32_t* fb, uint32_t* fb_n,
                   size_t slice);
// kp_node_max_component_sets: match[k * n + j] = MatchNode(node j, P[k]) (P in
// device memory), then the first-fit set simulation by one wave (A in device memory).
int node_match(stream_t st, const NodeView& v, const ClaimProg* P, int K, uint8_t* match);
int node_sets(stream_t st, const NodeSetsArgs* A);
// kp_filter_reasons: out[(b - b0) * C + r] = pair_reason of binding b in [b0, b0 + nb), cluster rank r.
int reasons(stream_t st, const SnapView& s, const BatchView& bv, int b0, int nb, uint32_t* out);
// kp_fit_diagnosis_batch. fit_hist: the dense reason histogram rows dense[i][hist_stride]
// (zeroed by the caller) of the n bindings list[i] by bitset algebra (body_fit_hist; requires
// s.n_bits > 0), frow[i] the binding's row of flt_rows or -1. reason_hist: the same rows from
// n rows of reason words words[i][C] (body_reason_hist). hist_count: nbins[i] = the row's
// non-zero bins; hist_write: the bins at offsets[i] .. and n_fit / n_del (body_hist_write).
int fit_hist(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* list, const int32_t* frow, int n,
             const uint64_t* flt_rows, uint32_t* dense);
int reason_hist(stream_t st, const SnapView& s, const uint32_t* words, int n, uint32_t* dense);
int hist_count(stream_t st, int n, int U, const uint32_t* dense, uint32_t* nbins);
int hist_write(stream_t st, int n, int U, const uint32_t* uid_ref, const uint32_t* dense, const uint64_t* offsets,
               uint32_t* reason, uint32_t* taint_ref, uint32_t* count, uint32_t* n_fit, uint32_t* n_del);
// kp_affected_bindings over a watch's bv.B bindings (bv: progs / instrs / ipool only; wprog[b]
// a program id, kWatchAlways or kWatchNever): cnt[b] = 1 when binding b's affinity matches one
// of the changed clusters. affected (body_affected; requires s.n_bits > 0): the clusters as
// n_cw distinct words cw_word[j] < s.W with their bits cw_mask[j]; affected_rows
// (body_affected_rows): as n distinct ranks < s.C. affected_write: the listed bindings'
// indices at offsets[b] (the scan of cnt), ascending.
int affected(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* wprog, const int32_t* cw_word,
             const uint64_t* cw_mask, int n_cw, uint32_t* cnt);
int affected_rows(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* wprog, const int32_t* ranks,
                  int n, uint32_t* cnt);
int affected_write(stream_t st, int n, const uint32_t* cnt, const uint64_t* offsets, uint32_t* out);
// CSR offsets[n + 1] of the per-binding results (counts of OK bindings), on the device;
// part: ceil(n / kOffChunk) u64 of scratch.
int offsets(stream_t st, const int32_t* status, const uint32_t* count, int n, uint64_t* off, uint64_t* part);
// (in_idx holds snapshot ranks; out_idx gets perm[rank], the caller's cluster index)
int compact(stream_t st, const uint64_t* start, const uint32_t* count, const uint64_t* offsets, const uint32_t* in_idx,
            const int32_t* in_rep, uint32_t* out_idx, int32_t* out_rep, int n, const uint32_t* perm);
// The packed result form (kp_results_packed), in compact's place: out[offsets[b] + i] = the
// packed word of binding b's entry i (perm[rank] | replicas << 16, 0xFFFF for escaped
// replicas) and wide_count[b] = its escaped entries (body_pack); then, with wide_offsets
// scanned from those counts (offsets above), the escaped replicas in entry order at
// out[wide_offsets[b] ..] (body_pack_wide).
int pack(stream_t st, const uint64_t* start, const uint64_t* offsets, const uint32_t* in_idx, const int32_t* in_rep,
         uint32_t* out, uint32_t* wide_count, int n, const uint32_t* perm);
int pack_wide(stream_t st, const uint64_t* start, const uint64_t* offsets, const uint64_t* wide_offsets,
              const int32_t* in_rep, int32_t* out, int n);
// The delta result form (kp_results_delta), before the scans: flag[b] = 1 and mcount[b] =
// count[b] for a binding whose result differs from its spec.Clusters, 0 and 0 otherwise
// (body_changed over every binding; body_changed_long over list[0, n), the bindings whose
// header satisfies kp::changed_long, which body_changed leaves to it). changed_list, after
// the scans of flag (chg_off) and mcount (moff), both [n + 1]: the changed bindings'
// indices, ascending, and out_off[0 .. n_changed] = their CSR offsets.
int changed(stream_t st, const BatchView& bv, const int32_t* status, const uint64_t* start, const uint32_t* count,
            const uint32_t* in_idx, const int32_t* in_rep, uint32_t* flag, uint32_t* mcount);
int changed_long(stream_t st, const SnapView& s, const BatchView& bv, const int32_t* list, int n, const int32_t* status,
                 const uint64_t* start, const uint32_t* count, const uint32_t* in_idx, const int32_t* in_rep,
                 uint32_t* flag, uint32_t* mcount);
int changed_list(stream_t st, int n, const uint32_t* flag, const uint64_t* chg_off, const uint64_t* moff,
                 uint32_t* changed, uint64_t* out_off);

}  // namespace dev
}  // namespace kp
