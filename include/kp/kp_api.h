/*
 * kp_api.h — C-ABI of the MI355X batched placement engine ("kp") for Karmada's
 * scheduling hot path (genericScheduler.Schedule).
 *
 * Two layers live in this header:
 *
 *   1. The OBJECT MODEL: plain C structs that mirror the subset of the Karmada
 *      API types the placement path reads. A cgo shim fills them from the Go
 *      objects; the Python test harness fills them through
 *      ctypes. Field names follow the Go/JSON names of the reference types:
 *        kp_cluster          <- clusterv1alpha1.Cluster
 *                               (pkg/apis/cluster/v1alpha1/types.go:43-377)
 *        kp_binding          <- workv1alpha2.ResourceBindingSpec + Status subset
 *                               (pkg/apis/work/v1alpha2/binding_types.go:71-300,443-467)
 *        kp_cluster_affinity <- policyv1alpha1.ClusterAffinity
 *                               (pkg/apis/policy/v1alpha1/propagation_types.go:445-772)
 *      Strings are (ptr,len) views; slices are (ptr,count). Nothing is retained
 *      after a call returns (cgo pointer rules): the engine copies/packs inputs.
 *
 *   2. The ENTRY POINTS (kp_*), each replacing a reference interface:
 *        kp_schedule_batch          <- core.ScheduleAlgorithm.Schedule
 *                                      (pkg/scheduler/core/generic_scheduler.go:37-49,71-116)
 *        kp_filter_batch            <- framework.FilterPlugin.Filter for the in-tree filter set
 *                                      (pkg/scheduler/framework/interface.go:85-98,
 *                                       pkg/scheduler/framework/runtime/framework.go:93-122)
 *        kp_filter_reasons          <- framework.FitError's Diagnosis (framework/types.go:56-90)
 *        kp_score_batch             <- framework.ScorePlugin.Score summed by RunScorePlugins
 *                                      (pkg/scheduler/framework/interface.go:215-232,
 *                                       pkg/scheduler/framework/runtime/framework.go:126-170)
 *        kp_max_available_replicas  <- estimatorclient.ReplicaEstimator.MaxAvailableReplicas
 *                                      for the GeneralEstimator
 *                                      (pkg/estimator/client/interface.go:39-71,
 *                                       pkg/estimator/client/general.go:57-108)
 *        kp_max_available_component_sets <- ReplicaEstimator.MaxAvailableComponentSets
 *                                      (general.go:154-292)
 *        kp_model_grades            <- getAllocatableModelings over modeling.AddToResourceSummary
 *                                      (pkg/controllers/status/cluster_status_controller.go:642-677)
 *        kp_node_max_replicas       <- noderesource.nodeResourceEstimator.Estimate (estimator server,
 *                                      pkg/estimator/server/framework/plugins/noderesource)
 *        kp_node_max_component_sets <- noderesource.nodeResourceEstimator.EstimateComponents
 *        kp_snapshot_create         <- cache.Cache.Snapshot (pkg/scheduler/cache/cache.go:124-139)
 *        kp_schedule_affinities     <- Scheduler.scheduleResourceBindingWithClusterAffinities
 *                                      (pkg/scheduler/scheduler.go:584-585,618-684)
 *        kp_affected_bindings       <- Scheduler.enqueueAffectedBindings / enqueueAffectedCRBs
 *                                      (pkg/scheduler/event_handler.go:400-491)
 *
 * Return convention: 0 = OK, <0 = KP_E* ; kp_last_error() gives the text.
 * No exceptions cross the ABI. An engine handle is not re-entrant.
 */
#ifndef KP_API_H
#define KP_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KP_ABI_VERSION 16

/* ------------------------------------------------------------------------- */
/* Object model                                                              */
/* ------------------------------------------------------------------------- */

typedef struct kp_str {
  const char* ptr;
  uint32_t len;
} kp_str;

/* map[string]string entry (labels, matchLabels). */
typedef struct kp_label {
  kp_str key;
  kp_str value;
} kp_label;

/* metav1.LabelSelectorRequirement / corev1.NodeSelectorRequirement. `op` is the
 * operator string exactly as in the API ("In", "NotIn", "Exists", ...). */
typedef struct kp_requirement {
  kp_str key;
  kp_str op;
  const kp_str* values;
  uint32_t n_values;
} kp_requirement;

/* policyv1alpha1.ClusterAffinity (propagation_types.go). */
typedef struct kp_cluster_affinity {
  uint8_t has_label_selector; /* LabelSelector != nil */
  const kp_label* match_labels;
  uint32_t n_match_labels;
  const kp_requirement* match_expressions;
  uint32_t n_match_expressions;
  uint8_t has_field_selector; /* FieldSelector != nil */
  const kp_requirement* field_expressions;
  uint32_t n_field_expressions;
  const kp_str* cluster_names;
  uint32_t n_cluster_names;
  const kp_str* exclude_clusters;
  uint32_t n_exclude_clusters;
} kp_cluster_affinity;

/* policyv1alpha1.ClusterAffinityTerm: {AffinityName, ClusterAffinity, OverflowAffinities}. */
typedef struct kp_affinity_term {
  kp_str affinity_name;
  kp_cluster_affinity affinity;
  const kp_cluster_affinity* overflow; /* OverflowAffinities[i].ClusterAffinity */
  uint32_t n_overflow;
} kp_affinity_term;

/* corev1.Toleration (TolerationSeconds is irrelevant for placement). */
typedef struct kp_toleration {
  kp_str key;
  kp_str op; /* "", "Equal", "Exists", "Lt", "Gt", ... */
  kp_str value;
  kp_str effect;
} kp_toleration;

/* corev1.Taint. */
typedef struct kp_taint {
  kp_str key;
  kp_str value;
  kp_str effect;
} kp_taint;

/* policyv1alpha1.SpreadConstraint (MaxGroups/MinGroups are Go `int`). */
typedef struct kp_spread_constraint {
  kp_str spread_by_field; /* "cluster" | "region" | "zone" | "provider" | "" */
  kp_str spread_by_label;
  int64_t max_groups;
  int64_t min_groups;
} kp_spread_constraint;

/* policyv1alpha1.StaticClusterWeight. */
typedef struct kp_static_weight {
  kp_cluster_affinity target;
  int64_t weight;
} kp_static_weight;

/* corev1.ResourceList entry: name + resource.Quantity string ("100m", "2Gi", ...). */
typedef struct kp_resource {
  kp_str name;
  kp_str quantity;
} kp_resource;

/* workv1alpha2.TargetCluster (Components omitted: multi-template gate is off). */
typedef struct kp_target_cluster {
  kp_str name;
  int32_t replicas;
} kp_target_cluster;

/* workv1alpha2.Component (pkg/apis/work/v1alpha2/binding_types.go): one pod template
 * of a multi-template workload; ReplicaRequirements.ResourceRequest only (the
 * NodeClaim never filters the estimator's model nodes, which carry no Node object,
 * scheduling_simulator_components.go:149-153). */
typedef struct kp_component {
  kp_str name;
  int32_t replicas;
  uint8_t has_replica_requirements;
  const kp_resource* resource_request;
  uint32_t n_resource_request;
} kp_component;

/* ResourceBindingSpec + the status fields Schedule reads. */
typedef struct kp_binding {
  kp_str uid; /* spec.Resource.UID: FNV tie-break (pkg/util/helper/binding.go:117-144) */
  kp_str api_version;
  kp_str kind;
  kp_str namespace_;
  kp_str name;
  int32_t replicas;
  uint8_t has_replica_requirements; /* spec.ReplicaRequirements != nil */
  uint8_t has_node_claim;           /* ReplicaRequirements.NodeClaim != nil: no effect on the
                                       general estimator (a NodeClaim converts without error and
                                       every model node matches it, accurate.go:155-177,
                                       scheduling_simulator_components.go:149-153) */
  const kp_resource* resource_request;
  uint32_t n_resource_request;
  uint32_t n_components; /* len(spec.Components) */
  const kp_component* components; /* spec.Components (binding_types.go:89-98): read only with the
                                     MultiplePodTemplatesScheduling gate on, for bindings
                                     isMultiTemplateSchedulingApplicable accepts
                                     (core/estimation.go:43-65); NULL there -> KP_EINVAL */
  const kp_target_cluster* clusters; /* spec.Clusters (previous result) */
  uint32_t n_clusters;
  const kp_str* eviction_from; /* spec.GracefulEvictionTasks[].FromCluster */
  uint32_t n_eviction_from;
  uint8_t has_reschedule_triggered_at;
  uint8_t has_last_scheduled_time;
  int64_t reschedule_triggered_at_ns; /* unix nanoseconds */
  int64_t last_scheduled_time_ns;
  kp_str observed_affinity_name; /* status.SchedulerObservedAffinityName */
  /* spec.Placement */
  uint8_t has_cluster_affinity;
  kp_cluster_affinity cluster_affinity;
  const kp_affinity_term* cluster_affinities;
  uint32_t n_cluster_affinities;
  const kp_toleration* tolerations; /* ClusterTolerations */
  uint32_t n_tolerations;
  const kp_spread_constraint* spread_constraints;
  uint32_t n_spread_constraints;
  uint8_t has_replica_scheduling;
  kp_str replica_scheduling_type;     /* "Duplicated" | "Divided" */
  kp_str replica_division_preference; /* "Aggregated" | "Weighted" */
  uint8_t has_weight_preference;
  const kp_static_weight* static_weights;
  uint32_t n_static_weights;
  kp_str dynamic_weight; /* "AvailableReplicas" | "" */
} kp_binding;

/* Cluster.Status.APIEnablements flattened to (GroupVersion, Resources[].Kind) pairs. */
typedef struct kp_api_enablement {
  kp_str group_version;
  kp_str kind;
} kp_api_enablement;

/* clusterv1alpha1.ResourceModelRange / ResourceModel / AllocatableModeling. */
typedef struct kp_model_range {
  kp_str name;
  kp_str min;
  kp_str max;
} kp_model_range;

typedef struct kp_resource_model {
  uint32_t grade;
  const kp_model_range* ranges;
  uint32_t n_ranges;
} kp_resource_model;

typedef struct kp_allocatable_modeling {
  uint32_t grade;
  int64_t count;
} kp_allocatable_modeling;

/* clusterv1alpha1.Cluster subset. */
typedef struct kp_cluster {
  kp_str name;
  uint8_t deleting; /* !DeletionTimestamp.IsZero() */
  const kp_label* labels;
  uint32_t n_labels;
  kp_str provider;
  kp_str region;
  kp_str zone;
  const kp_str* zones;
  uint32_t n_zones;
  const kp_taint* taints;
  uint32_t n_taints;
  const kp_api_enablement* api_enablements;
  uint32_t n_api_enablements;
  const kp_resource_model* resource_models; /* Spec.ResourceModels */
  uint32_t n_resource_models;
  uint8_t has_resource_summary; /* Status.ResourceSummary != nil */
  const kp_resource* allocatable;
  uint32_t n_allocatable;
  const kp_resource* allocated;
  uint32_t n_allocated;
  const kp_resource* allocating;
  uint32_t n_allocating;
  const kp_allocatable_modeling* allocatable_modelings;
  uint32_t n_allocatable_modelings;
} kp_cluster;


/* In-tree plugin names (pkg/scheduler/framework/plugins/registry.go:33-50). */
enum {
  KP_PLUGIN_API_ENABLEMENT = 1u << 0,
  KP_PLUGIN_TAINT_TOLERATION = 1u << 1,
  KP_PLUGIN_CLUSTER_AFFINITY = 1u << 2,
  KP_PLUGIN_SPREAD_CONSTRAINT = 1u << 3,
  KP_PLUGIN_CLUSTER_LOCALITY = 1u << 4,
  KP_PLUGIN_CLUSTER_EVICTION = 1u << 5,
  KP_PLUGIN_ALL = 0x3fu
};

/* Flags and gates that change results (cmd/scheduler/app/options/options.go:130-165,
 * pkg/features/features.go:162-189). */
typedef struct kp_options {
  uint8_t enable_empty_workload_propagation;   /* --enable-empty-workload-propagation */
  uint8_t customized_cluster_resource_modeling; /* feature gate, default on */
  uint8_t multiple_pod_templates_scheduling;    /* feature gate MultiplePodTemplatesScheduling, alpha, default off */
  uint32_t enabled_plugins;                     /* KP_PLUGIN_* bitmask (--plugins) */
  /* Filter or score plugins the scheduler's registry holds beyond the in-tree set
   * (app.WithPlugin, cmd/scheduler/app/scheduler.go:90). RunFilterPlugins and
   * RunScorePlugins (runtime/framework.go:93-170) run every registered plugin, so
   * the batch path, which computes the in-tree set only, would place differently:
   * kp_schedule_batch, kp_schedule_affinities and kp_multi_schedule return
   * KP_ENOTSUP for a snapshot with n_out_of_tree_plugins > 0, except that a batch
   * holding those plugins' filter verdicts (kp_batch_create_filters, filter-only
   * plugins, n_plugins equal to this count) schedules, and so does
   * kp_schedule_affinities_ex with such answers. The per-pair entry
   * points (kp_filter_reasons, kp_score_batch, kp_max_available_replicas) still
   * answer for the in-tree set, for the framework to combine with the others. */
  uint32_t n_out_of_tree_plugins;
} kp_options;

/* ------------------------------------------------------------------------- */
/* Results                                                                   */
/* ------------------------------------------------------------------------- */

/* Error class of one Schedule call (framework/types.go:61-99). */
enum {
  KP_STATUS_OK = 0,
  KP_STATUS_FIT_ERROR = 1,     /* *framework.FitError */
  KP_STATUS_UNSCHEDULABLE = 2, /* *framework.UnschedulableError (possibly wrapped) */
  KP_STATUS_ERROR = 3          /* any other error */
};

/* The reference error site that produced a non-OK status. */
enum {
  KP_ERR_NONE = 0,                   /* with KP_STATUS_ERROR: a request the packer rejected (never the select
                                        paths: a region spread selects any number of clusters up to the
                                        snapshot's, and spec.Clusters may repeat names at any length) */
  KP_ERR_FIT = 1,                    /* generic_scheduler.go:84-89; arg = NumAllClusters */
  KP_ERR_REGION_MIN_GROUPS = 2,      /* select_clusters_by_region.go:30-32 */
  KP_ERR_REGION_CLUSTER_MIN = 3,     /* select_clusters_by_region.go:37-39 */
  KP_ERR_CLUSTER_MIN_GROUPS = 4,     /* select_clusters_by_cluster.go:28-30 */
  KP_ERR_CLUSTER_RESOURCE = 5,       /* select_clusters_by_cluster.go:39-41; arg = needCnt */
  KP_ERR_SPREAD_UNSUPPORTED = 6,     /* select_clusters.go:54 */
  KP_ERR_NO_CLUSTERS = 7,            /* common.go:55-57 */
  KP_ERR_UNSUPPORTED_STRATEGY = 8,   /* common.go:143-148 */
  KP_ERR_OVERFLOW_NOT_ENOUGH = 9,    /* common.go:132-134 */
  KP_ERR_FRESH_NOT_ENOUGH = 10,      /* assignment.go:218-221 wrapping division_algorithm.go:76-78; arg = available */
  KP_ERR_SCALE_DOWN_NOT_ENOUGH = 11, /* assignment.go:228-231; arg = available */
  KP_ERR_SCALE_UP_NOT_ENOUGH = 12,   /* assignment.go:236-239; arg = available */
  KP_ERR_UNDEFINED_STRATEGY = 13,    /* division_algorithm.go:97-99 */
  KP_ERR_RESULT_CAPACITY = 14,       /* engine limit, no reference site: a serial result list
                                        outgrew the batch's result pool (arg = its length);
                                        never expected, reported instead of written */
  KP_ERR_SETS_CAPACITY = 15,         /* engine limit, no reference site: the binding's
                                        MaxAvailableComponentSets simulation needed more than
                                        the device's node runs in one cluster (arg = the
                                        cluster's caller index); only that binding fails */
  KP_ERR_OVERFLOW_TERMS = 16         /* engine limit, no reference site: the observed
                                        ClusterAffinities term plus its overflow affinities
                                        number more than 63, the orders the sortClusters key
                                        holds (getClusterOverflowOrder, common.go:156-170,
                                        takes any number); arg = that count */
};

/* Per-batch results, engine-owned, valid until the next call on the engine.
 * Targets of binding b are entries [offsets[b], offsets[b+1]) of cluster_idx /
 * replicas; cluster_idx indexes the caller's cluster array given to
 * kp_snapshot_create. Order inside one binding follows the reference where it
 * is deterministic; compare as a multiset (test/helper/scheduler.go:26-40). */
typedef struct kp_results {
  uint64_t n_bindings;
  const int32_t* status;   /* KP_STATUS_* */
  const int32_t* err_code; /* KP_ERR_* */
  const int64_t* err_arg;
  const uint64_t* offsets; /* n_bindings + 1 */
  const uint32_t* cluster_idx;
  const int32_t* replicas;
  uint64_t n_targets;
} kp_results;

/* The packed form of kp_results (kp_schedule_batch_packed): 4 bytes per target where
 * kp_results has 8, for a caller that walks the result once. n_bindings, status,
 * err_code, err_arg, offsets and n_targets hold exactly what kp_results holds for the
 * same call, and entry i of `targets` is entry i of cluster_idx / replicas:
 *   bits [15:0]  the caller's cluster index (a batch never has more than 65 536 clusters);
 *   bits [31:16] the replicas, or 0xFFFF when they lie outside 0..65534 (negative values
 *                and 65535 itself included): the entry is then "escaped".
 * The escaped entries' replicas stand in wide_replicas in entry order: the k-th 0xFFFF
 * entry of `targets` takes wide_replicas[k]. The escaped entries of binding b are
 * wide_replicas[wide_offsets[b] .. wide_offsets[b+1]), so one binding decodes from
 * offsets[b] and wide_offsets[b] alone; wide_offsets (n_bindings + 1) may be NULL when
 * n_wide == 0. kp_results_unpack is the decoder's definition. Engine-owned, valid until
 * the next call on the engine, as kp_results. */
typedef struct kp_results_packed {
  uint64_t n_bindings;
  const int32_t* status;
  const int32_t* err_code;
  const int64_t* err_arg;
  const uint64_t* offsets; /* n_bindings + 1 */
  const uint32_t* targets; /* n_targets packed words */
  uint64_t n_targets;
  const int32_t* wide_replicas; /* n_wide escaped replicas, entry order */
  uint64_t n_wide;
  const uint64_t* wide_offsets; /* n_bindings + 1, or NULL when n_wide == 0 */
} kp_results_packed;

/* The delta form of kp_results (kp_schedule_batch_delta): the targets of the bindings whose
 * placement the call CHANGED, compared on the device with the spec.Clusters the binding was
 * packed with. It is what patchScheduleResultForResourceBinding (pkg/scheduler/
 * scheduler.go:686-718) needs: a patch for the changed bindings, nothing for the others.
 * For binding b of the batch, after the call:
 *   - status[b] != KP_STATUS_OK: b is never listed as changed. It has no targets in any
 *     form; the caller acts on the status, which is returned for every binding.
 *   - status[b] == KP_STATUS_OK: b is UNCHANGED exactly when its result equals spec.Clusters
 *     as a multiset of (cluster, replicas) pairs, where spec.Clusters means all n_clusters
 *     entries the caller passed: the comparison of helper.IsScheduleResultEqual
 *     (test/helper/scheduler.go:26-40). So
 *       . a spec.Clusters name the snapshot does not hold makes the binding changed;
 *       . a repeated name makes it changed (a result never repeats a cluster, so lists of
 *         equal size cannot match);
 *       . an empty result against an empty spec.Clusters is unchanged;
 *       . replicas compare as full int32: negative and wrapped values and the
 *         zero-replica entries of enable_empty_workload_propagation included. No replicas
 *         value serves as an "absent" sentinel.
 * One deliberate difference from the reference: its merge patch compares the list in
 * order, so a result that only reorders spec.Clusters is patched there and is reported
 * unchanged here. The two states are equal under the reference's own result equality, and
 * the engine's entry order is the reference's only where that is deterministic (kp_results).
 *
 * status, err_code and err_arg (n_bindings each) are byte for byte what kp_schedule_batch
 * returns for the same batch. changed holds the n_changed changed bindings' batch indices,
 * ascending; the targets of changed[i] are entries [offsets[i], offsets[i+1]) of
 * cluster_idx / replicas, in the entry order and with the caller's cluster indices of
 * kp_results. n_targets = offsets[n_changed]; n_targets_all = what kp_results.n_targets
 * would have been. Nothing but the three status arrays is sized by n_bindings. Engine-owned,
 * valid until the next call on the engine, as kp_results. */
typedef struct kp_results_delta {
  uint64_t n_bindings;
  const int32_t* status;    /* n_bindings, as kp_results */
  const int32_t* err_code;
  const int64_t* err_arg;
  uint64_t n_changed;
  const uint32_t* changed;  /* n_changed batch indices, ascending */
  const uint64_t* offsets;  /* n_changed + 1: CSR over the changed bindings only */
  const uint32_t* cluster_idx;
  const int32_t* replicas;
  uint64_t n_targets;       /* targets of the changed bindings */
  uint64_t n_targets_all;   /* what kp_results.n_targets would have been */
} kp_results_delta;

/* Results of kp_schedule_affinities, engine-owned like kp_results. `results` holds
 * each binding's final Schedule outcome: the first successful term's targets, or,
 * when every term failed, the FIRST term's error class/code/arg with no targets
 * (scheduler.go:657-673). affinity_index[b] = the ClusterAffinities index that
 * succeeded (its AffinityName becomes Status.SchedulerObservedAffinityName,
 * scheduler.go:676-678), or -1 when the observed name stays as it was (all terms
 * failed, or the binding has no ClusterAffinities). attempts[b] = Schedule calls
 * made for binding b. rounds = batched passes run (1 + the largest retry depth). */
typedef struct kp_affinity_results {
  kp_results results;
  const int32_t* affinity_index;
  const int32_t* attempts;
  uint32_t rounds;
} kp_affinity_results;

/* Per-stage timing of the last kp_schedule_batch call (milliseconds, host clock
 * around device work; kernel-only numbers come from rocprof). */
typedef struct kp_stage_times {
  double pair_ms;      /* filter + estimate stage: k_est_class + k_filter, or the pair kernel */
  double select_ms;    /* candidate/group/select/divide kernels after the filter stage */
  double host_ms;      /* host group-combination (region DFS) */
  double copy_ms;      /* device -> host result copies */
  double total_ms;
  float pair_kernel_ms;   /* filter + estimate stage kernels (HIP events) */
  float select_kernel_ms; /* select kernels after the filter stage (HIP events) */
  uint64_t n_slow;        /* bindings that took the exact serial path */
  uint32_t pair_launches; /* filter-stage kernel launches (2: k_est_class + k_filter, 1: pair kernel) */
  uint32_t pair_kind;     /* estimator instance: 0 generic, 1 mixed, 2 summary-only, 8/16 model-only */
  float filter_kernel_ms; /* k_filter alone (HIP events), 0 with the pair kernel */
  uint32_t bits;          /* 1: bitset filter + estimator-class rows; 0: per-binding pair rows */
  float sel_all_kernel_ms; /* the two-kernel path's SEL_ALL select kernel alone (HIP events) */
  uint32_t n_sel_all;      /* bindings of the SEL_ALL select kernel (SelectBestClusters selects all) */
  uint32_t n_classes;      /* estimator-class rows computed (bits == 1; row 0 = non-workload) */
  uint32_t n_top;          /* SEL_ALL bindings given to k_select_top (deciding-candidate subsets) */
  uint32_t n_top_fallback; /* of those, the ones it handed to the full-candidate kernel */
  float top_kernel_ms;     /* k_select_top alone (HIP events on its stream), 0 when it did not run */
  uint32_t n_cluster;       /* cluster-spread bindings (selectBestClustersByCluster) */
  uint32_t n_cluster_order; /* of those, the ones selected over their estimator-class order */
  float cluster_kernel_ms;  /* the cluster-spread select kernel alone (HIP events on its stream) */
  uint32_t n_region;        /* region-spread bindings (selectBestClustersByRegion) */
  uint32_t n_region_order;  /* of those, the ones whose final selection walked their estimator-class order */
  uint32_t n_region_wide;   /* of those, the ones k_region_wide scheduled or errored: a selection of more than
                               256 clusters, or a repeated spec.Clusters of more than 256 entries */
} kp_stage_times;

/* ------------------------------------------------------------------------- */
/* Entry points                                                              */
/* ------------------------------------------------------------------------- */

typedef struct kp_engine kp_engine;
typedef struct kp_snapshot kp_snapshot;
typedef struct kp_batch kp_batch;

enum {
  KP_OK = 0,
  KP_EINVAL = -1,
  KP_ENOMEM = -2,
  KP_EDEVICE = -3,
  KP_ENOTSUP = -4,
  KP_ESTATE = -5
};

int kp_abi_version(void);

/* Creates an engine bound to HIP device `device` (one HIP stream). */
int kp_engine_create(int device, kp_engine** out);
void kp_engine_destroy(kp_engine* e);
const char* kp_last_error(const kp_engine* e);

/* Packs a cluster list (cache.Snapshot) into the device SoA layout and uploads it.
 * Replaces the per-Schedule List+DeepCopy (cache.go:124-139) by one upload.
 * KP_ENOTSUP above 2^18 = 262 144 clusters: that is the bound of the encoding (the rank
 * field of the sort key), not of the engine. A snapshot is usable only up to what
 * kp_batch_create accepts over it, see there: about 18.6k clusters on gfx950. */
int kp_snapshot_create(kp_engine* e, const kp_cluster* clusters, uint64_t n_clusters,
                       const kp_options* opts, kp_snapshot** out);
void kp_snapshot_destroy(kp_snapshot* s);
/* Applies cluster events to a snapshot in place: `clusters` are new versions of
 * clusters already in it (matched by name). Only those rows are re-packed; the
 * device copy is refreshed. This replaces re-snapshotting all clusters on every
 * informer event (cache.go:124-139, event_handler.go:314-378). *dict_grew = 1
 * when the update added names, keys, GVKs or resources to the snapshot's
 * dictionaries or changed its set of regions: batches packed before the call
 * must then be re-created (their compiled selectors resolve strings against the
 * old dictionaries; their region buffers are sized by the region count), and
 * kp_schedule_batch returns KP_ESTATE for a region-spread batch whose region
 * count no longer matches; otherwise they stay valid. Adding or removing
 * clusters needs kp_snapshot_create. */
int kp_snapshot_update(kp_engine* e, kp_snapshot* s, const kp_cluster* clusters, uint64_t n_clusters,
                       int* dict_grew);
/* ---- which bindings a cluster event affects ---------------------------------------------
 * reconcileCluster (pkg/scheduler/event_handler.go:388-397) lists every ResourceBinding and
 * ClusterResourceBinding per cluster object and requeues those whose current affinity matches
 * it (enqueueAffectedBindings / enqueueAffectedCRBs, event_handler.go:400-491). A kp_watch
 * holds, per binding, the compiled selector of the one affinity those loops read;
 * kp_affected_bindings answers for a set of clusters at once, on the device.
 *
 * Binding i of a watch, by mode[i] (mode == NULL: every binding KP_WATCH_MATCH):
 *   KP_WATCH_SKIP    never listed. For the bindings the loops skip: another scheduler's name
 *                    (schedulerNameFilter) or suspended scheduling; kp_binding carries neither.
 *   KP_WATCH_ALWAYS  listed whenever n_clusters > 0. For a ClusterAffinities binding whose
 *                    Status.SchedulerObservedGeneration differs from its Generation
 *                    (event_handler.go:419-426).
 *   KP_WATCH_MATCH   the affinity is cluster_affinities[getAffinityIndex(observed_affinity_name)]
 *                    .affinity when n_cluster_affinities > 0 (tested first, as the reference
 *                    does; index 0 for an empty or unknown name, helper.go:99-110), else
 *                    cluster_affinity when has_cluster_affinity, else nil. Nil: listed.
 *                    Otherwise listed exactly when util.ClusterMatches holds for at least one of
 *                    the listed clusters in the snapshot's current state.
 * Nothing else plays a part: not the term's overflow affinities, tolerations, the GVK, spread
 * constraints, eviction tasks, spec.Clusters, kp_options.enabled_plugins or the cluster's
 * deleting flag (a batch's filter reads all of these, so a kp_batch cannot answer this).
 *
 * The watch remembers its snapshot and the state of the snapshot's dictionaries:
 * kp_affected_bindings returns KP_ESTATE (kp_last_error says why) with another snapshot, and
 * after a kp_snapshot_update on it that reported dict_grew = 1; an update with dict_grew = 0
 * leaves the watch valid. One event batch is: kp_affected_bindings over the old state,
 * kp_snapshot_update, a new watch if dict_grew, kp_affected_bindings over the new state, the
 * union of both lists to the queue (the reference adds the old and the new object,
 * event_handler.go:351-352, and the queue dedups).
 * n_bindings must be below 2^31 (KP_EINVAL). Nothing of `bindings` is retained. */
typedef struct kp_watch kp_watch;
enum { KP_WATCH_MATCH = 0, KP_WATCH_ALWAYS = 1, KP_WATCH_SKIP = 2 };
/* mode may be NULL (all KP_WATCH_MATCH). */
int kp_watch_create(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings, uint64_t n_bindings,
                    const uint8_t* mode, kp_watch** out);
void kp_watch_destroy(kp_watch* w);
typedef struct kp_affected {
  uint64_t n;
  const uint32_t* bindings; /* ascending, distinct; engine-owned until the next call on the engine */
} kp_affected;
/* The watch's bindings that the clusters cluster_idx[0, n_clusters) affect (caller indices as
 * given to kp_snapshot_create; repeats allowed). KP_EINVAL for an index at or beyond the
 * snapshot's cluster count and for a null pointer; n_clusters == 0 gives an empty list and
 * launches nothing. Under kp_engine_set_profile the call's launches are what
 * kp_last_kernel_times reports. */
int kp_affected_bindings(kp_engine* e, const kp_watch* w, const kp_snapshot* s, const uint32_t* cluster_idx,
                         uint64_t n_clusters, kp_affected* out);

/* Packed snapshot as one relocatable byte image (for RCCL broadcast) and back. */
int kp_snapshot_export(const kp_snapshot* s, const void** bytes, uint64_t* n_bytes);
int kp_snapshot_import(kp_engine* e, const void* bytes, uint64_t n_bytes, kp_snapshot** out);

/* Packs a batch of bindings against a snapshot and uploads them to HBM.
 * KP_ENOTSUP ("snapshot too large for one workgroup's LDS") when a selection kernel's
 * working set over the snapshot does not fit one workgroup's LDS; the schedule calls
 * check again (a kp_snapshot_update can change the region and template counts). The
 * kernels gather 8 B per cluster, 10 B in the region-spread stages, beside 12-19 KB of
 * fixed lists, so with gfx950's 163 840 B per workgroup the ceiling is 18 624 clusters
 * (about 18.6k) for a batch without spread bindings and 14 336 (about 14.3k) for one
 * with cluster or region spread bindings (at 16 regions; every further region takes 12 B).
 * The cluster count rounds up to 64, so the next accepted step is 64 clusters lower. */
int kp_batch_create(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings,
                    uint64_t n_bindings, kp_batch** out);
void kp_batch_destroy(kp_batch* b);

/* ---- packed-record reuse across scheduling cycles --------------------------------
 * The scheduler re-runs Schedule for bindings whose spec did not change: Duplicated and
 * non-workload bindings on every reconcile, bindings with terminating target clusters,
 * requeued failures (pkg/scheduler/scheduler.go:437-468); a changed spec moves
 * metadata.generation. A kp_pack_cache keeps each binding's packed record (its binding
 * header and pool slices, snapshot ids resolved) keyed by (metadata.uid,
 * metadata.generation), and kp_batch_create_keyed copies a record instead of re-packing
 * the binding when the key matches and so do the status fields the record depends on
 * (status.schedulerObservedAffinityName, spec.rescheduleTriggeredAt,
 * status.lastScheduledTime, compared field by field). Records are tied to the snapshot's
 * dictionaries: a different snapshot, or a kp_snapshot_update that grew them
 * (dict_grew = 1), empties the cache. The batch is byte-for-byte the one
 * kp_batch_create packs from the same bindings. A cache is used by one call at a time. */
typedef struct kp_pack_cache kp_pack_cache;
typedef struct kp_binding_key {
  kp_str uid;         /* metadata.uid */
  int64_t generation; /* metadata.generation */
} kp_binding_key;
typedef struct kp_pack_cache_stats {
  uint64_t hits, misses; /* over the cache's lifetime */
  uint64_t entries;      /* records held */
  uint64_t last_hits;    /* of the last kp_batch_create_keyed */
} kp_pack_cache_stats;
/* max_entries: records kept (0: 4M); past it the cache is emptied before the next batch. */
int kp_pack_cache_create(uint64_t max_entries, kp_pack_cache** out);
void kp_pack_cache_destroy(kp_pack_cache* c);
int kp_pack_cache_get_stats(const kp_pack_cache* c, kp_pack_cache_stats* out);
/* Diagnostic: a 64-bit digest of a batch's packed host image (binding headers, pools,
 * routes, and each binding's estimator class as its first binding), equal for two
 * batches exactly when they pack the same records (the tests compare keyed and fresh). */
int kp_batch_digest(const kp_batch* b, uint64_t* out);
/* kp_batch_create with keys[i] for bindings[i] (keys[i].uid empty: never cached). */
int kp_batch_create_keyed(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings,
                          const kp_binding_key* keys, uint64_t n_bindings, kp_pack_cache* cache,
                          kp_batch** out);

/* ---- the other ReplicaEstimators' answers ------------------------------------------
 * calAvailableReplicas (pkg/scheduler/core/util.go:57-110) asks every registered
 * ReplicaEstimator and keeps, per cluster, the minimum of the answers that are not
 * UnauthenticReplica (-1) (mergeReplicaResults, util.go:157-170); only then does a leftover
 * MaxInt32 become spec.Replicas. The multi-template path merges the same way
 * (core/estimation.go:77-113). The engine computes the GeneralEstimator; with
 * --enable-scheduler-estimator the caller hands in what the scheduler-estimator client
 * answered.
 *
 * kp_estimates: the answers of the estimators other than the GeneralEstimator, already
 * merged by the caller into one row per distinct request (min over those estimators of the
 * answers that are not -1; -1 where none answered). Nothing is retained after the call. */
typedef struct kp_estimates {
  uint32_t n_rows;
  uint64_t n_clusters;   /* must equal the snapshot's cluster count */
  const int32_t* rows;   /* n_rows * n_clusters, caller cluster order; -1 = UnauthenticReplica */
  const int32_t* row_of; /* n_bindings entries: the binding's row, or -1 for none */
} kp_estimates;
/* kp_batch_create (keys and cache NULL) or kp_batch_create_keyed (both given) with
 * estimates. A binding with row r schedules over min(general(c), rows[r][c]) where
 * rows[r][c] != -1 and over general(c) elsewhere, MaxInt32 then becoming spec.Replicas; a
 * binding that takes MaxAvailableComponentSets (gate on, cluster spread [1,1]) is merged
 * the same way; a non-workload binding (replicas == 0, no components) calls no estimator
 * (util.go:69-73) and ignores its row. Every schedule call on the batch uses the rows
 * (kp_schedule_batch, _submit / _collect and the packed forms). A binding's estimator class
 * is (request, row): a packed record (kp_pack_cache) keeps the request alone, so the keys'
 * records are reused from cycle to cycle while the rows change. est == NULL or n_rows == 0:
 * the batch is byte for byte the one kp_batch_create / _keyed makes (equal
 * kp_batch_digest). KP_EINVAL (kp_last_error says which) when n_clusters differs from the
 * snapshot's cluster count, a row_of entry is outside -1..n_rows-1, or a row value is
 * below -1.
 * The per-pair entry points on such a batch (kp_max_available_replicas, kp_filter_*,
 * kp_score_batch) keep answering for the in-tree set only: kp_max_available_replicas is
 * the GeneralEstimator's answer, not the merged one. kp_schedule_affinities takes estimates
 * through kp_schedule_affinities_ex; kp_multi_* does not take them. */
int kp_batch_create_estimates(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings,
                              const kp_binding_key* keys /* may be NULL */, uint64_t n_bindings,
                              kp_pack_cache* cache /* may be NULL */, const kp_estimates* est /* may be NULL */,
                              kp_batch** out);

/* ---- out-of-tree filter plugins' verdicts ---------------------------------------------
 * RunFilterPlugins (runtime/framework.go:93-105) is an AND over every registered filter
 * plugin, and a plugin's verdict is per (binding, cluster). The engine computes the in-tree
 * set; a scheduler that registers filter plugins of its own (app.WithPlugin) hands in their
 * verdicts. Score plugins do not qualify: NormalizeScore runs over the
 * feasible set, which is not known before the filter has run.
 *
 * kp_filter_answers: the out-of-tree filter plugins' verdicts, already ANDed by the caller
 * into one row per distinct binding class. Nothing is retained after the call. */
typedef struct kp_filter_answers {
  uint32_t n_rows;
  uint64_t n_clusters;   /* must equal the snapshot's cluster count */
  const uint64_t* rows;  /* n_rows * ceil(n_clusters/64) words, caller cluster order, the layout
                            of kp_filter_batch's out_mask: bit set = every out-of-tree filter
                            plugin returned Success for this cluster */
  const int32_t* row_of; /* n_bindings entries: the binding's row, or -1 (no plugin objected) */
  uint32_t n_plugins;    /* how many registered out-of-tree plugins the rows fold in; the caller
                            attests that all of them are filter-only (no Score) */
} kp_filter_answers;
/* kp_batch_create_estimates with filter answers. Cluster c is feasible for binding b iff the
 * in-tree filter set passes it and bit c of b's row is set (a cluster named in spec.Clusters
 * included); everything downstream (the FitError when nothing fits, locality, scale-down,
 * spread, division) runs over that set. The schedule calls on the batch (kp_schedule_batch,
 * _submit / _collect and the packed forms) run when flt->n_plugins equals the snapshot's
 * n_out_of_tree_plugins (a batch without answers counts as 0) and return KP_ENOTSUP
 * otherwise. kp_filter_batch returns the merged mask; kp_filter_reasons reports the in-tree
 * reason where there is one and KP_REASON_OUT_OF_TREE where the in-tree set fits and the row
 * rejects; kp_score_batch and kp_max_available_replicas are unchanged. The rows are not part
 * of a binding's packed record or estimator class: a keyed batch reuses every record while
 * the rows change. flt == NULL or n_rows == 0: the batch is byte for byte the one
 * kp_batch_create_estimates makes (equal kp_batch_digest) and nothing new is allocated,
 * uploaded or launched for it (a non-NULL flt with n_rows == 0 still states its n_plugins for
 * the gate: plugins registered, none objected). Bits at or above n_clusters in a row's last word are ignored.
 * KP_EINVAL (kp_last_error says which) when n_clusters differs from the snapshot's cluster
 * count, rows is null, row_of is null with n_bindings > 0, a row_of entry is outside
 * -1..n_rows-1, or n_rows > 0 with n_plugins == 0. kp_schedule_affinities takes answers
 * through kp_schedule_affinities_ex; kp_multi_* takes none. */
int kp_batch_create_filters(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings,
                            const kp_binding_key* keys /* may be NULL */, uint64_t n_bindings,
                            kp_pack_cache* cache /* may be NULL */, const kp_estimates* est /* may be NULL */,
                            const kp_filter_answers* flt /* may be NULL */, kp_batch** out);

/* ---- the scheduler's assumed workloads (SchedulingOvercommitProtection) -------------------
 * With the gate on, the scheduler records every patched placement's footprint per cluster
 * (updateAssumptionsCache, pkg/scheduler/scheduler.go:720-779) and every later Schedule call
 * hands those footprints to the estimators as AssumedWorkloads (calAvailableReplicas,
 * core/util.go:78-93; buildAssumedWorkloadsByCluster, core/estimation.go:115-139). The
 * GeneralEstimator deducts them: pods and per-resource demand added to the summary's
 * Allocating (deductAssumedWorkloadsFromSummary, estimator/client/general.go:110-151) and,
 * on the model path, each workload placed first-fit over the model-grade nodes with
 * SimulateScheduling(components, 1) before the request is counted (general.go:507-553).
 * For one Schedule call the map is a constant input, as the snapshot is: a kp_assumptions
 * deducts it once per cluster on the device, and a batch made over it answers over the
 * deducted availability.
 *
 * kp_assumed_entry: one AssumedWorkload of one cluster. The entries of one cluster are
 * deducted in the order given (the reference's order is a Go map iteration,
 * GetAssumedWorkloads, cache.go:287: pass the list as it came, parity holds for that order);
 * entries of different clusters may interleave. Nothing is retained after the call. */
typedef struct kp_assumed_entry {
  uint32_t cluster;             /* caller's cluster index (kp_snapshot_create order) */
  const kp_component* components; /* Replicas + ResourceRequest; no NodeClaim: model nodes carry no
                                     Node object, every one matches
                                     (scheduling_simulator_components.go:149-153) */
  uint32_t n_components;
} kp_assumed_entry;
typedef struct kp_assumptions kp_assumptions;
/* n == 0 succeeds (the gate off: an empty map). KP_EINVAL for a cluster index at or beyond
 * the snapshot's count, negative replicas and an unparsable quantity; KP_ENOTSUP for more
 * than 16 components in one workload, a negative quantity, a cluster whose summed demand of
 * one resource (or of pods) leaves int64, and a cluster whose residual model nodes need more
 * node runs than min(its model node count, 4096); kp_last_error names the entry or cluster.
 * The deduction is that of the snapshot's state at this call: after a kp_snapshot_update,
 * kp_batch_create_assumed and the schedule calls of its batches return KP_ESTATE. */
int kp_assumptions_create(kp_engine* e, const kp_snapshot* s, const kp_assumed_entry* entries, uint64_t n,
                          kp_assumptions** out);
/* Batches made over it keep what they need: it may be destroyed before them. */
void kp_assumptions_destroy(kp_assumptions* a);
/* kp_batch_create over the deducted availability: kp_schedule_batch, its _submit / _collect,
 * _packed and _delta forms and kp_max_available_replicas answer with, at every cluster that
 * has entries, the GeneralEstimator's answer over the deducted summary and model nodes (the
 * value replaces the undeducted one; clusters without entries are untouched); filter, score
 * and reasons do not change. a == NULL or made with n == 0: in every respect a
 * kp_batch_create batch (nothing allocated, launched or waited for). KP_ENOTSUP for a
 * binding that takes MaxAvailableComponentSets (multiple_pod_templates_scheduling on and
 * isMultiTemplateSchedulingApplicable). Assumptions do not combine with
 * kp_batch_create_estimates / _filters / _keyed, kp_schedule_affinities* or kp_multi_*:
 * none of them takes a kp_assumptions. */
int kp_batch_create_assumed(kp_engine* e, const kp_snapshot* s, const kp_assumptions* a, const kp_binding* bindings,
                            uint64_t n, kp_batch** out);

/* genericScheduler.Schedule for every binding of the batch. */
int kp_schedule_batch(kp_engine* e, kp_batch* b, kp_results* out);
/* kp_schedule_batch in two halves, for a caller that keeps batches in flight (a scheduler
 * draining its queue): _submit queues the batch's kernels and per-binding read-backs on the
 * engine's stream (it waits only where the region chain's host step does) and returns;
 * _collect waits for them, copies the CSR back and fills *out exactly as kp_schedule_batch
 * does. A batch holds one submitted call at a time (KP_ESTATE otherwise); an engine may hold
 * several submitted batches, collected in any order. Submitting the next batch before
 * collecting the last keeps the GPU queue fed while the host reads results back. Not with
 * kp_engine_set_profile (KP_EINVAL). */
int kp_schedule_batch_submit(kp_engine* e, kp_batch* b);
int kp_schedule_batch_collect(kp_engine* e, kp_batch* b, kp_results* out);

/* kp_schedule_batch with the results in the packed form (kp_results_packed): the same
 * kernels, then the result gathered as one packed word per target plus the escaped
 * replicas, so half the bytes cross the bus unless most entries are escaped.
 * _submit_packed / _collect_packed are the two halves with the contract of
 * kp_schedule_batch_submit / _collect: one submitted call per batch in either format
 * (KP_ESTATE on a second submit, or on a collect with nothing submitted; KP_EINVAL with
 * kp_engine_set_profile). A submitted call is collected by its own format's function:
 * the other one returns KP_ESTATE and leaves the call collectable. A batch may be
 * scheduled in either format from call to call. KP_ENOTSUP for a snapshot of more than
 * 65 536 clusters (the bound of the 16-bit index field; kp_batch_create's LDS ceiling is
 * lower, so no batch reaches it). */
int kp_schedule_batch_packed(kp_engine* e, kp_batch* b, kp_results_packed* out);
int kp_schedule_batch_submit_packed(kp_engine* e, kp_batch* b);
int kp_schedule_batch_collect_packed(kp_engine* e, kp_batch* b, kp_results_packed* out);
/* Expands packed results into caller-provided arrays of in->n_targets entries each, the
 * cluster_idx / replicas of kp_results. Plain host code: no engine, no device. */
int kp_results_unpack(const kp_results_packed* in, uint32_t* cluster_idx, int32_t* replicas);

/* kp_schedule_batch with the results in the delta form (kp_results_delta): the same
 * kernels, then each binding's result compared with its spec.Clusters on the device, and
 * only the changed bindings' indices and targets copied back. Batches of every
 * kp_batch_create* variant schedule in this form, their estimator and filter rows honoured
 * (and the out-of-tree plugin gate applied) as by kp_schedule_batch.
 * _submit_delta / _collect_delta are the two halves with the contract of the packed ones:
 * one submitted call per batch across the three formats (KP_ESTATE on a second submit, or
 * on a collect with nothing submitted; KP_EINVAL from either half while
 * kp_engine_set_profile is on, a submitted call staying collectable for later), a submitted
 * call is collected by its own format's function (another's returns KP_ESTATE and leaves
 * the call collectable), and a batch may change format from call to call. A completed
 * delta call is a completed schedule call for kp_fit_diagnosis_batch(bindings == NULL).
 * kp_schedule_affinities* and kp_multi_* have no delta form. */
int kp_schedule_batch_delta(kp_engine* e, kp_batch* b, kp_results_delta* out);
int kp_schedule_batch_submit_delta(kp_engine* e, kp_batch* b);
int kp_schedule_batch_collect_delta(kp_engine* e, kp_batch* b, kp_results_delta* out);

/* Scheduler.scheduleResourceBindingWithClusterAffinities (scheduler.go:618-684),
 * batched: bindings with n_cluster_affinities > 0 start at getAffinityIndex of their
 * observed name (helper.go:99-110; index 0 when util.RescheduleRequired), and every
 * binding whose term failed is re-packed with the next term's name and scheduled
 * again in the next round, all failing bindings of a round in one batch. Bindings
 * without ClusterAffinities run once (scheduleResourceBinding, scheduler.go:584-600). */
int kp_schedule_affinities(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings, uint64_t n_bindings,
                           kp_affinity_results* out);

/* The estimators' answers and the out-of-tree filter plugins' verdicts for the retry loop.
 * An estimator reads the request, not the term, so est->row_of has one entry per binding as
 * in kp_batch_create_estimates. A filter plugin sees the spec with the current term's
 * affinity substituted (scheduler.go:630-640), so its verdict may differ from term to term:
 * flt->row_of has one entry per (binding, term), found through term_off. */
typedef struct kp_affinity_answers {
  const kp_estimates* est;      /* may be NULL; row_of has n_bindings entries */
  const kp_filter_answers* flt; /* may be NULL; rows / n_rows / n_clusters / n_plugins as in
                                   kp_batch_create_filters, row_of per (binding, term) */
  const uint64_t* term_off;     /* n_bindings + 1 entries when flt has rows: binding i's verdict rows are
                                   flt->row_of[term_off[i] + t], t = 0 .. max(1, n_cluster_affinities) - 1 */
} kp_affinity_answers;
/* kp_schedule_affinities with answers: every round's batch merges them as a
 * kp_batch_create_filters batch does, a binding's verdict row being that of the term it is
 * trying. The error kept when every term fails is that of the first attempted term as the
 * answered batch reports it: a FitError where the row rejects what the in-tree set passes,
 * KP_ERR_* with the capacity the estimates reduce. The rows are uploaded once per call and
 * brought into cluster rank order on the device; each round's batch borrows them. The call
 * runs when (flt ? flt->n_plugins : 0) equals the snapshot's n_out_of_tree_plugins (a flt
 * with n_rows == 0 still states its n_plugins) and returns KP_ENOTSUP otherwise. ans == NULL,
 * answers without rows and row_of entries all -1 give kp_schedule_affinities' results, and
 * nothing is allocated, uploaded or launched for them. KP_EINVAL (kp_last_error says which)
 * under the rules of kp_batch_create_estimates and kp_batch_create_filters, and when flt has
 * rows and term_off is null, is not non-decreasing, or term_off[i + 1] - term_off[i] differs
 * from max(1, n_cluster_affinities) of binding i. Nothing is retained after the call. */
int kp_schedule_affinities_ex(kp_engine* e, const kp_snapshot* s, const kp_binding* bindings, uint64_t n_bindings,
                              const kp_affinity_answers* ans /* may be NULL */, kp_affinity_results* out);

/* FilterPlugin boundary: feasibility of every (binding, cluster) pair after
 * RunFilterPlugins (+ the skip-deleting rule of findClustersThatFit).
 * out_mask: n_bindings * ceil(n_clusters/64) words, bit c%64 of word c/64 set
 * when cluster c (caller order) fits. */
int kp_filter_batch(kp_engine* e, kp_batch* b, uint64_t* out_mask);

/* FitError diagnosis (framework/types.go:56-90; findClustersThatFit,
 * generic_scheduler.go:119-163): per pair the Result of RunFilterPlugins
 * (runtime/framework.go:93-105, plugins in canonical order), n_bindings*n_clusters
 * words in caller cluster order: bits [7:0] = KP_REASON_*, bits [31:8] = argument.
 * KP_REASON_FIT pairs fit; KP_REASON_DELETING clusters are skipped before the
 * plugins run and are absent from Diagnosis.ClusterToResultMap. The argument of
 * KP_REASON_TAINT is the index of the untolerated taint among the cluster's
 * NoSchedule/NoExecute taints in spec.taints order (FindMatchingUntoleratedTaint);
 * 0 otherwise. */
enum {
  KP_REASON_FIT = 0,
  KP_REASON_API = 1,             /* api_enablement.go:77 "cluster(s) did not have the API resource" */
  KP_REASON_TAINT = 2,           /* taint_toleration.go:83 "cluster(s) had untolerated taint {%s}" */
  KP_REASON_AFFINITY = 3,        /* cluster_affinity.go:89 "...did not match the placement cluster affinity constraint" */
  KP_REASON_SPREAD_PROVIDER = 4, /* spread_constraint.go:57 "cluster(s) did not have provider property" */
  KP_REASON_SPREAD_REGION = 5,   /* spread_constraint.go:59 "cluster(s) did not have region property" */
  KP_REASON_SPREAD_ZONES = 6,    /* spread_constraint.go:61 "cluster(s) did not have zones property" */
  KP_REASON_EVICTION = 7,        /* cluster_eviction.go:53 "cluster(s) is in the process of eviction" */
  KP_REASON_OUT_OF_TREE = 8,     /* the in-tree set fits, the batch's kp_filter_answers row rejects (the
                                    plugin's own message is the caller's; the registry's plugin order is a
                                    map iteration, so "in-tree first" is as faithful as any) */
  KP_REASON_DELETING = 255       /* generic_scheduler.go:138-142 (skipped) */
};
int kp_filter_reasons(kp_engine* e, kp_batch* b, uint32_t* out_reasons);

/* FitError diagnosis of a batch's failed bindings at batch cost: FitError.Error()
 * (framework/types.go:73-89) never looks at pairs, it counts clusters per distinct reason
 * string, so this call returns that histogram per binding instead of kp_filter_reasons'
 * n_bindings*n_clusters words. A bin is one distinct reason string of the reference:
 * KP_REASON_API and KP_REASON_AFFINITY .. KP_REASON_OUT_OF_TREE are one bin each;
 * KP_REASON_TAINT is one bin per distinct taint text, i.e. per (key, value, effect) of the
 * cluster's first untolerated NoSchedule/NoExecute taint (the taint kp_filter_reasons'
 * argument indexes). Within a binding the bins are ordered by reason code, then taint_ref;
 * empty bins are absent. Per binding n_fit + n_deleting + the sum of its counts = n_clusters.
 *
 * taint_ref names a taint the caller can print: a caller cluster index in bits [17:0] and
 * above them the index of the taint among that cluster's NoSchedule/NoExecute taints (the
 * encoding of kp_filter_reasons' argument). The cluster is the snapshot-wide representative
 * of the triple, the lowest caller cluster index that carries it (with its first position
 * there), fixed when the snapshot is created, updated or imported; it need not be a cluster
 * this binding rejected.
 *
 * bindings != NULL: exactly those n batch indices, strictly ascending and below the batch
 * size (KP_EINVAL otherwise). bindings == NULL (n ignored): the bindings whose status was
 * KP_STATUS_FIT_ERROR in the batch's last completed schedule call, plain or packed, one
 * call or submit + collect; KP_ESTATE when there is none, or while a submitted call is not
 * collected. The arrays belong to the engine and stay valid until the next call on it.
 * enabled_plugins and a kp_batch_create_filters batch's rows are honoured as by
 * kp_filter_reasons, and like it the call is not refused for n_out_of_tree_plugins > 0. */
typedef struct kp_fit_diagnosis {
  uint64_t n_bindings;          /* bindings diagnosed */
  const uint64_t* binding;      /* n_bindings: index in the batch, ascending */
  const uint64_t* offsets;      /* n_bindings + 1: CSR into the three arrays below */
  const uint32_t* reason;       /* KP_REASON_* (1..8; never FIT or DELETING) */
  const uint32_t* taint_ref;    /* KP_REASON_TAINT: (caller cluster index) | (taint index << 18); else 0 */
  const uint32_t* count;        /* clusters in this bin, > 0 */
  const uint32_t* n_fit;        /* n_bindings: clusters that pass every filter */
  const uint32_t* n_deleting;   /* n_bindings: clusters skipped as deleting */
  uint64_t n_bins;
} kp_fit_diagnosis;
int kp_fit_diagnosis_batch(kp_engine* e, kp_batch* b, const uint64_t* bindings /* may be NULL */, uint64_t n,
                           kp_fit_diagnosis* out);

/* ScorePlugin boundary: summed score (RunScorePlugins) per pair; n_bindings*n_clusters. */
int kp_score_batch(kp_engine* e, kp_batch* b, int64_t* out_scores);

/* ReplicaEstimator boundary (GeneralEstimator.MaxAvailableReplicas): for binding
 * `binding` of the batch and the given caller cluster indices, writes the
 * estimator answer per cluster in input order (general.go:57-64). */
int kp_max_available_replicas(kp_engine* e, kp_batch* b, uint64_t binding,
                              const uint32_t* cluster_idx, uint64_t n, int32_t* out);

/* ReplicaEstimator.MaxAvailableComponentSets for the GeneralEstimator
 * (estimator/client/general.go:154-292): for one component list (one set = every
 * component's Replicas), the number of complete sets each cluster cluster_idx[i]
 * (caller order) holds, written to out[i]: the pod and resource-summary bounds
 * (quantityAsInt64 by each Quantity's format), then, with the
 * CustomizedClusterResourceModeling gate and models, the first-fit simulation over
 * the model-grade nodes (SchedulingSimulator.SimulateScheduling,
 * scheduling_simulator_components.go:51-131). Assumed workloads are empty
 * (kp_assumptions serve the single-template path only). KP_ENOTSUP when the snapshot's options
 * have the MultiplePodTemplatesScheduling gate off (the scheduler then never calls
 * it, core/util.go:113-118), or when a cluster's simulation exceeds the device
 * run capacity (kp_last_error says which). */
int kp_max_available_component_sets(kp_engine* e, const kp_snapshot* s, const kp_component* components,
                                    uint32_t n_components, const uint32_t* cluster_idx, uint64_t n, int32_t* out);

/* ---- member-cluster nodes ------------------------------------
 * A member cluster's node as the cluster status controller and the estimator
 * server see it: corev1.Node plus the non-terminal pods bound to it. `requested`
 * is their summed effective requests (util.Resource.AddPodRequest: cpu, memory,
 * ephemeral-storage and scalar resources), n_pods their count. */
typedef struct kp_node {
  kp_str name;
  const kp_label* labels;
  uint32_t n_labels;
  const kp_taint* taints;
  uint32_t n_taints;
  int32_t unschedulable; /* node.Spec.Unschedulable */
  const kp_resource* allocatable; /* node.Status.Allocatable */
  uint32_t n_allocatable;
  const kp_resource* requested;
  uint32_t n_requested;
  uint32_t n_pods;
} kp_node;

/* The resource-model grade histogram of a cluster: getAllocatableModelings
 * (controllers/status/cluster_status_controller.go:642-677) over
 * modeling.InitSummary / AddToResourceSummary (pkg/modeling/modeling.go:75-223).
 * Each node's available resources (getNodeAvailable, :613-639; the walk stops at
 * the first node with no pod room, as the reference's `break` does) go to the grade
 * getIndex picks (searchLastLessElement per resource name, the minimum over names);
 * out_counts[k] = AllocatableModeling.Count of models[k]. KP_EINVAL for
 * InitSummary's error and for models without ranges. Replaces the Go function
 * getAllocatableModelings. */
int kp_model_grades(kp_engine* e, const kp_resource_model* models, uint32_t n_models, const kp_node* nodes,
                    uint64_t n_nodes, int64_t* out_counts);

/* corev1.NodeSelectorTerm of a required node affinity: MatchExpressions over node
 * labels (In, NotIn, Exists, DoesNotExist, Gt, Lt) and MatchFields over the node's
 * fields (metadata.name; In / NotIn with exactly one value). */
typedef struct kp_node_selector_term {
  const kp_requirement* match_expressions;
  uint32_t n_match_expressions;
  const kp_requirement* match_fields;
  uint32_t n_match_fields;
} kp_node_selector_term;

/* pb.NodeClaim of the estimator request (pkg/estimator/pb): nodeSelector,
 * tolerations and the required node affinity. has_node_affinity != 0 when
 * NodeAffinityBytes decodes to a NodeSelector (pb/helpers.go:40-55); its terms are
 * ORed (nodeaffinity.LazyErrorNodeSelector.Match), a term that fails to parse or is
 * empty never matches, and a selector with no usable term matches no node. */
typedef struct kp_node_claim {
  const kp_label* node_selector;
  uint32_t n_node_selector;
  const kp_toleration* tolerations;
  uint32_t n_tolerations;
  int32_t has_node_affinity;
  const kp_node_selector_term* node_affinity_terms;
  uint32_t n_node_affinity_terms;
} kp_node_claim;

/* pb.Component of an estimator server request: Replicas and ReplicaRequirements
 * (ResourceRequest, NodeClaim). has_replica_requirements == 0: nil requirements
 * (only the pod count is required, every node matches). */
typedef struct kp_node_component {
  int32_t replicas;
  uint8_t has_replica_requirements;
  const kp_resource* resource_request;
  uint32_t n_resource_request;
  const kp_node_claim* node_claim; /* NULL: no NodeClaim */
} kp_node_component;

/* pb.AssumedWorkload: a workload admitted but possibly not yet visible in node
 * accounting, deducted first (one set, SimulateScheduling(components, 1)). */
typedef struct kp_assumed_workload {
  const kp_node_component* components;
  uint32_t n_components;
} kp_assumed_workload;

/* The accurate estimator's per-node path: nodeResourceEstimator.Estimate
 * (estimator/server/framework/plugins/noderesource/noderesource.go:70-131): the
 * assumed workloads deducted in order (one first-fit set each), then the sum over
 * the nodes that MatchNode accepts (nodeSelector, required node affinity,
 * tolerations incl. the unschedulable taint; filter.go:38-99) of int32(MaxDivided)
 * of the node's available resources (allocatable - requested, clamped at 0; pods =
 * allocatable pods - n_pods, util/resource.go:96-115,221-248; noderesource.go:
 * 135-144) for `request`. claim may be NULL (no NodeClaim). *out = the int32 sum
 * (Go's atomic int32 adds wrap). Replaces AccurateSchedulerEstimatorServer.
 * EstimateReplicas for one request (estimate.go:33-76; 0 when there are no nodes). */
int kp_node_max_replicas(kp_engine* e, const kp_node* nodes, uint64_t n_nodes, const kp_resource* request,
                         uint32_t n_request, const kp_node_claim* claim, const kp_assumed_workload* assumed,
                         uint32_t n_assumed, int32_t* out);

/* The accurate estimator's component-set path: nodeResourceEstimator.EstimateComponents
 * (noderesource.go:146-190): the assumed workloads deducted as above, then the
 * first-fit simulation (SchedulingSimulator.SimulateScheduling,
 * scheduling_simulator_components.go:51-131) of complete component sets over the
 * nodes' available resources, each component placed on the nodes that MatchNode
 * accepts for its NodeClaim, up to MaxInt32 sets. n_components == 0 -> *out =
 * MaxInt32 (noNodeConstraint, the reference's Noopperation result); otherwise *out
 * = the set count (0 = the reference's Unschedulable "no enough resources").
 * KP_ENOTSUP past 16 components per set, 64 in all, 16 assumed workloads or 7
 * distinct requested resources. */
int kp_node_max_component_sets(kp_engine* e, const kp_node* nodes, uint64_t n_nodes,
                               const kp_node_component* components, uint32_t n_components,
                               const kp_assumed_workload* assumed, uint32_t n_assumed, int32_t* out);

/* Last schedule call's stage timings. */
int kp_last_stage_times(const kp_engine* e, kp_stage_times* out);

/* Per-kernel times of the last kp_schedule_batch, with profiling on
 * (kp_engine_set_profile(e, 1): an event pair around every launch on its own
 * stream; off by default). One entry per kernel name: the summed HIP-event time of
 * its launches, their count, and the bindings (or class rows) they covered. */
typedef struct kp_kernel_time {
  char name[32];
  float ms;
  uint32_t launches;
  uint64_t units;
} kp_kernel_time;
int kp_engine_set_profile(kp_engine* e, int on);
/* *n_out = the number of entries; at most `cap` are written to out. */
int kp_last_kernel_times(const kp_engine* e, kp_kernel_time* out, uint32_t cap, uint32_t* n_out);

/* Host threads an engine packs a batch on (kp_batch_create); default: the
 * hardware threads, at most 16. */
int kp_engine_set_threads(kp_engine* e, int n_threads);

/* A replica of snapshot `src` (of another engine, on another device) on engine e's
 * device: the packed device image copied device to device (hipMemcpyPeer, over xGMI
 * between the GPUs of one node) instead of re-packed and re-uploaded. The replica
 * schedules exactly as `src` does. */
int kp_snapshot_replicate(kp_engine* e, const kp_snapshot* src, kp_snapshot** out);

/* ---- one scheduler process over N GPUs (SURVEY §8(b) Threading, §8(e)) ------------
 * Replaces the reference scheduler's single worker (pkg/scheduler/scheduler.go:327):
 * a kp_multi owns one engine per device (own HIP streams); its snapshot is packed on
 * the first device and replicated onto the others (kp_snapshot_replicate); a batch
 * is cut into contiguous binding shards at equal prefix sums of the §8(e) cost
 * C + Replicas*log2 C, one per device; kp_multi_schedule runs the shards
 * concurrently (one host thread per device, no cross-device traffic) and returns one
 * CSR in binding order, identical to kp_schedule_batch over the whole batch on one
 * device. Result buffers belong to the batch and stay valid until its next
 * kp_multi_schedule or destruction. Verified on the host build (several simulated
 * devices, tests/test_multi.py) and on one physical GPU only: the cross-device
 * replication (hipMemcpyPeerAsync) has not run on two or more GPUs yet. */
typedef struct kp_multi kp_multi;
typedef struct kp_multi_snapshot kp_multi_snapshot;
typedef struct kp_multi_batch kp_multi_batch;

int kp_multi_create(const int* devices, uint32_t n_devices, kp_multi** out);
void kp_multi_destroy(kp_multi* m);
const char* kp_multi_last_error(const kp_multi* m);
uint32_t kp_multi_devices(const kp_multi* m);
/* The engine of the i-th device (stage times, diagnosis entry points); owned by m. */
kp_engine* kp_multi_engine(kp_multi* m, uint32_t i);

int kp_multi_snapshot_create(kp_multi* m, const kp_cluster* clusters, uint64_t n_clusters, const kp_options* opts,
                             kp_multi_snapshot** out);
/* kp_snapshot_update on every replica (same semantics, same dict_grew). If it fails on
 * any device the others may already have applied the rows, so the multi snapshot is
 * marked invalid: this call, kp_multi_batch_create and kp_multi_schedule on it return
 * KP_ESTATE until it is destroyed and created again. */
int kp_multi_snapshot_update(kp_multi* m, kp_multi_snapshot* s, const kp_cluster* clusters, uint64_t n_clusters,
                             int* dict_grew);
void kp_multi_snapshot_destroy(kp_multi_snapshot* s);
/* The i-th device's replica; owned by s. */
kp_snapshot* kp_multi_snapshot_replica(kp_multi_snapshot* s, uint32_t i);

/* The shard cuts kp_multi_batch_create uses: starts[0..n_shards], starts[0] = 0,
 * starts[n_shards] = n_bindings. */
int kp_multi_shard_cuts(const kp_binding* bindings, uint64_t n_bindings, uint64_t n_clusters, uint32_t n_shards,
                        uint64_t* starts);
int kp_multi_batch_create(kp_multi* m, const kp_multi_snapshot* s, const kp_binding* bindings, uint64_t n_bindings,
                          kp_multi_batch** out);
void kp_multi_batch_destroy(kp_multi_batch* b);
/* The batch's shard cuts (n_devices + 1 entries). */
int kp_multi_batch_shards(const kp_multi_batch* b, uint64_t* starts);
/* genericScheduler.Schedule for every binding, the shards on their devices at once. */
int kp_multi_schedule(kp_multi* m, kp_multi_batch* b, kp_results* out);

#ifdef __cplusplus
}
#endif

#endif /* KP_API_H */
