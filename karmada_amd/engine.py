"""Host-side mirror of the reference scheduling interface over libkp.so.

The product path: Python objects -> kp_api.h structs (api.World) -> libkp.so
(C-ABI, HIP kernels on gfx950). There is no CPU fallback: if libkp.so is
missing or no GPU is visible, construction raises.

Mirrors (reference file:line):
  GenericScheduler.schedule  <- genericScheduler.Schedule
                                 (pkg/scheduler/core/generic_scheduler.go:70-121)
  GenericScheduler.filter    <- findClustersThatFit (generic_scheduler.go:123-150)
  GenericScheduler.score     <- prioritizeClusters (generic_scheduler.go:152-181)
  GenericScheduler.max_available_replicas
                             <- estimator.ReplicaEstimator.MaxAvailableReplicas
                                 (pkg/estimator/client/interface.go:34-37) via
                                 calAvailableReplicas (core/util.go:56-118)
  Watch.affected / GenericScheduler.affected_bindings
                             <- Scheduler.enqueueAffectedBindings / enqueueAffectedCRBs
                                 (pkg/scheduler/event_handler.go:400-491)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

from karmada_amd import api

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libkp.so")
KP_ABI_VERSION = 16

_LIBS = {}

# C-ABI entry points declared in include/kp/kp_api.h
EXPORTS = (
    "kp_abi_version", "kp_engine_create", "kp_engine_destroy", "kp_last_error", "kp_snapshot_create",
    "kp_snapshot_destroy", "kp_snapshot_export", "kp_snapshot_import", "kp_snapshot_update", "kp_batch_create",
    "kp_batch_destroy", "kp_batch_create_keyed", "kp_batch_create_estimates", "kp_batch_create_filters", "kp_batch_digest", "kp_pack_cache_create", "kp_pack_cache_destroy",
    "kp_pack_cache_get_stats",
    "kp_schedule_batch", "kp_schedule_batch_submit", "kp_schedule_batch_collect",
    "kp_schedule_batch_packed", "kp_schedule_batch_submit_packed", "kp_schedule_batch_collect_packed", "kp_results_unpack",
    "kp_schedule_batch_delta", "kp_schedule_batch_submit_delta", "kp_schedule_batch_collect_delta",
    "kp_schedule_affinities", "kp_schedule_affinities_ex", "kp_filter_batch", "kp_filter_reasons", "kp_fit_diagnosis_batch", "kp_score_batch", "kp_max_available_replicas", "kp_max_available_component_sets",
    "kp_model_grades", "kp_node_max_replicas", "kp_node_max_component_sets", "kp_last_stage_times",
    "kp_engine_set_threads", "kp_snapshot_replicate", "kp_engine_set_profile", "kp_last_kernel_times",
    "kp_watch_create", "kp_watch_destroy", "kp_affected_bindings",
    "kp_assumptions_create", "kp_assumptions_destroy", "kp_batch_create_assumed",
    "kp_multi_create", "kp_multi_destroy", "kp_multi_last_error", "kp_multi_devices", "kp_multi_engine",
    "kp_multi_snapshot_create", "kp_multi_snapshot_update", "kp_multi_snapshot_destroy", "kp_multi_snapshot_replica",
    "kp_multi_shard_cuts", "kp_multi_batch_create", "kp_multi_batch_destroy", "kp_multi_batch_shards",
    "kp_multi_schedule",
)

KP_OK, KP_EINVAL, KP_ENOMEM, KP_EDEVICE, KP_ENOTSUP, KP_ESTATE = 0, -1, -2, -3, -4, -5


class EngineError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH):
    """Loads libkp.so and declares the C-ABI signatures. Raises if it is absent."""
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise EngineError(f"{path} is missing: build it with `make -C karmada_amd/csrc` "
                          "(there is no CPU fallback)")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.kp_abi_version.restype = C.c_int
    L.kp_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.kp_engine_destroy.argtypes = [vp]
    L.kp_last_error.restype = C.c_char_p
    L.kp_last_error.argtypes = [vp]
    L.kp_snapshot_create.argtypes = [vp, C.POINTER(api.kp_cluster), C.c_uint64, C.POINTER(api.kp_options),
                                     C.POINTER(vp)]
    L.kp_snapshot_destroy.argtypes = [vp]
    L.kp_batch_create.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.c_uint64, C.POINTER(vp)]
    L.kp_batch_destroy.argtypes = [vp]
    L.kp_batch_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kp_pack_cache_create.argtypes = [C.c_uint64, C.POINTER(vp)]
    L.kp_pack_cache_destroy.argtypes = [vp]
    L.kp_pack_cache_get_stats.argtypes = [vp, C.POINTER(api.kp_pack_cache_stats)]
    L.kp_batch_create_keyed.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.POINTER(api.kp_binding_key), C.c_uint64,
                                        vp, C.POINTER(vp)]
    L.kp_batch_create_estimates.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.POINTER(api.kp_binding_key),
                                            C.c_uint64, vp, C.POINTER(api.kp_estimates), C.POINTER(vp)]
    L.kp_batch_create_filters.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.POINTER(api.kp_binding_key),
                                          C.c_uint64, vp, C.POINTER(api.kp_estimates),
                                          C.POINTER(api.kp_filter_answers), C.POINTER(vp)]
    L.kp_assumptions_create.argtypes = [vp, vp, C.POINTER(api.kp_assumed_entry), C.c_uint64, C.POINTER(vp)]
    L.kp_assumptions_destroy.argtypes = [vp]
    L.kp_assumptions_destroy.restype = None
    L.kp_batch_create_assumed.argtypes = [vp, vp, vp, C.POINTER(api.kp_binding), C.c_uint64, C.POINTER(vp)]
    L.kp_schedule_batch.argtypes = [vp, vp, C.POINTER(api.kp_results)]
    L.kp_schedule_batch_submit.argtypes = [vp, vp]
    L.kp_schedule_batch_collect.argtypes = [vp, vp, C.POINTER(api.kp_results)]
    L.kp_schedule_batch_packed.argtypes = [vp, vp, C.POINTER(api.kp_results_packed)]
    L.kp_schedule_batch_submit_packed.argtypes = [vp, vp]
    L.kp_schedule_batch_collect_packed.argtypes = [vp, vp, C.POINTER(api.kp_results_packed)]
    L.kp_results_unpack.argtypes = [C.POINTER(api.kp_results_packed), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    L.kp_schedule_batch_delta.argtypes = [vp, vp, C.POINTER(api.kp_results_delta)]
    L.kp_schedule_batch_submit_delta.argtypes = [vp, vp]
    L.kp_schedule_batch_collect_delta.argtypes = [vp, vp, C.POINTER(api.kp_results_delta)]
    L.kp_schedule_affinities.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.c_uint64,
                                         C.POINTER(api.kp_affinity_results)]
    L.kp_schedule_affinities_ex.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.c_uint64,
                                            C.POINTER(api.kp_affinity_answers), C.POINTER(api.kp_affinity_results)]
    L.kp_filter_batch.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.kp_score_batch.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.kp_filter_reasons.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
    L.kp_fit_diagnosis_batch.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(api.kp_fit_diagnosis)]
    L.kp_max_available_replicas.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64,
                                            C.POINTER(C.c_int32)]
    L.kp_max_available_component_sets.argtypes = [vp, vp, C.POINTER(api.kp_component), C.c_uint32,
                                                  C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_int32)]
    L.kp_last_stage_times.argtypes = [vp, C.POINTER(api.kp_stage_times)]
    L.kp_model_grades.argtypes = [vp, C.POINTER(api.kp_resource_model), C.c_uint32, C.POINTER(api.kp_node),
                                  C.c_uint64, C.POINTER(C.c_int64)]
    L.kp_node_max_replicas.argtypes = [vp, C.POINTER(api.kp_node), C.c_uint64, C.POINTER(api.kp_resource), C.c_uint32,
                                       C.POINTER(api.kp_node_claim), C.POINTER(api.kp_assumed_workload), C.c_uint32,
                                       C.POINTER(C.c_int32)]
    L.kp_node_max_component_sets.argtypes = [vp, C.POINTER(api.kp_node), C.c_uint64, C.POINTER(api.kp_node_component),
                                             C.c_uint32, C.POINTER(api.kp_assumed_workload), C.c_uint32,
                                             C.POINTER(C.c_int32)]
    L.kp_snapshot_export.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.kp_snapshot_import.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(vp)]
    L.kp_snapshot_update.argtypes = [vp, vp, C.POINTER(api.kp_cluster), C.c_uint64, C.POINTER(C.c_int)]
    L.kp_engine_set_threads.argtypes = [vp, C.c_int]
    L.kp_engine_set_profile.argtypes = [vp, C.c_int]
    L.kp_last_kernel_times.argtypes = [vp, C.POINTER(api.kp_kernel_time), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kp_snapshot_replicate.argtypes = [vp, vp, C.POINTER(vp)]
    L.kp_watch_create.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(vp)]
    L.kp_watch_destroy.argtypes = [vp]
    L.kp_affected_bindings.argtypes = [vp, vp, vp, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(api.kp_affected)]
    L.kp_multi_create.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(vp)]
    L.kp_multi_destroy.argtypes = [vp]
    L.kp_multi_last_error.restype = C.c_char_p
    L.kp_multi_last_error.argtypes = [vp]
    L.kp_multi_devices.restype = C.c_uint32
    L.kp_multi_devices.argtypes = [vp]
    L.kp_multi_engine.restype = vp
    L.kp_multi_engine.argtypes = [vp, C.c_uint32]
    L.kp_multi_snapshot_create.argtypes = [vp, C.POINTER(api.kp_cluster), C.c_uint64, C.POINTER(api.kp_options),
                                           C.POINTER(vp)]
    L.kp_multi_snapshot_update.argtypes = [vp, vp, C.POINTER(api.kp_cluster), C.c_uint64, C.POINTER(C.c_int)]
    L.kp_multi_snapshot_destroy.argtypes = [vp]
    L.kp_multi_snapshot_replica.restype = vp
    L.kp_multi_snapshot_replica.argtypes = [vp, C.c_uint32]
    L.kp_multi_shard_cuts.argtypes = [C.POINTER(api.kp_binding), C.c_uint64, C.c_uint64, C.c_uint32,
                                      C.POINTER(C.c_uint64)]
    L.kp_multi_batch_create.argtypes = [vp, vp, C.POINTER(api.kp_binding), C.c_uint64, C.POINTER(vp)]
    L.kp_multi_batch_destroy.argtypes = [vp]
    L.kp_multi_batch_shards.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kp_multi_schedule.argtypes = [vp, vp, C.POINTER(api.kp_results)]
    if L.kp_abi_version() != KP_ABI_VERSION:
        raise EngineError("libkp.so ABI version mismatch")
    _LIBS[path] = L
    return L


@dataclass
class TargetCluster:
    """workv1alpha2.TargetCluster (pkg/apis/work/v1alpha2/binding_types.go)."""
    name: str
    replicas: int


@dataclass
class ScheduleResult:
    """core.ScheduleResult (generic_scheduler.go:54-56) plus the error the reference returns."""
    suggested_clusters: List[TargetCluster] = field(default_factory=list)
    status: int = api.STATUS_OK
    err: int = 0
    arg: int = 0
    observed_affinity_name: Optional[str] = None  # set by schedule_with_affinities

    @property
    def error(self) -> Optional[str]:
        if self.status == api.STATUS_OK:
            return None
        return f"{api.ERR_NAMES.get(self.err, self.err)} ({self.arg})"


class Engine:
    """One HIP device + stream (kp_engine)."""

    def __init__(self, device: int = 0, lib_path: str = LIB_PATH):
        self.L = load_library(lib_path)
        h = C.c_void_p()
        rc = self.L.kp_engine_create(device, C.byref(h))
        if rc != KP_OK:
            raise EngineError(f"kp_engine_create(device={device}) failed: rc={rc}")
        self.h = h

    def _check(self, rc: int, what: str):
        if rc != KP_OK:
            raise EngineError(f"{what}: rc={rc}: {self.L.kp_last_error(self.h).decode(errors='replace')}")

    def close(self):
        if self.h:
            self.L.kp_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def model_grades(self, models: Sequence[dict], nodes: Sequence[dict]) -> List[int]:
        """getAllocatableModelings' AllocatableModeling counts, one per model
        (kp_model_grades; cluster_status_controller.go:642-677)."""
        w = api.World()
        ma, nm = w.models(models)
        na, nn = w.nodes(nodes)
        out = (C.c_int64 * max(1, nm))()
        self._check(self.L.kp_model_grades(self.h, ma, nm, na, nn, out), "kp_model_grades")
        return [int(out[i]) for i in range(nm)]

    def node_max_replicas(self, nodes: Sequence[dict], request: Optional[Dict[str, str]],
                          node_claim: Optional[dict] = None, assumed: Optional[Sequence[dict]] = None) -> int:
        """The estimator server's per-node answer (kp_node_max_replicas;
        noderesource.go:70-131) for one ReplicaRequirements, after the assumed
        workloads' deduction."""
        w = api.World()
        na, nn = w.nodes(nodes)
        ra, nr = w.resources(request)
        claim = w.node_claim(node_claim)
        aa, namd = w.assumed_workloads(assumed)
        out = C.c_int32()
        self._check(self.L.kp_node_max_replicas(self.h, na, nn, ra, nr, C.byref(claim) if claim is not None else None,
                                                aa, namd, C.byref(out)), "kp_node_max_replicas")
        return int(out.value)

    def node_max_component_sets(self, nodes: Sequence[dict], components: Sequence[dict],
                                assumed: Optional[Sequence[dict]] = None) -> int:
        """The estimator server's component-set answer (kp_node_max_component_sets;
        noderesource.go:146-190): complete sets of `components` the nodes hold."""
        w = api.World()
        na, nn = w.nodes(nodes)
        ca, nc = w.node_components(components)
        aa, namd = w.assumed_workloads(assumed)
        out = C.c_int32()
        self._check(self.L.kp_node_max_component_sets(self.h, na, nn, ca, nc, aa, namd, C.byref(out)),
                    "kp_node_max_component_sets")
        return int(out.value)

    def stage_times(self) -> Dict[str, float]:
        t = api.kp_stage_times()
        self._check(self.L.kp_last_stage_times(self.h, C.byref(t)), "kp_last_stage_times")
        return {k: getattr(t, k) for k, _ in api.kp_stage_times._fields_}

    def set_profile(self, on: bool = True):
        """Per-kernel HIP-event timing of kp_schedule_batch (kp_engine_set_profile)."""
        self._check(self.L.kp_engine_set_profile(self.h, int(on)), "kp_engine_set_profile")

    def kernel_times(self) -> Dict[str, dict]:
        """{kernel name: {ms, launches, units}} of the last kp_schedule_batch (profiling on)."""
        n = C.c_uint32()
        self._check(self.L.kp_last_kernel_times(self.h, None, 0, C.byref(n)), "kp_last_kernel_times")
        arr = (api.kp_kernel_time * max(1, n.value))()
        self._check(self.L.kp_last_kernel_times(self.h, arr, n.value, C.byref(n)), "kp_last_kernel_times")
        return {arr[i].name.decode(): {"ms": arr[i].ms, "launches": arr[i].launches, "units": arr[i].units}
                for i in range(n.value)}


class Snapshot:
    """cache.Snapshot (pkg/scheduler/cache/snapshot.go) packed into HBM."""

    def __init__(self, engine: Engine, clusters: Sequence[dict], opts: Optional[api.kp_options] = None):
        self.engine = engine
        self.names = [c["name"] for c in clusters]
        w = api.World()
        ca, n = w.clusters(clusters)
        self.opts = opts or api.options()
        h = C.c_void_p()
        engine._check(engine.L.kp_snapshot_create(engine.h, ca, n, C.byref(self.opts), C.byref(h)),
                      "kp_snapshot_create")
        self.h = h

    @classmethod
    def from_structs(cls, engine: Engine, ca, n: int, names: List[str], opts: api.kp_options):
        self = cls.__new__(cls)
        self.engine, self.names, self.opts = engine, names, opts
        h = C.c_void_p()
        engine._check(engine.L.kp_snapshot_create(engine.h, ca, n, C.byref(opts), C.byref(h)), "kp_snapshot_create")
        self.h = h
        return self

    def to_bytes(self) -> bytes:
        """Packed snapshot bytes (kp_snapshot_export) for broadcast to other ranks."""
        p, n = C.c_void_p(), C.c_uint64()
        self.engine._check(self.engine.L.kp_snapshot_export(self.h, C.byref(p), C.byref(n)), "kp_snapshot_export")
        return C.string_at(p, n.value)

    @classmethod
    def from_bytes(cls, engine: Engine, data: bytes, names: List[str]):
        """kp_snapshot_import: the packed snapshot of another rank, uploaded to this engine's device."""
        self = cls.__new__(cls)
        self.engine, self.names, self.opts = engine, names, None
        h = C.c_void_p()
        engine._check(engine.L.kp_snapshot_import(engine.h, data, len(data), C.byref(h)), "kp_snapshot_import")
        self.h = h
        return self

    def update_structs(self, ca, n: int) -> bool:
        """kp_snapshot_update: re-pack the n clusters of `ca` (existing names) in place.
        Returns True when the dictionaries grew (batches packed before must be re-created)."""
        grew = C.c_int(0)
        self.engine._check(self.engine.L.kp_snapshot_update(self.engine.h, self.h, ca, n, C.byref(grew)),
                           "kp_snapshot_update")
        return bool(grew.value)

    def update(self, clusters: Sequence[dict]) -> bool:
        """Cluster events (informer updates) applied to the packed snapshot; see update_structs."""
        w = api.World()
        ca, n = w.clusters(clusters)
        return self.update_structs(ca, n)

    def close(self):
        if getattr(self, "h", None):
            self.engine.L.kp_snapshot_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PackCache:
    """Packed binding records kept across scheduling cycles (kp_pack_cache): a binding
    whose (metadata.uid, metadata.generation) and scheduler status fields match a record
    is copied instead of re-packed (pkg/scheduler/scheduler.go:437-468 re-runs Schedule
    for bindings whose spec did not change)."""

    def __init__(self, engine: "Engine", max_entries: int = 0):
        self.L = engine.L
        h = C.c_void_p()
        if self.L.kp_pack_cache_create(max_entries, C.byref(h)) != KP_OK:
            raise EngineError("kp_pack_cache_create failed")
        self.h = h

    def stats(self) -> dict:
        st = api.kp_pack_cache_stats()
        self.L.kp_pack_cache_get_stats(self.h, C.byref(st))
        return {"hits": st.hits, "misses": st.misses, "entries": st.entries, "last_hits": st.last_hits}

    def close(self):
        if getattr(self, "h", None):
            self.L.kp_pack_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Assumptions:
    """The scheduler's assumed workloads deducted once per cluster (kp_assumptions): `entries` is
    [(cluster index or name, [component dicts])], one per AssumedWorkload, each cluster's in the
    order they are to be deducted. An empty list is the gate off."""

    def __init__(self, snap: Snapshot, entries: Sequence[tuple] = ()):
        self.snap = snap
        eng = snap.engine
        idx = {n: i for i, n in enumerate(snap.names)}
        w = api.World()
        ea, n = w.assumed_entries([(idx[c] if isinstance(c, str) else c, comps) for c, comps in entries])
        h = C.c_void_p()
        eng._check(eng.L.kp_assumptions_create(eng.h, snap.h, ea, n, C.byref(h)), "kp_assumptions_create")
        self.h = h
        self.n = n

    def close(self):
        if getattr(self, "h", None):
            self.snap.engine.L.kp_assumptions_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """A batch of ResourceBindings packed against one snapshot (kp_batch). With `cache`
    and `keys` ((uid, generation) per binding, api.binding_keys) it is created through
    kp_batch_create_keyed: bindings whose record the cache holds skip packing. With
    `estimates` = (rows, row_of) it is created through kp_batch_create_estimates: rows is an
    int32 array [R, C] of the other estimators' merged answers (caller cluster order, -1 =
    no answer), row_of each binding's row (-1 for none). With `filters` = (rows, row_of,
    n_plugins) it is created through kp_batch_create_filters (together with `estimates`, if
    given): rows is a bool array [R, C] of the out-of-tree filter plugins' ANDed verdicts
    (caller cluster order, True = passed), row_of each binding's row (-1: no plugin
    objected), n_plugins the number of registered out-of-tree plugins they fold in. With
    `assumed` (an Assumptions) it is created through kp_batch_create_assumed and answers over
    the deducted availability; the engine has no entry point that combines assumptions with
    a cache, estimates or filters, so that is refused here (EngineError, KP_ENOTSUP)."""

    def __init__(self, snap: Snapshot, bindings: Sequence[dict] = (), structs=None, cache: "PackCache" = None,
                 keys=None, generations: Sequence[int] = None, estimates=None, filters=None,
                 assumed: "Assumptions" = None):
        self.snap = snap
        eng = snap.engine
        if assumed is not None and (cache is not None or estimates is not None or filters is not None):
            raise EngineError(f"kp_batch_create_assumed: rc={KP_ENOTSUP}: assumed workloads do not combine with a "
                              "pack cache, estimates or filter answers")
        if structs is None:
            w = api.World()
            ba, n = w.bindings(bindings)
            self._w = w
        else:
            ba, n = structs
        self.n = n
        h = C.c_void_p()
        if cache is not None and keys is None:  # (uid from each binding, metadata.generation given)
            keys = api.binding_keys(ba, n, generations if generations is not None else [0] * n)
        est = None
        if estimates is not None:
            rows, row_of = estimates
            if len(row_of) != n:
                raise ValueError(f"estimates: row_of has {len(row_of)} entries for {n} bindings")
            est, self._est = api.estimates(rows, row_of)
        if assumed is not None:
            eng._check(eng.L.kp_batch_create_assumed(eng.h, snap.h, assumed.h, ba, n, C.byref(h)),
                       "kp_batch_create_assumed")
        elif filters is not None:
            rows, row_of, n_plugins = filters
            if len(row_of) != n:
                raise ValueError(f"filters: row_of has {len(row_of)} entries for {n} bindings")
            flt, self._flt = api.filter_answers(rows, row_of, n_plugins)
            self._keys = keys if cache is not None else None
            eng._check(eng.L.kp_batch_create_filters(eng.h, snap.h, ba, self._keys, n,
                                                     cache.h if cache is not None else None,
                                                     C.byref(est) if est is not None else None, C.byref(flt),
                                                     C.byref(h)), "kp_batch_create_filters")
        elif estimates is not None:
            self._keys = keys if cache is not None else None
            eng._check(eng.L.kp_batch_create_estimates(eng.h, snap.h, ba, self._keys, n,
                                                       cache.h if cache is not None else None, C.byref(est),
                                                       C.byref(h)), "kp_batch_create_estimates")
        elif cache is not None:
            self._keys = keys
            eng._check(eng.L.kp_batch_create_keyed(eng.h, snap.h, ba, keys, n, cache.h, C.byref(h)),
                       "kp_batch_create_keyed")
        else:
            eng._check(eng.L.kp_batch_create(eng.h, snap.h, ba, n, C.byref(h)), "kp_batch_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.snap.engine.L.kp_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def digest(self) -> int:
        """kp_batch_digest: the packed image's digest (equal for equal packs)."""
        d = C.c_uint64()
        self.snap.engine._check(self.snap.engine.L.kp_batch_digest(self.h, C.byref(d)), "kp_batch_digest")
        return d.value

    def schedule_raw(self) -> api.kp_results:
        r = api.kp_results()
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch(eng.h, self.h, C.byref(r)), "kp_schedule_batch")
        return r

    def submit(self):
        """kp_schedule_batch_submit: queue this batch's schedule call (collect() finishes it)."""
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_submit(eng.h, self.h), "kp_schedule_batch_submit")

    def collect(self) -> api.kp_results:
        """kp_schedule_batch_collect: the results of the submitted call (as schedule_raw)."""
        r = api.kp_results()
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_collect(eng.h, self.h, C.byref(r)), "kp_schedule_batch_collect")
        return r

    def schedule_packed_raw(self) -> api.kp_results_packed:
        """kp_schedule_batch_packed: the results in 4 bytes per target (api.kp_results_packed)."""
        r = api.kp_results_packed()
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_packed(eng.h, self.h, C.byref(r)), "kp_schedule_batch_packed")
        return r

    def submit_packed(self):
        """kp_schedule_batch_submit_packed: submit() for a call collected by collect_packed()."""
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_submit_packed(eng.h, self.h), "kp_schedule_batch_submit_packed")

    def collect_packed(self) -> api.kp_results_packed:
        """kp_schedule_batch_collect_packed: the results of the call submit_packed() queued."""
        r = api.kp_results_packed()
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_collect_packed(eng.h, self.h, C.byref(r)),
                   "kp_schedule_batch_collect_packed")
        return r

    def unpack(self, r: api.kp_results_packed):
        """kp_results_unpack: (cluster_idx, replicas) ctypes arrays of r.n_targets entries."""
        ci = (C.c_uint32 * max(1, r.n_targets))()
        rep = (C.c_int32 * max(1, r.n_targets))()
        eng = self.snap.engine
        if eng.L.kp_results_unpack(C.byref(r), ci, rep) != KP_OK:
            raise EngineError("kp_results_unpack: the packed results are inconsistent")
        return ci, rep

    def schedule_delta_raw(self) -> api.kp_results_delta:
        """kp_schedule_batch_delta: every binding's status, and the targets of the bindings whose
        placement differs from the spec.Clusters they were packed with (api.kp_results_delta)."""
        r = api.kp_results_delta()
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_delta(eng.h, self.h, C.byref(r)), "kp_schedule_batch_delta")
        return r

    def submit_delta(self):
        """kp_schedule_batch_submit_delta: submit() for a call collected by collect_delta()."""
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_submit_delta(eng.h, self.h), "kp_schedule_batch_submit_delta")

    def collect_delta(self) -> api.kp_results_delta:
        """kp_schedule_batch_collect_delta: the results of the call submit_delta() queued."""
        r = api.kp_results_delta()
        eng = self.snap.engine
        eng._check(eng.L.kp_schedule_batch_collect_delta(eng.h, self.h, C.byref(r)),
                   "kp_schedule_batch_collect_delta")
        return r

    def schedule_delta(self):
        """(statuses, {index: result dict}): (status, err, arg) of every binding, and the
        api.results_to_python dict of each binding whose placement changed."""
        r = self.schedule_delta_raw()
        st = [(int(r.status[i]), int(r.err_code[i]), int(r.err_arg[i])) for i in range(r.n_bindings)]
        out = {}
        for i in range(r.n_changed):
            b = int(r.changed[i])
            tg = sorted((int(r.cluster_idx[k]), int(r.replicas[k])) for k in range(r.offsets[i], r.offsets[i + 1]))
            out[b] = {"status": st[b][0], "err": st[b][1], "arg": st[b][2], "targets": tg}
        return st, out

    def fit_diagnosis_raw(self, bindings: Optional[Sequence[int]] = None) -> api.kp_fit_diagnosis:
        """kp_fit_diagnosis_batch: the engine's arrays, valid until the next call on it."""
        d = api.kp_fit_diagnosis()
        eng = self.snap.engine
        if bindings is None:
            arr, n = None, 0
        else:
            n = len(bindings)
            arr = (C.c_uint64 * max(1, n))(*bindings)
        eng._check(eng.L.kp_fit_diagnosis_batch(eng.h, self.h, arr, n, C.byref(d)), "kp_fit_diagnosis_batch")
        return d

    def fit_diagnosis(self, bindings: Optional[Sequence[int]] = None) -> List[tuple]:
        """The FitError reason histogram of each listed binding (strictly ascending batch
        indices), or with bindings=None of every binding whose status was STATUS_FIT_ERROR in
        this batch's last completed schedule call: (index, n_fit, n_deleting, [(reason,
        taint_ref, count), ...]), the bins by reason code, then taint_ref. A REASON_TAINT
        bin's taint_ref names the taint: caller cluster index | taint index << 18
        (GenericScheduler.fit_errors resolves it)."""
        d = self.fit_diagnosis_raw(bindings)
        out = []
        for i in range(d.n_bindings):
            lo, hi = d.offsets[i], d.offsets[i + 1]
            out.append((int(d.binding[i]), int(d.n_fit[i]), int(d.n_deleting[i]),
                        [(int(d.reason[k]), int(d.taint_ref[k]), int(d.count[k])) for k in range(lo, hi)]))
        return out

    def schedule(self, packed: bool = False) -> List[dict]:
        """Results as api.results_to_python dicts (cluster indices in snapshot input order).
        packed: through kp_schedule_batch_packed and kp_results_unpack (the same dicts)."""
        if packed:
            p = self.schedule_packed_raw()
            ci, rep = self.unpack(p)
            return api.results_to_python(p.status, p.err_code, p.err_arg, p.offsets, ci, rep, p.n_bindings)
        r = self.schedule_raw()
        return api.results_to_python(r.status, r.err_code, r.err_arg, r.offsets, r.cluster_idx, r.replicas,
                                     r.n_bindings)


class Watch:
    """The bindings a cluster event can affect (kp_watch): per binding the compiled selector
    of the one affinity enqueueAffectedBindings / enqueueAffectedCRBs evaluate
    (pkg/scheduler/event_handler.go:400-491). modes: api.WATCH_* per binding (None: all
    WATCH_MATCH). A watch answers for the snapshot it was made over until a Snapshot.update
    on it returns True (the dictionaries grew): then make a new one."""

    def __init__(self, snap: Snapshot, bindings: Sequence[dict] = (), structs=None,
                 modes: Optional[Sequence[int]] = None):
        self.snap = snap
        eng = snap.engine
        if structs is None:
            w = api.World()
            ba, n = w.bindings(bindings)
        else:
            ba, n = structs
        self.n = n
        marr = None
        if modes is not None:
            if len(modes) != n:
                raise ValueError(f"modes has {len(modes)} entries for {n} bindings")
            marr = (C.c_uint8 * max(1, n))(*modes)
        h = C.c_void_p()
        eng._check(eng.L.kp_watch_create(eng.h, snap.h, ba, n, marr, C.byref(h)), "kp_watch_create")
        self.h = h

    def affected_raw(self, idx: Sequence[int], snap: Optional[Snapshot] = None) -> api.kp_affected:
        """kp_affected_bindings over caller cluster indices (a sequence, or a ctypes c_uint32
        array): the engine's list, valid until the next call on the engine. snap: the snapshot
        to answer over (default: the watch's own)."""
        eng = self.snap.engine
        out = api.kp_affected()
        arr = idx if isinstance(idx, C.Array) else (C.c_uint32 * max(1, len(idx)))(*idx)
        eng._check(eng.L.kp_affected_bindings(eng.h, self.h, (snap or self.snap).h, arr, len(idx), C.byref(out)),
                   "kp_affected_bindings")
        return out

    def affected(self, clusters: Sequence) -> List[int]:
        """The indices of the bindings to requeue for the changed clusters (names or caller
        indices, repeats allowed) in the snapshot's current state, ascending."""
        if any(isinstance(c, str) for c in clusters):
            pos = {n: i for i, n in enumerate(self.snap.names)}
            clusters = [pos[c] if isinstance(c, str) else c for c in clusters]
        r = self.affected_raw([int(c) for c in clusters])
        return [int(r.bindings[i]) for i in range(r.n)]

    def close(self):
        if getattr(self, "h", None):
            self.snap.engine.L.kp_watch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiEngine:
    """One scheduler process over N GPUs (kp_multi): an engine per device, the snapshot
    replicated device to device, each batch sharded by cost across the devices and
    scheduled concurrently, results merged in binding order. Replaces the reference
    scheduler's single worker (pkg/scheduler/scheduler.go:327)."""

    def __init__(self, devices: Sequence[int], lib_path: str = LIB_PATH):
        self.L = load_library(lib_path)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.L.kp_multi_create(devs, len(devices), C.byref(h))
        if rc != KP_OK:
            raise EngineError(f"kp_multi_create(devices={list(devices)}) failed: rc={rc}")
        self.h = h
        self.n_devices = int(self.L.kp_multi_devices(h))

    def _check(self, rc: int, what: str):
        if rc != KP_OK:
            raise EngineError(f"{what}: rc={rc}: {self.L.kp_multi_last_error(self.h).decode(errors='replace')}")

    def stage_times(self, i: int) -> Dict[str, float]:
        """kp_last_stage_times of device i's engine (its shard's last schedule)."""
        t = api.kp_stage_times()
        e = self.L.kp_multi_engine(self.h, i)
        if self.L.kp_last_stage_times(e, C.byref(t)) != KP_OK:
            raise EngineError("kp_last_stage_times")
        return {k: getattr(t, k) for k, _ in api.kp_stage_times._fields_}

    def snapshot(self, ca, n: int, opts: api.kp_options) -> "MultiSnapshot":
        return MultiSnapshot(self, ca, n, opts)

    def close(self):
        if getattr(self, "h", None):
            self.L.kp_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiSnapshot:
    """kp_multi_snapshot: packed on the first device, replicas on the others."""

    def __init__(self, m: MultiEngine, ca, n: int, opts: api.kp_options):
        self.m, self.opts, self.n_clusters = m, opts, n
        h = C.c_void_p()
        m._check(m.L.kp_multi_snapshot_create(m.h, ca, n, C.byref(opts), C.byref(h)), "kp_multi_snapshot_create")
        self.h = h

    def update_structs(self, ca, n: int) -> bool:
        grew = C.c_int(0)
        self.m._check(self.m.L.kp_multi_snapshot_update(self.m.h, self.h, ca, n, C.byref(grew)),
                      "kp_multi_snapshot_update")
        return bool(grew.value)

    def close(self):
        if getattr(self, "h", None):
            self.m.L.kp_multi_snapshot_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiBatch:
    """kp_multi_batch: a batch cut into per-device shards."""

    def __init__(self, snap: MultiSnapshot, structs):
        self.snap = snap
        m = snap.m
        ba, n = structs
        self.n = n
        h = C.c_void_p()
        m._check(m.L.kp_multi_batch_create(m.h, snap.h, ba, n, C.byref(h)), "kp_multi_batch_create")
        self.h = h

    def shards(self) -> List[int]:
        D = self.snap.m.n_devices
        out = (C.c_uint64 * (D + 1))()
        self.snap.m._check(self.snap.m.L.kp_multi_batch_shards(self.h, out), "kp_multi_batch_shards")
        return [int(out[i]) for i in range(D + 1)]

    def schedule_raw(self) -> api.kp_results:
        r = api.kp_results()
        m = self.snap.m
        m._check(m.L.kp_multi_schedule(m.h, self.h, C.byref(r)), "kp_multi_schedule")
        return r

    def schedule(self) -> List[dict]:
        r = self.schedule_raw()
        return api.results_to_python(r.status, r.err_code, r.err_arg, r.offsets, r.cluster_idx, r.replicas,
                                     r.n_bindings)

    def close(self):
        if getattr(self, "h", None):
            self.snap.m.L.kp_multi_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GenericScheduler:
    """genericScheduler (generic_scheduler.go:38-121) over a snapshot, batched."""

    def __init__(self, engine: Engine, clusters: Sequence[dict], opts: Optional[api.kp_options] = None):
        self.snapshot = Snapshot(engine, clusters, opts)

    def schedule(self, bindings: Sequence[dict], assumed: "Assumptions" = None) -> List[ScheduleResult]:
        """Schedule for every binding; with `assumed` (an Assumptions over this snapshot) over the
        availability left after the scheduler's assumed workloads."""
        b = Batch(self.snapshot, bindings, assumed=assumed)
        out = []
        names = self.snapshot.names
        for r in b.schedule():
            sr = ScheduleResult(status=r["status"], err=r["err"], arg=r["arg"])
            sr.suggested_clusters = [TargetCluster(names[i], rep) for i, rep in r["targets"]]
            out.append(sr)
        b.close()
        return out

    def schedule_changed(self, bindings: Sequence[dict], assumed: "Assumptions" = None):
        """schedule() for a requeue (patchScheduleResultForResourceBinding, scheduler.go:686-718):
        (results, changed). results holds every binding's ScheduleResult with its status;
        suggested_clusters is filled only for the bindings listed in `changed`, the ascending
        indices of those whose placement differs from their spec.clusters as a set of
        (name, replicas) pairs. The others keep the placement they hold: nothing to patch."""
        b = Batch(self.snapshot, bindings, assumed=assumed)
        try:
            st, delta = b.schedule_delta()
        finally:
            b.close()
        names = self.snapshot.names
        out = [ScheduleResult(status=s, err=e, arg=a) for s, e, a in st]
        for i, r in delta.items():
            out[i].suggested_clusters = [TargetCluster(names[c], rep) for c, rep in r["targets"]]
        return out, sorted(delta)

    def schedule_affinities_raw(self, structs, estimates=None, filters=None):
        """kp_schedule_affinities over packed kp_binding structs: (results dicts, affinity_index, attempts, rounds).
        With `estimates` = (rows, row_of) as for Batch and / or `filters` = (rows, row_of, n_plugins), row_of
        holding a list per binding with one row id per term, it is kp_schedule_affinities_ex."""
        ba, n = structs
        eng = self.snapshot.engine
        r = api.kp_affinity_results()
        if estimates is None and filters is None:
            eng._check(eng.L.kp_schedule_affinities(eng.h, self.snapshot.h, ba, n, C.byref(r)), "kp_schedule_affinities")
        else:
            n_terms = [max(1, int(ba[i].n_cluster_affinities)) for i in range(n)]
            ans, keep = api.affinity_answers(n_terms, estimates, filters, len(self.snapshot.names))
            eng._check(eng.L.kp_schedule_affinities_ex(eng.h, self.snapshot.h, ba, n, C.byref(ans), C.byref(r)),
                       "kp_schedule_affinities_ex")
            del keep
        rr = r.results
        res = api.results_to_python(rr.status, rr.err_code, rr.err_arg, rr.offsets, rr.cluster_idx, rr.replicas,
                                    rr.n_bindings)
        return res, [int(r.affinity_index[i]) for i in range(n)], [int(r.attempts[i]) for i in range(n)], r.rounds

    def schedule_with_affinities(self, bindings: Sequence[dict]) -> List[ScheduleResult]:
        """schedule_affinities without answers."""
        return self.schedule_affinities(bindings)

    def schedule_affinities(self, bindings: Sequence[dict], estimates=None, filters=None) -> List[ScheduleResult]:
        """Scheduler.scheduleResourceBindingWithClusterAffinities (scheduler.go:618-684) per binding,
        batched: every term retry of a round runs as one device batch. Each result carries the
        AffinityName that became Status.SchedulerObservedAffinityName (None: unchanged).
        estimates: (rows, row_of), the scheduler-estimator's answers as for Batch. filters:
        (rows, row_of, n_plugins), the out-of-tree filter plugins' verdicts, row_of[i] a list
        with binding i's row id for each of its terms (one entry without ClusterAffinities):
        a plugin sees the spec with the term's affinity substituted."""
        w = api.World()
        structs = w.bindings(bindings)
        res, aff, _, _ = self.schedule_affinities_raw(structs, estimates, filters)
        names = self.snapshot.names
        out = []
        for b, r, a in zip(bindings, res, aff):
            sr = ScheduleResult(status=r["status"], err=r["err"], arg=r["arg"])
            sr.suggested_clusters = [TargetCluster(names[i], rep) for i, rep in r["targets"]]
            terms = (b.get("placement") or {}).get("clusterAffinities") or []
            sr.observed_affinity_name = terms[a].get("affinityName") if a >= 0 else None
            out.append(sr)
        return out

    def filter(self, bindings: Sequence[dict], filters=None) -> List[List[str]]:
        """Feasible cluster names per binding (findClustersThatFit); filters: out-of-tree
        filter verdicts (Batch's `filters=`), ANDed in."""
        b = Batch(self.snapshot, bindings, filters=filters)
        eng = self.snapshot.engine
        C_ = len(self.snapshot.names)
        W = (C_ + 63) // 64
        m = (C.c_uint64 * max(1, b.n * W))()
        eng._check(eng.L.kp_filter_batch(eng.h, b.h, m), "kp_filter_batch")
        out = []
        for i in range(b.n):
            out.append([self.snapshot.names[c] for c in range(C_) if (m[i * W + (c >> 6)] >> (c & 63)) & 1])
        b.close()
        return out

    def affected_bindings(self, bindings: Sequence[dict], changed: Sequence,
                          modes: Optional[Sequence[int]] = None) -> List[int]:
        """enqueueAffectedBindings (event_handler.go:400-444) for the changed clusters (names
        or indices) at once: the indices of the bindings to requeue, ascending (Watch)."""
        w = Watch(self.snapshot, bindings, modes=modes)
        try:
            return w.affected(changed)
        finally:
            w.close()

    def filter_reasons(self, bindings: Sequence[dict], filters=None) -> List[List[int]]:
        """kp_filter_reasons: the KP_REASON_* word of every (binding, cluster) pair; filters:
        out-of-tree filter verdicts (Batch's `filters=`), reported as REASON_OUT_OF_TREE where
        the in-tree set fits."""
        b = Batch(self.snapshot, bindings, filters=filters)
        eng = self.snapshot.engine
        C_ = len(self.snapshot.names)
        r = (C.c_uint32 * max(1, b.n * C_))()
        eng._check(eng.L.kp_filter_reasons(eng.h, b.h, r), "kp_filter_reasons")
        out = [[int(r[i * C_ + c]) for c in range(C_)] for i in range(b.n)]
        b.close()
        return out

    def fit_error(self, binding: dict, clusters: Sequence[dict], filters=None, out_of_tree=None) -> str:
        """FitError{NumAllClusters, Diagnosis}.Error() for one binding (generic_scheduler.go:84-89);
        `clusters` are the snapshot's cluster dicts in its caller order. filters: the binding's
        out-of-tree filter verdicts (Batch's `filters=`); out_of_tree: the text of
        KP_REASON_OUT_OF_TREE, one string or {cluster name: text} (the rejecting plugin's own
        reason: the engine sees the verdict only)."""
        codes = self.filter_reasons([binding], filters=filters)[0]

        def text(code, cl):
            oot = out_of_tree.get(cl["name"]) if isinstance(out_of_tree, dict) else out_of_tree
            return api.reason_text(code, cl, oot)
        reasons = {cl["name"]: text(code, cl) for cl, code in zip(clusters, codes)
                   if code not in (api.REASON_FIT, api.REASON_DELETING)}
        return api.fit_error_message(len(clusters), reasons)

    def fit_errors(self, bindings: Sequence[dict], clusters: Sequence[dict], results=None, filters=None,
                   out_of_tree: Optional[str] = None) -> Dict[int, str]:
        """FitError.Error() of every failed binding of one batch, {binding index: text}, from
        one kp_fit_diagnosis_batch call (the reason histograms; no per-pair words cross the
        bus). results: the ScheduleResults schedule(bindings) returned, whose STATUS_FIT_ERROR
        entries are diagnosed; without them the batch is scheduled here first. clusters,
        filters: as fit_error; out_of_tree: the one text of REASON_OUT_OF_TREE bins."""
        b = Batch(self.snapshot, bindings, filters=filters)
        try:
            if results is None:
                b.schedule_raw()
                diag = b.fit_diagnosis()
            else:
                diag = b.fit_diagnosis([i for i, r in enumerate(results) if r.status == api.STATUS_FIT_ERROR])
        finally:
            b.close()
        mask = (1 << api.TAINT_REF_CLUSTER_BITS) - 1
        out = {}
        for idx, _, _, bins in diag:
            hist = {}
            for reason, ref, count in bins:
                word = reason | (ref >> api.TAINT_REF_CLUSTER_BITS) << 8
                text = api.reason_text(word, clusters[ref & mask], out_of_tree)
                hist[text] = hist.get(text, 0) + count
            out[idx] = api.fit_error_histogram_message(len(clusters), hist)
        return out

    def score(self, bindings: Sequence[dict]) -> List[List[int]]:
        """Summed plugin scores per (binding, cluster) (prioritizeClusters)."""
        b = Batch(self.snapshot, bindings)
        eng = self.snapshot.engine
        C_ = len(self.snapshot.names)
        s = (C.c_int64 * max(1, b.n * C_))()
        eng._check(eng.L.kp_score_batch(eng.h, b.h, s), "kp_score_batch")
        out = [[int(s[i * C_ + c]) for c in range(C_)] for i in range(b.n)]
        b.close()
        return out

    def max_available_component_sets(self, components: Sequence[dict], clusters: Sequence[str]) -> List[int]:
        """GeneralEstimator.MaxAvailableComponentSets (general.go:154-162) for one
        component list; raises EngineError (KP_ENOTSUP) with the gate off."""
        eng = self.snapshot.engine
        w = api.World()
        ca, nc = w.components(components)
        idx = {n: i for i, n in enumerate(self.snapshot.names)}
        ci = (C.c_uint32 * max(1, len(clusters)))(*[idx[n] for n in clusters])
        out = (C.c_int32 * max(1, len(clusters)))()
        eng._check(eng.L.kp_max_available_component_sets(eng.h, self.snapshot.h, ca, nc, ci, len(clusters), out),
                   "kp_max_available_component_sets")
        return [int(out[i]) for i in range(len(clusters))]

    def max_available_replicas(self, binding: dict, clusters: Sequence[str],
                               assumed: "Assumptions" = None) -> List[int]:
        """GeneralEstimator.MaxAvailableReplicas for one binding's request (with `assumed`: after
        the assumed workloads are deducted)."""
        b = Batch(self.snapshot, [binding], assumed=assumed)
        eng = self.snapshot.engine
        idx = {n: i for i, n in enumerate(self.snapshot.names)}
        ci = (C.c_uint32 * max(1, len(clusters)))(*[idx[n] for n in clusters])
        out = (C.c_int32 * max(1, len(clusters)))()
        eng._check(eng.L.kp_max_available_replicas(eng.h, b.h, 0, ci, len(clusters), out),
                   "kp_max_available_replicas")
        b.close()
        return [int(out[i]) for i in range(len(clusters))]
