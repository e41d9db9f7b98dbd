"""Region spread whose selection does not fit stage B's 256-item lists: a cluster
MaxGroups above 256 (selectBestClustersByRegion takes min(clusters of the selected
regions, MaxGroups) clusters with no upper bound, select_clusters_by_region.go:41-63)
and a spec.Clusters that repeats names past 256 entries. k_region_b marks such a
binding and k_region_wide schedules it with its lists in a global slot
(kp_kernels.h body_region_wide); kp_stage_times.n_region_wide counts them.

Every expected value is the oracle's on the same structs, compared for every binding.
The expected n_region_wide comes from the inputs alone: with every cluster feasible
and at least 2 x 350 (R = 2) or 3 x 140 (R = 5) clusters in the selected regions, a
binding's selection exceeds 256 exactly when its cluster MaxGroups does. StaticWeight
bindings ignore spread constraints (select_clusters.go:28-80) and never count."""
import functools
import os

import pytest

from karmada_amd import api, synth
from karmada_amd.engine import PKG, Batch, MultiBatch, MultiEngine, Snapshot
import oracle_lib as O

CPUSIM = os.path.join(PKG, "libkp_cpusim.so")
APPS = [{"groupVersion": "apps/v1", "resources": [{"kind": "Deployment"}]}]
STRATEGIES = ("Duplicated", "DynamicWeight", "Aggregated", "StaticWeight")


def scheduling(strategy):
    if strategy == "Duplicated":
        return {"replicaSchedulingType": "Duplicated"}
    if strategy == "Aggregated":
        return {"replicaSchedulingType": "Divided", "replicaDivisionPreference": "Aggregated"}
    rs = {"replicaSchedulingType": "Divided", "replicaDivisionPreference": "Weighted"}
    if strategy == "DynamicWeight":
        rs["weightPreference"] = {"dynamicWeight": "AvailableReplicas"}
    else:
        rs["weightPreference"] = {"staticWeightList": [
            {"targetCluster": {"clusterNames": ["m0001", "m0002", "m0500"]}, "weight": 3},
            {"targetCluster": {"labelSelector": {"matchLabels": {"odd": "1"}}}, "weight": 1}]}
    return rs


def binding(uid, strategy, rmin, rmax, cmax, clusters=None, cpu="1", replicas=500):
    d = {"uid": uid, "replicas": replicas, "replicaRequirements": {"resourceRequest": {"cpu": cpu}},
         "placement": {"spreadConstraints": [{"spreadByField": "region", "minGroups": rmin, "maxGroups": rmax},
                                             {"spreadByField": "cluster", "minGroups": 1, "maxGroups": cmax}],
                       "replicaScheduling": scheduling(strategy)}}
    if clusters:
        d["clusters"] = clusters
    return d


def fleet(C, region_of, tainted=lambda i: False):
    out = []
    for i in range(C):
        c = {"name": "m%04d" % i, "region": "r%d" % region_of(i), "labels": {"odd": str(i & 1)}, "apiEnablements": APPS,
             "resourceSummary": {"allocatable": {"cpu": str(4 + (7 * i) % 13), "pods": "110"}}}
        if tainted(i):
            c["taints"] = [{"key": "drain", "value": "yes", "effect": "NoSchedule"}]
        out.append(c)
    return out


class Case:
    """Packed clusters and bindings (the World keeps their memory), the oracle's results
    (computed once, shared by the host-build and GPU tests) and the expected wide count."""

    def __init__(self, clusters, bindings, n_wide):
        self.w = api.World()
        self.names = [c["name"] for c in clusters]
        self.ca, self.nc = self.w.clusters(clusters)
        self.bs, self.n = self.w.bindings(bindings)
        self.dicts = bindings
        self.opts = api.options()
        self.want = O.schedule_c(self.ca, self.nc, self.bs, self.n, self.opts, O.FAST, 1)
        self.n_wide = n_wide

    def run(self, engine):
        snap = Snapshot.from_structs(engine, self.ca, self.nc, self.names, self.opts)
        b = Batch(snap, structs=(self.bs, self.n))
        got = b.schedule()
        t = engine.stage_times()
        b.close()
        snap.close()
        return got, t

    def check(self, got):
        assert len(got) == len(self.want) == self.n
        bad = [i for i in range(self.n) if got[i] != self.want[i]]
        assert not bad, (f"{len(bad)}/{self.n} differ; first {bad[0]} ({self.dicts[bad[0]]['uid']}): "
                         f"got={str(got[bad[0]])[:400]} want={str(self.want[bad[0]])[:400]}")
        assert not [r for r in got if r["status"] == 3 and r["err"] == 0]


PREVIOUS = [{"name": "m%04d" % i, "replicas": 3} for i in (3, 10, 101, 400, 699)]


@functools.lru_cache(maxsize=None)
def boundary(R):
    """C = 700, region r{i % R}: cluster MaxGroups 8 .. 1000 around the 256-item lists, every
    strategy, with and without a previous placement."""
    rmin, rmax = (2, 2) if R == 2 else (3, 5)
    bindings, n_wide = [], 0
    for cmax in (8, 256, 257, 300, 1000):
        for strategy in STRATEGIES:
            for prev in (None, PREVIOUS):
                bindings.append(binding(f"b-{R}-{cmax}-{strategy}-{'p' if prev else 'n'}", strategy, rmin, rmax, cmax, prev))
                n_wide += 1 if cmax > 256 and strategy != "StaticWeight" else 0
    if R == 5:  # the issue's row: spec.Clusters = every second cluster of the first 600, 2 replicas each
        every2 = [{"name": "m%04d" % i, "replicas": 2} for i in range(0, 600, 2)]
        for strategy in STRATEGIES[:3]:
            bindings.append(binding(f"b-5-300-{strategy}-every2", strategy, rmin, rmax, 300, every2))
            n_wide += 1
    return Case(fleet(700, lambda i: i % R), bindings, n_wide)


def check_boundary(engine, R):
    case = boundary(R)
    got, t = case.run(engine)
    print(f"R={R}: n_region={t['n_region']} n_region_wide={t['n_region_wide']} expected {case.n_wide}")
    case.check(got)
    assert t["n_region_wide"] == case.n_wide and case.n_wide > 0
    dup = [r for r, d in zip(got, case.dicts) if "Duplicated" in d["uid"]]
    assert all(r["status"] == 0 for r in dup)
    assert max(len(r["targets"]) for r in dup) > 256


@pytest.mark.parametrize("R", [2, 5])
def test_boundary_host_build(cpusim_engine, R):
    check_boundary(cpusim_engine, R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 5])
def test_boundary_gpu(gpu_engine, R):
    check_boundary(gpu_engine, R)


@functools.lru_cache(maxsize=None)
def repeated():
    """spec.Clusters of 300 entries m{i % 280} (20 names twice) and its first 200 entries (none
    twice), 1 replica each: only the former needs the wide path."""
    bindings = []
    for cnt in (300, 200):
        prev = [{"name": "m%04d" % (i % 280), "replicas": 1} for i in range(cnt)]
        for strategy in STRATEGIES[:3]:
            bindings.append(binding(f"rep-{cnt}-{strategy}", strategy, 2, 3, 8, prev))
    return Case(fleet(700, lambda i: i % 5), bindings, 3)


def check_repeated(engine):
    case = repeated()
    got, t = case.run(engine)
    print(f"repeated: n_region={t['n_region']} n_region_wide={t['n_region_wide']}")
    case.check(got)
    assert t["n_region_wide"] == case.n_wide


def test_repeated_targets_host_build(cpusim_engine):
    check_repeated(cpusim_engine)


@pytest.mark.gpu
def test_repeated_targets_gpu(gpu_engine):
    check_repeated(gpu_engine)


def test_narrow_batch_unchanged(cpusim_engine):
    """A batch whose cluster MaxGroups stay within the lists (synthetic config 4): no binding
    is classified wide, so k_region_wide is not launched and counts nothing."""
    u = synth.Universe(4, 4, 400, 0, 300)
    opts = api.options()
    want = O.schedule_c(u.clusters, u.n_clusters, u.bindings, u.n_bindings, opts, O.FAST, 1)
    snap = Snapshot.from_structs(cpusim_engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
    got = b.schedule()
    t = cpusim_engine.stage_times()
    b.close()
    snap.close()
    assert got == want
    assert t["n_region"] > 0 and t["n_region_wide"] == 0


def region8(i):
    """Eight regions of unequal size: region k holds (k + 1) / 36 of the clusters."""
    v, k = (7 * i) % 36, 0
    while v >= k + 1:
        v -= k + 1
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def large():
    """C = 5000, 8 unequal regions, a tenth of the clusters tainted, two estimator classes,
    cluster MaxGroups on both sides of the lists and up to the whole fleet."""
    bindings = []
    for i in range(64):
        cmax = (200, 257, 1000, 5000)[i % 4]
        strategy = STRATEGIES[(i // 4) % 4]
        prev = [{"name": "m%04d" % ((13 * i + 97 * k) % 5000), "replicas": 2} for k in range(40)] if i % 3 == 0 else None
        bindings.append(binding(f"l-{i}-{cmax}-{strategy}", strategy, 2, 4, cmax, prev, cpu=str(1 + (i // 16) % 2)))
    return Case(fleet(5000, region8, lambda i: i % 10 == 3), bindings, None)


@pytest.mark.gpu
@pytest.mark.parametrize("lds_sort", [True, False], ids=["lds-sort", "slot-sort"])
def test_large_snapshot_gpu(gpu_engine, lds_sort, monkeypatch):
    """The candidate sort in LDS, and (KP_WIDE_LDS=0, read when the batch is created) in the
    global slot, where it runs whenever the keys do not fit beside the rest."""
    if not lds_sort:
        monkeypatch.setenv("KP_WIDE_LDS", "0")
    case = large()
    got, t = case.run(gpu_engine)
    print(f"large: n_region={t['n_region']} n_region_wide={t['n_region_wide']} select_kernel_ms={t['select_kernel_ms']:.3f}")
    case.check(got)
    assert t["n_region_wide"] > 0
    assert sum(1 for r in got if r["status"] == 0) > len(got) // 2


def test_multi_device_merge_host_build():
    """kp_multi over 2 emulated devices: the merged results equal the single engine's (the
    oracle's) and the shards' n_region_wide add up."""
    case = boundary(5)
    m = MultiEngine([0, 1], lib_path=CPUSIM)
    s = m.snapshot(case.ca, case.nc, case.opts)
    b = MultiBatch(s, (case.bs, case.n))
    got = b.schedule()
    wide = [m.stage_times(d)["n_region_wide"] for d in range(2)]
    b.close()
    s.close()
    m.close()
    case.check(got)
    assert sum(wide) == case.n_wide, wide
