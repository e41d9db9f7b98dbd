"""The delta result form (kp_results_delta, kp_schedule_batch_delta): the status arrays for
every binding, and indices and targets only of the bindings whose result differs from the
spec.Clusters they were packed with, as a multiset of (cluster, replicas) pairs (k_changed,
k_changed_long, the scans, k_compact over the masked counts, k_changed_list; kp_kernels.h).

The expected delta is never the engine's: it is derived here, with a sort-based multiset
compare, from the ORACLE's results and the bindings' own spec.Clusters. The engine's wide
result of the same batch is a second witness (the same flags must follow from it), and the
delta arrays must equal, element by element, what numpy selects from that wide result with
the derived flags. Each check runs on the host build and, marked gpu, on the device."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from karmada_amd import api, synth
from karmada_amd.engine import KP_ABI_VERSION, Batch, EngineError, GenericScheduler, Snapshot
import oracle_lib as O
from test_packed_results import Packed, Wide, arr

APPS = [{"groupVersion": "apps/v1", "resources": [{"kind": "Deployment"}]}]
DUP = {"replicaScheduling": {"replicaSchedulingType": "Duplicated"}}


def _s(x):
    """The bytes of a kp_str (by its length: the pointer need not be NUL-terminated)."""
    if not x.len:
        return ""
    return C.string_at(C.cast(C.byref(x), C.POINTER(C.c_void_p))[0], x.len).decode()


def prev_of(b):
    """spec.Clusters of a kp_binding: all n_clusters entries, as (name, replicas)."""
    return [(_s(b.clusters[j].name), int(b.clusters[j].replicas)) for j in range(b.n_clusters)]


def flags_from(results, prevs, names):
    """changed[b] from result dicts: OK and the (name, replicas) lists differ once sorted."""
    out = []
    for r, p in zip(results, prevs):
        got = sorted((names[i], rep) for i, rep in r["targets"])
        out.append(r["status"] == api.STATUS_OK and got != sorted(p))
    return np.array(out, dtype=bool)


class Delta:
    def __init__(self, d):
        n, k, t = d.n_bindings, d.n_changed, d.n_targets
        self.n, self.n_changed, self.n_targets, self.n_targets_all = n, k, t, d.n_targets_all
        self.status, self.err, self.arg = arr(d.status, n, np.int32), arr(d.err_code, n, np.int32), arr(d.err_arg, n, np.int64)
        self.changed = arr(d.changed, k, np.uint32)
        self.offsets = arr(d.offsets, k + 1, np.uint64)
        self.cidx, self.rep = arr(d.cluster_idx, t, np.uint32), arr(d.replicas, t, np.int32)

    def raw(self):
        return tuple(a.tobytes() for a in (self.status, self.err, self.arg, self.changed, self.offsets, self.cidx, self.rep))


def check_delta(d, w, flags):
    """Delta d against what numpy selects from the wide result w with the derived flags."""
    for a, b, what in ((d.status, w.status, "status"), (d.err, w.err, "err_code"), (d.arg, w.arg, "err_arg")):
        assert np.array_equal(a, b), what
    assert d.n == w.n and d.n_targets_all == w.n_targets
    off = w.offsets.astype(np.int64)
    cnt = np.where(flags, off[1:] - off[:-1], 0)
    want_changed = np.flatnonzero(flags).astype(np.uint32)
    assert d.n_changed == len(want_changed) and np.array_equal(d.changed, want_changed), \
        (sorted(set(d.changed.tolist()) ^ set(want_changed.tolist()))[:10])
    want_off = np.concatenate(([0], np.cumsum(cnt[flags]))).astype(np.uint64)
    assert np.array_equal(d.offsets, want_off)
    keep = np.repeat(flags, off[1:] - off[:-1])
    assert d.n_targets == int(keep.sum()) == int(want_off[-1])
    assert np.array_equal(d.cidx, w.cidx[keep]) and np.array_equal(d.rep, w.rep[keep])


def run_batch(engine, snap, structs, want, names, **kw):
    """One batch scheduled wide, then delta: checked against the oracle's `want`; returns
    (Delta, Wide, flags)."""
    ba, n = structs
    prevs = [prev_of(ba[i]) for i in range(n)]
    flags = flags_from(want, prevs, names)
    b = Batch(snap, structs=structs, **kw)
    try:
        w = Wide(b.schedule_raw())
        d = Delta(b.schedule_delta_raw())
    finally:
        b.close()
    assert w.dicts() == want  # the wide call is the oracle's, so the second witness stands on it
    assert np.array_equal(flags_from(w.dicts(), prevs, names), flags)
    check_delta(d, w, flags)
    return d, w, flags


# ---- 1: layout ---------------------------------------------------------------------------

def test_struct_layout(tmp_path):
    """The ctypes mirror of kp_results_delta has the header's layout; the ABI version stays 16."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in api.kp_results_delta._fields_]
    assert fields == ["n_bindings", "status", "err_code", "err_arg", "n_changed", "changed", "offsets", "cluster_idx",
                      "replicas", "n_targets", "n_targets_all"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kp/kp_api.h"\nint main(void) {\n'
                   '  printf("%zu\\n%d\\n", sizeof(kp_results_delta), KP_ABI_VERSION);\n' +
                   "".join(f'  printf("%zu\\n", offsetof(kp_results_delta, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(api.kp_results_delta), 16] + [getattr(api.kp_results_delta, f).offset for f in fields]
    assert KP_ABI_VERSION == 16


def test_exports(cpusim_engine):
    from karmada_amd import engine
    for name in ("kp_schedule_batch_delta", "kp_schedule_batch_submit_delta", "kp_schedule_batch_collect_delta"):
        assert name in engine.EXPORTS and hasattr(cpusim_engine.L, name)
    assert cpusim_engine.L.kp_abi_version() == 16


# ---- 2: hand-made classes ----------------------------------------------------------------

NC = 130  # two 64-cluster words and not a multiple of 64
NAMES = ["m%04d" % i for i in range(NC)]


def fleet():
    return [{"name": NAMES[i], "labels": {"g63": str(int(i < 63)), "g64": str(int(i < 64)), "g65": str(int(i < 65))},
             "apiEnablements": APPS, "resourceSummary": {"allocatable": {"cpu": "64", "pods": "110"}}}
            for i in range(NC)]


def full(rep, n=NC):
    return [{"name": NAMES[i], "replicas": rep} for i in range(n)]


def edit(lst, i, rep):
    out = [dict(t) for t in lst]
    out[i]["replicas"] = rep
    return out


def hand_bindings():
    """(uid, binding, expected changed) by name."""
    def dup(uid, rep, clusters, sel=None):
        p = dict(DUP)
        pl = {"replicaScheduling": p["replicaScheduling"]}
        if sel:
            pl["clusterAffinity"] = {"labelSelector": {"matchLabels": {sel: "1"}}}
        return {"uid": uid, "replicas": rep, "placement": pl, "clusters": clusters}
    out = [
        ("exact", dup("exact", 3, full(3)), False),
        ("reversed", dup("reversed", 3, full(3)[::-1]), False),
        ("off-by-one", dup("off-by-one", 3, edit(full(3), 77, 4)), True),
        ("missing", dup("missing", 3, full(3)[:-1]), True),
        ("extra-absent", dup("extra-absent", 3, full(3) + [{"name": "ghost", "replicas": 3}]), True),
        ("absent-for-one", dup("absent-for-one", 3, full(3)[:-1] + [{"name": "ghost", "replicas": 3}]), True),
        ("repeated", dup("repeated", 3, full(3)[:-1] + [full(3)[5]]), True),
        ("repeated-short", dup("repeated-short", 3, full(3, 63)[:-1] + [full(3)[5]], "g63"), True),
        ("empty-prev", dup("empty-prev", 3, []), True),
        ("zero-empty", {"uid": "zero-empty", "replicas": 0, "replicaRequirements": {"resourceRequest": {"cpu": "1"}},
                        "clusters": [], "placement": {"replicaScheduling": {
                            "replicaSchedulingType": "Divided", "replicaDivisionPreference": "Aggregated"}}}, False),
        ("zero-nonworkload", dup("zero-nonworkload", 0, full(0)), False),
        ("fit-error", {"uid": "fit-error", "replicas": 3, "clusters": full(3, 4), "placement": {
            "replicaScheduling": DUP["replicaScheduling"], "clusterAffinity": {"clusterNames": ["nowhere"]}}}, False),
        ("r65535", dup("r65535", 65535, full(65535)), False),
        ("r65535-vs-65534", dup("r65535-vs-65534", 65535, edit(full(65535), 129, 65534)), True),
        ("rmax", dup("rmax", 2147483647, full(2147483647)), False),
        ("rmax-vs-minus-one", dup("rmax-vs-minus-one", 2147483647, edit(full(2147483647), 0, -1)), True),
        ("minus-one", dup("minus-one", 3, edit(full(3), 64, -1)), True),
        ("int-min", dup("int-min", 3, edit(full(3), 63, -2147483648)), True),
        ("minus-one-short", dup("minus-one-short", 3, edit(full(3, 63), 10, -1), "g63"), True),
        ("int-min-short", dup("int-min-short", 3, edit(full(3, 64), 63, -2147483648), "g64"), True),
    ]
    for n in (63, 64, 65):  # on each side of the wave's 64 lanes: k_changed / k_changed_long
        out.append((f"sel{n}", dup(f"sel{n}", 7, full(7, n), f"g{n}"), False))
        out.append((f"sel{n}-last", dup(f"sel{n}-last", 7, edit(full(7, n), n - 1, 8), f"g{n}"), True))
        out.append((f"sel{n}-reversed", dup(f"sel{n}-reversed", 7, full(7, n)[::-1], f"g{n}"), False))
    return out


class Hand:
    def __init__(self, clusters, bindings, opts=None):
        self.w = api.World()
        self.names = [c["name"] for c in clusters]
        self.ca, self.nc = self.w.clusters(clusters)
        self.bs, self.n = self.w.bindings(bindings)
        self.opts = opts or api.options()
        self.want = O.schedule_c(self.ca, self.nc, self.bs, self.n, self.opts, O.FAST, 1)

    def run(self, engine):
        snap = Snapshot.from_structs(engine, self.ca, self.nc, self.names, self.opts)
        try:
            return run_batch(engine, snap, (self.bs, self.n), self.want, self.names)
        finally:
            snap.close()


@functools.lru_cache(maxsize=None)
def hand():
    hb = hand_bindings()
    return hb, Hand(fleet(), [b for _, b, _ in hb])


def check_hand(engine):
    hb, case = hand()
    by = {uid: i for i, (uid, _, _) in enumerate(hb)}
    want = case.want
    assert want[by["exact"]]["targets"] == [(i, 3) for i in range(NC)]
    assert want[by["zero-empty"]] == {"status": 0, "err": 0, "arg": 0, "targets": []}
    assert want[by["fit-error"]]["status"] == api.STATUS_FIT_ERROR
    assert len(want[by["sel63"]]["targets"]) == 63 and len(want[by["sel65"]]["targets"]) == 65
    d, w, flags = case.run(engine)
    got = set(d.changed.tolist())
    for uid, _, changed in hb:
        assert flags[by[uid]] == changed, f"{uid}: derived from the oracle"
        assert (by[uid] in got) == changed, f"{uid}: the engine"
    assert d.status[by["fit-error"]] == api.STATUS_FIT_ERROR and by["fit-error"] not in got
    print(f"hand-made: {d.n_changed} changed / {d.n - d.n_changed} not listed, {d.n_targets} of {d.n_targets_all} targets")


def test_hand_made_host_build(cpusim_engine):
    check_hand(cpusim_engine)


@pytest.mark.gpu
def test_hand_made_gpu(gpu_engine):
    check_hand(gpu_engine)


def check_zero_replica_entries(engine):
    """enable_empty_workload_propagation keeps replicas-0 entries in a result: a spec.Clusters
    of zeros equals it, and a zero against a three does not (0 is no sentinel)."""
    zeros = full(0)
    bs = [{"uid": "z-same", "replicas": 0, "placement": DUP, "clusters": zeros},
          {"uid": "z-one-three", "replicas": 0, "placement": DUP, "clusters": edit(zeros, 100, 3)},
          {"uid": "three-one-zero", "replicas": 3, "placement": DUP, "clusters": edit(full(3), 100, 0)}]
    case = Hand(fleet(), bs, api.options(empty_workload_propagation=True))
    assert case.want[0]["targets"] == [(i, 0) for i in range(NC)]
    d, w, flags = case.run(engine)
    assert flags.tolist() == [False, True, True] and d.changed.tolist() == [1, 2]


def test_zero_replica_entries_host_build(cpusim_engine):
    check_zero_replica_entries(cpusim_engine)


@pytest.mark.gpu
def test_zero_replica_entries_gpu(gpu_engine):
    check_zero_replica_entries(gpu_engine)


# ---- 3: two cycles -----------------------------------------------------------------------

def cycle_bindings():
    req = {"resourceRequest": {"cpu": "1"}}
    div = lambda pref, extra=None: {"replicaScheduling": dict({"replicaSchedulingType": "Divided",  # noqa: E731
                                                                "replicaDivisionPreference": pref}, **(extra or {}))}
    dyn = div("Weighted", {"weightPreference": {"dynamicWeight": "AvailableReplicas"}})
    sw = div("Weighted", {"weightPreference": {"staticWeightList": [
        {"targetCluster": {"labelSelector": {"matchLabels": {"g63": "1"}}}, "weight": 3},
        {"targetCluster": {"labelSelector": {"matchLabels": {"g63": "0"}}}, "weight": 1}]}})
    out = []
    for i in range(10):
        out.append({"uid": f"dyn-{i}", "replicas": 40 + 7 * i, "replicaRequirements": req, "placement": dyn})
        out.append({"uid": f"agg-{i}", "replicas": 90 + 11 * i, "replicaRequirements": req, "placement": div("Aggregated")})
        out.append({"uid": f"sw-{i}", "replicas": 200 + 13 * i, "replicaRequirements": req, "placement": sw})
        out.append({"uid": f"dup-{i}", "replicas": 1 + i, "placement": DUP})
    return out


@functools.lru_cache(maxsize=None)
def cycles():
    """Cycle one's oracle results become cycle two's spec.Clusters; every third binding then
    asks for more replicas (a known perturbed subset)."""
    first = Hand(fleet(), cycle_bindings())
    assert all(r["status"] == 0 and r["targets"] for r in first.want)
    second, perturbed = [], []
    for i, (b, r) in enumerate(zip(cycle_bindings(), first.want)):
        b = dict(b, clusters=[{"name": NAMES[c], "replicas": rep} for c, rep in r["targets"]])
        if i % 3 == 0:
            b["replicas"] += 5
            perturbed.append(i)
        second.append(b)
    return first, Hand(fleet(), second), perturbed


def check_cycles(engine):
    first, second, perturbed = cycles()
    snap = Snapshot.from_structs(engine, first.ca, first.nc, first.names, first.opts)
    try:
        b = Batch(snap, structs=(first.bs, first.n))
        assert b.schedule() == first.want  # cycle one: plain kp_schedule_batch
        b.close()
        d, w, flags = run_batch(engine, snap, (second.bs, second.n), second.want, second.names)
    finally:
        snap.close()
    changed = set(np.flatnonzero(flags).tolist())
    print(f"two cycles: {len(changed)} changed of {second.n}, {len(changed & set(perturbed))} of {len(perturbed)} perturbed")
    assert 0 < d.n_changed < d.n
    assert changed & set(perturbed) and set(range(second.n)) - changed - set(perturbed)
    assert changed <= set(perturbed)  # an unperturbed binding keeps the placement it holds


def test_two_cycles_host_build(cpusim_engine):
    check_cycles(cpusim_engine)


@pytest.mark.gpu
def test_two_cycles_gpu(gpu_engine):
    check_cycles(gpu_engine)


# ---- 4: synthetic universes --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def universe(config, seed, C_, n, multi=False):
    u = synth.Universe(config, seed, C_, 0, n)
    opts = api.options(multi_templates=True) if multi else api.options()
    want = O.schedule_c(u.clusters, u.n_clusters, u.bindings, u.n_bindings, opts, O.FAST, 8)
    return u, opts, want


def check_synth(engine, key):
    u, opts, want = universe(*key)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    try:
        d, w, flags = run_batch(engine, snap, u.binding_slice(0, u.n_bindings), want, u.names)
    finally:
        snap.close()
    ok = w.status == api.STATUS_OK
    with_prev = sum(1 for i in range(u.n_bindings) if u.bindings[i].n_clusters)
    print(f"config {key[0]}: {d.n_changed} changed, {int((ok & ~flags).sum())} unchanged, {int((~ok).sum())} not OK; "
          f"{with_prev} hold a spec.Clusters; {d.n_targets} of {d.n_targets_all} targets")
    return d, flags, ok


SYNTH = [(3, 5, 300, 512), (4, 5, 300, 512), (5, 5, 400, 512), (9, 1, 300, 512, True), (6, 5, 150, 512), (8, 5, 64, 512)]
SYNTH_IDS = ["config3", "config4", "config5", "config9-multi", "config6", "config8"]


@pytest.mark.parametrize("key", SYNTH, ids=SYNTH_IDS)
def test_synthetic_host_build(cpusim_engine, key):
    check_synth(cpusim_engine, key)


@pytest.mark.gpu
@pytest.mark.parametrize("key", SYNTH, ids=SYNTH_IDS)
def test_synthetic_gpu(gpu_engine, key):
    check_synth(gpu_engine, key)


@functools.lru_cache(maxsize=None)
def settled(config, seed, C_, n):
    """The universe's bindings with spec.Clusters set to the oracle's results (a fleet at
    rest), every fifth binding's first entry then off by one: long and short lists on both
    sides, most bindings unchanged. The oracle schedules the rewritten bindings again."""
    u, opts, first = universe(config, seed, C_, n)
    ba = (api.kp_binding * n)()
    keep, perturbed = [], []
    for i in range(n):
        ba[i] = u.bindings[i]
        tg = [api.kp_target_cluster(u.clusters[c].name, rep) for c, rep in first[i]["targets"]]
        if tg and i % 5 == 0:
            tg[0].replicas += 1
            perturbed.append(i)
        a = (api.kp_target_cluster * max(1, len(tg)))(*tg)
        keep.append(a)
        ba[i].clusters, ba[i].n_clusters = a, len(tg)
    want = O.schedule_c(u.clusters, u.n_clusters, ba, n, opts, O.FAST, 8)
    return u, opts, ba, keep, want, perturbed


def check_settled(engine, key):
    u, opts, ba, _, want, perturbed = settled(*key)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    try:
        d, w, flags = run_batch(engine, snap, (ba, key[3]), want, u.names)
    finally:
        snap.close()
    ok = w.status == api.STATUS_OK
    long_lists = sum(1 for i in range(key[3]) if ba[i].n_clusters > 64)
    print(f"settled config {key[0]}: {d.n_changed} changed, {int((ok & ~flags).sum())} unchanged, "
          f"{long_lists} lists past 64 entries, {d.n_targets} of {d.n_targets_all} targets")
    assert 0 < d.n_changed and int((ok & ~flags).sum()) > 0
    assert long_lists > 0 or key[0] != 3  # (config 4's spread constraints keep its lists short)


@pytest.mark.parametrize("key", [(3, 5, 300, 512), (4, 5, 300, 512)], ids=["config3", "config4"])
def test_settled_fleet_host_build(cpusim_engine, key):
    check_settled(cpusim_engine, key)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(3, 5, 300, 512), (4, 5, 300, 512)], ids=["config3", "config4"])
def test_settled_fleet_gpu(gpu_engine, key):
    check_settled(gpu_engine, key)


def check_filters(engine):
    """A batch of kp_batch_create_filters: its rows are honoured by the delta call (the oracle
    sees them as evictions, as tests/test_extra_filters.py does)."""
    import test_extra_filters as TF
    u, opts, _ = universe(3, 5, 300, 512)
    ba, n = u.binding_slice(0, u.n_bindings)
    ok, row_of = TF.make_rows(7, u, ba, n)
    want = TF.expected(u, ba, n, opts, ok, row_of)
    plain = universe(3, 5, 300, 512)[2]
    assert want != plain  # the rows decide something
    snap = TF.snap_for(engine, u, opts, 1)
    try:
        d, w, flags = run_batch(engine, snap, (ba, n), want, u.names, filters=(ok, row_of, 1))
        # the out-of-tree refusal applies unchanged: a batch without answers, one plugin registered
        b = Batch(snap, structs=(ba, n))
        with pytest.raises(EngineError, match="rc=-4"):
            b.schedule_delta_raw()
        b.close()
    finally:
        snap.close()
    print(f"filter rows: {d.n_changed} changed of {d.n}")


def test_filter_rows_host_build(cpusim_engine):
    check_filters(cpusim_engine)


@pytest.mark.gpu
def test_filter_rows_gpu(gpu_engine):
    check_filters(gpu_engine)


def test_sets_overflow_host_build(cpusim_engine, monkeypatch):
    """KP_ERR_SETS_CAPACITY (forced by KP_SETS_RUNS_CAP=1) is set by the host after the device
    compared: the failed bindings leave the changed list and n_targets_all, as they leave the
    wide CSR."""
    monkeypatch.setenv("KP_SETS_RUNS_CAP", "1")
    u, opts, want = universe(9, 1, 300, 600, True)
    snap = Snapshot.from_structs(cpusim_engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
    try:
        w = Wide(b.schedule_raw())
        d = Delta(b.schedule_delta_raw())
    finally:
        b.close()
        snap.close()
    failed = np.flatnonzero(w.err == 15)
    assert len(failed) and any(want[i]["targets"] for i in failed)
    prevs = [prev_of(u.bindings[i]) for i in range(u.n_bindings)]
    kept = [i for i in range(u.n_bindings) if i not in set(failed.tolist())]
    assert [w.dicts()[i] for i in kept] == [want[i] for i in kept]
    for i in failed:
        want[i] = dict(want[i], status=api.STATUS_ERROR, targets=[])
    check_delta(d, w, flags_from(want, prevs, u.names))


# ---- 5: the LDS table at the documented ceilings -----------------------------------------

@functools.lru_cache(maxsize=None)
def ceiling(config, C_):
    """The config's first bindings (a spread binding among config 4's) and a Duplicated pair
    whose spec.Clusters is the oracle's fleet-wide result, once matching and once with its
    last entry off by one."""
    u = synth.Universe(config, 5, C_, 0, 6)
    opts = api.options()
    w = api.World()
    one, _ = w.bindings([{"uid": "fleet", "replicas": 2, "placement": DUP}])
    first = O.schedule_c(u.clusters, u.n_clusters, one, 1, opts, O.FAST, 1)[0]
    # (the table is indexed by cluster rank, so its carve is past 64 KB whatever the list's
    # length: the list must only reach the ranks up there)
    assert first["status"] == 0 and len(first["targets"]) > 8192 and first["targets"][-1][0] > (C_ * 15) // 16
    tg = [{"name": u.names[c], "replicas": rep} for c, rep in first["targets"]]
    pair, _ = w.bindings([{"uid": "fleet-same", "replicas": 2, "placement": DUP, "clusters": tg[::-1]},
                          {"uid": "fleet-last", "replicas": 2, "placement": DUP, "clusters": edit(tg, len(tg) - 1, 3)}])
    n = u.n_bindings + 2
    ba = (api.kp_binding * n)()
    for i in range(u.n_bindings):
        ba[i] = u.bindings[i]
    ba[n - 2], ba[n - 1] = pair[0], pair[1]
    want = O.schedule_c(u.clusters, u.n_clusters, ba, n, opts, O.FAST, 4)
    return u, opts, w, ba, n, want


def check_ceiling(engine, config, C_):
    u, opts, _, ba, n, want = ceiling(config, C_)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    try:
        d, w, flags = run_batch(engine, snap, (ba, n), want, u.names)
    finally:
        snap.close()
    assert not flags[n - 2] and flags[n - 1]
    assert (n - 1) in d.changed.tolist() and (n - 2) not in d.changed.tolist()


@pytest.mark.parametrize("config,C_", [(3, 18624), (4, 14336)], ids=["18624", "14336-spread"])
def test_ceiling_host_build(cpusim_engine, config, C_):
    if config == 4:
        u = ceiling(config, C_)[0]
        assert any(u.bindings[i].n_spread_constraints for i in range(u.n_bindings))
    check_ceiling(cpusim_engine, config, C_)


@pytest.mark.gpu
def test_ceiling_gpu(gpu_engine):
    check_ceiling(gpu_engine, 3, 18624)


# ---- 6: call forms -----------------------------------------------------------------------

def check_call_forms(engine):
    u, opts, ba, _, want, _ = settled(3, 5, 300, 512)
    n = 512
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=(ba, n))
    fresh = Batch(snap, structs=(ba, n))  # never sees a delta call
    try:
        digest = b.digest()
        one = Delta(b.schedule_delta_raw())
        assert 0 < one.n_changed < n
        b.submit_delta()
        with pytest.raises(EngineError, match="rc=-5"):
            b.collect()
        with pytest.raises(EngineError, match="rc=-5"):
            b.collect_packed()
        for again in (b.submit, b.submit_packed, b.submit_delta):
            with pytest.raises(EngineError, match="rc=-5"):
                again()
        assert Delta(b.collect_delta()).raw() == one.raw()
        with pytest.raises(EngineError, match="rc=-5"):
            b.collect_delta()  # nothing submitted
        b.submit()
        with pytest.raises(EngineError, match="rc=-5"):
            b.collect_delta()
        w = Wide(b.collect())
        p = Packed(b, b.schedule_packed_raw())
        fw = Wide(fresh.schedule_raw())
        fp = Packed(fresh, fresh.schedule_packed_raw())
        for a, c in ((w.status, fw.status), (w.err, fw.err), (w.arg, fw.arg), (w.offsets, fw.offsets), (w.cidx, fw.cidx),
                     (w.rep, fw.rep)):
            assert np.array_equal(a, c)
        assert p.raw() == fp.raw() and np.array_equal(p.offsets, fp.offsets)
        assert Delta(b.schedule_delta_raw()).raw() == one.raw()  # and back again
        assert b.digest() == digest == fresh.digest()
        engine.set_profile(True)
        try:
            for half in (b.submit_delta, b.collect_delta):
                with pytest.raises(EngineError, match="rc=-1"):
                    half()
            assert Delta(b.schedule_delta_raw()).raw() == one.raw()
            kt = engine.kernel_times()
            assert kt["k_changed"]["launches"] == 1 and kt["k_changed"]["units"] == n
            assert kt["k_changed_long"]["launches"] == 1 and kt["k_changed_list"]["launches"] == 1
            fresh.schedule_raw()
            assert not any(k.startswith("k_changed") for k in engine.kernel_times())
        finally:
            engine.set_profile(False)
        # the empty batch
        e = Batch(snap, structs=(ba, 0))
        r = e.schedule_delta_raw()
        assert (r.n_bindings, r.n_changed, r.n_targets, r.n_targets_all, r.offsets[0]) == (0, 0, 0, 0, 0)
        e.submit_delta()
        assert e.collect_delta().n_changed == 0
        e.close()
        b.submit_delta()  # destroyed with a delta call in flight: the batch waits for it
    finally:
        b.close()
        fresh.close()
        snap.close()


def test_call_forms_host_build(cpusim_engine):
    check_call_forms(cpusim_engine)


@pytest.mark.gpu
def test_call_forms_gpu(gpu_engine):
    check_call_forms(gpu_engine)


def check_python_forms(engine):
    """Batch.schedule_delta, GenericScheduler.schedule_changed and fit_diagnosis after a delta call."""
    hb, case = hand()
    bindings = [b for _, b, _ in hb]
    want_changed = [i for i, (_, _, c) in enumerate(hb) if c]
    gs = GenericScheduler(engine, fleet())
    res, changed = gs.schedule_changed(bindings)
    assert changed == want_changed
    for i, (r, o) in enumerate(zip(res, case.want)):
        assert (r.status, r.err, r.arg) == (o["status"], o["err"], o["arg"])
        got = sorted((NAMES.index(t.name), t.replicas) for t in r.suggested_clusters)
        assert got == (o["targets"] if i in changed else [])
    b = Batch(gs.snapshot, bindings)
    try:
        st, delta = b.schedule_delta()
        assert sorted(delta) == want_changed and all(delta[i] == case.want[i] for i in delta)
        assert st == [(o["status"], o["err"], o["arg"]) for o in case.want]
        after_delta = b.fit_diagnosis()  # "the last completed schedule call" is the delta call
        b.schedule_raw()
        assert after_delta == b.fit_diagnosis()
        assert [d[0] for d in after_delta] == [i for i, o in enumerate(case.want) if o["status"] == api.STATUS_FIT_ERROR]
    finally:
        b.close()
        gs.snapshot.close()
    errs = GenericScheduler(engine, fleet())
    try:
        assert list(errs.fit_errors(bindings, fleet())) == [d[0] for d in after_delta]
    finally:
        errs.snapshot.close()


def test_python_forms_host_build(cpusim_engine):
    check_python_forms(cpusim_engine)


@pytest.mark.gpu
def test_python_forms_gpu(gpu_engine):
    check_python_forms(gpu_engine)
