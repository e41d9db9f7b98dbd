"""The packed result form (kp_results_packed, kp_schedule_batch_packed): 4 bytes per
target, the caller's cluster index in bits [15:0] and the replicas in bits [31:16], with
0xFFFF there for replicas outside 0..65534, whose values stand in wide_replicas in entry
order (k_pack, the scan of the escape counts, k_pack_wide; kp_kernels.h).

Every comparison is element by element, in order. The per-binding arrays and the arrays
kp_results_unpack expands equal kp_schedule_batch's on the same batch; targets, n_wide,
wide_replicas and wide_offsets equal what numpy derives from that wide result; the decoded
dicts equal the oracle's. Each check runs on the host build and, marked gpu, on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

from karmada_amd import api, synth
from karmada_amd.engine import Batch, EngineError, Snapshot
import oracle_lib as O

APPS = [{"groupVersion": "apps/v1", "resources": [{"kind": "Deployment"}]}]
ESC = 0xFFFF


def arr(ptr, n, dtype):
    """A copy of n entries behind a ctypes pointer (engine-owned until the next call)."""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class Wide:
    def __init__(self, r):
        n, t = r.n_bindings, r.n_targets
        self.n, self.n_targets = n, t
        self.status, self.err, self.arg = arr(r.status, n, np.int32), arr(r.err_code, n, np.int32), arr(r.err_arg, n, np.int64)
        self.offsets = arr(r.offsets, n + 1, np.uint64)
        self.cidx, self.rep = arr(r.cluster_idx, t, np.uint32), arr(r.replicas, t, np.int32)

    def dicts(self):
        return api.results_to_python(self.status, self.err, self.arg, [int(x) for x in self.offsets], self.cidx, self.rep, self.n)


class Packed:
    def __init__(self, batch, p):
        n, t = p.n_bindings, p.n_targets
        self.n, self.n_targets, self.n_wide = n, t, p.n_wide
        self.status, self.err, self.arg = arr(p.status, n, np.int32), arr(p.err_code, n, np.int32), arr(p.err_arg, n, np.int64)
        self.offsets = arr(p.offsets, n + 1, np.uint64)
        self.targets = arr(p.targets, t, np.uint32)
        self.wide_replicas = arr(p.wide_replicas, p.n_wide, np.int32)
        self.wide_offsets = arr(p.wide_offsets, n + 1, np.uint64) if p.wide_offsets else None
        ci, rep = batch.unpack(p)  # kp_results_unpack, the decoder's definition
        self.cidx = np.frombuffer(ci, dtype=np.uint32)[:t].copy()
        self.rep = np.frombuffer(rep, dtype=np.int32)[:t].copy()

    def raw(self):
        wo = self.wide_offsets if self.wide_offsets is not None else np.zeros(0, np.uint64)
        return self.targets.tobytes(), self.wide_replicas.tobytes(), wo.tobytes()


def escaped(rep):
    return (rep < 0) | (rep >= 65535)


def in_cluster_order(r):
    """(cluster_idx, replicas) with each binding's entries sorted: the result as a set per binding."""
    owner = np.repeat(np.arange(r.n), np.diff(r.offsets.astype(np.int64)))
    order = np.lexsort((r.rep, r.cidx, owner))
    return r.cidx[order], r.rep[order]


def check_same(p, w):
    """Packed p against the wide result w of the same batch; returns the escape mask."""
    assert p.n == w.n and p.n_targets == w.n_targets
    if p.cidx.shape == w.cidx.shape and np.array_equal(p.offsets, w.offsets):  # figures first, then the assertions
        moved = int(((p.cidx != w.cidx) | (p.rep != w.rep)).sum())
        same_sets = all(np.array_equal(a, b) for a, b in zip(in_cluster_order(p), in_cluster_order(w)))
        print(f"packed vs wide: {p.n_targets} entries, {moved} differ in place, equal as per-binding sets: {same_sets}")
    for a, b, what in ((p.status, w.status, "status"), (p.err, w.err, "err_code"), (p.arg, w.arg, "err_arg"),
                       (p.offsets, w.offsets, "offsets"), (p.cidx, w.cidx, "cluster_idx"), (p.rep, w.rep, "replicas")):
        assert a.shape == b.shape and np.array_equal(a, b), (what, np.flatnonzero(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))
    esc = escaped(w.rep)
    assert p.n_wide == int(esc.sum())
    hi = np.where(esc, ESC, w.rep.astype(np.int64)).astype(np.uint32)
    assert np.array_equal(p.targets, (w.cidx & 0xFFFF) | (hi << 16))
    assert np.array_equal(p.wide_replicas, w.rep[esc])
    want_wo = np.concatenate(([0], np.cumsum(esc)))[w.offsets.astype(np.int64)].astype(np.uint64)
    if p.wide_offsets is None:
        assert p.n_wide == 0
    else:
        assert np.array_equal(p.wide_offsets, want_wo)
    return esc


def both(batch):
    """(Packed, Wide) of one batch: the wide call first, copied before the packed call reuses its buffers."""
    w = Wide(batch.schedule_raw())
    p = Packed(batch, batch.schedule_packed_raw())
    return p, w


def mixed_bindings(w, esc):
    """Bindings whose list holds escaped and unescaped entries."""
    cs = np.concatenate(([0], np.cumsum(esc)))
    off = w.offsets.astype(np.int64)
    ne = cs[off[1:]] - cs[off[:-1]]
    cnt = off[1:] - off[:-1]
    return int(((ne > 0) & (ne < cnt)).sum())


def test_struct_layout(tmp_path):
    """The ctypes mirror of kp_results_packed has the header's layout (host compiler)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in api.kp_results_packed._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kp/kp_api.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(kp_results_packed));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(kp_results_packed, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(api.kp_results_packed)] + [getattr(api.kp_results_packed, f).offset for f in fields]


# ---- 1, 2: hand-made fleets --------------------------------------------------------------

def fleet(C_):
    return [{"name": "m%04d" % i, "labels": {"odd": str(i & 1)}, "apiEnablements": APPS,
             "resourceSummary": {"allocatable": {"cpu": "64", "pods": "110"}}} for i in range(C_)]


class Case:
    """Packed clusters and bindings (the World keeps their memory) and the oracle's results,
    computed once and shared by the host-build and GPU tests."""

    def __init__(self, clusters, bindings):
        self.w = api.World()
        self.names = [c["name"] for c in clusters]
        self.ca, self.nc = self.w.clusters(clusters)
        self.bs, self.n = self.w.bindings(bindings)
        self.opts = api.options()
        self.want = O.schedule_c(self.ca, self.nc, self.bs, self.n, self.opts, O.FAST, 1)

    def run(self, engine):
        snap = Snapshot.from_structs(engine, self.ca, self.nc, self.names, self.opts)
        b = Batch(snap, structs=(self.bs, self.n))
        try:
            p, w = both(b)
            esc = check_same(p, w)
            assert Wide.dicts(p) == self.want
            assert b.schedule(packed=True) == self.want
        finally:
            b.close()
            snap.close()
        return p, w, esc


BOUNDARY = (0, 1, 65534, 65535, 65536, 2147483647)


@functools.lru_cache(maxsize=None)
def boundary():
    return Case(fleet(130), [{"uid": f"dup-{r}", "replicas": r,
                              "placement": {"replicaScheduling": {"replicaSchedulingType": "Duplicated"}}} for r in BOUNDARY])


def check_boundary(engine):
    case = boundary()
    for r, want in zip(BOUNDARY, case.want):  # every cluster is a target with spec.Replicas
        assert want["status"] == 0 and want["targets"] == [(i, r) for i in range(130)], r
    p, w, esc = case.run(engine)
    off = w.offsets.astype(np.int64)
    per = [int(esc[off[i]:off[i + 1]].sum()) for i in range(len(BOUNDARY))]
    assert per == [0, 0, 0, 130, 130, 130]
    assert p.n_wide == 390
    assert list(np.diff(p.wide_offsets.astype(np.int64))) == per
    i = BOUNDARY.index(65535)
    assert np.all(p.targets[off[i]:off[i + 1]] >> 16 == ESC) and np.all(p.rep[off[i]:off[i + 1]] == 65535)
    i = BOUNDARY.index(65534)
    assert np.all(p.targets[off[i]:off[i + 1]] >> 16 == 65534)


def test_escape_boundary_host_build(cpusim_engine):
    check_boundary(cpusim_engine)


@pytest.mark.gpu
def test_escape_boundary_gpu(gpu_engine):
    check_boundary(gpu_engine)


HEAVY = (5, 70, 100, 150, 199)


@functools.lru_cache(maxsize=None)
def mixed():
    """StaticWeight over 200 clusters, five of them (spread through the name order) at weight
    1000 and the rest at 1, a million replicas: 192 each for the light ones, about 192 000 for
    the heavy ones."""
    sw = [{"targetCluster": {"clusterNames": ["m%04d" % i for i in HEAVY]}, "weight": 1000},
          {"targetCluster": {"labelSelector": {"matchLabels": {"odd": "0"}}}, "weight": 1},
          {"targetCluster": {"labelSelector": {"matchLabels": {"odd": "1"}}}, "weight": 1}]
    return Case(fleet(200), [{"uid": "static-mixed", "replicas": 1000000, "placement": {"replicaScheduling": {
        "replicaSchedulingType": "Divided", "replicaDivisionPreference": "Weighted",
        "weightPreference": {"staticWeightList": sw}}}}])


def chunks_mixed(rep):
    """64-entry chunks of a list that hold escaped and unescaped entries."""
    esc = escaped(np.asarray(rep, dtype=np.int64))
    return [k for k in range(0, len(esc), 64) if esc[k:k + 64].any() and not esc[k:k + 64].all()]


def check_mixed(engine):
    case = mixed()
    want = case.want[0]
    assert want["status"] == 0 and len(want["targets"]) > 128
    assert len(chunks_mixed([r for _, r in want["targets"]])) >= 2  # (the oracle's list, in cluster order)
    p, w, esc = case.run(engine)
    assert len(chunks_mixed(w.rep)) >= 2  # and the engine's, in its entry order
    assert p.n_wide == len(HEAVY)


def test_mixed_list_host_build(cpusim_engine):
    check_mixed(cpusim_engine)


@pytest.mark.gpu
def test_mixed_list_gpu(gpu_engine):
    check_mixed(gpu_engine)


# ---- 3, 4, 7: synthetic universes --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def universe(config, seed, C_, n, multi=False):
    u = synth.Universe(config, seed, C_, 0, n)
    opts = api.options(multi_templates=True) if multi else api.options()
    want = O.schedule_c(u.clusters, u.n_clusters, u.bindings, u.n_bindings, opts, O.FAST, 8)
    return u, opts, want


def run_universe(engine, key):
    u, opts, want = universe(*key)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
    try:
        p, w = both(b)
    finally:
        b.close()
        snap.close()
    esc = check_same(p, w)
    return p, w, esc, Wide.dicts(p), want


def check_synth(engine, key, wide, mixed_min=0):
    p, w, esc, dicts, want = run_universe(engine, key)
    assert dicts == want
    print(f"config {key[0]}: targets {p.n_targets} escaped {p.n_wide} mixed bindings {mixed_bindings(w, esc)} "
          f"longest list {int(np.diff(w.offsets.astype(np.int64)).max())}")
    if wide:
        assert p.n_wide > 0 and mixed_bindings(w, esc) >= mixed_min
    else:
        assert p.n_wide == 0
        assert p.wide_offsets is None or not p.wide_offsets.any()
    return p, w


@pytest.mark.parametrize("key,wide,mixed_min", [((8, 5, 300, 600), True, 1), ((7, 5, 300, 300), True, 1),
                                                ((6, 5, 150, 800), False, 0), ((3, 5, 400, 1500), False, 0)],
                         ids=["config8", "config7", "config6", "config3"])
def test_synthetic_host_build(cpusim_engine, key, wide, mixed_min):
    p, w = check_synth(cpusim_engine, key, wide, mixed_min)
    if key[0] == 6:  # zero-replica targets stay unescaped; fit errors and other errors beside the results
        assert int((w.rep == 0).sum()) > 0
        assert {0, 1} < set(w.status.tolist()) and len(set(w.err.tolist())) > 3


@pytest.mark.gpu
@pytest.mark.parametrize("key,wide", [((8, 5, 5000, 4000), True), ((3, 5, 5000, 4000), False)], ids=["config8", "config3"])
def test_synthetic_gpu(gpu_engine, key, wide):
    """The packed call against a separate kp_schedule_batch call, entry by entry, in order.

    Two calls emit a binding's targets in the same order only because the multi-wave select
    kernels fill their party lists in thread order (GpuBlk::wave_reserve, kp_blk.h). While
    the waves reserved their places as they finished, config 3 at this size had 8 852 to
    12 734 of its 210 331 entries in other places from one call to the next (every binding
    equal as a set). test_synthetic_sets_gpu checks the same data as sets."""
    check_synth(gpu_engine, key, wide, 1 if wide else 0)


@pytest.mark.gpu
def test_synthetic_sets_gpu(gpu_engine):
    """Config 3 on the device with each binding's targets compared as a set: the packed call
    against the wide call and the oracle, and the packed arrays against their own expansion."""
    u, opts, want = universe(3, 5, 5000, 4000)
    snap = Snapshot.from_structs(gpu_engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
    try:
        p, w = both(b)
    finally:
        b.close()
        snap.close()
    for a, c in ((p.status, w.status), (p.err, w.err), (p.arg, w.arg), (p.offsets, w.offsets)):
        assert np.array_equal(a, c)
    for a, c in zip(in_cluster_order(p), in_cluster_order(w)):
        assert np.array_equal(a, c)
    assert Wide.dicts(p) == want
    check_same(p, p)  # targets, n_wide, wide_replicas and wide_offsets follow from the expanded arrays
    assert p.n_wide == 0


def test_sets_overflow_repack_host_build(cpusim_engine, monkeypatch):
    """KP_ERR_SETS_CAPACITY (a component-set simulation outgrowing its node runs, forced by
    KP_SETS_RUNS_CAP=1): the host drops the affected bindings' packed words and escaped
    values and renumbers both offset arrays, as it re-packs the wide CSR."""
    monkeypatch.setenv("KP_SETS_RUNS_CAP", "1")
    p, w, esc, dicts, want = run_universe(cpusim_engine, (9, 1, 300, 600, True))
    failed = [i for i, g in enumerate(dicts) if g["err"] == 15]
    assert failed and len(failed) < len(dicts)
    for i in failed:
        assert dicts[i]["status"] == api.STATUS_ERROR and dicts[i]["targets"] == []
    keep = [i for i in range(len(dicts)) if dicts[i]["err"] != 15]
    assert [dicts[i] for i in keep] == [want[i] for i in keep]
    assert any(want[i]["targets"] for i in failed)  # the re-pack dropped something


def check_per_binding(engine, key):
    """Each binding decoded alone from offsets[b] and wide_offsets[b], without the helper."""
    u, opts, _ = universe(*key)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
    try:
        w = Wide(b.schedule_raw())
        r = b.schedule_packed_raw()
        n = r.n_bindings
        off, tg = arr(r.offsets, n + 1, np.int64), arr(r.targets, r.n_targets, np.uint32)
        assert r.n_wide > 0
        wo, wr = arr(r.wide_offsets, n + 1, np.int64), arr(r.wide_replicas, r.n_wide, np.int32)
    finally:
        b.close()
        snap.close()
    assert np.array_equal(off, w.offsets.astype(np.int64))
    for i in range(n):
        words = tg[off[i]:off[i + 1]]
        hi = words >> 16
        rep = hi.astype(np.int32)
        is_esc = hi == ESC
        assert wo[i + 1] - wo[i] == int(is_esc.sum()), i
        rep[is_esc] = wr[wo[i]:wo[i + 1]]
        assert np.array_equal(words & 0xFFFF, w.cidx[off[i]:off[i + 1]]), i
        assert np.array_equal(rep, w.rep[off[i]:off[i + 1]]), i


def test_per_binding_decode_host_build(cpusim_engine):
    check_per_binding(cpusim_engine, (8, 5, 300, 600))


@pytest.mark.gpu
def test_per_binding_decode_gpu(gpu_engine):
    check_per_binding(gpu_engine, (8, 5, 5000, 4000))


def check_determinism(engine, key):
    u, opts, _ = universe(*key)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
    try:
        runs = [Packed(b, b.schedule_packed_raw()).raw() for _ in range(3)]
    finally:
        b.close()
        snap.close()
    assert len(runs[0][1]) > 0
    assert runs[0] == runs[1] == runs[2]


def test_determinism_host_build(cpusim_engine):
    check_determinism(cpusim_engine, (8, 5, 300, 600))


@pytest.mark.gpu
def test_determinism_gpu(gpu_engine):
    check_determinism(gpu_engine, (8, 5, 5000, 4000))


# ---- 5: submit / collect and format switching --------------------------------------------

def check_submit_collect(engine, C_, n):
    u = synth.Universe(8, 5, C_, 0, 2 * n)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, api.options())
    b1 = Batch(snap, structs=u.binding_slice(0, n))
    b2 = Batch(snap, structs=u.binding_slice(n, 2 * n))
    w1, w2 = Wide(b1.schedule_raw()), Wide(b2.schedule_raw())
    assert escaped(w1.rep).any() and escaped(w2.rep).any()
    for order in ((b1, b2), (b2, b1)):  # both in flight, collected in either order
        b1.submit_packed()
        b2.submit_packed()
        got = {id(b): Packed(b, b.collect_packed()) for b in order}
        check_same(got[id(b1)], w1)
        check_same(got[id(b2)], w2)
    # the same batch packed, wide, packed: each call's results are complete
    check_same(Packed(b1, b1.schedule_packed_raw()), w1)
    again = Wide(b1.schedule_raw())
    assert np.array_equal(again.cidx, w1.cidx) and np.array_equal(again.rep, w1.rep) and np.array_equal(again.offsets, w1.offsets)
    check_same(Packed(b1, b1.schedule_packed_raw()), w1)
    # a call is collected by its own format's function; the other leaves it collectable
    b1.submit_packed()
    with pytest.raises(EngineError, match="rc=-5"):
        b1.collect()
    check_same(Packed(b1, b1.collect_packed()), w1)
    b1.submit()
    with pytest.raises(EngineError, match="rc=-5"):
        b1.collect_packed()
    again = Wide(b1.collect())
    assert np.array_equal(again.cidx, w1.cidx) and np.array_equal(again.rep, w1.rep)
    b2.submit_packed()
    with pytest.raises(EngineError, match="rc=-5"):
        b2.submit_packed()  # the previous call is not collected
    with pytest.raises(EngineError, match="rc=-5"):
        b2.submit()
    check_same(Packed(b2, b2.collect_packed()), w2)
    with pytest.raises(EngineError, match="rc=-5"):
        b2.collect_packed()  # nothing submitted
    b1.submit_packed()  # destroyed with a packed call in flight: the batch waits for it
    b1.close()
    b2.close()
    snap.close()


def test_submit_collect_host_build(cpusim_engine):
    check_submit_collect(cpusim_engine, 300, 300)


def test_submit_refused_while_pending_host_build(cpusim_engine):
    """Both submit calls refuse a batch whose previous call is not collected with KP_ESTATE
    (-5), each under its own name (one body in engine.cpp serves the two)."""
    u = synth.Universe(8, 5, 64, 0, 8)
    snap = Snapshot.from_structs(cpusim_engine, u.clusters, u.n_clusters, u.names, api.options())
    b = Batch(snap, structs=u.binding_slice(0, 8))
    for first, collect in ((b.submit, b.collect), (b.submit_packed, b.collect_packed)):
        first()
        with pytest.raises(EngineError, match=r"rc=-5: kp_schedule_batch_submit: the batch's previous call is not collected"):
            b.submit()
        with pytest.raises(EngineError,
                           match=r"rc=-5: kp_schedule_batch_submit_packed: the batch's previous call is not collected"):
            b.submit_packed()
        collect()  # the pending call is untouched by the refusals
    b.close()
    snap.close()


@pytest.mark.gpu
def test_submit_collect_gpu(gpu_engine):
    check_submit_collect(gpu_engine, 5000, 2000)


# ---- 6: nothing to return -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_errors():
    """Every cluster carries a NoSchedule taint no binding tolerates: FitError for all."""
    clusters = fleet(70)
    for c in clusters:
        c["taints"] = [{"key": "drain", "value": "yes", "effect": "NoSchedule"}]
    return Case(clusters, [{"uid": f"e-{i}", "replicas": 3 + i,
                            "placement": {"replicaScheduling": {"replicaSchedulingType": "Duplicated"}}} for i in range(9)])


def check_nothing(engine):
    case = all_errors()
    assert all(r["status"] == api.STATUS_FIT_ERROR and not r["targets"] for r in case.want)
    p, w, _ = case.run(engine)
    assert p.n == 9 and p.n_targets == 0 and p.n_wide == 0 and not p.offsets.any()
    # the empty batch
    snap = Snapshot.from_structs(engine, case.ca, case.nc, case.names, case.opts)
    b = Batch(snap, structs=(case.bs, 0))
    try:
        r = b.schedule_packed_raw()
        assert r.n_bindings == 0 and r.n_targets == 0 and r.n_wide == 0 and r.offsets[0] == 0
        assert b.schedule(packed=True) == []
        b.submit_packed()
        r = b.collect_packed()
        assert r.n_bindings == 0 and r.n_targets == 0 and r.n_wide == 0
    finally:
        b.close()
        snap.close()


def test_nothing_to_return_host_build(cpusim_engine):
    check_nothing(cpusim_engine)


@pytest.mark.gpu
def test_nothing_to_return_gpu(gpu_engine):
    check_nothing(gpu_engine)
