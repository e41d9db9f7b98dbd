"""kp_pack_cache: packed binding records reused across scheduling cycles (VERDICT r5
item 6). The reference re-runs Schedule for bindings whose spec did not change
(pkg/scheduler/scheduler.go:437-468: Duplicated / non-workload bindings on every
reconcile, terminating target clusters, requeued failures); a spec change moves
metadata.generation. A batch created through kp_batch_create_keyed must be the batch
kp_batch_create packs from the same bindings (kp_batch_digest over headers, pools,
routes and estimator classes) and schedule identically, whichever records it reused;
a changed generation or scheduler status field, or a snapshot whose dictionaries grew,
re-packs."""
import ctypes as C
import os
import random

import pytest

from karmada_amd import api, synth
from karmada_amd.engine import Batch, PackCache, Snapshot


def copy_bindings(src, idx):
    arr = (api.kp_binding * max(1, len(idx)))()
    for j, i in enumerate(idx):
        arr[j] = src[i]
    return arr


def run_case(engine, n_bind=9000, n_clusters=300, schedule_check=True):
    os.environ["KP_PACK_THREADS"] = "3"
    try:
        u = synth.Universe(6, 11, n_clusters, 0, n_bind)
        opts = api.options()
        snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
        n = u.n_bindings
        gens = [1 + (i % 7) for i in range(n)]
        keys = api.binding_keys(u.bindings, n, gens)
        fresh = Batch(snap, structs=(u.bindings, n))
        d0 = fresh.digest()
        cache = PackCache(engine)
        cold = Batch(snap, structs=(u.bindings, n), cache=cache, keys=keys)
        assert cold.digest() == d0
        st = cache.stats()
        assert st["last_hits"] == 0 and st["entries"] == n, st
        warm = Batch(snap, structs=(u.bindings, n), cache=cache, keys=keys)
        assert warm.digest() == d0
        assert cache.stats()["last_hits"] == n
        if schedule_check:
            assert warm.schedule() == fresh.schedule()
        for b in (fresh, cold, warm):
            b.close()

        # the next cycle: shuffled, some bindings with a new generation, some with a
        # changed status (lastScheduledTime, observed affinity name), some new ones
        rng = random.Random(5)
        idx = list(range(n))
        rng.shuffle(idx)
        idx = idx[: n - 500]
        arr = copy_bindings(u.bindings, idx)
        g2 = [gens[i] for i in idx]
        bumped = set(rng.sample(range(len(idx)), 700))
        for j in bumped:
            g2[j] += 1
        touched = set(rng.sample(range(len(idx)), 300)) - bumped
        for j in touched:
            arr[j].has_last_scheduled_time = 1
            arr[j].last_scheduled_time_ns = arr[j].last_scheduled_time_ns + 12345
        names = set(rng.sample(range(len(idx)), 100)) - bumped - touched
        keep = []
        for j in names:
            nm = C.create_string_buffer(b"other-term")
            keep.append(nm)
            arr[j].observed_affinity_name = api.kp_str(C.cast(nm, C.c_char_p), 10)
        k2 = api.binding_keys(arr, len(idx), g2)
        want = Batch(snap, structs=(arr, len(idx)))
        got = Batch(snap, structs=(arr, len(idx)), cache=cache, keys=k2)
        assert got.digest() == want.digest()
        assert cache.stats()["last_hits"] == len(idx) - len(bumped) - len(touched) - len(names)
        if schedule_check:
            assert got.schedule() == want.schedule()
        got.close()
        want.close()

        # a snapshot whose dictionaries grew: the records resolved against the old ones
        assert snap.update([{"name": u.names[0], "labels": {"brand-new-key": "v"},
                             "resourceSummary": {"allocatable": {"cpu": "8", "pods": "110"}}}])  # dict_grew
        after = Batch(snap, structs=(u.bindings, n), cache=cache, keys=keys)
        assert cache.stats()["last_hits"] == 0
        fresh2 = Batch(snap, structs=(u.bindings, n))
        assert after.digest() == fresh2.digest()
        after.close()
        fresh2.close()
        cache.close()
        snap.close()
    finally:
        os.environ.pop("KP_PACK_THREADS", None)


def test_pack_cache_reuse_matches_fresh_pack(cpusim_engine):
    run_case(cpusim_engine)


def test_pack_cache_keys_required(cpusim_engine):
    u = synth.Universe(3, 3, 64, 0, 16)
    snap = Snapshot.from_structs(cpusim_engine, u.clusters, u.n_clusters, u.names, api.options())
    h = C.c_void_p()
    L = cpusim_engine.L
    assert L.kp_batch_create_keyed(cpusim_engine.h, snap.h, u.bindings, None, u.n_bindings, None, C.byref(h)) != 0
    snap.close()


@pytest.mark.gpu
def test_pack_cache_reuse_matches_fresh_pack_gpu(gpu_engine):
    run_case(gpu_engine, n_bind=9000, n_clusters=300)


# ---- the packer's stages: one image whatever the threads, the chunks and the records ----------

N_CLUSTERS = 130


class Mixed:
    """Bindings of synth configs 2 (tolerations, static-weight rules), 3 (summary and model
    requests) and 6 (multi-term affinities with overflow terms, spec.Clusters, name and exclude
    lists) interleaved, over config 6's clusters (the configs share cluster and label names),
    every 50th binding given a zone list; evictions come with configs 2 and 3. Seeds differ, so
    no two bindings share a uid."""

    def __init__(self, n):
        self.us = [synth.Universe(cfg, 100 + cfg, N_CLUSTERS, 0, n // 3 + 1) for cfg in (2, 3, 6)]
        self.u = self.us[2]
        self.n = n
        self.arr = (api.kp_binding * n)()
        for i in range(n):
            self.arr[i] = self.us[i % 3].bindings[i // 3]
        self.w = api.World()
        zones = self.w.affinity({"fieldSelector": {"matchExpressions": [
            {"key": "zone", "operator": "In", "values": ["region-00-a", "region-01-b", "region-02-c"]}]}})
        for i in range(0, n, 50):
            self.arr[i].has_cluster_affinity = 1
            self.arr[i].cluster_affinity = zones
            self.arr[i].n_cluster_affinities = 0

    def features(self):
        """How many bindings use each thing that puts references into the pools."""
        f = dict.fromkeys(["filter affinity", "overflow terms", "static weights", "evictions", "targets", "requests",
                           "tolerations", "names", "excludes", "zones"], 0)
        def sv(s):
            return (s.ptr or b"")[:s.len]

        for i in range(self.n):
            b = self.arr[i]
            term = [b.cluster_affinities[k] for k in range(b.n_cluster_affinities)
                    if sv(b.cluster_affinities[k].affinity_name) == sv(b.observed_affinity_name)]
            a = b.cluster_affinity
            f["filter affinity"] += bool(b.has_cluster_affinity or term)
            f["overflow terms"] += bool(not b.has_cluster_affinity and term and term[0].n_overflow)
            f["static weights"] += bool(b.n_static_weights)
            f["evictions"] += bool(b.n_eviction_from)
            f["targets"] += bool(b.n_clusters)
            f["requests"] += bool(b.n_resource_request)
            f["tolerations"] += bool(b.n_tolerations)
            f["names"] += bool(b.has_cluster_affinity and a.n_cluster_names)
            f["excludes"] += bool(b.has_cluster_affinity and a.n_exclude_clusters)
            f["zones"] += bool(b.has_cluster_affinity and a.n_field_expressions)
        return f


def digests(engine, snap, arr, n, threads):
    """The image's digest from an unkeyed, a keyed cold and a keyed warm creation, and from a
    warm one after 10 % of the keys' generations moved (hits and misses inside every chunk)."""
    os.environ["KP_PACK_THREADS"] = str(threads)
    try:
        gens = [1 + i % 5 for i in range(n)]
        moved = list(gens)
        for j in random.Random(n).sample(range(n), n // 10):
            moved[j] += 1
        out = {}
        cache = PackCache(engine)
        for form, g in (("unkeyed", None), ("cold", gens), ("warm", gens), ("warm, 10 % moved", moved)):
            kw = {} if g is None else {"cache": cache, "keys": api.binding_keys(arr, n, g)}
            b = Batch(snap, structs=(arr, n), **kw)
            out[form] = b.digest()
            b.close()
            if g is not None:
                want = {"cold": 0, "warm": n, "warm, 10 % moved": n - n // 10}[form]
                assert cache.stats()["last_hits"] == want, (form, cache.stats())
        cache.close()
        return out
    finally:
        os.environ.pop("KP_PACK_THREADS", None)


def digest_invariance(engine):
    m = Mixed(8193)
    feats = m.features()
    assert all(feats.values()), feats
    snap = Snapshot.from_structs(engine, m.u.clusters, m.u.n_clusters, m.u.names, api.options())
    try:
        for n, threads in ((8193, (1, 3)), (1025, (1,))):
            got = {(t, form): d for t in threads for form, d in digests(engine, snap, m.arr, n, t).items()}
            assert len(set(got.values())) == 1, (n, got)
    finally:
        snap.close()


def test_pack_digest_invariance(cpusim_engine):
    digest_invariance(cpusim_engine)


@pytest.mark.gpu
def test_pack_digest_invariance_gpu(gpu_engine):
    digest_invariance(gpu_engine)


def filter_masks(engine, b, n_clusters):
    W = (n_clusters + 63) // 64
    m = (C.c_uint64 * (b.n * W))()
    engine._check(engine.L.kp_filter_batch(engine.h, b.h, m), "kp_filter_batch")
    return [tuple(m[i * W:(i + 1) * W]) for i in range(b.n)]


def position_independence(engine):
    """The same 64 bindings at [0, 64) of a batch and at [1024, 1088), the second chunk, behind
    1024 others whose first one alone leaves every pool non-empty (an always-kept toleration:
    tols; cluster names: ipool, progs, instrs; a request: ipool, lpool), so the chunk merge
    rebases the 64 by a non-zero delta in all five pools. Packed fresh and served from records."""
    import oracle_lib as O
    m = Mixed(1024 + 64)
    u, opts = m.u, api.options()
    w = api.World()
    first, _ = w.bindings([{
        "uid": "first", "name": "first", "replicas": 2, "replicaRequirements": {"resourceRequest": {"cpu": "1"}},
        "placement": {"clusterAffinity": {"clusterNames": [u.names[1], u.names[2]]},
                      "clusterTolerations": [{"operator": "Exists"}]}}])
    behind = (api.kp_binding * (1024 + 64))()
    behind[0] = first[0]
    for i in range(1, 1024):
        behind[i] = m.arr[64 + i]
    for j in range(64):
        behind[1024 + j] = m.arr[j]
    the64 = copy_bindings(m.arr, range(64))
    nc = u.n_clusters
    want = O.schedule_c(u.clusters, nc, the64, 64, opts, O.FAST, 4)
    OL = O.lib()
    W = (nc + 63) // 64
    want_mask = []
    for j in range(64):
        words = [0] * W
        for c in range(nc):
            if not u.clusters[c].deleting and OL.kpo_filter(C.pointer(u.clusters[c]), C.pointer(the64[j]), C.byref(opts)) == 0:
                words[c >> 6] |= 1 << (c & 63)
        want_mask.append(tuple(words))
    snap = Snapshot.from_structs(engine, u.clusters, nc, u.names, opts)
    cache = PackCache(engine)
    k64 = api.binding_keys(the64, 64, [1] * 64)
    kall = api.binding_keys(behind, 1024 + 64, [1] * (1024 + 64))
    try:
        for form in ("fresh", "cold", "records"):
            kw64 = {} if form == "fresh" else {"cache": cache, "keys": k64}
            kwall = {} if form == "fresh" else {"cache": cache, "keys": kall}
            front = Batch(snap, structs=(the64, 64), **kw64)
            if form != "fresh":
                assert cache.stats()["last_hits"] == (0 if form == "cold" else 64), (form, cache.stats())
            back = Batch(snap, structs=(behind, 1024 + 64), **kwall)
            if form != "fresh":  # the 64 from the records `front` made; the 1024 too once they have theirs
                assert cache.stats()["last_hits"] == (64 if form == "cold" else 1024 + 64), (form, cache.stats())
            fm, bm = filter_masks(engine, front, nc), filter_masks(engine, back, nc)
            fs, bs = front.schedule(), back.schedule()
            for j in range(64):
                assert fm[j] == bm[1024 + j] == want_mask[j], (form, j)
                assert fs[j] == bs[1024 + j] == want[j], (form, j, fs[j], bs[1024 + j], want[j])
            front.close()
            back.close()
    finally:
        cache.close()
        snap.close()


def test_pack_position_independence(cpusim_engine):
    position_independence(cpusim_engine)


@pytest.mark.gpu
def test_pack_position_independence_gpu(gpu_engine):
    position_independence(gpu_engine)
