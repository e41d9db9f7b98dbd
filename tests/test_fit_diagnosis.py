"""kp_fit_diagnosis_batch: the FitError reason histogram of each listed binding against the
per-pair oracle kpo_filter_reason (RunFilterPluginsReason). The expected bins of a binding
are the histogram of its C oracle words by code, and for KP_REASON_TAINT by the text of the
taint the argument indexes, so the snapshot's taint-uid table is checked independently of
the engine: a taint_ref must print the same text, and name the lowest caller cluster index
that carries it."""
import ctypes as C

import numpy as np
import pytest

from karmada_amd import api, synth
from karmada_amd.engine import KP_EINVAL, KP_ESTATE, Batch, GenericScheduler, Snapshot
import oracle_lib as O

OL = O.lib()
OL.kpo_filter_reason.restype = C.c_uint32
REF_BITS = api.TAINT_REF_CLUSTER_BITS
DEPLOY = [{"groupVersion": "apps/v1", "resources": [{"kind": "Deployment"}]}]


def _s(k):
    return (k.ptr or b"")[:k.len].decode()


def taint_texts(cl):
    """The texts of a kp_cluster's NoSchedule/NoExecute taints, in spec order."""
    ts = [cl.taints[i] for i in range(cl.n_taints)]
    return [api.taint_string({"key": _s(t.key), "value": _s(t.value), "effect": _s(t.effect)})
            for t in ts if _s(t.effect) in ("NoSchedule", "NoExecute")]


def representatives(ca, nc):
    """{taint text: taint_ref}: the lowest caller cluster index carrying it, first position."""
    rep = {}
    for c in range(nc):
        for k, text in enumerate(taint_texts(ca[c])):
            rep.setdefault(text, c | k << REF_BITS)
    return rep


def histogram(ca, words):
    """(n_fit, n_deleting, {(code, taint text or None): count}) of one binding's reason words."""
    bins, n_fit, n_del = {}, 0, 0
    texts = {}
    for c, w in enumerate(words):
        code = w & 0xFF
        if code == api.REASON_FIT:
            n_fit += 1
        elif code == api.REASON_DELETING:
            n_del += 1
        else:
            text = None
            if code == api.REASON_TAINT:
                if c not in texts:
                    texts[c] = taint_texts(ca[c])
                text = texts[c][w >> 8]
            bins[(code, text)] = bins.get((code, text), 0) + 1
    return n_fit, n_del, bins


def oracle_words(ca, nc, ba, i, opts):
    return [OL.kpo_filter_reason(C.byref(ca[c]), C.byref(ba[i]), C.byref(opts)) for c in range(nc)]


def check_entry(ca, nc, rep, entry, want):
    """One binding's diagnosis against (n_fit, n_deleting, bins) of its reason words."""
    idx, n_fit, n_del, bins = entry
    order = [(r, ref) for r, ref, _ in bins]
    assert order == sorted(set(order)), f"binding {idx}: bins not in (reason, taint_ref) order: {order}"
    got = {}
    for reason, ref, count in bins:
        assert count > 0 and 1 <= reason <= 8
        text = None
        if reason == api.REASON_TAINT:
            text = taint_texts(ca[ref & ((1 << REF_BITS) - 1)])[ref >> REF_BITS]
            assert rep[text] == ref, f"binding {idx}: {text} named by {ref:#x}, representative {rep[text]:#x}"
        else:
            assert ref == 0
        assert (reason, text) not in got, f"binding {idx}: two bins for {(reason, text)}"
        got[(reason, text)] = count
    assert (n_fit, n_del, got) == want, f"binding {idx}: got {(n_fit, n_del, got)}, want {want}"
    assert n_fit + n_del + sum(got.values()) == nc


def check(engine, ca, nc, names, structs, opts, bindings="all", filters=None, words=None):
    """Diagnoses `bindings` of the batch (all of them by default) and checks every entry
    against the oracle (or against the given per-binding reason words). Returns the entries
    and the wanted histograms."""
    ba, nb = structs
    snap = Snapshot.from_structs(engine, ca, nc, names, opts)
    b = Batch(snap, structs=structs, filters=filters)
    lst = list(range(nb)) if bindings == "all" else bindings
    got = b.fit_diagnosis(lst)
    b.close()
    snap.close()
    assert [g[0] for g in got] == lst
    rep = representatives(ca, nc)
    wants = []
    for g in got:
        w = words[g[0]] if words is not None else oracle_words(ca, nc, ba, g[0], opts)
        wants.append(histogram(ca, w))
        check_entry(ca, nc, rep, g, wants[-1])
    return got, wants


def check_universe(engine, config, seed, nc, nb, opts, **kw):
    u = synth.Universe(config, seed, nc, 0, nb)
    return check(engine, u.clusters, u.n_clusters, u.names, u.binding_slice(0, nb), opts, **kw)


def check_dicts(engine, clusters, bindings, opts=None, **kw):
    w = api.World()
    ca, nc = w.clusters(clusters)
    structs = w.bindings(bindings)
    return check(engine, ca, nc, [c["name"] for c in clusters], structs, opts or api.options(), **kw)


def reached(wants):
    codes = set()
    for _, n_del, bins in wants:
        codes |= {code for code, _ in bins}
        if n_del:
            codes.add(api.REASON_DELETING)
    return codes


@pytest.mark.parametrize("config,seed,nc,nb", [(6, 31, 120, 150), (4, 4, 200, 60), (3, 3, 150, 60)])
def test_histograms_cpusim(cpusim_engine, config, seed, nc, nb):
    _, wants = check_universe(cpusim_engine, config, seed, nc, nb, api.options())
    if config == 6:  # the edge workload reaches every reason
        assert {1, 2, 3, 255} <= reached(wants), reached(wants)
        assert any(n_fit for n_fit, _, _ in wants)


@pytest.mark.parametrize("plugins", [api.PLUGIN_ALL & ~api.PLUGIN_TAINT_TOLERATION, api.PLUGIN_SPREAD_CONSTRAINT, 0])
def test_plugin_sets_cpusim(cpusim_engine, plugins):
    check_universe(cpusim_engine, 6, 32, 90, 120, api.options(plugins=plugins))


def _rc(engine, batch, bindings=None, n=0, out=True):
    d = api.kp_fit_diagnosis()
    arr = None if bindings is None else (C.c_uint64 * max(1, len(bindings)))(*bindings)
    return engine.L.kp_fit_diagnosis_batch(engine.h, batch.h, arr, len(bindings) if bindings is not None else n,
                                           C.byref(d) if out else None)


def test_null_list_is_the_fit_error_bindings(cpusim_engine):
    u = synth.Universe(6, 31, 120, 0, 150)  # (row 0 of the verdicts rejects every cluster: FitError)
    snap = Snapshot.from_structs(cpusim_engine, u.clusters, u.n_clusters, u.names, api.options(out_of_tree_plugins=1))
    b = Batch(snap, structs=u.binding_slice(0, 150), filters=filter_rows(3, 120, 150))
    assert _rc(cpusim_engine, b) == KP_ESTATE  # no schedule call yet
    for packed in (False, True):
        res = b.schedule(packed=packed)
        failed = [i for i, r in enumerate(res) if r["status"] == api.STATUS_FIT_ERROR]
        assert failed
        got = b.fit_diagnosis()
        assert [g[0] for g in got] == failed
        assert got == b.fit_diagnosis(failed)
        assert all(g[1] == 0 for g in got)  # a FitError binding fits nowhere
    b.submit()
    assert _rc(cpusim_engine, b) == KP_ESTATE  # submitted, not collected
    assert b.fit_diagnosis(failed) == got      # an explicit list needs no schedule call
    b.collect()
    assert b.fit_diagnosis() == got
    b.close()
    snap.close()


FIVE = [
    {"name": "m1", "taints": [{"key": "a", "value": "x", "effect": "NoSchedule"}], "apiEnablements": DEPLOY},
    {"name": "m2", "taints": [{"key": "b", "value": "", "effect": "PreferNoSchedule"},
                              {"key": "c", "value": "", "effect": "NoExecute"}], "apiEnablements": DEPLOY},
    {"name": "m3", "apiEnablements": []},
    {"name": "m4", "deleting": True, "apiEnablements": DEPLOY},
    {"name": "m5", "labels": {"env": "dev"}, "apiEnablements": DEPLOY},
]
WEB = {"apiVersion": "apps/v1", "kind": "Deployment", "name": "web", "namespace": "default", "replicas": 2,
       "placement": {"clusterAffinity": {"labelSelector": {"matchLabels": {"env": "prod"}}},
                     "clusterTolerations": [{"key": "z", "operator": "Exists", "effect": "NoSchedule"}]}}


def test_fit_errors_message(cpusim_engine):
    """The five-cluster case of test_fit_error_from_engine: {c:NoExecute} has an empty value
    and is taint 0 of m2, whose PreferNoSchedule taint is not among the indexed ones."""
    g = GenericScheduler(cpusim_engine, FIVE)
    ok = dict(WEB, name="ok", placement={"clusterTolerations": [{"operator": "Exists"}]})
    msgs = g.fit_errors([ok, WEB], FIVE)
    want = ("0/5 clusters are available: 1 cluster(s) did not have the API resource, "
            "1 cluster(s) did not match the placement cluster affinity constraint, "
            "1 cluster(s) had untolerated taint {a=x:NoSchedule}, 1 cluster(s) had untolerated taint {c:NoExecute}.")
    assert msgs == {1: want}
    assert want == g.fit_error(WEB, FIVE)
    assert g.fit_errors([ok, WEB], FIVE, results=g.schedule([ok, WEB])) == {1: want}
    check_dicts(cpusim_engine, FIVE, [ok, WEB])


def taint(k, v="", e="NoSchedule"):
    return {"key": k, "value": v, "effect": e}


def binding(name, **placement):
    return {"apiVersion": "apps/v1", "kind": "Deployment", "name": name, "namespace": "default", "replicas": 1,
            "placement": placement}


def test_bins_are_per_triple_not_per_list(cpusim_engine):
    """Three distinct taint lists start with the same taint, and one list's first untolerated
    taint depends on the binding's tolerations."""
    lists = [[taint("a", "1"), taint("b", "1")], [taint("a", "1"), taint("c", "1", "NoExecute")], [taint("a", "1")],
             [taint("b", "1"), taint("a", "1")], [taint("c", "1", "NoExecute")], []]
    clusters = [{"name": "c%02d" % i, "taints": lists[i % len(lists)], "apiEnablements": DEPLOY} for i in range(23)]
    tol_a = {"key": "a", "operator": "Equal", "value": "1", "effect": "NoSchedule"}
    tol_b = {"key": "b", "operator": "Exists"}
    bs = [binding("none"), binding("a", clusterTolerations=[tol_a]), binding("b", clusterTolerations=[tol_b]),
          binding("ab", clusterTolerations=[tol_a, tol_b]), binding("all", clusterTolerations=[{"operator": "Exists"}])]
    got, wants = check_dicts(cpusim_engine, clusters, bs)
    a, b, c = "a=1:NoSchedule", "b=1:NoSchedule", "c=1:NoExecute"
    assert wants[0][2] == {(2, a): 12, (2, b): 4, (2, c): 4}  # three lists share the bin of a
    assert wants[1][2] == {(2, b): 8, (2, c): 8}              # ... and split once a is tolerated
    assert wants[4] == (23, 0, {})
    assert [len(g[3]) for g in got] == [3, 2, 2, 1, 0]


def test_spec_clusters_pass_api_and_taints(cpusim_engine):
    """TargetContains: a cluster named in spec.Clusters passes APIEnablement and
    TaintToleration whatever it lacks; ClusterAffinity still applies to it."""
    clusters = [{"name": "t1", "taints": [taint("a", "1")], "apiEnablements": [], "labels": {"env": "prod"}},
                {"name": "t2", "taints": [taint("a", "1")], "apiEnablements": []},
                {"name": "t3", "taints": [taint("a", "1")], "apiEnablements": DEPLOY},
                {"name": "t4", "apiEnablements": DEPLOY}]
    prod = {"labelSelector": {"matchLabels": {"env": "prod"}}}
    tgt = [{"name": "t1", "replicas": 1}, {"name": "t2", "replicas": 1}]
    bs = [dict(binding("plain")), dict(binding("named"), clusters=tgt),
          dict(binding("named-prod", clusterAffinity=prod), clusters=tgt)]
    _, wants = check_dicts(cpusim_engine, clusters, bs)
    assert wants[0] == (1, 0, {(1, None): 2, (2, "a=1:NoSchedule"): 1})
    assert wants[1] == (3, 0, {(2, "a=1:NoSchedule"): 1})
    assert wants[2] == (1, 0, {(3, None): 2, (2, "a=1:NoSchedule"): 1})


def filter_rows(seed, nc, nb, n_rows=5):
    rng = np.random.default_rng(seed)
    ok = rng.random((n_rows, nc)) < 0.6
    ok[0, :] = False
    row_of = rng.integers(-1, n_rows, nb).astype(np.int32)
    return ok, row_of, 1


def check_out_of_tree(engine, nc, nb, seed=7):
    """A batch with out-of-tree rows: the bins are those of kp_filter_reasons' words on it."""
    u = synth.Universe(6, seed, nc, 0, nb)
    flt = filter_rows(seed, nc, nb)
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, api.options(out_of_tree_plugins=1))
    b = Batch(snap, structs=u.binding_slice(0, nb), filters=flt)
    r = (C.c_uint32 * (nb * nc))()
    engine._check(engine.L.kp_filter_reasons(engine.h, b.h, r), "kp_filter_reasons")
    failed = [i for i, x in enumerate(b.schedule()) if x["status"] == api.STATUS_FIT_ERROR]
    by_status = b.fit_diagnosis()
    b.close()
    snap.close()
    words = [[r[i * nc + c] for c in range(nc)] for i in range(nb)]
    got, wants = check(engine, u.clusters, nc, u.names, u.binding_slice(0, nb), api.options(out_of_tree_plugins=1),
                       filters=flt, words=words)
    assert api.REASON_OUT_OF_TREE in reached(wants)
    assert failed and by_status == [got[i] for i in failed]  # the NULL list: the FitError bindings


def test_out_of_tree_rows_cpusim(cpusim_engine):
    check_out_of_tree(cpusim_engine, 130, 60)


def test_fallback_pair_rows(cpusim_engine, monkeypatch):
    """KP_PAIR_ROWS=1: k_reasons over the listed bindings in several chunks, the list with
    gaps (several runs per chunk), and with out-of-tree rows."""
    monkeypatch.setenv("KP_PAIR_ROWS", "1")
    monkeypatch.setenv("KP_REASONS_CHUNK", str(7 * 120))
    lst = [i for i in range(150) if i % 5 != 3]
    check_universe(cpusim_engine, 6, 31, 120, 150, api.options(), bindings=lst)
    check_out_of_tree(cpusim_engine, 130, 60)


def test_fallback_many_taint_lists(cpusim_engine, monkeypatch):
    """More than 64 distinct taint lists: the snapshot has no bitset rows."""
    clusters = [{"name": "c%03d" % i, "apiEnablements": DEPLOY if i % 7 else [],
                 "taints": [taint("k%d" % (i % 70), "v"), taint("shared", "", "NoExecute")][i % 3 == 0:]}
                for i in range(150)]
    bs = [binding("b%d" % j, clusterTolerations=[{"key": "k%d" % k, "operator": "Exists"} for k in range(j, 70, 3)])
          for j in range(9)]
    monkeypatch.setenv("KP_REASONS_CHUNK", str(4 * 150))
    got, wants = check_dicts(cpusim_engine, clusters, bs)
    assert max(len(g[3]) for g in got) > 40


@pytest.mark.parametrize("nc", [1, 65, 127, 129])
def test_padding_bits_are_not_counted(cpusim_engine, nc):
    got, _ = check_universe(cpusim_engine, 6, 5, nc, 40, api.options())
    assert len(got) == 40
    assert check_universe(cpusim_engine, 6, 5, nc, 40, api.options(), bindings=[])[0] == []


def test_update_and_import_follow(cpusim_engine):
    """kp_snapshot_update changes a cluster's taints (a new triple, a new representative),
    then export / import: the uid table follows."""
    clusters = [{"name": "u%d" % i, "taints": [taint("a", "1")] if i in (2, 5) else [], "apiEnablements": DEPLOY}
                for i in range(8)]
    bs = [binding("none"), binding("a", clusterTolerations=[{"key": "a", "operator": "Exists"}])]
    w = api.World()
    structs = w.bindings(bs)
    snap = Snapshot(cpusim_engine, clusters)
    rep0 = representatives(*w.clusters(clusters))
    assert rep0 == {"a=1:NoSchedule": 2}

    def diagnose(sn, ca, nc):
        b = Batch(sn, structs=structs)
        got = b.fit_diagnosis([0, 1])
        b.close()
        rep = representatives(ca, nc)
        for g in got:
            check_entry(ca, nc, rep, g, histogram(ca, oracle_words(ca, nc, structs[0], g[0], api.options())))
        return got

    before = diagnose(snap, *w.clusters(clusters))
    assert before[0][3] == [(2, 2, 2)]
    changed = [dict(c) for c in clusters]
    changed[1]["taints"] = [taint("z", "9", "NoExecute"), taint("a", "1")]
    changed[2]["taints"] = []
    snap.update(changed)  # (the dictionaries grow: the batches below are new ones)
    ca, nc = w.clusters(changed)
    after = diagnose(snap, ca, nc)
    assert after[0][3] == [(2, 1, 1), (2, 1 | 1 << REF_BITS, 1)]  # u1 by z; u5 by a, which u1 now represents
    assert after[1][3] == [(2, 1, 1)]
    assert representatives(ca, nc) == {"z=9:NoExecute": 1, "a=1:NoSchedule": 1 | 1 << REF_BITS}
    imp = Snapshot.from_bytes(cpusim_engine, snap.to_bytes(), [c["name"] for c in changed])
    assert diagnose(imp, ca, nc) == after
    imp.close()
    snap.close()


def test_einval(cpusim_engine):
    u = synth.Universe(6, 31, 40, 0, 10)
    snap = Snapshot.from_structs(cpusim_engine, u.clusters, u.n_clusters, u.names, api.options())
    b = Batch(snap, structs=u.binding_slice(0, 10))
    assert _rc(cpusim_engine, b, [3, 2]) == KP_EINVAL      # unsorted
    assert _rc(cpusim_engine, b, [2, 2]) == KP_EINVAL      # repeated
    assert _rc(cpusim_engine, b, [0, 10]) == KP_EINVAL     # out of range
    assert _rc(cpusim_engine, b, [0, 1], out=False) == KP_EINVAL
    assert _rc(cpusim_engine, b, [0, 9]) == 0
    b.close()
    snap.close()


# ---- GPU ---------------------------------------------------------------------------------
# 700 clusters are 11 words per row (lanes 11..63 idle: a reduction that reads them shows);
# 5 000 are 79 words, a second trip of the lane loop.

@pytest.mark.gpu
def test_histograms_gpu(gpu_engine):
    _, wants = check_universe(gpu_engine, 6, 31, 700, 300, api.options())
    assert {1, 2, 3, 255} <= reached(wants)


@pytest.mark.gpu
def test_fit_error_list_gpu(gpu_engine):
    u = synth.Universe(4, 4, 5000, 0, 20)
    snap = Snapshot.from_structs(gpu_engine, u.clusters, u.n_clusters, u.names, api.options())
    b = Batch(snap, structs=u.binding_slice(0, 20))
    res = b.schedule()
    failed = [i for i, r in enumerate(res) if r["status"] == api.STATUS_FIT_ERROR]
    got = b.fit_diagnosis()
    b.close()
    snap.close()
    assert [g[0] for g in got] == failed
    rep = representatives(u.clusters, 5000)
    for g in got:
        check_entry(u.clusters, 5000, rep, g,
                    histogram(u.clusters, oracle_words(u.clusters, 5000, u.bindings, g[0], api.options())))
    # (and bindings that fit somewhere, over the same 79-word rows)
    check(gpu_engine, u.clusters, 5000, u.names, u.binding_slice(0, 20), api.options(), bindings=[0, 7, 19])


@pytest.mark.gpu
def test_padding_gpu(gpu_engine):
    check_universe(gpu_engine, 6, 5, 129, 40, api.options())


@pytest.mark.gpu
def test_out_of_tree_rows_gpu(gpu_engine):
    check_out_of_tree(gpu_engine, 130, 60)


@pytest.mark.gpu
def test_fallback_pair_rows_gpu(gpu_engine, monkeypatch):
    monkeypatch.setenv("KP_PAIR_ROWS", "1")
    monkeypatch.setenv("KP_REASONS_CHUNK", str(64 * 700))
    check_universe(gpu_engine, 6, 31, 700, 300, api.options())
