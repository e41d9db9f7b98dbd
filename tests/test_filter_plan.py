"""Shape tests of k_filter as it stands (kp_filter.h: body_filter walking filter_word
for each word; taints_tolerated_regs), checked as test_filter_bits.py checks the filter:
every (binding, cluster) pair against the oracle's RunFilterPlugins (kpo_filter), in
the bits mode and against the per-pair evaluator (KP_PAIR_ROWS=1).

There is no filter plan in the tree: the file keeps the name under which these shapes
were asked for, when a per-binding plan of 128 entries was to be built. That plan was
measured and dropped, so the cases of 128 and 129 row references
and of more than 64 terms or instructions sit on no boundary of the current code; they
stay as plain long predicates. The boundaries that do exist are the word loop and the
tolerations body_filter keeps in registers (kTolRegs = 4).

Cluster counts sit around the word and wave boundaries: C = 1, 64, 65 (W = 1, 1, 2),
4096 / 4097 (W = 64 / 65: a lane's second word appears) and 8192 / 8193 (W = 128 / 129).
The bindings (_shapes) hold: a single value, values no cluster carries under In and
NotIn, several terms of several instructions, an instruction of more than 64 values,
row instructions mixed with cluster names, excludes and field Gt/Lt, the long
predicates above; no, several and more tolerations than kTolRegs (the ones that match
placed last); spec.Clusters members that fail APIEnablement and TaintToleration, with
eviction tasks. One universe holds 64 distinct taint lists (kTsetRowsMax).

The packer never emits an empty filter list with ClusterAffinity on and BF_AFF_ALL
clear (a binding with an affinity always compiles at least one program), so that
shape cannot be stated here; an affinity that can never match (OP_FALSE) and an
affinity term without instructions (matches everything) are.
"""
import functools
import random

import pytest

from karmada_amd import api
from test_filter_bits import _filter, _oracle

ENV = ["a", "b", "c", "d", "e"]
NSHARD = 140
SHARDS = ["s%d" % i for i in range(NSHARD)]
PROV = ["aws", "gcp", "12", "7", "-3"]
REGS = ["r1", "r2", "100", "5"]
ZONES = ["z1", "z2", "z3", "z4"]
GVKS = [("apps/v1", "Deployment"), ("batch/v1", "Job")]


def _clusters(nc, seed, tsets):
    """nc clusters; the first tsets - 1 carry a taint list of their own."""
    r = random.Random(seed)
    out = []
    for i in range(nc):
        d = {"name": "m-%05d" % i, "labels": {"shard": SHARDS[i % NSHARD]}}
        if r.random() < 0.8:
            d["labels"]["env"] = r.choice(ENV)
        if r.random() < 0.85:
            d["provider"] = r.choice(PROV)
        if r.random() < 0.85:
            d["region"] = r.choice(REGS)
        if r.random() < 0.8:
            d["zones"] = r.sample(ZONES, r.randint(1, 3))
        if i < tsets - 1:
            d["taints"] = [{"key": "k%d" % i, "value": "v", "effect": "NoSchedule"}]
            if i % 3 == 0:
                d["taints"].append({"key": "maint", "value": "x", "effect": "NoExecute"})
        elif r.random() < 0.1 and tsets > 1:
            d["taints"] = [dict(t) for t in out[0]["taints"]]  # (no further distinct list)
        d["apiEnablements"] = [{"groupVersion": gv, "resources": [{"kind": k}]} for gv, k in GVKS if r.random() < 0.9]
        d["deleting"] = r.random() < 0.03
        out.append(d)
    return out


def _lbl(key, op, values=None):
    e = {"key": key, "operator": op}
    if values is not None:
        e["values"] = list(values)
    return e


def _aff(label=(), field=(), names=None, exclude=None):
    a = {}
    if label:
        a["labelSelector"] = {"matchExpressions": list(label)}
    if field:
        a["fieldSelector"] = {"matchExpressions": list(field)}
    if names:
        a["clusterNames"] = names
    if exclude:
        a["exclude"] = exclude
    return a


def _terms(affs):
    """One affinity term (observed) with the rest as its overflow affinities: the
    filter ORs them for a workload."""
    return {"clusterAffinities": [dict(affs[0], affinityName="t0", overflowAffinities=affs[1:])]}


def _shapes(names):
    some = [names[i] for i in sorted({0, len(names) // 3, len(names) // 2, len(names) - 1})]
    tol = lambda key, op="Exists", value="", effect="": {"key": key, "operator": op, "value": value, "effect": effect}
    P = []  # (placement, extra binding fields)
    P.append(({}, {}))                                                          # no affinity: BF_AFF_ALL
    P.append(({"clusterAffinity": _aff([_lbl("env", "In", ["a"])])}, {}))       # one term, one value
    P.append(({"clusterAffinity": _aff([_lbl("env", "In", ["s5"])])}, {}))      # a value no cluster carries
    P.append(({"clusterAffinity": _aff([_lbl("env", "NotIn", ["s5", "s6"])])}, {}))  # NotIn of absent values: all
    P.append(({"clusterAffinity": _aff([_lbl("env", "In", ["s5", "b"]), _lbl("shard", "NotIn", ["s1", "a"])])}, {}))
    P.append(({"clusterAffinity": _aff([_lbl("nokey", "In", ["a"])])}, {}))     # never matches: OP_FALSE
    P.append(({"clusterAffinity": {}}, {}))                                     # a term without instructions
    P.append(({"clusterAffinity": _aff([_lbl("env", "Exists"), _lbl("shard", "DoesNotExist")])}, {}))
    # several terms with several instructions each
    P.append((_terms([
        _aff([_lbl("env", "In", ["a", "b"]), _lbl("shard", "NotIn", SHARDS[:7])], [_lbl("provider", "In", ["aws"])]),
        _aff([_lbl("env", "DoesNotExist")], [_lbl("zone", "In", ["z1", "z3"]), _lbl("region", "NotIn", ["r1"])]),
        _aff([_lbl("shard", "In", SHARDS[3:9])], [_lbl("zone", "DoesNotExist")]),
        _aff([], [_lbl("region", "Exists"), _lbl("provider", "DoesNotExist")]),
    ]), {}))
    # an instruction with more than 64 values
    P.append(({"clusterAffinity": _aff([_lbl("shard", "In", SHARDS[10:80])])}, {}))
    P.append(({"clusterAffinity": _aff([_lbl("shard", "NotIn", SHARDS[:66]), _lbl("env", "In", ["c", "d"])])}, {}))
    # row instructions mixed with names, excludes and field Gt / Lt
    P.append(({"clusterAffinity": _aff([_lbl("env", "In", ["a", "b", "c"])], [_lbl("provider", "Gt", ["6"])],
                                       names=names[: max(1, len(names) * 2 // 3)], exclude=some)}, {}))
    P.append((_terms([
        _aff([_lbl("env", "NotIn", ["a"])], [_lbl("region", "Lt", ["50"])], exclude=some[:2]),
        _aff([_lbl("shard", "In", SHARDS[:3])], [_lbl("provider", "Lt", ["10"]), _lbl("zone", "Exists")]),
        _aff([], [], names=some),
    ]), {}))
    # long predicates: 128 row references, and one more (no boundary in the current code)
    P.append(({"clusterAffinity": _aff([_lbl("shard", "In", SHARDS[:100]), _lbl("env", "NotIn", SHARDS[100:128])])}, {}))
    P.append(({"clusterAffinity": _aff([_lbl("shard", "In", SHARDS[:101]), _lbl("env", "NotIn", SHARDS[100:128])])}, {}))
    P.append(({"clusterAffinity": _aff([_lbl("shard", "In", SHARDS[:139]), _lbl("env", "In", ["a", "e"])])}, {}))
    # more than 64 terms; more than 64 instructions (30 terms of 3)
    P.append((_terms([_aff([_lbl("shard", "In", [SHARDS[2 * j]])]) for j in range(70)]), {}))
    P.append((_terms([_aff([_lbl("shard", "In", SHARDS[j:j + 30:10]), _lbl("env", "NotIn", [ENV[j % 5]])],
                           [_lbl("zone", "In", [ZONES[j % 4]])]) for j in range(30)]), {}))
    # 70 terms of 2 instructions
    P.append((_terms([_aff([_lbl("shard", "NotIn", [SHARDS[j]]), _lbl("env", "Exists")]) for j in range(70)]), {}))
    # tolerations: several, more than the register count (the matching ones last), any-key
    few = [tol("k1"), tol("k2", "Equal", "v", "NoSchedule"), tol("maint", "Equal", "x")]
    # (keys the snapshot knows as strings, or the packer drops the toleration)
    many = [tol("s%d" % j) for j in range(1, 6)] + [tol("k0", "Equal", "v"), tol("maint"), tol("k3", "Exists", "", "NoExecute")]
    P.append(({"clusterTolerations": few}, {}))
    P.append(({"clusterTolerations": many, "clusterAffinity": _aff([_lbl("env", "NotIn", ["a"])])}, {}))
    P.append(({"clusterTolerations": [tol("", "Exists", "", "NoSchedule")]}, {}))
    P.append(({"clusterTolerations": [tol("")]}, {}))
    P.append(({"clusterTolerations": [tol("k%d" % j) for j in range(0, 62, 2)]}, {}))
    # spec.Clusters members that fail APIEnablement and TaintToleration pass through
    # TargetContains; eviction tasks remove clusters again
    tgt = [{"name": n, "replicas": 1} for n in names[:5] + some]
    P.append(({}, {"apiVersion": "nope/v9", "kind": "Thing", "clusters": tgt}))
    P.append(({"clusterAffinity": _aff([_lbl("shard", "NotIn", ["s1"])])},
              {"apiVersion": "nope/v9", "kind": "Thing", "clusters": tgt,
               "gracefulEvictionTasks": [{"fromCluster": names[0]}, {"fromCluster": some[-1]}]}))
    P.append(({"clusterTolerations": few, "spreadConstraints": [{"spreadByField": "zone", "maxGroups": 2, "minGroups": 1}]},
              {"clusters": tgt[:3], "gracefulEvictionTasks": [{"fromCluster": names[len(names) // 2]}]}))
    out = []
    for p, extra in P:
        d = {"apiVersion": "apps/v1", "kind": "Deployment", "replicas": 3, "placement": p,
             "schedulerObservedAffinityName": "t0"}
        d.update(extra)
        out.append(d)
    return out


# (cluster count, seed, distinct taint lists)
UNIVERSES = [(1, 11, 2), (64, 12, 5), (65, 13, 5), (200, 14, 64), (4096, 15, 9), (4097, 16, 9), (8192, 17, 3),
             (8193, 18, 3)]
IDS = ["C%d" % u[0] for u in UNIVERSES]
# shapes kept at the large counts: no affinity, one value, NotIn of absent values, several
# terms, > 64 values, both mixed shapes, 128 and 129 row references, > 64 terms, > 64
# instructions, tolerations (several, past the registers, any key), spec.Clusters + eviction
LARGE = [0, 1, 3, 8, 9, 11, 12, 13, 14, 16, 17, 19, 20, 21, 25, 26]


@functools.lru_cache(maxsize=None)
def _universe(nc, seed, tsets):
    """Clusters, bindings and the oracle's answer: computed once, shared by every test."""
    clusters = _clusters(nc, seed, tsets)
    bindings = _shapes([c["name"] for c in clusters])
    if nc >= 4096:  # the word loop is what these counts are about: one binding of each kind
        bindings = [bindings[i] for i in LARGE]
    opts = api.options()
    return clusters, bindings, [sorted(x) for x in _oracle(clusters, bindings, opts)]


def _check(engine, u, rows):
    clusters, bindings, want = _universe(*u)
    got = _filter(engine, clusters, bindings, api.options(), rows)
    bad = [i for i in range(len(bindings)) if sorted(got[i]) != want[i]]
    assert not bad, (bad, len(got[bad[0]]), len(want[bad[0]]), bindings[bad[0]]["placement"])


def test_shapes_are_not_trivial():
    """The shapes select something and not everything where they are meant to."""
    clusters, bindings, want = _universe(200, 14, 64)
    live = sum(1 for c in clusters if not c["deleting"])
    sizes = [len(w) for w in want]
    assert sizes[2] == 0 and sizes[5] == 0              # absent value under In, OP_FALSE
    assert 0 < sizes[1] < live and 0 < sizes[8] < live and 0 < sizes[11] < live
    assert 0 < sizes[13] <= sizes[14] < live            # 128 and 129 row references (one shard more)
    assert len(set(sizes)) > 12


@pytest.mark.parametrize("rows", [False, True], ids=["bits", "rows"])
@pytest.mark.parametrize("u", UNIVERSES, ids=IDS)
def test_filter_plan_cpusim(cpusim_engine, u, rows):
    _check(cpusim_engine, u, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [False, True], ids=["bits", "rows"])
@pytest.mark.parametrize("u", UNIVERSES, ids=IDS)
def test_filter_plan_gpu(gpu_engine, u, rows):
    _check(gpu_engine, u, rows)
