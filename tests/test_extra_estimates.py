"""kp_batch_create_estimates: the other ReplicaEstimators' answers merged into a batch's
available replicas (calAvailableReplicas, pkg/scheduler/core/util.go:57-110, and
mergeReplicaResults, util.go:157-170).

The oracle computes the GeneralEstimator only, so the expected placements come from the
oracle over a capped world: for the GeneralEstimator min(general(c), x) with x >= 0 is what
the oracle computes for cluster c once its allocatable.pods is lowered so that the allowed
pod number becomes min(allowed, x) (oracle.cpp maxAvailableReplicas), and for a
component-set binding min(allowed, x * podsPerSet) (maxAvailableComponentSets). -1 entries
leave the cluster alone. One world per row (and per podsPerSet for component sets);
test_capped_cluster_is_the_minimum proves the helper on the oracle alone."""
import ctypes as C
import os

import numpy as np
import pytest

from karmada_amd import api, synth
from karmada_amd.engine import Batch, EngineError, PackCache, Snapshot
import oracle_lib as O

MAXI = 2**31 - 1
ENGINES = [pytest.param("cpusim_engine", id="cpusim"),
           pytest.param("gpu_engine", id="gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=ENGINES)
def eng(request):
    os.environ.setdefault("KP_CPUSIM_THREADS", "8")
    return request.getfixturevalue(request.param)


# ---------------------------------------------------------------------------------------
# the capped world
# ---------------------------------------------------------------------------------------
def _s(x):
    return C.string_at(x.ptr, x.len).decode() if x.len else ""


def _oracle():
    L = O.lib()
    L.kpo_estimator_part.argtypes = [C.POINTER(api.kp_cluster), C.POINTER(api.kp_binding), C.POINTER(api.kp_options),
                                     C.c_int, C.c_int, C.POINTER(C.c_int64)]
    return L


def allowed_pods(u):
    """getAllowedPodNumber of every cluster of the universe (kpo_estimator_part, part 3)."""
    if not hasattr(u, "_allowed"):
        L, opts, b, out = _oracle(), api.options(), api.kp_binding(), C.c_int64()
        u._allowed = []
        for c in range(u.n_clusters):
            L.kpo_estimator_part(C.byref(u.clusters[c]), C.byref(b), C.byref(opts), 3, O.FAST, C.byref(out))
            u._allowed.append(int(out.value))
    return u._allowed


def cap_cluster(cl, allowed, cap, keep):
    """A copy of kp_cluster `cl` whose allowed pod number is min(allowed, cap): allocatable.pods
    holds that number, and the allocated / allocating lists lose their pods entries."""
    out = api.kp_cluster.from_buffer_copy(cl)
    if not cl.has_resource_summary or allowed <= 0 or cap >= allowed:
        return out  # (no summary, or nothing allowed: the answer is 0 either way)
    q = str(int(cap)).encode()
    keep.append(q)
    alloc = (api.kp_resource * cl.n_allocatable)()
    seen = False
    for j in range(cl.n_allocatable):
        alloc[j] = cl.allocatable[j]
        if _s(cl.allocatable[j].name) == "pods":
            alloc[j].quantity = api.kp_str(q, len(q))
            seen = True
    assert seen  # allowed > 0 needs allocatable.pods
    keep.append(alloc)
    out.allocatable = alloc
    for field, nfield in (("allocated", "n_allocated"), ("allocating", "n_allocating")):
        src, n = getattr(cl, field), getattr(cl, nfield)
        rest = [src[j] for j in range(n) if _s(src[j].name) != "pods"]
        arr = (api.kp_resource * max(1, len(rest)))(*rest)
        keep.append(arr)
        setattr(out, field, arr)
        setattr(out, nfield, len(rest))
    return out


def capped_world(u, row, pods_per_set=0):
    """The universe's clusters capped by `row` (caller order; -1 leaves a cluster alone).
    pods_per_set > 0: the component-set cap x * podsPerSet."""
    al, keep = allowed_pods(u), []
    ca = (api.kp_cluster * u.n_clusters)()
    for c in range(u.n_clusters):
        x = int(row[c])
        cap = al[c] if x < 0 else (x * pods_per_set if pods_per_set > 0 else x)
        ca[c] = cap_cluster(u.clusters[c], al[c], cap, keep)
    keep.append(ca)
    return ca, keep


def pods_per_set(b):
    return sum(int(b.components[j].replicas) for j in range(b.n_components))


def takes_sets(b, opts):
    if not opts.multiple_pod_templates_scheduling or b.n_components == 0:
        return False
    return any(_s(b.spread_constraints[j].spread_by_field) == "cluster" and
               b.spread_constraints[j].min_groups == 1 and b.spread_constraints[j].max_groups == 1
               for j in range(b.n_spread_constraints))


def binding_array(u, idx):
    ba = (api.kp_binding * max(1, len(idx)))()
    for k, i in enumerate(idx):
        ba[k] = u.bindings[i]
    return ba


def expected(u, ba, n, opts, rows, row_of):
    """The oracle's placements of bindings ba[0, n): each over its row's world."""
    groups = {}
    for i in range(n):
        r = int(row_of[i])
        if r < 0:
            key = (-1, 0)
        else:
            pps = pods_per_set(ba[i]) if takes_sets(ba[i], opts) else 0
            # (podsPerSet <= 0: the answer is the allowed pod number itself, capped as a replica count)
            key = (r, pps if pps > 0 else 0)
        groups.setdefault(key, []).append(i)
    out = [None] * n
    for (r, pps), idx in sorted(groups.items()):
        if r < 0:
            ca, keep = u.clusters, None
        else:
            ca, keep = capped_world(u, rows[r], pps)
        sub = (api.kp_binding * len(idx))()
        for k, i in enumerate(idx):
            sub[k] = ba[i]
        res = O.schedule_c(ca, u.n_clusters, sub, len(idx), opts, O.FAST, 4)
        for k, i in enumerate(idx):
            out[i] = res[k]
        del keep
    return out


def compare(got, want, label):
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    if bad:
        msg = [f"{label}: {len(bad)}/{len(want)} differ"]
        for i in bad[:4]:
            msg += [f"  {i}: engine={got[i]}", f"  {i}: oracle={want[i]}"]
        pytest.fail("\n".join(msg))


def make_rows(seed, n_rows, n_clusters, small=24):
    """Rows holding -1, 0, small answers (below most general answers), answers far above
    them, and MaxInt32. Row r leaves 3 * (15, 5, 2)[r % 3] percent of the clusters to the
    general answer (-1, far above, MaxInt32), so some rows bind nearly everywhere."""
    rng = np.random.RandomState(seed)
    kind = rng.randint(0, 100, size=(n_rows, n_clusters))
    rows = rng.randint(1, small, size=(n_rows, n_clusters)).astype(np.int64)
    p = np.array([(15, 5, 2)[r % 3] for r in range(n_rows)])[:, None]
    rows[kind < p] = -1
    rows[(kind >= p) & (kind < 2 * p)] = 10**6 + rng.randint(0, 1000)
    rows[(kind >= 2 * p) & (kind < 3 * p)] = MAXI
    rows[kind >= 88] = 0
    return rows.astype(np.int32)


def schedule_with(engine, u, ba, n, opts, estimates, env=None, **kw):
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=(ba, n), estimates=estimates, **kw)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        out = b.schedule()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    times = engine.stage_times()
    b.close()
    snap.close()
    return out, times


# ---------------------------------------------------------------------------------------
# the helper, on the oracle alone
# ---------------------------------------------------------------------------------------
def test_capped_cluster_is_the_minimum():
    L = _oracle()
    u = synth.Universe(6, 56, 40, 0, 200)
    opts = api.options()
    al = allowed_pods(u)
    no_summary = [c for c in range(u.n_clusters) if not u.clusters[c].has_resource_summary]
    assert no_summary, "the universe needs a cluster without a resource summary"
    bs = [i for i in range(u.n_bindings) if u.bindings[i].has_replica_requirements][:6] + \
         [i for i in range(u.n_bindings) if not u.bindings[i].has_replica_requirements][:2]
    triples = above = zero = 0
    for c in list(range(0, u.n_clusters, 3)) + no_summary:
        for i in bs:
            bp = C.byref(u.bindings[i])
            orig = L.kpo_max_available_replicas(C.byref(u.clusters[c]), bp, C.byref(opts), O.FAST)
            for x in (0, 1, 7, max(0, orig - 1), orig, orig + 1, 10**6, MAXI):
                keep = []
                cc = cap_cluster(u.clusters[c], al[c], x, keep)
                got = L.kpo_max_available_replicas(C.byref(cc), bp, C.byref(opts), O.FAST)
                assert got == min(orig, x), (c, i, x, orig, got)
                triples += 1
                above += x > orig
                zero += x == 0
    assert triples >= 300 and above >= 50 and zero >= 30


def test_kp_estimates_layout(tmp_path):
    """The ctypes mirror of kp_estimates has the header's layout (size and field offsets,
    compiled from the header itself), and the ABI version is 16."""
    import subprocess
    from karmada_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "est.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kp/kp_api.h"\nint main(void) {\n'
                   '  printf("%d %zu %zu %zu %zu %zu\\n", KP_ABI_VERSION, sizeof(kp_estimates),\n'
                   '         offsetof(kp_estimates, n_rows), offsetof(kp_estimates, n_clusters),\n'
                   '         offsetof(kp_estimates, rows), offsetof(kp_estimates, row_of));\n  return 0;\n}\n')
    exe = tmp_path / "est"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    E = api.kp_estimates
    assert got == [engine.KP_ABI_VERSION, C.sizeof(E), E.n_rows.offset, E.n_clusters.offset, E.rows.offset,
                   E.row_of.offset]
    assert engine.KP_ABI_VERSION == 16


# ---------------------------------------------------------------------------------------
# case 1: the mixed batch (and its pair-row reruns, case 3)
# ---------------------------------------------------------------------------------------
def _s_kind(b):
    fields = tuple(_s(b.spread_constraints[j].spread_by_field) for j in range(b.n_spread_constraints))
    if b.replicas == 0 and b.n_components == 0:
        return "nonworkload"
    if fields == ("cluster",):
        return "cluster-spread"
    if fields == ("region", "cluster"):
        return "region-spread"
    if fields:
        return None
    if not b.has_replica_scheduling:
        return None
    if _s(b.replica_scheduling_type) == "Duplicated":
        strat = "dup"
    elif _s(b.replica_division_preference) == "Aggregated":
        strat = "agg"
    elif _s(b.dynamic_weight):
        strat = "dyn"
    elif b.has_weight_preference:
        strat = "static"
    else:
        return None
    return strat + ("+prev" if b.n_clusters > 0 else "")


MIXED_KINDS = ("dup", "dup+prev", "static", "static+prev", "dyn", "dyn+prev", "agg", "agg+prev", "cluster-spread",
               "region-spread", "nonworkload")


# (Duplicated, StaticWeight and non-workload bindings do not read the estimates: fewer of them)
MIXED_DEFAULT = {"dup": 2, "dup+prev": 2, "static": 2, "static+prev": 2, "dyn": 7, "dyn+prev": 6, "agg": 7, "agg+prev": 6,
                 "cluster-spread": 6, "region-spread": 6, "nonworkload": 2}


def pick_mixed(u, per_kind):
    """Bindings of the edge workload by kind: every strategy, with and without a previous
    spec.Clusters, cluster spread, region spread and non-workloads, in binding order."""
    got = {k: [] for k in MIXED_KINDS}
    for i in range(u.n_bindings):
        k = _s_kind(u.bindings[i])
        if k in got and len(got[k]) < per_kind.get(k, 4):
            got[k].append(i)
    assert all(got[k] for k in MIXED_KINDS), {k: len(v) for k, v in got.items()}
    return sorted(i for v in got.values() for i in v)


def request_key(b):
    if not b.has_replica_requirements:
        return None
    return tuple(sorted((_s(b.resource_request[j].name), _s(b.resource_request[j].quantity))
                        for j in range(b.n_resource_request)))


_MIXED = {}


def mixed_case(n_clusters, n_rows=3, per_kind=None, seed=11):
    """(universe, bindings, n, opts, rows, row_of, want, want_plain), computed once per shape."""
    key = (n_clusters, n_rows, seed)
    if key not in _MIXED:
        u = synth.Universe(6, seed, n_clusters, 0, 900)
        idx = pick_mixed(u, per_kind or MIXED_DEFAULT)
        ba, n = binding_array(u, idx), len(idx)
        opts = api.options()
        rows = make_rows(100 + n_clusters, n_rows, n_clusters)
        row_of = np.array([(k % (n_rows + 1)) - 1 for k in range(n)], dtype=np.int32)
        want = expected(u, ba, n, opts, rows, row_of)
        plain = O.schedule_c(u.clusters, u.n_clusters, ba, n, opts, O.FAST, 4)
        _MIXED[key] = (u, ba, n, opts, rows, row_of, want, plain)
    return _MIXED[key]


@pytest.mark.parametrize("n_clusters", [64, 65, 130])
def test_mixed_batch(eng, n_clusters):
    u, ba, n, opts, rows, row_of, want, plain = mixed_case(n_clusters)
    assert 40 <= n <= 56
    # the rows hold every kind of entry
    assert (rows == -1).any() and (rows == 0).any() and (rows == MAXI).any() and ((rows > 10**5) & (rows < MAXI)).any()
    # classes: the same requests with different rows, different requests with the same row
    by_req, by_row = {}, {}
    for i in range(n):
        if _s_kind(ba[i]) == "nonworkload":
            continue
        by_req.setdefault(request_key(ba[i]), set()).add(int(row_of[i]))
        by_row.setdefault(int(row_of[i]), set()).add(request_key(ba[i]))
    assert any(len(v) > 1 for v in by_req.values()) and any(len(v) > 1 for k, v in by_row.items() if k >= 0)
    # not vacuous (oracle results only): the rows change a quarter of the bindings that have one
    with_row = [i for i in range(n) if row_of[i] >= 0]
    moved = [i for i in with_row if want[i] != plain[i]]
    assert 4 * len(moved) >= len(with_row), (len(moved), len(with_row))
    got, _ = schedule_with(eng, u, ba, n, opts, (rows, row_of))
    compare(got, want, f"mixed batch C={n_clusters}")


@pytest.mark.parametrize("env", [{"KP_PAIR_ROWS": "1"}, {"KP_PAIR_GENERIC": "1"}], ids=["pair-rows", "pair-generic"])
@pytest.mark.parametrize("n_clusters", [64, 65, 130])
def test_mixed_batch_pair_row_mode(eng, n_clusters, env):
    u, ba, n, opts, rows, row_of, want, _ = mixed_case(n_clusters)
    got, times = schedule_with(eng, u, ba, n, opts, (rows, row_of), env=env)
    assert times["bits"] == 0
    compare(got, want, f"mixed batch C={n_clusters} {env}")


# ---------------------------------------------------------------------------------------
# case 2: neutral inputs
# ---------------------------------------------------------------------------------------
def test_neutral_inputs(eng):
    u, ba, n, opts, rows, row_of, _, plain = mixed_case(65)
    # an all -1 row: the batch without estimates
    none = np.full((1, u.n_clusters), -1, dtype=np.int32)
    got, _ = schedule_with(eng, u, ba, n, opts, (none, np.zeros(n, dtype=np.int32)))
    compare(got, plain, "all -1 row")
    # est == NULL and n_rows == 0: the digest of kp_batch_create
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, opts)
    b0 = Batch(snap, structs=(ba, n))
    h = C.c_void_p()
    eng._check(eng.L.kp_batch_create_estimates(eng.h, snap.h, ba, None, n, None, None, C.byref(h)),
               "kp_batch_create_estimates")
    d = C.c_uint64()
    eng._check(eng.L.kp_batch_digest(h, C.byref(d)), "kp_batch_digest")
    eng.L.kp_batch_destroy(h)
    b1 = Batch(snap, structs=(ba, n), estimates=(np.zeros((0, u.n_clusters), dtype=np.int32), np.zeros(n)))
    assert d.value == b0.digest() == b1.digest()
    b2 = Batch(snap, structs=(ba, n), estimates=(rows, row_of))
    assert b2.digest() != b0.digest()  # (the class split shows in the digest)
    for b in (b0, b1, b2):
        b.close()
    snap.close()
    # a non-workload binding with a row is unchanged (it calls no estimator)
    nw = [i for i in range(u.n_bindings) if _s_kind(u.bindings[i]) == "nonworkload"][:16]
    wl = [i for i in range(u.n_bindings) if _s_kind(u.bindings[i]) == "dyn"][:4]
    bn, m = binding_array(u, nw + wl), len(nw) + len(wl)
    zero = np.zeros((1, u.n_clusters), dtype=np.int32)
    ro = np.array([0] * len(nw) + [-1] * len(wl), dtype=np.int32)
    want = O.schedule_c(u.clusters, u.n_clusters, bn, m, opts, O.FAST, 4)
    assert sum(1 for k in range(len(nw)) if want[k]["status"] == api.STATUS_OK and want[k]["targets"]) >= 4
    got, _ = schedule_with(eng, u, bn, m, opts, (zero, ro))
    compare(got, want, "non-workload bindings with an all-zero row")


# ---------------------------------------------------------------------------------------
# case 4: no class orders (singleton classes), case 5: class orders and k_select_top
# ---------------------------------------------------------------------------------------
_SHARED = {}


def test_singleton_classes_without_orders(eng):
    if "single" not in _SHARED:
        u = synth.Universe(10, 5, 200, 0, 40)
        ba, n, opts = u.bindings, u.n_bindings, api.options()
        assert len({request_key(ba[i]) for i in range(n)}) == n  # every binding its own request
        assert all(_s_kind(ba[i]) in ("dyn", "agg", "dyn+prev", "agg+prev") for i in range(n))
        rows = make_rows(7, 4, u.n_clusters, small=12)
        row_of = np.array([(i // 2) % 4 if i % 2 == 0 else -1 for i in range(n)], dtype=np.int32)
        want = expected(u, ba, n, opts, rows, row_of)
        plain = O.schedule_c(u.clusters, u.n_clusters, ba, n, opts, O.FAST, 4)
        assert sum(want[i] != plain[i] for i in range(n) if row_of[i] >= 0) >= n // 8
        _SHARED["single"] = (u, ba, n, opts, rows, row_of, want)
    u, ba, n, opts, rows, row_of, want = _SHARED["single"]
    eng.set_profile(True)
    try:
        got, times = schedule_with(eng, u, ba, n, opts, (rows, row_of))
        kt = eng.kernel_times()
    finally:
        eng.set_profile(False)
    compare(got, want, "singleton classes")
    assert times["bits"] == 1 and "k_class_order" not in kt and "k_est_extra" in kt
    # the bindings without a row keep the feasible-only rows of the singleton classes
    assert any("(feasible)" in k for k in kt), sorted(kt)
    assert kt["k_est_extra"]["units"] == int((row_of >= 0).sum())


def test_class_orders_and_select_top(eng):
    if "orders" not in _SHARED:
        u = synth.Universe(3, 3, 300, 0, 4000)
        by_req = {}
        for i in range(u.n_bindings):
            by_req.setdefault(request_key(u.bindings[i]), []).append(i)
        kinds = sorted(by_req, key=lambda k: -len(by_req[k]))[:4]
        assert len(kinds) == 4 and all(len(by_req[k]) >= 64 for k in kinds)
        idx = sorted(i for k in kinds for i in by_req[k][:64])
        ba, n, opts = binding_array(u, idx), len(idx), api.options()
        assert n == 256
        rows = make_rows(9, 3, u.n_clusters, small=40)
        row_of = np.array([k % 3 for k in range(n)], dtype=np.int32)
        assert len({(request_key(ba[k]), int(row_of[k])) for k in range(n)}) == 12
        want = expected(u, ba, n, opts, rows, row_of)
        _SHARED["orders"] = (u, ba, n, opts, rows, row_of, want)
    u, ba, n, opts, rows, row_of, want = _SHARED["orders"]
    got, times = schedule_with(eng, u, ba, n, opts, (rows, row_of))
    compare(got, want, "class orders")
    assert times["bits"] == 1 and times["n_top"] > 0


# ---------------------------------------------------------------------------------------
# case 6: component sets
# ---------------------------------------------------------------------------------------
def test_component_sets(eng):
    if "sets" not in _SHARED:
        u = synth.Universe(9, 1, 70, 0, 400)
        opts = api.options(multi_templates=True)
        sets = [i for i in range(u.n_bindings) if takes_sets(u.bindings[i], opts)][:30]
        other = [i for i in range(u.n_bindings) if not takes_sets(u.bindings[i], opts)][:10]
        idx = sorted(sets + other)
        ba, n = binding_array(u, idx), len(idx)
        assert len(sets) == 30 and len({pods_per_set(u.bindings[i]) for i in sets}) > 1
        rows = make_rows(13, 3, u.n_clusters, small=6)
        row_of = np.array([(k % 4) - 1 for k in range(n)], dtype=np.int32)
        want = expected(u, ba, n, opts, rows, row_of)
        plain = O.schedule_c(u.clusters, u.n_clusters, ba, n, opts, O.FAST, 4)
        moved = [k for k in range(n) if row_of[k] >= 0 and takes_sets(ba[k], opts) and want[k] != plain[k]]
        assert len(moved) >= 5, len(moved)
        _SHARED["sets"] = (u, ba, n, opts, rows, row_of, want)
    u, ba, n, opts, rows, row_of, want = _SHARED["sets"]
    got, _ = schedule_with(eng, u, ba, n, opts, (rows, row_of))
    compare(got, want, "component sets")
    got, times = schedule_with(eng, u, ba, n, opts, (rows, row_of), env={"KP_PAIR_ROWS": "1"})
    assert times["bits"] == 0
    compare(got, want, "component sets, pair rows")


# ---------------------------------------------------------------------------------------
# case 7: keyed cycles, case 8: the other schedule forms
# ---------------------------------------------------------------------------------------
def test_keyed_cycles_follow_their_rows(eng):
    u, ba, n, opts, rows, row_of, want, _ = mixed_case(65)
    if "keyed" not in _SHARED:
        rows2 = make_rows(777, 3, u.n_clusters)
        row_of2 = np.roll(row_of, 1)
        _SHARED["keyed"] = (rows2, row_of2, expected(u, ba, n, opts, rows2, row_of2))
    rows2, row_of2, want2 = _SHARED["keyed"]
    assert want2 != want
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, opts)
    cache = PackCache(eng)
    b1 = Batch(snap, structs=(ba, n), cache=cache, generations=[1] * n, estimates=(rows, row_of))
    assert cache.stats()["last_hits"] == 0
    compare(b1.schedule(), want, "keyed cycle 1")
    b2 = Batch(snap, structs=(ba, n), cache=cache, generations=[1] * n, estimates=(rows2, row_of2))
    assert cache.stats()["last_hits"] == n
    compare(b2.schedule(), want2, "keyed cycle 2")
    # the records hold the request key alone: a cycle without estimates is kp_batch_create's batch
    b3 = Batch(snap, structs=(ba, n), cache=cache, generations=[1] * n)
    b4 = Batch(snap, structs=(ba, n))
    assert cache.stats()["last_hits"] == n and b3.digest() == b4.digest()
    for b in (b1, b2, b3, b4):
        b.close()
    cache.close()
    snap.close()


def test_other_schedule_forms(eng):
    u, ba, n, opts, rows, row_of, want, _ = mixed_case(130)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, opts)
    b = Batch(snap, structs=(ba, n), estimates=(rows, row_of))
    compare(b.schedule(), want, "schedule")
    compare(b.schedule(), want, "a second schedule call")
    b.submit()
    r = b.collect()
    compare(api.results_to_python(r.status, r.err_code, r.err_arg, r.offsets, r.cluster_idx, r.replicas, r.n_bindings),
            want, "submit / collect")
    compare(b.schedule(packed=True), want, "packed")
    b.submit_packed()
    p = b.collect_packed()
    ci, rep = b.unpack(p)
    compare(api.results_to_python(p.status, p.err_code, p.err_arg, p.offsets, ci, rep, p.n_bindings), want,
            "submit / collect, packed")
    b.close()
    snap.close()


# ---------------------------------------------------------------------------------------
# case 9: validation, case 10: nothing new without estimates
# ---------------------------------------------------------------------------------------
def test_validation(eng):
    u, ba, n, opts, rows, row_of, _, _ = mixed_case(65)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, opts)

    def rejected(r, ro, text):
        with pytest.raises(EngineError) as ei:
            Batch(snap, structs=(ba, n), estimates=(r, ro))
        assert "rc=-1" in str(ei.value) and text in str(ei.value), str(ei.value)

    rejected(rows[:, :64], row_of, "n_clusters")
    rejected(np.concatenate([rows, rows[:, :1]], axis=1), row_of, "n_clusters")
    for v in (3, -2):
        ro = row_of.copy()
        ro[5] = v
        rejected(rows, ro, "row_of[5]")
    r = rows.copy()
    r[1, 17] = -2
    rejected(r, row_of, "rows[1][17]")
    # the per-pair estimator entry point keeps the GeneralEstimator's answer
    b = Batch(snap, structs=(ba, n), estimates=(rows, row_of))
    b.schedule()
    L = O.lib()
    idx = (C.c_uint32 * u.n_clusters)(*range(u.n_clusters))
    out = (C.c_int32 * u.n_clusters)()
    checked = lowered = 0
    for i in range(n):
        if row_of[i] < 0 or _s_kind(ba[i]) == "nonworkload":
            continue
        eng._check(eng.L.kp_max_available_replicas(eng.h, b.h, i, idx, u.n_clusters, out), "kp_max_available_replicas")
        for c in range(u.n_clusters):
            g = L.kpo_max_available_replicas(C.byref(u.clusters[c]), C.byref(ba[i]), C.byref(opts), O.FAST)
            assert out[c] == g, (i, c, out[c], g)
            lowered += 0 <= rows[row_of[i], c] < g
        checked += 1
    assert checked >= 20 and lowered > 100  # (the rows would have lowered these answers)
    b.close()
    snap.close()


def test_no_new_work_without_estimates(eng):
    u, ba, n, opts, rows, row_of, _, _ = mixed_case(65)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, opts)
    eng.set_profile(True)
    try:
        b = Batch(snap, structs=(ba, n), estimates=(rows, row_of))
        b.schedule()
        with_est = eng.kernel_times()
        b.close()
        b = Batch(snap, structs=(ba, n))
        b.schedule()
        without = eng.kernel_times()
        b.close()
        # rows that no binding uses: nothing to merge either
        b = Batch(snap, structs=(ba, n), estimates=(rows, np.full(n, -1, dtype=np.int32)))
        b.schedule()
        unused = eng.kernel_times()
        b.close()
    finally:
        eng.set_profile(False)
        snap.close()
    assert "k_est_extra" in with_est and with_est["k_est_extra"]["launches"] == 1
    assert "k_est_extra" not in without and "k_est_extra" not in unused
    assert set(with_est) - {"k_est_extra"} == set(without)


# ---------------------------------------------------------------------------------------
# case 11: rows that span many workgroups
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_large_rows(gpu_engine):
    u, ba, n, opts, rows, row_of, want, plain = mixed_case(5000, n_rows=8, per_kind={
        "dup": 5, "dup+prev": 5, "static": 5, "static+prev": 5, "dyn": 8, "dyn+prev": 6, "agg": 8, "agg+prev": 6,
        "cluster-spread": 6, "region-spread": 6, "nonworkload": 4})
    assert n == 64
    assert sum(want[i] != plain[i] for i in range(n) if row_of[i] >= 0) >= 8
    got, _ = schedule_with(gpu_engine, u, ba, n, opts, (rows, row_of))
    compare(got, want, "C = 5000")
