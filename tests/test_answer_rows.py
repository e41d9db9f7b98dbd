"""The one intake of kp_estimates / kp_filter_answers (csrc/answers.cpp): the same checks and
the same device-ranked, shared rows behind kp_batch_create_estimates / _filters and
kp_schedule_affinities_ex.

The reference side is the oracle alone, by the constructions of test_extra_estimates (an
estimate row is the oracle over a world whose allocatable pods the row caps), of
test_extra_filters (a verdict row is the oracle over the binding with the rejected clusters
evicted) and of test_affinities_answers (the retry loop restated, one oracle call a round).
The expected error texts are literals recorded from the host build of the commit before the
intake was unified."""
import ctypes as C
import os

import numpy as np
import pytest

from karmada_amd import api, engine as E, synth
from karmada_amd.engine import Batch, Snapshot
import oracle_lib as O
import test_affinities_answers as TA
import test_extra_estimates as TE
import test_extra_filters as TF

ENGINES = [pytest.param("cpusim_engine", id="cpusim"),
           pytest.param("gpu_engine", id="gpu", marks=pytest.mark.gpu)]
SHAPES = [64, 65, 130]  # exactly one word; one cluster into a second word; three words with padding
OK = api.STATUS_OK


@pytest.fixture(params=ENGINES)
def eng(request):
    os.environ.setdefault("KP_CPUSIM_THREADS", "8")
    return request.getfixturevalue(request.param)


# ---------------------------------------------------------------------------------------
# same answers, two doors
# ---------------------------------------------------------------------------------------
_DOORS = {}


def doors_case(n_clusters):
    """56 bindings of the edge workload with no ClusterAffinities term or exactly one, three
    estimate rows and four verdict rows (all pass, none passes, half, most), and what the
    oracle places with and without them; once per shape."""
    if n_clusters not in _DOORS:
        u = synth.Universe(6, 11, n_clusters, 0, 900)
        per_kind, idx = {}, []
        for i in range(u.n_bindings):
            b, k = u.bindings[i], TE._s_kind(u.bindings[i])
            if k is None or b.n_cluster_affinities > 1 or per_kind.get((k, b.n_cluster_affinities), 0) >= 4:
                continue
            per_kind[(k, int(b.n_cluster_affinities))] = per_kind.get((k, int(b.n_cluster_affinities)), 0) + 1
            idx.append(i)
        idx = idx[:56]
        ba, n = TE.binding_array(u, idx), len(idx)
        for k in range(n):  # (the one term is the current one for kp_schedule_batch too)
            if ba[k].n_cluster_affinities:
                ba[k].observed_affinity_name = ba[k].cluster_affinities[0].affinity_name
        opts = api.options()
        rng = np.random.RandomState(400 + n_clusters)
        erows = TE.make_rows(300 + n_clusters, 3, n_clusters)
        erow_of = np.array([(k % 4) - 1 for k in range(n)], dtype=np.int32)
        ok = np.array([np.ones(n_clusters, bool), np.zeros(n_clusters, bool), rng.rand(n_clusters) < 0.5,
                       rng.rand(n_clusters) < 0.9])
        frow_of = np.array([(2, 3, -1, 2, 0, 3, 2, 1, 3)[k % 9] for k in range(n)], dtype=np.int32)
        want = TF.expected(u, ba, n, opts, ok, frow_of, estimates=(erows, erow_of))
        plain = O.schedule_c(u.clusters, u.n_clusters, ba, n, opts, O.FAST, 4)
        _DOORS[n_clusters] = dict(u=u, ba=ba, n=n, opts=opts, est=(erows, erow_of), ok=ok, frow_of=frow_of,
                                  want=want, plain=plain)
    return _DOORS[n_clusters]


def through_both_doors(eng, c, label):
    u, ba, n, opts, want = c["u"], c["ba"], c["n"], c["opts"], c["want"]
    terms = [int(ba[i].n_cluster_affinities) for i in range(n)]
    assert n <= 64 and set(terms) == {0, 1} and terms.count(1) >= 8
    # not vacuous (oracle results only)
    assert 2 * sum(w["status"] == OK for w in want) >= n
    assert sum(w["targets"] != p["targets"] for w, p in zip(want, c["plain"])) >= 8
    batch, _ = TF.schedule_with(eng, u, ba, n, opts, (c["ok"], c["frow_of"], 1), estimates=c["est"])
    TE.compare(batch, want, f"{label}: kp_batch_create_filters + kp_schedule_batch")
    res, aff, att, rounds = TA.run(eng, c, estimates=c["est"], filters=(c["ok"], [[int(r)] for r in c["frow_of"]], 1))
    TE.compare(res, want, f"{label}: kp_schedule_affinities_ex")
    assert rounds == 1 and att == [1] * n
    assert aff == [0 if t and w["status"] == OK else -1 for t, w in zip(terms, want)]
    assert res == batch


@pytest.mark.parametrize("n_clusters", SHAPES)
def test_same_answers_two_doors(eng, n_clusters):
    through_both_doors(eng, doors_case(n_clusters), f"C={n_clusters}")


def test_dirty_pool(eng):
    """A larger batch without rows is created, scheduled and destroyed first, so the pooled
    blocks the rows and their staging copy take have been written before: the padding
    ([65, 128) of an estimate row, bits 1..63 of a verdict row's second word) must still read
    as -1 / zero bits."""
    c = doors_case(65)
    u = c["u"]
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, c["opts"])
    b = Batch(snap, structs=u.binding_slice(0, 300))
    assert len(b.schedule()) == 300 > c["n"]
    b.close()
    snap.close()
    through_both_doors(eng, c, "dirty pool")


# ---------------------------------------------------------------------------------------
# one batch after another on shared rows
# ---------------------------------------------------------------------------------------
_ROUNDS = {}


def rounds_case():
    """48 two-term bindings at C = 130, five estimate rows, and verdict rows per term of which
    every third binding's first attempted term gets the all-zero row."""
    if not _ROUNDS:
        u = synth.Universe(6, 5, 130, 0, TA.N_UNIVERSE)
        idx = [i for i in range(u.n_bindings) if TE._s_kind(u.bindings[i]) and
               u.bindings[i].n_cluster_affinities == 2 and TA.start_term(u.bindings[i]) == 0][:48]
        ba, n = TE.binding_array(u, idx), len(idx)
        opts = api.options()
        rng = np.random.RandomState(77)
        erows = TE.make_rows(77, 5, 130)
        erow_of = np.array([(k % 6) - 1 for k in range(n)], dtype=np.int32)
        ok = np.array([np.ones(130, bool), np.zeros(130, bool), rng.rand(130) < 0.5, rng.rand(130) < 0.9])
        per_term = [[1, (0, 2, 3)[(k // 3) % 3]] if k % 3 == 0 else [(2, 3, -1)[k % 3], 3] for k in range(n)]
        want = TA.oracle_term_loop(u, ba, n, opts, est=(erows, erow_of), flt=(ok, per_term))
        _ROUNDS.update(u=u, ba=ba, n=n, opts=opts, est=(erows, erow_of), ok=ok, per_term=per_term, want=want)
    return _ROUNDS


def test_rounds_share_the_rows(eng):
    c = rounds_case()
    n, want = c["n"], c["want"]
    assert n == 48
    # not vacuous (oracle results only): second attempts happen, and some succeed there
    assert sum(a >= 2 for a in want[2]) >= n // 3 and sum(a == 1 for a in want[1]) >= 4
    got = TA.run(eng, c, estimates=c["est"], filters=(c["ok"], c["per_term"], 1))
    assert got[3] >= 2
    TA.compare(got, want, "two rounds on shared rows")
    assert TA.run(eng, c, estimates=c["est"], filters=(c["ok"], c["per_term"], 1)) == got


# ---------------------------------------------------------------------------------------
# pinned texts: one wrong input per check and entry point
# ---------------------------------------------------------------------------------------
# 6 bindings with 0, 1, 2, 0, 1, 2 terms (term_off 0 1 2 4 5 6 8) over 64 clusters, 2 estimate
# rows and 3 verdict rows.
EST_FAULTS = [
    ("n_clusters", "n_clusters is 63, the snapshot holds 64 clusters"),
    ("rows_null", "rows or row_of is null"),
    ("row_of_null", "rows or row_of is null"),
    ("n_rows", "more than 2^31 - 1 rows"),
    ("row_of_high", "row_of[3] = 2 is outside -1..1"),
    ("row_of_low", "row_of[3] = -2 is outside -1..1"),
    ("cell", "rows[1][17] = -2 is below -1 (UnauthenticReplica)"),
]
FLT_FAULTS = [
    ("n_clusters", "n_clusters is 63, the snapshot holds 64 clusters"),
    ("rows_null", "rows is null"),
    ("row_of_null", "row_of is null"),
    ("n_plugins", "n_rows is 3 with n_plugins == 0"),
    ("n_rows", "more than 2^31 - 1 rows"),
    ("row_of_high", "row_of[3] = 3 is outside -1..2"),
    ("row_of_low", "row_of[3] = -2 is outside -1..2"),
]
PINNED = (
    [("create_estimates", f, "kp_batch_create_estimates: " + t) for f, t in EST_FAULTS] +
    [("create_filters", f, "kp_batch_create_filters: " + t) for f, t in FLT_FAULTS] +
    [("affinities_est", "n_clusters", "kp_schedule_affinities_ex: est->n_clusters is 63, the snapshot holds 64 clusters"),
     ("affinities_est", "rows_null", "kp_schedule_affinities_ex: est->rows or est->row_of is null"),
     ("affinities_est", "row_of_null", "kp_schedule_affinities_ex: est->rows or est->row_of is null"),
     ("affinities_est", "n_rows", "kp_schedule_affinities_ex: est: more than 2^31 - 1 rows"),
     ("affinities_est", "row_of_high", "kp_schedule_affinities_ex: est->row_of[3] = 2 is outside -1..1"),
     ("affinities_est", "row_of_low", "kp_schedule_affinities_ex: est->row_of[3] = -2 is outside -1..1"),
     ("affinities_est", "cell",
      "kp_schedule_affinities_ex: est->rows[1][17] = -2 is below -1 (UnauthenticReplica)"),
     ("affinities_flt", "n_clusters", "kp_schedule_affinities_ex: flt->n_clusters is 63, the snapshot holds 64 clusters"),
     ("affinities_flt", "rows_null", "kp_schedule_affinities_ex: flt->rows is null"),
     ("affinities_flt", "row_of_null", "kp_schedule_affinities_ex: flt->row_of is null"),
     ("affinities_flt", "n_plugins", "kp_schedule_affinities_ex: flt->n_rows is 3 with n_plugins == 0"),
     ("affinities_flt", "n_rows", "kp_schedule_affinities_ex: flt: more than 2^31 - 1 rows"),
     ("affinities_flt", "row_of_high", "kp_schedule_affinities_ex: flt->row_of[3] = 3 is outside -1..2"),
     ("affinities_flt", "row_of_low", "kp_schedule_affinities_ex: flt->row_of[3] = -2 is outside -1..2"),
     ("affinities_flt", "term_off_null", "kp_schedule_affinities_ex: term_off is null while flt has rows"),
     ("affinities_flt", "term_off_down",
      "kp_schedule_affinities_ex: term_off is not non-decreasing: term_off[3] is below term_off[2]"),
     ("affinities_flt", "term_off_count",
      "kp_schedule_affinities_ex: term_off[3] - term_off[2] is 3, binding 2 has 2 term(s) (max(1, n_cluster_affinities))")])


def provoke(eng, snaps, ba, door, fault):
    """(rc, kp_last_error) of the entry point behind `door` given inputs right in everything
    but `fault`."""
    n, terms = 6, [1, 1, 2, 1, 1, 2]
    erows = np.full((2, 64), 5, dtype=np.int32)
    erow_of = np.array([0, 1, -1, 0, 1, -1], dtype=np.int32)
    words = np.full((3, 1), 2**64 - 1, dtype=np.uint64)
    frow_of = np.array([0, 1, 2, -1, 0, 1, 2, -1], dtype=np.int32)  # one entry per (binding, term)
    term_off = np.array([0, 1, 2, 4, 5, 6, 8], dtype=np.uint64)
    on_est = door in ("create_estimates", "affinities_est")
    if not door.startswith("affinities"):
        frow_of = frow_of[:n].copy()
    if fault == "cell":
        erows[1, 17] = -2
    if fault in ("row_of_high", "row_of_low"):
        (erow_of if on_est else frow_of)[3] = -2 if fault == "row_of_low" else (2 if on_est else 3)
    if fault == "term_off_down":
        term_off[3] = 1
    if fault == "term_off_count":
        term_off[3:] += 1
    est = api.kp_estimates(2, 64, erows.ctypes.data_as(C.POINTER(C.c_int32)), erow_of.ctypes.data_as(C.POINTER(C.c_int32)))
    flt = api.kp_filter_answers(3, 64, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                frow_of.ctypes.data_as(C.POINTER(C.c_int32)), 1)
    x = est if on_est else flt
    if fault == "n_clusters":
        x.n_clusters = 63
    if fault == "rows_null":
        x.rows = None
    if fault == "row_of_null":
        x.row_of = None
    if fault == "n_rows":
        x.n_rows = 2**31  # (checked before a row is read)
    if fault == "n_plugins":
        flt.n_plugins = 0
    # (the gate: a registry without out-of-tree plugins unless the call brings one plugin's verdicts)
    snap = snaps[0 if on_est or fault == "n_plugins" else 1]
    h = C.c_void_p()
    if door == "create_estimates":
        rc = eng.L.kp_batch_create_estimates(eng.h, snap.h, ba, None, n, None, C.byref(est), C.byref(h))
    elif door == "create_filters":
        rc = eng.L.kp_batch_create_filters(eng.h, snap.h, ba, None, n, None, None, C.byref(flt), C.byref(h))
    else:
        ans = api.kp_affinity_answers(C.pointer(est) if on_est else None, None if on_est else C.pointer(flt),
                                      None if fault == "term_off_null" else term_off.ctypes.data_as(C.POINTER(C.c_uint64)))
        rc = eng.L.kp_schedule_affinities_ex(eng.h, snap.h, ba, n, C.byref(ans), C.byref(api.kp_affinity_results()))
    assert not h.value
    return rc, eng.L.kp_last_error(eng.h).decode()


def test_pinned_texts(eng):
    u = synth.Universe(6, 9, 64, 0, 400)
    by_terms = {t: [i for i in range(u.n_bindings) if u.bindings[i].n_cluster_affinities == t] for t in (0, 1, 2)}
    ba = TE.binding_array(u, [by_terms[t][k] for k in (0, 1) for t in (0, 1, 2)])
    assert [int(ba[i].n_cluster_affinities) for i in range(6)] == [0, 1, 2, 0, 1, 2]
    snaps = [Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options(out_of_tree_plugins=p))
             for p in (0, 1)]
    assert provoke(eng, snaps, ba, "affinities_flt", None)[0] == 0 and provoke(eng, snaps, ba, "affinities_est", None)[0] == 0
    got = [(door, fault) + provoke(eng, snaps, ba, door, fault) for door, fault, _ in PINNED]
    for s in snaps:
        s.close()
    assert len(PINNED) == 31
    bad = [(g, text) for g, (_, _, text) in zip(got, PINNED) if g[2:] != (E.KP_EINVAL, text)]
    assert not bad, bad
