"""Kernel helpers of kp_select.h, run on the host through libkp_cpusim.so
(test-only), against the oracle's restatement of the reference:

  webster_par  vs AllocateWebsterSeats (pkg/util/helper/webstermethod.go:112-161)
  wsel_max     vs the Aggregated prefix cut's value threshold
               (pkg/scheduler/core/division_algorithm.go:81-89), brute force.
"""
import ctypes as C
import os
import random

import pytest

from karmada_amd import api
from karmada_amd.engine import PKG
import oracle_lib as O

SIM = C.CDLL(os.path.join(PKG, "libkp_cpusim.so"))
SIM.kpsim_webster.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int, C.c_int32, C.c_int, C.c_int,
                              C.POINTER(C.c_int32)]
SIM.kpsim_wsel_max.restype = C.c_int64
SIM.kpsim_wsel_max.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_int64]


def oracle_webster(votes, N, desc):
    L = O.lib()
    w = api.World()
    n = len(votes)
    names, _ = w.arr(api.kp_str, [w.s(f"c{i:06d}") for i in range(n)])
    vv = (C.c_int64 * max(1, n))(*votes)
    out = (C.c_int32 * max(1, n))()
    k = L.kpo_allocate_webster(N, names, vv, n, None, None, 0, 2 if desc else 1, api.kp_str(None, 0), out, n)
    assert k == n
    return [out[i] for i in range(n)]


def sim_webster(votes, N, desc, ecap):
    n = len(votes)
    vv = (C.c_int32 * max(1, n))(*votes)
    rr = (C.c_uint32 * max(1, n))(*range(n))
    out = (C.c_int32 * max(1, n))()
    SIM.kpsim_webster(vv, rr, n, N, 1 if desc else 0, ecap, out)
    return [out[i] for i in range(n)]


def vote_sets(rng):
    for _ in range(60):
        n = rng.choice([1, 2, 3, 7, 12, 13, 50, 200, 700, 3000])
        kind = rng.choice(["uniform", "ties", "zeros", "huge", "powers", "one-big"])
        if kind == "uniform":
            v = [rng.randint(0, 1000) for _ in range(n)]
        elif kind == "ties":
            v = [rng.choice([3, 5, 15, 45]) for _ in range(n)]
        elif kind == "zeros":
            v = [rng.choice([0, 0, 0, 1, 2]) for _ in range(n)]
        elif kind == "huge":
            v = [rng.randint(0, 2**31 - 1) for _ in range(n)]
        elif kind == "powers":
            v = [3 ** rng.randint(0, 12) for _ in range(n)]
        else:
            v = [1] * n
            v[rng.randrange(n)] = 100000
        yield v


@pytest.mark.parametrize("seed", range(6))
def test_webster_par_matches_reference_heap(seed):
    rng = random.Random(seed)
    for votes in vote_sets(rng):
        if sum(votes) == 0:
            continue
        N = rng.choice([1, 2, 5, 17, 100, 999, 4000, 65536])
        desc = rng.random() < 0.5
        want = oracle_webster(votes, N, desc)
        # 0: bisection only; 4: no party compaction; 128 / 160: the capacities the kernels
        # carve (kOrderEcap, KP_TOP_ECAP); 256: compaction that overflows on crowded votes
        # (exact N-th largest, retry); 4096: compaction
        for ecap in (0, 4, 64, 128, 160, 256, 4096):
            got = sim_webster(votes, N, desc, ecap)
            assert got == want, (votes[:20], N, desc, ecap)


@pytest.mark.parametrize("seed", range(4))
def test_webster_quota_adjust(seed):
    """webster_par's few-party search (compacted list within the enumeration area): t*
    from the quota counts at V/2N, adjusted by dropping or adding single priorities; ties
    across parties at t*, N far above and below the party count, one dominant party."""
    rng = random.Random(500 + seed)
    for _ in range(150):
        n = rng.randint(1, 64)
        kind = rng.choice(["uniform", "ties", "narrow", "one-big", "tiny"])
        if kind == "uniform":
            v = [rng.randint(1, 5000) for _ in range(n)]
        elif kind == "ties":
            v = [rng.choice([6, 10, 30, 42]) for _ in range(n)]
        elif kind == "narrow":
            lo = rng.randint(1, 300)
            v = [rng.randint(lo, lo + 3) for _ in range(n)]
        elif kind == "one-big":
            v = [rng.randint(1, 3) for _ in range(n)]
            v[rng.randrange(n)] = rng.randint(1000, 100000)
        else:
            v = [rng.randint(0, 2) for _ in range(n)]
        if sum(v) == 0:
            continue
        N = rng.choice([1, 2, n // 2 + 1, n, n + 1, 3 * n, 97, 1000, 20000])
        desc = rng.random() < 0.5
        want = oracle_webster(v, N, desc)
        for ecap in (64, 256):
            assert sim_webster(v, N, desc, ecap) == want, (v, N, desc, ecap)


@pytest.mark.parametrize("seed", range(4))
def test_webster_first_seat_case(seed):
    """webster_par's first-seat case (P >= N and vmax < 3 v_N: t* = v_N from a rank select
    of the compacted list): votes in a narrow band, ties at v_N, and the boundary vmax =
    3 v_N where a second seat ties with v_N (the general path)."""
    rng = random.Random(100 + seed)
    cases = [([300, 100, 100], 2), ([299, 100, 100], 2), ([300, 100, 100, 100], 3), ([7, 7, 7, 7], 2)]
    for _ in range(40):
        n = rng.choice([2, 5, 13, 40, 100, 127])
        lo = rng.randint(1, 5000)
        v = [rng.randint(lo, 3 * lo - 1) for _ in range(n)]
        if rng.random() < 0.5:  # a tie group straddling the N-th place
            v += [sorted(v)[n // 2]] * rng.randint(1, 5)
        cases.append((v, rng.randint(1, len(v))))
    for votes, N in cases:
        for desc in (False, True):
            want = oracle_webster(votes, N, desc)
            for ecap in (64, 256, 4096):
                assert sim_webster(votes, N, desc, ecap) == want, (votes[:20], N, desc, ecap)


def test_wsel_max_brute_force():
    rng = random.Random(7)
    for _ in range(300):
        n = rng.randint(1, 60)
        vals = [rng.choice([0, 1, 2, 5, 255, 256, 257, 65535, 65536, rng.randint(0, 2**31 - 1)]) for _ in range(n)]
        tot = sum(vals)
        if tot == 0:
            continue
        target = rng.randint(1, tot)
        want = max(v for v in set(vals) if v > 0 and sum(x for x in vals if x >= v) >= target)
        arr = (C.c_int32 * n)(*vals)
        assert SIM.kpsim_wsel_max(arr, n, target) == want, (vals, target)


SIM.kpsim_sort_tcl.restype = C.c_int
SIM.kpsim_sort_tcl.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_int, C.c_int]


def _sort(reps, mode):
    n = len(reps)
    names = (C.c_uint32 * max(1, n))(*range(n))
    rr = (C.c_int32 * max(1, n))(*reps)
    ok = SIM.kpsim_sort_tcl(names, rr, n, mode)
    return ok, [names[i] for i in range(n)], [rr[i] for i in range(n)]


@pytest.mark.parametrize("seed", range(3))
def test_sort_tcl_wave_form_matches_serial_and_oracle(seed):
    """sort.Sort(TargetClustersList) (division_algorithm.go:31-36): the wave
    emulation (kp_pdq.h, one lane here) and the serial emulation (kp_algo.h)
    give the oracle's permutation (unstable: equal replicas keep Go's order)."""
    import pdq_cases
    L = O.lib()
    L.kpo_sort_target_clusters.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32]
    for n, kind, reps in pdq_cases.cases(seed):
        ids = (C.c_uint32 * max(1, n))(*range(n))
        rr = (C.c_int32 * max(1, n))(*reps)
        L.kpo_sort_target_clusters(rr, ids, n)
        want = [ids[i] for i in range(n)]
        _, serial, _ = _sort(reps, 0)
        ok, wave, wrep = _sort(reps, 1)
        assert serial == want, (n, kind)
        assert ok == 1, (n, kind)
        assert wave == want, (n, kind)
        assert wrep == [reps[i] for i in want]


SIM.kpsim_select_groups.restype = C.c_int
SIM.kpsim_select_groups.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int, C.c_int64, C.c_int64,
                                    C.c_int64, C.POINTER(C.c_int32)]


@pytest.mark.parametrize("seed", range(4))
def test_select_groups_device_form_matches_oracle(seed):
    """selectGroups (select_groups.go:102-224): the device form (one thread,
    two passes, no path list) picks the oracle's DFS + prioritizePaths answer,
    including the subpath walk, the no-backtracking case (#groups == min) and
    the reference's errors."""
    L = O.lib()
    rng = random.Random(100 + seed)
    w = api.World()
    for _ in range(400):
        R = rng.choice([1, 2, 3, 4, 6, 8, 12, 16])
        vals = [rng.choice([0, 1, 1, 2, 3, 5, 8]) for _ in range(R)]
        wts = [rng.choice([0, 1000, 2000, 2500, rng.randint(0, 10**6), 10**9]) for _ in range(R)]
        present = [r for r in range(R) if vals[r] > 0]
        min_c = rng.choice([0, 1, 2, 3, len(present)])
        max_c = rng.choice([min_c, min_c + 1, 3, 5, 16])
        target = rng.choice([0, 1, 2, 4, 7, 12, 30])
        out = (C.c_int32 * max(1, R))()
        got = SIM.kpsim_select_groups((C.c_int32 * R)(*vals), (C.c_int64 * R)(*wts), R, min_c, max_c, target, out)
        # oracle: regions with clusters only (host step, select_clusters_by_region.go:25-40)
        n = len(present)
        if n < min_c:
            want = -2
        else:
            names, _ = w.arr(api.kp_str, [w.s(f"r{r:03d}") for r in present])
            o = (C.c_uint32 * max(1, n))()
            k = L.kpo_select_groups(names, (C.c_int64 * max(1, n))(*[vals[r] for r in present]),
                                    (C.c_int64 * max(1, n))(*[wts[r] for r in present]), n, min_c, max_c, target, o)
            want = [present[o[i]] for i in range(k)] if k > 0 else -3
        if isinstance(want, list):
            assert got == len(want), (vals, wts, min_c, max_c, target, got, want)
            assert [out[i] for i in range(got)] == want, (vals, wts, min_c, max_c, target)
        else:
            assert got == want, (vals, wts, min_c, max_c, target, got)


# ---- k_select_top's DynamicWeight stop rule (kp_top.h), pinned against the reference heap ----
def oracle_webster_named(votes, names, N, desc):
    """AllocateWebsterSeats over parties named c<index> (the tie order), the faithful heap."""
    L = O.lib()
    w = api.World()
    n = len(votes)
    arr, _ = w.arr(api.kp_str, [w.s(f"c{i:06d}") for i in names])
    vv = (C.c_int64 * max(1, n))(*votes)
    out = (C.c_int32 * max(1, n))()
    assert L.kpo_allocate_webster(N, arr, vv, n, None, None, 0, 2 if desc else 1, api.kp_str(None, 0), out, n) == n
    return dict(zip(names, (out[i] for i in range(n))))


def seats_above(v, vmin):
    """#{k >= 0 : v / (2k+1) > vmin} for integers v, vmin > 0 (exact; for v < 2^31 the
    float64 priority compares the same way, its distance to vmin being > 2^-31 relative)."""
    return ((v - 1) // vmin + 1) // 2 if v > vmin else 0


def top_stop_subset(votes, N, chunk=64):
    """The walk of k_select_top for a DynamicWeight binding with no scheduled clusters:
    parties in (votes desc, name asc) order, 64 per step; it stops once the walked votes
    cover N and the walked parties hold >= N seat priorities strictly above the
    smallest walked vote vmin (then t* > vmin >= every unwalked priority)."""
    order = sorted(range(len(votes)), key=lambda i: (-votes[i], i))
    for end in range(chunk, len(order) + chunk, chunk):
        sub = order[:end]
        vmin = votes[sub[-1]]
        if vmin > 0 and sum(votes[i] for i in sub) >= N and sum(seats_above(votes[i], vmin) for i in sub) >= N:
            return sub
    return order


@pytest.mark.parametrize("seed", range(8))
def test_top_dynamic_stop_rule_vs_heap(seed):
    """Adversarial vote sets: votes at odd multiples of vmin (+-1), ties at vmin spanning
    the chunk and the stop, a few huge votes over many small ones, N at the count
    boundary. Webster over the stopped subset gives every party of the full set its
    seats, and every party left out gets none."""
    rng = random.Random(500 + seed)
    for _ in range(40):
        kind = rng.choice(["odd_multiples", "ties", "heavy_head", "uniform", "boundary"])
        n = rng.choice([65, 130, 300, 700, 2000])
        if kind == "odd_multiples":
            base = rng.randint(1, 50)
            votes = [(2 * rng.randint(0, 20) + 1) * base + rng.choice([-1, 0, 1]) for _ in range(n)]
        elif kind == "ties":
            votes = [rng.choice([7, 21, 35, 63]) for _ in range(n)]
        elif kind == "heavy_head":
            votes = [rng.randint(10**6, 10**7) for _ in range(5)] + [rng.randint(1, 30) for _ in range(n - 5)]
        elif kind == "uniform":
            votes = [rng.randint(0, 1000) for _ in range(n)]
        else:
            base = rng.randint(2, 9)
            votes = [base * rng.choice([1, 3, 5, 9]) for _ in range(n)]
        votes = [max(0, v) for v in votes]
        tot = sum(votes)
        if tot == 0:
            continue
        N = min(rng.choice([1, 5, 64, 200, 1000, 5000, tot]), tot, 20000)
        desc = rng.random() < 0.5
        full = oracle_webster_named(votes, list(range(n)), N, desc)
        sub = top_stop_subset(votes, N)
        sub = sorted(sub)  # (the parties in name order, as oracle_webster passes them)
        part = oracle_webster_named([votes[i] for i in sub], sub, N, desc)
        assert all(full[i] == part[i] for i in sub), (kind, n, N)
        left = set(range(n)) - set(sub)
        assert all(full[i] == 0 for i in left), (kind, n, N)
