"""webster_par (kp_select.h) itself, at every block shape the kernels launch it with,
against the oracle's faithful heap (AllocateWebsterSeats, webstermethod.go:112-161: the
literal heap loop, names in rank order), exit by exit.

libkp_blktest.so's kp_webster_par_selftest runs one block per party list and reports, per
list, which exit produced t* and which tie route webster_tail took (the KP_EXIT marks of
kp_select.h, compiled into the test library only). Every party's seats must equal the
heap's; where the party list was compacted, the seats read by walking w.pl after the return
must equal them too and every seated party must be in the list.

One set of lists (LISTS) serves every combination, so the heap runs once. The combinations:

  block  GpuBlk at 64 / 128 / 256 / 512 / 1024 threads, WaveBlk (one wave, k_select_top's
         waves), and the host block CpuBlk (not a gpu test).
  cap    SelScratch.cap, the u64 entries of sc.buf:
           0     bisection only (no caller carves it; webster_par's documented floor)
           64    sel_all_ecap's floor (k_select_all*, body_sw, k_fused at Cp <= 128) and
                 k_select_top's 64-entry slices: enumeration area, no party list
           128   kOrderEcap: sel_all_fast's scratch in the class-order kernel (kp_kernels.h),
                 and top_ecap of a 128-entry k_select_top slice
           160   KP_TOP_ECAP: k_select_top's slices of 192 entries and more
           256   sel_all_ecap(Cp) = Cp / 2 takes every multiple of 32 between its two ends;
                 256 (Cp = 512) stands for the interior
           1024  KP_ECAP_MAX: carve_sel_scratch at Cp >= 2048
  pre    0: webster_par's own first pass; 1: the caller's (WebPre), as kp_paths.h hands it.

Coverage is asserted, not reported: in every combination each exit that can be reached is
taken by at least MIN_LISTS lists (REACH below says which can, and why the others cannot).

Two things the list families cannot contain, by webster_par's own arithmetic:
  * a quota adjustment of more than kAdjMax = 64 steps. The list holds np <= 64 parties.
    With Lb = 1 it holds every party, sum(N v / V) = N and each count is that quotient
    rounded, so |C - N| <= np / 2 <= 32. With Lb > 1 (P > N) the N-th largest vote is in
    the list, so N <= np <= 64, counts can only miss (C <= N + 32) and C >= 0 gives at most
    N <= 64 additions. Steps 0, 1 and 64 are built below (quota_steps64); 65 cannot be.
  * hence the first-seat case and the bracket with a compacted list of np <= 64 parties:
    such lists always leave through the hand-off or the quota adjustment.
"""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "karmada_amd", "libkp_blktest.so")

# WebExit (kp_select.h)
WX = {"reg": 1 << 0, "drop": 1 << 1, "add": 1 << 2, "first": 1 << 3, "bracket": 1 << 4, "enum": 1 << 5,
      "tie_all": 1 << 8, "tie_rank": 1 << 9, "tie_bisect": 1 << 10, "compact_first": 1 << 12,
      "compact_retry": 1 << 13, "retry_full": 1 << 14}
T_MASK, TIE_MASK, COMPACT_MASK = 0x3F, 0x700, 0x3000
MIN_LISTS = 10
RANK_MAX = (1 << 22) - 1  # kRankMask

CAPS = [0, 64, 128, 160, 256, 1024]
HOST = ("host", 0, 1)
DEVICE_BLOCKS = [("gpu64", 1, 64), ("gpu128", 1, 128), ("gpu256", 1, 256), ("gpu512", 1, 512),
                 ("gpu1024", 1, 1024), ("wave64", 2, 64)]


def reach(block, cap):
    """The exits a (block, cap) combination can reach (pre does not enter any decision)."""
    name, _, nth = block
    r = {"bracket", "tie_all", "tie_bisect", "no_compact"}  # every cap: bisection to one ulp, M >= T, T > ecap
    if cap >= 64:  # an enumeration area: at most 64 priorities left, at most 64 tied parties
        r |= {"enum", "tie_rank"}
    if cap > 64:  # a party list (pcap = cap - 64)
        r |= {"compact_first", "compact_retry", "retry_full"}
        # a compacted list of at most 64 parties: webster_reg on a one-wave block when it has
        # a lane per party (the host block has one lane: single-party lists only), the quota
        # adjustment otherwise
        if name in ("gpu64", "wave64"):
            r |= {"reg"}
        elif name == "host":
            r |= {"reg", "drop", "add"}
        else:
            r |= {"drop", "add"}
    if cap - 64 > 64:  # first seats: a compacted list of 65 .. min(128, pcap) parties
        r |= {"first"}
    return r


# ---------------------------------------------------------------------------------------
# The lists: (family, votes, N, desc, ranks). Seeded; built once.
# ---------------------------------------------------------------------------------------
def _ranks(rng, n, style):
    if style == 0:
        return list(range(n))
    if style == 1:  # permuted
        r = list(range(n))
        rng.shuffle(r)
        return r
    r = rng.sample(range(RANK_MAX), n)  # sparse, with the largest rank there is
    r[rng.randrange(n)] = RANK_MAX
    return r


def _contraction_pairs(rng):
    """Two parties with votes near 2^31 whose priorities v_i / (2 k_i + 1) and v_j / (2 k_j + 1)
    differ by one part in v_i v_j: v_i a - b v_j = +-1 with a = 2 k_j + 1, b = 2 k_i + 1 past
    2^12, so v_i * fl(1 / t) lies within a few ulps of the odd integer b at t = v_j / a (the
    band in which w_count_r defers to w_count, and where a contracted v * rt - 1.0 would move
    a count if it moved any). N sweeps the seats around that priority."""
    out = []
    while len(out) < 12:
        vj = rng.randrange(2**30, 2**31 - 1) | 1
        a = 2 * rng.randrange(2100, 9000) + 1
        try:
            inv = pow(a, -1, vj)
        except ValueError:
            continue
        for sign in (1, -1):
            vi = inv if sign == 1 else vj - inv
            b, rem = divmod(vi * a - sign, vj)
            if rem or b % 2 == 0 or b < 4097 or vi >= 2**31:
                continue
            n0 = (a + 1) // 2 + (b + 1) // 2
            if n0 + 2 > 65536:
                continue
            out.append((vi, vj, n0))
            break
    return out


@functools.lru_cache(maxsize=None)
def lists():
    rng = random.Random(20240607)
    out = []

    def add(fam, votes, N, desc=None, style=None):
        i = len(out)
        out.append((fam, list(votes), N, (i & 1) if desc is None else desc,
                    _ranks(rng, len(votes), i % 3 if style is None else style)))

    # quota adjustment, both directions: few parties, N far above and below their number,
    # ties across parties at t*, one dominant party, zero votes mixed in
    for n in (1, 2, 3, 5, 8, 13, 31, 32, 33, 50, 63, 64):
        for kind in range(6):
            for N in rng.sample([1, 2, n // 2 + 1, n, n + 1, 3 * n, 97, 1000, 20000], 3):
                if kind == 0:
                    v = [rng.randint(1, 5000) for _ in range(n)]
                elif kind == 1:
                    v = [rng.choice([6, 10, 30, 42]) for _ in range(n)]
                elif kind == 2:
                    v = [rng.choice([7, 21, 35]) for _ in range(n)]
                elif kind == 3:
                    lo = rng.randint(1, 300)
                    v = [rng.randint(lo, lo + 3) for _ in range(n)]
                elif kind == 4:
                    v = [rng.randint(1, 3) for _ in range(n)]
                    v[rng.randrange(n)] = rng.randint(1000, 100000)
                else:
                    v = [rng.randint(0, 2) for _ in range(n)]
                    v[rng.randrange(n)] = 1
                add("quota", v, N)
    # a single party (the host block's hand-off): N = 1 and large
    for i in range(12):
        add("one_party", [rng.choice([1, 7, 2**31 - 1, rng.randint(1, 10**6)])], rng.choice([1, 2, 100, 65536]))
    # quota steps 0 and 1: equal votes with N a multiple of the party count, and one more / less
    for n in (2, 7, 40, 64):
        for d in (-1, 0, 1):
            add("quota_steps01", [30] * n, 3 * n + d)
    # quota steps 64 (kAdjMax): 64 large parties in one octave bin hold no priority at
    # V / 2N because 1500 one-vote parties below Lb carry most of V; N = 64 are all added
    for i in range(12):
        v = [rng.randint(16, 19) for _ in range(64)] + [1] * 1500
        rng.shuffle(v)
        add("quota_steps64", v, 64)
    # first seats: votes in [lo, 3 lo), a tie group straddling the N-th place, N near the
    # party count so that the whole list is compacted; np = 128 and 129; vmax == 3 v_N
    for n in (65, 80, 96, 97, 110, 127, 128, 129):
        for _ in range(8):
            lo = rng.randint(1, 5000)
            v = [rng.randint(lo, 3 * lo - 1) for _ in range(n)]
            N = rng.randint(max(1, n - 12), n)
            if rng.random() < 0.6:
                tie = sorted(v, reverse=True)[N - 1]
                for _ in range(rng.randint(1, 5)):
                    v[rng.randrange(n)] = tie
            add("first_seat", v, N)
    for n in (65, 96, 128, 129):
        add("first_seat_all", [rng.randint(100, 299) for _ in range(n)], n)  # P == N: Lb = 1
        v = [100] * (n - 10) + [rng.randint(101, 299) for _ in range(9)] + [300]  # vmax == 3 v_N
        add("first_seat_3vN", v, n - 3)
        v = [100] * (n - 10) + [rng.randint(101, 299) for _ in range(9)] + [299]
        add("first_seat_3vN", v, n - 3)
    # a crowded octave bin: the first compaction overflows pcap, kth_largest_vote runs and the
    # retry fits (N small) or does not (N large, or the votes all equal)
    for n in (200, 700, 1100, 3000):
        for N in (5, 40, 80, 150, 600, 900, 2000):
            if N >= n:
                continue
            add("crowded_wide", [rng.randrange(2**20, 2**20 + 2**17) for _ in range(n)], N)
            add("crowded_narrow", [rng.randint(1024, 1087) for _ in range(n)], N)
    for n in (1100, 3000):  # (past KP_ECAP_MAX's 960-entry list on the retry too)
        for N in (970, 1000, 1050):
            add("crowded_full", [rng.randint(1024, 1087) for _ in range(n)], N)
            add("crowded_full", [rng.randrange(2**20, 2**20 + 2**17) for _ in range(n)], N)
    for n in (100, 161, 200, 1100):
        for N in (3, 30, 90):
            add("crowded_small", [rng.randrange(2**20, 2**20 + 2**17) for _ in range(n)] + [5] * 20, N)
    # more than ecap parties tied at t* with N inside the tie group: webster_tail's bisection
    # over tie_key, both name orders, sparse and permuted ranks; N past the party count ties
    # every party's second priority
    for n in (65, 97, 129, 200, 700):
        for v0 in (7, 21, 1, 2**31 - 1):
            for N in (1, n // 2, n - 1, n + n // 2):
                for desc in (0, 1):
                    add("tie_bisect", [v0] * n, N, desc, 1 + (len(out) & 1))
    for n in (100, 200):
        for N in (60, 150):
            for desc in (0, 1):
                v = [7] * n + [rng.choice([21, 35, 49]) for _ in range(10)]
                rng.shuffle(v)
                add("tie_bisect_mixed", v, N, desc, 2)
    # bracket, bisection, enumeration: huge votes, powers of 3, votes t (2k + 1) so that many
    # priorities are equal doubles; zero votes mixed in; party counts around every threshold
    sizes = [1, 2, 63, 64, 65, 96, 97, 127, 128, 129, 192, 193, 200, 700, 960, 961, 1100, 3000]
    for n in sizes:
        for kind in range(5):
            for N in rng.sample([1, 2, 5, 17, 100, 999, 4000], 2):
                if kind == 0:
                    v = [rng.randint(0, 2**31 - 1) for _ in range(n)]
                elif kind == 1:
                    v = [3 ** rng.randint(0, 19) for _ in range(n)]
                elif kind == 2:
                    t = rng.choice([1, 2, 5, 1000, 99991])
                    v = [t * (2 * rng.randint(0, 20) + 1) for _ in range(n)]
                elif kind == 3:
                    v = [rng.choice([0, 0, 0, 1, 2]) for _ in range(n)]
                    v[rng.randrange(n)] = 2
                else:
                    v = [rng.randint(0, 1000) for _ in range(n)]
                    v[rng.randrange(n)] = 1000
                add("general", v, N)
    for n in (2, 3, 64, 65):
        add("general_bigN", [rng.randint(1, 2**31 - 1) for _ in range(n)], 65536)
        add("general_bigN", [3 ** rng.randint(0, 19) for _ in range(n)], 65536)
    # more than 64 equal priorities at t* among many parties: the bracket meets at one ulp
    for n in (200, 700):
        for t in (1, 3, 1000):
            for N in (n // 2, n, 2 * n):
                add("bracket_equal", [t * (2 * rng.randint(0, 3) + 1) for _ in range(n)], N)
    # contraction band
    for vi, vj, n0 in _contraction_pairs(rng):
        for d in (-2, -1, 0, 1, 2):
            add("contraction", [vi, vj], n0 + d)
    # degenerate: mode 0 (all votes zero), mode 1 (N <= 0), N = 1
    for n in (1, 2, 64, 65, 200, 1100):
        add("all_zero", [0] * n, rng.choice([1, 5, 1000]))
        add("all_zero", [0] * n, 0)
        add("no_seats", [rng.randint(0, 50) for _ in range(n - 1)] + [3], 0)
        add("no_seats", [rng.randint(0, 50) for _ in range(n - 1)] + [3], -5)
        add("one_seat", [rng.randint(0, 50) for _ in range(n - 1)] + [3], 1)
    return out


class Flat:
    """The lists concatenated for the self-test."""

    def __init__(self):
        ls = lists()
        self.nl = len(ls)
        self.offs = np.zeros(self.nl + 1, np.int32)
        self.offs[1:] = np.cumsum([len(l[1]) for l in ls])
        self.votes = np.array([v for l in ls for v in l[1]], np.int32)
        self.ranks = np.array([r for l in ls for r in l[4]], np.uint32)
        self.N = np.array([l[2] for l in ls], np.int32)
        self.desc = np.array([l[3] for l in ls], np.int32)
        self.total = int(self.offs[-1])


@functools.lru_cache(maxsize=None)
def flat():
    return Flat()


@functools.lru_cache(maxsize=None)
def reference():
    """The heap's seats per party, flat; zero for the lists the Dispenser never hands to
    Webster (no votes, binding.go:98-101) or that ask for no seat."""
    import oracle_lib as O
    from karmada_amd import api
    L = O.lib()
    L.kpo_set_webster_fast(0)  # the literal heap loop
    w = api.World()
    nmax = max(len(l[1]) for l in lists())
    names, _ = w.arr(api.kp_str, [w.s(f"c{i:06d}") for i in range(nmax)])
    f = flat()
    want = np.zeros(f.total, np.int32)
    for j, (_, votes, N, desc, ranks) in enumerate(lists()):
        n = len(votes)
        if sum(votes) == 0 or N <= 0:
            continue
        order = sorted(range(n), key=lambda i: ranks[i])  # party order[k] gets the k-th name
        vv = (C.c_int64 * n)(*[votes[i] for i in order])
        out = (C.c_int32 * n)()
        k = L.kpo_allocate_webster(N, names, vv, n, None, None, 0, 2 if desc else 1, api.kp_str(None, 0), out, n)
        assert k == n
        a = int(f.offs[j])
        for pos, i in enumerate(order):
            want[a + i] = out[pos]
    return want


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run_selftest(block, cap, pre):
    lib = C.CDLL(LIB)
    fn = lib.kp_webster_par_selftest
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32),
                   C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    f = flat()
    seats = np.full(f.total, -1, np.int32)
    pl_rank = np.zeros(f.total, np.uint32)
    pl_seats = np.zeros(f.total, np.int32)
    info = np.zeros((f.nl, 5), np.int64)
    msg = C.create_string_buffer(256)
    rc = fn(block[1], block[2], cap, pre, _ptr(f.votes, C.c_int32), _ptr(f.ranks, C.c_uint32),
            _ptr(f.offs, C.c_int32), _ptr(f.N, C.c_int32), _ptr(f.desc, C.c_int32), f.nl, _ptr(seats, C.c_int32),
            _ptr(pl_rank, C.c_uint32), _ptr(pl_seats, C.c_int32), _ptr(info, C.c_int64), msg, 256)
    assert rc == 0, msg.value.decode()
    return seats, pl_rank, pl_seats, info


@functools.lru_cache(maxsize=None)
def host_run(cap, pre):
    return run_selftest(HOST, cap, pre)


def exits_of(info_row):
    """The exit names of one list's marks (+ 'no_compact' for a mode-2 list without a party list)."""
    mode, _, _, _, ex = (int(x) for x in info_row)
    names = {k for k, b in WX.items() if ex & b}
    if mode == 2 and not ex & COMPACT_MASK:
        names.add("no_compact")
    return names


def coverage(info):
    cnt = {}
    for row in info:
        for k in exits_of(row):
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


def check(block, cap, pre):
    ls, f, want = lists(), flat(), reference()
    seats, pl_rank, pl_seats, info = run_selftest(block, cap, pre) if block is not HOST else host_run(cap, pre)
    label = f"{block[0]} cap={cap} pre={pre}"
    # 1. every party's seats are the heap's; modes 0 and 1 where no seat is due
    bad = np.nonzero(seats != want)[0]
    if len(bad):
        j = int(np.searchsorted(f.offs, bad[0], side="right")) - 1
        a, b = int(f.offs[j]), int(f.offs[j + 1])
        pytest.fail(f"{label}: {len(bad)} parties differ from the heap; first list {j} ({ls[j][0]}, n={b - a}, "
                    f"N={ls[j][2]}, desc={ls[j][3]}, exit={int(info[j][4]):#x}): votes={ls[j][1][:12]} "
                    f"got={seats[a:b][:12].tolist()} want={want[a:b][:12].tolist()}")
    for j, (fam, votes, N, _, ranks) in enumerate(ls):
        mode, compact, npar, Lb, ex = (int(x) for x in info[j])
        want_mode = 0 if sum(votes) == 0 else 1 if N <= 0 else 2
        assert mode == want_mode, (label, j, fam, mode)
        if mode != 2:
            assert ex == 0 and not compact, (label, j, fam)
            continue
        # 2. exactly one t* exit; one tie route unless the hand-off decided (webster_reg has its own)
        t, tie, cm = ex & T_MASK, ex & TIE_MASK, ex & COMPACT_MASK
        assert t and t & (t - 1) == 0, (label, j, fam, hex(ex))
        assert (tie == 0) if t == WX["reg"] else (tie and tie & (tie - 1) == 0), (label, j, fam, hex(ex))
        assert bool(cm) == bool(compact) and cm != COMPACT_MASK, (label, j, fam, hex(ex))
        assert not (cm and ex & WX["retry_full"]), (label, j, fam, hex(ex))
        # 3. the party list after the return: the parties with votes >= Lb, each once, with
        # web_seats' answer; every seated party is among them
        a, b = int(f.offs[j]), int(f.offs[j + 1])
        if compact:
            assert 0 <= npar <= max(0, cap - 64) and npar <= b - a, (label, j, fam, npar)
            by_rank = {ranks[i]: i for i in range(b - a)}
            got = {}
            for q in range(npar):
                got[int(pl_rank[a + q])] = int(pl_seats[a + q])
            assert len(got) == npar, (label, j, fam, "a party twice in pl")
            assert set(got) == {ranks[i] for i in range(b - a) if votes[i] >= Lb}, (label, j, fam, Lb)
            for r, s in got.items():
                assert s == int(want[a + by_rank[r]]), (label, j, fam, r, s)
            assert all(ranks[i] in got for i in range(b - a) if want[a + i] > 0), (label, j, fam)
        else:
            assert (pl_rank[a:b] == 0xFFFFFFFF).all(), (label, j, fam)
    # 4. coverage: every reachable exit by MIN_LISTS lists, no unreachable one at all
    cnt, r = coverage(info), reach(block, cap)
    short = {k: cnt.get(k, 0) for k in sorted(r) if cnt.get(k, 0) < MIN_LISTS}
    assert not short, f"{label}: exits taken by fewer than {MIN_LISTS} lists: {short} (all: {cnt})"
    stray = {k: v for k, v in cnt.items() if k not in r}
    assert not stray, f"{label}: exits REACH rules out were taken: {stray}"
    return info


def check_against_host(block, cap, pre, info):
    """The device's exits equal the host block's wherever nth is not part of the decision:
    everything but which of the hand-off and the quota adjustment takes a compacted list of
    at most min(64, cap) parties (the only test on nwaves() / nth())."""
    h = host_run(cap, pre)[3]
    assert (info[:, :4] == h[:, :4]).all(), f"{block[0]} cap={cap} pre={pre}: mode / compact / np / Lb differ"
    one_wave = block[0] in ("gpu64", "wave64")
    quota = WX["reg"] | WX["drop"] | WX["add"]
    for j in range(len(h)):
        he, de = int(h[j][4]), int(info[j][4])
        if he & quota:
            assert h[j][1] and 0 < h[j][2] <= min(64, cap)
            assert de & COMPACT_MASK == he & COMPACT_MASK, (j, hex(he), hex(de))
            if one_wave:
                assert de & ~COMPACT_MASK == WX["reg"], (j, hex(he), hex(de))
            elif he & WX["reg"]:  # one party: the host block's only hand-off
                assert de & T_MASK in (WX["drop"], WX["add"]), (j, hex(he), hex(de))
            else:
                assert de == he, (j, hex(he), hex(de))
        else:
            assert de == he, (j, lists()[j][0], hex(he), hex(de))


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("cap", CAPS)
def test_webster_par_host_block(cap, pre):
    """The host block (CpuBlk): the lists and the expected exits, checked without a GPU."""
    check(HOST, cap, pre)


def test_webster_par_lists_are_fixed():
    """Both pre settings take the same exits on the host block (pre enters no decision), and
    the named regression lists stay where the families put them."""
    for cap in CAPS:
        assert (host_run(cap, 0)[3] == host_run(cap, 1)[3]).all(), cap
    fams = {l[0] for l in lists()}
    assert {"quota_steps64", "quota_steps01", "contraction", "tie_bisect", "crowded_wide", "crowded_full",
            "first_seat_3vN"} <= fams
    # quota_steps64 is what it says: all 64 seats are additions from C = 0 (t* = the smallest
    # large vote, every large party one seat)
    f, want = flat(), reference()
    for j, l in enumerate(lists()):
        if l[0] == "quota_steps64":
            a, b = int(f.offs[j]), int(f.offs[j + 1])
            assert [int(s) for s in want[a:b]] == [1 if v > 1 else 0 for v in l[1]]
            assert int(host_run(128, 0)[3][j][4]) & T_MASK == WX["add"]


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("block", DEVICE_BLOCKS, ids=[b[0] for b in DEVICE_BLOCKS])
def test_webster_par_on_device(block, cap, pre):
    """Exact seats, the pl walk, exit coverage, and the host block's exits on the device."""
    info = check(block, cap, pre)
    check_against_host(block, cap, pre, info)
