"""The kernels' LDS budgets at the size where a snapshot stops fitting one workgroup.

Every selection kernel carves its working set out of dynamic LDS, 8 B per cluster (10 B
in the region stages), so kp_batch_create refuses a snapshot past about 18.6k clusters
(about 14.3k with spread bindings): batch_lds_check, DESIGN.md §8. The tests here pin
those ceilings, schedule at them with the LDS essentially full, and cross the sizes at
which the launch set changes below them: C = 16 384 / 16 385 (the class orders stop; the
feasible-only k_est_class rows then need the > 64 KB opt-in) and, on the host build, the
sizes at which Cp, W and the bitonic pad P step.

The host build (libkp_cpusim.so) gives each workgroup exactly the bytes its launcher asked
for and a guard band behind them (dev_cpu.cpp grid()), so a carve that outgrows its size
function fails the launch there; test_guard_catches_an_under_asking_launcher shows the
guard firing. The gpu-marked variants run the same functions on libkp.so, where an LDS
overrun raises nothing and shows only as a placement that differs from the oracle's.
"""
import functools
import os

import pytest

from karmada_amd import api, synth
from karmada_amd.engine import KP_EDEVICE, KP_ENOTSUP, Batch, EngineError, PKG, Snapshot
import oracle_lib as O
from test_gpu_parity import compare

N_BINDINGS = 200
SEED = 5
# The ceilings on a device with 163 840 B of LDS per workgroup (gfx950, and what the host
# build reports): k_select_all's 8 B per cluster without spread bindings, k_region_a /
# k_region_b's 10 B per cluster (k_select_cluster: 8 B plus its serial lists) with them.
LDS_GFX950 = 163840
CEILING = {3: 18624, 7: 18624, 10: 18624, 4: 14336, 5: 14336, 6: 14336}
# Bracket of the bisection: the largest size the suite ran before these tests is accepted,
# and 8 B per cluster alone outgrow 163 840 B past 20 480 clusters (20 544: the next Cp).
ACCEPTED, REFUSED = 10000, 20544


@pytest.fixture(scope="module")
def cpusim(cpusim_engine):
    os.environ.setdefault("KP_CPUSIM_THREADS", "8")
    return cpusim_engine


def try_batch(engine, u, n_clusters, n_bindings):
    """None when a batch of the universe's first n_bindings bindings is accepted over its
    first n_clusters clusters, else the refusal's text."""
    snap = Snapshot.from_structs(engine, u.clusters, n_clusters, u.names[:n_clusters], api.options())
    try:
        Batch(snap, structs=u.binding_slice(0, n_bindings)).close()
        return None
    except EngineError as x:
        return str(x)
    finally:
        snap.close()


@functools.lru_cache(maxsize=None)
def _largest_c(engine, config):
    # (cluster i of a synth universe does not depend on how many follow it, so a prefix of
    # the largest universe stands for the smaller ones; the parity and refusal tests below
    # generate theirs at the size itself)
    u = synth.Universe(config, SEED, REFUSED, 0, 32)
    lo, hi = ACCEPTED, REFUSED  # accepted, refused
    assert try_batch(engine, u, lo, 32) is None
    why = try_batch(engine, u, hi, 32)
    assert why is not None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        msg = try_batch(engine, u, mid, 32)
        if msg is None:
            lo = mid
        else:
            hi, why = mid, msg
    # "... (<need> > <the device's bytes per workgroup> bytes)"
    return lo, int(why.rsplit(">", 1)[1].split()[0])


def largest_c(engine, config):
    """The largest cluster count, found by bisection in steps of one, at which Batch
    creation succeeds for the config (32 bindings per probe)."""
    return _largest_c(engine, config)[0]


def device_lds(engine, config):
    """LDS bytes per workgroup of the engine's device, as the refusal above the ceiling states them."""
    return _largest_c(engine, config)[1]


def schedule(engine, u, env=None, profile=False):
    """The universe scheduled by the engine; with profile, also the call's kernel_times()."""
    snap = Snapshot.from_structs(engine, u.clusters, u.n_clusters, u.names, api.options())
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    b = None
    try:
        b = Batch(snap, structs=u.binding_slice(0, u.n_bindings))
        if profile:
            engine.set_profile(True)
        got = b.schedule()
        kt = engine.kernel_times() if profile else None
    finally:
        if profile:
            engine.set_profile(False)
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        if b is not None:
            b.close()
        snap.close()
    return (got, kt) if profile else got


def oracle(u):
    ba, n = u.binding_slice(0, u.n_bindings)
    return O.schedule_c(u.clusters, u.n_clusters, ba, n, api.options(), O.FAST, 8)


def parity(engine, config, n_clusters, env=None, label=""):
    u = synth.Universe(config, SEED, n_clusters, 0, N_BINDINGS)
    compare(schedule(engine, u, env), oracle(u), f"config {config} C={n_clusters} {label}")


# ---- the largest accepted C -------------------------------------------------------------
def check_largest_c(engine, config, pinned):
    c = largest_c(engine, config)
    print(f"config {config}: largest accepted C = {c}")
    if pinned:
        assert c == CEILING[config]


@pytest.mark.parametrize("config", sorted(CEILING))
def test_largest_c_cpusim(cpusim, config):
    check_largest_c(cpusim, config, True)  # (the host build reports gfx950's 163 840 B)


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CEILING))
def test_largest_c_gpu(gpu_engine, config):
    # a device with another LDS size has other ceilings: the tests below run at what the
    # bisection gives there, printed by check_largest_c
    check_largest_c(gpu_engine, config, device_lds(gpu_engine, config) == LDS_GFX950)


# ---- parity at the ceiling --------------------------------------------------------------
AT_CEILING = [
    (3, None), (4, None), (5, None), (6, None), (7, None), (10, None),
    (3, {"KP_PAIR_ROWS": "1"}), (6, {"KP_PAIR_ROWS": "1"}),
    (3, {"KP_ORDER_AMORT": "1000000"}),  # k_select_top's histogram route
]
AT_CEILING_IDS = [f"{c}" + ("-" + "-".join(e).lower() if e else "") for c, e in AT_CEILING]


@pytest.mark.parametrize("config,env", AT_CEILING, ids=AT_CEILING_IDS)
def test_parity_at_ceiling_cpusim(cpusim, config, env):
    parity(cpusim, config, largest_c(cpusim, config), env, "ceiling")


@pytest.mark.gpu
@pytest.mark.parametrize("config,env", AT_CEILING, ids=AT_CEILING_IDS)
def test_parity_at_ceiling_gpu(gpu_engine, config, env):
    parity(gpu_engine, config, largest_c(gpu_engine, config), env, "ceiling")


# ---- refusal just above -----------------------------------------------------------------
def check_refusal(engine, config):
    """One Cp step above the ceiling kp_batch_create refuses: no batch exists, so no
    kp_schedule_batch can start. (Nothing is launched above the ceiling.)"""
    c = largest_c(engine, config) + 1
    u = synth.Universe(config, SEED, c, 0, 32)
    msg = try_batch(engine, u, c, 32)
    assert msg is not None, f"config {config}: a batch over {c} clusters was accepted"
    assert f"rc={KP_ENOTSUP}" in msg and "too large for one workgroup's LDS" in msg, msg
    assert try_batch(engine, u, c - 1, 32) is None  # (and the engine still takes the next batch)


@pytest.mark.parametrize("config", sorted(CEILING))
def test_refusal_above_ceiling_cpusim(cpusim, config):
    check_refusal(cpusim, config)


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CEILING))
def test_refusal_above_ceiling_gpu(gpu_engine, config):
    check_refusal(gpu_engine, config)


# ---- the class-order switch -------------------------------------------------------------
def check_order_switch(engine, config, n_clusters):
    """pack.cpp builds no class orders above C = 16 384 (with_orders): the launch set
    changes between 16 384 and 16 385, the placements do not."""
    u = synth.Universe(config, SEED, n_clusters, 0, N_BINDINGS)
    # (a batch builds class orders when each serves KP_ORDER_AMORT bindings, 4 by default;
    # 200 bindings of configs 3 and 7 fall in more classes than that, so one binding per
    # class is made enough, on both sides of the switch. Config 10 has a class per binding
    # and never builds them.)
    got, kt = schedule(engine, u, {"KP_ORDER_AMORT": "1"} if config in (3, 7) else None, profile=True)
    compare(got, oracle(u), f"config {config} C={n_clusters} order switch")
    ran = {k for k, v in kt.items() if v["launches"] > 0}
    print(f"config {config} C={n_clusters}: kernels {sorted(ran)}")
    if config in (3, 7):
        assert ("k_class_order" in ran) == (n_clusters <= 16384), sorted(ran)
    if config == 10 and n_clusters > 16384:
        # the feasible-only rows: 4 B per cluster of LDS, past 64 KB at this size (the
        # hipFuncSetAttribute opt-in of dev::est_class)
        assert any(k.endswith("(feasible)") for k in ran), sorted(ran)


@pytest.mark.parametrize("n_clusters", [16384, 16385])
@pytest.mark.parametrize("config", [3, 7, 10])
def test_class_order_switch_cpusim(cpusim, config, n_clusters):
    check_order_switch(cpusim, config, n_clusters)


@pytest.mark.gpu
@pytest.mark.parametrize("n_clusters", [16384, 16385])
@pytest.mark.parametrize("config", [3, 7, 10])
def test_class_order_switch_gpu(gpu_engine, config, n_clusters):
    check_order_switch(gpu_engine, config, n_clusters)


# ---- word and power-of-two edges --------------------------------------------------------
@pytest.mark.parametrize("n_clusters", [63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193])
@pytest.mark.parametrize("config", [3, 6, 7])
def test_edges_cpusim(cpusim, config, n_clusters):
    """Cp, W (64 clusters a word) and the bitonic pad P (next power of two) step at these
    sizes: the carves under the guard band on both sides of each step."""
    parity(cpusim, config, n_clusters, None, "edge")


@pytest.mark.gpu
@pytest.mark.parametrize("n_clusters", [4097, 8193])
def test_edges_gpu(gpu_engine, n_clusters):
    parity(gpu_engine, 6, n_clusters, None, "edge")


# ---- the guard itself -------------------------------------------------------------------
def test_guard_catches_an_under_asking_launcher(cpusim):
    """KP_CPUSIM_LDS_SHRINK takes bytes off every launch's LDS request on the host build,
    as a launcher that under-asks would (the host build once corrected such a launcher
    itself and kept 1 KB of slack behind every request): the schedule call then fails
    with KP_EDEVICE and the guard's text, naming the kernel; without the knob the same
    call is exact."""
    u = synth.Universe(3, SEED, 300, 0, N_BINDINGS)
    want = oracle(u)
    compare(schedule(cpusim, u), want, "config 3 C=300")
    with pytest.raises(EngineError) as x:
        schedule(cpusim, u, {"KP_CPUSIM_LDS_SHRINK": "16"})
    msg = str(x.value)
    assert f"rc={KP_EDEVICE}" in msg, msg
    assert "k_" in msg and "wrote past its" in msg and "guard band damaged at offset" in msg, msg
    compare(schedule(cpusim, u), want, "config 3 C=300, after the refused call")


def test_shrink_knob_is_host_only():
    """The hook exists in dev_cpu.cpp alone: no source of libkp.so reads it."""
    src = os.path.join(PKG, "csrc")
    for f in sorted(os.listdir(src)):
        if f.endswith((".cpp", ".hip", ".h")) and f not in ("dev_cpu.cpp", "kp_env.h"):
            with open(os.path.join(src, f)) as fh:
                assert "KP_CPUSIM_LDS_SHRINK" not in fh.read(), f
