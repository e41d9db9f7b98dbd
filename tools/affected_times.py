"""Kernel times of kp_affected_bindings beside k_filter, over config 3 (100k bindings x 5k
clusters by default).

One watch over the universe's bindings; for changed sets of 1, 64 and all clusters one warm
call and then --calls calls under kp_engine_set_profile, each reporting the HIP-event time of
k_affected (k_affected_rows with --rows), of the scan (k_offsets: k_offsets_a + _b) and of
k_affected_write, the list's length, and the call's wall time with profiling off (a host clock
around the call, which ends in the read-back's synchronise). Beside them, in the same run:
k_filter's time over a batch of the same bindings (a profiled kp_schedule_batch), the nearest
existing kernel and an upper bound for the all-clusters case; the host time of
kp_watch_create; and the wall time of enqueueAffectedBindings restated over the oracle's
ClusterMatches (tests/test_affected.py) for one cluster on one thread, a Python loop of one
kpo_cluster_matches call per binding, whose list the engine's must equal. Needs a HIP
device. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from karmada_amd import api, synth  # noqa: E402
from karmada_amd.engine import Batch, Engine, EngineError, Snapshot, Watch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--bindings", type=int, default=None)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rows", action="store_true", help="the per-pair evaluator (KP_PAIR_ROWS=1) instead of the bitset rows")
    args = ap.parse_args()
    cfg = 3
    C_, B = synth.CONFIGS[cfg]
    C_, B = args.clusters or C_, args.bindings or B
    if args.rows:
        os.environ["KP_PAIR_ROWS"] = "1"
    try:
        eng = Engine(0)
    except EngineError as ex:
        sys.exit(f"affected_times: no HIP device: {ex}")
    u = synth.Universe(cfg, cfg, C_, 0, B)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options())
    structs = u.binding_slice(0, B)
    t0 = time.perf_counter()
    watch = Watch(snap, structs=structs)
    create_ms = 1e3 * (time.perf_counter() - t0)
    kern = "k_affected_rows" if args.rows else "k_affected"
    line = {"config": f"config{cfg}: {B} bindings x {C_} clusters", "mode": "rows" if args.rows else "bits",
            "calls": args.calls, "watch_create_ms": round(create_ms, 2), "sets": {}}
    sets = {"1": [C_ // 2], "64": [(i * C_) // 64 for i in range(64)], "all": list(range(C_))}
    for name, lst in sets.items():
        idx = (C.c_uint32 * len(lst))(*lst)
        watch.affected_raw(idx)  # (warm: the kernels' code objects, the page-locked list)
        eng.set_profile(False)
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            watch.affected_raw(idx)
            wall.append(round(1e3 * (time.perf_counter() - t0), 4))
        eng.set_profile(True)
        runs = []
        for _ in range(args.calls):
            n = watch.affected_raw(idx).n
            kt = eng.kernel_times()
            runs.append({k: round(kt[k]["ms"], 4) for k in (kern, "k_offsets", "k_affected_write")})
        eng.set_profile(False)
        line["sets"][name] = {"clusters": len(idx), "listed": int(n), "kernel_ms": runs, "wall_ms": wall}
    # k_filter over a batch of the same bindings, same run
    batch = Batch(snap, structs=structs)
    batch.schedule_raw()
    eng.set_profile(True)
    flt = []
    for _ in range(args.calls):
        batch.schedule_raw()
        kt = eng.kernel_times()  # (no k_filter under --rows: the pair kernel filters there)
        flt.append(round(kt["k_filter"]["ms"], 4) if "k_filter" in kt else None)
    eng.set_profile(False)
    line["k_filter_ms"] = flt
    # the restated reference loop for one cluster, one thread
    import test_affected as TA
    one = sets["1"][0]
    affs = [TA.current_affinity(u.bindings[i]) for i in range(B)]
    t0 = time.perf_counter()
    want = sorted(TA.enqueue_affected(u.clusters[one], affs))
    line["reference_loop_one_cluster_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    got = watch.affected([one])
    line["equal_reference_one_cluster"] = got == want
    print(json.dumps(line), flush=True)
    for x in (batch, watch, snap, eng):
        x.close()
    if got != want:
        sys.exit("affected_times: the engine's list differs from the restated reference")


if __name__ == "__main__":
    main()
