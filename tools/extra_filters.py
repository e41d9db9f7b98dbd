"""Cost of out-of-tree filter answers on the schedule path (kp_batch_create_filters).

Workload: config 3 at its default size (100k bindings x 5k clusters), one engine, one batch
at a time. The same bindings are packed twice against snapshots of the same clusters:
plainly (no out-of-tree plugin registered), and with --rows rows (64) of density --density
(0.95), every workload binding (spec.Replicas > 0) given row `its index mod rows`, against a
registry holding one out-of-tree plugin. Measured, alternating in this one process
(--rounds):
  serial   mean total_ms of kp_stage_times and wall ms per kp_schedule_batch, both batches;
then, with kp_engine_set_profile, each batch's per-kernel HIP-event times: k_filter_extra's
own time beside k_filter's. The placements differ (the rows reject clusters), so the serial
totals show the cost of the feature together with the smaller feasible sets downstream.
Needs a HIP device. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from karmada_amd import api, synth  # noqa: E402
from karmada_amd.engine import Batch, Engine, EngineError, Snapshot  # noqa: E402


def serial(eng, batch, steps):
    batch.schedule_raw()
    st = []
    t0 = time.perf_counter()
    for _ in range(steps):
        batch.schedule_raw()
        st.append(eng.stage_times())
    wall = 1e3 * (time.perf_counter() - t0) / steps
    return {"total_ms": round(sum(s["total_ms"] for s in st) / steps, 4), "wall_ms": round(wall, 4)}


def profiled(eng, batch):
    eng.set_profile(True)
    try:
        batch.schedule_raw()
        batch.schedule_raw()
        kt = eng.kernel_times()
    finally:
        eng.set_profile(False)
    return {k: {"ms": round(v["ms"], 4), "units": v["units"]} for k, v in kt.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--density", type=float, default=0.95, help="share of the clusters a row passes")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--bindings", type=int, default=None)
    args = ap.parse_args()
    cfg = 3
    C_, B = synth.CONFIGS[cfg]
    C_, B = args.clusters or C_, args.bindings or B
    try:
        eng = Engine(0)
    except EngineError as ex:
        sys.exit(f"extra_filters: no HIP device: {ex}")
    u = synth.Universe(cfg, cfg, C_, 0, B)
    snap0 = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options())
    snap1 = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options(out_of_tree_plugins=1))
    row_of = np.array([i % args.rows if u.bindings[i].replicas > 0 else -1 for i in range(B)], dtype=np.int32)
    ok = np.random.RandomState(1).rand(args.rows, C_) < args.density
    structs = u.binding_slice(0, B)
    t0 = time.perf_counter()
    plain = Batch(snap0, structs=structs)
    t1 = time.perf_counter()
    flt = Batch(snap1, structs=structs, filters=(ok, row_of, 1))
    t2 = time.perf_counter()
    line = {"config": f"config{cfg}: {B} bindings x {C_} clusters", "rows": args.rows, "density": args.density,
            "with_row": int((row_of >= 0).sum()), "steps": args.steps,
            "create_ms": {"plain": round(1e3 * (t1 - t0), 2), "filters": round(1e3 * (t2 - t1), 2)}}
    runs = {"plain": [], "filters": []}
    for _ in range(args.rounds):
        runs["plain"].append(serial(eng, plain, args.steps))
        runs["filters"].append(serial(eng, flt, args.steps))
    line["serial"] = runs
    kp, kf = profiled(eng, plain), profiled(eng, flt)
    if "k_filter_extra" in kp or "k_filter_extra" not in kf:
        sys.exit("extra_filters: k_filter_extra must run for the batch with answers only")
    w = (C_ + 63) // 64
    line["extra_upload_bytes"] = 8 * line["with_row"] + 8 * args.rows * w
    line["k_filter_extra_ms"] = kf["k_filter_extra"]["ms"]
    line["k_filter_ms"] = {"plain": kp["k_filter"]["ms"], "filters": kf["k_filter"]["ms"]}
    line["kernels_ms"] = {name: {"plain": kp.get(name, {}).get("ms"), "filters": kf.get(name, {}).get("ms")}
                          for name in sorted(set(kp) | set(kf))}
    print(json.dumps(line), flush=True)
    for b in (flt, plain):
        b.close()
    snap0.close()
    snap1.close()
    eng.close()


if __name__ == "__main__":
    main()
