"""Cost of the scheduler's assumed workloads on the schedule path (kp_batch_create_assumed).

Workload: config 3 at its default size (100k bindings x 5k clusters), one engine, one batch
at a time. --share percent of the clusters (1 and 25 are the recorded points) carry
--workloads (100) assumed workloads each: a one-component workload of 1..3 replicas of
cpu 250m..1 / memory 256Mi..1Gi. The same bindings are packed twice against one snapshot:
plainly and over the assumptions. Measured, alternating in this one process (--rounds):
  create   wall ms of kp_assumptions_create (host packing, upload, k_assume_cluster, sync);
  serial   mean total_ms of kp_stage_times and wall ms per kp_schedule_batch, both batches;
then, with kp_engine_set_profile, each batch's per-kernel HIP-event times: k_est_assumed's
own time, and a check that it runs for the assumed batch only. Needs a HIP device. Prints one
JSON line.

--plain-only measures the plain batch alone, and --tree <checkout> takes the package and the
library from another checkout of the project (the parent commit's, built there): the neutral
comparison is this commit's and the parent's plain batch, a process each, alternating in one
job on one device."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--share", type=float, default=1.0, help="percent of the clusters that carry assumed workloads")
    ap.add_argument("--workloads", type=int, default=100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--bindings", type=int, default=None)
    ap.add_argument("--plain-only", action="store_true", help="the plain batch alone (no assumptions are made)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from karmada_amd import api, synth
    from karmada_amd.engine import Batch, Engine, EngineError, Snapshot
    cfg = 3
    C_, B = synth.CONFIGS[cfg]
    C_, B = args.clusters or C_, args.bindings or B
    try:
        eng = Engine(0)
    except EngineError as ex:
        sys.exit(f"assumed: no HIP device: {ex}")
    u = synth.Universe(cfg, cfg, C_, 0, B)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options())
    structs = u.binding_slice(0, B)
    if args.plain_only:
        plain = Batch(snap, structs=structs)
        runs = [serial(eng, plain, args.steps) for _ in range(args.rounds)]
        print(json.dumps({"config": f"config{cfg}: {B} bindings x {C_} clusters", "tree": os.path.abspath(args.tree),
                          "steps": args.steps, "plain": runs, "kernels": sorted(profiled(eng, plain))}), flush=True)
        plain.close()
        snap.close()
        eng.close()
        return
    from karmada_amd.engine import Assumptions
    rng = np.random.RandomState(1)
    n_assumed = max(1, int(round(C_ * args.share / 100.0)))
    chosen = sorted(rng.choice(C_, size=n_assumed, replace=False).tolist())
    entries = []
    for c in chosen:
        for _ in range(args.workloads):
            req = {"cpu": "%dm" % rng.randint(250, 1001), "memory": "%dMi" % rng.randint(256, 1025)}
            entries.append((c, [{"replicas": int(rng.randint(1, 4)), "replicaRequirements": {"resourceRequest": req}}]))
    create = []
    a = None
    for _ in range(args.rounds):
        if a is not None:
            a.close()
        t0 = time.perf_counter()
        a = Assumptions(snap, entries)
        create.append(round(1e3 * (time.perf_counter() - t0), 3))
    plain = Batch(snap, structs=structs)
    assumed = Batch(snap, structs=structs, assumed=a)
    line = {"config": f"config{cfg}: {B} bindings x {C_} clusters", "assumed_clusters": n_assumed,
            "workloads_per_cluster": args.workloads, "steps": args.steps, "assumptions_create_ms": create}
    runs = {"plain": [], "assumed": []}
    for _ in range(args.rounds):
        runs["plain"].append(serial(eng, plain, args.steps))
        runs["assumed"].append(serial(eng, assumed, args.steps))
    line["serial"] = runs
    kp, ka = profiled(eng, plain), profiled(eng, assumed)
    if "k_est_assumed" in kp or "k_est_assumed" not in ka:
        sys.exit("assumed: k_est_assumed must run for the assumed batch only")
    line["k_est_assumed_ms_per_call"] = ka["k_est_assumed"]["ms"]  # (the last call's)
    line["k_est_assumed_rows"] = ka["k_est_assumed"]["units"]
    print(json.dumps(line), flush=True)
    for b in (assumed, plain):
        b.close()
    a.close()
    snap.close()
    eng.close()


if __name__ == "__main__":
    main()
