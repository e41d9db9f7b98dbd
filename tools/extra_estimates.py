"""Cost of the other estimators' answers on the schedule path (kp_batch_create_estimates).

Workload: config 3 at its default size (100k bindings x 5k clusters), one engine, one batch
at a time. The same bindings are packed twice against one snapshot: plainly, and with
--rows rows (64) assigned by request class (every distinct ReplicaRequirements takes row
`its index mod rows`; --split k > 1 spreads the bindings of one request over k rows instead,
which multiplies the estimator classes). A row holds, per cluster, -1 (10%), MaxInt32 (10%)
or an answer drawn from 0..--cap. Measured, alternating in this one process (--rounds):
  serial   mean total_ms of kp_stage_times and wall ms per kp_schedule_batch, both batches;
then, with kp_engine_set_profile, each batch's per-kernel HIP-event times: k_est_extra's own
time and the kernels the class split makes longer (k_est_class*, k_class_order). The extra
upload is computed from the class counts the profile reports: 4 bytes per class (its row id),
per class with a row (the list) and per padded row entry. Needs a HIP device. Prints one
JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from karmada_amd import api, synth  # noqa: E402
from karmada_amd.engine import Batch, Engine, EngineError, Snapshot  # noqa: E402


def request_key(b):
    if not b.has_replica_requirements:
        return None
    return tuple((C.string_at(r.name.ptr, r.name.len), C.string_at(r.quantity.ptr, r.quantity.len))
                 for r in (b.resource_request[j] for j in range(b.n_resource_request)))


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
    ap.add_argument("--split", type=int, default=1, help="rows the bindings of one request are spread over")
    ap.add_argument("--cap", type=int, default=200, help="largest answer drawn for a row entry")
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
        sys.exit(f"extra_estimates: no HIP device: {ex}")
    u = synth.Universe(cfg, cfg, C_, 0, B)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options())
    kinds = {}
    row_of = np.empty(B, dtype=np.int32)
    for i in range(B):
        k = kinds.setdefault(request_key(u.bindings[i]), len(kinds))
        row_of[i] = (k * args.split + i % args.split) % args.rows
    rng = np.random.RandomState(1)
    rows = rng.randint(0, args.cap + 1, size=(args.rows, C_)).astype(np.int32)
    mark = rng.randint(0, 10, size=rows.shape)
    rows[mark == 0] = -1
    rows[mark == 1] = 2**31 - 1
    structs = u.binding_slice(0, B)
    t0 = time.perf_counter()
    plain = Batch(snap, structs=structs)
    t1 = time.perf_counter()
    est = Batch(snap, structs=structs, estimates=(rows, row_of))
    t2 = time.perf_counter()
    line = {"config": f"config{cfg}: {B} bindings x {C_} clusters", "rows": args.rows, "split": args.split,
            "request_kinds": len(kinds), "steps": args.steps,
            "create_ms": {"plain": round(1e3 * (t1 - t0), 2), "estimates": round(1e3 * (t2 - t1), 2)}}
    runs = {"plain": [], "estimates": []}
    for _ in range(args.rounds):
        runs["plain"].append(serial(eng, plain, args.steps))
        runs["estimates"].append(serial(eng, est, args.steps))
    line["serial"] = runs
    kp, ke = profiled(eng, plain), profiled(eng, est)
    if "k_est_extra" in kp or "k_est_extra" not in ke:
        sys.exit("extra_estimates: k_est_extra must run for the batch with estimates only")

    def classes(kt):
        return sum(v["units"] for k, v in kt.items() if k.startswith("k_est_class"))

    cp = (C_ + 63) // 64 * 64
    with_row = ke["k_est_extra"]["units"]
    line["classes"] = {"plain": classes(kp), "estimates": classes(ke), "with_row": with_row}
    line["extra_upload_bytes"] = 4 * (classes(ke) + with_row + args.rows * cp)
    line["k_est_extra_ms"] = ke["k_est_extra"]["ms"]
    line["kernels_ms"] = {name: {"plain": kp.get(name, {}).get("ms"), "estimates": ke.get(name, {}).get("ms")}
                          for name in sorted(set(kp) | set(ke))}
    print(json.dumps(line), flush=True)
    for b in (est, plain):
        b.close()
    snap.close()
    eng.close()


if __name__ == "__main__":
    main()
