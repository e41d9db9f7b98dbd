"""Copy-back cost of the two result formats: kp_schedule_batch (8 bytes per target)
against kp_schedule_batch_packed (4 bytes per target plus 4 per escaped entry).

Workload and engine setup are bench.py's: config 3 at its default size, one engine
(own HIP stream, KP_STREAMS=1, blocking host waits) per lane, every lane with its own
snapshot replica and batch of the same bindings. Timed, for each format in turn
(--rounds times, alternating in this one process):
  serial   one batch at a time on lane 0: mean copy_ms and total_ms of kp_stage_times;
  lanes    --lanes batches in flight, one host thread per lane: ms per step from the
           (warmup x lanes)-th completion to the --steps-th after it, as bench.py does.
Before any timing the packed result, expanded by kp_results_unpack, is compared with the
wide one (the per-binding arrays entry by entry, each binding's targets as a set; whether
the entry order matched too is reported), and the bytes each format copies back per batch
are computed from n_targets, n_wide and B. Needs a HIP device. Prints one JSON line.

--formats wide runs only the wide calls (nothing of the packed interface is touched)."""
import argparse
import json
import os
import sys
import threading
import time

os.environ.setdefault("KP_STREAMS", "1")
os.environ.setdefault("KP_SYNC_BLOCK", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from karmada_amd import api, synth  # noqa: E402
from karmada_amd.engine import Batch, Engine, EngineError, Snapshot  # noqa: E402


def view(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n and ptr else np.zeros(0, dtype)


def call(batch, fmt):
    return batch.schedule_packed_raw() if fmt == "packed" else batch.schedule_raw()


def wide_arrays(w):
    n, t = w.n_bindings, w.n_targets
    return [view(w.status, n, np.int32), view(w.err_code, n, np.int32), view(w.err_arg, n, np.int64),
            view(w.offsets, n + 1, np.uint64), view(w.cluster_idx, t, np.uint32), view(w.replicas, t, np.int32)]


def by_cluster(a):
    """The target arrays with each binding's entries in cluster order. A binding's targets are
    a set (kp_api.h: compare as a multiset), so the formats are compared as sets; whether two
    calls also agreed on the entry order is reported beside it."""
    owner = np.repeat(np.arange(len(a[3]) - 1), np.diff(a[3].astype(np.int64)))
    order = np.lexsort((a[5], a[4], owner))
    return a[:4] + [a[4][order], a[5][order]]


def check_equal(batch):
    """The packed result of `batch`, unpacked, against its wide result: the per-binding arrays
    entry by entry, each binding's targets as a set and, reported, whether they were also in
    the same order (next to the same for two wide calls). Returns the counts and those flags."""
    wide = wide_arrays(batch.schedule_raw())
    again = wide_arrays(batch.schedule_raw())
    n, t = len(wide[0]), len(wide[4])
    p = batch.schedule_packed_raw()
    if p.n_bindings != n or p.n_targets != t:
        sys.exit(f"packed_results: {p.n_bindings} bindings / {p.n_targets} targets packed, {n} / {t} wide")
    ci, rep = batch.unpack(p)
    packed = [view(p.status, n, np.int32), view(p.err_code, n, np.int32), view(p.err_arg, n, np.int64),
              view(p.offsets, n + 1, np.uint64), np.frombuffer(ci, dtype=np.uint32)[:t].copy(),
              np.frombuffer(rep, dtype=np.int32)[:t].copy()]
    for name, a, b in zip(("status", "err_code", "err_arg", "offsets", "cluster_idx", "replicas"), by_cluster(wide),
                          by_cluster(packed)):
        if not np.array_equal(a, b):
            sys.exit(f"packed_results: {name} differs between the formats at {np.flatnonzero(a != b)[:5]}")
    esc = (wide[5] < 0) | (wide[5] >= 65535)
    if int(esc.sum()) != p.n_wide:
        sys.exit(f"packed_results: n_wide {p.n_wide}, {int(esc.sum())} replicas outside 0..65534")
    in_order = bool(np.array_equal(wide[4], packed[4]) and np.array_equal(wide[5], packed[5]))
    wide_in_order = bool(np.array_equal(wide[4], again[4]) and np.array_equal(wide[5], again[5]))
    return int(n), int(t), int(p.n_wide), in_order, wide_in_order


def serial(eng, batch, fmt, steps):
    call(batch, fmt)  # (warm: the page-locked buffers sized, the format's kernels loaded)
    st = []
    t0 = time.perf_counter()
    for _ in range(steps):
        call(batch, fmt)
        st.append(eng.stage_times())
    wall = 1e3 * (time.perf_counter() - t0) / steps
    return {"copy_ms": round(sum(s["copy_ms"] for s in st) / steps, 4),
            "total_ms": round(sum(s["total_ms"] for s in st) / steps, 4), "wall_ms": round(wall, 4)}


def in_flight(lanes, fmt, steps, warmup):
    """bench.py's drive loop: ms per step over `steps` completions with every lane mid-stream."""
    n_warm = warmup * len(lanes)
    lock = threading.Lock()
    clock = {"done": 0, "t0": None, "t1": None}

    def drive(k):
        b_k = lanes[k][2]
        while True:
            with lock:
                if clock["done"] >= n_warm + steps:
                    break
            call(b_k, fmt)
            with lock:
                now = time.perf_counter()
                clock["done"] += 1
                if clock["done"] == n_warm:
                    clock["t0"] = now
                elif clock["done"] == n_warm + steps:
                    clock["t1"] = now

    time.sleep(float(os.environ.get("KP_BENCH_SETTLE_S", "0.3")))
    th = [threading.Thread(target=drive, args=(k,)) for k in range(len(lanes))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    return round(1e3 * (clock["t1"] - clock["t0"]) / steps, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--steps", type=int, default=300, help="timed completions of an in-flight run")
    ap.add_argument("--warmup", type=int, default=5, help="warm-up steps per lane")
    ap.add_argument("--serial-steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3, help="times each format is measured, alternating")
    ap.add_argument("--formats", default="wide,packed")
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--bindings", type=int, default=None)
    args = ap.parse_args()
    formats = [f for f in args.formats.split(",") if f]
    if not formats or set(formats) - {"wide", "packed"} or args.lanes < 1 or args.warmup < 1 or args.steps < 1:
        sys.exit("packed_results: --formats takes wide and/or packed; --lanes, --warmup and --steps at least 1")
    cfg = 3
    C_, B = synth.CONFIGS[cfg]
    C_, B = args.clusters or C_, args.bindings or B
    try:
        eng = Engine(0)
    except EngineError as ex:
        sys.exit(f"packed_results: no HIP device: {ex}")
    u = synth.Universe(cfg, cfg, C_, 0, B)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options())
    lanes = [(eng, snap, Batch(snap, structs=u.binding_slice(0, B)))]
    for _ in range(1, args.lanes):
        e2 = Engine(0)
        s2 = Snapshot.from_bytes(e2, snap.to_bytes(), u.names)
        lanes.append((e2, s2, Batch(s2, structs=u.binding_slice(0, B))))
    line = {"config": f"config{cfg}: {B} bindings x {C_} clusters", "lanes": args.lanes, "steps": args.steps,
            "warmup": args.warmup, "serial_steps": args.serial_steps, "formats": formats}
    if "packed" in formats:
        n, t, nw, in_order, wide_in_order = check_equal(lanes[0][2])
        per_binding = 16 * n + 8 * (n + 1)  # status, err_code (4 each), err_arg (8), offsets
        bytes_ = {"wide": 8 * t + per_binding, "packed": 4 * t + 4 * nw + per_binding + 8 * (n + 1)}
        if bytes_["wide"] - bytes_["packed"] != 4 * t - 4 * nw - 8 * (n + 1):
            sys.exit("packed_results: byte arithmetic")
        line.update({"equal": True, "same_entry_order": in_order, "two_wide_calls_same_entry_order": wide_in_order,
                     "n_targets": t, "n_wide": nw, "per_binding_bytes": per_binding,
                     "wide_offsets_bytes": 8 * (n + 1), "bytes_per_batch": bytes_,
                     "bytes_ratio": round(bytes_["packed"] / bytes_["wide"], 4)})
    runs = {f: {"serial": [], "lanes_ms_per_step": []} for f in formats}
    for _ in range(args.rounds):
        for f in formats:
            runs[f]["serial"].append(serial(eng, lanes[0][2], f, args.serial_steps))
        for f in formats:
            runs[f]["lanes_ms_per_step"].append(in_flight(lanes, f, args.steps, args.warmup))
    line["runs"] = runs
    print(json.dumps(line), flush=True)
    for e_k, s_k, b_k in reversed(lanes):
        b_k.close()
        s_k.close()
        e_k.close()


if __name__ == "__main__":
    main()
