"""Cost of the delta result form on a fleet at rest: kp_schedule_batch (every binding's
targets copied back) against kp_schedule_batch_delta (the changed bindings' alone).

The batch is the metric configuration's second cycle: config 3 at its default size is
scheduled once, every binding's spec.Clusters is set to that result, and a stated share of
the bindings that hold targets (--share, e.g. 0.01 and 0.10) then get the first entry of
their spec.Clusters raised by one replica, so that their placement differs. Engine setup is
bench.py's (one engine per lane, KP_STREAMS=1, blocking host waits, every lane its own
snapshot replica and batch). Timed, for each format in turn (--rounds times, alternating):
  serial   one batch at a time on lane 0: mean copy_ms and total_ms of kp_stage_times;
  lanes    --lanes batches in flight, one host thread per lane: ms per step from the
           (warmup x lanes)-th completion to the --steps-th after it, as bench.py does.
Before any timing the delta result is checked against the wide one of the same batch (the
flags derived here from the wide result and the bindings' spec.Clusters), the bytes each
format copies back are computed, and one profiled delta call gives k_changed's own time.

--tree DIR imports karmada_amd (and its libkp.so) from another checkout, --formats wide
runs the wide calls alone: together they time an older library on the same batch.
Needs a HIP device. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

os.environ.setdefault("KP_STREAMS", "1")
os.environ.setdefault("KP_SYNC_BLOCK", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def view(np, ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n and ptr else np.zeros(0, dtype)


def second_cycle(np, api, u, r, share):
    """The universe's bindings with spec.Clusters = the wide result r, the first entry of every
    k-th binding that holds targets one replica up. Returns (bindings, what keeps them alive,
    the perturbed indices)."""
    n, t = int(r.n_bindings), int(r.n_targets)
    off = view(np, r.offsets, n + 1, np.int64)
    cidx, rep = view(np, r.cluster_idx, t, np.int64), view(np, r.replicas, t, np.int32)
    status = view(np, r.status, n, np.int32)
    assert C.sizeof(api.kp_target_cluster) == 24 and api.kp_target_cluster.replicas.offset == 16
    name_ptr = np.array([C.cast(C.byref(u.clusters[c].name), C.POINTER(C.c_uint64))[0] for c in range(u.n_clusters)],
                        dtype=np.uint64)
    name_len = np.array([u.clusters[c].name.len for c in range(u.n_clusters)], dtype=np.uint32)
    tg = np.zeros(max(1, t), dtype=[("ptr", "u8"), ("len", "u4"), ("p0", "u4"), ("rep", "i4"), ("p1", "u4")])
    tg["ptr"][:t], tg["len"][:t], tg["rep"][:t] = name_ptr[cidx], name_len[cidx], rep
    held = np.flatnonzero((status == 0) & (off[1:] > off[:-1]))
    perturbed = held[::max(1, int(round(1 / share)))] if share > 0 else held[:0]
    tg["rep"][off[perturbed]] += 1
    ba = (api.kp_binding * n)()
    C.memmove(ba, u.bindings, n * C.sizeof(api.kp_binding))
    base = tg.ctypes.data
    for i in range(n):
        k = int(off[i + 1] - off[i]) if status[i] == 0 else 0
        ba[i].clusters = C.cast(C.c_void_p(base + 24 * int(off[i])), C.POINTER(api.kp_target_cluster))
        ba[i].n_clusters = k
    return ba, (tg, off, cidx), perturbed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--steps", type=int, default=120, help="timed completions of an in-flight run")
    ap.add_argument("--warmup", type=int, default=5, help="warm-up steps per lane")
    ap.add_argument("--serial-steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="times each format is measured, alternating")
    ap.add_argument("--formats", default="wide,delta")
    ap.add_argument("--share", type=float, default=0.01, help="share of the placed bindings perturbed")
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--bindings", type=int, default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout to import karmada_amd from")
    args = ap.parse_args()
    formats = [f for f in args.formats.split(",") if f]
    if not formats or set(formats) - {"wide", "delta"} or min(args.lanes, args.warmup, args.steps, args.serial_steps) < 1:
        sys.exit("delta_ab: --formats takes wide and/or delta; --lanes, --warmup and the step counts at least 1")
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    from karmada_amd import api, synth
    from karmada_amd.engine import Batch, Engine, EngineError, Snapshot

    def call(batch, fmt):
        return batch.schedule_delta_raw() if fmt == "delta" else batch.schedule_raw()

    cfg = 3
    C_, B = synth.CONFIGS[cfg]
    C_, B = args.clusters or C_, args.bindings or B
    try:
        eng = Engine(0)
    except EngineError as ex:
        sys.exit(f"delta_ab: no HIP device: {ex}")
    u = synth.Universe(cfg, cfg, C_, 0, B)
    snap = Snapshot.from_structs(eng, u.clusters, u.n_clusters, u.names, api.options())
    first = Batch(snap, structs=u.binding_slice(0, B))
    ba, keep, perturbed = second_cycle(np, api, u, first.schedule_raw(), args.share)
    first.close()
    lanes = [(eng, snap, Batch(snap, structs=(ba, B)))]
    for _ in range(1, args.lanes):
        e2 = Engine(0)
        s2 = Snapshot.from_bytes(e2, snap.to_bytes(), u.names)
        lanes.append((e2, s2, Batch(s2, structs=(ba, B))))
    line = {"config": f"config{cfg}, second cycle: {B} bindings x {C_} clusters", "tree": os.path.abspath(args.tree),
            "share": args.share, "perturbed": int(len(perturbed)), "lanes": args.lanes, "steps": args.steps,
            "warmup": args.warmup, "serial_steps": args.serial_steps, "formats": formats}
    b0 = lanes[0][2]
    w = b0.schedule_raw()
    n, t = int(w.n_bindings), int(w.n_targets)
    off = view(np, w.offsets, n + 1, np.int64)
    wc, wr, ws = view(np, w.cluster_idx, t, np.int64), view(np, w.replicas, t, np.int32), view(np, w.status, n, np.int32)
    per_binding = 16 * n
    line.update({"n_targets_all": t, "bytes_per_batch": {"wide": 8 * t + per_binding + 8 * (n + 1)}})
    if "delta" in formats:
        # the flags from the wide result and the bindings' spec.Clusters: sizes, then each
        # side's (cluster, replicas) pairs sorted within the binding and compared in place
        tg, poff, pc = keep
        pr = tg["rep"][:len(pc)]
        cnt_w, cnt_p = off[1:] - off[:-1], poff[1:] - poff[:-1]
        size_eq = cnt_w == cnt_p
        own_w, own_p = np.repeat(np.arange(n), cnt_w), np.repeat(np.arange(n), cnt_p)
        ow, op = np.lexsort((wr, wc, own_w)), np.lexsort((pr, pc, own_p))
        sw, sp = size_eq[own_w[ow]], size_eq[own_p[op]]
        differ = (wc[ow][sw] != pc[op][sp]) | (wr[ow][sw] != pr[op][sp])
        flags = (ws == 0) & (~size_eq | (np.bincount(own_w[ow][sw][differ], minlength=n) > 0))
        d = b0.schedule_delta_raw()
        k, dt = int(d.n_changed), int(d.n_targets)
        want = np.flatnonzero(flags)
        keep_t = np.repeat(flags, off[1:] - off[:-1])
        ok = (k == len(want) and np.array_equal(view(np, d.changed, k, np.int64), want) and dt == int(keep_t.sum()) and
              int(d.n_targets_all) == t and np.array_equal(view(np, d.status, n, np.int32), ws) and
              np.array_equal(np.sort(view(np, d.cluster_idx, dt, np.int64)), np.sort(wc[keep_t])))
        if not ok:
            sys.exit(f"delta_ab: the delta result ({k} changed, {dt} targets) is not the wide one's ({len(want)}, "
                     f"{int(keep_t.sum())})")
        line.update({"equal": True, "n_changed": k, "n_targets": dt})
        line["bytes_per_batch"]["delta"] = per_binding + 24 + 4 * k + 8 * (k + 1) + 8 * dt
        eng.set_profile(True)
        b0.schedule_delta_raw()
        kt = eng.kernel_times()
        eng.set_profile(False)
        line["kernel_ms"] = {name: round(v["ms"], 4) for name, v in kt.items()
                             if name.startswith("k_changed") or name in ("k_offsets", "k_compact")}

    def serial(fmt):
        call(b0, fmt)  # (warm: the page-locked buffers sized, the format's kernels loaded)
        st = []
        t0 = time.perf_counter()
        for _ in range(args.serial_steps):
            call(b0, fmt)
            st.append(eng.stage_times())
        wall = 1e3 * (time.perf_counter() - t0) / args.serial_steps
        return {"copy_ms": round(sum(s["copy_ms"] for s in st) / len(st), 4),
                "total_ms": round(sum(s["total_ms"] for s in st) / len(st), 4), "wall_ms": round(wall, 4)}

    def in_flight(fmt):
        """bench.py's drive loop: ms per step over --steps completions with every lane mid-stream."""
        n_warm = args.warmup * len(lanes)
        lock = threading.Lock()
        clock = {"done": 0, "t0": None, "t1": None}

        def drive(j):
            while True:
                with lock:
                    if clock["done"] >= n_warm + args.steps:
                        break
                call(lanes[j][2], fmt)
                with lock:
                    now = time.perf_counter()
                    clock["done"] += 1
                    if clock["done"] == n_warm:
                        clock["t0"] = now
                    elif clock["done"] == n_warm + args.steps:
                        clock["t1"] = now

        th = [threading.Thread(target=drive, args=(j,)) for j in range(len(lanes))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        return round(1e3 * (clock["t1"] - clock["t0"]) / args.steps, 4)

    runs = {f: {"serial": [], "lanes_ms_per_step": []} for f in formats}
    for _ in range(args.rounds):
        for f in formats:
            runs[f]["serial"].append(serial(f))
        for f in formats:
            runs[f]["lanes_ms_per_step"].append(in_flight(f))
    line["runs"] = runs
    print(json.dumps(line), flush=True)
    for e_k, s_k, b_k in reversed(lanes):
        b_k.close()
        s_k.close()
        e_k.close()
    del keep


if __name__ == "__main__":
    main()
