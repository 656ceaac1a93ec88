#!/usr/bin/env python3
"""The sliding length(N) window on the C3 shape: the C3 stream (10k keys, 1000 events per event-time ms,
per-event sends, device-resident pushes), count/min/max/avg group by k, with N chosen so that the window
holds what C3's time(10 sec) holds: N = 10 000 ms x the generator's events per ms.

  current   `insert into` (current events): records, key-partition replay with lazy expiry
  all       `insert all events`: the closed-form operation indices (k_len_ops) and the wave-per-key replay
  nogroup   the same aggregators without group-by, `all events`: ONE key, whose adds and removes the
            reference folds in sequence (double += / -= in arrival order), so it is replayed serially —
            reported separately, on a smaller push and window (--nogroup-batch, --nogroup-n)

Prints one JSON line per query; --out appends them to a file. Run in the same session as
`bench.py --workload c3` and `--workload c3all`, the time-window lines these are read against.
Kernel statistics of one push: `rocprofv3 --kernel-trace --stats -- python scripts/bench_length.py --steps 1
--warmup 1 --only all`.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EVENTS_PER_MS = 1000   # the C3 generator's rate
KEYS = 10_000
WINDOW_MS = 10_000     # C3: time(10 sec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 25)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nogroup-batch", type=int, default=1 << 20)
    ap.add_argument("--nogroup-n", type=int, default=1 << 18)
    ap.add_argument("--only", choices=["current", "all", "nogroup"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from siddhi_amd import abi, runtime, synth

    dev = torch.device("cuda:0")
    N = WINDOW_MS * EVENTS_PER_MS
    schema = abi.Schema.parse("k string, v double, ts long")
    aggs = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]
    nb = args.warmup + args.steps
    lines = []
    cases = [("current", args.batch, N, True, "current"), ("all", args.batch, N, True, "all"),
             ("nogroup", args.nogroup_batch, args.nogroup_n, False, "all")]
    batches, batch_of = None, None
    for name, B, n_len, grouped, output in cases:
        if args.only and name != args.only:
            continue
        if batch_of != B:
            batches = None
            torch.cuda.empty_cache()
            batches = [synth.torch_keyed_stream(i * B, B, 0xC3, KEYS, EVENTS_PER_MS, dev)[1] for i in range(nb)]
            batch_of = B
            torch.cuda.synchronize()
        spec = abi.QuerySpec(schema, "length", n_len, group_by=["k"] if grouped else (), aggs=aggs,
                             key_capacity=KEYS if grouped else 1, output=output)
        q = runtime.GpuQuery(spec)
        if output == "all":
            q.set_device_flushes()   # as bench.py's c3all: the per-send flush layout stays in HBM
        else:
            q.set_compact_flushes()  # as bench.py's c3: a row per event, flush i = row i

        def push(i):
            cols = batches[i]
            return q.push_device(B, cols[2].data_ptr(), [c.data_ptr() for c in cols], 1)

        for i in range(args.warmup):
            push(i)
        torch.cuda.synchronize()
        rows, dev_ms, kern_ms, t0 = 0, 0.0, 0.0, time.perf_counter()
        for i in range(args.warmup, nb):
            rows += push(i).contents.n_rows
            st = q.stats()
            dev_ms += st.push_ms
            kern_ms += st.main_kernel_ms
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        q.close()
        lines.append(json.dumps({
            "workload": f"length({n_len}) count/min/max/avg " + ("group by k, 10k keys" if grouped else "no group-by")
                        + f", C3 stream ({EVENTS_PER_MS} events/ms), per-event sends, insert {output} events",
            "query": name, "window_events": n_len, "window_derivation": f"{WINDOW_MS} ms x {EVENTS_PER_MS} events/ms",
            "batch": B, "steps": args.steps, "warmup": args.warmup, "events_per_s": B * args.steps / el,
            "device_ms_per_push": dev_ms / args.steps, "replay_ms_per_push": kern_ms / args.steps,
            "wall_ms_per_push": el * 1e3 / args.steps, "rows": rows}))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
