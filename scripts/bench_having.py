#!/usr/bin/env python3
"""`having` on the C2 shape: timeBatch(1 sec), count/min/max/avg by 100k keys, device-resident pushes of
2^22 events, per-event sends. Three queries over the same batches in one run:

  having   the query with `having count() >= 2` (the sort-and-walk path with k_hv_walk)
  plain    the same query without `having` (the multisplit aggregation path)
  current  the same window with stream.current.event (the sort-and-walk path with k_sc_walk): the
           yardstick, `having` adds one program evaluation per event to that pipeline

Prints one JSON line with the three events/s figures; --out also writes it to a file.
Kernel statistics of k_hv_walk: run this script under `rocprofv3 --kernel-trace --stats -- python ...`.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from siddhi_amd import abi, runtime, synth

    dev = torch.device("cuda:0")
    B, nb = args.batch, args.warmup + args.steps
    schema = abi.Schema.parse("k string, v double, ts long")
    aggs = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]

    def spec(**kw):
        return abi.QuerySpec(schema, "timeBatch", 1000, group_by=["k"], aggs=aggs, key_capacity=100_000, **kw)

    batches = [synth.torch_keyed_stream(i * B, B, 0xC2, 100_000, 1000, dev)[1] for i in range(nb)]
    torch.cuda.synchronize()
    res = {}
    for name, sp in (("having", spec(having=(">=", ("agg", 0), ("long", 2)))), ("plain", spec()),
                     ("current", spec(stream_current=True))):
        q = runtime.GpuQuery(sp)
        rows = 0

        def push(i):
            cols = batches[i]
            return q.push_device(B, cols[2].data_ptr(), [c.data_ptr() for c in cols], 1)

        for i in range(args.warmup):
            push(i)
        torch.cuda.synchronize()
        dev_ms, t0 = 0.0, time.perf_counter()
        for i in range(args.warmup, nb):
            rows += push(i).contents.n_rows
            dev_ms += q.stats().push_ms
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        q.close()
        res[name] = {"events_per_s": B * args.steps / el, "device_ms_per_push": dev_ms / args.steps,
                     "wall_ms_per_push": el * 1e3 / args.steps, "rows": rows}
    out = {"workload": "C2 timeBatch(1 sec) count/min/max/avg by 100k keys, per-event sends, device-resident",
           "batch": B, "steps": args.steps, "warmup": args.warmup, **res,
           "having_over_current": res["having"]["events_per_s"] / res["current"]["events_per_s"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
