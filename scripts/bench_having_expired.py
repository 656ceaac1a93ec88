#!/usr/bin/env python3
"""`having` with all-events output on the C2 shape: timeBatch(1 sec, true) ... insert all events,
count/min/max/avg by 100k keys, device-resident pushes of 2^22 events, per-event sends. Two queries over the
same batches in one run:

  having   with `having count() >= 2`: k_hvx_walk (the fold, then the ordered remove pass of every closing
           window with the min / max deques) and the rows of the passing heads
  plain    the same query without `having` (k_sc_walk, constant expired rows): the yardstick

--no-having times `plain` alone (a library that refuses the having query, for the yardstick on an earlier
build: SH_LIB=<that library>). Prints one JSON line; --out appends it to a file.
Kernel statistics: run this script under `rocprofv3 --kernel-trace --stats -- python ...`, in a run of its own.
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-having", action="store_true")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from siddhi_amd import abi, runtime, synth

    dev = torch.device("cuda:0")
    B, nb = args.batch, args.warmup + args.steps
    schema = abi.Schema.parse("k string, v double, ts long")
    aggs = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]

    def spec(**kw):
        return abi.QuerySpec(schema, "timeBatch", 1000, group_by=["k"], aggs=aggs, key_capacity=100_000,
                             stream_current=True, output="all", **kw)

    batches = [synth.torch_keyed_stream(i * B, B, 0xC2, 100_000, 1000, dev)[1] for i in range(nb)]
    torch.cuda.synchronize()
    variants = [("plain", spec())]
    if not args.no_having:
        variants.insert(0, ("having", spec(having=(">=", ("agg", 0), ("long", 2)))))
    res = {}
    for name, sp in variants:
        q = runtime.GpuQuery(sp)
        rows = 0

        def push(i):
            cols = batches[i]
            return q.push_device(B, cols[2].data_ptr(), [c.data_ptr() for c in cols], 1)

        for i in range(args.warmup):
            push(i)
        torch.cuda.synchronize()
        dev_ms, walk_ms, t0 = 0.0, 0.0, time.perf_counter()
        for i in range(args.warmup, nb):
            rows += push(i).contents.n_rows
            st = q.stats()
            dev_ms += st.push_ms
            walk_ms += st.main_kernel_ms
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        q.close()
        res[name] = {"events_per_s": B * args.steps / el, "device_ms_per_push": dev_ms / args.steps,
                     "walk_ms_per_push": walk_ms / args.steps, "wall_ms_per_push": el * 1e3 / args.steps, "rows": rows}
    out = {"workload": "C2 timeBatch(1 sec, true) insert all events, count/min/max/avg by 100k keys, per-event "
                       "sends, device-resident",
           "label": args.label, "library": os.path.basename(runtime.LIB_PATH), "batch": B, "steps": args.steps,
           "warmup": args.warmup, **res}
    if "having" in res:
        out["having_over_plain"] = res["having"]["events_per_s"] / res["plain"]["events_per_s"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
