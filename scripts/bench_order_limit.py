#!/usr/bin/env python3
"""`order by` / `limit` / `offset` (sh_query_set_order) measured against the same query without it, in one run.

The streams are bench.py's: siddhi_amd.synth's SplitMix64 keyed stream (k, v double, ts long; seed 0xC2), built
on the device for the device pushes (synth.torch_keyed_stream) and on the host for the host pushes
(synth.keyed_stream). Every comparison pushes the same batches into a query with the spec and into one without
it, alternating the two step by step, and reports both medians: nothing here is compared with an earlier number.

  a   the C2 shape: timeBatch(1 sec) count / min / max / avg by 100k keys, per-event sends, with and without
      `order by avg desc limit 10` — device pushes (a_dev) and host pushes (a_host: the D2H copy and the host
      rows of a flush fall from 100k rows to 10)
  b   many flushes per call: lengthBatch(256) over 64 keys with per-event sends, and time(10 sec) over 64 keys
      with sends of 1000 events — `order by count desc, k limit 10` (b_dev, b_host)
  c   the crossover of the two sort routes: lengthBatch(m) over m keys dealt round-robin (every flush holds
      exactly m rows), calls of about 2^18 rows, m = 16 .. 1024, each with SH_ORD_BLOCK_MAX=0 (radix passes) and
      =1024 (one workgroup per flush); the pass's cost is the ordered push minus the plain push

Prints one JSON line; --out also writes it to a file. The pass's own kernel times: run one section under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_order_limit.py --only a_dev --steps 5`, in a run of its
own (the k_ord_* kernels and the radix sort's).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 22, help="events per push of the shapes a and b")
    ap.add_argument("--only", default="a_dev,a_host,b_dev,b_host,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))

    import numpy as np
    import torch

    from siddhi_amd import abi, runtime, synth

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    schema = abi.Schema.parse("k int, v double, ts long")
    nb = args.warmup + args.steps
    res = {"steps": args.steps, "warmup": args.warmup}

    def compare(name, plain, ordered, batches, push, events, env=None):
        """alternate the two queries over the same batches; medians of the steps after the warm-up"""
        old = os.environ.get("SH_ORD_BLOCK_MAX")
        if env is not None:
            os.environ["SH_ORD_BLOCK_MAX"] = env  # (read when a query is created)
        qs = {"plain": runtime.GpuQuery(plain), "ordered": runtime.GpuQuery(ordered)}
        if env is not None:
            if old is None:
                del os.environ["SH_ORD_BLOCK_MAX"]
            else:
                os.environ["SH_ORD_BLOCK_MAX"] = old
        t = {"plain": [], "ordered": []}
        rows = {"plain": 0, "ordered": 0}
        c0 = runtime.order_debug_counts()
        for i, b in enumerate(batches):
            for which in (("plain", "ordered") if i % 2 == 0 else ("ordered", "plain")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = push(qs[which], b)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    t[which].append(dt)
                    rows[which] += o.contents.n_rows
        c1 = runtime.order_debug_counts()
        for q in qs.values():
            q.close()
        mp, mo = statistics.median(t["plain"]), statistics.median(t["ordered"])
        res[name] = {
            "events_per_push": events, "plain_ms": mp * 1e3, "ordered_ms": mo * 1e3, "pass_ms": (mo - mp) * 1e3,
            "plain_events_per_s": events / mp, "ordered_events_per_s": events / mo,
            "plain_ms_min_max": [min(t["plain"]) * 1e3, max(t["plain"]) * 1e3],
            "ordered_ms_min_max": [min(t["ordered"]) * 1e3, max(t["ordered"]) * 1e3],
            "rows_per_push": {k: v / max(1, len(t[k])) for k, v in rows.items()},
            "calls_block_route": c1[1] - c0[1], "calls_global_route": c1[2] - c0[2],
        }
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)

    def dev_batches(B, keys, epm, n=nb):
        out = [synth.torch_keyed_stream(i * B, B, 0xC2, keys, epm, dev) for i in range(n)]
        torch.cuda.synchronize()
        return out

    def host_batches(B, keys, epm, ss, n=nb):
        return [abi.HostBatch(schema, *synth.keyed_stream(i * B, B, 0xC2, keys, epm), ss) for i in range(n)]

    def push_dev(ss):
        return lambda q, b: q.push_device(len(b[0]), b[0].data_ptr(), [c.data_ptr() for c in b[1]], ss)

    def push_host(q, b):
        return q.push_raw(b)

    B = args.batch
    c2 = dict(group_by=["k"], aggs=[("count", None), ("min", "v"), ("max", "v"), ("avg", "v")], key_capacity=100_000)
    top = dict(order_by=[("agg", 3, "desc")], limit=10)
    if "a_dev" in only:
        compare("a_dev_c2_timeBatch_100k_keys", abi.QuerySpec(schema, "timeBatch", 1000, **c2),
                abi.QuerySpec(schema, "timeBatch", 1000, **c2, **top), dev_batches(B, 100_000, 1000), push_dev(1), B)
    if "a_host" in only:
        compare("a_host_c2_timeBatch_100k_keys", abi.QuerySpec(schema, "timeBatch", 1000, **c2),
                abi.QuerySpec(schema, "timeBatch", 1000, **c2, **top), host_batches(B, 100_000, 1000, 1), push_host, B)
    few = dict(group_by=["k"], aggs=[("count", None), ("min", "v"), ("max", "v"), ("avg", "v")], key_capacity=128)
    top_b = dict(order_by=[("agg", 0, "desc"), ("key", 0)], limit=10)
    Bb = min(B, 1 << 20)
    for leg in ("b_dev", "b_host"):
        if leg not in only:
            continue
        for nm, window, param, ss in (("lengthBatch256_64_keys", "lengthBatch", 256, 1), ("time10s_64_keys_send1000", "time", 10_000, 1000)):
            batches = dev_batches(Bb, 64, 1000) if leg == "b_dev" else host_batches(Bb, 64, 1000, ss)
            compare(f"{leg}_{nm}", abi.QuerySpec(schema, window, param, **few),
                    abi.QuerySpec(schema, window, param, **few, **top_b), batches,
                    push_dev(ss) if leg == "b_dev" else push_host, Bb)
    if "c" in only:
        rows_per_call = 1 << 18
        for m in (16, 64, 128, 256, 512, 1024):
            n = rows_per_call  # one row per event: every lengthBatch(m) flush holds m distinct keys
            batches = []
            for i in range(nb):
                idx = torch.arange(i * n, (i + 1) * n, dtype=torch.int64, device=dev)
                k = (idx % m).to(torch.int32)
                v = ((idx * 2654435761) % 1000003).to(torch.float64) / 7.0
                ts = synth.T0 + idx // 1000
                batches.append((ts, [k.contiguous(), v.contiguous(), ts.clone()]))
            torch.cuda.synchronize()
            kw = dict(group_by=["k"], aggs=[("count", None), ("avg", "v")], key_capacity=max(16, 2 * m))
            for route, env in (("global", "0"), ("block", "1024")):
                compare(f"c_flush{m}_{route}", abi.QuerySpec(schema, "lengthBatch", m, **kw),
                        abi.QuerySpec(schema, "lengthBatch", m, **kw, order_by=[("agg", 1, "desc")], limit=10),
                        batches, push_dev(0), n, env=env)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
