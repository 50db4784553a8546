"""Grouped flat collectives (nexrRingGroupStart / nexrRingGroupEnd: the recorded calls as flat group launches and
ONE completion wait) against the same calls through nexrRingAllReduceFlat one by one (a launch and a wait each):
fp32 sum, thread ranks on one GPU, device memory, SIMPLE, at 2, 4 and 8 ranks; W in {1, 4, 16, 64} all-reduces of
4 KiB, 64 KiB, 1 MiB and 4 MiB per rank each, and one mixed bucket list. Every rank count runs in a child process of
its own under `timeout`; the child alternates the two modes, batch by batch, on ONE communicator. A batch is timed
on the host clock from its first call to the return of its last (the group: of nexrRingGroupEnd) and checked exact
on the device against oracle.ring's fold: the works share their inputs and have outputs of their own, so one
expected buffer per size serves them all. Reported per mode: p25, median and p75 of `calls` batches after warm-up.
The group kernel alone at W = 1 is timed with HIP events (nexrFlatGroup on a stream) beside flat_kernel
(nexrFlatAllReduce) on the same buffers and parts: the ratio is the price of the table lookup. After a child that
faulted, aborted or ran into its limit nothing more is started. DESIGN §8.11 has the table.
    python tools/flat_group_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/flat_group_probe.py --child RANKS CALLS"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RANKS = (2, 4, 8)
SIZES = (4 << 10, 64 << 10, 1 << 20, 4 << 20)   # bytes per rank and work
WORKS = (1, 4, 16, 64)
MIXED = (4 << 10, 4 << 10, 64 << 10, 1 << 20, 64 << 10, 4 << 10, 4 << 20, 1 << 20, 4 << 10, 64 << 10, 64 << 10,
         4 << 10, 1 << 20, 4 << 10, 64 << 10, 4 << 10)
WARMUP = 3
CHILD_LIMIT_S = 240
F32, SUM = 7, 0


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def child(n, calls):
    import numpy as np
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    ring = importlib.import_module("nex-nccl_amd.ring")
    from oracle import ring as oring
    assert torch.cuda.is_available(), "the probe needs a GPU"
    rng = np.random.default_rng(n)
    send, exp = {}, {}
    for size in SIZES:
        x = [rng.standard_normal(size // 4).astype(np.float32) for _ in range(n)]
        send[size] = [torch.from_numpy(v).cuda() for v in x]
        want = np.ascontiguousarray(oring.ring_allreduce_expected(x, F32, SUM)[0]).view(np.int32).copy()
        exp[size] = torch.from_numpy(want).cuda()
    # outputs: one [n, count] block per work
    most = {size: max(WORKS + (MIXED.count(size),)) for size in SIZES}
    recv = {size: torch.zeros(most[size], n, size // 4, dtype=torch.float32, device="cuda") for size in SIZES}

    def batch_of(sizes):
        used, works = {}, []
        for size in sizes:
            k = used.get(size, 0)
            used[size] = k + 1
            works.append((size, [t.data_ptr() for t in send[size]], [recv[size][k, r].data_ptr() for r in range(n)]))
        return works, used

    def run_batch(comm, works, grouped):
        t0 = time.perf_counter()
        if grouped:
            comm.group_start()
        for size, sp, rp in works:
            comm.all_reduce_flat(sp, rp, size // 4, F32, SUM)
        if grouped:
            comm.group_end()
        return (time.perf_counter() - t0) * 1e3

    def exact(used):
        return all(bool((recv[size][:k].view(torch.int32) == exp[size]).all()) for size, k in used.items())

    def measure(comm, sizes):
        works, used = batch_of(sizes)
        times, ok, queued = {"group": [], "single": []}, {"group": True, "single": True}, {"group": set(), "single": set()}
        for k in range(2 * (WARMUP + calls)):
            mode = ("group", "single")[k % 2]
            for size in used:
                recv[size].zero_()
            torch.cuda.synchronize()
            dt = run_batch(comm, works, mode == "group")
            ok[mode] = ok[mode] and exact(used)
            queued[mode].add(comm.queued())
            if k >= 2 * WARMUP:
                times[mode].append(dt)
        out = {m: dict(_stats(times[m]), exact=bool(ok[m]), queued=sorted(queued[m])) for m in times}
        out["single_over_group"] = round(out["single"]["median_ms"] / out["group"]["median_ms"], 3)
        return out

    row = {"ranks": n, "gpus_visible": torch.cuda.device_count(), "batches": [], "kernel_w1": []}
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000) as comm:
        for size in SIZES:
            for w in WORKS:
                row["batches"].append(dict({"bytes_per_rank": size, "works": w}, **measure(comm, [size] * w)))
        row["mixed"] = dict({"bytes_per_rank": list(MIXED), "works": len(MIXED)}, **measure(comm, list(MIXED)))
        stats = comm.group_stats()
        row["group_stats"] = stats
    # the kernels alone at W = 1: HIP events round nexrFlatGroup and nexrFlatAllReduce on a stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for size in SIZES:
            count = size // 4
            parts = [(0, count, (4 << 20) // 8 * 4 // 512 * 512 // 4)]
            sp, rp = [t.data_ptr() for t in send[size]], [recv[size][0, r].data_ptr() for r in range(n)]
            work = [{"coll": nexr.FLAT_GROUP_ALL_REDUCE, "inputs": sp, "outputs": rp, "n_elts": count, "datatype": F32,
                     "dev_red_op": SUM, "red_op_arg": 0, "parts": parts}]
            launches = {"group_kernel": lambda s: nexr.flat_group(n, work, True, stream=s),
                        "flat_kernel": lambda s: nexr.flat_all_reduce(sp, rp, count, F32, SUM, 0, True, parts, stream=s)}
            ev, outs = {m: [] for m in launches}, {}
            for k in range(2 * (WARMUP + calls)):
                mode = ("group_kernel", "flat_kernel")[k % 2]
                recv[size][0].zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                launches[mode](stream.cuda_stream)
                b.record(stream)
                stream.synchronize()
                outs[mode] = recv[size][0].clone()
                if k >= 2 * WARMUP:
                    ev[mode].append(a.elapsed_time(b))
            res = {m: _stats(ev[m]) for m in ev}
            res["exact"] = bool(torch.equal(outs["group_kernel"].view(torch.int32), outs["flat_kernel"].view(torch.int32)))
            res["group_over_flat"] = round(res["group_kernel"]["median_ms"] / res["flat_kernel"]["median_ms"], 3)
            row["kernel_w1"].append(dict({"bytes_per_rank": size}, **res))
    return row


def _all_exact(row):
    rows = row["batches"] + [row["mixed"]]
    return all(r["group"]["exact"] and r["single"]["exact"] for r in rows) and all(r["exact"] for r in row["kernel_w1"])


def main():
    calls, out = 30, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped = [], None
    for n in RANKS:
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                            "--child", str(n), str(calls)], capture_output=True, text=True)
        if p.returncode != 0:
            stopped = {"ranks": n, "returncode": p.returncode, "stderr": p.stderr[-500:]}
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print("ranks %d: done" % n, file=sys.stderr, flush=True)
    res = {"workload": "W ring all-reduces of bytes_per_rank each (shared inputs, outputs of their own), fp32 sum, SIMPLE "
                       "communicator, device memory, thread ranks on one GPU: inside nexrRingGroupStart / "
                       "nexrRingGroupEnd (group) and one by one through nexrRingAllReduceFlat (single)",
           "timing": "host clock around each batch; the two modes alternately, batch by batch, in one process; p25 / "
                     "median / p75 of `calls` batches per mode after %d warm-up batches each; kernel_w1: HIP events "
                     "round nexrFlatGroup with one work and round nexrFlatAllReduce on the same buffers" % WARMUP,
           "rows": rows, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0 if not stopped and all(_all_exact(r) for r in rows) else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]))))
        sys.exit(0)
    sys.exit(main())
