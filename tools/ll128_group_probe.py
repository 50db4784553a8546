"""C1's schedule (fp32 sum all-reduce, 4 MiB per rank, thread ranks on one GPU, device memory) with the LL128
protocol at 2, 3, 4 and 8 ranks, by how the LL128 steps run (nexrRingCommGetQueued): 0 host-sequenced (the
default, one launch and one completion wait per step) and 3 group launches on one stream
(nexrRingCommSetLLGroup: nexrReduceCopyLL128StepsGroup, the ordered hand-off). The method is
tools/ll_group_probe.py's: every (ranks, mode) runs in a child process of its own under `timeout`, twice in
alternation so that the spread between two runs of the same code shows; a child times each all-reduce on
the host clock (the call returns after its device wait), checks every call exact, and reports the median
of its calls after warm-up. After a child that faulted, aborted or ran into its limit nothing more is
started. DESIGN §8.3 has the table.
    python tools/ll128_group_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/ll128_group_probe.py --child RANKS MODE CALLS"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANKS = (2, 3, 4, 8)
COUNT = 1 << 20  # 4 MiB of fp32 per rank
WARMUP = 3
CHILD_LIMIT_S = 120


def child(n, mode, calls):
    import numpy as np
    import torch
    ring = importlib.import_module("nex-nccl_amd.ring")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    rng = np.random.default_rng(n)
    # small integers: fp32 sums are exact in any fold order
    x = [rng.integers(-1000, 1000, COUNT).astype(np.float32) for _ in range(n)]
    expect = np.sum(x, axis=0, dtype=np.float32)
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(COUNT, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
    times, exact, queued = [], True, set()
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, protocol=ring.PROTO_LL128, timeout_ms=10000) as comm:
        if mode == 3:
            comm.set_ll_group(True)
        for k in range(WARMUP + calls):
            for r in recv:
                r.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            comm.all_reduce(sp, rp, COUNT, 7, 0)
            dt = time.perf_counter() - t0
            exact = exact and all(np.array_equal(r.cpu().numpy(), expect) for r in recv)
            queued.add(comm.queued())
            if k >= WARMUP:
                times.append(dt * 1e3)
    times.sort()
    return {"ranks": n, "mode": mode, "queued": sorted(queued), "exact": bool(exact), "calls": len(times),
            "median_ms": round(statistics.median(times), 4), "min_ms": round(times[0], 4),
            "p25_ms": round(times[len(times) // 4], 4), "p75_ms": round(times[3 * len(times) // 4], 4),
            "gpus_visible": torch.cuda.device_count()}


def main():
    calls, out = 30, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped = [], None
    for rnd in range(2):
        for n in RANKS:
            for mode in (0, 3):
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                    "--child", str(n), str(mode), str(calls)], capture_output=True, text=True)
                if p.returncode != 0:
                    stopped = {"ranks": n, "mode": mode, "round": rnd, "returncode": p.returncode,
                               "stderr": p.stderr[-500:]}
                    break
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["round"] = rnd
                rows.append(row)
            if stopped:
                break
        if stopped:
            break
    res = {"workload": "ring all-reduce, fp32 sum, 4 MiB per rank, LL128, device memory, thread ranks on one GPU",
           "timing": "host clock around each blocking call, median of `calls` after %d warm-up calls" % WARMUP,
           "rows": rows, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 1 if stopped or not all(r["exact"] for r in rows) else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]))))
        sys.exit(0)
    sys.exit(main())
