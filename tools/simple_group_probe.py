"""C1's payload (fp32 sum all-reduce, 4 MiB per rank, thread ranks on one GPU, device memory) with the SIMPLE
protocol at 2, 4 and 8 ranks and at 4 ranks x 2 channels, by how the SIMPLE steps run
(nexrRingCommGetQueued): 0 host-sequenced (the default: one launch, one completion wait and the host's
head / tail stores per slice) and 3 group launches on one stream (nexrRingCommSetSimpleGroup:
nexrReduceCopySimpleStepsGroup, tails and heads in device memory). Every configuration runs in a child
process of its own under `timeout`; the child switches the option off and on ALTERNATELY, call by call, on
one communicator, times each all-reduce on the host clock (the call returns after its device wait), checks
every call exact against the oracle's ring fold (oracle.ring.ring_allreduce_expected), and reports p25,
median and p75 per mode over `calls` calls each after warm-up. After a child that faulted, aborted or ran
into its limit nothing more is started. DESIGN §8.3 has the table.
    python tools/simple_group_probe.py [--calls 20] [--out profiles/NAME.json]
    python tools/simple_group_probe.py --child RANKS CHANNELS CALLS"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((2, 1), (4, 1), (8, 1), (4, 2))  # (ranks, channels)
COUNT = 1 << 20  # 4 MiB of fp32 per rank
WARMUP = 3       # per mode
CHILD_LIMIT_S = 120
F32, SUM = 7, 0


def child(n, channels, calls):
    import numpy as np
    import torch
    ring = importlib.import_module("nex-nccl_amd.ring")
    from oracle.ring import ring_allreduce_expected
    assert torch.cuda.is_available(), "the probe needs a GPU"
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(COUNT).astype(np.float32) for _ in range(n)]
    expect = ring_allreduce_expected(x, F32, SUM, n_channels=channels)
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(COUNT, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
    times, queued, exact = {0: [], 3: []}, {0: set(), 3: set()}, True
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000, n_channels=channels) as comm:
        for k in range(2 * (WARMUP + calls)):
            mode = 3 if k & 1 else 0
            comm.set_simple_group(mode == 3)
            for r in recv:
                r.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            comm.all_reduce(sp, rp, COUNT, F32, SUM)
            dt = time.perf_counter() - t0
            exact = exact and all(r.cpu().numpy().tobytes() == np.asarray(e).tobytes() for r, e in zip(recv, expect))
            queued[mode].add(comm.queued())
            if k >= 2 * WARMUP:
                times[mode].append(dt * 1e3)
    row = {"ranks": n, "channels": channels, "exact": bool(exact), "gpus_visible": torch.cuda.device_count()}
    for mode, name in ((0, "off"), (3, "on")):
        t = sorted(times[mode])
        row[name] = {"queued": sorted(queued[mode]), "calls": len(t), "p25_ms": round(t[len(t) // 4], 4),
                     "median_ms": round(statistics.median(t), 4), "p75_ms": round(t[3 * len(t) // 4], 4),
                     "min_ms": round(t[0], 4)}
    return row


def main():
    calls, out = 20, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped = [], None
    for n, channels in CONFIGS:
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                            "--child", str(n), str(channels), str(calls)], capture_output=True, text=True)
        if p.returncode != 0:
            stopped = {"ranks": n, "channels": channels, "returncode": p.returncode, "stderr": p.stderr[-500:]}
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"workload": "ring all-reduce, fp32 sum, 4 MiB per rank, SIMPLE, device memory, thread ranks on one GPU",
           "timing": "host clock around each blocking call; option off and on alternately, call by call, in one "
                     "process; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each" % WARMUP,
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
