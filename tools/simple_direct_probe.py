"""DirectWrite against FIFOs for the SIMPLE ring collectives (nexrRingCommSetDirect), thread ranks on one GPU,
device memory. Workloads: C1's payload (fp32 sum all-reduce, 4 MiB per rank, out of place) at 2, 4 and 8 ranks
and at 4 ranks x 2 channels; an all-gather into 4 MiB per rank and a broadcast of 4 MiB, out of place, at 2 and
8 ranks. Settings: host-sequenced steps and group launches (nexrRingCommSetSimpleGroup), each through FIFOs and
direct. ONE child process per (workload, setting) under `timeout`; every setting of a workload runs twice, the
settings in alternation (A B C D A B C D), so that a drift of the machine shows as a difference between a
setting's two runs. A child makes 3 warm-up calls and then `calls` timed ones on the host clock (a call returns
after its device wait), checks EVERY call exact against oracle.ring, and reports its median. After a child that
faulted, aborted or ran into its limit nothing more is started. A library without the option (an older build of
this tree, for the baseline) runs the two FIFO settings only. DESIGN §8.3 has the table.
    python tools/simple_direct_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/simple_direct_probe.py --child COLL RANKS CHANNELS GROUP DIRECT CALLS"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("all_reduce", 2, 1), ("all_reduce", 4, 1), ("all_reduce", 8, 1), ("all_reduce", 4, 2),
             ("all_gather", 2, 1), ("all_gather", 8, 1), ("broadcast", 2, 1), ("broadcast", 8, 1))
SETTINGS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (group launches, direct)
COUNT = 1 << 20  # 4 MiB of fp32
WARMUP = 3
CHILD_LIMIT_S = 120
F32, SUM = 7, 0


def child(coll, n, channels, group, direct, calls):
    import numpy as np
    import torch
    ring = importlib.import_module("nex-nccl_amd.ring")
    from oracle.ring import all_gather_expected, broadcast_expected, ring_allreduce_expected
    assert torch.cuda.is_available(), "the probe needs a GPU"
    rng = np.random.default_rng(n)
    per = COUNT // n
    x = [rng.standard_normal(per if coll == "all_gather" else COUNT).astype(np.float32) for _ in range(n)]
    expect = (ring_allreduce_expected(x, F32, SUM, n_channels=channels) if coll == "all_reduce"
              else all_gather_expected(x) if coll == "all_gather" else broadcast_expected(x, 0))
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(COUNT, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
    times, exact, slices, queued = [], True, set(), set()
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000, n_channels=channels) as comm:
        comm.set_simple_group(bool(group))
        if direct:
            comm.set_direct(True)
        for k in range(WARMUP + calls):
            for r in recv:
                r.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if coll == "all_reduce":
                comm.all_reduce(sp, rp, COUNT, F32, SUM)
            elif coll == "all_gather":
                comm.all_gather(sp, rp, per, F32)
            else:
                comm.broadcast(sp, rp, COUNT, F32, 0)
            dt = time.perf_counter() - t0
            exact = exact and all(r.cpu().numpy().tobytes() == np.asarray(e).tobytes() for r, e in zip(recv, expect))
            queued.add(comm.queued())
            if hasattr(comm, "direct_slices"):
                slices.add(comm.direct_slices())
            if k >= WARMUP:
                times.append(dt * 1e3)
    t = sorted(times)
    return {"coll": coll, "ranks": n, "channels": channels, "group": group, "direct": direct, "exact": bool(exact),
            "queued": sorted(queued), "slices_direct_fifo": sorted(slices), "calls": len(t),
            "median_ms": round(statistics.median(t), 4), "p25_ms": round(t[len(t) // 4], 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def main():
    calls, out = 30, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(1, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    ring = importlib.import_module("nex-nccl_amd.ring")
    settings = SETTINGS if hasattr(ring.RingComm, "set_direct") else tuple(s for s in SETTINGS if not s[1])
    rows, stopped = [], None
    for coll, n, channels in WORKLOADS:
        for rep in range(2):
            for group, direct in settings:
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                    "--child", coll, str(n), str(channels), str(group), str(direct), str(calls)],
                                   capture_output=True, text=True)
                if p.returncode != 0:
                    stopped = {"coll": coll, "ranks": n, "channels": channels, "group": group, "direct": direct,
                               "returncode": p.returncode, "stderr": p.stderr[-500:]}
                    break
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["run"] = rep
                rows.append(row)
                print(json.dumps(row), flush=True)
            if stopped:
                break
        if stopped:
            break
    res = {"workloads": "SIMPLE ring collectives, fp32, 4 MiB per rank, device memory, thread ranks on one GPU, out of place",
           "timing": "host clock around each blocking call; one child process per (workload, setting, run), two runs per "
                     "setting in alternation; median / p25 / p75 of %d calls after %d warm-up calls" % (calls, WARMUP),
           "has_direct": len(settings) == len(SETTINGS), "rows": rows, "stopped": stopped}
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 1 if stopped or not all(r["exact"] for r in rows) else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        a = sys.argv[i + 1:i + 7]
        print(json.dumps(child(a[0], int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]))))
        sys.exit(0)
    sys.exit(main())
