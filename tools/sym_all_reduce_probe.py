"""The symmetric all-reduce (nexrRingAllReduceSymmetric: one launch, peer loads and stores) against the ring
all-reduce of the same communicator, fp32 sum, thread ranks on one GPU, device memory, SIMPLE, at 2, 4 and 8
ranks and 64 KiB, 4 MiB (C1's payload) and 64 MiB per rank. Every configuration runs in a child process of
its own under `timeout`; the child alternates three modes call by call on ONE communicator: the symmetric
call, the host-sequenced ring (nexrRingCommSetSimpleGroup off) and the ring in group launches (on). Each call
is timed on the host clock (it returns after its device wait) and checked exact on the device: the symmetric
call against tests/sym_cases.py's owner-first fp32 fold, the ring calls against oracle.ring's fold. Reported
per mode: p25, median and p75 of `calls` calls after warm-up. The symmetric kernel alone is also timed with
HIP events (nexrSymAllReduce on a stream, median of `calls`), with 2 * n * nBytes / time as a fraction of
8 TB/s. After a child that faulted, aborted or ran into its limit nothing more is started. DESIGN §8.4 has the
table.
    python tools/sym_all_reduce_probe.py [--calls 20] [--out profiles/NAME.json]
    python tools/sym_all_reduce_probe.py --child RANKS BYTES CALLS"""
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
SIZES = (64 << 10, 4 << 20, 64 << 20)  # bytes per rank
WARMUP = 3                            # per mode
CHILD_LIMIT_S = 150
F32, SUM = 7, 0
MODES = ("symmetric", "ring_host_sequenced", "ring_group")
PEAK_BYTES_PER_S = 8e12


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def child(n, n_bytes, calls):
    import numpy as np
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    ring = importlib.import_module("nex-nccl_amd.ring")
    import sym_cases as sc
    from oracle.ring import ring_allreduce_expected
    assert torch.cuda.is_available(), "the probe needs a GPU"
    count = n_bytes // 4
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
    owner, _ = sc.owner_map(n, 1, 4, count, sp[0] % 16, (sp[0] - rp[0]) % 16)
    exp_sym = torch.from_numpy(sc.expected(sc.F32, [v.view(np.uint32) for v in x], owner).view(np.int32)).cuda()
    ring_exp = ring_allreduce_expected(x, F32, SUM)
    assert all(np.asarray(e).tobytes() == np.asarray(ring_exp[0]).tobytes() for e in ring_exp)
    exp_ring = torch.from_numpy(np.asarray(ring_exp[0]).view(np.int32).copy()).cuda()
    times, queued, exact = {m: [] for m in MODES}, {m: set() for m in MODES}, {m: True for m in MODES}
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000) as comm:
        for k in range(3 * (WARMUP + calls)):
            mode = MODES[k % 3]
            if mode != "symmetric":
                comm.set_simple_group(mode == "ring_group")
            for r in recv:
                r.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "symmetric":
                comm.all_reduce_symmetric(sp, rp, count, F32, SUM, 1)
            else:
                comm.all_reduce(sp, rp, count, F32, SUM)
            dt = time.perf_counter() - t0
            want = exp_sym if mode == "symmetric" else exp_ring
            exact[mode] = exact[mode] and all(bool(torch.equal(r.view(torch.int32), want)) for r in recv)
            queued[mode].add(comm.queued())
            if k >= 3 * WARMUP:
                times[mode].append(dt * 1e3)
    # the kernel alone: HIP events round nexrSymAllReduce on a stream
    stream = torch.cuda.Stream()
    ev = []
    with torch.cuda.stream(stream):
        for k in range(WARMUP + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            nexr.sym_all_reduce(sp, rp, count, F32, n_blocks=1, stream=stream.cuda_stream)
            b.record(stream)
            stream.synchronize()
            if k >= WARMUP:
                ev.append(a.elapsed_time(b))
    exact["symmetric"] = exact["symmetric"] and all(bool(torch.equal(r.view(torch.int32), exp_sym)) for r in recv)
    row = {"ranks": n, "bytes_per_rank": n_bytes, "gpus_visible": torch.cuda.device_count(),
           "exact": {m: bool(v) for m, v in exact.items()}}
    for m in MODES:
        row[m] = dict(_stats(times[m]), queued=sorted(queued[m]))
    ks = _stats(ev)
    moved = 2 * n * n_bytes
    ks["fraction_of_8TBps"] = round(moved / (ks["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
    row["symmetric_kernel_hip_events"] = ks
    return row


def main():
    calls, out = 20, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped = [], None
    for n in RANKS:
        for n_bytes in SIZES:
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                "--child", str(n), str(n_bytes), str(calls)], capture_output=True, text=True)
            if p.returncode != 0:
                stopped = {"ranks": n, "bytes_per_rank": n_bytes, "returncode": p.returncode, "stderr": p.stderr[-500:]}
                break
            rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("ranks %d, %d bytes per rank: done" % (n, n_bytes), file=sys.stderr, flush=True)
        if stopped:
            break
    res = {"workload": "all-reduce, fp32 sum, SIMPLE communicator, device memory, thread ranks on one GPU",
           "timing": "host clock around each blocking call; the three modes alternately, call by call, in one "
                     "process; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; "
                     "symmetric_kernel_hip_events: HIP events round nexrSymAllReduce alone, "
                     "fraction_of_8TBps = 2 * ranks * bytes_per_rank / median / 8e12" % WARMUP,
           "rows": rows, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    ok = not stopped and all(all(r["exact"].values()) for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]))))
        sys.exit(0)
    sys.exit(main())
