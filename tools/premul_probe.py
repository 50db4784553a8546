"""What a scalar per rank costs the flat all-reduce: the launches with a scalar per rank (nexrFlatAllReducePreMul
beneath nexrRingAllReduceFlat under a user-created PreMulSum op, include/nexr_ring.h) against the existing flat
all-reduce under ncclAvg, which moves the same bytes with ONE factor. fp32, 4 MiB per rank, SIMPLE, device memory,
thread ranks on one GPU, at 2, 4 and 8 ranks. Every configuration runs in a child process of its own under
`timeout`, and the whole set runs `--runs` times (2: the yardstick kernel's own spread between two runs is what a
difference is read against). The child alternates, call by call on ONE communicator:
    premul_immediate     nexrRingAllReduceFlat, a user op with n distinct host-immediate scalars
    premul_device        the same with the scalars in a device buffer (the kernel reads them)
    avg_flat             nexrRingAllReduceFlat under ncclAvg: the existing PreMulSum kernel, the yardstick
    ring_host_sequenced  nexrRingAllReduce with the user op, every option off
Each call is timed on the host clock (it returns after its device wait) and checked exact on the device against
tests/premul_cases.py's expected bytes (ncclAvg: oracle.ring's). Reported per mode: p25, median and p75 of `calls`
calls after warm-up. The three kernels alone are also timed with HIP events (the nexrFlat* entries on a stream).
After a child that faulted, aborted or ran into its limit nothing more is started. DESIGN §8.10 has the table.
    python tools/premul_probe.py [--calls 30] [--runs 2] [--out profiles/NAME.json]
    python tools/premul_probe.py --child RANKS BYTES CALLS"""
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
BYTES = 4 << 20   # per rank
WARMUP = 3        # per mode
CHILD_LIMIT_S = 150
F32, SUM, AVG, PREMULSUM = 7, 0, 4, 3
MODES = ("premul_immediate", "premul_device", "avg_flat", "ring_host_sequenced")
KERNELS = ("premul_immediate", "premul_device", "avg_flat")
PEAK_BYTES_PER_S = 8e12


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def child(n, n_bytes, calls):
    import numpy as np
    import torch
    import oracle
    import premul_cases as pc
    from oracle import ring as oring
    nexr = importlib.import_module("nex-nccl_amd")
    ring = importlib.import_module("nex-nccl_amd.ring")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    count = n_bytes // 4
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
    bits = pc.scalar_bits(F32, n)
    scalars = torch.from_numpy(pc.scalar_array(F32, bits).view(np.int32).copy()).cuda()
    addrs = [scalars.data_ptr() + 4 * r for r in range(n)]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()

    pre = [oracle.reduce_copy([v], 1, F32, PREMULSUM, s, [s], False)[0] for v, s in zip(x, bits)]
    exp_user = dev(oring.ring_allreduce_expected(pre, F32, SUM)[0])
    exp_avg = dev(oring.ring_allreduce_expected(x, F32, AVG)[0])

    def exact(mode):
        want = exp_avg if mode == "avg_flat" else exp_user
        return all(bool(torch.equal(r.view(torch.int32), want)) for r in recv)

    row = {"ranks": n, "bytes_per_rank": n_bytes, "gpus_visible": torch.cuda.device_count()}
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000) as comm:
        h_imm = comm.create_premul_sum(list(pc.scalar_array(F32, bits)), F32, ring.SCALAR_HOST_IMMEDIATE)
        h_dev = comm.create_premul_sum(addrs, F32, ring.SCALAR_DEVICE)
        times, queued, ok = {m: [] for m in MODES}, {m: set() for m in MODES}, {m: True for m in MODES}
        for k in range(len(MODES) * (WARMUP + calls)):
            mode = MODES[k % len(MODES)]
            for r in recv:
                r.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "premul_immediate":
                comm.all_reduce_flat(sp, rp, count, F32, h_imm)
            elif mode == "premul_device":
                comm.all_reduce_flat(sp, rp, count, F32, h_dev)
            elif mode == "avg_flat":
                comm.all_reduce_flat(sp, rp, count, F32, AVG)
            else:
                comm.all_reduce(sp, rp, count, F32, h_imm)
            dt = time.perf_counter() - t0
            ok[mode] = ok[mode] and exact(mode)
            queued[mode].add(comm.queued())
            if k >= len(MODES) * WARMUP:
                times[mode].append(dt * 1e3)
        row["host_clock"] = {m: dict(_stats(times[m]), queued=sorted(queued[m]), exact=bool(ok[m])) for m in MODES}
    # the kernels alone: HIP events round the nexrFlat* entries on a stream, alternately
    parts = [(0, count, (4 << 20) // 8 * 4 // 512 * 512 // 4)]   # one channel, the default FIFO's SIMPLE ring chunk
    _op, one_over_n = oracle.host_to_dev_red_op(AVG, F32, n)
    stream = torch.cuda.Stream()
    launches = {
        "premul_immediate": lambda s: nexr.flat_all_reduce_premul(sp, rp, count, F32, bits, False, True, parts, stream=s),
        "premul_device": lambda s: nexr.flat_all_reduce_premul(sp, rp, count, F32, addrs, True, True, parts, stream=s),
        "avg_flat": lambda s: nexr.flat_all_reduce(sp, rp, count, F32, PREMULSUM, one_over_n, True, parts, stream=s)}
    ev, kok = {m: [] for m in KERNELS}, {m: True for m in KERNELS}
    with torch.cuda.stream(stream):
        for k in range(len(KERNELS) * (WARMUP + calls)):
            mode = KERNELS[k % len(KERNELS)]
            for r in recv:
                r.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            launches[mode](stream.cuda_stream)
            b.record(stream)
            stream.synchronize()
            kok[mode] = kok[mode] and exact(mode)
            if k >= len(KERNELS) * WARMUP:
                ev[mode].append(a.elapsed_time(b))
    row["kernel_hip_events"] = {}
    for m in KERNELS:
        ks = _stats(ev[m])
        ks["exact"] = bool(kok[m])
        ks["fraction_of_8TBps"] = round(2 * n * n_bytes / (ks["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
        row["kernel_hip_events"][m] = ks
    return row


def _all_exact(row):
    return all(v["exact"] for part in ("host_clock", "kernel_hip_events") for v in row[part].values())


def main():
    calls, runs, out = 30, 2, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--runs" in args:
        runs = max(1, int(args[args.index("--runs") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped = [], None
    for run in range(runs):
        for n in RANKS:
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                "--child", str(n), str(BYTES), str(calls)], capture_output=True, text=True)
            if p.returncode != 0:
                stopped = {"run": run, "ranks": n, "bytes_per_rank": BYTES, "returncode": p.returncode,
                           "stderr": p.stderr[-500:]}
                break
            rows.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), run=run))
            print("run %d, ranks %d, %d bytes per rank: done" % (run, n, BYTES), file=sys.stderr, flush=True)
        if stopped:
            break
    res = {"workload": "ring all-reduce, fp32, SIMPLE communicator, device memory, thread ranks on one GPU: a "
                       "user-created PreMulSum op with n distinct scalars (host-immediate, device-resident) through "
                       "the launches with a scalar per rank, against ncclAvg through the existing flat launch",
           "timing": "host clock around each blocking call; the modes alternately, call by call, in one process; "
                     "p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; kernel_hip_events: "
                     "HIP events round the nexrFlat* entry alone, the three alternately; fraction_of_8TBps = "
                     "2n * bytes_per_rank / median / 8e12; every configuration `runs` times" % WARMUP,
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
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]))))
        sys.exit(0)
    sys.exit(main())
