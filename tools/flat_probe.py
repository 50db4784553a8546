"""The flat collectives (nexrRingAllReduceFlat, nexrRingReduceScatterFlat, nexrRingReduceFlat: the ring's chain in
one launch, the ring's bytes) against the ring collectives of the same communicator: fp32 sum, thread ranks on one
GPU, device memory, SIMPLE, 4 MiB per rank (the reduce-scatter: its n-chunk input), at 2, 4 and 8 ranks. Every
configuration runs in a child process of its own under `timeout`; the child alternates, call by call on ONE
communicator, per collective: the flat call, the plain host-sequenced ring call (nexrRingCommSetSimpleGroup off)
and the ring in SIMPLE group launches (on); for the all-reduce also nexrRingAllReduceSymmetric. Each call is timed on
the host clock (it returns after its device wait) and checked exact on the device: the flat and the ring calls
against oracle.ring's fold (one expected buffer: they must agree byte for byte), the symmetric call against
tests/sym_cases.py's owner-first fp32 fold. Reported per mode: p25, median and p75 of `calls` calls after warm-up.
The flat kernels alone are also timed with HIP events (the nexrFlat* entries on a stream). After a child that
faulted, aborted or ran into its limit nothing more is started. DESIGN §8.7 has the table.
    python tools/flat_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/flat_probe.py --child RANKS BYTES CALLS"""
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
F32, SUM = 7, 0
COLLECTIVES = ("all_reduce", "reduce_scatter", "reduce")
MODES = {"all_reduce": ("flat", "ring_host_sequenced", "ring_group", "symmetric"),
         "reduce_scatter": ("flat", "ring_host_sequenced", "ring_group"),
         "reduce": ("flat", "ring_host_sequenced", "ring_group")}
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
    from oracle import ring as oring
    assert torch.cuda.is_available(), "the probe needs a GPU"
    count = n_bytes // 4
    per = count // n          # the reduce-scatter's recvcount: its input is the same 4 MiB
    root = n - 1
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()

    owner, _ = sc.owner_map(n, 1, 4, count, sp[0] % 16, (sp[0] - rp[0]) % 16)
    exp_sym = dev(sc.expected(sc.F32, [v.view(np.uint32) for v in x], owner))
    exp_ar = dev(oring.ring_allreduce_expected(x, F32, SUM)[0])
    exp_rs = [dev(e) for e in oring.reduce_scatter_expected(x, F32, SUM)]
    exp_rd = dev(oring.reduce_expected(x, F32, SUM, root))

    def exact(coll, mode):
        if coll == "all_reduce":
            want = exp_sym if mode == "symmetric" else exp_ar
            return all(bool(torch.equal(r.view(torch.int32), want)) for r in recv)
        if coll == "reduce_scatter":
            return all(bool(torch.equal(recv[r][:per].view(torch.int32), exp_rs[r])) for r in range(n))
        return bool(torch.equal(recv[root].view(torch.int32), exp_rd))

    row = {"ranks": n, "bytes_per_rank": n_bytes, "gpus_visible": torch.cuda.device_count()}
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000) as comm:
        for coll in COLLECTIVES:
            modes = MODES[coll]
            times, queued, ok = {m: [] for m in modes}, {m: set() for m in modes}, {m: True for m in modes}
            for k in range(len(modes) * (WARMUP + calls)):
                mode = modes[k % len(modes)]
                if mode.startswith("ring"):
                    comm.set_simple_group(mode == "ring_group")
                for r in recv:
                    r.zero_()
                torch.cuda.synchronize()
                flat = mode == "flat"
                t0 = time.perf_counter()
                if mode == "symmetric":
                    comm.all_reduce_symmetric(sp, rp, count, F32, SUM, 1)
                elif coll == "all_reduce":
                    (comm.all_reduce_flat if flat else comm.all_reduce)(sp, rp, count, F32, SUM)
                elif coll == "reduce_scatter":
                    (comm.reduce_scatter_flat if flat else comm.reduce_scatter)(sp, rp, per, F32, SUM)
                else:
                    (comm.reduce_flat if flat else comm.reduce)(sp, rp, count, F32, SUM, root)
                dt = time.perf_counter() - t0
                ok[mode] = ok[mode] and exact(coll, mode)
                queued[mode].add(comm.queued())
                if k >= len(modes) * WARMUP:
                    times[mode].append(dt * 1e3)
            row[coll] = {m: dict(_stats(times[m]), queued=sorted(queued[m]), exact=bool(ok[m])) for m in modes}
    # the kernels alone: HIP events round the nexrFlat* entries on a stream
    parts = [(0, count, (4 << 20) // 8 * 4 // 512 * 512 // 4)]   # one channel, the default FIFO's SIMPLE ring chunk
    stream = torch.cuda.Stream()
    launches = {"all_reduce": lambda s: nexr.flat_all_reduce(sp, rp, count, F32, SUM, 0, True, parts, stream=s),
                "reduce_scatter": lambda s: nexr.flat_reduce_scatter(sp, rp, per, F32, SUM, 0, True, stream=s),
                "reduce": lambda s: nexr.flat_reduce(sp, rp[root], root, count, F32, SUM, 0, True, stream=s)}
    moved = {"all_reduce": 2 * n * n_bytes, "reduce_scatter": (n + 1) * n_bytes, "reduce": (n + 1) * n_bytes}
    with torch.cuda.stream(stream):
        for coll in COLLECTIVES:
            ev = []
            for r in recv:
                r.zero_()
            for k in range(WARMUP + calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                launches[coll](stream.cuda_stream)
                b.record(stream)
                stream.synchronize()
                if k >= WARMUP:
                    ev.append(a.elapsed_time(b))
            ks = _stats(ev)
            ks["exact"] = exact(coll, "flat")
            ks["fraction_of_8TBps"] = round(moved[coll] / (ks["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
            row[coll]["flat_kernel_hip_events"] = ks
    return row


def _all_exact(row):
    return all(v["exact"] for coll in COLLECTIVES for v in row[coll].values())


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
                            "--child", str(n), str(BYTES), str(calls)], capture_output=True, text=True)
        if p.returncode != 0:
            stopped = {"ranks": n, "bytes_per_rank": BYTES, "returncode": p.returncode, "stderr": p.stderr[-500:]}
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print("ranks %d, %d bytes per rank: done" % (n, BYTES), file=sys.stderr, flush=True)
    res = {"workload": "ring all-reduce, reduce-scatter (the n-chunk input is bytes_per_rank) and reduce (root n - 1), "
                       "fp32 sum, SIMPLE communicator, device memory, thread ranks on one GPU",
           "timing": "host clock around each blocking call; a collective's modes alternately, call by call, in one "
                     "process; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; "
                     "flat_kernel_hip_events: HIP events round the nexrFlat* entry alone, fraction_of_8TBps = "
                     "(2n | n + 1 | n + 1) * bytes_per_rank / median / 8e12" % WARMUP,
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
