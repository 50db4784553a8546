"""The flat tree all-reduce, broadcast and all-gather (nexrTreeAllReduceFlat, nexrRingBroadcastFlat,
nexrRingAllGatherFlat: one launch each, the FIFO collective's bytes) against the FIFO calls of the same
communicator: fp32 sum, thread ranks on one GPU, device memory, 4 MiB per rank (the all-gather: its n-chunk
output), at 2, 4 and 8 ranks, SIMPLE, LL and LL128, a binary tree over single ranks (treeRanksPerNode = 1). Every
(protocol, ranks) runs in a child process of its own under `timeout`; the child alternates, call by call on ONE
communicator: the flat tree, the plain tree host-sequenced, the plain tree under nexrRingCommSetLLGroup (LL and
LL128 only) and nexrRingAllReduceFlat; then the flat broadcast against the FIFO one and the flat all-gather
against the FIFO one. Each call is timed on the host clock (it returns after its device wait) and checked exact
on the device: every tree mode against oracle.ring's tree fold, the flat ring against its ring fold, the copies
against their inputs. Reported per mode: p25, median and p75 of `calls` calls after warm-up. The flat kernels alone
are also timed with HIP events (the nexrFlat* / nexrSymAllGather entries on a stream), with their algorithmic
bytes as a share of 8 TB/s. After a child that faulted, aborted or ran into its limit nothing more is started.
DESIGN §8.8 has the table.
    python tools/flat_tree_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/flat_tree_probe.py --child PROTOCOL RANKS BYTES CALLS"""
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
PROTOCOLS = ("simple", "ll", "ll128")
PROTO_ID = {"simple": 0, "ll": 1, "ll128": 2}
BYTES = 4 << 20   # per rank
WARMUP = 3        # per mode
CHILD_LIMIT_S = 150
F32, SUM = 7, 0
PEAK_BYTES_PER_S = 8e12


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def child(protocol, n, n_bytes, calls):
    import numpy as np
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    ring = importlib.import_module("nex-nccl_amd.ring")
    from oracle import ring as oring
    assert torch.cuda.is_available(), "the probe needs a GPU"
    count = n_bytes // 4
    per = count // n          # the all-gather's sendcount: its output is the same 4 MiB
    root = n - 1
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()

    links = oring.tree_topology(n, 1, 0)
    exp_tree = dev(oring.tree_allreduce_expected(x, F32, SUM, links, protocol)[0])
    # the flat ring must give the FIFO ring's bytes (taken below); the SIMPLE FIFO ring is itself checked against
    # the oracle's default-FIFO ring fold
    exp_ring = dev(oring.ring_allreduce_expected(x, F32, SUM)[0]) if protocol == "simple" else None
    exp_bc = send[root].view(torch.int32)
    exp_ag = torch.cat([t[:per] for t in send]).view(torch.int32)

    def exact(what):
        if what == "tree":
            return all(bool(torch.equal(r.view(torch.int32), exp_tree)) for r in recv)
        if what == "ring":   # the flat ring is checked against the FIFO ring's bytes of the first call
            return all(bool(torch.equal(r, ring_ref)) for r in recv)
        if what == "broadcast":
            return all(bool(torch.equal(r.view(torch.int32), exp_bc)) for r in recv)
        return all(bool(torch.equal(r[:per * n].view(torch.int32), exp_ag)) for r in recv)

    row = {"protocol": protocol, "ranks": n, "bytes_per_rank": n_bytes, "gpus_visible": torch.cuda.device_count()}
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=20000, protocol=PROTO_ID[protocol],
                       tree_ranks_per_node=1) as comm:
        comm.all_reduce(sp, rp, count, F32, SUM)   # the FIFO ring's bytes, which the flat ring must give
        torch.cuda.synchronize()
        ring_ref = recv[0].clone()
        if exp_ring is not None:
            assert bool(torch.equal(ring_ref.view(torch.int32), exp_ring)), "the FIFO ring against the oracle"
        groups = (("all_reduce", ("flat_tree", "tree_host_sequenced") + (("tree_group",) if protocol != "simple" else ())
                   + ("flat_ring",)),
                  ("broadcast", ("flat", "fifo")), ("all_gather", ("flat", "fifo")))
        for coll, modes in groups:
            times, queued, ok = {m: [] for m in modes}, {m: set() for m in modes}, {m: True for m in modes}
            for k in range(len(modes) * (WARMUP + calls)):
                mode = modes[k % len(modes)]
                if protocol != "simple":
                    comm.set_ll_group(mode == "tree_group")
                for r in recv:
                    r.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "flat_tree":
                    comm.tree_all_reduce_flat(sp, rp, count, F32, SUM)
                elif mode.startswith("tree"):
                    comm.tree_all_reduce(sp, rp, count, F32, SUM)
                elif mode == "flat_ring":
                    comm.all_reduce_flat(sp, rp, count, F32, SUM)
                elif coll == "broadcast":
                    (comm.broadcast_flat if mode == "flat" else comm.broadcast)(sp, rp, count, F32, root)
                else:
                    (comm.all_gather_flat if mode == "flat" else comm.all_gather)(sp, rp, per, F32)
                dt = time.perf_counter() - t0
                what = "ring" if mode == "flat_ring" else "tree" if coll == "all_reduce" else coll
                ok[mode] = ok[mode] and exact(what)
                queued[mode].add(comm.queued())
                if k >= len(modes) * WARMUP:
                    times[mode].append(dt * 1e3)
            row[coll] = {m: dict(_stats(times[m]), queued=sorted(queued[m]), exact=bool(ok[m])) for m in modes}
    # the kernels alone: HIP events round the entries on a stream
    stream = torch.cuda.Stream()
    user_first = protocol == "simple"
    launches = {"all_reduce": lambda s: nexr.flat_tree_all_reduce(sp, rp, count, F32, SUM, 0, user_first, [links],
                                                                  [(0, count, 0)], stream=s),
                "broadcast": lambda s: nexr.flat_broadcast(sp[root], rp, n_bytes, stream=s),
                "all_gather": lambda s: nexr.sym_all_gather(sp, rp, per * 4, stream=s)}
    moved = {"all_reduce": 2 * n * n_bytes, "broadcast": (n + 1) * n_bytes, "all_gather": (n + 1) * per * 4 * n}
    checks = {"all_reduce": "tree", "broadcast": "broadcast", "all_gather": "all_gather"}
    with torch.cuda.stream(stream):
        for coll in ("all_reduce", "broadcast", "all_gather"):
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
            ks["exact"] = exact(checks[coll])
            ks["fraction_of_8TBps"] = round(moved[coll] / (ks["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
            row[coll]["flat_kernel_hip_events"] = ks
    return row


def _all_exact(row):
    return all(v["exact"] for coll in ("all_reduce", "broadcast", "all_gather") for v in row[coll].values())


def main():
    calls, out = 30, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped = [], None
    for protocol in PROTOCOLS:
        for n in RANKS:
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                "--child", protocol, str(n), str(BYTES), str(calls)], capture_output=True, text=True)
            if p.returncode != 0:
                stopped = {"protocol": protocol, "ranks": n, "bytes_per_rank": BYTES, "returncode": p.returncode,
                           "stderr": p.stderr[-500:]}
                break
            rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("%s, ranks %d, %d bytes per rank: done" % (protocol, n, BYTES), file=sys.stderr, flush=True)
        if stopped:
            break
    res = {"workload": "tree all-reduce (a binary tree over single ranks), broadcast (root n - 1) and all-gather (the "
                       "n-chunk output is bytes_per_rank), fp32 sum, device memory, thread ranks on one GPU, the "
                       "default FIFO of each protocol",
           "timing": "host clock around each blocking call; a collective's modes alternately, call by call, in one "
                     "process; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; "
                     "flat_kernel_hip_events: HIP events round the nexrFlatTreeAllReduce / nexrFlatBroadcast / "
                     "nexrSymAllGather entry alone, fraction_of_8TBps = (2n | n + 1 | n + 1) * bytes_per_rank / median "
                     "/ 8e12; flat_ring is checked against the same communicator's FIFO ring call" % WARMUP,
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
        print(json.dumps(child(sys.argv[i + 1], int(sys.argv[i + 2]), int(sys.argv[i + 3]), int(sys.argv[i + 4]))))
        sys.exit(0)
    sys.exit(main())
