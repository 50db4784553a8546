"""The symmetric LL collectives (nexrRingAllReduceSymmetricLL, nexrRingReduceScatterSymmetricLL,
nexrRingAllGatherSymmetricLL: one launch each, data through flagged lines in per-rank windows) against their
peer load / store siblings and the ring's own collectives of the same communicator: fp32 sum, thread ranks on
one GPU, device memory, an LL communicator, at 2, 4 and 8 ranks and 1 KiB, 8 KiB, 64 KiB and 256 KiB per rank
(the all-reduce's buffer; for the reduce-scatter and the all-gather the whole n-chunk buffer, a chunk being
that over the ranks). Every configuration runs in a child process of its own under `timeout`; the child
alternates, call by call on ONE communicator, for each of all_reduce, reduce_scatter and all_gather:
    ll1_*, ll4_*, ll16_*    the symmetric LL call with nBlocks = 1, 4, 16;
    sym_*                   its LD / ST sibling (all_reduce_symmetric, reduce_scatter_symmetric, ...);
    group_*                 the ring's own collective in LL group launches (nexrRingCommSetLLGroup on, queued 3);
    ring_*                  the ring's own collective with the option off: host-sequenced (queued 0), or device
                            runs (queued 2) where the communicator's streams allow them; queued() is recorded.
Each call is timed on the host clock (it returns after its device wait) and checked exact on the device
against its own rule: the LL calls against the rank-0-first fp32 fold (tests/sym_ll_cases.py), the siblings
against the owner-first / rank-r-first folds (tests/sym_cases.py), the ring against oracle.ring, the
all-gathers against the inputs in rank order. Reported per mode: p25, median and p75 of `calls` calls after
warm-up. Each symmetric kernel alone is also timed between HIP events (nexrSymLL* / nexrSym* on a stream, median
of `calls`). After a child that faulted, aborted or ran into its limit nothing more is started. DESIGN §8.6
has the table.
    python tools/sym_ll_probe.py [--calls 20] [--out profiles/NAME.json]
    python tools/sym_ll_probe.py --child RANKS BYTES CALLS"""
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
SIZES = (1 << 10, 8 << 10, 64 << 10, 256 << 10)  # bytes per rank
BLOCKS = (1, 4, 16)
COLLS = ("all_reduce", "reduce_scatter", "all_gather")
KINDS = tuple("ll%d" % b for b in BLOCKS) + ("sym", "group", "ring")
MODES = tuple("%s_%s" % (k, c) for c in COLLS for k in KINDS)
WARMUP = 3  # per mode
CHILD_LIMIT_S = 240
F32, SUM = 7, 0
LL_BUFF = 8 * 512 * 8 * 16


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
    import sym_ll_cases as lc
    from oracle.ring import reduce_scatter_expected, ring_allreduce_expected_ll
    assert torch.cuda.is_available(), "the probe needs a GPU"
    count = n_bytes // 4  # elements per rank
    c = count // n        # elements per chunk
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    g = [rng.standard_normal(c).astype(np.float32) for _ in range(n)]  # the all-gather's inputs
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()
    send, gin = [dev(v) for v in x], [dev(v) for v in g]
    part = [torch.zeros(c, dtype=torch.int32, device="cuda") for _ in range(n)]
    recv = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    sp, gp, pp, rp = ([t.data_ptr() for t in ts] for ts in (send, gin, part, recv))
    xu = [v.view(np.uint32) for v in x]
    owner, _ = sc.owner_map(n, 1, 4, count, sp[0] % 16, (sp[0] - rp[0]) % 16)
    want = {
        "ll_all_reduce": [dev(lc.ar_expected(sc.F32, xu))] * n,
        "ll_reduce_scatter": [dev(v) for v in lc.rs_expected(sc.F32, xu, c)],
        "sym_all_reduce": [dev(sc.expected(sc.F32, xu, owner))] * n,
        "sym_reduce_scatter": [dev(sc.fold_from(sc.F32, [u[r * c:(r + 1) * c] for u in xu], r)) for r in range(n)],
        "ring_all_reduce": [dev(np.asarray(v)) for v in ring_allreduce_expected_ll(x, F32, SUM, LL_BUFF)],
        "ring_reduce_scatter": [dev(np.asarray(v)) for v in reduce_scatter_expected(x, F32, SUM, "ll")],
        "all_gather": [dev(np.concatenate(g))] * n,
    }
    same = lambda got, exp: all(bool(torch.equal(a, b)) for a, b in zip(got, exp))

    def verdict(kind, coll):
        if coll == "all_gather":
            return same(recv, want["all_gather"])
        rule = "ll" if kind.startswith("ll") else "sym" if kind == "sym" else "ring"
        return same(recv if coll == "all_reduce" else part, want["%s_%s" % (rule, coll)])

    times, queued, exact = {m: [] for m in MODES}, {m: set() for m in MODES}, {m: True for m in MODES}
    with ring.RingComm(n, ring.DEVICE_MEMORY, LL_BUFF, None, 10000, ring.PROTO_LL) as comm:
        for k in range(len(MODES) * (WARMUP + calls)):
            mode = MODES[k % len(MODES)]
            kind, coll = mode.split("_", 1)
            if kind in ("group", "ring"):
                comm.set_ll_group(kind == "group")
            for t in part + recv:
                t.zero_()
            torch.cuda.synchronize()
            B = int(kind[2:]) if kind.startswith("ll") else 0
            t0 = time.perf_counter()
            if coll == "all_reduce":
                if B:
                    comm.all_reduce_symmetric_ll(sp, rp, count, F32, SUM, B)
                elif kind == "sym":
                    comm.all_reduce_symmetric(sp, rp, count, F32, SUM, 1)
                else:
                    comm.all_reduce(sp, rp, count, F32, SUM)
            elif coll == "reduce_scatter":
                if B:
                    comm.reduce_scatter_symmetric_ll(sp, pp, c, F32, SUM, B)
                elif kind == "sym":
                    comm.reduce_scatter_symmetric(sp, pp, c, F32, SUM)
                else:
                    comm.reduce_scatter(sp, pp, c, F32, SUM)
            else:
                if B:
                    comm.all_gather_symmetric_ll(gp, rp, c, F32, B)
                elif kind == "sym":
                    comm.all_gather_symmetric(gp, rp, c, F32)
                else:
                    comm.all_gather(gp, rp, c, F32)
            dt = time.perf_counter() - t0
            exact[mode] = exact[mode] and verdict(kind, coll)
            queued[mode].add(comm.queued())
            if k >= len(MODES) * WARMUP:
                times[mode].append(dt * 1e3)
    # the kernels alone: HIP events round one nexrSymLL* / nexrSym* call on a stream
    wbytes = nexr.sym_ll_window_bytes(n, max(BLOCKS))
    wins = [torch.zeros(wbytes + 16, dtype=torch.uint8, device="cuda") for _ in range(n)]
    wp = [w.data_ptr() + (-w.data_ptr()) % 16 for w in wins]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    ll = dict(status=status.data_ptr(), timeout_us=5_000_000, stream=h)
    kernels = {}
    for b in BLOCKS:
        kernels["ll%d_all_reduce" % b] = lambda b=b: nexr.sym_ll_all_reduce(sp, rp, count, F32, wp, wbytes, n_blocks=b, **ll)
        kernels["ll%d_reduce_scatter" % b] = lambda b=b: nexr.sym_ll_reduce_scatter(sp, pp, c, F32, wp, wbytes, n_blocks=b, **ll)
        kernels["ll%d_all_gather" % b] = lambda b=b: nexr.sym_ll_all_gather(gp, rp, 4 * c, wp, wbytes, n_blocks=b, **ll)
    kernels["sym_all_reduce"] = lambda: nexr.sym_all_reduce(sp, rp, count, F32, 1, stream=h)
    kernels["sym_reduce_scatter"] = lambda: nexr.sym_reduce_scatter(sp, pp, c, F32, stream=h)
    kernels["sym_all_gather"] = lambda: nexr.sym_all_gather(gp, rp, 4 * c, stream=h)
    ev = {name: [] for name in kernels}
    with torch.cuda.stream(stream):
        for k in range(WARMUP + calls):
            for name, call in kernels.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                stream.synchronize()
                if k >= WARMUP:
                    ev[name].append(a.elapsed_time(b))
                kind, coll = name.split("_", 1)
                exact[name] = exact[name] and verdict(kind, coll)
    row = {"ranks": n, "bytes_per_rank": n_bytes, "chunk_bytes": 4 * c, "gpus_visible": torch.cuda.device_count(),
           "ll_status": int(status.item()), "exact": {m: bool(v) for m, v in exact.items()}}
    for m in MODES:
        row[m] = dict(_stats(times[m]), queued=sorted(queued[m]))
    row["kernel_hip_events"] = {name: _stats(t) for name, t in ev.items()}
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
    res = {"workload": "all-reduce, reduce-scatter and all-gather, fp32 sum, LL communicator, device memory, thread "
                       "ranks on one GPU; bytes_per_rank is the all-reduce's buffer and the n-chunk buffer of the "
                       "other two",
           "timing": "host clock around each blocking call; the %d modes alternately, call by call, in one process; "
                     "p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; kernel_hip_events: HIP "
                     "events round one nexrSymLL* (ll<nBlocks>_*) or nexrSym* (sym_*) call alone on a stream"
                     % (len(MODES), WARMUP),
           "round_packs": 256, "rows": rows, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    ok = not stopped and all(all(r["exact"].values()) and r["ll_status"] == 0 for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]))))
        sys.exit(0)
    sys.exit(main())
