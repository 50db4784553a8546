"""The symmetric reduce-scatter and all-gather (nexrRingReduceScatterSymmetric, nexrRingAllGatherSymmetric: one
launch each, peer loads and stores) against the ring's own reduce_scatter and all_gather of the same
communicator: fp32 sum, thread ranks on one GPU, device memory, SIMPLE, at 2, 4 and 8 ranks and 64 KiB, 4 MiB
and 64 MiB per rank (the whole n-chunk buffer: a rank's reduce-scatter input and its all-gather output; a chunk
is that over the ranks). Every configuration runs in a child process of its own under `timeout`; the child
alternates eight modes call by call on ONE communicator:
    sym_reduce_scatter, sym_all_gather          the symmetric calls, out of place;
    ring_reduce_scatter, ring_all_gather        the ring, host-sequenced (nexrRingCommSetSimpleGroup off);
    group_reduce_scatter, group_all_gather      the ring in group launches (on);
    sym_pair                                    reduce_scatter_symmetric into chunk r of the receive buffer, then
                                                all_gather_symmetric in place on it, timed together;
    sym_all_reduce                              all_reduce_symmetric of the same buffer.
Each call is timed on the host clock (it returns after its device wait) and checked exact on the device: the
symmetric reduce-scatter against tests/sym_cases.py's fold from rank r on, the ring's against oracle.ring, the
all-gathers against the inputs in rank order, the all-reduce against the owner-first fold. Reported per mode:
p25, median and p75 of `calls` calls after warm-up. Both kernels alone are also timed with HIP events
(nexrSymReduceScatter / nexrSymAllGather on a stream, median of `calls`), with their algorithmic bytes over
that time as a fraction of 8 TB/s: (n^2 + n) * chunk bytes for the reduce-scatter (n^2 chunks read, n written),
(n + n^2) * chunk bytes for the all-gather out of place (n read, n^2 written; in place n of the n^2 stores are
skipped: the pair's all-gather). After a child that faulted, aborted or ran into its limit nothing more is
started. DESIGN §8.5 has the table.
    python tools/sym_rs_ag_probe.py [--calls 20] [--out profiles/NAME.json]
    python tools/sym_rs_ag_probe.py --child RANKS BYTES CALLS"""
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
SIZES = (64 << 10, 4 << 20, 64 << 20)  # bytes per rank: n chunks
WARMUP = 3                            # per mode
CHILD_LIMIT_S = 240
F32, SUM = 7, 0
MODES = ("sym_reduce_scatter", "sym_all_gather", "ring_reduce_scatter", "ring_all_gather", "group_reduce_scatter",
         "group_all_gather", "sym_pair", "sym_all_reduce")
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
    from oracle.ring import reduce_scatter_expected
    assert torch.cuda.is_available(), "the probe needs a GPU"
    count = n_bytes // 4      # elements per rank
    c = count // n            # elements per chunk
    rng = np.random.default_rng(n)
    x = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    g = [rng.standard_normal(c).astype(np.float32) for _ in range(n)]  # the all-gather's inputs
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()
    send, gin = [dev(v) for v in x], [dev(v) for v in g]
    part = [torch.zeros(c, dtype=torch.int32, device="cuda") for _ in range(n)]
    recv = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    sp, gp, pp, rp = ([t.data_ptr() for t in ts] for ts in (send, gin, part, recv))
    chunk_p = [rp[r] + 4 * r * c for r in range(n)]
    xu = [v.view(np.uint32) for v in x]
    sym_chunks = [sc.fold_from(sc.F32, [u[r * c:(r + 1) * c] for u in xu], r) for r in range(n)]
    exp_sym_rs = [dev(v) for v in sym_chunks]
    exp_ring_rs = [dev(np.asarray(v)) for v in reduce_scatter_expected(x, F32, SUM)]
    exp_ag = dev(np.concatenate(g))
    exp_pair = dev(np.concatenate(sym_chunks))
    owner, _ = sc.owner_map(n, 1, 4, count, sp[0] % 16, (sp[0] - rp[0]) % 16)
    exp_ar = dev(sc.expected(sc.F32, xu, owner))
    same = lambda got, want: all(bool(torch.equal(a, b)) for a, b in zip(got, want))
    times, queued, exact = {m: [] for m in MODES}, {m: set() for m in MODES}, {m: True for m in MODES}
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, timeout_ms=10000) as comm:
        for k in range(len(MODES) * (WARMUP + calls)):
            mode = MODES[k % len(MODES)]
            if mode.startswith(("ring_", "group_")):
                comm.set_simple_group(mode.startswith("group_"))
            for t in part + recv:
                t.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "sym_reduce_scatter":
                comm.reduce_scatter_symmetric(sp, pp, c, F32, SUM)
            elif mode == "sym_all_gather":
                comm.all_gather_symmetric(gp, rp, c, F32)
            elif mode.endswith("_reduce_scatter"):
                comm.reduce_scatter(sp, pp, c, F32, SUM)
            elif mode.endswith("_all_gather"):
                comm.all_gather(gp, rp, c, F32)
            elif mode == "sym_pair":
                comm.reduce_scatter_symmetric(sp, chunk_p, c, F32, SUM)
                comm.all_gather_symmetric(chunk_p, rp, c, F32)
            else:
                comm.all_reduce_symmetric(sp, rp, count, F32, SUM, 1)
            dt = time.perf_counter() - t0
            if mode == "sym_reduce_scatter":
                ok = same(part, exp_sym_rs)
            elif mode.endswith("_reduce_scatter"):
                ok = same(part, exp_ring_rs)
            elif mode.endswith("_all_gather"):
                ok = same(recv, [exp_ag] * n)
            elif mode == "sym_pair":
                ok = same(recv, [exp_pair] * n)
            else:
                ok = same(recv, [exp_ar] * n)
            exact[mode] = exact[mode] and ok
            queued[mode].add(comm.queued())
            if k >= len(MODES) * WARMUP:
                times[mode].append(dt * 1e3)
    # the kernels alone: HIP events round nexrSymReduceScatter / nexrSymAllGather on a stream
    stream = torch.cuda.Stream()
    ev = {"reduce_scatter": [], "all_gather": []}
    with torch.cuda.stream(stream):
        for k in range(WARMUP + calls):
            for what in ev:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                if what == "reduce_scatter":
                    nexr.sym_reduce_scatter(sp, pp, c, F32, stream=stream.cuda_stream)
                else:
                    nexr.sym_all_gather(gp, rp, 4 * c, stream=stream.cuda_stream)
                b.record(stream)
                stream.synchronize()
                if k >= WARMUP:
                    ev[what].append(a.elapsed_time(b))
    exact["sym_reduce_scatter"] = exact["sym_reduce_scatter"] and same(part, exp_sym_rs)
    exact["sym_all_gather"] = exact["sym_all_gather"] and same(recv, [exp_ag] * n)
    row = {"ranks": n, "bytes_per_rank": n_bytes, "chunk_bytes": 4 * c, "gpus_visible": torch.cuda.device_count(),
           "exact": {m: bool(v) for m, v in exact.items()}}
    for m in MODES:
        row[m] = dict(_stats(times[m]), queued=sorted(queued[m]))
    for what, moved in (("reduce_scatter", (n * n + n) * 4 * c), ("all_gather", (n + n * n) * 4 * c)):
        ks = _stats(ev[what])
        ks["algorithmic_bytes"] = moved
        ks["fraction_of_8TBps"] = round(moved / (ks["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
        row["sym_%s_kernel_hip_events" % what] = ks
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
    res = {"workload": "reduce-scatter and all-gather, fp32 sum, SIMPLE communicator, device memory, thread ranks on "
                       "one GPU; bytes_per_rank is the n-chunk buffer",
           "timing": "host clock around each blocking call (sym_pair: two calls); the eight modes alternately, call by "
                     "call, in one process; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; "
                     "sym_*_kernel_hip_events: HIP events round nexrSymReduceScatter / nexrSymAllGather alone, "
                     "fraction_of_8TBps = algorithmic_bytes / median / 8e12 with (n^2 + n) * chunk_bytes for both "
                     "(reduce-scatter: n^2 chunks read, n written; all-gather out of place: n read, n^2 written)"
                     % WARMUP,
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
