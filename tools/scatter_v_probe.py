"""The reduce-scatter and the all-gather with a count per rank in one launch (nexrFlatReduceScatterv,
nexrFlatAllGatherv) against what the parent commit offers, on one GPU in device memory. n = 2 / 4 / 8 / 16 ranks; a
mean of 256 B, 4 KiB, 64 KiB and 1 MiB per piece in float32 (Sum, user input first); two count patterns: `uniform`
(every piece the mean) and `skew` (seeded, a quarter of the pieces empty, the others uniform in [1, 8/3 * mean), so
the mean stays). Modes of either collective, alternated call by call on one stream:
  v_host          the new entry with host counts
  v_device        the new entry with the counts in device memory: no host read
  readback_v_host (a) the counts copied to the host by hipMemcpy behind the stream's work, then v_host: what a
                  caller whose counts are born on the GPU needs without device counts
  group           (b) the parent's best spelling of the same bytes: the non-empty pieces as n NEXR_FLAT_GROUP_REDUCE
                  (root d) or NEXR_FLAT_GROUP_COPY (n destinations) works in ONE nexrFlatGroup call, which is what n
                  reduce / broadcast calls inside comm.group() under nexrRingCommSetFlat become
  even            (c) uniform pattern only: nexrFlatReduceScatter / nexrSymAllGather (nexrRingAllGatherFlat's launch)
                  of the same bytes: what the prologue and the unaligned accesses cost
Every rank count runs in a child process of its own under `timeout`. A call is timed between HIP events and on the
host clock from the call to the return of the stream's synchronisation. Every call, timed ones included, writes into
zeroed outputs and is compared byte for byte with the rule: nexrFlatReduce with root d on piece d, computed once
(tests/test_scatter_v_gpu.py pins it to the CPU oracle), or torch slices for the all-gather. Reported per mode: p25,
median and p75 of `calls` calls after warm-up; the whole set runs twice (`runs`), and `summary` holds per row the two
runs' spread and the ratios of the baselines to the new entry. After a child that faulted, aborted or ran into its
limit nothing more is started. DESIGN §8.14 has the table.
    python tools/scatter_v_probe.py [--calls 30] [--out profiles/NAME.json]"""
import ctypes
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.alltoallv_probe import _dump, _stats  # noqa: E402

RANKS = (2, 4, 8, 16)
SIZES = (256, 4 << 10, 64 << 10, 1 << 20)   # mean bytes per piece
PATTERNS = ("uniform", "skew")
KINDS = ("reduce_scatter", "all_gather")
MODES = ("v_host", "v_device", "readback_v_host", "group", "even")
ESZ, F32, SUM = 4, 7, 0
WARMUP = 3
CHILD_LIMIT_S = 400


def vector(n, mean_bytes, pattern):
    mean = mean_bytes // ESZ
    if pattern == "uniform":
        return np.full(n, mean, np.uint64)
    rng = np.random.default_rng(n * 1000003 + mean)
    counts = rng.integers(1, max(2, mean * 8 // 3), n).astype(np.uint64)
    counts[rng.random(n) < 0.25] = 0
    counts[0] = counts[0] if counts.any() else mean  # never all empty: such a call launches nothing
    return counts


def child(n, calls):
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    L = nexr.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    stream = torch.cuda.Stream()
    s = ctypes.c_void_p(stream.cuda_stream)
    gen = torch.Generator().manual_seed(n)
    rows = []
    for kind in KINDS:
        scatter = kind == "reduce_scatter"
        for pattern in PATTERNS:
            for B in SIZES:
                counts = [int(c) for c in vector(n, B, pattern)]
                off = [sum(counts[:d]) for d in range(n + 1)]
                total = off[n]
                in_elts = [total] * n if scatter else counts
                out_elts = counts if scatter else [total] * n
                modes = [m for m in MODES if m != "even" or pattern == "uniform"]
                ins = [torch.randint(-8, 9, (max(e, 1),), generator=gen).float().cuda() for e in in_elts]
                outs = {m: [torch.zeros(max(e, 1), dtype=torch.float32, device="cuda") for e in out_elts]
                        for m in modes}
                arr = lambda ps: (ctypes.c_void_p * n)(*ps)  # noqa: E731
                a_in = arr([t.data_ptr() for t in ins])
                a_out = {m: arr([t.data_ptr() for t in outs[m]]) for m in modes}
                if scatter:  # the rule: nexrFlatReduce with root d on piece d
                    rule = [torch.zeros(c, dtype=torch.float32, device="cuda") for c in counts]
                    for d, c in enumerate(counts):
                        if c:
                            nexr.flat_reduce([t.data_ptr() + off[d] * ESZ for t in ins], rule[d].data_ptr(), d, c, F32,
                                             SUM, 0, True)
                    torch.cuda.synchronize()
                else:
                    rule = [torch.cat([t[:c] for t, c in zip(ins, counts)])] * n
                host_counts = (ctypes.c_uint64 * n)(*counts)
                read_back = (ctypes.c_uint64 * n)()
                dev_counts = torch.tensor(counts, dtype=torch.int64).cuda()
                status = torch.zeros(1, dtype=torch.int32, device="cuda")
                caps_in, caps_out = (ctypes.c_size_t * n)(*in_elts), (ctypes.c_size_t * n)(*out_elts)
                pieces = [d for d in range(n) if counts[d]]
                g = outs["group"]
                works, keep = nexr.flat_group_works(
                    [{"coll": nexr.FLAT_GROUP_REDUCE, "inputs": [t.data_ptr() + off[d] * ESZ for t in ins],
                      "outputs": [g[d].data_ptr()] * n, "n_elts": counts[d], "datatype": F32, "dev_red_op": SUM,
                      "red_op_arg": 0, "root": d} if scatter else
                     {"coll": nexr.FLAT_GROUP_COPY, "inputs": [ins[d].data_ptr()],
                      "outputs": [t.data_ptr() + off[d] * ESZ for t in g], "n_elts": counts[d] * ESZ} for d in pieces])
                info = nexr.FlatGroupInfo()

                def v(mode, cnt, residence):
                    word = ctypes.c_void_p(status.data_ptr())
                    if scatter:
                        return L.nexrFlatReduceScatterv(n, a_in, a_out[mode], cnt, residence, F32, SUM, 0, 1, caps_in,
                                                        caps_out, word, 0, s)
                    return L.nexrFlatAllGatherv(n, a_in, a_out[mode], cnt, residence, ESZ, caps_in, caps_out, word, 0, s)

                def call(mode):
                    if mode == "v_host":
                        return v(mode, ctypes.cast(host_counts, ctypes.c_void_p), 1)
                    if mode == "v_device":
                        return v(mode, ctypes.c_void_p(dev_counts.data_ptr()), 0)
                    if mode == "group":
                        return L.nexrFlatGroup(n, works, len(pieces), 1, 0, None, ctypes.byref(info), s)
                    if mode == "even" and scatter:
                        return L.nexrFlatReduceScatter(n, a_in, a_out[mode], counts[0], F32, SUM, 0, 1, s)
                    if mode == "even":
                        return L.nexrSymAllGather(n, a_in, a_out[mode], counts[0] * ESZ, s)
                    stream.synchronize()  # the copy is ordered behind the stream's work, as the producer's kernel is
                    rc = hip.hipMemcpy(read_back, ctypes.c_void_p(dev_counts.data_ptr()), n * 8, 2)  # DeviceToHost
                    return rc or v(mode, ctypes.cast(read_back, ctypes.c_void_p), 1)

                with torch.cuda.stream(stream):
                    host, ev, ok = {m: [] for m in modes}, {m: [] for m in modes}, {m: True for m in modes}
                    for k in range(len(modes) * (WARMUP + calls)):
                        mode = modes[k % len(modes)]
                        for t in outs[mode]:
                            t.zero_()
                        stream.synchronize()
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        a.record(stream)
                        rc = call(mode)
                        b.record(stream)
                        stream.synchronize()
                        dt = (time.perf_counter() - t0) * 1e3
                        ok[mode] = ok[mode] and rc == 0 and all(
                            torch.equal(x[:y.numel()].view(torch.int32), y.view(torch.int32))
                            for x, y in zip(outs[mode], rule))
                        if k >= len(modes) * WARMUP:
                            host[mode].append(dt)
                            ev[mode].append(a.elapsed_time(b))
                del keep
                rows.append({"collective": kind, "ranks": n, "pattern": pattern, "mean_bytes_per_piece": B,
                             "total_bytes": total * ESZ, "pieces": len(pieces), "group_launches": info.launches,
                             "group_fill_launches": info.fillLaunches, "exact": {m: bool(ok[m]) for m in modes},
                             "host_clock": {m: _stats(host[m]) for m in modes},
                             "hip_events": {m: _stats(ev[m]) for m in modes}})
    return rows


def _summary(runs):
    """Per row, from the medians of both runs: the spread between them, and each baseline over the new entry."""
    out = []
    for first, second in zip(*runs):
        row = {k: first[k] for k in ("collective", "ranks", "pattern", "mean_bytes_per_piece")}
        for clock in ("host_clock", "hip_events"):
            med = {m: [r[clock][m]["median_ms"] for r in (first, second)] for m in first[clock]}
            entry = {"spread_pct": {m: round(100 * abs(med[m][0] - med[m][1]) / max(min(med[m]), 1e-6), 1) for m in med}}
            for base, new in (("readback_v_host", "v_device"), ("group", "v_host"), ("even", "v_host")):
                if base in med:
                    entry["%s_over_%s" % (base, new)] = [round(med[base][k] / max(med[new][k], 1e-6), 3) for k in (0, 1)]
            row[clock] = entry
        out.append(row)
    return out


def main():
    calls, out = 30, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(30, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    runs, stopped = [[], []], None
    for run in (0, 1):
        for n in RANKS:
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                "--child", str(n), str(calls)], capture_output=True, text=True)
            if p.returncode != 0:
                stopped = {"run": run, "ranks": n, "returncode": p.returncode, "stderr": p.stderr[-500:]}
                break
            runs[run] += json.loads(p.stdout.strip().splitlines()[-1])
            print("run %d, ranks %d: done" % (run, n), file=sys.stderr, flush=True)
        if stopped:
            break
    res = {"workload": "reduce-scatter (float32, Sum) and all-gather with a count per rank (4-byte elements, packed) "
                       "between `ranks` buffers in device memory on one GPU; modes and patterns as the module's "
                       "docstring lists them",
           "timing": "the modes alternately, call by call, on one stream in one process per rank count; HIP events "
                     "round the call, and the host clock from the call to the return of the stream's synchronisation; "
                     "p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; every call writes "
                     "zeroed outputs and is compared byte for byte with the rule; the whole set twice (runs)" % WARMUP,
           "runs": runs, "summary": _summary(runs) if not stopped else None, "stopped": stopped}
    text = _dump(res)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    exact = all(all(r["exact"].values()) for run in runs for r in run)
    print("exact: %s, stopped: %s" % (exact, stopped), file=sys.stderr)
    return 0 if not stopped and exact else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]))))
        sys.exit(0)
    sys.exit(main())
