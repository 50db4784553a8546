"""The all-to-all in one launch (nexrFlatAllToAll) against the two ways the parent commit could spell it, on one GPU
in device memory: the same blocks as n * n NEXR_FLAT_GROUP_COPY works in ONE nexrFlatGroup call (a table, beyond 8
ranks in fill launches), and n * n device-to-device hipMemcpyAsync on one stream. n = 2 / 4 / 8 / 16 ranks, B = 256 B,
4 KiB, 64 KiB and 1 MiB per pair. Every rank count runs in a child process of its own under `timeout`; the child
alternates the three modes call by call on one stream, with the argument arrays built once (the C calls are timed,
not their Python wrappers). A call is timed on the host clock from the call to the return of the stream's
synchronisation, and between HIP events; every call's outputs are zeroed before it and compared byte for byte
with the grouped copies' output afterwards (which is itself checked once against the index rule). Reported per
mode: p25, median and p75 of `calls` calls after warm-up; the whole set runs twice (`runs`), and `summary` holds per
row the two runs' medians, their spread and the ratios of the baselines to the new entry. After a child that
faulted, aborted or ran into its limit nothing more is started. DESIGN §8.12 has the table.
    python tools/alltoall_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/alltoall_probe.py --child RANKS CALLS [--only BYTES]   (one row: for a kernel trace)"""
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANKS = (2, 4, 8, 16)
SIZES = (256, 4 << 10, 64 << 10, 1 << 20)   # bytes per pair
MODES = ("alltoall", "group_copies", "memcpy")
WARMUP = 3
CHILD_LIMIT_S = 200
D2D = 3  # hipMemcpyDeviceToDevice


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def child(n, calls, only=None):
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    L = nexr.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    stream = torch.cuda.Stream()
    s = ctypes.c_void_p(stream.cuda_stream)
    gen = torch.Generator().manual_seed(n)
    rows = []
    for B in (SIZES if only is None else (only,)):
        row_bytes = n * B
        ins = [torch.randint(0, 256, (row_bytes,), dtype=torch.uint8, generator=gen).cuda() for _ in range(n)]
        outs = {m: [torch.zeros(row_bytes, dtype=torch.uint8, device="cuda") for _ in range(n)] for m in MODES}
        rule = [torch.cat([ins[src][d * B:(d + 1) * B] for src in range(n)]) for d in range(n)]
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        a_in, a_out = arr(ins), arr(outs["alltoall"])
        blocks = [(src, d) for d in range(n) for src in range(n)]
        works, keep = nexr.flat_group_works(
            [{"coll": nexr.FLAT_GROUP_COPY, "inputs": [ins[src].data_ptr() + d * B],
              "outputs": [outs["group_copies"][d].data_ptr() + src * B], "n_elts": B, "datatype": 0, "dev_red_op": 0,
              "red_op_arg": 0, "root": 0} for src, d in blocks])
        info = nexr.FlatGroupInfo()
        copies = [(outs["memcpy"][d].data_ptr() + src * B, ins[src].data_ptr() + d * B) for src, d in blocks]

        def call(mode):
            if mode == "alltoall":
                return L.nexrFlatAllToAll(n, a_in, a_out, B, 0, s)
            if mode == "group_copies":
                return L.nexrFlatGroup(n, works, len(blocks), 1, 0, None, ctypes.byref(info), s)
            for dst, src in copies:
                rc = hip.hipMemcpyAsync(dst, src, B, D2D, s)
                if rc:
                    return rc
            return 0

        with torch.cuda.stream(stream):
            assert call("group_copies") == 0
            stream.synchronize()
            ref = [t.clone() for t in outs["group_copies"]]
            rule_ok = all(torch.equal(a, b) for a, b in zip(ref, rule))
            host, ev, ok = {m: [] for m in MODES}, {m: [] for m in MODES}, {m: True for m in MODES}
            for k in range(len(MODES) * (WARMUP + calls)):
                mode = MODES[k % len(MODES)]
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
                ok[mode] = ok[mode] and rc == 0 and all(torch.equal(x, y) for x, y in zip(outs[mode], ref))
                if k >= len(MODES) * WARMUP:
                    host[mode].append(dt)
                    ev[mode].append(a.elapsed_time(b))
        del keep
        rows.append({"ranks": n, "bytes_per_pair": B, "bytes_moved": 2 * n * n * B, "rule_exact": bool(rule_ok),
                     "group_launches": info.launches, "group_fill_launches": info.fillLaunches,
                     "group_table_bytes": info.tableBytes,
                     "host_clock": {m: dict(_stats(host[m]), exact=bool(ok[m])) for m in MODES},
                     "hip_events": {m: _stats(ev[m]) for m in MODES}})
    return rows


def _summary(runs):
    """Per row: the medians of both runs, the spread between them, and each baseline over the new entry."""
    out = []
    for first, second in zip(*runs):
        row = {"ranks": first["ranks"], "bytes_per_pair": first["bytes_per_pair"]}
        for clock in ("host_clock", "hip_events"):
            med = {m: [r[clock][m]["median_ms"] for r in (first, second)] for m in MODES}
            entry = {m + "_ms": med[m] for m in MODES}
            entry["spread_pct"] = {m: round(100 * abs(med[m][0] - med[m][1]) / min(med[m]), 1) for m in MODES}
            for base in MODES[1:]:
                entry[base + "_over_alltoall"] = [round(med[base][k] / med["alltoall"][k], 3) for k in (0, 1)]
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
    res = {"workload": "all-to-all of bytes_per_pair between every pair of `ranks` buffers in device memory on one GPU: "
                       "nexrFlatAllToAll (alltoall), the same blocks as n * n NEXR_FLAT_GROUP_COPY works in one "
                       "nexrFlatGroup call (group_copies), and n * n hipMemcpyAsync on one stream (memcpy)",
           "timing": "the three modes alternately, call by call, on one stream in one process per rank count; host "
                     "clock from the call to the return of the stream's synchronisation, and HIP events round the "
                     "call; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; the whole set "
                     "twice (runs); every call's outputs compared byte for byte with the grouped copies'" % WARMUP,
           "runs": runs, "summary": _summary(runs) if not stopped else None, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    exact = all(r["rule_exact"] and all(v["exact"] for v in r["host_clock"].values()) for run in runs for r in run)
    return 0 if not stopped and exact else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else None
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]), only)))
        sys.exit(0)
    sys.exit(main())
