"""The all-to-all with a count per pair in one launch (nexrFlatAllToAllv) against what the parent commit offers, on
one GPU in device memory. n = 2 / 4 / 8 / 16 ranks; a mean of 256 B, 4 KiB, 64 KiB and 1 MiB per pair in 4-byte
elements; two count patterns: `uniform` (every pair the mean) and `skew` (seeded, a quarter of the blocks empty, the
others uniform in [1, 8/3 * mean), so the mean per pair stays). Modes, alternated call by call on one stream:
  v_host          nexrFlatAllToAllv with host counts
  v_device        nexrFlatAllToAllv with the counts in device memory: no host read
  group_copies    (a) the non-empty blocks as NEXR_FLAT_GROUP_COPY works in ONE nexrFlatGroup call
  alltoall        (b) nexrFlatAllToAll, uniform pattern only: what the offset prologue and the search cost
  readback_v_host (c) the matrix copied to the host by hipMemcpy behind the stream's work, the stream synchronised,
                  then v_host: what a caller whose counts are born on the GPU needs without device counts
Every rank count runs in a child process of its own under `timeout`. A call is timed between HIP events and on the
host clock from the call to the return of the stream's synchronisation; the outputs of every mode's warm-up calls
are compared byte for byte with the packed rule (torch slices). Reported per mode: p25, median and p75 of `calls`
calls after warm-up; the whole set runs twice (`runs`), and `summary` holds per row what follows from the two runs'
medians: their spread and the ratios of the baselines to the new entry. The file keeps one line per mode. After a
child that faulted, aborted or ran into its limit nothing more is started. DESIGN §8.13 has the table.
    python tools/alltoallv_probe.py [--calls 30] [--out profiles/NAME.json]"""
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANKS = (2, 4, 8, 16)
SIZES = (256, 4 << 10, 64 << 10, 1 << 20)   # mean bytes per pair
PATTERNS = ("uniform", "skew")
MODES = ("v_host", "v_device", "group_copies", "alltoall", "readback_v_host")
ESZ = 4
WARMUP = 3
CHILD_LIMIT_S = 240


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def matrix(n, mean_bytes, pattern):
    mean = mean_bytes // ESZ
    if pattern == "uniform":
        return np.full((n, n), mean, np.uint64)
    rng = np.random.default_rng(n * 1000003 + mean)
    counts = rng.integers(1, max(2, mean * 8 // 3), (n, n)).astype(np.uint64)
    counts[rng.random((n, n)) < 0.25] = 0
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
    for pattern in PATTERNS:
        for B in SIZES:
            counts = matrix(n, B, pattern)
            byts = counts.astype(np.int64) * ESZ
            send_off, recv_off = np.cumsum(byts, axis=1) - byts, np.cumsum(byts, axis=0) - byts
            in_elts, out_elts = [int(v) for v in counts.sum(axis=1)], [int(v) for v in counts.sum(axis=0)]
            modes = [m for m in MODES if m != "alltoall" or pattern == "uniform"]
            ins = [torch.randint(0, 256, (max(e, 1) * ESZ,), dtype=torch.uint8, generator=gen).cuda() for e in in_elts]
            outs = {m: [torch.zeros(max(e, 1) * ESZ, dtype=torch.uint8, device="cuda") for e in out_elts] for m in modes}
            rule = [torch.cat([ins[src][send_off[src, d]:send_off[src, d] + byts[src, d]] for src in range(n)])
                    for d in range(n)]
            arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
            a_in = arr(ins)
            a_out = {m: arr(outs[m]) for m in modes}
            host_counts = (ctypes.c_uint64 * (n * n))(*[int(c) for c in counts.reshape(-1)])
            read_back = (ctypes.c_uint64 * (n * n))()
            dev_counts = torch.from_numpy(counts.reshape(-1).view(np.int64).copy()).cuda()
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            caps_in, caps_out = (ctypes.c_size_t * n)(*in_elts), (ctypes.c_size_t * n)(*out_elts)
            blocks = [(src, d) for d in range(n) for src in range(n) if byts[src, d]]
            works, keep = nexr.flat_group_works(
                [{"coll": nexr.FLAT_GROUP_COPY, "inputs": [ins[src].data_ptr() + int(send_off[src, d])],
                  "outputs": [outs["group_copies"][d].data_ptr() + int(recv_off[src, d])], "n_elts": int(byts[src, d]),
                  "datatype": 0, "dev_red_op": 0, "red_op_arg": 0, "root": 0} for src, d in blocks])
            info = nexr.FlatGroupInfo()

            def v(mode, cnt, residence):
                return L.nexrFlatAllToAllv(n, a_in, a_out[mode], cnt, residence, ESZ, caps_in, caps_out,
                                           ctypes.c_void_p(status.data_ptr()), 0, s)

            def call(mode):
                if mode == "v_host":
                    return v(mode, ctypes.cast(host_counts, ctypes.c_void_p), 1)
                if mode == "v_device":
                    return v(mode, ctypes.c_void_p(dev_counts.data_ptr()), 0)
                if mode == "group_copies":
                    return L.nexrFlatGroup(n, works, len(blocks), 1, 0, None, ctypes.byref(info), s)
                if mode == "alltoall":
                    return L.nexrFlatAllToAll(n, a_in, a_out[mode], B, 0, s)
                stream.synchronize()  # the copy is ordered behind the stream's work, as the router's kernel would be
                rc = hip.hipMemcpy(read_back, ctypes.c_void_p(dev_counts.data_ptr()), n * n * 8, 2)  # DeviceToHost
                return rc or v(mode, ctypes.cast(read_back, ctypes.c_void_p), 1)

            with torch.cuda.stream(stream):
                host, ev, ok = {m: [] for m in modes}, {m: [] for m in modes}, {m: True for m in modes}
                for k in range(len(modes) * (WARMUP + calls)):
                    mode = modes[k % len(modes)]
                    warm = k < len(modes) * WARMUP
                    if warm:
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
                    ok[mode] = ok[mode] and rc == 0
                    if warm:
                        ok[mode] = ok[mode] and all(torch.equal(x[:y.numel()], y) for x, y in zip(outs[mode], rule))
                    else:
                        host[mode].append(dt)
                        ev[mode].append(a.elapsed_time(b))
            del keep
            rows.append({"ranks": n, "pattern": pattern, "mean_bytes_per_pair": B, "bytes_moved": int(2 * byts.sum()),
                         "blocks": len(blocks), "group_launches": info.launches,
                         "group_fill_launches": info.fillLaunches, "exact": {m: bool(ok[m]) for m in modes},
                         "host_clock": {m: _stats(host[m]) for m in modes},
                         "hip_events": {m: _stats(ev[m]) for m in modes}})
    return rows


def _summary(runs):
    """Per row, from the medians of both runs: the spread between them, and each baseline over the new entry."""
    out = []
    for first, second in zip(*runs):
        row = {k: first[k] for k in ("ranks", "pattern", "mean_bytes_per_pair")}
        for clock in ("host_clock", "hip_events"):
            med = {m: [r[clock][m]["median_ms"] for r in (first, second)] for m in first[clock]}
            entry = {"spread_pct": {m: round(100 * abs(med[m][0] - med[m][1]) / max(min(med[m]), 1e-6), 1) for m in med}}
            for base, new in (("group_copies", "v_host"), ("alltoall", "v_host"), ("readback_v_host", "v_device")):
                if base in med:
                    entry["%s_over_%s" % (base, new)] = [round(med[base][k] / max(med[new][k], 1e-6), 3) for k in (0, 1)]
            row[clock] = entry
        out.append(row)
    return out


def _dump(v, depth=0, width=118):
    """JSON with a value on one line where it fits (a mode's figures do), and short neighbours sharing a line."""
    flat = json.dumps(v)
    if not isinstance(v, (dict, list)) or not v or depth + len(flat) <= width:
        return flat
    items = [json.dumps(k) + ": " + _dump(x, depth + 1, width) for k, x in v.items()] if isinstance(v, dict) else \
            [_dump(x, depth + 1, width) for x in v]
    lines = []
    for item in items:
        if lines and "\n" not in item and "\n" not in lines[-1] and depth + len(lines[-1]) + len(item) + 3 <= width:
            lines[-1] += ", " + item
        else:
            lines.append(item)
    pad = " " * (depth + 1)
    body = ",\n".join(pad + line for line in lines)
    return "%s\n%s\n%s%s" % (flat[0], body, " " * depth, flat[-1])


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
    res = {"workload": "all-to-all with a count per pair (4-byte elements, packed) between `ranks` buffers in device "
                       "memory on one GPU; modes and patterns as the module's docstring lists them",
           "timing": "the modes alternately, call by call, on one stream in one process per rank count; HIP events "
                     "round the call, and the host clock from the call to the return of the stream's synchronisation; "
                     "p25 / median / p75 of `calls` calls per mode after %d warm-up calls each, whose outputs are "
                     "compared byte for byte with the packed rule; the whole set twice (runs)" % WARMUP,
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
