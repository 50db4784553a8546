"""The pitched all-to-all and the last-dim all-gather in one launch (nexrFlatAllToAll2D, nexrFlatAllGather2D) against
what the parent commit offers for the same result, on one GPU in device memory:
  pitched          the new entry
  flat_permute     (a) nexrFlatAllToAll plus the permuting copies round it, one per rank and side whose layout is rows
                   (torch: out.view(..).copy_(in.view(..).permute(1, 0, 2)), into buffers made once); (b) for the
                   gather nexrSymAllGather plus that copy
  flat_alone       (c) nexrFlatAllToAll alone on the same bytes (not the same result): what the index arithmetic costs
n = 2 / 4 / 8 / 16 ranks; block rows of 256 B, 4 KiB and 64 KiB with R chosen so that a buffer is 64 KiB, 1 MiB or
16 MiB (shapes with fewer than two rows are left out); the three layout pairs and the gather. Every rank count runs in
a child process of its own under `timeout`; the child alternates the modes call by call on one stream, with the
argument arrays built once. A call is timed between HIP events; every call's outputs are zeroed before it and compared
byte for byte with the rule (torch's permute of the inputs; flat_alone with nexrFlatAllToAll's own rule) afterwards.
Reported per mode: p25, median and p75 of `calls` calls after warm-up; the whole set runs twice (`runs`), and `summary`
holds per row the two runs' medians, their spread and the ratios of the baselines to the new entry. After a child
that faulted, aborted or ran into its limit nothing more is started. DESIGN §8.15 has the table.
    python tools/pitched_probe.py [--calls 30] [--out profiles/NAME.json]"""
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.alltoall_probe import _stats  # noqa: E402

RANKS = (2, 4, 8, 16)
SHAPES = ((256, 64 << 10), (256, 1 << 20), (256, 16 << 20), (4 << 10, 1 << 20), (4 << 10, 16 << 20),
          (64 << 10, 16 << 20))  # (bytes per block row, bytes per buffer)
BLOCKS, ROWS = 0, 1
OPS = {"rows_blocks": (ROWS, BLOCKS), "blocks_rows": (BLOCKS, ROWS), "rows_rows": (ROWS, ROWS), "gather": None}
MODES = ("pitched", "flat_permute", "flat_alone")
WARMUP = 3
CHILD_LIMIT_S = 240


def child(n, calls):
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    L = nexr.lib()
    stream = torch.cuda.Stream()
    s = ctypes.c_void_p(stream.cuda_stream)
    gen = torch.Generator().manual_seed(n)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    rows = []
    for B, size in SHAPES:
        R = size // (n * B)
        if R < 2:
            continue
        for op, lay in OPS.items():
            gather = lay is None
            modes = MODES[:2] if gather else MODES
            ins = [torch.randint(0, 256, ((1 if gather else n) * R * B,), dtype=torch.uint8, generator=gen).cuda()
                   for _ in range(n)]
            outs = {m: [torch.zeros(n * R * B, dtype=torch.uint8, device="cuda") for _ in range(n)] for m in modes}
            tmp_in = [torch.zeros_like(t) for t in ins]
            tmp_out = [torch.zeros(n * R * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
            # the rule: x[s][k][r] is block row (k, r) of input s, y[d][s][r] = x[s][d][r]
            if gather:
                y = [torch.stack([t.view(R, B) for t in ins])] * n
            else:
                x = [t.view(n, R, B) if lay[0] == BLOCKS else t.view(R, n, B).permute(1, 0, 2) for t in ins]
                y = [torch.stack([x[src][d] for src in range(n)]) for d in range(n)]
            rows_out = gather or lay[1] == ROWS
            want = {m: [(t.permute(1, 0, 2) if rows_out else t).contiguous().view(-1) for t in y] for m in modes[:2]}
            if not gather:
                flat = [t.view(n, R * B) for t in ins]
                want["flat_alone"] = [torch.cat([flat[src][d] for src in range(n)]) for d in range(n)]
            a_in, a_tmp_in, a_tmp_out = arr(ins), arr(tmp_in), arr(tmp_out)
            a_out = {m: arr(outs[m]) for m in modes}

            def call(mode):
                if mode == "pitched":
                    if gather:
                        return L.nexrFlatAllGather2D(n, a_in, a_out[mode], R, B, 0, s)
                    return L.nexrFlatAllToAll2D(n, a_in, a_out[mode], R, B, lay[0], lay[1], 0, s)
                if mode == "flat_alone":
                    return L.nexrFlatAllToAll(n, a_in, a_out[mode], R * B, 0, s)
                pre = not gather and lay[0] == ROWS
                for k in range(n if pre else 0):
                    tmp_in[k].view(n, R, B).copy_(ins[k].view(R, n, B).permute(1, 0, 2))
                src, dst = (a_tmp_in if pre else a_in), (a_tmp_out if rows_out else a_out[mode])
                rc = L.nexrSymAllGather(n, src, dst, R * B, s) if gather else L.nexrFlatAllToAll(n, src, dst, R * B, 0, s)
                for k in range(n if rows_out else 0):
                    outs[mode][k].view(R, n, B).copy_(tmp_out[k].view(n, R, B).permute(1, 0, 2))
                return rc

            with torch.cuda.stream(stream):
                ev, ok = {m: [] for m in modes}, {m: True for m in modes}
                for k in range(len(modes) * (WARMUP + calls)):
                    mode = modes[k % len(modes)]
                    for t in outs[mode]:
                        t.zero_()
                    stream.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    rc = call(mode)
                    b.record(stream)
                    stream.synchronize()
                    ok[mode] = ok[mode] and rc == 0 and all(torch.equal(p, q) for p, q in zip(outs[mode], want[mode]))
                    if k >= len(modes) * WARMUP:
                        ev[mode].append(a.elapsed_time(b))
            rows.append({"ranks": n, "op": op, "row_bytes": B, "rows": R, "buffer_bytes": n * R * B,
                         "hip_events": {m: dict(_stats(ev[m]), exact=bool(ok[m])) for m in modes}})
    return rows


def _summary(runs):
    """Per row: the medians of both runs, the spread between them, and each baseline over the new entry."""
    out = []
    for first, second in zip(*runs):
        modes = list(first["hip_events"])
        med = {m: [r["hip_events"][m]["median_ms"] for r in (first, second)] for m in modes}
        row = {k: first[k] for k in ("ranks", "op", "row_bytes", "rows", "buffer_bytes")}
        row.update({m + "_ms": med[m] for m in modes})
        row["spread_pct"] = {m: round(100 * abs(med[m][0] - med[m][1]) / min(med[m]), 1) for m in modes}
        for base in modes[1:]:
            row[base + "_over_pitched"] = [round(med[base][k] / med["pitched"][k], 3) for k in (0, 1)]
        out.append(row)
    return out


def main():
    import subprocess
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
    res = {"workload": "n buffers of buffer_bytes = n * rows * row_bytes in device memory on one GPU, exchanged along "
                       "the inner dimension (rows_blocks: the Ulysses forward, blocks_rows: its backward, rows_rows) or "
                       "gathered along the last one (inputs of rows * row_bytes): the new entry (pitched), "
                       "nexrFlatAllToAll / nexrSymAllGather plus the permuting copies (flat_permute), and "
                       "nexrFlatAllToAll alone on the same bytes (flat_alone, another result)",
           "timing": "the modes alternately, call by call, on one stream in one process per rank count; HIP events "
                     "round the call; p25 / median / p75 of `calls` calls per mode after %d warm-up calls each; the "
                     "whole set twice (runs); every call's outputs compared byte for byte with the rule" % WARMUP,
           "runs": runs, "summary": _summary(runs) if not stopped else None, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    exact = all(v["exact"] for run in runs for r in run for v in r["hip_events"].values())
    return 0 if not stopped and exact else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        print(json.dumps(child(int(sys.argv[i + 1]), int(sys.argv[i + 2]))))
        sys.exit(0)
    sys.exit(main())
