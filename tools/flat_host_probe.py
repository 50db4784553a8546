"""The flat collectives on a HOST-memory communicator (nexrRingCommSetFlat on thread ranks in host memory: one
nexrFlatHost* launch that reads and writes pinned user buffers in place over the link, pageable ones staged)
against the host-sequenced FIFO call of the SAME communicator in the SAME run: fp32 sum, SIMPLE, the default FIFOs,
C1's payload of 4 MiB per rank (the reduce-scatter: its n-chunk input) at 2, 4 and 8 ranks; the ring all-reduce, the
tree all-reduce, the reduce-scatter and the broadcast; user buffers of four kinds:

  registered  numpy arrays, each registered on its own with nexrHostRegister (as bench.py's host_registered leg)
  alloc       one nexrHostMemAlloc allocation per buffer
  pinned      torch pin_memory() tensors, unknown to the library
  pageable    numpy arrays

Every row runs in a child process of its own under a time limit; the child alternates flat and plain calls on ONE
communicator, times each on the host clock (either returns with its outputs complete), and compares every call's
outputs byte for byte with the first plain call's. Reported per mode: p25, median and p75 of `calls` calls after
warm-up. Two sweeps ride along at 2 ranks, ring all-reduce: the grid cap (NEXR_HOST_GRID = 8 .. 128 and 0, the
one-shot grid) on registered buffers, and the window chunk (NEXR_FLAT_HOST_CHUNK_BYTES = 1 .. 32 MiB) on pageable
ones, and again for the pageable rows that pipeline (ring and tree all-reduce, broadcast) at 64 MiB per rank with
chunks of 4 .. 64 MiB (16 windows .. one); both knobs are read once per process, so every point is a child. After a child that faulted, aborted or ran
into its limit nothing more is started. DESIGN §8.9 has the table.
    python tools/flat_host_probe.py [--calls 30] [--ranks 2,4,8] [--no-sweeps | --large-chunk-sweep-only]
                                    [--out profiles/NAME.json]
    python tools/flat_host_probe.py --child RANKS KIND CALLS"""
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

RANKS = (2, 4, 8)
KINDS = ("registered", "alloc", "pinned", "pageable")
COLLECTIVES = ("all_reduce", "tree", "reduce_scatter", "broadcast")
BYTES = 4 << 20   # per rank
WARMUP = 3
CHILD_LIMIT_S = 120
F32, SUM = 7, 0
GRIDS = (8, 16, 32, 64, 128, 0)
CHUNKS_MIB = (1, 2, 4, 8, 16, 32)
LARGE_BYTES = 64 << 20                      # per rank: twice the default chunk
LARGE_CHUNKS_MIB = (4, 8, 16, 32, 64)       # 16, 8, 4, 2 windows and one
WINDOWED = ("all_reduce", "tree", "broadcast")


def _stats(t):
    t = sorted(t)
    return {"calls": len(t), "p25_ms": round(t[len(t) // 4], 4), "median_ms": round(statistics.median(t), 4),
            "p75_ms": round(t[3 * len(t) // 4], 4), "min_ms": round(t[0], 4)}


def child(n, kind, calls, collectives=COLLECTIVES, n_bytes=BYTES):
    import numpy as np
    import torch
    nexr = importlib.import_module("nex-nccl_amd")
    ring = importlib.import_module("nex-nccl_amd.ring")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    torch.cuda.init()
    count = n_bytes // 4
    keep, handles, allocs = [], [], []

    def buffer(values):
        """A float32 buffer of the kind holding `values`: (address, numpy view)."""
        if kind == "alloc":
            addr = nexr.host_mem_alloc(values.nbytes)
            allocs.append(addr)
            view = np.ctypeslib.as_array((ctypes.c_float * values.size).from_address(addr))
        elif kind == "pinned":
            t = torch.empty(values.size, dtype=torch.float32).pin_memory()
            keep.append(t)
            view = t.numpy()
        else:
            view = np.empty(values.size, np.float32)
            if kind == "registered":
                handles.append(nexr.host_register(view.ctypes.data, view.nbytes))
        view[:] = values
        keep.append(view)
        return view.ctypes.data, view

    rng = np.random.default_rng(n)
    x = [rng.integers(-1000, 1000, count).astype(np.float32) for _ in range(n)]
    send = [buffer(v) for v in x]
    recv = [buffer(np.zeros(count, np.float32)) for _ in range(n)]
    sp, rp = [a for a, _ in send], [a for a, _ in recv]
    per = count // n
    out = {"ranks": n, "kind": kind, "bytes_per_rank": n_bytes, "rows": {}}
    try:
        with ring.RingComm(n, ring.HOST_MEMORY, 0, None, protocol=ring.PROTO_SIMPLE, timeout_ms=20000,
                           tree_ranks_per_node=1 if n % 2 else 2) as comm:
            for coll in collectives:
                def call():
                    if coll == "all_reduce":
                        comm.all_reduce(sp, rp, count, F32, SUM)
                    elif coll == "tree":
                        comm.tree_all_reduce(sp, rp, count, F32, SUM)
                    elif coll == "reduce_scatter":
                        comm.reduce_scatter(sp, rp, per, F32, SUM)
                    else:
                        comm.broadcast(sp, rp, count, F32, n - 1)

                def outputs():
                    m = per if coll == "reduce_scatter" else count
                    return [v[:m].copy() for _, v in recv]

                def clear():
                    for _, v in recv:
                        v[:] = 0

                times = {"flat": [], "plain": []}
                want = None
                for it in range(WARMUP + calls):
                    for mode in ("plain", "flat"):
                        on = mode == "flat"
                        comm.set_flat(on, tree=on, copies=on)
                        clear()
                        if on:
                            nexr.flat_host_stats(reset=True)
                        before = comm.queued()
                        t0 = time.perf_counter()
                        call()
                        dt = (time.perf_counter() - t0) * 1e3
                        # 4 after a routed call, 0 after a plain ring call; a plain SIMPLE tree call does not
                        # report, so the previous call's report stays
                        report = 4 if on else before if coll == "tree" else 0
                        assert comm.queued() == report, (coll, mode, before, comm.queued())
                        got = outputs()
                        if want is None:
                            want = got
                        for a, b in zip(got, want):   # every call, byte for byte
                            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (coll, mode, it)
                        if it >= WARMUP:
                            times[mode].append(dt)
                st = nexr.flat_host_stats()
                row = {m: _stats(t) for m, t in times.items()}
                row["speedup_median"] = round(row["plain"]["median_ms"] / row["flat"]["median_ms"], 3)
                row["last_flat_call"] = st
                out["rows"][coll] = row
    finally:
        for h in handles:
            nexr.host_deregister(h)
        keep.clear()
        for a in allocs:
            nexr.host_mem_free(a)
    print("FLAT-HOST-PROBE " + json.dumps(out))


def run_child(n, kind, calls, env=None, collectives=None, n_bytes=BYTES):
    """One row in a process of its own. Returns (result or None, exit status)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), kind, str(calls),
           ",".join(collectives or COLLECTIVES), str(n_bytes)]
    try:
        p = subprocess.run(cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        return None, 124
    for line in p.stdout.splitlines():
        if line.startswith("FLAT-HOST-PROBE "):
            return json.loads(line[len("FLAT-HOST-PROBE "):]), p.returncode
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    return None, p.returncode


def main(argv):
    if argv[:1] == ["--child"]:
        colls = tuple(argv[4].split(",")) if len(argv) > 4 else COLLECTIVES
        child(int(argv[1]), argv[2], int(argv[3]), colls, int(argv[5]) if len(argv) > 5 else BYTES)
        return 0
    calls, out_path, ranks, sweeps, large_only = 30, None, RANKS, True, False
    for i, a in enumerate(argv):
        if a == "--calls":
            calls = int(argv[i + 1])
        elif a == "--out":
            out_path = argv[i + 1]
        elif a == "--ranks":
            ranks = tuple(int(v) for v in argv[i + 1].split(","))
        elif a == "--no-sweeps":
            sweeps = False
        elif a == "--large-chunk-sweep-only":
            large_only, sweeps = True, False
    result = {"tool": "tools/flat_host_probe.py", "calls": calls, "rows": [], "grid_sweep": [], "chunk_sweep": [],
              "chunk_sweep_large": []}

    def finish(status):
        result["status"] = status
        text = json.dumps(result, indent=1)
        if out_path:
            with open(out_path, "w") as f:
                f.write(text + "\n")
        print(text)
        return 0 if status == "ok" else 1

    for n in () if large_only else ranks:
        for kind in KINDS:
            res, rc = run_child(n, kind, calls)
            if res is None:   # nothing more is started after a child that failed
                return finish("child %d %s ended with %d" % (n, kind, rc))
            result["rows"].append(res)
            print("%d ranks %-10s " % (n, kind) + "  ".join(
                "%s %.3f/%.3f ms" % (c, r["flat"]["median_ms"], r["plain"]["median_ms"]) for c, r in res["rows"].items()),
                file=sys.stderr)
    if sweeps:
        for g in GRIDS:
            res, rc = run_child(2, "registered", calls, {"NEXR_HOST_GRID": str(g)}, ("all_reduce",))
            if res is None:
                return finish("grid child %d ended with %d" % (g, rc))
            result["grid_sweep"].append({"NEXR_HOST_GRID": g, **res["rows"]["all_reduce"]})
        for mib in CHUNKS_MIB:
            res, rc = run_child(2, "pageable", calls, {"NEXR_FLAT_HOST_CHUNK_BYTES": str(mib << 20)}, ("all_reduce",))
            if res is None:
                return finish("chunk child %d MiB ended with %d" % (mib, rc))
            result["chunk_sweep"].append({"chunk_mib": mib, **res["rows"]["all_reduce"]})
    if sweeps or large_only:   # the pageable rows that pipeline, at a payload beyond the default chunk
        for mib in LARGE_CHUNKS_MIB:
            res, rc = run_child(2, "pageable", calls, {"NEXR_FLAT_HOST_CHUNK_BYTES": str(mib << 20)}, WINDOWED,
                                LARGE_BYTES)
            if res is None:
                return finish("large chunk child %d MiB ended with %d" % (mib, rc))
            result["chunk_sweep_large"].append({"chunk_mib": mib, "bytes_per_rank": LARGE_BYTES, **res["rows"]})
    return finish("ok")


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
