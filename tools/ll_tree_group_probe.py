"""C1's payload (fp32 sum, 4 MiB per rank, thread ranks on one GPU, device memory) as a TREE all-reduce, LL
and LL128, at 2, 4 and 8 ranks (tree_ranks_per_node 1) and at 8 ranks with tree_ranks_per_node 2 (one rank
with three children), by how the steps run: option off, host-sequenced (one launch and one host wait a
step, up to 2n - 1 rank threads taking turns), against nexrRingCommSetLLGroup on, the call's 2n - 1
Primitives in group launches on one stream (nexrRingCommGetQueued 3). Every (setting, option) runs in a
child process of its own under `timeout`, twice in alternation so that the spread between two runs of the
same code shows; a child times each call on the host clock (the call returns after its last device wait),
checks every call exact against oracle.ring.tree_allreduce_expected, and reports the median of its calls
after warm-up. LL runs on the default FIFO. LL128 starts on the default too; where the group's grid is not
resident with it (the call then reports 0), the option-on child of the first round steps down BUFFS until
it is, and every other child of that setting runs on the FIFO it found (buff_bytes in each row). After a
child that failed, faulted or ran into its limit nothing more is started. DESIGN §8.3 has the table.
    python tools/ll_tree_group_probe.py [--calls 30] [--out profiles/NAME.json]
    python tools/ll_tree_group_probe.py --child PROTO RANKS PER_NODE ON BUFF CALLS"""
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = ((2, 1), (4, 1), (8, 1), (8, 2))  # (ranks, tree_ranks_per_node)
PROTOS = ("ll", "ll128")
COUNT = 1 << 20  # 4 MiB of fp32 per rank
WARMUP = 3
CHILD_LIMIT_S = 150
# LL128 FIFOs to try, largest first (0: the default, 8 slots of 600 KiB; whole 2 KiB slices a slot)
BUFFS = (0, 8 * 2048 * 75, 8 * 2048 * 32, 8 * 2048 * 8)


def child(proto, n, per_node, on, buff, calls):
    import numpy as np
    import torch
    from oracle.ring import tree_allreduce_expected, tree_topology
    ring = importlib.import_module("nex-nccl_amd.ring")
    assert torch.cuda.is_available(), "the probe needs a GPU"
    rng = np.random.default_rng(n)
    x = [rng.integers(-1000, 1000, COUNT).astype(np.float32) for _ in range(n)]
    expect = [e.tobytes() for e in tree_allreduce_expected(x, 7, 0, tree_topology(n, per_node, 0), proto)]
    send = [torch.from_numpy(v).cuda() for v in x]
    recv = [torch.zeros(COUNT, dtype=torch.float32, device="cuda") for _ in range(n)]
    sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
    protocol = ring.PROTO_LL if proto == "ll" else ring.PROTO_LL128
    want = 3 if on else 0
    # buff < 0: find the largest FIFO of BUFFS with which the call runs as asked (one call each)
    tries = BUFFS if buff < 0 else (buff,)
    for b in tries:
        times, exact, queued = [], True, set()
        with ring.RingComm(n, ring.DEVICE_MEMORY, b, None, protocol=protocol, timeout_ms=10000,
                           tree_ranks_per_node=per_node) as comm:
            if on:
                comm.set_ll_group(True)
            for k in range(WARMUP + calls):
                for r in recv:
                    r.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                comm.tree_all_reduce(sp, rp, COUNT, 7, 0)
                dt = time.perf_counter() - t0
                exact = exact and all(r.cpu().numpy().tobytes() == e for r, e in zip(recv, expect))
                queued.add(comm.queued())
                if queued != {want} and b != tries[-1]:
                    break  # the group did not fit with this FIFO: the next smaller one
                if k >= WARMUP:
                    times.append(dt * 1e3)
        if len(times) == calls:
            break
    times.sort()
    return {"proto": proto, "ranks": n, "per_node": per_node, "on": int(on), "buff_bytes": b,
            "queued": sorted(queued), "exact": bool(exact), "calls": len(times),
            "median_ms": round(statistics.median(times), 4), "min_ms": round(times[0], 4),
            "p25_ms": round(times[len(times) // 4], 4), "p75_ms": round(times[3 * len(times) // 4], 4),
            "gpus_visible": torch.cuda.device_count()}


def main():
    calls, out = 30, None
    args = sys.argv[1:]
    if "--calls" in args:
        calls = max(20, int(args[args.index("--calls") + 1]))
    if "--out" in args:
        out = args[args.index("--out") + 1]
    rows, stopped, buffs = [], None, {}
    for rnd in range(2):
        for proto in PROTOS:
            for n, per_node in SETTINGS:
                # on first in the first round (it finds the FIFO), off first in the second
                for on in ((1, 0) if rnd == 0 else (0, 1)):
                    key = (proto, n, per_node)
                    buff = 0 if proto == "ll" else buffs.get(key, -1)
                    env = dict(os.environ)
                    env.pop("NEXR_TEST_LL_GROUP_RESIDENT", None)
                    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable,
                                        os.path.abspath(__file__), "--child", proto, str(n), str(per_node), str(on),
                                        str(buff), str(calls)], env=env, capture_output=True, text=True)
                    row = None
                    if p.returncode == 0:
                        row = json.loads(p.stdout.strip().splitlines()[-1])
                    if row is None or not row["exact"] or row["queued"] != [3 if on else 0]:
                        stopped = {"proto": proto, "ranks": n, "per_node": per_node, "on": on, "round": rnd,
                                   "returncode": p.returncode, "row": row, "stderr": p.stderr[-500:]}
                        break
                    buffs[key] = row["buff_bytes"]
                    row["round"] = rnd
                    rows.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                if stopped:
                    break
            if stopped:
                break
        if stopped:
            break
    res = {"workload": "tree all-reduce, fp32 sum, 4 MiB per rank, LL and LL128, device memory, thread ranks on one "
                       "GPU; off: host-sequenced steps, on: group launches (nexrRingCommSetLLGroup)",
           "timing": "host clock around each blocking call, median of `calls` after %d warm-up calls" % WARMUP,
           "rows": rows, "stopped": stopped}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        a = sys.argv[i + 1:i + 7]
        print(json.dumps(child(a[0], int(a[1]), int(a[2]), bool(int(a[3])), int(a[4]), int(a[5]))))
        sys.exit(0)
    sys.exit(main())
