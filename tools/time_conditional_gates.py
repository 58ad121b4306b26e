"""Times conditional gates (A.BatchConditionalGate) on 2^10 trajectories of 20 qubits in ONE complex64 tensor (2^30 elements),
next to the route they replace, measured in the same process: a host loop of 2^10 prebuilt A.ControlledGate calls under
condition=when(selector[b:b+1], ...) on the 2^10 separate 2^20-element tensors that the slices are.

    X correction, about half match    selector[b] = b & 1
    X correction, all match           selector[b] = 1
    X correction, none match          selector[b] = 0: every tile is left before its first access; about a launch
    dense t = 2, one high control     a random 4 x 4 unitary under a control on the top bit of a trajectory, all match

The state is restored from a copy before every call, outside the timed region.  HIP events around the whole call, two warm-up
calls, the median of REPEATS timed calls, one process.  A row LOSES to its comparison when its median exceeds the comparison's
by more than the sum of the two min..max spreads.

    python tools/time_conditional_gates.py [--repeats 5] [--out-dir profiles]

writes conditional_gates_timing.json and conditional_gates_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from time_born import DEV, clocks  # noqa: E402
from time_measure import timed  # noqa: E402

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log2b", type=int, default=10)
    ap.add_argument("--qubits", type=int, default=20)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    reps, lb, nq = args.repeats, args.log2b, args.qubits
    B, n = 2 ** lb, 2 ** (lb + nq)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    backup = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    state = torch.empty_like(backup)
    batched = state.view((B,) + (2,) * nq)                     # dim 0 is the batch, dim 1 + d the qubit on memory bit nq - 1 - d
    single = batched[0]
    restore = lambda: state.copy_(backup)
    rng = np.random.default_rng(2)
    u4, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    selectors = {"about half match": torch.arange(B, dtype=torch.int64, device=DEV) & 1,
                 "all match": torch.ones(B, dtype=torch.int64, device=DEV), "none match": torch.zeros(B, dtype=torch.int64, device=DEV)}
    mid = nq - 1 - nq // 2                                      # the qubit on memory bit nq // 2
    steps = [(f"X correction, {name}", X, [mid], [], sel) for name, sel in selectors.items()]
    steps.append(("dense t = 2, one high control, all match", u4, [mid, nq - 1], [0], selectors["all match"]))
    rows = []

    def add(step, route, fn, kind):
        med, lo, hi = timed(fn, restore, reps)
        rows.append({"step": step, "route": route, "kind": kind, "ms_median": med, "ms_min": lo, "ms_max": hi})
        print(f"{step:44s} {route:52s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]", flush=True)

    for step, u, targets, controls, sel in steps:
        gate = A.BatchConditionalGate(batched.shape, batched.stride(), batched.dtype, {1: u}, [1 + d for d in targets], [0], DEV,
                                      [1 + d for d in controls])
        one = A.ControlledGate(single.shape, single.stride(), single.dtype, u, targets, controls, DEV)
        conds = [A.when(sel[b:b + 1], 1) for b in range(B)]    # (prebuilt: the loop only enqueues)
        add(step, "BatchConditionalGate, one tensor, one launch", lambda: gate(batched, sel), "new")

        def loop():
            for b in range(B):
                one(batched[b], conds[b])
        add(step, f"loop of {B} ControlledGate(condition=when) calls  [comparison]", loop, "comparison")

    verdicts = []
    for r in rows:
        if r["kind"] != "new":
            continue
        c = [c for c in rows if c["kind"] == "comparison" and c["step"] == r["step"]][0]
        spread = (r["ms_max"] - r["ms_min"]) + (c["ms_max"] - c["ms_min"])
        r["comparison_ms_median"], r["loses"] = c["ms_median"], bool(r["ms_median"] > c["ms_median"] + spread)
        verdicts.append(r["loses"])

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_B": lb, "qubits": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing); the state is "
           "restored before every call, outside the timed region", "rows_that_lose": int(sum(verdicts)), "clocks": clocks(),
           "device_memory_free_bytes": free, "device_memory_total_bytes": total, "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "conditional_gates_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "conditional_gates_timing.md"), "w") as f:
        f.write(f"# Conditional gates: 2^{lb} trajectories of {nq} qubits in one complex64 tensor ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process; the state is restored from a "
                f"copy before every call, outside the timed region.  The comparison is a host loop of {B} prebuilt `ControlledGate` calls "
                f"under `condition=when(selector[b:b+1], 1)` on the {B} slices as separate tensors, with the same selector.  A row loses "
                "when its median exceeds the comparison's by more than the sum of the two min..max spreads.  complex128 is not measured.\n\n")
        f.write("| step | route | median ms | min..max ms | comparison ms | loses |\n|---|---|---:|---:|---:|---|\n")
        for r in rows:
            cmp_ms = f"{r['comparison_ms_median']:.3f}" if "comparison_ms_median" in r else ""
            loses = ("yes" if r["loses"] else "no") if "loses" in r else ""
            f.write(f"| {r['step']} | {r['route']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | {cmp_ms} | {loses} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows), "rows_that_lose": int(sum(verdicts))}))


if __name__ == "__main__":
    main()
