"""Times batched trajectory steps (A.BatchChannelOp, A.collapse_batch_) on 2^10 trajectories of 20 qubits in ONE complex64
tensor (2^30 elements), next to the route of the parent commit measured in the same process: a host loop of 2^10 prebuilt
A.ChannelOp / A.measure.collapse_ calls on the 2^10 separate 2^20-element tensors that the slices are, with the same uniforms.

    depolarizing(0.01)        FIXED: about 99 % of the trajectories draw the identity and their tiles are skipped
    amplitude_damping(0.1)    DIAGONAL: the marginal q[B, 2] plus one pass
    a one-qubit measurement   the marginal plus the streaming collapse

each on three target positions (memory bits 0, 10 and 19 of a trajectory).  Then the same non-identity step (bit_flip(1.0): every
tile works) on 2^28 elements cut into trajectories of 2^20 .. 2^6 elements: what a part-filled tile costs.

The state is restored from a copy before every call, outside the timed region.  HIP events around the whole call, two warm-up
calls, the median of REPEATS timed calls, one process.  A row LOSES to its comparison when its median exceeds the comparison's
by more than the sum of the two min..max spreads.

    python tools/time_trajectories.py [--repeats 5] [--out-dir profiles]

writes trajectories_timing.json and trajectories_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from time_born import DEV, clocks  # noqa: E402
from time_measure import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log2b", type=int, default=10)
    ap.add_argument("--qubits", type=int, default=20)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    reps, lb, nq = args.repeats, args.log2b, args.qubits
    B, n = 2 ** lb, 2 ** (lb + args.qubits)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    backup = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    state = torch.empty_like(backup)
    batched = state.view((B,) + (2,) * nq)                     # dim 0 is the batch, dim 1 + d the qubit on memory bit nq - 1 - d
    single = batched[0]
    restore = lambda: state.copy_(backup)
    uniforms = torch.rand(B, dtype=torch.float64, device=DEV, generator=g)
    rows = []

    def add(step, bit, route, fn, kind, note=""):
        med, lo, hi = timed(fn, restore, reps)
        rows.append({"step": step, "memory_bit": bit, "route": route, "kind": kind, "ms_median": med, "ms_min": lo, "ms_max": hi,
                     "note": note})
        print(f"{step:26s} bit {bit:2d}  {route:44s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]  {note}", flush=True)

    for bit in (0, nq // 2, nq - 1):
        dim = nq - 1 - bit
        for name, ch in (("depolarizing(0.01)", A.depolarizing(0.01)), ("amplitude_damping(0.1)", A.amplitude_damping(0.1))):
            op = A.BatchChannelOp(batched.shape, batched.stride(), batched.dtype, ch, [1 + dim], [0], DEV)
            one = A.ChannelOp(single.shape, single.stride(), single.dtype, ch, [dim], DEV)
            restore()
            j, _ = op(batched, uniforms=uniforms)
            idle = float((j == 0).double().mean()) if ch.form == "FIXED" else 0.0
            note = f"{100 * idle:.1f} % of the tiles skipped (identity drawn)" if ch.form == "FIXED" else ""
            add(name, bit, "BatchChannelOp, one tensor", lambda: op(batched, uniforms=uniforms), "new", note)

            def loop():
                for b in range(B):
                    one(batched[b], uniform=uniforms[b:b + 1], device=True)
            add(name, bit, f"loop of {B} ChannelOp calls  [comparison]", loop, "comparison")
        add("measure one qubit", bit, "collapse_batch_, one tensor", lambda: A.collapse_batch_(batched, [1 + dim], [0], uniforms=uniforms), "new")

        def mloop():
            for b in range(B):
                A.measure.collapse_(batched[b], [dim], uniform=uniforms[b:b + 1])
        add("measure one qubit", bit, f"loop of {B} measure.collapse_ calls  [comparison]", mloop, "comparison")

    verdicts = []
    for r in rows:
        if r["kind"] != "new":
            continue
        c = [c for c in rows if c["kind"] == "comparison" and (c["step"], c["memory_bit"]) == (r["step"], r["memory_bit"])][0]
        spread = (r["ms_max"] - r["ms_min"]) + (c["ms_max"] - c["ms_min"])
        r["comparison_ms_median"], r["loses"] = c["ms_median"], bool(r["ms_median"] > c["ms_median"] + spread)
        verdicts.append(r["loses"])

    # part-filled tiles: every tile works (bit_flip(1.0) draws X everywhere), 2^28 elements, the target on memory bit 0
    small, total_bits = [], 28
    flip = A.Channel.mixture([0.0, 1.0], [[[1, 0], [0, 1]], [[0, 1], [1, 0]]])
    part = state[:2 ** total_bits]
    for s in (20, 12, 11, 10, 8, 6):
        view = part.view((2 ** (total_bits - s),) + (2,) * s)
        op = A.BatchChannelOp(view.shape, view.stride(), view.dtype, flip, [s], [0], DEV)
        u = torch.rand(op.B, dtype=torch.float64, device=DEV, generator=g)
        med, lo, hi = timed(lambda: op(view, uniforms=u), restore, reps)
        gbs = 2 * 8 * 2 ** total_bits / med / 1e6
        small.append({"log2_trajectory": s, "log2_B": total_bits - s, "tile_bits": op.tile_bits, "n_tiles": op.n_tiles, "ms_median": med,
                      "ms_min": lo, "ms_max": hi, "GB_per_s": gbs})
        print(f"bit_flip(1.0) on 2^{total_bits - s} trajectories of 2^{s}: tile 2^{op.tile_bits}, {med:.3f} ms [{lo:.3f}, {hi:.3f}], {gbs:.0f} GB/s", flush=True)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_B": lb, "qubits": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing); the state is "
           "restored before every call, outside the timed region", "rows_that_lose": int(sum(verdicts)), "clocks": clocks(),
           "device_memory_free_bytes": free, "device_memory_total_bytes": total, "rows": rows, "part_filled_tiles": small}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "trajectories_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "trajectories_timing.md"), "w") as f:
        f.write(f"# Batched trajectory steps: 2^{lb} trajectories of {nq} qubits in one complex64 tensor ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process; the state is restored from a "
                "copy before every call, outside the timed region.  The comparison is the parent commit's route in the same process: a "
                f"host loop of {B} prebuilt `ChannelOp` (device=True) / `measure.collapse_` calls on the {B} slices as separate tensors, "
                "with the same uniforms.  A row loses when its median exceeds the comparison's by more than the sum of the two min..max "
                "spreads.  complex128 is not measured.\n\n")
        f.write("| step | memory bit | route | median ms | min..max ms | comparison ms | loses | note |\n|---|---:|---|---:|---:|---:|---|---|\n")
        for r in rows:
            cmp_ms = f"{r['comparison_ms_median']:.3f}" if "comparison_ms_median" in r else ""
            loses = ("yes" if r["loses"] else "no") if "loses" in r else ""
            f.write(f"| {r['step']} | {r['memory_bit']} | {r['route']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | {cmp_ms} | "
                    f"{loses} | {r['note']} |\n")
        f.write(f"\n## Part-filled tiles: bit_flip(1.0) (X on every trajectory, no tile skipped) on 2^{total_bits} elements, target on memory bit 0\n\n")
        f.write("| trajectory | B | tile | tiles | median ms | min..max ms | GB/s (read + write) |\n|---|---|---|---:|---:|---:|---:|\n")
        for r in small:
            f.write(f"| 2^{r['log2_trajectory']} | 2^{r['log2_B']} | 2^{r['tile_bits']} | {r['n_tiles']} | {r['ms_median']:.3f} | "
                    f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['GB_per_s']:.0f} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows), "rows_that_lose": int(sum(verdicts))}))


if __name__ == "__main__":
    main()
