"""Times the two-state circuits (A.PauliPairCircuit: one launch per run and a finish launch) and A.adjoint_gradient on complex64
tensors of 2^30 random elements, next to the route that exists without them, timed in the same process: per step A.pauli_apply
into a third buffer, A.overlap, and two A.pauli_evolve_ (eight passes over a state-sized vector, three buffers).  HIP events
around the whole call, two warm-up calls, the median of REPEATS timed calls.

    python tools/time_adjoint.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes adjoint_timing.json and adjoint_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from time_born import DEV, clocks, timed  # noqa: E402


def ising(nq, j=-1.0, h=-0.7):
    return [(j, {a: "Z", a + 1: "Z"}) for a in range(nq - 1)] + [(h, {d: "X"}) for d in range(nq)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    nq, reps = args.log2n, args.repeats
    n = 2 ** nq
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    mk = lambda: torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2)).view((2,) * nq)
    lam, phi, third = mk(), mk(), mk()                        # dim d is memory bit nq - 1 - d
    state_bytes = n * 8
    rows = []

    def add(name, route, steps, runs, med, lo, hi, max_rank=None):    # (every row: `reps` timed calls after 2 warm-ups)
        passes = 4 * runs if route == "pair" else 8 * steps if route == "separate" else None
        rows.append({"name": name, "route": route, "steps": steps, "max_rank": max_rank, "runs": runs, "passes": passes,
                     "repeats": reps, "warmup": 2, "ms_median": med, "ms_min": lo, "ms_max": hi,
                     "nominal_tbs": None if passes is None else passes * state_bytes / med / 1e9})
        print(rows[-1], flush=True)

    def separate(steps):
        """The route without the two-state kernel: P phi, <lam|P phi>, then the step on each state."""
        def fn():
            for step in steps:
                A.pauli_apply(phi, step[-1], out=third)
                A.overlap(lam, third)
                A.pauli_evolve_(phi, [step])
                A.pauli_evolve_(lam, [step])
        return fn

    def pair(steps, max_rank=None):
        circ = A.PauliPairCircuit(phi.shape, phi.stride(), phi.dtype, steps, DEV, None, max_rank)
        return circ, (lambda: circ(lam, phi, device=True))

    bit = lambda b: nq - 1 - b
    for name, string in (("diagonal", {bit(0): "Z", bit(nq - 1): "Z"}), ("in-tile flip", {bit(5): "X"}), ("high flip", {bit(nq - 1): "X"})):
        steps = [(0.3, string)]
        circ, fn = pair(steps)
        add(f"one measured step, {name}", "pair", 1, circ.n_runs, *timed(fn, reps)[:3], max_rank=circ.max_rank)
        add(f"one measured step, {name}", "separate", 1, 1, *timed(separate(steps), reps)[:3])
    back = [(-t, p) for t, p in reversed(A.trotter_steps(ising(nq), 0.05))]
    for max_rank in range(A._native.PAULI_ADJOINT_MAX_RANK + 1):
        circ, fn = pair(back, max_rank)
        add("backward sweep of one Ising Trotter step", "pair", len(back), circ.n_runs, *timed(fn, reps)[:3], max_rank=max_rank)
    add("backward sweep of one Ising Trotter step", "separate", len(back), len(back), *timed(separate(back), reps)[:3])
    del third
    rot = A.trotter_steps(ising(nq), 0.05)
    add("adjoint_gradient, one Ising Trotter step as the ansatz", "gradient", len(rot), None,
        *timed(lambda: A.adjoint_gradient(phi, rot, ising(nq)), reps)[:3])
    os.makedirs(args.out_dir, exist_ok=True)
    record = {"device": torch.cuda.get_device_name(0), "log2n": nq, "dtype": "complex64", "repeats": reps, "clocks": clocks(), "rows": rows}
    with open(os.path.join(args.out_dir, "adjoint_timing.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out_dir, "adjoint_timing.md"), "w") as f:
        f.write(f"# Two-state Pauli circuits and adjoint gradients: 2^{nq} complex64, {record['device']}\n\n")
        f.write("Median of %d calls after 2 warm-ups, HIP events around the whole call, one process.  `pair`: A.PauliPairCircuit "
                "(4 passes per run); `separate`: pauli_apply + overlap + two pauli_evolve_ per step (8 passes per step).\n\n" % reps)
        f.write("| case | route | steps | max_rank | runs | ms (median) | min | max | nominal TB/s |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            tbs = "" if r["nominal_tbs"] is None else f"{r['nominal_tbs']:.2f}"
            f.write(f"| {r['name']} | {r['route']} | {r['steps']} | {r['max_rank']} | {r['runs']} | {r['ms_median']:.2f} | "
                    f"{r['ms_min']:.2f} | {r['ms_max']:.2f} | {tbs} |\n")


if __name__ == "__main__":
    main()
