"""Times the in-place Pauli circuits (A.PauliCircuit: one launch per run) on a 2^30-element complex64 tensor of random data, next
to the out-of-place route measured in the same process: A.pauli_rotate into a given `out` for one rotation, and a ping-pong loop
of such calls (prebuilt operators, two buffers) for a Trotter step.  HIP events around the whole call, two warm-up calls, the median
of REPEATS timed calls; extra device memory = the peak above what is allocated before the call (the state itself not counted).

    python tools/time_pauli_evolve.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes pauli_evolve_timing.json and pauli_evolve_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from time_born import DEV, READ_PROBE_TBS, clocks, timed  # noqa: E402


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
    x = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    cube = x.view((2,) * nq)                                  # dim d is memory bit nq - 1 - d
    rng = np.random.default_rng(1)
    state_bytes = n * 8
    rows = []

    def add(name, route, steps, runs, launches, med, lo, hi, extra, max_rank=None):
        moved = 2 * launches * state_bytes
        rows.append({"name": name, "route": route, "steps": steps, "max_rank": max_rank, "runs": runs, "launches": launches,
                     "ms_median": med, "ms_min": lo, "ms_max": hi, "extra_bytes": extra, "nominal_bytes_moved": moved,
                     "fraction_of_read_probe": moved / (med * 1e-3) / (READ_PROBE_TBS * 1e12)})
        print(f"{name:44s} {route:34s} runs {runs:3d} launches {launches:3d} {med:9.3f} ms [{lo:.3f}, {hi:.3f}] "
              f"{rows[-1]['fraction_of_read_probe']:6.1%} extra {extra / 2 ** 20:9.2f} MiB", flush=True)

    def in_place(name, steps, max_rank=None):
        circ = A.PauliCircuit(cube.shape, cube.stride(), cube.dtype, steps, DEV, max_rank)
        med, lo, hi, extra = timed(lambda: circ(cube), reps)
        add(name, "in place (PauliCircuit)", len(steps), circ.n_runs, circ.n_runs, med, lo, hi, extra, circ.max_rank if max_rank is not None else None)

    def out_of_place(name, steps):
        """The route without the in-place kernels: one out-of-place rotation per step, ping-pong between the state and a second buffer."""
        other = torch.empty_like(cube)
        ops = [A.PauliSumOperator(cube.shape, cube.stride(), cube.dtype, [(np.cos(th), {}), (-1j * np.sin(th), p)], DEV) for th, p in steps]

        def call():
            src, dst = cube, other
            for op in ops:
                op(src, out=dst)
                src, dst = dst, src
        torch.cuda.synchronize()
        med, lo, hi, extra = timed(call, reps)
        add(name, "out of place (pauli_rotate, out given)", len(steps), len(steps), len(steps), med, lo, hi, extra + state_bytes)
        del other
        torch.cuda.empty_cache()

    mixed = {d: str(rng.choice(list("XYZ"))) for d in range(nq)}
    singles = [("one Z-type rotation  Z_3 Z_17", {3: "Z", 17: "Z"}), ("one X inside the tile (memory bit 3)", {nq - 1 - 3: "X"}),
               ("one X on the slowest bit (X_0)", {0: "X"}), (f"one weight-{nq} mixed string", mixed)]
    for name, p in singles:
        in_place(name, [(0.3, p)])
        out_of_place(name, [(0.3, p)])
    tfim = [(-1.0, {q: "Z", q + 1: "Z"}) for q in range(nq - 1)] + [(-0.7, {q: "X"}) for q in range(nq)]
    heis = [(0.25, {q: letter, q + 1: letter}) for q in range(nq - 1) for letter in "XYZ"]
    for name, terms in ((f"Ising chain, first-order step ({len(tfim)} rotations)", tfim),
                        (f"Heisenberg chain, first-order step ({len(heis)} rotations)", heis)):
        steps = A.trotter_steps(terms, 0.05)
        for max_rank in (0, 1, 2, 3, 4):
            in_place(name, steps, max_rank)
        out_of_place(name, steps)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "read_probe_TBps": READ_PROBE_TBS, "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total,
           "mixed_string": "".join(mixed[d] for d in range(nq)), "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "pauli_evolve_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "pauli_evolve_timing.md"), "w") as f:
        f.write(f"# In-place Pauli circuits on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call.  In place: a prebuilt `PauliCircuit`, one "
                "launch per run.  Out of place: prebuilt two-term `PauliSumOperator`s (what `pauli_rotate` builds) writing into a given "
                "`out`, ping-pong between the state and a second buffer, one launch per rotation.  Nominal bytes = launches x (one read + "
                f"one write of the {state_bytes / 2 ** 30:.0f} GiB state); fraction = nominal bytes / time / {READ_PROBE_TBS} TB/s "
                "(tools/probes/read_probe.hip).  Extra device memory: the peak above the state itself (the second buffer included).\n\n")
        f.write("| circuit | route | steps | max_rank | runs | launches | median ms | min..max ms | fraction | extra device memory |\n"
                "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            mr = "-" if r["max_rank"] is None else str(r["max_rank"])
            f.write(f"| {r['name']} | {r['route']} | {r['steps']} | {mr} | {r['runs']} | {r['launches']} | {r['ms_median']:.3f} | "
                    f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['fraction_of_read_probe']:.1%} | {r['extra_bytes'] / 2 ** 20:.2f} MiB |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
