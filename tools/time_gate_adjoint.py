"""Times the two-state gate circuits (A.GatePairCircuit: one launch per run and a finish launch) and A.gate_adjoint_gradient on
complex64 tensors of 2^30 random elements, next to the route that exists without them, timed in the same process: per measured
gate a copy of phi into a third buffer, A.apply_gate_ of M on the copy, A.overlap, and A.apply_gate_ of the gate on each state
(ten passes over a state-sized vector, three buffers); two A.apply_gate_ for a gate that is not measured.  HIP events around the
whole call, two warm-up calls, the median of REPEATS timed calls.

    python tools/time_gate_adjoint.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes gate_adjoint_timing.json and gate_adjoint_timing.md into --out-dir.  complex128 is not timed: the files say so."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from time_born import DEV, clocks, timed  # noqa: E402

CNOT = np.eye(4)[[0, 1, 3, 2]].astype(np.complex128)


def ising(nq, j=-1.0, h=-0.7):
    return [(j, {a: "Z", a + 1: "Z"}) for a in range(nq - 1)] + [(h, {d: "X"}) for d in range(nq)]


def ansatz(nq, layers=2, seed=3):
    """RY and RZ on every qubit and a CNOT ring, `layers` times: entries of gate_adjoint_gradient's `gates`."""
    rng = np.random.default_rng(seed)
    gates = []
    for _ in range(layers):
        gates += [A.parametric_gate("ry", float(rng.uniform(-np.pi, np.pi)), q) for q in range(nq)]
        gates += [A.parametric_gate("rz", float(rng.uniform(-np.pi, np.pi)), q) for q in range(nq)]
        gates += [(CNOT, (q, (q + 1) % nq)) for q in range(nq)]
    return gates


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

    def add(name, route, gates, measured, runs, med, lo, hi, max_rank=None):    # (every row: `reps` timed calls after 2 warm-ups)
        passes = 4 * runs if route == "pair" else 10 * measured + 4 * (gates - measured) if route == "separate" else None
        rows.append({"name": name, "route": route, "gates": gates, "measured": measured, "max_rank": max_rank, "runs": runs, "passes": passes,
                     "repeats": reps, "warmup": 2, "ms_median": med, "ms_min": lo, "ms_max": hi,
                     "nominal_tbs": None if passes is None else passes * state_bytes / med / 1e9})
        print(rows[-1], flush=True)

    def separate(gates, measure):
        """The route without the two-state kernel: copy, M on the copy, <lam|M phi>, then the gate on each state."""
        def fn():
            for (u, dims), m in zip(gates, measure):
                if m is not None:
                    third.copy_(phi)
                    A.apply_gate_(third, m, dims)
                    A.overlap(lam, third)
                A.apply_gate_(phi, u, dims)
                A.apply_gate_(lam, u, dims)
        return fn

    def pair(gates, measure, max_rank=None):
        circ = A.GatePairCircuit(phi.shape, phi.stride(), phi.dtype, gates, DEV, measure, max_rank)
        return circ, (lambda: circ(lam, phi, device=True))

    def ratio(name):
        """separate / pair per case (per max_rank where several were timed)."""
        sep = [r for r in rows if r["name"] == name and r["route"] == "separate"][0]["ms_median"]
        return {str(r["max_rank"]): sep / r["ms_median"] for r in rows if r["name"] == name and r["route"] == "pair"}

    bit = lambda b: nq - 1 - b
    ry, dry, _ = A.parametric_gate("ry", 0.7, 0)
    rzz, drzz, _ = A.parametric_gate("rzz", 0.7, (0, 1))
    crx, dcrx, _ = A.parametric_gate("crx", 0.7, (0, 1))
    singles = [("register target", ry, dry, (bit(0),)), ("piece target", ry, dry, (bit(5),)), ("high target", ry, dry, (bit(nq - 1),)),
               ("two-qubit on two high bits", crx, dcrx, (bit(nq - 1), bit(nq - 4))), ("diagonal", rzz, drzz, (bit(nq - 1), bit(3)))]
    ratios = {}
    for name, u, du, dims in singles:
        name = f"one measured gate, {name}"
        gates, measure = [(u.conj().T, dims)], [du @ u.conj().T]
        circ, fn = pair(gates, measure)
        add(name, "pair", 1, 1, circ.n_runs, *timed(fn, reps)[:3], max_rank=circ.max_rank)
        add(name, "separate", 1, 1, 1, *timed(separate(gates, measure), reps)[:3])
        ratios[name] = ratio(name)
    forward = ansatz(nq)
    back = [(np.asarray(gate[0]).conj().T, gate[-1]) for gate in reversed(forward)]
    back_measure = [gate[1] @ np.asarray(gate[0]).conj().T if len(gate) == 3 else None for gate in reversed(forward)]
    n_meas = sum(m is not None for m in back_measure)
    name = f"backward sweep of a {nq}-qubit two-layer RY/RZ + CNOT-ring ansatz"
    for max_rank in range(A._native.GATES_ADJOINT_MAX_RANK + 1):
        circ, fn = pair(back, back_measure, max_rank)
        add(name, "pair", len(back), n_meas, circ.n_runs, *timed(fn, reps)[:3], max_rank=max_rank)
    add(name, "separate", len(back), n_meas, len(back), *timed(separate(back, back_measure), reps)[:3])
    ratios[name] = ratio(name)
    terms = ising(nq)
    name = "gate_adjoint_gradient of that ansatz, Ising terms"
    add(name, "gradient", len(forward), n_meas, None, *timed(lambda: A.gate_adjoint_gradient(phi, forward, terms), reps)[:3])
    fwd = A.GateCircuit(phi.shape, phi.stride(), phi.dtype, [(gate[0], gate[-1]) for gate in forward], DEV)
    ham = A.PauliSumOperator(phi.shape, phi.stride(), phi.dtype, terms, DEV)
    sweep = separate(back, back_measure)

    def gradient_separate():
        lam.copy_(ham(fwd(phi)))
        A.overlap(phi, lam)
        sweep()
    add(name, "gradient, separate sweep", len(forward), n_meas, None, *timed(gradient_separate, reps)[:3])
    ratios[name] = {"None": rows[-1]["ms_median"] / rows[-2]["ms_median"]}
    os.makedirs(args.out_dir, exist_ok=True)
    record = {"device": torch.cuda.get_device_name(0), "log2n": nq, "dtype": "complex64", "complex128": "unmeasured", "repeats": reps,
              "clocks": clocks(), "rows": rows, "separate_over_pair": ratios}
    with open(os.path.join(args.out_dir, "gate_adjoint_timing.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out_dir, "gate_adjoint_timing.md"), "w") as f:
        f.write(f"# Two-state gate circuits and adjoint gradients: 2^{nq} complex64, {record['device']}\n\n")
        f.write("Median of %d calls after 2 warm-ups, HIP events around the whole call, one process.  `pair`: A.GatePairCircuit "
                "(4 passes per run); `separate`: copy + apply_gate_ + overlap + two apply_gate_ per measured gate (10 passes), two "
                "apply_gate_ per fixed gate (4 passes).  complex128: unmeasured.\n\n" % reps)
        f.write("| case | route | gates | measured | max_rank | runs | ms (median) | min | max | nominal TB/s |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            tbs = "" if r["nominal_tbs"] is None else f"{r['nominal_tbs']:.2f}"
            f.write(f"| {r['name']} | {r['route']} | {r['gates']} | {r['measured']} | {r['max_rank']} | {r['runs']} | {r['ms_median']:.2f} | "
                    f"{r['ms_min']:.2f} | {r['ms_max']:.2f} | {tbs} |\n")
        f.write("\n## separate / pair (above 1: the two-state kernel wins)\n\n| case | max_rank | ratio |\n|---|---|---|\n")
        for case, by_rank in ratios.items():
            for rank, value in by_rank.items():
                f.write(f"| {case} | {rank} | {value:.2f} |\n")


if __name__ == "__main__":
    main()
