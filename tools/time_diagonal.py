"""Times the diagonal operators (artensor_amd/diagonal.py) on 2^30 complex64 amplitudes against the term-by-term routes they
replace, in one process, and writes profiles/diagonal_timing.{json,md}.

Per problem -- a 30-qubit ring MaxCut (K = 30), a Sherrington-Kirkpatrick instance (K = 435) and a 3-local instance with 56
groups -- the rows PHASE, MULTIPLY, EXPECT and PAIR: the median of 10 calls after 2 warm-ups, HIP events around the call,
every object prebuilt.  Comparisons: PHASE against a PauliCircuit of the K Z rotations, PAIR against the PauliPairCircuit of
the same rotations with every step measured, EXPECT against pauli_sum_expectation (which also pays its host work and one
synchronisation per call: it has no prebuilt form).  MULTIPLY has no in-place comparison.  One more row: a p = 1
qaoa_gradient on the ring against adjoint_gradient with the bonds as rotations that share one parameter (whole calls, wall
clock around a synchronisation, the median of 3).

    python tools/time_diagonal.py [--qubits 30] [--calls 10]
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402

DEV = "cuda:0"


def problems(n, rng):
    z = lambda *bits: {n - 1 - b: "Z" for b in bits}                      # noqa: E731  (memory bit -> dim of a contiguous state)
    ring = A.maxcut_terms([(q, (q + 1) % n) for q in range(n)])
    sk = [(float(rng.choice([-1.0, 1.0])) / np.sqrt(n), z(a, b)) for a, b in itertools.combinations(range(n), 2)]
    low, high = list(range(10)), list(range(10, n))
    local3 = []
    for k in range(3):                                                     # every pattern of at most two low bits, three times
        for pat in [()] + [(b,) for b in low] + list(itertools.combinations(low, 2)):
            hs = [int(h) for h in rng.choice(high, size=3 - len(pat), replace=False)]
            local3.append((float(rng.standard_normal()), z(*pat, *hs)))
    return {"ring-maxcut": ring, "sherrington-kirkpatrick": sk, "3-local": local3}


def median_ms(fn, calls, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    n, rng = args.qubits, np.random.default_rng(0)
    shape = (2,) * n
    amps = torch.zeros(1 << n, dtype=torch.complex64, device=DEV)
    torch.view_as_real(amps).normal_(generator=torch.Generator(DEV).manual_seed(1)).mul_(2.0 ** (-(n + 1) / 2))
    amps, lam = amps.view(shape), torch.empty(1 << n, dtype=torch.complex64, device=DEV).view(shape)
    lam.copy_(amps)
    gamma, rows = 0.37, []
    for name, terms in problems(n, rng).items():
        op = A.DiagonalOperator(shape, amps.stride(), amps.dtype, terms, DEV)
        rot = [(gamma * c, s) for c, s in terms if s]                      # (the constant of MaxCut is a global phase: no rotation)
        circ = A.PauliCircuit(shape, amps.stride(), amps.dtype, rot, DEV)
        pair = A.PauliPairCircuit(shape, amps.stride(), amps.dtype, rot, DEV)
        info = A.diagonal_info(shape, amps.stride(), terms)
        base = {"problem": name, "K": info["K"], "G": info["G"], "n_static": info["n_static"]}
        rows.append(dict(base, op="PHASE", ms=median_ms(lambda: op.evolve_(amps, gamma), args.calls),
                         ref="PauliCircuit", ref_ms=median_ms(lambda: circ(amps), args.calls)))
        rows.append(dict(base, op="EXPECT", ms=median_ms(lambda: op.moments(amps, device=True), args.calls),
                         ref="pauli_sum_expectation", ref_ms=median_ms(lambda: A.pauli_sum_expectation(amps, terms), args.calls)))
        rows.append(dict(base, op="PAIR", ms=median_ms(lambda: op.pair_(lam, amps, gamma, device=True), args.calls),
                         ref="PauliPairCircuit", ref_ms=median_ms(lambda: pair(lam, amps, device=True), args.calls)))
        rows.append(dict(base, op="MULTIPLY", ms=median_ms(lambda: op.multiply_(lam), args.calls), ref=None, ref_ms=None))
        lam.copy_(amps)
        print(json.dumps(rows[-4:]), flush=True)
    ring = problems(n, np.random.default_rng(0))["ring-maxcut"]
    bonds = [(c, s) for c, s in ring if s]
    rotations = [(gamma * c, s) for c, s in bonds] + [(0.21, {q: "X"}) for q in range(n)]
    params = [0] * len(bonds) + [1] * n

    def wall(fn):
        out = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(out)

    del lam
    torch.cuda.empty_cache()
    rows.append({"problem": "ring-maxcut", "K": len(ring), "op": "qaoa_gradient p=1", "ms": wall(lambda: A.qaoa_gradient(amps, ring, [gamma], [0.21])),
                 "ref": "adjoint_gradient", "ref_ms": wall(lambda: A.adjoint_gradient(amps, rotations, ring, params))})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    state_gib = (8 << n) / 2 ** 30
    with open(os.path.join(ROOT, "profiles", "diagonal_timing.json"), "w") as fh:
        json.dump({"qubits": n, "dtype": "complex64", "state_gib": state_gib, "calls": args.calls, "device": torch.cuda.get_device_name(0),
                   "rows": rows}, fh, indent=1)
    with open(os.path.join(ROOT, "profiles", "diagonal_timing.md"), "w") as fh:
        fh.write(f"# Diagonal operators, 2^{n} complex64 ({state_gib:.0f} GiB), median of {args.calls} calls\n\n")
        fh.write("| problem | K | G | operation | ms | GB/s of the pass | comparison | ms | ratio |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            moved = {"PHASE": 2, "MULTIPLY": 2, "EXPECT": 1, "PAIR": 4}.get(r["op"])
            bw = f"{moved * (8 << n) / r['ms'] / 1e6:.0f}" if moved else ""
            ref = f"{r['ref']} | {r['ref_ms']:.2f} | {r['ref_ms'] / r['ms']:.1f}x" if r["ref"] else " | | "
            fh.write(f"| {r['problem']} | {r['K']} | {r.get('G', '')} | {r['op']} | {r['ms']:.2f} | {bw} | {ref} |\n")


if __name__ == "__main__":
    main()
