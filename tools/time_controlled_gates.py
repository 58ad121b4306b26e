"""Times the controlled gates (A.ControlledGate: one launch per gate) on 2^30 complex64 amplitudes on random data: t = 1 under
one control at memory bit 0 (a LOW control), at bit 15 and at bit 29; X under c = 2, 4, 10 and 29 controls (mcx_ on everything);
a dense t = 2 gate under c = 3; and a call whose classical condition does not hold.  Next to each row, in the same process, the
comparison route where there is one: A.WideGate with the embedded matrix |v><v| (x) U + (1 - |v><v|) (x) I wherever c + t <= 5, and
A.GateCircuit with the 4 x 4 matrix (what apply_gate_ runs) for CNOT / CZ.  HIP events around the whole call, two warm-up calls, the
median of REPEATS timed calls, prebuilt objects.  Run it under a time limit of its own (`timeout 600 python tools/...`).

    python tools/time_controlled_gates.py [--repeats 10] [--out-dir profiles]

writes controlled_gates_timing.json and controlled_gates_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from time_born import DEV, clocks, timed  # noqa: E402

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.diag([1.0, -1.0]).astype(np.complex128)


def embedded(u, c):
    """controls (all wanted 1) on the c most significant digits, the targets below them"""
    e = np.eye(u.shape[0] << c, dtype=np.complex128)
    e[-u.shape[0]:, -u.shape[0]:] = u
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    nq, reps = 30, args.repeats
    n = 2 ** nq
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    cube = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2)).view((2,) * nq)
    rng = np.random.default_rng(1)

    def unitary(dim):
        q, r = np.linalg.qr(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim)))
        return q * (np.diag(r) / np.abs(np.diag(r)))

    bit = lambda b: nq - 1 - b                                # dim of memory bit b
    u1, u2 = unitary(2), unitary(4)
    holds_not = torch.tensor([2], dtype=torch.int64, device=DEV)
    # (label, matrix, target bits, control bits, condition, narrow comparison matrix or None)
    cases = [
        ("t 1 dense, no control", u1, [7], [], None, None),
        ("t 1 dense, control at bit 0 (low)", u1, [7], [0], None, None),
        ("t 1 dense, control at bit 15", u1, [7], [15], None, None),
        ("t 1 dense, control at bit 29", u1, [7], [29], None, None),
        ("CNOT, control at bit 29", X, [7], [29], None, "narrow"),
        ("CZ, control at bit 15", Z, [7], [15], None, "narrow"),
        ("X, c 2", X, [7], [29, 3], None, None),
        ("X, c 4", X, [7], [29, 3, 15, 22], None, None),
        ("X, c 10", X, [7], [29, 3, 15, 22, 0, 11, 19, 25, 9, 27], None, None),
        ("X, c 29 (mcx_ on everything)", X, [7], [b for b in range(nq) if b != 7], None, None),
        ("t 2 dense, c 3", u2, [12, 2], [28, 17, 6], None, None),
        ("t 1 dense, control at bit 29, condition does not hold", u1, [7], [29], A.when(holds_not, 1, mask=1), None),
    ]
    rows = []
    for label, m, tbits, cbits, cond, narrow in cases:
        targets, controls = tuple(bit(b) for b in tbits), tuple(bit(b) for b in cbits)
        gate = A.ControlledGate(cube.shape, cube.stride(), cube.dtype, m, targets, controls, DEV)
        info = A.controlled_gate_info(cube.shape, cube.stride(), m, targets, controls)
        med, lo, hi, extra = timed(lambda: gate(cube, cond), reps)
        row = {"case": label, "t": len(tbits), "c": len(cbits), "c_high": info["c_high"], "c_low": info["c_low"], "target_bits": tbits,
               "control_bits": cbits, "n_tiles": info["n_tiles"], "bytes_read": info["bytes_read"], "ms_median": med, "ms_min": lo,
               "ms_max": hi, "extra_bytes": extra, "condition_holds": cond is None,
               "gbps": (0.0 if cond is not None else 2 * info["bytes_read"] / (med * 1e-3) / 1e9)}
        if len(tbits) + len(cbits) <= 5:
            wide = A.WideGate(cube.shape, cube.stride(), cube.dtype, embedded(m, len(cbits)), controls + targets, DEV)
            row["wide_ms_median"], row["wide_ms_min"], row["wide_ms_max"], _ = timed(lambda: wide(cube), reps)
        if narrow:
            circ = A.GateCircuit(cube.shape, cube.stride(), cube.dtype, [(embedded(m, 1), controls + targets)], DEV)
            row["narrow_ms_median"], row["narrow_ms_min"], row["narrow_ms_max"], _ = timed(lambda: circ(cube), reps)
        rows.append(row)
        print(row, flush=True)
    name = torch.cuda.get_device_name(0)
    out = {"device": name, "clocks": clocks(), "n": n, "dtype": "complex64", "repeats": reps, "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "controlled_gates_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    lines = [f"# Controlled gates on 2^30 complex64 amplitudes ({name})", "",
             f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, prebuilt objects, one process.  GB/s: read "
             "+ write of the elements whose high controls match, over the median time.  wide: `WideGate` with the embedded matrix "
             "(c + t <= 5); narrow: `GateCircuit` with the 4 x 4 matrix (what `apply_gate_` runs).", "",
             "| case | t | c (high + low) | tiles | median ms | min..max ms | GB/s | wide ms | narrow ms | controlled / wide |",
             "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        wide = f"{r['wide_ms_median']:.3f}" if "wide_ms_median" in r else ""
        narrow = f"{r['narrow_ms_median']:.3f}" if "narrow_ms_median" in r else ""
        ratio = f"{r['ms_median'] / r['wide_ms_median']:.2f}" if "wide_ms_median" in r else ""
        lines.append(f"| {r['case']} | {r['t']} | {r['c_high']} + {r['c_low']} | {r['n_tiles']} | {r['ms_median']:.3f} | "
                     f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['gbps']:.0f} | {wide} | {narrow} | {ratio} |")
    with open(os.path.join(args.out_dir, "controlled_gates_timing.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
