"""Times one trajectory step of a noise channel (A.channel_, A.ChannelOp) on 2^30 complex64 amplitudes, form by form, next to
what each form is predicted to cost and next to the comparison route of the parent commit, A.apply_channel_ (one or two qubits
only), measured in the same process with the same Kraus set and the same forced uniform:

    FIXED, identity drawn      about one launch (two small launches, no pass over the state)
    FIXED, a Pauli drawn       one wide-gate pass               (reference row: a prebuilt WideGate of that Pauli)
    DIAGONAL                   the marginal plus one pass       (reference rows: marginal_probabilities, WideGate)
    DENSE                      the RDM plus one pass            (reference rows: reduced_density_matrix, WideGate)

The state is restored from a copy before every call, outside the timed region.  HIP events around the whole call, two warm-up
calls, the median of REPEATS timed calls, one process.  A row LOSES to its comparison when its median exceeds the comparison's
by more than the sum of the two min..max spreads.

    python tools/time_channel.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes channel_timing.json and channel_timing.md into --out-dir."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from time_born import DEV, clocks  # noqa: E402
from time_measure import timed  # noqa: E402

H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


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
    backup = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    state = torch.empty_like(backup)
    cube = state.view((2,) * nq)
    restore = lambda: state.copy_(backup)
    nothing = lambda: None
    bit = lambda b: nq - 1 - b                                 # dim of memory bit b
    mid, top = nq // 2, nq - 1
    copy_ms = timed(restore, nothing, reps)
    print(f"copy probe {copy_ms[0]:.3f} ms", flush=True)
    rows = []

    def add(name, draw, bits, route, fn, kind):
        med, lo, hi = timed(fn, restore, reps)
        rows.append({"name": name, "draw": draw, "memory_bits": list(bits), "route": route, "kind": kind, "ms_median": med,
                     "ms_min": lo, "ms_max": hi})
        print(f"{name:28s} {draw:18s} {str(list(bits)):14s} {route:40s} {med:9.3f} ms  [{lo:.3f}, {hi:.3f}]", flush=True)

    def channel_rows(name, ch, draw, u, bits, compare, references=()):
        dims = [bit(b) for b in bits]
        restore()
        op = A.ChannelOp(cube.shape, cube.stride(), cube.dtype, ch, dims, DEV)
        j, _ = op(cube, uniform=u)
        draw = f"{draw} (j = {j})"
        add(name, draw, bits, "channel_(device=False)", lambda: A.channel_(cube, ch, dims, uniform=u), "new")
        add(name, draw, bits, "ChannelOp(device=True)", lambda: op(cube, uniform=u, device=True), "new-op")
        if compare:
            kraus = ch.kraus
            restore()
            jc, _ = A.apply_channel_(cube, kraus, dims, uniform=u)
            assert jc == j, (name, j, jc)
            add(name, draw, bits, "apply_channel_  [comparison]", lambda: A.apply_channel_(cube, kraus, dims, uniform=u), "comparison")
        for ref in references:
            if ref == "pass":
                gate = A.WideGate(cube.shape, cube.stride(), cube.dtype, ch.matrices[j], dims, DEV)
                add(name, draw, bits, "WideGate of operator j  [reference]", lambda: gate(cube), "reference")
            elif ref == "marginal":
                add(name, draw, bits, "marginal_probabilities  [reference]", lambda: A.marginal_probabilities(cube, dims), "reference")
            elif ref == "rdm":
                add(name, draw, bits, "reduced_density_matrix  [reference]", lambda: A.reduced_density_matrix(cube, dims), "reference")

    dep = A.depolarizing(0.01)
    channel_rows("depolarizing(0.01)", dep, "identity", 0.5, [mid], True)
    for b in (0, mid, top):
        channel_rows("depolarizing(0.01)", dep, "Pauli X", 0.992, [b], True, ("pass",))
    ad = A.amplitude_damping(0.1)
    for b in (0, mid, top):
        channel_rows("amplitude_damping(0.1)", ad, "K_0", 0.3, [b], True, ("marginal", "pass") if b == mid else ())
        channel_rows("amplitude_damping(0.1)", ad, "K_1", 0.99, [b], True)
    dense = A.Channel.from_kraus([H @ k @ H for k in ad.kraus])
    channel_rows("DENSE one-qubit set", dense, "K_0", 0.3, [mid], True, ("rdm", "pass"))
    dep2 = A.depolarizing(0.01, 2)
    channel_rows("depolarizing(0.01, 2)", dep2, "identity", 0.5, [1, top], True)
    channel_rows("depolarizing(0.01, 2)", dep2, "a Pauli string", 0.9951, [1, top], True, ("pass",))
    dep3 = A.depolarizing(0.01, 3)
    channel_rows("depolarizing(0.01, 3)", dep3, "identity", 0.5, [0, mid, top], False)
    channel_rows("depolarizing(0.01, 3)", dep3, "a Pauli string", 0.9951, [0, mid, top], False, ("pass",))

    # the verdict of every row that has a comparison
    verdicts = []
    for r in rows:
        if r["kind"] not in ("new", "new-op"):
            continue
        cmp_ = [c for c in rows if c["kind"] == "comparison" and (c["name"], c["draw"], c["memory_bits"]) == (r["name"], r["draw"], r["memory_bits"])]
        if not cmp_:
            continue
        c = cmp_[0]
        spread = (r["ms_max"] - r["ms_min"]) + (c["ms_max"] - c["ms_min"])
        r["comparison_ms_median"], r["loses"] = c["ms_median"], bool(r["ms_median"] > c["ms_median"] + spread)
        verdicts.append(r["loses"])
    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing); the state is "
           "restored before every call, outside the timed region", "copy_probe": {"ms_median": copy_ms[0], "ms_min": copy_ms[1], "ms_max": copy_ms[2]},
           "rows_that_lose": int(sum(verdicts)), "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total,
           "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "channel_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "channel_timing.md"), "w") as f:
        f.write(f"# Noise-channel steps on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process; the state is restored from a "
                f"copy before every call, outside the timed region (copy probe: {copy_ms[0]:.3f} ms).  The draw is forced by `uniform`.  "
                "`apply_channel_` is the comparison route (host draw from a reduced density matrix, one or two qubits only) with the same "
                "Kraus set and uniform; reference rows time the parts a form is predicted to cost.  A row loses when its median exceeds "
                "the comparison's by more than the sum of the two min..max spreads.  complex128 is not measured.\n\n")
        f.write("| channel | draw | memory bits | route | median ms | min..max ms | comparison ms | loses |\n|---|---|---|---|---:|---:|---:|---|\n")
        for r in rows:
            cmp_ms = f"{r['comparison_ms_median']:.3f}" if "comparison_ms_median" in r else ""
            loses = ("yes" if r["loses"] else "no") if "loses" in r else ""
            f.write(f"| {r['name']} | {r['draw']} | {r['memory_bits']} | {r['route']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                    f"{cmp_ms} | {loses} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows), "rows_that_lose": int(sum(verdicts))}))


if __name__ == "__main__":
    main()
