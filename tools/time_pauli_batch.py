"""Times Pauli expectation values per trajectory (A.pauli_expectation_batch, A.pauli_sum_expectation_batch) on 2^10 trajectories
of 20 qubits in ONE complex64 tensor (2^30 elements), next to the route without them measured in the same process: a host loop of
2^10 A.pauli_expectation(slice_b, ..., device=True) calls on the slices as separate tensors.

    one Z string                         Z on every qubit: no partner
    one X inside the tile                X on memory bit 5 of a trajectory
    one X on the highest local bit       X on memory bit 19: half the local tiles, weight 2
    16 Z / ZZ strings                    one group, one pass
    transverse-field Ising, 39 terms     19 ZZ (one group, two passes) + 20 X (a group each): 22 passes, then one matmul

Then one Z string on 2^28 elements cut into trajectories of 2^20, 2^12, 2^10, 2^8 and 2^6 elements; there the loop is timed over
its first 4096 slices and scaled to B where B is larger (marked in the note).

Bytes read / time is reported as a fraction of the 7.2 TB/s read probe.  HIP events around the whole call, two warm-up calls,
the median of REPEATS timed calls, one process; the state is only read.  A row LOSES to its comparison when its median exceeds
the comparison's by more than the sum of the two min..max spreads.

    python tools/time_pauli_batch.py [--repeats 5] [--out-dir profiles]

writes pauli_batch_timing.json and pauli_batch_timing.md into --out-dir."""
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

READ_PROBE_TBS = 7.2
LOOP_CAP = 4096


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
    state = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    batched = state.view((B,) + (2,) * nq)                     # dim 0 is the batch, dim 1 + d the qubit on memory bit nq - 1 - d
    nothing = lambda: None                                     # noqa: E731  (the state is only read)
    rows = []

    def on_bits(ops, nd=nq, lead=0):
        """{dim: letter} of a view whose dim lead + d holds memory bit nd - 1 - d, from {memory bit: letter}."""
        return {lead + nd - 1 - b: c for b, c in ops.items()}

    def add(case, route, fn, kind, passes=0, elements=n, note=""):
        med, lo, hi = timed(fn, nothing, reps)
        frac = passes * elements * 8 / (med * 1e-3) / (READ_PROBE_TBS * 1e12) if passes else None
        rows.append({"case": case, "route": route, "kind": kind, "ms_median": med, "ms_min": lo, "ms_max": hi, "passes": passes,
                     "fraction_of_read_probe": frac, "note": note})
        print(f"{case:36s} {route:46s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]  " + (f"{100 * frac:.0f} % of the read probe  " if passes else "") + note,
              flush=True)

    def compare(case, view, strings, batch_view_strings, passes, elements, terms=None):
        """One row for the batched call on `view` (dim 0 the batch) and one for the loop over its slices."""
        Bv = view.shape[0]
        if terms is None:
            add(case, "pauli_expectation_batch, one tensor", lambda: A.pauli_expectation_batch(view, batch_view_strings, [0]), "new", passes, elements)
        else:
            add(case, "pauli_sum_expectation_batch, one tensor", lambda: A.pauli_sum_expectation_batch(view, terms, [0]), "new", passes, elements)
        count = min(Bv, LOOP_CAP)

        def loop():
            for b in range(count):
                A.pauli_expectation(view[b], strings, device=True)
        med, lo, hi = timed(loop, nothing, reps)
        scale = Bv / count
        note = f"timed over the first {count} slices, scaled by {scale:g}" if scale != 1 else ""
        rows.append({"case": case, "route": f"loop of {Bv} pauli_expectation calls  [comparison]", "kind": "comparison", "ms_median": med * scale,
                     "ms_min": lo * scale, "ms_max": hi * scale, "passes": 0, "fraction_of_read_probe": None, "note": note})
        print(f"{case:36s} {'loop of ' + str(Bv) + ' pauli_expectation calls':46s} {med * scale:10.3f} ms  [{lo * scale:.3f}, {hi * scale:.3f}]  {note}",
              flush=True)

    singles = [("one Z string", {b: "Z" for b in range(nq)}), ("one X inside the tile", {5: "X"}),
               ("one X on the highest local bit", {nq - 1: "X"})]
    for case, ops in singles:
        compare(case, batched, on_bits(ops), on_bits(ops, lead=1), 1, n)
    zz = [{b: "Z"} for b in range(8)] + [{b: "Z", b + 1: "Z"} for b in range(8)]
    compare("16 Z / ZZ strings, one pass", batched, [on_bits(o) for o in zz], [on_bits(o, lead=1) for o in zz], 1, n)
    ising = [(-1.0, {b: "Z", b + 1: "Z"}) for b in range(nq - 1)] + [(-0.5, {b: "X"}) for b in range(nq)]
    info = A.pauli_batch_info(batched.shape, batched.stride(), [on_bits(o, lead=1) for _, o in ising], [0])
    compare(f"transverse-field Ising, {len(ising)} terms", batched, [on_bits(o) for _, o in ising], None, info["n_launches"], n,
            terms=[(c, on_bits(o, lead=1)) for c, o in ising])

    total_bits = 28
    part = state[:2 ** total_bits]
    for s in (20, 12, 10, 8, 6):
        view = part.view((2 ** (total_bits - s),) + (2,) * s)
        ops = {b: "Z" for b in range(s)}
        compare(f"one Z string, 2^{total_bits - s} trajectories of 2^{s}", view, on_bits(ops, s), on_bits(ops, s, 1), 1, 2 ** total_bits)

    verdicts = []
    for r in rows:
        if r["kind"] != "new":
            continue
        c = [c for c in rows if c["kind"] == "comparison" and c["case"] == r["case"]][0]
        spread = (r["ms_max"] - r["ms_min"]) + (c["ms_max"] - c["ms_min"])
        r["comparison_ms_median"], r["loses"] = c["ms_median"], bool(r["ms_median"] > c["ms_median"] + spread)
        verdicts.append(r["loses"])

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_B": lb, "qubits": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing); the state is only "
           "read", "read_probe_TB_per_s": READ_PROBE_TBS, "rows_that_lose": int(sum(verdicts)), "clocks": clocks(),
           "device_memory_free_bytes": free, "device_memory_total_bytes": total, "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "pauli_batch_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "pauli_batch_timing.md"), "w") as f:
        f.write(f"# Pauli expectation values per trajectory: 2^{lb} trajectories of {nq} qubits in one complex64 tensor ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process; the state is only read.  The "
                "comparison is the route without the batched call, in the same process: a host loop of B `pauli_expectation(slice_b, ..., "
                f"device=True)` calls on the slices as separate tensors (timed over the first {LOOP_CAP} slices and scaled where B is "
                "larger).  `% of read probe` is passes x bytes of the tensor / time against the 7.2 TB/s read probe.  A row loses when "
                "its median exceeds the comparison's by more than the sum of the two min..max spreads.  complex128 is not measured.\n\n")
        f.write("| case | route | median ms | min..max ms | passes | % of read probe | comparison ms | loses | note |\n"
                "|---|---|---:|---:|---:|---:|---:|---|---|\n")
        for r in rows:
            cmp_ms = f"{r['comparison_ms_median']:.3f}" if "comparison_ms_median" in r else ""
            loses = ("yes" if r["loses"] else "no") if "loses" in r else ""
            frac = f"{100 * r['fraction_of_read_probe']:.0f}" if r["fraction_of_read_probe"] is not None else ""
            f.write(f"| {r['case']} | {r['route']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['passes'] or ''} | {frac} | "
                    f"{cmp_ms} | {loses} | {r['note']} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows), "rows_that_lose": int(sum(verdicts))}))


if __name__ == "__main__":
    main()
