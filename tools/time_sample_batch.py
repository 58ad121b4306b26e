"""Times bitstring sampling per trajectory (A.sample_batch) on 2^10 trajectories of 20 qubits in ONE complex64 tensor (2^30
elements) with S = 1 and S = 2^10 shots per trajectory, next to the route without it measured in the same process: a host loop of
B born.sample(slice_b, uniforms=u[b]) calls on the slices as separate tensors (each of which synchronises with the host).

Then S = 1 on 2^28 elements cut into trajectories of 2^20, 2^12, 2^10, 2^8 and 2^6 elements; there the loop is timed over its
first 4096 slices and scaled to B where B is larger (marked "scaled").  Last, batch_dims=() on the whole 2^30 tensor next to the
unbatched born.sample on it.

Bytes read / time is reported as a fraction of the 7.2 TB/s read probe, a pass being one reading of the tensor (the S = 1 call
reads it once for the block sums and again only the blocks that hold a target).  HIP events around the whole call, two warm-up
calls, the median of REPEATS timed calls, one process; the state is only read.  A row LOSES to its comparison when its median
exceeds the comparison's by more than the sum of the two min..max spreads.

    python tools/time_sample_batch.py [--repeats 5] [--out-dir profiles]

writes sample_batch_timing.json and sample_batch_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from artensor_amd import born  # noqa: E402
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
    nothing = lambda: None                                     # noqa: E731  (the state is only read)
    rows = []

    def add(case, route, fn, kind, passes=0, elements=n, note="", scale=1.0):
        med, lo, hi = (x * scale for x in timed(fn, nothing, reps))
        frac = passes * elements * 8 / (med * 1e-3) / (READ_PROBE_TBS * 1e12) if passes else None
        rows.append({"case": case, "route": route, "kind": kind, "ms_median": med, "ms_min": lo, "ms_max": hi, "passes": passes,
                     "fraction_of_read_probe": frac, "note": note})
        print(f"{case:44s} {route:44s} {med:10.3f} ms  [{lo:.3f}, {hi:.3f}]  " + (f"{100 * frac:.0f} % of the read probe  " if passes else "") + note,
              flush=True)

    def compare(case, view, S):
        """One row for the batched call on `view` [B, 2^s] (dim 0 the batch) and one for the loop over its slices."""
        Bv = view.shape[0]
        u = torch.rand((Bv, S), dtype=torch.float64, device=DEV, generator=g)
        info = A.sample_batch_info(view.shape, view.stride(), [0], S)
        add(case, f"sample_batch, one tensor ({info['form']}, {info['launches']} launches)", lambda: A.sample_batch(view, [0], uniforms=u), "new", 1,
            view.numel())
        count = min(Bv, LOOP_CAP)

        def loop():
            for b in range(count):
                born.sample(view[b], uniforms=u[b])
        scale = Bv / count
        add(case, f"loop of {Bv} born.sample calls  [comparison]", loop, "comparison",
            note=f"scaled: timed over the first {count} slices, times {scale:g}" if scale != 1 else "", scale=scale)

    batched = state.view(B, 2 ** nq)
    for S in (1, 2 ** 10):
        compare(f"2^{lb} trajectories of {nq} qubits, S = {S}", batched, S)
    total_bits = 28
    part = state[:2 ** total_bits]
    for s in (20, 12, 10, 8, 6):
        compare(f"2^{total_bits - s} trajectories of 2^{s} elements, S = 1", part.view(2 ** (total_bits - s), 2 ** s), 1)
    for S in (1, 2 ** 10):
        u = torch.rand((1, S), dtype=torch.float64, device=DEV, generator=g)
        case = f"batch_dims=(), 2^{lb + nq} elements, S = {S}"
        add(case, "sample_batch, batch_dims=()", lambda: A.sample_batch(state, (), uniforms=u), "new", 1, n)
        add(case, "born.sample on the whole tensor  [comparison]", lambda: born.sample(state, uniforms=u[0]), "comparison", 1, n)

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
    with open(os.path.join(args.out_dir, "sample_batch_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "sample_batch_timing.md"), "w") as f:
        f.write(f"# Bitstring sampling per trajectory: 2^{lb} trajectories of {nq} qubits in one complex64 tensor ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process; the state is only read.  The "
                "comparison is the route without the batched call, in the same process: a host loop of B `born.sample(slice_b, "
                f"uniforms=u[b])` calls on the slices as separate tensors (timed over the first {LOOP_CAP} slices and scaled where B is "
                "larger: marked scaled), and for `batch_dims=()` the unbatched `born.sample` on the whole tensor.  `% of read probe` is "
                "one reading of the tensor / time against the 7.2 TB/s read probe.  A row loses when its median exceeds the "
                "comparison's by more than the sum of the two min..max spreads.  complex128 is not measured.\n\n")
        f.write("| case | route | median ms | min..max ms | % of read probe | comparison ms | loses | note |\n"
                "|---|---|---:|---:|---:|---:|---|---|\n")
        for r in rows:
            cmp_ms = f"{r['comparison_ms_median']:.3f}" if "comparison_ms_median" in r else ""
            loses = ("yes" if r["loses"] else "no") if "loses" in r else ""
            frac = f"{100 * r['fraction_of_read_probe']:.0f}" if r["fraction_of_read_probe"] is not None else ""
            f.write(f"| {r['case']} | {r['route']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | {frac} | "
                    f"{cmp_ms} | {loses} | {r['note']} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows), "rows_that_lose": int(sum(verdicts))}))


if __name__ == "__main__":
    main()
