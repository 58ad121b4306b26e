"""Times y = H a (A.pauli_sum_apply: one launch per call) on a 2^30-element complex64 tensor of random data, next to two routes
measured in the same process: A.pauli_sum_expectation on the same terms (the cost, before this kernel, of touching every group
once: one pass per group and sixteen terms) and the torch formulation (flip / sign multiply / add per term on the contiguous
tensor, within a time budget).  HIP events around the whole call, two warm-up calls, the median of REPEATS timed calls; fraction =
(bytes read + bytes written of the info call) / time / the 7.2 TB/s of tools/probes/read_probe.hip.

    python tools/time_pauli_apply.py [--log2n 30] [--repeats 10] [--torch-budget-s 60] [--out-dir profiles]

writes pauli_apply_timing.json and pauli_apply_timing.md into --out-dir."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from time_born import DEV, READ_PROBE_TBS, clocks, timed  # noqa: E402


def torch_apply(x, terms, nq):
    """sum_k c_k P_k x on the contiguous flat tensor x (dim d of the [2]*nq cube is memory bit nq - 1 - d): every letter is a
    3-dim view (above, 2, below) -- flip for X, a sign multiply for Z, both and a factor i for Y = i X Z."""
    sign = torch.tensor([1.0, -1.0], dtype=x.dtype, device=x.device).view(1, 2, 1)
    out = torch.zeros_like(x)
    for c, p in terms:
        v, phase = x, complex(c)
        for d, letter in p.items():
            v3 = v.view(2 ** d, 2, 2 ** (nq - 1 - d))
            if letter in "ZY":
                v3 = v3 * sign
            if letter in "XY":
                v3 = v3.flip(1)
            if letter == "Y":
                phase *= 1j
            v = v3.reshape(-1)
        out.add_(v, alpha=phase)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-budget-s", type=float, default=60.0)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    nq, reps = args.log2n, args.repeats
    n = 2 ** nq
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    cube = x.view((2,) * nq)                                  # dim d is memory bit nq - 1 - d
    out = torch.empty_like(cube)
    rng = np.random.default_rng(1)
    rows, spent = [], [0.0]

    def fraction(info, ms):
        return (info["bytes_read"] + info["bytes_written"]) / (ms * 1e-3) / (READ_PROBE_TBS * 1e12)

    def native(name, terms, compare=False):
        info = A.pauli_apply_info(cube.shape, cube.stride(), terms)
        med, lo, hi, extra = timed(lambda: A.pauli_sum_apply(cube, terms), reps)
        op = A.PauliSumOperator(cube.shape, cube.stride(), cube.dtype, terms, DEV)
        op_med, op_lo, op_hi, op_extra = timed(lambda: op(cube, out=out), reps)
        row = {"name": name, "terms": len(terms), "groups": info["n_groups"], "xmask_hi": info["n_xmask_hi"], "launches": info["n_launches"],
               "table_bytes": info["table_bytes"], "bytes_read": info["bytes_read"], "bytes_written": info["bytes_written"],
               "ms_median": med, "ms_min": lo, "ms_max": hi, "fraction_of_read_probe": fraction(info, med), "extra_bytes": extra,
               "operator_ms_median": op_med, "operator_ms_min": op_lo, "operator_ms_max": op_hi,
               "operator_fraction_of_read_probe": fraction(info, op_med), "operator_extra_bytes": op_extra}
        print(f"{name:52s} {med:9.3f} ms [{lo:.3f}, {hi:.3f}] {row['fraction_of_read_probe']:6.1%};  prebuilt operator, out given "
              f"{op_med:9.3f} ms {row['operator_fraction_of_read_probe']:6.1%}", flush=True)
        if compare:
            strings = [p for _, p in terms]
            pinfo = A.pauli_info(cube.shape, cube.stride(), strings)
            emed, elo, ehi, eextra = timed(lambda: A.pauli_sum_expectation(cube, terms), reps)
            row["expectation"] = {"ms_median": emed, "ms_min": elo, "ms_max": ehi, "launches": pinfo["n_launches"],
                                  "bytes_read": pinfo["bytes_read"], "extra_bytes": eextra}
            print(f"    pauli_sum_expectation, {pinfo['n_launches']} passes: {emed:9.3f} ms [{elo:.3f}, {ehi:.3f}]", flush=True)
            row["torch"] = torch_row(terms)
            print(f"    torch: {row['torch']}", flush=True)
        rows.append(row)

    def torch_row(terms):
        """ONE warm-up call and up to three timed calls on the wall clock; no further torch call once the budget is spent."""
        if spent[0] > args.torch_budget_s:
            return {"status": "not run: time budget"}
        try:
            t0 = time.perf_counter()
            ref = torch_apply(x, terms, nq)
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            spent[0] += first
            diff = float((ref - A.pauli_sum_apply(cube, terms).reshape(-1)).abs().max())
            del ref
            ms = []
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            while len(ms) < 3 and spent[0] <= args.torch_budget_s:
                t0 = time.perf_counter()
                torch_apply(x, terms, nq)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                spent[0] += ms[-1] * 1e-3
            extra = torch.cuda.max_memory_allocated() - before
            return {"status": "run", "first_call_ms": first * 1e3, "ms": ms, "ms_median": float(np.median(ms)) if ms else None,
                    "extra_bytes": extra, "max_abs_diff_to_native": diff}
        except Exception as e:  # torch may refuse a shape
            torch.cuda.empty_cache()
            return {"status": f"refused: {type(e).__name__}: {str(e)[:160]}"}

    def zz(q):
        return {q: "Z", q + 1: "Z"}

    mixed = {d: str(rng.choice(list("XYZ"))) for d in range(nq)}
    native("one Z string  Z_3 Z_17", [(1.0, {3: "Z", 17: "Z"})])
    native("one X inside the tile (memory bit 3)", [(1.0, {nq - 1 - 3: "X"})])
    native("one X on the slowest bit (X_0)", [(1.0, {0: "X"})])
    native(f"one weight-{nq} mixed string", [(1.0, mixed)])
    tfim = [(-1.0, zz(q)) for q in range(nq - 1)] + [(-0.7, {q: "X"}) for q in range(nq)]
    native(f"transverse-field Ising sum ({len(tfim)} terms)", tfim, compare=True)
    heis = [(0.25, {q: letter, q + 1: letter}) for q in range(nq - 1) for letter in "XYZ"]
    native(f"Heisenberg chain XX + YY + ZZ on {nq - 1} bonds ({len(heis)} terms)", heis, compare=True)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernel + torch plumbing); torch rows: "
           "wall clock around the call and a synchronisation", "read_probe_TBps": READ_PROBE_TBS, "clocks": clocks(),
           "device_memory_free_bytes": free, "device_memory_total_bytes": total, "torch_budget_s": args.torch_budget_s,
           "mixed_string": "".join(mixed[d] for d in range(nq)), "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "pauli_apply_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    gib = 2.0 ** 30
    with open(os.path.join(args.out_dir, "pauli_apply_timing.md"), "w") as f:
        f.write(f"# y = H a on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call.  `pauli_sum_apply` packs and uploads "
                "the term table and allocates y in every call; the operator columns time a prebuilt `PauliSumOperator` writing into a "
                f"given `out`.  Fraction = (bytes read + bytes written) / time / {READ_PROBE_TBS} TB/s (tools/probes/read_probe.hip) with "
                f"the nominal bytes of the info call: {rows[0]['bytes_read'] / gib:.0f} GiB read + {rows[0]['bytes_written'] / gib:.0f} GiB "
                "written per call, whatever the number of groups -- partner tiles count as part of the one reading of `a`, so a row "
                "whose partner tiles miss the caches moves more bytes than its fraction says.\n\n")
        f.write("| call | terms | groups | distinct xm_hi | median ms | min..max ms | fraction | extra device memory | operator median ms | "
                "operator min..max ms | operator fraction | operator extra memory |\n|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r['name']} | {r['terms']} | {r['groups']} | {r['xmask_hi']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                    f"{r['fraction_of_read_probe']:.1%} | {r['extra_bytes'] / 2 ** 20:.2f} MiB | {r['operator_ms_median']:.3f} | "
                    f"{r['operator_ms_min']:.3f}..{r['operator_ms_max']:.3f} | {r['operator_fraction_of_read_probe']:.1%} | "
                    f"{r['operator_extra_bytes'] / 2 ** 20:.2f} MiB |\n")
        f.write("\nThe same terms by the two other routes, same process:\n\n| Hamiltonian | route | passes over the state | median ms | min..max ms | "
                "extra device memory |\n|---|---|---:|---:|---:|---:|\n")
        for r in rows:
            if "expectation" not in r:
                continue
            e, t = r["expectation"], r["torch"]
            f.write(f"| {r['name']} | `pauli_sum_expectation` (a number, not a state) | {e['launches']} | {e['ms_median']:.3f} | "
                    f"{e['ms_min']:.3f}..{e['ms_max']:.3f} | {e['extra_bytes'] / 2 ** 20:.2f} MiB |\n")
            if t["status"] == "run" and t["ms"]:
                f.write(f"| {r['name']} | torch flip / multiply / add per term (wall clock, {len(t['ms'])} calls; max abs difference to the "
                        f"native result {t['max_abs_diff_to_native']:.2e}) | - | {t['ms_median']:.1f} | {min(t['ms']):.1f}..{max(t['ms']):.1f} | "
                        f"{t['extra_bytes'] / 2 ** 20:.0f} MiB |\n")
            else:
                f.write(f"| {r['name']} | torch flip / multiply / add per term | - | {t['status']} | - | - |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
