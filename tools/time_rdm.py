"""Times reduced density matrices on a 2^30-element complex64 tensor of random data (and one complex128 case at 2^29) against the
torch formulation they replace, in one process: HIP events around the whole call, two warm-up calls, the median of REPEATS timed
calls (torch: ONE call on the wall clock, within a time budget), the peak extra device memory of one call, and the time as a
fraction of

    max(bytes read / 7.2 TB/s, FLOP on the matrix cores / 46 TFLOP/s)

(tools/probes/read_probe.hip; tools/probes/f64_mfma_probe.hip measured 45-47.5 TFLOP/s for v_mfma_f64_16x16x4_f64).

    python tools/time_rdm.py [--log2n 30] [--repeats 10] [--torch-budget-s 240] [--out-dir profiles]

writes rdm_timing.json and rdm_timing.md into --out-dir."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from artensor_amd import rdm  # noqa: E402

READ_PROBE_TBS = 7.2
F64_MFMA_TFLOPS = 46.0
DEV = "cuda:0"


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), extra


def positions(k, nq):
    mixed = [nq // 2] if k == 1 else sorted({(i * (nq - 1)) // (k - 1) for i in range(k)})
    return {"fastest": list(range(nq - k, nq)), "slowest": list(range(k)), "mixed": mixed}


def torch_rdm(t, keep):
    """permute + reshape + to(complex128) + matmul on a contiguous [2]*n tensor with ascending `keep`.  torch copies at most 16
    dims, so runs of adjacent kept and of adjacent dropped dims are merged first (a view); more than 16 runs: RuntimeError."""
    shape, kept_pos = [], []
    for d in range(t.dim()):
        if shape and (d in keep) == ((d - 1) in keep):
            shape[-1] *= 2
        else:
            shape.append(2)
            if d in keep:
                kept_pos.append(len(shape) - 1)
    rest = [i for i in range(len(shape)) if i not in kept_pos]
    m = t.reshape(shape).permute(kept_pos + rest).reshape(2 ** len(keep), -1).to(torch.complex128)
    return m @ m.mH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-budget-s", type=float, default=240.0)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    nq, reps = args.log2n, args.repeats
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    rows = []

    def run(label, t, keep, elem_bytes):
        n = t.numel()
        info = rdm.rdm_info(t.shape, t.stride(), keep, t.dtype)
        med, lo, hi, extra = timed(lambda: A.reduced_density_matrix(t, keep), reps)
        bound_ms = max(n * elem_bytes / (READ_PROBE_TBS * 1e12), info["flops"] / (F64_MFMA_TFLOPS * 1e12)) * 1e3
        row = {"name": label, "dtype": str(t.dtype), "log2_elements": n.bit_length() - 1, "keep": keep, "info": info, "ms_median": med,
               "ms_min": lo, "ms_max": hi, "extra_bytes": extra, "bound_ms": bound_ms, "bound_is": "read" if
               n * elem_bytes / (READ_PROBE_TBS * 1e12) >= info["flops"] / (F64_MFMA_TFLOPS * 1e12) else "mfma",
               "fraction_of_bound": bound_ms / med}
        row.update({"torch": "not run", "torch_ms": None, "torch_extra_bytes": None, "max_abs_diff_over_trace": None})
        rows.append(row)
        print(f"{label:34s} {med:9.3f} ms [{lo:.3f}, {hi:.3f}]  bound {bound_ms:8.3f} ms ({row['bound_is']}) -> {row['fraction_of_bound']:6.1%}  "
              f"extra {extra / 2 ** 20:8.2f} MiB", flush=True)
        write(rows)

    def run_torch(row, t):
        """ONE call of the torch formulation (a complex128 matmul with two rows takes a minute): its time includes whatever the
        BLAS library does on a first call of a shape.  Stops being run once the budget is spent."""
        if spent[0] > args.torch_budget_s:
            row["torch"] = "not run: time budget"
            return
        keep = row["keep"]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before, t0 = torch.cuda.memory_allocated(), time.perf_counter()
        try:
            want = torch_rdm(t, keep)
            torch.cuda.synchronize()
            row["torch_ms"] = (time.perf_counter() - t0) * 1e3
            row["torch_extra_bytes"] = torch.cuda.max_memory_allocated() - before
            got = A.reduced_density_matrix(t, keep)
            row["max_abs_diff_over_trace"] = float((got - want).abs().max() / want.diagonal().real.sum())
            row["torch"] = "ok"
            del got, want
        except torch.cuda.OutOfMemoryError:
            row["torch"] = "out of memory"
        except RuntimeError as e:
            if "too many" not in str(e):
                raise
            row["torch"] = "refused: more than 16 dims"
        spent[0] += time.perf_counter() - t0
        torch.cuda.empty_cache()
        print(f"torch, {row['name']:34s} {row['torch']}: {row['torch_ms']} ms, {row['torch_extra_bytes']} B", flush=True)
        write(rows)

    def write(rows):
        free, total = torch.cuda.mem_get_info()
        doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "repeats": reps, "warmup": 2,
               "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing); torch rows: one call, wall clock",
               "read_probe_TBps": READ_PROBE_TBS, "f64_mfma_TFLOPs": F64_MFMA_TFLOPS, "device_memory_free_bytes": free,
               "device_memory_total_bytes": total, "rows": rows}
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "rdm_timing.json"), "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(args.out_dir, "rdm_timing.md"), "w") as f:
            f.write(f"# Reduced density matrices of random amplitudes ({doc['device']})\n\n")
            f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call; extra memory = peak device memory of "
                    f"one call above what was allocated before it; bound = max(bytes read / {READ_PROBE_TBS} TB/s, matrix-core FLOP / "
                    f"{F64_MFMA_TFLOPS} TFLOP/s), fraction = bound / time.  torch = permute + reshape + to(complex128) + matmul, ONE call "
                    f"(wall clock; no further torch call once {args.torch_budget_s} s have gone into them).\n\n")
            f.write("| case | tiles x splits | median ms | min..max ms | bound ms | fraction | extra memory | torch ms | torch memory |\n"
                    "|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
            for r in rows:
                tt = f"{r['torch_ms']:.1f} | {r['torch_extra_bytes'] / 2 ** 30:.1f} GiB" if r["torch"] == "ok" else f"{r['torch']} | -"
                f.write(f"| {r['name']} | {r['info']['tiles']} x {r['info']['splits']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                        f"{r['bound_ms']:.2f} ({r['bound_is']}) | {r['fraction_of_bound']:.1%} | {r['extra_bytes'] / 2 ** 20:.1f} MiB | {tt} |\n")
            f.write(f"\nDevice memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")

    spent = [0.0]
    x = torch.view_as_complex(torch.randn(2 ** nq, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2)).view((2,) * nq)
    for k in (1, 4, 6, 8, 10):
        for where, keep in positions(k, nq).items():
            run(f"complex64 2^{nq}, k={k} {where}", x, keep, 8)
    for row in sorted(rows, key=lambda r: -len(r["keep"])):      # the larger matrices first: BLAS is at its best there
        run_torch(row, x)
    del x
    torch.cuda.empty_cache()
    nz = nq - 1
    z = torch.view_as_complex(torch.randn(2 ** nz, 2, device=DEV, generator=g, dtype=torch.float64) * 2.0 ** (-(nz + 1) / 2)).view((2,) * nz)
    run(f"complex128 2^{nz}, k=6 mixed", z, positions(6, nz)["mixed"], 16)
    run_torch(rows[-1], z)
    del z

    write(rows)
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
