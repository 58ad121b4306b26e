"""Times the Krylov vector algebra (A.krylov_dots, A.krylov_combine_) and one fully re-orthogonalised Lanczos iteration on
2^30-element complex64 vectors of random data, next to the torch formulation of the same iteration (torch.vdot / torch.add(alpha=) /
torch.linalg.vector_norm) measured in the same process.  HIP events around the whole call, two warm-up calls, the median of
REPEATS timed calls; TB/s = the nominal bytes of the info call / time.

A row needs its vectors to be distinct allocations (repeating one pointer would be served from the caches): m = 32 needs 33 vectors
of 8 GiB.  A row whose vectors do not fit runs at half the size and says so.

    python tools/time_krylov.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes krylov_timing.json and krylov_timing.md into --out-dir."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from artensor_amd import _native  # noqa: E402
from time_born import DEV, READ_PROBE_TBS, clocks, timed  # noqa: E402

B = _native.KRYLOV_BATCH


def ising(nq):
    return [(-1.0, {q: "Z", q + 1: "Z"}) for q in range(nq - 1)] + [(-0.7, {q: "X"}) for q in range(nq)]


def make_vectors(count, nq):
    """`count` random [2] * nq complex64 tensors of norm about 1, or None when they do not fit."""
    g = torch.Generator(device=DEV)
    g.manual_seed(count)
    try:
        free, _ = torch.cuda.mem_get_info()
        if (count + 3) * 8 * 2 ** nq > free:                   # (three more: the torch route's temporaries)
            return None
        return [torch.view_as_complex(torch.randn(2 ** nq, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2)).view((2,) * nq)
                for _ in range(count)]
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def torch_iteration(op, basis, w):
    """One fully re-orthogonalised step by torch: the dots one by one, each subtraction its own pass, the norm, the division."""
    op(basis[-1], out=w)
    h = [torch.vdot(v.reshape(-1), w.reshape(-1)) for v in basis]
    for c, v in zip(h, basis):
        w = torch.add(w, v, alpha=-complex(c))
    beta = torch.linalg.vector_norm(w)
    return w / beta


def native_iteration(op, basis, w):
    op(basis[-1], out=w)
    h, _ = A.krylov_dots(basis, w)
    n2 = A.krylov_combine_(w, [1.0] + list(-h), [w] + basis)
    A.krylov_combine_(w, [1.0 / math.sqrt(n2)], [w])
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    reps = args.repeats
    rows, iters = [], []

    def with_vectors(count, fn):
        for nq in (args.log2n, args.log2n - 1):
            vs = make_vectors(count, nq)
            if vs is not None:
                fn(vs, nq)
                del vs
                torch.cuda.empty_cache()
                return
        rows.append({"name": f"{count} vectors", "status": "not run: the vectors do not fit at either size"})

    for m in (1, 3, B, B + 1, 32):
        def run(vs, nq, m=m):
            w, xs = vs[-1], vs[:-1]
            info = A.krylov_info(w.shape, w.stride(), m)
            med, lo, hi, extra = timed(lambda: A.krylov_dots(xs, w, device=True), reps)
            rows.append({"name": f"krylov_dots, m = {m}", "m": m, "log2n": nq, "launches": info["dots_launches"], "bytes": info["dots_bytes_read"],
                         "ms_median": med, "ms_min": lo, "ms_max": hi, "TBps": info["dots_bytes_read"] / med / 1e9, "extra_bytes": extra})
            print(rows[-1], flush=True)
            y = w
            c = [0.3 + 0.1j * (j + 1) for j in range(m)]
            nbytes = info["combine_bytes_read"] + info["combine_bytes_written"]
            med, lo, hi, extra = timed(lambda: A.krylov_combine_(y, c, xs, device=True), reps)
            rows.append({"name": f"krylov_combine_, m = {m}", "m": m, "log2n": nq, "launches": 1, "bytes": nbytes, "ms_median": med,
                         "ms_min": lo, "ms_max": hi, "TBps": nbytes / med / 1e9, "extra_bytes": extra})
            print(rows[-1], flush=True)
        with_vectors(m + 1, run)

    for j in (10, 30):
        def run(vs, nq, j=j):
            terms = ising(nq)
            w, basis = vs[-1], vs[:-1]
            op = A.PauliSumOperator(w.shape, w.stride(), w.dtype, terms, DEV)
            med, lo, hi, extra = timed(lambda: op(basis[-1], out=w), reps)
            row = {"name": f"Lanczos iteration j = {j}, full re-orthogonalisation ({j + 1} vectors)", "j": j, "log2n": nq,
                   "apply_ms_median": med}
            med, lo, hi, extra = timed(lambda: native_iteration(op, basis, w), reps)
            row.update({"ms_median": med, "ms_min": lo, "ms_max": hi, "extra_bytes": extra})
            try:
                med, lo, hi, extra = timed(lambda: torch_iteration(op, basis, w), max(3, reps // 3), warmup=1)
                row["torch"] = {"status": "run", "ms_median": med, "ms_min": lo, "ms_max": hi, "extra_bytes": extra}
            except torch.OutOfMemoryError as e:
                torch.cuda.empty_cache()
                row["torch"] = {"status": f"not run: {str(e)[:120]}"}
            iters.append(row)
            print(row, flush=True)
        with_vectors(j + 2, run)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": args.log2n, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "batch": B, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing, and "
           "for the iteration rows the host synchronisations that fetch the dots and the norm)", "read_probe_TBps": READ_PROBE_TBS,
           "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total, "rows": rows, "iterations": iters}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "krylov_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "krylov_timing.md"), "w") as f:
        f.write(f"# Krylov vector algebra on complex64 vectors ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process.  Bytes are the nominal ones "
                f"of `krylov_info`: dots read m + ceil(m / {B}) vectors, a combination reads m and writes one.  Every vector is its own "
                "allocation; a row at 2^(n-1) elements did not fit at 2^n.\n\n")
        f.write("| call | log2 elements | streaming launches | GiB moved | median ms | min..max ms | TB/s | extra device memory |\n"
                "|---|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            if "status" in r:
                f.write(f"| {r['name']} | - | - | - | {r['status']} | - | - | - |\n")
                continue
            f.write(f"| {r['name']} | {r['log2n']} | {r['launches']} | {r['bytes'] / 2 ** 30:.0f} | {r['ms_median']:.3f} | "
                    f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['TBps']:.2f} | {r['extra_bytes'] / 2 ** 20:.2f} MiB |\n")
        f.write("\nOne Lanczos iteration on the Ising chain (apply, dots against the basis, one combination with y = w, the scale pass) and "
                "the same work by torch.vdot / torch.add(alpha=) / torch.linalg.vector_norm / a division:\n\n"
                "| iteration | log2 elements | apply alone ms | native median ms | min..max ms | native extra memory | torch median ms | "
                "torch min..max ms | torch extra memory |\n|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in iters:
            t = r["torch"]
            tail = (f"{t['ms_median']:.1f} | {t['ms_min']:.1f}..{t['ms_max']:.1f} | {t['extra_bytes'] / 2 ** 30:.1f} GiB" if t["status"] == "run"
                    else f"{t['status']} | - | -")
            f.write(f"| {r['name']} | {r['log2n']} | {r['apply_ms_median']:.3f} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                    f"{r['extra_bytes'] / 2 ** 20:.2f} MiB | {tail} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows), "iterations": len(iters)}))


if __name__ == "__main__":
    main()
