"""Times the matrix-core gates (A.MatrixGate: one launch per gate) on 2^30 complex64 amplitudes, in ONE process: one dense gate
of k = 3..7 with its targets all low, all in memory bits 2-9, all at or above the tile and mixed, on random data; A.WideGate for
k = 3..5 on the same targets; then the n30 circuit of tests/golden/n30_gates.npz from |0..0> through fuse_gates_wide(w) +
BlockCircuit(max_rank 0) for w = 4..7 at mfma_from 3 and 6, next to fuse_gates(4) + FusedCircuit.  HIP events around the whole
call, two warm-up calls, the median of REPEATS timed calls, prebuilt objects.

Per single-gate row the bound max(16 GiB / COPY_RATE, 8 * 2^k * 2^30 / MFMA_RATE) and the fraction of it reached.  COPY_RATE is
the tile-structured copy probe's traffic rate (read + write: 8 GiB in 3.66 ms), MFMA_RATE what tools/probes/f64_mfma_probe.hip
reaches; both are measurements of the README, not of this run.

    python tools/time_matrix_gates.py [--repeats 10] [--out-dir profiles]

writes matrix_gates_timing.json and matrix_gates_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from artensor_amd.fixtures import load_case  # noqa: E402
from time_born import DEV, clocks, timed  # noqa: E402
from time_gates import amp_rel  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
COPY_RATE = 2 * 2.35e12                                        # bytes of traffic per second (README: the copy probe)
MFMA_RATE = 46e12                                              # float64 FLOP per second (README: the f64 MFMA probe, 45-47.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out-dir", default="profiles")
    args = ap.parse_args()
    nq, reps = 30, args.repeats
    n = 2 ** nq
    singles, circuits = [], []

    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    cube = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2)).view((2,) * nq)
    rng = np.random.default_rng(1)

    def unitary(dim):
        q, r = np.linalg.qr(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim)))
        return q * (np.diag(r) / np.abs(np.diag(r)))

    bit = lambda b: nq - 1 - b                                # dim of memory bit b
    places = {"low": [0, 1, 2, 3, 4, 5, 6], "bits 2-9": [3, 5, 8, 6, 9, 2, 7], "at or above the tile": [20, 29, 14, 25, 17, 22, 27],
              "mixed": [0, 29, 7, 13, 3, 21, 10]}
    for k in (3, 4, 5, 6, 7):
        for place, bits in places.items():
            m = unitary(2 ** k)
            dims = tuple(bit(b) for b in bits[:k])
            row = {"k": k, "targets": place, "bits": bits[:k]}
            floor = max(2 * n * 8 / COPY_RATE, 8 * 2 ** k * n / MFMA_RATE) * 1e3
            for name, make in (("matrix", A.MatrixGate), ("wide", A.WideGate)):
                if name == "wide" and k > 5:
                    row["wide_ms_median"] = None
                    continue
                gate = make(cube.shape, cube.stride(), cube.dtype, m, dims, DEV)
                med, lo, hi, extra = timed(lambda: gate(cube), reps)
                row.update({f"{name}_ms_median": med, f"{name}_ms_min": lo, f"{name}_ms_max": hi, f"{name}_extra_bytes": extra})
            row.update({"bound_ms": floor, "fraction_of_bound": floor / row["matrix_ms_median"],
                        "tflops": 8 * 2 ** k * n / (row["matrix_ms_median"] * 1e-3) / 1e12})
            singles.append(row)
            print(json.dumps(row), flush=True)
    del cube
    torch.cuda.empty_cache()

    g30 = load_case(os.path.join(GOLDEN, "n30_gates.npz"))
    bonds = [(g30.tensors[k], g30.meta["inds"][k]) for k in range(len(g30.meta["inds"]))]
    gates = A.gates_from_bonds(bonds, nq)
    case = load_case(os.path.join(GOLDEN, "n30_dense.npz"))
    strings = case.meta["google_bitstrings"]
    truth = np.load(os.path.join(GOLDEN, "c128_truth_gpu.npz"))["n30_dense_at_google"].reshape(-1)
    rms = 2.0 ** -15

    def at_google(t):
        flat = t.as_strided((n,), (1,), t.storage_offset())
        st = t.stride()
        pos = torch.tensor([sum(int(c) * st[q] for q, c in enumerate(b)) for b in strings], device=DEV)
        return flat[pos].cpu().numpy()

    state = torch.zeros(n, dtype=torch.complex64, device=DEV).view((2,) * nq)
    routes = [("fuse_gates(4) + FusedCircuit  [comparison]", A.fuse_gates(gates, 4),
               lambda gl: A.FusedCircuit(state.shape, state.stride(), state.dtype, gl, DEV, 0))]
    for w in (4, 5, 6, 7):
        for mf in (3, 6):
            routes.append((f"fuse_gates_wide({w}) + BlockCircuit(mfma_from={mf})", A.fuse_gates_wide(gates, w),
                           lambda gl, mf=mf: A.BlockCircuit(state.shape, state.stride(), state.dtype, gl, DEV, 0, mf)))
    for name, glist, make in routes:
        circ = make(glist)

        def call():
            state.zero_()
            state.view(-1)[0] = 1
            circ(state)
        med, lo, hi, extra = timed(call, reps)
        widths = [sum(len(d) == w for _, d in glist) for w in range(1, 8)]
        circuits.append({"route": name, "gates": len(glist), "gates_by_width": widths, "launches": circ.n_launches,
                         "matrix_gates": getattr(circ, "n_matrix", 0), "ms_median": med, "ms_min": lo, "ms_max": hi,
                         "extra_bytes": extra, "amp_rel_at_google": amp_rel(at_google(state), truth, rms)})
        print(json.dumps(circuits[-1]), flush=True)
        del circ

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "copy_rate_bytes_per_s": COPY_RATE, "mfma_rate_flop_per_s": MFMA_RATE, "complex128": "unmeasured",
           "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total, "single_gates": singles,
           "n30_circuit": circuits}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "matrix_gates_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "matrix_gates_timing.md"), "w") as f:
        f.write(f"# Matrix-core gates on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, prebuilt objects, one process.  "
                "bound = max(16 GiB / the copy probe's rate, 8 * 2^k * 2^30 FLOP / the f64 MFMA probe's rate); complex128: unmeasured.\n\n")
        f.write("| k | targets (memory bits) | MatrixGate median ms | min..max ms | TFLOP/s | bound ms | bound / time | WideGate median ms |\n"
                "|---:|---|---:|---:|---:|---:|---:|---:|\n")
        for r in singles:
            wide = "-" if r["wide_ms_median"] is None else f"{r['wide_ms_median']:.3f}"
            f.write(f"| {r['k']} | {r['targets']} {r['bits']} | {r['matrix_ms_median']:.3f} | {r['matrix_ms_min']:.3f}..{r['matrix_ms_max']:.3f} | "
                    f"{r['tflops']:.1f} | {r['bound_ms']:.2f} | {r['fraction_of_bound']:.2f} | {wide} |\n")
        f.write("\nThe n30 circuit from |0..0> (the reset is inside the timed call; max_rank 0); amp_rel: the result at Google's 10 000 "
                "bitstrings against the complex128 truth of the tensor-network amplitudes.\n\n")
        f.write("| route | gates (of width 1..7) | launches | on the matrix cores | median ms | min..max ms | amp_rel |\n|---|---:|---:|---:|---:|---:|---:|\n")
        for r in circuits:
            f.write(f"| {r['route']} | {r['gates']} {r['gates_by_width']} | {r['launches']} | {r['matrix_gates']} | {r['ms_median']:.3f} | "
                    f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['amp_rel_at_google']:.2e} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"single_gates": len(singles), "circuits": len(circuits)}))


if __name__ == "__main__":
    main()
