"""Times the wide gates (A.WideGate: one launch per gate) on 2^30 complex64 amplitudes: one gate of k = 3, 4, 5, dense and
diagonal, with its targets all low, all in memory bits 2-9, all at or above the tile and mixed, on random data; then the n30
circuit of tests/golden/n30_gates.npz from |0..0> through A.FusedCircuit after fuse_gates at widths 2..5 (max_rank 0), next to the
comparison route merge_gates + GateCircuit(max_rank=0) measured in the same process.  HIP events around the whole call, two
warm-up calls, the median of REPEATS timed calls (the circuit rows reset the state inside the timed region); extra device memory =
the peak above what is allocated before the call.  Per single-gate row the float64 fma per amplitude of the arithmetic contract,
4 * 2^k (a diagonal matrix: 4), and the fma rate they imply.

    python tools/time_wide_gates.py [--repeats 10] [--out-dir profiles]

writes wide_gates_timing.json and wide_gates_timing.md into --out-dir."""
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
    places = {"low": [0, 1, 2, 3, 4], "bits 2-9": [3, 5, 8, 6, 9], "at or above the tile": [20, 29, 14, 25, 17], "mixed": [0, 29, 7, 13, 3]}
    for k in (3, 4, 5):
        for place, bits in places.items():
            for form in ("dense", "diagonal"):
                m = unitary(2 ** k)
                if form == "diagonal":
                    m = np.diag(np.diag(m))
                gate = A.WideGate(cube.shape, cube.stride(), cube.dtype, m, tuple(bit(b) for b in bits[:k]), DEV)
                med, lo, hi, extra = timed(lambda: gate(cube), reps)
                fma = 4 * 2 ** k if form == "dense" else 4
                rate = fma * n / (med * 1e-3) / 1e12
                singles.append({"k": k, "targets": place, "bits": bits[:k], "form": form, "ms_median": med, "ms_min": lo, "ms_max": hi,
                                "extra_bytes": extra, "fma_per_amplitude": fma, "tera_fma_per_s": rate,
                                "gb_per_s": 2 * n * 8 / (med * 1e-3) / 1e9})
                print(f"k {k} {place:22s} {form:9s} {med:9.3f} ms [{lo:.3f}, {hi:.3f}] {fma:4d} fma/amp {rate:7.3f} Tfma/s", flush=True)
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
    routes = [("merge_gates + GateCircuit(max_rank=0)  [comparison]", A.merge_gates(gates), A.GateCircuit)]
    routes += [(f"fuse_gates(width {w}) + FusedCircuit(max_rank=0)", A.fuse_gates(gates, w), A.FusedCircuit) for w in (2, 3, 4, 5)]
    for name, glist, make in routes:
        circ = make(state.shape, state.stride(), state.dtype, glist, DEV, 0)

        def call():
            state.zero_()
            state.view(-1)[0] = 1
            circ(state)
        med, lo, hi, extra = timed(call, reps)
        launches = circ.n_launches if hasattr(circ, "n_launches") else circ.n_runs
        widths = [sum(len(d) == w for _, d in glist) for w in range(1, 6)]
        circuits.append({"route": name, "gates": len(glist), "gates_by_width": widths, "launches": launches, "ms_median": med,
                         "ms_min": lo, "ms_max": hi, "extra_bytes": extra, "amp_rel_at_google": amp_rel(at_google(state), truth, rms)})
        print(f"{name:56s} gates {len(glist):4d} {widths} launches {launches:4d} {med:9.3f} ms [{lo:.3f}, {hi:.3f}] "
              f"extra {extra / 2 ** 20:.2f} MiB amp_rel {circuits[-1]['amp_rel_at_google']:.2e}", flush=True)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total, "single_gates": singles,
           "n30_circuit": circuits}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "wide_gates_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "wide_gates_timing.md"), "w") as f:
        f.write(f"# Wide gates on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, prebuilt objects, one process.  "
                "fma per amplitude: the float64 fma of the arithmetic contract, 4 * 2^k (4 for a diagonal matrix); the rate is that "
                "count times 2^30 over the median time.\n\n")
        f.write("| k | targets (memory bits) | matrix | median ms | min..max ms | GB/s (read + write) | fma / amplitude | Tfma/s |\n"
                "|---:|---|---|---:|---:|---:|---:|---:|\n")
        for r in singles:
            f.write(f"| {r['k']} | {r['targets']} {r['bits']} | {r['form']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                    f"{r['gb_per_s']:.0f} | {r['fma_per_amplitude']} | {r['tera_fma_per_s']:.2f} |\n")
        f.write("\nThe n30 circuit from |0..0> (the reset is inside the timed call); amp_rel: the result at Google's 10 000 bitstrings "
                "against the complex128 truth of the tensor-network amplitudes.\n\n")
        f.write("| route | gates (of width 1..5) | launches | median ms | min..max ms | extra device memory | amp_rel |\n"
                "|---|---:|---:|---:|---:|---:|---:|\n")
        for r in circuits:
            f.write(f"| {r['route']} | {r['gates']} {r['gates_by_width']} | {r['launches']} | {r['ms_median']:.3f} | "
                    f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['extra_bytes'] / 2 ** 20:.2f} MiB | {r['amp_rel_at_google']:.2e} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"single_gates": len(singles), "circuits": len(circuits)}))


if __name__ == "__main__":
    main()
