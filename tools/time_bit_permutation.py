"""Times the in-place bit permutations (A.BitPermutation: one launch per pass) on 2^30 complex64 amplitudes: one transposition
with both bits below a 128-byte line, one low and one high bit, two high bits; a cycle on 8 high bits (one pass); the 30-bit
reversal; the 30-bit rotation by one; relayout_ to contiguous of a state whose 30 dims lie in memory in a seeded random order (the
shape of a permuted contraction result).  Next to each row the parent's routes, timed in the same process: the chain of SWAP gates
(A.GateCircuit, one SWAP per transposition of the cycles) and .contiguous() of the permuted view where torch can copy it -- its
copy takes at most 16 merged dims and crawls well before that, so it is timed up to 8 merged dims and otherwise recorded as
refused -- with its second buffer.  The yardstick of one pass is the project's copy probe of the same state, 3.66 ms.

Then one experiment: the n30 circuit of tests/golden/n30_gates.npz after merge_gates, from |0..0>, as it is and after
relayout_(state, busiest_dims_order(gates, 30)) with the relayout inside the timed call.

HIP events around the whole call, two warm-up calls, the median of REPEATS timed calls, prebuilt objects, one process.

    python tools/time_bit_permutation.py [--repeats 10] [--out-dir profiles]

writes bit_permutation_timing.json and bit_permutation_timing.md into --out-dir."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden")
COPY_PROBE_MS = 3.66                                          # README, measurement section: a copy of 2^30 complex64
SWAP = np.eye(4)[[0, 2, 1, 3]]


def cycles_of(dst):
    seen, out = set(), []
    for b in range(len(dst)):
        c = []
        while b not in seen and dst[b] != b:
            seen.add(b)
            c.append(b)
            b = dst[b]
        if c:
            out.append(c)
    return out


def merged_dims(perm):
    """Dims of x.permute(perm) of a contiguous x after merging runs of adjacent dims."""
    return 1 + sum(1 for a, b in zip(perm, perm[1:]) if b != a + 1)


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
    dim = lambda b: nq - 1 - b                                # dim of memory bit b of the contiguous cube
    ident = list(range(nq))

    def swap_bits(x, y):
        d = list(ident)
        d[x], d[y] = y, x
        return d
    cyc8 = list(ident)
    for b in range(22, 30):
        cyc8[b] = 22 + (b - 22 + 1) % 8
    cases = [("transposition, bits 0 and 2 (low / low)", swap_bits(0, 2)),
             ("transposition, bits 1 and 29 (low / high)", swap_bits(1, 29)),
             ("transposition, bits 20 and 29 (high / high)", swap_bits(20, 29)),
             ("cycle on the 8 bits 22..29", cyc8),
             ("reversal of all 30 bits", [nq - 1 - b for b in range(nq)]),
             ("rotation by one of all 30 bits", [(b + 1) % nq for b in range(nq)])]
    rows = []
    for name, dst in cases:
        info = A.bit_permutation_info(cube.shape, cube.stride(), cube.dtype, dst_bit=dst)
        p = A.BitPermutation(cube.shape, cube.stride(), cube.dtype, dst_bit=dst, device=DEV)
        med, lo, hi, extra = timed(lambda: p(cube), reps)
        row = {"name": name, "passes": info["passes"], "moved_high": info["moved_high"],
               "load_degree": [q["load_degree"] for q in info["pass_info"]], "store_degree": [q["store_degree"] for q in info["pass_info"]],
               "ms_median": med, "ms_min": lo, "ms_max": hi, "extra_bytes": extra, "bytes_moved": info["bytes_moved"],
               "gb_per_s": info["bytes_moved"] / (med * 1e-3) / 1e9, "ratio_to_copy_probe_per_pass": med / info["passes"] / COPY_PROBE_MS}
        # the parent's routes: a chain of SWAP gates ...
        swaps = [(SWAP, (dim(c[0]), dim(x))) for c in cycles_of(dst) for x in c[1:]]
        chain = A.GateCircuit(cube.shape, cube.stride(), cube.dtype, swaps, DEV)
        cmed, clo, chi, cextra = timed(lambda: chain(cube), reps)
        row.update({"swap_gates": len(swaps), "swap_launches": chain.n_runs, "swap_ms_median": cmed, "swap_ms_min": clo, "swap_ms_max": chi})
        # ... and torch's copy of the permuted view: the new dim k of the cube is the old dim of the bit that moves to bit of dim k
        inv = [0] * nq
        for b, c in enumerate(dst):
            inv[c] = b
        perm = [dim(inv[dim(k)]) for k in range(nq)]
        runs = merged_dims(perm)
        if runs > 16:
            row["torch"] = f"refused: {runs} merged dims (at most 16)"
        elif runs > 8:
            row["torch"] = f"not timed: {runs} merged dims"
        else:
            tmed, tlo, thi, textra = timed(lambda: cube.permute(perm).contiguous(), reps)
            row.update({"torch": "contiguous()", "torch_ms_median": tmed, "torch_extra_bytes": textra})
        rows.append(row)
        print(json.dumps(row), flush=True)

    # relayout_ of a permuted layout: the dims in memory in a seeded random order
    order = [int(k) for k in np.random.default_rng(30).permutation(nq)]
    strides = [0] * nq
    for pos, k in enumerate(reversed(order)):
        strides[k] = 1 << pos
    permuted = torch.as_strided(cube, (2,) * nq, strides)
    info = A.bit_permutation_info(permuted.shape, permuted.stride(), cube.dtype, order=None)
    fwd = A.BitPermutation(permuted.shape, permuted.stride(), cube.dtype, order=ident, device=DEV)
    back = A.BitPermutation(cube.shape, cube.stride(), cube.dtype, order=order, device=DEV)   # contiguous -> the permuted layout again

    def there_and_back():
        back(fwd(permuted))
    med, lo, hi, extra = timed(there_and_back, reps)
    fmed = timed(lambda: fwd(permuted), reps)[0]                            # (the data no longer means anything: only time)
    rows.append({"name": "relayout_ to contiguous of 30 dims in a random memory order", "passes": info["passes"],
                 "moved_high": info["moved_high"], "load_degree": [q["load_degree"] for q in info["pass_info"]],
                 "store_degree": [q["store_degree"] for q in info["pass_info"]], "ms_median": fmed, "ms_min": None, "ms_max": None,
                 "there_and_back_ms_median": med, "there_and_back_passes": fwd.passes + back.passes, "extra_bytes": extra,
                 "bytes_moved": info["bytes_moved"], "gb_per_s": info["bytes_moved"] / (fmed * 1e-3) / 1e9,
                 "ratio_to_copy_probe_per_pass": fmed / info["passes"] / COPY_PROBE_MS,
                 "torch": f"refused: {1 + sum(1 for k in range(nq - 1) if strides[k] != 2 * strides[k + 1])} merged dims (at most 16)"})
    print(json.dumps(rows[-1]), flush=True)
    del cube, permuted
    torch.cuda.empty_cache()

    # ---- the experiment: the n30 circuit as it is, and with the busiest dims moved under the tile first
    g30 = load_case(os.path.join(GOLDEN, "n30_gates.npz"))
    bonds = [(g30.tensors[k], g30.meta["inds"][k]) for k in range(len(g30.meta["inds"]))]
    gates = A.merge_gates(A.gates_from_bonds(bonds, nq))
    state = torch.zeros(n, dtype=torch.complex64, device=DEV).view((2,) * nq)
    plain = A.GateCircuit(state.shape, state.stride(), state.dtype, gates, DEV)
    order = A.busiest_dims_order(gates, nq)
    move = A.BitPermutation(state.shape, state.stride(), state.dtype, order=order, device=DEV)
    moved_circ = A.GateCircuit(state.shape, move.new_strides, state.dtype, gates, DEV)

    def reset():
        state.zero_()
        state.view(-1)[0] = 1

    def as_it_is():
        reset()
        plain(state)

    def remapped():
        reset()
        moved_circ(move(state))
    experiment = {"gates": len(gates), "order": order}
    med, lo, hi, _ = timed(as_it_is, reps)
    experiment["as_it_is"] = {"launches": plain.n_runs, "ms_median": med, "ms_min": lo, "ms_max": hi}
    pos = torch.randint(0, 2, (4096, nq), generator=torch.Generator().manual_seed(2))
    weights = torch.tensor(state.stride())
    sample_plain = state.view(-1)[(pos * weights).sum(1).to(DEV)].cpu()
    med, lo, hi, _ = timed(remapped, reps)
    experiment["remapped"] = {"launches": moved_circ.n_runs, "relayout_passes": move.passes, "ms_median": med, "ms_min": lo, "ms_max": hi}
    sample_moved = state.view(-1)[(pos * torch.tensor(move.new_strides)).sum(1).to(DEV)].cpu()
    experiment["max_abs_difference_at_4096_indices"] = float((sample_plain - sample_moved).abs().max())
    experiment["relayout_alone_ms_median"] = timed(lambda: move(state), reps)[0]
    print(json.dumps(experiment), flush=True)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "copy_probe_ms": COPY_PROBE_MS, "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total,
           "rows": rows, "n30_experiment": experiment}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bit_permutation_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "bit_permutation_timing.md"), "w") as f:
        f.write(f"# In-place bit permutations on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, prebuilt objects, one process.  "
                f"h: moved bits at or above a 128-byte line.  Ratio: time per pass over the copy probe of the same state ({COPY_PROBE_MS} ms).  "
                "Degrees: the bank-conflict degree of the load / store phase of each pass under the bank model.\n\n")
        f.write("| permutation | h | passes | load / store degree | median ms | min..max ms | GB/s (nominal) | per pass / copy probe | "
                "SWAP chain: gates, launches, median ms | torch .contiguous() |\n|---|---:|---:|---|---:|---:|---:|---:|---|---|\n")
        for r in rows:
            span = f"{r['ms_min']:.3f}..{r['ms_max']:.3f}" if r["ms_min"] is not None else "-"
            chain = f"{r['swap_gates']}, {r['swap_launches']}, {r['swap_ms_median']:.3f}" if "swap_gates" in r else "-"
            tor = f"{r['torch_ms_median']:.3f} ms, {r['torch_extra_bytes'] / 2 ** 30:.1f} GiB more" if "torch_ms_median" in r else r["torch"]
            f.write(f"| {r['name']} | {r['moved_high']} | {r['passes']} | {r['load_degree']} / {r['store_degree']} | {r['ms_median']:.3f} | {span} | "
                    f"{r['gb_per_s']:.0f} | {r['ratio_to_copy_probe_per_pass']:.2f} | {chain} | {tor} |\n")
        e = experiment
        f.write(f"\nThe n30 circuit after merge_gates ({e['gates']} gates) from |0..0>, the reset inside the timed call: as it is "
                f"{e['as_it_is']['ms_median']:.3f} ms in {e['as_it_is']['launches']} launches; after relayout_ to busiest_dims_order, the "
                f"relayout inside the call, {e['remapped']['ms_median']:.3f} ms in {e['remapped']['relayout_passes']} + "
                f"{e['remapped']['launches']} launches (the relayout alone {e['relayout_alone_ms_median']:.3f} ms); largest difference of "
                f"the two results at 4096 random indices {e['max_abs_difference_at_4096_indices']:.3e}.\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
