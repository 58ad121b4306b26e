"""Times the in-place gate circuits (A.GateCircuit: one launch per run) on 2^30 complex64 amplitudes: one gate per addressing
class on random data, then the n30 circuit of tests/golden/n30_gates.npz through the fused route at max_rank 0..4, with and
without merge_gates, next to the contraction-engine route A.state_vec measured in the same process.  HIP events around the whole
call, two warm-up calls, the median of REPEATS timed calls (the circuit rows start from |0..0> every call: the reset is inside
the timed region for both routes); extra device memory = the peak above what is allocated before the call.  The n30 result is
compared at Google's 10 000 bitstrings with the complex128 truth of the tensor-network amplitudes (amp_rel as the tests define it).

    python tools/time_gates.py [--repeats 10] [--out-dir profiles] [--skip-state-vec]

writes gates_timing.json and gates_timing.md into --out-dir."""
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


def amp_rel(got, want, rms):
    got, want = np.asarray(got, dtype=np.complex128).reshape(-1), np.asarray(want, dtype=np.complex128).reshape(-1)
    return float((np.abs(got - want) / np.maximum(np.abs(want), rms)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--skip-state-vec", action="store_true")
    args = ap.parse_args()
    nq, reps = 30, args.repeats
    n = 2 ** nq
    state_bytes = n * 8
    rows = []

    def add(name, route, gates, max_rank, runs, med, lo, hi, extra, err=None):
        rows.append({"name": name, "route": route, "gates": gates, "max_rank": max_rank, "runs": runs, "ms_median": med, "ms_min": lo,
                     "ms_max": hi, "extra_bytes": extra, "amp_rel_at_google": err})
        print(f"{name:40s} {route:28s} gates {gates:5d} runs {runs:4d} {med:10.3f} ms [{lo:.3f}, {hi:.3f}] extra "
              f"{extra / 2 ** 20:9.2f} MiB" + ("" if err is None else f" amp_rel {err:.2e}"), flush=True)

    # ---- one gate per addressing class, random data --------------------------------------------------------------------------
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    cube = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2)).view((2,) * nq)
    rng = np.random.default_rng(1)

    def unitary(dim):
        q, r = np.linalg.qr(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim)))
        return q * (np.diag(r) / np.abs(np.diag(r)))

    bit = lambda b: nq - 1 - b                                # dim of memory bit b
    singles = [("one qubit, register bit 0", (0,)), ("one qubit, piece bit 5", (5,)), ("one qubit, high bit 29", (29,)),
               ("two qubits, register 0, 1", (1, 0)), ("two qubits, register 0, piece 5", (5, 0)), ("two qubits, register 0, high 29", (29, 0)),
               ("two qubits, piece 3, 7", (7, 3)), ("two qubits, piece 5, high 29", (29, 5)), ("two qubits, high 20, 29", (29, 20)),
               ("two qubits, diagonal, high 20, 29", (29, 20))]
    for name, bits in singles:
        m = unitary(2 ** len(bits))
        if "diagonal" in name:
            m = np.diag(np.diag(m))
        circ = A.GateCircuit(cube.shape, cube.stride(), cube.dtype, [(m, tuple(bit(b) for b in bits))], DEV)
        med, lo, hi, extra = timed(lambda: circ(cube), reps)
        add(name, "in place (GateCircuit)", 1, None, circ.n_runs, med, lo, hi, extra)
    del cube
    torch.cuda.empty_cache()

    # ---- the n30 circuit ------------------------------------------------------------------------------------------------------
    g30 = load_case(os.path.join(GOLDEN, "n30_gates.npz"))
    bonds = [(g30.tensors[k], g30.meta["inds"][k]) for k in range(len(g30.meta["inds"]))]
    gates = A.gates_from_bonds(bonds, nq)
    case = load_case(os.path.join(GOLDEN, "n30_dense.npz"))
    strings = case.meta["google_bitstrings"]
    truth = np.load(os.path.join(GOLDEN, "c128_truth_gpu.npz"))["n30_dense_at_google"].reshape(-1)
    rms = 2.0 ** -15

    def at_google(t):
        flat = t.as_strided((n,), (1,), t.storage_offset())    # the state in memory order (t is a dense permuted view)
        st = t.stride()
        pos = torch.tensor([sum(int(c) * st[q] for q, c in enumerate(b)) for b in strings], device=DEV)
        return flat[pos].cpu().numpy()

    state = torch.zeros(n, dtype=torch.complex64, device=DEV).view((2,) * nq)
    for label, glist in (("n30 circuit", gates), ("n30 circuit, merge_gates", A.merge_gates(gates))):
        for max_rank in (0, 1, 2, 3, 4):
            circ = A.GateCircuit(state.shape, state.stride(), state.dtype, glist, DEV, max_rank)

            def call():
                state.zero_()
                state.view(-1)[0] = 1
                circ(state)
            med, lo, hi, extra = timed(call, reps)
            add(label, "in place (GateCircuit)", len(glist), max_rank, circ.n_runs, med, lo, hi, extra, amp_rel(at_google(state), truth, rms))
    del state
    torch.cuda.empty_cache()
    if not args.skip_state_vec:
        out = []

        def call():
            out[:] = [A.state_vec(bonds, nq, device=DEV)]
        med, lo, hi, extra = timed(call, reps)
        add("n30 circuit", "A.state_vec (contraction engine)", len(bonds), None, 0, med, lo, hi, extra, amp_rel(at_google(out[0]), truth, rms))

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total, "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "gates_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "gates_timing.md"), "w") as f:
        f.write(f"# In-place gate circuits on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, prebuilt `GateCircuit`, one launch per "
                "run.  The single-gate rows run on random data; the circuit rows start from |0..0> inside the timed call, `A.state_vec` "
                f"included (it allocates and initialises its own state).  Extra device memory: the peak above what was allocated before "
                f"the call (the in-place state of {state_bytes / 2 ** 30:.0f} GiB is allocated before; `state_vec` allocates its own).  "
                "amp_rel: the result at Google's 10 000 bitstrings against the complex128 truth of the tensor-network amplitudes.\n\n")
        f.write("| circuit | route | gates | max_rank | runs | median ms | min..max ms | extra device memory | amp_rel |\n"
                "|---|---|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            mr = "-" if r["max_rank"] is None else str(r["max_rank"])
            err = "-" if r["amp_rel_at_google"] is None else f"{r['amp_rel_at_google']:.2e}"
            f.write(f"| {r['name']} | {r['route']} | {r['gates']} | {mr} | {r['runs'] or '-'} | {r['ms_median']:.3f} | "
                    f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['extra_bytes'] / 2 ** 20:.2f} MiB | {err} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
