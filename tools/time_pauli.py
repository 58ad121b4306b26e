"""Times Pauli-string and Hamiltonian expectation values on a 2^30-element complex64 tensor of random data, and the route the
same one- and two-qubit operators took before (A.expectation through the reduced density matrix), in one process: HIP events, two
warm-up calls, the median of REPEATS timed calls, and bytes read / time as a fraction of the 7.2 TB/s of
tools/probes/read_probe.hip.

    python tools/time_pauli.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes pauli_timing.json and pauli_timing.md into --out-dir."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from time_born import DEV, READ_PROBE_TBS, clocks, timed  # noqa: E402


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
    x = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    cube = x.view((2,) * nq)                                  # dim d is memory bit nq - 1 - d
    rng = np.random.default_rng(1)
    rows = []

    def zz(q):
        return {q: "Z", q + 1: "Z"}

    def add(name, kind, fn, strings=None, bytes_read=None, pair=None):
        info = A.pauli_info(cube.shape, cube.stride(), strings) if strings is not None else None
        nbytes = info["bytes_read"] if info else bytes_read
        med, lo, hi, extra = timed(fn, reps)
        rows.append({"name": name, "kind": kind, "ms_median": med, "ms_min": lo, "ms_max": hi, "bytes_read": nbytes,
                     "launches": info["n_launches"] if info else None, "groups": info["n_groups"] if info else None,
                     "fraction_of_read_probe": nbytes / (med * 1e-3) / (READ_PROBE_TBS * 1e12), "extra_bytes": extra, "replaces": pair})
        print(f"{name:58s} {med:9.3f} ms  [{lo:.3f}, {hi:.3f}]  {rows[-1]['fraction_of_read_probe']:6.1%} of read probe  "
              f"extra {extra / 2 ** 20:9.2f} MiB", flush=True)

    def native(name, strings, pair=None):
        add(name, "native", lambda: A.pauli_expectation(cube, strings, device=True), strings=strings, pair=pair)

    z16 = [{q: "Z"} for q in range(8)] + [zz(q) for q in range(8)]
    z29 = [{q: "Z"} for q in range(14)] + [zz(q) for q in range(15)]
    mixed30 = "".join(rng.choice(list("XYZ"), nq))
    native("one Z string <Z_3 Z_17>", [{3: "Z", 17: "Z"}])
    native("16 Z/ZZ strings (1 launch)", z16)
    native("29 Z/ZZ strings (2 launches)", z29)
    native("one string, xm inside the tile <X on memory bit 3>", [{nq - 1 - 3: "X"}])
    native("one string, xm on the slowest bit <X_0>", [{0: "X"}])
    native(f"one weight-{nq} mixed string", [mixed30])
    tfim = [(-1.0, zz(q)) for q in range(nq - 1)] + [(-0.7, {q: "X"}) for q in range(nq)]
    add(f"transverse-field Ising sum, {nq} qubits ({len(tfim)} terms)", "native", lambda: A.pauli_sum_expectation(cube, tfim),
        strings=[p for _, p in tfim])

    # the route of the parent commit: the reduced density matrix of the operator's dims, then tr(rho op)
    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    Z = np.diag([1.0, -1.0]).astype(np.complex128)
    rdm_cases = (("<Z_3> through the RDM", Z, [3], {3: "Z"}), ("<X_0> through the RDM", X, [0], {0: "X"}),
                 ("<Z_3 Z_17> through the RDM", np.kron(Z, Z), [3, 17], {3: "Z", 17: "Z"}),
                 (f"<X on memory bit 3> through the RDM", X, [nq - 1 - 3], {nq - 1 - 3: "X"}))
    agree = {}
    for name, op, dims, string in rdm_cases:
        add(name, "rdm", lambda op=op, dims=dims: A.expectation(cube, op, dims), bytes_read=8 * n)
        agree[name] = {"rdm": A.expectation(cube, op, dims).real, "pauli": A.pauli_expectation(cube, string)}
    add(f"transverse-field Ising sum through the RDM ({len(tfim)} calls)", "rdm",
        lambda: sum(c * A.expectation(cube, np.kron(Z, Z) if len(p) == 2 else X, sorted(p)).real for c, p in tfim),
        bytes_read=8 * n * len(tfim), pair=f"transverse-field Ising sum, {nq} qubits ({len(tfim)} terms)")
    agree["tfim"] = {"rdm": sum(c * A.expectation(cube, np.kron(Z, Z) if len(p) == 2 else X, sorted(p)).real for c, p in tfim),
                     "pauli": A.pauli_sum_expectation(cube, tfim)}

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "read_probe_TBps": READ_PROBE_TBS, "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total,
           "terms_per_launch": A.pauli_info(cube.shape, cube.stride(), "Z" * nq)["terms_per_launch"], "mixed_string": mixed30,
           "rows": rows, "agreement": agree}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "pauli_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "pauli_timing.md"), "w") as f:
        f.write(f"# Pauli-string expectation values on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call (device=True except the sums, which "
                f"return a host number); fraction = bytes read / time / {READ_PROBE_TBS} TB/s (tools/probes/read_probe.hip); bytes read "
                "= launches x 8 GiB for the Pauli rows, one reading of the state per call for the RDM rows.\n\n")
        f.write("| call | groups | launches | median ms | min..max ms | fraction of read probe | extra device memory |\n"
                "|---|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r['name']} | {r['groups'] if r['groups'] is not None else '-'} | "
                    f"{r['launches'] if r['launches'] is not None else '-'} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                    f"{r['fraction_of_read_probe']:.1%} | {r['extra_bytes'] / 2 ** 20:.2f} MiB |\n")
        f.write("\nAgreement of the two routes (normalised values):\n\n| operator | through the RDM | Pauli pass |\n|---|---:|---:|\n")
        for k, v in agree.items():
            f.write(f"| {k} | {v['rdm']:.12e} | {v['pauli']:.12e} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"agreement": agree}))


if __name__ == "__main__":
    main()
