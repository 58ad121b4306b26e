"""Times the Born-statistics entry points on a 2^30-element complex64 tensor of random data against the torch
formulations they replace, in one process: HIP events, two warm-up calls, the median of REPEATS timed calls, the peak
extra device memory of one call, and bytes read / time as a fraction of the 7.2 TB/s of tools/probes/read_probe.hip.

    python tools/time_born.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes born_timing.json and born_timing.md into --out-dir."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import artensor_amd as A  # noqa: E402
from artensor_amd import born  # noqa: E402

READ_PROBE_TBS = 7.2
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


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # the tool is optional
        return [f"rocm-smi not available: {e}"]


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
    y = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    cube = x.view((2,) * nq)
    fast, slow = list(range(nq - 10, nq)), list(range(10))
    mixed = [0, 1, 2, 10, 11, 12, 13, nq - 3, nq - 2, nq - 1]
    plan = born.born_plan(n)
    rows = []

    def add(name, kind, fn, bytes_read, pair=None):
        med, lo, hi, extra = timed(fn, reps)
        rows.append({"name": name, "kind": kind, "ms_median": med, "ms_min": lo, "ms_max": hi, "bytes_read": bytes_read,
                     "fraction_of_read_probe": bytes_read / (med * 1e-3) / (READ_PROBE_TBS * 1e12), "extra_bytes": extra,
                     "replaces": pair})
        print(f"{name:46s} {med:9.3f} ms  [{lo:.3f}, {hi:.3f}]  {rows[-1]['fraction_of_read_probe']:6.1%} of read probe  "
              f"extra {extra / 2 ** 20:9.2f} MiB", flush=True)

    add("native norm2", "native", lambda: A.norm2(x, device=True), 8 * n)
    add("native overlap(a, b)", "native", lambda: A.overlap(x, y, device=True), 16 * n)
    add("native fidelity(a, b)", "native", lambda: A.fidelity(x, y, device=True), 16 * n)
    add("native block sums + prefix", "native", lambda: born.block_sums(x), 8 * n)
    for label, keep in (("10 fastest", fast), ("10 slowest", slow), ("10 mixed", mixed)):
        add(f"native marginal, {label} dims", "native", lambda keep=keep: A.marginal_probabilities(cube, keep), 8 * n)
    for lm in (10, 16, 20):
        u = torch.rand(2 ** lm, dtype=torch.float64, device=DEV, generator=g)
        idx, _ = A.sample(x, uniforms=u)
        touched = int(torch.unique(idx[:, 0] >> plan["block_bits"]).numel())
        add(f"native sample, 2^{lm} samples", "native", lambda u=u: A.sample(x, uniforms=u),
            8 * n + touched * 8 * 2 ** plan["block_bits"])

    def notebook_fidelity():
        return (x.conj() @ y.reshape(-1)).abs() / (x.abs().square().sum().sqrt() * y.abs().square().sum().sqrt())

    add("torch notebook fidelity expression", "torch", notebook_fidelity, 16 * n, "native fidelity(a, b)")
    add("torch view_as_real(x).square().sum(float64)", "torch",
        lambda: torch.view_as_real(x).square().sum(dtype=torch.float64), 8 * n, "native norm2")
    views = {"10 fastest": ((2 ** (nq - 10), 2 ** 10), (1, 0)), "10 slowest": ((2 ** 10, 2 ** (nq - 10)), (0, 1)),
             "10 mixed": ((8, 2 ** 7, 16, 2 ** (nq - 17), 8), (0, 2, 4, 1, 3))}
    for label, (shape, perm) in views.items():
        add(f"torch permute+reshape+sum marginal, {label}", "torch",
            lambda shape=shape, perm=perm: x.view(shape).permute(perm).reshape(1024, -1).abs().square().sum(1, dtype=torch.float64),
            8 * n, f"native marginal, {label} dims")

    # the two sides compute the same numbers
    f_native, f_torch = float(A.fidelity(x, y)), float(notebook_fidelity()) ** 2
    m_native = A.marginal_probabilities(cube, mixed).reshape(-1)
    m_torch = x.view(views["10 mixed"][0]).permute(views["10 mixed"][1]).reshape(1024, -1).abs().square().sum(1, dtype=torch.float64)
    agree = {"fidelity_native": f_native, "fidelity_torch": f_torch,
             "marginal_mixed_max_rel_diff": float((m_native - m_torch).abs().max() / m_torch.abs().max())}
    by_name = {r["name"]: r for r in rows}
    verdicts = []
    for r in rows:
        if r["replaces"]:
            nat = by_name[r["replaces"]]
            verdicts.append({"native": nat["name"], "torch": r["name"], "faster": nat["ms_median"] < r["ms_median"],
                             "less_memory": nat["extra_bytes"] < r["extra_bytes"]})
    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing)",
           "read_probe_TBps": READ_PROBE_TBS, "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total,
           "born_plan": plan, "rows": rows, "agreement": agree, "verdicts": verdicts}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "born_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "born_timing.md"), "w") as f:
        f.write(f"# Born statistics on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call; extra memory = peak device memory of "
                f"one call above what was allocated before it; fraction = bytes read / time / {READ_PROBE_TBS} TB/s "
                "(tools/probes/read_probe.hip).\n\n")
        f.write("| call | median ms | min..max ms | fraction of read probe | extra device memory |\n|---|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r['name']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | "
                    f"{r['fraction_of_read_probe']:.1%} | {r['extra_bytes'] / 2 ** 20:.2f} MiB |\n")
        f.write("\n| native | torch | faster | less memory |\n|---|---|---|---|\n")
        for v in verdicts:
            f.write(f"| {v['native']} | {v['torch']} | {'yes' if v['faster'] else 'NO'} | {'yes' if v['less_memory'] else 'NO'} |\n")
        f.write(f"\nAgreement: fidelity {f_native:.6e} (native) / {f_torch:.6e} (torch, float32 sums); "
                f"mixed marginal max relative difference {agree['marginal_mixed_max_rel_diff']:.2e}.\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"verdicts": verdicts, "agreement": agree}))


if __name__ == "__main__":
    main()
