"""Times measurement (A.measure_, A.postselect_, A.reset_) on 2^30 complex64 amplitudes: one qubit at memory bit 0, a middle bit
and the top bit, k = 4 and k = 10, with device=False (one 32-byte copy to the host ends the call) and device=True (no
synchronisation); the collapse launch alone (artn_measure_collapse on a prepared record); and the comparison route of the parent
commit measured in the same process: marginal_probabilities + a host draw + the scaled projector through apply_gate_ (k <= 2) or
apply_wide_gate_ (k = 4).  The state is restored from a copy before every call, outside the timed region, so that every call
collapses a full state.  HIP events around the whole call, two warm-up calls, the median of REPEATS timed calls.

For the collapse alone a fraction is reported with the nominal bytes of measure_info:
    (bytes written / write rate of the copy probe + bytes read / the 7.2 TB/s of tools/probes/read_probe.hip) / time
where the copy probe is a device-to-device copy of the whole state timed here (its write rate = bytes of the state / time); the
zero fill of the state is timed next to it for reference.

    python tools/time_measure.py [--log2n 30] [--repeats 10] [--out-dir profiles]

writes measure_timing.json and measure_timing.md into --out-dir."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import artensor_amd as A  # noqa: E402
from artensor_amd import _native  # noqa: E402
from artensor_amd import measure as M  # noqa: E402
from artensor_amd.born import _marginal_desc  # noqa: E402
from time_born import DEV, READ_PROBE_TBS, clocks  # noqa: E402


def timed(fn, prepare, repeats, warmup=2):
    """median, min, max ms of fn(); prepare() runs before every call, outside the timed region"""
    ms = []
    for it in range(warmup + repeats):
        prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


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
    backup = torch.view_as_complex(torch.randn(n, 2, device=DEV, generator=g) * 2.0 ** (-(nq + 1) / 2))
    state = torch.empty_like(backup)
    cube = state.view((2,) * nq)
    restore = lambda: state.copy_(backup)
    nothing = lambda: None
    bit = lambda b: nq - 1 - b                                 # dim of memory bit b
    mid = nq // 2
    state_bytes = n * 8

    copy_ms = timed(restore, nothing, reps)
    fill_ms = timed(lambda: state.zero_(), nothing, reps)
    write_tbs = state_bytes / (copy_ms[0] * 1e-3) / 1e12
    fill_tbs = state_bytes / (fill_ms[0] * 1e-3) / 1e12
    print(f"copy probe {copy_ms[0]:.3f} ms: write rate {write_tbs:.2f} TB/s; zero fill {fill_ms[0]:.3f} ms: {fill_tbs:.2f} TB/s", flush=True)

    places = {"1 qubit, memory bit 0": [0], f"1 qubit, memory bit {mid}": [mid], f"1 qubit, memory bit {nq - 1}": [nq - 1],
              "2 qubits": [1, nq - 1], "k = 4": [0, 7, mid, nq - 1], "k = 10": [0, 1, 2, 10, 11, 12, 13, nq - 3, nq - 2, nq - 1]}
    rows = []

    def add(name, route, k, bits, fn, info=None):
        med, lo, hi = timed(fn, restore, reps)
        row = {"name": name, "route": route, "k": k, "memory_bits": bits, "ms_median": med, "ms_min": lo, "ms_max": hi}
        if info is not None:
            ideal = info["bytes_written"] / (write_tbs * 1e12) + info["bytes_read"] / (READ_PROBE_TBS * 1e12)
            row.update(bytes_written=info["bytes_written"], bytes_read=info["bytes_read"], fraction=ideal / (med * 1e-3))
        rows.append(row)
        frac = f"  {row['fraction']:6.1%} of the probes" if info is not None else ""
        print(f"{name:44s} {route:34s} {med:9.3f} ms  [{lo:.3f}, {hi:.3f}]{frac}", flush=True)

    u = 0.37
    for place, bits in places.items():
        dims = [bit(b) for b in bits]
        k = len(dims)
        info = A.measure_info(cube.shape, cube.stride(), dims)
        add(place, "measure_(device=False)", k, bits, lambda: A.measure_(cube, dims, uniform=u))
        add(place, "measure_(device=True)", k, bits, lambda: A.measure_(cube, dims, uniform=u, device=True))
        if k in (1, 4):
            add(place, "postselect_(device=False)", k, bits, lambda: A.postselect_(cube, dims, 2 ** k - 1))
            add(place, "reset_(device=False)", k, bits, lambda: A.reset_(cube, dims, uniform=u))
            add(place, "reset_(device=True)", k, bits, lambda: A.reset_(cube, dims, uniform=u, device=True))
        add(place, "marginal_probabilities alone", k, bits, lambda: A.marginal_probabilities(cube, dims))

        # the collapse launch alone: a record prepared once from the full state
        restore()
        q = A.marginal_probabilities(cube, dims)
        rec = torch.empty(4, dtype=torch.float64, device=DEV)
        uni = torch.full((1,), u, dtype=torch.float64, device=DEV)
        d, _ = _marginal_desc(cube.shape, cube.stride(), dims, cube.dtype)
        lib = _native.lib()
        _native.check(lib.artn_measure_choose(q.data_ptr(), 2 ** k, uni.data_ptr(), -1, 1, rec.data_ptr(), _native.current_stream_ptr(state.device)))
        torch.cuda.synchronize()

        def collapse(reset=0):
            _native.check(lib.artn_measure_collapse(ctypes.byref(d), state.data_ptr(), rec.data_ptr(), reset,
                                                    _native.current_stream_ptr(state.device)))
        add(place, "collapse launch alone", k, bits, collapse, info)
        add(place, "reset launches alone (move + clear)", k, bits, lambda: collapse(1), info)

        # the comparison route: marginal + host draw + the scaled projector as a gate
        if k in (1, 2, 4):
            apply = A.apply_gate_ if k <= 2 else A.apply_wide_gate_

            def projector_route():
                qh = A.marginal_probabilities(cube, dims).reshape(-1).cpu().numpy()
                o, total = M.choose_outcome(qh, u)
                proj = np.zeros((2 ** k, 2 ** k), dtype=np.complex128)
                proj[o, o] = np.sqrt(total / qh[o])
                apply(cube, proj, dims)
            add(place, f"marginal + host draw + {apply.__name__}  [comparison]", k, bits, projector_route)

    free, total = torch.cuda.mem_get_info()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "log2_elements": nq, "dtype": "complex64",
           "repeats": reps, "warmup": 2, "timer": "HIP events around the whole call (enqueue + kernels + torch plumbing); the state is "
           "restored before every call, outside the timed region", "read_probe_TBps": READ_PROBE_TBS,
           "copy_probe": {"ms_median": copy_ms[0], "ms_min": copy_ms[1], "ms_max": copy_ms[2], "write_TBps": write_tbs},
           "zero_fill": {"ms_median": fill_ms[0], "ms_min": fill_ms[1], "ms_max": fill_ms[2], "write_TBps": fill_tbs},
           "clocks": clocks(), "device_memory_free_bytes": free, "device_memory_total_bytes": total, "rows": rows}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "measure_timing.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "measure_timing.md"), "w") as f:
        f.write(f"# Measurement on 2^{nq} complex64 amplitudes ({doc['device']})\n\n")
        f.write(f"Median of {reps} calls after 2 warm-up calls, HIP events around the whole call, one process; the state is restored from a "
                "copy before every call, outside the timed region.  Copy probe (device-to-device copy of the state): "
                f"{copy_ms[0]:.3f} ms, write rate {write_tbs:.2f} TB/s; zero fill of the state: {fill_ms[0]:.3f} ms, {fill_tbs:.2f} TB/s.  "
                "Fraction (collapse and reset launches alone): (nominal bytes written / the copy probe's write rate + nominal bytes read / "
                f"{READ_PROBE_TBS} TB/s of tools/probes/read_probe.hip) / time.\n\n")
        f.write("| measured | route | median ms | min..max ms | fraction |\n|---|---|---:|---:|---:|\n")
        for r in rows:
            frac = f"{r['fraction']:.1%}" if "fraction" in r else ""
            f.write(f"| {r['name']} {r['memory_bits']} | {r['route']} | {r['ms_median']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} | {frac} |\n")
        f.write("\nClocks: " + "; ".join(doc["clocks"]) + f"; device memory free {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB.\n")
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
