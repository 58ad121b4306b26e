"""Host only: what the executor compiles for every fixture under tests/golden/, as JSON lines.

    python tools/dump_launch_lists.py OUT.jsonl

Dense fixtures (slice 0 of a sliced one, one slab of an output-partitioned one): _compile_dense(scheme, leaf shapes,
dtype) for complex64, complex64 under precision("bf16") and complex128 -- one record per launch (steps, operand ids,
result shape, planner info, the raw bytes of its descriptors) and one for the small-step program.  Sparse fixtures:
chain_schedule, fusion_schedule and _plan_small_program on the leaf shapes.  Two trees compile the same plans exactly when their outputs are equal byte for
byte; the planner switches (ARTN_CHAIN_PLAN, ARTN_NO_FUSE, ARTN_NO_PROGRAM, ARTN_OWN_LAYOUTS) and the library (ARTN_LIB)
come from the environment.  Uses only names an older tree has too."""
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import artensor_amd as A  # noqa: E402
from artensor_amd import contraction as C  # noqa: E402
from artensor_amd.fixtures import load_case  # noqa: E402


def _plain(v):
    """ids, shapes and schedule entries as JSON values (the scalar-one operand as a fixed string)"""
    if v is C._ONE:
        return "_ONE"
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    return v


def _hex(d):
    return None if d is None else bytes(d).hex()


def _program(prog):
    if prog is None:
        return None
    return {"ext_ids": _plain(prog.ext_ids), "ws_bytes": prog.ws_bytes, "outputs": _plain(prog.outputs),
            "step_out": _plain(prog.step_out), "n_groups": prog.n_groups,
            "host_image": hashlib.sha256(prog.host_image.numpy().tobytes()).hexdigest()}


def _leaf_shapes(case):
    tensors = case.fresh_tensors(device="cpu")
    if case.slicing_indices:
        tensors = A.apply_slice(tensors, case.slicing_indices, A.slice_assignments(len(case.slicing_indices), 0))
    shapes = {k: tuple(t.shape) for k, t in tensors.items() if isinstance(t, torch.Tensor)}
    for leaf, dim, _qubit in case.meta.get("fixed", ()):   # (a slab of an output-partitioned plan: those dims are fixed)
        shapes[leaf] = tuple(None if d == dim else e for d, e in enumerate(shapes[leaf]))
    return {k: tuple(e for e in sh if e is not None) for k, sh in shapes.items()}


def dump(out):
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        name = os.path.basename(path)
        try:
            case = load_case(path)
        except KeyError:
            continue   # (not a contraction case: recorded truths, gate lists)
        if not case.scheme:
            continue
        shapes = _leaf_shapes(case)
        if len(case.scheme[0]) > 2:
            prog, main = C._plan_small_program(case.scheme, shapes, torch.complex64)
            rec = {"case": name, "chain_schedule": _plain(C.chain_schedule(case.scheme)),
                   "fusion_schedule": _plain(C.fusion_schedule(case.scheme)), "program": _program(prog), "main": _plain(main)}
            out.write(json.dumps(rec, sort_keys=True) + "\n")
            continue
        for mode, dtype in (("c64", torch.complex64), ("c64_bf16", torch.complex64), ("c128", torch.complex128)):
            with C.precision("bf16" if mode == "c64_bf16" else None):
                prog, ops = C._compile_dense(case.scheme, shapes, dtype)
            out.write(json.dumps({"case": name, "mode": mode, "program": _program(prog), "n_ops": len(ops)}, sort_keys=True) + "\n")
            for op in ops:
                rec = {"case": name, "mode": mode, "steps": _plain(op.steps), "i": _plain(op.i), "j": _plain(op.j),
                       "j2": _plain(op.j2), "j3": _plain(op.j3), "out_shape": _plain(op.out_shape), "sum_rows": op.sum_rows,
                       "info": op.info, "d1": _hex(op.d1), "d2": _hex(op.d2), "d3": _hex(op.d3)}
                out.write(json.dumps(rec, sort_keys=True) + "\n")


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        dump(f)
