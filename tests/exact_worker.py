"""Worker of test_exact_contraction_gpu.py::test_switches_read_when_the_library_loads: the exact-integer cases that need a
switch the library reads once per process.  Started with ARTN_XROW64=0 ARTN_WIDE=1 ARTN_WIDE_MIN_TILES=1:
  the row-streaming cases of tests/exact_cases.py, which must now be planned onto the 16-row shape of artn_k_xrow (m_tile_bits 4);
  exact_cases.wide_pairs(): 6 + 6, 5 + 6 and 6 + 5 contracted bits at 2^18 elements on artn_k_wide, classes wide and dense.
Every case: path from the planner's own answer, the exactness condition on the reference, then `==`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import artensor_amd as A
from artensor_amd import contraction as C
import exact_cases as E
import exact_contraction as X


def main():
    assert os.environ.get("ARTN_XROW64") == "0" and os.environ.get("ARTN_WIDE") == "1" and os.environ.get("ARTN_WIDE_MIN_TILES") == "1"
    gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    done = 0
    for name, case in E.cases().items():
        if not name.startswith("xrow"):
            continue
        info = A.step_info(case.eqs[0], case.a_shape, case.b_shapes[0])
        assert info["kernel"] == E.KERNEL_XGEMM and info["m_tile_bits"] == 4, (name, info)
        a, smalls, _, _ = E.operands(case)
        want, _, q = E.exact_result(case, (a, smalls, None, None))
        got = A.contract(case.eqs[0], gpu(a), gpu(smalls[0])).cpu().numpy()
        assert np.array_equal(got, want.astype(np.complex64)), name
        print(f"{name} on 16-row blocks: range quantity {X.headroom(q, 'complex64')}")
        done += 1
    assert done == 5, done
    for case in E.wide_pairs():
        path, info = E.planned(case)   # (asserts is_wide on the planner's answer)
        k1, k2 = (len(E.X.contracted_labels(eq)) for eq in case.eqs)
        assert path == (E.KERNEL_BITS, 1, k1, k2, 0) and E.is_wide(info), (case.name, path)
        a, smalls, _, _ = E.operands(case)
        want, _, q = E.exact_result(case, (a, smalls, False, None))
        got = C.contract2(case.eqs[0], gpu(a), gpu(smalls[0]), case.eqs[1], gpu(smalls[1]))
        assert got is not None, case.name
        assert np.array_equal(got.cpu().numpy(), want.astype(np.complex64)), case.name
        print(f"{case.name} on artn_k_wide: range quantity {X.headroom(q, 'complex64')}")
        done += 1
    assert done == 11, done
    print("exact worker ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
