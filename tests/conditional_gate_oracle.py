"""numpy oracle of the conditional gates of artensor_amd.trajectories: for every trajectory b the selector word picks a case,
and the controlled matrix of that case is applied to slice b in complex128.  Nothing here shares code with the library."""
import numpy as np

import trajectories_oracle as TO


def case_of(o, cases, mask=None):
    """Index of the case that selector word `o` names in the list of (key, matrix) pairs, or None: o < 0, or no key matches."""
    o = int(o)
    if o < 0:
        return None
    key = o if mask is None else o & int(mask)
    for j, (k, _) in enumerate(cases):
        if int(k) == key:
            return j
    return None


def is_identity(u):
    u = np.asarray(u)
    return bool((u == np.eye(u.shape[0])).all())


def apply_controlled(psi, u, targets, controls=(), values=None):
    """u on `targets` (the first listed the most significant digit) of the part of psi whose `controls` have `values`; a
    complex128 copy."""
    psi = np.array(psi, dtype=np.complex128)
    t = len(targets)
    values = [1] * len(controls) if values is None else list(values)
    idx = [slice(None)] * psi.ndim
    for d, v in zip(controls, values):
        idx[d] = int(v)
    part = psi[tuple(idx)]
    sub = [d - sum(c < d for c in controls) for d in targets]
    u = np.asarray(u, dtype=np.complex128).reshape((2,) * (2 * t))
    out = np.tensordot(u, part, axes=(list(range(t, 2 * t)), sub))        # the row digits come first, in the order listed
    psi[tuple(idx)] = np.moveaxis(out, list(range(t)), sub)
    return psi


def conditional_oracle(logical, selector, cases, targets, batch_dims, controls=(), values=None, mask=None):
    """The whole tensor after the conditional gate, complex128.  cases: list of (key, matrix)."""
    cases = list(cases.items()) if isinstance(cases, dict) else list(cases)
    sl = TO.slices(np.asarray(logical).astype(np.complex128), batch_dims)
    sub_t = TO.rest_dims(np.ndim(logical), targets, batch_dims)
    sub_c = TO.rest_dims(np.ndim(logical), controls, batch_dims)
    for b in range(sl.shape[0]):
        j = case_of(selector[b], cases, mask)
        if j is not None:
            sl[b] = apply_controlled(sl[b], cases[j][1], sub_t, sub_c, values)
    return TO.unslice(sl, np.shape(logical), batch_dims)
