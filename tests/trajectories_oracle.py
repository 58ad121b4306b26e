"""numpy oracle of artensor_amd.trajectories: the trajectory of a flat memory index, the slices of a batched tensor, the batch
fields, and the choice per trajectory through measure.choose_outcome.  Nothing here shares code with the library's plan."""
import numpy as np

from artensor_amd.measure import choose_outcome


def _log2(x):
    x = int(x)
    assert x >= 1 and x & (x - 1) == 0, x
    return x.bit_length() - 1


def batch_size(shape, batch_dims):
    B = 1
    for x in batch_dims:
        B *= int(shape[x])
    return B


def batch_index(flat, shape, strides, batch_dims):
    """Trajectory of the element at flat memory index `flat` (an int or an integer array): the mixed-radix integer of the digits of
    the batch dims, the first listed one the most significant."""
    flat = np.asarray(flat, dtype=np.int64)
    b = np.zeros_like(flat)
    for x in batch_dims:
        e, s = int(shape[x]), int(strides[x])
        b = b * e + (flat // s) % e
    return b


def batch_index_brute(shape, strides, batch_dims):
    """flat memory index -> trajectory, by walking every multi-index of the tensor."""
    out = {}
    for idx in np.ndindex(*shape):
        flat = sum(int(i) * int(s) for i, s in zip(idx, strides))
        b = 0
        for x in batch_dims:
            b = b * int(shape[x]) + int(idx[x])
        out[flat] = b
    return out


def fields(shape, strides, batch_dims):
    """The batch dims merged where they are adjacent in memory and in order: [(shift, width, pos)], the most significant first."""
    out, pos = [], sum(_log2(shape[x]) for x in batch_dims)
    for x in batch_dims:
        w, s = _log2(shape[x]), _log2(strides[x])
        if w == 0:
            continue
        pos -= w
        if out and out[-1][0] == s + w:                        # this dim sits right below the previous one
            out[-1] = (s, out[-1][1] + w, pos)
        else:
            out.append((s, w, pos))
    return out


def slices(logical, batch_dims):
    """[B, ...rest]: the trajectories of a host array in its logical dim order, the other dims in their order (a copy)."""
    nb = len(batch_dims)
    moved = np.moveaxis(logical, list(batch_dims), list(range(nb)))
    B = batch_size(logical.shape, batch_dims)
    return np.ascontiguousarray(moved).reshape((B,) + moved.shape[nb:])


def unslice(sl, shape, batch_dims):
    """The inverse of slices()."""
    nb = len(batch_dims)
    rest = [x for x in range(len(shape)) if x not in batch_dims]
    moved = sl.reshape([shape[x] for x in batch_dims] + [shape[x] for x in rest])
    return np.moveaxis(moved, list(range(nb)), list(batch_dims))


def rest_dims(n_dims, dims, batch_dims):
    """`dims` renumbered for a slice."""
    rest = [x for x in range(n_dims) if x not in batch_dims]
    return [rest.index(x) for x in dims]


def choose(q, uniforms):
    """Outcome per trajectory of q [B, D] under uniforms [B]."""
    return [choose_outcome(q[b], uniforms[b])[0] for b in range(q.shape[0])]
