"""Batch-position independence: the tools of tests/test_gpu_position_independence.py (pinned on the CPU by
tests/test_batch_position_helper.py).

A problem's result must not depend on where it sits in the batch, so the same problems in another order must give the same
BITS.  An arrangement is an index array idx: position j of the arranged batch holds problem idx[j] of the natural one.
Every tensor has the batch as its last axis ([nx, B], [np, B], [B], [N, B], [N, nx, B], [dim, B], [n_rows, nx, B]).
"""
import numpy as np
import torch


def permutations(B, seed):
    """{name: idx} of the three arrangements of B problems (int64 arrays, position j holds problem idx[j]):
    reverse  problem p goes to B-1-p: another group slot, another wave, someone else in the ragged tail;
    rotate1  problem p goes to p+1 and the last becomes the first: every problem moves one group slot;
    shuffle  numpy.random.default_rng(seed).permutation(B), rotated by one where it would leave problem 0 in place."""
    ar = np.arange(B, dtype=np.int64)
    shuffle = np.random.default_rng(seed).permutation(B).astype(np.int64)
    if B > 1 and shuffle[0] == 0:
        shuffle = np.roll(shuffle, 1)
    return {"reverse": ar[::-1].copy(), "rotate1": np.roll(ar, 1), "shuffle": shuffle}


def _index(idx, device):
    return torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int64, device=device)


def take(t, idx):
    """The arranged tensor: out[..., j] = t[..., idx[j]], contiguous.  idx may be shorter than the batch (a prefix)."""
    return t.index_select(t.dim() - 1, _index(idx, t.device)).contiguous()


def put_back(t, idx):
    """take's inverse for a permutation idx: out[..., idx[j]] = t[..., j], contiguous (natural order again)."""
    idx = np.asarray(idx)
    if t.shape[-1] != idx.size or not np.array_equal(np.sort(idx), np.arange(idx.size)):
        raise ValueError("put_back needs a permutation of the whole batch")
    out = torch.empty_like(t, memory_format=torch.contiguous_format)
    out.index_copy_(t.dim() - 1, _index(idx, t.device), t)
    return out


def layout(position, L):
    """(wave, group, first lane) of the problem at `position` when L lanes work on a problem and 64 // L problems share a wave
    (the fused kernels: L = intervals; one lane per problem: L = 1)."""
    ppw = 64 // L
    return int(position) // ppw, int(position) % ppw, (int(position) % ppw) * L


def _bits(t):
    """The bit pattern as integers: a NaN equals itself, -0 differs from +0."""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def _ulps(va, vb, dtype):
    """Distance of two values in units in the last place (floats: on the ordered integer line; integers: their difference)."""
    if dtype not in (torch.float32, torch.float64):
        return abs(int(va) - int(vb))
    ftype, itype, width = (np.float32, np.int32, 32) if dtype == torch.float32 else (np.float64, np.int64, 64)

    def ordered(v):
        i = int(np.array(v, dtype=ftype).view(itype))
        return i if i >= 0 else -(i + (1 << (width - 1)))   # sign-magnitude -> two's complement order; -0 lands on 0
    if np.isnan(va) or np.isnan(vb):
        return float("nan")
    return abs(ordered(va) - ordered(vb))


def first_difference(a, b, L, idx=None, name="output"):
    """None where a and b (both in natural order, batch last) have the same bits; else a message for the first problem that
    differs: its index, its (wave, group, first lane) for a group width L in the natural layout and in the arrangement idx
    that produced b (None: the natural one again, e.g. another handle), the first differing entry, both values and their
    distance in ulps."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "%s: shapes / dtypes differ: %s %s against %s %s" % (name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    B = a.shape[-1]
    ne = (_bits(a) != _bits(b)).reshape(-1, B)
    bad = ne.any(dim=0)
    if not bool(bad.any()):
        return None
    p = int(torch.nonzero(bad)[0, 0])
    row = int(torch.nonzero(ne[:, p])[0, 0])
    entry = tuple(int(i) for i in np.unravel_index(row, tuple(a.shape[:-1]))) if a.dim() > 1 else ()
    va, vb = a.reshape(-1, B)[row, p].item(), b.reshape(-1, B)[row, p].item()
    if idx is None:
        pos = p
    else:
        where = np.nonzero(np.asarray(idx) == p)[0]
        pos = int(where[0]) if where.size else -1
    fmt = "%r" if a.dtype in (torch.float32, torch.float64) else "%d"
    return ("%s: problem %d differs (%d of %d problems do); natural layout (wave, group, first lane) = %s, arranged at position "
            "%d = %s, L = %d; first differing entry %s: " + fmt + " against " + fmt + ", %s ulps") % (
                name, p, int(bad.sum()), B, layout(p, L), pos, layout(pos, L) if pos >= 0 else None, L, entry + (p,), va, vb,
                _ulps(va, vb, a.dtype))
