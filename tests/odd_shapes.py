"""Shared helpers of the odd-extent tests (a plain module, imported by the test files that need it).

The library accepts every odd extent of at least 3 per axis, and a hierarchy needs every level it builds odd.  Extents that
are not 2^k + 1 leave the last x-tile of a row partly filled and give the odd-x half of an x-split row pad entries the
2^k + 1 rows of the same width do not have; these helpers build such cases and look at the pads."""
import math

import numpy as np

import pde_multigrid_amd as P
from pde_multigrid_amd.multigrid import xs_geometry, xs_pack


def levels(n, nlevels=0):
    """the extents of every level of a hierarchy (csrc/host/mg_multigrid.c: numGrids = floor(log2(min - 1)), each coarse
    extent (n - 1) / 2 + 1), or of its first `nlevels` levels"""
    count = nlevels or int(math.log2(min(n) - 1))
    out = [tuple(int(k) for k in n)]
    while len(out) < count:
        out.append(tuple((k - 1) // 2 + 1 for k in out[-1]))
    return out


def hierarchy_ok(n, nlevels=0):
    """is every extent of every level odd and at least 3?"""
    return all(k >= 3 and k % 2 == 1 for lvl in levels(n, nlevels) for k in lvl)


# NaNs with payloads of their own: a pad entry that is read as data turns the result into NaN, one that is written no longer
# has this bit pattern
POISON = {np.dtype(np.float64): np.array(0x7FF8DEADBEEF0001, np.uint64).view(np.float64),
          np.dtype(np.float32): np.array(0x7FC0BEEF, np.uint32).view(np.float32)}


def pad_mask(sx, dtype):
    """True at the pad entries of an x-split row of sx points"""
    H, Pt = xs_geometry(sx, np.dtype(dtype).itemsize)
    m = np.ones(Pt, bool)
    m[:(sx + 1) // 2] = False
    m[H:H + sx // 2] = False
    return m


def pack_poisoned(a):
    """P.xs_pack with every pad entry set to the poison NaN"""
    out = xs_pack(a)
    out[..., pad_mask(a.shape[-1], a.dtype)] = POISON[a.dtype]
    return out


def run_poisoned(ctx, arrays, call, dtype):
    """upload every array (reference layout) in the x-split layout with poisoned pads, run call(*device pointers) and download
    every array again as stored, pads included.  Returns (uploaded, downloaded), both lists of padded arrays."""
    ups = [pack_poisoned(np.ascontiguousarray(a, dtype)) for a in arrays]
    ptrs = [ctx.to_device(u) for u in ups]
    try:
        P.check(call(*ptrs))
        return ups, [ctx.to_host(p, u.shape, dtype) for p, u in zip(ptrs, ups)]
    finally:
        for p in ptrs:
            ctx.free(p)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def pads_unchanged(up, out, sx, zero_ok=False):
    """the pad entries of `out` (x-split rows of sx points) are those of `up`, bit for bit; zero_ok: or +0.0 (a call that
    zero-fills a whole array writes its pads with the zeros they hold by invariant)"""
    m = pad_mask(sx, up.dtype)
    got, was = bits(out[..., m]), bits(up[..., m])
    ok = got == was
    if zero_ok:
        ok |= got == 0
    return bool(ok.all())
