"""Shared helpers of the z-slab entry tests (a plain module, imported by test_slab_cases_cpu.py and test_gpu_slab_entries.py).

A z-slab entry of include/mgx.h works on a WINDOW: a local array of consecutive z-planes of a level, starting at a global plane
`off`.  On the planes it says it writes it must give the bits of the whole-grid operator applied to the global array, and it must
leave every other word of the window as it was.  The helpers cut windows out of global arrays (reference layout, [z, y, x]),
stitch the expected window together from a whole-grid result, and poison what a call may not read: a NaN that shows up in a
result was read outside the contract, a poison word that changed was written outside it."""
import numpy as np

import oracle as O
from odd_shapes import POISON, pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import xs_unpack


def window(global_array, off, nplanes):
    """the planes [off, off + nplanes) of a global array, as an array of its own"""
    assert 0 <= off and nplanes >= 1 and off + nplanes <= global_array.shape[0], (off, nplanes, global_array.shape)
    return np.array(global_array[off:off + nplanes], copy=True, order="C")


def colour_mask(n3, colour):
    """True where (x + y + z_global) & 1 == colour (0 = red, 1 = black), over the whole grid"""
    sx, sy, sz = n3
    z, y, x = np.ogrid[:sz, :sy, :sx]
    return ((x + y + z) & 1) == colour


def interior_mask(n3):
    """True at the interior points of the grid (every point no face holds)"""
    m = np.zeros(O.shape(n3), bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def xy_interior_mask(n3):
    """True at the (x, y)-interior points of every plane, the planes z = 0 and sz - 1 included"""
    m = np.zeros(O.shape(n3), bool)
    m[:, 1:-1, 1:-1] = True
    return m


def expected(window_before, global_result, off, written_planes, mask=None):
    """the window with exactly the listed GLOBAL planes replaced by the whole-grid result; mask (a global boolean array)
    restricts the replacement to its True points"""
    out = window_before.copy()
    for z in written_planes:
        assert off <= z < off + out.shape[0], (z, off, out.shape)
        if mask is None:
            out[z - off] = global_result[z]
        else:
            m = mask[z]
            out[z - off][m] = global_result[z][m]
    return out


def poison_planes(win, off, keep):
    """every plane of the window whose GLOBAL index is not in `keep` becomes poison, whole"""
    keep = set(keep)
    for k in range(win.shape[0]):
        if off + k not in keep:
            win[k] = POISON[win.dtype]
    return win


def poison_points(win, off, mask, planes=None):
    """the points of `mask` (a global boolean array) become poison, on every plane of the window or on the listed GLOBAL ones"""
    for k in range(win.shape[0]):
        if planes is None or off + k in planes:
            win[k][mask[off + k]] = POISON[win.dtype]
    return win


def is_poison(a):
    w = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.ascontiguousarray(a).view(w) == POISON[a.dtype].view(w)


def span(lo, hi, sz, below=1, above=2):
    """(off, nplanes) of a window that holds the global planes [lo, hi] and, where the grid allows, `below` / `above` surplus
    planes under / over them"""
    off = max(lo - below, 0)
    top = min(hi + above, sz - 1)
    return off, top - off + 1


def run_slab(ctx, arrays, call, dtype, zero_ok=()):
    """odd_shapes.run_poisoned, the pads of every array checked (zero_ok: indices of arrays a call may zero-fill); returns
    the downloaded arrays in the reference layout"""
    ups, outs = run_poisoned(ctx, arrays, call, dtype)
    for i, (u, o, a) in enumerate(zip(ups, outs, arrays)):
        assert pads_unchanged(u, o, a.shape[-1], zero_ok=i in zero_ok), "pad entries of array %d changed" % i
    return [xs_unpack(o, a.shape[-1]) for o, a in zip(outs, arrays)]
