"""Lists of face points that one rim launch does not cover (a plain module, imported by test_long_lists_cpu.py and
test_gpu_zzz_long_face_lists.py).

Every operation on the face unknowns runs through RIM_FOR_EACH_POINT (csrc/mgx_rim3d.hpp): at most 4096 blocks of 256 threads, each
thread striding over the list by the size of the launch.  A list longer than CAP = 4096 * 256 entries is covered in rounds; from its
second round on a thread handles a point that may lie on another face, of another kind (whole rows against x-face points), than
its first.  This module restates the list (rim_list, rim_point) in numpy: how long it is, in how many rounds a launch covers it and
in which round every face unknown is visited; and it holds the shapes the tests use, thin grids whose faces are large: the list is
long where a face is, and the grid behind it may be five planes thick."""
import numpy as np

import op_restated as OP
import oracle as O
import pde_multigrid_amd as P

RIM_THREADS, RIM_MAX_BLOCKS = 256, 4096
CAP = RIM_MAX_BLOCKS * RIM_THREADS
DTYPES = [np.float64, np.float32]
# the faces in the kernel's order z-low, z-high, y-low, y-high, x-low, x-high: their bits in the mask
FACE_BITS = (4, 5, 2, 3, 0, 1)


def face_counts(n3, bc, dtype):
    """the listed entries of the six faces, in the kernel's order: whole rows of P storage positions (pads included) for the z- and
    the y-faces, the points of the open square for the x-faces; 0 for a face whose bit is clear"""
    sx, sy, sz = (int(k) for k in n3)
    pitch = P.xs_geometry(sx, np.dtype(dtype).itemsize)[1]
    cnt = [pitch * sy, pitch * sy, pitch * (sz - 2), pitch * (sz - 2), (sy - 2) * (sz - 2), (sy - 2) * (sz - 2)]
    return [c if (int(bc) >> b) & 1 else 0 for c, b in zip(cnt, FACE_BITS)]


def listed(n3, bc, dtype):
    """the length of the list: pads and Dirichlet entries included, as in the library"""
    return sum(face_counts(n3, bc, dtype))


def rounds(n3, bc, dtype):
    """the rounds of the grid stride a full launch needs"""
    return -(-listed(n3, bc, dtype) // CAP)


def visits(n3, bc, dtype):
    """(round_of, count): at every unknown the list visits the round (0, 1, ...) of its latest visit, -1 elsewhere; and how often
    every point is visited as an unknown (the library lists every face unknown once: an edge belongs to the z-face, else to the
    y-face).  Both in the reference layout."""
    sx, sy, sz = (int(k) for k in n3)
    H, pitch = P.xs_geometry(sx, np.dtype(dtype).itemsize)
    rnd = np.full(O.shape(n3), -1, np.int64)
    count = np.zeros(O.shape(n3), np.int64)
    start = 0
    for k, cnt in enumerate(face_counts(n3, bc, dtype)):
        u = np.arange(cnt, dtype=np.int64)
        t = start + u
        start += cnt
        if k < 4:  # whole rows: storage position u % P of row u // P, through the x-split position to x
            row, j = u // pitch, u % pitch
            x = np.where(j < H, 2 * j, 2 * (j - H) + 1)
            if k < 2:
                y, z = row, np.full_like(u, 0 if k == 0 else sz - 1)
            else:
                y, z = np.full_like(u, 0 if k == 2 else sy - 1), 1 + row
        else:
            q, rem = u // (sy - 2), u % (sy - 2)
            x, y, z = np.full_like(u, 0 if k == 4 else sx - 1), 1 + rem, 1 + q
        keep = x < sx  # a pad position otherwise
        x, y, z, t = x[keep], y[keep], z[keep], t[keep]
        on = (x == 0) * 1 | (x == sx - 1) * 2 | (y == 0) * 4 | (y == sy - 1) * 8 | (z == 0) * 16 | (z == sz - 1) * 32
        keep = (on & ~int(bc)) == 0  # no unknown otherwise: it lies on a Dirichlet face too
        x, y, z, t = x[keep], y[keep], z[keep], t[keep]
        flat = (z * sy + y) * sx + x
        rnd.ravel()[flat] = t // CAP  # t grows along the list: of two visits the later one stays
        count += np.bincount(flat, minlength=count.size).reshape(count.shape)
    return rnd, count


_round_of = {}


def round_of(n3, bc, dtype):
    """visits()[0], computed once per case and shared (do not modify it)"""
    key = (tuple(int(k) for k in n3), int(bc), np.dtype(dtype).name)
    if key not in _round_of:
        _round_of[key] = visits(n3, bc, dtype)[0]
    return _round_of[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def diagnose(got, want, rnd):
    """None where got has want's bits; else the diagnosis: how many points differ, the lowest round of the list in which one of them
    lies (round 0 wrong: the body itself; wrong from round 1 on: the stride or what a thread carries from one round to the next)
    and how many lie off the list"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape == rnd.shape and got.dtype == want.dtype, (got.shape, want.shape, rnd.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    if not bad.any():
        return None
    r = rnd[bad]
    on = r[r >= 0]
    first = tuple(int(k) for k in np.argwhere(bad)[0])
    return "%d points differ: %d on the list, the lowest round %s (per round %s); %d off the list; the first at (z, y, x) = %s, round %d" % (
        int(bad.sum()), on.size, int(on.min()) if on.size else None, np.bincount(on).tolist() if on.size else [], int((r < 0).sum()), first,
        int(rnd[first]))


# ------------------------------------------------------------------------------------------ the shapes
# (name, the listed shape, mask, entries (fp64, fp32), rounds (fp64, fp32)).  A: two large z-faces; with both z-faces flagged the
# second round holds the last rows of z-high and, with mask 63, ALL y- and x-face points.  B: twice as wide, three rounds with all
# six faces; mask 37 has one face per axis.  Y: the large faces are the y-faces, the tail in rows of y-high.  C and F: the coarse and
# the fine grid of the transfers, restrict_bc lists C, interpolate_bc and interpolate_correct_bc list F.
A, B, Y = (1025, 513, 5), (2049, 513, 5), (1025, 5, 513)
F, C = (2049, 1025, 5), (1025, 513, 3)
TABLE = [
    ("A", A, 48, (1067040, 1083456), (2, 2)),
    ("A", A, 63, (1076346, 1092858), (2, 2)),
    ("B", B, 37, (1066557, 1074813), (2, 2)),
    ("B", B, 63, (2133114, 2149626), (3, 3)),
    ("Y", Y, 12, (1062880, 1079232), (2, 2)),
    ("Y", Y, 63, (1076346, 1092858), (2, 2)),
    ("C", C, 48, (1067040, 1083456), (2, 2)),
    ("C", C, 63, (1070142, 1086590), (2, 2)),
    ("F", F, 48, (4231200, 4264000), (5, 5)),
    ("F", F, 63, (4249722, 4282618), (5, 5)),
]
SHAPES = {name: n3 for name, n3, _, _, _ in TABLE}
MASKS = {name: [bc for nm, _, bc, _, _ in TABLE if nm == name] for name in SHAPES}
# the longest lists of the shapes the other files use: one round
CONTROLS = [(513, 5, 5), (17, 17, 17)]


def strided_face_unknowns(n3, bc, dtype):
    """the face unknowns visited after the first round"""
    return round_of(n3, bc, dtype) >= 1


def all_face_unknowns_listed_once(n3, bc, dtype):
    """does the list visit exactly the face unknowns of op_restated, every one once?"""
    rnd, count = visits(n3, bc, dtype)
    m = OP.face_unknowns(n3, bc)
    return bool(np.array_equal(rnd >= 0, m) and np.array_equal(count, m.astype(np.int64)))
