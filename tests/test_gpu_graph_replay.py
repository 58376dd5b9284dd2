"""use_graph against eager runs after every change of state.

With use_graph a hierarchy captures VCycle into a HIP graph on the first call and replays it while the record of its host-side
inputs (mg_common.h mg_graph_record) is unchanged.  A record that misses an input replays a cycle of the wrong algorithm and
nothing reports it.  Every test here runs one sequence of calls on two hierarchies built from the same data -- one with
use_graph, one eager -- and after every call compares v of level 0 bit for bit, the coarse levels' v and f too, and, where the
oracle can state the step (a red-black V-cycle from level 0), the oracle's cycle from the same v and f.  Every change of state
is followed by three calls: one capture and two replays."""
import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import hierarchy_ok

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box: no spacing is a power of two
R2 = [0, 1, 0, 2]
A2 = [-1.0, -2.0, 0.0, -3.0]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(shape, dtype, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(dtype)


class Twin:
    """the same calls on a use_graph hierarchy and an eager one; `oracle(v, f, v1, v2, nlevels)` states a V-cycle from level 0"""

    def __init__(self, make, oracle=None, coarse=True):
        self.g, self.e = make(), make()
        self.g.use_graph = True
        self.oracle = oracle
        self.coarse = coarse
        self.steps = 0

    def close(self):
        self.g.close()
        self.e.close()

    def both(self, fn):
        out = [fn(self.g), fn(self.e)]
        self.check()
        return out

    def check(self, what=""):
        self.steps += 1
        tag = "step %d %s" % (self.steps, what)
        v = self.e.download_v(0)
        assert np.isfinite(v).all(), tag + ": v[0] not finite (NaN payloads are not compared)"
        assert bits_equal(self.g.download_v(0), v), tag + ": v[0]"
        if self.coarse:
            for l in range(1, self.e.numGrids):
                assert bits_equal(self.g.download_v(l), self.e.download_v(l)), tag + ": v[%d]" % l
                assert bits_equal(self.g.download_f(l), self.e.download_f(l)), tag + ": f[%d]" % l

    def record(self, gridID):
        return bytes(self.g._mg.contents.graph_rec[gridID])

    def vcycle(self, gridID, v1, v2, reps=3):
        """reps calls; with reps >= 3 the last one must be a replay (flags set by a capture may need a second one to settle):
        the slot's record stays as it was, which a capture under another record would change"""
        for i in range(reps):
            pinned = self.oracle is not None and gridID == 0 and self.e._mg.contents.smoother == 0
            if pinned:
                v, f = self.e.download_v(0), self.e.download_f(0)
            before = self.record(gridID)
            self.g.VCycle(gridID, v1, v2)
            if i == reps - 1 and reps >= 3:
                assert self.g._mg.contents.graph_exec[gridID] and self.record(gridID) == before, \
                    "step %d: V(%d, %d) from %d captured again instead of replaying" % (self.steps + 1, v1, v2, gridID)
            self.e.VCycle(gridID, v1, v2)
            self.check("V(%d, %d) from %d" % (v1, v2, gridID))
            if pinned:
                want = self.oracle(v, f, v1, v2, self.e.numGrids)
                assert bits_equal(self.e.download_v(0), want), "step %d: eager V(%d, %d) against the oracle" % (self.steps, v1, v2)

    def fmg(self, gridID, v0, v1, v2):
        self.both(lambda m: m.FullMultiGridVCycle(gridID, v0, v1, v2))

    def set(self, field, value):
        setattr(self.g._mg.contents, field, value)
        setattr(self.e._mg.contents, field, value)

    def numGrids(self, k):
        self.g.numGrids = k
        self.e.numGrids = k

    def smoother(self, name, omega=None):
        self.g.set_smoother(name, omega)
        self.e.set_smoother(name, omega)


# ---------------------------------------------------------------------------------------------------------------------- 3D
def _twin3(ctx, n3, dtype, layout, seed, nlevels=0):
    v, f = _rand(O.shape(n3), dtype, seed), _rand(O.shape(n3), dtype, seed + 1)

    def make():
        # CORRECT residual: the cycles converge.  With REF_COMPAT (the reference's sign quirk) fp32 runs of this length
        # overflow to inf / NaN, whose payloads the GPU and the CPU oracle need not share
        mg = P.MultiGrid3D(ctx, n3, RG, dtype, nlevels=nlevels, layout=layout, residual_mode=P.CORRECT)
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        return mg

    def oracle(v, f, v1, v2, nl):
        mode = t.e._mg.contents.residual_mode
        return O.cycle3d(n3, RG, nlevels=nl, mode=0, v1=v1, v2=v2, v=v, f=f, residual_mode=mode, dtype=dtype)

    t = Twin(make, oracle)
    return t


def _boundary_data(shape, dtype, seed):
    """random values everywhere, the boundary included (a nonzero rim)"""
    return _rand(shape, dtype, seed, 0.5, 1.5)


def _state_changes_3d(t, dtype):
    t.vcycle(0, 2, 2)
    for v1, v2 in ((0, 2), (2, 0), (1, 3), (3, 3), (2, 2)):
        t.vcycle(0, v1, v2)
    mode = t.e._mg.contents.residual_mode
    t.set("residual_mode", 1 - mode)
    t.vcycle(0, 2, 2)
    t.set("residual_mode", mode)
    t.vcycle(0, 2, 2)
    t.smoother("jacobi")  # the default omega
    t.vcycle(0, 2, 2)
    t.smoother("jacobi", 0.8)
    t.vcycle(0, 2, 2)
    t.smoother("rbgs")
    t.vcycle(0, 2, 2)
    t.set("fuse", 0)
    t.vcycle(0, 2, 2)
    t.set("fuse", 1)
    t.vcycle(0, 2, 2)
    k = t.e.numGrids
    if k > 2:
        t.numGrids(k - 1)
        t.vcycle(0, 2, 2)
        t.numGrids(k)
        t.vcycle(0, 2, 2)
    for gid in (1, 0, 2, 0):
        if gid < k:
            t.vcycle(gid, 2, 2, reps=1 if gid == 0 else 3)
    t.fmg(0, 1, 2, 2)
    t.vcycle(0, 2, 2, reps=1)
    t.fmg(0, 1, 2, 2)
    t.vcycle(0, 2, 2)
    # the arrays change under the replays
    shape0, shape1 = O.shape(t.e.size(0)), O.shape(t.e.size(1))
    t.both(lambda m: m.upload_v(0, _boundary_data(shape0, dtype, 11)))
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.upload_f(0, _rand(shape0, dtype, 12)))
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.upload_v(1, _boundary_data(shape1, dtype, 13)))
    t.both(lambda m: m.upload_f(1, _boundary_data(shape1, dtype, 14)))
    t.vcycle(1, 2, 2)
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.Relax(0, 2))
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.Relax(1, 3))
    t.vcycle(1, 1, 1)
    t.vcycle(0, 1, 1)
    t.both(lambda m: m.setToValue_v(0, 0.25, True))
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.setToValue_v(1, 0.0, True))
    t.vcycle(1, 2, 2)
    t.vcycle(0, 2, 2)
    r_g, r_e = t.both(lambda m: m.CalculateResidual(0))
    assert bits_equal(r_g, r_e)
    n_g, n_e = t.both(lambda m: m.ResidualNorm(0))
    # the state is compared bit for bit above; the norm itself adds per-workgroup partial sums with atomics, in no fixed order
    want = float(np.sqrt(np.sum(r_e.astype(np.float64) ** 2)))
    assert abs(n_g - want) <= 1e-5 * want and abs(n_e - want) <= 1e-5 * want
    t.vcycle(0, 2, 2)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("layout", ["xsplit", "natural"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_3d_state_changes_65(ctx, layout, dtype):
    t = _twin3(ctx, (65, 65, 65), dtype, layout, 1)
    _state_changes_3d(t, dtype)
    t.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("layout", ["xsplit", "natural"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_3d_state_changes_odd_extents(ctx, layout, dtype):
    """rows that end inside an x-tile (x = 97: 49 + 48 x-split halves), three levels, the coarsest (25 x 21 x 15) too large
    for the one-workgroup tail kernel: it runs Relax from zero and Relax on the pipelined / plain kernels"""
    n3 = (97, 81, 57)
    assert hierarchy_ok(n3, 3) and not hierarchy_ok(n3)
    t = _twin3(ctx, n3, dtype, layout, 2, nlevels=3)
    _state_changes_3d(t, dtype)
    t.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("layout", ["xsplit", "natural"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_3d_tail_kernel_sweep_counts(ctx, layout, dtype):
    """17^3: the whole cycle is the one-workgroup tail kernel; V(4097, 1) after V(1, 1) and V(4096, 1) after V(0, 1)"""
    t = _twin3(ctx, (17, 17, 17), dtype, layout, 3)
    _state_changes_3d(t, dtype)
    t.vcycle(0, 1, 1)
    t.vcycle(0, 4097, 1)
    t.vcycle(0, 0, 1)
    t.vcycle(0, 4096, 1)
    t.vcycle(0, 1, 4097, reps=1)
    t.close()


@pytest.mark.timeout(900)
def test_3d_hbm_levels_fp64(ctx):
    """385 x 129 x 65 fp64: level 0 runs the HBM kernels (the fused way down, the correcting pass)"""
    n3 = (385, 129, 65)
    t = _twin3(ctx, n3, np.float64, "xsplit", 4)
    t.coarse = False  # the coarse levels are compared by the smaller cases; v[0] here
    t.vcycle(0, 2, 2)
    t.vcycle(0, 1, 3)
    t.smoother("jacobi")
    t.vcycle(0, 2, 2)
    t.smoother("rbgs")
    t.set("residual_mode", P.REF_COMPAT)
    t.vcycle(0, 2, 2)
    t.set("residual_mode", P.CORRECT)
    t.vcycle(0, 2, 2)
    t.set("fuse", 0)
    t.vcycle(0, 2, 2, reps=2)
    t.set("fuse", 1)
    t.both(lambda m: m.upload_v(0, _boundary_data(O.shape(n3), np.float64, 15)))
    t.vcycle(0, 2, 2)
    t.numGrids(3)
    t.vcycle(0, 2, 2)
    t.close()


# ---------------------------------------------------------------------------------------------------------------------- PCG
def test_pcg_interleaved_with_cycles(ctx):
    n3 = (65, 33, 129)
    rng = [0, 1, 0, 2, 0, 1]
    f, v0 = _rand(O.shape(n3), np.float64, 21), _rand(O.shape(n3), np.float64, 22)

    def make():
        mg = P.MultiGrid3D(ctx, n3, rng, np.float64, residual_mode=P.CORRECT)
        mg.upload_f(0, f)
        mg.upload_v(0, v0)
        return mg

    t = Twin(make)
    for v1, v2, extra in ((1, 1, "V"), (2, 2, "FMG"), (1, 1, "V"), (1, 2, None), (1, 1, None)):
        rg, re_ = t.both(lambda m: m.PCG(v1, v2, 1e-9, 60))
        assert rg[0] == re_[0] and rg[1] == re_[1] and rg[2] == re_[2] and bits_equal(rg[3], re_[3]), (v1, v2)
        if extra == "V":
            t.vcycle(0, 2, 2, reps=2)
        elif extra == "FMG":
            t.fmg(0, 1, 2, 2)
            t.both(lambda m: m.upload_v(0, v0))
    t.close()


# ---------------------------------------------------------------------------------------------------------------------- 2D
def _twin2(ctx, n2, dtype, seed):
    v, f = _rand(O.shape(n2), dtype, seed), _rand(O.shape(n2), dtype, seed + 1)

    def make():
        mg = P.MultiGrid2D(ctx, n2, R2, A2, 2, dtype)
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        return mg

    def oracle(v, f, v1, v2, nl):
        return O.cycle2d(n2, R2, A2, 2, nlevels=nl, mode=0, v1=v1, v2=v2, v=v, f=f, dtype=dtype)

    return Twin(make, oracle)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n2", [(129, 65), (257, 257)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_2d_state_changes(ctx, n2, dtype):
    t = _twin2(ctx, n2, dtype, 5)
    t.vcycle(0, 2, 2)
    t.smoother("jacobi")  # default omega: fuse = 2 and smoother = 1 packed into the same key bit
    t.vcycle(0, 2, 2)
    t.smoother("jacobi", 0.8)
    t.vcycle(0, 2, 2)
    t.smoother("rbgs")
    t.vcycle(0, 2, 2)
    for fuse in (1, 0, 2):
        t.set("fuse", fuse)
        t.vcycle(0, 2, 2)
    t.set("fuse", 0)
    t.smoother("jacobi")
    t.vcycle(0, 2, 2)  # (fuse = 0, jacobi) against (fuse = 2, rbgs)
    t.smoother("rbgs")
    t.set("fuse", 2)
    t.vcycle(0, 2, 2)
    t.vcycle(0, 4, 4)
    t.vcycle(0, 5, 4)  # past the fast path's 4 sweeps
    t.vcycle(0, 4, 5)
    t.vcycle(0, 1, 1)
    t.vcycle(0, 4097, 1)
    t.vcycle(0, 1, 1)
    k = t.e.numGrids
    t.numGrids(k - 2)
    t.vcycle(0, 2, 2)
    t.numGrids(k)
    t.vcycle(0, 2, 2)
    for gid in (1, 0, 2, 0):
        t.vcycle(gid, 2, 2, reps=1 if gid == 0 else 3)
    t.fmg(0, 1, 2, 2)
    t.vcycle(0, 2, 2, reps=1)
    t.fmg(0, 1, 2, 2)
    shape0, shape1 = O.shape(t.e.size(0)), O.shape(t.e.size(1))
    t.both(lambda m: m.upload_v(0, _boundary_data(shape0, dtype, 31)))
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.upload_f(0, _rand(shape0, dtype, 32)))
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.upload_v(1, _boundary_data(shape1, dtype, 33)))
    t.both(lambda m: m.upload_f(1, _boundary_data(shape1, dtype, 34)))
    t.vcycle(1, 2, 2)
    t.vcycle(0, 2, 2)
    t.both(lambda m: m.Relax(0, 2))
    t.vcycle(0, 2, 2)
    t.close()


# ---------------------------------------------------------------------------------------------------------------------- context
def test_context_parameters_between_replays():
    """a fresh context, 65^3 fp32, V(3,3): the resident kernel runs inside the captured cycle; changing a parameter that
    forbids it must capture again (and so must re-enabling it), a speed-only parameter must not change the bits"""
    n3 = [65, 65, 65]
    c = P.Context(0)
    try:
        mg = P.MultiGrid3D(c, n3, RG, np.float32)
        mg.use_graph = True
        reps = 0

        def cycles(k=3):
            nonlocal reps
            for _ in range(k):
                mg.VCycle(0, 3, 3)
            reps += k
            assert bits_equal(mg.download_v(0), O.cycle3d(n3, RG, mode=0, v1=3, v2=3, reps=reps, dtype=np.float32)), reps

        cycles()
        resident = c.last_relax_kernel()
        assert resident.startswith("relax3d_xs_resident2_kernel"), resident
        c.set_param("gpu.exclusive", 0)
        cycles()
        assert "resident" not in c.last_relax_kernel(), c.last_relax_kernel()
        c.set_param("gpu.exclusive", 1)
        cycles()
        assert c.last_relax_kernel() == resident
        c.set_param("relax3d.resident", 0)
        cycles()
        assert "resident" not in c.last_relax_kernel(), c.last_relax_kernel()
        c.set_param("relax3d.resident", 1)
        cycles()
        assert c.last_relax_kernel() == resident
        c.set_param("relax3d.ty", 2)  # speed only
        cycles()
        c.set_param("relax3d.ty", 4)
        cycles()
        c.clear_abort(reenable=True)  # nothing had given up: the resident kernel stays allowed
        cycles()
        assert c.last_relax_kernel() == resident
        mg.close()
        c.sync()
    finally:
        c.close()


def test_context_generation():
    """mgx_ctx_generation grows with every parameter change and every clear_abort, and only then"""
    c = P.Context(0)
    try:
        g0 = c.generation()
        assert c.generation() == g0
        mg = P.MultiGrid3D(c, [17] * 3, RG, np.float64)
        mg.VCycle(0, 2, 2)
        c.sync()
        assert c.generation() == g0, "a cycle and a healthy sync change nothing"
        c.set_param("relax3d.ty", 2)
        g1 = c.generation()
        assert g1 > g0
        c.set_param("gpu.exclusive", 1)  # the value it already had: a spurious capture is harmless, a missed one is not
        g2 = c.generation()
        assert g2 > g1
        c.clear_abort(reenable=False)
        assert c.generation() > g2
        mg.close()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------- slab
@pytest.mark.timeout(600)
@pytest.mark.parametrize("ca_min_planes", [None, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_slab_one_rank_state_changes(dtype, ca_min_planes):
    n3 = [33, 17, 33]
    c = P.Context(0)
    try:
        v0, f0 = _rand(O.shape(n3), dtype, 41), _rand(O.shape(n3), dtype, 42)
        g = P.DistMultiGrid3D(c, n3, RG, dtype, min_planes=8, use_graph=True, ca_min_planes=ca_min_planes)
        e = P.DistMultiGrid3D(c, n3, RG, dtype, min_planes=8, use_graph=False, ca_min_planes=ca_min_planes)
        assert g.numDist >= 2
        state = {"v": v0.copy(), "f": f0.copy()}

        def down(mg):
            out = np.full(O.shape(n3), np.nan, dtype)
            mg.download_v_into(0, out)
            return out

        def both(fn):
            fn(g)
            fn(e)
            got = down(g)
            assert np.isfinite(got).all() and bits_equal(got, down(e))
            return got

        def vc(v1, v2, reps=3):
            for i in range(reps):
                want = O.cycle3d(n3, RG, nlevels=e.numGrids, mode=0, v1=v1, v2=v2, v=state["v"], f=state["f"], dtype=dtype)
                before = bytes(g._mg.contents.graph_rec)
                state["v"] = both(lambda m: m.VCycle(0, v1, v2))
                assert bits_equal(state["v"], want), (v1, v2)
                if i == reps - 1 and reps >= 3:  # the flags have settled: the last call replays
                    assert g._mg.contents.graph_exec and bytes(g._mg.contents.graph_rec) == before, (v1, v2, "captured again")

        both(lambda m: m.upload_f(0, f0))
        both(lambda m: m.upload_v(0, v0))
        vc(2, 2)
        vc(1, 3)
        vc(1, 1)
        vc(4097, 1, reps=1)
        vc(1, 1)
        k = e.numGrids
        for m in (g, e):
            m.numGrids = k - 1
        vc(2, 2)
        for m in (g, e):
            m.numGrids = k
        vc(2, 2)
        v1_, f1_ = _boundary_data(O.shape(n3), dtype, 43), _rand(O.shape(n3), dtype, 44)
        both(lambda m: m.upload_v(0, v1_))
        both(lambda m: m.upload_f(0, f1_))
        state["v"], state["f"] = v1_.copy(), f1_.copy()
        vc(2, 2)
        for k_ in (1, 2, 3):
            want = O.relax3d(n3, RG, state["v"], state["f"], k_, dtype=dtype)
            state["v"] = both(lambda m: m.Relax(0, k_))
            assert bits_equal(state["v"], want), k_
            vc(2, 2)
        state["v"] = both(lambda m: m.zero_v(0))
        assert not state["v"].any()
        vc(2, 2)
        g.close()
        e.close()
        c.sync()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------- Jacobi
def jacobi_vcycle3d(n3, rng, v, f, v1, v2, omega, nlevels, mode, dtype):
    """the reference's VCycle (N3/MultiGrid3D.cpp:623-647) with the weighted-Jacobi smoother, stated with the oracle's
    operators: Relax(v1); r = residual; f' = Restrict(r); v' = 0; VCycle(coarse); v += Interpolate(v'); Relax(v2)"""
    v = O.jacobi3d(n3, rng, v, f, omega, v1, dtype=dtype)
    if nlevels > 1:
        r = O.residual3d(n3, rng, v, f, mode, dtype=dtype)
        nc = O.csize(n3)
        fc = O.restrict3d(n3, r, dtype=dtype)
        vc = O.set3d(nc, np.ones(O.shape(nc), dtype), 0, True, dtype=dtype)
        vc = jacobi_vcycle3d(nc, rng, vc, fc, v1, v2, omega, nlevels - 1, mode, dtype)
        e = O.interpolate3d(n3, np.zeros(O.shape(n3), dtype), vc, dtype=dtype)
        v = O.correct3d(n3, v, e, dtype=dtype)
    return O.jacobi3d(n3, rng, v, f, omega, v2, dtype=dtype)


def jacobi_vcycle2d(n2, rng, A, alfa, v, f, v1, v2, omega, nlevels, dtype):
    """MultiGrid2D::VCycle (N2/MultiGrid2D.cpp:314-340) with the weighted-Jacobi smoother, from the oracle's operators"""
    v = O.jacobi2d(n2, rng, A, alfa, v, f, omega, v1, dtype=dtype)
    if nlevels > 1:
        r = O.residual2d(n2, rng, A, alfa, v, f, dtype=dtype)
        nc = O.csize(n2)
        fc = O.restrict2d(n2, r, dtype=dtype)
        vc = O.set2d(nc, np.ones(O.shape(nc), dtype), 0, True, dtype=dtype)
        vc = jacobi_vcycle2d(nc, rng, A, alfa, vc, fc, v1, v2, omega, nlevels - 1, dtype)
        e = O.interpolate2d(n2, np.zeros(O.shape(n2), dtype), vc, dtype=dtype)
        v = O.correct2d(n2, v, e, dtype=dtype)
    return O.jacobi2d(n2, rng, A, alfa, v, f, omega, v2, dtype=dtype)


def test_jacobi_restatement_has_the_cycle_order_of_the_oracle():
    """the restatement's skeleton with the red-black smoother is the oracle's own V-cycle, bit for bit"""
    n3, dtype = (33, 17, 49), np.float64
    v, f = _rand(O.shape(n3), dtype, 55), _rand(O.shape(n3), dtype, 56)
    saved = O.jacobi3d
    try:
        O.jacobi3d = lambda n, rng, v, f, omega, k, dtype: O.relax3d(n, rng, v, f, k, dtype=dtype)
        for mode in (P.REF_COMPAT, P.CORRECT):
            got = jacobi_vcycle3d(n3, RG, v, f, 2, 1, 0.0, 4, mode, dtype)
            assert bits_equal(got, O.cycle3d(n3, RG, nlevels=4, mode=0, v1=2, v2=1, v=v, f=f, residual_mode=mode, dtype=dtype))
    finally:
        O.jacobi3d = saved


@pytest.mark.timeout(600)
@pytest.mark.parametrize("omega", [None, 0.8])
@pytest.mark.parametrize("mode", [P.REF_COMPAT, P.CORRECT])
@pytest.mark.parametrize("layout", ["xsplit", "natural"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_3d_jacobi_vcycle_restated(ctx, dtype, layout, mode, omega):
    """the eager Jacobi V-cycle, fused (default) and unfused, against the restatement, bit for bit"""
    n3 = (65, 33, 97)  # every level of the reference's rule odd
    v, f = _rand(O.shape(n3), dtype, 51), _rand(O.shape(n3), dtype, 52)
    for fuse in (True, False):
        mg = P.MultiGrid3D(ctx, n3, RG, dtype, residual_mode=mode, layout=layout, fuse=fuse)
        mg.set_smoother("jacobi", omega)
        w = mg._mg.contents.omega  # the hierarchy's own value of the default
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        want = v
        for v1, v2 in ((2, 2), (1, 3), (3, 0)):
            mg.VCycle(0, v1, v2)
            want = jacobi_vcycle3d(n3, RG, want, f, v1, v2, w, mg.numGrids, mode, dtype)
            assert bits_equal(mg.download_v(0), want), (fuse, v1, v2)
        mg.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("omega", [None, 0.8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_2d_jacobi_vcycle_restated(ctx, dtype, omega):
    n2 = (129, 65)
    v, f = _rand(O.shape(n2), dtype, 53), _rand(O.shape(n2), dtype, 54)
    for fuse in (2, 1, 0):
        mg = P.MultiGrid2D(ctx, n2, R2, A2, 2, dtype, fuse=fuse)
        mg.set_smoother("jacobi", omega)
        w = mg._mg.contents.omega
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        want = v
        for v1, v2 in ((2, 2), (1, 3), (5, 0)):
            mg.VCycle(0, v1, v2)
            want = jacobi_vcycle2d(n2, R2, A2, 2, want, f, v1, v2, w, mg.numGrids, dtype)
            assert bits_equal(mg.download_v(0), want), (fuse, v1, v2)
        mg.close()
