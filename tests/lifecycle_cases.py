"""What test_lifecycle_cpu.py and test_gpu_zzzzz_lifecycle.py share (a plain module, like op_cases.py): the settings
record S of a 3D hierarchy, the three ways to get a hierarchy with the settings S -- fresh() from the constructor, restated() in numpy,
apply() on a live one --, the hand-written walks through the setters, the disturbances that run between a setter and its probe, and
the probe: one call sequence that runs on a library hierarchy (Lib) and on a restated one (Rest).

The question the walks ask: after any history of setters and calls, is a hierarchy whose settings are S the machine that
MultiGrid3D(..., **S) builds?  Every walk is a list of (kind, value) steps, legal by the rules of include/mg_multigrid.h (legal()
states them); together they hold every ordered pair of setter kinds and every kind followed by itself with other values.  The layout
is x-split, the smoother red-black and residual_mode CORRECT throughout."""
import contextlib
import dataclasses
import functools
import math

import numpy as np

import op_restated as R
import oracle as O
import pin_restated as PR
import semi_restated as SR

KINDS = ("shift", "coefficient", "capacity", "face_mean", "neumann", "wall", "pinned", "numGrids", "use_graph")
RG = (-1.0, 1.0, 0.0, 2.0, 0.5, 3.0)  # no spacing is a power of two
UNIT = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
ZERO = R.ZERO
PCG_MAXIT = 30
BE_DT, BE_KAPPA = 0.5, 0.5  # BackwardEuler(1, dt, kappa): the shift it leaves is t(1 / (kappa dt)) = 4


def pcg_tol(dtype):
    """the tolerances of test_gpu_zzzz_pin.py (fp64) and test_gpu_graph_replay.py / solve3d_pcg (fp32)"""
    return 1e-9 if np.dtype(dtype) == np.float64 else 2e-5


# ------------------------------------------------------------------------------------------ the settings record
@dataclasses.dataclass(frozen=True)
class S:
    """the settings of one hierarchy.  a, c, pin and pin_values are NAMES of seeded fields (field()), so that a record prints, hashes
    and compares; beta and g are in the order of the mask's bits"""
    n3: tuple
    rng: tuple
    dtype: type
    coarsening: str = "full"
    numGrids: int = 0
    shift: float = 0.0
    a: str = None
    c: str = None
    mean: str = "arithmetic"
    bc: int = 0
    beta: tuple = ZERO
    g: tuple = ZERO
    pin: str = None
    pin_values: str = None

    @property
    def plain(self):
        """no setting in effect: the hierarchy of the Poisson problem (the mean counts only with a coefficient)"""
        return (self.shift == 0 and self.a is None and self.c is None and self.bc == 0 and not any(self.beta) and not any(self.g)
                and self.pin is None)

    @property
    def cleared(self):
        """everything as the constructor's defaults have it"""
        return self.plain and self.mean == "arithmetic" and self.numGrids == max_grids(self)

    @property
    def regular(self):
        """the closed box needs a shift or a beta > 0 (mg_multigrid.h: _set_boundary, _set_wall)"""
        return not (self.bc == 63 and self.shift == 0 and not any(b > 0 for b in self.beta))


def plan(s):
    """(sizes, masks) of every level the hierarchy allocates"""
    return SR.plan(s.n3, list(s.rng)) if s.coarsening == "semi" else R.full_plan(s.n3)


def max_grids(s):
    return len(plan(s)[0])


def start(n3, rng, dtype, coarsening="full"):
    s = S(tuple(n3), tuple(float(x) for x in rng), np.dtype(dtype).type, coarsening)
    return dataclasses.replace(s, numGrids=max_grids(s))


_SEEDS = {"a1": 21, "a2": 31, "c1": 22, "c2": 32, "g1": 5, "g2": 15, "v0": 6, "f": 7, "v1": 13}


@functools.lru_cache(maxsize=None)
def _field(name, n3, dtype):
    if name in ("ball", "plate", "black"):
        m = PR.ball(n3) if name == "ball" else PR.plate(n3, (n3[2] // 2) | 1) if name == "plate" else PR.point(n3, (2, 3, 4))
        m.setflags(write=False)
        return m
    u = np.random.default_rng(_SEEDS[name])
    if name[0] == "a":
        out = np.exp(u.uniform(-1.0, 1.0, O.shape(n3))).astype(dtype)
    elif name[0] == "c":
        out = u.uniform(0.5, 2.0, O.shape(n3)).astype(dtype)
    elif name == "v1":  # a coarse level's data with a non-zero rim
        out = u.uniform(0.5, 1.5, O.shape(n3)).astype(dtype)
    else:
        out = u.uniform(-1.0, 1.0, O.shape(n3)).astype(dtype)
    out.setflags(write=False)
    return out


def field(s, name, n3=None):
    """the seeded array of a name of the record (None: None), over level 0 or over n3; computed once, read-only"""
    return None if name is None else _field(name, tuple(n3 or s.n3), s.dtype)


def faces(bc):
    return [bool((bc >> k) & 1) for k in range(6)]


# ------------------------------------------------------------------------------------------ three ways to a hierarchy with the settings S
def fresh(ctx, s):
    """MultiGrid3D built directly from the constructor's keywords"""
    import pde_multigrid_amd as P
    kw = {}
    if s.bc:
        kw["neumann"] = faces(s.bc)
    if any(s.beta) or any(s.g):
        kw.update(robin=s.beta, wall_flux=s.g)
    mg = P.MultiGrid3D(ctx, s.n3, list(s.rng), s.dtype, residual_mode=P.CORRECT, coarsening=s.coarsening, shift=s.shift,
                       coefficient=field(s, s.a), capacity=field(s, s.c), face_mean=s.mean, pinned=field(s, s.pin),
                       pinned_values=field(s, s.pin_values), **kw)
    if s.numGrids != mg.maxGrids:
        mg.numGrids = s.numGrids
    return mg


def _truncate(H, k):
    """numGrids = k: the cycles of the restatement end at the last entry of `sizes`"""
    H.sizes = H.sizes[:k]
    return H


def operator(s):
    return R.Op(s.n3, list(s.rng), s.dtype, s.shift, field(s, s.a), field(s, s.c), s.bc, s.beta, s.mean)


def restated(s, always_pin=False):
    """op_restated.Hierarchy, or pin_restated.PinHierarchy when there are pins (always_pin: with an empty set too, for the hybrid of
    the observability test); the flux goes through its wall g and add_wall_flux"""
    if s.pin is None and not always_pin:
        return _truncate(R.Hierarchy(operator(s), s.coarsening, s.g), s.numGrids)
    pin = field(s, s.pin) if s.pin else np.zeros(O.shape(s.n3), bool)
    return _truncate(PR.PinHierarchy(operator(s), pin, field(s, s.pin_values), s.coarsening, wall_g=s.g), s.numGrids)


def hybrid(prev, now):
    """level 0 of `now` over the coarse levels of `prev`: their operators, coefficient arrays, pin sets and pin values"""
    H, old = restated(now, True), restated(prev, True)
    for name in ("ops", "a", "c", "pins", "gs"):
        getattr(H, name)[1:] = getattr(old, name)[1:]
    return H


def advance(s, step):
    """the record after one setter"""
    kind, val = step
    if kind == "shift":
        return dataclasses.replace(s, shift=float(np.dtype(s.dtype).type(val)))
    if kind == "coefficient":
        return dataclasses.replace(s, a=val)
    if kind == "capacity":
        return dataclasses.replace(s, c=val)
    if kind == "face_mean":
        return dataclasses.replace(s, mean=val)
    if kind == "neumann":
        return dataclasses.replace(s, bc=int(val))
    if kind == "wall":
        beta, g = val or (ZERO, ZERO)
        return dataclasses.replace(s, beta=tuple(float(x) for x in beta), g=tuple(float(x) for x in g))
    if kind == "pinned":
        pin, values = val or (None, None)
        return dataclasses.replace(s, pin=pin, pin_values=values)
    if kind == "numGrids":
        return dataclasses.replace(s, numGrids=max_grids(s) + int(val))  # val <= 0: levels below the maximum
    assert kind == "use_graph", kind
    return s


def apply(mg, s, step):
    """one setter on a live hierarchy; returns the new record"""
    kind, val = step
    new = advance(s, step)
    if kind == "shift":
        mg.shift = val
    elif kind == "coefficient":
        mg.set_coefficient(field(s, val))
    elif kind == "capacity":
        mg.set_capacity(field(s, val))
    elif kind == "face_mean":
        mg.set_face_mean(val)
    elif kind == "neumann":
        mg.set_neumann(faces(val))
    elif kind == "wall":
        mg.set_wall(new.beta, new.g)
    elif kind == "pinned":
        mg.set_pinned(field(s, new.pin), field(s, new.pin_values))
    elif kind == "numGrids":
        mg.numGrids = new.numGrids
    else:
        mg.use_graph = bool(val)
    return new


def drops_graphs(s, step):
    """does mg_multigrid.h say that this setter drops the captured graphs?  The shift and new values in the coefficient's arrays are
    read through the record instead, and a mean without a coefficient, numGrids and use_graph change no launch that was captured"""
    kind, val = step
    new = advance(s, step)
    if kind == "coefficient":
        return (s.a is None) != (val is None)
    if kind == "capacity":
        return not (s.c is None and val is None)
    if kind == "face_mean":
        return s.a is not None and s.mean != val
    if kind == "neumann":
        return s.bc != new.bc
    if kind == "wall":
        return (s.beta, s.g) != (new.beta, new.g)
    if kind == "pinned":
        return not (s.pin is None and new.pin is None)
    return False


def legal(s, step):
    """None, or why mg_multigrid.h refuses the step on a hierarchy with the settings s (or refuses to use the result)"""
    kind, val = step
    new = advance(s, step)
    if kind == "capacity" and val is not None and s.a is None:
        return "a capacity needs a coefficient"
    if kind == "coefficient" and val is None and s.c is not None:
        return "the coefficient cannot go while a capacity is set"
    if kind == "neumann":
        if new.bc and s.coarsening == "semi":
            return "a semi-coarsened hierarchy refuses masks"
        if any((s.beta[k] or s.g[k]) and not (new.bc >> k) & 1 for k in range(6)):
            return "a face can only be cleared once it carries no wall data"
    if kind == "wall" and any((new.beta[k] or new.g[k]) and not (s.bc >> k) & 1 for k in range(6)):
        return "wall data on a face the mask does not flag"
    if kind == "wall" and any(b < 0 for b in new.beta):
        return "beta < 0"
    if kind == "numGrids" and not 2 <= new.numGrids <= max_grids(s):
        return "numGrids outside 2 .. maxGrids (the probe cycles from level 1)"
    if kind == "shift" and not val >= 0:
        return "shift < 0"
    if not new.regular:
        return "the closed box needs a shift or a beta > 0" + (" (and pins refuse it)" if new.pin else "")
    return None


def changes_operator(s, step):
    return step[0] != "use_graph" and advance(s, step) != s


def reaches_coarse_levels(s, step):
    """False for the steps exempt, by name, from the hybrid check: the flux g alone (it touches level 0's right-hand side only,
    mg_multigrid.h _set_wall) and numGrids (no level's operator changes: the cycle ends elsewhere)"""
    new = advance(s, step)
    if step[0] == "numGrids":
        return False
    if step[0] == "wall" and new.beta == s.beta:
        return False
    return True


# ------------------------------------------------------------------------------------------ the walks
@dataclasses.dataclass(frozen=True)
class Walk:
    name: str
    n3: tuple
    rng: tuple
    coarsening: str
    graph: bool  # the long-lived hierarchy starts with use_graph (a use_graph step changes it)
    rot: int     # the disturbance of step i is number rot + i of the rotation
    steps: tuple
    ends_plain: bool = False


B1 = (0.0, 0.0, 1.5, 0.0, 0.0, 0.0)   # y-low convective (the walls of test_gpu_zzzz_pin.py, mask 0b100101)
B2 = (0.75, 0.0, 1.5, 0.0, 0.0, 2.0)  # x-low and z-high too
G1 = (0.5, 0.0, 0.0, 0.0, 0.0, -0.25)
B63 = (1.0, 0.0, 1.5, 0.0, 0.0, 2.0)  # what makes the closed box regular without a shift

WALKS = (
    Walk("walls on a non-cubic grid", (33, 17, 9), RG, "full", True, 0, (
        ("neumann", 0b100101), ("wall", (B1, ZERO)), ("wall", (B2, G1)), ("shift", 0.75), ("neumann", 0b110101), ("coefficient", "a1"),
        ("wall", (B1, G1)), ("face_mean", "harmonic"), ("neumann", 0b100101), ("capacity", "c1"), ("wall", (B2, ZERO)),
        ("pinned", ("ball", "g1")), ("neumann", 0b101101), ("numGrids", -1), ("wall", (B1, ZERO)), ("use_graph", False))),
    Walk("walls, second half", (33, 17, 9), RG, "full", False, 3, (
        ("shift", 0.75), ("neumann", 0b000011), ("neumann", 0b100111), ("pinned", ("plate", "g1")), ("wall", (B2, ZERO)),
        ("numGrids", -1), ("neumann", 0b110111), ("use_graph", True), ("wall", (B2, G1)), ("coefficient", "a1"), ("neumann", 0b100111),
        ("face_mean", "harmonic"), ("wall", (B2, ZERO)), ("capacity", "c1"), ("neumann", 0b101111), ("shift", 2.5))),
    Walk("the closed box, then everything cleared", (33, 17, 9), RG, "full", True, 5, (
        ("shift", 1.0), ("neumann", 63), ("shift", 2.5), ("wall", (B63, ZERO)), ("shift", 0.0), ("use_graph", False), ("neumann", 63 - 2),
        ("use_graph", True), ("wall", (ZERO, ZERO)), ("use_graph", False), ("use_graph", True), ("neumann", 0)), True),
    Walk("four levels: numGrids and the fields", (17, 33, 17), RG, "full", False, 1, (
        ("numGrids", -1), ("numGrids", -2), ("shift", 0.75), ("numGrids", 0), ("coefficient", "a1"), ("numGrids", -1),
        ("face_mean", "harmonic"), ("numGrids", 0), ("capacity", "c1"), ("numGrids", -1), ("pinned", ("ball", "g1")), ("numGrids", 0),
        ("use_graph", True), ("numGrids", -1), ("capacity", "c2"), ("capacity", None))),
    Walk("four levels: the fields among themselves", (17, 33, 17), RG, "full", True, 4, (
        ("coefficient", "a1"), ("coefficient", "a2"), ("shift", 0.75), ("shift", 2.5), ("capacity", "c1"), ("coefficient", "a1"),
        ("face_mean", "harmonic"), ("face_mean", "arithmetic"), ("shift", 0.75), ("face_mean", "harmonic"), ("capacity", "c2"),
        ("face_mean", "arithmetic"), ("coefficient", "a2"), ("capacity", "c1"), ("shift", 2.5), ("coefficient", "a1"))),
    Walk("four levels: pins", (17, 33, 17), RG, "full", False, 7, (
        ("pinned", ("ball", "g1")), ("pinned", ("plate", "g2")), ("shift", 0.75), ("pinned", ("ball", "g2")), ("coefficient", "a1"),
        ("pinned", ("black", "g1")), ("face_mean", "harmonic"), ("pinned", ("ball", "g1")), ("capacity", "c1"),
        ("pinned", ("plate", "g1")), ("use_graph", True), ("pinned", ("ball", "g1")), ("numGrids", -1), ("face_mean", "arithmetic"),
        ("pinned", None), ("capacity", None))),
    Walk("semi-coarsened", (9, 9, 65), RG, "semi", True, 2, (
        ("coefficient", "a1"), ("use_graph", False), ("coefficient", "a2"), ("shift", 0.75), ("use_graph", True), ("shift", 2.5),
        ("capacity", "c1"), ("use_graph", False), ("capacity", "c2"), ("face_mean", "harmonic"), ("use_graph", True),
        ("face_mean", "arithmetic"), ("pinned", ("ball", "g1")), ("use_graph", False), ("pinned", ("plate", "g1")), ("numGrids", -2))),
    Walk("there and back to plain", (33, 33, 33), UNIT, "full", False, 2, (
        ("use_graph", True), ("shift", 0.75), ("coefficient", "a1"), ("neumann", 0b000100), ("capacity", "c1"), ("pinned", ("ball", "g1")),
        ("numGrids", -2), ("pinned", None), ("wall", (B1, ZERO)), ("wall", None), ("neumann", 0), ("capacity", None), ("coefficient", None),
        ("shift", 0.0), ("numGrids", 0)), True),
)


# ------------------------------------------------------------------------------------------ the disturbances
DISTURBANCES = ("Eigen(2)", "PCG in every krylov mode", "PCG(precond='f32')", "BackwardEuler(1)", "VCycle(1, 1, 1)", "upload_v(1)",
                "setToValue_v", "a refused setter")


def _applies(name, s, step):
    fp64 = np.dtype(s.dtype) == np.float64
    if name == "Eigen(2)":
        return fp64 and s.pin is None
    if name == "PCG(precond='f32')":  # (an fp32 hierarchy has no fp32 twin: the wrapper refuses before the library is asked)
        return fp64
    if name == "BackwardEuler(1)":  # it replaces a shift the walk has: the stretches about the unshifted operator stay unshifted;
        return s.shift != 0 and step[0] != "shift"  # not the one this step has just set, which the probe could then not see
    return True


def disturbance(s, i, step):
    """number i of the rotation, or the next one that the settings (and the step they come from) allow"""
    for k in range(len(DISTURBANCES)):
        name = DISTURBANCES[(i + k) % len(DISTURBANCES)]
        if _applies(name, s, step):
            return name
    raise AssertionError("no disturbance applies")


def after_disturbance(s, name):
    """the record after a disturbance: BackwardEuler's shift stays set (mg_multigrid.h: "The shift it sets STAYS SET afterwards")"""
    if name == "BackwardEuler(1)":
        return dataclasses.replace(s, shift=float(np.dtype(s.dtype).type(1.0 / (BE_KAPPA * BE_DT))))
    return s


def krylov_modes(s):
    """PCG's modes on a hierarchy with the settings s: krylov = True is refused with a mask"""
    return (False, "weighted") if s.bc else (False, True, "weighted")


@dataclasses.dataclass(frozen=True)
class State:
    index: int
    step: tuple
    prev_step: tuple
    before: S         # the settings the setter meets
    set: S            # ... and leaves
    disturbance: str
    now: S            # the settings the probe meets
    use_graph: bool


def states(walk, dtype):
    """the walk, step by step"""
    s = start(walk.n3, walk.rng, dtype, walk.coarsening)
    graph, prev, out = walk.graph, None, []
    for i, step in enumerate(walk.steps):
        mid = advance(s, step)
        if step[0] == "use_graph":
            graph = bool(step[1])
        d = disturbance(mid, walk.rot + i, step)
        now = after_disturbance(mid, d)
        out.append(State(i, step, prev, s, mid, d, now, graph))
        s, prev = now, step
    return out


def refusals(s):
    """setter calls that a hierarchy with the settings s must refuse (from the refusal tests of the feature files), as
    (name, call(mg)); every one applies to every s unless it says otherwise"""
    shape = O.shape(s.n3)
    bad_a = np.ones(shape, s.dtype)
    bad_a[1, 2, 3] = -1.0
    bad_pin = np.zeros(shape, bool)
    bad_pin[4, 0, 3] = True
    out = [("shift = -1", lambda mg: setattr(mg, "shift", -1.0)),
           ("a coefficient with a negative entry", lambda mg: mg.set_coefficient(bad_a)),
           ("a pin on the boundary", lambda mg: mg.set_pinned(bad_pin)),
           ("face_mean 7", lambda mg: mg._call("set_face_mean", 7))]
    if s.a is None:
        out.append(("a capacity without a coefficient", lambda mg: mg.set_capacity(np.ones(shape, s.dtype))))
    if s.c is not None:
        out.append(("the coefficient cleared under a capacity", lambda mg: mg.set_coefficient(None)))
    if s.coarsening == "semi":
        out.append(("a mask on a semi-coarsened hierarchy", lambda mg: mg.set_neumann([1, 0, 0, 0, 0, 0])))
    if s.bc != 63:
        k = [k for k in range(6) if not (s.bc >> k) & 1][0]
        beta = list(s.beta)
        beta[k] = 1.0
        out.append(("a beta on a face the mask does not flag", lambda mg: mg.set_wall(beta, s.g)))
    if any(s.beta) or any(s.g):
        out.append(("a face cleared while it carries wall data", lambda mg: mg.set_neumann(None)))
    return out


# ------------------------------------------------------------------------------------------ the probe
class Lib:
    """a library hierarchy under the probe"""

    def __init__(self, mg, ctx):
        self.mg, self.ctx = mg, ctx

    def upload(self, v0, f):
        self.mg.upload_v(0, v0)
        if f is not None:
            self.mg.upload_f(0, f)

    def add_wall_flux(self):
        self.mg.add_wall_flux()

    def relax(self, l, k):
        self.mg.Relax(l, k)

    def residual(self, l):
        return self.mg.CalculateResidual(l)

    def norm(self, l):
        return self.mg.ResidualNorm(l)

    def vcycle(self, l, v1, v2):
        self.mg.VCycle(l, v1, v2)

    def fmg(self, l, v0, v1, v2):
        self.mg.FullMultiGridVCycle(l, v0, v1, v2)

    def v(self, l):
        return self.mg.download_v(l)

    def f(self, l):
        return self.mg.download_f(l)

    def pcg(self, v1, v2, tol, maxit):
        return self.mg.PCG(v1, v2, tol, maxit, krylov="weighted")

    def kernels(self):
        c = self.ctx
        return (c.last_relax_kernel(), c.last_rr_kernel(), c.last_corr_kernel(), c.last_block3_kernel())

    def graph(self):
        """(is there a captured cycle from level 0, the record it was captured under), None on an eager hierarchy"""
        if not self.mg.use_graph:
            return None
        m = self.mg._mg.contents
        return bool(m.graph_exec[0]), bytes(m.graph_rec[0])


class Rest:
    """a restated hierarchy under the probe: the thin adapter"""

    def __init__(self, H):
        self.H = H

    def upload(self, v0, f):
        H = self.H
        if isinstance(H, PR.PinHierarchy):
            H.set_v(v0)
        else:
            H.v[0] = np.array(v0, H.ops[0].dtype)
        if f is not None:
            H.f[0] = np.array(f, H.ops[0].dtype)

    def add_wall_flux(self):
        self.H.add_wall_flux()

    def relax(self, l, k):
        self.H.relax(l, k)

    def residual(self, l):
        return self.H.residual(l)

    def norm(self, l):
        return math.sqrt(R.fsum_sq(self.H.residual(l)))

    def vcycle(self, l, v1, v2):
        self.H.vcycle(l, v1, v2)

    def fmg(self, l, v0, v1, v2):
        self.H.fmg(l, v0, v1, v2)

    def v(self, l):
        return self.H.v[l].copy()

    def f(self, l):
        return self.H.f[l].copy()

    def pcg(self, v1, v2, tol, maxit):
        return None  # (the feature files compare PCG with the restated solver)

    def kernels(self):
        return None

    def graph(self):
        return None


@dataclasses.dataclass
class Probed:
    items: list      # (call, level, array name, value) in call order
    kernels: tuple   # the four last_*_kernel names after the first V-cycle
    replay: tuple    # graph() before and after the third V-cycle
    pcg: tuple       # (k, rel, conv, hist) or None


def probe(h, s):
    """the call sequence of the issue on a hierarchy with the settings s.  Level 0's arrays are recorded after every call, the levels
    below from the first V-cycle on -- before it they hold what the hierarchy's history left there, which no call of the probe reads:
    every cycle writes a coarse level whole before it reads it.  PCG starts from the uploaded v0 again, as the solves of the feature
    files do: from the iterate FullMultiGridVCycle leaves, a relative tolerance would ask fp32 for what it cannot give."""
    v0, f = field(s, "v0"), field(s, "f")
    items = []

    def top(call):
        items.append((call, 0, "v", h.v(0)))
        items.append((call, 0, "f", h.f(0)))

    def levels(call):
        for l in range(s.numGrids):
            items.append((call, l, "v", h.v(l)))
            items.append((call, l, "f", h.f(l)))

    h.upload(v0, f)
    if any(s.g):
        h.add_wall_flux()
    top("upload + add_wall_flux")
    h.relax(0, 1)
    top("Relax(0, 1)")
    items.append(("CalculateResidual(0)", 0, "r", h.residual(0)))
    items.append(("ResidualNorm(0)", 0, "norm", h.norm(0)))
    kernels = replay = None
    for i in range(3):
        before = h.graph()
        h.vcycle(0, 2, 2)
        if i == 0:
            kernels = h.kernels()
        if i == 2:
            replay = (before, h.graph())
        levels("VCycle(0, 2, 2) #%d" % (i + 1))
    h.fmg(0, 1, 2, 2)
    levels("FullMultiGridVCycle(0, 1, 2, 2)")
    if s.numGrids > 1:
        h.vcycle(1, 1, 1)
        levels("VCycle(1, 1, 1)")
    h.upload(v0, None)
    res = h.pcg(2, 2, pcg_tol(s.dtype), PCG_MAXIT)
    if res is not None:
        k, rel, conv, hist = res
        items += [("PCG", 0, "k", k), ("PCG", 0, "conv", conv), ("PCG", 0, "hist", np.asarray(hist)), ("PCG", 0, "x", h.v(0)), ("PCG", 0, "f", h.f(0))]
    return Probed(items, kernels, replay, res)


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return False
        return a.tobytes() == b.tobytes()
    return a == b


def first_difference(A, B, skip=("norm",), calls=None, level0=False):
    """None when the items of two probes agree bit for bit, else "call, level, array, first index" of the first that does not.  skip:
    array names left out (the norm is compared by its tolerance, PCG's by the caller); calls: only these; level0: only level 0"""
    def keep(it):
        return it[2] not in skip and (calls is None or it[0] in calls) and not (level0 and it[1] != 0)
    a, b = [it for it in A.items if keep(it)], [it for it in B.items if keep(it)]
    for x, y in zip(a, b):
        if x[:3] != y[:3]:
            return "the probes differ in their calls: %r against %r" % (x[:3], y[:3])
        if not _same(x[3], y[3]):
            where = ""
            if isinstance(x[3], np.ndarray) and isinstance(y[3], np.ndarray) and x[3].shape == y[3].shape and x[3].ndim == 3:
                w = np.uint32 if x[3].dtype == np.float32 else np.uint64
                z, yy, xx = np.argwhere(np.ascontiguousarray(x[3]).view(w) != np.ascontiguousarray(y[3]).view(w))[0]
                where = ", first at (x, y, z) = (%d, %d, %d): %r against %r" % (xx, yy, z, x[3][z, yy, xx], y[3][z, yy, xx])
            elif not isinstance(x[3], np.ndarray):
                where = ": %r against %r" % (x[3], y[3])
            return "%s, level %d, %s%s" % (x[0], x[1], x[2], where)
    if len(a) != len(b):
        return "the probes differ in length: %d items against %d" % (len(a), len(b))
    return None


def item(p, call, level, name):
    for it in p.items:
        if it[:3] == (call, level, name):
            return it[3]
    raise KeyError((call, level, name))


# ------------------------------------------------------------------------------------------ the restated solve
@contextlib.contextmanager
def _levels(k):
    """op_restated.fcg and pin_restated.pin_fcg build their own hierarchy: inside, those end at numGrids = k"""
    h0, p0 = R.Hierarchy, PR.PinHierarchy
    R.Hierarchy = lambda *a, **kw: _truncate(h0(*a, **kw), k)
    PR.PinHierarchy = lambda *a, **kw: _truncate(p0(*a, **kw), k)
    try:
        yield
    finally:
        R.Hierarchy, PR.PinHierarchy = h0, p0


def restated_solve(s, maxit=PCG_MAXIT):
    """the probe's PCG by the restated solver: (iterations, converged, true relative residual)"""
    op = operator(s)
    f = op.add_flux(field(s, "f"), s.g) if any(s.g) else field(s, "f")
    with _levels(s.numGrids):
        if s.pin is None:
            x, k, hist, conv, rel, _ = R.fcg(op, field(s, "v0"), f, pcg_tol(s.dtype), maxit, 2, 2, s.coarsening)
        else:
            x, k, hist, conv, rel = PR.pin_fcg(op, field(s, s.pin), field(s, s.pin_values), field(s, "v0"), f, pcg_tol(s.dtype), maxit, 2, 2,
                                               s.coarsening)
    return k, conv, rel


# ------------------------------------------------------------------------------------------ coverage
def pairs(walks=WALKS):
    """{(kind A, kind B): [(walk name, index of B's step)]} over every A immediately followed by B; a kind that follows itself counts
    only with another value"""
    out = {}
    for w in walks:
        for i in range(1, len(w.steps)):
            (ka, va), (kb, vb) = w.steps[i - 1], w.steps[i]
            if ka == kb and va == vb:
                continue
            out.setdefault((ka, kb), []).append((w.name, i))
    return out


def coverage_table(walks=WALKS):
    """the pairs x walks table of the issue, as text: rows = the first kind, columns = the second, entries = the walks' numbers"""
    got = pairs(walks)
    number = {w.name: str(i) for i, w in enumerate(walks)}
    lines = ["%-12s" % "A \\ B" + "".join("%-12s" % k[:11] for k in KINDS)]
    for a in KINDS:
        lines.append("%-12s" % a[:11] + "".join("%-12s" % ",".join(sorted({number[n] for n, _ in got.get((a, b), [])}) or ["-"])[:11] for b in KINDS))
    return "\n".join(lines)
