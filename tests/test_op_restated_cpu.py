"""The bits of tests/op_restated.py are pinned: tests/golden/restated_digests.json holds, per case, one SHA-256 digest over the result
arrays and the exact integers and float.hex() strings of the scalars that the seven per-operator restatements gave which op_restated
replaced -- every case through the module that owned it and through every other module that could express it, all of which agreed.
Every case listed in the fixture is recomputed here and compared exactly; a case this file cannot compute is a failure."""
import hashlib
import json
import os

import numpy as np
import pytest

import op_cases as C
import op_restated as R
import oracle as O

with open(os.path.join(os.path.dirname(__file__), "golden", "restated_digests.json")) as fh:
    FIXTURE = json.load(fh)
RNG = [0, 1, 0, 2, 0.5, 3]  # the three spacings differ on every grid below
S_OF = {"shift0": 0.0, "shift35": 3.5, "coef": 0.75, "cap": 0.75, "cap0": 0.75}
WALL_BETA, WALL_G = (2.0, 0.0, 0.5, 0.0, 0.0, 1.0), (0.0, 1.5, 0.0, 0.0, -0.5, 1.0)
SOLVE_KEYS = ("x", "iterations", "history", "converged", "true_rel", "removed")


def rec(x):
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    return float(x).hex()


def arrays_digest(results):
    """SHA-256 over the name, dtype, shape and SHA-256 of every result array, in the order of the names"""
    lines = ["%s %s %s %s\n" % (k, x.dtype.name, list(x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest())
             for k, x in sorted(results.items()) if isinstance(x, np.ndarray)]
    return hashlib.sha256("".join(lines).encode()).hexdigest()


def draw(n3, dtype, seed, k):
    g = np.random.default_rng(seed)
    return [g.uniform(-1, 1, O.shape(n3)).astype(dtype) for _ in range(k)]


def operator(n3, dtype, op, bc=0, beta="zeros", mean="arithmetic", rng=RNG):
    a = None if op.startswith("shift") else C.smooth_coefficient(n3, dtype)
    c = C.smooth_capacity(n3, dtype) if op == "cap" else C.random_capacity(n3, dtype, 3) if op == "cap0" else None
    b = beta if isinstance(beta, tuple) else C.mixed_betas(bc) if beta == "mixed" else R.ZERO
    return R.Op(n3, rng, dtype, S_OF[op], a, c, bc, b, mean)


def point(n3, dtype, op, bc, beta, mean):
    A = operator(n3, dtype, op, bc, beta, mean)
    v, f, q = draw(n3, dtype, 2, 3)
    flux = tuple((k - 1.5) if (bc >> k) & 1 else 0.0 for k in range(6))
    return {"relax": A.relax(v, f, 2), "residual": A.residual(v, f), "apply_A": A.apply_A(v), "rhs": A.rhs(v, q, 0.7), "add_flux": A.add_flux(f, flux)}


def cycle(n3, dtype, op, bc, beta, mean, coarsening):
    v, f = draw(n3, dtype, 5, 2)
    H = R.Hierarchy(operator(n3, dtype, op, bc, beta, mean), coarsening)
    H.v[0], H.f[0] = v.copy(), f.copy()
    H.vcycle(0, 2, 2)
    out = {"vcycle_v0": H.v[0].copy(), "vcycle_fcoarsest": H.f[-1].copy()}
    H = R.Hierarchy(operator(n3, dtype, op, bc, beta, mean), coarsening)
    H.f[0] = f.copy()
    H.fmg(0, 1, 2, 2)
    return dict(out, fmg_v0=H.v[0], fmg_fcoarsest=H.f[-1])


def cycles_to(n3, dtype, op, bc):
    v, f = draw(n3, dtype, 7, 2)
    out = R.cycles_to(operator(n3, dtype, op, bc), v, f, 2, 2, 1e-4 if dtype == np.float32 else 1e-9, 30)
    return dict(zip(("x", "cycles", "rel", "converged"), out))


def fcg(n3, dtype, loop):
    """one case per flexible-CG loop the fixture's modules had"""
    v0, f = C.start(n3, dtype)
    a, c = C.smooth_coefficient(n3, dtype), C.smooth_capacity(n3, dtype)
    zero, kw = np.zeros_like(v0), {}
    op, v0 = {
        "shift": (R.Op(n3, C.UNIT, dtype, 3.5), v0),
        "coef": (R.Op(n3, C.UNIT, dtype, 0.75, a), v0),
        "coef_semi": (R.Op(n3, RNG, dtype, 0.75, a), v0),
        "neumann": (R.Op(n3, C.UNIT, dtype, 0.0, a, bc=37), v0),
        "closed_box": (R.Op(n3, C.UNIT, dtype, 0.0, a, bc=63), zero),
        "closed_box_plain_dots": (R.Op(n3, C.UNIT, dtype, 0.0, bc=63), zero),
        "cap": (R.Op(n3, C.UNIT, dtype, 100.0, a, c, 37), v0),
        "cap_semi": (R.Op(n3, RNG, dtype, 100.0, a, c), v0),
        "lossy_wall": (R.Op(n3, C.UNIT, dtype, 0.0, a, bc=63, beta=WALL_BETA), v0),
        "harmonic": (R.Op(n3, C.UNIT, dtype, 0.75, C.jump_coefficient(n3, 100, dtype), c, 37, C.mixed_betas(37), "harmonic"), v0),
    }[loop]
    if loop.endswith("_semi"):
        kw["coarsening"] = "semi"
    if loop == "closed_box_plain_dots":
        kw["weighted"] = False
    return dict(zip(SOLVE_KEYS, R.fcg(op, v0, f, tol=1e-4 if dtype == np.float32 else 1e-10, **kw)))


def euler(n3, dtype, op, bc, walls, mean):
    H = R.Hierarchy(operator(n3, dtype, op, bc, WALL_BETA if walls else R.ZERO, mean), g=WALL_G if walls else R.ZERO)
    H.v[0] = C.gaussian(n3).astype(dtype)
    out = H.backward_euler(2, 1e-2, 0.5, 2, 2, 1e-4 if dtype == np.float32 else 1e-9, 30, source=draw(n3, dtype, 9, 1)[0])
    return dict(zip(("v0", "cycles", "worst", "converged"), (H.v[0],) + tuple(out)))


def table(n3, dtype, case):
    out = C.solved(case, n3[0], dtype)
    assert out[1] == C.CASES[case][3]
    return dict(zip(SOLVE_KEYS, out))


KINDS = {"point": point, "cycle": cycle, "cycles_to": cycles_to, "fcg": fcg, "euler": euler, "table": table}


def test_the_fixture_is_not_thinned():
    assert len(FIXTURE) >= 150, len(FIXTURE)
    assert {name.split(":")[0] for name in FIXTURE} == set(KINDS)


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_op_restated_has_the_recorded_bits(name):
    kind, _, params = name.partition(":")
    kw = dict(p.split("=") for p in params.split(","))
    n3 = tuple(int(k) for k in kw.pop("grid").split("x"))
    dtype = np.dtype(kw.pop("dtype")).type
    for k in ("bc", "walls", "case"):
        if k in kw:
            kw[k] = int(kw[k])
    got = KINDS[kind](n3, dtype, **kw)
    want = FIXTURE[name]
    assert arrays_digest(got) == want["arrays"], name
    scalars = set(want) - {"arrays"}
    for k in scalars:  # (without `removed` where only loops that returned no mean owned the case)
        assert rec(got[k]) == want[k], (name, k)
