#!/usr/bin/env python3
"""How tests/golden/restated_digests.json was made -- kept so that the pin can be audited, not run by any test.  It needs the seven
per-operator restatements that tests/op_restated.py replaced (tests/{shift,coef,neumann,neumann_krylov,cap,robin,hmean}_restated.py),
so it runs only in a checkout of the last commit that has them, from that checkout's root with the library and the oracle built:

    git worktree add ../parent 0a6eacb && cd ../parent && python -c "import __graft_entry__ as g; g.build()"
    python <this file> OUT.json        # OUT.json is tests/golden/restated_digests.json, byte for byte

Every case goes through the module that owned it and through every other module that can express it; `one()` fails if two of them
disagree on a result."""
import hashlib, itertools, json, os, sys

import numpy as np

ROOT = os.getcwd()
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
import cap_restated as CA, coef_restated as CO, hmean_restated as HM, neumann_krylov_restated as NK
import neumann_restated as NR, oracle as O, robin_restated as RR, shift_restated as SH

RNG, UNIT, ZERO = [0, 1, 0, 2, 0.5, 3], [0, 1, 0, 1, 0, 1], (0.0,) * 6
GRIDS = {"9x9x17": (9, 9, 17), "17x9x9": (17, 9, 9), "17x17x17": (17, 17, 17)}
OPS = {"shift0": 0.0, "shift35": 3.5, "coef": 0.75, "cap": 0.75, "cap0": 0.75}  # name -> s


def fields(op, n3, dtype):
    a = None if op.startswith("shift") else CO.smooth_coefficient(n3, dtype)
    c = CA.smooth_capacity(n3, dtype) if op == "cap" else CA.random_capacity(n3, dtype, 3) if op == "cap0" else None
    return a, c


def rec(x):
    if isinstance(x, np.ndarray):
        return {"dtype": x.dtype.name, "shape": list(x.shape), "sha256": hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()}
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    return float(x).hex()


def pack(recs):
    """one digest per case: SHA-256 over the name, dtype, shape and digest of every result array; the scalars as they are"""
    lines = ["%s %s %s %s\n" % (k, r["dtype"], r["shape"], r["sha256"]) for k, r in sorted(recs.items()) if isinstance(r, dict)]
    return dict({k: r for k, r in recs.items() if not isinstance(r, dict)}, arrays=hashlib.sha256("".join(lines).encode()).hexdigest())


def one(routes, what):
    """the one record all routes agree on"""
    recs = {k: rec(v) for k, v in routes.items()}
    first = next(iter(recs.values()))
    assert all(r == first for r in recs.values()), (what, recs)
    return first


def draw(n3, dtype, seed, k):
    g = np.random.default_rng(seed)
    return [g.uniform(-1, 1, O.shape(n3)).astype(dtype) for _ in range(k)]


def flux(bc):
    return tuple((k - 1.5) if (bc >> k) & 1 else 0.0 for k in range(6))


def point(op, bc, beta, mean, dtype, n3):
    s = OPS[op]
    a, c = fields(op, n3, dtype)
    v, f, q = draw(n3, dtype, 2, 3)
    b = RR.mixed_betas(bc) if beta == "mixed" else ZERO
    R = {k: {} for k in ("relax", "residual", "apply_A", "rhs", "add_flux")}
    ar, nowall = mean == "arithmetic", beta == "zeros"
    if ar and nowall and a is None and bc == 0:
        R["relax"]["SH"], R["residual"]["SH"] = SH.relax(n3, RNG, v, f, s, 2, dtype), SH.residual(n3, RNG, v, f, s, dtype)
        R["apply_A"]["SH"], R["rhs"]["SH"] = SH.apply_A(n3, RNG, v, s, dtype), SH.rhs(v, q, 0.7, s, dtype)
    if ar and nowall and a is not None and c is None and bc == 0:
        R["relax"]["CO"], R["residual"]["CO"] = CO.relax(n3, RNG, v, f, a, s, 2, dtype), CO.residual(n3, RNG, v, f, a, s, dtype)
        R["apply_A"]["CO"] = CO.apply_A(n3, RNG, v, a, s, dtype)
    if ar and nowall and c is None:
        R["relax"]["NR"], R["residual"]["NR"] = NR.relax(n3, RNG, v, f, a, s, 2, bc, dtype), NR.residual(n3, RNG, v, f, a, s, bc, dtype)
        R["apply_A"]["NR"] = NR.apply_A(n3, RNG, v, a, s, bc, dtype)
        R["rhs"]["NR"] = NR.rhs(v, q, 0.7, s, bc, dtype)
    if ar and nowall and c is not None:
        R["relax"]["CA"], R["residual"]["CA"] = CA.relax(n3, RNG, v, f, a, c, s, 2, dtype, bc), CA.residual(n3, RNG, v, f, a, c, s, dtype, bc)
        R["apply_A"]["CA"] = CA.apply_A(n3, RNG, v, a, c, s, dtype, bc)
    if c is not None:  # the right-hand side knows neither walls nor means
        R["rhs"]["CA"] = CA.rhs(v, c, q, 0.7, s, dtype, bc)
    else:
        R["rhs"]["NR'"] = NR.rhs(v, q, 0.7, s, bc, dtype)
    if ar:
        R["relax"]["RR"], R["residual"]["RR"] = RR.relax(n3, RNG, v, f, a, c, s, 2, bc, b, dtype), RR.residual(n3, RNG, v, f, a, c, s, bc, b, dtype)
        R["apply_A"]["RR"] = RR.apply_A(n3, RNG, v, a, c, s, bc, b, dtype)
    if a is not None:
        R["relax"]["HM"], R["residual"]["HM"] = HM.relax(n3, RNG, v, f, a, s, 2, dtype, c, bc, b, mean), HM.residual(n3, RNG, v, f, a, s, dtype, c, bc, b, mean)
        R["apply_A"]["HM"] = HM.apply_A(n3, RNG, v, a, s, dtype, c, bc, b, mean)
    R["add_flux"]["RR"] = RR.add_flux(n3, RNG, f, flux(bc), bc, dtype)
    return {k: one(r, k) for k, r in R.items()}


def hierarchies(op, bc, beta, mean, dtype, n3, coarsening, g=ZERO):
    """every parent hierarchy that expresses the case"""
    s = OPS[op]
    a, c = fields(op, n3, dtype)
    b = beta if isinstance(beta, tuple) else RR.mixed_betas(bc) if beta == "mixed" else ZERO
    ar, nowall, full = mean == "arithmetic", not any(b) and g == ZERO, coarsening == "full"
    H = {}
    if ar and nowall and a is None and bc == 0:
        H["SH"] = SH.Hierarchy(n3, RNG, s, dtype, coarsening)
    if ar and nowall and a is not None and c is None and bc == 0:
        H["CO"] = CO.Hierarchy(n3, RNG, a, s, dtype, coarsening)
    if ar and nowall and c is None and full:
        H["NR"] = NR.Hierarchy(n3, RNG, a, s, bc, dtype)
    if ar and nowall and c is not None:
        H["CA"] = CA.Hierarchy(n3, RNG, a, c, s, bc, dtype, coarsening)
    if ar and full:  # robin_restated.Hierarchy takes the mask's transfers whatever the mask
        H["RR"] = RR.Hierarchy(n3, RNG, a, c, s, bc, b, g, dtype)
    if a is not None:
        H["HM"] = HM.Hierarchy(n3, RNG, a, s, c, bc, b, g, dtype, coarsening, mean)
    assert H, (op, bc, beta, mean, coarsening)
    return H


def cycle(op, bc, beta, mean, dtype, n3, coarsening):
    R = {k: {} for k in ("vcycle_v0", "vcycle_fcoarsest", "fmg_v0", "fmg_fcoarsest")}
    v, f = draw(n3, dtype, 5, 2)
    for name, H in hierarchies(op, bc, beta, mean, dtype, n3, coarsening).items():
        H.v[0], H.f[0] = v.copy(), f.copy()
        H.vcycle(0, 2, 2)
        R["vcycle_v0"][name], R["vcycle_fcoarsest"][name] = H.v[0].copy(), H.f[-1].copy()
    for name, H in hierarchies(op, bc, beta, mean, dtype, n3, coarsening).items():
        H.f[0] = f.copy()
        H.fmg(0, 1, 2, 2)
        R["fmg_v0"][name], R["fmg_fcoarsest"][name] = H.v[0].copy(), H.f[-1].copy()
    return {k: one(r, k) for k, r in R.items()}


def cycles_to(op, bc, dtype, n3):
    s, tol = OPS[op], 1e-4 if dtype == np.float32 else 1e-9
    a, c = fields(op, n3, dtype)
    v, f = draw(n3, dtype, 7, 2)
    R = {k: {} for k in ("x", "cycles", "rel", "converged")}

    def put(name, out):
        for k, val in zip(R, out):
            R[k][name] = val
    if a is None and bc == 0:
        put("SH", SH.cycles_to(n3, RNG, s, v, f, 2, 2, tol, 30, dtype))
    if a is not None and c is None and bc == 0:
        put("CO", CO.cycles_to(n3, RNG, a, s, v, f, 2, 2, tol, 30, dtype))
    for name, H in hierarchies(op, bc, "zeros", "arithmetic", dtype, n3, "full").items():
        if hasattr(H, "cycle_to"):
            H.v[0], H.f[0] = v.copy(), f.copy()
            k, rel, conv = H.cycle_to(2, 2, tol, 30)
            put(name, (H.v[0], k, rel, conv))
    return {k: one(r, k) for k, r in R.items()}


def fcg(loop, dtype, n3):
    """every parent CG loop on a case of its own (and through every other loop that expresses the case)"""
    tol = 1e-4 if dtype == np.float32 else 1e-10
    v0, f = NK.start(n3, dtype)
    a, c = CO.smooth_coefficient(n3, dtype), CA.smooth_capacity(n3, dtype)
    keys = ("x", "iterations", "history", "converged", "true_rel", "removed")
    R = {k: {} for k in keys}

    def put(name, out):
        for k, val in zip(keys, out):
            R[k][name] = np.asarray(val, np.float64) if k == "history" else val
    if loop == "shift":  # the two loops without weights take the cycle as an argument and report neither true_rel nor a mean
        put("SH", SH.fcg_restated(n3, UNIT, 3.5, v0, f, SH.m_cycle(n3, UNIT, 3.5, 2, 2, dtype), tol, 60, dtype))
        put("NK", NK.wfcg(n3, UNIT, None, 3.5, 0, v0, f, tol=tol, dtype=dtype))
    elif loop == "coef":
        put("CO", CO.fcg_restated(n3, UNIT, a, 0.75, v0, f, CO.m_cycle(n3, UNIT, a, 0.75, 2, 2, dtype), tol, 60, dtype))
        put("NK", NK.wfcg(n3, UNIT, a, 0.75, 0, v0, f, tol=tol, dtype=dtype))
        put("HM", HM.fcg(n3, UNIT, a, 0.75, v0, f, tol=tol, dtype=dtype, mean="arithmetic"))
    elif loop == "coef_semi":
        put("CO", CO.fcg_restated(n3, RNG, a, 0.75, v0, f, CO.m_cycle(n3, RNG, a, 0.75, 2, 2, dtype, "semi"), tol, 60, dtype))
        put("HM", HM.fcg(n3, RNG, a, 0.75, v0, f, tol=tol, dtype=dtype, coarsening="semi", mean="arithmetic"))
    elif loop == "neumann":
        put("NK", NK.wfcg(n3, UNIT, a, 0.0, 37, v0, f, tol=tol, dtype=dtype))
        put("RR", RR._wfcg(n3, UNIT, a, None, 0.0, 37, ZERO, v0, f, tol, 60, 2, 2, dtype))
    elif loop == "closed_box":  # mask 63 without a shift: the projection
        put("NK", NK.wfcg(n3, UNIT, a, 0.0, 63, np.zeros_like(v0), f, tol=tol, dtype=dtype))
    elif loop == "closed_box_plain_dots":
        put("NK", NK.wfcg(n3, UNIT, None, 0.0, 63, np.zeros_like(v0), f, tol=tol, dtype=dtype, weighted=False))
    elif loop == "cap":
        put("CA", CA.fcg(n3, UNIT, a, c, 100.0, 37, v0, f, tol=tol, dtype=dtype))
        put("RR", RR._wfcg(n3, UNIT, a, c, 100.0, 37, ZERO, v0, f, tol, 60, 2, 2, dtype))
        put("HM", HM.fcg(n3, UNIT, a, 100.0, v0, f, c, 37, tol=tol, dtype=dtype, mean="arithmetic"))
    elif loop == "cap_semi":
        put("CA", CA.fcg(n3, RNG, a, c, 100.0, 0, v0, f, tol=tol, dtype=dtype, coarsening="semi"))
    elif loop == "lossy_wall":
        beta = (2.0, 0.0, 0.5, 0.0, 0.0, 1.0)
        put("RR", RR.wfcg(n3, UNIT, a, None, 0.0, 63, beta, v0, f, tol=tol, dtype=dtype))
        put("HM", HM.fcg(n3, UNIT, a, 0.0, v0, f, None, 63, beta, tol=tol, dtype=dtype, mean="arithmetic"))
    elif loop == "harmonic":
        put("HM", HM.fcg(n3, UNIT, CO.jump_coefficient(n3, 100, dtype), 0.75, v0, f, c, 37, RR.mixed_betas(37), tol=tol, dtype=dtype))
    if not R["true_rel"]:
        del R["true_rel"]
    if not R["removed"]:
        del R["removed"]
    else:
        assert all(m == 0.0 for m in R["removed"].values()) or loop.startswith("closed_box")
    return {k: one(r, k) for k, r in R.items()}


def euler(op, bc, walls, mean, dtype, n3):
    a, c = fields(op, n3, dtype)
    beta, g = ((2.0, 0.0, 0.5, 0.0, 0.0, 1.0), (0.0, 1.5, 0.0, 0.0, -0.5, 1.0)) if walls else (ZERO, ZERO)
    tol = 1e-4 if dtype == np.float32 else 1e-9
    src = draw(n3, dtype, 9, 1)[0]
    R = {k: {} for k in ("v0", "cycles", "worst", "converged")}
    Hs = {k: H for k, H in hierarchies(op, bc, beta, mean, dtype, n3, "full", g).items() if hasattr(H, "backward_euler")}
    for name, H in Hs.items():
        H.v[0] = NR.gaussian(n3).astype(dtype)
        out = H.backward_euler(2, 1e-2, 0.5, 2, 2, tol, 30, source=src)
        for k, val in zip(R, (H.v[0],) + tuple(out)):
            R[k][name] = val
    return {k: one(r, k) for k, r in R.items()}


def name(kind, **kw):
    return kind + ":" + ",".join("%s=%s" % (k, v) for k, v in kw.items())


def main(out):
    D = {}
    for dt, grid in itertools.product(("float32", "float64"), ("9x9x17", "17x9x9")):
        dtype, n3 = np.dtype(dt).type, GRIDS[grid]
        for op, bc, beta, mean in itertools.product(OPS, (0, 37, 63), ("zeros", "mixed"), ("arithmetic", "harmonic")):
            if (beta == "mixed" and bc == 0) or (mean == "harmonic" and op.startswith("shift")):
                continue  # no face to put a beta on; no coefficient to take a mean of
            D[name("point", op=op, bc=bc, beta=beta, mean=mean, dtype=dt, grid=grid)] = point(op, bc, beta, mean, dtype, n3)
        for op, bc in itertools.product(("shift35", "coef", "cap0"), (0, 37, 63)):
            D[name("cycle", op=op, bc=bc, beta="zeros", mean="arithmetic", dtype=dt, grid=grid, coarsening="full")] = cycle(op, bc, "zeros", "arithmetic", dtype, n3, "full")
        for op in ("shift35", "coef", "cap0"):
            D[name("cycle", op=op, bc=0, beta="zeros", mean="arithmetic", dtype=dt, grid=grid, coarsening="semi")] = cycle(op, 0, "zeros", "arithmetic", dtype, n3, "semi")
        for op, bc, beta, mean, co in (("coef", 37, "mixed", "arithmetic", "full"), ("cap", 63, "mixed", "harmonic", "full"), ("coef", 0, "zeros", "harmonic", "semi")):
            D[name("cycle", op=op, bc=bc, beta=beta, mean=mean, dtype=dt, grid=grid, coarsening=co)] = cycle(op, bc, beta, mean, dtype, n3, co)
    for dt in ("float32", "float64"):
        dtype = np.dtype(dt).type
        for op, bc in (("shift35", 0), ("coef", 0), ("coef", 37), ("cap", 63)):
            D[name("cycles_to", op=op, bc=bc, dtype=dt, grid="17x9x9")] = cycles_to(op, bc, dtype, GRIDS["17x9x9"])
        for loop in ("shift", "coef", "neumann", "closed_box", "closed_box_plain_dots", "cap", "lossy_wall", "harmonic"):
            D[name("fcg", loop=loop, dtype=dt, grid="17x17x17")] = fcg(loop, dtype, GRIDS["17x17x17"])
        for loop in ("coef_semi", "cap_semi"):
            D[name("fcg", loop=loop, dtype=dt, grid="17x9x9")] = fcg(loop, dtype, GRIDS["17x9x9"])
        for op, bc, walls, mean in (("coef", 37, 0, "arithmetic"), ("cap", 63, 0, "arithmetic"), ("coef", 63, 1, "arithmetic"), ("cap", 63, 1, "arithmetic"),
                                    ("cap0", 63, 1, "harmonic")):
            D[name("euler", op=op, bc=bc, walls=walls, mean=mean, dtype=dt, grid="17x9x9")] = euler(op, bc, walls, mean, dtype, GRIDS["17x9x9"])
    for case in NK.EXACT_17:  # the table rows whose count is recorded at 17^3
        x, k, hist, conv, rel, removed = NK.solved(case, 17)
        assert conv and k == NK.CASES[case][3], (case, k)
        D[name("table", case=case, dtype="float64", grid="17x17x17")] = {
            k_: rec(v) for k_, v in zip(("x", "iterations", "history", "converged", "true_rel", "removed"), (x, k, np.asarray(hist), conv, rel, removed))}
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(pack(D[k]), sort_keys=True, separators=(",", ":"))) for k in sorted(D)) + "\n}\n")
    print(len(D), "cases ->", out, os.path.getsize(out), "bytes")


main(sys.argv[1])
