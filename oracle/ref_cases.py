#!/usr/bin/python3
"""The seeded cases of tests/test_oracle_vs_ref.py and their stored digests -- TEST INFRASTRUCTURE.

Every case is a function of an implementation module M, either `refshim` (the UNMODIFIED compiled reference,
oracle/_ref/libmgref.so) or `oracle` (the float restatement).  Both take the same arguments, and a case returns its
outputs as {label: array}.  tests/golden/ref_digests.json stores the SHA-256 of each reference output's bytes, with
its shape and dtype.  The test can then pin the restatement to the reference bit for bit where the reference was
never built.  Where it was built, the test also compares the two directly and checks the stored digests.

    python oracle/ref_cases.py          # rewrites tests/golden/ref_digests.json (needs oracle/_ref, `make -C oracle ref`)
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_digests.json")
A = [-1, -2, 0, -3]


def digest(a):
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": a.dtype.name, "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def ops3d(M, n, seed):
    rng = np.random.default_rng(seed)
    n3, rg = [n] * 3, [-1, 1, 0, 2, 0.5, 3]
    shape = lambda k: tuple(reversed(k))  # noqa: E731
    csz = tuple((k - 1) // 2 + 1 for k in n3)
    v = rng.uniform(-1, 1, shape(n3)).astype(np.float32)
    f = rng.uniform(-1, 1, shape(n3)).astype(np.float32)
    c = rng.uniform(-1, 1, shape(csz)).astype(np.float32)
    out = {"relax%d" % k: M.relax3d(n3, rg, v, f, k) for k in (1, 2, 5)}
    out["residual"] = M.residual3d(n3, rg, v, f)
    out["restrict"] = M.restrict3d(n3, v)
    out["interpolate"] = M.interpolate3d(n3, v, c)
    out["correct"] = M.correct3d(n3, v, f)
    for b in (0, 1):
        out["set%d" % b] = M.set3d(n3, v, -7.25, b)
    out["vcycle31x2"] = M.cycle3d(n3, rg, mode=0, v1=3, v2=1, reps=2, v=v, f=f)
    out["fmg212"] = M.cycle3d(n3, rg, mode=1, v0=2, v1=1, v2=2, v=v, f=f)
    return out


def analytic3d(M, n, nlev):
    r = [0, 1, 0, 1, 0, 1]
    return {"vcycle": M.cycle3d([n] * 3, r, nlevels=nlev, mode=0), "fmg": M.cycle3d([n] * 3, r, nlevels=nlev, mode=1)}


def ops2d(M, n, seed):
    rng = np.random.default_rng(seed)
    n2, rg = [n] * 2, [0, 20, -3, 20]
    cn = (n - 1) // 2 + 1
    v = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    f = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    c = rng.uniform(-1, 1, (cn, cn)).astype(np.float32)
    out = {"relax%d" % k: M.relax2d(n2, rg, A, 2, v, f, k) for k in (1, 4)}
    out["residual"] = M.residual2d(n2, rg, A, 2, v, f)
    out["restrict"] = M.restrict2d(n2, v)
    out["interpolate"] = M.interpolate2d(n2, v, c)
    out["correct"] = M.correct2d(n2, v, f)
    for b in (0, 1):
        out["set%d" % b] = M.set2d(n2, v, 3.5, b)
    out["vcycle22x2"] = M.cycle2d(n2, rg, A, 2, mode=0, reps=2, v=v, f=f)
    out["fmg222"] = M.cycle2d(n2, rg, A, 2, mode=1, v0=2, v=v, f=f)
    return out


def thesis2d(M):
    # thesis runs use [0,20]^2
    return {"fmg_1_20_20": M.cycle2d([129] * 2, [0, 20, 0, 20], A, 2, mode=1, v0=1, v1=20, v2=20)}


def ops1d(M, n, seed):
    rng = np.random.default_rng(seed)
    rg = [0, 1]
    v = rng.uniform(-1, 1, n).astype(np.float32)
    f = rng.uniform(-1, 1, n).astype(np.float32)
    c = rng.uniform(-1, 1, (n - 1) // 2 + 1).astype(np.float32)
    out = {"relax%d" % k: M.relax1d(n, rg, v, f, k) for k in (1, 4)}
    out["residual"] = M.residual1d(n, rg, v, f)
    out["restrict"] = M.restrict1d(n, v)
    out["interpolate"] = M.interpolate1d(n, v, c)
    out["correct"] = M.correct1d(n, v, f)
    out["vcycle22x2"] = M.cycle1d(n, rg, mode=0, reps=2, v=v, f=f)
    out["fmg222"] = M.cycle1d(n, rg, mode=1, v0=2, v=v, f=f)
    return out


# name -> case; the parameters are those of the tests
OPS3D = [(5, 1), (9, 2), (17, 3), (33, 4)]
ANALYTIC3D = [(17, 0), (33, 3), (65, 0)]
OPS2D = [(9, 1), (17, 2), (65, 3)]
OPS1D = [(9, 1), (33, 2), (257, 3)]
CASES = dict(
    [("3d_ops_n%d_seed%d" % p, (lambda M, p=p: ops3d(M, *p))) for p in OPS3D]
    + [("3d_analytic_n%d_nlev%d" % p, (lambda M, p=p: analytic3d(M, *p))) for p in ANALYTIC3D]
    + [("2d_ops_n%d_seed%d" % p, (lambda M, p=p: ops2d(M, *p))) for p in OPS2D]
    + [("2d_thesis_range_analytic", thesis2d)]
    + [("1d_ops_n%d_seed%d" % p, (lambda M, p=p: ops1d(M, *p))) for p in OPS1D])


def main():
    sys.path.insert(0, HERE)
    import refshim as R
    if not R.available():
        sys.exit("oracle/_ref/libmgref.so missing: run `make -C oracle ref` (needs the reference sources)")
    out = {"_what": "SHA-256 of the bytes, shape and dtype of every output of the compiled reference on the seeded cases "
                    "of oracle/ref_cases.py (written by `python oracle/ref_cases.py`)",
           "_glibc_note": "the analytic cases evaluate libm sin: digests taken with glibc 2.35"}
    for name, case in CASES.items():
        out[name] = {label: digest(a) for label, a in case(R).items()}
    with open(DIGESTS, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", DIGESTS)


if __name__ == "__main__":
    main()
