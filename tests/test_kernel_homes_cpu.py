"""CPU suite: one home per kernel.  The library is built with -fno-gpu-rdc, so every unit that launches a
kernel template carries a copy of that kernel: a kernel held by two units is a launch site in the wrong file.  Reads names and
units from the objects `make` leaves in csrc/build (tools/kernel_table.py); inspects no instructions.  Skips only where the build
or the LLVM tools are absent: no build directory, or one that a copy of the tree left without a single object (a build that
compiles nothing fails at `make` and never gets here)."""
import collections
import glob
import importlib.util
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pde_multigrid_amd", "csrc")
BUILD = os.path.join(CSRC, "build")
STENCIL_UNITS = {"mgx_shift3d", "mgx_coef3d", "mgx_rim3d"}  # one instance of mgx_stencil3d.hpp's kernels per operator set
PIPELINED = ("relax3d_xs_pipe_kernel", "relax3d_xs_pipe_v2_kernel")


def _kernel_table():
    spec = importlib.util.spec_from_file_location("kernel_table", os.path.join(ROOT, "tools", "kernel_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _base(name):  # "void mgx::relax3d_xs_kernel<double, 4, 4, 0>(...)" -> "relax3d_xs_kernel"
    return re.match(r"(?:void )?(?:(?:\w+|\(anonymous namespace\))::)*(\w+)", name).group(1)


@pytest.fixture(scope="module")
def holders():
    kt = _kernel_table()
    if not glob.glob(os.path.join(BUILD, "mgx_*.o")):  # absent, or left behind empty by a copy of the tree without object files
        pytest.skip("no build in " + BUILD)
    tools = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
    if not all(os.path.exists(os.path.join(kt.LLVM, t)) for t in tools):
        pytest.skip("no LLVM tools under " + kt.LLVM)
    units = collections.defaultdict(list)  # demangled kernel name -> the units that hold it
    for row in kt.table(BUILD):
        f = row.split("\t")
        units[f[-1]].append(f[0])
    assert len(units) > 500, len(units)  # the library has some 700 kernels: fewer means the table was not read
    return units


def test_every_kernel_has_one_home(holders):
    shared = set(re.findall(r"__global__[^;{]*?\b(\w+_kernel)\s*\(", open(os.path.join(CSRC, "mgx_stencil3d.hpp")).read()))
    assert shared, "no kernels found in mgx_stencil3d.hpp"
    wrong = []
    for name, us in sorted(holders.items()):
        if len(us) == 1:
            continue
        if _base(name) in shared and len(set(us)) == len(us) and set(us) <= STENCIL_UNITS:
            continue
        wrong.append((name, us))
    assert not wrong, wrong


def test_pipelined_kernels_only_in_their_unit(holders):
    found = {k: 0 for k in PIPELINED}
    for name, us in holders.items():
        if _base(name) in found:
            found[_base(name)] += 1
            assert us == ["mgx_pipe3d"], (name, us)
    assert all(found.values()), found
