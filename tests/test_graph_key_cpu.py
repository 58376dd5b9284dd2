"""CPU suite: the record a captured cycle is replayed under (use_graph; mg_graph_record in csrc/host/mg_common.h).

A replay is only right when every host-side input of the captured launch sequence is what it was at capture time, so the
record must change whenever any single input changes -- including the pairs the packed keys it replaced could not tell apart
(2D fuse = 2 with either smoother; v1 = 1 against v1 = 4097) -- and be the same for the same state, whatever padding bytes the
state struct carries.  A C driver is compiled against the header with gcc -std=c11 and UBSan (no recovery): any undefined
behaviour of the serialiser fails the run."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <limits.h>
#include <stdio.h>
#include "mg_common.h"

static int fails = 0, checks = 0;
#define EXPECT(cond, ...) do { checks++; if (!(cond)) { fails++; printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

/* a state with every field set, built over a buffer of `fill` bytes so that padding differs between two builds */
static void base(mgGraphState* s, unsigned char fill) {
    memset(s, fill, sizeof *s);
    s->kind = MG_GRAPH_3D;
    s->gridID = 0; s->v1 = 2; s->v2 = 2; s->numGrids = 6; s->residual_mode = 0; s->fuse = 2; s->smoother = 0;
    s->alfa = 2; s->ca_min_planes = 16;
    const double omega = 2.0 / 3.0;
    s->omega_bits = mg_real_bits(&omega, sizeof omega);
    for (int k = 0; k < 4; k++) { const double a = -1.0 - k; s->matrixA_bits[k] = mg_real_bits(&a, sizeof a); }
    s->extra = 0; s->inline_bytes = 96ull << 20; s->generation = 7;
    for (int a = 0; a < MG_GRAPH_FLAG_ARRAYS; a++)
        for (int l = 0; l < MG_MAX_LEVELS; l++) s->flags.a[a][l] = (unsigned char)((a + l) % 3 == 0);
}

static void rec_of(const mgGraphState* s, mgGraphRec* r) {
    memset(r, 0x5a, sizeof *r);
    mg_graph_record(s, r);
}

static int differs(const mgGraphState* a, const mgGraphState* b) {
    mgGraphRec ra, rb;
    rec_of(a, &ra);
    rec_of(b, &rb);
    return !mg_graph_rec_equal(&ra, &rb);
}

/* change one field of the base state by `edit` and expect a different record */
#define ONE(name, edit) do { mgGraphState s0, s1; base(&s0, 0); base(&s1, 0); { mgGraphState* s = &s1; edit; } \
                             EXPECT(differs(&s0, &s1), "%s", name); } while (0)

int main(void) {
    /* identical states, different padding bytes and record garbage: identical records */
    {
        mgGraphState a, b;
        base(&a, 0x00);
        base(&b, 0xff);
        EXPECT(!differs(&a, &b), "identical states give different records");
        mgGraphRec r1, r2;
        memset(&r1, 0, sizeof r1); memset(&r2, 0xff, sizeof r2);
        mg_graph_record(&a, &r1); mg_graph_record(&a, &r2);
        EXPECT(mg_graph_rec_equal(&r1, &r2), "the record depends on its old contents");
    }
    ONE("kind", s->kind = MG_GRAPH_PCG3D);
    ONE("gridID", s->gridID = 1);
    ONE("v1", s->v1 = 3);
    ONE("v2", s->v2 = 3);
    ONE("numGrids", s->numGrids = 5);
    ONE("residual_mode", s->residual_mode = 1);
    ONE("fuse", s->fuse = 1);
    ONE("smoother", s->smoother = 1);
    ONE("alfa", s->alfa = 3);
    ONE("ca_min_planes", s->ca_min_planes = 0);
    ONE("extra", s->extra = 1);
    ONE("extra high word", s->extra = 1ull << 40);
    ONE("inline_bytes", s->inline_bytes = 0);
    ONE("generation", s->generation = 8);
    ONE("generation high word", s->generation = 7 + (1ull << 32));
    ONE("omega", { const double w = 0.8; s->omega_bits = mg_real_bits(&w, sizeof w); });
    ONE("omega last bit", s->omega_bits ^= 1);
    ONE("omega as fp32", { const float w = 2.0f / 3.0f; s->omega_bits = mg_real_bits(&w, sizeof w); });
    for (int k = 0; k < 4; k++) {
        char name[64];
        snprintf(name, sizeof name, "matrixA[%d]", k);
        ONE(name, s->matrixA_bits[k] ^= 1ull << 63);
    }
    for (int a = 0; a < MG_GRAPH_FLAG_ARRAYS; a++)
        for (int l = 0; l < MG_MAX_LEVELS; l++) {
            char name[64];
            snprintf(name, sizeof name, "flag array %d level %d", a, l);
            ONE(name, s->flags.a[a][l] ^= 1);
            snprintf(name, sizeof name, "flag array %d level %d high bit", a, l);
            ONE(name, s->flags.a[a][l] ^= 0x80);
        }
    /* the pairs the packed 2D key mapped to one value: fuse << 32 | smoother << 33 */
    ONE("2D fuse=2 smoother 0 -> 1", s->smoother = 1);
    {
        mgGraphState a, b;
        base(&a, 0); base(&b, 0);
        a.fuse = 2; a.smoother = 0;
        b.fuse = 0; b.smoother = 1;
        EXPECT(differs(&a, &b), "(fuse=2, smoother=0) against (fuse=0, smoother=1)");
        a.fuse = 1; a.smoother = 1;
        b.fuse = 3; b.smoother = 0;
        EXPECT(differs(&a, &b), "(fuse=1, smoother=1) against (fuse=3, smoother=0)");
    }
    /* sweep counts kept in 12 bits by the packed keys */
    {
        mgGraphState a, b;
        base(&a, 0); base(&b, 0);
        a.v1 = 1; b.v1 = 4097;
        EXPECT(differs(&a, &b), "v1 = 1 against v1 = 4097");
        a.v1 = 0; b.v1 = 4096;
        EXPECT(differs(&a, &b), "v1 = 0 against v1 = 4096");
        a.v1 = 2; b.v1 = 2; a.v2 = 1; b.v2 = 4097;
        EXPECT(differs(&a, &b), "v2 = 1 against v2 = 4097");
        /* v1 and v2 cannot trade places */
        a.v1 = 1; a.v2 = 2; b.v1 = 2; b.v2 = 1;
        EXPECT(differs(&a, &b), "(v1, v2) = (1, 2) against (2, 1)");
    }
    /* extreme values: no arithmetic on them, so nothing may overflow */
    {
        mgGraphState a, b;
        base(&a, 0); base(&b, 0);
        a.v1 = INT_MAX; a.v2 = INT_MIN; a.numGrids = INT_MAX; a.alfa = INT_MIN; a.ca_min_planes = -1;
        a.omega_bits = ~0ull; a.generation = ~0ull; a.inline_bytes = ~0ull; a.extra = ~0ull;
        b = a;
        EXPECT(!differs(&a, &b), "extreme state");
        b.v2 = INT_MIN + 1;
        EXPECT(differs(&a, &b), "v2 = INT_MIN against INT_MIN + 1");
        /* the omega that the packed 3D key multiplied by 1000003 in signed 64-bit arithmetic */
        const double w = 2.0 / 3.0;
        a.omega_bits = mg_real_bits(&w, sizeof w);
        b = a;
        EXPECT(!differs(&a, &b), "omega = 2/3");
    }
    /* the widened bit pattern of a float is its 32 bits, zero-extended */
    {
        const float x = -0.0f;
        EXPECT(mg_real_bits(&x, sizeof x) == 0x80000000ull, "mg_real_bits(-0.0f)");
        const double y = -0.0;
        EXPECT(mg_real_bits(&y, sizeof y) == 0x8000000000000000ull, "mg_real_bits(-0.0)");
    }
    printf("sizeof_rec %zu\nsizeof_flags %zu\n", sizeof(mgGraphRec), sizeof(mgGraphFlags));
    printf("checks %d\nfails %d\n", checks, fails);
    return fails != 0;
}
"""


def test_graph_record_changes_with_every_field_under_ubsan(tmp_path):
    assert shutil.which("gcc"), "gcc is part of the build (pde_multigrid_amd/csrc/Makefile)"
    src = tmp_path / "graph_record.c"
    src.write_text(DRIVER)
    exe = tmp_path / "graph_record"
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pde_multigrid_amd", "csrc", "host")]
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=undefined",
                           "-fno-sanitize-recover=all"] + inc + [str(src), "-lm", "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr, p.stderr
    out = dict(line.split(" ", 1) for line in p.stdout.strip().splitlines() if not line.startswith("FAIL"))
    assert out["fails"] == "0"
    # every single-field change above was checked: 18 scalar edits, 4 matrixA words, 2 per flag byte, the pairs
    assert int(out["checks"]) >= 18 + 4 + 2 * 6 * 32 + 10
    # multigrid.py mirrors the structs that hold records and flags
    from pde_multigrid_amd.multigrid import GraphFlags, GraphRec
    assert int(out["sizeof_rec"]) == C.sizeof(GraphRec)
    assert int(out["sizeof_flags"]) == C.sizeof(GraphFlags)
