/* mg_common.h -- helpers shared by the stamped host-layer sources (C11). */
#ifndef MG_COMMON_H
#define MG_COMMON_H
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mg_multigrid.h"

#define MG_CAT_(a, b) a##b
#define MG_CAT(a, b) MG_CAT_(a, b)
#define MG_CAT3(a, b, c) MG_CAT(MG_CAT(a, b), c)

#define MG_PI (3.141592653589793) /* N3/inclusion.h:9 */

static inline int mg_fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    mgx_set_last_error(buf);
    return status;
}

/* MG_CA_TRACE=1 in the environment: the slab driver prints the launches and exchanges of its communication-avoiding
 * schedule (level, pass, plane ranges) to stderr -- a debugging aid, read once */
static inline int mg_ca_trace(void) {
    static int on = -1;
    if (on < 0) { const char* e = getenv("MG_CA_TRACE"); on = e && *e && *e != '0'; }
    return on;
}

/* ---- use_graph: the record a captured cycle is replayed under ---------------------------------------------------------
 * Every host-side input of a cycle's launch sequence (the device arrays and their sizes are fixed for a hierarchy's life).
 * Fields a hierarchy does not have stay 0; flag arrays hold only the levels its cycle reads, 0 elsewhere. */
enum { MG_GRAPH_2D = 1, MG_GRAPH_3D = 2, MG_GRAPH_PCG3D = 3, MG_GRAPH_SLAB = 4 };
typedef struct mgGraphState {
    unsigned kind; /* MG_GRAPH_*: which body the sequence runs */
    int gridID, v1, v2, numGrids, residual_mode, fuse, smoother, alfa, ca_min_planes;
    unsigned long long omega_bits;      /* bit pattern of omega (fp32: the low 32 bits) */
    unsigned long long matrixA_bits[4]; /* 2D: bit patterns of matrixA */
    unsigned long long extra;           /* what else the caller's body depends on */
    unsigned long long inline_bytes;    /* slab: the inline-exchange threshold */
    unsigned long long generation;      /* mgx_ctx_generation of the context */
    mgGraphFlags flags;                 /* see mgGraphFlags */
} mgGraphState;

/* the bit pattern of a float or double, widened without arithmetic */
static inline unsigned long long mg_real_bits(const void* x, size_t size) {
    unsigned long long b = 0;
    unsigned char* d = (unsigned char*)&b;
    const unsigned char* s = (const unsigned char*)x;
    for (size_t i = 0; i < size && i < sizeof b; i++) d[i] = s[i]; /* little-endian: the value's bits, high bytes 0 */
    return b;
}

/* serialise *s into *rec: one word per int field (converted to unsigned, which is exact modulo 2^32), two per 64-bit
 * field, four flag bytes per word.  Pure: no signed arithmetic, no padding bytes read. */
static inline void mg_graph_record(const mgGraphState* s, mgGraphRec* rec) {
    unsigned* w = rec->w;
    unsigned n = 0;
    w[n++] = s->kind;
    w[n++] = (unsigned)s->gridID;
    w[n++] = (unsigned)s->v1;
    w[n++] = (unsigned)s->v2;
    w[n++] = (unsigned)s->numGrids;
    w[n++] = (unsigned)s->residual_mode;
    w[n++] = (unsigned)s->fuse;
    w[n++] = (unsigned)s->smoother;
    w[n++] = (unsigned)s->alfa;
    w[n++] = (unsigned)s->ca_min_planes;
    const unsigned long long wide[8] = {s->omega_bits,     s->matrixA_bits[0], s->matrixA_bits[1], s->matrixA_bits[2],
                                        s->matrixA_bits[3], s->extra,          s->inline_bytes,     s->generation};
    for (unsigned i = 0; i < 8; i++) {
        w[n++] = (unsigned)wide[i]; /* the low 32 bits */
        w[n++] = (unsigned)(wide[i] >> 32);
    }
    for (unsigned a = 0; a < MG_GRAPH_FLAG_ARRAYS; a++)
        for (unsigned l = 0; l < MG_MAX_LEVELS; l += 4)
            w[n++] = (unsigned)s->flags.a[a][l] | (unsigned)s->flags.a[a][l + 1] << 8 | (unsigned)s->flags.a[a][l + 2] << 16 |
                     (unsigned)s->flags.a[a][l + 3] << 24;
}
_Static_assert(10 + 2 * 8 + MG_GRAPH_FLAG_ARRAYS * MG_MAX_LEVELS / 4 == MG_GRAPH_REC_WORDS, "mg_graph_record fills the record");

/* 1 when two records are equal word for word */
static inline int mg_graph_rec_equal(const mgGraphRec* a, const mgGraphRec* b) { return !memcmp(a, b, sizeof *a); }

#define MG_TRY(expr)            \
    do {                        \
        int st_ = (expr);       \
        if (st_) return st_;    \
    } while (0)

#define MG_REQUIRE(cond, status, ...)                      \
    do {                                                   \
        if (!(cond)) return mg_fail(status, __VA_ARGS__);  \
    } while (0)

#endif
