"""ctypes views of the C host layer (include/mg_multigrid.h) and of the raw operator C-ABI
(include/mgx.h).  numpy arrays are indexed [z, y, x] (x fastest in memory): the reference's
idx = x + y*sx + z*sx*sy.  Sizes are given as (sx, sy, sz) like the reference's sizeXYZ."""
import ctypes as C

import numpy as np

from ._lib import CORRECT, REF_COMPAT, check, lib


def _ct(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return "f32", C.c_float
    if dtype == np.float64:
        return "f64", C.c_double
    raise TypeError("dtype must be float32 or float64, got %s" % dtype)


def _ip(a):
    return (C.c_int * len(a))(*[int(x) for x in a])


def _rp(a, ct):
    return (ct * len(a))(*[float(x) for x in a])


def _shape(n):
    return tuple(int(k) for k in reversed(tuple(n)))


def _count(n):
    c = 1
    for k in n:
        c *= int(k)
    return c


def num_grids(min_size):
    return lib.mg_num_grids(int(min_size))


def coarse_size(n):
    return tuple(lib.mg_coarse_size(int(k)) for k in n)


def grid_spacing(n, rng, dtype):
    """h = range/(real)(size-1) evaluated in `dtype` like Grid3D's constructor (N3/Grid3D.cpp:31-45)."""
    t = np.dtype(dtype).type
    return [t(t(rng[2 * d + 1]) - t(rng[2 * d])) / t(int(n[d]) - 1) for d in range(len(n))]


class Context:
    """One HIP device context (compute + comm stream)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib.mgx_ctx_create(int(device), C.byref(self._h)))
        self.device = int(device)

    def close(self):
        if self._h:
            lib.mgx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(lib.mgx_ctx_sync(self._h))

    # -- raw device memory --------------------------------------------------
    def malloc(self, nbytes):
        p = C.c_void_p()
        check(lib.mgx_malloc(self._h, C.c_size_t(int(nbytes)), C.byref(p)))
        return p

    def free(self, p):
        check(lib.mgx_free(self._h, p))

    def last_relax_kernel(self):
        return lib.mgx_ctx_last_relax_kernel(self._h).decode()

    def last_rr_kernel(self):
        """the fused black pass + residual + restrict kernel of the most recent smooth_residual_restrict call ("" = not fused)"""
        return lib.mgx_ctx_last_rr_kernel(self._h).decode()

    def last_corr_kernel(self):
        """the correcting red pass of the most recent interpolate_correct_relax call ("" = the correction was a pass of its own)"""
        return lib.mgx_ctx_last_corr_kernel(self._h).decode()

    def last_block3_kernel(self):
        """the three-pass kernel of the most recent smooth_residual_restrict / relax_block3 call ("" = passes one launch each)"""
        return lib.mgx_ctx_last_block3_kernel(self._h).decode()

    def set_param(self, name, value):
        check(lib.mgx_ctx_set_param(self._h, name.encode(), C.c_int(int(value))))

    def generation(self):
        """mgx_ctx_generation: grows whenever what the context launches may have changed (parameters, given-up waits)"""
        g = C.c_ulonglong()
        check(lib.mgx_ctx_generation(self._h, C.byref(g)))
        return int(g.value)

    def clear_abort(self, reenable=False):
        """after sync() reported a given-up wait between workgroups: clear the condition (mgx_ctx_clear_abort)"""
        check(lib.mgx_ctx_clear_abort(self._h, C.c_int(1 if reenable else 0)))

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        check(lib.mgx_memcpy_h2d(self._h, p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)))
        return p

    def to_host(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        check(lib.mgx_memcpy_d2h(self._h, out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes)))
        return out

    # -- events on the compute stream -----------------------------------------
    def event(self):
        e = C.c_void_p()
        check(lib.mgx_event_create(self._h, C.byref(e)))
        return e

    def record(self, e):
        check(lib.mgx_event_record(self._h, e))

    def elapsed_ms(self, e0, e1):
        ms = C.c_float()
        check(lib.mgx_event_elapsed_ms(self._h, e0, e1, C.byref(ms)))
        return float(ms.value)

    # -- RCCL -------------------------------------------------------------------
    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * 128)()
        check(lib.mgx_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check(lib.mgx_comm_init(self._h, buf, int(rank), int(nranks)))

    def comm_init_rehearsal(self, unique_id, virtual_rank, virtual_nranks):
        """one rank of a larger job rehearsed on this GPU alone (mgx_comm_init_rehearsal): timing only"""
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check(lib.mgx_comm_init_rehearsal(self._h, buf, int(virtual_rank), int(virtual_nranks)))

    def comm_info(self):
        """(ranks the communicator reports, RCCL version code)"""
        n, v = C.c_int(0), C.c_int(0)
        check(lib.mgx_comm_info(self._h, C.byref(n), C.byref(v)))
        return n.value, v.value

    def comm_set_inline(self, on):
        """collectives on the compute stream (True) or on the comm stream (False): mgx_comm_set_inline"""
        check(lib.mgx_comm_set_inline(self._h, C.c_int(int(bool(on)))))


# --------------------------------------------------------------------------- raw operators
def xs_geometry(sx, itemsize):
    """(H, P): offset of the odd-x half and row pitch of the x-split layout (both multiples of a 128-byte line)"""
    al = 128 // itemsize
    H = ((sx + 1) // 2 + al - 1) // al * al
    return H, H + (sx // 2 + al - 1) // al * al


def xs_pack(a):
    """numpy restatement of the x-split layout: every x-row as its even-x half then, from the next 128-byte
    boundary on, its odd-x half; rows padded to the pitch with zeros"""
    a = np.asarray(a)
    sx = a.shape[-1]
    H, P = xs_geometry(sx, a.dtype.itemsize)
    out = np.zeros(a.shape[:-1] + (P,), a.dtype)
    out[..., :(sx + 1) // 2] = a[..., 0::2]
    out[..., H:H + sx // 2] = a[..., 1::2]
    return out


def xs_unpack(a, sx):
    a = np.asarray(a)
    H, P = xs_geometry(sx, a.dtype.itemsize)
    assert a.shape[-1] == P
    out = np.empty(a.shape[:-1] + (sx,), a.dtype)
    out[..., 0::2] = a[..., :(sx + 1) // 2]
    out[..., 1::2] = a[..., H:H + sx // 2]
    return out


class _Ops:
    """Per-operator entry points of mgx.h on numpy arrays (reference layout): upload, launch, download.
    Used by the parity tests; the cycle code in C keeps everything resident instead.  With
    xsplit=True the arrays are converted to the x-split layout on the host and the mgx3dxs_
    twins are called."""

    def __init__(self, dim, xsplit=False):
        self.dim = dim
        self.xsplit = xsplit
        self.p = ("mgx%ddxs_" if xsplit else "mgx%dd_") % dim

    def _fn(self, name, dtype):
        s, ct = _ct(dtype)
        return getattr(lib, self.p + name + "_" + s), ct

    def _run(self, ctx, arrays, call, out_index, out_shape, dtype):
        conv = xs_pack if self.xsplit else (lambda a: a)
        ptrs = [ctx.to_device(conv(np.ascontiguousarray(a, dtype=dtype))) if a is not None else None for a in arrays]
        try:
            check(call(*ptrs))
            if not self.xsplit:
                return ctx.to_host(ptrs[out_index], out_shape, dtype)
            P_ = xs_geometry(out_shape[-1], np.dtype(dtype).itemsize)[1]
            return xs_unpack(ctx.to_host(ptrs[out_index], tuple(out_shape[:-1]) + (P_,), dtype), out_shape[-1])
        finally:
            for p in ptrs:
                if p is not None:
                    ctx.free(p)

    def restrict(self, ctx, fine, n, cn=None, dtype=None):
        dtype = dtype or fine.dtype
        fn, _ = self._fn("restrict", dtype)
        cn = cn if cn is not None else coarse_size(n)
        coarse = np.zeros(_shape(cn), dtype)
        return self._run(ctx, [fine, coarse], lambda f, c: fn(ctx._h, f, _ip(n), c, _ip(cn)), 1, _shape(cn), dtype)

    def interpolate(self, ctx, fine, n, coarse, cn=None, dtype=None):
        dtype = dtype or fine.dtype
        fn, _ = self._fn("interpolate", dtype)
        cn = cn if cn is not None else coarse_size(n)
        return self._run(ctx, [fine, coarse], lambda f, c: fn(ctx._h, f, _ip(n), c, _ip(cn)), 0, _shape(n), dtype)

    def apply_correction(self, ctx, fine, n, err, en=None, dtype=None):
        dtype = dtype or fine.dtype
        fn, _ = self._fn("apply_correction", dtype)
        en = en if en is not None else n
        return self._run(ctx, [fine, err], lambda f, e: fn(ctx._h, f, _ip(n), e, _ip(en)), 0, _shape(n), dtype)

    def set(self, ctx, grid, n, value, modify_boundaries, dtype=None):
        dtype = dtype or grid.dtype
        fn, ct = self._fn("set", dtype)
        return self._run(ctx, [grid], lambda g: fn(ctx._h, g, _ip(n), ct(value), C.c_int(int(modify_boundaries))), 0,
                         _shape(n), dtype)


class _Ops3D(_Ops):
    def __init__(self, xsplit=False):
        super().__init__(3, xsplit)

    def pack(self, ctx, a):
        """device-side Natural -> XSplit conversion (mgx3dxs_pack), returned as stored (padded rows)"""
        s, _ = _ct(a.dtype)
        n = tuple(reversed(a.shape))
        fn = getattr(lib, "mgx3dxs_elems_" + s)
        fn.restype = C.c_size_t
        elems = fn(_ip(n))
        P_ = xs_geometry(n[0], a.dtype.itemsize)[1]
        assert elems == P_ * n[1] * n[2]
        src, dst = ctx.to_device(a), ctx.to_device(np.zeros(elems, a.dtype))
        try:
            check(getattr(lib, "mgx3dxs_pack_" + s)(ctx._h, src, dst, _ip(n)))
            return ctx.to_host(dst, a.shape[:-1] + (P_,), a.dtype)
        finally:
            ctx.free(src)
            ctx.free(dst)

    def unpack(self, ctx, a, sx):
        s, _ = _ct(a.dtype)
        n = (sx,) + tuple(reversed(a.shape[:-1]))
        src, dst = ctx.to_device(a), ctx.malloc(sx * a.shape[0] * a.shape[1] * a.dtype.itemsize)
        try:
            check(getattr(lib, "mgx3dxs_unpack_" + s)(ctx._h, src, dst, _ip(n)))
            return ctx.to_host(dst, a.shape[:-1] + (sx,), a.dtype)
        finally:
            ctx.free(src)
            ctx.free(dst)

    def relax(self, ctx, v, f, n, rng, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, _ip(n), h, C.c_int(ncycles)), 0, _shape(n), dtype)

    def relax_pp(self, ctx, v, f, n, rng, ncycles, w=None, w_rim_valid=False, dtype=None):
        """x-split only: relax with a ping-pong partner w (one launch per red+black sweep where the level takes it);
        w defaults to an array of NaNs (its boundary is then copied from v by the call)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_pp", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        if w is None:
            w = np.full(_shape(n), np.nan, dtype)
        return self._run(ctx, [v, w, f], lambda a, ww, b: fn(ctx._h, a, ww, b, _ip(n), h, C.c_int(ncycles), C.c_int(int(w_rim_valid))),
                         0, _shape(n), dtype)

    def relax_from_zero_pp(self, ctx, v, f, n, rng, ncycles, rim_is_zero, w=None, w_rim_valid=False, dtype=None):
        """x-split only: relax_from_zero with a ping-pong partner (mgx3dxs_relax_from_zero_pp)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_from_zero_pp", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        if w is None:
            w = np.full(_shape(n), np.nan, dtype)
        return self._run(ctx, [v, w, f], lambda a, ww, b: fn(ctx._h, a, ww, b, _ip(n), h, C.c_int(ncycles), C.c_int(int(rim_is_zero)),
                                                            C.c_int(int(w_rim_valid))), 0, _shape(n), dtype)

    def interpolate_correct_relax_pp(self, ctx, v, f, n, rng, coarse, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("interpolate_correct_relax_pp", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        cn = coarse_size(n)
        w = np.full(_shape(n), np.nan, dtype)
        return self._run(ctx, [v, w, f, coarse], lambda a, ww, b, c: fn(ctx._h, a, ww, b, _ip(n), h, c, _ip(cn), C.c_int(ncycles), C.c_int(0)),
                         0, _shape(n), dtype)

    def sweep_once(self, ctx, vin, vout, f, n, rng, zero=False, dtype=None):
        """x-split only: one out-of-place sweep vin -> vout (interior of vout) by the level's one-launch kernel"""
        dtype = dtype or vin.dtype
        fn, ct = self._fn("sweep_once", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [vin, vout, f], lambda a, o, b: fn(ctx._h, a, o, b, _ip(n), h, C.c_int(int(zero))), 1, _shape(n), dtype)

    def relax_pp_takes(self, ctx, n, ncycles, dtype=np.float64):
        s, _ = _ct(dtype)
        return bool(getattr(lib, "mgx3dxs_relax_pp_takes_" + s)(ctx._h, _ip(n), C.c_int(ncycles)))

    def block3_up_takes(self, ctx, n, ncycles, dtype=np.float64):
        """does interpolate_correct_relax_pp run the passes B, R, B after the correcting red pass in one launch?"""
        s, _ = _ct(dtype)
        return bool(getattr(lib, "mgx3dxs_block3_up_takes_" + s)(ctx._h, _ip(n), C.c_int(ncycles)))

    def block3_corr_takes(self, ctx, n, ncycles, dtype=np.float64):
        """does interpolate_correct_relax_block3 run the passes R', B, R as one in-place launch?"""
        s, _ = _ct(dtype)
        return bool(getattr(lib, "mgx3dxs_block3_corr_takes_" + s)(ctx._h, _ip(n), C.c_int(ncycles)))

    def residual(self, ctx, v, f, n, rng, mode=REF_COMPAT, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        r = np.zeros(_shape(n), dtype)
        return self._run(ctx, [v, f, r], lambda a, b, c: fn(ctx._h, a, b, c, _ip(n), h, C.c_int(mode)), 2, _shape(n), dtype)

    def residual_restrict(self, ctx, v, f, n, rng, mode=REF_COMPAT, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_restrict", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        cn = coarse_size(n)
        coarse = np.zeros(_shape(cn), dtype)
        return self._run(ctx, [v, f, coarse], lambda a, b, c: fn(ctx._h, a, b, _ip(n), h, C.c_int(mode), c, _ip(cn)), 2,
                         _shape(cn), dtype)

    def interpolate_correct(self, ctx, v, n, coarse, dtype=None):
        dtype = dtype or v.dtype
        fn, _ = self._fn("interpolate_correct", dtype)
        cn = coarse_size(n)
        return self._run(ctx, [v, coarse], lambda a, c: fn(ctx._h, a, _ip(n), c, _ip(cn)), 0, _shape(n), dtype)

    # ---- transfers of a semi-coarsened step (x-split only): cn keeps some axes of n and halves the others
    def restrict_axes(self, ctx, fine, n, cn, coarse=None, dtype=None):
        """coarse: the array the call writes into (every point is written; default zeros)"""
        dtype = dtype or fine.dtype
        fn, _ = self._fn("restrict_axes", dtype)
        coarse = np.zeros(_shape(cn), dtype) if coarse is None else coarse
        return self._run(ctx, [fine, coarse], lambda f, c: fn(ctx._h, f, _ip(n), c, _ip(cn)), 1, _shape(cn), dtype)

    def interpolate_axes(self, ctx, fine, n, coarse, cn, dtype=None):
        dtype = dtype or fine.dtype
        fn, _ = self._fn("interpolate_axes", dtype)
        return self._run(ctx, [fine, coarse], lambda f, c: fn(ctx._h, f, _ip(n), c, _ip(cn)), 0, _shape(n), dtype)

    def residual_restrict_axes(self, ctx, v, f, n, rng, cn, mode=REF_COMPAT, coarse=None, coarse_rim_is_zero=False, dtype=None):
        """coarse: the array the call writes into (default NaN: the call has to zero the boundary itself)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_restrict_axes", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        coarse = np.full(_shape(cn), np.nan, dtype) if coarse is None else coarse
        return self._run(ctx, [v, f, coarse], lambda a, b, c: fn(ctx._h, a, b, _ip(n), h, C.c_int(mode), c, _ip(cn),
                                                                 C.c_int(int(coarse_rim_is_zero))), 2, _shape(cn), dtype)

    def interpolate_correct_axes(self, ctx, v, n, coarse, cn, dtype=None):
        dtype = dtype or v.dtype
        fn, _ = self._fn("interpolate_correct_axes", dtype)
        return self._run(ctx, [v, coarse], lambda a, c: fn(ctx._h, a, _ip(n), c, _ip(cn)), 0, _shape(n), dtype)

    def interpolate_correct_colour(self, ctx, v, n, coarse, colour, dtype=None):
        """x-split only: correct the points with (x+y+z) % 2 == colour (-1 = all)"""
        dtype = dtype or v.dtype
        fn, _ = self._fn("interpolate_correct_colour", dtype)
        cn = coarse_size(n)
        return self._run(ctx, [v, coarse], lambda a, c: fn(ctx._h, a, _ip(n), c, _ip(cn), C.c_int(colour)), 0, _shape(n), dtype)

    def relax_from_zero(self, ctx, v, f, n, rng, ncycles, rim_is_zero, dtype=None):
        """v := 0, then ncycles sweeps; with rim_is_zero the given v must have zero boundary entries (its interior is ignored)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_from_zero", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, _ip(n), h, C.c_int(ncycles), C.c_int(int(rim_is_zero))), 0, _shape(n),
                         dtype)

    def smooth_residual_restrict(self, ctx, v, f, n, rng, ncycles, from_zero=False, v_rim_is_zero=False, mode=REF_COMPAT, dtype=None):
        """x-split only: (v_out, coarse_f) of Relax(ncycles) + CalculateResidual + Restrict in one call
        (mgx3dxs_smooth_residual_restrict: the last black pass inside the residual+restrict launch where the level takes it)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("smooth_residual_restrict", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        cn = coarse_size(n)
        pv, pf = ctx.to_device(xs_pack(np.ascontiguousarray(v, dtype))), ctx.to_device(xs_pack(np.ascontiguousarray(f, dtype)))
        pc = ctx.to_device(xs_pack(np.full(_shape(cn), np.nan, dtype)))  # the call has to zero the coarse boundary itself
        try:
            check(fn(ctx._h, pv, pf, _ip(n), h, C.c_int(ncycles), C.c_int(int(from_zero)), C.c_int(int(v_rim_is_zero)), C.c_int(mode), pc,
                     _ip(cn), C.c_int(0)))
            isz = np.dtype(dtype).itemsize
            out_v = xs_unpack(ctx.to_host(pv, tuple(_shape(n)[:-1]) + (xs_geometry(n[0], isz)[1],), dtype), n[0])
            out_c = xs_unpack(ctx.to_host(pc, tuple(_shape(cn)[:-1]) + (xs_geometry(cn[0], isz)[1],), dtype), cn[0])
            return out_v, out_c
        finally:
            for q in (pv, pf, pc):
                ctx.free(q)

    def relax_block3(self, ctx, vin, f, n, rng, first_colour=0, store_both=False, vout=None):
        """x-split fp64 only: colour passes first_colour, 1 - first_colour, first_colour in one launch (mgx3dxs_relax_block3_f64).
        Reads vin's other colour and faces and f, writes into vout (default: vin itself, in place) and returns vout"""
        h = _rp(grid_spacing(n, rng, np.float64), C.c_double)
        arrs = [vin, f] if vout is None else [vin, f, vout]
        if vout is None:
            call = lambda a, b: lib.mgx3dxs_relax_block3_f64(ctx._h, a, a, b, _ip(n), h, C.c_int(first_colour), C.c_int(int(store_both)))
            return self._run(ctx, arrs, call, 0, _shape(n), np.float64)
        call = lambda a, b, c: lib.mgx3dxs_relax_block3_f64(ctx._h, a, c, b, _ip(n), h, C.c_int(first_colour), C.c_int(int(store_both)))
        return self._run(ctx, arrs, call, 2, _shape(n), np.float64)

    def relax_block3_corr(self, ctx, v, f, n, rng, coarse):
        """x-split fp64 only: the passes R', B, R of the way up in one in-place launch (mgx3dxs_relax_block3_corr_f64): the first red
        pass reads black through the correction from `coarse`; only the red interior points of v are written"""
        h = _rp(grid_spacing(n, rng, np.float64), C.c_double)
        cn = coarse_size(n)
        return self._run(ctx, [v, f, coarse], lambda a, b, c: lib.mgx3dxs_relax_block3_corr_f64(ctx._h, a, b, _ip(n), h, c, _ip(cn)), 0,
                         _shape(n), np.float64)

    def interpolate_correct_relax_block3(self, ctx, v, f, n, rng, coarse, ncycles, dtype=None):
        """x-split only: interpolate_correct_relax with R', B, R in one launch where block3_corr_takes says so"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("interpolate_correct_relax_block3", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        cn = coarse_size(n)
        return self._run(ctx, [v, f, coarse], lambda a, b, c: fn(ctx._h, a, b, _ip(n), h, c, _ip(cn), C.c_int(ncycles)), 0, _shape(n),
                         dtype)

    def interpolate_correct_relax(self, ctx, v, f, n, rng, coarse, ncycles, dtype=None):
        """x-split only: v += Interpolate(coarse) on the interior, then ncycles >= 1 red-black sweeps, in one call"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("interpolate_correct_relax", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        cn = coarse_size(n)
        return self._run(ctx, [v, f, coarse], lambda a, b, c: fn(ctx._h, a, b, _ip(n), h, c, _ip(cn), C.c_int(ncycles)), 0, _shape(n),
                         dtype)

    def jacobi(self, ctx, v, f, n, rng, omega, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("jacobi", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, np.zeros_like(v), f], lambda a, t, b: fn(ctx._h, a, t, b, _ip(n), h, ct(omega), C.c_int(ncycles)),
                         0, _shape(n), dtype)

    def norm2(self, ctx, x):
        s, _ = _ct(x.dtype)
        out = C.c_double()
        p = ctx.to_device(x)
        try:
            check(getattr(lib, "mgx_norm2_" + s)(ctx._h, p, C.c_size_t(x.size), C.byref(out)))
        finally:
            ctx.free(p)
        return float(out.value)


    # ---- the shifted operator (Laplacian - s) u = f (x-split only, mgx3dxs_*_shift)
    def relax_shift(self, ctx, v, f, n, rng, s, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_shift", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, _ip(n), h, ct(s), C.c_int(ncycles)), 0, _shape(n), dtype)

    def relax_shift_from_zero(self, ctx, v, f, n, rng, s, ncycles, rim_is_zero, dtype=None):
        """v := 0, then ncycles sweeps; with rim_is_zero the given v must have zero boundary entries (its interior is ignored)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_shift_from_zero", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, _ip(n), h, ct(s), C.c_int(ncycles), C.c_int(int(rim_is_zero))), 0,
                         _shape(n), dtype)

    def residual_shift(self, ctx, v, f, n, rng, s, store=True, want_sum=True, dtype=None):
        """(r, sum of squares): r None with store=False, the sum None with want_sum=False"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_shift", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        arrays = [xs_pack(np.ascontiguousarray(a, dtype)) for a in (v, f)] + [xs_pack(np.zeros(_shape(n), dtype)) if store else None]
        (_, _, ro), sums = self._krylov(ctx, n, arrays, [],
                                        lambda w, s0, a, b, c: fn(ctx._h, a, b, c, _ip(n), h, ct(s), w if want_sum else None,
                                                                  s0 if want_sum else None), dtype, 1)
        return (xs_unpack(ro, n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def residual_restrict_shift(self, ctx, v, f, n, rng, s, cn, coarse=None, coarse_rim_is_zero=False, dtype=None):
        """coarse: the array the call writes into (default NaN: the call has to zero the boundary itself)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_restrict_shift", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        coarse = np.full(_shape(cn), np.nan, dtype) if coarse is None else coarse
        return self._run(ctx, [v, f, coarse], lambda a, b, c: fn(ctx._h, a, b, _ip(n), h, ct(s), c, _ip(cn),
                                                                 C.c_int(int(coarse_rim_is_zero))), 2, _shape(cn), dtype)

    def laplace_dot_shift(self, ctx, p, n, rng, s, q=None, dtype=None):
        """q = A p with A = Laplacian - s, and <p, q>: returns (q, pq); q: the array written into (default zeros)"""
        dtype = dtype or p.dtype
        fn, ct = self._fn("laplace_dot_shift", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        pp = xs_pack(np.ascontiguousarray(p, dtype))
        qq = np.zeros_like(pp) if q is None else xs_pack(np.ascontiguousarray(q, dtype))
        (_, qo), sums = self._krylov(ctx, n, [pp, qq], [], lambda w, s0, a, b: fn(ctx._h, a, b, _ip(n), h, ct(s), w, s0), dtype, 1)
        return xs_unpack(qo, n[0]), float(sums[0])

    def shift_rhs(self, ctx, u, q, qscale, s, n, f=None, dtype=None):
        """f = (-(s*u)) - qscale*q on the interior (q None: -(s*u)); f: the array written into (default zeros)"""
        dtype = dtype or u.dtype
        fn, ct = self._fn("shift_rhs", dtype)
        f = np.zeros(_shape(n), dtype) if f is None else f
        return self._run(ctx, [u, q, f], lambda a, b, c: fn(ctx._h, a, b, ct(qscale), ct(s), c, _ip(n)), 2, _shape(n), dtype)

    # ---- the variable-coefficient operator div(a grad u) - s u = f (x-split only, mgx3dxs_*_coef); a holds all points
    def relax_coef(self, ctx, v, f, a, n, rng, s, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_coef", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, _ip(n), h, ct(s), C.c_int(ncycles)), 0, _shape(n), dtype)

    def relax_coef_from_zero(self, ctx, v, f, a, n, rng, s, ncycles, rim_is_zero, dtype=None):
        """v := 0, then ncycles sweeps; with rim_is_zero the given v must have zero boundary entries (its interior is ignored)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_coef_from_zero", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, _ip(n), h, ct(s), C.c_int(ncycles), C.c_int(int(rim_is_zero))), 0,
                         _shape(n), dtype)

    def residual_coef(self, ctx, v, f, a, n, rng, s, store=True, want_sum=True, dtype=None):
        """(r, sum of squares): r None with store=False, the sum None with want_sum=False"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_coef", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        arrays = [xs_pack(np.ascontiguousarray(x, dtype)) for x in (v, f, a)] + [xs_pack(np.zeros(_shape(n), dtype)) if store else None]
        (_, _, _, ro), sums = self._krylov(ctx, n, arrays, [],
                                           lambda w, s0, x, b, c, d: fn(ctx._h, x, b, c, d, _ip(n), h, ct(s), w if want_sum else None,
                                                                        s0 if want_sum else None), dtype, 1)
        return (xs_unpack(ro, n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def apply_coef_dot(self, ctx, p, a, n, rng, s, q=None, dtype=None):
        """q = A p with A = div(a grad .) - s, and <p, q>: returns (q, pq); q: the array written into (default zeros)"""
        dtype = dtype or p.dtype
        fn, ct = self._fn("apply_coef_dot", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        pp, aa = xs_pack(np.ascontiguousarray(p, dtype)), xs_pack(np.ascontiguousarray(a, dtype))
        qq = np.zeros_like(pp) if q is None else xs_pack(np.ascontiguousarray(q, dtype))
        (_, _, qo), sums = self._krylov(ctx, n, [pp, aa, qq], [], lambda w, s0, x, c, b: fn(ctx._h, x, c, b, _ip(n), h, ct(s), w, s0), dtype, 1)
        return xs_unpack(qo, n[0]), float(sums[0])

    # ---- the operator with a capacity div(a grad u) - (s c) u = f (x-split only, mgx3dxs_*_cap): the _coef wrappers with c after a,
    # and their _bc forms through bc != None
    def relax_cap(self, ctx, v, f, a, c, n, rng, s, ncycles, bc=None, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_cap" if bc is None else "relax_cap_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        tail = [] if bc is None else [C.c_int(bc)]
        return self._run(ctx, [v, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, _ip(n), h, ct(s), C.c_int(ncycles), *tail), 0,
                         _shape(n), dtype)

    def relax_cap_from_zero(self, ctx, v, f, a, c, n, rng, s, ncycles, rim_is_zero, dtype=None):
        """v := 0, then ncycles sweeps; with rim_is_zero the given v must have zero boundary entries (its interior is ignored)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_cap_from_zero", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, _ip(n), h, ct(s), C.c_int(ncycles),
                                                                    C.c_int(int(rim_is_zero))), 0, _shape(n), dtype)

    def residual_cap(self, ctx, v, f, a, c, n, rng, s, bc=None, store=True, want_sum=True, dtype=None):
        """(r, sum of squares): r None with store=False, the sum None with want_sum=False; with bc over all unknowns"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_cap" if bc is None else "residual_cap_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        tail = [] if bc is None else [C.c_int(bc)]
        arrays = [xs_pack(np.ascontiguousarray(x, dtype)) for x in (v, f, a, c)] + [xs_pack(np.zeros(_shape(n), dtype)) if store else None]
        (_, _, _, _, ro), sums = self._krylov(ctx, n, arrays, [],
                                              lambda w, s0, x, b, aa, cc, d: fn(ctx._h, x, b, aa, cc, d, _ip(n), h, ct(s),
                                                                                w if want_sum else None, s0 if want_sum else None, *tail),
                                              dtype, 1, None if bc is None else self._krylov_work_bc)
        return (xs_unpack(ro, n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def apply_cap_dot(self, ctx, p, a, c, n, rng, s, bc=None, q=None, dtype=None):
        """q = A p with A = div(a grad .) - s c, and <p, q> (with bc: at every unknown, and <p, q>_W): returns (q, pq)"""
        dtype = dtype or p.dtype
        fn, ct = self._fn("apply_cap_dot" if bc is None else "apply_cap_dot_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        tail = [] if bc is None else [C.c_int(bc)]
        q = np.zeros(_shape(n), dtype) if q is None else q
        arrays = [xs_pack(np.ascontiguousarray(x, dtype)) for x in (p, a, c, q)]
        (_, _, _, qo), sums = self._krylov(ctx, n, arrays, [], lambda w, s0, x, aa, cc, b: fn(ctx._h, x, aa, cc, b, _ip(n), h, ct(s), w, s0, *tail),
                                           dtype, 1, None if bc is None else self._krylov_work_bc)
        return xs_unpack(qo, n[0]), float(sums[0])

    def cap_rhs(self, ctx, u, c, q, qscale, s, n, bc=None, f=None, dtype=None):
        """f = (-((s*c)*u)) - qscale*q on the interior, with bc on all unknowns (q None: -((s*c)*u)); f: the array written into"""
        dtype = dtype or u.dtype
        fn, ct = self._fn("cap_rhs" if bc is None else "cap_rhs_bc", dtype)
        tail = [] if bc is None else [C.c_int(bc)]
        f = np.zeros(_shape(n), dtype) if f is None else f
        return self._run(ctx, [u, c, q, f], lambda a, cc, b, d: fn(ctx._h, a, cc, b, ct(qscale), ct(s), d, _ip(n), *tail), 3, _shape(n), dtype)

    # ---- homogeneous Neumann faces (x-split only, mgx3dxs_*_bc): the wrappers above with the face mask bc as their last argument
    def relax_shift_bc(self, ctx, v, f, n, rng, s, ncycles, bc, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_shift_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, _ip(n), h, ct(s), C.c_int(ncycles), C.c_int(bc)), 0, _shape(n), dtype)

    def relax_coef_bc(self, ctx, v, f, a, n, rng, s, ncycles, bc, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_coef_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, _ip(n), h, ct(s), C.c_int(ncycles), C.c_int(bc)), 0, _shape(n),
                         dtype)

    def residual_shift_bc(self, ctx, v, f, n, rng, s, bc, store=True, want_sum=True, dtype=None):
        """(r, sum of squares over all unknowns): r None with store=False, the sum None with want_sum=False"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_shift_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        arrays = [xs_pack(np.ascontiguousarray(a, dtype)) for a in (v, f)] + [xs_pack(np.zeros(_shape(n), dtype)) if store else None]
        (_, _, ro), sums = self._krylov(ctx, n, arrays, [],
                                        lambda w, s0, a, b, c: fn(ctx._h, a, b, c, _ip(n), h, ct(s), w if want_sum else None,
                                                                  s0 if want_sum else None, C.c_int(bc)), dtype, 1)
        return (xs_unpack(ro, n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def residual_coef_bc(self, ctx, v, f, a, n, rng, s, bc, store=True, want_sum=True, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_coef_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        arrays = [xs_pack(np.ascontiguousarray(x, dtype)) for x in (v, f, a)] + [xs_pack(np.zeros(_shape(n), dtype)) if store else None]
        (_, _, _, ro), sums = self._krylov(ctx, n, arrays, [],
                                           lambda w, s0, x, b, c, d: fn(ctx._h, x, b, c, d, _ip(n), h, ct(s), w if want_sum else None,
                                                                        s0 if want_sum else None, C.c_int(bc)), dtype, 1)
        return (xs_unpack(ro, n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def restrict_bc(self, ctx, fine, n, bc, coarse=None, dtype=None):
        """coarse: the array the call writes into (every point is written; default zeros)"""
        dtype = dtype or fine.dtype
        fn, _ = self._fn("restrict_bc", dtype)
        cn = coarse_size(n)
        coarse = np.zeros(_shape(cn), dtype) if coarse is None else coarse
        return self._run(ctx, [fine, coarse], lambda f, c: fn(ctx._h, f, _ip(n), c, _ip(cn), C.c_int(bc)), 1, _shape(cn), dtype)

    def interpolate_bc(self, ctx, fine, n, coarse, bc, dtype=None):
        dtype = dtype or fine.dtype
        fn, _ = self._fn("interpolate_bc", dtype)
        cn = coarse_size(n)
        return self._run(ctx, [fine, coarse], lambda f, c: fn(ctx._h, f, _ip(n), c, _ip(cn), C.c_int(bc)), 0, _shape(n), dtype)

    def interpolate_correct_bc(self, ctx, v, n, coarse, bc, dtype=None):
        dtype = dtype or v.dtype
        fn, _ = self._fn("interpolate_correct_bc", dtype)
        cn = coarse_size(n)
        return self._run(ctx, [v, coarse], lambda a, c: fn(ctx._h, a, _ip(n), c, _ip(cn), C.c_int(bc)), 0, _shape(n), dtype)

    def shift_rhs_bc(self, ctx, u, q, qscale, s, n, bc, f=None, dtype=None):
        """f = (-(s*u)) - qscale*q on all unknowns (q None: -(s*u)); f: the array written into (default zeros)"""
        dtype = dtype or u.dtype
        fn, ct = self._fn("shift_rhs_bc", dtype)
        f = np.zeros(_shape(n), dtype) if f is None else f
        return self._run(ctx, [u, q, f], lambda a, b, c: fn(ctx._h, a, b, ct(qscale), ct(s), c, _ip(n), C.c_int(bc)), 2, _shape(n), dtype)

    def set_rim_bc(self, ctx, v, n, value, bc, dtype=None):
        """v := value at the unknowns on the faces of bc, nothing else"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("set_rim_bc", dtype)
        return self._run(ctx, [v], lambda a: fn(ctx._h, a, _ip(n), ct(value), C.c_int(bc)), 0, _shape(n), dtype)

    # ---- convective and prescribed-flux walls (x-split only, mgx3dxs_*_wall): the _bc wrappers with the six betas behind bc;
    # a: None = the shifted operator, c: None = no capacity
    def _wall_name(self, base, a, c):
        return {"relax": "relax_%s_wall", "residual": "residual_%s_wall"}[base] % ("cap" if c is not None else "coef" if a is not None else "shift")

    def relax_wall(self, ctx, v, f, a, c, n, rng, s, ncycles, bc, beta, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn(self._wall_name("relax", a, c), dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta, ct)
        arrays = [v, f] + [x for x in (a, c) if x is not None]
        return self._run(ctx, arrays, lambda vp, fp, *ac: fn(ctx._h, vp, fp, *ac, _ip(n), h, ct(s), C.c_int(ncycles), C.c_int(bc), b), 0,
                         _shape(n), dtype)

    def residual_wall(self, ctx, v, f, a, c, n, rng, s, bc, beta, store=True, want_sum=True, dtype=None):
        """(r, sum of squares over all unknowns): r None with store=False, the sum None with want_sum=False"""
        dtype = dtype or v.dtype
        fn, ct = self._fn(self._wall_name("residual", a, c), dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta, ct)
        arrays = [xs_pack(np.ascontiguousarray(x, dtype)) for x in (v, f, a, c) if x is not None]
        arrays.append(xs_pack(np.zeros(_shape(n), dtype)) if store else None)
        outs, sums = self._krylov(ctx, n, arrays, [],
                                  lambda w, s0, *ptrs: fn(ctx._h, *ptrs, _ip(n), h, ct(s), w if want_sum else None, s0 if want_sum else None,
                                                          C.c_int(bc), b), dtype, 1, self._krylov_work_bc)
        return (xs_unpack(outs[-1], n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def apply_dot_wall(self, ctx, p, a, c, n, rng, s, bc, beta, q=None, dtype=None):
        """q = A p at every unknown and <p, q>_W: returns (q, pq); q: the array written into (default zeros)"""
        dtype = dtype or p.dtype
        name = "apply_cap_dot_wall" if c is not None else "apply_coef_dot_wall" if a is not None else "laplace_dot_shift_wall"
        fn, ct = self._fn(name, dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta, ct)
        q = np.zeros(_shape(n), dtype) if q is None else q
        outs, sums = self._krylov_bc(ctx, n, [x for x in (p, a, c) if x is not None] + [q], [],
                                     lambda w, s0, *ptrs: fn(ctx._h, *ptrs, _ip(n), h, ct(s), w, s0, C.c_int(bc), b), dtype, 1)
        return outs[-1], float(sums[0])

    def wall_rhs(self, ctx, f, n, rng, g, bc, dtype=None):
        """f -= 2 g / h at the unknowns on the faces of bc with g != 0"""
        dtype = dtype or f.dtype
        fn, ct = self._fn("wall_rhs", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [f], lambda fp: fn(ctx._h, fp, _ip(n), h, _rp(g, ct), C.c_int(bc)), 0, _shape(n), dtype)

    # ---- pinned interior nodes (x-split only, mgx3dxs_pin_*): mask in the reference layout, values an array over the grid
    def pin_list(self, n, mask, values=None, dtype=np.float64):
        """(idx, val, end): the list of a mask as the library builds it (host arrays)"""
        s, ct = _ct(dtype)
        fn = getattr(lib, "mgx3dxs_pin_list_" + s)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        assert mask.shape == _shape(n), (mask.shape, n)
        end = (C.c_uint * 2)()
        check(fn(_ip(n), mask.ctypes.data_as(C.c_void_p), None, None, None, end))
        idx, val = np.zeros(max(end[1], 1), np.uint32), np.zeros(max(end[1], 1), dtype)
        vals = None if values is None else np.ascontiguousarray(values, dtype)
        check(fn(_ip(n), mask.ctypes.data_as(C.c_void_p), None if vals is None else vals.ctypes.data_as(C.c_void_p),
                 idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), end))
        return idx[:end[1]], val[:end[1]], (int(end[0]), int(end[1]))

    def pin_put(self, ctx, v, n, mask, values=None, first=None, count=None, dtype=None):
        """v with the values (None: zeros) at the list entries [first, first + count) of the mask's pinned points (default: all)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("pin_put", dtype)
        idx, val, end = self.pin_list(n, mask, values, dtype)
        first = 0 if first is None else int(first)
        count = end[1] - first if count is None else int(count)
        assert 0 <= first and first + count <= end[1], (first, count, end)
        di = ctx.to_device(idx) if len(idx) else None
        dv = ctx.to_device(val) if values is not None and len(val) else None
        try:
            return self._run(ctx, [v], lambda a: fn(ctx._h, a, di, dv, C.c_uint(first), C.c_uint(count)), 0, _shape(n), dtype)
        finally:
            for p in (di, dv):
                if p is not None:
                    ctx.free(p)

    def relax_pin(self, ctx, v, f, n, rng, s, ncycles, mask, values=None, a=None, c=None, mean=None, bc=0, beta=None, dtype=None):
        """ncycles sweeps of the operator that a, c and mean say (a None: shifted; mean "harmonic": the _hmean entry) with the mask's
        points pinned to values (None: zeros); v should hold them on entry"""
        dtype = dtype or v.dtype
        harm = mean == "harmonic"
        assert mean in (None, "arithmetic", "harmonic") and not (harm and a is None)
        name = "relax_hmean_pin" if harm else "relax_cap_pin" if c is not None else "relax_coef_pin" if a is not None else "relax_shift_pin"
        fn, ct = self._fn(name, dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta if beta is not None else [0.0] * 6, ct)
        idx, val, end = self.pin_list(n, mask, values, dtype)
        di = ctx.to_device(idx) if len(idx) else None
        dv = ctx.to_device(val) if values is not None and len(val) else None
        arrays = [v, f] + ([a, c] if harm else [x for x in (a, c) if x is not None])
        try:
            return self._run(ctx, arrays, lambda vp, fp, *ac: fn(ctx._h, vp, fp, *ac, _ip(n), h, ct(s), C.c_int(ncycles), C.c_int(bc), b, di,
                                                                  (C.c_uint * 2)(*end), dv), 0, _shape(n), dtype)
        finally:
            for p in (di, dv):
                if p is not None:
                    ctx.free(p)

    # ---- harmonic-mean face coefficients (x-split only, mgx3dxs_*_hmean): views of the four entries, which take the _wall form;
    # c: None = no capacity, bc: None = the interior alone, beta: None = six zeros (homogeneous Neumann faces)
    def relax_hmean(self, ctx, v, f, a, n, rng, s, ncycles, c=None, bc=None, beta=None, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_hmean_wall", dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta if beta is not None else [0.0] * 6, ct)
        return self._run(ctx, [v, f, a, c], lambda vp, fp, ap, cp: fn(ctx._h, vp, fp, ap, cp, _ip(n), h, ct(s), C.c_int(ncycles),
                                                                    C.c_int(bc or 0), b), 0, _shape(n), dtype)

    def relax_hmean_from_zero(self, ctx, v, f, a, n, rng, s, ncycles, rim_is_zero, c=None, dtype=None):
        """v := 0, then ncycles sweeps; with rim_is_zero the given v must have zero boundary entries (its interior is ignored)"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax_hmean_from_zero", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        return self._run(ctx, [v, f, a, c], lambda vp, fp, ap, cp: fn(ctx._h, vp, fp, ap, cp, _ip(n), h, ct(s), C.c_int(ncycles),
                                                                    C.c_int(int(rim_is_zero))), 0, _shape(n), dtype)

    def residual_hmean(self, ctx, v, f, a, n, rng, s, c=None, bc=None, beta=None, store=True, want_sum=True, dtype=None):
        """(r, sum of squares over all unknowns): r None with store=False, the sum None with want_sum=False"""
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_hmean_wall", dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta if beta is not None else [0.0] * 6, ct)
        arrays = [xs_pack(np.ascontiguousarray(x, dtype)) if x is not None else None for x in (v, f, a, c)]
        arrays.append(xs_pack(np.zeros(_shape(n), dtype)) if store else None)
        outs, sums = self._krylov(ctx, n, arrays, [],
                                  lambda w, s0, *ptrs: fn(ctx._h, *ptrs, _ip(n), h, ct(s), w if want_sum else None, s0 if want_sum else None,
                                                          C.c_int(bc or 0), b), dtype, 1, self._krylov_work_bc)
        return (xs_unpack(outs[-1], n[0]) if store else None), (float(sums[0]) if want_sum else None)

    def apply_hmean_dot(self, ctx, p, a, n, rng, s, c=None, bc=None, beta=None, q=None, dtype=None):
        """q = A p at every unknown and <p, q>_W (without a mask: on the interior, and <p, q>): returns (q, pq); q: the array written
        into (default zeros)"""
        dtype = dtype or p.dtype
        fn, ct = self._fn("apply_hmean_dot_wall", dtype)
        h, b = _rp(grid_spacing(n, rng, dtype), ct), _rp(beta if beta is not None else [0.0] * 6, ct)
        q = np.zeros(_shape(n), dtype) if q is None else q
        outs, sums = self._krylov_bc(ctx, n, [p, a, c, q], [],
                                     lambda w, s0, *ptrs: fn(ctx._h, *ptrs, _ip(n), h, ct(s), w, s0, C.c_int(bc or 0), b), dtype, 1)
        return outs[-1], float(sums[0])

    # ---- vector kernels of the preconditioned CG solve (x-split only; every array in the reference layout on the host)
    # every work array is uploaded with WORK_GUARD sentinel doubles behind the elements the library asks for, and the
    # sentinels are looked at after the call: a kernel that writes into the next WORK_GUARD doubles behind its work array
    # fails the call (a write further out is not seen)
    WORK_GUARD = 1024
    WORK_SENTINEL = 0x7FF8C0DEC0DE0001

    def _work_alloc(self, ctx, elems):
        host = np.zeros(max(int(elems), 1) + self.WORK_GUARD, np.float64)
        host[-self.WORK_GUARD:] = np.array(self.WORK_SENTINEL, np.uint64).view(np.float64)
        return ctx.to_device(host), max(int(elems), 1)

    def _work_check(self, ctx, work, elems):
        tail = ctx.to_host(C.c_void_p(work.value + 8 * elems), (self.WORK_GUARD,), np.float64).view(np.uint64)
        bad = np.nonzero(tail != self.WORK_SENTINEL)[0]
        if bad.size:
            raise AssertionError("work array of %d doubles: %d entries behind it were written, the first at +%d" % (elems, bad.size, bad[0]))

    def _krylov_work(self, ctx, n, dtype):
        s, _ = _ct(dtype)
        fn = getattr(lib, "mgx3dxs_krylov_work_elems_" + s)
        fn.restype = C.c_size_t
        return self._work_alloc(ctx, fn(_ip(n)))

    def _krylov(self, ctx, n, arrays, scalars, call, dtype, nsum, work_alloc=None):
        """upload arrays (x-split) and the device doubles `scalars`, run call(work, sums, *scalar ptrs, *array ptrs), return
        (arrays as stored, padded rows, sums)"""
        assert self.xsplit, "the Krylov kernels exist for the x-split layout only"
        work, welems = (work_alloc or self._krylov_work)(ctx, n, dtype)
        dev = [ctx.to_device(np.array(scalars + [0.0] * nsum, np.float64))]
        ptrs = [ctx.to_device(a) if a is not None else None for a in arrays]
        try:
            sp = [C.c_void_p(dev[0].value + 8 * i) for i in range(len(scalars) + nsum)]
            check(call(work, *sp, *ptrs))
            self._work_check(ctx, work, welems)
            sums = ctx.to_host(dev[0], (len(scalars) + nsum,), np.float64)[len(scalars):]
            return [ctx.to_host(p, a.shape, dtype) if p is not None else None for p, a in zip(ptrs, arrays)], sums
        finally:
            for p in ptrs + dev + [work]:
                if p is not None:
                    ctx.free(p)

    def laplace_dot(self, ctx, p, n, rng, q=None, packed=False, dtype=None):
        """q = A p (CORRECT Laplacian) and <p, q>: returns (q, pq).  q: the array written into (default zeros; its boundary
        and pad entries are left as they are).  packed=True: p and q are given, and q returned, as stored (x-split)."""
        dtype = dtype or p.dtype
        fn, ct = self._fn("laplace_dot", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        pp = p if packed else xs_pack(np.ascontiguousarray(p, dtype))
        qq = np.zeros_like(pp) if q is None else (q if packed else xs_pack(np.ascontiguousarray(q, dtype)))
        (_, qo), sums = self._krylov(ctx, n, [pp, qq], [], lambda w, s0, a, b: fn(ctx._h, a, b, _ip(n), h, w, s0), dtype, 1)
        return (qo if packed else xs_unpack(qo, n[0])), float(sums[0])

    def cg_update(self, ctx, x, p, r, q, n, alpha, dtype=None):
        """x += (real)alpha p (x None: skipped); r -= (real)alpha q; arrays packed (x-split).  Returns (x, r, <r, r>)."""
        dtype = dtype or r.dtype
        fn, _ = self._fn("cg_update", dtype)
        (xo, _, ro, _), sums = self._krylov(ctx, n, [x, p, r, q], [float(alpha)],
                                            lambda w, a, s0, xp, pp, rp, qp: fn(ctx._h, xp, pp, rp, qp, _ip(n), a, w, s0), dtype, 1)
        return xo, ro, float(sums[0])

    def dot2(self, ctx, a, b, c, n, dtype=None):
        """(<a, b>, <a, c>) over the interior (c None: <a, c> is None); arrays packed (x-split)"""
        dtype = dtype or a.dtype
        fn, _ = self._fn("dot2", dtype)
        _, sums = self._krylov(ctx, n, [a, b, c], [], lambda w, s0, s1, ap, bp, cp: fn(ctx._h, ap, bp, cp, _ip(n), w, s0), dtype, 2)
        return float(sums[0]), (float(sums[1]) if c is not None else None)

    def cg_direction(self, ctx, x, p, z, n, alpha=None, beta=None, dtype=None):
        """x += (real)alpha p (x None: skipped); then p = z + (real)beta p, or p = z when beta is None (z None: p kept);
        arrays packed (x-split).  Returns (x, p)."""
        dtype = dtype or p.dtype
        fn, _ = self._fn("cg_direction", dtype)

        def call(w, a, b, xp, pp, zp):
            return fn(ctx._h, xp, pp, zp, _ip(n), a if alpha is not None else None, b if beta is not None else None)
        (xo, po, _), _ = self._krylov(ctx, n, [x, p, z], [float(alpha or 0.0), float(beta or 0.0)], call, dtype, 0)
        return xo, po

    # ---- the same over ALL unknowns of a grid with the face mask bc (mgx3dxs_*_bc): the dots weighted by 1/2 per Neumann face an
    # unknown lies on, cg_update's <r, r> unweighted; arrays in the reference layout
    def _krylov_work_bc(self, ctx, n, dtype):
        fn = getattr(lib, "mgx3dxs_krylov_work_elems_bc_" + _ct(dtype)[0])
        fn.restype = C.c_size_t
        return self._work_alloc(ctx, fn(_ip(n)))

    def _krylov_bc(self, ctx, n, arrays, scalars, call, dtype, nsum):
        """_krylov with the larger work array and arrays given and returned in the reference layout"""
        packed = [xs_pack(np.ascontiguousarray(a, dtype)) if a is not None else None for a in arrays]
        outs, sums = self._krylov(ctx, n, packed, scalars, call, dtype, nsum, self._krylov_work_bc)
        return [xs_unpack(o, n[0]) if o is not None else None for o in outs], sums

    def laplace_dot_shift_bc(self, ctx, p, n, rng, s, bc, q=None, dtype=None):
        """q = A p at every unknown (A = Laplacian - s) and <p, q>_W: returns (q, pq); q: the array written into (default zeros)"""
        dtype = dtype or p.dtype
        fn, ct = self._fn("laplace_dot_shift_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        q = np.zeros(_shape(n), dtype) if q is None else q
        (_, qo), sums = self._krylov_bc(ctx, n, [p, q], [], lambda w, s0, a, b: fn(ctx._h, a, b, _ip(n), h, ct(s), w, s0, C.c_int(bc)), dtype, 1)
        return qo, float(sums[0])

    def apply_coef_dot_bc(self, ctx, p, a, n, rng, s, bc, q=None, dtype=None):
        """q = A p at every unknown (A = div(a grad .) - s) and <p, q>_W: returns (q, pq)"""
        dtype = dtype or p.dtype
        fn, ct = self._fn("apply_coef_dot_bc", dtype)
        h = _rp(grid_spacing(n, rng, dtype), ct)
        q = np.zeros(_shape(n), dtype) if q is None else q
        (_, _, qo), sums = self._krylov_bc(ctx, n, [p, a, q], [],
                                           lambda w, s0, x, c, b: fn(ctx._h, x, c, b, _ip(n), h, ct(s), w, s0, C.c_int(bc)), dtype, 1)
        return qo, float(sums[0])

    def cg_update_bc(self, ctx, x, p, r, q, n, alpha, bc, dtype=None):
        """x += (real)alpha p (x None: skipped); r -= (real)alpha q at every unknown.  Returns (x, r, <r, r> unweighted)."""
        dtype = dtype or r.dtype
        fn, _ = self._fn("cg_update_bc", dtype)
        (xo, _, ro, _), sums = self._krylov_bc(ctx, n, [x, p, r, q], [float(alpha)],
                                               lambda w, a, s0, xp, pp, rp, qp: fn(ctx._h, xp, pp, rp, qp, _ip(n), a, w, s0, C.c_int(bc)), dtype, 1)
        return xo, ro, float(sums[0])

    def dot2_bc(self, ctx, a, b, c, n, bc, dtype=None):
        """(<a, b>_W, <a, c>_W) over all unknowns (c None: <a, c>_W is None)"""
        dtype = dtype or a.dtype
        fn, _ = self._fn("dot2_bc", dtype)
        _, sums = self._krylov_bc(ctx, n, [a, b, c], [], lambda w, s0, s1, ap, bp, cp: fn(ctx._h, ap, bp, cp, _ip(n), w, s0, C.c_int(bc)), dtype, 2)
        return float(sums[0]), (float(sums[1]) if c is not None else None)

    def cg_direction_bc(self, ctx, x, p, z, n, bc, alpha=None, beta=None, dtype=None):
        """cg_direction at every unknown.  Returns (x, p)."""
        dtype = dtype or p.dtype
        fn, _ = self._fn("cg_direction_bc", dtype)

        def call(w, a, b, xp, pp, zp):
            return fn(ctx._h, xp, pp, zp, _ip(n), a if alpha is not None else None, b if beta is not None else None, C.c_int(bc))
        (xo, po, _), _ = self._krylov_bc(ctx, n, [x, p, z], [float(alpha or 0.0), float(beta or 0.0)], call, dtype, 0)
        return xo, po

    def project_bc(self, ctx, a, n, bc, dtype=None):
        """a -= (real)mean with mean = sum_W(a) / sum(W) over all unknowns.  Returns (a, mean)."""
        dtype = dtype or a.dtype
        fn, _ = self._fn("project_bc", dtype)
        (ao,), sums = self._krylov_bc(ctx, n, [a], [], lambda w, s0, ap: fn(ctx._h, ap, _ip(n), w, s0, C.c_int(bc)), dtype, 1)
        return ao, float(sums[0])

    # ---- vector kernels of the mixed-precision solve (fp64 only): fp64 arrays and fp32 arrays (r32, z32) packed (x-split), each
    # in its own precision's geometry; s / inv_s are applied as given (the solver passes powers of two)
    def _mixed(self, ctx, n, arrays, scalars, call, nsum):
        """upload arrays (each in its own dtype) and the device doubles `scalars`, run call(work, *scalar ptrs, *array ptrs),
        return (arrays as stored, sums)"""
        assert self.xsplit, "the mixed kernels exist for the x-split layout only"
        fn = lib.mgx3dxs_mixed_work_elems_f64
        fn.restype = C.c_size_t
        work, welems = self._work_alloc(ctx, fn(_ip(n)))
        dev = ctx.to_device(np.array(scalars + [0.0] * nsum + [0.0], np.float64))
        ptrs = [ctx.to_device(a) if a is not None else None for a in arrays]
        try:
            sp = [C.c_void_p(dev.value + 8 * i) for i in range(len(scalars) + nsum)]
            check(call(work, *sp, *ptrs))
            self._work_check(ctx, work, welems)
            sums = ctx.to_host(dev, (len(scalars) + nsum,), np.float64)[len(scalars):]
            return [ctx.to_host(p, a.shape, a.dtype) if p is not None else None for p, a in zip(ptrs, arrays)], sums
        finally:
            for p in ptrs + [dev, work]:
                if p is not None:
                    ctx.free(p)

    def correct_residual_demote(self, ctx, x, b, r32, n, rng, s, z=None, inv_sz=1.0, xo=None):
        """[xo = x + float64(z) * inv_sz;] r = b - A xo (A x without z); r32 = float32(r s); returns (xo or None, r32, <r, r>).
        xo: the array corrected into (default: a copy of x, so its boundary and pads are x's)"""
        h = _rp(grid_spacing(n, rng, np.float64), C.c_double)
        if z is not None and xo is None:
            xo = x.copy()
        fn = lib.mgx3dxs_correct_residual_demote_f64

        def call(w, s0, xp, op, bp, zp, rp):
            return fn(ctx._h, xp, op, bp, zp, C.c_double(inv_sz), rp, C.c_double(s), _ip(n), h, w, s0)
        (_, xo_, _, _, ro), sums = self._mixed(ctx, n, [x, xo if z is not None else None, b, z, r32], [], call, 1)
        return xo_, ro, float(sums[0])

    def correct_residual_demote_plan(self, ctx, n, rng, with_correction=False):
        """what correct_residual_demote launches on this level with the context's present parameters: a dict of rows (per
        wave), zchunk (planes per run), gx, gy, gz (tiles across x and y, plane runs), mode (1: dividing, 3: exact
        reciprocals) and launches"""
        out = (C.c_int * 7)()
        h = _rp(grid_spacing(n, rng, np.float64), C.c_double)
        check(lib.mgx3dxs_correct_residual_demote_plan_f64(ctx._h, _ip(n), h, C.c_int(int(with_correction)), out))
        return dict(zip(("rows", "zchunk", "gx", "gy", "gz", "mode", "launches"), out))

    def demote(self, ctx, r, r32, n, s):
        """r32 = float32(r s) on the interior; returns r32"""
        (_, ro), _ = self._mixed(ctx, n, [r, r32], [], lambda w, rp, op: lib.mgx3dxs_demote_f64(ctx._h, rp, op, C.c_double(s), _ip(n)), 0)
        return ro

    def cg_update_demote(self, ctx, x, p, r, q, r32, n, alpha, s):
        """x += alpha p (x None: skipped); r -= alpha q; r32 = float32(r s).  Returns (x, r, r32, <r, r>)."""
        def call(w, a, s0, xp, pp, rp, qp, op):
            return lib.mgx3dxs_cg_update_demote_f64(ctx._h, xp, pp, rp, qp, op, C.c_double(s), _ip(n), a, w, s0)
        (xo, _, ro, _, o32), sums = self._mixed(ctx, n, [x, p, r, q, r32], [float(alpha)], call, 1)
        return xo, ro, o32, float(sums[0])

    def dot2_mixed(self, ctx, z32, inv_s, b, c, n):
        """(<z, b>, <z, c>) with z = float64(z32) * inv_s (c None: <z, c> is None)"""
        def call(w, s0, s1, zp, bp, cp):
            return lib.mgx3dxs_dot2_mixed_f64(ctx._h, zp, C.c_double(inv_s), bp, cp, _ip(n), w, s0)
        _, sums = self._mixed(ctx, n, [z32, b, c], [], call, 2)
        return float(sums[0]), (float(sums[1]) if c is not None else None)

    def cg_direction_mixed(self, ctx, x, p, z32, inv_s, n, alpha=None, beta=None):
        """x += alpha p (x None: skipped); p = z + beta p, or p = z when beta is None, z = float64(z32) * inv_s.  Returns (x, p)."""
        def call(w, a, b, xp, pp, zp):
            return lib.mgx3dxs_cg_direction_mixed_f64(ctx._h, xp, pp, zp, C.c_double(inv_s), _ip(n), a if alpha is not None else None,
                                                      b if beta is not None else None)
        (xo, po, _), _ = self._mixed(ctx, n, [x, p, z32], [float(alpha or 0.0), float(beta or 0.0)], call, 0)
        return xo, po

    # ---- block vector kernels of the eigensolver (fp64 only, mgx3dxs_block_*_f64): arrays packed (x-split), as stored, so that
    # a caller controls the pad and Dirichlet entries too; bc is the face mask the weights are formed from
    def _block(self, ctx, n, arrays, nsum, call):
        """upload the packed arrays, run call(work, sums, ptrs), return (arrays as stored afterwards, sums)"""
        assert self.xsplit, "the block kernels exist for the x-split layout only"
        fn = lib.mgx3dxs_block_work_elems_f64
        fn.restype = C.c_size_t
        work, welems = self._work_alloc(ctx, fn(_ip(n)))
        dev, selems = self._work_alloc(ctx, nsum)  # (the sums with the same guards behind them)
        ptrs = [ctx.to_device(np.ascontiguousarray(a, np.float64)) if a is not None else None for a in arrays]
        try:
            check(call(work, dev, ptrs))
            self._work_check(ctx, work, welems)
            self._work_check(ctx, dev, selems)
            sums = ctx.to_host(dev, (selems,), np.float64)[:nsum]
            return [ctx.to_host(p, a.shape, np.float64) if p is not None else None for p, a in zip(ptrs, arrays)], sums
        finally:
            for p in ptrs + [dev, work]:
                if p is not None:
                    ctx.free(p)

    @staticmethod
    def _pp(ptrs):
        return (C.c_void_p * len(ptrs))(*[p.value if p is not None else None for p in ptrs])

    def block_gram(self, ctx, U, V, c, n, bc):
        """(<U_i, V_j>_W as an array of len(U) x len(V), <U_i, c V_j>_W likewise or None without c)"""
        nu, nv = len(U), len(V)

        def call(w, s, p):
            return lib.mgx3dxs_block_gram_f64(ctx._h, C.c_int(nu), self._pp(p[:nu]), C.c_int(nv), self._pp(p[nu:nu + nv]), p[nu + nv], _ip(n),
                                              C.c_int(bc), w, s)
        _, sums = self._block(ctx, n, list(U) + list(V) + [c], 2 * nu * nv, call)
        return sums[:nu * nv].reshape(nu, nv).copy(), (sums[nu * nv:].reshape(nu, nv).copy() if c is not None else None)

    def block_combine(self, ctx, S, Y, n, bc, out=None, alias=None):
        """out_i = sum_j Y[j][i] S_j at the unknowns.  out: the arrays written into (default zeros); alias = {i: j}: output i
        IS input j on the device (out[i] is then ignored).  Returns the outputs as stored afterwards."""
        Y = np.ascontiguousarray(Y, np.float64)
        nin, nout = Y.shape
        assert nin == len(S)
        alias = alias or {}
        out = [np.zeros_like(S[0]) for _ in range(nout)] if out is None else list(out)
        own = [i for i in range(nout) if i not in alias]

        def call(w, s, p):
            outs = [p[alias[i]] if i in alias else p[nin + own.index(i)] for i in range(nout)]
            return lib.mgx3dxs_block_combine_f64(ctx._h, C.c_int(nin), self._pp(p[:nin]), C.c_int(nout), self._pp(outs),
                                                 Y.ctypes.data_as(C.c_void_p), _ip(n), C.c_int(bc))
        res, _ = self._block(ctx, n, list(S) + [out[i] for i in own], 0, call)
        return [res[alias[i]] if i in alias else res[nin + own.index(i)] for i in range(nout)]

    def block_residual(self, ctx, AX, X, c, mu, n, bc, R=None):
        """R_i = AX_i + mu_i (c X_i) at the unknowns, 0 at the Dirichlet points.  Returns (R, <R_i, R_i>_W, <X_i, X_i>_W)."""
        k = len(X)
        mu = np.ascontiguousarray(mu, np.float64)
        R = [np.zeros_like(X[0]) for _ in range(k)] if R is None else list(R)

        def call(w, s, p):
            return lib.mgx3dxs_block_residual_f64(ctx._h, C.c_int(k), self._pp(p[:k]), self._pp(p[k:2 * k]), p[3 * k],
                                                  mu.ctypes.data_as(C.c_void_p), self._pp(p[2 * k:3 * k]), _ip(n), C.c_int(bc), w, s)
        res, sums = self._block(ctx, n, list(AX) + list(X) + R + [c], 2 * k, call)
        return res[2 * k:3 * k], sums[:k].copy(), sums[k:].copy()

    def eigen_start(self, ctx, index, n, bc, v=None):
        """the start vector `index` of the eigensolver, as stored; v: the array written into (default zeros)"""
        H, P_ = xs_geometry(n[0], 8)
        v = np.zeros(_shape(n)[:-1] + (P_,), np.float64) if v is None else v
        (vo,), _ = self._block(ctx, n, [v], 0, lambda w, s, p: lib.mgx3dxs_eigen_start_f64(ctx._h, p[0], C.c_int(index), _ip(n), C.c_int(bc)))
        return vo


class _Ops2D(_Ops):
    def __init__(self):
        super().__init__(2)

    def _geom(self, n, rng, A, dtype, ct):
        t = np.dtype(dtype).type
        return (_rp(grid_spacing(n, rng, dtype), ct), _rp([t(rng[0]), t(rng[2])], ct), _rp(A, ct))

    def relax(self, ctx, v, f, n, rng, A, alfa, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("relax", dtype)
        h, a, AA = self._geom(n, rng, A, dtype, ct)
        return self._run(ctx, [v, f], lambda x, y: fn(ctx._h, x, y, _ip(n), h, a, AA, C.c_int(alfa), C.c_int(ncycles)), 0,
                         _shape(n), dtype)

    def jacobi(self, ctx, v, f, n, rng, A, alfa, omega, ncycles, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("jacobi", dtype)
        h, a, AA = self._geom(n, rng, A, dtype, ct)
        return self._run(ctx, [v, np.zeros_like(v), f],
                         lambda x, t, y: fn(ctx._h, x, t, y, _ip(n), h, a, AA, C.c_int(alfa), ct(omega), C.c_int(ncycles)), 0,
                         _shape(n), dtype)

    def residual(self, ctx, v, f, n, rng, A, alfa, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual", dtype)
        h, a, AA = self._geom(n, rng, A, dtype, ct)
        r = np.zeros(_shape(n), dtype)
        return self._run(ctx, [v, f, r], lambda x, y, z: fn(ctx._h, x, y, z, _ip(n), h, a, AA, C.c_int(alfa)), 2, _shape(n),
                         dtype)


    def residual_restrict(self, ctx, v, f, n, rng, A, alfa, dtype=None):
        dtype = dtype or v.dtype
        fn, ct = self._fn("residual_restrict", dtype)
        h, a, AA = self._geom(n, rng, A, dtype, ct)
        cn = coarse_size(n)
        c = np.zeros(_shape(cn), dtype)
        return self._run(ctx, [v, f, c], lambda x, y, z: fn(ctx._h, x, y, _ip(n), h, a, AA, C.c_int(alfa), z, _ip(cn)), 2,
                         _shape(cn), dtype)

    def interpolate_correct(self, ctx, v, n, coarse, dtype=None):
        dtype = dtype or v.dtype
        fn, _ = self._fn("interpolate_correct", dtype)
        cn = coarse_size(n)
        return self._run(ctx, [v, coarse], lambda x, c: fn(ctx._h, x, _ip(n), c, _ip(cn)), 0, _shape(n), dtype)


def _ops2d_fused_down(self, ctx, v, f, n, rng, A, alfa, ncycles, v_zero=False, restrict=True, dtype=None):
    """(v_out, coarse_f) of mgx2d_relax_residual_restrict"""
    dtype = dtype or v.dtype
    fn, ct = self._fn("relax_residual_restrict", dtype)
    h, a, AA = self._geom(n, rng, A, dtype, ct)
    cn = coarse_size(n)
    pv, pf = ctx.to_device(np.ascontiguousarray(v, dtype)), ctx.to_device(np.ascontiguousarray(f, dtype))
    po, pc = ctx.to_device(np.full(_shape(n), np.nan, dtype)), ctx.to_device(np.full(_shape(cn), np.nan, dtype))
    try:
        check(fn(ctx._h, pv, po, pf, _ip(n), h, a, AA, C.c_int(alfa), C.c_int(ncycles), C.c_int(int(v_zero)),
                 pc if restrict else None, _ip(cn) if restrict else None))
        return ctx.to_host(po, _shape(n), dtype), (ctx.to_host(pc, _shape(cn), dtype) if restrict else None)
    finally:
        for p in (pv, pf, po, pc):
            ctx.free(p)


def _ops2d_fused_up(self, ctx, v, f, n, rng, A, alfa, coarse, ncycles, dtype=None):
    dtype = dtype or v.dtype
    fn, ct = self._fn("interpolate_correct_relax", dtype)
    h, a, AA = self._geom(n, rng, A, dtype, ct)
    cn = coarse_size(n)
    pv, pf = ctx.to_device(np.ascontiguousarray(v, dtype)), ctx.to_device(np.ascontiguousarray(f, dtype))
    po, pc = ctx.to_device(np.full(_shape(n), np.nan, dtype)), ctx.to_device(np.ascontiguousarray(coarse, dtype))
    try:
        check(fn(ctx._h, pv, po, pf, _ip(n), h, a, AA, C.c_int(alfa), pc, _ip(cn), C.c_int(ncycles)))
        return ctx.to_host(po, _shape(n), dtype)
    finally:
        for p in (pv, pf, po, pc):
            ctx.free(p)


_Ops2D.relax_residual_restrict = _ops2d_fused_down
_Ops2D.interpolate_correct_relax = _ops2d_fused_up

ops3d = _Ops3D()
ops3dxs = _Ops3D(xsplit=True)
ops2d = _Ops2D()


# --------------------------------------------------------------------------- hierarchy views
MG_GRAPH_REC_WORDS = 74  # mg_multigrid.h
MG_GRAPH_FLAG_ARRAYS = 6


class GraphRec(C.Structure):
    """mgGraphRec: the record a captured cycle is replayed under (mg_common.h mg_graph_record)"""
    _fields_ = [("w", C.c_uint * MG_GRAPH_REC_WORDS)]


class GraphFlags(C.Structure):
    """mgGraphFlags: the rim flags a captured cycle left behind"""
    _fields_ = [("a", (C.c_ubyte * 32) * MG_GRAPH_FLAG_ARRAYS)]


FACE_MEANS = {"arithmetic": 0, "harmonic": 1}  # MG_FACE_MEAN_*


def face_mean_mode(name):
    if not isinstance(name, str) or name not in FACE_MEANS:
        raise ValueError("face_mean must be 'arithmetic' or 'harmonic', not %r" % (name,))
    return FACE_MEANS[name]


class _PinSlot(C.Structure):
    """the last eight bytes of the unused graph_key: the table of the pinned nodes"""
    _fields_ = [("graph_key_head_", C.c_longlong * 28), ("pin", C.c_void_p)]


class _GraphKey(C.Union):
    """the unused graph_key of mgMultiGrid3D_<r>, whose first four bytes hold face_mean and whose last eight the pin table"""
    _anonymous_ = ("pin_",)
    _fields_ = [("graph_key", C.c_longlong * 29), ("face_mean", C.c_int), ("pin_", _PinSlot)]


def _grid3_struct(ct):
    class Grid3D(C.Structure):
        _fields_ = [("h_v", C.c_void_p), ("h_f", C.c_void_p), ("d_v", C.c_void_p), ("d_f", C.c_void_p),
                    ("d_r", C.c_void_p), ("d_e", C.c_void_p), ("sizeX", C.c_int), ("sizeY", C.c_int), ("sizeZ", C.c_int),
                    ("sizeXYZ", C.c_int * 3), ("h_x", ct), ("h_y", ct), ("h_z", ct), ("x_a", ct), ("x_b", ct),
                    ("y_a", ct), ("y_b", ct), ("z_a", ct), ("z_b", ct), ("d_a", C.c_void_p)]

    class MultiGrid3D(C.Structure):
        _anonymous_ = ("graph_key_",)
        _fields_ = [("grids3D", C.POINTER(C.POINTER(Grid3D))), ("numGrids", C.c_int), ("maxGrids", C.c_int),
                    ("ctx", C.c_void_p), ("residual_mode", C.c_int), ("fuse", C.c_int), ("layout", C.c_int),
                    ("smoother", C.c_int), ("omega", ct), ("use_graph", C.c_int), ("capturing", C.c_int),
                    ("graph_exec", C.c_void_p * 32), ("graph_key_", _GraphKey), ("wall", C.c_void_p), ("cap", C.c_void_p), ("pcg_fproj", C.c_void_p),
                    ("f_rim_zero", C.c_ubyte * 32),
                    ("v_rim_zero", C.c_ubyte * 32), ("e_rim_valid", C.c_ubyte * 32), ("pcg_x", C.c_void_p),
                    ("pcg_b", C.c_void_p), ("pcg_p", C.c_void_p), ("pcg_q", C.c_void_p), ("pcg_state", C.c_void_p),
                    ("pcg_work", C.c_void_p), ("pcg_graph_exec", C.c_void_p), ("bc", C.c_int), ("bc_reserved", C.c_int),
                    ("graph_rec", GraphRec * 32), ("graph_post", GraphFlags * 32), ("pcg_graph_rec", GraphRec),
                    ("pcg_graph_post", GraphFlags), ("pcg_mixed", C.c_void_p), ("coarsen", C.c_ubyte * 32), ("shift", ct)]

    return Grid3D, MultiGrid3D


def _grid2_struct(ct):
    class Grid2D(C.Structure):
        _fields_ = [("h_v", C.c_void_p), ("h_f", C.c_void_p), ("d_v", C.c_void_p), ("d_f", C.c_void_p),
                    ("d_r", C.c_void_p), ("d_e", C.c_void_p), ("sizeX", C.c_int), ("sizeY", C.c_int),
                    ("sizeXY", C.c_int * 2), ("h_x", ct), ("h_y", ct), ("x_a", ct), ("x_b", ct), ("y_a", ct), ("y_b", ct)]

    class MultiGrid2D(C.Structure):
        _fields_ = [("grids2D", C.POINTER(C.POINTER(Grid2D))), ("numGrids", C.c_int), ("maxGrids", C.c_int),
                    ("matrixA", ct * 4), ("sizeA", C.c_int), ("alfa", C.c_int), ("ctx", C.c_void_p), ("fuse", C.c_int),
                    ("smoother", C.c_int), ("omega", ct), ("use_graph", C.c_int), ("capturing", C.c_int),
                    ("graph_exec", C.c_void_p * 32), ("graph_key", C.c_longlong * 32), ("graph_rec", GraphRec * 32)]

    return Grid2D, MultiGrid2D


def _grid1_struct(ct):
    class Grid1D(C.Structure):
        _fields_ = [("h_v", C.POINTER(ct)), ("h_f", C.POINTER(ct)), ("sizeX", C.c_int), ("h_x", ct), ("x_a", ct),
                    ("x_b", ct)]

    class MultiGrid1D(C.Structure):
        _fields_ = [("grids1D", C.POINTER(C.POINTER(Grid1D))), ("numGrids", C.c_int), ("maxGrids", C.c_int)]

    return Grid1D, MultiGrid1D


def krylov_mode(krylov):
    """the C value of a `krylov` argument: False / 0 -> 0 (plain cycling), True / 1 -> 1 (flexible CG over the interior),
    "weighted" / 2 -> 2 (flexible CG in the weighted inner product over all unknowns, MG_KRYLOV_WEIGHTED)"""
    if isinstance(krylov, str):
        if krylov != "weighted":
            raise ValueError("krylov must be False, True, 2 or 'weighted', not %r" % (krylov,))
        return 2
    if not isinstance(krylov, (bool, np.bool_)) and krylov == 2:
        return 2
    return int(bool(krylov))


class _MGBase:
    _prefix = None

    def _call(self, name, *args):
        return check(getattr(lib, "%s_%s_%s" % (self._prefix, self._sfx, name))(self._mg, *args))

    @property
    def numGrids(self):
        return self._mg.contents.numGrids

    @numGrids.setter
    def numGrids(self, k):
        if not 1 <= int(k) <= self._mg.contents.maxGrids:
            raise ValueError("numGrids must be in [1, %d]" % self._mg.contents.maxGrids)
        self._mg.contents.numGrids = int(k)

    @property
    def use_graph(self):
        """2D / 3D: capture VCycle into a HIP graph on first use and replay it (mg_multigrid.h)"""
        return bool(self._mg.contents.use_graph)

    @use_graph.setter
    def use_graph(self, on):
        self._mg.contents.use_graph = 1 if on else 0

    @property
    def maxGrids(self):
        return self._mg.contents.maxGrids

    def set_smoother(self, name, omega=None):
        """'rbgs' = red-black Gauss-Seidel (the reference's smoother), 'jacobi' = weighted Jacobi (addition)"""
        self._mg.contents.smoother = {"rbgs": 0, "jacobi": 1}[name]
        if omega is not None:
            self._mg.contents.omega = float(omega)

    def VCycle(self, gridID, v1, v2):
        self._call("VCycle", C.c_int(gridID), C.c_int(v1), C.c_int(v2))

    def FullMultiGridVCycle(self, gridID, v0, v1, v2):
        self._call("FullMultiGridVCycle", C.c_int(gridID), C.c_int(v0), C.c_int(v1), C.c_int(v2))

    def close(self):
        if self._mg:
            getattr(lib, "%s_%s_destroy" % (self._prefix, self._sfx))(self._mg)
            self._mg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiGrid3D(_MGBase):
    """MultiGrid3D(finestGridSizeXYZ, range) of the reference (N3/MultiGrid3D.h:6-33) on one MI355X."""
    _prefix = "mgMultiGrid3D"

    def __init__(self, ctx, finestGridSizeXYZ, rng, dtype=np.float64, nlevels=0, residual_mode=REF_COMPAT, fuse=True,
                 layout="xsplit", coarsening="full", shift=0.0, coefficient=None, neumann=None, capacity=None, robin=None,
                 wall_flux=None, face_mean="arithmetic", pinned=None, pinned_values=None):
        """coarsening="semi": every level halves only the axes with the smallest spacing (semi_plan, mg_multigrid.h) -- the
        hierarchy for grids whose spacings differ; always x-split; nlevels caps its level count.
        shift = s >= 0: the hierarchy of (Laplacian - s) u = f (the `shift` property).
        coefficient = a > 0 at every point of the finest grid: the hierarchy of div(a grad u) - s u = f (set_coefficient).
        neumann = six truthy values (x-low, x-high, y-low, y-high, z-low, z-high): the faces with du/dn = 0 (set_neumann).
        capacity = c >= 0 at every point of the finest grid: the hierarchy of div(a grad u) - (s c) u = f (set_capacity; needs
        a coefficient).
        robin, wall_flux = six numbers each (the faces' order): beta >= 0 and g of the wall law a du/dn + beta u = g on the
        faces of `neumann` (set_wall).
        face_mean = "arithmetic" or "harmonic": the mean of the two nodes' coefficients a face carries (set_face_mean).
        pinned, pinned_values = a boolean mask over level 0 and the values of its true points: interior points whose value is data
        (set_pinned)."""
        mean = face_mean_mode(face_mean)
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self._sfx, self._ct = _ct(dtype)
        self._G, self._M = _grid3_struct(self._ct)
        self._mg = C.POINTER(self._M)()
        if coarsening not in ("full", "semi"):
            raise ValueError("coarsening must be 'full' or 'semi', not %r" % (coarsening,))
        lay = {"natural": 0, "xsplit": 1}[layout]
        if coarsening == "semi":
            if not lay:
                raise ValueError("a semi-coarsened hierarchy is always x-split: layout='natural' is not available")
            fn = getattr(lib, "mgMultiGrid3D_%s_create_semi" % self._sfx)
            check(fn(ctx._h, _ip(finestGridSizeXYZ), _rp(rng, self._ct), C.c_int(int(nlevels)), C.byref(self._mg)))
        else:
            fn = getattr(lib, "mgMultiGrid3D_%s_create_levels" % self._sfx)
            check(fn(ctx._h, _ip(finestGridSizeXYZ), _rp(rng, self._ct), C.c_int(lay), C.c_int(int(nlevels)), C.byref(self._mg)))
            if nlevels:
                self.numGrids = nlevels
        self._mg.contents.residual_mode = int(residual_mode)
        self._mg.contents.fuse = int(bool(fuse))
        if shift != 0:  # (a NaN too: rejected by the setter)
            try:
                self.shift = shift
            except Exception:
                self.close()
                raise
        if mean:
            try:
                self.set_face_mean(face_mean)
            except Exception:
                self.close()
                raise
        if coefficient is not None:
            try:
                self.set_coefficient(coefficient)
            except Exception:
                self.close()
                raise
        if neumann is not None:
            try:
                self.set_neumann(neumann)
            except Exception:
                self.close()
                raise
        if capacity is not None:
            try:
                self.set_capacity(capacity)
            except Exception:
                self.close()
                raise
        if robin is not None or wall_flux is not None:
            try:
                self.set_wall(robin, wall_flux)
            except Exception:
                self.close()
                raise
        if pinned is not None:
            try:
                self.set_pinned(pinned, pinned_values)
            except Exception:
                self.close()
                raise

    def set_pinned(self, mask, values=None):
        """mask: booleans over level 0 (reference layout), True at the interior points whose value is DATA: an electrode or a
        thermostat inside the volume, everything outside a body that is no box, a pressure pinned at one point.  values: their
        values, an array over level 0 read at the true points (None: zeros).  A pinned point is no unknown: v holds its value before
        and after every call, its neighbours read it as they read a Dirichlet face point, the smoother never changes it, the residual
        and every vector of PCG are exactly 0 there, and ResidualNorm and PCG's stopping rule sum over the remaining unknowns.  The
        operator on those is the old one with rows and columns struck out: still symmetric, in the weighted product too.  A coarse
        point is pinned when its coincident fine point is, or one of that point's two neighbours along an axis the step halves; the
        values go down by injection.  Works with every operator of the hierarchy (shift, coefficient with either face mean,
        capacity, walls), on full and semi-coarsened hierarchies, in cycles, PCG (every krylov), BackwardEuler and use_graph.  A True
        on the boundary of the box is refused (Dirichlet face points are data already; a wall unknown cannot be pinned).  Needs
        layout="xsplit", the red-black smoother and residual_mode=CORRECT; PCG(precond="f32") and Eigen are not available, nor is
        the closed box (all six faces walls, no shift, no robin > 0).  None or all False: no pins -- the hierarchy is then, launch for
        launch, one that never had any."""
        if mask is None:
            self._call("set_pinned", None, None)
            return
        shape = _shape(self.size(0))
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if mask.shape != shape:
            raise ValueError("the mask of the pinned nodes has shape %r, level 0 has %r" % (mask.shape, shape))
        vp = None
        if values is not None:
            values = np.ascontiguousarray(values, self.dtype)
            if values.shape != shape:
                raise ValueError("the values of the pinned nodes have shape %r, level 0 has %r" % (values.shape, shape))
            vp = values.ctypes.data_as(C.c_void_p)
        self._call("set_pinned", mask.ctypes.data_as(C.c_void_p), vp)

    def pinned(self, gridID=0):
        """the mask of level gridID's pinned points (booleans, reference layout)"""
        out = np.zeros(_shape(self.size(gridID)), np.uint8)
        self._call("get_pinned", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out.astype(bool)

    def pinned_count(self, gridID=0):
        out = C.c_size_t()
        self._call("pinned_count", C.c_int(gridID), C.byref(out))
        return int(out.value)

    def set_wall(self, robin=None, flux=None):
        """robin, flux: six numbers each, one per face in the order x-low, x-high, y-low, y-high, z-low, z-high (None: zeros):
        beta >= 0 and g of the wall law  a du/dn + beta u = g  (n outward) on the faces flagged by set_neumann, in the units of the
        hierarchy's operator div(a grad u) (a = 1 without a coefficient); beta = g = 0 is the insulated wall.  With BackwardEuler's
        kappa a physical  kappa a du/dn + B u = G  is beta = B / kappa, g = G / kappa -- nothing is rescaled here.  beta enters the
        operator of every level (a diagonal term 2 beta / h at the face unknowns, from the level's own spacing); g enters level 0's
        right-hand side: call add_wall_flux() once after upload_f (BackwardEuler does it for every step, solve3d_pcg for its
        rhs).  A beta > 0 makes the closed box regular: all six faces with shift = 0 are then accepted, and
        PCG(krylov="weighted") projects nothing.  A value other than 0 on a face that is not flagged is refused, and set_neumann
        refuses to clear a face that still carries one.  PCG(precond="f32") is not available with walls.  All zeros: the hierarchy
        is, launch for launch, one that never had a wall.  Data that vary along a face: subtract 2 g(P) / h from f at the face
        yourself (h the spacing along the face's axis)."""
        vals = []
        for name, x in (("robin", robin), ("flux", flux)):
            x = [0.0] * 6 if x is None else [float(t) for t in x]
            if len(x) != 6:
                raise ValueError("%s takes six values (x-low, x-high, y-low, y-high, z-low, z-high), not %d" % (name, len(x)))
            vals.append(x)
        self._call("set_wall", _rp(vals[0], self._ct), _rp(vals[1], self._ct))

    @property
    def wall(self):
        """(robin, flux) as set_wall takes them"""
        b, g = (self._ct * 6)(), (self._ct * 6)()
        self._call("get_wall", b, g)
        return tuple(float(x) for x in b), tuple(float(x) for x in g)

    def add_wall_flux(self):
        """f[0] -= 2 g / h at the unknowns on the faces with a flux g != 0 (mgx3dxs_wall_rhs): once per right-hand side"""
        self._call("add_wall_flux")

    def set_neumann(self, faces):
        """faces: six truthy values, one per face in the order x-low, x-high, y-low, y-high, z-low, z-high (None: all False).  A
        true one makes that face a wall with du/dn = 0 on every level: its points, but for those on a Dirichlet face too, become
        unknowns, and v there is part of the solution instead of data.  Needs layout="xsplit", the red-black smoother,
        residual_mode=CORRECT and coarsening="full"; PCG and BackwardEuler then take krylov=False or krylov="weighted" (CG in the
        inner product weighted by 1/2 per wall an unknown lies on; krylov=True is refused), PCG(precond="f32") is not available,
        and all six faces need a shift > 0 -- but for PCG(krylov="weighted"), which solves that singular system in the projected
        sense.  A prescribed flux or a convective wall: set_wall.  All False: the hierarchy is what it was without walls."""
        faces = [0] * 6 if faces is None else [int(bool(x)) for x in faces]
        if len(faces) != 6:
            raise ValueError("neumann takes six values (x-low, x-high, y-low, y-high, z-low, z-high), not %d" % len(faces))
        self._call("set_boundary", _ip(faces))

    @property
    def neumann(self):
        """the six faces' flags as set_neumann takes them"""
        return tuple(bool((self._mg.contents.bc >> k) & 1) for k in range(6))

    def set_coefficient(self, a):
        """a: the coefficient of div(a grad u) - shift u = f at ALL points of level 0 (reference layout, finite and > 0), restricted
        down the levels by the hierarchy's own transfers; every call then works with that operator (needs layout="xsplit", the
        red-black smoother and residual_mode=CORRECT; PCG(precond="f32") is not available).  None: back to the constant-coefficient
        operators.  New values replace the old ones in the same device arrays."""
        if a is None:
            self._call("set_coefficient", None)
            return
        a = np.ascontiguousarray(a, self.dtype)
        if a.shape != _shape(self.size(0)):
            raise ValueError("the coefficient has shape %r, level 0 has %r" % (a.shape, _shape(self.size(0))))
        self._call("set_coefficient", a.ctypes.data_as(C.c_void_p))

    @property
    def has_coefficient(self):
        return bool(self.grid(0).d_a)

    def download_coefficient(self, gridID=0):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_coefficient", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out

    def set_capacity(self, c):
        """c: the capacity of div(a grad u) - (shift c) u = f at ALL points of level 0 (reference layout, finite and >= 0), restricted
        down the levels as the coefficient is; every call then works with that operator, and BackwardEuler steps
        c u_t = kappa div(a grad u) + q.  Needs a coefficient (set_coefficient first; an array of ones serves);
        PCG(precond="f32") is not available.  None: back to the scalar shift.  New values replace the old ones in the same device
        arrays."""
        if c is None:
            self._call("set_capacity", None)
            return
        c = np.ascontiguousarray(c, self.dtype)
        if c.shape != _shape(self.size(0)):
            raise ValueError("the capacity has shape %r, level 0 has %r" % (c.shape, _shape(self.size(0))))
        self._call("set_capacity", c.ctypes.data_as(C.c_void_p))

    def set_face_mean(self, mean):
        """mean: "arithmetic" (the default) or "harmonic" -- the coefficient a face between two nodes carries: (aP + aQ) / 2, right
        where a material boundary lies on a node plane, or 2 aP aQ / (aP + aQ), the series conductance, right for node-valued
        materials (voxel data, a layer one node thick) whose boundary lies midway between two nodes.  It may be set before or after
        the coefficient and counts only while the hierarchy has one; every level is re-discretised with it, the coefficient goes
        down the levels as before, and every call (cycles, PCG, BackwardEuler, walls, capacity, use_graph) works with it.  The
        harmonic mean needs every a * a to be a normal, finite number of the hierarchy's precision: a coefficient outside that range
        is refused here and by set_coefficient.  Anything else raises ValueError."""
        self._call("set_face_mean", C.c_int(face_mean_mode(mean)))

    @property
    def face_mean(self):
        return "harmonic" if self._mg.contents.face_mean == FACE_MEANS["harmonic"] else "arithmetic"

    @property
    def has_capacity(self):
        return bool(self._mg.contents.cap)

    def download_capacity(self, gridID=0):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_capacity", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out

    @property
    def shift(self):
        """s >= 0 of the operator (Laplacian - s) u = f every call of the hierarchy works with (0: the Poisson problem).  A non-zero
        shift needs layout="xsplit", the red-black smoother and residual_mode=CORRECT; PCG(precond="f32") is not available."""
        return float(self._mg.contents.shift)

    @shift.setter
    def shift(self, s):
        self._call("set_shift", self._ct(s))

    def BackwardEuler(self, nsteps, dt, kappa, source=None, v1=2, v2=2, tol=1e-10, maxit=100, krylov=True):
        """nsteps implicit steps of u_t = kappa Laplacian(u) + q on level 0: v[0] holds u (its boundary = the Dirichlet data, fixed
        in time), source = q (reference layout) or None.  Every step is one PCG(v1, v2, tol, maxit, krylov) solve of
        (Laplacian - s) u' = -s u - q / kappa with s = 1 / (kappa dt), which stays set as the hierarchy's shift afterwards.
        Returns (iterations of all steps, worst true relative residual of a step, converged); it stops at the first step
        that does not converge.  krylov as in PCG: with walls False or "weighted"."""
        src = None
        if source is not None:
            source = np.ascontiguousarray(source, self.dtype)
            assert source.shape == _shape(self.size(0))
            src = self.ctx.to_device(xs_pack(source) if self._mg.contents.layout else source)
        it, conv = C.c_int(), C.c_int()
        worst = C.c_double()
        try:
            self._call("BackwardEuler", C.c_int(int(nsteps)), C.c_double(dt), C.c_double(kappa), src, C.c_int(v1), C.c_int(v2),
                       C.c_double(tol), C.c_int(maxit), C.c_int(krylov_mode(krylov)), C.byref(it), C.byref(worst), C.byref(conv))
        finally:
            if src is not None:
                self.ctx.free(src)
        return int(it.value), float(worst.value), bool(conv.value)

    def grid(self, gridID):
        return self._mg.contents.grids3D[gridID].contents

    def size(self, gridID):
        return tuple(self.grid(gridID).sizeXYZ)

    @property
    def masks(self):
        """the axes halved between level l and l + 1 (bit 0 = x, 1 = y, 2 = z), one entry per level, 0 for the last"""
        k = self.maxGrids
        return tuple(int(self._mg.contents.coarsen[l]) if l + 1 < k else 0 for l in range(k))

    def Relax(self, gridID, ncycles):
        self._call("Relax", self._mg.contents.grids3D[gridID], C.c_int(ncycles))

    def CalculateResidual(self, gridID):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_residual", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out

    def ResidualNorm(self, gridID=0):
        out = C.c_double()
        self._call("ResidualNorm", C.c_int(gridID), C.byref(out))
        return float(out.value)

    def InitF(self, gridID):
        self._call("InitF", C.c_int(gridID))

    def DiffStats(self, gridID=0):
        """(mean |diff|, max |diff|, relative L2) of diff = analytic - v  (Grid3D::PrintDiff as numbers)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._call("DiffStats", C.c_int(gridID), C.byref(a), C.byref(b), C.byref(c))
        return float(a.value), float(b.value), float(c.value)

    def setToValue_v(self, gridID, value, modifyBoundaries):
        g = self.grid(gridID)
        self._call("setToValue", C.c_void_p(g.d_v), _ip(g.sizeXYZ), self._ct(value), C.c_int(int(modifyBoundaries)))

    def interpolate_correct(self, gridID):
        """v[gridID] += Interpolate(v[gridID+1]) on the interior (the fused VCycle step)."""
        g0, g1 = self.grid(gridID), self.grid(gridID + 1)
        pfx = "mgx3dxs_" if self._mg.contents.layout else "mgx3d_"
        check(getattr(lib, pfx + "interpolate_correct_" + self._sfx)(self.ctx._h, C.c_void_p(g0.d_v), _ip(g0.sizeXYZ),
                                                                     C.c_void_p(g1.d_v), _ip(g1.sizeXYZ)))

    def upload_v(self, gridID, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.size == _count(self.size(gridID))
        self._call("upload_v", C.c_int(gridID), arr.ctypes.data_as(C.c_void_p))

    def upload_f(self, gridID, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.size == _count(self.size(gridID))
        self._call("upload_f", C.c_int(gridID), arr.ctypes.data_as(C.c_void_p))

    def download_v(self, gridID=0):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_v", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out

    def download_f(self, gridID=0):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_f", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out

    def PCG(self, v1=2, v2=2, tol=1e-10, maxit=100, krylov=True, precond="f64"):
        """Solve on level 0 to a relative residual < tol from the guess in v[0] (its boundary = the Dirichlet data): flexible CG
        preconditioned by one V(v1, v2) cycle from zero per iteration, or plain V-cycles with krylov=False.  Needs the x-split
        layout and residual_mode=CORRECT.  Returns (iters, rel_res, converged, history): rel_res is the TRUE relative
        residual of the result, history one relative residual per iteration.

        fp32 cannot reach tolerances much below 1e-6 and fp64 cycles stream twice the bytes: an fp64 hierarchy with
        precond="f32" (mgMultiGrid3D_f64_PCG_mixed) keeps the iterate, the residual and the stopping test in fp64 and runs
        the V-cycle in fp32 on a twin hierarchy it builds on first use -- fp64 tolerances in close to fp32 time, for the
        twin's extra device memory (four fp32 arrays per level).  With krylov=False that is defect correction, whose
        history holds true residuals.

        krylov="weighted" (or 2): flexible CG in the inner product that weights an unknown by 1/2 per wall (set_neumann) it lies
        on, in which the operator with walls is symmetric -- the Krylov solver of a hierarchy with walls, where krylov=True is
        refused; without walls it is krylov=True bit for bit.  With all six faces walls and shift 0 it solves the singular system
        in the projected sense: A v = f - mean_W(f), v keeps the weighted mean of the guess, rel_res is against the projected
        right-hand side and pcg_removed_mean is mean_W(f)."""
        if precond not in ("f64", "f32"):
            raise ValueError("precond must be 'f64' or 'f32', not %r" % (precond,))
        if precond == "f32" and self.dtype != np.float64:
            raise ValueError("precond='f32' needs an fp64 hierarchy (the fp32 one already runs its V-cycle in fp32)")
        it, conv = C.c_int(), C.c_int()
        rel = C.c_double()
        hist = np.zeros(int(maxit), np.float64)
        mode = krylov_mode(krylov)
        self._call("PCG_mixed" if precond == "f32" else "PCG", C.c_int(v1), C.c_int(v2), C.c_double(tol), C.c_int(maxit),
                   C.c_int(min(mode, 1) if precond == "f32" else mode), C.byref(it), C.byref(rel), C.byref(conv), hist.ctypes.data_as(C.c_void_p),
                   C.c_int(len(hist)))
        return int(it.value), float(rel.value), bool(conv.value), hist[:it.value].copy()

    def Eigen(self, k, tol=1e-8, maxit=200, v1=2, v2=2, vectors=True, guess=None):
        """The k smallest eigenvalues and eigenvectors of the hierarchy's operator (mgMultiGrid3D_f64_Eigen):
        -(div(a grad x)) [+ the walls' diagonal] = lambda c x on the unknowns, by LOBPCG with block size k (1 .. 8), one
        V(v1, v2) cycle from zero per residual as the preconditioner.  The shift of the hierarchy is a spectral shift only
        (lambda does not depend on it), so a closed insulated box, whose lowest eigenvalue is 0, is solved with any shift > 0.
        fp64 hierarchies, x-split layout, residual_mode=CORRECT.

        Returns (lam, X, info): lam ascending; X of shape (k, nz, ny, nx) with <x_i, c x_j>_W = delta_ij (sign unspecified), or
        None with vectors=False; info = {"iterations", "residuals", "converged"}, the residuals being
        ||A_s x + mu c x||_W / (mu ||x||_W) with mu = lambda + shift, each below tol when converged.  guess: k start vectors of
        that shape (read at the unknowns only); the default start is pseudo-random and the same on every call.  v[0] and f[0]
        are left as they were."""
        if self.dtype != np.float64:
            raise ValueError("Eigen needs an fp64 hierarchy (the eigensolver is fp64 only), not %s" % self.dtype)
        k = int(k)
        kk = max(1, min(k, 8))
        shape = _shape(self.size(0))
        gp = None
        if guess is not None:
            guess = np.ascontiguousarray(guess, np.float64)
            if guess.shape != (k,) + shape:
                raise ValueError("guess must have the shape %r, not %r" % ((k,) + shape, guess.shape))
            gp = guess.ctypes.data_as(C.c_void_p)
        lam, res = np.zeros(kk, np.float64), np.zeros(kk, np.float64)
        X = np.zeros((kk,) + shape, np.float64) if vectors else None
        it, conv = C.c_int(), C.c_int()
        self._call("Eigen", C.c_int(k), C.c_int(v1), C.c_int(v2), C.c_double(tol), C.c_int(maxit), lam.ctypes.data_as(C.c_void_p),
                   res.ctypes.data_as(C.c_void_p), C.byref(it), C.byref(conv), X.ctypes.data_as(C.c_void_p) if vectors else None, gp)
        return lam, X, {"iterations": int(it.value), "residuals": res, "converged": bool(conv.value)}

    @property
    def pcg_removed_mean(self):
        """the weighted mean the last PCG removed from the right-hand side: mean_W(f) after PCG(krylov="weighted") in a closed box
        without a shift, 0 after every other solve"""
        out = C.c_double()
        self._call("pcg_removed_mean", C.byref(out))
        return float(out.value)


class MultiGrid2D(_MGBase):
    """MultiGrid2D(finestGridSizeXY, range, A, A_size, alfa) (N2/MultiGrid2D.h:6-37) on one MI355X."""
    _prefix = "mgMultiGrid2D"

    def __init__(self, ctx, finestGridSizeXY, rng, A, alfa, dtype=np.float64, nlevels=0, fuse=True):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self._sfx, self._ct = _ct(dtype)
        self._G, self._M = _grid2_struct(self._ct)
        self._mg = C.POINTER(self._M)()
        fn = getattr(lib, "mgMultiGrid2D_%s_create" % self._sfx)
        check(fn(ctx._h, _ip(finestGridSizeXY), _rp(rng, self._ct), _rp(A, self._ct), C.c_int(2), C.c_int(alfa),
                 C.byref(self._mg)))
        # fuse: True = the library default (2: cache-resident cycle kernels), 1 = fused operators only, False / 0 = one
        # launch per reference call
        self._mg.contents.fuse = 2 if fuse is True else int(fuse)
        if nlevels:
            self.numGrids = nlevels

    def grid(self, gridID):
        return self._mg.contents.grids2D[gridID].contents

    def MeanAbsoluteError(self, gridID=0):
        out = C.c_double()
        self._call("MeanAbsoluteError", C.c_int(gridID), C.byref(out))
        return float(out.value)

    def size(self, gridID):
        return tuple(self.grid(gridID).sizeXY)

    def Relax(self, gridID, ncycles):
        self._call("Relax", self._mg.contents.grids2D[gridID], C.c_int(ncycles))

    def upload_v(self, gridID, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.size == _count(self.size(gridID))
        self._call("upload_v", C.c_int(gridID), arr.ctypes.data_as(C.c_void_p))

    def upload_f(self, gridID, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.size == _count(self.size(gridID))
        self._call("upload_f", C.c_int(gridID), arr.ctypes.data_as(C.c_void_p))

    def download_v(self, gridID=0):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_v", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out

    def download_f(self, gridID=0):
        out = np.empty(_shape(self.size(gridID)), self.dtype)
        self._call("download_f", C.c_int(gridID), out.ctypes.data_as(C.c_void_p))
        return out


class MultiGrid1D(_MGBase):
    """MultiGrid1D(finestGridSize, range) (N1/MultiGrid1D.h:6-31): host-only C (BASELINE configs[0])."""
    _prefix = "mgMultiGrid1D"

    def __init__(self, finestGridSize, rng, dtype=np.float32, nlevels=0):
        self.dtype = np.dtype(dtype)
        self._sfx, self._ct = _ct(dtype)
        self._G, self._M = _grid1_struct(self._ct)
        self._mg = C.POINTER(self._M)()
        fn = getattr(lib, "mgMultiGrid1D_%s_create" % self._sfx)
        check(fn(C.c_int(finestGridSize), _rp(rng, self._ct), C.byref(self._mg)))
        if nlevels:
            self.numGrids = nlevels

    def grid(self, gridID):
        return self._mg.contents.grids1D[gridID].contents

    def _view(self, ptr, n):
        return np.ctypeslib.as_array(ptr, shape=(n,))

    def v(self, gridID=0):
        g = self.grid(gridID)
        return self._view(g.h_v, g.sizeX)

    def f(self, gridID=0):
        g = self.grid(gridID)
        return self._view(g.h_f, g.sizeX)

    def Relax(self, gridID, ncycles):
        self._call("Relax", self._mg.contents.grids1D[gridID], C.c_int(ncycles))

    def CalculateResidual(self, gridID):
        g = self.grid(gridID)
        r = np.empty(g.sizeX, self.dtype)
        self._call("CalculateResidual", self._mg.contents.grids1D[gridID], r.ctypes.data_as(C.c_void_p))
        return r

    def Restrict(self, fine):
        fine = np.ascontiguousarray(fine, self.dtype)
        coarse = np.empty((fine.size - 1) // 2 + 1, self.dtype)
        self._call("Restrict", fine.ctypes.data_as(C.c_void_p), C.c_int(fine.size), coarse.ctypes.data_as(C.c_void_p),
                   C.c_int(coarse.size))
        return coarse

    def Interpolate(self, fine, coarse):
        fine = np.ascontiguousarray(fine, self.dtype).copy()
        coarse = np.ascontiguousarray(coarse, self.dtype)
        self._call("Interpolate", fine.ctypes.data_as(C.c_void_p), C.c_int(fine.size), coarse.ctypes.data_as(C.c_void_p),
                   C.c_int(coarse.size))
        return fine

    def ApplyCorrection(self, fine, err):
        fine = np.ascontiguousarray(fine, self.dtype).copy()
        err = np.ascontiguousarray(err, self.dtype)
        self._call("ApplyCorrection", fine.ctypes.data_as(C.c_void_p), C.c_int(fine.size), err.ctypes.data_as(C.c_void_p),
                   C.c_int(err.size))
        return fine

    def setToValue(self, grid, value, modifyBoundaries):
        grid = np.ascontiguousarray(grid, self.dtype).copy()
        self._call("setToValue", grid.ctypes.data_as(C.c_void_p), C.c_int(grid.size), self._ct(value),
                   C.c_int(int(modifyBoundaries)))
        return grid


# --------------------------------------------------------------------------- z-slab decomposition
class SlabPlan(C.Structure):
    _fields_ = [("zlo", C.c_int), ("zhi", C.c_int), ("glo", C.c_int), ("ghi", C.c_int), ("zoff", C.c_int), ("nzl", C.c_int),
                ("ubeg", C.c_int), ("uend", C.c_int)]


class SemiPlan(C.Structure):
    _fields_ = [("nlevels", C.c_int), ("n", (C.c_int * 3) * 32), ("mask", C.c_ubyte * 32)]


def semi_plan(n3, rng, max_levels=0):
    """mg_semi_plan: (sizes, masks) of the semi-coarsened hierarchy of an n3 = (sx, sy, sz) grid on rng -- one (sx, sy, sz) and
    one mask (bit 0 = x, 1 = y, 2 = z: the axes halved on the way to the next level; 0 for the last) per level"""
    p = SemiPlan()
    check(lib.mg_semi_plan(_ip(n3), _rp(rng, C.c_double), C.c_int(int(max_levels)), C.byref(p)))
    return [tuple(p.n[l]) for l in range(p.nlevels)], tuple(int(p.mask[l]) for l in range(p.nlevels))


def dist_num_levels(sizeZ, nranks, numGrids, min_planes=4):
    return lib.mg_dist_num_levels(int(sizeZ), int(nranks), int(numGrids), int(min_planes))


def slab_plan(sizeZ, rank, nranks):
    p = SlabPlan()
    check(lib.mg_slab_plan(int(sizeZ), int(rank), int(nranks), C.byref(p)))
    return p


class LocalGroup:
    """In-process test transport: `nranks` host threads, one Context each, same device (mgx_comm_init_local)."""

    def __init__(self, nranks):
        self._g = C.c_void_p()
        check(lib.mgx_local_group_create(int(nranks), C.byref(self._g)))
        self.nranks = nranks

    def attach(self, ctx, rank):
        check(lib.mgx_comm_init_local(ctx._h, self._g, int(rank)))

    def set_test_hooks(self, delay_us=0, drop_waits=False):
        """delay_us: every transfer starts that late on the receiving comm stream; drop_waits: mgx_comm_wait becomes a
        no-op (fault injection -- results must then be WRONG, which is what the negative test checks)"""
        check(lib.mgx_local_group_set_test_hooks(self._g, int(delay_us), int(bool(drop_waits))))

    def close(self):
        if self._g:
            lib.mgx_local_group_destroy(self._g)
            self._g = C.c_void_p()


def _dist_struct(ct):
    class Slab3D(C.Structure):
        _fields_ = [("d_v", C.c_void_p), ("d_f", C.c_void_p), ("sizeXYZ", C.c_int * 3), ("plan", SlabPlan), ("h_x", ct),
                    ("h_y", ct), ("h_z", ct), ("x_a", ct), ("y_a", ct), ("z_a", ct), ("level", C.c_int)]

    class DistMultiGrid3D(C.Structure):
        _fields_ = [("slabs", C.POINTER(C.POINTER(Slab3D))), ("numDist", C.c_int), ("numGrids", C.c_int), ("maxGrids", C.c_int),
                    ("tail", C.c_void_p), ("ctx", C.c_void_p), ("rank", C.c_int), ("nranks", C.c_int),
                    ("residual_mode", C.c_int), ("d_share", C.c_void_p), ("d_bplane", C.c_void_p), ("d_norm", C.c_void_p),
                    ("norm_count", C.c_int), ("inline_bytes", C.c_longlong), ("v_rim_zero", C.c_ubyte * 32),
                    ("use_graph", C.c_int), ("graph_exec", C.c_void_p), ("graph_key", C.c_longlong), ("graph_warm", C.c_int),
                    ("pack_halos", C.c_int), ("d_stage", C.c_void_p), ("stage_half", C.c_size_t),
                    ("ca_min_planes", C.c_int), ("gv", C.c_byte * 32), ("gf", C.c_byte * 32), ("comm_pending", C.c_int),
                    ("n_exchanges", C.c_longlong), ("graph_rec", GraphRec), ("graph_post", GraphFlags)]

    return Slab3D, DistMultiGrid3D


class DistMultiGrid3D(_MGBase):
    """One rank's part of a z-slab decomposed 3D hierarchy (include/mg_multigrid.h, mgDistMultiGrid3D_<r>).
    The context must already carry a communicator (Context.comm_init for RCCL, LocalGroup.attach for the
    in-process test transport) unless it runs alone."""
    _prefix = "mgDistMultiGrid3D"

    def __init__(self, ctx, finestGridSizeXYZ, rng, dtype=np.float64, nlevels=0, residual_mode=REF_COMPAT, min_planes=4,
                 inline_bytes=None, use_graph=False, pack_halos=None, ca_min_planes=None):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self._sfx, self._ct = _ct(dtype)
        self._S, self._M = _dist_struct(self._ct)
        self._mg = C.POINTER(self._M)()
        self.n = tuple(int(k) for k in finestGridSizeXYZ)
        fn = getattr(lib, "mgDistMultiGrid3D_%s_create" % self._sfx)
        check(fn(ctx._h, _ip(finestGridSizeXYZ), _rp(rng, self._ct), C.c_int(min_planes), C.byref(self._mg)))
        if nlevels:
            self.numGrids = nlevels
        self._mg.contents.residual_mode = int(residual_mode)
        if inline_bytes is not None:  # None: the library default (mg_multigrid.h); 0: every level overlapped
            self._mg.contents.inline_bytes = int(inline_bytes)
        self._mg.contents.use_graph = int(bool(use_graph))  # opt-in: VCycle(0, ...) captured (RCCL calls included) and replayed
        if pack_halos is not None:  # None: the library default (0 = whole planes)
            self._mg.contents.pack_halos = int(bool(pack_halos))
        if ca_min_planes is not None:  # None: the library default (16); 0: one exchange per colour pass on every level
            self._mg.contents.ca_min_planes = int(ca_min_planes)

    @property
    def n_exchanges(self):
        """halo exchanges + collectives this rank has enqueued since the hierarchy was created"""
        return int(self._mg.contents.n_exchanges)

    @property
    def inline_bytes(self):
        return self._mg.contents.inline_bytes

    @property
    def numDist(self):
        return self._mg.contents.numDist

    @property
    def rank(self):
        return self._mg.contents.rank

    @property
    def nranks(self):
        return self._mg.contents.nranks

    def plan(self, gridID=0):
        return self._mg.contents.slabs[gridID].contents.plan

    def Relax(self, gridID, ncycles):
        self._call("Relax", C.c_int(gridID), C.c_int(ncycles))

    def zero_v(self, gridID=0):
        self._call("zero_v", C.c_int(gridID))

    def ResidualNorm(self, gridID=0):
        """l2 norm of the residual over the whole grid (slab sums + all-reduce); the same value on every rank"""
        out = C.c_double()
        self._call("ResidualNorm", C.c_int(gridID), C.byref(out))
        return float(out.value)

    def ResidualNormRecord(self, gridID=0):
        self._call("ResidualNormRecord", C.c_int(gridID))

    def ResidualNormHistory(self):
        buf = (C.c_double * 255)()
        n = C.c_int()
        self._call("ResidualNormHistory", buf, C.c_int(255), C.byref(n))
        return [float(buf[i]) for i in range(n.value)]

    def slab(self, gridID=0):
        return self._mg.contents.slabs[gridID].contents

    def relax_colour_local(self, gridID, colour):
        """one colour pass on this rank's slab WITHOUT the ghost exchange (kernel timing only)"""
        g = self.slab(gridID)
        p = g.plan
        h = (self._ct * 3)(g.h_x, g.h_y, g.h_z)
        check(getattr(lib, "mgx3dxs_relax_colour_slab_" + self._sfx)(self.ctx._h, C.c_void_p(g.d_v), C.c_void_p(g.d_f),
                                                                      C.c_int(g.sizeXYZ[0]), C.c_int(g.sizeXYZ[1]), h,
                                                                      C.c_int(colour), C.c_int(p.ubeg - p.zoff),
                                                                      C.c_int(p.uend - p.zoff), C.c_int(p.zoff)))

    def upload_v(self, gridID, full):
        full = np.ascontiguousarray(full, self.dtype)
        self._call("upload_v", C.c_int(gridID), full.ctypes.data_as(C.c_void_p))

    def upload_f(self, gridID, full):
        full = np.ascontiguousarray(full, self.dtype)
        self._call("upload_f", C.c_int(gridID), full.ctypes.data_as(C.c_void_p))

    def download_owned(self, gridID=0):
        """this rank's owned planes [plan.zlo, plan.zhi) of level gridID as an array of its own (reference layout)"""
        p = self.plan(gridID)
        g = self.slab(gridID)
        sx, sy = g.sizeXYZ[0], g.sizeXYZ[1]
        out = np.empty((p.zhi - p.zlo, sy, sx), self.dtype)
        # the C entry addresses planes of a whole-grid host array: hand it the address plane 0 would have
        base = out.ctypes.data - p.zlo * sx * sy * self.dtype.itemsize
        self._call("download_v", C.c_int(gridID), C.c_void_p(base))
        return out

    def download_v_into(self, gridID, full):
        """writes this rank's owned planes into `full` (a whole-grid array in the reference layout)"""
        assert full.dtype == self.dtype and full.flags.c_contiguous
        self._call("download_v", C.c_int(gridID), full.ctypes.data_as(C.c_void_p))


# --------------------------------------------------------------------------- solve(grid, rhs, nlevels)
def solve3d(ctx, grid, rhs, rng, nlevels=0, fmg=False, v0=1, v1=2, v2=2, ncycles=1, residual_mode=REF_COMPAT):
    grid = np.ascontiguousarray(grid).copy()
    s, ct = _ct(grid.dtype)
    rhs = np.ascontiguousarray(rhs, grid.dtype)
    n = tuple(reversed(grid.shape))
    check(getattr(lib, "mg3d_solve_" + s)(ctx._h, grid.ctypes.data_as(C.c_void_p), rhs.ctypes.data_as(C.c_void_p), _ip(n),
                                          _rp(rng, ct), C.c_int(nlevels), C.c_int(int(fmg)), C.c_int(v0), C.c_int(v1),
                                          C.c_int(v2), C.c_int(ncycles), C.c_int(residual_mode)))
    return grid


def solve3d_from_zero(ctx, n, rng, dtype=np.float64, rhs=None, nlevels=0, fmg=False, v0=1, v1=2, v2=2, ncycles=1,
                      residual_mode=REF_COMPAT):
    """mg3d_solve_from_zero: the guess is the reference's InitV state (zeros, nothing uploaded); rhs=None: the reference's
    own right-hand side, built on the device -- then the only transfer of the call is the result"""
    s, ct = _ct(dtype)
    out = np.empty(_shape(n), dtype)
    r = np.ascontiguousarray(rhs, dtype).ctypes.data_as(C.c_void_p) if rhs is not None else None
    check(getattr(lib, "mg3d_solve_from_zero_" + s)(ctx._h, out.ctypes.data_as(C.c_void_p), r, _ip(n), _rp(rng, ct), C.c_int(nlevels),
                                                    C.c_int(int(fmg)), C.c_int(v0), C.c_int(v1), C.c_int(v2), C.c_int(ncycles),
                                                    C.c_int(residual_mode)))
    return out


def solve3d_pcg(ctx, grid, rhs, rng, nlevels=0, v1=2, v2=2, tol=1e-10, maxit=100, krylov=True, precond="f64", coarsening="full",
                shift=0.0, coefficient=None, neumann=None, capacity=None, robin=None, wall_flux=None, face_mean="arithmetic",
                pinned=None, pinned_values=None):
    """mg3d_solve_pcg: grid = guess with its Dirichlet boundary; returns (solution, iters, rel_res, converged).
    precond="f32" (fp64 grids only): mg3d_solve_pcg_mixed, the V-cycle in fp32 (MultiGrid3D.PCG).
    coarsening="semi": the same solve on a semi-coarsened hierarchy (MultiGrid3D(coarsening="semi")) built here for the call.
    shift = s > 0: the solve of (Laplacian - s) u = rhs (MultiGrid3D(shift=s)), on a hierarchy built here likewise.
    coefficient = a > 0 at every point: the solve of div(a grad u) - shift u = rhs (MultiGrid3D(coefficient=a)), likewise.
    neumann = six truthy values: the faces with du/dn = 0 (MultiGrid3D(neumann=...)), likewise; needs krylov=False or
    krylov="weighted" (MultiGrid3D.PCG).
    capacity = c >= 0 at every point, with a coefficient: the solve of div(a grad u) - (shift c) u = rhs, likewise.
    robin, wall_flux = six numbers each: the walls' beta and g (MultiGrid3D.set_wall); the flux is folded into rhs here.
    face_mean = "arithmetic" or "harmonic": the face coefficients of a solve with a coefficient (MultiGrid3D.set_face_mean).
    pinned, pinned_values = the mask and the values of interior points whose value is data (MultiGrid3D.set_pinned); the solution
    holds the values there."""
    face_mean_mode(face_mean)
    grid = np.ascontiguousarray(grid).copy()
    s, ct = _ct(grid.dtype)
    if precond not in ("f64", "f32"):
        raise ValueError("precond must be 'f64' or 'f32', not %r" % (precond,))
    if precond == "f32" and s != "f64":
        raise ValueError("precond='f32' needs an fp64 grid")
    if coarsening not in ("full", "semi"):
        raise ValueError("coarsening must be 'full' or 'semi', not %r" % (coarsening,))
    if coarsening == "semi" or shift != 0 or coefficient is not None or capacity is not None or (neumann is not None and any(neumann)) or \
            robin is not None or wall_flux is not None or pinned is not None:
        mg = MultiGrid3D(ctx, tuple(reversed(grid.shape)), rng, grid.dtype, nlevels=nlevels, residual_mode=CORRECT, coarsening=coarsening,
                         shift=shift, coefficient=coefficient, neumann=neumann, capacity=capacity, robin=robin, wall_flux=wall_flux,
                         face_mean=face_mean, pinned=pinned, pinned_values=pinned_values)
        try:
            mg.upload_v(0, grid)
            if rhs is not None:
                mg.upload_f(0, rhs)
            mg.add_wall_flux()
            it, rel, conv, _ = mg.PCG(v1, v2, tol, maxit, krylov, precond)
            return mg.download_v(0), it, rel, conv
        finally:
            mg.close()
    if precond == "f32":
        s = "mixed_f64"
    r = np.ascontiguousarray(rhs, grid.dtype).ctypes.data_as(C.c_void_p) if rhs is not None else None
    n = tuple(reversed(grid.shape))
    it, conv = C.c_int(), C.c_int()
    rel = C.c_double()
    check(getattr(lib, "mg3d_solve_pcg_" + s)(ctx._h, grid.ctypes.data_as(C.c_void_p), r, _ip(n), _rp(rng, ct), C.c_int(nlevels),
                                              C.c_int(v1), C.c_int(v2), C.c_double(tol), C.c_int(maxit),
                                              C.c_int(min(krylov_mode(krylov), 1) if precond == "f32" else krylov_mode(krylov)), C.byref(it),
                                              C.byref(rel), C.byref(conv)))
    return grid, int(it.value), float(rel.value), bool(conv.value)


def solve2d(ctx, grid, rhs, rng, A, alfa, nlevels=0, fmg=False, v0=1, v1=2, v2=2, ncycles=1):
    grid = np.ascontiguousarray(grid).copy()
    s, ct = _ct(grid.dtype)
    rhs = np.ascontiguousarray(rhs, grid.dtype)
    n = tuple(reversed(grid.shape))
    check(getattr(lib, "mg2d_solve_" + s)(ctx._h, grid.ctypes.data_as(C.c_void_p), rhs.ctypes.data_as(C.c_void_p), _ip(n),
                                          _rp(rng, ct), _rp(A, ct), C.c_int(alfa), C.c_int(nlevels), C.c_int(int(fmg)),
                                          C.c_int(v0), C.c_int(v1), C.c_int(v2), C.c_int(ncycles)))
    return grid


def solve1d(grid, rhs, rng, nlevels=0, fmg=False, v0=1, v1=2, v2=2, ncycles=1):
    grid = np.ascontiguousarray(grid).copy()
    s, ct = _ct(grid.dtype)
    rhs = np.ascontiguousarray(rhs, grid.dtype)
    check(getattr(lib, "mg1d_solve_" + s)(grid.ctypes.data_as(C.c_void_p), rhs.ctypes.data_as(C.c_void_p),
                                          C.c_int(grid.size), _rp(rng, ct), C.c_int(nlevels), C.c_int(int(fmg)),
                                          C.c_int(v0), C.c_int(v1), C.c_int(v2), C.c_int(ncycles)))
    return grid
