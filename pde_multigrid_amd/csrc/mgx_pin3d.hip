// mgx_pin3d.hip -- PINNED interior nodes, x-split layout.  DESIGN.md section 22.
//
// A pinned point is an interior point whose value is data: its neighbours read it as they read a Dirichlet face point, the
// smoother never keeps an update of it, and the residual, A p and every CG vector are exactly 0 there.  The tuned interior
// kernels run unchanged (they do update a pinned point, with a value nobody may read); every operation that has to respect the
// pins is the existing entry followed by a short launch over the LIST of pinned points that puts the data -- the values, or
// zeros -- back.  The pattern is the face unknowns' (mgx_rim3d.hip): tuned interior launch, then a list launch.
//
// The list: 32-bit storage offsets into the x-split array (a level whose storage does not fit 32 bits is MGX_ERR_SIZE), the red
// points ((x + y + z) even) first, then the black ones, each colour sorted by offset; end[0] = the number of red points, end[1] =
// the number of all.  A launch covers a range [first, first + count) of it: one colour (what a colour pass of the smoother
// overwrote) or both.  One thread per listed point, 256 threads, grid-stride, at most RIM_MAX_BLOCKS blocks; plain vector stores,
// nothing else.  Neighbouring list entries are neighbouring (or near) storage positions: the stores of a wave fall into few lines.
//
// This file is the kernel's one home: the drivers of mgx_rim3d.hpp reach it through pin_put_launch.
#include "mgx_rim3d.hpp"

namespace mgx {

// v[idx[t]] = val ? val[t] : 0 for t in [first, first + count)
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) pin_put3d_xs_kernel(real* __restrict__ v, const unsigned* __restrict__ idx,
                                                                   const real* __restrict__ val, unsigned first, unsigned count) {
    for (u64 t = (u64)blockIdx.x * RIM_THREADS + threadIdx.x; t < count; t += (u64)gridDim.x * RIM_THREADS) {
        const size_t k = (size_t)first + (size_t)t;
        v[idx[k]] = val ? val[k] : (real)0;
    }
}

template <class real>
void pin_put_launch(mgx_ctx* ctx, real* v, const unsigned* idx, const real* val, unsigned first, unsigned count) {
    if (!count) return;
    const u64 b = ((u64)count + RIM_THREADS - 1) / RIM_THREADS;
    MGX_LAUNCH((pin_put3d_xs_kernel<real>), dim3((unsigned)(b > RIM_MAX_BLOCKS ? RIM_MAX_BLOCKS : b)), dim3(RIM_THREADS), 0, ctx->compute, v,
               idx, val, first, count);
}
template void pin_put_launch<float>(mgx_ctx*, float*, const unsigned*, const float*, unsigned, unsigned);
template void pin_put_launch<double>(mgx_ctx*, double*, const unsigned*, const double*, unsigned, unsigned);

template <class real>
static int pin_put3d(mgx_ctx* ctx, real* v, const unsigned* idx, const real* val, unsigned first, unsigned count) {
    MGX_REQUIRE(ctx && v && (idx || !count), MGX_ERR_INVALID, "pin_put: NULL argument");
    MGX_REQUIRE((u64)first + count <= 0xffffffffull, MGX_ERR_INVALID, "pin_put: the range %u + %u does not fit 32 bits", first, count);
    if (!count) return MGX_OK;
    MGX_USE(ctx);
    pin_put_launch<real>(ctx, v, idx, val, first, count);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// the list of a mask in the reference layout (host arrays): idx == NULL counts only.  A true entry on the boundary is refused,
// naming the first one.  With values (reference layout, all points) and val: val[t] = the value of the list's point t.
template <class real>
static int pin_list3d(const int n[3], const unsigned char* mask, const real* values, unsigned* idx, real* val, unsigned end[2]) {
    MGX_REQUIRE(n && mask && end && (idx || !val), MGX_ERR_INVALID, "pin_list: NULL argument");
    for (int d = 0; d < 3; d++) MGX_REQUIRE(valid_size(n[d]), MGX_ERR_SIZE, "pin_list: size[%d] = %d is not odd and >= 3", d, n[d]);
    const Geo<XSplit, real> g(n[0], n[1]);
    MGX_REQUIRE((u64)g.PL * (u64)n[2] <= 0xffffffffull, MGX_ERR_SIZE, "pin_list: %llu storage positions do not fit 32-bit offsets",
                (u64)g.PL * (u64)n[2]);
    const int sx = n[0], sy = n[1], sz = n[2];
    u64 cnt[2] = {0, 0};
    for (int z = 0; z < sz; z++)
        for (int y = 0; y < sy; y++)
            for (int x = 0; x < sx; x++) {
                if (!mask[((size_t)z * sy + y) * sx + x]) continue;
                MGX_REQUIRE(x > 0 && x < sx - 1 && y > 0 && y < sy - 1 && z > 0 && z < sz - 1, MGX_ERR_INVALID,
                            "pin_list: the point (%d, %d, %d) lies on the boundary of the box: only interior points can be pinned", x, y, z);
                cnt[(x + y + z) & 1]++;
            }
    end[0] = (unsigned)cnt[0], end[1] = (unsigned)(cnt[0] + cnt[1]);
    if (!idx) return MGX_OK;
    size_t at[2] = {0, (size_t)cnt[0]};
    for (int z = 1; z < sz - 1; z++)
        for (int y = 1; y < sy - 1; y++) {
            const size_t row = g.row(y, z), m = ((size_t)z * sy + y) * sx;
            for (int par = 0; par < 2; par++)  // the even-x half of the row is stored first: ascending offsets
                for (int x = par ? 1 : 2; x < sx - 1; x += 2)
                    if (mask[m + x]) {
                        const size_t k = at[(x + y + z) & 1]++;
                        idx[k] = (unsigned)(row + g.pos(x));
                        if (val) val[k] = values ? values[m + x] : (real)0;
                    }
        }
    return MGX_OK;
}

}  // namespace mgx

#define MGX_PIN3D_API(SFX, real)                                                                                                      \
    extern "C" int mgx3dxs_pin_put_##SFX(mgx_ctx* ctx, real* v, const unsigned* idx, const real* val, unsigned first, unsigned count) { \
        return mgx::pin_put3d<real>(ctx, v, idx, val, first, count);                                                                  \
    }                                                                                                                                 \
    extern "C" int mgx3dxs_pin_list_##SFX(const int n[3], const unsigned char* mask, const real* values, unsigned* idx, real* val,      \
                                          unsigned end[2]) {                                                                          \
        return mgx::pin_list3d<real>(n, mask, values, idx, val, end);                                                                 \
    }

MGX_PIN3D_API(f32, float)
MGX_PIN3D_API(f64, double)
