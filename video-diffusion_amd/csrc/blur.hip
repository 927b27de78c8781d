// Deblurring (this project's extension): the measurement operator of DPS (dps.hip) and of particle steering's built-in reward for one real
// k x k kernel w, k odd, 1 <= k <= 15, applied to every channel plane of every frame at "same" size with zeros outside the plane, in the
// orientation of torch's conv2d (correlation), c = k / 2:
//   (A x)[i][j]   = sum_{a,b} w[a][b] x[i + a - c][j + b - c]
//   (A^T r)[p][q] = sum_{a,b} w[a][b] r[p - a + c][q - b + c]        (exact adjoint: the padding is zeros)
// Summation order, both forms, every kernel here: acc = 0, then a = 0 .. k-1 outermost, b = 0 .. k-1 innermost, acc = acc + w[a][b] * v --
// the product rounded to fp32, then the sum rounded to fp32, never a fused multiply-add (contraction is off) -- taps that fall outside the
// plane take part with v = 0.  tests/blur_restated.py restates it.
//   blur_residual_kernel  r = y - A x_0 per element of the latent frames (x_0 through pass_x0, as every sampler pass forms it) and one
//                         fp64 partial of sum r^2 per block;
//   blur_seed_kernel      rho_b from the item's partials and the two seeds of the backward pass: q = -(A^T r) / rho_b through the clamp
//                         q_r = q [-1 <= x_0r <= 1], d eps = -b q_r and the direct part d_x = a q_r (dps_seed_kernel's, but for q);
//   blur_apply_kernel     A x or A^T x of a tensor.
// Neither form stays inside a quad of lanes as the cell mean does: a block works on tiles of kTile x kTile outputs whose operand, with a
// halo of c on every side, lies in LDS -- kTile + 14 rows at most of kLw floats: 8 columns of halo on either side, so that a 16-byte
// global load is wholly inside the plane or wholly outside it, and one float of padding, so that the four rows a group of 32 lanes reads
// (a lane: four consecutive outputs of a row, eight lanes a row) fall on four distinct residues mod 4 of the banks.  A thread slides a
// window of four values along its row: one LDS read per tap beyond the first three.  The taps are read at block-uniform addresses.
// No floating-point atomics: sum r^2 is folded in fp64 in a fixed order (thread, wave, block, then the blocks in index order), and the grid
// of the residual pass is laid out per item, so an item's rho does not depend on B and is the same on every run.
#include "vd_common.h"
#include <algorithm>

namespace vd {

namespace {
constexpr int kTile = 32, kHaloCols = 8, kLw = kTile + 2 * kHaloCols + 1, kLh = kTile + 2 * (kMaxBlurTaps / 2);
static_assert(kMaxBlurTaps / 2 <= kHaloCols && kTile % 4 == 0 && kTile * kTile / 4 == 256, "tile geometry");

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Four values of row `row` of a plane at columns col .. col + 3 (col a multiple of 4, possibly negative), 0 outside the plane.
// VEC (W % 4 == 0, p 16-byte aligned): the four are inside together or outside together.
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int row, int col, int H, int W, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (row < 0 || row >= H) return;
    if (VEC) {
        if (col >= 0 && col < W) {
            const float4 q = *reinterpret_cast<const float4*>(p + (size_t)row * W + col);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e >= 0 && col + e < W) v[e] = p[(size_t)row * W + col + e];
    }
}
// ... and the store of the elements that lie inside the plane (row inside by the caller)
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int row, int col, int W, const float (&v)[4]) {
    if (VEC) {
        if (col < W) *reinterpret_cast<float4*>(p + (size_t)row * W + col) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < W) p[(size_t)row * W + col + e] = v[e];
    }
}

// The tile (row0, col0) of a plane into LDS with its halo: lds[li][lj] = f(row0 - c + li, col0 - kHaloCols + lj), li < kTile + 2c,
// lj < kTile + 2 kHaloCols, in quads of four columns; get(row, col, v) hands out four values (0 outside the plane).
template <class Get>
__device__ __forceinline__ void fill_tile(float* lds, int row0, int col0, int c, Get get) {
    constexpr int QW = (kTile + 2 * kHaloCols) / 4;
    const int quads = (kTile + 2 * c) * QW;
    for (int q = threadIdx.x; q < quads; q += 256) {
        const int li = q / QW, lq = q - li * QW;
        float v[4];
        get(row0 - c + li, col0 - kHaloCols + lq * 4, v);
        float* d = lds + li * kLw + lq * 4;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
}

// The thread's four outputs (tile row ty, tile columns 4 tx .. 4 tx + 3) in the documented order.  Forward: the operand of tap (a, b) of
// output (ty, j) is lds[ty + a][kHaloCols - c + j + b]; adjoint: lds[ty + 2c - a][kHaloCols + c + j - b].
template <bool ADJ>
__device__ __forceinline__ void conv4(const float* lds, const float* __restrict__ w, int k, int ty, int tx, float (&acc)[4]) {
#pragma clang fp contract(off)
    const int c = k >> 1;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
    for (int a = 0; a < k; ++a) {
        const float* row = lds + (ty + (ADJ ? 2 * c - a : a)) * kLw + tx * 4 + (ADJ ? kHaloCols + c : kHaloCols - c);
        const float* wr = w + a * k;
        if (!ADJ) {
            float v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3];
            for (int b = 0; b < k; ++b) {
                const float t = wr[b];
                acc[0] = acc[0] + t * v0; acc[1] = acc[1] + t * v1; acc[2] = acc[2] + t * v2; acc[3] = acc[3] + t * v3;
                v0 = v1; v1 = v2; v2 = v3; v3 = row[b + 4];          // (b + 4 <= k + 3: column <= kHaloCols + c + kTile + 3 < kLw)
            }
        } else {
            float v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3];
            for (int b = 0; b < k; ++b) {
                const float t = wr[b];
                acc[0] = acc[0] + t * v0; acc[1] = acc[1] + t * v1; acc[2] = acc[2] + t * v2; acc[3] = acc[3] + t * v3;
                v3 = v2; v2 = v1; v1 = v0; v0 = row[-b - 1];         // (column >= kHaloCols + c - k >= 0)
            }
        }
    }
}

__device__ __forceinline__ unsigned tiles_of(int n) { return (unsigned)(n + kTile - 1) / kTile; }
}  // namespace

// ------------------------------------------------------------------ blur_residual_kernel
// blockIdx.z is the item, blockIdx.y walks the item's 3 T planes, blockIdx.x a plane's tiles (row-major).  Per tile: x_0 into LDS (the
// tile's own elements also into `xstart` when given), then per thread its four outputs, r = y - acc, and r^2 added in fp64, in column
// order, to the thread's running sum; the block's sum is folded by wave shuffles and across its four waves in wave order, and written to
// part[b][blockIdx.y * gridDim.x + blockIdx.x].  Frames that are not latent: nothing is written to r (blur_seed_kernel does not read it
// there); with `xstart` they still get their x_0.  An index t outside the schedule: the item writes NaN partials (and NaN into `xstart`).
template <bool VEC>
__global__ __launch_bounds__(256) void blur_residual_kernel(BlurArgs a) {
#pragma clang fp contract(off)
    __shared__ float lds[kLh * kLw];
    __shared__ double red[4];
    const int H = a.H, W = a.W, k = a.k, c = k >> 1;
    const size_t hw = (size_t)H * W;
    const unsigned b = blockIdx.z, planes = (unsigned)a.T * 3, tx_n = tiles_of(W), tiles = tiles_of(H) * tx_n;
    const int NT = a.num_timesteps;
    const long long t = a.t[b];
    const bool t_ok = t >= 0 && t < NT;
    const float sr = t_ok ? a.tab[TAB_SQRT_RECIP * NT + t] : 0.f, srm1 = t_ok ? a.tab[TAB_SQRT_RECIPM1 * NT + t] : 0.f;
    const int ty = threadIdx.x >> 3, tx = threadIdx.x & 7;
    double acc = t_ok ? 0.0 : (double)__builtin_nanf("");
    for (unsigned plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const size_t frame = (size_t)b * a.T + plane / 3, base = ((size_t)b * planes + plane) * hw;
        const bool latent = a.lat[frame] == 1.0f;
        if (!latent && !a.xstart) continue;                        // (uniform over the block: a plane lies in one frame)
        const bool conv = latent && t_ok;
        for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int row0 = (int)(tile / tx_n) * kTile, col0 = (int)(tile % tx_n) * kTile;
            // a frame that only hands out its x_0 needs no halo
            fill_tile(lds, row0, col0, conv ? c : 0, [&](int row, int col, float (&v)[4]) {
                float x[4], s[4];
                load4<VEC>(a.x + base, row, col, H, W, x);
                load4<VEC>(a.eps + base, row, col, H, W, s);
                bool nonfinite = false;                            // the sampler pass of the step reads the same values and raises the bit
                const bool own = row >= row0 && row < row0 + kTile && row < H && col >= col0 && col < col0 + kTile;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = row >= 0 && row < H && col + e >= 0 && col + e < W;
                    v[e] = !in ? 0.f : t_ok ? pass_x0(x[e], s[e], false, sr, srm1, a.clip, nonfinite) : __builtin_nanf("");
                }
                if (a.xstart && own) store4<VEC>(a.xstart + base, row, col, W, v);
            });
            if (conv) {
                __syncthreads();
                const int row = row0 + ty, col = col0 + tx * 4;
                if (row < H && col < W) {
                    float s[4], y[4], r[4];
                    conv4<false>(lds, a.taps, k, ty, tx, s);
                    load4<VEC>(a.y + base, row, col, H, W, y);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        r[e] = y[e] - s[e];
                        if (col + e < W) acc += (double)r[e] * (double)r[e];
                    }
                    store4<VEC>(a.r + base, row, col, W, r);
                }
            }
            __syncthreads();
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        a.part[(size_t)b * a.nblk + blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the grid of one item: its planes along y, a plane's tiles along x, dps_partials_per_item() blocks at most -- a function of (T, H, W)
// alone, so that an item's partials, and their number, do not depend on B
static dim3 blur_residual_grid(const BlurArgs& a) {
    const size_t cap = dps_partials_per_item();
    const size_t tiles = (size_t)((a.H + kTile - 1) / kTile) * ((a.W + kTile - 1) / kTile), planes = (size_t)a.T * 3;
    const unsigned gy = (unsigned)std::min<size_t>(planes, cap);
    const unsigned gx = (unsigned)std::min<size_t>(tiles, std::max<size_t>(cap / gy, 1));
    return dim3(gx, gy, (unsigned)a.B);
}

static bool blur_vec(const BlurArgs& a) {
    return a.W % 4 == 0 && al16(a.x) && al16(a.eps) && al16(a.y) && al16(a.r) && (!a.xstart || al16(a.xstart));
}

static int check_blur_args(const BlurArgs& a, const char* who, bool seed) {
    VD_REQUIRE(a.x && a.eps && a.y && a.lat && a.t && a.tab && a.num_timesteps > 0 && a.r && a.part && a.taps && (!seed || (a.deps && a.dxd)),
               std::string(who) + ": null tensor");
    VD_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.H > 0 && a.W > 0, std::string(who) + ": shape");
    VD_REQUIRE((double)a.T * 3.0 * (double)a.H * (double)a.W < 2147483648.0, std::string(who) + ": an item of fewer than 2^31 elements");
    VD_REQUIRE(blur_served(a.k), "blur: the kernel is k x k with k odd and 1 <= k <= 15");
    return 0;
}

// ------------------------------------------------------------------ blur_seed_kernel
// Grid (blocks of an item, B).  Thread 0 of every block folds the item's partials in index order in fp64, rho_b = fp32(sqrt(sum)); block
// 0 writes it.  Then the block walks the item's (plane, tile) pairs: 0 on a frame that is not latent or where rho_b == 0; else r with its
// halo into LDS and, per element, in fp32, one rounding each,
//   q = -(A^T r) / rho_b,  q_r = q where !clip or -1 <= x_0r <= 1 else 0 (x_0r = xstart_from_eps(a, x_t, b, eps): the sampler pass's
//   bits),  d eps = (-b) * q_r,  d_x = a * q_r.
// An index t outside the schedule: NaN on every element of the item and in rho_b, and bit 0 of the error word.
template <bool VEC>
__global__ __launch_bounds__(256) void blur_seed_kernel(BlurArgs a) {
#pragma clang fp contract(off)
    __shared__ float lds[kLh * kLw];
    __shared__ float rho_s;
    const int b = blockIdx.y;
    const int NT = a.num_timesteps;
    const long long t = a.t[b];
    const bool t_ok = t >= 0 && t < NT;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int j = 0; j < a.nblk; ++j) s += a.part[(size_t)b * a.nblk + j];
        const float rho = t_ok ? (float)sqrt(s) : __builtin_nanf("");
        rho_s = rho;
        if (blockIdx.x == 0) {
            if (a.rho) a.rho[b] = rho;
            if (!t_ok && a.err) atomicOr(a.err, VD_ERR_TIMESTEP);
        }
    }
    __syncthreads();
    const float rho = rho_s;
    const float sr = t_ok ? a.tab[TAB_SQRT_RECIP * NT + t] : 0.f, srm1 = t_ok ? a.tab[TAB_SQRT_RECIPM1 * NT + t] : 0.f;
    const int H = a.H, W = a.W, k = a.k, c = k >> 1;
    const size_t hw = (size_t)H * W;
    const unsigned planes = (unsigned)a.T * 3, tx_n = tiles_of(W), tiles = tiles_of(H) * tx_n;
    const int ty = threadIdx.x >> 3, tx = threadIdx.x & 7;
    for (unsigned wi = blockIdx.x; wi < planes * tiles; wi += gridDim.x) {
        const unsigned plane = wi / tiles, tile = wi - plane * tiles;
        const size_t base = ((size_t)b * planes + plane) * hw;
        const int row0 = (int)(tile / tx_n) * kTile, col0 = (int)(tile % tx_n) * kTile;
        const int row = row0 + ty, col = col0 + tx * 4;
        const bool mine = row < H && col < W;
        float de[4], dx[4];
        const bool conv = t_ok && a.lat[(size_t)b * a.T + plane / 3] == 1.0f && rho != 0.f;      // (uniform over the block)
        if (!conv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) de[e] = dx[e] = t_ok ? 0.f : __builtin_nanf("");
        } else {
            fill_tile(lds, row0, col0, c, [&](int rr, int cc, float (&v)[4]) { load4<VEC>(a.r + base, rr, cc, H, W, v); });
            __syncthreads();
            if (mine) {
                float s[4], xv[4], ev[4];
                conv4<true>(lds, a.taps, k, ty, tx, s);
                load4<VEC>(a.x + base, row, col, H, W, xv);
                load4<VEC>(a.eps + base, row, col, H, W, ev);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float q = -s[e] / rho;
                    const float x0r = xstart_from_eps(sr, xv[e], srm1, ev[e]);
                    const float qr = (!a.clip || (x0r >= -1.0f && x0r <= 1.0f)) ? q : 0.f;
                    de[e] = -srm1 * qr;
                    dx[e] = sr * qr;
                }
            }
            __syncthreads();
        }
        if (mine) {
            store4<VEC>(a.deps + base, row, col, W, de);
            store4<VEC>(a.dxd + base, row, col, W, dx);
        }
    }
}

static void launch_blur_residual_kernel(const BlurArgs& a, hipStream_t s) {
    const dim3 grid = blur_residual_grid(a);
    if (blur_vec(a)) hipLaunchKernelGGL(blur_residual_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(blur_residual_kernel<false>, grid, dim3(256), 0, s, a);
}

int launch_blur_seed(BlurArgs a, hipStream_t s) {
    if (int rc = check_blur_args(a, "blur_seed", true)) return rc;
    const dim3 rg = blur_residual_grid(a);
    a.nblk = (int)(rg.x * rg.y);
    launch_blur_residual_kernel(a, s);
    const size_t work = (size_t)a.T * 3 * ((a.H + kTile - 1) / kTile) * ((a.W + kTile - 1) / kTile);
    const unsigned nb = (unsigned)std::min<size_t>(work, std::max<size_t>(4096 / a.B, 1));
    const bool v4 = a.W % 4 == 0 && al16(a.x) && al16(a.eps) && al16(a.r) && al16(a.deps) && al16(a.dxd);
    if (v4) hipLaunchKernelGGL(blur_seed_kernel<true>, dim3(nb, a.B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(blur_seed_kernel<false>, dim3(nb, a.B), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// The residual pass alone (particle steering's built-in reward: particles.hip): r and the per-item partials of sum r^2, no seed pass.
// *nblk: partials per item of this launch.  deps, dxd, rho and err are not read.
int launch_blur_residual(BlurArgs a, int* nblk, hipStream_t s) {
    if (int rc = check_blur_args(a, "blur_residual", false)) return rc;
    VD_REQUIRE(nblk, "blur_residual: null tensor");
    const dim3 rg = blur_residual_grid(a);
    a.nblk = (int)(rg.x * rg.y);
    *nblk = a.nblk;
    launch_blur_residual_kernel(a, s);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ blur_apply_kernel
// out = A x (adjoint == 0) or A^T x of `planes` planes of H x W; the block walks the (plane, tile) pairs.
template <bool VEC, bool ADJ>
__global__ __launch_bounds__(256) void blur_apply_kernel(const float* __restrict__ x, const float* __restrict__ taps, int k, size_t planes, int H,
                                                         int W, float* __restrict__ out) {
    __shared__ float lds[kLh * kLw];
    const int c = k >> 1;
    const size_t hw = (size_t)H * W;
    const unsigned tx_n = tiles_of(W), tiles = tiles_of(H) * tx_n;
    const int ty = threadIdx.x >> 3, tx = threadIdx.x & 7;
    for (size_t wi = blockIdx.x; wi < planes * tiles; wi += gridDim.x) {
        const size_t plane = wi / tiles;
        const unsigned tile = (unsigned)(wi - plane * tiles);
        const int row0 = (int)(tile / tx_n) * kTile, col0 = (int)(tile % tx_n) * kTile;
        fill_tile(lds, row0, col0, c, [&](int rr, int cc, float (&v)[4]) { load4<VEC>(x + plane * hw, rr, cc, H, W, v); });
        __syncthreads();
        const int row = row0 + ty, col = col0 + tx * 4;
        if (row < H && col < W) {
            float s[4];
            conv4<ADJ>(lds, taps, k, ty, tx, s);
            store4<VEC>(out + plane * hw, row, col, W, s);
        }
        __syncthreads();
    }
}

int launch_blur_apply(const float* x, const float* taps, int k, int adjoint, size_t planes, int H, int W, float* out, hipStream_t s) {
    VD_REQUIRE(x && taps && out && x != out, "blur: null tensor, or out == x");
    VD_REQUIRE(planes > 0 && H > 0 && W > 0 && (double)H * (double)W < 2147483648.0, "blur: shape");
    VD_REQUIRE(blur_served(k), "blur: the kernel is k x k with k odd and 1 <= k <= 15");
    const size_t work = planes * ((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile);
    const unsigned grid = (unsigned)std::min<size_t>(work, 4096);
    const bool vec = W % 4 == 0 && al16(x) && al16(out);
    if (vec && adjoint) hipLaunchKernelGGL((blur_apply_kernel<true, true>), dim3(grid), dim3(256), 0, s, x, taps, k, planes, H, W, out);
    else if (vec) hipLaunchKernelGGL((blur_apply_kernel<true, false>), dim3(grid), dim3(256), 0, s, x, taps, k, planes, H, W, out);
    else if (adjoint) hipLaunchKernelGGL((blur_apply_kernel<false, true>), dim3(grid), dim3(256), 0, s, x, taps, k, planes, H, W, out);
    else hipLaunchKernelGGL((blur_apply_kernel<false, false>), dim3(grid), dim3(256), 0, s, x, taps, k, planes, H, W, out);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
