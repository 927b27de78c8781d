// Diffusion posterior sampling (this project's extension; DPS, Chung, Kim, McCann, Klasky, Ye, ICLR 2023) for the "cell mean" operators
// of measure.hip: behind a reverse step the sample moves down the gradient of rho_b = ||y - A x_0(x_t)||_2 with respect to x_t, per batch
// item, on the frames with lat == 1.  Three streaming passes around the engine's backward-data pass:
//   dps_residual_kernel   r = y - A x_0 per cell of the latent frames (x_0 through pass_x0, as every sampler pass forms it) and one
//                         fp64 partial of sum r^2 per block;
//   dps_seed_kernel       rho_b from the item's partials, and the two seeds of the backward pass: q = -r / (rho_b n_c) on every element
//                         of a cell, through the clamp q_r = q [-1 <= x_0r <= 1], d eps = -b q_r and the direct part d_x = a q_r;
//   dps_final_kernel      g = d_x + dx_net / s and, on the latent frames, sample = fmaf(-zeta, g, sample').
// No floating-point atomics: sum r^2 is folded in fp64 in a fixed order (thread, wave, block, then the blocks in index order), and the
// grid of the residual pass is laid out per item, so an item's rho does not depend on B and is the same on every run.
#include "vd_common.h"
#include <algorithm>

namespace vd {

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the value of lane (id ^ M), M in {1, 2, 4, 8} (measure.hip: DPP inside a quad, the swizzle crossbar across the quads of a row of 16)
template <int M>
__device__ __forceinline__ float lane_xor(float v) {
    int i = __float_as_int(v);
    if constexpr (M == 1) i = __builtin_amdgcn_update_dpp(0, i, 0xB1, 0xF, 0xF, true);
    else if constexpr (M == 2) i = __builtin_amdgcn_update_dpp(0, i, 0x4E, 0xF, 0xF, true);
    else i = __builtin_amdgcn_ds_swizzle(i, (M << 10) | 0x1F);
    return __int_as_float(i);
}

template <int V> __device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
    if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
}  // namespace

// ------------------------------------------------------------------ dps_residual_kernel
// The thread -> cell map and the summation order of a cell are measurement_project_kernel's (a row segment per lane and channel, the
// channels' segment sums in channel order, the xor butterfly over the cell's L lanes; no LDS in the cell's reduction).  blockIdx.z is the
// item, blockIdx.y walks the item's planes (gray: its frames), blockIdx.x and the thread the lanes of a plane.  Lane 0 of a cell writes
// r = y - sum / n_c and adds r^2, in fp64, to its own running sum; the block's sum is folded by wave shuffles and across its four waves
// in wave order, and written to part[b][blockIdx.y * gridDim.x + blockIdx.x].  Frames that are not latent: nothing is written to r
// (dps_seed_kernel does not read it there); with `xstart` they still get their x_0.  An index t outside the schedule: the item writes
// NaN partials (and NaN into `xstart`), and the seed pass poisons it.
template <int S, bool GRAY, bool VEC>
__global__ __launch_bounds__(256) void dps_residual_kernel(DpsArgs a) {
    constexpr int SEG = S < 4 ? S : 4, NC = VEC ? 4 / SEG : 1, E = SEG * NC, HX = S > 4 ? S / 4 : 1, L = S * HX, CH = GRAY ? 3 : 1;
    constexpr int UW = HX * E;
    __shared__ double red[4];
    const size_t hw = (size_t)a.H * a.W;
    const unsigned ux = (unsigned)a.W / UW, uy = (unsigned)a.H / S, ws = (unsigned)a.W / S;
    const unsigned b = blockIdx.z;
    const unsigned planes = (unsigned)a.T * (GRAY ? 1 : 3);         // of this item
    const unsigned lanes = uy * ux * L;
    const int NT = a.num_timesteps;
    const float n = (float)(S * S * CH);
    const long long t = a.t[b];
    const bool t_ok = t >= 0 && t < NT;
    const float sr = t_ok ? a.tab[TAB_SQRT_RECIP * NT + t] : 0.f, srm1 = t_ok ? a.tab[TAB_SQRT_RECIPM1 * NT + t] : 0.f;
    double acc = t_ok ? 0.0 : (double)__builtin_nanf("");
    for (unsigned plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const size_t frame = (size_t)b * a.T + (GRAY ? plane : plane / 3), c0 = GRAY ? 0 : plane % 3;
        const bool latent = a.lat[frame] == 1.0f;
        if (!latent && !a.xstart) continue;                       // (uniform over the block: a plane lies in one frame)
        for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < lanes; g += gridDim.x * 256) {
            const unsigned l = g % L, u = g / L, cx = u % ux, cy = u / ux;
            const unsigned row = cy * S + l / HX, col = cx * UW + (l % HX) * E;
            float v[CH][E];
            bool nonfinite = false;                                // the sampler pass of the step reads the same values and raises the bit
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const size_t i = (frame * 3 + c0 + c) * hw + row * (unsigned)a.W + col;
                float s[E], x[E];
                if (VEC) {
                    *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(a.eps + i);
                    *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(a.x + i);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) { s[e] = a.eps[i + e]; x[e] = a.x[i + e]; }
                }
#pragma unroll
                for (int e = 0; e < E; ++e) v[c][e] = t_ok ? pass_x0(x[e], s[e], false, sr, srm1, a.clip, nonfinite) : __builtin_nanf("");
                if (a.xstart) {
                    if (VEC) *reinterpret_cast<float4*>(a.xstart + i) = *reinterpret_cast<const float4*>(v[c]);
                    else {
#pragma unroll
                        for (int e = 0; e < E; ++e) a.xstart[i + e] = v[c][e];
                    }
                }
            }
            if (!latent || !t_ok) continue;                        // (uniform over the block)
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                float p = 0.f;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    float q = v[c][k * SEG];
#pragma unroll
                    for (int j = 1; j < SEG; ++j) q += v[c][k * SEG + j];
                    p = c == 0 ? q : p + q;
                }
                if constexpr (L >= 2) p += lane_xor<1>(p);
                if constexpr (L >= 4) p += lane_xor<2>(p);
                if constexpr (L >= 16) { p += lane_xor<4>(p); p += lane_xor<8>(p); }
                if (l == 0) {
                    const size_t yi = ((frame * (GRAY ? 1 : 3) + c0) * uy + cy) * ws + col / S + k;
                    const float r = a.y[yi] - p / n;
                    a.r[yi] = r;
                    acc += (double)r * (double)r;
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        a.part[(size_t)b * a.nblk + blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the grid of one item: its planes along y, a plane's lanes along x, kDpsItemBlocks blocks at most -- a function of (T, H, W, scale, gray,
// form) alone, so that an item's partials, and their number, do not depend on B
constexpr int kDpsItemBlocks = 128;
template <int S, bool GRAY>
static dim3 residual_grid(const DpsArgs& a, bool vec) {
    constexpr int SEG = S < 4 ? S : 4, HX = S > 4 ? S / 4 : 1, L = S * HX;
    const size_t uw = (size_t)HX * (vec ? 4 : SEG);
    const size_t lanes = (size_t)(a.H / S) * (a.W / uw) * L, planes = (size_t)a.T * (GRAY ? 1 : 3);
    const unsigned gy = (unsigned)std::min<size_t>(planes, kDpsItemBlocks);
    const unsigned gx = (unsigned)std::min<size_t>((lanes + 255) / 256, std::max<size_t>(kDpsItemBlocks / gy, 1));
    return dim3(gx, gy, (unsigned)a.B);
}
template <int S, bool GRAY>
static void launch_residual(const DpsArgs& a, bool vec, hipStream_t s) {
    const dim3 grid = residual_grid<S, GRAY>(a, vec);
    if (vec) hipLaunchKernelGGL((dps_residual_kernel<S, GRAY, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((dps_residual_kernel<S, GRAY, false>), grid, dim3(256), 0, s, a);
}

static bool dps_vec(const DpsArgs& a) { return a.W % 4 == 0 && al16(a.x) && al16(a.eps) && (!a.xstart || al16(a.xstart)); }

static dim3 dps_residual_grid(const DpsArgs& a) {
    const bool vec = dps_vec(a);
    switch (a.scale * 2 + (a.gray ? 1 : 0)) {
        case 3: return residual_grid<1, true>(a, vec);
        case 4: return residual_grid<2, false>(a, vec);
        case 5: return residual_grid<2, true>(a, vec);
        case 8: return residual_grid<4, false>(a, vec);
        case 9: return residual_grid<4, true>(a, vec);
        case 16: return residual_grid<8, false>(a, vec);
        default: return residual_grid<8, true>(a, vec);
    }
}

size_t dps_partials_per_item() { return kDpsItemBlocks; }      // doubles per item at most, whatever the operator and the form

// ------------------------------------------------------------------ dps_seed_kernel
// Grid (blocks of an item, B).  Thread 0 of every block folds the item's partials in index order in fp64, rho_b = fp32(sqrt(sum)); block
// 0 writes it.  Then, per element of the item: 0 on a frame that is not latent or where rho_b == 0; else, in fp32, one rounding each,
//   q = -r_cell / (rho_b * n_c),  q_r = q where !clip or -1 <= x_0r <= 1 else 0 (x_0r = xstart_from_eps(a, x_t, b, eps): the sampler pass's
//   bits),  d eps = (-b) * q_r,  d_x = a * q_r.
// rho_b * n_c is exact for the plain operators (n_c a power of two) and one rounding with gray.  An index t outside the schedule: NaN on
// every element of the item and in rho_b, and bit 0 of the error word.
template <int V>
__global__ __launch_bounds__(256) void dps_seed_kernel(DpsArgs a) {
#pragma clang fp contract(off)
    __shared__ float rho_s;
    const int b = blockIdx.y;
    const int NT = a.num_timesteps;
    const long long t = a.t[b];
    const bool t_ok = t >= 0 && t < NT;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < a.nblk; ++k) s += a.part[(size_t)b * a.nblk + k];
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
    const int S = a.scale, Cy = a.gray ? 1 : 3;
    const float den = rho * (float)(S * S * (a.gray ? 3 : 1));
    const unsigned W = (unsigned)a.W, hw = (unsigned)a.H * W, fe = 3 * hw, uy = (unsigned)a.H / S, ws = W / S;
    const unsigned per = (unsigned)a.T * fe;                     // fewer than 2^31 elements per item (launch_dps_seed checks)
    const size_t base = (size_t)b * per;
    for (unsigned j = (blockIdx.x * 256 + threadIdx.x) * V; j < per; j += gridDim.x * 256 * V) {
        const unsigned f = j / fe, rem = j - f * fe, c = rem / hw, p = rem - c * hw, row = p / W, col = p - row * W;
        float de[V], dx[V];
        if (!t_ok) {
#pragma unroll
            for (int k = 0; k < V; ++k) de[k] = dx[k] = __builtin_nanf("");
        } else if (a.lat[(size_t)b * a.T + f] != 1.0f || rho == 0.f) {
#pragma unroll
            for (int k = 0; k < V; ++k) de[k] = dx[k] = 0.f;
        } else {
            float xv[V], ev[V];
            ldv<V>(a.x + base + j, xv);
            ldv<V>(a.eps + base + j, ev);
            const size_t yrow = ((((size_t)b * a.T + f) * Cy + (a.gray ? 0 : c)) * uy + row / S) * ws;
#pragma unroll
            for (int k = 0; k < V; ++k) {                          // (V == 4: W % 4 == 0, the four elements lie in one row)
                const float q = -a.r[yrow + (col + k) / S] / den;
                const float x0r = xstart_from_eps(sr, xv[k], srm1, ev[k]);
                const float qr = (!a.clip || (x0r >= -1.0f && x0r <= 1.0f)) ? q : 0.f;
                de[k] = -srm1 * qr;
                dx[k] = sr * qr;
            }
        }
        stv<V>(a.deps + base + j, de);
        stv<V>(a.dxd + base + j, dx);
    }
}

int launch_dps_seed(DpsArgs a, hipStream_t s) {
    VD_REQUIRE(a.x && a.eps && a.y && a.lat && a.t && a.tab && a.num_timesteps > 0 && a.r && a.part && a.deps && a.dxd, "dps_seed: null tensor");
    VD_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.H > 0 && a.W > 0, "dps_seed: shape");
    VD_REQUIRE((double)a.T * 3.0 * (double)a.H * (double)a.W < 2147483648.0, "dps_seed: an item of fewer than 2^31 elements");
    VD_REQUIRE(measurement_served(a.scale, a.gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
    VD_REQUIRE(a.H % a.scale == 0 && a.W % a.scale == 0, "measurement: H and W must be divisible by scale");
    const bool vec = dps_vec(a);
    const dim3 rg = dps_residual_grid(a);
    a.nblk = (int)(rg.x * rg.y);
    switch (a.scale * 2 + (a.gray ? 1 : 0)) {
        case 3: launch_residual<1, true>(a, vec, s); break;
        case 4: launch_residual<2, false>(a, vec, s); break;
        case 5: launch_residual<2, true>(a, vec, s); break;
        case 8: launch_residual<4, false>(a, vec, s); break;
        case 9: launch_residual<4, true>(a, vec, s); break;
        case 16: launch_residual<8, false>(a, vec, s); break;
        default: launch_residual<8, true>(a, vec, s); break;
    }
    const size_t per = (size_t)a.T * 3 * a.H * a.W;
    const bool v4 = a.W % 4 == 0 && al16(a.x) && al16(a.eps) && al16(a.deps) && al16(a.dxd);
    const unsigned nb = (unsigned)std::min<size_t>((per / (v4 ? 4 : 1) + 255) / 256, std::max<size_t>(4096 / a.B, 1));
    if (v4) hipLaunchKernelGGL(dps_seed_kernel<4>, dim3(nb, a.B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dps_seed_kernel<1>, dim3(nb, a.B), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// The residual pass alone (particle steering's built-in reward: particles.hip): r and the per-item partials of sum r^2, no seed pass.
// *nblk: partials per item of this launch.  deps, dxd, rho and err are not read.
int launch_dps_residual(DpsArgs a, int* nblk, hipStream_t s) {
    VD_REQUIRE(a.x && a.eps && a.y && a.lat && a.t && a.tab && a.num_timesteps > 0 && a.r && a.part && nblk, "dps_residual: null tensor");
    VD_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.H > 0 && a.W > 0, "dps_residual: shape");
    VD_REQUIRE(measurement_served(a.scale, a.gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
    VD_REQUIRE(a.H % a.scale == 0 && a.W % a.scale == 0, "measurement: H and W must be divisible by scale");
    const bool vec = dps_vec(a);
    const dim3 rg = dps_residual_grid(a);
    a.nblk = (int)(rg.x * rg.y);
    *nblk = a.nblk;
    switch (a.scale * 2 + (a.gray ? 1 : 0)) {
        case 3: launch_residual<1, true>(a, vec, s); break;
        case 4: launch_residual<2, false>(a, vec, s); break;
        case 5: launch_residual<2, true>(a, vec, s); break;
        case 8: launch_residual<4, false>(a, vec, s); break;
        case 9: launch_residual<4, true>(a, vec, s); break;
        case 16: launch_residual<8, false>(a, vec, s); break;
        default: launch_residual<8, true>(a, vec, s); break;
    }
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ dps_final_kernel
// g = d_x + dx_net * (1 / s) on every element (1 / s a power of two: launch_grad_rescale), written to `grad` when given; on the frames with
// lat == 1 sample = fmaf(-zeta, g, sample), every other frame keeps the bits the sampler pass wrote.
template <int V>
__global__ __launch_bounds__(256) void dps_final_kernel(const float* __restrict__ dxd, const float* __restrict__ dx_net, const float* __restrict__ gs,
                                                        const float* __restrict__ lat, long fe, size_t total, float zeta,
                                                        float* __restrict__ sample, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const float inv_s = gs[1];
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (size_t)gridDim.x * 256 * V) {
        float d[V], n[V], g[V];
        ldv<V>(dxd + i, d);
        ldv<V>(dx_net + i, n);
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = d[k] + n[k] * inv_s;
        if (grad) stv<V>(grad + i, g);
        if (lat[i / fe] == 1.0f) {
            float sv[V];
            ldv<V>(sample + i, sv);
#pragma unroll
            for (int k = 0; k < V; ++k) sv[k] = fmaf(-zeta, g[k], sv[k]);
            stv<V>(sample + i, sv);
        }
    }
}

int launch_dps_final(const float* dxd, const float* dx_net, const float* gs, const float* lat, int B, int T, long frame_elems, float zeta,
                     float* sample, float* grad, hipStream_t s) {
    VD_REQUIRE(dxd && dx_net && gs && lat && sample, "dps_final: null tensor");
    VD_REQUIRE(B > 0 && T > 0 && frame_elems > 0, "dps_final: shape");
    const size_t total = (size_t)B * T * frame_elems;
    const bool v4 = frame_elems % 4 == 0 && al16(dxd) && al16(dx_net) && al16(sample) && al16(grad);
    const unsigned grid = (unsigned)std::min<size_t>((total / (v4 ? 4 : 1) + 255) / 256, 4096);
    if (v4) hipLaunchKernelGGL(dps_final_kernel<4>, dim3(grid), dim3(256), 0, s, dxd, dx_net, gs, lat, frame_elems, total, zeta, sample, grad);
    else hipLaunchKernelGGL(dps_final_kernel<1>, dim3(grid), dim3(256), 0, s, dxd, dx_net, gs, lat, frame_elems, total, zeta, sample, grad);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
