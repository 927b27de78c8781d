// Loss-guided sampling (this project's extension): behind a reverse step the sample moves down the gradient, with respect to x_t, of a
// caller's differentiable function of the step's x_0 prediction, on the frames with lat == 1.  The caller hands in the cotangent of x_0
// (d loss / d pred_xstart); three streaming passes around the engine's backward-data pass carry it to x_t:
//   guide_seed_kernel    through the clamp of clip_denoised, c_r = cot [-1 <= x_0r <= 1], and through x_0 = a x_t - b eps: the seed of the
//                        backward pass d eps = -b c_r and the direct part d_x = a c_r;
//   guide_norm_kernel    (normalize only) fp64 partial sums of g^2 per item, g = d_x + dx_net / s;
//   guide_final_kernel   g = d_x + dx_net / s, the item's multiplier m_b (scale_b, or scale_b / ||g_b||_2) and, on the latent frames,
//                        sample = fmaf(-m_b, g, sample').
// No floating-point atomics: sum g^2 is folded in fp64 in a fixed order (thread, wave, block, then the blocks in index order), and the
// grid of the norm pass is laid out per item, so an item's norm does not depend on B and is the same on every run.
#include "vd_common.h"
#include <algorithm>

namespace vd {

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int V> __device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
    if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
}  // namespace

// ------------------------------------------------------------------ guide_seed_kernel
// Grid (blocks of an item, B).  Per element of the item: 0 on a frame that is not latent; else, in fp32, one rounding each,
//   c_r = cot where !clip or -1 <= x_0r <= 1 else 0 (x_0r = xstart_from_eps(a, x_t, b, eps): the sampler pass's bits),
//   d eps = (-b) * c_r,  d_x = a * c_r.
// An index t outside the schedule: NaN on every element of the item, and bit 0 of the error word.  V = 4: W % 4 == 0 keeps a group of
// four in one frame, and the item's length a multiple of four.
template <int V>
__global__ __launch_bounds__(256) void guide_seed_kernel(GuideSeedArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int NT = a.num_timesteps;
    const long long t = a.t[b];
    const bool t_ok = t >= 0 && t < NT;
    if (!t_ok && blockIdx.x == 0 && threadIdx.x == 0 && a.err) atomicOr(a.err, VD_ERR_TIMESTEP);
    const float sr = t_ok ? a.tab[TAB_SQRT_RECIP * NT + t] : 0.f, srm1 = t_ok ? a.tab[TAB_SQRT_RECIPM1 * NT + t] : 0.f;
    const unsigned fe = 3u * (unsigned)a.H * (unsigned)a.W;
    const unsigned per = (unsigned)a.T * fe;                     // fewer than 2^31 elements per item (launch_guide_seed checks)
    const size_t base = (size_t)b * per;
    for (unsigned j = (blockIdx.x * 256 + threadIdx.x) * V; j < per; j += gridDim.x * 256 * V) {
        const unsigned f = j / fe;
        float de[V], dx[V];
        if (!t_ok) {
#pragma unroll
            for (int k = 0; k < V; ++k) de[k] = dx[k] = __builtin_nanf("");
        } else if (a.lat[(size_t)b * a.T + f] != 1.0f) {
#pragma unroll
            for (int k = 0; k < V; ++k) de[k] = dx[k] = 0.f;
        } else {
            float xv[V], ev[V], cv[V];
            ldv<V>(a.x + base + j, xv);
            ldv<V>(a.eps + base + j, ev);
            ldv<V>(a.cot + base + j, cv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float x0r = xstart_from_eps(sr, xv[k], srm1, ev[k]);
                const float cr = (!a.clip || (x0r >= -1.0f && x0r <= 1.0f)) ? cv[k] : 0.f;
                de[k] = -srm1 * cr;
                dx[k] = sr * cr;
            }
        }
        stv<V>(a.deps + base + j, de);
        stv<V>(a.dxd + base + j, dx);
    }
}

int launch_guide_seed(const GuideSeedArgs& a, hipStream_t s) {
    VD_REQUIRE(a.x && a.eps && a.cot && a.lat && a.t && a.tab && a.num_timesteps > 0 && a.deps && a.dxd, "guide_seed: null tensor");
    VD_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.H > 0 && a.W > 0, "guide_seed: shape");
    VD_REQUIRE((double)a.T * 3.0 * (double)a.H * (double)a.W < 2147483648.0, "guide_seed: an item of fewer than 2^31 elements");
    const size_t per = (size_t)a.T * 3 * a.H * a.W;
    const bool v4 = a.W % 4 == 0 && al16(a.x) && al16(a.eps) && al16(a.cot) && al16(a.deps) && al16(a.dxd);
    const unsigned nb = (unsigned)std::min<size_t>((per / (v4 ? 4 : 1) + 255) / 256, std::max<size_t>(4096 / a.B, 1));
    if (v4) hipLaunchKernelGGL(guide_seed_kernel<4>, dim3(nb, a.B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(guide_seed_kernel<1>, dim3(nb, a.B), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ guide_norm_kernel
// The sibling of masked_dot_kernel (ode_nll.hip) for a value that exists in no tensor: grid (guide_norm_blocks(per), B), an item's grid a
// function of `per` alone.  A thread walks groups of four consecutive elements of the item, forms g = d_x + dx_net * (1 / s) in fp32 -- the
// final pass's g, bit for bit -- and adds (double)g * (double)g, exact, in element order to its own fp64 sum, an element only where its
// frame has lat == 1.  The 16-byte form loads a group at once, the scalar form element by element with the item's end checked: the same
// additions in the same order.  Thread sums fold by wave shuffles, the four waves in wave order, into part[b][blockIdx.x].
template <bool VEC>
__global__ __launch_bounds__(256) void guide_norm_kernel(const float* __restrict__ dxd, const float* __restrict__ dx_net, const float* __restrict__ gs,
                                                         const float* __restrict__ lat, int T, unsigned fe, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int b = blockIdx.y;
    const float inv_s = gs[1];
    const unsigned per = (unsigned)T * fe, groups = (per + 3u) >> 2;
    const float* pd = dxd + (size_t)b * per;
    const float* pn = dx_net + (size_t)b * per;
    const float* l = lat + (size_t)b * T;
    double acc = 0.0;
    for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const unsigned j = g << 2;
        if constexpr (VEC) {
            if (l[j / fe] != 1.0f) continue;
            float d[4], n[4];
            ldv<4>(pd + j, d);
            ldv<4>(pn + j, n);
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float v = d[k] + n[k] * inv_s; acc += (double)v * (double)v; }
        } else {
#pragma unroll
            for (unsigned k = 0; k < 4; ++k)
                if (j + k < per && l[(j + k) / fe] == 1.0f) { const float v = pd[j + k] + pn[j + k] * inv_s; acc += (double)v * (double)v; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

constexpr int kGuideNormBlocks = 64;
int guide_norm_blocks(long per) { return (int)std::min<long>(((per + 3) / 4 + 255) / 256, kGuideNormBlocks); }

int launch_guide_norm(const float* dxd, const float* dx_net, const float* gs, const float* lat, int B, int T, long frame_elems, double* part,
                      hipStream_t s) {
    VD_REQUIRE(dxd && dx_net && gs && lat && part, "guide_norm: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0, "guide_norm: shape");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "guide_norm: an item of fewer than 2^31 elements");
    const int nblk = guide_norm_blocks((long)T * frame_elems);
    if (frame_elems % 4 == 0 && al16(dxd) && al16(dx_net))
        hipLaunchKernelGGL(guide_norm_kernel<true>, dim3(nblk, B), dim3(256), 0, s, dxd, dx_net, gs, lat, T, (unsigned)frame_elems, part);
    else
        hipLaunchKernelGGL(guide_norm_kernel<false>, dim3(nblk, B), dim3(256), 0, s, dxd, dx_net, gs, lat, T, (unsigned)frame_elems, part);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ guide_final_kernel
// Grid (blocks of an item, B).  Thread 0 of every block forms the item's multiplier: m_b = scale_b, or with the norm pass's partials
// n_b = fp32(sqrt(sum)) -- the partials folded in index order in fp64; block 0 writes n_b -- and m_b = n_b == 0 ? 0 : scale_b / n_b, one
// fp32 division.  Then, per element: g = d_x + dx_net * (1 / s) (dps_final_kernel's arithmetic; 1 / s a power of two), written to `grad`
// when given; on the frames with lat == 1 sample = fmaf(-m_b, g, sample), every other frame keeps the bits the sampler pass wrote.
template <int V>
__global__ __launch_bounds__(256) void guide_final_kernel(const float* __restrict__ dxd, const float* __restrict__ dx_net, const float* __restrict__ gs,
                                                          const float* __restrict__ lat, int T, unsigned fe, const float* __restrict__ scale,
                                                          const double* __restrict__ part, int nblk, float* __restrict__ sample,
                                                          float* __restrict__ grad, float* __restrict__ grad_norm) {
#pragma clang fp contract(off)
    __shared__ float m_s;
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        float m = scale[b];
        if (part) {
            double s = 0.0;
            for (int k = 0; k < nblk; ++k) s += part[(size_t)b * nblk + k];
            const float n = (float)sqrt(s);
            m = n == 0.f ? 0.f : m / n;
            if (blockIdx.x == 0 && grad_norm) grad_norm[b] = n;
        }
        m_s = m;
    }
    __syncthreads();
    const float m = m_s, inv_s = gs[1];
    const unsigned per = (unsigned)T * fe;
    const size_t base = (size_t)b * per;
    for (unsigned j = (blockIdx.x * 256 + threadIdx.x) * V; j < per; j += gridDim.x * 256 * V) {
        float d[V], n[V], g[V];
        ldv<V>(dxd + base + j, d);
        ldv<V>(dx_net + base + j, n);
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = d[k] + n[k] * inv_s;
        if (grad) stv<V>(grad + base + j, g);
        if (lat[(size_t)b * T + j / fe] == 1.0f) {
            float sv[V];
            ldv<V>(sample + base + j, sv);
#pragma unroll
            for (int k = 0; k < V; ++k) sv[k] = fmaf(-m, g[k], sv[k]);
            stv<V>(sample + base + j, sv);
        }
    }
}

int launch_guide_final(const float* dxd, const float* dx_net, const float* gs, const float* lat, int B, int T, long frame_elems,
                       const float* scale, const double* part, float* sample, float* grad, float* grad_norm, hipStream_t s) {
    VD_REQUIRE(dxd && dx_net && gs && lat && scale && sample, "guide_final: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0, "guide_final: shape");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "guide_final: an item of fewer than 2^31 elements");
    const size_t per = (size_t)T * frame_elems;
    const int nblk = part ? guide_norm_blocks((long)per) : 0;
    const bool v4 = frame_elems % 4 == 0 && al16(dxd) && al16(dx_net) && al16(sample) && al16(grad);
    const unsigned nb = (unsigned)std::min<size_t>((per / (v4 ? 4 : 1) + 255) / 256, std::max<size_t>(4096 / B, 1));
    if (v4) hipLaunchKernelGGL(guide_final_kernel<4>, dim3(nb, B), dim3(256), 0, s, dxd, dx_net, gs, lat, T, (unsigned)frame_elems, scale, part, nblk, sample, grad, grad_norm);
    else hipLaunchKernelGGL(guide_final_kernel<1>, dim3(nb, B), dim3(256), 0, s, dxd, dx_net, gs, lat, T, (unsigned)frame_elems, scale, part, nblk, sample, grad, grad_norm);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
