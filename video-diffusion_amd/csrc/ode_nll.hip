// Probability-flow ODE likelihood (this project's extension; Song, Sohl-Dickstein, Kingma, Kumar, Ermon, Poole, ICLR 2021, with the
// Skilling-Hutchinson trace estimate): the streaming passes around the engine's backward-data pass.
//   rademacher_kernel   a probe v: +-1.0f on the frames with lat == 1, 0 elsewhere, from the engine's Philox stream;
//   masked_dot_kernel   per item sum over its latent frames of a * b in fp64 (v^T (J^T v), and x_T^T x_T of the prior term), one partial per
//   + masked_fold_kernel  block, folded in index order by a second launch;
//   ode_heun_kernel     the corrector x_{i+1} = r_{i+1} (x_i / r_i + (sigma_{i+1} - sigma_i) / 2 (eps + eps')) on the latent frames;
//   keep_frames_kernel  behind the Euler move, which runs on every frame: the frames that are not latent get the bits of x back;
//   dequantize_kernel   uniform noise of one 8-bit bin on the latent frames (the job's default input);
//   scale_by_kernel     out = in * gs[1] behind a backward pass that ran on a power-of-two multiple (launch_grad_rescale).
// The predictor (and the whole Euler step) is deterministic_kernel<SAMPLER_DDIM_REVERSE> of misc.hip with its clamp off: with u = x / r
// and sigma = sqrt_recipm1 it is u' = u + (sigma' - sigma) eps.  No floating-point atomics anywhere: a result is the same on every run.
#include "vd_common.h"
#include <algorithm>

namespace vd {

namespace {
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

// ------------------------------------------------------------------ rademacher_kernel
// Element j of item b in probe k reads ONE bit of the Philox stream (seed, .): block item_offset[b] + k * nb + (j >> 7) with
// nb = ceil(per / 128) blocks per probe, word (j >> 5) & 3 of the block's four, bit j & 31 of that word; a set bit is -1.0f, a clear one
// +1.0f.  128 consecutive elements share a block, so a probe consumes nb blocks and probes k, k + 1 never overlap.  Nothing depends on B
// or on b beyond item_offset[b]: item b of a batched call has the bits of the call on b alone.  Grid (blocks of an item, B); V = 4: four
// elements per thread, one 16-byte store (frame_elems % 4 == 0 keeps them in one frame and j & 31 <= 28 in one word); V = 1: any size and
// alignment, same bits.
template <int V>
__global__ __launch_bounds__(256) void rademacher_kernel(float* __restrict__ out, const float* __restrict__ lat, int T, unsigned fe,
                                                         unsigned long long seed, const unsigned long long* __restrict__ item_offset,
                                                         unsigned long long probe) {
    const int b = blockIdx.y;
    const unsigned per = (unsigned)T * fe;                             // fewer than 2^31 elements per item (launch_rademacher checks)
    const unsigned long long base = item_offset[b] + probe * (unsigned long long)((per + 127u) >> 7);
    float* o = out + (size_t)b * per;
    for (unsigned j = (blockIdx.x * 256 + threadIdx.x) * V; j < per; j += gridDim.x * 256 * V) {
        float v[V];
        if (lat[(size_t)b * T + j / fe] == 1.0f) {
            unsigned r[4];
            philox4x32_10(base + (j >> 7), seed, r);
            const unsigned w = r[(j >> 5) & 3];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = ((w >> ((j + k) & 31)) & 1u) ? -1.0f : 1.0f;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = 0.0f;
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(o + j) = make_float4(v[0], v[1], v[2], v[3]);
        else o[j] = v[0];
    }
}

int launch_rademacher(float* out, const float* lat, int B, int T, long frame_elems, unsigned long long seed,
                      const unsigned long long* item_offset, unsigned long long probe, hipStream_t s) {
    VD_REQUIRE(out && lat && item_offset, "rademacher: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0, "rademacher: shape");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "rademacher: an item of fewer than 2^31 elements");
    const size_t per = (size_t)T * frame_elems;
    const bool v4 = frame_elems % 4 == 0 && al16(out);
    const unsigned nb = (unsigned)std::min<size_t>((per / (v4 ? 4 : 1) + 255) / 256, std::max<size_t>(4096 / B, 1));
    if (v4) hipLaunchKernelGGL(rademacher_kernel<4>, dim3(nb, B), dim3(256), 0, s, out, lat, T, (unsigned)frame_elems, seed, item_offset, probe);
    else hipLaunchKernelGGL(rademacher_kernel<1>, dim3(nb, B), dim3(256), 0, s, out, lat, T, (unsigned)frame_elems, seed, item_offset, probe);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ masked_dot_kernel, masked_fold_kernel
// Grid (masked_dot_blocks(per), B): an item's grid is a function of `per` alone, so its sum does not depend on B.  A thread walks groups of
// four consecutive elements 4g .. 4g + 3 of the item and adds (double)a * (double)b -- exact: 48 significand bits -- in element order to
// its own fp64 sum, an element only where its frame has lat == 1; the 16-byte form (frame_elems % 4 == 0, both tensors aligned) loads a
// group at once, the scalar form element by element with the item's end checked: the same additions in the same order, the same bits.
// Thread sums fold by wave shuffles, the four waves in wave order, into part[b][blockIdx.x].
template <bool VEC>
__global__ __launch_bounds__(256) void masked_dot_kernel(const float* __restrict__ a, const float* __restrict__ bv, const float* __restrict__ lat,
                                                         int T, unsigned fe, double* __restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const unsigned per = (unsigned)T * fe, groups = (per + 3u) >> 2;
    const float* pa = a + (size_t)b * per;
    const float* pb = bv + (size_t)b * per;
    const float* l = lat + (size_t)b * T;
    double acc = 0.0;
    for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const unsigned j = g << 2;
        if constexpr (VEC) {
            if (l[j / fe] != 1.0f) continue;
            const float4 x = *reinterpret_cast<const float4*>(pa + j), y = *reinterpret_cast<const float4*>(pb + j);
            acc += (double)x.x * (double)y.x;
            acc += (double)x.y * (double)y.y;
            acc += (double)x.z * (double)y.z;
            acc += (double)x.w * (double)y.w;
        } else {
#pragma unroll
            for (unsigned k = 0; k < 4; ++k)
                if (j + k < per && l[(j + k) / fe] == 1.0f) acc += (double)pa[j + k] * (double)pb[j + k];
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One thread per item: s = part[b][0] + part[b][1] + ... in index order; out[b] = ((accumulate ? out[b] : 0) + s) / divisor.
__global__ void masked_fold_kernel(const double* __restrict__ part, int nblk, int B, int accumulate, double divisor, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += part[(size_t)b * nblk + k];
    if (accumulate) s = out[b] + s;
    out[b] = s / divisor;
}

constexpr int kMaskedDotBlocks = 64;
int masked_dot_blocks(long per) { return (int)std::min<long>(((per + 3) / 4 + 255) / 256, kMaskedDotBlocks); }

int launch_masked_dot(const float* a, const float* b, const float* lat, int B, int T, long frame_elems, double* part, int accumulate,
                      double divisor, double* out, hipStream_t s) {
    VD_REQUIRE(a && b && lat && part && out, "masked_dot: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0, "masked_dot: shape");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "masked_dot: an item of fewer than 2^31 elements");
    VD_REQUIRE(divisor > 0.0, "masked_dot: divisor");
    const long per = (long)T * frame_elems;
    const int nblk = masked_dot_blocks(per);
    if (frame_elems % 4 == 0 && al16(a) && al16(b))
        hipLaunchKernelGGL(masked_dot_kernel<true>, dim3(nblk, B), dim3(256), 0, s, a, b, lat, T, (unsigned)frame_elems, part);
    else
        hipLaunchKernelGGL(masked_dot_kernel<false>, dim3(nblk, B), dim3(256), 0, s, a, b, lat, T, (unsigned)frame_elems, part);
    hipLaunchKernelGGL(masked_fold_kernel, dim3((B + 63) / 64), dim3(64), 0, s, part, nblk, B, accumulate, divisor, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ ode_heun_kernel
// Per item b at index t = t[b], with r = TAB_SQRT_ACP and sigma = TAB_SQRT_RECIPM1 at t and t + 1, on the frames with lat == 1, in fp32
// with one rounding per operation and nothing fused:
//   h = 0.5f * (sigma' - sigma)   (the halving is exact),   s = eps + eps2,   q = x / r,   w = q + h * s,   out = r' * w;
// every other frame: out = x, bit for bit.  out may alias x.  An index with t < 0 or t + 1 >= num_timesteps (there is no next level):
// NaN on every element of the item and bit 0 of `err`.  V = 4: 16-byte accesses (frame_elems % 4 == 0 keeps a group in one frame).
template <int V>
__global__ __launch_bounds__(256) void ode_heun_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ eps2,
                                                       const int64_t* __restrict__ t, const float* __restrict__ tab, int NT,
                                                       const float* __restrict__ lat, int T, unsigned fe, float* __restrict__ out,
                                                       int* __restrict__ err) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const unsigned per = (unsigned)T * fe;
    const long long ti = t[b];
    const bool t_ok = ti >= 0 && ti + 1 < NT;
    if (!t_ok && err && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, VD_ERR_TIMESTEP);
    const float r0 = t_ok ? tab[TAB_SQRT_ACP * NT + ti] : 1.f, r1 = t_ok ? tab[TAB_SQRT_ACP * NT + ti + 1] : 1.f;
    const float s0 = t_ok ? tab[TAB_SQRT_RECIPM1 * NT + ti] : 0.f, s1 = t_ok ? tab[TAB_SQRT_RECIPM1 * NT + ti + 1] : 0.f;
    const float h = 0.5f * (s1 - s0);
    const size_t base = (size_t)b * per;
    for (unsigned j = (blockIdx.x * 256 + threadIdx.x) * V; j < per; j += gridDim.x * 256 * V) {
        float xv[V], o[V];
        if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4*>(x + base + j); xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w; }
        else xv[0] = x[base + j];
        if (!t_ok) {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = __builtin_nanf("");
        } else if (lat[(size_t)b * T + j / fe] == 1.0f) {
            float e1[V], e2[V];
            if constexpr (V == 4) {
                const float4 p = *reinterpret_cast<const float4*>(eps + base + j), q = *reinterpret_cast<const float4*>(eps2 + base + j);
                e1[0] = p.x; e1[1] = p.y; e1[2] = p.z; e1[3] = p.w; e2[0] = q.x; e2[1] = q.y; e2[2] = q.z; e2[3] = q.w;
            } else { e1[0] = eps[base + j]; e2[0] = eps2[base + j]; }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float s = e1[k] + e2[k];
                const float q = xv[k] / r0;
                const float w = q + h * s;
                o[k] = r1 * w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = xv[k];
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(out + base + j) = make_float4(o[0], o[1], o[2], o[3]);
        else out[base + j] = o[0];
    }
}

int launch_ode_heun(const float* x, const float* eps, const float* eps2, const int64_t* t, const float* tab, int num_timesteps,
                    const float* lat, int B, int T, long frame_elems, float* out, int* err, hipStream_t s) {
    VD_REQUIRE(x && eps && eps2 && t && tab && lat && out, "ode_heun: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0 && num_timesteps > 0, "ode_heun: shape");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "ode_heun: an item of fewer than 2^31 elements");
    const size_t per = (size_t)T * frame_elems;
    const bool v4 = frame_elems % 4 == 0 && al16(x) && al16(eps) && al16(eps2) && al16(out);
    const unsigned nb = (unsigned)std::min<size_t>((per / (v4 ? 4 : 1) + 255) / 256, std::max<size_t>(4096 / B, 1));
    if (v4) hipLaunchKernelGGL(ode_heun_kernel<4>, dim3(nb, B), dim3(256), 0, s, x, eps, eps2, t, tab, num_timesteps, lat, T, (unsigned)frame_elems, out, err);
    else hipLaunchKernelGGL(ode_heun_kernel<1>, dim3(nb, B), dim3(256), 0, s, x, eps, eps2, t, tab, num_timesteps, lat, T, (unsigned)frame_elems, out, err);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ keep_frames_kernel
// out = x on the frames with lat != 1, untouched elsewhere: behind the Euler move, which deterministic_kernel makes on every frame, the
// frames that are not latent get their bits back (observed and padding frames do not move along the ODE).
template <int V>
__global__ __launch_bounds__(256) void keep_frames_kernel(const float* __restrict__ x, const float* __restrict__ lat, unsigned fe, size_t total,
                                                          float* __restrict__ out) {
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (size_t)gridDim.x * 256 * V) {
        if (lat[i / fe] == 1.0f) continue;
        if constexpr (V == 4) *reinterpret_cast<float4*>(out + i) = *reinterpret_cast<const float4*>(x + i);
        else out[i] = x[i];
    }
}

int launch_keep_frames(const float* x, const float* lat, int B, int T, long frame_elems, float* out, hipStream_t s) {
    VD_REQUIRE(x && lat && out && B > 0 && T > 0 && frame_elems > 0, "keep_frames: arguments");
    const size_t total = (size_t)B * T * frame_elems;
    const bool v4 = frame_elems % 4 == 0 && al16(x) && al16(out);
    const unsigned grid = (unsigned)std::min<size_t>((total / (v4 ? 4 : 1) + 255) / 256, 4096);
    if (v4) hipLaunchKernelGGL(keep_frames_kernel<4>, dim3(grid), dim3(256), 0, s, x, lat, (unsigned)frame_elems, total, out);
    else hipLaunchKernelGGL(keep_frames_kernel<1>, dim3(grid), dim3(256), 0, s, x, lat, (unsigned)frame_elems, total, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ dequantize_kernel
// Uniform dequantisation of 8-bit data on [-1, 1] (bin width 2 / 256): on the frames with lat == 1 out = x + (2 / 256) u with
// u = (w >> 8) * 2^-24 in [0, 1), w = word j & 3 of the Philox block (seed, item_offset[b] + (j >> 2)) for element j of item b -- the block
// element j of vd_randn(., seed, item_offset[b]) reads; one rounded product (exact: a power of two) and one rounded sum.  Other frames:
// the bits of x.  out may alias x.  Element by element: the pass runs once per window.
__global__ __launch_bounds__(256) void dequantize_kernel(const float* __restrict__ x, const float* __restrict__ lat, int T, unsigned fe,
                                                         unsigned long long seed, const unsigned long long* __restrict__ item_offset,
                                                         float* __restrict__ out) {
    const int b = blockIdx.y;
    const unsigned per = (unsigned)T * fe;
    const size_t base = (size_t)b * per;
    const unsigned long long off = item_offset[b];
    for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < per; j += gridDim.x * 256) {
        float v = x[base + j];
        if (lat[(size_t)b * T + j / fe] == 1.0f) {
            unsigned r[4];
            philox4x32_10(off + (j >> 2), seed, r);
            v += 0.0078125f * ((float)(r[j & 3] >> 8) * 5.9604644775390625e-8f);
        }
        out[base + j] = v;
    }
}

int launch_dequantize(const float* x, const float* lat, int B, int T, long frame_elems, unsigned long long seed,
                      const unsigned long long* item_offset, float* out, hipStream_t s) {
    VD_REQUIRE(x && lat && item_offset && out, "dequantize: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0, "dequantize: shape");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "dequantize: an item of fewer than 2^31 elements");
    const size_t per = (size_t)T * frame_elems;
    const unsigned nb = (unsigned)std::min<size_t>((per + 255) / 256, std::max<size_t>(4096 / B, 1));
    hipLaunchKernelGGL(dequantize_kernel, dim3(nb, B), dim3(256), 0, s, x, lat, T, (unsigned)frame_elems, seed, item_offset, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ scale_by_kernel
// out[i] = in[i] * gs[1]: the 1 / s behind a backward pass that ran on s * cotangent (s a power of two: exact unless the result is subnormal)
__global__ __launch_bounds__(256) void scale_by_kernel(const float* __restrict__ in, const float* __restrict__ gs, size_t n, float* __restrict__ out) {
    const float inv_s = gs[1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = in[i] * inv_s;
}

int launch_scale_by(const float* in, const float* gs, size_t n, float* out, hipStream_t s) {
    VD_REQUIRE(in && gs && out && n > 0, "scale_by: arguments");
    hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, in, gs, n, out);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
