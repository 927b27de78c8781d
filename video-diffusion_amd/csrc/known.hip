// Pixel-mask inpainting (this project's extension; RePaint, Lugmayr et al. 2022): the merge pass that closes a step while a known region
// is set, and the forward jump x_{t-1} -> x_t of the resampling walk.  Both are elementwise streaming passes over [B][T][3][hw] tensors.
#include "vd_common.h"
#include <algorithm>

namespace vd {

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------ known_merge_kernel
// W = 4: a thread owns four consecutive elements, which lie in one channel plane of one frame (hw % 4 == 0) and share one Philox block
// (element index % 4 == 0); W = 1: element by element.  The mask is read first: a group without a known pixel, or in a frame that is not
// latent, reads no known_src, draws nothing and writes nothing -- `sample` keeps its bits there.
template <int W>
__global__ __launch_bounds__(256) void known_merge_kernel(KnownMergeArgs a) {
    const size_t hw = (size_t)a.hw, fr = 3 * hw, per = (size_t)a.T * fr, total = (size_t)a.B * per;
    if (a.dstate) { a.seed = a.dstate[0]; a.offset = a.dstate[1]; }
    const unsigned long long off = a.offset + (unsigned long long)(total / 4);
    const int NT = a.num_timesteps;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total / W; g += (size_t)gridDim.x * 256) {
        const size_t i = g * W, frame = i / fr, pix = i % hw;
        const long long t = a.t[i / per];
        if (t < 0 || t >= NT) {                              // the sampler pass poisoned the item already: the known pixels follow
#pragma unroll
            for (int e = 0; e < W; ++e) a.sample[i + e] = __builtin_nanf("");
            continue;
        }
        if (a.lat[frame] != 1.0f) continue;
        float m[W], k[W], z[W], o[W];
        bool any = false;
        if (W == 4) *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(a.known_mask + frame * hw + pix);
        else m[0] = a.known_mask[frame * hw + pix];
#pragma unroll
        for (int e = 0; e < W; ++e) any |= m[e] != 0.0f;
        if (!any) continue;
        if (W == 4) {
            *reinterpret_cast<float4*>(k) = *reinterpret_cast<const float4*>(a.known_src + i);
            *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(a.sample + i);
        } else { k[0] = a.known_src[i]; o[0] = a.sample[i]; }
        if (t >= 1) {
            if (a.noise) {
                if (W == 4) *reinterpret_cast<float4*>(z) = *reinterpret_cast<const float4*>(a.noise + i);
                else z[0] = a.noise[i];
            } else if (W == 4) {
                const f32x4 n4 = normal4_at(a.seed, off, (unsigned long long)g);
#pragma unroll
                for (int e = 0; e < W; ++e) z[e] = n4[e];
            } else z[0] = normal_at(a.seed, off, (unsigned long long)i);
            const float sa = a.tab[TAB_SQRT_ACP * NT + (t - 1)], s1 = a.tab[TAB_SQRT_1M_ACP * NT + (t - 1)];
#pragma unroll
            for (int e = 0; e < W; ++e) if (m[e] != 0.0f) o[e] = fmaf(s1, z[e], sa * k[e]);       // q_sample_kernel's rounding order
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) if (m[e] != 0.0f) o[e] = k[e];                            // t == 0: the source itself
        }
        if (W == 4) *reinterpret_cast<float4*>(a.sample + i) = *reinterpret_cast<const float4*>(o);
        else a.sample[i] = o[0];
    }
}

int launch_known_merge(const KnownMergeArgs& a, hipStream_t s) {
    VD_REQUIRE(a.sample && a.known_src && a.known_mask && a.lat && a.t && a.tab, "known_merge_kernel: null tensor");
    VD_REQUIRE(a.B > 0 && a.T > 0 && a.hw > 0 && a.num_timesteps > 0, "known_merge_kernel: shape");
    const size_t total = (size_t)a.B * a.T * 3 * a.hw;
    const bool v4 = a.hw % 4 == 0 && al16(a.sample) && al16(a.known_src) && al16(a.known_mask) && al16(a.noise);
    const size_t groups = v4 ? total / 4 : total;
    const int grid = (int)std::min<size_t>((groups + 255) / 256, 4096);
    if (v4) hipLaunchKernelGGL(known_merge_kernel<4>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(known_merge_kernel<1>, dim3(grid), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ q_jump_kernel
// x_t = sqrt(1 - beta_t) x_{t-1} + sqrt(beta_t) z on the latent frames (all pixels); the two coefficients come from rows of their own:
// 1 - alpha_t in fp32 would lose three digits at beta = 1e-4.  In place, a frame that is not latent is not written.
template <int W>
__global__ __launch_bounds__(256) void q_jump_kernel(QJumpArgs a) {
    const size_t fr = 3 * (size_t)a.hw, per = (size_t)a.T * fr, total = (size_t)a.B * per;
    if (a.dstate) { a.seed = a.dstate[0]; a.offset = a.dstate[1]; }
    const int NT = a.num_timesteps;
    const bool inplace = a.out == a.x;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total / W; g += (size_t)gridDim.x * 256) {
        const size_t i = g * W;
        const long long t = a.t[i / per];
        float x[W], z[W], o[W];
        if (t < 0 || t >= NT) {
#pragma unroll
            for (int e = 0; e < W; ++e) a.out[i + e] = __builtin_nanf("");
            continue;
        }
        const bool lat = a.lat[i / fr] == 1.0f;
        if (!lat && inplace) continue;
        if (W == 4) *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(a.x + i);
        else x[0] = a.x[i];
        if (lat) {
            if (a.noise) {
                if (W == 4) *reinterpret_cast<float4*>(z) = *reinterpret_cast<const float4*>(a.noise + i);
                else z[0] = a.noise[i];
            } else if (W == 4) {
                const f32x4 n4 = normal4_at(a.seed, a.offset, (unsigned long long)g);
#pragma unroll
                for (int e = 0; e < W; ++e) z[e] = n4[e];
            } else z[0] = normal_at(a.seed, a.offset, (unsigned long long)i);
            const float sa = a.rows[t], sb = a.rows[NT + t];
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = fmaf(sb, z[e], sa * x[e]);
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = x[e];
        }
        if (W == 4) *reinterpret_cast<float4*>(a.out + i) = *reinterpret_cast<const float4*>(o);
        else a.out[i] = o[0];
    }
}

int launch_q_jump(const QJumpArgs& a, hipStream_t s) {
    VD_REQUIRE(a.x && a.out && a.lat && a.t && a.rows, "q_jump_kernel: null tensor");
    VD_REQUIRE(a.B > 0 && a.T > 0 && a.hw > 0 && a.num_timesteps > 0, "q_jump_kernel: shape");
    const size_t total = (size_t)a.B * a.T * 3 * a.hw;
    const bool v4 = (3 * a.hw) % 4 == 0 && al16(a.x) && al16(a.out) && al16(a.noise);      // a group stays inside one frame
    const size_t groups = v4 ? total / 4 : total;
    const int grid = (int)std::min<size_t>((groups + 255) / 256, 4096);
    if (v4) hipLaunchKernelGGL(q_jump_kernel<4>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(q_jump_kernel<1>, dim3(grid), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
