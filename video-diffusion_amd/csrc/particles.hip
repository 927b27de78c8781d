// Particle steering (this project's extension; Feynman-Kac steering, Singhal et al. 2025; the twisted diffusion sampler of Wu et al. 2023
// without its gradient proposal): sequential Monte Carlo over the reverse chain.  B = G*K items, item g*K + k is particle k of group g.
// Two passes behind a step:
//   particle_weights_kernel   per group: the weight update from the items' rewards, the effective sample size, and -- when the weights
//                             have degenerated -- the ancestors of a systematic resampling; at t == 0 the pick of one particle;
//   particle_gather_kernel    item i of up to four tensors takes the content of item ancestors[i].
// No floating-point atomics; every sum runs in index order in fp64, so a group's numbers do not depend on G or on the run.
#include "vd_common.h"
#include <algorithm>
#include <cmath>

namespace vd {

// ------------------------------------------------------------------ particle_weights_kernel
// One block per group, thread k owns particle k (K <= 256).  The reward of item b: rewards[b], or from the nblk fp64 partials of the
// residual pass (dps.hip) folded in index order, r = -(sum * inv_two_var).  Then, with -inf absorbing (a particle whose reward or
// log-weight is -inf stays at -inf):
//   logw_k += lambda (r_k - rprev_k), rprev_k = r_k;  m = max logw;  p_k = exp(logw_k - m) / sum_j exp(logw_j - m);  ESS = 1 / sum p_k^2;
//   c_k = sum_{j <= k} p_j, and c_k = 1 from the last k with p_k > 0 on.
// m == -inf: the group is left as it is (identity ancestors, ESS 0, chosen 0 at t == 0) and its `degenerate` counter goes up.
// All logw bit-equal, or t == 0, or ESS >= tau K: identity ancestors.  Otherwise a_i = min{k : c_k > (u + i) / K} (the last k with
// p_k > 0 when (u + i) / K rounds to 1), ancestors[g K + i] = g K + a_i, rprev_i = rprev_{a_i}, logw_i = 0, the `resamples` counter goes up.
// t == 0 (t[g K], the group's index): chosen[g] = min{k : c_k > u2}; otherwise -1.  u = uni[2 g], u2 = uni[2 g + 1], both in [0, 1); without
// `uni` they are the two 53-bit halves of Philox block (seed, offset + pos + g) -- pos = 3/4 of a step's range, which no other draw of a
// step uses (include/vd_amd.h).
// The sequential sums are thread 0's, over one LDS array: four waves hold a group of 256, a shuffle does not cross them.
__device__ __forceinline__ double uniform53(unsigned hi, unsigned lo) {      // [0, 1): 27 bits of hi above 26 bits of lo, times 2^-53
    return (double)(((unsigned long long)(hi >> 5) << 26) | (unsigned long long)(lo >> 6)) * 1.1102230246251565e-16;
}

__global__ __launch_bounds__(256) void particle_weights_kernel(ParticleArgs a) {
#pragma clang fp contract(off)                                     // one rounding per operation: everything but exp matches IEEE fp64 step by step
    __shared__ double sh[256];
    __shared__ double shr[256];
    __shared__ double s_m, s_tot;
    __shared__ int s_eq, s_resample, s_last;
    __shared__ double s_u[2];
    const int g = blockIdx.x, k = threadIdx.x, K = a.K;
    const size_t b = (size_t)g * K + (k < K ? k : 0);
    const double ninf = -__builtin_inf();
    const bool final_step = a.t[(size_t)g * K] == 0;
    double lw = ninf, r = ninf;
    if (k < K) {
        if (a.rewards) r = a.rewards[b];
        else {
            double s = 0.0;
            for (int j = 0; j < a.nblk; ++j) s += a.part[b * a.nblk + j];
            r = -(s * a.inv_two_var);
        }
        lw = a.logw[b];
        if (r == ninf || lw == ninf) lw = ninf;
        else lw += a.lambda * (r - a.rprev[b]);
        sh[k] = lw;
        shr[k] = r;
    }
    if (k == 0) {
        if (a.uni) { s_u[0] = a.uni[2 * g]; s_u[1] = a.uni[2 * g + 1]; }
        else {
            unsigned w[4];
            philox4x32_10((a.dstate ? a.dstate[1] : a.offset) + a.pos + (unsigned long long)g, a.dstate ? a.dstate[0] : a.seed, w);
            s_u[0] = uniform53(w[0], w[1]);
            s_u[1] = uniform53(w[2], w[3]);
        }
    }
    __syncthreads();
    if (k == 0) {
        double m = sh[0];
        int eq = 1;
        const long long first = __double_as_longlong(sh[0]);
        for (int j = 1; j < K; ++j) {
            m = sh[j] > m ? sh[j] : m;
            eq &= __double_as_longlong(sh[j]) == first;
        }
        s_m = m; s_eq = eq;
    }
    __syncthreads();
    const double m = s_m;
    if (m == ninf) {                                               // (uniform over the block)
        if (k < K) { a.logw[b] = lw; a.rprev[b] = r; a.ancestors[b] = (int)b; }
        if (k == 0) { a.ess[g] = 0.0; a.chosen[g] = final_step ? 0 : -1; a.counters[2 * g + 1] += 1; }
        return;
    }
    const double e = k < K ? exp(lw - m) : 0.0;
    if (k < K) sh[k] = e;
    __syncthreads();
    if (k == 0) {
        double tot = 0.0;
        for (int j = 0; j < K; ++j) tot += sh[j];
        s_tot = tot;
    }
    __syncthreads();
    const double p = e / s_tot;
    if (k < K) sh[k] = p;
    __syncthreads();
    if (k == 0) {
        double s2 = 0.0, c = 0.0;
        int last = 0;
        for (int j = 0; j < K; ++j) { s2 += sh[j] * sh[j]; if (sh[j] > 0.0) last = j; }
        const double ess = 1.0 / s2;
        for (int j = 0; j < K; ++j) { c += sh[j]; sh[j] = j >= last ? 1.0 : c; }
        a.ess[g] = ess;
        s_last = last;
        s_resample = !s_eq && !final_step && ess < a.tau * (double)K;
        int ch = -1;
        if (final_step) {
            const double u2 = s_u[1];
            ch = last;
            for (int j = 0; j < K; ++j) if (sh[j] > u2) { ch = j; break; }
        }
        a.chosen[g] = ch;
        if (s_resample) a.counters[2 * g] += 1;
    }
    __syncthreads();
    if (k >= K) return;
    if (!s_resample) { a.logw[b] = lw; a.rprev[b] = r; a.ancestors[b] = (int)b; return; }
    const double thr = (s_u[0] + (double)k) / (double)K;
    int anc = s_last;
    for (int j = 0; j < K; ++j) if (sh[j] > thr) { anc = j; break; }
    a.logw[b] = 0.0;
    a.rprev[b] = shr[anc];
    a.ancestors[b] = g * K + anc;
}

int launch_particle_weights(const ParticleArgs& a, hipStream_t s) {
    VD_REQUIRE(a.G > 0 && a.K >= 1 && a.K <= kMaxParticles, "particle_weights: K particles per group, 1 <= K <= 256");
    VD_REQUIRE((double)a.G * a.K < 2147483648.0, "particle_weights: fewer than 2^31 items");
    VD_REQUIRE((a.rewards != nullptr) != (a.part != nullptr), "particle_weights: the rewards, or the partials of the residual pass");
    VD_REQUIRE(a.rewards || a.nblk > 0, "particle_weights: partials per item");
    VD_REQUIRE(a.t && a.logw && a.rprev && a.ancestors && a.chosen && a.ess && a.counters, "particle_weights: null tensor");
    VD_REQUIRE(a.lambda >= 0.0 && a.lambda <= 1.7976931348623157e308, "particle_weights: lambda must be finite and not negative");
    VD_REQUIRE(a.tau >= 0.0 && a.tau <= 1.0, "particle_weights: ess_threshold must lie in [0, 1]");
    hipLaunchKernelGGL(particle_weights_kernel, dim3(a.G), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ particle_gather_kernel
// Item i of each tensor takes the content of item anc[i]; blockIdx.y is the tensor.  A thread owns one column -- V consecutive floats at
// the same offset of every item -- and nobody else touches it, so one launch serves any map, cycles included, without a grid-wide wait:
// first the moved items whose source is itself overwritten (anc[anc[i]] != anc[i]) are copied into `scratch`, then every moved item is
// written, from its source where that keeps its content, else from the scratch copy the same thread made.  An item with anc[i] == i (or
// an index outside [0, B), which the launcher's callers never produce) is neither read nor written; a launch in which nothing moves
// reads the B indices and ends.
template <int V>
__global__ __launch_bounds__(256) void particle_gather_kernel(GatherArgs a) {
    const int B = a.B;
    int moved = 0;
    for (int i = threadIdx.x; i < B; i += 256) moved |= a.anc[i] != i;
    if (!__syncthreads_or(moved)) return;
    float* x = a.x[blockIdx.y];
    float* sc = a.scratch + (size_t)blockIdx.y * B * a.per;
    const size_t per = (size_t)a.per;
    for (size_t col = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; col < per; col += (size_t)gridDim.x * 256 * V) {
        for (int i = 0; i < B; ++i) {
            const int s = a.anc[i];
            if (s == i || (unsigned)s >= (unsigned)B || a.anc[s] == s) continue;
            if (V == 4) *reinterpret_cast<float4*>(sc + i * per + col) = *reinterpret_cast<const float4*>(x + s * per + col);
            else sc[i * per + col] = x[s * per + col];
        }
        for (int i = 0; i < B; ++i) {
            const int s = a.anc[i];
            if (s == i || (unsigned)s >= (unsigned)B) continue;
            const float* src = a.anc[s] == s ? x + s * per : sc + i * per;
            if (V == 4) *reinterpret_cast<float4*>(x + i * per + col) = *reinterpret_cast<const float4*>(src + col);
            else x[i * per + col] = src[col];
        }
    }
}

int launch_particle_gather(const GatherArgs& a, hipStream_t s) {
    VD_REQUIRE(a.n >= 1 && a.n <= 4 && a.B > 0 && a.per > 0 && a.anc && a.scratch, "particle_gather: 1..4 tensors of B items of `per` floats");
    bool v4 = a.per % 4 == 0 && (reinterpret_cast<uintptr_t>(a.scratch) & 15) == 0;
    for (int k = 0; k < a.n; ++k) {
        VD_REQUIRE(a.x[k], "particle_gather: null tensor");
        v4 = v4 && (reinterpret_cast<uintptr_t>(a.x[k]) & 15) == 0;
    }
    const size_t cols = v4 ? (size_t)a.per / 4 : (size_t)a.per;
    const unsigned grid = (unsigned)std::min<size_t>((cols + 255) / 256, 2048);
    if (v4) hipLaunchKernelGGL(particle_gather_kernel<4>, dim3(grid, a.n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(particle_gather_kernel<1>, dim3(grid, a.n), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
