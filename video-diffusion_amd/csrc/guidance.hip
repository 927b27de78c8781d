// Guidance rescale and dynamic thresholding (this project's extensions to guided sampling), gfx950, wave64.
// Both need one statistic per batch item over the elements of its LATENT frames (latent_mask == 1) -- two moments for the rescale, two
// exact order statistics for the threshold -- on the device, inside the step, in one stream: no host round trip, no allocation, so the
// passes are captured into window graphs like every other pass of a step.  The tensors are [B][T][frame_elems]; frame_elems % 4 == 0
// with 16-byte aligned tensors takes 16-byte accesses (a group of four then lies inside one frame), anything else runs element by element.
// The workload is tiny beside a UNet forward (1.57 M floats at the headline shape): the passes are written for exactness and
// run-to-run determinism -- fp64 partial sums folded in a fixed order, integer atomics only -- not tuned.
#include <algorithm>

#include "vd_common.h"

namespace vd {

namespace {
constexpr int kGuidMaxBlocks = 64;      // blocks per item at most (grid-stride inside an item)
constexpr int kSelPasses = 4;           // radix select: four 8-bit digits of the 32-bit pattern of |x| (bit 31 is 0)
constexpr int kSelState = 8;            // words per item: prefix[2], rank[2], bad, same, unused[2]

template <int V> __device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
    if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// scratch of one launch_cfg_rescale / launch_dynamic_threshold, carved from one 256-byte aligned region
struct GuidScratch {
    double* part;            // [B][kGuidMaxBlocks][4] rescale: block partials {S1_c, S2_c, S1_g, S2_g}
    float* factor;           // [B]
    float* s;                // [B]
    unsigned* hist;          // [kSelPasses][B][2][256] -- zeroed in the stream, with `state`, before the select
    unsigned* state;         // [B][kSelState]
    size_t zero_bytes;       // hist + state
};
inline size_t r256(size_t n) { return (n + 255) & ~(size_t)255; }
inline GuidScratch carve(void* base, int B) {
    char* p = static_cast<char*>(base);
    GuidScratch g;
    g.part = reinterpret_cast<double*>(p); p += r256((size_t)B * kGuidMaxBlocks * 4 * sizeof(double));
    g.factor = reinterpret_cast<float*>(p); p += r256((size_t)B * sizeof(float));
    g.s = reinterpret_cast<float*>(p); p += r256((size_t)B * sizeof(float));
    g.hist = reinterpret_cast<unsigned*>(p);
    g.state = g.hist + (size_t)kSelPasses * B * 2 * 256;
    g.zero_bytes = ((size_t)kSelPasses * B * 2 * 256 + (size_t)B * kSelState) * sizeof(unsigned);
    return g;
}
inline int item_blocks(long groups) { return (int)std::min<long>(std::max<long>((groups + 255) / 256, 1), kGuidMaxBlocks); }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// first latent frame of item b and the number of its latent frames (thread 0 of a block; T <= a few hundred)
__device__ __forceinline__ void latent_frames(const float* lat, int b, int T, int* first, int* count) {
    int f0 = -1, n = 0;
    for (int k = 0; k < T; ++k)
        if (lat[(size_t)b * T + k] == 1.f) { if (f0 < 0) f0 = k; ++n; }
    *first = f0; *count = n;
}
}  // namespace

size_t guidance_scratch_bytes(int B) {
    const uintptr_t base = 4096;
    GuidScratch g = carve(reinterpret_cast<void*>(base), B);
    return (size_t)(reinterpret_cast<uintptr_t>(g.hist) - base) + r256(g.zero_bytes);
}

// ------------------------------------------------------------------ guidance rescale (Lin et al. 2023, section 3.4), two passes
// Pass 1, combine and moments: g = cfg_combine_one(c, u, w) in registers -- the bits cfg_combine_kernel writes -- and, over the item's
// latent elements, the fp64 sums of (v - v0) and (v - v0)^2 for v = c and v = g, v0 being the item's FIRST latent element of that tensor.
// A difference of two floats is exact in fp64 (or, 2^29 apart and more, far beyond what the sums resolve anyway), so a constant item has
// S1 = S2 = 0 and sigma = 0 exactly, and a mean of 30 spreads costs the variance no digit.  Nothing but the block partials is written,
// so `out` of pass 2 may alias out_c or out_u.  Each thread sums its elements in index order, a wave folds by shuffles, the block's four
// waves through LDS, pass 2 the blocks in index order: the same tree on every run.
template <int V>
__global__ __launch_bounds__(256) void cfg_moments_kernel(const float* out_c, const float* out_u, float w, const float* lat, int T,
                                                          long fe, long per, double* part) {
    __shared__ int f0_s;
    __shared__ double red[4][4];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) { int n; latent_frames(lat, b, T, &f0_s, &n); }
    __syncthreads();
    const int f0 = f0_s;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (f0 >= 0) {
        const float* c = out_c + (size_t)b * per;
        const float* u = out_u + (size_t)b * per;
        const float c0 = c[(size_t)f0 * fe];
        const double kc = (double)c0, kg = (double)cfg_combine_one(c0, u[(size_t)f0 * fe], w);
        const long groups = per / V;
        for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
            const long j = g * V;
            if (lat[(size_t)b * T + j / fe] != 1.f) continue;
            float cv[V], uv[V];
            ldv<V>(c + j, cv);
            ldv<V>(u + j, uv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const double dc = (double)cv[k] - kc, dg = (double)cfg_combine_one(cv[k], uv[k], w) - kg;
                acc[0] += dc; acc[1] += dc * dc; acc[2] += dg; acc[3] += dg * dg;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < 4; ++q) red[threadIdx.x >> 6][q] = acc[q];
    __syncthreads();
    if (threadIdx.x < 4)
        part[((size_t)b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Pass 2, factor and apply: every block folds the item's partials (index order) into
//   var = (S2 - S1^2 / n) / n,  f = 1 + phi (sigma_c / sigma_g - 1)   in fp64, rounded once to fp32;
// f = 1 where sigma_g = 0 or the item has no latent frame (a sigma that is not a number gives f = NaN: the sampler pass behind flags it).
// out = fp32(g * f) on latent frames, g itself on the others.
template <int V>
__global__ __launch_bounds__(256) void cfg_rescale_apply_kernel(const float* out_c, const float* out_u, float w, const float* lat, int T,
                                                                long fe, long per, float phi, const double* part, int nblk, float* out,
                                                                float* factor_out) {
    __shared__ float f_s;
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        int f0, nl;
        latent_frames(lat, b, T, &f0, &nl);
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < nblk; ++k)
            for (int q = 0; q < 4; ++q) S[q] += part[((size_t)b * nblk + k) * 4 + q];
        float f = 1.0f;
        if (nl > 0) {
            const double n = (double)nl * (double)fe;
            const double vc = fmax((S[1] - S[0] * S[0] / n) / n, 0.0), vg = fmax((S[3] - S[2] * S[2] / n) / n, 0.0);
            const double sc = sqrt(vc), sg = sqrt(vg);
            // (fmax drops a NaN operand: take the not-a-number case from the sums themselves)
            if (!(S[1] == S[1]) || !(S[3] == S[3]) || !(S[0] == S[0]) || !(S[2] == S[2])) f = __builtin_nanf("");
            else if (sg != 0.0) f = (float)(1.0 + (double)phi * (sc / sg - 1.0));
        }
        f_s = f;
        if (blockIdx.x == 0 && factor_out) factor_out[b] = f;
    }
    __syncthreads();
    const float f = f_s;
    const float* c = out_c + (size_t)b * per;
    const float* u = out_u + (size_t)b * per;
    float* o = out + (size_t)b * per;
    const long groups = per / V;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long j = g * V;
        const bool latent = lat[(size_t)b * T + j / fe] == 1.f;
        float cv[V], uv[V], ov[V];
        ldv<V>(c + j, cv);
        ldv<V>(u + j, uv);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float gk = cfg_combine_one(cv[k], uv[k], w);
            ov[k] = latent ? gk * f : gk;
        }
        stv<V>(o + j, ov);
    }
}

int launch_cfg_rescale(const float* out_c, const float* out_u, float w, const float* lat, int B, int T, long frame_elems, float phi,
                       float* out, float* factor_out, void* scratch, hipStream_t s) {
    VD_REQUIRE(out_c && out_u && lat && out && scratch, "cfg_rescale: null tensor");
    VD_REQUIRE(B > 0 && B <= 65535 && T > 0 && frame_elems > 0 && (double)T * (double)frame_elems < 2147483648.0, "cfg_rescale: shape");
    VD_REQUIRE(w == w && fabsf(w) <= 3.4028234e38f, "cfg_scale must be finite");
    VD_REQUIRE(phi >= 0.f && phi <= 1.f, "guidance_rescale must lie in [0, 1]");
    const long per = (long)T * frame_elems;
    const bool v4 = frame_elems % 4 == 0 && al16(out_c) && al16(out_u) && al16(out);
    const int nblk = item_blocks(per / (v4 ? 4 : 1));
    GuidScratch g = carve(scratch, B);
    const dim3 grid(nblk, B), blk(256);
    if (v4) {
        hipLaunchKernelGGL(cfg_moments_kernel<4>, grid, blk, 0, s, out_c, out_u, w, lat, T, frame_elems, per, g.part);
        hipLaunchKernelGGL(cfg_rescale_apply_kernel<4>, grid, blk, 0, s, out_c, out_u, w, lat, T, frame_elems, per, phi, g.part, nblk, out, factor_out);
    } else {
        hipLaunchKernelGGL(cfg_moments_kernel<1>, grid, blk, 0, s, out_c, out_u, w, lat, T, frame_elems, per, g.part);
        hipLaunchKernelGGL(cfg_rescale_apply_kernel<1>, grid, blk, 0, s, out_c, out_u, w, lat, T, frame_elems, per, phi, g.part, nblk, out, factor_out);
    }
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ dynamic thresholding (Saharia et al. 2022, section 2.3)
// Per item, over the n elements of its latent frames: a = sorted |x_0|, h = (n - 1) p, s = a[k0] + (h - k0) (a[k1] - a[k0]) with k0 = floor(h),
// k1 = min(k0 + 1, n - 1) (torch.quantile's linear interpolation), s <- max(s, 1), x_0 <- clamp(x_0, -s, s) / s.  a[k0] and a[k1] are EXACT:
// a radix select over the bit patterns of |x_0| (for floats without their sign bit the unsigned order of the patterns is the order of
// the values, zeros and denormals included), most significant 8-bit digit first.  Per pass: a histogram of the digit over the elements
// whose higher digits equal the prefix found so far (LDS integer atomics per block, then one global integer atomic per non-empty bin;
// integer sums do not depend on the order of arrival), then one small block per item walks the 256 bins, appends the digit that holds
// the rank to the prefix and rebases the rank.  The two ranks are neighbours and nearly always share their prefix: while they do, one
// histogram serves both (state word `same`).  Counters and state are zeroed in the stream in front of the first pass, by a kernel.
//
// x_0 pass (and the first histogram: no prefix yet).  src is the network output: with x != null an epsilon-model's, x_0 formed as the
// sampler passes form it (xstart_from_eps: two rounded products, one subtraction); with x == null the x_0 prediction itself.  An index t
// outside the schedule reads no table and leaves 0: the sampler pass behind poisons that item.  A latent x_0 that is not finite marks
// the item (state word `bad`).
// The counters and the state of one select, zeroed by a kernel: a captured step stays kernel nodes only.  (With hipMemsetAsync here the
// window graph held a memset node, and its replays left every latent frame poisoned -- the `bad` word read as set -- whenever another
// window graph had been instantiated before this one; the eager step and a first graph were right.  ROCm 7; not pursued further.)
__global__ __launch_bounds__(256) void dt_zero_kernel(unsigned* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

template <int V>
__global__ __launch_bounds__(256) void dt_xstart_kernel(const float* src, const float* x, const int64_t* t, const float* tab, int NT,
                                                        const float* lat, int T, long fe, long per, float* x0, unsigned* hist,
                                                        unsigned* state) {
    __shared__ unsigned lh[256];
    const int b = blockIdx.y;
    lh[threadIdx.x] = 0;
    __syncthreads();
    float sr = 1.f, srm1 = 0.f;
    bool t_ok = true;
    if (x) {
        const long long tl = t[b];
        t_ok = tl >= 0 && tl < NT;
        if (t_ok) { sr = tab[TAB_SQRT_RECIP * NT + (int)tl]; srm1 = tab[TAB_SQRT_RECIPM1 * NT + (int)tl]; }
    }
    const size_t base = (size_t)b * per;
    const long groups = per / V;
    bool bad = false;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long j = g * V;
        const bool latent = lat[(size_t)b * T + j / fe] == 1.f;
        float sv[V], xv[V], ov[V];
        ldv<V>(src + base + j, sv);
        if (x) ldv<V>(x + base + j, xv);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float v = !x ? sv[k] : (t_ok ? xstart_from_eps(sr, xv[k], srm1, sv[k]) : 0.f);
            ov[k] = v;
            if (latent) {
                const unsigned bits = __float_as_uint(v) & 0x7fffffffu;
                bad |= bits >= 0x7f800000u;
                atomicAdd(&lh[bits >> 24], 1u);
            }
        }
        stv<V>(x0 + base + j, ov);
    }
    __syncthreads();
    const unsigned cnt = lh[threadIdx.x];
    if (cnt) atomicAdd(&hist[((size_t)b * 2 + 0) * 256 + threadIdx.x], cnt);
    if (bad) atomicOr(&state[(size_t)b * kSelState + 4], 1u);
}

// histogram of digit `pass` (1..3) over the latent elements whose higher digits equal prefix[r]
template <int V>
__global__ __launch_bounds__(256) void dt_hist_kernel(const float* x0, const float* lat, int T, long fe, long per, int pass,
                                                      unsigned* hist, const unsigned* state) {
    __shared__ unsigned lh[2][256];
    const int b = blockIdx.y;
    lh[0][threadIdx.x] = 0; lh[1][threadIdx.x] = 0;
    __syncthreads();
    const unsigned* st = state + (size_t)b * kSelState;
    const unsigned p0 = st[0], p1 = st[1];
    const bool same = st[5] != 0;
    const int shift = 24 - 8 * pass;
    const unsigned himask = ~0u << (shift + 8);
    const size_t base = (size_t)b * per;
    const long groups = per / V;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long j = g * V;
        if (lat[(size_t)b * T + j / fe] != 1.f) continue;
        float v[V];
        ldv<V>(x0 + base + j, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const unsigned bits = __float_as_uint(v[k]) & 0x7fffffffu;
            const unsigned d = (bits >> shift) & 255u;
            if ((bits & himask) == p0) atomicAdd(&lh[0][d], 1u);
            if (!same && (bits & himask) == p1) atomicAdd(&lh[1][d], 1u);
        }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
        const unsigned cnt = lh[r][threadIdx.x];
        if (cnt) atomicAdd(&hist[((size_t)b * 2 + r) * 256 + threadIdx.x], cnt);
    }
}

// One block per item: the digit of pass `pass` for both ranks.  Pass 0 first derives the ranks from the mask and p; the last pass ends in
// s (fp64, the interpolation as three separately rounded operations -- no fused multiply-add, so that a host restatement in fp64 gets
// the same bits -- rounded once to fp32, then max(s, 1); NaN for a marked item; 1 for an item without latent frame).
__global__ __launch_bounds__(256) void dt_scan_kernel(const unsigned* hist, unsigned* state, const float* lat, int T, long fe, float p,
                                                      int pass, float* s_out) {
    __shared__ unsigned h[2][256];
    const int b = blockIdx.x;
    unsigned* st = state + (size_t)b * kSelState;
    h[0][threadIdx.x] = hist[((size_t)b * 2 + 0) * 256 + threadIdx.x];
    h[1][threadIdx.x] = hist[((size_t)b * 2 + 1) * 256 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    int f0, nl;
    latent_frames(lat, b, T, &f0, &nl);
    if (nl == 0) { if (pass == kSelPasses - 1) s_out[b] = 1.0f; return; }
    const unsigned n = (unsigned)nl * (unsigned)fe;
    const double hq = (double)(n - 1) * (double)p;
    const unsigned k0 = (unsigned)floor(hq);
    unsigned prefix[2], rank[2];
    bool same = true;
    if (pass == 0) { prefix[0] = prefix[1] = 0; rank[0] = k0; rank[1] = k0 + 1 < n ? k0 + 1 : n - 1; }
    else { prefix[0] = st[0]; prefix[1] = st[1]; rank[0] = st[2]; rank[1] = st[3]; same = st[5] != 0; }
    const int shift = 24 - 8 * pass;
    for (int r = 0; r < 2; ++r) {
        const unsigned* hr = h[same ? 0 : r];
        unsigned cum = 0, d = 0;
        for (; d < 255; ++d) {
            const unsigned c = hr[d];
            if (rank[r] < cum + c) break;
            cum += c;
        }
        rank[r] -= cum;
        prefix[r] |= d << shift;
    }
    st[0] = prefix[0]; st[1] = prefix[1]; st[2] = rank[0]; st[3] = rank[1];
    st[5] = prefix[0] == prefix[1] ? 1u : 0u;
    if (pass == kSelPasses - 1) {
        float s;
        if (st[4]) s = __builtin_nanf("");
        else {
            const double a0 = (double)__uint_as_float(prefix[0]), a1 = (double)__uint_as_float(prefix[1]);
            const double s64 = __dadd_rn(a0, __dmul_rn(hq - (double)k0, __dsub_rn(a1, a0)));
            s = fmaxf((float)s64, 1.0f);
        }
        s_out[b] = s;
    }
}

// latent frames: clamp(x_0, -s, s) / s, NaN for a marked item (with bit 1 of the error word); other frames: the static clamp as the sampler
// passes apply it (a value that is not finite stays as it is: the pass behind deals with it as it always did).  s = 1 is the static clamp
// to the bit: a division by 1 is exact.
template <int V>
__global__ __launch_bounds__(256) void dt_apply_kernel(float* x0, const float* lat, int T, long fe, long per, const float* s_in,
                                                       const unsigned* state, int* err) {
    const int b = blockIdx.y;
    const float s = s_in[b];
    const bool bad = state[(size_t)b * kSelState + 4] != 0;
    if (bad && err && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, VD_ERR_NONFINITE);
    const size_t base = (size_t)b * per;
    const long groups = per / V;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long j = g * V;
        const bool latent = lat[(size_t)b * T + j / fe] == 1.f;
        float v[V];
        ldv<V>(x0 + base + j, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (latent) v[k] = bad ? __builtin_nanf("") : fminf(fmaxf(v[k], -s), s) / s;
            else if (fabsf(v[k]) <= 3.4028234e38f) v[k] = fminf(fmaxf(v[k], -1.0f), 1.0f);
        }
        stv<V>(x0 + base + j, v);
    }
}

int launch_dynamic_threshold(const DynThreshArgs& a, hipStream_t s) {
    VD_REQUIRE(a.src && a.lat && a.out && a.scratch && (!a.x || (a.t && a.tab && a.num_timesteps > 0)), "dynamic_threshold: null tensor");
    VD_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.frame_elems > 0 && (double)a.T * (double)a.frame_elems < 2147483648.0,
               "dynamic_threshold: shape");
    VD_REQUIRE(a.p > 0.f && a.p <= 1.f, "dynamic_threshold must lie in (0, 1]");
    const long fe = a.frame_elems, per = (long)a.T * fe;
    const bool v4 = fe % 4 == 0 && al16(a.src) && al16(a.x) && al16(a.out);
    const int nblk = item_blocks(per / (v4 ? 4 : 1));
    GuidScratch g = carve(a.scratch, a.B);
    float* s_buf = a.s_out ? a.s_out : g.s;
    const dim3 grid(nblk, a.B), blk(256);
    const size_t hp = (size_t)a.B * 2 * 256;            // one pass' histograms
    hipLaunchKernelGGL(dt_zero_kernel, dim3((unsigned)std::min<size_t>((g.zero_bytes / 4 + 255) / 256, 1024)), blk, 0, s, g.hist, g.zero_bytes / 4);
    if (v4) hipLaunchKernelGGL(dt_xstart_kernel<4>, grid, blk, 0, s, a.src, a.x, a.t, a.tab, a.num_timesteps, a.lat, a.T, fe, per, a.out, g.hist, g.state);
    else hipLaunchKernelGGL(dt_xstart_kernel<1>, grid, blk, 0, s, a.src, a.x, a.t, a.tab, a.num_timesteps, a.lat, a.T, fe, per, a.out, g.hist, g.state);
    for (int pass = 0; pass < kSelPasses; ++pass) {
        if (pass > 0) {
            if (v4) hipLaunchKernelGGL(dt_hist_kernel<4>, grid, blk, 0, s, a.out, a.lat, a.T, fe, per, pass, g.hist + pass * hp, g.state);
            else hipLaunchKernelGGL(dt_hist_kernel<1>, grid, blk, 0, s, a.out, a.lat, a.T, fe, per, pass, g.hist + pass * hp, g.state);
        }
        hipLaunchKernelGGL(dt_scan_kernel, dim3(a.B), blk, 0, s, g.hist + pass * hp, g.state, a.lat, a.T, fe, a.p, pass, s_buf);
    }
    if (v4) hipLaunchKernelGGL(dt_apply_kernel<4>, grid, blk, 0, s, a.out, a.lat, a.T, fe, per, s_buf, g.state, a.err);
    else hipLaunchKernelGGL(dt_apply_kernel<1>, grid, blk, 0, s, a.out, a.lat, a.T, fe, per, s_buf, g.state, a.err);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
