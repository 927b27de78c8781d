// Temporal self-attention for long windows, 33 <= T <= 128 frames: the operator of attn_temporal.hip
// (RPEAttention._forward, unet.py:486-536; RPE.forward_qk / forward_v, unet.py:357-378)
//
//   w[t,s] = q't.(ks + Rk[t,s]) + scale*ks.Rq[s,t]      q' = q*scale
//   w -= inf where the frame mask forbids (t,s)          (unet.py:511-524)
//   o[t] = sum_s softmax_s(w)[t,s] * (vs + Rv[t,s])
//
// The T <= 32 kernels keep a pixel's whole T x T score image in LDS; at T = 64 that no longer fits.  Here a block owns ONE
// query tile of 16 frames and walks the keys in tiles of 16 with an online softmax: per (pixel, query frame) a running
// maximum m and sum l, and accumulators rescaled by exp(m_old - m_new) whenever the maximum grows.  A key tile that is masked
// for a whole row (>= 16 padding frames with allow_interactions_between_padding=False) leaves m = -inf: such a tile
// contributes p = 0 and alpha = 1 instead of exp(-inf - -inf).  Every row has at least one allowed key (t itself, or a frame
// of its own kind), so l > 0 at the end.  fp32 operands and fp32 accumulation whatever VD_MATH says.
#include "vd_common.h"

namespace vd {

namespace {

__device__ __forceinline__ f32x4 mfma_l(float x, float y, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0); }

// X[a] (register a, lane row c) -> X[c] (register c, lane row a): rows of 16 lanes
__device__ __forceinline__ void rows_regs_transpose_l(float& x0, float& x1, float& x2, float& x3) {
    auto u = [](float f) { return __builtin_bit_cast(unsigned, f); };
    auto f = [](unsigned v) { return __builtin_bit_cast(float, v); };
    auto p01 = __builtin_amdgcn_permlane16_swap(u(x0), u(x1), false, false);
    auto p23 = __builtin_amdgcn_permlane16_swap(u(x2), u(x3), false, false);
    auto q02 = __builtin_amdgcn_permlane32_swap(p01[0], p23[0], false, false);
    auto q13 = __builtin_amdgcn_permlane32_swap(p01[1], p23[1], false, false);
    x0 = f(q02[0]); x2 = f(q02[1]); x1 = f(q13[0]); x3 = f(q13[1]);
}

__device__ __forceinline__ bool frame_pair_allowed(const AttnTemporalArgs& a, int b, int t, int s) {
    if (!a.mask) return true;
    const float mt = a.mask[b * a.T + t], ms = a.mask[b * a.T + s];
    float allowed = mt * ms;
    if (a.allow_pad) allowed += (1.f - mt) * (1.f - ms);
    else if (t == s) allowed = 1.f;
    return allowed != 0.f;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// Matrix-pipe kernel (pixels % 16 == 0, head dim F = 16*NJ <= 128).  Block = 16 pixels x one query tile (16 frames) of one
// (batch, head); eight waves.  The GEMM layouts are those of attn_temporal_mfma_kernel with the key range cut to one tile:
//
//   S1  wave w: q' k^T of pixels 2w, 2w+1 (M = t, N = s)                            -> LDS s1[px][t][s]
//   S2  wave w: query frames w, w+8 of the tile: q'.Rk with M = px, N = s           -> LDS s2[px][t][s]
//   S3  wave w: key frames w, w+8 of the tile: k.Rq' with M = px, N = t             -> LDS s3[px][t][s]
//   softmax step, one (px, t) row per thread: w = s1 + s2 + s3, mask, running max / sum, p and the rescale factor -> LDS
//   V   wave w (< NJ): features 16w..16w+15.  One accumulator per query frame (M = px, N = f), rescaled by alpha, then
//       + a Rv of the tile (M = px), then + a v of the tile, which is a per-pixel product (M = t, N = f): its image is turned
//       into the accumulator layout by 4x4 transposes between lane rows and registers (v_permlane16_swap + permlane32_swap).
//
// At the end the accumulators are divided by l and written (64-byte runs).  Frames past T are clamped on load; keys past T carry p = 0, queries past T are not
// written.  Two barriers per key tile: the softmax step reads what every wave's S step wrote, and the V step reads its p.
// ---------------------------------------------------------------------------------------------------------------------
template <int NJ, bool RPE>
__global__ __launch_bounds__(512, 2) void attn_temporal_long_mfma_kernel(AttnTemporalArgs a) {
    constexpr int RS = 17, PS = 16 * RS;                   // score tile [16 px][16 t][RS]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* pb = smem;                                      // p of the current key tile
    float* al = pb + 16 * PS;                              // [px][t] rescale factor, at the end 1/l
    float* s1 = al + 256;
    float* s2 = s1 + 16 * PS;                              // (RPE only)
    float* s3 = s2 + 16 * PS;
    const int T = a.T, C = a.C, HW = a.HW, C3 = 3 * a.C, F = 16 * NJ;
    const int NQ = (T + 15) >> 4;
    const int b = blockIdx.z / NQ, t0 = 16 * (blockIdx.z - b * NQ), h = blockIdx.y, p0 = blockIdx.x * 16;
    const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, i16 = l & 15, g = l >> 4;
    const float* qb = a.qkv + ((size_t)b * T * HW + p0) * C3 + h * F;
    auto row = [&](int t, int px) { return qb + ((size_t)t * HW + px) * C3; };       // q at +0, k at +C, v at +2C
    auto ld4 = [](const float* p) { return *reinterpret_cast<const f32x4*>(p); };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const size_t rbase = (size_t)b * T * T * C + h * F;                              // + (i*T + j)*C: R[b][i][j][h*F ..]
    const int tq = min(t0 + i16, T - 1);                                             // this lane's query frame (S1 rows, S3 columns)

    f32x4 acc[16];                                         // o of query frame t0 + tile: (px = 4g + r, f = i16), unnormalised
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = zero4;
    float m_run = -INFINITY, l_run = 0.f;                  // softmax state of row tid (tid < 256: px = tid / 16, t = t0 + tid % 16)

    const int NK = (T + 15) >> 4;
#pragma unroll 1
    for (int kt = 0; kt < NK; ++kt) {
        const int s0 = 16 * kt;
        const int sk = min(s0 + i16, T - 1);                                         // this lane's key frame (S1, S2 columns)
        // ---- S: the three score terms of the tile, one walk over the features
        f32x4 a1[2], a2[2], a3[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) { a1[u] = zero4; a2[u] = zero4; a3[u] = zero4; }
        const int tf[2] = {min(t0 + wv, T - 1), min(t0 + wv + 8, T - 1)};          // S2: query frames of this wave
        const int sf[2] = {min(s0 + wv, T - 1), min(s0 + wv + 8, T - 1)};          // S3: key frames of this wave
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int fo = 16 * j + 4 * g;
            f32x4 qa[2], kb[2], x2[2], r2[2], x3[2], r3[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                qa[u] = ld4(row(tq, 2 * wv + u) + fo);
                kb[u] = ld4(row(sk, 2 * wv + u) + C + fo);
                if constexpr (RPE) {
                    x2[u] = ld4(row(tf[u], i16) + fo);
                    r2[u] = ld4(a.Rk + rbase + ((size_t)tf[u] * T + sk) * C + fo);
                    x3[u] = ld4(row(sf[u], i16) + C + fo);
                    r3[u] = ld4(a.Rq + rbase + ((size_t)sf[u] * T + tq) * C + fo);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    a1[u] = mfma_l(qa[u][e] * a.scale, kb[u][e], a1[u]);
                    if constexpr (RPE) {
                        a2[u] = mfma_l(x2[u][e] * a.scale, r2[u][e], a2[u]);
                        a3[u] = mfma_l(x3[u][e], r3[u][e] * a.scale, a3[u]);
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s1[(2 * wv + u) * PS + (4 * g + r) * RS + i16] = a1[u][r];                 // (t = 4g+r, s = i16)
                if constexpr (RPE) {
                    s2[(4 * g + r) * PS + (wv + 8 * u) * RS + i16] = a2[u][r];             // (px = 4g+r, s = i16)
                    s3[(4 * g + r) * PS + i16 * RS + wv + 8 * u] = a3[u][r];               // (px = 4g+r, t = i16)
                }
            }
        __syncthreads();

        // ---- online softmax step (fp32, like th.softmax(w.float()))
        if (tid < 256) {
            const int px = tid >> 4, tl = tid & 15, t = min(t0 + tl, T - 1);
            const int o = px * PS + tl * RS;
            float w[16];
            float mx = m_run;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                float v = s1[o + s];
                if constexpr (RPE) v = v + s2[o + s] + s3[o + s];
                if (s0 + s >= T || !frame_pair_allowed(a, b, t, s0 + s)) v = -INFINITY;
                w[s] = v;
                mx = fmaxf(mx, v);
            }
            const bool none = mx == -INFINITY;                                       // no allowed key so far: nothing to rescale
            const float alpha = none ? 1.f : __expf(m_run - mx);
            float sum = 0.f;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float p = none ? 0.f : __expf(w[s] - mx);
                pb[o + s] = p;
                sum += p;
            }
            l_run = l_run * alpha + sum;
            m_run = mx;
            al[tid] = alpha;
        }
        __syncthreads();

        // ---- V: o *= alpha; o += p Rv (M = px), then p v of the tile (M = t, per pixel) turned into the same layout and added
        if (wv < NJ) {
            const int f0 = h * F + 16 * wv + i16;
#pragma unroll
            for (int tl = 0; tl < 16; ++tl)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[tl][r] *= al[(4 * g + r) * 16 + tl];
            if constexpr (RPE) {
                const float* rvb = a.Rv + (size_t)b * T * T * C + f0;
#pragma unroll 1
                for (int k4 = 0; k4 < 4; ++k4) {
                    const int s = min(s0 + 4 * k4 + g, T - 1);
                    float rr[16];
#pragma unroll
                    for (int tl = 0; tl < 16; ++tl) rr[tl] = rvb[((size_t)min(t0 + tl, T - 1) * T + s) * C];
#pragma unroll
                    for (int tl = 0; tl < 16; ++tl) acc[tl] = mfma_l(pb[i16 * PS + tl * RS + 4 * k4 + g], rr[tl], acc[tl]);
                }
            }
            f32x4 pv[16];
#pragma unroll
            for (int px = 0; px < 16; ++px) pv[px] = zero4;
            const float* vb = a.qkv + ((size_t)b * T * HW + p0) * C3 + 2 * C + f0;
#pragma unroll 1
            for (int k4 = 0; k4 < 4; ++k4) {
                const int s = min(s0 + 4 * k4 + g, T - 1);
                float vr[16];
#pragma unroll
                for (int px = 0; px < 16; ++px) vr[px] = vb[((size_t)s * HW + px) * C3];
#pragma unroll
                for (int px = 0; px < 16; ++px) pv[px] = mfma_l(pb[px * PS + i16 * RS + 4 * k4 + g], vr[px], pv[px]);
            }
            // (tile px = 4A+Bq, row c, reg d) = pv[px][t = 4c + d]  ->  (tile tl = 4c+d, row A, reg Bq) = pv[px = 4A+Bq][t = tl]
#pragma unroll
            for (int bq = 0; bq < 4; ++bq)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    float x0 = pv[bq][d], x1 = pv[4 + bq][d], x2 = pv[8 + bq][d], x3 = pv[12 + bq][d];
                    rows_regs_transpose_l(x0, x1, x2, x3);
                    acc[d][bq] += x0; acc[4 + d][bq] += x1; acc[8 + d][bq] += x2; acc[12 + d][bq] += x3;
                }
        }
    }
    __syncthreads();                                       // every wave is past its last V step (which reads al)
    if (tid < 256) al[tid] = 1.0f / l_run;
    __syncthreads();

    if (wv < NJ) {
        const int f0 = h * F + 16 * wv + i16;
#pragma unroll
        for (int tl = 0; tl < 16; ++tl) {
            const int t = t0 + tl;
            if (t < T) {
                float* o = a.out + (((size_t)b * T + t) * HW + p0 + 4 * g) * C + f0;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[(size_t)r * C] = acc[tl][r] * al[(4 * g + r) * 16 + tl];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Generic kernel: any head dim that is a multiple of 8 (the matrix-pipe kernel takes F % 16 == 0, F <= 128), any pixel count.
// Block = one pixel x one query tile of 16 frames of one (batch, head).  The score strip [16][T] of that pixel lives in LDS
// (8 KB at T = 128); a thread owns (t, s) pairs, then (t, 4 features) of the output.
// ---------------------------------------------------------------------------------------------------------------------
template <bool RPE>
__global__ __launch_bounds__(256) void attn_temporal_long_kernel(AttnTemporalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sc[];          // [16][T+1]
    const int T = a.T, C = a.C, HW = a.HW, C3 = 3 * a.C, F = C / a.heads, F4 = F >> 2, TS = T + 1;
    const int NQ = (T + 15) >> 4;
    const int b = blockIdx.z / NQ, t0 = 16 * (blockIdx.z - b * NQ), h = blockIdx.y, p = blockIdx.x;
    const int nq = min(16, T - t0);
    const int tid = threadIdx.x;
    const float* qb = a.qkv + ((size_t)b * T * HW + p) * C3 + h * F;   // + t*HW*C3: q at +0, k at +C, v at +2C
    const size_t fr = (size_t)HW * C3;
    auto ld4 = [](const float* x) { return *reinterpret_cast<const f32x4*>(x); };

    for (int pr = tid; pr < nq * T; pr += 256) {
        const int tl = pr / T, s = pr - tl * T, t = t0 + tl;
        const float* q = qb + t * fr;
        const float* k = qb + s * fr + C;
        const float* rk = RPE ? a.Rk + (((size_t)b * T + t) * T + s) * C + h * F : nullptr;
        const float* rq = RPE ? a.Rq + (((size_t)b * T + s) * T + t) * C + h * F : nullptr;
        float acc = 0.f;
        for (int f = 0; f < F; f += 4) {
            const f32x4 qv = ld4(q + f) * a.scale, kv = ld4(k + f);
            if constexpr (RPE) {
                const f32x4 kr = kv + ld4(rk + f), rqv = ld4(rq + f) * a.scale;
                acc += qv.x * kr.x + qv.y * kr.y + qv.z * kr.z + qv.w * kr.w + kv.x * rqv.x + kv.y * rqv.y + kv.z * rqv.z + kv.w * rqv.w;
            } else {
                acc += qv.x * kv.x + qv.y * kv.y + qv.z * kv.z + qv.w * kv.w;
            }
        }
        sc[tl * TS + s] = frame_pair_allowed(a, b, t, s) ? acc : -INFINITY;
    }
    __syncthreads();
    if (tid < nq) {
        float* r = sc + tid * TS;
        float mx = -INFINITY;
        for (int s = 0; s < T; ++s) mx = fmaxf(mx, r[s]);
        float sum = 0.f;
        for (int s = 0; s < T; ++s) { const float e = mx == -INFINITY ? 0.f : __expf(r[s] - mx); r[s] = e; sum += e; }
        const float inv = 1.0f / sum;
        for (int s = 0; s < T; ++s) r[s] *= inv;
    }
    __syncthreads();
    for (int item = tid; item < nq * F4; item += 256) {
        const int tl = item / F4, f4 = item - tl * F4, t = t0 + tl;
        const float* ar = sc + tl * TS;
        const float* vb = qb + 2 * C + 4 * f4;
        const float* rv = RPE ? a.Rv + (((size_t)b * T + t) * T) * C + h * F + 4 * f4 : nullptr;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < T; ++s) {
            f32x4 v = ld4(vb + s * fr);
            if constexpr (RPE) v += ld4(rv + (size_t)s * C);
            o += v * ar[s];
        }
        *reinterpret_cast<f32x4*>(a.out + (((size_t)b * T + t) * HW + p) * C + h * F + 4 * f4) = o;
    }
}

template <int NJ, bool RPE>
static int launch_long_mfma(const AttnTemporalArgs& a, hipStream_t s) {
    constexpr int PS = 16 * 17;
    constexpr size_t lds = ((size_t)(RPE ? 4 : 2) * 16 * PS + 256) * sizeof(float);
    if (lds > 48 * 1024) VD_RAISE_LDS((&attn_temporal_long_mfma_kernel<NJ, RPE>), lds);
    dim3 grid(a.HW / 16, a.heads, a.B * ((a.T + 15) / 16));
    hipLaunchKernelGGL((attn_temporal_long_mfma_kernel<NJ, RPE>), grid, dim3(512), lds, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

template <bool RPE>
static int launch_long_generic(const AttnTemporalArgs& a, hipStream_t s) {
    const size_t lds = (size_t)16 * (a.T + 1) * sizeof(float);
    dim3 grid(a.HW, a.heads, a.B * ((a.T + 15) / 16));
    hipLaunchKernelGGL((attn_temporal_long_kernel<RPE>), grid, dim3(256), lds, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

template <bool RPE>
static int launch_long_nj(const AttnTemporalArgs& a, int nj, hipStream_t s) {
    switch (nj) {
        case 1: return launch_long_mfma<1, RPE>(a, s);
        case 2: return launch_long_mfma<2, RPE>(a, s);
        case 3: return launch_long_mfma<3, RPE>(a, s);
        case 4: return launch_long_mfma<4, RPE>(a, s);
        case 5: return launch_long_mfma<5, RPE>(a, s);
        case 6: return launch_long_mfma<6, RPE>(a, s);
        case 7: return launch_long_mfma<7, RPE>(a, s);
        default: return launch_long_mfma<8, RPE>(a, s);
    }
}

// T in 33..kMaxWindowFrames; the caller (launch_attn_temporal) has checked the RPE pointers.  The kernel is the one
// attn_temporal_variant() names: chosen by the per-item shape alone (pixels, head dim), never by the batch.
int launch_attn_temporal_long(const AttnTemporalArgs& a, hipStream_t s) {
    const bool rpe = a.Rk != nullptr;
    const AttnTemporalVariant v = attn_temporal_variant(a.T, a.HW, a.C, a.heads, rpe);
    VD_REQUIRE(v.family == AttnTemporalVariant::kLongMfma || v.family == AttnTemporalVariant::kLongGeneric, "long temporal window: 33..128 frames");
    if (v.family == AttnTemporalVariant::kLongMfma) return rpe ? launch_long_nj<true>(a, v.p0, s) : launch_long_nj<false>(a, v.p0, s);
    return rpe ? launch_long_generic<true>(a, s) : launch_long_generic<false>(a, s);
}

}  // namespace vd
