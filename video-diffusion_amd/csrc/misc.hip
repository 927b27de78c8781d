// Small HBM-bound kernels around the UNet torso and the per-step posterior update, gfx950.
#include <algorithm>

#include "vd_common.h"

namespace vd {

// ------------------------------------------------------------------ network input (CondMargVideoModel.forward,
// unet.py:951-983,991-1013): 5 channels [x*lat + obs_src*obs + x*(1-any), obs, kinda_marg]; per-frame timesteps;
// attention mask.  The 5-channel 3x3 stem (input_blocks.0.0) has K = 45: far too thin for the implicit-GEMM conv
// kernels (13 TFLOP/s with the channels padded to 32), so the input is written directly as its im2col matrix
// [B*T*H*W][Kpad = 64], k = tap*5 + channel (zeros for taps outside the image and for k >= 45), and the stem runs as a
// plain K = 64 GEMM on gemm_frag_kernel.
__global__ __launch_bounds__(256) void assemble_kernel(AssembleArgs a) {
    const int n = a.frame_list ? a.frame_list[blockIdx.y] : blockIdx.y;      // source frame; the im2col rows go to block blockIdx.y
    const int HW = a.H * a.W;
    const float om = a.obs_mask[n], lm = a.lat_mask[n], km = a.km_mask[n];
    const float any = fminf(om + lm + km, 1.0f);
    const int Cs = a.cond_mode == 0 ? 5 : (a.cond_mode == 1 ? 6 : 3);      // stem input channels (unet.py:932-940)
    if (blockIdx.x == 0 && threadIdx.x == 0 && !a.frame_list) {
        const float t = a.t_model[n / a.T];
        const float tobs = a.obs_t_mode == 0 ? 0.f : (a.obs_t_mode == 1 ? t : t - 1.f);
        // 'channel': observed frames carry the timestep of their source (unet.py:991-1013); 'duplicate' / 'all': every frame
        // keeps t; 't=0' (unet.py:1018-1019): `timesteps[obs_mask == 1] = -1` writes through a (B, 1) -> (B, T) expanded tensor,
        // i.e. ONE stored value per batch item: all frames of an item with any observed frame get -1 (mirrored as computed)
        float tf = t;
        if (a.cond_mode == 0) tf = tobs * om + t * (1.f - om);
        else if (a.cond_mode == 2) {
            bool any_obs = false;
            for (int k = 0; k < a.T; ++k) any_obs |= a.obs_mask[(n / a.T) * a.T + k] == 1.f;
            if (any_obs) tf = -1.f;
        }
        a.t_frames[n] = tf;
        a.amask[n] = any;
    }
    // Block = a strip of up to 64 pixels of one image row.  The three source rows of the strip (+ one column either side) are read ONCE, along
    // x (coalesced), mixed into the Cs stem channels and kept in LDS; an im2col row of Kpad = 64 floats is nine shifted copies of those and
    // leaves as sixteen 16-byte stores of neighbouring lanes.  (First version: thread = (pixel, tap), every tap re-reading x and x0 with
    // scalar loads and Cs scalar stores: 71 us for the 134 MB of the headline window; 16-byte stores alone, the gathers still per lane: 79.)
    if (a.scalars_only) return;
    constexpr int SW = 64;
    __shared__ float tile[3][SW + 2][6];
    __shared__ int lut[256];
    const int strips = (a.W + SW - 1) / SW;
    const int y = blockIdx.x / strips, x0 = (blockIdx.x - y * strips) * SW;
    for (int i = threadIdx.x; i < 9 * (SW + 2); i += 256) {
        const int xx = i % (SW + 2), rc = i / (SW + 2), r = rc % 3, c = rc / 3;
        const int yy = y + r - 1, gx = x0 + xx - 1;
        const bool in = yy >= 0 && yy < a.H && gx >= 0 && gx < a.W;
        float xv = 0.f, ov = 0.f;
        if (in) {
            const size_t q = ((size_t)n * 3 + c) * HW + yy * a.W + gx;
            xv = a.x[q];
            ov = a.obs_src[q];
        }
        if (a.cond_mode == 0) {
            tile[r][xx][c] = in ? xv * lm + ov * om + xv * (1.f - any) : 0.f;
            if (c == 0) { tile[r][xx][3] = in ? om : 0.f; tile[r][xx][4] = in ? km : 0.f; }
        } else if (a.cond_mode == 1) {                                      // obs_src = x0 (unet.py:1014-1017)
            tile[r][xx][c] = in ? xv * lm + xv * (1.f - any) : 0.f;
            tile[r][xx][3 + c] = in ? ov * om : 0.f;
        } else tile[r][xx][c] = xv;
    }
    for (int k = threadIdx.x; k < a.Kpad; k += 256) {                     // column k -> its float in the tile of pixel 0 (or none)
        const int tap = k / Cs, c = k - tap * Cs;
        lut[k] = k < 9 * Cs ? ((tap / 3) * (SW + 2) + tap % 3) * 6 + c : -1;
    }
    __syncthreads();
    const int qpr = a.Kpad >> 2, sh = 31 - __clz(qpr);                      // (Kpad / 4 is a power of two: launch_assemble)
    const float* tf = &tile[0][0][0];
    for (int i = threadIdx.x; i < SW * qpr; i += 256) {
        const int px = i >> sh, j = i & (qpr - 1);
        if (x0 + px >= a.W) continue;
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = lut[4 * j + e];
            out[e] = o >= 0 ? tf[o + px * 6] : 0.f;
        }
        *reinterpret_cast<f32x4*>(a.x_cols + ((size_t)blockIdx.y * HW + (size_t)y * a.W + x0 + px) * a.Kpad + 4 * j) = out;
    }
}

int launch_assemble(const AssembleArgs& a, hipStream_t s) {
    VD_REQUIRE(a.Kpad >= 64 && a.Kpad <= 256 && (a.Kpad & (a.Kpad - 1)) == 0, "padded im2col width: 64, 128 or 256");
    VD_REQUIRE(!(a.frame_list && a.scalars_only), "assemble: a frame list writes im2col rows only");
    if (a.frame_list && a.n_list == 0) return 0;
    const dim3 grid(a.scalars_only ? 1 : a.H * ((a.W + 63) / 64), a.frame_list ? a.n_list : a.B * a.T);
    hipLaunchKernelGGL(assemble_kernel, grid, dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ frame-granular gather / scatter (window prefix cache)
template <bool SCATTER>
__global__ __launch_bounds__(256) void move_rows_kernel(const float* __restrict__ src, const int* __restrict__ list, size_t row4,
                                                        float* __restrict__ dst) {
    const int i = blockIdx.y, f = list[i];
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src) + (size_t)(SCATTER ? i : f) * row4;
    f32x4* d4 = reinterpret_cast<f32x4*>(dst) + (size_t)(SCATTER ? f : i) * row4;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < row4; k += (size_t)gridDim.x * 256) d4[k] = s4[k];
}

static int move_rows(bool scatter, const float* src, const int* list, int n, size_t row_floats, float* dst, hipStream_t s) {
    VD_REQUIRE(row_floats % 4 == 0, "frame rows in 16-byte units");
    if (n == 0) return 0;
    const size_t row4 = row_floats / 4;
    const int bx = (int)std::min<size_t>((row4 + 1023) / 1024, 64);
    if (scatter) hipLaunchKernelGGL(move_rows_kernel<true>, dim3(bx, n), dim3(256), 0, s, src, list, row4, dst);
    else hipLaunchKernelGGL(move_rows_kernel<false>, dim3(bx, n), dim3(256), 0, s, src, list, row4, dst);
    VD_HIP(hipGetLastError());
    return 0;
}
int launch_gather_rows(const float* src, const int* list, int n, size_t row_floats, float* dst, hipStream_t s) {
    return move_rows(false, src, list, n, row_floats, dst, s);
}
int launch_scatter_rows(const float* src, const int* list, int n, size_t row_floats, float* dst, hipStream_t s) {
    return move_rows(true, src, list, n, row_floats, dst, s);
}

// src [n][split][C][2] -> dst [frame][C][2] (one entry per frame and channel: the sum over the producer's pixel ranges, fp64)
__global__ void scatter_stats_kernel(const double* __restrict__ src, int split, int C, const int* __restrict__ list,
                                     double* __restrict__ dst) {
    const int i = blockIdx.x, f = list[i];
    for (int k = threadIdx.x; k < 2 * C; k += blockDim.x) {
        double v = 0;
        for (int sp = 0; sp < split; ++sp) v += src[((size_t)i * split + sp) * 2 * C + k];
        dst[(size_t)f * 2 * C + k] = v;
    }
}
int launch_scatter_stats(const double* src, int split, int C, const int* list, int n, double* dst, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(scatter_stats_kernel, dim3(n), dim3(256), 0, s, src, split, C, list, dst);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ sinusoidal embedding (nn.py:89-107)
// out[n] = [cos(t*f_i) | sin(t*f_i)], f from a host-built table so the angles match the reference bit for bit.
__global__ void sinus_kernel(const float* __restrict__ t, const float* __restrict__ freqs, int half, int dim,
                             float* __restrict__ out) {
    const int n = blockIdx.x;
    const float tv = t[n];
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        const float arg = tv * freqs[i];
        out[(size_t)n * dim + i] = cosf(arg);
        out[(size_t)n * dim + half + i] = sinf(arg);
    }
    if ((dim & 1) && threadIdx.x == 0) out[(size_t)n * dim + dim - 1] = 0.f;
}

int launch_sinus_embed(const float* t, int n, int dim, const float* freqs, float* out, hipStream_t s) {
    hipLaunchKernelGGL(sinus_kernel, dim3(n), dim3(64), 0, s, t, freqs, dim / 2, dim, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// frame embedding values (unet.py:914-926): t = fi (- mean over the window when centred)
__global__ void frame_t_kernel(const int64_t* __restrict__ fidx, int T, int center, float* __restrict__ tv) {
    const int b = blockIdx.x;
    float mean = 0.f;
    if (center) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += (float)fidx[b * T + t];
        mean = s / (float)T;
    }
    for (int t = threadIdx.x; t < T; t += blockDim.x) tv[b * T + t] = (float)fidx[b * T + t] - mean;
}

int launch_frame_t(const int64_t* fidx, int B, int T, int center, float* tv, hipStream_t s) {
    hipLaunchKernelGGL(frame_t_kernel, dim3(B), dim3(64), 0, s, fidx, T, center, tv);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ RPENet hidden layer (unet.py:283-296)
// One block per (batch item, query frame, net): the T key frames of a query frame share the timestep-embedding row, and a thread keeps its
// channel's four constants in registers (one block per (b, t, s) row -- 30 k blocks of 1.5 KB each -- wrote its 47 / 75 MB at 1.6 TB/s: 2 x 38 us).
__global__ __launch_bounds__(256) void rpe_hidden_tab_kernel(const float* __restrict__ te, int te_ld, const float* __restrict__ wbase,
                                                             const long long* __restrict__ tab, const int64_t* __restrict__ fidx, int T, int C,
                                                             float* __restrict__ E, size_t zs_e) {
    __shared__ float feat[64][3];
    const long long* tz = tab + 3 * blockIdx.y;
    te += tz[0];
    const float* Wd = wbase + tz[1];
    const float* bd = wbase + tz[2];
    E += blockIdx.y * zs_e;
    const int bt = blockIdx.x, b = bt / T;      // rows (b*T + t)*T + s, s = 0 .. T-1
    for (int s0 = 0; s0 < T; s0 += 64) {
        const int ns = min(64, T - s0);
        __syncthreads();
        if ((int)threadIdx.x < ns) {
            const float d = (float)(fidx[bt] - fidx[b * T + s0 + threadIdx.x]);
            feat[threadIdx.x][0] = logf(1.0f + fmaxf(d, 0.f));
            feat[threadIdx.x][1] = logf(1.0f + fmaxf(-d, 0.f));
            feat[threadIdx.x][2] = d == 0.f ? 1.f : 0.f;
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const float bc = bd[c], w0 = Wd[c * 3], w1 = Wd[c * 3 + 1], w2 = Wd[c * 3 + 2], tv = te[(size_t)bt * te_ld + c];
            for (int k = 0; k < ns; ++k) {
                const float lin = bc + feat[k][0] * w0 + feat[k][1] * w1 + feat[k][2] * w2;
                E[((size_t)bt * T + s0 + k) * C + c] = silu_f(tv + lin);
            }
        }
    }
}

int launch_rpe_hidden_tab(const float* te, int te_ld, const float* wbase, const long long* tab, const int64_t* fidx, int B, int T, int C,
                          float* E, int nz, size_t zs_e, hipStream_t s) {
    hipLaunchKernelGGL(rpe_hidden_tab_kernel, dim3(B * T, nz), dim3(256), 0, s, te, te_ld, wbase, tab, fidx, T, C, E, zs_e);
    VD_HIP(hipGetLastError());
    return 0;
}

// bucket-table relative positions (RPE.get_bucket_ids, unet.py:330-347; iRPE eq. 18)
__global__ __launch_bounds__(256) void rpe_table_kernel(const float* __restrict__ table, const int64_t* __restrict__ fidx,
                                                        int T, int C, float alpha, float beta, float gamma, double lg,
                                                        float* __restrict__ R) {
    const int row = blockIdx.x;
    const int s_ = row % T, bt = row / T, b = bt / T;
    const long long d = fidx[bt] - fidx[b * T + s_];
    long long id = d;
    const float ad = fabsf((float)d);
    if (ad > alpha) {
        // The bucket is a truncation, and at some integer distances the value truncated is an exact integer (alpha, beta, gamma =
        // 3, 7, 20: d = 20 -> 7.0), which the reference's CPU float32 evaluation returns as such.  In device float32 (logf one ulp low)
        // d = 20 landed at 6.9999995: the neighbouring table row.  So: the value in fp64, snapped to an integer it is within 1e-6 of
        // (the float32 reference cannot tell such a value from the integer either), then the reference's minimum and truncation.
        double v = (double)alpha + log((double)ad / (double)alpha) / lg * ((double)beta - (double)alpha);
        const double r = rint(v);
        if (fabs(v - r) < 1e-6) v = r;
        v = fmin((double)beta, v);              // (alpha == beta == gamma: v is NaN, the reference's cast undefined; here: beta)
        id = (long long)(int)v * (d > 0 ? 1 : -1);
    }
    const int nb = 2 * (int)beta + 1;
    if (id < 0) id += nb;                       // negative indices wrap, as torch indexing does
    for (int c = threadIdx.x; c < C; c += 256) R[(size_t)row * C + c] = table[(size_t)id * C + c];
}

int launch_rpe_table(const float* table, const int64_t* fidx, int B, int T, int C, float alpha, float beta,
                     float gamma, float* R, hipStream_t s) {
    const double lg = log((double)gamma / (double)alpha);
    hipLaunchKernelGGL(rpe_table_kernel, dim3(B * T * T), dim3(256), 0, s, table, fidx, T, C, alpha, beta, gamma, lg, R);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ h + spatial_encoding (+ frame embedding)
__global__ __launch_bounds__(256) void posenc_kernel(const float* __restrict__ x, const float* __restrict__ P,
                                                     const float* __restrict__ femb, size_t per_frame4, int C4,
                                                     size_t total4, float* __restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        if (P) v += reinterpret_cast<const f32x4*>(P)[i % per_frame4];
        if (femb) v += reinterpret_cast<const f32x4*>(femb)[(i / per_frame4) * C4 + (i % C4)];
        reinterpret_cast<f32x4*>(y)[i] = v;
    }
}

int launch_posenc_add(const float* x, const float* P, const float* femb, int nfr, int HW, int C, float* y,
                      hipStream_t s) {
    const size_t total4 = (size_t)nfr * HW * C / 4;
    const int grid = (int)std::min<size_t>((total4 + 255) / 256, 4096);
    hipLaunchKernelGGL(posenc_kernel, dim3(grid), dim3(256), 0, s, x, P, femb, (size_t)HW * C / 4, C / 4, total4, y);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ output head: GN-affine + SiLU + conv3x3 C->Cout (<=4)
// NHWC in, NCHW out (the caller's layout).  16x16 output pixels per block, the activated halo tile
// staged through LDS 32 channels at a time; VALU (3 output channels cannot feed a 32x32 MFMA tile).
constexpr int OT = 16;
template <int NCO>      // accumulators per pixel: 4 (eps: 3 outputs) or 8 (learn_sigma: eps | variance values, 6 outputs)
__global__ __launch_bounds__(256) void out_conv_kernel(const float* __restrict__ x, const float* __restrict__ affA,
                                                       const float* __restrict__ affB, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int H, int W, int C, int Cout,
                                                       float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[(OT + 2) * (OT + 2) * 36];
    __shared__ __attribute__((aligned(16))) float ws[9 * NCO * 32];
    const int n = blockIdx.z, y0 = blockIdx.y * OT, x0 = blockIdx.x * OT;
    const int tid = threadIdx.x, ty = tid / OT, tx = tid % OT;
    float acc[NCO];
#pragma unroll
    for (int co = 0; co < NCO; ++co) acc[co] = 0.f;
    for (int c0 = 0; c0 < C; c0 += 32) {
        __syncthreads();
        for (int i = tid; i < (OT + 2) * (OT + 2) * 8; i += 256) {
            const int pix = i >> 3, q = i & 7;
            const int iy = y0 + pix / (OT + 2) - 1, ix = x0 + pix % (OT + 2) - 1;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                v = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + iy) * W + ix) * C + c0 + q * 4);
                const f32x4 A = *reinterpret_cast<const f32x4*>(affA + (size_t)n * C + c0 + q * 4);
                const f32x4 B = *reinterpret_cast<const f32x4*>(affB + (size_t)n * C + c0 + q * 4);
                v = v * A + B;
                v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w);
            }
            *reinterpret_cast<f32x4*>(tile + pix * 36 + q * 4) = v;
        }
        for (int i = tid; i < 9 * NCO * 32; i += 256) {
            const int tap = i / (NCO * 32), co = (i / 32) % NCO, c = i % 32;
            ws[i] = co < Cout ? w[((size_t)tap * Cout + co) * C + c0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float* tp = tile + ((ty + tap / 3) * (OT + 2) + tx + tap % 3) * 36;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(tp + q * 4);
#pragma unroll
                for (int co = 0; co < NCO; ++co) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + (tap * NCO + co) * 32 + q * 4);
                    acc[co] += v.x * wv.x + v.y * wv.y + v.z * wv.z + v.w * wv.w;
                }
            }
        }
    }
    const int oy = y0 + ty, ox = x0 + tx;
    if (oy < H && ox < W)
        for (int co = 0; co < Cout; ++co) out[(((size_t)n * Cout + co) * H + oy) * W + ox] = acc[co] + bias[co];
}

int launch_out_conv(const float* x, const float* affA, const float* affB, const float* w, const float* bias, int nfr,
                    int H, int W, int C, int Cout, float* out_nchw, hipStream_t s) {
    VD_REQUIRE(Cout <= 8 && C % 32 == 0, "output head: Cout <= 8, C multiple of 32");
    const dim3 grid((W + OT - 1) / OT, (H + OT - 1) / OT, nfr);
    if (Cout <= 4) hipLaunchKernelGGL(out_conv_kernel<4>, grid, dim3(256), 0, s, x, affA, affB, w, bias, H, W, C, Cout, out_nchw);
    else hipLaunchKernelGGL(out_conv_kernel<8>, grid, dim3(256), 0, s, x, affA, affB, w, bias, H, W, C, Cout, out_nchw);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ output head as GEMM + gather (engine.hip: forward)
// ------------------------------------------------------------------ the output head's GEMM (unet.py:744-749,838)
// T[pixel][co * 9 + tap] = silu(h[pixel][:] * A[frame][:] + B[frame][:]) . w[co][:][tap]: the head's 3x3 conv (C -> 3 | 6 channels behind
// GroupNorm + SiLU) as a 1x1 GEMM over its 27 | 54 (cout, tap) columns, followed by out_gather_kernel.  C is 128 and N is 32: no tile of
// the general kernels fits (the generic fp32 kernel ran it at 1.4 TB/s, 185 us of the headline step for 268 MB).  Here: fp32 MFMA
// 32x32x2 (exact fp32 products; the k order is free as long as A and B agree, so one float4 per lane feeds four MFMAs), the weights of a
// column tile resident in registers, a block = 1024 pixels of one frame (its (A, B) in LDS), a wave = 8 tiles of 32 pixels with the next
// tile's rows requested before the current one is multiplied.  Bound by the read of h.
template <int NCT, int CMAX>
__global__ __launch_bounds__(256, 2) void head_gemm_kernel(const float* __restrict__ h, const float* __restrict__ affA, const float* __restrict__ affB,
                                                           const float* __restrict__ Wt, int HW, int C, int TPW, float* __restrict__ T) {
    constexpr int NI = CMAX / 8, LDT = 32 * NCT;
    __shared__ __attribute__((aligned(16))) float sab[2 * CMAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 31, kh = lane >> 5;
    const size_t pix_blk = (size_t)blockIdx.x * (128 * TPW);          // 128 TPW pixels of ONE frame (HW % 1024 == 0; TPW = 8 | 2: tiles per wave)
    const int n = (int)(pix_blk / HW);
    for (int c = tid; c < C; c += 256) { sab[c] = affA[(size_t)n * C + c]; sab[CMAX + c] = affB[(size_t)n * C + c]; }
    const int ni = C >> 3;
    f32x4 w[NCT][NI];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int i = 0; i < NI; ++i)
            w[ct][i] = i < ni ? *reinterpret_cast<const f32x4*>(Wt + (size_t)(ct * 32 + lr) * C + 8 * i + 4 * kh) : f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const size_t pix0 = pix_blk + (size_t)wv * TPW * 32;
    const float* src = h + (pix0 + lr) * C + 4 * kh;
    f32x4 xa[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) xa[i] = i < ni ? *reinterpret_cast<const f32x4*>(src + 8 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int it = 0; it < TPW; ++it) {
        f32x4 xn[NI];
        const float* nsrc = src + (size_t)(it + 1 < TPW ? it + 1 : it) * 32 * C;
#pragma unroll
        for (int i = 0; i < NI; ++i) xn[i] = i < ni ? *reinterpret_cast<const f32x4*>(nsrc + 8 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x16 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (i < ni) {
                const f32x4 Aq = *reinterpret_cast<const f32x4*>(sab + 8 * i + 4 * kh), Bq = *reinterpret_cast<const f32x4*>(sab + CMAX + 8 * i + 4 * kh);
                f32x4 v = xa[i] * Aq + Bq;
                v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], w[ct][i][e], acc[ct], 0, 0, 0);
            }
        }
        float* dst = T + (pix0 + (size_t)it * 32 + 4 * kh) * LDT + lr;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(size_t)((r & 3) + 8 * (r >> 2)) * LDT + ct * 32] = acc[ct][r];
#pragma unroll
        for (int i = 0; i < NI; ++i) xa[i] = xn[i];
    }
}

// (32 columns: the 3-channel head; the 6-channel head of a learn_sigma network needs twice the weight registers and stays on the generic kernel)
bool head_gemm_supported(int HW, int C, int ldt) { return HW % 1024 == 0 && C % 8 == 0 && C <= 128 && ldt == 32; }

// tiles of 32 pixels per wave: a small window (one rank's share of a strong-scaling split: 16 frames = 64 blocks of 1024 pixels) takes
// 256-pixel blocks: head 58 -> 29 us there
int head_gemm_tiles_per_wave(int nfr, int HW) { return (size_t)nfr * HW / 1024 < 512 ? 2 : 8; }

int launch_head_gemm(const float* h, const float* affA, const float* affB, const float* Wt, int nfr, int HW, int C, int ldt, float* T, hipStream_t s) {
    VD_REQUIRE(head_gemm_supported(HW, C, ldt), "output head GEMM: whole 1024-pixel blocks of a frame, C <= 128, 32 columns");
    const int tpw = head_gemm_tiles_per_wave(nfr, HW);
    const dim3 grid((unsigned)((size_t)nfr * HW / (128 * tpw)));
    hipLaunchKernelGGL((head_gemm_kernel<1, 128>), grid, dim3(256), 0, s, h, affA, affB, Wt, HW, C, tpw, T);
    VD_HIP(hipGetLastError());
    return 0;
}

// T[pixel][co * 9 + tap] holds what tap `tap` of output channel co contributes FROM this pixel; output pixel (y, x) sums the entry of
// tap (dy, dx) at pixel (y + dy - 1, x + dx - 1).  Block = 16 x 16 output pixels: the 18 x 18 halo of T rows is staged through LDS
// with coalesced 16-byte loads (rows padded to an odd number of quads: lanes of a row walk different banks), then 9 * Cout LDS reads
// per pixel.  NCHW out.
template <int LDT>
__global__ __launch_bounds__(256) void out_gather_kernel(const float* __restrict__ T, const float* __restrict__ bias, int H, int W, int Cout,
                                                         float* __restrict__ out) {
    constexpr int ROW = LDT + 4;                                      // floats per staged pixel
    __shared__ __attribute__((aligned(16))) float tile[(OT + 2) * (OT + 2) * ROW];
    const int n = blockIdx.z, y0 = blockIdx.y * OT, x0 = blockIdx.x * OT;
    const int tid = threadIdx.x, ty = tid / OT, tx = tid % OT;
    for (int i = tid; i < (OT + 2) * (OT + 2) * (LDT / 4); i += 256) {
        const int pix = i / (LDT / 4), q = i - pix * (LDT / 4);
        const int iy = y0 + pix / (OT + 2) - 1, ix = x0 + pix % (OT + 2) - 1;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const f32x4*>(T + (((size_t)n * H + iy) * W + ix) * LDT + q * 4);
        *reinterpret_cast<f32x4*>(tile + pix * ROW + q * 4) = v;
    }
    __syncthreads();
    const int oy = y0 + ty, ox = x0 + tx;
    if (oy >= H || ox >= W) return;
    for (int co = 0; co < Cout; ++co) {
        float acc = bias[co];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc += tile[((ty + tap / 3) * (OT + 2) + tx + tap % 3) * ROW + co * 9 + tap];
        out[(((size_t)n * Cout + co) * H + oy) * W + ox] = acc;
    }
}

int launch_out_gather(const float* T, const float* bias, int nfr, int H, int W, int ldt, int Cout, float* out_nchw, hipStream_t s) {
    VD_REQUIRE((ldt == 32 || ldt == 64) && 9 * Cout <= ldt, "output head: 3 or 6 output channels");
    const dim3 grid((W + OT - 1) / OT, (H + OT - 1) / OT, nfr);
    if (ldt == 32) hipLaunchKernelGGL(out_gather_kernel<32>, grid, dim3(256), 0, s, T, bias, H, W, Cout, out_nchw);
    else hipLaunchKernelGGL(out_gather_kernel<64>, grid, dim3(256), 0, s, T, bias, H, W, Cout, out_nchw);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ Philox4x32-10 + Box-Muller (vd_common.h: philox4x32_10, normal_at, normal4_at)
__global__ __launch_bounds__(256) void randn_kernel(float* out, size_t n, unsigned long long seed,
                                                    unsigned long long offset) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = normal_at(seed, offset, i);
}

int launch_randn(float* out, long n, unsigned long long seed, unsigned long long offset, hipStream_t s) {
    const int grid = (int)std::min<long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(randn_kernel, dim3(grid), dim3(256), 0, s, out, (size_t)n, seed, offset);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ sampler passes (the closing pass of a step, one launch)
// The head every pass shares.  An index t outside the schedule (the reference raises IndexError in _extract_into_tensor) reads no table:
// every non-null output of group i is poisoned.  Bit 0 of the error word is map_t_kernel's, in the entries that run the network before
// this pass; the network-free entries poison only.
__device__ __forceinline__ void splat(float& v, float q) { v = q; }
__device__ __forceinline__ void splat(float4& v, float q) { v = make_float4(q, q, q, q); }
template <class V>      // float | float4: the width group i is counted in
__device__ __forceinline__ bool pass_t(const SamplerPassArgs& a, size_t item, size_t i, int& t) {
    const long long tl = a.t[item];
    if (tl >= 0 && tl < a.num_timesteps) { t = (int)tl; return true; }
    V q;
    splat(q, __builtin_nanf(""));
    if (a.sample) reinterpret_cast<V*>(a.sample)[i] = q;
    if (a.xstart) reinterpret_cast<V*>(a.xstart)[i] = q;
    if (a.mean) reinterpret_cast<V*>(a.mean)[i] = q;
    return false;
}
// (pass_x0, the x_0 head of every pass, lives in vd_common.h: measure.hip forms the same bits with it)

// p_sample (gaussian_diffusion.py:319-343,374-382,208-227,438-443) and ddim_sample (:597-634), element by element (any per).
// Coefficients are float32 casts of the float64 tables, exactly what _extract_into_tensor yields.
__global__ __launch_bounds__(256) void posterior_kernel(SamplerPassArgs a) {
    const size_t total = (size_t)a.B * a.per;
    if (a.dstate) { a.seed = a.dstate[0]; a.offset = a.dstate[1]; }
    const int NT = a.num_timesteps;
    const float* src = a.x0_given ? a.x0_given : a.eps;
    bool nonfinite = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int t;
        if (!pass_t<float>(a, i / a.per, i, t)) continue;
        const float* tb = a.tab + t;
        const float x = a.x[i];
        float x0 = pass_x0(x, src[i], a.x0_given != nullptr, tb[TAB_SQRT_RECIP * NT], tb[TAB_SQRT_RECIPM1 * NT], a.clip, nonfinite);
        // this pass alone turns an INFINITE x0 into NaN too (eps = +inf would leave pred_xstart and p_sample's sample at -inf, not at the
        // NaN bit 1's readers are told of); the deterministic passes below hand it through as it is
        if (!(fabsf(x0) <= 3.4028234e38f)) x0 = __builtin_nanf("");
        if (a.xstart) a.xstart[i] = x0;
        if (a.mean) a.mean[i] = tb[TAB_COEF1 * NT] * x0 + tb[TAB_COEF2 * NT] * x;
        if (!a.sample) continue;                 // p_mean_variance only
        const float z = a.noise ? a.noise[i] : normal_at(a.seed, a.offset, i);
        const float nz = t != 0 ? 1.0f : 0.0f;
        float smp;
        if (a.sampler == SAMPLER_P) {
            const float mean = tb[TAB_COEF1 * NT] * x0 + tb[TAB_COEF2 * NT] * x;
            smp = mean + nz * expf(0.5f * tb[TAB_LOGVAR * NT]) * z;
        } else {
            const float e2 = (tb[TAB_SQRT_RECIP * NT] * x - x0) / tb[TAB_SQRT_RECIPM1 * NT];
            const float ab = tb[TAB_ACP * NT], abp = tb[TAB_ACP_PREV * NT];
            const float sigma = a.eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
            const float mean = x0 * sqrtf(abp) + sqrtf(1.f - abp - sigma * sigma) * e2;
            smp = mean + nz * sigma * z;
        }
        a.sample[i] = smp;
    }
    if (nonfinite && a.err) atomicOr(a.err, VD_ERR_NONFINITE);     // (never taken on a healthy step: no cost beside the compare above)
}

// The two samplers that draw no noise: the eta = 0 DDIM update from x_0 (or D) towards the cumulative alpha `ab`,
// e = (sr x - D) / srm1, sample = D sqrt(ab) + sqrt(1 - ab) e.  Four elements per thread and pass (16-byte accesses; per % 4 == 0 keeps a
// group inside one batch item); sample may alias x: the update is elementwise.
//   ddim_reverse_sample (gaussian_diffusion.py:636-668), x_t -> x_{t+1} in the reference's operation order: ab = alphas_cumprod_next[t] =
//     append(alphas_cumprod[1:], 0.0)[t], the TAB_ACP row at t + 1 (0 behind the last step); the float32 cast is elementwise, so these are
//     _extract_into_tensor's bits.  D = x_0.
//   dpmpp_2m_sample (this project's extension), x_t -> x_{t-1}: ab = TAB_ACP_PREV at t; with history D = D_t + w[t] (D_t - D_prev), else
//     D = D_t.  At t = 0 ab = 1 and w = 0: sample = D_t, nothing infinite.  Whether there is history is DATA (a null pointer, or a device
//     word that is 0), so one captured graph serves a window's first and later steps.  hist may alias xstart (in-place history): group i
//     is read before it is written, by the same thread.
template <int S>
__device__ __forceinline__ float deterministic_one(float x, float src, bool given, float prev, bool have, float w, float sr, float srm1,
                                                   float r, float s, int clip, float& x0_out, bool& nonfinite) {
    const float x0 = pass_x0(x, src, given, sr, srm1, clip, nonfinite);
    x0_out = x0;
    if constexpr (S == SAMPLER_DPMPP_2M) {
        const float d = have ? x0 + w * (x0 - prev) : x0;
        const float e = (sr * x - d) / srm1;
        return d * r + s * e;
    } else {
        const float e = (sr * x - x0) / srm1;
        return x0 * r + s * e;
    }
}

template <int S>        // SAMPLER_DDIM_REVERSE | SAMPLER_DPMPP_2M
__global__ __launch_bounds__(256) void deterministic_kernel(SamplerPassArgs a) {
    const size_t per4 = (size_t)a.per / 4, total4 = (size_t)a.B * per4;
    const int NT = a.num_timesteps;
    const float4* x4 = reinterpret_cast<const float4*>(a.x);
    const float4* src4 = reinterpret_cast<const float4*>(a.x0_given ? a.x0_given : a.eps);
    const bool given = a.x0_given != nullptr;
    const float4* hist4 = reinterpret_cast<const float4*>(a.hist);
    bool have = false;
    if constexpr (S == SAMPLER_DPMPP_2M) have = hist4 != nullptr && (a.hist_on == nullptr || *a.hist_on != 0ULL);
    float4* sample4 = reinterpret_cast<float4*>(a.sample);
    float4* xstart4 = reinterpret_cast<float4*>(a.xstart);
    bool nonfinite = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        int t;
        if (!pass_t<float4>(a, i / per4, i, t)) continue;
        const float sr = a.tab[TAB_SQRT_RECIP * NT + t], srm1 = a.tab[TAB_SQRT_RECIPM1 * NT + t];
        float ab, w = 0.0f;
        if constexpr (S == SAMPLER_DPMPP_2M) { ab = a.tab[TAB_ACP_PREV * NT + t]; w = a.w[t]; }
        else ab = t + 1 < NT ? a.tab[TAB_ACP * NT + t + 1] : 0.0f;
        const float r = sqrtf(ab), s = sqrtf(1.0f - ab);
        const float4 x = x4[i], src = src4[i];
        const float4 p = have ? hist4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 x0, o;
        o.x = deterministic_one<S>(x.x, src.x, given, p.x, have, w, sr, srm1, r, s, a.clip, x0.x, nonfinite);
        o.y = deterministic_one<S>(x.y, src.y, given, p.y, have, w, sr, srm1, r, s, a.clip, x0.y, nonfinite);
        o.z = deterministic_one<S>(x.z, src.z, given, p.z, have, w, sr, srm1, r, s, a.clip, x0.z, nonfinite);
        o.w = deterministic_one<S>(x.w, src.w, given, p.w, have, w, sr, srm1, r, s, a.clip, x0.w, nonfinite);
        if (xstart4) xstart4[i] = x0;
        sample4[i] = o;
    }
    if (nonfinite && a.err) atomicOr(a.err, VD_ERR_NONFINITE);
}

// dpmpp_2m_sde_sample (this project's extension: SDE-DPM-Solver++(2M)), x_t -> x_{t-1}: the one pass that reads history AND noise.  It is
// ddim_sample's update at eta = 1 on the extrapolated prediction, as dpmpp_2m_sample is the eta = 0 update on it:
//   D = D_t + w[t] (D_t - D_prev) with history, else D_t;   sigma = sqrt((1 - abp) / (1 - ab)) sqrt(1 - ab / abp);   e = (sr x - D) / srm1
//   sample = D sqrt(abp) + sqrt(1 - abp - sigma^2) e + [t != 0] sigma z;   pred_xstart = D_t (the next step's history, not D)
// At t = 0 abp = 1, w = 0, sigma = 0: sample = D_0, nothing infinite, no noise.  z of element i is noise[i] or normal_at(seed, offset, i) --
// ddim_sample's draw for the same state; {seed, offset} from `dstate` when set.  The head, the NaN of a non-finite x_0 and the error word
// are posterior_kernel's; history as data (null, or a device word that is 0) and hist aliasing xstart are deterministic_kernel's.
// V = float4: four elements per thread and pass, 16-byte accesses, one Philox block (normal4_at: normal_at's bits) -- per % 4 == 0 keeps a
// group inside one batch item.  V = float: any per and any alignment, element by element (launch_sampler_pass chooses).
__device__ __forceinline__ void pass_ld(const float* p, size_t i, float (&o)[1]) { o[0] = p[i]; }
__device__ __forceinline__ void pass_ld(const float* p, size_t i, float (&o)[4]) {
    const float4 v = reinterpret_cast<const float4*>(p)[i];
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void pass_st(float* p, size_t i, const float (&o)[1]) { p[i] = o[0]; }
__device__ __forceinline__ void pass_st(float* p, size_t i, const float (&o)[4]) { reinterpret_cast<float4*>(p)[i] = make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ void pass_normal(unsigned long long seed, unsigned long long offset, size_t i, float (&o)[1]) { o[0] = normal_at(seed, offset, i); }
__device__ __forceinline__ void pass_normal(unsigned long long seed, unsigned long long offset, size_t i, float (&o)[4]) {
    const f32x4 z = normal4_at(seed, offset, i);
    o[0] = z[0]; o[1] = z[1]; o[2] = z[2]; o[3] = z[3];
}

template <class V>      // float | float4
__global__ __launch_bounds__(256) void dpmpp_2m_sde_kernel(SamplerPassArgs a) {
    constexpr int W = sizeof(V) / sizeof(float);
    const size_t perv = (size_t)a.per / W, total = (size_t)a.B * perv;
    if (a.dstate) { a.seed = a.dstate[0]; a.offset = a.dstate[1]; }
    const int NT = a.num_timesteps;
    const float* src = a.x0_given ? a.x0_given : a.eps;
    const bool given = a.x0_given != nullptr;
    const bool have = a.hist != nullptr && (a.hist_on == nullptr || *a.hist_on != 0ULL);
    bool nonfinite = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int t;
        if (!pass_t<V>(a, i / perv, i, t)) continue;
        const float* tb = a.tab + t;
        const float sr = tb[TAB_SQRT_RECIP * NT], srm1 = tb[TAB_SQRT_RECIPM1 * NT];
        const float ab = tb[TAB_ACP * NT], abp = tb[TAB_ACP_PREV * NT], w = a.w[t];
        const float sigma = sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
        const float r = sqrtf(abp), c = sqrtf(fmaxf(1.f - abp - sigma * sigma, 0.f));
        const float sz = t != 0 ? sigma : 0.0f;
        float x[W], sv[W], p[W] = {}, z[W], x0[W], o[W];
        pass_ld(a.x, i, x);
        pass_ld(src, i, sv);
        if (have) pass_ld(a.hist, i, p);
        if (a.noise) pass_ld(a.noise, i, z);
        else pass_normal(a.seed, a.offset, i, z);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float d0 = pass_x0(x[k], sv[k], given, sr, srm1, a.clip, nonfinite);
            if (!(fabsf(d0) <= 3.4028234e38f)) d0 = __builtin_nanf("");         // as posterior_kernel: an infinite x_0 leaves as NaN too
            x0[k] = d0;
            const float d = have ? d0 + w * (d0 - p[k]) : d0;
            const float e = (sr * x[k] - d) / srm1;
            const float mean = d * r + c * e;
            o[k] = mean + sz * z[k];
        }
        if (a.xstart) pass_st(a.xstart, i, x0);
        pass_st(a.sample, i, o);
    }
    if (nonfinite && a.err) atomicOr(a.err, VD_ERR_NONFINITE);
}

static int launch_dpmpp_2m_sde(const SamplerPassArgs& a, hipStream_t s) {
    const std::string k = "dpmpp_2m_sde_kernel: ";
    VD_REQUIRE(a.B > 0 && a.per > 0, k + "B and the elements per item must be positive");
    VD_REQUIRE(a.x && (a.eps || a.x0_given) && a.t && a.tab && a.sample, k + "null tensor");
    VD_REQUIRE(!a.mean, k + "the pass writes no posterior mean");
    VD_REQUIRE(a.w, "dpmpp_2m_sde_sample: no multistep weight row for the bound schedule (vd_set_multistep_weights, after vd_set_schedule)");
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool v4 = a.per % 4 == 0 && al16(a.x) && al16(a.eps) && al16(a.x0_given) && al16(a.hist) && al16(a.noise) && al16(a.sample) && al16(a.xstart);
    const size_t groups = (size_t)a.B * (v4 ? a.per / 4 : a.per);
    const int grid = (int)std::min<size_t>((groups + 255) / 256, 4096);
    if (v4) hipLaunchKernelGGL(dpmpp_2m_sde_kernel<float4>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dpmpp_2m_sde_kernel<float>, dim3(grid), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// unipc_sample (this project's extension: UniPC of Zhao et al. 2023, data prediction, multistep order 2, B(h) = e^-h - 1), x_t -> x_{t-1}:
// the forward the step runs at the PREDICTED point x~_t first corrects that point, then predicts the next one -- one pass, both linear:
//   D_t    = the head every pass shares (pass_x0; a non-finite one leaves as NaN and raises bit 1, as in dpmpp_2m_sde_kernel)
//   x^c_t  = c0 base + c1 D1 + c2 D2 + c3 D_t      base = x^c_{t+1}, D1 = D_{t+1}, D2 = D_{t+2};  order min(2, n);  n = 0: x^c_t = x~_t
//   sample = p0 x^c_t + p1 D_t + p2 D1             order min(2, n + 1)
//   state  <- (x^c_t, D_t, D1)
// n = min(count, num_timesteps - 1 - t): the steps behind this one, never more than the schedule has above t -- so a row that does not exist
// (vd_set_unipc_rows leaves it zero) is never selected, whatever count a caller hands.  count is DATA (the host's, or a device word), so one
// captured graph serves a window's first, second and later steps.  Each sum is one rounded product and a chain of fused multiply-adds, in
// the order written: 4 roundings into x^c_t, 3 more into the sample (tests/unipc_restated.py counts on it).  At t = 0 the predictor row is
// (0, 1, 0): sample = D_0.  The state may be updated in place and the sample may alias x: element i is read and then written by one thread.
// V = float4 | float as in dpmpp_2m_sde_kernel (launch_unipc chooses).
template <class V>
__global__ __launch_bounds__(256) void unipc_kernel(SamplerPassArgs a) {
    constexpr int W = sizeof(V) / sizeof(float);
    const size_t perv = (size_t)a.per / W, total = (size_t)a.B * perv;
    const int NT = a.num_timesteps;
    const float* src = a.x0_given ? a.x0_given : a.eps;
    const bool given = a.x0_given != nullptr;
    const bool state = a.ubase != nullptr;
    const unsigned long long cnt = !state ? 0ULL : a.hist_on ? *a.hist_on : (unsigned long long)a.count;
    bool nonfinite = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int t;
        if (!pass_t<V>(a, i / perv, i, t)) {         // (sample and pred_xstart are poisoned by now) the state of the item as well
            V q;
            splat(q, __builtin_nanf(""));
            if (a.ubase_out) reinterpret_cast<V*>(a.ubase_out)[i] = q;
            if (a.ud1_out) reinterpret_cast<V*>(a.ud1_out)[i] = q;
            if (a.ud2_out) reinterpret_cast<V*>(a.ud2_out)[i] = q;
            continue;
        }
        const int above = NT - 1 - t;
        const int n = cnt < (unsigned long long)above ? (int)cnt : above;
        const float sr = a.tab[TAB_SQRT_RECIP * NT + t], srm1 = a.tab[TAB_SQRT_RECIPM1 * NT + t];
        const float* cr = a.urows + (size_t)(n >= 2 ? UNIPC_C2 : UNIPC_C1) * NT + t;
        const float* pr = a.urows + (size_t)(n >= 1 ? UNIPC_P2 : UNIPC_P1) * NT + t;
        const float p0 = pr[0], p1 = pr[NT], p2 = pr[2 * NT];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
        if (n >= 1) { c0 = cr[0]; c1 = cr[NT]; c2 = cr[2 * NT]; c3 = cr[3 * NT]; }
        float x[W], sv[W], bs[W] = {}, d1[W] = {}, d2[W] = {}, x0[W], xc[W], o[W];
        pass_ld(a.x, i, x);
        pass_ld(src, i, sv);
        if (state) { pass_ld(a.ubase, i, bs); pass_ld(a.ud1, i, d1); pass_ld(a.ud2, i, d2); }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float dt = pass_x0(x[k], sv[k], given, sr, srm1, a.clip, nonfinite);
            if (!(fabsf(dt) <= 3.4028234e38f)) dt = __builtin_nanf("");
            x0[k] = dt;
            // a tensor the order does not reach is not used, whatever it holds (a window's buffers before its first step: any bits)
            const float e1 = n >= 1 ? d1[k] : 0.f, e2 = n >= 2 ? d2[k] : 0.f;
            xc[k] = n >= 1 ? fmaf(c3, dt, fmaf(c2, e2, fmaf(c1, e1, c0 * bs[k]))) : x[k];
            o[k] = fmaf(p2, e1, fmaf(p1, dt, p0 * xc[k]));
            d1[k] = e1;
        }
        if (a.xstart) pass_st(a.xstart, i, x0);
        if (a.ubase_out) pass_st(a.ubase_out, i, xc);
        if (a.ud2_out) pass_st(a.ud2_out, i, d1);
        if (a.ud1_out) pass_st(a.ud1_out, i, x0);
        pass_st(a.sample, i, o);
    }
    if (nonfinite && a.err) atomicOr(a.err, VD_ERR_NONFINITE);
}

static int launch_unipc(const SamplerPassArgs& a, hipStream_t s) {
    const std::string k = "unipc_kernel: ";
    VD_REQUIRE(a.B > 0 && a.per > 0, k + "B and the elements per item must be positive");
    VD_REQUIRE(a.x && (a.eps || a.x0_given) && a.t && a.tab && a.sample, k + "null tensor");
    VD_REQUIRE(!a.mean, k + "the pass writes no posterior mean");
    VD_REQUIRE(a.urows, "unipc_sample: no coefficient rows for the bound schedule (vd_set_unipc_rows, after vd_set_schedule)");
    VD_REQUIRE((a.ubase != nullptr) == (a.ud1 != nullptr) && (a.ud1 != nullptr) == (a.ud2 != nullptr), k + "the state read is three tensors, or none");
    VD_REQUIRE((a.ubase_out != nullptr) == (a.ud1_out != nullptr) && (a.ud1_out != nullptr) == (a.ud2_out != nullptr), k + "the state written is three tensors, or none");
    VD_REQUIRE(a.count >= 0 && (a.ubase || a.count == 0), k + "a step count without a state");
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool v4 = a.per % 4 == 0 && al16(a.x) && al16(a.eps) && al16(a.x0_given) && al16(a.sample) && al16(a.xstart) && al16(a.ubase) && al16(a.ud1) &&
                    al16(a.ud2) && al16(a.ubase_out) && al16(a.ud1_out) && al16(a.ud2_out);
    const size_t groups = (size_t)a.B * (v4 ? a.per / 4 : a.per);
    const int grid = (int)std::min<size_t>((groups + 255) / 256, 4096);
    if (v4) hipLaunchKernelGGL(unipc_kernel<float4>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(unipc_kernel<float>, dim3(grid), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

int launch_sampler_pass(const SamplerPassArgs& a, hipStream_t s) {
    VD_REQUIRE(sampler_valid(a.sampler), "sampler pass: sampler");
    if (a.sampler == SAMPLER_DPMPP_2M_SDE) return launch_dpmpp_2m_sde(a, s);
    if (a.sampler == SAMPLER_UNIPC) return launch_unipc(a, s);
    const bool f4 = !sampler_draws_noise(a.sampler);        // the float4 passes; posterior_kernel takes any per and any alignment
    if (f4) {
        const std::string k = std::string(a.sampler == SAMPLER_DPMPP_2M ? "dpmpp_2m" : "ddim_reverse") + "_kernel: ";
        VD_REQUIRE(a.B > 0 && a.per > 0 && a.per % 4 == 0, k + "3*H*W elements per frame, a multiple of 4");
        auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        VD_REQUIRE(a.x && (a.eps || a.x0_given) && a.t && a.tab && a.sample, k + "null tensor");
        VD_REQUIRE(!sampler_has_history(a.sampler) || a.w, "dpmpp_2m_sample: no multistep weight row for the bound schedule (vd_set_multistep_weights, after vd_set_schedule)");
        VD_REQUIRE(al16(a.x) && al16(a.eps) && al16(a.x0_given) && al16(a.hist) && al16(a.sample) && al16(a.xstart), k + "16-byte aligned tensors");
    }
    const size_t groups = (size_t)a.B * (f4 ? a.per / 4 : a.per);
    const int grid = (int)std::min<size_t>((groups + 255) / 256, 4096);
    if (a.sampler == SAMPLER_DDIM_REVERSE) hipLaunchKernelGGL(deterministic_kernel<SAMPLER_DDIM_REVERSE>, dim3(grid), dim3(256), 0, s, a);
    else if (a.sampler == SAMPLER_DPMPP_2M) hipLaunchKernelGGL(deterministic_kernel<SAMPLER_DPMPP_2M>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(posterior_kernel, dim3(grid), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ classifier-free guidance on the observed frames (one pass)
// cfg_scale (this project's extension): out_c is the network output of the step, out_u the output of the same call with the observation
// mask zeroed; d = out_c - out_u (one fp32 subtraction), out_g = fmaf(w, d, out_u) (one fused multiply-add).  A d that is not finite
// comes out NaN whatever w is (w = 0 would otherwise hide an inf of out_c), so that the sampler pass behind it sets VD_ERR_NONFINITE.
// w = 0 hands out_u through as it is: the fma would turn a -0 of out_u into +0 whenever w d is +0.  Pure streaming: two reads and one
// write per element, four elements per thread and pass while the three tensors are 16-byte aligned, the n % 4 last ones (or, unaligned,
// all of them) one by one; out may alias out_c or out_u: the pass is elementwise.
// (cfg_combine_one lives in vd_common.h: the combine-and-moments pass of guidance.hip produces the same bits with it.)
__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* out_c, const float* out_u, float w, size_t n4, size_t n, float* out) {
    const float4* c4 = reinterpret_cast<const float4*>(out_c);
    const float4* u4 = reinterpret_cast<const float4*>(out_u);
    float4* o4 = reinterpret_cast<float4*>(out);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < n4; i += stride) {
        const float4 c = c4[i], u = u4[i];
        float4 o;
        o.x = cfg_combine_one(c.x, u.x, w);
        o.y = cfg_combine_one(c.y, u.y, w);
        o.z = cfg_combine_one(c.z, u.z, w);
        o.w = cfg_combine_one(c.w, u.w, w);
        o4[i] = o;
    }
    for (size_t j = 4 * n4 + tid; j < n; j += stride) out[j] = cfg_combine_one(out_c[j], out_u[j], w);
}

int launch_cfg_combine(const float* out_c, const float* out_u, float w, long long n, float* out, hipStream_t s) {
    VD_REQUIRE(out_c && out_u && out && n > 0, "cfg_combine_kernel: null tensor or no element");
    VD_REQUIRE(w == w && fabsf(w) <= 3.4028234e38f, "cfg_scale must be finite");
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const size_t n4 = al16(out_c) && al16(out_u) && al16(out) ? (size_t)n / 4 : 0;
    const size_t work = std::max<size_t>(n4, (size_t)n - 4 * n4);
    const int grid = (int)std::min<size_t>((work + 255) / 256, 4096);
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(grid), dim3(256), 0, s, out_c, out_u, w, n4, (size_t)n, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// q_sample (gaussian_diffusion.py:190-206)
__global__ __launch_bounds__(256) void q_sample_kernel(const float* x0, const float* noise, const int64_t* t,
                                                       const float* tab, int NT, size_t per, size_t total, float* out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        long long tt = t[i / per];
        if (tt < 0) tt += NT;                   // t-1 at t=0 wraps like numpy/torch indexing (gaussian_diffusion.py:565-568)
        if (tt < 0 || tt >= NT) { out[i] = __builtin_nanf(""); continue; }       // IndexError in the reference
        out[i] = fmaf(tab[TAB_SQRT_1M_ACP * NT + tt], noise[i], tab[TAB_SQRT_ACP * NT + tt] * x0[i]);   // (one rounding order for this kernel and q_sample_prev_kernel)
    }
}

int launch_q_sample(const float* x0, const float* noise, const int64_t* t, const float* tab, int num_timesteps, int B,
                    long per, float* out, hipStream_t s) {
    const size_t total = (size_t)B * per;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid), dim3(256), 0, s, x0, noise, t, tab, num_timesteps, (size_t)per,
                       total, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// The window executor's `observed_frames = 'x_t_minus_1'` (gaussian_diffusion.py:565-568: x_t_minus_1 = q_sample(x0, t - 1, fresh
// noise) before every step of p_sample_loop): t and the Philox {seed, offset} are read from device memory, the noise is
// element i of the stream at offset + draw_offset, index t - 1 = -1 wraps to the last entry like the reference's negative index.
__global__ __launch_bounds__(256) void q_sample_prev_kernel(const float* x0, const long long* t, const float* tab, int NT, size_t per, size_t total,
                                                            const unsigned long long* dstate, unsigned long long draw_offset, float* out) {
    const unsigned long long seed = dstate[0], offset = dstate[1] + draw_offset;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        long long tt = t[i / per] - 1;
        if (tt < 0) tt += NT;
        if (tt < 0 || tt >= NT) { out[i] = __builtin_nanf(""); continue; }
        out[i] = fmaf(tab[TAB_SQRT_1M_ACP * NT + tt], normal_at(seed, offset, i), tab[TAB_SQRT_ACP * NT + tt] * x0[i]);
    }
}

int launch_q_sample_prev(const float* x0, const int64_t* t, const float* tab, int num_timesteps, int B, long per, const unsigned long long* dstate,
                         unsigned long long draw_offset, float* out, hipStream_t s) {
    const size_t total = (size_t)B * per;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(q_sample_prev_kernel, dim3(grid), dim3(256), 0, s, x0, reinterpret_cast<const long long*>(t), tab, num_timesteps, (size_t)per,
                       total, dstate, draw_offset, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ NLL terms (gaussian_diffusion.py:750-790, losses.py)
__device__ __forceinline__ float approx_std_normal_cdf(float x) {          // losses.py:38-43
    return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

// grid (nblk, B): block (k, b) sums its slice of batch element b; thread-local and cross-thread sums in fp64, one partial
// triple per block (deterministic: no atomics), folded by vb_final_kernel.
__global__ __launch_bounds__(256) void vb_terms_kernel(VbArgs a) {
    const int b = blockIdx.y;
    const long long tl = a.t[b];
    const int NT = a.num_timesteps;
    const bool ok = tl >= 0 && tl < NT;
    const int t = ok ? (int)tl : 0;
    const float* tb = a.tab + t;
    const float sr = tb[TAB_SQRT_RECIP * NT], srm1 = tb[TAB_SQRT_RECIPM1 * NT], c1 = tb[TAB_COEF1 * NT], c2 = tb[TAB_COEF2 * NT];
    const float lv = tb[TAB_LOGVAR * NT], tlv = tb[TAB_POST_LOGVAR * NT];
    const float inv_stdv = expf(-0.5f * lv), e_dlv = expf(tlv - lv), e_mlv = expf(-lv);
    const long fsz = a.per / a.T;
    double s0 = 0, s1 = 0, s2 = 0;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < a.per; j += (long)gridDim.x * 256) {
        const size_t i = (size_t)b * a.per + j;
        const float xs = a.x_start[i], xt = a.x_t[i];
        float x0 = a.start_x ? a.eps[i] : sr * xt - srm1 * a.eps[i];  // START_X: pred_xstart = process_xstart(model_output) (gaussian_diffusion.py:326-341)
        const bool bad = !(fabsf(x0) <= 3.4028234e38f);               // (posterior_kernel: a non-finite eps must not be clamped into range)
        if (bad && a.err) atomicOr(a.err, VD_ERR_NONFINITE);
        if (a.clip && !bad) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        if (a.pred_xstart) a.pred_xstart[i] = ok ? x0 : __builtin_nanf("");
        const float mean = c1 * x0 + c2 * xt, tmean = c1 * xs + c2 * xt;
        const float m = a.mask ? a.mask[(size_t)b * a.T + j / fsz] : 1.0f;
        float term;
        if (t == 0) {                                                      // decoder NLL (losses.py:46-76)
            const float cx = xs - mean;
            const float cdf_plus = approx_std_normal_cdf(inv_stdv * (cx + 1.0f / 255.0f));
            const float cdf_min = approx_std_normal_cdf(inv_stdv * (cx - 1.0f / 255.0f));
            const float lp = xs < -0.999f ? logf(fmaxf(cdf_plus, 1e-12f))
                           : xs > 0.999f ? logf(fmaxf(1.0f - cdf_min, 1e-12f)) : logf(fmaxf(cdf_plus - cdf_min, 1e-12f));
            term = -lp;
        } else {                                                           // KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) (losses.py:13-35)
            const float d = tmean - mean;
            term = 0.5f * (-1.0f + lv - tlv + e_dlv + d * d * e_mlv);
        }
        s0 += (double)(term * m);
        const float dx = x0 - xs;
        s1 += (double)(dx * dx * m);
        if (a.noise) {
            const float e2 = (sr * xt - x0) / srm1 - a.noise[i];           // _predict_eps_from_xstart (gaussian_diffusion.py:392-396)
            s2 += (double)(e2 * e2 * m);
        }
    }
    if (!ok && a.err && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.err, VD_ERR_TIMESTEP);   // (eps_mse_kernel: one thread per item; no map_t_kernel on this path)
    __shared__ double red[3][256];
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 3) a.part[((size_t)b * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = ok ? red[threadIdx.x][0] : __builtin_nan("");
}

__global__ void vb_final_kernel(const double* part, int nblk, double per, float* vb, float* xstart_mse, float* mse, float scale0) {
    const int b = blockIdx.x;                                               // launched with one thread per item
    double s[3] = {0, 0, 0};
    for (int k = 0; k < nblk; ++k)
        for (int q = 0; q < 3; ++q) s[q] += part[((size_t)b * nblk + k) * 3 + q];
    if (vb) vb[b] = (float)(s[0] / per) * scale0;                           // mean_flat(...) / ln 2
    if (xstart_mse) xstart_mse[b] = (float)(s[1] / per);
    if (mse) mse[b] = (float)(s[2] / per);
}

int vb_terms_blocks(long per) { return (int)std::max<long>(1, std::min<long>(64, (per + 256 * 16 - 1) / (256 * 16))); }

int launch_vb_terms(const VbArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(vb_terms_kernel, dim3(a.nblk, a.B), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(vb_final_kernel, dim3(a.B), dim3(1), 0, s, a.part, a.nblk, (double)a.per, a.vb, a.xstart_mse,
                       a.noise ? a.mse : nullptr, 1.4426950408889634f);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ observed-frame search (scripts/video_optimal_schedule.py)
// The search ranks candidates by calc_bpd_loop_subsampled's `mse` alone (gaussian_diffusion.py:975-990): the KL / decoder-NLL
// terms of vb_terms_kernel are never read, and only latent frames count.  Noise is item b's own Philox stream
// (seed, item_offset[b]) -- element j is what vd_randn(out, per, seed, item_offset[b]) writes at j -- so x_t needs no noise tensor.

// x_t = q_sample(x_start, t[b], noise) with q_sample_kernel's rounding; a thread = one quad of one item (per % 4 == 0)
__global__ __launch_bounds__(256) void score_q_sample_kernel(ScoreArgs a, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long tl = a.t[b];
    const int NT = a.num_timesteps;
    const bool ok = tl >= 0 && tl < NT;
    const float sa = ok ? a.tab[TAB_SQRT_ACP * NT + tl] : 0.f, s1 = ok ? a.tab[TAB_SQRT_1M_ACP * NT + tl] : 0.f;
    const unsigned long long off = a.noise ? 0ull : a.item_offset[b];
    const long nq = a.per / 4;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const size_t i4 = ((size_t)b * a.per) / 4 + q;
        f32x4 o;
        if (ok) {
            const f32x4 xs = reinterpret_cast<const f32x4*>(a.x_start)[i4];
            const f32x4 z = a.noise ? reinterpret_cast<const f32x4*>(a.noise)[i4] : normal4_at(a.seed, off, (unsigned long long)q);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaf(s1, z[e], sa * xs[e]);
        } else {
            const float nanv = __builtin_nanf("");                  // IndexError in the reference (q_sample_kernel)
            o = f32x4{nanv, nanv, nanv, nanv};
        }
        reinterpret_cast<f32x4*>(out)[i4] = o;
    }
}

// grid (nblk, B): block (k, b) sums its slice of item b over the LATENT frames, noise and x_t regenerated in registers, pred_xstart as
// vb_terms_kernel forms it; fp64 sums, one partial per block (no atomics in the sum), folded in block order by eps_mse_final_kernel.
__global__ __launch_bounds__(256) void eps_mse_kernel(ScoreArgs a) {
    const int b = blockIdx.y;
    const long long tl = a.t[b];
    const int NT = a.num_timesteps;
    const bool ok = tl >= 0 && tl < NT;
    const int t = ok ? (int)tl : 0;
    const float* tb = a.tab + t;
    const float sr = tb[TAB_SQRT_RECIP * NT], srm1 = tb[TAB_SQRT_RECIPM1 * NT], sa = tb[TAB_SQRT_ACP * NT], s1 = tb[TAB_SQRT_1M_ACP * NT];
    const unsigned long long off = a.noise ? 0ull : a.item_offset[b];
    const long fq = a.per / a.T / 4, nq = a.per / 4;               // quads per frame / per item: a quad never straddles two frames
    double s = 0;
    bool bad_any = false;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float m = a.mask[(size_t)b * a.T + q / fq];
        if (m == 0.f) continue;                                     // observed and padding frames: nothing is read
        const size_t i4 = ((size_t)b * a.per) / 4 + q;
        const f32x4 xs = reinterpret_cast<const f32x4*>(a.x_start)[i4], ev = reinterpret_cast<const f32x4*>(a.eps)[i4];
        const f32x4 z = a.noise ? reinterpret_cast<const f32x4*>(a.noise)[i4] : normal4_at(a.seed, off, (unsigned long long)q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xt = fmaf(s1, z[e], sa * xs[e]);
            float x0 = a.start_x ? ev[e] : sr * xt - srm1 * ev[e];
            const bool bad = !(fabsf(x0) <= 3.4028234e38f);         // (vb_terms_kernel: never clamp a non-finite output into range)
            bad_any |= bad;
            if (a.clip && !bad) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
            const double d = (double)((sr * xt - x0) / srm1 - z[e]);    // _predict_eps_from_xstart - noise
            s += d * d * (double)m;
        }
    }
    if (a.err) {
        if (bad_any && ok) atomicOr(a.err, VD_ERR_NONFINITE);     // (an item with a bad t is NaN already: bit 0 says why)
        if (!ok && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.err, VD_ERR_TIMESTEP);
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.part[(size_t)b * gridDim.x + blockIdx.x] = ok ? red[0] : __builtin_nan("");
}

__global__ void eps_mse_final_kernel(const double* __restrict__ part, int nblk, int B, double per, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0;
    for (int k = 0; k < nblk; ++k) s += part[(size_t)b * nblk + k];
    out[b] = s / per;                                               // mean_flat(tensor, mask): over ALL T*3*H*W elements
}

static int score_args_ok(const ScoreArgs& a) {
    VD_REQUIRE(a.per % (4 * a.T) == 0, "score: frames in 16-byte units");
    VD_REQUIRE(((uintptr_t)a.x_start | (uintptr_t)a.eps | (uintptr_t)a.noise) % 16 == 0, "score: tensors aligned to 16 bytes");
    return 0;
}

int launch_score_q_sample(const ScoreArgs& a, float* x_t, hipStream_t s) {
    if (int rc = score_args_ok(a)) return rc;
    VD_REQUIRE((uintptr_t)x_t % 16 == 0, "score: tensors aligned to 16 bytes");
    const int gx = (int)std::max<long>(1, std::min<long>(256, (a.per / 4 + 255) / 256));
    hipLaunchKernelGGL(score_q_sample_kernel, dim3(gx, a.B), dim3(256), 0, s, a, x_t);
    VD_HIP(hipGetLastError());
    return 0;
}

int launch_eps_mse(const ScoreArgs& a, double* mse_out, hipStream_t s) {
    if (int rc = score_args_ok(a)) return rc;
    hipLaunchKernelGGL(eps_mse_kernel, dim3(a.nblk, a.B), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(eps_mse_final_kernel, dim3((a.B + 63) / 64), dim3(64), 0, s, a.part, a.nblk, a.B, (double)a.per, mse_out);
    VD_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void prior_bpd_kernel(const float* x_start, const float* mask, const float* tab, int NT, int T,
                                                        long per, double* part) {
    const int b = blockIdx.y;
    const float sa = tab[TAB_SQRT_ACP * NT + NT - 1], lv = tab[TAB_LOG_1M_ACP * NT + NT - 1];
    const float ev = expf(lv);
    const long fsz = per / T;
    double s0 = 0;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < per; j += (long)gridDim.x * 256) {
        const float mu = sa * x_start[(size_t)b * per + j];
        const float m = mask ? mask[(size_t)b * T + j / fsz] : 1.0f;
        s0 += (double)(0.5f * (-1.0f - lv + ev + mu * mu) * m);              // normal_kl(mean, logvar, 0, 0)
    }
    __shared__ double red[256];
    red[threadIdx.x] = s0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)b * gridDim.x + blockIdx.x) * 3;
        p[0] = red[0]; p[1] = 0; p[2] = 0;
    }
}

int launch_prior_bpd(const float* x_start, const float* mask, const float* tab, int num_timesteps, int B, int T, long per,
                     double* part, int nblk, float* out, hipStream_t s) {
    hipLaunchKernelGGL(prior_bpd_kernel, dim3(nblk, B), dim3(256), 0, s, x_start, mask, tab, num_timesteps, T, per, part);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(vb_final_kernel, dim3(B), dim3(1), 0, s, part, nblk, (double)per, out, nullptr, nullptr, 1.4426950408889634f);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
