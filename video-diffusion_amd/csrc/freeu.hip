// FreeU (this project's extension; Si, Huang, Jiang, Liu: "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024): the two operators the
// decoder applies to the halves of a concat at its two lowest-resolution stages -- the spectral filter of the skip half and the scaling
// of the backbone half.  Tensors are channels-last [N][S*S][C] as everywhere in the forward; both passes are L2-bound on tensors of a
// few MB and need no matrix pipe.  Everything that is summed is summed in fp64 in a fixed order, without atomics: equal inputs give
// equal bits.
#include "vd_common.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace vd {

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// cos(2 pi k / S) | sin(2 pi k / S), k = 0 .. S-1, in double on the host (2 S values)
void freeu_trig_table(int S, double* out) {
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < S; ++k) { out[k] = std::cos(2.0 * pi * k / S); out[S + k] = std::sin(2.0 * pi * k / S); }
}

// ------------------------------------------------------------------ freeu_filter_kernel
// x' = Re ifft2(M . fft2(x)) per (frame, channel) plane with M = s on the four bins (u, v) in {0, S-1}^2 and 1 elsewhere, in its closed
// form: with theta = 2 pi / S,
//   x'[i,j] = x[i,j] + (s-1)/S^2 (m0 + ci cos(theta i) + si sin(theta i) + cj cos(theta j) + sj sin(theta j) + cd cos(theta (i+j)) + sd sin(theta (i+j)))
// where m0 = sum x, (ci, si) = sum x (cos, sin)(theta i'), (cj, sj) the same in j', (cd, sd) the same in i' + j' -- a rank-7 update.
// A block owns one frame and FU_CH consecutive channels: FU_CH/4 channel quads (a float4 each, contiguous across the quads of a pixel)
// times FU_SL pixel slices; slice r walks the pixels r, r + FU_SL, ...  Pass 1: the seven sums of a thread's four channels over its
// pixels, fp64, then over the slices in slice order through LDS.  Pass 2: the same thread re-reads its pixels (L2 / L1 by now) and
// writes x' rounded once to fp32.
constexpr int FU_CH = 32, FU_QUADS = FU_CH / 4, FU_SL = 32, FU_THREADS = FU_QUADS * FU_SL;

__global__ __launch_bounds__(FU_THREADS) void freeu_filter_kernel(const float* __restrict__ x, int S, int C, double k, const double* __restrict__ trig,
                                                                  float* __restrict__ y) {
    __shared__ double part[FU_SL][7][FU_CH];       // 56 KB
    __shared__ double tot[7][FU_CH];
    const int n = blockIdx.y, c0 = blockIdx.x * FU_CH;
    const int q = threadIdx.x % FU_QUADS, r = threadIdx.x / FU_QUADS, c = c0 + 4 * q;
    const bool live = c < C;                        // (C % 4 == 0: a quad is inside the tensor or outside it)
    const int HW = S * S;
    const float* xf = x + (size_t)n * HW * C;
    float* yf = y + (size_t)n * HW * C;
    const double* cs = trig;
    const double* sn = trig + S;
    double acc[7][4];
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][e] = 0.0;
    if (live) {
        for (int p = r; p < HW; p += FU_SL) {
            const int i = p / S, j = p - i * S, d = i + j < S ? i + j : i + j - S;
            const float4 v4 = *reinterpret_cast<const float4*>(xf + (size_t)p * C + c);
            const double v[4] = {v4.x, v4.y, v4.z, v4.w};
            const double w[6] = {cs[i], sn[i], cs[j], sn[j], cs[d], sn[d]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][e] += v[e];
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[1 + a][e] = fma(v[e], w[a], acc[1 + a][e]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[r][a][4 * q + e] = acc[a][e];
    __syncthreads();
    if (threadIdx.x < 7 * FU_CH) {
        const int a = threadIdx.x / FU_CH, ch = threadIdx.x % FU_CH;
        double s = 0.0;
        for (int rr = 0; rr < FU_SL; ++rr) s += part[rr][a][ch];
        tot[a][ch] = s;
    }
    __syncthreads();
    if (!live) return;
    double t[7][4];
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) t[a][e] = tot[a][4 * q + e];
    for (int p = r; p < HW; p += FU_SL) {
        const int i = p / S, j = p - i * S, d = i + j < S ? i + j : i + j - S;
        const float4 v4 = *reinterpret_cast<const float4*>(xf + (size_t)p * C + c);
        const double v[4] = {v4.x, v4.y, v4.z, v4.w};
        const double w[6] = {cs[i], sn[i], cs[j], sn[j], cs[d], sn[d]};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double u = t[0][e];
#pragma unroll
            for (int a = 0; a < 6; ++a) u = fma(t[1 + a][e], w[a], u);
            o[e] = (float)fma(k, u, v[e]);
        }
        *reinterpret_cast<float4*>(yf + (size_t)p * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

int launch_freeu_filter(const float* x, int N, int S, int C, double s, const double* trig, float* y, hipStream_t st) {
    VD_REQUIRE(x && y && x != y, "freeu_filter_kernel: null tensor, or in place (the skip tensors are not the filter's to write)");
    VD_REQUIRE(N > 0 && N <= 65535 && S <= 4096 && C > 0 && C % 4 == 0, "freeu_filter_kernel: shape (C a multiple of 4)");
    VD_REQUIRE(S >= 2, "freeu_filter_kernel: S >= 2 (at one pixel the four bins coincide and the published box is empty)");
    VD_REQUIRE(s == s && std::fabs(s) <= 1.7976931348623157e308, "freeu_filter_kernel: s must be finite");
    VD_REQUIRE(al16(x) && al16(y), "freeu_filter_kernel: tensors must be 16-byte aligned");
    if (s == 1.0) {                                 // the identity, to the bit (a -0.f would not survive x + 0 * u)
        VD_HIP(hipMemcpyAsync(y, x, (size_t)N * S * S * C * sizeof(float), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    VD_REQUIRE(trig, "freeu_filter_kernel: no cos / sin table");
    const double k = (s - 1.0) / ((double)S * S);
    hipLaunchKernelGGL(freeu_filter_kernel, dim3((C + FU_CH - 1) / FU_CH, N), dim3(FU_THREADS), 0, st, x, S, C, k, trig, y);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ freeu_mean_kernel
// The structure map of the adaptive form: m[n][p] = mean over ALL C channels of h[n][p][:], fp64.  One wavefront per pixel: lane l sums
// the quads l, l + 64, ... in order, then the butterfly over the 64 lanes (a fixed tree); lane 0 writes.
__global__ __launch_bounds__(256) void freeu_mean_kernel(const float* __restrict__ h, long long pixels, int C, double* __restrict__ m) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long p = wave; p < pixels; p += nwaves) {
        const float* row = h + (size_t)p * C;
        double s = 0.0;
        for (int c = 4 * lane; c < C; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(row + c);
            s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) m[p] = s / (double)C;
    }
}

// ------------------------------------------------------------------ freeu_backbone_kernel
// Channels c < C/2 of h are scaled, the others copied.  Plain (m == null): one fp32 multiply by (float)b.  Adaptive: by
// (b - 1) g + 1 with g = (m - lo) / (hi - lo), lo and hi the minimum and maximum of the frame's map, all in fp64, the product rounded
// once; hi == lo gives g = 0 (the published code divides 0 by 0 there).  A block owns a frame (blockIdx.y) and a run of its quads; every
// block of a frame reduces the frame's map itself (S*S doubles out of L2): min and max do not depend on the order.
__global__ __launch_bounds__(256) void freeu_backbone_kernel(const float* __restrict__ h, int HW, int C, double b, const double* __restrict__ m,
                                                             float* __restrict__ y) {
    __shared__ double red[2][4];
    const int n = blockIdx.y, H = C / 2, qpp = C / 4;
    const float* hf = h + (size_t)n * HW * C;
    float* yf = y + (size_t)n * HW * C;
    const double* mf = m ? m + (size_t)n * HW : nullptr;
    double lo = 0.0, inv = 0.0;
    if (mf) {
        double mn = mf[0], mx = mf[0];
        for (int p = threadIdx.x; p < HW; p += 256) { mn = fmin(mn, mf[p]); mx = fmax(mx, mf[p]); }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o, 64)); mx = fmax(mx, __shfl_xor(mx, o, 64)); }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
        __syncthreads();
        mn = fmin(fmin(red[0][0], red[0][1]), fmin(red[0][2], red[0][3]));
        mx = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
        lo = mn;
        inv = mx - mn;                               // the divisor (0: g = 0)
    }
    const float bf = (float)b;
    const long long quads = (long long)HW * qpp;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < quads; g += (long long)gridDim.x * 256) {
        const int p = (int)(g / qpp), c = 4 * (int)(g - (long long)p * qpp);
        const float4 v4 = *reinterpret_cast<const float4*>(hf + (size_t)g * 4);
        float v[4] = {v4.x, v4.y, v4.z, v4.w};
        if (c < H) {
            if (mf) {
                const double gg = inv != 0.0 ? (mf[p] - lo) / inv : 0.0;
                const double f = fma(b - 1.0, gg, 1.0);
#pragma unroll
                for (int e = 0; e < 4; ++e) if (c + e < H) v[e] = (float)((double)v[e] * f);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (c + e < H) v[e] = v[e] * bf;
            }
        }
        *reinterpret_cast<float4*>(yf + (size_t)g * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

int launch_freeu_backbone(const float* h, int N, int S, int C, double b, int adaptive, double* map, float* y, hipStream_t st) {
    VD_REQUIRE(h && y && h != y, "freeu_backbone_kernel: null tensor, or in place");
    VD_REQUIRE(N > 0 && N <= 65535 && S > 0 && S <= 4096 && C > 0 && C % 4 == 0, "freeu_backbone_kernel: shape (C a multiple of 4)");
    VD_REQUIRE(b == b && std::fabs(b) <= 1.7976931348623157e308, "freeu_backbone_kernel: b must be finite");
    VD_REQUIRE(al16(h) && al16(y), "freeu_backbone_kernel: tensors must be 16-byte aligned");
    VD_REQUIRE(!adaptive || map, "freeu_backbone_kernel: the adaptive form needs N * S * S doubles for the structure map");
    const int HW = S * S;
    if (adaptive) {
        const long long pixels = (long long)N * HW;
        hipLaunchKernelGGL(freeu_mean_kernel, dim3((unsigned)std::min<long long>((pixels + 3) / 4, 8192)), dim3(256), 0, st, h, pixels, C, map);
        VD_HIP(hipGetLastError());
    }
    const long long quads = (long long)HW * (C / 4);
    const int gx = (int)std::min<long long>((quads + 255) / 256, 64);
    hipLaunchKernelGGL(freeu_backbone_kernel, dim3(gx, N), dim3(256), 0, st, h, HW, C, b, adaptive ? map : nullptr, y);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
