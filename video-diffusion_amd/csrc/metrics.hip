// Per-frame SSIM and PSNR of a predicted video against its ground truth, and the paired squared distance of two sets of LPIPS
// embeddings, gfx950: the arithmetic of the reference's scripts/video_eval.py (compute_metrics_lazy :205-225, compute_lpips_lazy
// :228-252), which calls scikit-image 0.19.3 `structural_similarity` / `peak_signal_noise_ratio` and `lpips.LPIPS` per frame.
//
// Per channel plane, gt x in [0, 1] (float32), prediction y (float32, or uint8 read as (float)u / 255.0f -- the float32 image of
// u / 255.0 for all 256 values):
//   PSNR = 10 log10(1 / mse), mse = mean over the plane of (x - y)^2, the difference and its square in float32 (what skimage's float32
//          images give), the sum in float64; mse = 0 gives +inf.
//   SSIM = mean over the (H - 6)(W - 6) windows that lie wholly inside the plane (skimage crops 3 pixels per side, so its filter's
//          border mode never shows) of S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) with the 7 x 7 means
//          ux, uy, uxx, uyy, uxy, v* = 49/48 (u** - u* u*), C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = ssim_data_range.
// and per frame the mean over the C planes.
//
// ssim_strip_kernel: one block per (plane, strip of rows).  The strip's rows of x and y (its output rows + a 6-row halo; consecutive
// rows of a plane are one contiguous span, fetched with 16-byte loads where the alignment allows) are staged in LDS once, the
// squared error of the rows the strip owns is reduced from the same registers, and each thread then walks one output column of a
// run of rows: the five 7-tap row sums (x, y, xx, yy, xy) of the row that enters the window are formed from LDS (lane j reads
// columns j .. j + 6: consecutive lanes, consecutive banks), added to the running column sums, and the row sums that leave -- kept in
// a 7-deep register ring -- subtracted.  Every sum is float64: the products of float32 values are exact there and the variance
// terms cancel.  S is evaluated in float64 as well.  Each block writes two doubles (sum of S, sum of squared error) to a
// partials table; metrics_final_kernel adds a plane's partials in strip order, so there is no atomic and the result of a frame
// does not depend on what else is in the launch.  Traffic: gt and prediction are each read once (+ 6 halo rows per strip); 2 N doubles are written.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "../../include/vd_amd.h"
#include "vd_common.h"

namespace vd {
namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WIN = 7;                       // skimage's default win_size
constexpr int MT_TILE_ROWS = 32;                // rows of a strip in LDS (26 output rows + the 6-row halo)
constexpr int MT_LDS_BYTES = 60 * 1024;         // both planes of a strip (+ 4 KiB of reduction scratch: 64 KiB per block)
constexpr int MT_MAX_W = 1024;                  // 7 rows x 1024 x 2 planes x 4 B = 56 KiB

struct MetricsArgs {
    const float* gt;
    const void* pred;
    int pred_u8;
    int H, W;
    int rows_tile;       // input rows of a full strip
    int nstrips;
    int groups;          // row runs a strip's output rows are cut into (threads = groups x (W - 6) work items)
    double C1, C2;
    double* part;        // [plane][strip][2]
};

// fixed-order block sum of two doubles per thread; result valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
    const int tid = threadIdx.x;
    red[tid] = a;
    red[MT_THREADS + tid] = b;
    __syncthreads();
    for (int w = MT_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            red[tid] += red[tid + w];
            red[MT_THREADS + tid] += red[MT_THREADS + tid + w];
        }
        __syncthreads();
    }
    a = red[0];
    b = red[MT_THREADS];
}

// floats of one plane's tile, rounded so that the second plane starts 16-byte aligned
__host__ __device__ __forceinline__ int plane_floats(int rows_tile, int W) { return (rows_tile * W + 3) & ~3; }
inline int tile_rows(int W) { return std::min(MT_TILE_ROWS, (MT_LDS_BYTES - 16) / (2 * 4 * W)); }

__device__ __forceinline__ float u8f(unsigned v) { return (float)v / 255.0f; }

__global__ __launch_bounds__(MT_THREADS) void ssim_strip_kernel(MetricsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ double red[2 * MT_THREADS];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / a.nstrips, strip = blockIdx.x - plane * a.nstrips;
    const int W = a.W, H = a.H;
    const int out_step = a.rows_tile - (MT_WIN - 1);
    const int r0 = strip * out_step;
    const int rows = min(a.rows_tile, H - r0);              // input rows staged (>= 7)
    const int out_rows = rows - (MT_WIN - 1);
    // squared error: a strip owns its first out_step rows; the last strip owns all it stages
    const int own = (strip == a.nstrips - 1) ? rows * W : out_step * W;
    const int count = rows * W;
    float* tx = tile;
    float* ty = tile + plane_floats(a.rows_tile, W);
    const size_t base = ((size_t)plane * H + r0) * W;
    const float* gx = a.gt + base;
    double se = 0.0;

    const bool vec4 = ((reinterpret_cast<uintptr_t>(gx) & 15) == 0) && (count % 4 == 0) && (own % 4 == 0);
    if (a.pred_u8) {
        const unsigned char* gy = static_cast<const unsigned char*>(a.pred) + base;
        if (vec4 && (reinterpret_cast<uintptr_t>(gy) & 3) == 0) {
            for (int i = tid * 4; i < count; i += MT_THREADS * 4) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(gx + i);
                const unsigned u = *reinterpret_cast<const unsigned*>(gy + i);
                f32x4 y;
                y.x = u8f(u & 255u); y.y = u8f((u >> 8) & 255u); y.z = u8f((u >> 16) & 255u); y.w = u8f(u >> 24);
                *reinterpret_cast<f32x4*>(tx + i) = x;
                *reinterpret_cast<f32x4*>(ty + i) = y;
                if (i < own) {
                    const f32x4 d = x - y;
                    se += (double)(d.x * d.x); se += (double)(d.y * d.y); se += (double)(d.z * d.z); se += (double)(d.w * d.w);
                }
            }
        } else {
            for (int i = tid; i < count; i += MT_THREADS) {
                const float x = gx[i], y = u8f(gy[i]);
                tx[i] = x; ty[i] = y;
                if (i < own) { const float d = x - y; se += (double)(d * d); }
            }
        }
    } else {
        const float* gy = static_cast<const float*>(a.pred) + base;
        if (vec4 && (reinterpret_cast<uintptr_t>(gy) & 15) == 0) {
            for (int i = tid * 4; i < count; i += MT_THREADS * 4) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(gx + i);
                const f32x4 y = *reinterpret_cast<const f32x4*>(gy + i);
                *reinterpret_cast<f32x4*>(tx + i) = x;
                *reinterpret_cast<f32x4*>(ty + i) = y;
                if (i < own) {
                    const f32x4 d = x - y;
                    se += (double)(d.x * d.x); se += (double)(d.y * d.y); se += (double)(d.z * d.z); se += (double)(d.w * d.w);
                }
            }
        } else {
            for (int i = tid; i < count; i += MT_THREADS) {
                const float x = gx[i], y = gy[i];
                tx[i] = x; ty[i] = y;
                if (i < own) { const float d = x - y; se += (double)(d * d); }
            }
        }
    }
    __syncthreads();

    const int ncols = W - (MT_WIN - 1);
    const int run = (out_rows + a.groups - 1) / a.groups;    // output rows per work item
    const int items = a.groups * ncols;
    const double inv = 1.0 / (MT_WIN * MT_WIN), cov = (double)(MT_WIN * MT_WIN) / (MT_WIN * MT_WIN - 1);
    double ssum = 0.0;
    for (int it = tid; it < items; it += MT_THREADS) {
        const int g = it / ncols, j = it - g * ncols;
        const int o0 = g * run, o1 = min(o0 + run, out_rows);  // output rows [o0, o1): input rows [o0, o1 + 6)
        if (o0 >= o1) continue;
        const int nwalk = o1 - o0 + (MT_WIN - 1);
        double ring[MT_WIN][5];
#pragma unroll
        for (int k = 0; k < MT_WIN; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) ring[k][q] = 0.0;
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int rb = 0; rb < nwalk; rb += MT_WIN) {
#pragma unroll
            for (int k = 0; k < MT_WIN; ++k) {
                const int r = rb + k;
                if (r < nwalk) {
                    const float* px = tx + (o0 + r) * W + j;
                    const float* py = ty + (o0 + r) * W + j;
                    double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int t = 0; t < MT_WIN; ++t) {
                        const double x = (double)px[t], y = (double)py[t];
                        h[0] += x; h[1] += y; h[2] += x * x; h[3] += y * y; h[4] += x * y;
                    }
#pragma unroll
                    for (int q = 0; q < 5; ++q) { v[q] += h[q] - ring[k][q]; ring[k][q] = h[q]; }
                    if (r >= MT_WIN - 1) {
                        const double ux = v[0] * inv, uy = v[1] * inv, uxx = v[2] * inv, uyy = v[3] * inv, uxy = v[4] * inv;
                        const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
                        const double A1 = 2.0 * ux * uy + a.C1, A2 = 2.0 * vxy + a.C2;
                        const double B1 = ux * ux + uy * uy + a.C1, B2 = vx + vy + a.C2;
                        ssum += (A1 * A2) / (B1 * B2);
                    }
                }
            }
        }
    }
    block_sum2(ssum, se, red);
    if (tid == 0) {
        double* p = a.part + ((size_t)plane * a.nstrips + strip) * 2;
        p[0] = ssum;
        p[1] = se;
    }
}

// one thread per frame: a plane's partials in strip order, then the channel mean
__global__ void metrics_final_kernel(const double* part, int N, int C, int nstrips, double n_win, double n_pix, double* ssim, double* psnr) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s_acc = 0.0, p_acc = 0.0;
    for (int c = 0; c < C; ++c) {
        const double* p = part + ((size_t)n * C + c) * nstrips * 2;
        double s = 0.0, e = 0.0;
        for (int k = 0; k < nstrips; ++k) { s += p[2 * k]; e += p[2 * k + 1]; }
        s_acc += s / n_win;
        const double mse = e / n_pix;
        p_acc += mse == 0.0 ? (double)__builtin_inff() : 10.0 * log10(1.0 / mse);
    }
    ssim[n] = s_acc / C;
    psnr[n] = p_acc / C;
}

// block n: out[n] = sum_d (a[n][d] - b[n][d])^2, the differences and the sum in float64, fixed order
__global__ __launch_bounds__(MT_THREADS) void pair_sqdist_kernel(const float* a, const float* b, long long D, double* out) {
    __shared__ double red[2 * MT_THREADS];
    const int tid = threadIdx.x;
    const float* x = a + (size_t)blockIdx.x * D;
    const float* y = b + (size_t)blockIdx.x * D;
    double s = 0.0, unused = 0.0;
    if (D % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* y4 = reinterpret_cast<const f32x4*>(y);
        for (long long k = tid; k < D / 4; k += MT_THREADS) {
            const f32x4 u = x4[k], w = y4[k];
            const double d0 = (double)u.x - (double)w.x, d1 = (double)u.y - (double)w.y;
            const double d2 = (double)u.z - (double)w.z, d3 = (double)u.w - (double)w.w;
            s += d0 * d0; s += d1 * d1; s += d2 * d2; s += d3 * d3;
        }
    } else {
        for (long long k = tid; k < D; k += MT_THREADS) {
            const double d = (double)x[k] - (double)y[k];
            s += d * d;
        }
    }
    block_sum2(s, unused, red);
    if (tid == 0) out[blockIdx.x] = s;
}

// the partials table: one per device, grown on demand, owned by the library (hipFree waits for the device, so a launch that
// still reads the old table has finished before it goes)
struct MetricsWs {
    double* part = nullptr;
    size_t doubles = 0;
};
MetricsWs g_ws[64];
std::mutex g_ws_mutex;

}  // namespace
}  // namespace vd

using namespace vd;

extern "C" {

int vd_frame_metrics_plan(int H, int W, int* rows_tile, int* nstrips, int* groups) {
    VD_REQUIRE(H >= MT_WIN && W >= MT_WIN, "frame metrics: SSIM's 7 x 7 window needs H >= 7 and W >= 7");
    VD_REQUIRE(W <= MT_MAX_W, "frame metrics: frames are at most 1024 pixels wide (7 rows of both planes must fit the LDS tile)");
    VD_REQUIRE(rows_tile && nstrips && groups, "null argument");
    *rows_tile = tile_rows(W);
    const int out_step = *rows_tile - (MT_WIN - 1);
    *nstrips = (H - (MT_WIN - 1) + out_step - 1) / out_step;
    const int ncols = W - (MT_WIN - 1);
    *groups = std::max(1, std::min(MT_THREADS / ncols, std::min(*rows_tile, H) - (MT_WIN - 1)));
    return 0;
}

int vd_frame_metrics(int N, int C, int H, int W, const float* gt, const void* pred, int pred_is_u8, double ssim_data_range,
                     double* ssim_out, double* psnr_out, void* stream) {
    VD_REQUIRE(N >= 0 && C >= 1, "frame metrics: N >= 0 frames of C >= 1 channel planes");
    MetricsArgs a{};
    if (int rc = vd_frame_metrics_plan(H, W, &a.rows_tile, &a.nstrips, &a.groups)) return rc;
    VD_REQUIRE(gt && pred && ssim_out && psnr_out, "null argument");
    VD_REQUIRE(ssim_data_range > 0.0, "frame metrics: ssim_data_range must be positive");
    VD_REQUIRE((reinterpret_cast<uintptr_t>(gt) & 3) == 0 && (pred_is_u8 || (reinterpret_cast<uintptr_t>(pred) & 3) == 0),
               "frame metrics: float planes must be 4-byte aligned");
    if (N == 0) return 0;
    a.gt = gt; a.pred = pred; a.pred_u8 = pred_is_u8 ? 1 : 0;
    a.H = H; a.W = W;
    a.C1 = (0.01 * ssim_data_range) * (0.01 * ssim_data_range);
    a.C2 = (0.03 * ssim_data_range) * (0.03 * ssim_data_range);
    const long long blocks = (long long)N * C * a.nstrips;
    VD_REQUIRE(blocks <= 0x7fffffffLL, "frame metrics: N * C * strips exceeds the grid limit (2^31 - 1 blocks): split the call");
    int dev = 0;
    VD_HIP(hipGetDevice(&dev));
    VD_REQUIRE(dev >= 0 && dev < 64, "device ordinal beyond the per-device workspace table");
    {
        std::lock_guard<std::mutex> lock(g_ws_mutex);
        MetricsWs& ws = g_ws[dev];
        if (int rc = grow_ws(&ws.part, &ws.doubles, (size_t)blocks * 2)) return rc;
        a.part = ws.part;
    }
    const size_t lds = (size_t)2 * plane_floats(a.rows_tile, W) * sizeof(float);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ssim_strip_kernel, dim3((unsigned)blocks), dim3(MT_THREADS), lds, st, a);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(metrics_final_kernel, dim3((N + 63) / 64), dim3(64), 0, st, a.part, N, C, a.nstrips,
                       (double)(H - (MT_WIN - 1)) * (W - (MT_WIN - 1)), (double)H * W, ssim_out, psnr_out);
    VD_HIP(hipGetLastError());
    return 0;
}

// Test hook, as vd_scratch_fill: the current device's partials table -- one pair per block, stored by ssim_strip_kernel and folded by
// metrics_final_kernel in the same call -- set to `byte`.  The table's address stays.
int vd_frame_metrics_scratch_fill(int byte, long long* bytes_filled) {
    VD_REQUIRE(bytes_filled && byte >= 0 && byte <= 255, "scratch_fill: a byte 0..255 and where to report the bytes");
    *bytes_filled = 0;
    int dev = 0;
    VD_HIP(hipGetDevice(&dev));
    VD_REQUIRE(dev >= 0 && dev < 64, "device ordinal beyond the per-device workspace table");
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    MetricsWs& ws = g_ws[dev];
    VD_HIP(hipDeviceSynchronize());
    if (ws.part && ws.doubles) VD_HIP(hipMemset(ws.part, byte, ws.doubles * sizeof(double)));
    VD_HIP(hipDeviceSynchronize());
    *bytes_filled = ws.part ? (long long)(ws.doubles * sizeof(double)) : 0;
    return 0;
}

int vd_pair_sqdist(int N, long long D, const float* a, const float* b, double* out, void* stream) {
    VD_REQUIRE(N >= 0 && D >= 1, "pair distance: N >= 0 rows of D >= 1 values");
    if (N == 0) return 0;
    VD_REQUIRE(a && b && out, "null argument");
    hipLaunchKernelGGL(pair_sqdist_kernel, dim3(N), dim3(MT_THREADS), 0, static_cast<hipStream_t>(stream), a, b, D, out);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
