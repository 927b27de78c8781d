// Green-hallway pixel count of GQN-Mazes frames, gfx950: what `_count_hallway_pixels` of the reference's
// scripts/video_eval_room_seq_acc.py (:126-137) gets per frame from cv2.cvtColor(image[14:45], COLOR_RGB2HSV), cv2.inRange,
// cv2.erode with a 2 x 2 kernel and a count of the non-zero pixels, and the quantisation (x * 255).astype(np.uint8) in front of it.
//
// OpenCV's 8-bit RGB -> HSV is integer arithmetic on two reciprocal tables (12 fractional bits), restated in rgb_to_hsv below; the
// arithmetic is spelled out in include/vd_amd.h and DESIGN.md.  hsv_tables() rebuilds the tables in LDS per block (512 integer
// divisions) instead of fetching them: a lane's index is its pixel's value, so a table in memory would be a gather.
//
// hallway_counts_kernel: one block per frame.  Rows row0 .. row1 - 1 of a plane are ONE contiguous span of (row1 - row0) * W values,
// so the three planes' spans are walked four pixels per thread (a 4-byte load per plane of uint8 frames, a 16-byte load of
// float32 frames) where all three spans start aligned, with a scalar tail; otherwise pixel by pixel.  Nothing outside the spans is
// read.  The mask goes to LDS as one byte per pixel; the erosion reads the up to four bytes of a pixel's 2 x 2 neighbourhood from
// there, the count is reduced over each wave with shuffles and over the waves through LDS, and thread 0 stores the frame's count.
// Traffic: 3 (row1 - row0) W values read, one int written per frame.
#include <algorithm>
#include <string>

#include "../../include/vd_amd.h"
#include "vd_common.h"

namespace vd {
namespace {

constexpr int HW_THREADS = 256;
constexpr int HW_MAX_STRIP = 48 * 1024;         // pixels of a strip = bytes of its mask in LDS (+ 2 KiB of tables)

// sdiv[i] = round(255 * 4096 / i), hdiv[i] = round(180 * 4096 / (6 i)), both 0 at i = 0; no quotient is a tie, so
// floor((2 a + i) / (2 i)) is the rounding.  Needs blockDim.x >= 1; ends with a barrier.
__device__ __forceinline__ void hsv_tables(int* sdiv, int* hdiv) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        sdiv[i] = i ? (2 * 255 * 4096 + i) / (2 * i) : 0;
        hdiv[i] = i ? (2 * 30 * 4096 + i) / (2 * i) : 0;
    }
    __syncthreads();
}

__device__ __forceinline__ void rgb_to_hsv(int r, int g, int b, const int* sdiv, const int* hdiv, int& h, int& s, int& v) {
    v = max(r, max(g, b));
    const int d = v - min(r, min(g, b));
    s = (d * sdiv[v] + 2048) >> 12;
    const int hn = v == r ? g - b : v == g ? b - r + 2 * d : r - g + 4 * d;
    h = (hn * hdiv[d] + 2048) >> 12;                 // arithmetic shift: a floor
    if (h < 0) h += 180;
}

// 255 where inRange(hsv, (50, 25, 25), (70, 255, 255)), else 0
__device__ __forceinline__ unsigned green_mask(int r, int g, int b, const int* sdiv, const int* hdiv) {
    int h, s, v;
    rgb_to_hsv(r, g, b, sdiv, hdiv, h, s, v);
    return (h >= 50 && h <= 70 && s >= 25 && v >= 25) ? 255u : 0u;
}

// (uint8)(x * 255.0f) with the product clamped to 0..255 (a NaN becomes 0)
__device__ __forceinline__ int quant(float x) { return (int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

__global__ __launch_bounds__(HW_THREADS) void hallway_counts_kernel(const void* frames, int is_u8, int H, int W, int row0, int row1,
                                                                    int* counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mask[];
    __shared__ int sdiv[256], hdiv[256];
    __shared__ int red[HW_THREADS / 64];
    const int tid = threadIdx.x;
    hsv_tables(sdiv, hdiv);
    const size_t plane = (size_t)H * W;
    const size_t base = (size_t)blockIdx.x * 3 * plane + (size_t)row0 * W;     // the R span; G and B follow at + plane, + 2 plane
    const int cnt = (row1 - row0) * W;
    const int cnt4 = cnt & ~3;

    if (is_u8) {
        const unsigned char* p = static_cast<const unsigned char*>(frames) + base;
        const bool vec = ((reinterpret_cast<uintptr_t>(p) | plane) & 3) == 0;  // all three spans start 4-byte aligned
        int i = vec ? cnt4 : 0;
        for (int k = tid * 4; k < i; k += HW_THREADS * 4) {
            const unsigned r = *reinterpret_cast<const unsigned*>(p + k);
            const unsigned g = *reinterpret_cast<const unsigned*>(p + plane + k);
            const unsigned b = *reinterpret_cast<const unsigned*>(p + 2 * plane + k);
            unsigned m = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                m |= (green_mask((r >> (8 * q)) & 255, (g >> (8 * q)) & 255, (b >> (8 * q)) & 255, sdiv, hdiv) & 255u) << (8 * q);
            *reinterpret_cast<unsigned*>(mask + k) = m;
        }
        for (int k = i + tid; k < cnt; k += HW_THREADS)
            mask[k] = (unsigned char)green_mask(p[k], p[plane + k], p[2 * plane + k], sdiv, hdiv);
    } else {
        const float* p = static_cast<const float*>(frames) + base;
        const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (plane & 3) == 0;
        int i = vec ? cnt4 : 0;
        for (int k = tid * 4; k < i; k += HW_THREADS * 4) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(p + k);
            const f32x4 g = *reinterpret_cast<const f32x4*>(p + plane + k);
            const f32x4 b = *reinterpret_cast<const f32x4*>(p + 2 * plane + k);
            const unsigned m = green_mask(quant(r.x), quant(g.x), quant(b.x), sdiv, hdiv) |
                               green_mask(quant(r.y), quant(g.y), quant(b.y), sdiv, hdiv) << 8 |
                               green_mask(quant(r.z), quant(g.z), quant(b.z), sdiv, hdiv) << 16 |
                               green_mask(quant(r.w), quant(g.w), quant(b.w), sdiv, hdiv) << 24;
            *reinterpret_cast<unsigned*>(mask + k) = m;
        }
        for (int k = i + tid; k < cnt; k += HW_THREADS)
            mask[k] = (unsigned char)green_mask(quant(p[k]), quant(p[plane + k]), quant(p[2 * plane + k]), sdiv, hdiv);
    }
    __syncthreads();

    // erosion, anchor (1, 1): (y, x) stays when it and its in-strip neighbours (y, x-1), (y-1, x), (y-1, x-1) are all green
    int n = 0;
    for (int k = tid; k < cnt; k += HW_THREADS) {
        const int y = k / W, x = k - y * W;
        unsigned m = mask[k];
        if (x > 0) m &= mask[k - 1];
        if (y > 0) {
            m &= mask[k - W];
            if (x > 0) m &= mask[k - W - 1];
        }
        n += m != 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < HW_THREADS / 64; ++w) total += red[w];
        counts[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(HW_THREADS) void green_mask_kernel(long long n, const unsigned char* rgb, unsigned char* hsv,
                                                                unsigned char* mask) {
    __shared__ int sdiv[256], hdiv[256];
    hsv_tables(sdiv, hdiv);
    const long long step = (long long)gridDim.x * HW_THREADS;
    for (long long i = (long long)blockIdx.x * HW_THREADS + threadIdx.x; i < n; i += step) {
        const int r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        if (hsv) {
            int h, s, v;
            rgb_to_hsv(r, g, b, sdiv, hdiv, h, s, v);
            hsv[3 * i] = (unsigned char)h; hsv[3 * i + 1] = (unsigned char)s; hsv[3 * i + 2] = (unsigned char)v;
        }
        mask[i] = (unsigned char)green_mask(r, g, b, sdiv, hdiv);
    }
}

}  // namespace
}  // namespace vd

using namespace vd;

extern "C" {

int vd_hallway_max_strip(void) { return HW_MAX_STRIP; }

int vd_hallway_counts(int N, int H, int W, int row0, int row1, const void* frames, int is_u8, int* counts, void* stream) {
    VD_REQUIRE(N >= 0 && H >= 1 && W >= 1, "hallway counts: N >= 0 frames of H >= 1 rows and W >= 1 columns");
    VD_REQUIRE(0 <= row0 && row0 < row1 && row1 <= H, "hallway counts: the strip needs 0 <= row0 < row1 <= H");
    VD_REQUIRE((long long)(row1 - row0) * W <= HW_MAX_STRIP,
               "hallway counts: a strip holds at most " + std::to_string(HW_MAX_STRIP) + " pixels (its mask is kept in LDS), got " +
                   std::to_string((long long)(row1 - row0) * W));
    if (N == 0) return 0;
    VD_REQUIRE(frames && counts, "null argument");
    VD_REQUIRE(is_u8 || (reinterpret_cast<uintptr_t>(frames) & 3) == 0, "hallway counts: float frames must be 4-byte aligned");
    const size_t lds = ((size_t)(row1 - row0) * W + 3) & ~(size_t)3;
    hipLaunchKernelGGL(hallway_counts_kernel, dim3((unsigned)N), dim3(HW_THREADS), lds, static_cast<hipStream_t>(stream), frames,
                       is_u8 ? 1 : 0, H, W, row0, row1, counts);
    VD_HIP(hipGetLastError());
    return 0;
}

int vd_op_green_mask(long long n, const unsigned char* rgb, unsigned char* hsv, unsigned char* mask, void* stream) {
    VD_REQUIRE(n >= 0, "green mask: n >= 0 pixels");
    if (n == 0) return 0;
    VD_REQUIRE(rgb && mask, "null argument");
    const long long blocks = std::min<long long>((n + HW_THREADS - 1) / HW_THREADS, 1 << 16);
    hipLaunchKernelGGL(green_mask_kernel, dim3((unsigned)blocks), dim3(HW_THREADS), 0, static_cast<hipStream_t>(stream), n, rgb, hsv,
                       mask);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
