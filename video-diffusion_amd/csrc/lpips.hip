// LPIPS frame embedding (AlexNet features of the `lpips` package, net='alex', spatial=False) and the farthest-point frame
// selection of the adaptive-* frame schedulers, gfx950.
//
// Embedding (reference improved_diffusion/inference_util.py:15-31, LpipsEmbedder.forward), per frame x in [-1, 1]:
//   x' = (x - shift[c]) / scale[c]                                                  (lpips ScalingLayer; conv1's zero padding AFTER it)
//   a1 = relu(conv1 11x11/4 p2)  a2 = relu(conv2 5x5 p2 (maxpool3/2 a1))  a3 = relu(conv3 3x3 p1 (maxpool3/2 a2))
//   a4 = relu(conv4 3x3 p1 a3)    a5 = relu(conv5 3x3 p1 a4)                      (torchvision alexnet.features)
//   e_k[c][y][x] = sqrt(lin_k[c]) * a_k / (||a_k[:, y, x]||_2 + 1e-10) / sqrt(h_k w_k)   (normalize_tensor, scale_by_proj_weights,
//   embedding = concat_k flatten(e_k)                                                       not_spatial_average)
// Convolutions and max pools: the channels-last kernels of conv_cl.hip with kt = 1 and the frames on the T axis, bias + ReLU in
// the epilogue, activations NHWC.  conv1 (Cin = 3, K = 363 -> Kpad 384) gathers its operand element by element from the NCHW
// frames and applies the scaling layer to in-image taps only.  Every sum has a fixed order: results are run-to-run deterministic.
//
// Selection (reference inference_util.py:157-185): per batch item, picked[0] = always[0], nearest[f] = +inf; pick i = 1..n-1:
// nearest[f] = min(nearest[f], ||e[newest] - e[f]||^2) over all candidates f, then always[i] if i < n_always else the argmax of
// nearest (lowest index on ties, as np.argmax).  Two launches per pick, `newest` read from the picks in device memory: the
// whole selection is enqueued without a host synchronisation.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/vd_amd.h"
#include "vd_common.h"

namespace vd {
namespace {

// torchvision alexnet.features conv layers
constexpr int kCin[5] = {3, 64, 192, 384, 256};
constexpr int kCout[5] = {64, 192, 384, 256, 256};
constexpr int kKsz[5] = {11, 5, 3, 3, 3};
constexpr int kStride[5] = {4, 1, 1, 1, 1};
constexpr int kPad[5] = {2, 2, 1, 1, 1};

// One tap: a [nfr][hw][C] (NHWC) -> out[n][off + c*hw + p] = sqrt(lin[c]) * a[n][p][c] / (||a[n][p][:]|| + 1e-10) / sqrt(hw).
// Block = 64 pixels of one frame x 4 channel groups; the transposed write goes through a [64][33] LDS tile per 32 channels, so
// both the reads and the writes are row-contiguous.
__global__ __launch_bounds__(256) void lpips_tap_kernel(const float* act, const float* lin, int hw, int C, float* out, long long D,
                                                        long long off) {
    __shared__ float part[4][64];
    __shared__ float tile[64][33];
    const int tid = threadIdx.x, pl = tid & 63, g = tid >> 6;
    const int n = blockIdx.y, p0 = blockIdx.x * 64;
    const float* an = act + (size_t)n * hw * C;
    {
        const int p = min(p0 + pl, hw - 1), cq = C / 4;
        const float* row = an + (size_t)p * C + g * cq;
        float s = 0.f;
        for (int c = 0; c < cq; c += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
            s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
        }
        part[g][pl] = s;
    }
    __syncthreads();
    const float den = sqrtf(((part[0][pl] + part[1][pl]) + part[2][pl]) + part[3][pl]) + 1e-10f;
    const float rs = sqrtf((float)hw);
    float* on = out + (size_t)n * D + off;
    for (int c0 = 0; c0 < C; c0 += 32) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int idx = tid + 256 * t, pr = idx >> 3, q = idx & 7;
            const int p = min(p0 + pr, hw - 1);
            const f32x4 v = *reinterpret_cast<const f32x4*>(an + (size_t)p * C + c0 + q * 4);
            tile[pr][q * 4 + 0] = v.x; tile[pr][q * 4 + 1] = v.y; tile[pr][q * 4 + 2] = v.z; tile[pr][q * 4 + 3] = v.w;
        }
        __syncthreads();
        if (p0 + pl < hw) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int cc = g * 8 + j, c = c0 + cc;
                on[(size_t)c * hw + p0 + pl] = sqrtf(lin[c]) * (tile[pl][cc] / den) / rs;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- farthest-point selection
__global__ void fps_init_kernel(int* out, float* nearest, int B, int n, int ncand, int first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * ncand) nearest[i] = __builtin_inff();
    if (i < B) out[(size_t)i * n] = first;
    if (i == 0) out[(size_t)B * n] = 0;                    // error word
}

// block (f, b): d = sum_k (e[b][newest_b][k] - e[b][f][k])^2 in a fixed order (per-thread strided float4 partials, then a fixed
// tree), nearest[b][f] = min(nearest[b][f], d); a non-finite d sets bit 0 of the error word out[B*n]
__global__ __launch_bounds__(256) void fps_dist_kernel(const float* embs, int B, int ncand, long long D, int n, int i, int* out,
                                                       float* nearest) {
    __shared__ float red[256];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int newest = out[(size_t)b * n + i - 1];
    const f32x4* x = reinterpret_cast<const f32x4*>(embs + ((size_t)b * ncand + newest) * D);
    const f32x4* y = reinterpret_cast<const f32x4*>(embs + ((size_t)b * ncand + f) * D);
    const long long D4 = D / 4;
    float s = 0.f;
    for (long long k = tid; k < D4; k += 256) {
        const f32x4 u = x[k] - y[k];
        s = fmaf(u.x, u.x, s); s = fmaf(u.y, u.y, s); s = fmaf(u.z, u.z, s); s = fmaf(u.w, u.w, s);
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const float d = red[0];
        float& nr = nearest[(size_t)b * ncand + f];
        if (!isfinite(d)) atomicOr(out + (size_t)B * n, 1);
        nr = d < nr ? d : nr;
    }
}

// block b: pick i = forced (>= 0) or the argmax of nearest[b][:] (lowest index among equal maxima)
__global__ __launch_bounds__(256) void fps_pick_kernel(const float* nearest, int ncand, int n, int i, int forced, int* out) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (forced >= 0) {
        if (tid == 0) out[(size_t)b * n + i] = forced;
        return;
    }
    const float* nb = nearest + (size_t)b * ncand;
    float v = -__builtin_inff();
    int ix = ncand;
    for (int f = tid; f < ncand; f += 256) {
        const float u = nb[f];
        if (u > v || ix == ncand) { v = u; ix = f; }
    }
    bv[tid] = v; bi[tid] = ix;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const float u = bv[tid + w];
            const int j = bi[tid + w];
            if (j < ncand && (bi[tid] == ncand || u > bv[tid] || (u == bv[tid] && j < bi[tid]))) { bv[tid] = u; bi[tid] = j; }
        }
        __syncthreads();
    }
    if (tid == 0) out[(size_t)b * n + i] = bi[0];
}

bool lp_dims(int H, int W, int hs[5], int ws[5]) {
    if (H + 4 < 11 || W + 4 < 11) return false;
    int h = (H + 4 - 11) / 4 + 1, w = (W + 4 - 11) / 4 + 1;
    hs[0] = h; ws[0] = w;
    if (h < 3 || w < 3) return false;
    h = (h - 3) / 2 + 1; w = (w - 3) / 2 + 1;
    hs[1] = h; ws[1] = w;
    if (h < 3 || w < 3) return false;
    h = (h - 3) / 2 + 1; w = (w - 3) / 2 + 1;
    for (int l = 2; l < 5; ++l) { hs[l] = h; ws[l] = w; }
    return true;
}

long long lp_dim(int hs[5], int ws[5]) {
    long long d = 0;
    for (int l = 0; l < 5; ++l) d += (long long)kCout[l] * hs[l] * ws[l];
    return d;
}

// workspace floats per frame, a1 | p1 | a2 | p2 | a3 | a4 | a5 (NHWC)
void lp_ws_sizes(const int hs[5], const int ws[5], size_t sz[7]) {
    const size_t HW1 = (size_t)hs[0] * ws[0], HW2 = (size_t)hs[1] * ws[1], HW3 = (size_t)hs[2] * ws[2];
    const size_t v[7] = {HW1 * 64, HW2 * 64, HW2 * 192, HW3 * 192, HW3 * 384, HW3 * 256, HW3 * 256};
    for (int k = 0; k < 7; ++k) sz[k] = v[k];
}

// frames per pass: the workspace is bounded by 2^26 floats (256 MiB), the tap kernel's grid.y by 65535; at least one frame
int lp_chunk(const size_t sz[7]) {
    size_t per = 0;
    for (int k = 0; k < 7; ++k) per += sz[k];
    const size_t cap = (size_t)1 << 26;
    return (int)std::max<size_t>(1, std::min<size_t>(65535, cap / per));
}

}  // namespace
}  // namespace vd

struct vd_lpips {
    int dev = -1;
    float* w[5] = {};         // packed [Cout][Kpad]
    float* b[5] = {};
    float* lin[5] = {};
    float shift[3] = {-0.030f, -0.088f, -0.188f};    // lpips ScalingLayer defaults
    float scale[3] = {0.458f, 0.448f, 0.450f};
    unsigned loaded = 0;      // bit l: conv l+1 weight, 5+l: bias, 10+l: lin
    float* ws = nullptr;
    size_t ws_floats = 0;
};

using namespace vd;

extern "C" {

int vd_lpips_create(vd_lpips** out) {
    VD_REQUIRE(out, "null argument");
    vd_lpips* h = new vd_lpips();
    if (hipGetDevice(&h->dev) != hipSuccess) { delete h; set_error("hipGetDevice"); return -2; }
    *out = h;
    return 0;
}

void vd_lpips_destroy(vd_lpips* h) {
    if (!h) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->dev);
    for (int l = 0; l < 5; ++l) { (void)hipFree(h->w[l]); (void)hipFree(h->b[l]); (void)hipFree(h->lin[l]); }
    (void)hipFree(h->ws);
    (void)hipSetDevice(cur);
    delete h;
}

int vd_lpips_load_weight(vd_lpips* h, const char* name, const float* host, long long bytes) {
    VD_REQUIRE(h && name && host, "null argument");
    if (int rc = require_device(h->dev, "LPIPS")) return rc;
    const std::string s(name);
    const long long nf = bytes / (long long)sizeof(float);
    VD_REQUIRE(bytes % (long long)sizeof(float) == 0, "byte count not a multiple of 4");
    if (s == "shift" || s == "scale") {
        VD_REQUIRE(nf == 3, "scaling layer: 3 values");
        float* d = s == "shift" ? h->shift : h->scale;
        for (int c = 0; c < 3; ++c) d[c] = host[c];
        if (s == "scale") for (int c = 0; c < 3; ++c) VD_REQUIRE(h->scale[c] != 0.f, "scaling layer: zero scale");
        return 0;
    }
    for (int l = 0; l < 5; ++l) {
        const std::string L = std::to_string(l + 1);
        if (s == "conv" + L + ".weight") {
            VD_REQUIRE(nf == (long long)kCout[l] * kCin[l] * kKsz[l] * kKsz[l], "conv weight: size mismatch (OIHW expected)");
            if (int rc = conv_cl_load_weight(&h->w[l], host, kCout[l], kCin[l], kKsz[l] * kKsz[l])) return rc;
            h->loaded |= 1u << l;
            return 0;
        }
        if (s == "conv" + L + ".bias") {
            VD_REQUIRE(nf == kCout[l], "conv bias: size mismatch");
            if (int rc = upload_f32(&h->b[l], host, nf)) return rc;
            h->loaded |= 1u << (5 + l);
            return 0;
        }
        if (s == "lin" + L) {
            VD_REQUIRE(nf == kCout[l], "lin weight: size mismatch");
            for (long long c = 0; c < nf; ++c) VD_REQUIRE(host[c] >= 0.f, "lin weight: negative entry (sqrt of it is NaN)");
            if (int rc = upload_f32(&h->lin[l], host, nf)) return rc;
            h->loaded |= 1u << (10 + l);
            return 0;
        }
    }
    set_error("unexpected LPIPS weight name: " + s);
    return -1;
}

// Test hook, as vd_scratch_fill: the handle's workspace -- activations each embed writes before it reads them -- set to `byte`.  The
// weights and the buffer's address stay.
int vd_lpips_scratch_fill(vd_lpips* h, int byte, long long* bytes_filled) {
    VD_REQUIRE(h && bytes_filled && byte >= 0 && byte <= 255, "scratch_fill: a handle, a byte 0..255 and where to report the bytes");
    *bytes_filled = 0;
    if (int rc = require_device(h->dev, "LPIPS")) return rc;
    VD_HIP(hipDeviceSynchronize());
    if (h->ws && h->ws_floats) VD_HIP(hipMemset(h->ws, byte, h->ws_floats * sizeof(float)));
    VD_HIP(hipDeviceSynchronize());
    *bytes_filled = h->ws ? (long long)(h->ws_floats * sizeof(float)) : 0;
    return 0;
}

long long vd_lpips_dim(int H, int W) {
    int hs[5], ws[5];
    if (!lp_dims(H, W, hs, ws)) return -1;
    return lp_dim(hs, ws);
}

int vd_lpips_embed_chunk(int H, int W) {
    int hs[5], ws[5];
    if (!lp_dims(H, W, hs, ws)) return -1;
    size_t sz[7];
    lp_ws_sizes(hs, ws, sz);
    return lp_chunk(sz);
}

int vd_lpips_embed(vd_lpips* h, int N, int H, int W, const float* frames, float* out, void* stream) {
    VD_REQUIRE(h && frames && out, "null argument");
    VD_REQUIRE(h->loaded == (1u << 15) - 1, "LPIPS weights incomplete: conv1..5 weight/bias and lin1..5 are required");
    VD_REQUIRE(N >= 0, "negative frame count");
    if (int rc = require_device(h->dev, "LPIPS")) return rc;
    int hs[5], wds[5];
    VD_REQUIRE(lp_dims(H, W, hs, wds), "frames too small for the AlexNet feature stack");
    if (N == 0) return 0;
    const long long D = lp_dim(hs, wds);
    const int hp1 = hs[1], wp1 = wds[1];                  // pool1 output = conv2 input/output size
    size_t sz[7], per = 0;
    lp_ws_sizes(hs, wds, sz);
    for (size_t v : sz) per += v;
    const int chunk = std::min(N, lp_chunk(sz));          // what vd_lpips_embed_chunk answers, or all N frames
    if (int rc = grow_ws(&h->ws, &h->ws_floats, per * chunk)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    long long offs[5];
    offs[0] = 0;
    for (int l = 1; l < 5; ++l) offs[l] = offs[l - 1] + (long long)kCout[l - 1] * hs[l - 1] * wds[l - 1];

    for (int f0 = 0; f0 < N; f0 += chunk) {
        const int nf = std::min(chunk, N - f0);
        float* buf[7];
        float* p = h->ws;
        for (int k = 0; k < 7; ++k) { buf[k] = p; p += sz[k] * nf; }
        float* o = out + (size_t)f0 * D;

        auto conv = [&](int l, const float* src, int Hi, int Wi, float* dst) -> int {
            ConvClArgs a{};
            a.src = src; a.w = h->w[l]; a.bias = h->b[l]; a.out = dst; a.out_stride = kCout[l];
            a.T = nf; a.H = Hi; a.W = Wi; a.Cin = kCin[l]; a.Cout = kCout[l];
            a.kt = 1; a.kh = a.kw = kKsz[l]; a.st = 1; a.sh = a.sw = kStride[l]; a.pt = 0; a.ph = a.pw = kPad[l];
            a.To = nf; a.Ho = hs[l]; a.Wo = wds[l]; a.relu = 1;
            for (int c = 0; c < 3; ++c) { a.shift[c] = h->shift[c]; a.scale[c] = h->scale[c]; }
            return launch_conv_cl(a, l == 0 ? CG_NCHW_SCALED : CG_QUAD, st);
        };
        auto tap = [&](int l, const float* act) -> int {
            const int hw = hs[l] * wds[l];
            hipLaunchKernelGGL(lpips_tap_kernel, dim3((hw + 63) / 64, nf), dim3(256), 0, st, act, h->lin[l], hw, kCout[l], o, D, offs[l]);
            VD_HIP(hipGetLastError());
            return 0;
        };
        auto pool = [&](const float* src, int Hi, int Wi, int C, float* dst, int Ho, int Wo) -> int {
            return launch_maxpool_cl(PoolClArgs{src, dst, nf, Hi, Wi, C, 1, 3, 3, 1, 2, 2, 0, 0, 0, nf, Ho, Wo}, st);    // 3x3 / 2, VALID
        };
        int rc;
        if ((rc = conv(0, frames + (size_t)f0 * 3 * H * W, H, W, buf[0])) || (rc = tap(0, buf[0])) ||
            (rc = pool(buf[0], hs[0], wds[0], 64, buf[1], hp1, wp1)) ||
            (rc = conv(1, buf[1], hp1, wp1, buf[2])) || (rc = tap(1, buf[2])) ||
            (rc = pool(buf[2], hs[1], wds[1], 192, buf[3], hs[2], wds[2])) ||
            (rc = conv(2, buf[3], hs[2], wds[2], buf[4])) || (rc = tap(2, buf[4])) ||
            (rc = conv(3, buf[4], hs[2], wds[2], buf[5])) || (rc = tap(3, buf[5])) ||
            (rc = conv(4, buf[5], hs[2], wds[2], buf[6])) || (rc = tap(4, buf[6])))
            return rc;
    }
    return 0;
}

int vd_fps_select(int B, int n_cand, long long D, const float* embs, int n, const int* always_host, int n_always, float* work,
                  int* out, void* stream) {
    VD_REQUIRE(embs && always_host && work && out, "null argument");
    VD_REQUIRE(B > 0 && n_cand > 0 && n > 0 && D > 0, "empty problem");
    VD_REQUIRE(D % 4 == 0 && (reinterpret_cast<uintptr_t>(embs) & 15) == 0, "embedding rows: D % 4 == 0, 16-byte aligned");
    VD_REQUIRE(n_always >= 1, "at least one always-selected candidate (the first pick)");
    for (int i = 0; i < n_always; ++i) VD_REQUIRE(always_host[i] >= 0 && always_host[i] < n_cand, "always-selected index out of range");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int tot = std::max(B * n_cand, B + 1);
    hipLaunchKernelGGL(fps_init_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, out, work, B, n, n_cand, always_host[0]);
    VD_HIP(hipGetLastError());
    for (int i = 1; i < n; ++i) {
        hipLaunchKernelGGL(fps_dist_kernel, dim3(n_cand, B), dim3(256), 0, st, embs, B, n_cand, D, n, i, out, work);
        VD_HIP(hipGetLastError());
        hipLaunchKernelGGL(fps_pick_kernel, dim3(B), dim3(256), 0, st, work, n_cand, n, i, i < n_always ? always_host[i] : -1, out);
        VD_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
