// I3D video embedding for the Frechet video distance (Inception-v1 inflated to 3-D, Kinetics-400 RGB: what the TF-Hub module
// deepmind/i3d-kinetics-400/1 computes for the reference's create_id3_embedding(preprocess(videos, (224, 224))),
// improved_diffusion/frechet_video_distance.py:38-133), gfx950.
//
// Per video, uint8 [T][3][H][W]:
//   preprocess   TF1 resize_bilinear to 224 x 224 (align_corners=False, no half-pixel centres), then 2 x / 255 - 1, channels-last
//   Unit3D       conv3d (no bias) -> BatchNorm (inference) -> ReLU; the BatchNorm is folded into weight and bias by the caller
//   SAME padding per axis: total = max(k - s, 0) if size % s == 0 else max(k - size % s, 0), before = total / 2, the rest behind;
//                output size ceil(size / s).  Max pools ignore the padding (-inf), as TF does.
//   Conv3d_1a_7x7 /2, MaxPool 1,3,3 /1,2,2, Conv3d_2b_1x1, Conv3d_2c_3x3, MaxPool 1,3,3 /1,2,2, Mixed_3b, 3c, MaxPool 3,3,3 /2,
//   Mixed_4b..4f, MaxPool 2,2,2 /2, Mixed_5b, 5c, average pool 2,7,7 VALID, logits (1x1x1 with bias), mean over time -> 400 numbers.
//
// Convolutions and max pools: the channels-last kernels of conv_cl.hip, activations [T][H][W][C].  The output is written with
// a row stride, so the four branches of a Mixed block land in their channel slices of one tensor.  Cin % 4 == 0: the operand is
// gathered four channels at a time; otherwise (Conv3d_1a_7x7, Cin = 3) element by element.  Every sum has a fixed order, and
// videos are processed one after another with the same launches, so a video's feature does not depend on its batch.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/vd_amd.h"
#include "vd_common.h"

namespace vd {
namespace {

constexpr int kI3dMinFrames = 9;        // the time mean runs over ceil(ceil(ceil(T/2)/2)/2) - 1 positions
constexpr int kI3dMaxFrames = 1024;
constexpr int kI3dSide = 224;
constexpr int kI3dClasses = 400;
constexpr int kI3dFeat = 1024;

struct Same { int out, before; };
inline Same same_pad(int size, int k, int s) {
    const int total = size % s == 0 ? std::max(k - s, 0) : std::max(k - size % s, 0);
    return {(size + s - 1) / s, total / 2};
}

// TF1 resize_bilinear (align_corners=False, no half-pixel centres) of uint8 [T][3][H][W] to [T][S][S][3], then 2 x / 255 - 1.
// scale = in / float(out), src = dst * scale, lo = floor(src), hi = min(lo + 1, in - 1), lerp = src - lo, all float32; every
// product and sum rounded on its own (no contraction), as the expressions are written.
__global__ __launch_bounds__(256) void i3d_resize_kernel(const uint8_t* src, float* dst, int T, int H, int W, int S) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)T * S * S) return;
    const int ox = (int)(i % S), oy = (int)((i / S) % S);
    const long long t = i / ((long long)S * S);
    const float ys = __fmul_rn((float)oy, __fdiv_rn((float)H, (float)S));
    const float xs = __fmul_rn((float)ox, __fdiv_rn((float)W, (float)S));
    const int y0 = min((int)floorf(ys), H - 1), x0 = min((int)floorf(xs), W - 1);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float yl = __fsub_rn(ys, (float)y0), xl = __fsub_rn(xs, (float)x0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* pl = src + ((size_t)t * 3 + c) * H * W;
        const float tl = pl[(size_t)y0 * W + x0], tr = pl[(size_t)y0 * W + x1];
        const float bl = pl[(size_t)y1 * W + x0], br = pl[(size_t)y1 * W + x1];
        const float top = __fadd_rn(tl, __fmul_rn(__fsub_rn(tr, tl), xl));
        const float bot = __fadd_rn(bl, __fmul_rn(__fsub_rn(br, bl), xl));
        const float v = __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), yl));
        dst[(size_t)i * 3 + c] = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, v), 255.f), 1.f);
    }
}

// tail, part 1: x [t][7][7][1024] -> feat[c] = mean over the t - 1 positions p of the average of x[p..p+1][:][:][c]
// (average pool 2,7,7 VALID, then the time mean, which commutes with the logits layer); one thread per channel, fixed order
__global__ __launch_bounds__(256) void i3d_tail_pool_kernel(const float* x, int t, int hw, int C, float* feat) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float total = 0.f;
    for (int p = 0; p + 1 < t; ++p) {
        float s = 0.f;
        for (int q = 0; q < 2 * hw; ++q) s += x[((size_t)p * hw + q) * C + c];
        total += s / (float)(2 * hw);
    }
    feat[c] = total / (float)(t - 1);
}

// tail, part 2: out[o] = bias[o] + sum_c w[o][c] * feat[c]; one wave per output, strided partials then a fixed tree
__global__ __launch_bounds__(64) void i3d_logits_kernel(const float* feat, const float* w, const float* bias, int C, int K, float* out) {
    __shared__ float red[64];
    const int o = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int c = tid; c < C; c += 64) s = fmaf(w[(size_t)o * K + c], feat[c], s);
    red[tid] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[o] = red[0] + bias[o];
}

// ---------------------------------------------------------------- the network's table
struct Unit { std::string name; int cin, cout, k; };     // cubic kernels: 1, 3 or 7

const int kMixedIn[9] = {192, 256, 480, 512, 512, 512, 528, 832, 832};
const char* const kMixedName[9] = {"Mixed_3b", "Mixed_3c", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "Mixed_5b", "Mixed_5c"};
const int kMixedW[9][6] = {{64, 96, 128, 16, 32, 32},    {128, 128, 192, 32, 96, 64},  {192, 96, 208, 16, 48, 64},
                           {160, 112, 224, 24, 64, 64},  {128, 128, 256, 24, 64, 64},  {112, 144, 288, 32, 64, 64},
                           {256, 160, 320, 32, 128, 128}, {256, 160, 320, 32, 128, 128}, {384, 192, 384, 48, 128, 128}};

const std::vector<Unit>& units() {
    static const std::vector<Unit> u = [] {
        std::vector<Unit> v = {{"Conv3d_1a_7x7", 3, 64, 7}, {"Conv3d_2b_1x1", 64, 64, 1}, {"Conv3d_2c_3x3", 64, 192, 3}};
        for (int b = 0; b < 9; ++b) {
            const std::string n = kMixedName[b];
            const int* o = kMixedW[b];
            const int cin = kMixedIn[b];
            v.push_back({n + ".b0", cin, o[0], 1});
            v.push_back({n + ".b1a", cin, o[1], 1});
            v.push_back({n + ".b1b", o[1], o[2], 3});
            v.push_back({n + ".b2a", cin, o[3], 1});
            v.push_back({n + ".b2b", o[3], o[4], 3});
            v.push_back({n + ".b3b", cin, o[5], 1});
        }
        return v;
    }();
    return u;
}

int launch_conv(const float* src, const float* w, const float* bias, float* out, long long out_stride, int T, int H, int W, int Cin,
                int Cout, int kt, int kh, int kw, int st, int sh, int sw, int relu, hipStream_t stream) {
    const Same zt = same_pad(T, kt, st), zy = same_pad(H, kh, sh), zx = same_pad(W, kw, sw);
    ConvClArgs a{};
    a.src = src; a.w = w; a.bias = bias; a.out = out; a.out_stride = out_stride;
    a.T = T; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.kt = kt; a.kh = kh; a.kw = kw; a.st = st; a.sh = sh; a.sw = sw;
    a.pt = zt.before; a.ph = zy.before; a.pw = zx.before;
    a.To = zt.out; a.Ho = zy.out; a.Wo = zx.out; a.relu = relu;
    return launch_conv_cl(a, Cin % 4 == 0 ? CG_QUAD : CG_ELEM, stream);
}

int launch_pool(const float* src, float* dst, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw,
                hipStream_t stream) {
    const Same zt = same_pad(T, kt, st), zy = same_pad(H, kh, sh), zx = same_pad(W, kw, sw);
    return launch_maxpool_cl(PoolClArgs{src, dst, T, H, W, C, kt, kh, kw, st, sh, sw, zt.before, zy.before, zx.before, zt.out, zy.out, zx.out},
                             stream);
}

int launch_resize(const uint8_t* src, float* dst, int T, int H, int W, hipStream_t stream) {
    const long long n = (long long)T * kI3dSide * kI3dSide;
    hipLaunchKernelGGL(i3d_resize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, dst, T, H, W, kI3dSide);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace
}  // namespace vd

struct vd_i3d {
    int dev = -1;
    std::vector<float*> w, b;          // per unit: packed [Cout][Kpad], [Cout]
    float* lw = nullptr;               // logits [400][1024]
    float* lb = nullptr;
    int missing = 0;                   // tensors still to load
    float* ws = nullptr;
    size_t ws_floats = 0;
};

using namespace vd;

// the six regions of the workspace for a T-frame video, in floats: the preprocessed video, the two alternating main tensors, and
// a Mixed block's b1a / b2a outputs and pooled input
struct I3dPlan { size_t pre, main[2], tmp[3]; int t_last; };

static I3dPlan i3d_plan(int T) {
    I3dPlan p{};
    const size_t S = kI3dSide;
    p.pre = (size_t)T * S * S * 3;
    int t = T, hw = kI3dSide, side = 0;
    auto put = [&](size_t floats) { p.main[side] = std::max(p.main[side], floats); side ^= 1; };
    auto vol = [&](int c) { return (size_t)t * hw * hw * c; };
    t = same_pad(t, 7, 2).out; hw = same_pad(hw, 7, 2).out; put(vol(64));
    hw = same_pad(hw, 3, 2).out; put(vol(64));
    put(vol(64));
    put(vol(192));
    hw = same_pad(hw, 3, 2).out; put(vol(192));
    for (int b = 0; b < 9; ++b) {
        if (b == 2) { t = same_pad(t, 3, 2).out; hw = same_pad(hw, 3, 2).out; put(vol(480)); }
        if (b == 7) { t = same_pad(t, 2, 2).out; hw = same_pad(hw, 2, 2).out; put(vol(832)); }
        const int* o = kMixedW[b];
        p.tmp[0] = std::max(p.tmp[0], vol(o[1]));
        p.tmp[1] = std::max(p.tmp[1], vol(o[3]));
        p.tmp[2] = std::max(p.tmp[2], vol(kMixedIn[b]));
        put(vol(o[0] + o[2] + o[4] + o[5]));
    }
    p.t_last = t;
    return p;
}

static int i3d_embed_one(vd_i3d* h, int T, int H, int W, const uint8_t* video, float* out, hipStream_t st) {
    const I3dPlan p = i3d_plan(T);
    float* pre = h->ws;
    float* mainb[2] = {pre + p.pre, pre + p.pre + p.main[0]};
    float* tmp[3] = {mainb[1] + p.main[1], mainb[1] + p.main[1] + p.tmp[0], mainb[1] + p.main[1] + p.tmp[0] + p.tmp[1]};
    float* feat = tmp[2] + p.tmp[2];
    int rc, side = 0, t = T, hw = kI3dSide, u = 0;
    const float* x = pre;
    auto next = [&]() { float* y = mainb[side]; side ^= 1; return y; };
    auto unit = [&](const float* src, int Tt, int Hh, int s, float* dst, long long stride) -> int {
        const Unit& un = units()[u];
        const int r = launch_conv(src, h->w[u], h->b[u], dst, stride, Tt, Hh, Hh, un.cin, un.cout, un.k, un.k, un.k, s, s, s, 1, st);
        ++u;
        return r;
    };
    auto pool = [&](int kt, int ks, int sT, int sS, int C) -> int {
        float* y = next();
        const int r = launch_pool(x, y, t, hw, hw, C, kt, ks, ks, sT, sS, sS, st);
        t = same_pad(t, kt, sT).out; hw = same_pad(hw, ks, sS).out;
        x = y;
        return r;
    };
    if ((rc = launch_resize(video, pre, T, H, W, st))) return rc;
    {
        float* y = next();
        if ((rc = unit(x, t, hw, 2, y, 64))) return rc;
        t = same_pad(t, 7, 2).out; hw = same_pad(hw, 7, 2).out; x = y;
    }
    if ((rc = pool(1, 3, 1, 2, 64))) return rc;
    { float* y = next(); if ((rc = unit(x, t, hw, 1, y, 64))) return rc; x = y; }
    { float* y = next(); if ((rc = unit(x, t, hw, 1, y, 192))) return rc; x = y; }
    if ((rc = pool(1, 3, 1, 2, 192))) return rc;
    for (int b = 0; b < 9; ++b) {
        if (b == 2 && (rc = pool(3, 3, 2, 2, 480))) return rc;
        if (b == 7 && (rc = pool(2, 2, 2, 2, 832))) return rc;
        const int* o = kMixedW[b];
        const int ctot = o[0] + o[2] + o[4] + o[5];
        float* y = next();
        if ((rc = unit(x, t, hw, 1, y, ctot)) ||                                       // b0
            (rc = unit(x, t, hw, 1, tmp[0], o[1])) ||                                  // b1a
            (rc = unit(tmp[0], t, hw, 1, y + o[0], ctot)) ||                           // b1b
            (rc = unit(x, t, hw, 1, tmp[1], o[3])) ||                                  // b2a
            (rc = unit(tmp[1], t, hw, 1, y + o[0] + o[2], ctot)) ||                    // b2b
            (rc = launch_pool(x, tmp[2], t, hw, hw, kMixedIn[b], 3, 3, 3, 1, 1, 1, st)) ||
            (rc = unit(tmp[2], t, hw, 1, y + o[0] + o[2] + o[4], ctot)))               // b3b
            return rc;
        x = y;
    }
    hipLaunchKernelGGL(i3d_tail_pool_kernel, dim3(kI3dFeat / 256), dim3(256), 0, st, x, t, hw * hw, kI3dFeat, feat);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(i3d_logits_kernel, dim3(kI3dClasses), dim3(64), 0, st, feat, h->lw, h->lb, kI3dFeat, kI3dFeat, out);
    VD_HIP(hipGetLastError());
    return 0;
}

static int i3d_frames_ok(int T) {
    VD_REQUIRE(T >= kI3dMinFrames, "I3D needs videos of at least 9 frames (the time mean runs over ceil(T/8) - 1 positions)");
    VD_REQUIRE(T <= kI3dMaxFrames, "I3D: more frames than vd_i3d_max_frames() = 1024");
    return 0;
}

extern "C" {

int vd_i3d_max_frames(void) { return kI3dMaxFrames; }

int vd_i3d_create(vd_i3d** out) {
    VD_REQUIRE(out, "null argument");
    vd_i3d* h = new vd_i3d();
    if (hipGetDevice(&h->dev) != hipSuccess) { delete h; set_error("hipGetDevice"); return -2; }
    h->w.assign(units().size(), nullptr);
    h->b.assign(units().size(), nullptr);
    h->missing = 2 * (int)units().size() + 2;
    *out = h;
    return 0;
}

void vd_i3d_destroy(vd_i3d* h) {
    if (!h) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->dev);
    for (float* p : h->w) (void)hipFree(p);
    for (float* p : h->b) (void)hipFree(p);
    (void)hipFree(h->lw); (void)hipFree(h->lb); (void)hipFree(h->ws);
    (void)hipSetDevice(cur);
    delete h;
}

// a tensor counts as loaded once its device copy exists: `fresh` = there was none before this load
static int note_loaded(vd_i3d* h, bool fresh, const float* dev, int rc) {
    if (fresh && dev) --h->missing;
    return rc;
}
static int i3d_upload(vd_i3d* h, float** dst, const float* host, size_t n) {
    const bool fresh = !*dst;
    const int rc = upload_f32(dst, host, n);
    return note_loaded(h, fresh, *dst, rc);
}

int vd_i3d_load_weight(vd_i3d* h, const char* name, const float* host, long long bytes) {
    VD_REQUIRE(h && name && host, "null argument");
    if (int rc = require_device(h->dev, "I3D")) return rc;
    VD_REQUIRE(bytes % (long long)sizeof(float) == 0, "byte count not a multiple of 4");
    const std::string s(name);
    const long long nf = bytes / (long long)sizeof(float);
    if (s == "logits.weight") {
        VD_REQUIRE(nf == (long long)kI3dClasses * kI3dFeat, "logits weight: size mismatch ([400][1024] expected)");
        return i3d_upload(h, &h->lw, host, nf);
    }
    if (s == "logits.bias") {
        VD_REQUIRE(nf == kI3dClasses, "logits bias: size mismatch");
        return i3d_upload(h, &h->lb, host, nf);
    }
    for (size_t u = 0; u < units().size(); ++u) {
        const Unit& un = units()[u];
        if (s == un.name + ".bias") {
            VD_REQUIRE(nf == un.cout, "unit bias: size mismatch");
            return i3d_upload(h, &h->b[u], host, nf);
        }
        if (s == un.name + ".weight") {
            const int taps = un.k * un.k * un.k;
            VD_REQUIRE(nf == (long long)un.cout * un.cin * taps, "unit weight: size mismatch ([Cout][Cin][kt][kh][kw] expected)");
            const bool fresh = !h->w[u];
            const int rc = conv_cl_load_weight(&h->w[u], host, un.cout, un.cin, taps);
            return note_loaded(h, fresh, h->w[u], rc);
        }
    }
    set_error("unexpected I3D weight name: " + s);
    return -1;
}

int vd_i3d_embed(vd_i3d* h, int N, int T, int H, int W, const uint8_t* videos, float* out, void* stream) {
    VD_REQUIRE(h && videos && out, "null argument");
    VD_REQUIRE(N >= 0, "negative video count");
    if (int rc = i3d_frames_ok(T)) return rc;
    VD_REQUIRE(H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "frame size: 1 .. 8192 per side");
    VD_REQUIRE(h->missing == 0, "I3D weights incomplete: every unit's weight and bias and logits.weight / logits.bias are required");
    if (int rc = require_device(h->dev, "I3D")) return rc;
    if (N == 0) return 0;
    const I3dPlan p = i3d_plan(T);
    const size_t need = p.pre + p.main[0] + p.main[1] + p.tmp[0] + p.tmp[1] + p.tmp[2] + kI3dFeat;
    if (int rc = grow_ws(&h->ws, &h->ws_floats, need)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    for (int n = 0; n < N; ++n)
        if (int rc = i3d_embed_one(h, T, H, W, videos + (size_t)n * T * 3 * H * W, out + (size_t)n * kI3dClasses, st)) return rc;
    return 0;
}

// Test hook, as vd_scratch_fill: the handle's workspace -- the six regions of i3d_plan and the pooled features, each written by the
// embed that reads it -- set to `byte`.  The weights and the buffer's address stay.
int vd_i3d_scratch_fill(vd_i3d* h, int byte, long long* bytes_filled) {
    VD_REQUIRE(h && bytes_filled && byte >= 0 && byte <= 255, "scratch_fill: a handle, a byte 0..255 and where to report the bytes");
    *bytes_filled = 0;
    if (int rc = require_device(h->dev, "I3D")) return rc;
    VD_HIP(hipDeviceSynchronize());
    if (h->ws && h->ws_floats) VD_HIP(hipMemset(h->ws, byte, h->ws_floats * sizeof(float)));
    VD_HIP(hipDeviceSynchronize());
    *bytes_filled = h->ws ? (long long)(h->ws_floats * sizeof(float)) : 0;
    return 0;
}

int vd_op_conv3d_same(const float* x, const float* w, const float* bias, int T, int H, int W, int Cin, int Cout, int kt, int kh,
                      int kw, int st, int sh, int sw, int relu, float* out, long long out_stride, void* stream) {
    VD_REQUIRE(x && w && out, "null argument");
    VD_REQUIRE(T > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "empty problem");
    VD_REQUIRE(kt > 0 && kh > 0 && kw > 0 && st > 0 && sh > 0 && sw > 0, "kernel and stride: positive");
    VD_REQUIRE(out_stride >= Cout, "out_stride < Cout");
    VD_REQUIRE((long long)Cin * kt * kh * kw < (1 << 24), "reduction length beyond 2^24");
    VD_REQUIRE(Cin % 4 != 0 || (reinterpret_cast<uintptr_t>(x) & 15) == 0, "x: 16-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int taps = kt * kh * kw;
    float* packed = nullptr;
    VD_HIP(hipMalloc(reinterpret_cast<void**>(&packed), (size_t)Cout * conv_cl_kpad(Cin * taps) * sizeof(float)));
    int rc = launch_conv_cl_pack(w, packed, Cout, Cin, taps, s);
    if (!rc) rc = launch_conv(x, packed, bias, out, out_stride, T, H, W, Cin, Cout, kt, kh, kw, st, sh, sw, relu, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) { set_error("vd_op_conv3d_same: the kernels failed"); rc = -2; }
    (void)hipFree(packed);
    return rc;
}

int vd_op_maxpool3d_same(const float* x, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw, float* out,
                         void* stream) {
    VD_REQUIRE(x && out, "null argument");
    VD_REQUIRE(T > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "empty problem, or channels not a multiple of 4");
    VD_REQUIRE(kt > 0 && kh > 0 && kw > 0 && st > 0 && sh > 0 && sw > 0, "kernel and stride: positive");
    VD_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0, "x, out: 16-byte aligned");
    return launch_pool(x, out, T, H, W, C, kt, kh, kw, st, sh, sw, static_cast<hipStream_t>(stream));
}

int vd_op_resize_bilinear_tf1(const uint8_t* frames, int T, int H, int W, float* out, void* stream) {
    VD_REQUIRE(frames && out, "null argument");
    VD_REQUIRE(T > 0 && H > 0 && W > 0, "empty problem");
    return launch_resize(frames, out, T, H, W, static_cast<hipStream_t>(stream));
}

}  // extern "C"
