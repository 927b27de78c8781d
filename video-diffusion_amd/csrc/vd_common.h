// Common definitions for the gfx950 kernels and the step engine.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace vd {

// Longest window the forward serves (frames per item): the temporal attention and GroupNorm kernels are built for 1..32 frames
// (attn_temporal.hip, norm.hip) and for 33..128 (attn_temporal_long.hip, norm.hip's long form).  The guided step's backward
// kernels (use_gradient_method, backward.hip) stay at kMaxGuidedWindowFrames.
constexpr int kMaxWindowFrames = 128;
// Widest tensor the GroupNorm32 launchers serve, the two halves of a decoder concat counted together: a thread per channel quad and
// whole pixels in a block of 256 threads (norm.hip, backward.hip).  The launchers spell the number out in their requirements
// (`C <= 1024`, so that their messages do) beside a static_assert against this constant; vd_create refuses a model that would need
// more, by layer (engine.hip).
constexpr int kGnThreadsPerBlock = 256;
constexpr int kGnMaxChannels = 4 * kGnThreadsPerBlock;
#define VD_GN_LIMIT_IS_1024 static_assert(vd::kGnMaxChannels == 1024, "the GroupNorm launchers' `C <= 1024` is kGnMaxChannels")
constexpr int kMaxGuidedWindowFrames = 32;

// Error plumbing: every C-ABI entry returns 0 or a negative code; text via vd_last_error().
void set_error(const std::string& msg);
extern thread_local std::string g_last_error;

#define VD_HIP(call)                                                                   \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            vd::set_error(std::string(#call) + ": " + hipGetErrorString(e_));          \
            return -2;                                                                 \
        }                                                                              \
    } while (0)

#define VD_REQUIRE(cond, msg)                                                          \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            vd::set_error(std::string("requirement failed: ") + #cond + " -- " + msg); \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a DEVICE's copy of a function: raise it once per (launch site, device) -- a process
// that drives several devices must not find the flag of device 0 set when it launches on device 1.  `st` is the site's static.
struct LdsAttr { size_t have[64] = {}; };
inline int raise_dynamic_lds(LdsAttr& st, const void* fn, size_t bytes) {
    int dev = 0;
    VD_HIP(hipGetDevice(&dev));
    VD_REQUIRE(dev >= 0 && dev < 64, "device ordinal beyond the per-device attribute table");
    if (bytes > st.have[dev]) {
        VD_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        st.have[dev] = bytes;
    }
    return 0;
}
#define VD_RAISE_LDS(fn, bytes)                                                                        \
    do {                                                                                               \
        static vd::LdsAttr lds_attr_;                                                                  \
        if (int rc_ = vd::raise_dynamic_lds(lds_attr_, reinterpret_cast<const void*>(fn), (bytes))) return rc_; \
    } while (0)

// ---- small host pieces the feature networks and the metrics share (lpips.hip, i3d.hip, metrics.hip)
// *dst <- host[0..n), allocated on first use
inline int upload_f32(float** dst, const float* host, size_t n) {
    if (!*dst) VD_HIP(hipMalloc(reinterpret_cast<void**>(dst), n * sizeof(float)));
    VD_HIP(hipMemcpy(*dst, host, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
// grow a workspace to `need` elements (hipFree waits for the device, so a launch that still reads the old one has finished)
template <class T>
inline int grow_ws(T** ws, size_t* have, size_t need) {
    if (*have >= need) return 0;
    VD_HIP(hipFree(*ws));
    *ws = nullptr; *have = 0;
    VD_HIP(hipMalloc(reinterpret_cast<void**>(ws), need * sizeof(T)));
    *have = need;
    return 0;
}
// a handle is used on the device it was created on
inline int require_device(int dev, const char* what) {
    int cur = -1;
    VD_HIP(hipGetDevice(&cur));
    VD_REQUIRE(cur == dev, std::string("the ") + what + " handle belongs to another device");
    return 0;
}

// ---------------------------------------------------------------- kernel argument blocks
// Implicit-GEMM convolution / linear layer on NHWC activations (see igemm.hip).
struct IgemmArgs {
    const float* src0;   // [nfr][Hs][Ws][C0]
    const float* src1;   // [nfr][Hs][Ws][Cin-C0] or null  (virtual channel concat, unet.py:826-828)
    int C0, Cin;
    int nfr, Hs, Ws;     // stored source dims
    int ups;             // 1: source is read through a nearest x2 upsample (unet.py:69)
    int nfr_sel = 0;     // frames of the WHOLE layer call when this launch is a part of one (a frame range of a big window, the compact batch
                         // of a window suffix): kernel variants that are chosen by grid size (split-K, conv_wino_z128.hip) are chosen for it,
                         // so a frame's arithmetic does not depend on which other frames share its launch.  0: nfr
    int ups_phase = 0;   // with ups = 1: wwino holds the sub-pixel image (pack_conv3_wino_ups); conv_wino_r64.hip
    // gemm_split.hip, 1x1 over a (virtually concatenated) input, 128x128 tile: the column blocks 0 also write
    // side[m][k] = SiLU(A[m][k] * sideA[frame][k] + sideB[frame][k]) -- the GroupNorm(+FiLM)+SiLU image the ResBlock's first
    // conv reads (norm.hip: affine_act_kernel) -- from the A tile they stage anyway; side_hw = rows per frame (% 128 == 0)
    float* side = nullptr; const float* sideA = nullptr; const float* sideB = nullptr; int side_hw = 0;
    int stride, pad, ksz;
    int Ho, Wo;
    const float* w;      // [ksz*ksz][Cout][Cin]           (generic kernel)
    const float* wfrag;  // [tap][Cin/32][Cout/32][4][64][4] fragment-major (3x3 halo kernel / linear), or null
    const float* wwino;  // Winograd-transformed 3x3 weights [Cin/16][16][Cout/32][2][64][4] (conv_wino.hip), or null
    const float* bias;   // [Cout] or null
    const float* affA;   // [nfr][Cin] per-frame per-channel scale  (GroupNorm/FiLM folded), or null
    const float* affB;   // [nfr][Cin] shift
    int act;             // 1: SiLU on the (affine-transformed) input
    const float* res;    // [M][res_ld] residual added in the epilogue, or null
    int res_ld;
    const float* fbias;  // [nfr][fbias_ld] per-frame bias (ResBlock without scale-shift: h + emb_out, unet.py:196), or null
    int fbias_ld;
    float* out;          // [M][ldo]
    int ldo;
    int Cout, M;
    // GroupNorm statistics of the OUTPUT, produced by the epilogue (conv_wino.hip only): per (frame, block-of-frame,
    // channel) [sum, sum of squares] as doubles, the layout gn_stats_partial writes -> the consumer's GroupNorm needs no
    // pass over the tensor.  stats_split = blocks per frame (conv_wino_stats_split).  Null: not produced.
    double* stats;
    int stats_split;
    // gemm_split.hip (linear layers whose rows are the pixels of consecutive frames): rows per frame; the table is then
    // [frame][stats_split = stats_hw / rows of a wave tile][Cout][2] (gemm_split_stats_rows)
    int stats_hw;
    // gemm_frag.hip, gemm_split.hip: zcount > 1 runs zcount independent problems of identical shape in one launch (blockIdx.z), the
    // relative-position nets of ALL attention blocks of one width (engine.hip: rpe_all).  Problem z reads src0 + z*zs_a and writes
    // out + z*zs_out (element strides); its weights and bias sit at no constant stride: wfrag = zbase + ztab[2z], bias = zbase + ztab[2z + 1]
    // (float offsets, device table).  wfrag / bias themselves hold problem 0's (the shape checks read them).
    int zcount, zs_a, zs_out;
    const long long* ztab = nullptr; const float* zbase = nullptr;
    // wsplit == 2: wwino is the image of pack_conv3_wino_split (conv_wino_r64.hip).  Otherwise:
    // wfrag is the bf16-split image of the weights (gemm_split.hip: fp32 accuracy from six bf16 piece products)
    int wsplit;
    // conv_wino_r64.hip, small grids only: scratch for split-K partial outputs (conv_wino_r64_ksplit_floats), or null
    float* ksplit_ws;
    size_t ksplit_ws_floats;
};

struct AttnSpatialArgs {
    const float* qkv;    // [nfr*L][3C]: q | k | v, each [heads][F]
    float* out;          // [nfr*L][C]
    int nfr, L, C, heads;
    float scale;
};

struct AttnTemporalArgs {
    const float* qkv;    // [B*T*HW][3C]
    const float* Rk;     // [B][T][T][C] or null
    const float* Rq;
    const float* Rv;
    const float* mask;   // [B][T] (1 = real frame) or null
    float* out;          // [B*T*HW][C]
    int B, T, HW, C, heads;
    int allow_pad;       // allow_interactions_between_padding
    float scale;
};

// ---- channels-last convolution and max pool of the feature networks (conv_cl.hip; LPIPS' 2-D layers are kt = 1 with the frames on T)
// out[m][co] = relu?(bias[co] + sum_k src(m, k) * w[co][k]), m = (ot*Ho + oy)*Wo + ox, k = ((dt*kh + dy)*kw + dx)*Cin + ci
enum ConvClGather {
    CG_QUAD,          // src [T][H][W][Cin], Cin % 4 == 0: four channels at a time
    CG_ELEM,          // src [T][H][W][Cin], element by element
    CG_NCHW_SCALED    // src [T][3][H][W], element by element, (v - shift[c]) / scale[c] on in-image taps only (lpips ScalingLayer)
};
struct ConvClArgs {
    const float* src;
    const float* w;      // [Cout][K], K = conv_cl_kpad(Kreal), zero behind Kreal (launch_conv_cl_pack)
    const float* bias;   // [Cout] or null
    float* out;          // row m at out + m*out_stride, Cout floats
    long long out_stride;
    int T, H, W, Cin, Cout, kt, kh, kw, st, sh, sw, pt, ph, pw, To, Ho, Wo, relu;
    float shift[3], scale[3];   // CG_NCHW_SCALED
    int M, K, Kreal;     // set by launch_conv_cl
};
inline int conv_cl_kpad(int kreal) { return (kreal + 31) / 32 * 32; }
int launch_conv_cl(ConvClArgs a, ConvClGather g, hipStream_t s);
// [Cout][Cin][taps] (OIHW / OIDHW) -> [Cout][K], zero for k >= Cin * taps
int launch_conv_cl_pack(const float* w, float* packed, int Cout, int Cin, int taps, hipStream_t s);
// the same from host memory into *packed (allocated on first use); returns when the image is complete
int conv_cl_load_weight(float** packed, const float* host, int Cout, int Cin, int taps);
// max pool over the in-volume taps (padding ignored): [T][H][W][C] -> [To][Ho][Wo][C], C % 4 == 0
struct PoolClArgs {
    const float* src;
    float* dst;
    int T, H, W, C, kt, kh, kw, st, sh, sw, pt, ph, pw, To, Ho, Wo;
};
int launch_maxpool_cl(const PoolClArgs& a, hipStream_t s);

int launch_igemm(const IgemmArgs& a, hipStream_t s);
int igemm_frames_per_launch(const IgemmArgs& a);   // frames (rows) per launch: big windows are cut along the frame dimension
IgemmArgs igemm_first_launch(const IgemmArgs& a);  // the args of the first launch launch_igemm makes for `a` (`a` itself when not cut)
// the kernel launch_igemm takes for ONE launch's args: the sub-pixel form of conv_wino_r64.hip, the split GEMM (gemm_split.hip, 1x1 or
// implicit-im2col 3x3), conv_wino_z128.hip (plain or activating), conv_wino_r64.hip, gemm_frag.hip, the fp32 Winograd kernel
// (conv_wino.hip), the generic kernel (igemm.hip)
enum IgemmKernel { IK_R64_UPS, IK_SPLIT, IK_Z128, IK_R64, IK_FRAG, IK_WINO, IK_GENERIC };
IgemmKernel igemm_kernel(const IgemmArgs& a);
int igemm_tile_class(int M, int Cout);   // 0: 128x128, 1: 128x64, 2: 64x128, 3: 64x64
// linear / 1x1 path with fragment-major weights (gemm_frag.hip); wfrag = [K/32][N/32][4][64][4]
bool gemm_frag_supported(const IgemmArgs& a);
int launch_gemm_frag(const IgemmArgs& a, int tile_class, hipStream_t s);
void pack_linear_frag(const float* w, float* out_base, int rows, int K, int n_total, int row0);
// Winograd F(2x2,3x3) path (conv_wino.hip): 2.25x fewer MFMAs than the direct 3x3 kernels
bool conv_wino_supported(const IgemmArgs& a);
// rows of the whole layer call a launch belongs to (IgemmArgs::nfr_sel): what the tile classes are chosen for
inline int igemm_sel_M(const IgemmArgs& a) { return a.nfr_sel > a.nfr ? a.nfr_sel * a.Ho * a.Wo : a.M; }
int conv_wino_stats_split(int Hout);
// ---- exact three-way bf16 split of a pair of fp32 values (conv_wino_r64.hip, VD_MATH=bf16x6), plain VALU only: v_pk_*_f32
// and v_dot2c_f32_bf16 do not overlap the bf16 MFMA (tools/mfma_bf16_coissue.hip).  Every piece is rounded to NEAREST
// (v_cvt_pk_bf16_f32): rounds 1-3 truncated (v_and_b32 0xffff0000), which gave the three dropped piece products the sign of
// a*b -- a systematic bias of ~10 % of the mean error (tools/mode_check.py signed_mean_err) -- at the same instruction count.
// first half: p1 = bf16 pair of (x0, x1), r = x - p1 (exact in fp32)
__device__ __forceinline__ void split_a(float x0, float x1, unsigned& p1, float& r0, float& r1, unsigned) {
    float h0, h1;
    asm("v_cvt_pk_bf16_f32 %0, %5, %6\n\t"
        "v_lshlrev_b32 %3, 16, %0\n\t"
        "v_and_b32 %4, 0xffff0000, %0\n\t"
        "v_sub_f32 %1, %5, %3\n\t"
        "v_sub_f32 %2, %6, %4"
        : "=&v"(p1), "=&v"(r0), "=&v"(r1), "=&v"(h0), "=&v"(h1)
        : "v"(x0), "v"(x1));
}
// second half: p2 = bf16 pair of r, p3 = r - p2 (at most 8 significant bits are left: exactly a bf16 value)
__device__ __forceinline__ void split_b(float r0, float r1, unsigned& p2, unsigned& p3, unsigned) {
    float h0, h1;
    asm("v_cvt_pk_bf16_f32 %0, %4, %5\n\t"
        "v_lshlrev_b32 %2, 16, %0\n\t"
        "v_and_b32 %3, 0xffff0000, %0\n\t"
        "v_sub_f32 %2, %4, %2\n\t"
        "v_sub_f32 %3, %5, %3\n\t"
        "v_cvt_pk_bf16_f32 %1, %2, %3"
        : "=&v"(p2), "=&v"(p3), "=&v"(h0), "=&v"(h1)
        : "v"(r0), "v"(r1));
}

// ---- arithmetic of the matrix products (VD_MATH, read once per process; every rank of a job must agree: the packed weight
// image depends on it -- vd_weights_layout_id):
//   f16x3  (default)  an fp32 operand x is carried as TWO fp16 pieces, x ~ a0 + 2^-12 a1 with a0 = f16(x) (round to nearest
//                     even) and a1 = f16((x - a0) * 2^12) (x - a0 is exact in fp32): 22 significand bits, relative error
//                     <= 2^-22 for 2^-14 <= |x| <= 65504, absolute error <= 2^-37 below (tools/mfma_f16_coissue.hip measures
//                     2^-23 worst over 2^20 values per binade); |x| > 65504 becomes inf and the product NaN -- loudly, never
//                     silently.  A product a*b is THREE piece products on v_mfma_f32_32x32x16_f16 with fp32 accumulation:
//                     a0*b0 (exact in fp32: 11 x 11 bits) + a0*b1 + a1*(2^-12 b0); the dropped a1*b1 is <= 2^-22 |ab|.
//                     Weights are scaled per output channel by a power of two on the host (max |w s| in [2^13, 2^14): every
//                     piece, 2^-12 b0 included, sits in fp16's normal range down to 2^-15 of the row's largest weight) and the
//                     epilogue multiplies by 1/s -- exact.  Measured against fp64 the result is at least as close as the fp32
//                     MFMA's (max <= 1.06x, mean <= 1.02x: profiles/r04_split_accuracy.json; tests/test_gpu_ops.py asserts
//                     <= 1.5x / 1.25x): the rounding of the fp32 accumulator dominates, and every mode shares it.
//   bf16x6            the EXACT split: x = x1 + x2 + x3, three bf16 pieces, six piece products (the default of rounds 1-3).
//   fp32              every product on v_mfma_f32_32x32x2_f32 (gemm_frag.hip, conv_wino.hip).
enum { MATH_F16X3 = 0, MATH_BF16X6 = 1, MATH_FP32 = 2 };
int math_mode();
inline bool f16_math() { return math_mode() == MATH_F16X3; }
// Split weight images (gemm_split.hip, conv_wino_r64.hip) are followed by a trailer of 2 * N floats, N = output channels of
// the image: [N] the power-of-two scale s the row was multiplied with (1 in bf16x6), [N] its reciprocal.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
// device: the two fp16 pieces of a pair of fp32 values.  p0 = {f16(x0), f16(x1)}; p1 = {f16((x0 - p0.lo) * 4096), f16(...)}:
// v_fma_mix_f32 reads the fp16 half directly (x - a0 in one instruction).  Plain VALU issue cost each
// (tools/mfma_f16_coissue.hip: they co-issue with the f16 MFMA like v_fma_f32): 2.5 instructions per value in all.
__device__ __forceinline__ unsigned f16_pack(float x0, float x1) {
    unsigned p;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p) : "v"(x0), "v"(x1));
    return p;
}
__device__ __forceinline__ float f16_rem_lo(unsigned p0, float x0) {
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(p0), "v"(x0));
    return r;
}
__device__ __forceinline__ float f16_rem_hi(unsigned p0, float x1) {
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(p0), "v"(x1));
    return r;
}
// p1 = {f16(r0 * 2^12), f16(r1 * 2^12)}: v_ldexp_f32 + v_cvt_pk_f16_f32.  (v_fma_mixlo/hi_f16 would scale and round in one
// instruction each, but they write HALF a register: gfx950 needs a wait state behind such a write before the register is read
// again, hipcc pads every one with an s_nop, and with one wave per SIMD an s_nop is an issue slot like any other: the ISA of
// round 4's first f16x3 loop carried nine of them per Winograd position.)
__device__ __forceinline__ unsigned f16_pack_scaled(float r0, float r1) {
    float s0, s1;
    unsigned p;
    asm("v_ldexp_f32 %0, %1, 12" : "=v"(s0) : "v"(r0));
    asm("v_ldexp_f32 %0, %1, 12" : "=v"(s1) : "v"(r1));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p) : "v"(s0), "v"(s1));
    return p;
}
// host packers of the split images (split_pack.hip); sizes in uint16 INCLUDING the trailer
size_t split_image_u16(size_t n_out, size_t k_total);            // n_out * k_total * 3 + 4 * n_out
// fp32-accurate Winograd conv on the 16-bit matrix cores (conv_wino_r64.hip); weights: [Cin/16][16][Cout/32][3][64][8] + trailer
void pack_conv3_wino_split(const float* oihw, unsigned short* out, int O, int I);
bool conv_wino_r64_supported(const IgemmArgs& a);        // wsplit == 2
int launch_conv_wino_r64(const IgemmArgs& a, hipStream_t s);
// the same convolution with the column half of the output transform on the matrix pipe, 64 tiles x 128 couts per block
// (conv_wino_z128.hip): f16x3, maps >= 16 x 16, Cout % 128 == 0; same weight image
bool conv_wino_z128_supported(const IgemmArgs& a);
bool conv_wino_z128_shape(int nfr, int H, int Cin, int Cout);     // the shape half of that decision (grid fill; conv_wino_z128.hip)
int launch_conv_wino_z128(const IgemmArgs& a, hipStream_t s);
// ... and with the GroupNorm(+FiLM) affine + SiLU of the input applied in the kernel's patch staging (a.affA / a.affB / a.act = 1): no activation image
bool conv_wino_z128_act_shape(int nfr, int H, int Cin, int Cout);
bool conv_wino_z128_act_supported(const IgemmArgs& a);
// Upsample (nearest x2) + conv3x3 in its sub-pixel form (conv_wino_r64.hip): four phase kernels per real cout over the
// LOW-resolution map, one of the four Winograd columns structurally zero and skipped.  IgemmArgs::ups_phase selects it;
// the GroupNorm table then has conv_wino_ups_stats_split(Hs) entries per frame.
void pack_conv3_wino_ups(const float* oihw, unsigned short* out, int O, int I);     // image of 4*O phase kernels
int conv_wino_ups_stats_split(int Hs);
int conv_wino_r64_ksplit(int nfr, int Hl, int Cin, int Cout);            // slices of the channel loop a small grid is cut into (1: none)
size_t conv_wino_r64_ksplit_floats(int nfr, int Hl, int Cin, int Cout, int nfr_sel = 0);  // floats of scratch the caller then provides in ksplit_ws (slices chosen for nfr_sel frames)
bool gemm_split_supported(const IgemmArgs& a);
bool gemm_split_side_supported(const IgemmArgs& a);   // IgemmArgs::side (the ResBlock's activation image from the skip conv's A tiles)            // fp32-accurate GEMM on the bf16 matrix cores (gemm_split.hip)
bool conv_split_supported(const IgemmArgs& a);          // 3x3, stride 1|2: the same kernel over an implicit im2col A
void pack_conv3_split(const float* w_oihw, unsigned short* out, int Cout, int Cin);
int launch_gemm_split(const IgemmArgs& a, int tile_class, hipStream_t s);
int gemm_split_tile_class(int M, int Cout);               // igemm_tile_class, or 4 = the 128x192 tile
int gemm_split_stats_rows(int M, int Cout);               // rows of a wave tile = rows behind one GroupNorm partial sum (64 | 32)
void pack_linear_split(const float* w, unsigned short* out_base, int rows, int K, int n_total, int row0);          // blocks per frame = partial sums per (frame, channel)
int launch_conv_wino(const IgemmArgs& a, hipStream_t s);
// Which instantiation serves ONE launch's IgemmArgs in this process' VD_MATH.  Every kernel file keeps ONE table of its instantiations;
// its launcher dispatches through the table and its *_variant() reads the same row, so what vd_igemm_variant() prints is what is launched.
// name: null = refused (why: the requirement that failed).  ksplit: slices of the channel loop (conv_wino_r64.hip with scratch), else 1.
struct IgemmVariant { const char* name; int ksplit; const char* why; };
IgemmVariant igemm_variant(const IgemmArgs& a);                          // igemm.hip: igemm_kernel()'s choice, then the file's own
std::string igemm_variant_name(const IgemmVariant& v);                   // e.g. "conv3x3_wino_r64_kernel<true,false>+ksplit4" | "refused: ..."
void igemm_variant_names(std::vector<std::string>& out);                 // every row of every table that this process' mode can launch
IgemmVariant gemm_split_variant(const IgemmArgs& a, int tile_class);
IgemmVariant gemm_frag_variant(const IgemmArgs& a, int tile_class);
IgemmVariant conv_wino_variant(const IgemmArgs& a);
IgemmVariant conv_wino_r64_variant(const IgemmArgs& a);
IgemmVariant conv_wino_z128_variant(const IgemmArgs& a);
void gemm_split_variant_names(std::vector<std::string>& out);
void gemm_frag_variant_names(std::vector<std::string>& out);
void conv_wino_variant_names(std::vector<std::string>& out);
void conv_wino_r64_variant_names(std::vector<std::string>& out);
void conv_wino_z128_variant_names(std::vector<std::string>& out);
void pack_conv3_wino(const float* oihw, float* out, int O, int I);      // out: 16*O*I floats
int launch_attn_spatial(const AttnSpatialArgs& a, hipStream_t s);
// Which instantiation a spatial-attention shape runs on in this process' VD_MATH: the ONE place the choice is made (the table of
// attn_spatial.hip).  launch_attn_spatial dispatches through it and vd_attn_spatial_variant() prints it.  A function of L, the head
// dim and the mode alone (never of the frame count).  row: index into that table, -1 = refused.
struct AttnSpatialVariant {
    int row;
    int F, NW;           // head dim; waves per block of attn_spatial_split_kernel, 0 = attn_spatial_kernel<F> (VD_MATH=fp32)
    bool f16;            // the split kernel's F16
    const char* why;     // refused: the requirement that failed
};
AttnSpatialVariant attn_spatial_variant(int L, int C, int heads);
std::string attn_spatial_variant_name(const AttnSpatialVariant& v);     // e.g. "attn_spatial_split_kernel<64,true,8>"
int launch_attn_temporal(const AttnTemporalArgs& a, hipStream_t s);
// Which instantiation a temporal-attention shape runs on: the ONE place the choice is made (attn_temporal.hip).  Both launchers
// dispatch through it and vd_attn_temporal_variant() prints it, so what the tests ask for is what is launched.  A function of the
// per-item shape alone (never of B).  p0 / p1: NT, JM (kMfma) | PB, TMAX (kValu) | NJ, - (kLongMfma) | -, - (kLongGeneric).
struct AttnTemporalVariant {
    enum Family { kRefused = 0, kMfma, kValu, kLongMfma, kLongGeneric };
    Family family;
    int p0, p1;
    bool exact, rpe;     // exact: kMfma's EXACT
    size_t lds;          // kValu: dynamic LDS bytes of the block
    const char* why;     // kRefused: the requirement that failed
};
AttnTemporalVariant attn_temporal_variant(int T, int HW, int C, int heads, bool rpe);
std::string attn_temporal_variant_name(const AttnTemporalVariant& v);   // e.g. "attn_temporal_mfma_kernel<1,6,true,true>"
int launch_attn_temporal_long(const AttnTemporalArgs& a, hipStream_t s);   // 33 <= T <= kMaxWindowFrames (attn_temporal_long.hip)

// GroupNorm statistics over (pixels x channels-of-group) of one frame, 32 groups, virtual concat.
// part: workspace of nfr*split*C*2 doubles (per-channel fp64 sum / sum of squares per pixel range).
int launch_gn_stats(const float* src0, const float* src1, int C0, int C, int nfr, int HW, double* part, int split,
                    hipStream_t s);
int gn_stats_split(int nfr, int HW, int C);
// affA/affB[n][c] = fold(mean, rstd, gamma, beta, FiLM scale/shift).  film: [nfr][film_ld], scale at +0, shift at +C.
// count = elements per group (HW * C/32)
int launch_gn_affine(const double* part0, int split0, int C0, const double* part1, int split1, double count,
                     const float* gamma, const float* beta, const float* film, int film_ld, int nfr, int C, float* affA,
                     float* affB, hipStream_t s, float* mr_out = nullptr);      // mr_out: [nfr][32][2] mean, rstd (backward pass)
// launch_gn_affine + launch_affine_act in one launch: every block folds its frame's statistics itself (norm.hip).
struct GnFold { const double* part0; int split0; const double* part1; int split1; double count; const float* gamma; const float* beta;
                const float* film; int film_ld; };
int launch_affine_act_fold(const float* src0, const float* src1, int C0, int C, const GnFold& f, int nfr, int HW, int act, float* y,
                           hipStream_t s);
// y = x*A[n][c] + B[n][c]  (materialised normalisation for the attention residual, unet.py:474,538)
// y[n][p][0..C) = silu?(concat(src0, src1)[n][p][c] * A[n][c] + B[n][c])
int launch_affine_act(const float* src0, const float* src1, int C0, int C, const float* affA, const float* affB, int nfr,
                      int HW, int act, float* y, hipStream_t s);
int launch_affine_apply(const float* x, const float* affA, const float* affB, int nfr, int HW, int C, float* y,
                        hipStream_t s);
// Temporal GroupNorm: stats over (T x C/32) for every (b, pixel); writes the normalised tensor.
int launch_gn_temporal(const float* x, const float* gamma, const float* beta, int B, int T, int HW, int C, float* y,
                       hipStream_t s);

struct AssembleArgs {
    const float* x;      // [B][T][3][H][W]
    const float* obs_src;// frames substituted where obs_mask=1 (x0 / x / x_t_minus_1)
    const float* obs_mask, *lat_mask, *km_mask;   // [B*T]
    const float* t_model;// [B] value handed to the network (already mapped / rescaled)
    int obs_t_mode;      // 0: 'x_0' (obs frames see t=0), 1: 'x_t', 2: 'x_t_minus_1'
    int B, T, H, W, Kpad;
    int cond_mode;       // vd_config::cond_emb_type: 0 channel (5 stem channels), 1 duplicate|all (6), 2 t=0 (3)
    float* x_cols;       // [B*T*H*W][Kpad]: im2col of the stem's input for the 3x3 stem, k = tap*Cs + channel
    float* t_frames;     // [B*T]
    float* amask;        // [B*T] anything mask
    // window prefix cache (engine.hip): with a frame list the im2col rows of frames list[0..n_list) are written COMPACTLY
    // (row block i <- frame list[i]) and the per-frame scalars are left alone; scalars_only writes t_frames / amask of every
    // frame and no im2col
    const int* frame_list = nullptr;
    int n_list = 0;
    int scalars_only = 0;
};
int launch_assemble(const AssembleArgs& a, hipStream_t s);
// frame-granular moves of the window prefix cache: dst[i] = src[list[i]] (rows of row_floats), dst[list[i]] = src[i], and the
// GroupNorm partial table of a compact tensor folded to ONE entry per (frame, channel) at its frame's place
int launch_gather_rows(const float* src, const int* list, int n, size_t row_floats, float* dst, hipStream_t s);
int launch_scatter_rows(const float* src, const int* list, int n, size_t row_floats, float* dst, hipStream_t s);
int launch_scatter_stats(const double* src, int split, int C, const int* list, int n, double* dst, hipStream_t s);
// out[n] = [cos(t*f) | sin(t*f)] with the frequency table built on the host (nn.py:89-107)
int launch_sinus_embed(const float* t, int n, int dim, const float* freqs, float* out, hipStream_t s);
// RPENet hidden: E[b,t,s,c] = silu(te[b*T+t][c] + Wd[c][:]*feat(d) + bd[c]), d = fi[b,t]-fi[b,s]  (unet.py:283-296)
// nz nets at once (blockIdx.y): net z reads te + tab[3z], wbase + tab[3z + 1] (Wd), wbase + tab[3z + 2] (bd) and writes E + z*zs_e
int launch_rpe_hidden_tab(const float* te, int te_ld, const float* wbase, const long long* tab, const int64_t* fidx, int B, int T, int C,
                          float* E, int nz, size_t zs_e, hipStream_t s);
// bucket-table path (unet.py:330-347): R[b,t,s,:] = table[bucket(d)]
int launch_rpe_table(const float* table, const int64_t* fidx, int B, int T, int C, float alpha, float beta,
                     float gamma, float* R, hipStream_t s);
// h = x + P[pixel][c] (+ frame embedding [n][c])
int launch_posenc_add(const float* x, const float* P, const float* femb, int nfr, int HW, int C, float* y,
                      hipStream_t s);
// tv[b*T+t] = fidx - (center ? mean_t fidx : 0)   (unet.py:914-926)
int launch_frame_t(const int64_t* fidx, int B, int T, int center, float* tv, hipStream_t s);
// out conv: GN-affine + SiLU + conv3x3 (C -> Cout<=8), NHWC in, NCHW out  (unet.py:744-749,838).  The direct form, launched by
// vd_op_out_conv alone: the forward runs the head as the GEMM + gather below
int launch_out_conv(const float* x, const float* affA, const float* affB, const float* w, const float* bias, int nfr,
                    int H, int W, int C, int Cout, float* out_nchw, hipStream_t s);

// the head's first half as its own kernel: T[pixel][ldt] = silu(h * A + B) . Wt^T, Wt [ldt][C] fp32 (misc.hip)
bool head_gemm_supported(int HW, int C, int ldt);
int head_gemm_tiles_per_wave(int nfr, int HW);                           // the launch form of head_gemm_kernel: 2 | 8
int launch_head_gemm(const float* h, const float* affA, const float* affB, const float* Wt, int nfr, int HW, int C, int ldt, float* T, hipStream_t s);
// the head's second half: out_nchw[n][co][y][x] = bias[co] + sum_tap T[n][y + dy][x + dx][co * 9 + tap] (zero outside the image); T [nfr][H][W][ldt]
int launch_out_gather(const float* T, const float* bias, int nfr, int H, int W, int ldt, int Cout, float* out_nchw, hipStream_t s);

// The samplers of the step path.  The values are ABI (vd_window_begin's `sampler`, vd_posterior_update's `mode`).
enum Sampler { SAMPLER_P = 0, SAMPLER_DDIM = 1, SAMPLER_DDIM_REVERSE = 2, SAMPLER_DPMPP_2M = 3, SAMPLER_DPMPP_2M_SDE = 4, SAMPLER_UNIPC = 5 };
inline bool sampler_valid(int s) { return s >= SAMPLER_P && s <= SAMPLER_UNIPC; }
inline bool sampler_walks_up(int s) { return s == SAMPLER_DDIM_REVERSE; }                   // t += 1 per step; the others walk down to 0
inline bool sampler_draws_noise(int s) { return s == SAMPLER_P || s == SAMPLER_DDIM || s == SAMPLER_DPMPP_2M_SDE; }   // the others read no noise and no Philox state
inline bool sampler_has_history(int s) { return s == SAMPLER_DPMPP_2M || s == SAMPLER_DPMPP_2M_SDE || s == SAMPLER_UNIPC; }   // reads the previous step's x_0 prediction
inline bool sampler_is_unipc(int s) { return s == SAMPLER_UNIPC; }     // its history is three tensors, its rows vd_set_unipc_rows' (not the multistep weight row)
// the entries that take a `mode` (vd_posterior_update, vd_posterior_from_xstart, vd_dps_step) serve these two alone: sampler 4 draws
// noise too but has entries of its own
inline bool sampler_is_posterior(int s) { return s == SAMPLER_P || s == SAMPLER_DDIM; }
inline const char* sampler_name(int s) {
    return s == SAMPLER_P ? "p_sample" : s == SAMPLER_DDIM ? "ddim_sample" : s == SAMPLER_DDIM_REVERSE ? "ddim_reverse_sample"
         : s == SAMPLER_DPMPP_2M ? "dpmpp_2m_sample" : s == SAMPLER_DPMPP_2M_SDE ? "dpmpp_2m_sde_sample" : "unipc_sample";
}
// The closing pass of a step (misc.hip: launch_sampler_pass), one argument block for every sampler.
struct SamplerPassArgs {
    int sampler;            // Sampler
    const float* x;         // x_t   [B][per]
    const float* eps;       // model output (not read when x0_given is set)
    const float* x0_given;  // START_X models, the thresholded x_0 and the denoised_fn path: the x_0 prediction itself, or null
    const int64_t* t;       // [B] respaced index
    const float* tab;       // [NTAB][num_timesteps] float32 tables (gathered in f64 on host, cast like the reference)
    int num_timesteps;
    int B; long per;        // samplers that draw no noise: per % 4 == 0, every tensor 16-byte aligned (launch_sampler_pass checks);
                            // dpmpp_2m_sde, unipc: any per and alignment (16-byte accesses where per % 4 == 0 and every tensor is aligned)
    int clip;
    float* sample;          // x_{t-1} (x_{t+1}: ddim_reverse); may alias x: the update is elementwise.  Null: SAMPLER_P only (p_mean_variance)
    float* xstart;          // the x_0 prediction (dpmpp_2m: D_t, the next step's history), or null
    int* err;               // the engine's sticky error word: bit 1 is set when the network output (eps, or the x_0 handed in) is not
                            // finite -- the clamp of clip_denoised would otherwise turn a NaN into a plausible -1 silently
    // ---- p_sample, ddim_sample (dpmpp_2m_sde: noise, seed, offset and dstate; it reads no eta and writes no mean)
    float* mean = nullptr;              // p_mean_variance's 'mean' (posterior mean of the clipped x0 prediction), or null
    float eta = 0.f;
    const float* noise = nullptr;       // explicit noise or null (then Philox(seed, offset))
    unsigned long long seed = 0, offset = 0;
    const unsigned long long* dstate = nullptr;     // window executor: {seed, offset} read from device memory instead of the arguments
    // ---- dpmpp_2m_sample, dpmpp_2m_sde_sample
    const float* hist = nullptr;        // D_prev: the previous step's D_t, or null (no history).  May alias xstart: element i is read and then
                                        // written by the same thread, which is how the window executor keeps its history in place
    const unsigned long long* hist_on = nullptr;    // or null; a device word: 0 = this step has no history whatever `hist` holds (a window's first step)
    const float* w = nullptr;           // [num_timesteps] extrapolation weights (vd_set_multistep_weights); w[0] = w[num_timesteps - 1] = 0
    // ---- unipc_sample (it also reads hist_on: there the COUNT of finished steps, in place of `count`, when set)
    const float* urows = nullptr;       // [UNIPC_ROWS][num_timesteps] coefficient rows (vd_set_unipc_rows)
    const float *ubase = nullptr, *ud1 = nullptr, *ud2 = nullptr;      // the state read: x^c_{t+1}, D_{t+1}, D_{t+2}; all null = no state (count 0)
    float *ubase_out = nullptr, *ud1_out = nullptr, *ud2_out = nullptr; // the state written: x^c_t, D_t, D_{t+1}; all null = not kept.  Each may
                                        // alias any tensor read: element i is read and then written by the same thread
    int count = 0;                      // steps the chain has finished (host); the pass uses min(count, num_timesteps - 1 - t[b])
};
// unipc_sample's rows, per respaced index t: the corrector into t (move t+1 -> t) x^c = c0 base + c1 D1 + c2 D2 + c3 D_t at order 1 and
// order 2, then the predictor t -> t-1, sample = p0 x^c + p1 D_t + p2 D1, at order 1 and order 2
enum { UNIPC_C1 = 0, UNIPC_C2 = 4, UNIPC_P1 = 8, UNIPC_P2 = 11, UNIPC_ROWS = 14 };
enum { VD_ERR_TIMESTEP = 1, VD_ERR_NONFINITE = 2 };
int launch_sampler_pass(const SamplerPassArgs& a, hipStream_t s);
// cfg_scale (this project's extension: classifier-free guidance on the observed frames): out[i] = fmaf(w, out_c[i] - out_u[i], out_u[i]),
// NaN where the difference is not finite, out_u[i] itself at w = 0.  Any n > 0; out may alias out_c or out_u; 16-byte aligned tensors take
// the float4 path, others run element by element.  w must be finite.
int launch_cfg_combine(const float* out_c, const float* out_u, float w, long long n, float* out, hipStream_t s);
// The two element formulas more than one source needs bit for bit (misc.hip's sampler passes and cfg_combine_kernel, guidance.hip):
// one guided network output, and the x_0 prediction of an epsilon-model -- two products, each rounded, then one subtraction.
__device__ __forceinline__ float cfg_combine_one(float c, float u, float w) {
    const float d = c - u;
    if (!(fabsf(d) <= 3.4028234e38f)) return __builtin_nanf("");
    return w == 0.0f ? u : fmaf(w, d, u);
}
__device__ __forceinline__ float xstart_from_eps(float sr, float x, float srm1, float eps) {
#pragma clang fp contract(off)
    const float a = sr * x, b = srm1 * eps;
    return a - b;
}
// The x_0 prediction: an epsilon-model's through xstart_from_eps (two products, each rounded, then one subtraction -- never a fused
// multiply-add), or the one handed in.  The step through `denoised_fn` takes its x_0 from the p_sample pass (vd_p_mean_variance) and hands
// it to the *_from_xstart form of another: with one head, the fused step and that form agree to the bit for denoised_fn = identity.
// A network output that is not finite -- in the f16x3 arithmetic: an operand beyond fp16's range (|x| > 65504) anywhere in the network --
// must not leave through the clamp as a plausible -1 (fmaxf(NaN, -1) = -1): it is left as it is and raises `nonfinite`.
__device__ __forceinline__ float pass_x0(float x, float src, bool given, float sr, float srm1, int clip, bool& nonfinite) {
    float x0 = given ? src : xstart_from_eps(sr, x, srm1, src);
    const bool bad = !(fabsf(x0) <= 3.4028234e38f);
    nonfinite |= bad;
    if (clip && !bad) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    return x0;
}
// Guidance rescale and dynamic thresholding (guidance.hip; this project's extensions).  Tensors are [B][T][frame_elems], `lat` the [B*T]
// latent mask: an item's statistic runs over the elements of its frames with lat == 1.  `scratch`: guidance_scratch_bytes(B) bytes, 256-byte
// aligned, the caller's; nothing here allocates or waits for the device.
size_t guidance_scratch_bytes(int B);
// out = cfg_combine_one(out_c, out_u, w), times f = 1 + phi (sigma_c / sigma_g - 1) on the latent frames (f = 1 where sigma_g = 0 or nothing
// is latent); factor_out [B] or null; out may alias out_c or out_u
int launch_cfg_rescale(const float* out_c, const float* out_u, float w, const float* lat, int B, int T, long frame_elems, float phi,
                       float* out, float* factor_out, void* scratch, hipStream_t s);
struct DynThreshArgs {
    const float* src;       // the network output: eps (x != null) or the x_0 prediction itself (x == null)
    const float* x;         // x_t, or null
    const int64_t* t;       // [B] respaced index (read with x only)
    const float* tab;
    int num_timesteps;
    const float* lat;
    int B, T; long frame_elems;
    float p;                // the percentile, (0, 1]
    float* out;             // the finished x_0: latent frames clamp(x_0, -s, s) / s, other frames clamp(x_0, -1, 1); may alias src
    float* s_out;           // [B] the thresholds max(s, 1) (NaN for an item with a non-finite latent x_0), or null
    int* err;               // as SamplerPassArgs::err, or null
    void* scratch;
};
int launch_dynamic_threshold(const DynThreshArgs& a, hipStream_t s);
int launch_q_sample(const float* x0, const float* noise, const int64_t* t, const float* tab, int num_timesteps, int B,
                    long per, float* out, hipStream_t s);
int launch_randn(float* out, long n, unsigned long long seed, unsigned long long offset, hipStream_t s);
int launch_q_sample_prev(const float* x0, const int64_t* t, const float* tab, int num_timesteps, int B, long per, const unsigned long long* dstate,
                         unsigned long long draw_offset, float* out, hipStream_t s);

// Pixel-mask inpainting (known.hip; this project's extension, RePaint: Lugmayr et al. 2022).  Tensors are [B][T][3][hw] (the mask
// [B][T][hw], broadcast over the channels), `lat` the [B*T] latent mask.
// The merge, the closing pass of a step in place on `sample`: an element whose frame has lat == 1 and whose pixel has mask != 0 becomes
// q_sample(known_src, t - 1, z) in q_sample_kernel's rounding order (known_src itself at t == 0); every other element keeps its bits.
// z: noise[i], or normal_at(seed, offset + B*per/4, i) with per = T*3*hw -- the free quarter of a step's Philox range -- the pair read
// from `dstate` when given.  A t[b] outside the schedule: NaN for every element of item b; no error bit (the sampler pass set it).
// Four elements per thread while hw % 4 == 0 and the tensors are 16-byte aligned, else element by element: same bits.
struct KnownMergeArgs {
    float* sample;
    const float* known_src; const float* known_mask; const float* lat;
    const int64_t* t;       // [B] respaced index of the step that produced `sample`
    const float* tab; int num_timesteps;
    int B, T; long hw;
    const float* noise = nullptr;
    unsigned long long seed = 0, offset = 0;
    const unsigned long long* dstate = nullptr;
};
int launch_known_merge(const KnownMergeArgs& a, hipStream_t s);
// One forward diffusion step x_{t-1} -> x_t at index t[b] on the frames with lat == 1: out = fmaf(sqrt_beta[t], z, sqrt_alpha[t] * x);
// other frames out = x (in place: untouched).  rows: [2][num_timesteps] = sqrt(1 - beta) | sqrt(beta), float32 casts of the float64 values
// (1 - alpha is never formed in fp32).  z: noise[i] or normal_at(seed, offset, i), the pair from `dstate` when given.  Bad t[b]: NaN for item b.
struct QJumpArgs {
    const float* x; float* out;        // out may be x
    const float* lat;
    const int64_t* t;
    const float* rows; int num_timesteps;
    int B, T; long hw;
    const float* noise = nullptr;
    unsigned long long seed = 0, offset = 0;
    const unsigned long long* dstate = nullptr;
};
int launch_q_jump(const QJumpArgs& a, hipStream_t s);

// FreeU (freeu.hip; this project's extension, Si, Huang, Jiang, Liu 2024): the two operators on the halves of a decoder concat.
// Tensors are channels-last [N][S*S][C], C % 4 == 0, 16-byte aligned; never in place.  Sums in fp64, fixed order, no atomics.
// freeu_trig_table: cos(2 pi k / S) | sin(2 pi k / S), k < S, into 2 S host doubles; the launchers read its device copy (`trig`).
// launch_freeu_filter: per (frame, channel) plane y = Re ifft2(M . fft2(x)), M = s on the bins {0, S-1}^2 and 1 elsewhere (closed form,
// a rank-7 update); s == 1 copies.  launch_freeu_backbone: channels c < C/2 times (float)b (plain), or times (b - 1) g + 1 with g the
// per-frame min-max normalised channel mean (adaptive; `map`: N * S * S doubles of scratch; hi == lo: g = 0); the others copied.
void freeu_trig_table(int S, double* out);
int launch_freeu_filter(const float* x, int N, int S, int C, double s, const double* trig, float* y, hipStream_t st);
int launch_freeu_backbone(const float* h, int N, int S, int C, double b, int adaptive, double* map, float* y, hipStream_t st);

// Zero-shot restoration (measure.hip; this project's extension, DDNM: Wang, Yu, Zhang 2022): the projection of a step's x_0 prediction onto
// a measurement, x_0 <- x_0 + A^+(y - A x_0), for the "cell mean" operators.  Tensors are [B][T][3][H][W], `lat` the [B*T] latent mask.
// A cell is scale x scale pixels of one channel plane (gray: of the three planes of its frame); A is the mean over every cell,
// y [B][T][Cy][H/scale][W/scale] with Cy = 3 (gray: 1); A^+ replicates.  In one launch: x_0 = pass_x0(...) -- from (x, src = eps) with the
// tables at t[b], or src itself when x is null, clamped when `clip` -- then, on the frames with lat == 1, every element of a cell becomes
// x_0 + (y_cell - mean_cell(x_0)); other frames get x_0 unprojected.  out may alias src.  Fixed summation order, no atomics: an item's
// bits do not depend on B.  A cell with a value that is not finite comes out not finite; no error bit (the sampler pass behind it sets
// it).  A t[b] outside the schedule (x != null): item b of `out` is not written, the sampler pass poisons the item without reading it.
// 16-byte accesses while W % 4 == 0 and x, src, out are 16-byte aligned, else element by element: same bits.
struct MeasureArgs {
    const float* x;         // x_t, or null: src is the x_0 prediction itself
    const float* src;       // the network output (eps), or the x_0 prediction
    float* out;
    const float* y;
    const float* lat;
    const int64_t* t;       // [B] respaced index (read with x only)
    const float* tab; int num_timesteps;
    int B, T, H, W;
    int scale, gray, clip;
};
inline bool measurement_served(int scale, int gray) { return scale == 2 || scale == 4 || scale == 8 || (scale == 1 && gray); }
int launch_measurement_project(const MeasureArgs& a, hipStream_t s);

// Diffusion posterior sampling (dps.hip; this project's extension, DPS: Chung et al. 2023) on the operators above.  Tensors are
// [B][T][3][H][W], y [B][T][Cy][H/scale][W/scale], `lat` the [B*T] latent mask.  launch_dps_seed, two launches: per item b, over the cells
// of its frames with lat == 1, r = y - A x_0 with x_0 = pass_x0(x, eps, ...) at t[b] (clamped when `clip`), rho_b = sqrt(sum r^2) -- the
// sum folded in fp64 in a fixed order that does not depend on B, rounded once to fp32 -- and the cotangents of rho_b: q = -r_cell / (rho_b n_c)
// on every element of a cell (n_c = scale^2, gray: 3 scale^2), q_r = q where !clip or -1 <= x_0r <= 1 else 0, deps = -sqrt_recipm1[t] q_r,
// dxd = sqrt_recip[t] q_r; 0 on every other frame, and everywhere for an item with rho_b == 0 or no latent frame.  A t[b] outside the
// schedule: NaN in deps, dxd, rho and xstart of item b, and bit 0 of `err`.  16-byte accesses while W % 4 == 0 and the tensors are
// 16-byte aligned, else element by element: same bits.  No floating-point atomics.
struct DpsArgs {
    const float* x;         // x_t
    const float* eps;       // the network output
    const float* y;
    const float* lat;
    const int64_t* t;       // [B] respaced index
    const float* tab; int num_timesteps;
    int B, T, H, W;
    int scale, gray, clip;
    float* r;               // scratch: y's shape
    double* part;           // scratch: [B][dps_partials_per_item()]
    float* deps; float* dxd;
    float* xstart;          // the x_0 prediction of every frame (the sampler pass's bits), or null
    float* rho;             // [B], or null
    int* err;               // the engine's sticky error word, or null
    int nblk = 0;           // set by launch_dps_seed: partials per item of this launch
};
size_t dps_partials_per_item();
int launch_dps_seed(DpsArgs a, hipStream_t s);
// the residual pass of launch_dps_seed alone: r and part; *nblk = the partials per item it wrote
int launch_dps_residual(DpsArgs a, int* nblk, hipStream_t s);
// g = dxd + dx_net * gs[1] (launch_grad_rescale's 1 / s) -> grad (or null); sample = fmaf(-zeta, g, sample) on the frames with lat == 1
int launch_dps_final(const float* dxd, const float* dx_net, const float* gs, const float* lat, int B, int T, long frame_elems, float zeta,
                     float* sample, float* grad, hipStream_t s);

// Deblurring (blur.hip; this project's extension): DPS and the built-in reward of particle steering on the measurement y = w * x_0 + noise
// of one real k x k kernel w (k odd, 1 <= k <= kMaxBlurTaps), applied to every channel plane of every frame at "same" size with zeros
// outside the plane, oriented as torch's conv2d.  Tensors and y are [B][T][3][H][W].  launch_blur_seed is launch_dps_seed for this
// operator -- r = y - A x_0, rho_b, and q = -(A^T r) / rho_b in place of -r_cell / (rho_b n_c); everything else, the poisoning of an item
// whose t[b] lies outside the schedule included, as DpsArgs states it.  `taps`: k*k floats on the device, row-major.
constexpr int kMaxBlurTaps = 15;
inline bool blur_served(int k) { return k >= 1 && k <= kMaxBlurTaps && (k & 1); }
struct BlurArgs {
    const float* x;         // x_t
    const float* eps;       // the network output
    const float* y;
    const float* lat;
    const int64_t* t;       // [B] respaced index
    const float* tab; int num_timesteps;
    int B, T, H, W;
    const float* taps; int k;
    int clip;
    float* r;               // scratch: y's shape
    double* part;           // scratch: [B][dps_partials_per_item()]
    float* deps; float* dxd;
    float* xstart;          // the x_0 prediction of every frame (the sampler pass's bits), or null
    float* rho;             // [B], or null
    int* err;               // the engine's sticky error word, or null
    int nblk = 0;           // set by launch_blur_seed: partials per item of this launch
};
int launch_blur_seed(BlurArgs a, hipStream_t s);
// the residual pass of launch_blur_seed alone: r and part; *nblk = the partials per item it wrote
int launch_blur_residual(BlurArgs a, int* nblk, hipStream_t s);
// out = A x (adjoint == 0) or A^T x of `planes` planes of H x W; out != x
int launch_blur_apply(const float* x, const float* taps, int k, int adjoint, size_t planes, int H, int W, float* out, hipStream_t s);

// Separable linear measurements (linop.hip; this project's extension): the projection of measure.hip, DPS and the built-in reward of
// particle steering on a measurement y[b][t][c] = A_h x_0[b][t][c] A_w^T of two dense row-major matrices on the device, A_h (Mh x H) and
// A_w (Mw x W), 1 <= Mh <= H <= kMaxLinopSide, 1 <= Mw <= W <= kMaxLinopSide.  Tensors are [B][T][3][H][W], y and r [B][T][3][Mh][Mw].
// Every product is Z = L X R^T, the right factor first, each sum from 0 in ascending index order, product and sum each rounded to fp32.
// launch_linop_seed is launch_blur_seed for this operator -- r = y - A x_0, rho_b, and q = -(A_h^T r A_w) / rho_b; everything else, the
// poisoning of an item whose t[b] lies outside the schedule included, as DpsArgs states it.  x null (residual pass only): src is the x_0
// prediction itself, t and the tables are not read, and xstart may alias src.
constexpr int kMaxLinopSide = 128;
inline bool linop_served(int n, int m) { return m >= 1 && m <= n && n <= kMaxLinopSide; }
struct LinopArgs {
    const float* x;         // x_t, or null (residual pass): src is the x_0 prediction
    const float* src;       // the network output (eps), or the x_0 prediction
    const float* y;
    const float* lat;
    const int64_t* t;       // [B] respaced index (read with x only)
    const float* tab; int num_timesteps;
    int B, T, H, W, Mh, Mw;
    const float* A_h; const float* A_w;
    int clip;
    float* r;               // y's shape: the residual on the latent frames
    double* part;           // scratch: [B][dps_partials_per_item()]; null (residual pass only): sum r^2 is not kept
    float* deps; float* dxd;
    float* xstart;          // the x_0 prediction of every frame (the sampler pass's bits), or null
    float* rho;             // [B], or null
    int* err;               // the engine's sticky error word, or null
    int nblk = 0;           // set by the launchers: partials per item of this launch
};
int launch_linop_seed(LinopArgs a, hipStream_t s);
// the residual pass of launch_linop_seed alone: r, part and xstart where given; *nblk (or null) = the partials per item it wrote
int launch_linop_residual(LinopArgs a, int* nblk, hipStream_t s);
// x0 <- x0 + P_h r P_w^T on the frames with lat == 1, in place (P_h: H x Mh, P_w: W x Mw, on the device); other frames keep their bits
int launch_linop_project(float* x0, const float* r, const float* lat, const float* P_h, const float* P_w, int B, int T, int H, int W, int Mh,
                         int Mw, hipStream_t s);
// out = L x R^T of `planes` planes of Q x U (L: P x Q, R: S x U, on the device; out planes of P x S); out != x
int launch_linop_apply(const float* x, const float* L, int P, int Q, const float* R, int S, int U, size_t planes, float* out, hipStream_t s);

// Particle steering (particles.hip; this project's extension, Feynman-Kac steering: Singhal et al. 2025): B = G*K items, item g*K + k is
// particle k of group g.  launch_particle_weights, one block per group: the weight update logw += lambda (r - rprev) from the items' rewards
// (`rewards`, or r = -(sum_j part[b][j]) * inv_two_var, the partials folded in index order), p = softmax(logw), ess = 1 / sum p^2, and --
// unless the group's logw are bit-equal, t[g*K] == 0 or ess >= tau K -- systematic resampling at uni[2g]: ancestors[g*K + i] = g*K + a_i,
// rprev_i = rprev_{a_i}, logw_i = 0, counters[2g] += 1; otherwise identity ancestors.  t[g*K] == 0: chosen[g] = the inverse CDF at
// uni[2g + 1], else -1.  A group whose logw are all -inf: left as it is, counters[2g + 1] += 1.  Sums in index order in fp64, no atomics.
constexpr int kMaxParticles = 256;
struct ParticleArgs {
    int G, K;
    double lambda, tau;
    const double* rewards;  // [B], or null: from the partials
    const double* part; int nblk; double inv_two_var;
    const int64_t* t;       // [B] respaced index of the step just made (a group's items share it)
    const double* uni;      // [G][2], each in [0, 1); or null: words 0..3 of Philox block (seed, offset + pos + g), 53 bits each pair,
                            // the pair (seed, offset) read from `dstate` when given
    double* logw; double* rprev;                     // [B], updated in place
    int* ancestors; int* chosen; double* ess;        // [B], [G], [G]
    long long* counters;                             // [G][2]: resamplings, degenerate steps
    unsigned long long seed = 0, offset = 0, pos = 0;
    const unsigned long long* dstate = nullptr;
};
int launch_particle_weights(const ParticleArgs& a, hipStream_t s);
// launch_particle_gather, one launch: item i of each of the n <= 4 tensors x[k] ([B][per] floats) takes the content of item anc[i]; any map,
// cycles included.  scratch: n*B*per floats.  Items with anc[i] == i are neither read nor written; nothing moved: no traffic but the indices.
// 16-byte accesses while per % 4 == 0 and every pointer is 16-byte aligned, else element by element: same bits.
struct GatherArgs {
    float* x[4]; int n;
    int B; long long per;
    const int* anc;
    float* scratch;
};
int launch_particle_gather(const GatherArgs& a, hipStream_t s);

// Loss-guided sampling (guide.hip; this project's extension): a reverse step moved down the gradient of a caller's function of its x_0
// prediction.  Tensors are [B][T][3][H][W], `lat` the [B*T] latent mask.  launch_guide_seed: on the frames with lat == 1, with cot the
// caller's d loss / d x_0, c_r = cot where !clip or -1 <= x_0r <= 1 else 0 (x_0r = xstart_from_eps(...) at t[b]: the sampler pass's bits),
// deps = (-sqrt_recipm1[t]) c_r, dxd = sqrt_recip[t] c_r; 0 on every other frame.  A t[b] outside the schedule: NaN on the item and bit 0
// of `err`; a cot that is not finite propagates and raises nothing.  16-byte accesses while W % 4 == 0 and the tensors are 16-byte
// aligned, else element by element: same bits.
struct GuideSeedArgs {
    const float* x; const float* eps; const float* cot; const float* lat;
    const int64_t* t; const float* tab; int num_timesteps;
    int B, T, H, W, clip;
    float* deps; float* dxd;
    int* err;               // the engine's sticky error word, or null
};
int launch_guide_seed(const GuideSeedArgs& a, hipStream_t s);
// launch_guide_norm: part[b][k], k < guide_norm_blocks(per), the fp64 partial sums of g^2 over the item's frames with lat == 1,
// g = dxd + dx_net * gs[1] in fp32 (launch_guide_final's g), in an order that depends on (T, frame_elems) alone.
int guide_norm_blocks(long per);
int launch_guide_norm(const float* dxd, const float* dx_net, const float* gs, const float* lat, int B, int T, long frame_elems, double* part,
                      hipStream_t s);
// launch_guide_final: g = dxd + dx_net * gs[1] -> grad (or null); per item m_b = scale[b], or with `part` (launch_guide_norm's)
// n_b = fp32(sqrt(sum_k part[b][k])) -> grad_norm[b] (or null) and m_b = n_b == 0 ? 0 : scale[b] / n_b; sample = fmaf(-m_b, g, sample) on
// the frames with lat == 1, every other frame keeps its bits.
int launch_guide_final(const float* dxd, const float* dx_net, const float* gs, const float* lat, int B, int T, long frame_elems,
                       const float* scale, const double* part, float* sample, float* grad, float* grad_norm, hipStream_t s);

// Probability-flow ODE likelihood (ode_nll.hip; this project's extension, Song et al. 2021).  Tensors are [B][T][frame_elems], `lat` the
// [B*T] latent mask, an item has fewer than 2^31 elements.  16-byte accesses while frame_elems % 4 == 0 and the tensors are 16-byte
// aligned, else element by element: same bits.  No floating-point atomics.
// launch_rademacher: probe number `probe` of every item: +-1.0f on the frames with lat == 1, 0 elsewhere.  Element j of item b is bit
// j & 31 of word (j >> 5) & 3 of Philox block (seed, item_offset[b] + probe * ceil(per / 128) + (j >> 7)), per = T * frame_elems; set: -1.
int launch_rademacher(float* out, const float* lat, int B, int T, long frame_elems, unsigned long long seed,
                      const unsigned long long* item_offset, unsigned long long probe, hipStream_t s);
// launch_masked_dot, two launches: per item the fp64 sum of (double)a * (double)b over the elements of its frames with lat == 1, in an
// order that depends on (T, frame_elems) alone; out[b] = ((accumulate ? out[b] : 0) + sum) / divisor.  part: [B][masked_dot_blocks(per)].
int masked_dot_blocks(long per);
int launch_masked_dot(const float* a, const float* b, const float* lat, int B, int T, long frame_elems, double* part, int accumulate,
                      double divisor, double* out, hipStream_t s);
// launch_ode_heun: on the frames with lat == 1 out = r' * (x / r + 0.5f * (sigma' - sigma) * (eps + eps2)), r = TAB_SQRT_ACP and
// sigma = TAB_SQRT_RECIPM1 at t[b] and t[b] + 1, one fp32 rounding per operation; other frames: the bits of x.  out may alias x.  A t[b]
// with no next level (t < 0 or t + 1 >= num_timesteps): NaN for item b and bit 0 of `err` (or null).
int launch_ode_heun(const float* x, const float* eps, const float* eps2, const int64_t* t, const float* tab, int num_timesteps,
                    const float* lat, int B, int T, long frame_elems, float* out, int* err, hipStream_t s);
// out = x on the frames with lat != 1; the other frames of out are not touched
int launch_keep_frames(const float* x, const float* lat, int B, int T, long frame_elems, float* out, hipStream_t s);
// out = x + (2 / 256) u on the frames with lat == 1, u = (w >> 8) 2^-24 with w word j & 3 of Philox block (seed, item_offset[b] + (j >> 2));
// other frames: the bits of x.  out may alias x.
int launch_dequantize(const float* x, const float* lat, int B, int T, long frame_elems, unsigned long long seed,
                      const unsigned long long* item_offset, float* out, hipStream_t s);
// out = in * gs[1] (launch_grad_rescale's 1 / s)
int launch_scale_by(const float* in, const float* gs, size_t n, float* out, hipStream_t s);

enum { TAB_SQRT_RECIP = 0, TAB_SQRT_RECIPM1, TAB_COEF1, TAB_COEF2, TAB_LOGVAR, TAB_ACP, TAB_ACP_PREV,
       TAB_SQRT_ACP, TAB_SQRT_1M_ACP, TAB_POST_LOGVAR, TAB_LOG_1M_ACP, TAB_ALPHA, NTAB };

// ---- Philox4x32-10 + Box-Muller: the counter-based generator every source that draws noise shares bit for bit (misc.hip, known.hip)
__device__ __forceinline__ void philox4x32_10(unsigned long long ctr, unsigned long long key, unsigned (&o)[4]) {
    unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = 0x5eed5eedu, c3 = 0;
    unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// element i -> standard normal; elements 4j..4j+3 share one Philox block
__device__ __forceinline__ float normal_at(unsigned long long seed, unsigned long long offset, unsigned long long i) {
    unsigned r[4];
    philox4x32_10(offset + (i >> 2), seed, r);
    const int pair = (int)(i & 2);
    const float u1 = ((float)r[pair] + 1.0f) * 2.3283064365386963e-10f;       // (0,1]
    const float u2 = (float)r[pair + 1] * 2.3283064365386963e-10f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    return (i & 1) ? rad * sn : rad * cs;
}

// the four normals of Philox block q: elements 4q .. 4q+3 of normal_at, bit for bit
__device__ __forceinline__ f32x4 normal4_at(unsigned long long seed, unsigned long long offset, unsigned long long q) {
    unsigned r[4];
    philox4x32_10(offset + q, seed, r);
    f32x4 z;
#pragma unroll
    for (int pair = 0; pair < 4; pair += 2) {
        const float u1 = ((float)r[pair] + 1.0f) * 2.3283064365386963e-10f;
        const float u2 = (float)r[pair + 1] * 2.3283064365386963e-10f;
        const float rad = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        z[pair] = rad * cs;
        z[pair + 1] = rad * sn;
    }
    return z;
}

// ---- backward-data pieces of `use_gradient_method` (backward.hip)
struct GnBwdArgs {
    const float* x0; const float* x1;   // the GroupNorm's input: one tensor or a virtual concat [N][HW][C0] | [N][HW][C-C0]
    int C0, C;
    const float* A; const float* B;     // the forward's folded affine [N][C]
    const float* mr;                    // [N][32][2] group mean, rstd (gn_final_affine's optional output)
    const float* dy;                    // [N][HW][C] gradient w.r.t. act(x*A + B)
    int act;                            // 1: SiLU behind the affine
    int N, HW;
    float* dx0; float* dx1;             // gradients of the two sources, each assigned (acc = 0) or accumulated (acc = 1)
    int acc0, acc1;
    const float* extra;                 // [N][HW][C] added to the result (the ResBlock's skip path), or null
    double* part;                       // [N][gn_bwd_split][C][2] workspace
    float* K;                           // [N][32][2] workspace
};
int gn_bwd_split(int nfr, int HW, int C);
int launch_gn_bwd(const GnBwdArgs& a, hipStream_t s);
int launch_gn_temporal_bwd(const float* x, const float* gamma, const float* dy, int B, int T, int HW, int C, int accumulate,
                           float* dx, hipStream_t s);
int launch_attn_temporal_bwd(const AttnTemporalArgs& a, const float* dout, float* dqkv, hipStream_t s);
size_t attn_spatial_bwd_ws_floats(const AttnSpatialArgs& a);
int launch_attn_spatial_bwd(const AttnSpatialArgs& a, const float* dout, float* dqkv, float* ws, hipStream_t s);
int launch_zero_stuff2(const float* x, int nfr, int Ho, int Wo, int C, float* y, hipStream_t s);
int launch_sumpool2(const float* x, int nfr, int Ho, int Wo, int C, int accumulate, float* y, hipStream_t s);
int launch_add(const float* x, size_t n, int accumulate, float* y, hipStream_t s);
int launch_out_conv_bwd(const float* deps, const float* w, int nfr, int H, int W, int C, int Cout, float* da, hipStream_t s);
int launch_stem_col2im(const float* dcols, const float* obs, const float* lat, const float* km, int nfr, int H, int W, int Kpad, int cond_mode,
                       float* dx, hipStream_t s);
// return_attn_weights (unet.py:457-466): softmax weights averaged over the heads, |.|; temporal [B*HW][T][T], spatial [nfr][L][L]
int launch_attn_temporal_weights(const AttnTemporalArgs& a, float* out, hipStream_t s);
int launch_attn_spatial_weights(const AttnSpatialArgs& a, float* out, hipStream_t s);
struct GuidedArgs {
    const float* x; const float* eps; const float* noise; const float* xtm1;   // [B][per]
    const float* obs;                   // [B*T] the ORIGINAL observation mask (the network saw every frame as latent)
    const int64_t* t; const float* tab; int num_timesteps;
    int B, T; long per; int clip;
    float* deps; float* dxd;            // d loss / d eps, and the direct part of d loss / d x
    float* mean; float* xstart;         // the unguided posterior mean and the x_0 prediction
    int* err = nullptr;                 // sticky error word (bit 1: eps not finite)
    const float* gscale = nullptr;      // {s, 1 / s}: the backward pass ran on s * d loss / d eps (backward.hip: launch_grad_rescale); set before launch_guided_final
};
int launch_grad_rescale(float* deps, size_t n, float* gs, hipStream_t st);
int launch_guided_grad(const GuidedArgs& a, hipStream_t s);
int launch_guided_final(const GuidedArgs& a, const float* dx_net, const float* noise2, float* grad, float* mean_out, float* sample,
                        hipStream_t s);

// _vb_terms_bpd + the two MSEs of calc_bpd_loop_subsampled's loop body (gaussian_diffusion.py:750-790, 975-990), given eps
struct VbArgs {
    const float* x_start; const float* x_t; const float* eps;
    const float* noise;          // for mse = mean((eps_from_xstart - noise)^2); null: not computed
    const int64_t* t;            // [B]
    const float* tab; int num_timesteps;
    const float* mask;           // [B*T] latent_mask or null (mean_flat(..., mask): multiply, then mean over ALL elements)
    int B, T; long per;          // per = T*3*H*W
    int clip;
    float* pred_xstart;          // optional output
    double* part;                // [B][nblk][3] partial sums
    int nblk;
    float* vb; float* xstart_mse; float* mse;      // [B] outputs (the last two may be null)
    int* err = nullptr;          // sticky error word (bit 1: eps not finite)
    int start_x = 0;             // ModelMeanType.START_X (predict_xstart=True): `eps` holds the network's x_0 prediction itself
};
int launch_vb_terms(const VbArgs& a, hipStream_t s);
int vb_terms_blocks(long per);
// The observed-frame search's score (scripts/video_optimal_schedule.py:142-206): mean((eps_from_xstart - noise)^2) over the latent
// frames of each item, noise = the item's own Philox stream (seed, item_offset[b]) unless given; misc.hip
struct ScoreArgs {
    const float* x_start;        // [B][per]
    const float* eps;            // the network output at x_t (launch_score_q_sample does not read it)
    const float* noise;          // explicit draws or null
    const int64_t* t;            // [B]
    const float* tab; int num_timesteps;
    const float* mask;           // [B*T] latent_mask
    int B, T; long per;          // per = T*3*H*W
    int clip, start_x;
    unsigned long long seed; const unsigned long long* item_offset;   // [B] Philox block offsets (device)
    double* part; int nblk;      // [B][nblk] partial sums
    int* err;                    // sticky error word
};
int launch_score_q_sample(const ScoreArgs& a, float* x_t, hipStream_t s);
int launch_eps_mse(const ScoreArgs& a, double* mse_out, hipStream_t s);
// _prior_bpd (gaussian_diffusion.py:909-926): KL(q(x_T | x_0) || N(0, I)) in bits per dim, masked mean
int launch_prior_bpd(const float* x_start, const float* mask, const float* tab, int num_timesteps, int B, int T, long per,
                     double* part, int nblk, float* out, hipStream_t s);

// x * sigmoid(x) with v_exp_f32 + v_rcp_f32 (each <= 1 ulp): 5 VALU instructions instead of the ~15 of an IEEE
// division.  The operand transform of the conv kernels runs this on every staged input element.
__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

}  // namespace vd
