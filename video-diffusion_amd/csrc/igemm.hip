// Implicit-GEMM convolution / linear layer on fp32 MFMA (v_mfma_f32_32x32x2_f32), gfx950.
//
// One kernel covers every dense contraction of the denoise step:
//   conv3x3 s1/s2 (+fused nearest-x2 upsample, + virtual channel concat), conv1x1, nn.Linear.
// out[m][co] = bias[co] + res[m][co] + sum_{tap,ci} f(in[pixel(m)+tap][ci]) * w[tap][co][ci]
// with f(v) = silu(v*A[n][ci] + B[n][ci]) -- GroupNorm (+FiLM scale/shift) and SiLU of the *producer*
// folded into this kernel's operand load, so normalised activations are never materialised
// (ResBlock: unet.py:185-198).
//
// The tiling and the K loop are those of igemm_tile.h: K-step = (tap, 32 input channels), A tile [BM][32] gathered per tap
// from NHWC, B tile [BN][32] from weights stored [tap][Cout][Cin].
#include <algorithm>

#include <string>

#include "igemm_tile.h"
#include "vd_common.h"

namespace vd {

constexpr int BK = IG_BK;
constexpr int LDP = IG_LDP;

template <int BM, int BN>
__global__ __launch_bounds__(256) void igemm_kernel(IgemmArgs a) {
    constexpr int MI = BM / 64, NI = BN / 64;     // 32x32 tiles per wave in M / N
    constexpr int AR = BM / 32, BR = BN / 32;     // loader rows per thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                     // [2][BM][LDP]
    float* Bs = smem + 2 * BM * LDP;      // [2][BN][LDP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // ---- loader geometry: thread -> (row lrow + 32j, 4-float quad lq of the 32-channel chunk)
    const int lrow = tid >> 3, lq = tid & 7;
    const int HWo = a.Ho * a.Wo;
    const int Hl = a.Hs << a.ups, Wl = a.Ws << a.ups;
    int pn[AR], py[AR], px[AR];
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        int m = m0 + lrow + 32 * j;
        if (m < a.M) {
            int n = m / HWo, r = m - n * HWo;
            int oy = r / a.Wo;
            pn[j] = n; py[j] = oy * a.stride - a.pad; px[j] = (r - oy * a.Wo) * a.stride - a.pad;
        } else {
            pn[j] = -1; py[j] = 0; px[j] = 0;
        }
    }
    const int ntaps = a.ksz * a.ksz;
    const int nchunk = a.Cin / BK;
    const int nsteps = ntaps * nchunk;
    const int C1 = a.Cin - a.C0;
    unsigned avalid = 0;

    auto load = [&](int s, f32x4 (&ra)[AR], f32x4 (&rb)[BR]) {
        const int chunk = s / ntaps, tap = s - chunk * ntaps;
        const int kh = tap / a.ksz, kw = tap - kh * a.ksz;
        const int c = chunk * BK + lq * 4;
        const float* base; int cc, ld;
        if (c < a.C0) { base = a.src0; cc = c; ld = a.C0; } else { base = a.src1; cc = c - a.C0; ld = C1; }
        avalid = 0;
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            int iy = py[j] + kh, ix = px[j] + kw;
            const bool ok = pn[j] >= 0 && iy >= 0 && iy < Hl && ix >= 0 && ix < Wl;
            const size_t pix = ok ? ((size_t)pn[j] * a.Hs + (iy >> a.ups)) * a.Ws + (ix >> a.ups) : 0;   // out-of-image taps read pixel 0
            ra[j] = *reinterpret_cast<const f32x4*>(base + pix * ld + cc);
            avalid |= (ok ? 1u : 0u) << j;
        }
        const float* wt = a.w + ((size_t)tap * a.Cout) * a.Cin + c;
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const int co = min(n0 + lrow + 32 * j, a.Cout - 1);       // rows past Cout: duplicates, masked at the store
            rb[j] = *reinterpret_cast<const f32x4*>(wt + (size_t)co * a.Cin);
        }
    };
    auto fix = [&](int s, int j, f32x4 v) {
        const int c = s / ntaps * BK + lq * 4;
        if (a.affA) {
            const size_t fr = (size_t)max(pn[j], 0) * a.Cin + c;
            const f32x4 sa = *reinterpret_cast<const f32x4*>(a.affA + fr);
            const f32x4 sb = *reinterpret_cast<const f32x4*>(a.affB + fr);
            v = v * sa + sb;
        }
        if (a.act) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
        if (!(avalid & (1u << j))) v = f32x4{0.f, 0.f, 0.f, 0.f};   // zero padding AFTER norm+activation (conv pads its input)
        return v;
    };

    f32x16 acc[MI][NI];
    igemm_tile_loop<BM, BN>(As, Bs, nsteps, load, fix, acc);

    // ---- epilogue
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int co = n0 + wn * (BN / 2) + j * 32 + lr;
        if (co >= a.Cout) continue;
        const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            // residual loads batched ahead of the stores (unconditional, row clamped): one wait per tile
            // instead of one drained L2 round trip per element
            const int mb = m0 + wm * (BM / 2) + i * 32 + igemm_cd_row(0, lane);
            f32x16 v = acc[i][j];
            if (a.res) {
                f32x16 rv;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    rv[r] = a.res[(size_t)min(mb + igemm_cd_row(r, 0), a.M - 1) * a.res_ld + co];
                v += rv;
            }
            if (a.fbias) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    v[r] += a.fbias[(size_t)(min(mb + igemm_cd_row(r, 0), a.M - 1) / HWo) * a.fbias_ld + co];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mb + igemm_cd_row(r, 0);
                if (m < a.M) a.out[(size_t)m * a.ldo + co] = v[r] + bv;
            }
        }
    }
}

template <int BM, int BN>
static int launch_t(const IgemmArgs& a, hipStream_t s) {
    const size_t lds = 2 * (BM + BN) * LDP * sizeof(float);
    VD_RAISE_LDS((&igemm_kernel<BM, BN>), lds);
    dim3 grid((a.M + BM - 1) / BM, (a.Cout + BN - 1) / BN);
    hipLaunchKernelGGL((igemm_kernel<BM, BN>), grid, dim3(256), lds, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

// The ONE place that decides which kernel serves an IgemmArgs (the engine's profiler classes and its planning read the same answer)
IgemmKernel igemm_kernel(const IgemmArgs& a) {
    if (a.ups_phase) return IK_R64_UPS;                                 // sub-pixel weight image: only conv_wino_r64.hip reads it
    if (gemm_split_supported(a) || conv_split_supported(a)) return IK_SPLIT;
    if (conv_wino_z128_act_supported(a) || conv_wino_z128_supported(a)) return IK_Z128;
    if (conv_wino_r64_supported(a)) return IK_R64;
    if (gemm_frag_supported(a)) return IK_FRAG;
    if (conv_wino_supported(a)) return IK_WINO;
    return IK_GENERIC;
}

// ---- the generic kernel's instantiations: ONE table, read by the launcher and by igemm_variant() (vd_igemm_variant)
struct IgemmRow {
    int cls;                         // igemm_tile_class
    const char* name;
    int (*launch)(const IgemmArgs&, hipStream_t);
};
static const IgemmRow kIgemmRows[] = {{0, "igemm_kernel<128,128>", launch_t<128, 128>}, {1, "igemm_kernel<128,64>", launch_t<128, 64>},
                                      {2, "igemm_kernel<64,128>", launch_t<64, 128>}, {3, "igemm_kernel<64,64>", launch_t<64, 64>}};

static const IgemmRow* igemm_row(const IgemmArgs& a, int tile, const char** why) {
    if (a.wsplit) { *why = "split weight image given for a shape the split kernels do not cover"; return nullptr; }
    if (a.w == nullptr) { *why = "this shape runs on the generic kernel and needs [tap][Cout][Cin] weights"; return nullptr; }
    const int cls = tile >= 0 && tile <= 2 ? tile : 3;
    for (const IgemmRow& r : kIgemmRows)
        if (r.cls == cls) return &r;
    *why = "igemm.hip: no instantiation";
    return nullptr;
}

// what launch_igemm asks of a call before it looks at the kernels: null, or the requirement that failed
static const char* igemm_refusal(const IgemmArgs& a) {
    if (a.Cin % BK != 0) return "Cin must be a multiple of 32 (pad the operand)";
    if (!(a.C0 % BK == 0 && a.C0 <= a.Cin)) return "concat split must be a multiple of 32";
    if (!(a.src1 != nullptr || a.C0 == a.Cin)) return "second source missing";
    if (!(a.ksz == 1 || a.ksz == 3)) return "kernel size 1 or 3";
    if (!(a.M > 0 && a.Cout > 0)) return "empty problem";
    if (a.M != a.nfr * a.Ho * a.Wo) return "M != nfr*Ho*Wo";
    if (igemm_frames_per_launch(a) <= 0) return "one frame of this layer exceeds 2^28 elements";
    return nullptr;
}

// ONE launch's args (every operand small enough for the 32-bit byte offsets the kernels address with) -> igemm_kernel()'s choice, then the
// row of that file's table: named into *v (vd_igemm_variant: no launch), or launched when v is null.  One switch serves both.
static int igemm_one(const IgemmArgs& a, hipStream_t s, IgemmVariant* v) {
    const int tile = igemm_tile_class(igemm_sel_M(a), a.Cout);
    const char* why = nullptr;
    switch (igemm_kernel(a)) {
        case IK_R64_UPS:
            if (!conv_wino_r64_supported(a)) { why = "sub-pixel Upsample conv: shape not covered by conv_wino_r64.hip"; break; }
            return v ? (*v = conv_wino_r64_variant(a), 0) : launch_conv_wino_r64(a, s);
        case IK_SPLIT: return v ? (*v = gemm_split_variant(a, tile), 0) : launch_gemm_split(a, tile, s);
        case IK_Z128: return v ? (*v = conv_wino_z128_variant(a), 0) : launch_conv_wino_z128(a, s);
        case IK_R64: return v ? (*v = conv_wino_r64_variant(a), 0) : launch_conv_wino_r64(a, s);
        case IK_FRAG: return v ? (*v = gemm_frag_variant(a, tile), 0) : launch_gemm_frag(a, tile, s);
        case IK_WINO: return v ? (*v = conv_wino_variant(a), 0) : launch_conv_wino(a, s);
        case IK_GENERIC:
            if (const IgemmRow* r = igemm_row(a, tile, &why)) return v ? (*v = IgemmVariant{r->name, 1, nullptr}, 0) : r->launch(a, s);
            break;
    }
    if (v) { *v = IgemmVariant{nullptr, 1, why}; return 0; }
    VD_REQUIRE(false, why);
}

IgemmVariant igemm_variant(const IgemmArgs& a) {
    if (const char* why = igemm_refusal(a)) return IgemmVariant{nullptr, 1, why};
    IgemmVariant v{nullptr, 1, nullptr};
    (void)igemm_one(igemm_first_launch(a), nullptr, &v);
    return v;
}

std::string igemm_variant_name(const IgemmVariant& v) {
    if (!v.name) return std::string("refused: ") + (v.why ? v.why : "");
    return v.ksplit > 1 ? std::string(v.name) + "+ksplit" + std::to_string(v.ksplit) : std::string(v.name);
}

void igemm_variant_names(std::vector<std::string>& out) {
    gemm_split_variant_names(out);
    conv_wino_r64_variant_names(out);
    conv_wino_z128_variant_names(out);
    gemm_frag_variant_names(out);
    conv_wino_variant_names(out);
    for (const IgemmRow& r : kIgemmRows) out.push_back(r.name);
}

// Frames (rows, for a linear layer) per launch.  The fast kernels reach their operands through buffer descriptors with
// 32-bit byte offsets and bound each operand to 2^28 elements (*_supported); a window that is merely BIG -- 160 frames of
// 128x128x128 channels, BASELINE configs[4] -- is cut along the frame dimension into equal launches with the base
// pointers advanced.  Frames are independent in every one of these kernels (per-frame affine / bias / statistics rows
// move with them), so the results are those of one launch, bit for bit.
int igemm_frames_per_launch(const IgemmArgs& a) {
    const size_t lim = ((size_t)1 << 28) - 1;
    const size_t in_pf = (size_t)a.Hs * a.Ws * std::max(a.C0, a.Cin - a.C0);
    const size_t out_pf = (size_t)a.Ho * a.Wo * std::max(a.ldo, a.res ? a.res_ld : 0);
    const size_t pf = std::max(in_pf, out_pf);
    if (pf == 0 || (size_t)a.nfr * pf <= lim || a.zcount > 1) return a.nfr;
    const size_t align = (a.Hs == 1 && a.Ws == 1) ? 256 : 4;       // whole 128-row tiles / whole 4-frame groups (conv_wino_r64 TF4)
    size_t maxfr = lim / pf / align * align;
    if (maxfr == 0) return 0;
    const size_t nl = ((size_t)a.nfr + maxfr - 1) / maxfr;
    size_t per = ((size_t)a.nfr + nl - 1) / nl;                       // equal launches
    per = (per + align - 1) / align * align;
    return (int)std::min(per, maxfr);
}

// The launch of frames [f0, f0 + n) of a call that is cut along the frame dimension: base pointers advanced, kernel variants still
// chosen for the whole call (nfr_sel)
static IgemmArgs frame_range(const IgemmArgs& a, int f0, int n) {
    const size_t HWi = (size_t)a.Hs * a.Ws, HWo = (size_t)a.Ho * a.Wo;
    IgemmArgs b = a;
    b.nfr = n;
    b.nfr_sel = a.nfr_sel ? a.nfr_sel : a.nfr;
    b.M = b.nfr * a.Ho * a.Wo;
    b.src0 = a.src0 + (size_t)f0 * HWi * a.C0;
    if (a.src1) b.src1 = a.src1 + (size_t)f0 * HWi * (a.Cin - a.C0);
    if (a.res) b.res = a.res + (size_t)f0 * HWo * a.res_ld;
    b.out = a.out + (size_t)f0 * HWo * a.ldo;
    if (a.affA) { b.affA = a.affA + (size_t)f0 * a.Cin; b.affB = a.affB + (size_t)f0 * a.Cin; }
    if (a.fbias) b.fbias = a.fbias + (size_t)f0 * a.fbias_ld;
    if (a.stats) b.stats = a.stats + (size_t)f0 * a.stats_split * a.Cout * 2;
    if (a.side) { b.side = a.side + (size_t)f0 * HWo * a.Cin; b.sideA = a.sideA + (size_t)f0 * a.Cin; b.sideB = a.sideB + (size_t)f0 * a.Cin; }
    return b;
}

IgemmArgs igemm_first_launch(const IgemmArgs& a) {
    const int per = igemm_frames_per_launch(a);
    return per > 0 && per < a.nfr ? frame_range(a, 0, per) : a;
}

int launch_igemm(const IgemmArgs& a, hipStream_t s) {
    if (const char* why = igemm_refusal(a)) { set_error(std::string("requirement failed: ") + why); return -1; }
    const int per = igemm_frames_per_launch(a);
    if (per >= a.nfr) return igemm_one(a, s, nullptr);
    VD_REQUIRE(!(a.stats && a.stats_hw > 0), "GroupNorm partial sums from the split GEMM: one launch only (the tile choice, and with it the table, depends on M)");
    for (int f0 = 0; f0 < a.nfr; f0 += per) {
        const int rc = igemm_one(frame_range(a, f0, std::min(per, a.nfr - f0)), s, nullptr);
        if (rc) return rc;
    }
    return 0;
}

// Tile choice: big tiles when the grid still fills 256 CUs x 2 blocks, smaller ones otherwise.
// 0: 128x128, 1: 128x64, 2: 64x128, 3: 64x64
int igemm_tile_class(int M, int Cout) {
    const long t128 = (long)((M + 127) / 128) * ((Cout + 127) / 128);
    if (Cout <= 64) return M >= 128 * 512 ? 1 : 3;
    if (t128 >= 512) return 0;
    const long t64n = (long)((M + 63) / 64) * ((Cout + 127) / 128);
    if (t64n >= 384) return 2;
    return 3;
}

}  // namespace vd
