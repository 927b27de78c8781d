// Channels-last convolution, max pool and weight pack of the two feature networks (lpips.hip: AlexNet, 2-D, the frames on the T
// axis with kt = 1; i3d.hip: Inception-v1 inflated to 3-D), gfx950.
//
// The convolution is an implicit GEMM on the fp32 MFMA (igemm_tile.h: 64 x 64 block tile), fp32 operands and accumulation whatever
// VD_MATH says.  Reduction index k = ((dt*kh + dy)*kw + dx)*Cin + ci, weights packed [Cout][Kpad] once at load; pads and output
// sizes are the caller's (I3D: TF's SAME, LPIPS: AlexNet's).  The output is written with a row stride, so the branches of a Mixed
// block land in their channel slices of one tensor.  No split of the reduction and no atomics: every sum has a fixed order.
#include "igemm_tile.h"
#include "vd_common.h"

namespace vd {
namespace {

constexpr int CL_BM = 64, CL_BN = 64;

template <int G>
__global__ __launch_bounds__(256) void conv_cl_kernel(ConvClArgs a) {
    constexpr int AR = CL_BM / 32, BR = CL_BN / 32;
    __shared__ __attribute__((aligned(16))) float As[2 * CL_BM * IG_LDP];
    __shared__ __attribute__((aligned(16))) float Bs[2 * CL_BN * IG_LDP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * CL_BM, n0 = blockIdx.y * CL_BN;
    const int lrow = tid >> 3, lq = tid & 7;
    const int HWo = a.Ho * a.Wo;

    int pz[AR], py[AR], px[AR];
    bool pv[AR];
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        const int m = m0 + lrow + 32 * j;
        pv[j] = m < a.M;
        const int mm = pv[j] ? m : 0;
        const int ot = mm / HWo, r = mm - ot * HWo, oy = r / a.Wo;
        pz[j] = ot * a.st - a.pt; py[j] = oy * a.sh - a.ph; px[j] = (r - oy * a.Wo) * a.sw - a.pw;
    }

    // k -> (dt, dy, dx, c) and the source element of row j, or -1 for padding / a row or k beyond the problem
    auto locate = [&](int k, int j, int& c) -> long long {
        const int cin = G == CG_NCHW_SCALED ? 3 : a.Cin;
        const int tap = k / cin;
        c = k - tap * cin;
        const int q = tap / a.kw, dx = tap - q * a.kw;
        const int dt = q / a.kh, dy = q - dt * a.kh;
        const int it = pz[j] + dt, iy = py[j] + dy, ix = px[j] + dx;
        const bool ok = pv[j] && k < a.Kreal && it >= 0 && it < a.T && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        if (G == CG_NCHW_SCALED) return ok ? (long long)((((size_t)it * 3 + c) * a.H + iy) * a.W + ix) : -1;
        return ok ? (long long)((((size_t)it * a.H + iy) * a.W + ix) * a.Cin + c) : -1;
    };
    auto load = [&](int s, f32x4 (&ra)[AR], f32x4 (&rb)[BR]) {
        const int k0 = s * IG_BK + lq * 4;
        int c;
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            if constexpr (G == CG_QUAD) {
                const long long off = locate(k0, j, c);              // Cin % 4 == 0: four consecutive k share a tap
                const f32x4 v = *reinterpret_cast<const f32x4*>(a.src + (off < 0 ? 0 : off));
                ra[j] = off < 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long off = locate(k0 + e, j, c);
                    float v = a.src[off < 0 ? 0 : off];
                    if constexpr (G == CG_NCHW_SCALED) {
                        const float sh = c == 0 ? a.shift[0] : (c == 1 ? a.shift[1] : a.shift[2]);
                        const float sc = c == 0 ? a.scale[0] : (c == 1 ? a.scale[1] : a.scale[2]);
                        v = (v - sh) / sc;
                    }
                    ra[j][e] = off < 0 ? 0.f : v;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const int co = min(n0 + lrow + 32 * j, a.Cout - 1);       // rows past Cout: duplicates, masked at the store
            rb[j] = *reinterpret_cast<const f32x4*>(a.w + (size_t)co * a.K + k0);
        }
    };

    f32x16 acc[1][1];
    igemm_tile_loop<CL_BM, CL_BN>(As, Bs, a.K / IG_BK, load, [](int, int, f32x4 v) { return v; }, acc);

    const int co = n0 + wn * 32 + (lane & 31);
    if (co >= a.Cout) return;
    const float bv = a.bias ? a.bias[co] : 0.f;
    const int mb = m0 + wm * 32 + igemm_cd_row(0, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mb + igemm_cd_row(r, 0);
        const float v = acc[0][0][r] + bv;
        if (m < a.M) a.out[(size_t)m * a.out_stride + co] = a.relu ? fmaxf(v, 0.f) : v;
    }
}

__global__ __launch_bounds__(256) void conv_cl_pack_kernel(const float* w, float* packed, int Cout, int Cin, int taps, int K) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)Cout * K) return;
    const int o = (int)(i / K), k = (int)(i - (long long)o * K);
    const int tap = k / Cin, c = k - tap * Cin;
    packed[i] = tap < taps ? w[((size_t)o * Cin + c) * taps + tap] : 0.f;
}

// one thread per (output position, 4 channels)
__global__ __launch_bounds__(256) void maxpool_cl_kernel(PoolClArgs a) {
    const int C4 = a.C / 4;
    const long long total = (long long)a.To * a.Ho * a.Wo * C4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const long long p = i / C4;
    const int ox = (int)(p % a.Wo), oy = (int)((p / a.Wo) % a.Ho), ot = (int)(p / ((long long)a.Wo * a.Ho));
    const float ninf = -__builtin_inff();
    f32x4 m = {ninf, ninf, ninf, ninf};
    for (int dt = 0; dt < a.kt; ++dt) {
        const int it = ot * a.st - a.pt + dt;
        if (it < 0 || it >= a.T) continue;
        for (int dy = 0; dy < a.kh; ++dy) {
            const int iy = oy * a.sh - a.ph + dy;
            if (iy < 0 || iy >= a.H) continue;
            for (int dx = 0; dx < a.kw; ++dx) {
                const int ix = ox * a.sw - a.pw + dx;
                if (ix < 0 || ix >= a.W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(a.src + (((size_t)it * a.H + iy) * a.W + ix) * a.C + c4 * 4);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
    }
    *reinterpret_cast<f32x4*>(a.dst + (size_t)p * a.C + c4 * 4) = m;
}

}  // namespace

int launch_conv_cl(ConvClArgs a, ConvClGather g, hipStream_t s) {
    const long long M = (long long)a.To * a.Ho * a.Wo;
    VD_REQUIRE(M > 0 && M < (1ll << 31) - CL_BM, "conv: output positions beyond the 32-bit row index");
    VD_REQUIRE(g != CG_QUAD || a.Cin % 4 == 0, "conv: the four-channel gather needs Cin % 4 == 0");
    VD_REQUIRE(g != CG_NCHW_SCALED || a.Cin == 3, "conv: the scaling layer has 3 channels");
    a.M = (int)M;
    a.Kreal = a.Cin * a.kt * a.kh * a.kw;
    a.K = conv_cl_kpad(a.Kreal);
    const dim3 grid((a.M + CL_BM - 1) / CL_BM, (a.Cout + CL_BN - 1) / CL_BN);
    if (g == CG_QUAD) hipLaunchKernelGGL(conv_cl_kernel<CG_QUAD>, grid, dim3(256), 0, s, a);
    else if (g == CG_ELEM) hipLaunchKernelGGL(conv_cl_kernel<CG_ELEM>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_cl_kernel<CG_NCHW_SCALED>, grid, dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

int launch_conv_cl_pack(const float* w, float* packed, int Cout, int Cin, int taps, hipStream_t s) {
    const int K = conv_cl_kpad(Cin * taps);
    const long long n = (long long)Cout * K;
    hipLaunchKernelGGL(conv_cl_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, packed, Cout, Cin, taps, K);
    VD_HIP(hipGetLastError());
    return 0;
}

int conv_cl_load_weight(float** packed, const float* host, int Cout, int Cin, int taps) {
    const size_t nf = (size_t)Cout * Cin * taps;
    float* raw = nullptr;
    int rc = upload_f32(&raw, host, nf);
    if (!rc && !*packed && hipMalloc(reinterpret_cast<void**>(packed), (size_t)Cout * conv_cl_kpad(Cin * taps) * sizeof(float)) != hipSuccess) {
        set_error("hipMalloc of a packed conv weight"); rc = -2;
    }
    if (!rc) rc = launch_conv_cl_pack(raw, *packed, Cout, Cin, taps, nullptr);
    if (!rc && hipDeviceSynchronize() != hipSuccess) { set_error("packing a conv weight"); rc = -2; }
    (void)hipFree(raw);
    return rc;
}

int launch_maxpool_cl(const PoolClArgs& a, hipStream_t s) {
    const long long total = (long long)a.To * a.Ho * a.Wo * (a.C / 4);
    VD_REQUIRE(total > 0 && (total + 255) / 256 < (1ll << 31), "maxpool: grid too large");
    hipLaunchKernelGGL(maxpool_cl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
