// Zero-shot restoration (this project's extension; DDNM, Wang, Yu, Zhang 2022): the range/null-space projection of a step's x_0
// prediction onto a measurement y = A x, x_0 <- x_0 + A^+(y - A x_0), for the "cell mean" operators: A is the mean over every s x s
// pixel cell of one channel plane (gray: of all three planes), A^+ replicates a cell's value over the cell.  One streaming pass over
// [B][T][3][H][W]: every input element is read once, held in registers across the cell's reduction, and written once.
#include "vd_common.h"
#include <algorithm>

namespace vd {

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the value of lane (id ^ M) of the wave, M in {1, 2, 4, 8}: within a quad a DPP quad_perm (no LDS hardware at all), across quads of a
// row of 16 the ds_swizzle crossbar in its bit-mask mode (and 0x1f, or 0, xor M) -- neither needs an address register as ds_bpermute does
template <int M>
__device__ __forceinline__ float lane_xor(float v) {
    int i = __float_as_int(v);
    if constexpr (M == 1) i = __builtin_amdgcn_update_dpp(0, i, 0xB1, 0xF, 0xF, true);           // quad_perm:[1,0,3,2]
    else if constexpr (M == 2) i = __builtin_amdgcn_update_dpp(0, i, 0x4E, 0xF, 0xF, true);      // quad_perm:[2,3,0,1]
    else i = __builtin_amdgcn_ds_swizzle(i, (M << 10) | 0x1F);
    return __int_as_float(i);
}

// ------------------------------------------------------------------ measurement_project_kernel
// Thread -> cell map.  A thread owns one row segment per channel it serves (one channel; gray: the three of its frame).  A segment of
// a cell's row is SEG = min(S, 4) elements wide.  VEC: a thread's segment is four consecutive elements, one 16-byte access, holding
// NC = 4 / SEG cells' segments side by side (S = 1: four cells, S = 2: two, S >= 4: one); scalar form: one cell's segment, element by
// element.  The L = S * max(S / 4, 1) threads that cover one cell (S rows, S = 8: two segments across) are L consecutive lanes of one
// wave (L is 1, 2, 4 or 16 and divides 64), so the cell's sum is an xor butterfly over L lanes (lane_xor) -- no LDS memory, no atomics.
// Summation order of a cell, the same in both forms and whatever B is: a segment left to right; the channels' segment sums in channel
// order; then the butterfly at lane distance 1, 2, 4, 8.  a + b = b + a bit for bit, so the L lanes end with the same sum.
// A cell that holds a value that is not finite comes out not finite in every element: x + (y - mean) with mean Inf or NaN.
template <int S, bool GRAY, bool VEC>
__global__ __launch_bounds__(256) void measurement_project_kernel(MeasureArgs a) {
    constexpr int SEG = S < 4 ? S : 4, NC = VEC ? 4 / SEG : 1, E = SEG * NC, HX = S > 4 ? S / 4 : 1, L = S * HX, CH = GRAY ? 3 : 1;
    constexpr int UW = HX * E;                       // columns one lane group covers
    // blockIdx.y walks the planes (gray: the frames), blockIdx.x and the thread the lanes of one plane: every index below the plane's
    // base fits 32 bits (a plane holds fewer than 2^31 elements; launch_measurement_project checks), so no 64-bit division runs here
    const size_t hw = (size_t)a.H * a.W;
    const unsigned ux = (unsigned)a.W / UW, uy = (unsigned)a.H / S, ws = (unsigned)a.W / S;
    const unsigned planes = (unsigned)a.B * a.T * (GRAY ? 1 : 3);
    const unsigned lanes = uy * ux * L;              // a multiple of L, as the stride is: a lane group leaves the loop together
    const bool given = a.x == nullptr;
    const int NT = a.num_timesteps;
    const float n = (float)(S * S * CH);
    for (unsigned plane = blockIdx.y; plane < planes; plane += gridDim.y)
    for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < lanes; g += gridDim.x * 256) {
        const unsigned l = g % L, u = g / L, cx = u % ux, cy = u / ux;
        const size_t frame = GRAY ? plane : plane / 3, c0 = GRAY ? 0 : plane % 3;
        const unsigned row = cy * S + l / HX, col = cx * UW + (l % HX) * E;
        float sr = 0.f, srm1 = 0.f;
        if (!given) {
            const long long t = a.t[(unsigned)frame / (unsigned)a.T];
            if (t < 0 || t >= NT) continue;          // the sampler pass poisons the item and sets the error bit: nothing is read of `out`
            sr = a.tab[TAB_SQRT_RECIP * NT + t]; srm1 = a.tab[TAB_SQRT_RECIPM1 * NT + t];
        }
        float v[CH][E];
        bool nonfinite = false;                      // the sampler pass behind this one reads the same values and raises the bit
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const size_t i = (frame * 3 + c0 + c) * hw + row * (unsigned)a.W + col;
            float s[E], x[E];
            if (VEC) {
                *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(a.src + i);
                if (!given) *reinterpret_cast<float4*>(x) = *reinterpret_cast<const float4*>(a.x + i);
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) { s[e] = a.src[i + e]; if (!given) x[e] = a.x[i + e]; }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) v[c][e] = pass_x0(given ? 0.f : x[e], s[e], given, sr, srm1, a.clip, nonfinite);
        }
        const bool latent = a.lat[frame] == 1.0f;
        if (latent) {
            float p[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) {
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    float q = v[c][k * SEG];
#pragma unroll
                    for (int j = 1; j < SEG; ++j) q += v[c][k * SEG + j];
                    p[k] = c == 0 ? q : p[k] + q;
                }
                if constexpr (L >= 2) p[k] += lane_xor<1>(p[k]);
                if constexpr (L >= 4) p[k] += lane_xor<2>(p[k]);
                if constexpr (L >= 16) { p[k] += lane_xor<4>(p[k]); p[k] += lane_xor<8>(p[k]); }
                const float mean = p[k] / n;
                const float d = a.y[((frame * (GRAY ? 1 : 3) + c0) * uy + cy) * ws + col / S + k] - mean;
#pragma unroll
                for (int c = 0; c < CH; ++c)
#pragma unroll
                    for (int j = 0; j < SEG; ++j) v[c][k * SEG + j] += d;
            }
        } else if (given && a.out == a.src && !a.clip) continue;      // in place and nothing to do: the frame keeps its bits
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const size_t i = (frame * 3 + c0 + c) * hw + row * (unsigned)a.W + col;
            if (VEC) *reinterpret_cast<float4*>(a.out + i) = *reinterpret_cast<const float4*>(v[c]);
            else {
#pragma unroll
                for (int e = 0; e < E; ++e) a.out[i + e] = v[c][e];
            }
        }
    }
}

template <int S, bool GRAY>
static void launch_form(const MeasureArgs& a, bool vec, hipStream_t s) {
    constexpr int SEG = S < 4 ? S : 4, HX = S > 4 ? S / 4 : 1, L = S * HX;
    const size_t uw = (size_t)HX * (vec ? 4 : SEG);
    const size_t lanes = (size_t)(a.H / S) * (a.W / uw) * L, planes = (size_t)a.B * a.T * (GRAY ? 1 : 3);
    // about 4096 blocks in all, as the other streaming passes: the planes along y, a plane's lanes along x
    const unsigned gy = (unsigned)std::min<size_t>(planes, 4096);
    const unsigned gx = (unsigned)std::min<size_t>((lanes + 255) / 256, std::max<size_t>(4096 / gy, 1));
    const dim3 grid(gx, gy);
    if (vec) hipLaunchKernelGGL((measurement_project_kernel<S, GRAY, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((measurement_project_kernel<S, GRAY, false>), grid, dim3(256), 0, s, a);
}

int launch_measurement_project(const MeasureArgs& a, hipStream_t s) {
    VD_REQUIRE(a.src && a.out && a.y && a.lat, "measurement_project_kernel: null tensor");
    VD_REQUIRE(!a.x || (a.t && a.tab && a.num_timesteps > 0), "measurement_project_kernel: x_t without t and the tables");
    VD_REQUIRE(a.B > 0 && a.T > 0 && a.H > 0 && a.W > 0, "measurement_project_kernel: shape");
    VD_REQUIRE((size_t)a.H * a.W < ((size_t)1 << 31) && (size_t)a.B * a.T * 3 < ((size_t)1 << 31), "measurement_project_kernel: a plane of fewer than 2^31 elements, fewer than 2^31 planes");
    VD_REQUIRE(measurement_served(a.scale, a.gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
    VD_REQUIRE(a.H % a.scale == 0 && a.W % a.scale == 0, "measurement: H and W must be divisible by scale");
    const bool vec = a.W % 4 == 0 && al16(a.x) && al16(a.src) && al16(a.out);
    const int key = a.scale * 2 + (a.gray ? 1 : 0);
    switch (key) {
        case 3: launch_form<1, true>(a, vec, s); break;
        case 4: launch_form<2, false>(a, vec, s); break;
        case 5: launch_form<2, true>(a, vec, s); break;
        case 8: launch_form<4, false>(a, vec, s); break;
        case 9: launch_form<4, true>(a, vec, s); break;
        case 16: launch_form<8, false>(a, vec, s); break;
        default: launch_form<8, true>(a, vec, s); break;
    }
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
