// Separable linear measurements (this project's extension): the operator of the exact projection (DDNM), of DPS and of particle steering's
// built-in reward for a measurement that acts on every channel plane of every frame as Y = A_h X A_w^T, with two small dense matrices
// A_h (Mh x H) and A_w (Mw x W), 1 <= Mh <= H <= 128, 1 <= Mw <= W <= 128: bicubic and bilinear down-sampling, any separable blur with any
// padding and stride, the cell mean.  The adjoint is A_h^T R A_w, the back-projection P_h R P_w^T with P_h (H x Mh), P_w (W x Mw) -- the
// (truncated) pseudo-inverses, formed on the host.  All three are ONE two-sided product, Z = L X R^T with L (P x Q), X (Q x U), R (S x U),
// the right factor first:
//   tmp[q][s] = sum_u X[q][u] R[s][u]      acc = 0, then u = 0 .. U-1 ascending, acc = acc + X[q][u] * R[s][u]
//   Z[p][s]   = sum_q L[p][q] tmp[q][s]    acc = 0, then q = 0 .. Q-1 ascending, acc = acc + L[p][q] * tmp[q][s]
// -- the product rounded to fp32, then the sum rounded to fp32, never a fused multiply-add (contraction is off), tmp an fp32 value.
// Forward: L = A_h, R = A_w; adjoint: L = A_h^T, R = A_w^T; back-projection: L = P_h, R = P_w.  tests/linop_restated.py restates it.
//   linop_apply_kernel     Z = L X R^T of `planes` planes;
//   linop_residual_kernel  x_0 through pass_x0, as every sampler pass forms it (written out for every frame when asked), r = y - A x_0 per
//                          element of the latent frames and one fp64 partial of sum r^2 per block;
//   linop_project_kernel   x_0 <- x_0 + P_h r P_w^T on the latent frames, in place; other frames keep their bits;
//   linop_seed_kernel      rho_b from the item's partials and the two seeds of the backward pass: q = -(A_h^T r A_w) / rho_b through the
//                          clamp, d eps = -b q_r and the direct part d_x = a q_r (blur_seed_kernel's, for this operator).
// A block works on one plane and kChunk of its output columns s: the plane operand X lies in LDS (rows of U | 1 floats: the lanes of a
// wave read consecutive rows q at one u, on distinct banks), tmp[q][s] of the chunk beside it (rows of kChunk + 1 floats, written with q
// along the lanes, read with s along the lanes) -- at 128 x 128 that is 66 048 + 16 896 bytes of the CU's 160 KB; an operand with sides of
// at most 64 takes the SMALL form of each kernel, which declares 25 KB (same code, same bits, six blocks a CU).  The columns of an
// output are independent, so the split changes no bit.  The matrices are read from global memory at addresses that are uniform, or nearly,
// over a wave; an element (i, j) of one lies at p[i rs + j cs], so a transposed factor needs no copy.  Plain fp32 VALU arithmetic: the
// work is about 0.1 GFLOP on the headline window, and the matrix pipe would change the order of summation.
// No floating-point atomics: sum r^2 is folded in fp64 in a fixed order (thread, wave, block, then the blocks in index order), and the grid
// of the residual pass is laid out per item, so an item's rho does not depend on B and is the same on every run.
#include "vd_common.h"
#include <algorithm>

namespace vd {

namespace {
constexpr int kChunk = 32, kLdT = kChunk + 1, kXsFloats = kMaxLinopSide * (kMaxLinopSide + 1), kTmpFloats = kMaxLinopSide * kLdT;
static_assert((kXsFloats + kTmpFloats) * sizeof(float) + 64 <= 160 * 1024, "one block's operand and tmp fit the LDS of a CU");
// SMALL: the plane operand has sides of at most kSmallSide -- 25 KB of LDS in place of 83 KB, so that six blocks share a CU
constexpr int kSmallSide = 64;
template <bool SMALL> struct Lds {
    static constexpr int xs = SMALL ? kSmallSide * (kSmallSide + 1) : kXsFloats, tmp = SMALL ? kSmallSide * kLdT : kTmpFloats;
};
inline bool small_plane(int Q, int U) { return Q <= kSmallSide && U <= kSmallSide; }
#define LINOP_LAUNCH(kernel, vec, small, grid, stream, ...)                                                                 \
    do {                                                                                                                    \
        if (vec) {                                                                                                          \
            if (small) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(256), 0, stream, __VA_ARGS__);                   \
            else hipLaunchKernelGGL((kernel<true, false>), grid, dim3(256), 0, stream, __VA_ARGS__);                        \
        } else {                                                                                                            \
            if (small) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(256), 0, stream, __VA_ARGS__);                  \
            else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(256), 0, stream, __VA_ARGS__);                       \
        }                                                                                                                   \
    } while (0)

struct LinMat { const float* p; int rs, cs; };       // element (i, j) at p[i * rs + j * cs]
__host__ __device__ inline LinMat dense(const float* p, int cols) { return LinMat{p, cols, 1}; }
__host__ __device__ inline LinMat transposed(const float* p, int cols) { return LinMat{p, 1, cols}; }      // of a dense matrix with `cols` columns

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__host__ __device__ inline unsigned chunks_of(int n) { return (unsigned)(n + kChunk - 1) / kChunk; }

// Four values of row q of a Q x U plane at columns u .. u + 3 (u a multiple of 4); VEC (U % 4 == 0, p 16-byte aligned): one access.
// Elements at or beyond U are not read and come back 0.
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int q, int u, int U, float (&v)[4]) {
    if (VEC) {
        const float4 w = *reinterpret_cast<const float4*>(p + (size_t)q * U + u);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = u + e < U ? p[(size_t)q * U + u + e] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int q, int u, int U, const float (&v)[4]) {
    if (VEC) *reinterpret_cast<float4*>(p + (size_t)q * U + u) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (u + e < U) p[(size_t)q * U + u + e] = v[e];
    }
}

// The Q x U operand into LDS, xs[q * ldx + u], in quads of four columns; get(q, u, v) hands out four values.
template <class Get>
__device__ __forceinline__ void fill_plane(float* xs, int ldx, int Q, int U, Get get) {
    const int qw = (U + 3) >> 2;
    for (int i = threadIdx.x; i < Q * qw; i += 256) {
        const int q = i / qw, u = (i - q * qw) * 4;
        float v[4];
        get(q, u, v);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (u + e < U) xs[q * ldx + u + e] = v[e];
    }
}

// Columns s0 .. s0 + sc - 1 of Z = L X R^T in the documented order, X in LDS; epi(p, s, z) receives every element once.  All 256 threads
// of the block call it together (two barriers inside: in front of tmp's first read and behind its last).
template <class Epi>
__device__ __forceinline__ void two_sided(const float* xs, int ldx, float* tmp, LinMat L, LinMat R, int P, int Q, int U, int s0, int sc, Epi epi) {
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < Q * sc; i += 256) {
        const int sl = i / Q, q = i - sl * Q;
        const float* xr = xs + q * ldx;
        const float* rr = R.p + (size_t)(s0 + sl) * R.rs;
        float acc = 0.f;
#pragma unroll 4
        for (int u = 0; u < U; ++u) acc = acc + xr[u] * rr[(size_t)u * R.cs];
        tmp[q * kLdT + sl] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P * sc; i += 256) {
        const int p = i / sc, sl = i - p * sc;
        const float* lr = L.p + (size_t)p * L.rs;
        float acc = 0.f;
#pragma unroll 4
        for (int q = 0; q < Q; ++q) acc = acc + lr[(size_t)q * L.cs] * tmp[q * kLdT + sl];
        epi(p, s0 + sl, acc);
    }
    __syncthreads();
}
}  // namespace

static int check_sides(int H, int W, int Mh, int Mw) {
    VD_REQUIRE(linop_served(H, Mh) && linop_served(W, Mw), "linear operator: A_h is Mh x H and A_w is Mw x W with 1 <= Mh <= H <= 128 and 1 <= Mw <= W <= 128");
    return 0;
}

// ------------------------------------------------------------------ linop_apply_kernel
// out = L x R^T of `planes` planes of Q x U, out planes of P x S; the block walks the (plane, chunk) pairs.
template <bool VEC, bool SMALL>
__global__ __launch_bounds__(256) void linop_apply_kernel(const float* __restrict__ x, LinMat L, LinMat R, size_t planes, int P, int Q, int U,
                                                          int S, float* __restrict__ out) {
    __shared__ float xs[Lds<SMALL>::xs];
    __shared__ float tmp[Lds<SMALL>::tmp];
    const int ldx = U | 1;
    const unsigned nch = chunks_of(S);
    for (size_t wi = blockIdx.x; wi < planes * nch; wi += gridDim.x) {
        const size_t plane = wi / nch;
        const int s0 = (int)(wi - plane * nch) * kChunk, sc = min(kChunk, S - s0);
        const float* xp = x + plane * (size_t)Q * U;
        float* op = out + plane * (size_t)P * S;
        fill_plane(xs, ldx, Q, U, [&](int q, int u, float (&v)[4]) { load4<VEC>(xp, q, u, U, v); });
        __syncthreads();
        two_sided(xs, ldx, tmp, L, R, P, Q, U, s0, sc, [&](int p, int s, float z) { op[(size_t)p * S + s] = z; });
    }
}

int launch_linop_apply(const float* x, const float* L, int P, int Q, const float* R, int S, int U, size_t planes, float* out, hipStream_t s) {
    VD_REQUIRE(x && L && R && out && x != out, "linop: null tensor, or out == x");
    VD_REQUIRE(planes > 0 && planes < ((size_t)1 << 31), "linop: shape");
    VD_REQUIRE(P >= 1 && P <= kMaxLinopSide && Q >= 1 && Q <= kMaxLinopSide && S >= 1 && S <= kMaxLinopSide && U >= 1 && U <= kMaxLinopSide,
               "linop: L is P x Q and R is S x U with every side in 1 .. 128");
    const unsigned grid = (unsigned)std::min<size_t>(planes * chunks_of(S), 4096);
    LINOP_LAUNCH(linop_apply_kernel, U % 4 == 0 && al16(x), small_plane(Q, U), dim3(grid), s, x, dense(L, Q), dense(R, U), planes, P, Q, U, S, out);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ linop_residual_kernel
// blockIdx.z is the item, blockIdx.y walks the item's 3 T planes, blockIdx.x is the chunk of the plane's Mw output columns.  Per plane: x_0
// into LDS (by the block of chunk 0 also into `xstart` when given), then Z = A_h x_0 A_w^T of the chunk, r = y - Z, and r^2 added in fp64
// to the thread's running sum in the order the thread meets its elements; the block's sum is folded by wave shuffles and across its four
// waves in wave order, and written to part[b][blockIdx.y * gridDim.x + blockIdx.x] (part null: not kept).  Frames that are not latent:
// nothing is written to r; with `xstart` they still get their x_0.  An index t outside the schedule (x != null): the item writes NaN
// partials, NaN into r on its latent frames and NaN into `xstart`.  x null: src is the x_0 prediction itself (through the clamp when clip),
// t is not read; xstart may then alias src -- the clamp is idempotent -- and may not otherwise.
template <bool VEC, bool SMALL>
__global__ __launch_bounds__(256) void linop_residual_kernel(LinopArgs a) {
#pragma clang fp contract(off)
    __shared__ float xs[Lds<SMALL>::xs];
    __shared__ float tmp[Lds<SMALL>::tmp];
    __shared__ double red[4];
    const int H = a.H, W = a.W, Mh = a.Mh, Mw = a.Mw, ldx = W | 1;
    const size_t hw = (size_t)H * W, mm = (size_t)Mh * Mw;
    const unsigned b = blockIdx.z, planes = (unsigned)a.T * 3;
    const bool given = a.x == nullptr;
    const int NT = a.num_timesteps;
    const long long t = given ? 0 : a.t[b];
    const bool t_ok = given || (t >= 0 && t < NT);
    const float sr = !given && t_ok ? a.tab[TAB_SQRT_RECIP * NT + t] : 0.f, srm1 = !given && t_ok ? a.tab[TAB_SQRT_RECIPM1 * NT + t] : 0.f;
    const int s0 = (int)blockIdx.x * kChunk, sc = min(kChunk, Mw - s0);
    const bool hands_out = a.xstart && blockIdx.x == 0;
    double acc = t_ok ? 0.0 : (double)__builtin_nanf("");
    for (unsigned plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const size_t frame = (size_t)b * a.T + plane / 3, base = ((size_t)b * planes + plane) * hw, ybase = ((size_t)b * planes + plane) * mm;
        const bool latent = a.lat[frame] == 1.0f;                  // (uniform over the block: a plane lies in one frame)
        if (!latent && !hands_out) continue;
        if (latent && !t_ok) {
            for (int i = threadIdx.x; i < Mh * sc; i += 256) a.r[ybase + (size_t)(i / sc) * Mw + s0 + i % sc] = __builtin_nanf("");
            if (!hands_out) continue;
        }
        fill_plane(xs, ldx, H, W, [&](int q, int u, float (&v)[4]) {
            float x[4] = {0.f, 0.f, 0.f, 0.f}, s[4];
            if (!given) load4<VEC>(a.x + base, q, u, W, x);
            load4<VEC>(a.src + base, q, u, W, s);
            bool nonfinite = false;                                // the sampler pass of the step reads the same values and raises the bit
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = t_ok ? pass_x0(x[e], s[e], given, sr, srm1, a.clip, nonfinite) : __builtin_nanf("");
            if (hands_out) store4<VEC>(a.xstart + base, q, u, W, v);
        });
        __syncthreads();
        if (latent && t_ok)
            two_sided(xs, ldx, tmp, dense(a.A_h, H), dense(a.A_w, W), Mh, H, W, s0, sc, [&](int p, int s, float z) {
                const float r = a.y[ybase + (size_t)p * Mw + s] - z;
                a.r[ybase + (size_t)p * Mw + s] = r;
                acc += (double)r * (double)r;
            });
        else __syncthreads();
    }
    if (!a.part) return;
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        a.part[(size_t)b * a.nblk + blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the grid of one item: its planes along y, the chunks of a plane's Mw columns along x, dps_partials_per_item() blocks at most -- a
// function of (T, Mw) alone, so that an item's partials, and their number, do not depend on B
static dim3 linop_residual_grid(const LinopArgs& a) {
    const size_t cap = dps_partials_per_item();
    const unsigned gx = chunks_of(a.Mw);
    const unsigned gy = (unsigned)std::min<size_t>((size_t)a.T * 3, std::max<size_t>(cap / gx, 1));
    return dim3(gx, gy, (unsigned)a.B);
}

static int check_linop_args(const LinopArgs& a, const char* who, bool seed) {
    VD_REQUIRE(a.src && a.y && a.lat && a.r && a.A_h && a.A_w && (!seed || (a.x && a.part && a.deps && a.dxd)), std::string(who) + ": null tensor");
    VD_REQUIRE(!a.x || (a.t && a.tab && a.num_timesteps > 0), std::string(who) + ": x_t without t and the tables");
    VD_REQUIRE(!a.xstart || a.xstart != a.src || !a.x, std::string(who) + ": xstart may alias src only where src is the x_0 prediction");
    VD_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0, std::string(who) + ": shape");
    VD_REQUIRE((double)a.T * 3.0 * (double)a.H * (double)a.W < 2147483648.0, std::string(who) + ": an item of fewer than 2^31 elements");
    return check_sides(a.H, a.W, a.Mh, a.Mw);
}

static void launch_linop_residual_kernel(const LinopArgs& a, hipStream_t s) {
    const dim3 grid = linop_residual_grid(a);
    const bool vec = a.W % 4 == 0 && al16(a.x) && al16(a.src) && (!a.xstart || al16(a.xstart));
    LINOP_LAUNCH(linop_residual_kernel, vec, small_plane(a.H, a.W), grid, s, a);
}

// The residual pass alone (the projection; particle steering's built-in reward): r, the per-item partials of sum r^2 where a.part is
// given, x_0 where a.xstart is.  *nblk (or null): partials per item of this launch.  deps, dxd, rho and err are not read.
int launch_linop_residual(LinopArgs a, int* nblk, hipStream_t s) {
    if (int rc = check_linop_args(a, "linop_residual", false)) return rc;
    const dim3 rg = linop_residual_grid(a);
    a.nblk = (int)(rg.x * rg.y);
    if (nblk) *nblk = a.nblk;
    launch_linop_residual_kernel(a, s);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ linop_project_kernel
// x_0 <- x_0 + P_h r P_w^T on the planes of the frames with lat == 1, in place: the block walks the (plane, chunk of W columns) pairs, r's
// plane in LDS.  One addition per element, rounded to fp32.  A frame that is not latent is neither read nor written.  An r that is not
// finite (the residual pass's NaN for an item whose t lies outside the schedule) comes out not finite on every element it reaches.
template <bool VEC, bool SMALL>
__global__ __launch_bounds__(256) void linop_project_kernel(float* __restrict__ x0, const float* __restrict__ r, const float* __restrict__ lat,
                                                            LinMat Ph, LinMat Pw, unsigned planes, int H, int W, int Mh, int Mw) {
#pragma clang fp contract(off)
    __shared__ float xs[Lds<SMALL>::xs];
    __shared__ float tmp[Lds<SMALL>::tmp];
    const int ldx = Mw | 1;
    const unsigned nch = chunks_of(W);
    for (unsigned wi = blockIdx.x; wi < planes * nch; wi += gridDim.x) {
        const unsigned plane = wi / nch;
        if (lat[plane / 3] != 1.0f) continue;                      // (uniform over the block)
        const int s0 = (int)(wi - plane * nch) * kChunk, sc = min(kChunk, W - s0);
        const float* rp = r + (size_t)plane * Mh * Mw;
        float* xp = x0 + (size_t)plane * H * W;
        fill_plane(xs, ldx, Mh, Mw, [&](int q, int u, float (&v)[4]) { load4<VEC>(rp, q, u, Mw, v); });
        __syncthreads();
        two_sided(xs, ldx, tmp, Ph, Pw, H, Mh, Mw, s0, sc, [&](int p, int s, float z) { xp[(size_t)p * W + s] = xp[(size_t)p * W + s] + z; });
    }
}

int launch_linop_project(float* x0, const float* r, const float* lat, const float* P_h, const float* P_w, int B, int T, int H, int W, int Mh,
                         int Mw, hipStream_t s) {
    VD_REQUIRE(x0 && r && lat && P_h && P_w, "linop_project: null tensor");
    VD_REQUIRE(B > 0 && T > 0 && (double)B * T * 3.0 < 2147483648.0 / kChunk, "linop_project: shape");
    if (int rc = check_sides(H, W, Mh, Mw)) return rc;
    const unsigned planes = (unsigned)B * T * 3;
    const unsigned grid = (unsigned)std::min<size_t>((size_t)planes * chunks_of(W), 4096);
    LINOP_LAUNCH(linop_project_kernel, Mw % 4 == 0 && al16(r), small_plane(Mh, Mw), dim3(grid), s, x0, r, lat, dense(P_h, Mh), dense(P_w, Mw), planes, H, W, Mh, Mw);
    VD_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ linop_seed_kernel
// Grid (blocks of an item, B).  Thread 0 of every block folds the item's partials in index order in fp64, rho_b = fp32(sqrt(sum)); block
// 0 writes it.  Then the block walks the item's (plane, chunk of W columns) pairs: 0 on a frame that is not latent or where rho_b == 0;
// else r's plane into LDS and, per element, in fp32, one rounding each,
//   q = -(A_h^T r A_w) / rho_b,  q_r = q where !clip or -1 <= x_0r <= 1 else 0 (x_0r = xstart_from_eps(a, x_t, b, eps): the sampler pass's
//   bits),  d eps = (-b) * q_r,  d_x = a * q_r.
// An index t outside the schedule: NaN on every element of the item and in rho_b, and bit 0 of the error word.
template <bool VEC, bool SMALL>
__global__ __launch_bounds__(256) void linop_seed_kernel(LinopArgs a) {
#pragma clang fp contract(off)
    __shared__ float xs[Lds<SMALL>::xs];
    __shared__ float tmp[Lds<SMALL>::tmp];
    __shared__ float rho_s;
    const int b = blockIdx.y;
    const int NT = a.num_timesteps;
    const long long t = a.t[b];
    const bool t_ok = t >= 0 && t < NT;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int j = 0; j < a.nblk; ++j) s += a.part[(size_t)b * a.nblk + j];
        const float rho = t_ok ? (float)sqrt(s) : __builtin_nanf("");
        rho_s = rho;
        if (blockIdx.x == 0) {
            if (a.rho) a.rho[b] = rho;
            if (!t_ok && a.err) atomicOr(a.err, VD_ERR_TIMESTEP);
        }
    }
    __syncthreads();
    const float rho = rho_s;
    const float sr = t_ok ? a.tab[TAB_SQRT_RECIP * NT + t] : 0.f, srm1 = t_ok ? a.tab[TAB_SQRT_RECIPM1 * NT + t] : 0.f;
    const int H = a.H, W = a.W, Mh = a.Mh, Mw = a.Mw, ldx = Mw | 1;
    const size_t hw = (size_t)H * W, mm = (size_t)Mh * Mw;
    const unsigned planes = (unsigned)a.T * 3, nch = chunks_of(W);
    for (unsigned wi = blockIdx.x; wi < planes * nch; wi += gridDim.x) {
        const unsigned plane = wi / nch;
        const size_t base = ((size_t)b * planes + plane) * hw;
        const int s0 = (int)(wi - plane * nch) * kChunk, sc = min(kChunk, W - s0);
        const bool conv = t_ok && a.lat[(size_t)b * a.T + plane / 3] == 1.0f && rho != 0.f;      // (uniform over the block)
        if (!conv) {
            const float v = t_ok ? 0.f : __builtin_nanf("");
            for (int i = threadIdx.x; i < H * sc; i += 256) {
                const size_t o = base + (size_t)(i / sc) * W + s0 + i % sc;
                a.deps[o] = v; a.dxd[o] = v;
            }
            continue;
        }
        const float* rp = a.r + ((size_t)b * planes + plane) * mm;
        fill_plane(xs, ldx, Mh, Mw, [&](int q, int u, float (&v)[4]) { load4<VEC>(rp, q, u, Mw, v); });
        __syncthreads();
        two_sided(xs, ldx, tmp, transposed(a.A_h, H), transposed(a.A_w, W), H, Mh, Mw, s0, sc, [&](int p, int s, float z) {
            const size_t o = base + (size_t)p * W + s;
            const float q = -z / rho;
            const float x0r = xstart_from_eps(sr, a.x[o], srm1, a.src[o]);
            const float qr = (!a.clip || (x0r >= -1.0f && x0r <= 1.0f)) ? q : 0.f;
            a.deps[o] = -srm1 * qr;
            a.dxd[o] = sr * qr;
        });
    }
}

int launch_linop_seed(LinopArgs a, hipStream_t s) {
    if (int rc = check_linop_args(a, "linop_seed", true)) return rc;
    const dim3 rg = linop_residual_grid(a);
    a.nblk = (int)(rg.x * rg.y);
    launch_linop_residual_kernel(a, s);
    const size_t work = (size_t)a.T * 3 * chunks_of(a.W);
    const unsigned nb = (unsigned)std::min<size_t>(work, std::max<size_t>(4096 / a.B, 1));
    LINOP_LAUNCH(linop_seed_kernel, a.Mw % 4 == 0 && al16(a.r), small_plane(a.Mh, a.Mw), dim3(nb, a.B), s, a);
    VD_HIP(hipGetLastError());
    return 0;
}

}  // namespace vd
