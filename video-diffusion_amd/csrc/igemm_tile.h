// The K loop of the fp32 implicit-GEMM kernels (v_mfma_f32_32x32x2_f32), gfx950: igemm.hip (the engine's generic kernel) and
// conv_cl.hip (the channels-last conv of the LPIPS and I3D feature networks) differ in how an A quad is gathered, in what is
// done to it before it is staged, and in the epilogue; the pipeline between them is written here, once.
//
// Tiling (wave64, 256 threads = 4 waves as 2x2, each wave (BM/2)x(BN/2) as 32x32 MFMA tiles):
//   K-step = 32 reduction elements.  A tile [BM][32], B tile [BN][32] (both K-contiguous), rows padded to 36 floats:
//   ds_read_b128 of 16 lanes on 16 distinct 16-byte slots -> conflict-free (guide: LDS banking, ds_read_b128 lane groups).
//   Loader: thread -> (row lrow + 32j, 4-float quad lq of the K-step), lrow = tid >> 3, lq = tid & 7.
//   MFMA 32x32x2 takes one f32 per lane per operand with k = lane>>5; a lane's float4 from LDS
//   feeds 4 consecutive MFMAs (k order is free as long as A and B agree), so operand traffic is
//   one ds_read_b128 per 4 MFMAs per fragment.
//   Pipeline: global loads of step s+1 are issued before the MFMAs of step s (register staging:
//   the operand transform needs VALU anyway), written to the other LDS buffer after them; one
//   barrier per K-step.
//   Loads are unconditional (a padding tap reads element 0 and is zeroed before it is staged): a branch around a load makes
//   hipcc drain the whole queue (vmcnt(0)) at the join.
#pragma once
#include "vd_common.h"

namespace vd {

constexpr int IG_BK = 32;    // K-step
constexpr int IG_LDP = 36;   // padded LDS row (floats)

// C/D layout of the 32x32 MFMA: accumulator element r of a lane is column lane & 31, row igemm_cd_row(r, lane).  The map is the sum
// of an element part and a lane part, row(r, lane) = row(r, 0) + row(0, lane): an epilogue keeps the lane part in its base row.
__device__ __forceinline__ int igemm_cd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// As [2][BM][IG_LDP], Bs [2][BN][IG_LDP] in LDS; acc is zeroed here.
// load(s, ra, rb): issue the global loads of K-step s into the register stage (f32x4 ra[BM/32], rb[BN/32])
// fix(s, j, v)   : what is written to LDS for A row j (identity, or affine + SiLU + zero padding)
template <int BM, int BN, class Load, class Fix>
__device__ __forceinline__ void igemm_tile_loop(float* As, float* Bs, int nsteps, Load load, Fix fix,
                                                f32x16 (&acc)[BM / 64][BN / 64]) {
    constexpr int MI = BM / 64, NI = BN / 64;     // 32x32 tiles per wave in M / N
    constexpr int AR = BM / 32, BR = BN / 32;     // loader rows per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;
    const int lrow = tid >> 3, lq = tid & 7;
    f32x4 ra[AR], rb[BR];

    auto stage = [&](int s, int buf) {
        float* Ad = As + buf * BM * IG_LDP;
        float* Bd = Bs + buf * BN * IG_LDP;
#pragma unroll
        for (int j = 0; j < AR; ++j)
            *reinterpret_cast<f32x4*>(Ad + (lrow + 32 * j) * IG_LDP + lq * 4) = fix(s, j, ra[j]);
#pragma unroll
        for (int j = 0; j < BR; ++j)
            *reinterpret_cast<f32x4*>(Bd + (lrow + 32 * j) * IG_LDP + lq * 4) = rb[j];
    };
    auto compute = [&](int buf) {
        const float* Ab = As + buf * BM * IG_LDP + (wm * (BM / 2) + lr) * IG_LDP + lh * 4;
        const float* Bb = Bs + buf * BN * IG_LDP + (wn * (BN / 2) + lr) * IG_LDP + lh * 4;
#pragma unroll
        for (int kg = 0; kg < IG_BK / 8; ++kg) {
            f32x4 fa[MI], fb[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * IG_LDP + kg * 8);
#pragma unroll
            for (int j = 0; j < NI; ++j) fb[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * IG_LDP + kg * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
    };

#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load(0, ra, rb);
    stage(0, 0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) load(s + 1, ra, rb);
        compute(s & 1);
        if (more) stage(s + 1, (s + 1) & 1);
        __syncthreads();
    }
}

}  // namespace vd
