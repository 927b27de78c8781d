// What the Winograd F(2x2,3x3) conv kernels have in common, written once: conv_wino_r64.hip and conv_wino_z128.hip (the 16-bit
// kernels) share the patch image, the block map, the f16x3 register pieces and the whole output transform; conv_wino.hip (fp32 MFMA,
// another patch layout, both cout tiles exchanged in one pass) takes the statistics accumulation and the host helper.  The main loops, their slot tables and wait counts are the
// kernels' own.  Everything here is inlined into one-wave-per-SIMD kernels: tools/wino_asm_diff.py compares the generated code.
#pragma once
#include "vd_common.h"

namespace vd {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, (short)0, 0, 0)) wino_rsrc;
typedef __attribute__((address_space(3))) void* wino_lds_ptr;

// ---- host ---------------------------------------------------------------------------------------------------------------------
inline bool wino_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// Work items of a launch: tile groups (nbx: 16 x 16 output pixels of a frame, or with TF4 four frames of an 8 x 8 map) x cout blocks
// (ncb).  ksplit > 1: blockIdx.y = the block's slice of the channel chunks.  phase_cb > 0 (= real Cout / 32) and cgroup: the sub-pixel
// form of Upsample + conv (conv3x3_wino_r64_ups_kernel).
struct WinoItemGeom { int tiles_x, tiles_y, nbx, ncb, nitems, xcd_order; int ksplit = 1; int phase_cb = 0; int cgroup = 0; };

inline WinoItemGeom wino_item_geom(int Hl, int nfr, int Cout, int block_couts, bool tf4) {
    WinoItemGeom g;
    g.tiles_x = tf4 ? 1 : Hl / 16; g.tiles_y = g.tiles_x;
    g.nbx = g.tiles_x * g.tiles_y * (tf4 ? (nfr + 3) / 4 : nfr);
    g.ncb = Cout / block_couts;
    g.nitems = g.nbx * g.ncb;
    g.xcd_order = g.nbx % 8 == 0;
    return g;
}

// ---- cycle stamps of ONE work item (timing builds; wave 0 of block 7) into the file's own symbol: stamps 14 / 15 take the 100 MHz clock
#ifdef VD_WINO_TIMING
#define VD_WINO_STAMP(sym, i)                                                                         \
    do {                                                                                              \
        if (threadIdx.x == 0 && blockIdx.x == 7) {                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                        \
            sym[i] = (i) >= 14 ? __builtin_amdgcn_s_memrealtime() : __builtin_readcyclecounter();     \
            __builtin_amdgcn_sched_barrier(0);                                                        \
        }                                                                                             \
    } while (0)
#else
#define VD_WINO_STAMP(sym, i)
#endif

// ---- patch image of the 16-bit kernels ------------------------------------------------------------------------------------------
// LDS-DMA (buffer_load_dwordx4 ... lds: lane l of a request writes 16 bytes at M0 + 16 l whatever address it gathers from, zeros where
// that address fails the descriptor's range check): [row P][x parity 2][slot SPP][64 B = 16 channels of one pixel]; the four 16-byte
// quads of a pixel are stored at quad ^ ((row >> 1) & 3), so that the 16 lanes of a ds_read_b128 group (four tile rows x four tile
// columns) fall on 16 different bank quads.
// TF4 = false: one frame, 8 x 8 tiles (maps >= 16 x 16).  TF4 = true: FOUR frames of an 8 x 8 map, 4 x 4 tiles each, a 10 x 10 patch per
// frame at a frame stride of FSB bytes (every stride a multiple of 256 bytes, so the bank argument holds across tile rows and frames).
template <bool TF4> struct R64G {
    static constexpr int P = TF4 ? 10 : 18;                 // patch width
    static constexpr int SPP = TF4 ? 6 : 10;                // 64-byte pixel slots per plane row (P / 2 pixels + 1 pad)
    static constexpr int PLB = SPP * 64, RSB = 2 * PLB;
    static constexpr int FSB = TF4 ? P * RSB : 0;           // frame stride
    static constexpr int NX = TF4 ? 8 : 6;                  // DMA instructions per thread and patch (256 threads x 16 B each)
    static constexpr int XBUF = NX * 4096;
    static constexpr int MOFF = TF4 ? 2 * FSB : 8 * RSB;    // second M-tile: two frames / four tile rows further
    static constexpr int NB = 4;                            // patch buffers; one more only ever receives the requests past the last chunk
    static constexpr int LDS_BYTES = (NB + 1) * XBUF;       // 122880 | 163840 (the Z image of the output transform, 64 KB, overlays the patches)
};

// 16-byte LDS slot gs = e*256 + tid of a patch buffer -> what it holds: frame fl of the item, pixel (ly, lx) of the map, and the pixel's
// quad `quad` (the slot at quad position gs & 3 of patch row py holds quad (gs & 3) ^ ((py >> 1) & 3)); in: a slot of the image whose
// pixel lies inside the picture
struct WinoPatchSlot { int fl, ly, lx, quad; bool in; };
template <bool TF4>
__device__ __forceinline__ WinoPatchSlot wino_patch_slot(int gs, int oy0, int ox0, int Hl, int Wl) {
    using G = R64G<TF4>;
    constexpr int P = G::P, SPP = G::SPP;
    const int lq = gs & 3, ps0 = gs >> 2;
    const int fl = TF4 ? ps0 / (P * 2 * SPP) : 0, ps = TF4 ? ps0 % (P * 2 * SPP) : ps0;   // frame of the item, slot inside its image
    const int py = ps / (2 * SPP), r = ps % (2 * SPP), pxh = r % SPP, px = 2 * pxh + r / SPP;
    const int ly = oy0 + py - 1, lx = ox0 + px - 1;
    return {fl, ly, lx, lq ^ ((py >> 1) & 3), fl < (TF4 ? 4 : 1) && py < P && pxh < P / 2 && ly >= 0 && ly < Hl && lx >= 0 && lx < Wl};
}

// Request e of the patch of `chunk`: 16 bytes per thread from byte offset xo + 64 chunk.  A request past the item's last chunk must not
// land in the output transform's Z image.  It is NOT skipped by a branch: hipcc's s_waitcnt insertion merges the two paths of a
// conditional request to the one with FEWER loads in flight, i.e. every wait for a weight fragment behind it becomes a wait for the
// patch itself.  The request always issues; when it is late it goes through a descriptor of zero records (xnull: no memory access,
// zeros) into the spare fifth buffer.
template <class G>
__device__ __forceinline__ void wino_patch_dma(wino_rsrc xsrc, wino_rsrc xnull, char* lds, int wi, int chunk, int nchunk, int e, unsigned xo) {
#if defined(__HIP_DEVICE_COMPILE__)      // (hipcc's host pass drops a kernel whose body names this builtin)
    const bool live = chunk < nchunk;
    const int bufi = live ? (chunk & (G::NB - 1)) : G::NB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(live ? xsrc : xnull, (wino_lds_ptr)(lds + bufi * G::XBUF + e * 4096 + wi * 1024), 16, xo, chunk * 64, 0, 0);
#endif
}

// ---- block -> (tile group, first cout tile), NCT cout tiles per block: blocks are dealt to the 8 XCDs round-robin; inside an XCD the
// cout blocks of one patch are neighbours.  GROUPED: the kernel also takes the grouped walk (g.cgroup > 0)
template <int NCT, bool GROUPED = false>
__device__ __forceinline__ void wino_item(const WinoItemGeom& g, int& bx, int& cob0) {
    if (GROUPED && g.xcd_order && g.cgroup > 0) {
        // sub-pixel form: 4 x the cout blocks (16 .. 32 weight slices of 1 - 2 MB against 4 MB of L2 per XCD).  With the cout
        // block as the fast index every slice had two concurrent readers per XCD (one at 512 couts) and the loop waited on
        // weights from beyond the L2: 1452 -> 1252 us only for a quarter fewer MFMAs, 338 -> 351 at 512 couts.  Here an XCD
        // walks ALL its patches with four cout blocks before it takes the next four.
        const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3, px = g.nbx >> 3;
        const int c_lo = loc % g.cgroup, rest = loc / g.cgroup;
        cob0 = ((rest / px) * g.cgroup + c_lo) * NCT;
        bx = (rest % px) * 8 + xcd;
    } else if (g.xcd_order) {
        const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
        cob0 = (loc % g.ncb) * NCT;
        bx = (loc / g.ncb) * 8 + xcd;
    } else {
        bx = blockIdx.x % g.nbx;
        cob0 = (blockIdx.x / g.nbx) * NCT;
    }
}

// ---- f16x3 register pieces ------------------------------------------------------------------------------------------------------
// weight piece 2 = 2^-12 x piece 0 (split_pack.hip), formed in registers: four v_pk_mul_f16 instead of a 1 KiB load (exact: a power of
// two, fp16 subnormals honoured like the host's conversion)
__device__ __forceinline__ void wino_b_third(u32x4& b2, const u32x4& b0) {
    const unsigned two_m12 = 0x0c000c00u;                             // (2^-12, 2^-12) in fp16
    asm("v_pk_mul_f16 %0, %4, %8\n\tv_pk_mul_f16 %1, %5, %8\n\tv_pk_mul_f16 %2, %6, %8\n\tv_pk_mul_f16 %3, %7, %8"
        : "=&v"(b2[0]), "=&v"(b2[1]), "=&v"(b2[2]), "=&v"(b2[3]) : "v"(b0[0]), "v"(b0[1]), "v"(b0[2]), "v"(b0[3]), "s"(two_m12));
}
// the a1 piece of a channel pair, up to its conversion: r = x - a0 (v_fma_mix_f32 reads the fp16 half), r * 2^12.  Operand NUMBERS of
// the asm statement it is pasted into: r0, r1 (out), a0 (the packed pair), x0, x1; the statement places v_cvt_pk_f16_f32 itself
#define VD_WINO_A1(r0, r1, a0, x0, x1)                                                                                                 \
    "v_fma_mix_f32 %" #r0 ", %" #a0 ", -1.0, %" #x0 " op_sel_hi:[1,0,0]\n\tv_fma_mix_f32 %" #r1 ", %" #a0 ", -1.0, %" #x1 " op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t" \
    "v_ldexp_f32 %" #r0 ", %" #r0 ", 12\n\tv_ldexp_f32 %" #r1 ", %" #r1 ", 12\n\t"

// ---- output transform of the 16-bit kernels, one cout tile at a time ------------------------------------------------------------------
// Z[q] = sum_j M[wi][j] A[j][q] is wave-local; the sum over the rows crosses the waves through LDS; wave (p, q) = (wi >> 1, wi & 1) then
// owns output pixel (p, q) of every tile.  Z image: [plane 2*i + q 8][m 2][c4 4][lane 64][4 floats] = 64 KB over the patch buffers.

// Byte offsets of C/D register r of M-tile m (row = tile m*32 + (r & 3) + 8 (r >> 2) + 4 lh of the item) in the output / residual, channel
// c0.  PH, the sub-pixel form: pixel (y, x) of the low-resolution map goes to (2y, 2x + ppb) of the Ho x Wo output.  A frame past the
// end is neither read nor stored.
template <bool TF4, bool PH>
__device__ __forceinline__ void wino_out_offsets(unsigned (&oo)[2][16], int lh, int p, int q, int f0, int nfr, int oy0, int ox0, int Ho, int Wo, int ldo, int c0, int ppb) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tt = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int tx = TF4 ? tt & 3 : tt & 7, ty = TF4 ? (tt >> 2) & 3 : tt >> 3, nf = f0 + (TF4 ? tt >> 4 : 0);
            const unsigned o = PH ? (unsigned)(((nf * Ho + 2 * (oy0 + 2 * ty + p)) * Wo + 2 * (ox0 + 2 * tx + q) + ppb) * ldo + c0) * 4u
                                  : (unsigned)(((nf * Ho + oy0 + 2 * ty + p) * Wo + ox0 + 2 * tx + q) * ldo + c0) * 4u;
            oo[m][r] = nf < nfr ? o : 0x80000000u;
        }
}

// the wave's two Z planes (q = 0, 1) of M-tile m
__device__ __forceinline__ void wino_z_write(float* Zs, int wi, int lane, int m, const f32x16& z0, const f32x16& z1) {
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        *reinterpret_cast<f32x4*>(Zs + ((((wi * 2 + 0) * 2 + m) * 4 + c4) * 64 + lane) * 4) = f32x4{z0[4 * c4], z0[4 * c4 + 1], z0[4 * c4 + 2], z0[4 * c4 + 3]};
        *reinterpret_cast<f32x4*>(Zs + ((((wi * 2 + 1) * 2 + m) * 4 + c4) * 64 + lane) * 4) = f32x4{z1[4 * c4], z1[4 * c4 + 1], z1[4 * c4 + 2], z1[4 * c4 + 3]};
    }
}

// GroupNorm statistics of one stored value.  Explicit fma: left to -ffp-contract, hipcc fused the square into the sum in one unrolled
// copy of such a loop and not in the other -- a frame's statistics then depended on its place in a four-frame item (r04m)
__device__ __forceinline__ void wino_stat_add(float& s, float& ss, float y) { s += y; ss = __builtin_fmaf(y, y, ss); }

// M-tile m of the output: Y[p][q] = Z[p] + sgn (Z[p+1] + Z[p+2]), sgn = +1 (p = 0) / -1 (p = 1), Z[p + k][q] = plane wi + 2k; then
// y * winv (F16: the weight row's power-of-two scale leaves here) + residual + bias (b8[h]: registers 8h .. 8h + 7, two frames with TF4),
// the sixteen stores, and with `stats` the lane's (sum, sum of squares) per frame slot (TF4: 2m + (r >> 3))
template <bool F16, bool TF4>
__device__ __forceinline__ void wino_out_rows(const float* Zs, int wi, int lane, int m, float sgn, float winv, const f32x16& rv, const float (&b8)[2],
                                              wino_rsrc osrc, const unsigned (&oo)[16], int nso, bool stats, float (&gsum)[TF4 ? 4 : 1][2]) {
    const float* zw = Zs + wi * 2048 + lane * 4;
    f32x16 y;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        const float* zp = zw + (m * 4 + c4) * 256;
        const f32x4 v = *reinterpret_cast<const f32x4*>(zp) +
                        (*reinterpret_cast<const f32x4*>(zp + 2 * 2048) + *reinterpret_cast<const f32x4*>(zp + 4 * 2048)) * sgn;
        y[4 * c4] = v.x; y[4 * c4 + 1] = v.y; y[4 * c4 + 2] = v.z; y[4 * c4 + 3] = v.w;
    }
    if constexpr (F16) y = y * winv + rv;
    else y += rv;
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] += b8[r >> 3];
#pragma unroll
    for (int r = 0; r < 16; ++r) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)y[r]), osrc, oo[r], nso, 0);
    if (stats) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int fs = TF4 ? 2 * m + (r >> 3) : 0;
            wino_stat_add(gsum[fs][0], gsum[fs][1], y[r]);
        }
    }
}

// GroupNorm partial sums of a block's output: the lanes' floats as doubles in LDS (the Z planes are dead) [wave 4][lh 2][frame NFS][lr 32][2]
// -- 8 partials per (frame, channel): 4 waves (the 4 pixels of a tile) x 2 k-halves -- which one thread per (frame, channel) adds in a
// fixed order and writes to where(fs, c) of the partial table (nullptr: a frame past the end)
template <int NFS, class Where>
__device__ __forceinline__ void wino_stats_reduce(float* smem, int tid, int wi, int lh, int lr, const float (&gsum)[NFS][2], Where where) {
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem);
#pragma unroll
    for (int fs = 0; fs < NFS; ++fs) {
        double* d = red + ((((wi * 2 + lh) * NFS + fs) * 32 + lr) * 2);
        d[0] = (double)gsum[fs][0]; d[1] = (double)gsum[fs][1];
    }
    __syncthreads();
    if (tid < NFS * 32) {
        const int fs = tid >> 5, c = tid & 31;
        double s = 0.0, ss = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { s += red[((k * NFS + fs) * 32 + c) * 2]; ss += red[((k * NFS + fs) * 32 + c) * 2 + 1]; }
        double* o = where(fs, c);
        if (o) { o[0] = s; o[1] = ss; }
    }
}

}  // namespace vd
