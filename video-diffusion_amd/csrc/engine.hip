// Step engine: UNet topology, packed weights, the per-step launch sequence and the C ABI.
//
// One process per GPU owns one engine.  A denoise step is a fixed sequence of ~600 kernel launches
// on the caller's stream; activations live in one bump-allocated arena sized per (B, T) window (288 GB
// of HBM: no buffer reuse games, the same addresses every step, so the sequence is graph-capturable).
// Weights live in ONE packed device buffer in kernel-ready layouts (see Param::kind).
//
// Reference call path being replaced (paths relative to /root/reference/improved_diffusion):
//   _WrappedModel.__call__ respace.py:111-119 -> CondMargVideoModel.forward unet.py:949-1026 ->
//   UNetVideoModel.forward :898-912 -> UNetModel.forward :768-839 ; p_sample gaussian_diffusion.py:403-448.
#include <cmath>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include/vd_amd.h"
#include "vd_common.h"

namespace vd {

thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

int launch_frame_t(const int64_t* fidx, int B, int T, int center, float* tv, hipStream_t s);

// PK_CONV3: [tap][Cout][Cin] for the generic kernel (igemm.hip).  PK_LINF / PK_STEM: every nn.Linear, 1x1 conv and the stem as a
// matrix image -- the split image of gemm_split.hip (split_pack.hip; VD_MATH=fp32: the fragment-major fp32 image of gemm_frag.hip).
// PK_CONV3W: Winograd F(2x2,3x3) image (conv_wino_r64.hip; fp32: conv_wino.hip).  PK_CONV3S: stride-2 conv on the split GEMM.
enum ParamKind { PK_RAW = 0, PK_CONV3, PK_STEM, PK_POSENC, PK_OUTCONV, PK_LINF, PK_CONV3W, PK_CONV3S,
                 PK_CONV3WU };      // PK_CONV3WU: Upsample + conv3x3 in its sub-pixel form (conv_wino_r64.hip): image of 4 x Cout phase kernels

struct Param {
    std::string name;
    int nd = 0;
    long long shape[4] = {1, 1, 1, 1};
    size_t numel = 0;        // as stored in the checkpoint
    size_t packed = 0;       // floats in the packed buffer
    size_t off = 0;          // float offset in the packed buffer
    int kind = PK_RAW;
    bool loaded = false;
    // PK_LINF members of a batched matrix (all FiLM projections / all RPE time projections are ONE GEMM):
    // `off` is the base of the whole fragment-major image, rows [frag_row0, +shape[0]) of frag_rows in total
    int frag_rows = 0, frag_row0 = 0;
    // backward-data image (use_gradient_method): the transposed matrix of a linear layer / 1x1 conv, the 180-degree-rotated
    // transposed kernel of a 3x3 conv, in the layout of kind_bwd; -1: the backward pass does not need this parameter
    int kind_bwd = -1;
    size_t off_bwd = 0, packed_bwd = 0;
};

struct ResP {
    int cin, cout;
    int gn1w, gn1b, c1w, c1b, embw, embb, gn2w, gn2b, c2w, c2b, skw = -1, skb = -1;
    int film_off = 0;        // column offset in the batched emb projection
};
struct RpeP { int dw = -1, db = -1, tw = -1, tb = -1, ow = -1, ob = -1, table = -1; int te_off = 0; };
struct AttP { int normw, normb, qkvw, qkvb, projw, projb; };
struct AttnP { int C; AttP sp, tp; RpeP rq, rk, rv; };
struct ConvP { int w, b, c; };
struct Layer { int type; int idx; };      // 0 stem, 1 res, 2 attn, 3 down, 4 up
// An activation tensor [N][H][H][C]; part/split: its GroupNorm partial sums [N][split][C][2] when the producing
// convolution's epilogue wrote them (conv_wino.hip), else null and the consumer's GroupNorm runs the statistics pass.
struct Tens { float* p; int C, H; double* part = nullptr; int split = 0; };

// ---- tape of one forward pass, kept when the step is guided (use_gradient_method): every op with the tensors its
// backward reads.  Pointers are arena addresses; nothing of a taped forward is released before the backward has run.
struct TapeRes { int idx; Tens x0, x1; bool has_x1; int N; float *A1, *B1, *mr1, *h, *A2, *B2, *mr2, *o; };
struct TapeAttn { int idx; Tens x; int B, T; float *xn, *qkv, *Rk, *Rq, *Rv, *o, *xt, *A, *Bf, *mr, *xn2, *qkv2, *o2, *xs; const float* amask; };
struct TapeConv { int type, idx; Tens in, out; };                     // 0 stem, 3 down, 4 up
struct TapePos { Tens in, out; };
struct TapeOp { int kind, i; };                                       // kind: 0 conv, 1 res, 2 attn, 5 posenc
struct Tape {
    std::vector<TapeOp> ops;
    std::vector<TapeRes> res; std::vector<TapeAttn> attn; std::vector<TapeConv> conv; std::vector<TapePos> pos;
    Tens head; float *headA = nullptr, *headB = nullptr, *head_mr = nullptr;
    void clear() { ops.clear(); res.clear(); attn.clear(); conv.clear(); pos.clear(); }
};

static const int CH_MULT_256[] = {1, 1, 2, 2, 4, 4};
static const int CH_MULT_128[] = {1, 1, 2, 3, 4};
static const int CH_MULT_64[] = {1, 2, 3, 4};
static const int CH_MULT_32[] = {1, 2, 2, 2};
// VD_MATH (vd_common.h): f16x3 (default) and bf16x6 run every matrix product on the split kernels (gemm_split.hip,
// conv_wino_r64.hip) over 16-bit piece images; fp32 keeps them on the fp32 MFMA (gemm_frag.hip, conv_wino.hip).
static bool split_math() { return math_mode() != MATH_FP32; }

constexpr int STEM_KPAD = 64;          // im2col width of the 5-channel 3x3 stem (45 real columns)

// ---- the backward-data image of one forward weight (vd_load_weight_bwd, vd_pack_weight_bwd): the operator d out / d in of a layer as
// a forward layer of its own.  O, I: the FORWARD's outputs and inputs.
enum BwdKind { BWD_LINEAR = 0, BWD_STEM = 1, BWD_CONV3_WINO = 2, BWD_CONV3_GENERIC = 3 };

// floats of the image
static size_t bwd_image_floats(int kind, size_t O, size_t I) {
    if (kind == BWD_STEM) return (size_t)STEM_KPAD * O * 3 / 2 + 2 * STEM_KPAD;      // split image of [STEM_KPAD][O]
    if (kind == BWD_LINEAR) return I * O * 3 / 2 + 2 * I;                            // split image of W^T [I][O]
    if (kind == BWD_CONV3_WINO) return 16 * I * O * 3 / 2 + 2 * I;                   // Winograd-split image of I kernels over O channels
    return 9 * I * O;                                                                // [tap][I][O]
}

// host: forward weight ([O][I] linear / 1x1, OIHW 3x3) -> out[bwd_image_floats()]
static void pack_weight_bwd(const float* host, int kind, int O, int I, float* out) {
    if (kind == BWD_STEM) {                            // forward lin[o][k = tap*I + i]; backward matrix [k][o], rows 9 I .. STEM_KPAD - 1 zero
        std::vector<float> lt((size_t)STEM_KPAD * O, 0.f);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < 9; ++t) lt[(size_t)(t * I + i) * O + o] = host[((size_t)o * I + i) * 9 + t];
        pack_linear_split(lt.data(), reinterpret_cast<unsigned short*>(out), STEM_KPAD, O, STEM_KPAD, 0);
    } else if (kind == BWD_LINEAR) {                   // W[O][I] -> W^T[I][O]
        std::vector<float> wt((size_t)O * I);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i) wt[(size_t)i * O + o] = host[(size_t)o * I + i];
        pack_linear_split(wt.data(), reinterpret_cast<unsigned short*>(out), I, O, I, 0);
    } else {                                           // w'[i][o][ky][kx] = w[o][i][2-ky][2-kx]
        std::vector<float> wr((size_t)O * I * 9);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < 9; ++t) wr[((size_t)i * O + o) * 9 + t] = host[((size_t)o * I + i) * 9 + (8 - t)];
        if (kind == BWD_CONV3_WINO) {
            pack_conv3_wino_split(wr.data(), reinterpret_cast<unsigned short*>(out), I, O);
        } else {                                       // generic kernel: [tap][Cout' = I][Cin' = O]
            for (int i = 0; i < I; ++i)
                for (int o = 0; o < O; ++o)
                    for (int t = 0; t < 9; ++t) out[((size_t)t * I + i) * O + o] = wr[((size_t)i * O + o) * 9 + t];
        }
    }
}

static int bwd_kind_of(const Param& p) {
    return p.kind == PK_STEM ? BWD_STEM : p.kind_bwd == PK_LINF ? BWD_LINEAR : p.kind_bwd == PK_CONV3W ? BWD_CONV3_WINO : BWD_CONV3_GENERIC;
}

struct Arena {
    char* base = nullptr;
    size_t cap = 0, used = 0, peak = 0;     // cap: bytes this arena may hand out (the workspace up to its tail; 0 = unchecked)
    bool dry = false, overflow = false;
    template <class Tp> Tp* get(size_t n) {
        size_t bytes = (n * sizeof(Tp) + 255) & ~(size_t)255;
        if (!dry && cap && used + bytes > cap) {
            // the dry run that sized the workspace did not see this request: never write past the arena (the tail holds t_model
            // and the eps scratch).  The request is served from the base -- results are garbage -- and the forward fails loudly.
            overflow = true;
            return reinterpret_cast<Tp*>(base);
        }
        char* p = (dry ? reinterpret_cast<char*>(0x1000) : base) + used;     // dry run: distinct, never dereferenced (the backward keys gradients by tensor address)
        used += bytes;
        peak = std::max(peak, used);
        return reinterpret_cast<Tp*>(p);
    }
    // stack discipline for transients: everything is stream-ordered on one stream, so a released range may be handed
    // out again by the next get()
    size_t mark() const { return used; }
    void release(size_t m) { used = m; }
};

// ---- per-class kernel timing with HIP events on the launch stream (bench.py's live roofline figure)
enum ProfClass { PC_IGEMM_128x128 = 0, PC_IGEMM_128x64, PC_IGEMM_64x128, PC_IGEMM_64x64, PC_GN_STATS, PC_GN_TEMPORAL,
                 PC_ATTN_SPATIAL, PC_ATTN_TEMPORAL, PC_OUT_CONV, PC_ELEMENTWISE, PC_POSTERIOR,
                 PC_CONV_128x128, PC_CONV_128x64, PC_CONV_64x128, PC_CONV_64x64, PC_CONV_WINO, PC_CONV_WINO_R64, PC_IGEMM_128x192,
                 PC_CONV_WINO_R64_UPS, PC_CONV_WINO_Z128, PC_COUNT };
// names of the kernels a class runs on: [0] split arithmetic (f16x3 | bf16x6), [1] VD_MATH=fp32
static const char* kProfNames[PC_COUNT][2] = {
    {"gemm_split_kernel<128,128>", "gemm_frag_kernel<128,128>"}, {"gemm_split_kernel<128,64>", "gemm_frag_kernel<128,64>"},
    {"gemm_split_kernel<64,128>", "gemm_frag_kernel<64,128>"}, {"gemm_split_kernel<64,64>", "gemm_frag_kernel<64,64>"},
    {"gn_stats_partial", "gn_stats_partial"}, {"gn_temporal_kernel", "gn_temporal_kernel"},
    {"attn_spatial_kernel", "attn_spatial_kernel"}, {"attn_temporal_kernel", "attn_temporal_kernel"},
    {"out_conv_kernel", "out_conv_kernel"}, {"affine_act_kernel", "affine_act_kernel"}, {"posterior_kernel", "posterior_kernel"},
    {"igemm_kernel<128,128> 3x3", "igemm_kernel<128,128> 3x3"}, {"igemm_kernel<128,64> 3x3", "igemm_kernel<128,64> 3x3"},
    {"igemm_kernel<64,128> 3x3", "igemm_kernel<64,128> 3x3"}, {"igemm_kernel<64,64> 3x3", "igemm_kernel<64,64> 3x3"},
    {"conv3x3_wino_kernel", "conv3x3_wino_kernel"}, {"conv3x3_wino_r64_kernel", "conv3x3_wino_r64_kernel"},
    {"gemm_split_kernel<128,192>", "gemm_split_kernel<128,192>"},
    {"conv3x3_wino_r64_ups_kernel", "conv3x3_wino_r64_ups_kernel"}, {"conv3x3_wino_z128_kernel", "conv3x3_wino_z128_kernel"}};
struct ProfRec { int cls; double flops, bytes; hipEvent_t a, b; char tag[56]; };
struct Profiler {
    bool on = false;
    std::vector<ProfRec> recs;
};
static Profiler g_prof;
static const char* prof_name(int i) {
    if (i < 0 || i >= PC_COUNT) return "";
    return kProfNames[i][!split_math()];
}

struct ProfScope {
    hipStream_t st; bool live;
    ProfScope(int cls, double flops, double bytes, hipStream_t s, const char* tag = "") : st(s), live(g_prof.on) {
        if (!live) return;
        ProfRec r{cls, flops, bytes, nullptr, nullptr, {0}};
        snprintf(r.tag, sizeof(r.tag), "%s", tag);
        (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b);
        (void)hipEventRecord(r.a, st);
        g_prof.recs.push_back(r);
    }
    ~ProfScope() { if (live) (void)hipEventRecord(g_prof.recs.back().b, st); }
};
// no event records for a scope (a stream capture, the window prefix build pass): the switch is restored on every way out
struct ProfPause {
    bool was = g_prof.on;
    ProfPause() { g_prof.on = false; }
    ~ProfPause() { g_prof.on = was; }
};

// res_block decides from the SHAPE alone (conv_wino_z128_act_shape) that a conv activates in its own patch staging and then never
// materialises the activation image; the dispatcher takes the activating kernel only when conv_wino_z128_act_supported holds for the
// call as built (weight image, piece count, strides, size limits).  If the two ever disagree the conv would get a raw tensor plus
// (A, B) that no other kernel applies: say so here, by name, instead of failing later with the generic "no kernel covers" error.
static bool act_conv_will_dispatch(const IgemmArgs& g) {
    return g.affA && igemm_kernel(igemm_first_launch(g)) == IK_Z128;     // (the plain z128 kernel takes no affine)
}

static int igemm_p(const IgemmArgs& g, hipStream_t st, int cin_alg = 0) {
    const double taps = (double)g.ksz * g.ksz, cin = cin_alg ? cin_alg : g.Cin;
    const double in_pix = (double)g.nfr * g.Hs * g.Ws;
    const double nz = g.zcount > 1 ? g.zcount : 1;
    // algorithmic bytes: input once, output once (+ residual), weights once -- and, for a skip convolution that also writes the ResBlock's
    // GroupNorm + SiLU image from the A rows it stages (IgemmArgs::side: one more tensor of the input's size written by this launch, the
    // pass affine_act would otherwise be), that image: counted since r05 (round 4's figure omitted it and read as 2x traffic waste)
    const double bytes = nz * 4.0 * (in_pix * cin + (double)g.M * g.Cout * (g.res ? 2 : 1) + taps * cin * g.Cout + (g.side ? in_pix * cin : 0.0));
    const IgemmArgs one = igemm_first_launch(g);      // a big window goes out as several launches over frame ranges (igemm.hip)
    const IgemmKernel k = igemm_kernel(one);
    const bool wino = k == IK_R64_UPS || k == IK_Z128 || k == IK_R64 || k == IK_WINO;
    const int tile = igemm_tile_class(igemm_sel_M(one), g.Cout);
    int cls;
    switch (k) {
        case IK_R64_UPS: cls = PC_CONV_WINO_R64_UPS; break;
        case IK_Z128: cls = PC_CONV_WINO_Z128; break;
        case IK_R64: cls = PC_CONV_WINO_R64; break;
        case IK_WINO: cls = PC_CONV_WINO; break;
        case IK_SPLIT: cls = gemm_split_tile_class(igemm_sel_M(one), g.Cout) == 4 ? (int)PC_IGEMM_128x192 : tile; break;
        default: cls = tile + (g.ksz == 3 ? (int)PC_CONV_128x128 : 0);        // gemm_frag (1x1) | the generic kernel
    }
    char tag[56];
    snprintf(tag, sizeof(tag), "M=%d N=%d K=%d k%d s%d%s%s%s", g.M, g.Cout, g.Cin, g.ksz, g.stride, g.ups ? " ups" : "",
             g.affA ? " pro" : (g.act ? " act" : ""), g.res ? " res" : "");
    VD_REQUIRE(g.stats == nullptr || wino || (k == IK_SPLIT && g.stats_hw > 0),
               "GroupNorm partial sums requested from a kernel that has no such epilogue");
    ProfScope ps(cls, nz * 2.0 * g.M * g.Cout * cin * taps, bytes, st, tag);
    return launch_igemm(g, st);
}

static int affine_act(const float* src0, const float* src1, int C0, int C, const float* A, const float* B, int N, int HW,
                      float* y, hipStream_t st) {
    ProfScope ps(PC_ELEMENTWISE, 0.0, 8.0 * N * HW * C, st);
    return launch_affine_act(src0, src1, C0, C, A, B, N, HW, 1, y, st);
}

// FreeU for one forward (vd_set_freeu): the constants of the two stages, the cos / sin table of each stage's side, and the engine's
// buffers the modified halves of a concat go to -- one pair for every block: a block's kernels have read them before the next block's
// FreeU passes write them (one stream)
struct FreeUReq {
    double b[2], s[2];
    int adaptive;
    const double* trig[2];
    float *yh, *ys;                  // h' and skip'
    double* map;                     // the adaptive form's structure map, [N][S*S]
    double *ph, *ps;                 // GroupNorm partial sums of h' and skip' ([N][gn_stats_split][C][2]): handed on as Tens::part
};

struct FwdIn {
    int B, T;
    const float *x, *obs_src, *obs, *lat, *km, *t_model;
    const int64_t* fidx;
    int obs_mode;
    float* eps;
    const FreeUReq* fu = nullptr;    // null: the plain forward
};

// Window prefix cache (vd_window_begin, opt-in).  The input blocks before the first attention layer treat frames as
// independent batch entries, and in 'x_0' mode an observed frame's network input (its x0 pixels, the indicator channels, the
// timestep 0 embedding) does not change over the steps of a window: its activations there are computed once per window.
// A forward with a plan runs those blocks on the `n` listed frames only (a compact batch), scatters every block output --
// and its GroupNorm partial sums -- into a persistent full-size tensor that already holds the other frames' rows, and
// carries on from there with the full batch.
struct PrefixStore { std::vector<float*> tens; std::vector<double*> parts; std::vector<size_t> floats; };
struct PrefixPlan {
    int n = 0;                       // frames in the list
    const int* list = nullptr;       // device: compact index -> frame
    bool build_only = false;         // stop behind the prefix (the once-per-window pass over the observed frames)
    PrefixStore* store = nullptr;
};

// Window suffix skip (vd_window_begin, opt-in).  Behind the LAST attention layer the network treats frames as independent batch
// entries again (ResBlocks, Upsample, the output head: unet.py:820-839), and the caller keeps only the latent frames of a window
// (scripts/video_sample.py:170-186) while an observed frame's sample is replaced by the observation before the network sees it
// again (unet.py:958-983, modes 'x_0' and 'x_t_minus_1').  A forward with this plan gathers the `n` listed frames (every frame
// that is not a pure observation) out of the last attention layer's output and out of each skip tensor the remaining decoder
// blocks read -- rows and GroupNorm partial sums -- runs those blocks and the head on the compact batch, and scatters eps
// into a zeroed full-size tensor.  Kernel variants are chosen for the full frame count (IgemmArgs::nfr_sel): the listed frames'
// eps are those of the full forward, bit for bit.
struct SuffixPlan { int n = 0; const int* list = nullptr; };

static inline int out_t_cols(int Cout) { return (9 * Cout + 31) / 32 * 32; }       // columns of the head's (cout, tap) GEMM

// frames a layer call stands for when it runs on a part of them (conv_args -> IgemmArgs::nfr_sel); set around the compact suffix
static thread_local int g_sel_nfr = 0;

}  // namespace vd

using namespace vd;

struct vd_engine {
    vd_config cfg;
    int E = 0;                       // time_embed_dim
    std::vector<Param> params;
    std::unordered_map<std::string, int> pidx;
    std::vector<ResP> res;
    std::vector<AttnP> attn;
    std::vector<ConvP> convs;        // stem / down / up
    std::vector<std::vector<Layer>> input_blocks, output_blocks;
    std::vector<Layer> middle;
    int n_before_attn = 0, pos_res = 0, pos_ch = 0, final_ch = 0;
    int suf_blk = -2, suf_layer = -1;   // last attention layer: output block (-1: none in the decoder, the suffix starts at block 0) and layer in it
    int p_posenc = -1, p_te0w, p_te0b, p_te2w, p_te2b, p_outgw, p_outgb, p_outw, p_outb;
    size_t film_w_off = 0, film_b_off = 0, te_w_off = 0, te_b_off = 0;
    int film_total = 0, te_total = 0;
    size_t packed_total = 0;
    float* wbuf = nullptr;           // caller-owned packed weights
    bool wbuf_on_host = false;       // vd_set_weight_storage_host: the packed image is assembled in host memory
    int put(void* dst, const void* src, size_t bytes) {
        if (wbuf_on_host) { std::memcpy(dst, src, bytes); return 0; }
        VD_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    // rpe_all: the relative-position nets of ALL attention blocks at the start of a forward, two launches per channel width instead of two
    // per block (they depend on the timestep embedding and the frame indices only, unet.py:283-298).  Per width: the blocks of that width,
    // a device table of offsets (rpe_hidden: te column, Wd, bd; output layer: weight image, bias) and where the blocks' R tensors land.
    struct RpeGroup { int C; std::vector<int> blocks; long long* d_hid = nullptr; long long* d_out = nullptr; };
    std::vector<RpeGroup> rpe_groups;
    std::vector<float*> rpe_R;        // [attention block][3]: R of the running forward (k, q, v order of attn_block), or empty
    int rpe_all(const float* te, const int64_t* fidx, int B, int T, hipStream_t st, Arena& ar);
    int rpe_tables();
    void rpe_group_blocks();
    // small device tables
    float* d_freq_time = nullptr; int n_freq_time = 0;
    float* d_freq_frame = nullptr; int n_freq_frame = 0;
    float* d_tab = nullptr; int num_timesteps = 0;
    float* d_tmap = nullptr; float rescale = 1.f;
    float* d_w2m = nullptr;           // [num_timesteps] dpmpp_2m extrapolation weights of the bound schedule (vd_set_multistep_weights), or null
    float* d_unipc = nullptr;         // [UNIPC_ROWS][num_timesteps] unipc_sample's coefficient rows of the bound schedule (vd_set_unipc_rows), or null
    float* d_jump = nullptr;          // [2][num_timesteps] sqrt(1 - beta) | sqrt(beta) of the bound schedule (vd_set_jump_rows), or null
    // workspace: activations of one (B, T) window [0, ws_tail), then the step's tail: t_model [B] (256-byte rounded), the eps scratch,
    // a second scratch of its size for the unconditional output of a cfg step (cfg_scale != 1) -- dead behind the combine pass, it then holds
    // the finished x_0 of a dynamic-threshold step -- and the scratch of the two guidance passes (guidance.hip)
    char* ws = nullptr; size_t ws_cap = 0;
    bool ws_suf = false;
    int ws_B = 0, ws_T = 0; size_t ws_tail = 0;      // the window shape ws_tail was computed for (dry run of the topology)
    std::unordered_map<long long, size_t> ws_peaks;  // (B << 32 | T) -> arena peak
    static size_t tm_bytes(int B) { return ((size_t)B * sizeof(float) + 255) & ~(size_t)255; }
    size_t out_floats(int B, int T) const { return (size_t)B * T * (cfg.learn_sigma ? 6 : 3) * cfg.image_size * cfg.image_size; }
    size_t guid_off(int B, int T) const { return (tm_bytes(B) + 2 * out_floats(B, T) * sizeof(float) + 255) & ~(size_t)255; }
    size_t step_tail_bytes(int B, int T) const { return guid_off(B, T) + guidance_scratch_bytes(B); }
    float* step_tm() const { return reinterpret_cast<float*>(ws + ws_tail); }
    float* step_eps(int B) const { return reinterpret_cast<float*>(ws + ws_tail + tm_bytes(B)); }
    float* step_eps_u(int B, int T) const { return step_eps(B) + out_floats(B, T); }      // out_u of a cfg step
    void* step_guid(int B, int T) const { return ws + ws_tail + guid_off(B, T); }      // ws_tail is 256-byte rounded, hipMalloc's base more
    Arena step_arena() const { Arena a; a.base = ws; a.cap = ws_tail; return a; }     // the activations end where the tail begins
    // ---- use_gradient_method: second packed image (backward-data weights) + the tape of the guided step's forward
    float* wbuf_bwd = nullptr; bool wbuf_bwd_on_host = false; size_t packed_bwd_total = 0;
    Tape* tape = nullptr;
    // ---- loss guidance (vd_guide_begin / vd_guide_finish): the one taped pass that outlives a C call.  Its tape points into the arena and
    // its eps lies in DiffWs's tail, so it is good only while nothing else has touched the workspace or set a tape: forward(), backward(),
    // grow_ws() and vd_window_run() -- every path to the workspace -- open with drop_held(), as do the setters of what the finish reads.
    struct HeldPass {
        Tape tape; FwdIn fi; Arena ar;       // ar: where the forward left the arena, the mark the backward goes on from
        int B, T, clip; const long long* t;
        unsigned long long ticket;
    };
    std::unique_ptr<HeldPass> held;
    unsigned long long guide_seq = 0;        // tickets handed out so far (a ticket is never 0)
    unsigned long long guide_end_ticket = 0; const char* guide_end_why = "";      // how the last held pass ended
    void end_held(const char* why) {
        if (!held) return;
        guide_end_ticket = held->ticket; guide_end_why = why;
        held.reset();
    }
    void drop_held() { end_held("dropped by an engine call in between: one that runs the network, sizes the workspace or replays a window graph"); }
    // return_attn_weights: device buffers for the next forward, one pair per attention block in execution order
    std::vector<float*> attn_cap_t, attn_cap_s;
    int attn_seq = 0;
    // cfg_scale (vd_set_cfg_scale): 1 = off.  Any other value: every step runs a second forward with the all-zero observation mask below
    // and cfg_combine_kernel in front of its sampler pass
    float cfg_w = 1.f;
    float* d_cfg_zero = nullptr; size_t cfg_zero_cap = 0;   // [B*T] zeros: the observation mask of the unconditional forward
    // guidance rescale (vd_set_guidance_rescale; 0 = off; acts with cfg_w != 1) and dynamic thresholding (vd_set_dynamic_threshold; 0 = off;
    // acts with clip_denoised, whose clamp it replaces): engine state like cfg_w, part of a window graph's key
    float guid_phi = 0.f, dyn_p = 0.f;
    // FreeU (vd_set_freeu; all four constants 1 = off): in front of every output block of the two lowest-resolution decoder levels the
    // backbone half of the concat is scaled by b and the skip half filtered by s (freeu.hip), stage 1 = level 0.  fu_blk: per such block
    // the side and the channels of h and of the skip (build()); d_fu_trig: the cos / sin tables of the two sides, uploaded once by the
    // first vd_set_freeu that switches it on; d_fu: h', skip' and the structure map of one block (freeu_workspace), whose addresses a
    // captured window graph holds.  Engine state like cfg_w, part of a window graph's key.
    double fu_b[2] = {1.0, 1.0}, fu_s[2] = {1.0, 1.0};
    int fu_adaptive = 0;
    struct FuBlk { int S, Ch, Cs; };
    std::vector<FuBlk> fu_blk;
    int fu_per_stage = 0;
    double* d_fu_trig = nullptr;
    float* d_fu = nullptr; size_t fu_cap = 0;
    bool freeu_on() const { return fu_b[0] != 1.0 || fu_b[1] != 1.0 || fu_s[0] != 1.0 || fu_s[1] != 1.0; }
    // floats of d_fu's five parts for N frames, each the largest any block of the two stages needs, rounded to 256 bytes: h', skip', the
    // map, and the two statistics tables (doubles: two floats each)
    struct FuSizes { size_t nh = 0, ns = 0, nm = 0, nph = 0, nps = 0; size_t total() const { return nh + ns + nm + nph + nps; } };
    FuSizes freeu_floats(int N) const {
        FuSizes z;
        for (const FuBlk& k : fu_blk) {
            const int hw = k.S * k.S;
            z.nh = std::max(z.nh, (size_t)N * hw * k.Ch); z.ns = std::max(z.ns, (size_t)N * hw * k.Cs); z.nm = std::max(z.nm, 2 * (size_t)N * hw);
            z.nph = std::max(z.nph, 4 * (size_t)N * gn_stats_split(N, hw, k.Ch) * k.Ch);
            z.nps = std::max(z.nps, 4 * (size_t)N * gn_stats_split(N, hw, k.Cs) * k.Cs);
        }
        for (size_t* v : {&z.nh, &z.ns, &z.nm, &z.nph, &z.nps}) *v = (*v + 63) & ~(size_t)63;
        return z;
    }
    int freeu_workspace(int B, int T) {              // never inside a capture
        return grow(d_fu, fu_cap, freeu_floats(B * T).total(), true);
    }
    // the request of a (B, T) forward under the constants handed in (the engine's, or a window graph's key)
    int freeu_request(int B, int T, const double* b, const double* s, int adaptive, FreeUReq* q) const {
        const FuSizes z = freeu_floats(B * T);
        VD_REQUIRE(d_fu && fu_cap >= z.total() && d_fu_trig, "FreeU: buffers not sized (vd_set_freeu, then a step entry or vd_window_begin)");
        float* p = d_fu + z.nh + z.ns;
        *q = FreeUReq{{b[0], b[1]}, {s[0], s[1]}, adaptive, {d_fu_trig, d_fu_trig + 2 * (size_t)fu_blk.front().S},
                      d_fu, d_fu + z.nh, reinterpret_cast<double*>(p), reinterpret_cast<double*>(p + z.nm),
                      reinterpret_cast<double*>(p + z.nm + z.nph)};
        return 0;
    }
    // known region (vd_set_known_region; null = off): every sampling step ends in the merge pass of known.hip on its sample.  The caller's
    // tensors; a window graph's key carries the two addresses.  known_noise / seed / offset: the draws of the eager entries.
    const float *known_src = nullptr, *known_mask = nullptr, *known_noise = nullptr;
    unsigned long long known_seed = 0, known_offset = 0;
    // measurement (vd_set_measurement; null = off): the x_0 prediction of every step is projected onto it (measure.hip) before the sampler
    // pass reads it.  The caller's tensor; a window graph's key carries the address, the scale and the gray flag.
    const float* meas_y = nullptr;
    int meas_scale = 1, meas_gray = 0;
    // particle steering (vd_set_particles; part_K <= 1 = off): the batch is G groups of part_K particles; behind a step the caller hands
    // the items' rewards to vd_particle_apply, which updates the state below and resamples the caller's tensors (particles.hip).
    // part_B, part_state_K: the batch and the group size vd_particle_reset (or vd_window_begin) last zeroed the state for; the state outlives
    // vd_set_particles, so that it can be read behind a window whose begin() has restored the engine's setting.
    int part_K = 0, part_B = 0, part_state_K = 0;
    double part_lambda = 0.0, part_tau = 0.0;
    // the built-in reward (null: the rewards come through vd_particle_apply): r_b = -||y - A x_0||^2 / (2 sigma^2) on item b's latent
    // frames, for the cell-mean operators of measure.hip; the caller's tensor, like meas_y
    const float* part_y = nullptr;
    int part_scale = 1, part_gray = 0;
    double part_sigma = 0.0;
    // the blur kernel (vd_set_blur_kernel; blur_k 0: none): k x k taps in an engine-owned buffer of kMaxBlurTaps^2 floats whose address never
    // changes, so a window graph that reads it follows a change of taps at equal k.  part_blur (vd_set_particle_blur): the built-in
    // reward's operator is this kernel (blur.hip), y has the video's shape, and part_scale / part_gray are not read.
    float* d_blur_taps = nullptr;
    int blur_k = 0, part_blur = 0;
    // the separable linear operator (vd_set_linear_operator; lin_Mh 0: none): A_h, A_w, P_h, P_w in four engine-owned slots of
    // kMaxLinopSide^2 floats whose addresses never change, so a window graph that reads them follows new matrices of equal shape.
    // lin_back: P_h and P_w were handed in.  lin_y (vd_set_linear_measurement; null = off): the x_0 prediction of every step is projected
    // onto it (linop.hip) in the place of meas_y; the caller's tensor.  d_lin_r: the residual between the projection's two passes.
    // part_lin (vd_set_particle_linear): the built-in reward's operator is this one, y is [B][T][3][Mh][Mw].
    float* d_lin_mats = nullptr;
    int lin_Mh = 0, lin_Mw = 0, lin_back = 0, part_lin = 0;
    const float* lin_y = nullptr;
    float* d_lin_r = nullptr; size_t lin_r_cap = 0;
    const float* lin_mat(int i) const { return d_lin_mats + (size_t)i * kMaxLinopSide * kMaxLinopSide; }      // 0 A_h, 1 A_w, 2 P_h, 3 P_w
    double *d_part_logw = nullptr, *d_part_rprev = nullptr, *d_part_ess = nullptr;
    int *d_part_anc = nullptr, *d_part_chosen = nullptr;
    long long* d_part_counters = nullptr;
    size_t part_state_cap = 0;
    float* d_part_scratch = nullptr; size_t part_scratch_cap = 0;
    // ... of the built-in reward: the residual pass's r and partials, the x_0 prediction of a window whose sampler keeps none, and the
    // selector rows [2][num_timesteps] that make dps_residual_kernel's x_0 head read the sample at t == 0 and pred_xstart elsewhere
    float* d_part_r = nullptr; size_t part_r_cap = 0;
    double* d_part_partials = nullptr; size_t part_partials_cap = 0;
    float* d_part_x0 = nullptr; size_t part_x0_cap = 0;
    float* d_part_sel = nullptr; size_t part_sel_cap = 0; int part_sel_nt = 0;
    // the uniforms of the eager steps (vd_particle_draws): a device tensor [G][2], or Philox at (part_seed, part_offset) like a window's
    const double* part_uni = nullptr;
    unsigned long long part_seed = 0, part_offset = 0;
    bool part_draws_set = false;
    int mean_type = 0;                              // what the network's output IS: 0 eps (ModelMeanType.EPSILON), 1 x_0 (START_X)
    int* d_err = nullptr;                            // sticky device flags: bit 0 = timestep index out of range, bit 1 = network output not finite
    int device = -1;
    double* d_part = nullptr; size_t part_cap = 0;   // NLL partial sums
    // vd_score_windows: x_t of the scored batch, the device list of its latent frames (suffix plan) and the host copies around it
    float* d_score_xt = nullptr; size_t score_xt_cap = 0;
    int* d_score_list = nullptr; size_t score_list_cap = 0;
    std::vector<float> score_mask_h; std::vector<int> score_list_h;
    // ---- window executor (vd_window_*): device-resident step state + one captured graph per window signature
    struct WinKey {                  // the arguments of vd_window_begin a captured step depends on (zero-filled: compared bytewise)
        int B, T, obs_mode, sampler, clip, flags; float eta;      // flags: 1 prefix cache, 2 suffix skip
        float cfg_w;                                              // cfg_scale: a graph holds one forward (1) or two and the combine pass with this weight
        float guid_phi, dyn_p;                                    // guidance rescale / dynamic threshold: the passes a graph holds and their constants
        float* x; const float *obs_src, *obs, *lat, *km; const long long* fidx;
        const float *known_src, *known_mask;                      // known region: the merge pass a graph ends in reads them (null: none)
        const float* meas_y; int meas_scale, meas_gray;           // measurement: the projection pass a graph holds reads y (null: none)
        const float* part_y; int part_K, part_scale, part_gray;   // particle steering: the three passes a graph ends in and their constants (part_K 0: none)
        double part_lambda, part_tau, part_sigma;
        int part_blur_k;                                          // ... with the blur kernel as the reward's operator: its size (0: the cell mean); the taps' address is fixed
        int part_lin_Mh, part_lin_Mw;                             // ... with the linear operator as the reward's operator: y's sides (0: not); the matrices' addresses are fixed
        const float* lin_y; int lin_Mh, lin_Mw;                   // linear measurement: the two projection passes a graph holds read y (null: none)
        double fu_b[2], fu_s[2]; int fu_on, fu_adaptive;          // FreeU: the passes a graph's forwards hold and their constants (fu_on 0: none, all zero)
        bool operator==(const WinKey& o) const { return std::memcmp(this, &o, sizeof(WinKey)) == 0; }
    };
    struct WinGraph {
        WinKey key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        // window prefix cache: which frames are step-invariant (part of the signature: the compact batch size is baked into the
        // captured launches), the two device lists and the persistent tensors the captured step reads and writes
        std::vector<unsigned char> inv; int n_inv = 0, n_suf = 0;   // n_suf: frames the suffix runs on (0: all of them)
        int* d_lists = nullptr;                  // [n_act active frames | n_inv invariant frames]
        PrefixStore* store = nullptr;
        void release() {             // everything the graph owns; a graph the executor's stream may still run is drained first by the caller
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            if (d_lists) (void)hipFree(d_lists);
            if (store) { for (float* p : store->tens) if (p) (void)hipFree(p); for (double* p : store->parts) if (p) (void)hipFree(p); delete store; }
            exec = nullptr; graph = nullptr; d_lists = nullptr; store = nullptr;
        }
    };
    bool prefix_cache_on = false;                // vd_set_window_prefix_cache
    bool suffix_skip_on = false;                 // vd_set_window_suffix_skip
    std::vector<WinGraph> win_graphs;
    int win_cur = -1;
    bool win_lost = false;                               // the armed window's graph was dropped (workspace growth / new schedule)
    unsigned long long win_gen = 0;                      // bumped by every vd_window_begin: a run must name the window it continues
    long long win_left = 0;                              // steps the current window still has (t + 1; walking up: num_timesteps - t)
    long long* d_win_t = nullptr; size_t win_t_cap = 0;  // [B] current respaced index of the window
    float* d_win_xtm1 = nullptr; size_t win_xtm1_cap = 0; // 'x_t_minus_1' windows: the observed frames re-noised to t - 1, redrawn every step
    unsigned long long* d_win_rng = nullptr;             // {seed, Philox offset, steps the armed window has done}
    float* d_win_hist = nullptr; size_t win_hist_cap = 0; // samplers with history (dpmpp_2m, dpmpp_2m_sde): the previous step's x_0 prediction, updated in place by the pass
                                                          // (unipc: D_{t+1}, beside the two below)
    float* d_win_ubase = nullptr; size_t win_ubase_cap = 0; // unipc windows: the corrected state x^c_{t+1} ...
    float* d_win_ud2 = nullptr; size_t win_ud2_cap = 0;     // ... and D_{t+2}; all three updated in place by the pass

    ~vd_engine() {
        if (d_freq_time) (void)hipFree(d_freq_time);
        if (d_freq_frame) (void)hipFree(d_freq_frame);
        for (auto& g : rpe_groups) { if (g.d_hid) (void)hipFree(g.d_hid); if (g.d_out) (void)hipFree(g.d_out); }
        if (d_tab) (void)hipFree(d_tab);
        if (d_tmap) (void)hipFree(d_tmap);
        if (ws) (void)hipFree(ws);
        if (d_err) (void)hipFree(d_err);
        if (d_part) (void)hipFree(d_part);
        if (d_score_xt) (void)hipFree(d_score_xt);
        if (d_score_list) (void)hipFree(d_score_list);
        if (d_win_t) (void)hipFree(d_win_t);
        if (d_win_rng) (void)hipFree(d_win_rng);
        if (d_win_xtm1) (void)hipFree(d_win_xtm1);
        if (d_win_hist) (void)hipFree(d_win_hist);
        if (d_win_ubase) (void)hipFree(d_win_ubase);
        if (d_win_ud2) (void)hipFree(d_win_ud2);
        if (d_w2m) (void)hipFree(d_w2m);
        if (d_unipc) (void)hipFree(d_unipc);
        if (d_jump) (void)hipFree(d_jump);
        if (d_cfg_zero) (void)hipFree(d_cfg_zero);
        if (d_fu_trig) (void)hipFree(d_fu_trig);
        if (d_fu) (void)hipFree(d_fu);
        for (void* p : {(void*)d_part_logw, (void*)d_part_rprev, (void*)d_part_ess, (void*)d_part_anc, (void*)d_part_chosen,
                        (void*)d_part_counters, (void*)d_part_scratch, (void*)d_part_r, (void*)d_part_partials, (void*)d_part_x0,
                        (void*)d_part_sel, (void*)d_blur_taps, (void*)d_lin_mats, (void*)d_lin_r})
            if (p) (void)hipFree(p);
        for (auto& g : win_graphs) g.release();
    }

    // Captured window graphs bake addresses (workspace, schedule tables, step counters) and values (num_timesteps, rescale)
    // into their kernel arguments: whatever replaces one of those drops every graph first.  A graph may still be queued on
    // the executor's stream, so the device is drained before an exec is destroyed.
    void drop_window_graphs() {
        if (win_graphs.empty()) { win_cur = -1; return; }
        (void)hipDeviceSynchronize();
        for (auto& g : win_graphs) g.release();
        win_graphs.clear();
        win_cur = -1;
    }
    // Grow the device buffer p to at least n elements (contents not kept).  With held_by_graphs, captured window graphs point into
    // it: they are dropped before it moves (a window in flight is lost: vd_window_run then reports "window graphs invalidated").
    template <class Tp> int grow(Tp*& p, size_t& cap, size_t n, bool held_by_graphs) {
        if (n <= cap) return 0;
        if (held_by_graphs && p) { if (win_cur >= 0) win_lost = true; drop_window_graphs(); }
        if (p) VD_HIP(hipFree(p));
        p = nullptr; cap = 0;
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(Tp)));
        cap = n;
        return 0;
    }
    // The workspace of a window shape: the arena peak of its dry run (cached under `key`: the run walks the whole topology),
    // 256-byte rounded into *tail, plus `extra` bytes of the caller's own buffers behind it
    template <class DryRun> int grow_ws(long long key, size_t extra, DryRun dry_run, size_t* tail) {
        drop_held();
        if (int rc = rpe_tables()) return rc;
        auto it = ws_peaks.find(key);
        if (it == ws_peaks.end()) {
            size_t peak = 0;
            if (int rc = dry_run(&peak)) return rc;
            it = ws_peaks.emplace(key, peak).first;
        }
        *tail = (it->second + 255) & ~(size_t)255;
        return grow(ws, ws_cap, *tail + extra, true);
    }

    const float* W(int p) const { return wbuf + params[p].off; }
    void set_w(vd::IgemmArgs& g, int p) const {
        const int k = params[p].kind;
        g.w = g.wfrag = g.wwino = nullptr;
        if (k == PK_CONV3W) { g.wwino = W(p); g.wsplit = split_math() ? 2 : 0; }
        else if (k == PK_CONV3WU) { g.wwino = W(p); g.wsplit = 2; g.ups_phase = 1; }
        else if (k == PK_CONV3S) { g.wfrag = W(p); g.wsplit = 1; }
        else if (k == PK_LINF) { g.wfrag = W(p); g.wsplit = split_math(); }
        else g.w = W(p);
    }

    int add(const std::string& name, std::initializer_list<long long> shape, int kind = PK_RAW) {
        Param p;
        p.name = name;
        p.nd = (int)shape.size();
        int i = 0;
        p.numel = 1;
        for (long long s : shape) { p.shape[i++] = s; p.numel *= (size_t)s; }
        p.kind = kind;
        p.packed = p.numel;
        // split images: three 16-bit pieces per weight + the trailer of per-output scales (2 floats per output; split_pack.hip)
        const size_t O = (size_t)p.shape[0];
        if (kind == PK_STEM) p.packed = O * STEM_KPAD;
        if ((kind == PK_STEM || kind == PK_LINF) && split_math()) p.packed = p.packed * 3 / 2 + 2 * O;
        if (kind == PK_CONV3S) p.packed = p.numel * 3 / 2 + 2 * O;
        if (kind == PK_CONV3W) p.packed = split_math() ? (size_t)16 * O * p.shape[1] * 3 / 2 + 2 * O : (size_t)16 * O * p.shape[1];
        if (kind == PK_CONV3WU) p.packed = (size_t)4 * 16 * O * p.shape[1] * 3 / 2 + 8 * O;
        // output head: [tap][O][I] (out_conv_bwd, the op entry point) + [out_t_cols(O)][I], rows co * 9 + tap: the head as a 1x1 GEMM over
        // (cout, tap) columns followed by a 9-tap gather (misc.hip: out_gather_kernel)
        if (kind == PK_OUTCONV) p.packed = p.numel + (size_t)out_t_cols((int)O) * p.shape[1];
        params.push_back(p);
        pidx[name] = (int)params.size() - 1;
        return (int)params.size() - 1;
    }

    int build();
    int forward(const FwdIn& in, hipStream_t st, Arena& ar, const PrefixPlan* pp = nullptr, const SuffixPlan* sp = nullptr);
    int ensure_ws(int B, int T, bool suffix_plan = false);
    int res_block(const ResP& r, Tens x0, const Tens* x1, int N, const float* film_all, hipStream_t st, Arena& ar, Tens* out);
    int attn_block(const AttnP& a, Tens x, int B, int T, const int64_t* fidx, const float* amask,
                   hipStream_t st, Arena& ar, Tens* out);
    int gn_fold(const Tens& x0, const Tens* x1, int N, int gw, int gb, const float* film,
                int film_ld, hipStream_t st, Arena& ar, float** A, float** B, float** mr = nullptr);
    int gn_act(const Tens& x0, const Tens* x1, int N, int gw, int gb, const float* film, int film_ld, int act, float* y,
               hipStream_t st, Arena& ar);
    int backward(const FwdIn& in, const float* deps, float* dx, hipStream_t st, Arena& ar);
    int bwd_linear(const float* dy, int M, int pw, const float* res, float* out, hipStream_t st);
    int bwd_conv3(Tens dy, int N, int pw, int cout_bwd, const float* res, float* out, hipStream_t st, Arena& ar);
    int ensure_ws_guided(int B, int T);
    const float* WB(int p) const { return wbuf_bwd + params[p].off_bwd; }
    int linear(const float* a, int M, int K, int Nout, const float* wptr, const float* bptr, int act,
               const float* res, float* out, hipStream_t st, const Tens* stats_of = nullptr);
    void gemm_stats_table(Arena& ar, int M, int K, int Nout, Tens* t);
    void conv_split_stats_table(Arena& ar, const IgemmArgs& conv, int Cout, Tens* t);
};

// ------------------------------------------------------------------------------------------ topology
int vd_engine::build() {
    const int mc = cfg.num_channels, nrb = cfg.num_res_blocks;
    const int* mult; int nlev;
    switch (cfg.image_size) {
        case 256: mult = CH_MULT_256; nlev = 6; break;
        case 128: mult = CH_MULT_128; nlev = 5; break;
        case 64: mult = CH_MULT_64; nlev = 4; break;
        case 32: mult = CH_MULT_32; nlev = 4; break;
        default: set_error("unsupported image size: " + std::to_string(cfg.image_size)); return -1;
    }
    VD_REQUIRE(mc % 32 == 0, "num_channels must be a multiple of 32 (GroupNorm32)");
    VD_REQUIRE(cfg.num_heads > 0 && cfg.n_attention_ds >= 0 && cfg.n_attention_ds <= 8, "heads / attention_ds");
    E = mc * (cfg.time_embed_mult > 0 ? cfg.time_embed_mult : 4);
    auto in_att = [&](int ds) { for (int i = 0; i < cfg.n_attention_ds; ++i) if (cfg.attention_ds[i] == ds) return true; return false; };

    // The reference registers spatial_encoding first (a Parameter of the root module), but its shape is
    // known only after the input blocks are laid out; reserve the slot now.
    if (cfg.use_spatial_encoding) p_posenc = add("spatial_encoding", {1, 1, 1, 1}, PK_POSENC);
    p_te0w = add("time_embed.0.weight", {E, mc}, PK_LINF); p_te0b = add("time_embed.0.bias", {E});
    p_te2w = add("time_embed.2.weight", {E, E}, PK_LINF); p_te2b = add("time_embed.2.bias", {E});

    // 3x3 stride-1 convs at >= 8x8 with a multiple of 64 couts run as Winograd F(2x2,3x3); the rest on the generic kernel
    auto k3 = [&](int res_out, int cout) { return res_out >= 8 && cout % 64 == 0 ? (int)PK_CONV3W : (int)PK_CONV3; };
    // backward-data image of a 3x3 stride-1 conv with `co` outputs (= the forward's inputs) and `ci` inputs at resolution rs
    auto k3b = [&](int rs, int co, int ci) {
        return rs >= 8 && (rs & (rs - 1)) == 0 && co % 64 == 0 && ci % 32 == 0 && split_math() ? (int)PK_CONV3W : (int)PK_CONV3;
    };
    auto bwd3 = [&](int p, int rs) { params[p].kind_bwd = k3b(rs, (int)params[p].shape[1], (int)params[p].shape[0]); };
    auto bwdl = [&](int p) { params[p].kind_bwd = PK_LINF; };
    // The envelope: what no launch could serve is refused at the end of build(), by parameter, layer and limit, with the launchers'
    // own constant (kGnMaxChannels) and predicates (attn_temporal_variant at T = 1, attn_spatial_variant) -- not at the first
    // forward.  The first offending layer per parameter is named; the layout goes on so that both are found.
    std::string bad_width, bad_heads;
    auto gn_fits = [&](const std::string& layer, int C, int skip) {
        if (C <= kGnMaxChannels || !bad_width.empty()) return;
        bad_width = "num_channels=" + std::to_string(mc) + ": " + layer + " normalises " + std::to_string(C) + " channels" +
                    (skip ? " (" + std::to_string(C - skip) + " + " + std::to_string(skip) + " of the skip connection)" : std::string()) +
                    "; GroupNorm32 serves at most " + std::to_string(kGnMaxChannels) + " (vd_gn_max_channels)";
    };
    auto add_res = [&](const std::string& pre, int cin, int cout, int rs, int skip = 0) {
        gn_fits(pre + ".in_layers.0", cin, skip); gn_fits(pre + ".out_layers.0", cout, 0);
        ResP r; r.cin = cin; r.cout = cout;
        r.gn1w = add(pre + ".in_layers.0.weight", {cin}); r.gn1b = add(pre + ".in_layers.0.bias", {cin});
        r.c1w = add(pre + ".in_layers.2.weight", {cout, cin, 3, 3}, k3(rs, cout)); r.c1b = add(pre + ".in_layers.2.bias", {cout});
        const int eo = cfg.use_scale_shift_norm ? 2 * cout : cout;
        r.embw = add(pre + ".emb_layers.1.weight", {eo, E}, PK_LINF); r.embb = add(pre + ".emb_layers.1.bias", {eo});
        r.gn2w = add(pre + ".out_layers.0.weight", {cout}); r.gn2b = add(pre + ".out_layers.0.bias", {cout});
        r.c2w = add(pre + ".out_layers.3.weight", {cout, cout, 3, 3}, k3(rs, cout)); r.c2b = add(pre + ".out_layers.3.bias", {cout});
        if (cin != cout) {
            r.skw = add(pre + ".skip_connection.weight", {cout, cin, 1, 1}, PK_LINF); r.skb = add(pre + ".skip_connection.bias", {cout});
            bwdl(r.skw);
        }
        bwd3(r.c1w, rs); bwd3(r.c2w, rs);
        res.push_back(r);
        return (int)res.size() - 1;
    };
    auto add_att = [&](const std::string& pre, int C) {
        AttP a;
        a.qkvw = add(pre + ".qkv.weight", {3 * C, C}, PK_LINF); a.qkvb = add(pre + ".qkv.bias", {3 * C});
        a.projw = add(pre + ".proj_out.weight", {C, C}, PK_LINF); a.projb = add(pre + ".proj_out.bias", {C});
        a.normw = add(pre + ".norm.weight", {C}); a.normb = add(pre + ".norm.bias", {C});
        bwdl(a.qkvw); bwdl(a.projw);
        return a;
    };
    auto add_rpe = [&](const std::string& pre, int C) {
        RpeP r;
        if (cfg.use_rpe_net) {
            r.dw = add(pre + ".rpe_net.embed_distances.weight", {C, 3}); r.db = add(pre + ".rpe_net.embed_distances.bias", {C});
            r.tw = add(pre + ".rpe_net.embed_diffusion_time.weight", {C, E}, PK_LINF); r.tb = add(pre + ".rpe_net.embed_diffusion_time.bias", {C});
            r.ow = add(pre + ".rpe_net.out.weight", {C, C}, PK_LINF); r.ob = add(pre + ".rpe_net.out.bias", {C});
        } else {
            r.table = add(pre + ".lookup_table_weight", {2 * (long long)cfg.rp_beta + 1, cfg.num_heads, C / cfg.num_heads});
        }
        return r;
    };
    auto add_attn = [&](const std::string& pre, int C, int rs) {
        const int heads = cfg.num_heads, L = rs * rs;
        const std::string where = "num_heads=" + std::to_string(heads) + ": " + pre + " (" + std::to_string(C) + " channels at " + std::to_string(rs) + " x " +
                                  std::to_string(rs) + ", attention_resolutions " + std::to_string(rs) + ")";
        const AttnTemporalVariant tv = attn_temporal_variant(1, L, C, heads, true);
        const AttnSpatialVariant sv = attn_spatial_variant(L, C, heads);
        const bool t_no = tv.family == AttnTemporalVariant::kRefused;
        if (bad_heads.empty() && C % heads != 0)
            bad_heads = where + ": " + std::to_string(C) + " channels do not divide into " + std::to_string(heads) + " heads";
        else if (bad_heads.empty() && (t_no || sv.row < 0))
            bad_heads = where + " has head dim " + std::to_string(C / heads) + "; " +
                        (t_no ? std::string("temporal attention: ") + tv.why : std::string("spatial attention: ") + sv.why);
        gn_fits(pre + ".norm", C, 0);
        AttnP a; a.C = C;
        a.sp = add_att(pre + ".spatial_attention", C);
        a.tp = add_att(pre + ".temporal_attention", C);
        a.rq = add_rpe(pre + ".temporal_attention.rpe_q", C);
        a.rk = add_rpe(pre + ".temporal_attention.rpe_k", C);
        a.rv = add_rpe(pre + ".temporal_attention.rpe_v", C);
        attn.push_back(a);
        return (int)attn.size() - 1;
    };
    auto add_conv = [&](const std::string& pre, int cin, int cout, int kind, int rs_bwd) {
        ConvP c; c.c = cout;
        c.w = add(pre + ".weight", {cout, cin, 3, 3}, kind); c.b = add(pre + ".bias", {cout});
        if (kind == PK_STEM) params[c.w].kind_bwd = PK_LINF;          // [STEM_KPAD][cout]: dcols = dy * W
        else bwd3(c.w, rs_bwd);                                       // Down: a stride-1 conv of the zero-stuffed gradient at the INPUT resolution
        convs.push_back(c);
        return (int)convs.size() - 1;
    };

    std::vector<int> chans;
    VD_REQUIRE(cfg.cond_emb_type >= 0 && cfg.cond_emb_type <= 2, "cond_emb_type: 0 channel, 1 duplicate|all, 2 t=0");
    const int stem_in = cfg.cond_emb_type == 0 ? 5 : (cfg.cond_emb_type == 1 ? 6 : 3);         // unet.py:932-940
    input_blocks.push_back({Layer{0, add_conv("input_blocks.0.0", stem_in, mc, PK_STEM, cfg.image_size)}});
    chans.push_back(mc);
    int ch = mc, ds = 1, first_ds = -1, first_ch = -1;
    n_before_attn = -1;
    for (int lvl = 0; lvl < nlev; ++lvl) {
        for (int k = 0; k < nrb; ++k) {
            if (in_att(ds) && n_before_attn < 0) { n_before_attn = (int)input_blocks.size(); first_ds = ds; first_ch = ch; }
            const std::string pre = "input_blocks." + std::to_string(input_blocks.size());
            std::vector<Layer> blk;
            int ri = add_res(pre + ".0", ch, mult[lvl] * mc, cfg.image_size / ds);
            blk.push_back(Layer{1, ri});
            ch = mult[lvl] * mc;
            if (in_att(ds)) { int ai = add_attn(pre + ".1", ch, cfg.image_size / ds); if (ai < 0) return ai; blk.push_back(Layer{2, ai}); }
            input_blocks.push_back(blk);
            chans.push_back(ch);
        }
        if (lvl != nlev - 1) {
            const std::string pre = "input_blocks." + std::to_string(input_blocks.size());
            // Downsample (unet.py:98): stride-2 3x3 -> the split GEMM over an implicit im2col operand
            input_blocks.push_back({Layer{3, add_conv(pre + ".0.op", ch, ch, split_math() ? PK_CONV3S : PK_CONV3, cfg.image_size / ds)}});
            chans.push_back(ch);
            ds *= 2;
        }
    }
    if (n_before_attn < 0) { n_before_attn = (int)input_blocks.size(); first_ds = ds; first_ch = ch; }
    pos_res = cfg.image_size / first_ds; pos_ch = first_ch;
    if (p_posenc >= 0) {
        Param& p = params[p_posenc];
        p.nd = 4; p.shape[0] = 1; p.shape[1] = pos_ch; p.shape[2] = pos_res; p.shape[3] = pos_res;
        p.numel = p.packed = (size_t)pos_ch * pos_res * pos_res;
    }
    {
        int r0 = add_res("middle_block.0", ch, ch, cfg.image_size / ds);
        int a0 = add_attn("middle_block.1", ch, cfg.image_size / ds); if (a0 < 0) return a0;
        int r1 = add_res("middle_block.2", ch, ch, cfg.image_size / ds);
        middle = {Layer{1, r0}, Layer{2, a0}, Layer{1, r1}};
    }
    fu_blk.clear(); fu_per_stage = nrb + 1;
    for (int lvl = nlev - 1; lvl >= 0; --lvl) {
        for (int i = 0; i <= nrb; ++i) {
            const std::string pre = "output_blocks." + std::to_string(output_blocks.size());
            std::vector<Layer> blk;
            const int skip = chans.back(); chans.pop_back();
            if (lvl >= nlev - 2) fu_blk.push_back(FuBlk{cfg.image_size / ds, ch, skip});      // FreeU's two stages: the lowest two levels
            blk.push_back(Layer{1, add_res(pre + ".0", ch + skip, mc * mult[lvl], cfg.image_size / ds, skip)});
            ch = mc * mult[lvl];
            int li = 1;
            if (in_att(ds)) { int ai = add_attn(pre + "." + std::to_string(li++), ch, cfg.image_size / ds); if (ai < 0) return ai; blk.push_back(Layer{2, ai}); }
            if (lvl && i == nrb) {
                // Upsample + conv: the sub-pixel form where the split Winograd kernel serves the SOURCE map
                const int rs_src = cfg.image_size / ds;
                int kup = k3(2 * rs_src, ch);
                if (kup == PK_CONV3W && split_math() && rs_src >= 8 && (rs_src & (rs_src - 1)) == 0 && ch % 64 == 0) kup = PK_CONV3WU;
                blk.push_back(Layer{4, add_conv(pre + "." + std::to_string(li++) + ".conv", ch, ch, kup, 2 * rs_src)});
                ds /= 2;
            }
            output_blocks.push_back(blk);
        }
    }
    suf_blk = -1; suf_layer = -1;
    for (size_t i = 0; i < output_blocks.size(); ++i)
        for (size_t l = 0; l < output_blocks[i].size(); ++l)
            if (output_blocks[i][l].type == 2) { suf_blk = (int)i; suf_layer = (int)l; }
    if (!bad_width.empty() || !bad_heads.empty()) {
        set_error(bad_width + (!bad_width.empty() && !bad_heads.empty() ? ";  " : "") + bad_heads);
        return -1;
    }
    final_ch = ch;
    p_outgw = add("out.0.weight", {ch}); p_outgb = add("out.0.bias", {ch});
    const int oc = cfg.learn_sigma ? 6 : 3;                                                    // script_util.py:129-131
    p_outw = add("out.2.weight", {oc, mc, 3, 3}, PK_OUTCONV); p_outb = add("out.2.bias", {oc});
    VD_REQUIRE(final_ch == mc, "channel_mult[0] must be 1");

    // ---- packed layout: [FiLM weights | FiLM biases | rpe-time weights | rpe-time biases | everything else]
    size_t off = 0;
    auto place = [&](int p) { params[p].off = off; off += (params[p].packed + 3) & ~(size_t)3; };
    film_w_off = off; film_total = 0;
    for (auto& r : res) { r.film_off = film_total; place(r.embw); film_total += (int)params[r.embw].shape[0]; }
    film_b_off = off;
    for (auto& r : res) place(r.embb);
    te_total = 0;
    if (cfg.use_rpe_net) {
        te_w_off = off;
        for (auto& a : attn) for (RpeP* r : {&a.rq, &a.rk, &a.rv}) { r->te_off = te_total; place(r->tw); te_total += a.C; }
        te_b_off = off;
        for (auto& a : attn) for (RpeP* r : {&a.rq, &a.rk, &a.rv}) place(r->tb);
    }
    std::vector<char> placed(params.size(), 0);
    for (auto& r : res) { placed[r.embw] = placed[r.embb] = 1; }
    if (cfg.use_rpe_net) for (auto& a : attn) for (RpeP* r : {&a.rq, &a.rk, &a.rv}) { placed[r->tw] = placed[r->tb] = 1; }
    for (size_t i = 0; i < params.size(); ++i) if (!placed[i]) place((int)i);
    packed_total = off;
    // The batched projections are ONE fragment-major matrix each: members share the region base and own a row range.
    for (auto& r : res) { Param& p = params[r.embw]; p.off = film_w_off; p.frag_rows = film_total; p.frag_row0 = r.film_off; }
    if (cfg.use_rpe_net)
        for (auto& a : attn)
            for (RpeP* r : {&a.rq, &a.rk, &a.rv}) { Param& p = params[r->tw]; p.off = te_w_off; p.frag_rows = te_total; p.frag_row0 = r->te_off; }
    // ---- backward-data image (its own buffer, set only when a guided step is wanted: vd_set_bwd_weight_storage)
    size_t offb = 0;
    for (auto& p : params) {
        if (p.kind_bwd < 0) continue;
        p.packed_bwd = bwd_image_floats(bwd_kind_of(p), (size_t)p.shape[0], (size_t)p.shape[1]);
        p.off_bwd = offb;
        offb += (p.packed_bwd + 3) & ~(size_t)3;
    }
    packed_bwd_total = offb;
    for (auto& p : params)
        if (p.kind == PK_LINF) {
            if (!p.frag_rows) p.frag_rows = (int)p.shape[0];
            VD_REQUIRE(p.shape[0] % 32 == 0 && p.shape[1] % 32 == 0 && p.frag_row0 % 32 == 0, "linear layer dims must be multiples of 32");
        }
    return 0;
}

// ------------------------------------------------------------------------------------------ helpers
static IgemmArgs linear_args(int M, int K, int Nout) {
    IgemmArgs g{};
    g.C0 = K; g.Cin = K; g.nfr = M; g.Hs = 1; g.Ws = 1; g.stride = 1; g.ksz = 1; g.Ho = 1; g.Wo = 1;
    g.wsplit = split_math(); g.ldo = Nout; g.Cout = Nout; g.M = M; g.res_ld = Nout;
    return g;
}

// The output of a linear layer that is a GroupNorm's input (t: H x H pixels per frame, rows in (frame, pixel) order): where
// the split GEMM runs it in one launch, its epilogue writes the per-channel partial sums -- allocate the table (also in the
// arena's dry run) and let the tensor carry it; otherwise the tensor stays without and gn_fold runs a statistics pass
void vd_engine::gemm_stats_table(Arena& ar, int M, int K, int Nout, Tens* t) {
    IgemmArgs g = linear_args(M, K, Nout);
    g.wfrag = reinterpret_cast<const float*>(this);                                  // any non-null pointer: the shape test only
    const int HW = t->H * t->H, rows = gemm_split_stats_rows(M, Nout);
    if (!gemm_split_supported(g) || igemm_frames_per_launch(g) < M || HW % rows || M % HW) return;
    t->split = HW / rows;
    t->part = ar.get<double>((size_t)(M / HW) * t->split * Nout * 2);
}

// the same for a 3x3 conv that runs on the split GEMM's implicit-im2col mode (the stride-2 Downsample convs): the rows of
// its output are the Ho x Wo pixels of consecutive frames
void vd_engine::conv_split_stats_table(Arena& ar, const IgemmArgs& conv, int Cout, Tens* t) {
    IgemmArgs g = conv;
    g.wfrag = reinterpret_cast<const float*>(this); g.wsplit = split_math(); g.Cout = Cout; g.ldo = Cout; g.res_ld = Cout;
    const int HW = g.Ho * g.Wo, rows = gemm_split_stats_rows(g.M, Cout);
    if (!conv_split_supported(g) || igemm_frames_per_launch(g) < g.nfr || HW % rows) return;
    t->split = HW / rows;
    t->part = ar.get<double>((size_t)g.nfr * t->split * Cout * 2);
}

int vd_engine::linear(const float* a, int M, int K, int Nout, const float* wptr, const float* bptr, int act,
                      const float* resid, float* out, hipStream_t st, const Tens* stats_of) {
    IgemmArgs g = linear_args(M, K, Nout);
    g.src0 = a; g.wfrag = wptr;              // every nn.Linear weight is stored fragment-major (PK_LINF)
    g.bias = bptr; g.act = act; g.res = resid; g.out = out;
    if (stats_of && stats_of->part) { g.stats = stats_of->part; g.stats_split = stats_of->split; g.stats_hw = stats_of->H * stats_of->H; }
    return igemm_p(g, st);
}

// GroupNorm input of gn_fold / gn_act (x1: the second half of a virtual concat, or null): per-channel partial sums of each source --
// the table its producer wrote, or one statistics pass over it
static int gn_partials(const Tens& x0, const Tens* x1, int N, hipStream_t st, Arena& ar, const double* part[2], int split[2]) {
    const int HW = x0.H * x0.H;
    const Tens* src[2] = {&x0, x1};
    for (int i = 0; i < 2; ++i) {
        part[i] = nullptr; split[i] = 0;
        if (!src[i]) continue;
        if (src[i]->part) { part[i] = src[i]->part; split[i] = src[i]->split; continue; }
        split[i] = gn_stats_split(N, HW, src[i]->C);
        double* pt = ar.get<double>((size_t)N * split[i] * src[i]->C * 2);
        part[i] = pt;
        if (ar.dry) continue;
        ProfScope ps(PC_GN_STATS, 0.0, 4.0 * N * HW * src[i]->C, st);
        int rc = launch_gn_stats(src[i]->p, nullptr, src[i]->C, src[i]->C, N, HW, pt, split[i], st);
        if (rc) return rc;
    }
    return 0;
}

int vd_engine::gn_fold(const Tens& x0, const Tens* x1, int N, int gw, int gb,
                       const float* film, int film_ld, hipStream_t st, Arena& ar, float** A, float** Bp, float** mr) {
    const int HW = x0.H * x0.H, C = x0.C + (x1 ? x1->C : 0);
    const double* part[2]; int split[2];
    if (int rc = gn_partials(x0, x1, N, st, ar, part, split)) return rc;
    *A = ar.get<float>((size_t)N * C);
    *Bp = ar.get<float>((size_t)N * C);
    float* mrp = tape && mr ? ar.get<float>((size_t)N * 64) : nullptr;      // group mean / rstd for the backward pass
    if (mr) *mr = mrp;
    if (ar.dry) return 0;
    return launch_gn_affine(part[0], split[0], x0.C, part[1], split[1], (double)HW * (C / 32), W(gw), W(gb), film, film_ld, N,
                            C, *A, *Bp, st, mrp);
}

// The form gn_act takes for a layer call of `layer_frames` frames: 0 = the folding pass, 1 = gn_final_affine + the activation pass,
// from 64 MB of fp32 tensor on (see gn_act).  Exported as vd_gn_act_form.
static int gn_act_form(int layer_frames, int HW, int C) {
    constexpr size_t big = (size_t)64 << 20;
    return (size_t)layer_frames * HW * C * 4 >= big ? 1 : 0;
}

// GroupNorm(+FiLM) + SiLU of a (virtually concatenated) tensor into y in ONE launch: the activation pass folds the statistics
// itself (norm.hip: affine_act_fold_kernel).  For consumers that need nothing but y; not with a tape (the backward pass reads
// A, B and mean / rstd).
int vd_engine::gn_act(const Tens& x0, const Tens* x1, int N, int gw, int gb, const float* film, int film_ld, int act, float* y,
                      hipStream_t st, Arena& ar) {
    const int HW = x0.H * x0.H, C = x0.C + (x1 ? x1->C : 0);
    const double* part[2]; int split[2];
    if (int rc = gn_partials(x0, x1, N, st, ar, part, split)) return rc;
    // Big tensors (the 64 x 64 and 32 x 32 levels of a full window) take the two-launch form: (A, B) per (frame, channel) by
    // gn_final_affine, then the pass on many short blocks -- 5.95 TB/s against the 5.2 of the long blocks the in-kernel fold needs
    // (tools/probes/stream_probe.hip); the 7 us of the extra launch are repaid from ~64 MB on.  Same formulas and fp64 sums; the ORDER of the
    // sums differs (gn_final_affine deals a group's pairs to eight lanes, the folding pass walks them in sequence), so (A, B) agree to fp64
    // rounding -- after the cast to fp32 in practice to the bit, by construction to 1 ulp.  The 64 MB switch is by the
    // size of the whole layer call (g_sel_nfr): a full window and the compact suffix batch of the same layer take the same form.
    const bool two = gn_act_form(g_sel_nfr > N ? g_sel_nfr : N, HW, C) == 1;      // by the size of the whole layer call: the compact suffix batch takes the full window's form
    float* Aab = two ? ar.get<float>((size_t)N * C) : nullptr;
    float* Bab = two ? ar.get<float>((size_t)N * C) : nullptr;
    if (ar.dry) return 0;
    if (two) {
        int rc = launch_gn_affine(part[0], split[0], x0.C, part[1], split[1], (double)HW * (C / 32), W(gw), W(gb), film, film_ld, N, C, Aab, Bab, st);
        if (rc) return rc;
        ProfScope ps(PC_ELEMENTWISE, 0.0, 8.0 * N * HW * C, st);
        return launch_affine_act(x0.p, x1 ? x1->p : nullptr, x0.C, C, Aab, Bab, N, HW, act, y, st);
    }
    GnFold f{part[0], split[0], part[1], split[1], (double)HW * (C / 32), W(gw), W(gb), film, film_ld};
    ProfScope ps(PC_ELEMENTWISE, 0.0, 8.0 * N * HW * C, st);
    return launch_affine_act_fold(x0.p, x1 ? x1->p : nullptr, x0.C, C, f, N, HW, act, y, st);
}

// the epilogue of the Winograd conv (the kernel every PK_CONV3W weight runs on) writes the GroupNorm partial sums of
// its output: allocate the table and hand it to the launch
static double* stats_table(Arena& ar, int N, int Hout, int Cout, int* split) {
    *split = conv_wino_stats_split(Hout);
    return ar.get<double>((size_t)N * *split * Cout * 2);
}

// split-K scratch of a small-grid Winograd conv (conv_wino_r64.hip).  The dry run that sizes the workspace takes the largest
// request over every batch 1..N: the prefix-cache forward runs the same layer on a compact batch (fewer frames = a smaller
// grid = possibly MORE slices), and the arena must hold that too
static size_t ksplit_scratch(const Arena& ar, int N, int H, int cin, int cout) {
    if (!ar.dry) return conv_wino_r64_ksplit_floats(N, H, cin, cout, g_sel_nfr);
    size_t m = 0;
    for (int n = 1; n <= N; ++n) m = std::max(m, conv_wino_r64_ksplit_floats(n, H, cin, cout));
    for (int n = 1; n <= N; ++n) m = std::max(m, conv_wino_r64_ksplit_floats(n, H, cin, cout, N));     // a compact suffix: slices chosen for N frames
    return m;
}

// the source side of a convolution: nfr frames of Hs x Ws pixels, C0 channels of src0 (+ Cin - C0 of src1, a virtual concat),
// read through a nearest x2 upsample when ups = 1; the output size and M follow
static IgemmArgs conv_args(const float* src0, const float* src1, int C0, int Cin, int nfr, int Hs, int Ws, int ups, int stride,
                           int pad, int ksz) {
    IgemmArgs g{};
    g.src0 = src0; g.src1 = src1; g.C0 = C0; g.Cin = Cin;
    g.nfr = nfr; g.Hs = Hs; g.Ws = Ws; g.ups = ups; g.stride = stride; g.pad = pad; g.ksz = ksz;
    g.Ho = ((Hs << ups) + 2 * pad - ksz) / stride + 1;
    g.Wo = ((Ws << ups) + 2 * pad - ksz) / stride + 1;
    g.M = nfr * g.Ho * g.Wo;
    return g;
}

static IgemmArgs conv_args(Tens x0, const Tens* x1, int N, int ksz, int stride, int ups) {
    IgemmArgs g = conv_args(x0.p, x1 ? x1->p : nullptr, x0.C, x0.C + (x1 ? x1->C : 0), N, x0.H, x0.H, ups, stride, ksz == 3 ? 1 : 0, ksz);
    g.nfr_sel = g_sel_nfr;
    return g;
}

// The GEMM half of the PK_OUTCONV image: OIHW -> [out_t_cols(O)][I], rows co * 9 + tap, the rows past 9 O zero (vd_load_weight, vd_op_out_head)
static void pack_out_head(const float* oihw, int O, int I, float* wt) {
    std::fill(wt, wt + (size_t)out_t_cols(O) * I, 0.f);
    for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i)
            for (int t = 0; t < 9; ++t) wt[((size_t)o * 9 + t) * I + i] = oihw[((size_t)o * I + i) * 9 + t];
}

// out = conv3x3(silu(gn(h))) with 3 | 6 outputs (unet.py:744-749,838): T[pixel][cout * 9 + tap] = silu(A h + B) . w[cout][:][tap] as ONE
// 1x1 GEMM over the 27 | 54 (cout, tap) columns (head_gemm_kernel, or the generic kernel for shapes it does not take: GroupNorm
// affine + SiLU in the operand load), then
// eps[cout][y][x] = bias + sum over the 9 taps of T at the neighbour the tap points to (out_gather_kernel).
// h [nfr][H][W][C], (A, B) [nfr][C], Wt by pack_out_head, T [nfr][H][W][out_t_cols(Cout)] scratch, out [nfr][Cout][H][W].  The forward
// and vd_op_out_head launch through here; with `path` set nothing is launched and the path is named instead (vd_out_head_variant:
// the pointers are then only looked at for presence).  One switch serves both.
static int out_head(const float* h, const float* A, const float* Bf, const float* Wt, const float* bias, int nfr, int H, int W, int C, int Cout,
                    float* T, float* out, hipStream_t st, std::string* path = nullptr) {
    const int ldt = out_t_cols(Cout);
    int rc = 0;
    if (head_gemm_supported(H * W, C, ldt)) {
        if (path) { *path = "head_gemm/tpw" + std::to_string(head_gemm_tiles_per_wave(nfr, H * W)); return 0; }
        rc = launch_head_gemm(h, A, Bf, Wt, nfr, H * W, C, ldt, T, st);
    } else {
        IgemmArgs g = conv_args(h, nullptr, C, C, nfr, H, W, 0, 1, 0, 1);
        g.nfr_sel = g_sel_nfr;
        g.w = Wt; g.wsplit = 0; g.affA = A; g.affB = Bf; g.act = 1;
        g.out = T; g.ldo = ldt; g.Cout = ldt;
        if (path) {
            const IgemmVariant v = igemm_variant(g);
            *path = v.name ? "igemm/" + std::to_string(ldt) : igemm_variant_name(v);
            return 0;
        }
        rc = launch_igemm(g, st);
    }
    if (!rc) rc = launch_out_gather(T, bias, nfr, H, W, ldt, Cout, out, st);
    return rc;
}

int vd_engine::res_block(const ResP& r, Tens x0, const Tens* x1, int N, const float* film_all, hipStream_t st, Arena& ar, Tens* out) {
    const int H = x0.H, HW = H * H;
    const int cin = x0.C + (x1 ? x1->C : 0);
    VD_REQUIRE(cin == r.cin, "ResBlock input channels");
    const float* s1 = x1 ? x1->p : nullptr;
    float *A1 = nullptr, *B1 = nullptr, *A2 = nullptr, *B2 = nullptr, *mr1 = nullptr, *mr2 = nullptr;
    int rc;
    const float* film = film_all + r.film_off;
    // The skip convolution (1x1 over the block input, unet.py:159-166) reads the tensor the first GroupNorm+SiLU reads: where
    // it runs on the 128x128 tile of gemm_split.hip its column blocks 0 write that activation image from the rows they stage
    // (IgemmArgs::side) -- the block input, the largest tensor of a decoder block, is read once instead of twice.  Decided by
    // shape alone (the dry run lays the arena out the same way).
    IgemmArgs gsk{};
    bool fuse_skip = false;
    if (r.skw >= 0) {
        gsk = conv_args(x0, x1, N, 1, 1, 0);
        set_w(gsk, r.skw); gsk.Cout = r.cout; gsk.ldo = r.cout; gsk.side_hw = HW;
        IgemmArgs one = gsk; one.nfr = std::max(1, std::min(N, igemm_frames_per_launch(gsk)));
        one.M = (g_sel_nfr ? std::max(g_sel_nfr, one.nfr) : one.nfr) * HW;                     // (the tile class is chosen for the whole layer call)
        one.wfrag = one.wfrag ? one.wfrag : reinterpret_cast<const float*>(0x1000);      // dry run: no weight image yet, the shape decides
        fuse_skip = params[r.skw].kind == PK_LINF && split_math() && gemm_split_side_supported(one);
    }
    // the statistics folded by the activation pass itself (gn_act) wherever nothing else reads (A, B): not for the skip
    // convolution that writes the image (it takes the pair as arrays), not with a tape
    const bool fold = !tape;
    // Where conv_wino_z128.hip takes the convolution and one or two cout blocks share a patch, the GroupNorm(+FiLM) affine + SiLU runs in
    // the kernel's patch staging and the activation image is never written (conv_wino_z128_act_shape): the pair goes in as arrays.  The
    // dry run lays the arena out for both forms (a compact batch may decide differently).
    const int nsel = g_sel_nfr > N ? g_sel_nfr : N;
    const bool za1 = !tape && params[r.c1w].kind == PK_CONV3W && f16_math() && x0.C % 16 == 0 && conv_wino_z128_act_shape(nsel, H, cin, r.cout);
    // ... and then the skip convolution has no image to write: it runs as a plain 1x1 (the dry run keeps the larger layout: sk_early under the transient)
    if (za1 && !ar.dry) fuse_skip = false;
    const bool fold1 = fold && !fuse_skip;
    const bool za2 = !tape && params[r.c2w].kind == PK_CONV3W && f16_math() && conv_wino_z128_act_shape(nsel, H, r.cout, r.cout);
    if ((!fold1 || za1 || ar.dry) && (rc = gn_fold(x0, x1, N, r.gn1w, r.gn1b, nullptr, 0, st, ar, &A1, &B1, &mr1))) return rc;
    float* h = ar.get<float>((size_t)N * HW * r.cout);
    Tens ht{h, r.cout, H};
    if (params[r.c1w].kind == PK_CONV3W) ht.part = stats_table(ar, N, H, r.cout, &ht.split);
    Tens ot{nullptr, r.cout, H};
    if (params[r.c2w].kind == PK_CONV3W) ot.part = stats_table(ar, N, H, r.cout, &ot.split);
    float* sk_early = fuse_skip ? ar.get<float>((size_t)N * HW * r.cout) : nullptr;
    {   // SiLU(GroupNorm(concat(x0, x1))) once, into a transient; the conv then reads plain activations (norm.hip)
        const size_t mk = ar.mark();
        float* a1 = ar.get<float>((size_t)N * HW * cin);
        const size_t ksf = ksplit_scratch(ar, N, H, cin, r.cout);      // small grids: split-K scratch (conv_wino_r64.hip)
        float* ksw = ksf ? ar.get<float>(ksf) : nullptr;
        if (fold1 && !za1 && (rc = gn_act(x0, x1, N, r.gn1w, r.gn1b, nullptr, 0, 1, a1, st, ar))) return rc;
        if (!ar.dry) {
            if (fuse_skip) {
                gsk.bias = W(r.skb); gsk.out = sk_early; gsk.side = a1; gsk.sideA = A1; gsk.sideB = B1;
                if ((rc = igemm_p(gsk, st))) return rc;
            } else if (!fold1 && !za1 && (rc = affine_act(x0.p, s1, x0.C, cin, A1, B1, N, HW, a1, st))) return rc;
            Tens at{a1, cin, H};
            IgemmArgs g = conv_args(za1 ? x0 : at, za1 ? x1 : nullptr, N, 3, 1, 0);
            if (za1) { g.affA = A1; g.affB = B1; g.act = 1; }
            set_w(g, r.c1w); g.bias = W(r.c1b);
            g.out = h; g.ldo = r.cout; g.Cout = r.cout; g.stats = ht.part; g.stats_split = ht.split;
            g.ksplit_ws = ksw; g.ksplit_ws_floats = ksf;
            if (!cfg.use_scale_shift_norm) { g.fbias = film; g.fbias_ld = film_total; }    // h + emb_out (unet.py:196)
            VD_REQUIRE(!za1 || act_conv_will_dispatch(g), "res_block: in_layers conv was planned on conv_wino_z128's activating form (no activation image "
                                                          "written) but the call as built is not one it takes");
            if ((rc = igemm_p(g, st))) return rc;
        }
        ar.release(mk);
    }
    if ((!fold || za2 || ar.dry) && (rc = gn_fold(ht, nullptr, N, r.gn2w, r.gn2b, cfg.use_scale_shift_norm ? film : nullptr, film_total, st, ar, &A2, &B2, &mr2)))
        return rc;
    const float* skip = x0.p;
    if (fuse_skip) skip = sk_early;
    else if (r.skw >= 0) {
        float* sk = ar.get<float>((size_t)N * HW * r.cout);
        if (!ar.dry) {
            IgemmArgs g = conv_args(x0, x1, N, 1, 1, 0);
            set_w(g, r.skw); g.bias = W(r.skb); g.out = sk; g.ldo = r.cout; g.Cout = r.cout;
            if ((rc = igemm_p(g, st))) return rc;
        }
        skip = sk;
    } else {
        VD_REQUIRE(x1 == nullptr, "identity skip over a concatenated input");
    }
    float* o = ar.get<float>((size_t)N * HW * r.cout);
    {
        const size_t mk = ar.mark();
        float* a2 = ar.get<float>((size_t)N * HW * r.cout);
        const size_t ksf = ksplit_scratch(ar, N, H, r.cout, r.cout);
        float* ksw = ksf ? ar.get<float>(ksf) : nullptr;
        if (fold && !za2 && (rc = gn_act(ht, nullptr, N, r.gn2w, r.gn2b, cfg.use_scale_shift_norm ? film : nullptr, film_total, 1, a2, st, ar))) return rc;
        if (!ar.dry) {
            if (!fold && !za2 && (rc = affine_act(h, nullptr, r.cout, r.cout, A2, B2, N, HW, a2, st))) return rc;
            Tens at{a2, r.cout, H};
            IgemmArgs g = conv_args(za2 ? ht : at, nullptr, N, 3, 1, 0);
            if (za2) { g.affA = A2; g.affB = B2; g.act = 1; }
            set_w(g, r.c2w); g.bias = W(r.c2b);
            g.res = skip; g.res_ld = r.cout; g.out = o; g.ldo = r.cout; g.Cout = r.cout;
            g.stats = ot.part; g.stats_split = ot.split;
            g.ksplit_ws = ksw; g.ksplit_ws_floats = ksf;
            VD_REQUIRE(!za2 || act_conv_will_dispatch(g), "res_block: out_layers conv was planned on conv_wino_z128's activating form (no activation image "
                                                          "written) but the call as built is not one it takes");
            if ((rc = igemm_p(g, st))) return rc;
        }
        ar.release(mk);
    }
    ot.p = o;
    *out = ot;
    if (tape) {
        tape->ops.push_back(TapeOp{1, (int)tape->res.size()});
        tape->res.push_back(TapeRes{(int)(&r - res.data()), x0, x1 ? *x1 : Tens{}, x1 != nullptr, N, A1, B1, mr1, h, A2, B2, mr2, o});
    }
    return 0;
}

int vd_engine::attn_block(const AttnP& a, Tens x, int B, int T, const int64_t* fidx,
                          const float* amask, hipStream_t st, Arena& ar, Tens* out) {
    const int C = a.C, H = x.H, HW = H * H, N = B * T;
    const size_t tok = (size_t)N * HW;
    const float scale = 1.0f / sqrtf((float)(C / cfg.num_heads));
    int rc;
    // ---- temporal attention over the T frames of each (batch, pixel)      (unet.py:246-255)
    float* xn = ar.get<float>(tok * C);
    float* qkv = ar.get<float>(tok * 3 * C);
    // relative-position terms in memory order q, k, v: the RPE nets' come from rpe_all (start of the forward), the bucket tables' are built here
    const RpeP* rp[3] = {&a.rq, &a.rk, &a.rv};
    const size_t rrows = (size_t)B * T * T;
    const int blk = (int)(&a - attn.data());
    VD_REQUIRE(!cfg.use_rpe_net || !rpe_R.empty(), "attn_block: rpe_all has not run");
    float* Rall = cfg.use_rpe_net ? rpe_R[3 * blk] : ar.get<float>(3 * rrows * C);     // (memory order q, k, v)
    float* R[3] = {Rall + rrows * C, Rall, Rall + 2 * rrows * C};                      // k, q, v as the attention kernel takes them
    float* o = ar.get<float>(tok * C);
    float* xt = ar.get<float>(tok * C);
    Tens xt_t{xt, C, H};                               // the spatial attention's GroupNorm reads it: statistics from the proj_out GEMM
    gemm_stats_table(ar, (int)tok, C, C, &xt_t);
    if (!ar.dry) {
        { ProfScope ps(PC_GN_TEMPORAL, 0.0, 8.0 * tok * C, st);
          rc = launch_gn_temporal(x.p, W(a.tp.normw), W(a.tp.normb), B, T, HW, C, xn, st); }
        if (rc) return rc;
        if ((rc = linear(xn, (int)tok, C, 3 * C, W(a.tp.qkvw), W(a.tp.qkvb), 0, nullptr, qkv, st))) return rc;
        if (!cfg.use_rpe_net)
            for (int i = 0; i < 3; ++i)
                if ((rc = launch_rpe_table(W(rp[i]->table), fidx, B, T, C, cfg.rp_alpha, cfg.rp_beta, cfg.rp_gamma,
                                           Rall + i * rrows * C, st))) return rc;
        AttnTemporalArgs ta{qkv, R[0], R[1], R[2], amask, o, B, T, HW, C, cfg.num_heads,
                            cfg.allow_interactions_between_padding, scale};
        { const double Fd = C / cfg.num_heads;
          ProfScope ps(PC_ATTN_TEMPORAL, 10.0 * B * HW * cfg.num_heads * T * T * Fd, 16.0 * tok * C + 12.0 * rrows * C, st);
          rc = launch_attn_temporal(ta, st); }
        if (rc) return rc;
        if (!attn_cap_t.empty() && attn_seq < (int)attn_cap_t.size() && attn_cap_t[attn_seq] &&
            (rc = launch_attn_temporal_weights(ta, attn_cap_t[attn_seq], st))) return rc;
        // proj_out + residual on the NORMALISED activations (unet.py:537-538)
        if ((rc = linear(o, (int)tok, C, C, W(a.tp.projw), W(a.tp.projb), 0, xn, xt, st, &xt_t))) return rc;
    }
    // ---- spatial attention over the HW pixels of each frame               (unet.py:258-267)
    float *A = nullptr, *Bf = nullptr, *mrs = nullptr;
    const bool fold = !tape;
    if (!fold && (rc = gn_fold(xt_t, nullptr, N, a.sp.normw, a.sp.normb, nullptr, 0, st, ar, &A, &Bf, &mrs))) return rc;
    float* xn2 = ar.get<float>(tok * C);
    float* qkv2 = ar.get<float>(tok * 3 * C);
    float* o2 = ar.get<float>(tok * C);
    float* xs = ar.get<float>(tok * C);
    Tens xs_t{xs, C, H};                               // the block's output: the next ResBlock's GroupNorm (or a skip) reads it
    gemm_stats_table(ar, (int)tok, C, C, &xs_t);
    if (fold && (rc = gn_act(xt_t, nullptr, N, a.sp.normw, a.sp.normb, nullptr, 0, 0, xn2, st, ar))) return rc;
    if (!ar.dry) {
        if (!fold) { ProfScope ps(PC_ELEMENTWISE, 0.0, 8.0 * tok * C, st); rc = launch_affine_apply(xt, A, Bf, N, HW, C, xn2, st); }
        if (rc) return rc;
        if ((rc = linear(xn2, (int)tok, C, 3 * C, W(a.sp.qkvw), W(a.sp.qkvb), 0, nullptr, qkv2, st))) return rc;
        AttnSpatialArgs sa{qkv2, o2, N, HW, C, cfg.num_heads, scale};
        { ProfScope ps(PC_ATTN_SPATIAL, 4.0 * N * (double)HW * HW * C, 16.0 * tok * C, st); rc = launch_attn_spatial(sa, st); }
        if (rc) return rc;
        if (!attn_cap_s.empty() && attn_seq < (int)attn_cap_s.size() && attn_cap_s[attn_seq] &&
            (rc = launch_attn_spatial_weights(sa, attn_cap_s[attn_seq], st))) return rc;
        if ((rc = linear(o2, (int)tok, C, C, W(a.sp.projw), W(a.sp.projb), 0, xn2, xs, st, &xs_t))) return rc;
    }
    *out = xs_t;
    if (!ar.dry) ++attn_seq;
    if (tape) {
        tape->ops.push_back(TapeOp{2, (int)tape->attn.size()});
        tape->attn.push_back(TapeAttn{(int)(&a - attn.data()), x, B, T, xn, qkv, R[0], R[1], R[2], o, xt, A, Bf, mrs, xn2, qkv2, o2, xs, amask});
    }
    return 0;
}

// The relative-position nets of every attention block (RPENet, unet.py:283-298: silu(Linear(feat(d)) + Linear(emb)) -> Linear) read the
// timestep embedding and the frame indices only -- nothing a block computes.  Per block they were two small dependent launches (the three
// nets of a block batched): 22 of the ~210 launches of a step, each paying the ~5 us of a dependent dispatch on top of 5 - 15 us of work
// that leaves most CUs idle.  Here: per channel width ONE hidden-layer launch and ONE output-layer GEMM over all nets of that width (the
// 3 x 5 nets of 384 channels, the 3 x 6 of 512), at the start of the forward, in every arithmetic mode (the GEMM is gemm_split.hip's or,
// under VD_MATH=fp32, gemm_frag.hip's; both read the weights of problem z through IgemmArgs::ztab).  Same arithmetic per net: bit-identical R.
// The attention blocks by channel width (the dry run sizes the arena before any table exists: it needs the widths only)
void vd_engine::rpe_group_blocks() {
    if (!rpe_groups.empty()) return;
    for (size_t b = 0; b < attn.size(); ++b) {
        size_t gi = 0;
        while (gi < rpe_groups.size() && rpe_groups[gi].C != attn[b].C) ++gi;
        if (gi == rpe_groups.size()) rpe_groups.push_back(RpeGroup{attn[b].C, {}});
        rpe_groups[gi].blocks.push_back((int)b);
    }
}

// per width the device tables of offsets the two launches read (never inside a stream capture: ensure_ws calls this)
int vd_engine::rpe_tables() {
    if (!cfg.use_rpe_net || attn.empty() || !te_total) return 0;
    rpe_group_blocks();
    for (auto& g : rpe_groups) {
        if (g.d_hid) continue;
        const int nn = 3 * (int)g.blocks.size();
        std::vector<long long> th(3 * nn), to(2 * nn);
        for (size_t i = 0; i < g.blocks.size(); ++i) {
            const AttnP& a = attn[g.blocks[i]];
            const RpeP* rp[3] = {&a.rq, &a.rk, &a.rv};
            for (int k = 0; k < 3; ++k) {
                const int z = 3 * (int)i + k;
                th[3 * z] = rp[k]->te_off; th[3 * z + 1] = (long long)params[rp[k]->dw].off; th[3 * z + 2] = (long long)params[rp[k]->db].off;
                to[2 * z] = (long long)params[rp[k]->ow].off; to[2 * z + 1] = (long long)params[rp[k]->ob].off;
            }
        }
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&g.d_hid), th.size() * sizeof(long long)));
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&g.d_out), to.size() * sizeof(long long)));
        VD_HIP(hipMemcpy(g.d_hid, th.data(), th.size() * sizeof(long long), hipMemcpyHostToDevice));
        VD_HIP(hipMemcpy(g.d_out, to.data(), to.size() * sizeof(long long), hipMemcpyHostToDevice));
    }
    return 0;
}

int vd_engine::rpe_all(const float* te, const int64_t* fidx, int B, int T, hipStream_t st, Arena& ar) {
    rpe_R.clear();
    if (!cfg.use_rpe_net || attn.empty() || !te_total) return 0;
    rpe_group_blocks();
    const size_t rrows = (size_t)B * T * T;
    rpe_R.assign(3 * attn.size(), nullptr);
    int rc = 0;
    for (auto& g : rpe_groups) {
        const int nn = 3 * (int)g.blocks.size(), C = g.C;
        float* Rg = ar.get<float>((size_t)nn * rrows * C);
        for (size_t i = 0; i < g.blocks.size(); ++i)
            for (int k = 0; k < 3; ++k) rpe_R[3 * g.blocks[i] + k] = Rg + (3 * i + k) * rrows * C;
        const size_t mk = ar.mark();
        float* Eh = ar.get<float>((size_t)nn * rrows * C);
        ar.release(mk);                                                // a transient: the two launches are stream-ordered
        if (ar.dry) continue;
        VD_REQUIRE(g.d_hid && g.d_out, "rpe_all: offset tables missing (ensure_ws builds them)");
        if ((rc = launch_rpe_hidden_tab(te, te_total, wbuf, g.d_hid, fidx, B, T, C, Eh, nn, rrows * C, st))) return rc;
        IgemmArgs q = linear_args((int)rrows, C, C);
        q.src0 = Eh; q.out = Rg;
        q.wfrag = wbuf + params[attn[g.blocks[0]].rq.ow].off; q.bias = wbuf + params[attn[g.blocks[0]].rq.ob].off;   // (problem 0's: the shape checks read them)
        q.zcount = nn; q.zs_a = q.zs_out = (int)(rrows * C); q.ztab = g.d_out; q.zbase = wbuf;
        if ((rc = igemm_p(q, st))) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ forward
int vd_engine::forward(const FwdIn& in, hipStream_t st, Arena& ar, const PrefixPlan* pp, const SuffixPlan* sp) {
    const int B = in.B, T = in.T, N = B * T, S = cfg.image_size, mc = cfg.num_channels;
    int rc;
    drop_held();
    VD_REQUIRE(!pp || (!tape && !ar.dry && pp->store && n_before_attn > 0), "prefix plan: executor steps only");
    VD_REQUIRE(!sp || (!tape && sp->n > 0 && sp->n <= N && (ar.dry || sp->list)), "suffix plan: executor steps only, at least one frame");
    const FreeUReq* fu = in.fu;
    VD_REQUIRE(!fu || (!tape && !pp && !sp), "FreeU (vd_set_freeu): untaped forwards over all frames only");
    struct SelGuard { ~SelGuard() { g_sel_nfr = 0; } } sel_guard;      // (every return path leaves the selection hint cleared)
    const int Npre = pp ? pp->n : N;                                 // frames the blocks before the first attention layer run on
    float* x8 = ar.get<float>((size_t)Npre * S * S * STEM_KPAD);    // im2col of the network input
    float* tfr = ar.get<float>(N);
    float* amask = ar.get<float>(N);
    float* tsin = ar.get<float>((size_t)N * mc);
    float* e1 = ar.get<float>((size_t)N * E);
    float* emb = ar.get<float>((size_t)N * E);
    float* film = ar.get<float>((size_t)N * film_total);
    float* te = te_total ? ar.get<float>((size_t)N * te_total) : nullptr;
    float* ftv = cfg.use_frame_encoding ? ar.get<float>(N) : nullptr;
    float* femb = cfg.use_frame_encoding ? ar.get<float>((size_t)N * pos_ch) : nullptr;
    if (!ar.dry) {
        VD_REQUIRE(d_freq_time && n_freq_time == mc / 2, "vd_set_freqs not called (time frequencies)");
        AssembleArgs aa{in.x, in.obs_src, in.obs, in.lat, in.km, in.t_model, in.obs_mode, B, T, S, S, STEM_KPAD, cfg.cond_emb_type, x8, tfr, amask};
        if (pp) {                                                    // per-frame scalars of every frame, im2col of the listed ones
            AssembleArgs sc = aa; sc.scalars_only = 1;
            if ((rc = launch_assemble(sc, st))) return rc;
            aa.frame_list = pp->list; aa.n_list = pp->n;
        }
        if ((rc = launch_assemble(aa, st))) return rc;
        if ((rc = launch_sinus_embed(tfr, N, mc, d_freq_time, tsin, st))) return rc;
        if ((rc = linear(tsin, N, mc, E, W(p_te0w), W(p_te0b), 0, nullptr, e1, st))) return rc;
        if ((rc = linear(e1, N, E, E, W(p_te2w), W(p_te2b), 1, nullptr, emb, st))) return rc;
        // every ResBlock's emb_layers (SiLU -> Linear, unet.py:143-150) in ONE GEMM; same for RPENet's
        // embed_diffusion_time (no SiLU, unet.py:294)
        if ((rc = linear(emb, N, E, film_total, wbuf + film_w_off, wbuf + film_b_off, 1, nullptr, film, st))) return rc;
        if (te_total && (rc = linear(emb, N, E, te_total, wbuf + te_w_off, wbuf + te_b_off, 0, nullptr, te, st))) return rc;
        if (cfg.use_frame_encoding) {
            VD_REQUIRE(d_freq_frame && n_freq_frame == pos_ch / 2, "vd_set_freqs not called (frame frequencies)");
            if ((rc = launch_frame_t(in.fidx, B, T, cfg.enforce_position_invariance, ftv, st))) return rc;
            if ((rc = launch_sinus_embed(ftv, N, pos_ch, d_freq_frame, femb, st))) return rc;
        }
    }
    rpe_R.clear();
    if (!(pp && pp->build_only) && (rc = rpe_all(te, in.fidx, B, T, st, ar))) return rc;      // every block's relative-position tensors, up front
    attn_seq = 0;
    std::vector<Tens> hs;
    Tens h{x8, STEM_KPAD, S};
    int Nrun = Npre;                                                 // batch of the block being run: Npre in the prefix, N behind it
    const float* film_full = film;
    if (pp || ar.dry) {                                              // FiLM rows of the listed frames, compactly (the dry run sizes it for any list)
        float* fc = ar.get<float>((size_t)std::max(pp ? Npre : N, 1) * film_total);
        if (pp) {
            if ((rc = launch_gather_rows(film_full, pp->list, Npre, film_total, fc, st))) return rc;
            film = fc;
        }
    }
    auto run = [&](const std::vector<Layer>& blk, Tens in0, const Tens* in1, Tens* outp, size_t l0 = 0, size_t l1 = ~(size_t)0) -> int {
        const int N = Nrun;
        Tens cur = in0;
        const Tens* second = in1;
        for (size_t li = l0; li < std::min(l1, blk.size()); ++li) {
            const Layer& L = blk[li];
            Tens nxt{};
            if (L.type == 1) {
                if ((rc = res_block(res[L.idx], cur, second, N, film, st, ar, &nxt))) return rc;
            } else if (L.type == 2) {
                if ((rc = attn_block(attn[L.idx], cur, B, T, in.fidx, amask, st, ar, &nxt))) return rc;
            } else if (L.type == 0) {                                 // stem: im2col (assemble_kernel) x [64][mc] GEMM
                const ConvP& c = convs[L.idx];
                float* o = ar.get<float>((size_t)N * S * S * c.c);
                nxt = Tens{o, c.c, S};
                gemm_stats_table(ar, N * S * S, STEM_KPAD, c.c, &nxt);
                if (!ar.dry && (rc = linear(cur.p, N * S * S, STEM_KPAD, c.c, W(c.w), W(c.b), 0, nullptr, o, st, &nxt))) return rc;
                if (tape) { tape->ops.push_back(TapeOp{0, (int)tape->conv.size()}); tape->conv.push_back(TapeConv{0, L.idx, cur, nxt}); }
            } else {
                const ConvP& c = convs[L.idx];
                const int stride = L.type == 3 ? 2 : 1, ups = L.type == 4 ? 1 : 0;
                IgemmArgs g = conv_args(cur, nullptr, N, 3, stride, ups);
                float* o = ar.get<float>((size_t)g.M * c.c);
                nxt = Tens{o, c.c, g.Ho};
                const bool phase = params[c.w].kind == PK_CONV3WU;                    // sub-pixel Upsample conv: four table entries per tile group
                if (params[c.w].kind == PK_CONV3W) nxt.part = stats_table(ar, N, g.Ho, c.c, &nxt.split);
                else if (phase) { nxt.split = conv_wino_ups_stats_split(cur.H); nxt.part = ar.get<double>((size_t)N * nxt.split * c.c * 2); }
                else if (stride == 2) conv_split_stats_table(ar, g, c.c, &nxt);       // Downsample on the split GEMM
                const size_t mk = ar.mark();
                const size_t ksf = stride == 1 && !phase ? ksplit_scratch(ar, N, g.Ho, cur.C, c.c) : 0;
                float* ksw = ksf ? ar.get<float>(ksf) : nullptr;
                ar.release(mk);                                                       // a transient: the launches are stream-ordered
                if (!ar.dry) {
                    g.ksplit_ws = ksw; g.ksplit_ws_floats = ksf;
                    set_w(g, c.w); g.bias = W(c.b); g.out = o; g.ldo = c.c; g.Cout = c.c;
                    g.stats = nxt.part; g.stats_split = nxt.split;
                    if (nxt.part && params[c.w].kind != PK_CONV3W && !phase) g.stats_hw = g.Ho * g.Wo;
                    if ((rc = igemm_p(g, st))) return rc;
                }
                if (tape) { tape->ops.push_back(TapeOp{0, (int)tape->conv.size()}); tape->conv.push_back(TapeConv{L.type, L.idx, cur, nxt}); }
            }
            cur = nxt;
            second = nullptr;
            // a request the dry run did not see was served from the arena's base (Arena::get): stop before anything else is enqueued on
            // top of the aliased tensors -- inside a capture this also keeps the broken step out of the graph
            VD_REQUIRE(!ar.overflow, "workspace overflow: the forward asked for more than the dry run measured (this step's output is invalid)");
        }
        *outp = cur;
        return 0;
    };
    for (size_t i = 0; i < input_blocks.size(); ++i) {
        if (pp && (int)i < n_before_attn) {
            // compact batch -> this block's persistent full-size tensor (allocated by the window's first pass, outside the arena)
            Tens hc{};
            if (Npre > 0 && (rc = run(input_blocks[i], h, nullptr, &hc))) return rc;
            PrefixStore& ps = *pp->store;
            if (ps.tens.size() <= i) { ps.tens.resize(i + 1, nullptr); ps.parts.resize(i + 1, nullptr); ps.floats.resize(i + 1, 0); }
            if (Npre == 0) { VD_REQUIRE(ps.tens[i], "prefix cache: no tensor to reuse"); }
            else {
                const size_t per = (size_t)hc.H * hc.H * hc.C;
                if (!ps.tens[i]) {
                    VD_REQUIRE(pp->build_only, "prefix cache: the window's first pass allocates");
                    VD_HIP(hipMalloc(reinterpret_cast<void**>(&ps.tens[i]), (size_t)N * per * sizeof(float)));
                    ps.floats[i] = per | ((size_t)hc.C << 40) | ((size_t)hc.H << 52);
                    if (hc.part) VD_HIP(hipMalloc(reinterpret_cast<void**>(&ps.parts[i]), (size_t)N * hc.C * 2 * sizeof(double)));
                }
                VD_REQUIRE((ps.parts[i] != nullptr) == (hc.part != nullptr), "prefix cache: statistics table");
                if ((rc = launch_scatter_rows(hc.p, pp->list, Npre, per, ps.tens[i], st))) return rc;
                if (hc.part && (rc = launch_scatter_stats(hc.part, hc.split, hc.C, pp->list, Npre, ps.parts[i], st))) return rc;
            }
            const int Cc = (int)((ps.floats[i] >> 40) & 0xfff), Hc = (int)(ps.floats[i] >> 52);
            Tens full{ps.tens[i], Cc, Hc, ps.parts[i], ps.parts[i] ? 1 : 0};
            if ((int)i + 1 == n_before_attn) {
                if (pp->build_only) return 0;
                h = full; Nrun = N; film = const_cast<float*>(film_full);
            } else {
                h = hc;                                              // the next prefix block continues on the compact batch
            }
            hs.push_back(full);
        } else {
            if ((rc = run(input_blocks[i], h, nullptr, &h))) return rc;
            hs.push_back(h);
        }
        if ((int)i + 1 == n_before_attn && (cfg.use_spatial_encoding || cfg.use_frame_encoding)) {
            // added AFTER the skip push (unet.py:815-818): the skip keeps the un-encoded tensor
            const size_t n = (size_t)N * h.H * h.H * h.C;
            float* y = ar.get<float>(n);
            if (!ar.dry) {
                VD_REQUIRE(h.H == pos_res && h.C == pos_ch, "positional encoding shape");
                if ((rc = launch_posenc_add(h.p, cfg.use_spatial_encoding ? W(p_posenc) : nullptr, femb, N, h.H * h.H, h.C, y, st)))
                    return rc;
            }
            if (tape) { tape->ops.push_back(TapeOp{5, (int)tape->pos.size()}); tape->pos.push_back(TapePos{h, Tens{y, h.C, h.H}}); }
            h = Tens{y, h.C, h.H};
        }
    }
    if ((rc = run(middle, h, nullptr, &h))) return rc;
    // window suffix skip: from behind the last attention layer on, the listed frames only
    const int Nsuf = sp ? sp->n : N;
    bool compact = false;
    auto gather_t = [&](const Tens& t) -> Tens {                      // rows and GroupNorm partial sums of the listed frames
        const size_t per = (size_t)t.H * t.H * t.C;
        Tens c{ar.get<float>((size_t)Nsuf * per), t.C, t.H, nullptr, t.split};
        if (t.part) c.part = ar.get<double>((size_t)Nsuf * t.split * t.C * 2);
        if (!ar.dry) {
            if (launch_gather_rows(t.p, sp->list, Nsuf, per, c.p, st)) return Tens{};
            if (t.part && launch_gather_rows(reinterpret_cast<const float*>(t.part), sp->list, Nsuf, (size_t)t.split * t.C * 4,
                                             reinterpret_cast<float*>(c.part), st)) return Tens{};
        }
        return c;
    };
    auto go_compact = [&]() -> int {
        float* fc = ar.get<float>((size_t)Nsuf * film_total);
        if (!ar.dry && (rc = launch_gather_rows(film_full, sp->list, Nsuf, film_total, fc, st))) return rc;
        h = gather_t(h);
        VD_REQUIRE(ar.dry || h.p, "suffix skip: gather");
        film = fc; Nrun = Nsuf; g_sel_nfr = N; compact = true;
        return 0;
    };
    if (sp && suf_blk < 0 && (rc = go_compact())) return rc;
    for (size_t i = 0; i < output_blocks.size(); ++i) {
        Tens skip = hs.back(); hs.pop_back();
        if (sp && !compact && (int)i == suf_blk) {
            if ((rc = run(output_blocks[i], h, &skip, &h, 0, suf_layer + 1))) return rc;        // cat([h, hs.pop()]) read in place
            if ((rc = go_compact())) return rc;
            if ((rc = run(output_blocks[i], h, nullptr, &h, suf_layer + 1))) return rc;
            continue;
        }
        if (compact) { skip = gather_t(skip); VD_REQUIRE(ar.dry || skip.p, "suffix skip: gather"); }
        if (fu && i < fu_blk.size() && !ar.dry) {
            // FreeU: the block reads cat([h', skip']) -- both in the engine's buffers, never in place.  The producers' statistics tables do
            // not describe the modified values: one statistics pass over each modified half, here, into the engine's buffers as well --
            // left to gn_partials the tables would come out of the step arena, whose dry run sees the unmodified halves and sizes none
            const int sg = (int)i / fu_per_stage;
            auto stats = [&](Tens* t, double* part) -> int {
                t->split = gn_stats_split(N, t->H * t->H, t->C);
                t->part = part;
                ProfScope ps(PC_GN_STATS, 0.0, 4.0 * N * t->H * t->H * t->C, st);
                return launch_gn_stats(t->p, nullptr, t->C, t->C, N, t->H * t->H, part, t->split, st);
            };
            VD_REQUIRE(h.H == fu_blk[i].S && h.C == fu_blk[i].Ch && skip.H == h.H && skip.C == fu_blk[i].Cs, "FreeU: decoder block shape");
            const double bytes = 8.0 * N * h.H * h.H;
            if (fu->b[sg] != 1.0) {
                {   // (a profiler record closes before the next one opens)
                    ProfScope ps(PC_ELEMENTWISE, 1.0 * N * h.H * h.H * h.C, bytes * h.C * (fu->adaptive ? 1.5 : 1.0), st, "freeu_backbone");
                    if ((rc = launch_freeu_backbone(h.p, N, h.H, h.C, fu->b[sg], fu->adaptive, fu->map, fu->yh, st))) return rc;
                }
                h = Tens{fu->yh, h.C, h.H};
                if ((rc = stats(&h, fu->ph))) return rc;
            }
            if (fu->s[sg] != 1.0) {
                {
                    ProfScope ps(PC_ELEMENTWISE, 26.0 * N * h.H * h.H * skip.C, bytes * skip.C, st, "freeu_filter");
                    if ((rc = launch_freeu_filter(skip.p, N, skip.H, skip.C, fu->s[sg], fu->trig[sg], fu->ys, st))) return rc;
                }
                skip = Tens{fu->ys, skip.C, skip.H};
                if ((rc = stats(&skip, fu->ps))) return rc;
            }
        }
        if ((rc = run(output_blocks[i], h, &skip, &h))) return rc;
    }
    float *A, *Bf, *mrh = nullptr;
    if ((rc = gn_fold(h, nullptr, Nrun, p_outgw, p_outgb, nullptr, 0, st, ar, &A, &Bf, &mrh))) return rc;
    if (tape) { tape->head = h; tape->headA = A; tape->headB = Bf; tape->head_mr = mrh; }
    const int oc = cfg.learn_sigma ? 6 : 3;
    float* eps_c = compact ? ar.get<float>((size_t)Nsuf * oc * S * S) : nullptr;
    float* head_t = ar.get<float>((size_t)Nrun * S * S * out_t_cols(oc));
    if (!ar.dry) {
        VD_REQUIRE(h.H == S && h.C == final_ch, "output head shape");
        { // out = conv3x3(silu(gn(h))) with 3 | 6 outputs (unet.py:744-749,838): out_head()
          ProfScope ps(PC_OUT_CONV, 2.0 * Nrun * S * S * h.C * 27.0, 4.0 * Nrun * S * S * (h.C + 3.0), st);
          rc = out_head(h.p, A, Bf, W(p_outw) + (size_t)9 * oc * h.C, W(p_outb), Nrun, S, S, h.C, oc, head_t, compact ? eps_c : in.eps, st); }
        if (rc) return rc;
        if (compact) {                                               // the other frames' eps: zeros (their samples stay finite; nobody reads them)
            VD_HIP(hipMemsetAsync(in.eps, 0, (size_t)N * oc * S * S * sizeof(float), st));
            if ((rc = launch_scatter_rows(eps_c, sp->list, Nsuf, (size_t)oc * S * S, in.eps, st))) return rc;
        }
    }
    VD_REQUIRE(!ar.overflow, "workspace overflow: the forward asked for more than the dry run measured (this step's output is invalid)");
    return 0;
}

int vd_engine::ensure_ws(int B, int T, bool suffix_plan) {
    const bool suf = suffix_skip_on || suffix_plan;     // the window flag, or a call that hands forward() a SuffixPlan of its own (vd_score_windows)
    if (B == ws_B && T == ws_T && ws && ws_suf == suf) return 0;      // the common case: every step of a window
    // with a suffix plan the arena also holds the gathered skip tensors: sized for the worst list (every frame)
    const long long key = ((long long)B << 32) | (unsigned)T | (suf ? 1ll << 61 : 0);
    size_t tail = 0;
    int rc = grow_ws(key, step_tail_bytes(B, T), [&](size_t* peak) {
        Arena dry; dry.dry = true;
        FwdIn fi{}; fi.B = B; fi.T = T;
        int frc = forward(fi, nullptr, dry);
        if (!frc && suf) {
            Arena dry2; dry2.dry = true;
            SuffixPlan wp; wp.n = B * T;
            frc = forward(fi, nullptr, dry2, nullptr, &wp);
            dry.peak = std::max(dry.peak, dry2.peak);
        }
        *peak = dry.peak;
        return frc;
    }, &tail);
    if (rc) return rc;
    ws_B = B; ws_T = T; ws_tail = tail; ws_suf = suf;
    return 0;
}


// ------------------------------------------------------------------------------------------ backward (use_gradient_method)
// d(out)/d(in) of every taped op, walked in reverse.  Gradients live in the same arena behind the forward's tensors; a
// tensor's gradient buffer is created by its first consumer (assigned) and accumulated into by the others (the skip
// connections: an encoder output feeds the next encoder block AND a decoder block).
namespace {
struct GradMap {
    std::unordered_map<const float*, std::pair<float*, bool>> m;     // tensor -> (gradient, written)
    Arena* ar;
    float* get(const Tens& t, int N, bool* fresh) {
        auto it = m.find(t.p);
        if (it == m.end()) it = m.emplace(t.p, std::make_pair(ar->get<float>((size_t)N * t.H * t.H * t.C), false)).first;
        *fresh = !it->second.second;
        it->second.second = true;
        return it->second.first;
    }
    float* have(const float* p) const { auto it = m.find(p); return it == m.end() ? nullptr : it->second.first; }
};
}  // namespace

// The argument setup of bwd_linear / bwd_conv3, shared with vd_op_linear_bwd_data / vd_op_conv3_bwd_data: w_bwd is the backward image
// (vd_pack_weight_bwd)
static IgemmArgs bwd_linear_args(const float* dy, int M, int Kb, int Nb, const float* w_bwd, const float* resid, float* out) {
    IgemmArgs g = linear_args(M, Kb, Nb);
    g.src0 = dy; g.wfrag = w_bwd; g.wsplit = 1; g.res = resid; g.out = out;
    return g;
}

// floats of split-K scratch a backward 3x3 conv is offered (the Winograd-split image only)
static size_t bwd_conv3_scratch(const Arena& ar, int kind_bwd, Tens dy, int N, int cout_bwd) {
    return kind_bwd == PK_CONV3W ? ksplit_scratch(ar, N, dy.H, dy.C, cout_bwd) : 0;
}

static IgemmArgs bwd_conv3_args(Tens dy, int N, int kind_bwd, const float* w_bwd, int cout_bwd, const float* resid, float* out, float* ksplit_ws,
                                size_t ksplit_ws_floats) {
    IgemmArgs g = conv_args(dy, nullptr, N, 3, 1, 0);
    g.ksplit_ws = ksplit_ws; g.ksplit_ws_floats = ksplit_ws_floats;
    if (kind_bwd == PK_CONV3W) { g.wwino = w_bwd; g.wsplit = 2; } else { g.w = w_bwd; g.wsplit = 0; }
    g.res = resid; g.res_ld = cout_bwd; g.out = out; g.ldo = cout_bwd; g.Cout = cout_bwd;
    return g;
}

// out[M][K_fwd] = dy[M][N_fwd] * W  (+ res): the forward's split GEMM over the transposed image of parameter pw
int vd_engine::bwd_linear(const float* dy, int M, int pw, const float* resid, float* out, hipStream_t st) {
    const Param& p = params[pw];
    const int Kb = (int)p.shape[0], Nb = p.kind == PK_STEM ? STEM_KPAD : (int)p.shape[1];
    const IgemmArgs g = bwd_linear_args(dy, M, Kb, Nb, WB(pw), resid, out);
    VD_REQUIRE(gemm_split_supported(g), "backward linear layer: shape not covered by gemm_split.hip");
    return launch_igemm(g, st);
}

// out[N][H][H][cout_bwd] = conv3x3_s1(dy, rotated transposed kernel of parameter pw) (+ res, in place allowed)
int vd_engine::bwd_conv3(Tens dy, int N, int pw, int cout_bwd, const float* resid, float* out, hipStream_t st, Arena& ar) {
    const Param& p = params[pw];
    const size_t mk = ar.mark();
    const size_t ksf = bwd_conv3_scratch(ar, p.kind_bwd, dy, N, cout_bwd);
    float* ksw = ksf ? ar.get<float>(ksf) : nullptr;
    ar.release(mk);
    if (ar.dry) return 0;
    return launch_igemm(bwd_conv3_args(dy, N, p.kind_bwd, WB(pw), cout_bwd, resid, out, ksw, ksf), st);
}

int vd_engine::backward(const FwdIn& in, const float* deps, float* dx, hipStream_t st, Arena& ar) {
    const int B = in.B, T = in.T, N = B * T, S = cfg.image_size;
    const bool dry = ar.dry;
    int rc;
    drop_held();
    GradMap gm; gm.ar = &ar;
    bool fresh;
    // GroupNorm(+act) backward with its workspaces
    auto gn_bwd = [&](const Tens& x0, const Tens* x1, const float* A, const float* Bv, const float* mr, const float* dy, int act,
                      float* dx0, int acc0, float* dx1, int acc1, const float* extra) -> int {
        const int C = x0.C + (x1 ? x1->C : 0), HW = x0.H * x0.H;
        const size_t mk = ar.mark();
        double* part = ar.get<double>((size_t)N * gn_bwd_split(N, HW, C) * C * 2);
        float* K = ar.get<float>((size_t)N * 64);
        ar.release(mk);
        if (dry) return 0;
        GnBwdArgs a{x0.p, x1 ? x1->p : nullptr, x0.C, C, A, Bv, mr, dy, act, N, HW, dx0, dx1, acc0, acc1, extra, part, K};
        return launch_gn_bwd(a, st);
    };
    // ---- output head: eps = conv(silu(gn(h)))   (unet.py:744-749,838)
    {
        const Tens& h = tape->head;
        float* dh = gm.get(h, N, &fresh);
        const size_t mk = ar.mark();
        float* da = ar.get<float>((size_t)N * S * S * h.C);
        if (!dry && (rc = launch_out_conv_bwd(deps, W(p_outw), N, S, S, h.C, 3, da, st))) return rc;
        if ((rc = gn_bwd(h, nullptr, tape->headA, tape->headB, tape->head_mr, da, 1, dh, 0, nullptr, 0, nullptr))) return rc;
        ar.release(mk);
    }
    for (int oi = (int)tape->ops.size() - 1; oi >= 0; --oi) {
        const TapeOp op = tape->ops[oi];
        if (op.kind == 1) {                                              // ---- ResBlock (unet.py:185-198)
            const TapeRes& t = tape->res[op.i];
            const ResP& r = res[t.idx];
            const int H = t.x0.H, HW = H * H, cin = r.cin;
            float* d_o = gm.have(t.o);
            VD_REQUIRE(dry || d_o, "backward: ResBlock output without a gradient");
            if (!d_o) d_o = gm.get(Tens{t.o, r.cout, H}, N, &fresh);
            bool f0, f1 = true;
            float* dx0 = gm.get(t.x0, N, &f0);
            float* dx1 = t.has_x1 ? gm.get(t.x1, N, &f1) : nullptr;
            const size_t mk = ar.mark();
            float* d_a2 = ar.get<float>((size_t)N * HW * r.cout);
            float* d_h = ar.get<float>((size_t)N * HW * r.cout);
            float* d_a1 = ar.get<float>((size_t)N * HW * cin);
            float* d_sk = r.skw >= 0 ? ar.get<float>((size_t)N * HW * cin) : nullptr;
            if ((rc = bwd_conv3(Tens{d_o, r.cout, H}, N, r.c2w, r.cout, nullptr, d_a2, st, ar))) return rc;
            if ((rc = gn_bwd(Tens{t.h, r.cout, H}, nullptr, t.A2, t.B2, t.mr2, d_a2, 1, d_h, 0, nullptr, 0, nullptr))) return rc;
            if ((rc = bwd_conv3(Tens{d_h, r.cout, H}, N, r.c1w, cin, nullptr, d_a1, st, ar))) return rc;
            if (r.skw >= 0 && !dry && (rc = bwd_linear(d_o, N * HW, r.skw, nullptr, d_sk, st))) return rc;
            // the skip path's gradient (identity: d_o itself) rides on the GroupNorm backward's write
            if ((rc = gn_bwd(t.x0, t.has_x1 ? &t.x1 : nullptr, t.A1, t.B1, t.mr1, d_a1, 1, dx0, !f0, dx1, !f1, r.skw >= 0 ? d_sk : d_o))) return rc;
            ar.release(mk);
        } else if (op.kind == 2) {                                       // ---- FactorizedAttentionBlock (unet.py:236-267)
            const TapeAttn& t = tape->attn[op.i];
            const AttnP& a = attn[t.idx];
            const int C = a.C, H = t.x.H, HW = H * H;
            const size_t tok = (size_t)N * HW;
            const float scale = 1.0f / sqrtf((float)(C / cfg.num_heads));
            float* d_xs = gm.have(t.xs);
            VD_REQUIRE(dry || d_xs, "backward: attention output without a gradient");
            if (!d_xs) d_xs = gm.get(Tens{t.xs, C, H}, N, &fresh);
            float* dxin = gm.get(t.x, N, &fresh);
            const size_t mk = ar.mark();
            float* d_o2 = ar.get<float>(tok * C);
            float* d_qkv = ar.get<float>(tok * 3 * C);
            float* d_xn2 = ar.get<float>(tok * C);
            float* d_xt = ar.get<float>(tok * C);
            float* d_o = ar.get<float>(tok * C);
            float* d_xn = ar.get<float>(tok * C);
            AttnSpatialArgs sa{t.qkv2, nullptr, N, HW, C, cfg.num_heads, scale};
            float* sws = ar.get<float>(attn_spatial_bwd_ws_floats(sa));
            if (!dry) {
                // spatial half: xs = xn2 + proj(attn(qkv(xn2))), xn2 = gn(xt)
                if ((rc = bwd_linear(d_xs, (int)tok, a.sp.projw, nullptr, d_o2, st))) return rc;
                if ((rc = launch_attn_spatial_bwd(sa, d_o2, d_qkv, sws, st))) return rc;
                if ((rc = bwd_linear(d_qkv, (int)tok, a.sp.qkvw, d_xs, d_xn2, st))) return rc;
            }
            if ((rc = gn_bwd(Tens{t.xt, C, H}, nullptr, t.A, t.Bf, t.mr, d_xn2, 0, d_xt, 0, nullptr, 0, nullptr))) return rc;
            if (!dry) {
                // temporal half: xt = xn + proj(attn(qkv(xn), R)), xn = temporal gn(x)
                if ((rc = bwd_linear(d_xt, (int)tok, a.tp.projw, nullptr, d_o, st))) return rc;
                AttnTemporalArgs ta{t.qkv, t.Rk, t.Rq, t.Rv, t.amask, nullptr, t.B, t.T, HW, C, cfg.num_heads, cfg.allow_interactions_between_padding, scale};
                if ((rc = launch_attn_temporal_bwd(ta, d_o, d_qkv, st))) return rc;
                if ((rc = bwd_linear(d_qkv, (int)tok, a.tp.qkvw, d_xt, d_xn, st))) return rc;
                if ((rc = launch_gn_temporal_bwd(t.x.p, W(a.tp.normw), d_xn, t.B, t.T, HW, C, !fresh, dxin, st))) return rc;
            }
            ar.release(mk);
        } else if (op.kind == 5) {                                       // ---- + positional encodings: the gradient passes
            const TapePos& t = tape->pos[op.i];
            float* d_y = gm.have(t.out.p);
            VD_REQUIRE(dry || d_y, "backward: positional-encoding output without a gradient");
            if (!d_y) d_y = gm.get(t.out, N, &fresh);
            float* d_h = gm.get(t.in, N, &fresh);
            if (!dry && (rc = launch_add(d_y, (size_t)N * t.in.H * t.in.H * t.in.C, !fresh, d_h, st))) return rc;
        } else {
            const TapeConv& t = tape->conv[op.i];
            const ConvP& c = convs[t.idx];
            float* d_out = gm.have(t.out.p);
            VD_REQUIRE(dry || d_out, "backward: conv output without a gradient");
            if (!d_out) d_out = gm.get(t.out, N, &fresh);
            if (t.type == 0) {                                           // ---- stem: dcols = dy * W, then col2im onto x
                const size_t mk = ar.mark();
                float* dcols = ar.get<float>((size_t)N * S * S * STEM_KPAD);
                if (!dry) {
                    if ((rc = bwd_linear(d_out, N * S * S, c.w, nullptr, dcols, st))) return rc;
                    if ((rc = launch_stem_col2im(dcols, in.obs, in.lat, in.km, N, S, S, STEM_KPAD, cfg.cond_emb_type, dx, st))) return rc;
                }
                ar.release(mk);
            } else if (t.type == 3) {                                    // ---- Downsample (stride 2): stride-1 conv of the zero-stuffed gradient
                float* d_in = gm.get(t.in, N, &fresh);
                const size_t mk = ar.mark();
                float* dz = ar.get<float>((size_t)N * t.in.H * t.in.H * c.c);
                if (!dry && (rc = launch_zero_stuff2(d_out, N, t.out.H, t.out.H, c.c, dz, st))) return rc;
                if ((rc = bwd_conv3(Tens{dz, c.c, t.in.H}, N, c.w, t.in.C, fresh ? nullptr : d_in, d_in, st, ar))) return rc;
                ar.release(mk);
            } else {                                                     // ---- Upsample: conv backward at 2H, then the 2x2 sums
                float* d_in = gm.get(t.in, N, &fresh);
                const size_t mk = ar.mark();
                float* dup = ar.get<float>((size_t)N * t.out.H * t.out.H * t.in.C);
                if ((rc = bwd_conv3(Tens{d_out, c.c, t.out.H}, N, c.w, t.in.C, nullptr, dup, st, ar))) return rc;
                if (!dry && (rc = launch_sumpool2(dup, N, t.in.H, t.in.H, t.in.C, !fresh, d_in, st))) return rc;
                ar.release(mk);
            }
        }
    }
    return 0;
}

// A Tape on the engine while this object lives: forward() records into it, backward() reads it, no return path leaves a dead one behind.
// Its own tape, or `kept`: one that outlives the scope (the held pass of vd_guide_begin / vd_guide_finish).
struct TapeScope {
    vd_engine* e; Tape tp;
    explicit TapeScope(vd_engine* e_, Tape* kept = nullptr) : e(e_) { e->tape = kept ? kept : &tp; }
    ~TapeScope() { e->tape = nullptr; }
    TapeScope(const TapeScope&) = delete;
};

// The workspace of a differentiated pass (vd_guided_step, vd_dps_step, vd_eps_vjp, vd_ode_nll_eval) on a (B, T) window: the arena of the
// taped forward and the backward, and the pass's own buffers, which END where the buffer ends (ws_cap, also where a larger window grew it):
//   a header of kHeader bytes in rows of kRow floats: t_model [B] | obs_net [B*T] | lat_net [B*T] (the guided step's network masks) | gscale
//   kSlots slots of tot floats: eps | deps (ode_nll: the probe) | dxd | mean0 | dx_net | xstart0 | r | the fp64 partial sums (8-byte rounded)
// mean0 and xstart0 are the guided step's alone, r and the partials dps's and ode_nll's.  Addresses: valid behind ensure_ws_guided(B, T).
struct DiffWs {
    static constexpr int kRow = 256, kHeader = 4096, kSlots = 8;      // B <= kRow, and B * T <= kRow where the masks are written
    const vd_engine* e; size_t tot;
    DiffWs(const vd_engine* e_, int B, int T) : e(e_), tot((size_t)B * T * 3 * e_->cfg.image_size * e_->cfg.image_size) {}
    size_t bytes() const { return kHeader + kSlots * tot * sizeof(float); }
    bool partials_fit(size_t doubles) const { return doubles * sizeof(double) + 8 <= tot * sizeof(float); }
    char* tail() const { return e->ws + e->ws_cap - bytes(); }
    float* row(int i) const { return reinterpret_cast<float*>(tail()) + i * kRow; }
    float* slot(size_t i) const { return reinterpret_cast<float*>(tail() + kHeader) + i * tot; }
    float* t_model() const { return row(0); }   float* obs_net() const { return row(1); }   float* lat_net() const { return row(2); }
    float* eps() const { return slot(0); }      float* deps() const { return slot(1); }     float* probe() const { return slot(1); }
    float* dxd() const { return slot(2); }      float* mean0() const { return slot(3); }    float* dx_net() const { return slot(4); }
    float* xstart0() const { return slot(5); }  float* r() const { return slot(6); }        float* gscale() const { return row(3); }      // launch_grad_rescale's words
    double* partials() const { return reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(slot(7)) + 7) & ~(uintptr_t)7); }
    Arena arena() const { Arena a; a.base = e->ws; a.cap = (size_t)(tail() - e->ws); return a; }      // forward + backward live below the tail
};

// workspace of a differentiated pass: forward (taped, nothing released that the backward reads) + backward + DiffWs's tail
int vd_engine::ensure_ws_guided(int B, int T) {
    const long long key = ((long long)B << 32) | (unsigned)T | (1ll << 62);
    size_t tail = 0;
    int rc = grow_ws(key, DiffWs(this, B, T).bytes(), [&](size_t* peak) {
        Arena dry; dry.dry = true;
        TapeScope ts(this);
        FwdIn fi{}; fi.B = B; fi.T = T;
        int frc = forward(fi, nullptr, dry);
        if (!frc) frc = backward(fi, nullptr, nullptr, nullptr, dry);
        *peak = dry.peak;
        return frc;
    }, &tail);
    if (!rc) ws_B = ws_T = 0;              // the plain step recomputes its tail offsets on its next call
    return rc;
}

// device workspace of one operator call: released once the call's launches have run
struct OpScratch {
    hipStream_t st;
    std::vector<void*> bufs;
    explicit OpScratch(void* stream) : st(static_cast<hipStream_t>(stream)) {}
    template <class Tp> int get(Tp** p, size_t n) { VD_HIP(hipMalloc(reinterpret_cast<void**>(p), n * sizeof(Tp))); bufs.push_back(*p); return 0; }
    ~OpScratch() { if (!bufs.empty()) (void)hipStreamSynchronize(st); for (void* p : bufs) (void)hipFree(p); }
};

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char* vd_last_error(void) { return g_last_error.c_str(); }
const char* vd_version(void) {
    return math_mode() == MATH_F16X3 ? "vdamd 0.4 (gfx950; VD_MATH=f16x3: fp32 operands as two fp16 pieces (22 significand bits), three piece products, fp32 accumulation)"
           : math_mode() == MATH_BF16X6 ? "vdamd 0.4 (gfx950; VD_MATH=bf16x6: fp32 operands split exactly into three bf16 pieces, six piece products, fp32 accumulation)"
                                        : "vdamd 0.4 (gfx950; VD_MATH=fp32: every matrix product on the fp32 MFMA)";
}

int vd_create(const vd_config* cfg, vd_engine** out) {
    VD_REQUIRE(cfg && out, "null argument");
    vd_engine* e = new vd_engine();
    e->cfg = *cfg;
    int rc = e->build();
    if (rc) { delete e; return rc; }
    *out = e;
    return 0;
}

void vd_destroy(vd_engine* e) { if (e) (void)vd_guide_abort(e); delete e; }

int vd_param_count(vd_engine* e) { return e ? (int)e->params.size() : -1; }

int vd_param_info(vd_engine* e, int i, char* name, int cap, int* ndim, long long shape[4]) {
    VD_REQUIRE(e && i >= 0 && i < (int)e->params.size(), "parameter index");
    const Param& p = e->params[i];
    if (name && cap > 0) { std::strncpy(name, p.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (ndim) *ndim = p.nd;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = k < p.nd ? p.shape[k] : 1;
    return 0;
}

long long vd_weights_bytes(vd_engine* e) { return e ? (long long)(e->packed_total * sizeof(float)) : -1; }

// FNV-1a over everything that decides where a parameter's bytes sit in the packed buffer and how they are encoded
unsigned long long vd_weights_layout_id(vd_engine* e) {
    if (!e) return 0;
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](unsigned long long v) { for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xff; h *= 1099511628211ull; } };
    mix(math_mode()); mix(e->packed_total); mix(e->params.size());
    for (const Param& p : e->params) {
        for (char c : p.name) mix((unsigned char)c);
        mix(p.kind); mix(p.off); mix(p.packed); mix(p.frag_rows); mix(p.frag_row0);
    }
    return h;
}

// One process drives one GPU (the reference's launcher does the same, command_launchers.py:32-62): kernel attributes and
// CU counts are cached process-wide, an engine owns one workspace and runs its steps on one stream at a time.
static int g_bound_device = -1;

int vd_set_weight_storage(vd_engine* e, void* buf, long long bytes) {
    VD_REQUIRE(e && buf, "null argument");
    VD_REQUIRE(bytes >= (long long)(e->packed_total * sizeof(float)), "weight buffer too small");
    int dev = -1;
    VD_HIP(hipGetDevice(&dev));
    if (g_bound_device < 0) g_bound_device = dev;
    VD_REQUIRE(dev == g_bound_device, "libvdamd drives ONE device per process (one process per GPU); this process is already bound to another device");
    e->device = dev;
    // every captured forward holds addresses inside the image it was captured on: graphs go before another buffer takes its place
    if (e->wbuf && e->wbuf != static_cast<float*>(buf)) { if (e->win_cur >= 0) e->win_lost = true; e->drop_window_graphs(); }
    e->wbuf_on_host = false;
    e->wbuf = static_cast<float*>(buf);
    return 0;
}

int vd_set_weight_storage_host(vd_engine* e, void* host_buf, long long bytes) {
    VD_REQUIRE(e && host_buf, "null argument");
    VD_REQUIRE(bytes >= (long long)(e->packed_total * sizeof(float)), "weight buffer too small");
    // (as vd_set_weight_storage: the engine stops tracking the device image the captured graphs read)
    if (e->wbuf && e->wbuf != static_cast<float*>(host_buf)) { if (e->win_cur >= 0) e->win_lost = true; e->drop_window_graphs(); }
    e->wbuf = static_cast<float*>(host_buf);
    e->wbuf_on_host = true;
    return 0;
}

int vd_load_weight(vd_engine* e, const char* name, const float* host, long long numel) {
    VD_REQUIRE(e && name && host, "null argument");
    VD_REQUIRE(e->wbuf, "vd_set_weight_storage first");
    auto it = e->pidx.find(name);
    if (it == e->pidx.end()) { set_error(std::string("unexpected key in state_dict: ") + name); return -1; }
    Param& p = e->params[it->second];
    if ((long long)p.numel != numel) {
        set_error("size mismatch for " + p.name + ": expected " + std::to_string(p.numel) + " got " + std::to_string(numel));
        return -1;
    }
    std::vector<float> tmp;
    const float* src = host;
    int rc_put = 0;
    // a reload on a live model overwrites the image in place (captured graphs keep reading it: nothing is dropped); a step that reads the
    // weights may still run, on any stream, and a NULL-stream copy is not ordered behind torch's side streams.  Nothing has run before
    // the workspace exists.
    if (!e->wbuf_on_host && e->ws) VD_HIP(hipDeviceSynchronize());
    if (p.kind == PK_LINF && split_math()) {
        // rows [row0, row0+rows) of a [frag_rows][K] matrix -> K/16 contiguous pieces of its bf16-split fragment image
        const int rows = (int)p.shape[0], K = (int)p.shape[1];
        std::vector<unsigned short> sp(split_image_u16(rows, K));
        pack_linear_split(host, sp.data(), rows, K, rows, 0);
        const size_t piece = (size_t)(rows / 32) * 1536;                   // ushorts per k-step of this member
        for (int ks = 0; ks < K / 16; ++ks) {
            float* dst = e->wbuf + p.off + ((size_t)ks * (p.frag_rows / 32) + p.frag_row0 / 32) * 768;
            if ((rc_put = e->put(dst, sp.data() + ks * piece, piece * sizeof(unsigned short)))) return rc_put;
        }
        // the rows' scales and reciprocals into the trailer of the whole (batched) image
        const float* tr = reinterpret_cast<const float*>(sp.data() + (size_t)rows * K * 3);
        float* trd = e->wbuf + p.off + (size_t)p.frag_rows * K * 3 / 2;
        if ((rc_put = e->put(trd + p.frag_row0, tr, rows * sizeof(float)))) return rc_put;
        if ((rc_put = e->put(trd + p.frag_rows + p.frag_row0, tr + rows, rows * sizeof(float)))) return rc_put;
        p.loaded = true;
        return 0;
    }
    if (p.kind == PK_LINF) {
        // rows [row0, row0+rows) of a [frag_rows][K] matrix -> K/32 contiguous pieces of its fragment-major image
        const int rows = (int)p.shape[0], K = (int)p.shape[1];
        tmp.resize(p.numel);
        pack_linear_frag(host, tmp.data(), rows, K, rows, 0);
        const size_t piece = (size_t)(rows / 32) * 1024;
        for (int ch = 0; ch < K / 32; ++ch) {
            float* dst = e->wbuf + p.off + ((size_t)ch * (p.frag_rows / 32) + p.frag_row0 / 32) * 1024;
            if ((rc_put = e->put(dst, tmp.data() + ch * piece, piece * sizeof(float)))) return rc_put;
        }
        p.loaded = true;
        return 0;
    }
    if (p.kind == PK_CONV3W && split_math()) {
        tmp.resize(p.packed);
        pack_conv3_wino_split(host, reinterpret_cast<unsigned short*>(tmp.data()), (int)p.shape[0], (int)p.shape[1]);
        src = tmp.data();
    } else if (p.kind == PK_CONV3WU) {
        tmp.resize(p.packed);
        pack_conv3_wino_ups(host, reinterpret_cast<unsigned short*>(tmp.data()), (int)p.shape[0], (int)p.shape[1]);
        src = tmp.data();
    } else if (p.kind == PK_CONV3W) {
        tmp.resize(p.packed);
        pack_conv3_wino(host, tmp.data(), (int)p.shape[0], (int)p.shape[1]);
        src = tmp.data();
    } else if (p.kind == PK_CONV3S) {
        tmp.resize(p.packed);
        pack_conv3_split(host, reinterpret_cast<unsigned short*>(tmp.data()), (int)p.shape[0], (int)p.shape[1]);
        src = tmp.data();
    } else if (p.kind == PK_STEM) {                    // OIHW -> [O][k = tap*I + i] (zero padded) -> fragment-major linear
        const int O = (int)p.shape[0], I = (int)p.shape[1];
        std::vector<float> lin((size_t)O * STEM_KPAD, 0.f);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < 9; ++t) lin[(size_t)o * STEM_KPAD + t * I + i] = host[((size_t)o * I + i) * 9 + t];
        if (split_math()) {
            tmp.resize(p.packed);
            pack_linear_split(lin.data(), reinterpret_cast<unsigned short*>(tmp.data()), O, STEM_KPAD, O, 0);
        } else {
            tmp.resize((size_t)O * STEM_KPAD);
            pack_linear_frag(lin.data(), tmp.data(), O, STEM_KPAD, O, 0);
        }
        src = tmp.data();
    } else if (p.kind == PK_CONV3 || p.kind == PK_OUTCONV) {
        const int O = (int)p.shape[0], I = (int)p.shape[1];
        tmp.assign(p.packed, 0.f);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < 9; ++t) tmp[((size_t)t * O + o) * I + i] = host[((size_t)o * I + i) * 9 + t];
        if (p.kind == PK_OUTCONV) pack_out_head(host, O, I, tmp.data() + (size_t)9 * O * I);
        src = tmp.data();
    } else if (p.kind == PK_POSENC) {
        const int C = (int)p.shape[1], HW = (int)(p.shape[2] * p.shape[3]);
        tmp.resize((size_t)C * HW);
        for (int c = 0; c < C; ++c)
            for (int q = 0; q < HW; ++q) tmp[(size_t)q * C + c] = host[(size_t)c * HW + q];
        src = tmp.data();
    }
    if ((rc_put = e->put(e->wbuf + p.off, src, p.packed * sizeof(float)))) return rc_put;
    p.loaded = true;
    return 0;
}

int vd_weights_missing(vd_engine* e) {
    if (!e) return -1;
    int n = 0;
    for (auto& p : e->params) n += p.loaded ? 0 : 1;
    return n;
}

int vd_mark_weights_loaded(vd_engine* e) {
    VD_REQUIRE(e, "null argument");
    for (auto& p : e->params) p.loaded = true;
    return 0;
}

int vd_pos_channels(vd_engine* e) { return e ? e->pos_ch : -1; }
int vd_pos_resolution(vd_engine* e) { return e ? e->pos_res : -1; }

int vd_set_freqs(vd_engine* e, const float* tf, int nt, const float* ff, int nf) {
    VD_REQUIRE(e && tf && nt > 0, "time frequencies");
    // every captured forward reads the two tables: the graphs are dropped before a table they hold the address of is freed
    if (e->d_freq_time || (ff && nf > 0 && e->d_freq_frame)) { if (e->win_cur >= 0) e->win_lost = true; e->drop_window_graphs(); }
    if (e->d_freq_time) VD_HIP(hipFree(e->d_freq_time));
    VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_freq_time), nt * sizeof(float)));
    VD_HIP(hipMemcpy(e->d_freq_time, tf, nt * sizeof(float), hipMemcpyHostToDevice));
    e->n_freq_time = nt;
    if (ff && nf > 0) {
        if (e->d_freq_frame) VD_HIP(hipFree(e->d_freq_frame));
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_freq_frame), nf * sizeof(float)));
        VD_HIP(hipMemcpy(e->d_freq_frame, ff, nf * sizeof(float), hipMemcpyHostToDevice));
        e->n_freq_frame = nf;
    }
    return 0;
}

int vd_set_schedule(vd_engine* e, int nts, const float* tab, const int* tmap, float rescale) {
    VD_REQUIRE(e && tab && tmap && nts > 0, "schedule tables");
    // the tables' addresses, num_timesteps and rescale are kernel arguments of every captured window graph
    if (e->win_cur >= 0) e->win_lost = true;
    e->drop_window_graphs();
    e->drop_held();                      // vd_guide_finish's seed pass reads the rows of the schedule the pass began on
    if (e->d_tab) VD_HIP(hipFree(e->d_tab));
    if (e->d_tmap) VD_HIP(hipFree(e->d_tmap));
    if (e->d_w2m) { VD_HIP(hipFree(e->d_w2m)); e->d_w2m = nullptr; }      // the multistep weights belong to the schedule that goes
    if (e->d_unipc) { VD_HIP(hipFree(e->d_unipc)); e->d_unipc = nullptr; } // and so do unipc_sample's rows
    if (e->d_jump) { VD_HIP(hipFree(e->d_jump)); e->d_jump = nullptr; }   // and so do the jump rows
    VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_tab), (size_t)NTAB * nts * sizeof(float)));
    VD_HIP(hipMemcpy(e->d_tab, tab, (size_t)NTAB * nts * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float> tm(nts);
    for (int i = 0; i < nts; ++i) tm[i] = (float)tmap[i];
    VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_tmap), nts * sizeof(float)));
    VD_HIP(hipMemcpy(e->d_tmap, tm.data(), nts * sizeof(float), hipMemcpyHostToDevice));
    e->num_timesteps = nts;
    e->rescale = rescale;
    if (!e->d_err) {
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_err), sizeof(int)));
        VD_HIP(hipMemset(e->d_err, 0, sizeof(int)));
    }
    return 0;
}

// The dpmpp_2m extrapolation weights of the bound schedule, one float per respaced index (include/vd_amd.h).  A call of its own: the
// NTAB-row table of vd_set_schedule is public layout.  Captured sampler-3 graphs bake the row's address in: they are dropped when it moves.
int vd_set_multistep_weights(vd_engine* e, int nts, const float* w) {
    VD_REQUIRE(e && w, "multistep weights");
    VD_REQUIRE(e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(nts == e->num_timesteps, "multistep weights: one per index of the bound schedule (" + std::to_string(e->num_timesteps) + ")");
    if (e->d_w2m) {
        if (e->win_cur >= 0) e->win_lost = true;
        e->drop_window_graphs();
        VD_HIP(hipFree(e->d_w2m));
        e->d_w2m = nullptr;
    }
    VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_w2m), (size_t)nts * sizeof(float)));
    VD_HIP(hipMemcpy(e->d_w2m, w, (size_t)nts * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// unipc_sample's coefficient rows of the bound schedule, [UNIPC_ROWS][num_timesteps] (include/vd_amd.h).  A call of its own for the reason
// the multistep weights have one.  Captured sampler-5 graphs bake the table's address in: they are dropped when it moves.
int vd_set_unipc_rows(vd_engine* e, int nts, const float* rows) {
    VD_REQUIRE(e && rows, "unipc rows");
    VD_REQUIRE(e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(nts == e->num_timesteps, "unipc rows: " + std::to_string((int)UNIPC_ROWS) + " rows of one entry per index of the bound schedule (" + std::to_string(e->num_timesteps) + ")");
    if (e->d_unipc) {
        if (e->win_cur >= 0) e->win_lost = true;
        e->drop_window_graphs();
        VD_HIP(hipFree(e->d_unipc));
        e->d_unipc = nullptr;
    }
    VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_unipc), (size_t)UNIPC_ROWS * nts * sizeof(float)));
    VD_HIP(hipMemcpy(e->d_unipc, rows, (size_t)UNIPC_ROWS * nts * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// The coefficients of one forward diffusion step of the bound schedule, sqrt(1 - beta) | sqrt(beta) per respaced index (include/vd_amd.h:
// vd_q_jump).  Rows of their own for the reason the multistep weights are, and because 1 - TAB_ALPHA in fp32 loses three digits at beta = 1e-4.
// No captured graph reads them (vd_window_jump launches plainly): nothing is dropped.
int vd_set_jump_rows(vd_engine* e, int nts, const float* sqrt_alpha, const float* sqrt_beta) {
    VD_REQUIRE(e && sqrt_alpha && sqrt_beta, "jump rows");
    VD_REQUIRE(e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(nts == e->num_timesteps, "jump rows: one entry per index of the bound schedule (" + std::to_string(e->num_timesteps) + ")");
    if (!e->d_jump) VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_jump), 2 * (size_t)nts * sizeof(float)));
    VD_HIP(hipDeviceSynchronize());                  // a jump still in flight reads the old rows
    VD_HIP(hipMemcpy(e->d_jump, sqrt_alpha, (size_t)nts * sizeof(float), hipMemcpyHostToDevice));
    VD_HIP(hipMemcpy(e->d_jump + nts, sqrt_beta, (size_t)nts * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// ModelMeanType of the bound diffusion (gaussian_diffusion.py:29-36): 0 EPSILON (default), 1 START_X (predict_xstart=True,
// script_util.py:429-431).  Captured window graphs bake it in: they are dropped on a change.
int vd_set_model_mean_type(vd_engine* e, int type) {
    VD_REQUIRE(e && (type == 0 || type == 1), "model mean type: 0 EPSILON, 1 START_X");
    if (type != e->mean_type) { if (e->win_cur >= 0) e->win_lost = true; e->drop_window_graphs(); }
    e->mean_type = type;
    return 0;
}

int vd_device_errors(vd_engine* e, int* flags) {
    VD_REQUIRE(e && flags, "null argument");
    *flags = 0;
    if (!e->d_err) return 0;
    // The steps may have run on any stream -- torch's side streams are non-blocking, and a NULL-stream copy is not ordered behind
    // those: wait for the whole device first, so that the word read is the word every step issued so far has left, and the clear
    // cannot race a step still in flight (read + clear are then two operations on an idle device).
    VD_HIP(hipDeviceSynchronize());
    VD_HIP(hipMemcpy(flags, e->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (*flags) { VD_HIP(hipMemset(e->d_err, 0, sizeof(int))); VD_HIP(hipDeviceSynchronize()); }
    return 0;
}

// Test hook (include/vd_amd.h): every engine-owned SCRATCH buffer set to `byte` over its whole capacity, so that a test can say what
// a call finds in memory it has not written yet.  The rule: a buffer is scratch when no call reads it before that same call has
// written it; everything else is state and is not touched.  Every device pointer of struct vd_engine, once:
//
//   SCRATCH  ws                the activation arena and the step's tail (t_model, the two network outputs, the guidance scratch, DiffWs's
//                              tail): each forward, backward and step writes what it reads.  A held loss-guidance pass keeps its tape
//                              and eps there across two C calls: the fill ends it first, by name
//            d_fu              h', skip', the structure map and the two statistics tables of one FreeU block
//            d_lin_r           the residual between the linear projection's two passes
//            d_part_scratch    the gather's copy of the tensors it permutes
//            d_part_r          the built-in reward's residual
//            d_part_partials   ... and its per-block sums, folded by particle_weights_kernel in the same step
//            d_part_x0         the x_0 prediction of a steered window whose sampler keeps none, written by the step that reads it
//            d_part            the NLL entries' per-block sums
//            d_score_xt        vd_score_windows' x_t
//            d_score_list      ... and its suffix list, uploaded by the call that reads it (its first n entries, n of that call)
//   STATE    d_freq_time, d_freq_frame, d_tab, d_tmap, d_w2m, d_unipc, d_jump     the tables of the setters
//            d_hid, d_out      the relative-position nets' offset tables (rpe_tables)
//            d_cfg_zero        zeroed when it grows, read by every cfg_scale step after that
//            d_fu_trig         FreeU's cos / sin tables
//            d_blur_taps, d_lin_mats, d_part_sel                                  taps, operator matrices, the reward's selector rows
//            d_part_logw, d_part_rprev, d_part_ess, d_part_anc, d_part_chosen, d_part_counters    the particle state
//            d_err             the sticky flags
//            d_win_t, d_win_rng                                                   the armed window's counters and Philox triple
//            d_win_hist, d_win_ubase, d_win_ud2                                   ... and its carried history (the first step of a window does not
//                              read them: state from the second step on)
//            d_win_xtm1        redrawn by every step of an 'x_t_minus_1' window before the forward reads it: scratch in effect, kept as
//                              state because it belongs to the armed window
//            d_lists           a window graph's frame lists (WinGraph, beside its prefix store: state as well)
// The weights (wbuf, wbuf_bwd) are the caller's.  No address changes: nothing grows, nothing is freed, and the captured window graphs stay.
int vd_scratch_fill(vd_engine* e, int byte, long long* bytes_filled) {
    VD_REQUIRE(e && bytes_filled && byte >= 0 && byte <= 255, "scratch_fill: an engine, a byte 0..255 and where to report the bytes");
    *bytes_filled = 0;
    if (e->device >= 0) if (int rc = require_device(e->device, "engine")) return rc;
    e->end_held("dropped by vd_scratch_fill: the workspace the pass lives in was overwritten");
    VD_HIP(hipDeviceSynchronize());
    long long total = 0;
    auto fill = [&](void* p, size_t bytes) -> int {
        if (!p || !bytes) return 0;
        VD_HIP(hipMemset(p, byte, bytes));
        total += (long long)bytes;
        return 0;
    };
    int rc = fill(e->ws, e->ws_cap);
    if (!rc) rc = fill(e->d_fu, e->fu_cap * sizeof(float));
    if (!rc) rc = fill(e->d_lin_r, e->lin_r_cap * sizeof(float));
    if (!rc) rc = fill(e->d_part_scratch, e->part_scratch_cap * sizeof(float));
    if (!rc) rc = fill(e->d_part_r, e->part_r_cap * sizeof(float));
    if (!rc) rc = fill(e->d_part_partials, e->part_partials_cap * sizeof(double));
    if (!rc) rc = fill(e->d_part_x0, e->part_x0_cap * sizeof(float));
    if (!rc) rc = fill(e->d_part, e->part_cap * sizeof(double));
    if (!rc) rc = fill(e->d_score_xt, e->score_xt_cap * sizeof(float));
    if (!rc) rc = fill(e->d_score_list, e->score_list_cap * sizeof(int));
    if (rc) return rc;
    VD_HIP(hipDeviceSynchronize());
    *bytes_filled = total;
    return 0;
}

int vd_workspace_bytes(vd_engine* e, int B, int T, long long* bytes) {
    VD_REQUIRE(e && bytes && B > 0 && T > 0, "arguments");
    Arena dry; dry.dry = true;
    FwdIn fi{}; fi.B = B; fi.T = T;
    int rc = e->forward(fi, nullptr, dry);
    if (rc) return rc;
    *bytes = (long long)(((dry.peak + 255) & ~(size_t)255) + e->step_tail_bytes(B, T));      // the arena, then the step's tail (both output buffers)
    return 0;
}

static int check_ready(vd_engine* e, int B, int T) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(B > 0 && T > 0 && T <= kMaxWindowFrames, "window of 1.." + std::to_string(kMaxWindowFrames) + " frames (vd_max_window_frames)");
    VD_REQUIRE(e->wbuf && !e->wbuf_on_host, "weights not set (the packed image must live in device memory: vd_set_weight_storage)");
    int miss = vd_weights_missing(e);
    if (miss) {
        for (auto& p : e->params) if (!p.loaded) { set_error("missing key in state_dict: " + p.name + " (+" + std::to_string(miss - 1) + " more)"); break; }
        return -1;
    }
    return 0;
}

// the opening checks of the sampler entry points (vd_p_sample / vd_ddim_sample / vd_p_mean_variance / vd_window_begin): their
// steps end in the 3-channel posterior kernel, which a 6-channel network output must never reach
static int check_sampler(vd_engine* e, int B, int T, int obs_mode, int max_obs_mode, const char* obs_modes) {
    int rc = check_ready(e, B, T);
    if (rc) return rc;
    VD_REQUIRE(e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(obs_mode >= 0 && obs_mode <= max_obs_mode, obs_modes);
    VD_REQUIRE(!e->cfg.learn_sigma, "learn_sigma: the reference's sampler asserts on video tensors (gaussian_diffusion.py:283: model_output.shape == (B, 2*T, ...)); only the network forward is served");
    return 0;
}
static const char* const kObsModes = "observed_frames must be x_0 / x_t / x_t_minus_1";

int vd_max_window_frames(void) { return kMaxWindowFrames; }
int vd_gn_max_channels(void) { return kGnMaxChannels; }

int vd_unet_forward(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs,
                    const float* lat, const float* km, const long long* fidx, const float* t_model, int obs_mode,
                    float* eps, void* stream) {
    int rc = check_ready(e, B, T);
    if (rc) return rc;
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t_model && eps, "null tensor");
    VD_REQUIRE(obs_mode >= 0 && obs_mode <= 2, kObsModes);
    if ((rc = e->ensure_ws(B, T))) return rc;
    Arena ar = e->step_arena();
    FwdIn fi{B, T, x, obs_src, obs, lat, km, t_model, reinterpret_cast<const int64_t*>(fidx), obs_mode, eps};
    FreeUReq fq;
    if (e->freeu_on()) {                             // FreeU acts inside the network: the bare forward runs it too
        if ((rc = e->freeu_workspace(B, T)) || (rc = e->freeu_request(B, T, e->fu_b, e->fu_s, e->fu_adaptive, &fq))) return rc;
        fi.fu = &fq;
    }
    return e->forward(fi, static_cast<hipStream_t>(stream), ar);
}

// _WrappedModel.__call__ (respace.py:111-119): t_model = map[t] * rescale.  The reference raises IndexError for an index
// outside the table; here the step stays asynchronous: the network is fed NaN, the posterior kernel writes NaN for that
// batch element (misc.hip) and bit 0 of the engine's sticky error word is set for vd_device_errors().
__global__ void map_t_kernel(const int64_t* t, const float* tmap, float rescale, int B, int nts, float* out, int* err) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        const long long i = t[b];
        if (i < 0 || i >= nts) {
            out[b] = __builtin_nanf("");
            atomicOr(err, 1);
        } else {
            out[b] = tmap[i] * rescale;
        }
    }
}

static void map_t(const vd_engine* e, const long long* t, int B, float* tm, hipStream_t st) {
    hipLaunchKernelGGL(map_t_kernel, dim3((B + 63) / 64), dim3(64), 0, st, reinterpret_cast<const int64_t*>(t), e->d_tmap,
                       e->rescale, B, e->num_timesteps, tm, e->d_err);
}

// cfg_scale != 1: the all-zero observation mask of the unconditional forward, B*T floats.  Never inside a capture: a buffer that grew is
// zeroed on `st` and waited for, so that steps on any other stream find it zero.  Captured graphs hold its address (grow drops them).
static int cfg_zero_mask(vd_engine* e, int B, int T, hipStream_t st) {
    const size_t n = (size_t)B * T;
    if (n <= e->cfg_zero_cap) return 0;
    int rc = e->grow(e->d_cfg_zero, e->cfg_zero_cap, n, true);
    if (rc) return rc;
    VD_HIP(hipMemsetAsync(e->d_cfg_zero, 0, n * sizeof(float), st));
    VD_HIP(hipStreamSynchronize(st));
    return 0;
}

// One step, as the C entries and capture_window state it.
struct StepReq {
    int sampler;                                     // Sampler
    // the window tensors of one (B, T) batch, and the respaced index per item (device; the executor's moves between launches)
    int B, T;
    const float *x, *obs_src, *obs, *lat, *km;
    const long long* fidx;
    const long long* t;
    int obs_mode, clip;
    float eta = 0.f;
    // the noise of p_sample / ddim_sample: explicit, or Philox at (seed, offset), or at the {seed, offset} pair in device memory (`rng`)
    const float* noise = nullptr;
    unsigned long long seed = 0, offset = 0;
    const unsigned long long* rng = nullptr;
    // dpmpp_2m_sample, dpmpp_2m_sde_sample: the previous step's x_0 prediction or null; `hist_on` null, or a device word that is 0 while there is no history
    const float* hist = nullptr;
    const unsigned long long* hist_on = nullptr;
    // unipc_sample: the state read (x^c_{t+1}, D_{t+1}, D_{t+2}; all null: none) and written (all null: not kept; may be the tensors read), and
    // the chain's finished steps -- `count`, or the device word `hist_on` when that is set
    const float *ubase = nullptr, *ud1 = nullptr, *ud2 = nullptr;
    float *ubase_out = nullptr, *ud1_out = nullptr, *ud2_out = nullptr;
    int count = 0;
    // outputs, each optional except where the entry says otherwise; eps_out = the (guided) network output
    float *sample = nullptr, *xstart = nullptr, *mean = nullptr, *eps_out = nullptr;
    const PrefixPlan* pp = nullptr;
    const SuffixPlan* sp = nullptr;
    // the guidance constants of this step: the engine's switches (eager entries) or a window graph's key
    float cfg_w = 1.f, guid_phi = 0.f, dyn_p = 0.f;
    // FreeU (all four 1: off): the constants of the two decoder stages every forward of this step runs under, and the backbone form
    double fu_b[2] = {1.0, 1.0}, fu_s[2] = {1.0, 1.0};
    int fu_adaptive = 0;
    bool freeu() const { return fu_b[0] != 1.0 || fu_b[1] != 1.0 || fu_s[0] != 1.0 || fu_s[1] != 1.0; }
    // known region (null: none): the merge pass behind the sampler pass, in place on `sample`; its draws are known_noise, or Philox at
    // (known_seed, known_offset + B*per/4), or at the pair `rng` points to
    const float *known_src = nullptr, *known_mask = nullptr, *known_noise = nullptr;
    unsigned long long known_seed = 0, known_offset = 0;
    // measurement (null: none): the projection of the step's x_0 prediction onto y, in front of the sampler pass
    const float* meas_y = nullptr;
    int meas_scale = 1, meas_gray = 0;
    // particle steering with the built-in reward (part_K 0: none): behind the sampler pass the residual pass on the step's x_0 prediction, the
    // weights and the gather of `sample` and `xstart`; the uniforms are part_uni, or Philox at (part_seed, part_offset + 3/4 B per), or at
    // the pair `rng` points to
    int part_K = 0, part_scale = 1, part_gray = 0;
    const float* part_y = nullptr;
    double part_lambda = 0.0, part_tau = 0.0, part_sigma = 0.0;
    const double* part_uni = nullptr;
    unsigned long long part_seed = 0, part_offset = 0;
    // ... with the blur kernel as the reward's operator (part_blur_k 0: the cell mean at part_scale, part_gray)
    const float* part_taps = nullptr;
    int part_blur_k = 0;
    // ... with the linear operator as the reward's operator (part_lin_Mh 0: not)
    int part_lin_Mh = 0, part_lin_Mw = 0;
    // linear measurement (null: none): the projection of the step's x_0 prediction onto y under the engine's operator, in meas_y's place
    const float* lin_y = nullptr;
    int lin_Mh = 0, lin_Mw = 0;
};

// The window prefix cache and suffix skip cut a step short on the observed frames; two options need all of them.  cfg_scale != 1: in the
// unconditional forward the observed frames are padding frames whose content is whatever the window tensor holds -- neither "their
// network input cannot change" (prefix cache) nor "their output is never read" (suffix skip) holds for them.  Dynamic thresholding
// (`thresh`: on and clipping): its statistic runs over whole latent frames of the step.  (Guidance rescale acts only beside
// cfg_scale != 1: the first rule refuses it.)  vd_window_begin asks this of the engine's switches, step_launches of the plans it is handed.
static int refuse_cut_step(float cfg_w, bool thresh, bool prefix, bool suffix) {
    for (int i = 0; i < 2; ++i) {
        if (!(i ? suffix : prefix)) continue;
        const std::string sw = i ? "the window suffix skip (vd_set_window_suffix_skip)" : "the window prefix cache (vd_set_window_prefix_cache)";
        VD_REQUIRE(cfg_w == 1.f, "cfg_scale != 1 together with " + sw + " is not served");
        VD_REQUIRE(!thresh, "dynamic_threshold (vd_set_dynamic_threshold) together with " + sw + " is not served");
    }
    return 0;
}

// a sampler pass on the engine's tables: what the step and the network-free entries share; the caller adds its sampler's own fields
static SamplerPassArgs pass_args(const vd_engine* e, int sampler, int B, long long per, const float* x, const long long* t, int clip,
                                 float* sample, float* xstart) {
    SamplerPassArgs a{sampler, x, nullptr, nullptr, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, (long)per, clip,
                      sample, xstart, e->d_err};
    a.w = e->d_w2m;
    a.urows = e->d_unipc;
    return a;
}

// Particle steering with the built-in reward, behind the sampler pass (ensure_particle_ws has sized the buffers): the residual pass of
// dps.hip as it is -- handed (sample, pred_xstart) as its (x_t, eps) and the selector rows as its tables, its x_0 head gives the sample
// at t == 0 and pred_xstart elsewhere, exactly -- then the weights from its partials and the gather of both tensors (particles.hip).
static int particle_launches(vd_engine* e, const StepReq& r, const int64_t* t, size_t per, hipStream_t st) {
    const int B = r.B, T = r.T, S = e->cfg.image_size, K = r.part_K;
    VD_REQUIRE(r.part_y && r.sample && r.xstart, "particle steering: a step hands out its sample and its pred_xstart");
    VD_REQUIRE(!r.pp && !r.sp, "particle steering (vd_set_particles) together with the window prefix cache or suffix skip is not served");
    VD_REQUIRE(e->part_B == B && e->part_state_K == K && e->d_part_sel && e->part_sel_nt == e->num_timesteps, "particle steering: no state for this batch (vd_particle_reset)");
    int nblk = 0, rc;
    if (r.part_lin_Mh) {                                         // linop.hip's residual pass, handed the same tensors and rows
        LinopArgs la{r.sample, r.xstart, r.part_y, r.lat, t, e->d_part_sel, e->num_timesteps, B, T, S, S, r.part_lin_Mh, r.part_lin_Mw,
                     e->lin_mat(0), e->lin_mat(1), 0, e->d_part_r, e->d_part_partials, nullptr, nullptr, nullptr, nullptr, nullptr};
        ProfScope ps(PC_ELEMENTWISE, 2.0 * (r.part_lin_Mw + r.part_lin_Mh) * B * per, 4.0 * B * per * 3.0, st, "particle_linop_residual");
        if ((rc = launch_linop_residual(la, &nblk, st))) return rc;
    } else if (r.part_blur_k) {                                         // blur.hip's residual pass, handed the same tensors and rows
        BlurArgs ba{r.sample, r.xstart, r.part_y, r.lat, t, e->d_part_sel, e->num_timesteps, B, T, S, S, r.part_taps, r.part_blur_k, 0,
                    e->d_part_r, e->d_part_partials, nullptr, nullptr, nullptr, nullptr, nullptr};
        ProfScope ps(PC_ELEMENTWISE, 2.0 * r.part_blur_k * r.part_blur_k * B * per, 4.0 * B * per * 4.0, st, "particle_blur_residual");
        if ((rc = launch_blur_residual(ba, &nblk, st))) return rc;
    } else {
        DpsArgs da{r.sample, r.xstart, r.part_y, r.lat, t, e->d_part_sel, e->num_timesteps, B, T, S, S, r.part_scale, r.part_gray, 0,
                   e->d_part_r, e->d_part_partials, nullptr, nullptr, nullptr, nullptr, nullptr};
        ProfScope ps(PC_ELEMENTWISE, 2.0 * B * per, 4.0 * B * per * 2.0, st, "particle_residual");
        if ((rc = launch_dps_residual(da, &nblk, st))) return rc;
    }
    ParticleArgs pa{B / K, K, r.part_lambda, r.part_tau, nullptr, e->d_part_partials, nblk, 1.0 / (2.0 * r.part_sigma * r.part_sigma), t, r.part_uni,
                    e->d_part_logw, e->d_part_rprev, e->d_part_anc, e->d_part_chosen, e->d_part_ess, e->d_part_counters};
    pa.seed = r.part_seed; pa.offset = r.part_offset; pa.dstate = r.rng;
    pa.pos = (unsigned long long)B * per / 4 * 3;
    if ((rc = launch_particle_weights(pa, st))) return rc;
    GatherArgs ga{{r.sample, r.xstart, nullptr, nullptr}, 2, B, (long long)per, e->d_part_anc, e->d_part_scratch};
    ProfScope ps(PC_ELEMENTWISE, 0.0, 4.0 * B * per * 4.0, st, "particle_gather");
    return launch_particle_gather(ga, st);
}

// The launches of one step on `st`: t -> t_model, UNet forward, the sampler pass.  Nothing here allocates or waits, and `t`, `rng` and
// `hist_on` are read on the device, so the same launch sequence serves every step of a window (executor).
// cfg_w != 1 (cfg_scale): behind the forward a second one at the same batch size with the engine's all-zero observation mask (cfg_zero_mask
// has sized it) into the second output buffer, in the same arena, then cfg_combine_kernel in place over the first output -- which is what
// the sampler pass, and the caller's eps_out, then see.  Noise, t and the pass itself do not change.
// guid_phi != 0 with cfg_w != 1 (guidance rescale): the two passes of launch_cfg_rescale stand in for the combine pass.  dyn_p != 0 with
// clip (dynamic thresholding): launch_dynamic_threshold writes the finished x_0 into the second output buffer, and the sampler pass runs in
// its x0_given form with clip off -- the form `denoised_fn` uses, bit-matched to the fused step.  With both at 0 the launches are the ones above.
// known_src (a known region; run_step and vd_window_begin refuse it for a sampler that walks up): one more pass behind the sampler pass,
// launch_known_merge in place on the sample, drawing from the free quarter of the step's Philox range.  Null: no launch is added.
// meas_y (a measurement; refused together with a known region, a sampler that walks up and a cut step): one more pass in front of the
// sampler pass, launch_measurement_project.  Behind launch_dynamic_threshold it projects the finished x_0 in place; otherwise it forms
// x_0 itself (pass_x0: the sampler pass's head, clamp included) and writes the projected one into the second output buffer.  Either way
// the sampler pass then runs in its x0_given form with clip off, so pred_xstart, the mean and the 2M history are the projected x_0.
// Null: no launch is added.
// lin_y (a linear measurement; the same place, rules and refusals, and refused together with meas_y): two passes in front of the sampler
// pass, launch_linop_residual (x_0 and r = y - A x_0) and launch_linop_project (x_0 += P_h r P_w^T).  Null: no launch is added.
// part_K > 1 (particle steering with the built-in reward): particle_launches behind the sampler pass.  0: no launch is added.
static int step_launches(vd_engine* e, const StepReq& r, hipStream_t st) {
    int rc;
    const int B = r.B, T = r.T;
    const bool rescale = r.cfg_w != 1.f && r.guid_phi != 0.f, thresh = r.dyn_p != 0.f && r.clip;
    if ((rc = refuse_cut_step(r.cfg_w, thresh, r.pp != nullptr, r.sp != nullptr))) return rc;
    if (r.cfg_w != 1.f) {
        VD_REQUIRE(e->attn_cap_t.empty() && e->attn_cap_s.empty(), "cfg_scale != 1 together with return_attn_weights: a step makes two forwards");
        VD_REQUIRE(e->d_cfg_zero && e->cfg_zero_cap >= (size_t)B * T, "cfg_scale: zero observation mask not sized");
    }
    const size_t per = (size_t)T * 3 * e->cfg.image_size * e->cfg.image_size;
    float* tm = e->step_tm();
    float* eps = r.eps_out ? r.eps_out : e->step_eps(B);
    map_t(e, r.t, B, tm, st);
    Arena ar = e->step_arena();
    FwdIn fi{B, T, r.x, r.obs_src, r.obs, r.lat, r.km, tm, reinterpret_cast<const int64_t*>(r.fidx), r.obs_mode, eps};
    FreeUReq fq;
    if (r.freeu()) {                                 // both forwards of a cfg_scale step run it (fu = fi below)
        VD_REQUIRE(!r.pp && !r.sp, "FreeU (vd_set_freeu) together with the window prefix cache or suffix skip is not served");
        if ((rc = e->freeu_request(B, T, r.fu_b, r.fu_s, r.fu_adaptive, &fq))) return rc;
        fi.fu = &fq;
    }
    if ((rc = e->forward(fi, st, ar, r.pp, r.sp))) return rc;
    if (r.cfg_w != 1.f) {
        Arena au = e->step_arena();                  // the first forward's activations are dead: its output lives in the tail
        FwdIn fu = fi;
        fu.obs = e->d_cfg_zero; fu.eps = e->step_eps_u(B, T);
        if ((rc = e->forward(fu, st, au))) return rc;
        const long long n = (long long)e->out_floats(B, T);
        ProfScope ps(PC_ELEMENTWISE, 2.0 * n, rescale ? 20.0 * n : 12.0 * n, st, rescale ? "cfg_rescale" : "cfg_combine");
        if (rescale) rc = launch_cfg_rescale(eps, fu.eps, r.cfg_w, r.lat, B, T, (long)(per / T), r.guid_phi, eps, nullptr, e->step_guid(B, T), st);
        else rc = launch_cfg_combine(eps, fu.eps, r.cfg_w, n, eps, st);
        if (rc) return rc;
    }
    SamplerPassArgs pa = pass_args(e, r.sampler, B, (long long)per, r.x, r.t, r.clip, r.sample, r.xstart);
    // what the pass reads: the network output as eps, or an x_0 prediction -- the output of a START_X model
    // (pred_xstart = process_xstart(model_output), gaussian_diffusion.py:326-341) or the thresholded one
    (e->mean_type == 1 ? pa.x0_given : pa.eps) = eps;
    if (thresh) {                                    // the finished x_0 (out_u's buffer is free by now)
        DynThreshArgs da{eps, e->mean_type == 1 ? nullptr : r.x, pa.t, e->d_tab, e->num_timesteps, r.lat, B, T,
                         (long)(per / T), r.dyn_p, e->step_eps_u(B, T), nullptr, e->d_err, e->step_guid(B, T)};
        ProfScope ps(PC_ELEMENTWISE, 4.0 * B * per, 4.0 * B * per * 8.0, st, "dynamic_threshold");
        if ((rc = launch_dynamic_threshold(da, st))) return rc;
        pa.eps = nullptr; pa.x0_given = da.out;
        pa.clip = 0;
    }
    if (r.meas_y) {
        VD_REQUIRE(!r.pp && !r.sp, "a measurement (vd_set_measurement) together with the window prefix cache or suffix skip is not served");
        const int S = e->cfg.image_size;
        float* out = e->step_eps_u(B, T);
        // behind the threshold: its output, in place, as it is; else the network output through pass_x0 with the step's clamp
        MeasureArgs ma{thresh || e->mean_type == 1 ? nullptr : r.x, thresh ? out : eps, out, r.meas_y, r.lat, pa.t, e->d_tab, e->num_timesteps,
                       B, T, S, S, r.meas_scale, r.meas_gray, thresh ? 0 : r.clip};
        ProfScope ps(PC_ELEMENTWISE, 2.0 * B * per, 4.0 * B * per * (ma.x ? 3.0 : 2.0), st, "measurement_project");
        if ((rc = launch_measurement_project(ma, st))) return rc;
        pa.eps = nullptr; pa.x0_given = out;
        pa.clip = 0;
    }
    if (r.lin_y) {
        VD_REQUIRE(!r.pp && !r.sp, "a linear measurement (vd_set_linear_measurement) together with the window prefix cache or suffix skip is not served");
        const int S = e->cfg.image_size;
        float* out = e->step_eps_u(B, T);
        // the residual pass forms x_0 as launch_measurement_project does -- behind the threshold its output, in place, as it is; else the
        // network output through pass_x0 with the step's clamp -- and hands it out beside r; the second pass adds P_h r P_w^T in place
        LinopArgs la{thresh || e->mean_type == 1 ? nullptr : r.x, thresh ? out : eps, r.lin_y, r.lat, pa.t, e->d_tab, e->num_timesteps, B, T, S, S,
                     r.lin_Mh, r.lin_Mw, e->lin_mat(0), e->lin_mat(1), thresh ? 0 : r.clip, e->d_lin_r, nullptr, nullptr, nullptr, out, nullptr, nullptr};
        {
            ProfScope ps(PC_ELEMENTWISE, 2.0 * (r.lin_Mw + r.lin_Mh) * B * per, 4.0 * B * per * (la.x ? 3.0 : 2.0), st, "linop_residual");
            if ((rc = launch_linop_residual(la, nullptr, st))) return rc;
        }
        ProfScope ps(PC_ELEMENTWISE, 2.0 * (r.lin_Mw + r.lin_Mh) * B * per, 4.0 * B * per * 2.0, st, "linop_project");
        if ((rc = launch_linop_project(out, e->d_lin_r, r.lat, e->lin_mat(2), e->lin_mat(3), B, T, S, S, r.lin_Mh, r.lin_Mw, st))) return rc;
        pa.eps = nullptr; pa.x0_given = out;
        pa.clip = 0;
    }
    pa.mean = r.mean; pa.eta = r.eta; pa.noise = r.noise; pa.seed = r.seed; pa.offset = r.offset; pa.dstate = r.rng;
    pa.hist = r.hist; pa.hist_on = r.hist_on;
    if (sampler_is_unipc(r.sampler)) {
        pa.ubase = r.ubase; pa.ud1 = r.ud1; pa.ud2 = r.ud2; pa.count = r.count;
        pa.ubase_out = r.ubase_out; pa.ud1_out = r.ud1_out; pa.ud2_out = r.ud2_out;
    }
    if (!sampler_draws_noise(r.sampler)) rc = launch_sampler_pass(pa, st);
    else {
        ProfScope ps(PC_POSTERIOR, 0.0, 4.0 * B * per * 5.0, st);
        rc = launch_sampler_pass(pa, st);
    }
    if (!rc && r.part_K > 1) rc = particle_launches(e, r, pa.t, per, st);
    if (rc || !r.known_src || !r.sample) return rc;
    // known region: the known pixels of the latent frames of the sample, noised to the level the step just reached (known.hip)
    KnownMergeArgs ka{r.sample, r.known_src, r.known_mask, r.lat, pa.t, e->d_tab, e->num_timesteps, B, T, (long)(per / T / 3)};
    ka.noise = r.known_noise; ka.seed = r.known_seed; ka.offset = r.known_offset; ka.dstate = r.rng;
    ProfScope ps(PC_ELEMENTWISE, 2.0 * B * per, 4.0 * B * per * 3.0, st, "known_merge");
    return launch_known_merge(ka, st);
}

// what a sampler with history needs beside the schedule (run_step and vd_window_begin; `who` names the caller's sampler), and what sampler 5
// is refused together with: the corrector rebuilds the state from `base`, so a merge behind the pass would be discarded at the next step
static int require_history_rows(const vd_engine* e, int sampler, const std::string& who) {
    if (!sampler_has_history(sampler)) return 0;
    if (sampler_is_unipc(sampler)) {
        VD_REQUIRE(e->d_unipc, who + ": no coefficient rows for the bound schedule (vd_set_unipc_rows, after vd_set_schedule)");
        VD_REQUIRE(!e->known_src, who + " together with a known region (vd_set_known_region) is not served: the corrector rebuilds the state from its own, a merge behind the pass would be discarded");
        return 0;
    }
    VD_REQUIRE(e->d_w2m, who + ": no multistep weight row for the bound schedule (vd_set_multistep_weights, after vd_set_schedule)");
    return 0;
}

// what a measurement is refused together with, by name: the eager entries and vd_window_begin ask this of the engine's state
static int refuse_with_measurement(const vd_engine* e, int sampler) {
    VD_REQUIRE(!sampler_walks_up(sampler), std::string(sampler_name(sampler)) + " together with a measurement (vd_set_measurement) is not served: the projection constrains x_0 of a reverse step");
    VD_REQUIRE(!e->known_src, "a measurement (vd_set_measurement) together with a known region (vd_set_known_region) is not served");
    VD_REQUIRE(e->cfg.image_size % e->meas_scale == 0, "measurement: H and W must be divisible by scale");
    return 0;
}

// ... and a linear measurement, the same set under its own name, and the measurement itself
static int refuse_with_linear_measurement(const vd_engine* e, int sampler) {
    VD_REQUIRE(!sampler_walks_up(sampler), std::string(sampler_name(sampler)) + " together with a linear measurement (vd_set_linear_measurement) is not served: the projection constrains x_0 of a reverse step");
    VD_REQUIRE(!e->known_src, "a linear measurement (vd_set_linear_measurement) together with a known region (vd_set_known_region) is not served");
    VD_REQUIRE(!e->meas_y, "a linear measurement (vd_set_linear_measurement) together with a measurement (vd_set_measurement) is not served");
    VD_REQUIRE(e->lin_Mh && e->lin_back, "linear measurement: the installed operator has no back-projection (vd_set_linear_operator with P_h and P_w)");
    return 0;
}

// what particle steering (vd_set_particles) is refused together with, by name: a step whose sample is wanted asks this of the engine's state
static int refuse_with_particles(const vd_engine* e, int sampler, int B, float eta) {
    VD_REQUIRE(sampler_draws_noise(sampler) && (sampler != SAMPLER_DDIM || eta > 0.f), std::string(sampler_name(sampler)) + (sampler == SAMPLER_DDIM ? " at eta = 0" : "") +
               " together with particle steering (vd_set_particles) is not served: the step draws no noise, duplicated particles would never separate");
    VD_REQUIRE(B % e->part_K == 0, "particle steering (vd_set_particles): the batch of " + std::to_string(B) + " items is no multiple of the " + std::to_string(e->part_K) + " particles of a group");
    VD_REQUIRE(!e->known_src, "particle steering (vd_set_particles) together with a known region (vd_set_known_region) is not served");
    VD_REQUIRE(!e->meas_y, "particle steering (vd_set_particles) together with a measurement (vd_set_measurement) is not served");
    VD_REQUIRE(!e->lin_y, "particle steering (vd_set_particles) together with a linear measurement (vd_set_linear_measurement) is not served");
    VD_REQUIRE(e->attn_cap_t.empty() && e->attn_cap_s.empty(), "particle steering (vd_set_particles) together with return_attn_weights is not served");
    return 0;
}

// the particle state for B items, zeroed (never inside a capture; waits for the device: the steps that follow may run on any stream)
static int particle_state_reset(vd_engine* e, int B) {
    const size_t n = (size_t)B;
    if (n > e->part_state_cap) {
        size_t c0 = e->part_state_cap, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0;      // (one capacity for the six buffers)
        int rc = e->grow(e->d_part_logw, c0, n, true);
        if (!rc) rc = e->grow(e->d_part_rprev, c1, n, true);
        if (!rc) rc = e->grow(e->d_part_ess, c2, n, true);
        if (!rc) rc = e->grow(e->d_part_anc, c3, n, true);
        if (!rc) rc = e->grow(e->d_part_chosen, c4, n, true);
        if (!rc) rc = e->grow(e->d_part_counters, c5, 2 * n, true);
        if (rc) { e->part_state_cap = 0; return rc; }
        e->part_state_cap = n;
    }
    VD_HIP(hipMemset(e->d_part_logw, 0, n * sizeof(double)));
    VD_HIP(hipMemset(e->d_part_rprev, 0, n * sizeof(double)));
    VD_HIP(hipMemset(e->d_part_ess, 0, n * sizeof(double)));
    VD_HIP(hipMemset(e->d_part_anc, 0, n * sizeof(int)));
    VD_HIP(hipMemset(e->d_part_chosen, 0xff, n * sizeof(int)));
    VD_HIP(hipMemset(e->d_part_counters, 0, 2 * n * sizeof(long long)));
    VD_HIP(hipDeviceSynchronize());
    e->part_B = B; e->part_state_K = e->part_K;
    return 0;
}

// the buffers of the built-in reward for a (B, T) step (never inside a capture); x0: also the x_0 prediction of a window without history
static int ensure_particle_ws(vd_engine* e, int B, int T, bool x0) {
    const int S = e->cfg.image_size, sc = e->part_scale;
    const size_t per = (size_t)T * 3 * S * S;
    int rc = e->grow(e->d_part_r, e->part_r_cap, e->part_lin ? (size_t)B * T * 3 * e->lin_Mh * e->lin_Mw : e->part_blur ? (size_t)B * per : (size_t)B * T * (e->part_gray ? 1 : 3) * (S / sc) * (S / sc), true);
    if (!rc) rc = e->grow(e->d_part_partials, e->part_partials_cap, (size_t)B * dps_partials_per_item(), true);
    if (!rc) rc = e->grow(e->d_part_scratch, e->part_scratch_cap, 2 * (size_t)B * per, true);
    if (!rc && x0) rc = e->grow(e->d_part_x0, e->part_x0_cap, (size_t)B * per, true);
    if (rc) return rc;
    const int NT = e->num_timesteps;
    if (e->part_sel_nt != NT || !e->d_part_sel) {
        // rows TAB_SQRT_RECIP and TAB_SQRT_RECIPM1 as the residual pass reads them: x_0 = a x - b eps with (a, b) = (1, 0) at t == 0 -- the
        // sample -- and (0, -1) elsewhere -- pred_xstart; both exact
        if ((rc = e->grow(e->d_part_sel, e->part_sel_cap, 2 * (size_t)NT, true))) return rc;
        std::vector<float> rows(2 * (size_t)NT, 0.f);
        rows[0] = 1.f;
        for (int t = 1; t < NT; ++t) rows[(size_t)NT + t] = -1.f;
        VD_HIP(hipMemcpy(e->d_part_sel, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
        e->part_sel_nt = NT;
    }
    return 0;
}

// what a step needs sized before its launches (never inside a capture): the workspace, and the zero mask of a cfg_scale step
static int step_workspace(vd_engine* e, int B, int T, hipStream_t st) {
    int rc = e->ensure_ws(B, T);
    if (!rc && e->cfg_w != 1.f) rc = cfg_zero_mask(e, B, T, st);
    if (!rc && e->freeu_on()) rc = e->freeu_workspace(B, T);
    if (!rc && e->lin_y) rc = e->grow(e->d_lin_r, e->lin_r_cap, (size_t)B * T * 3 * e->lin_Mh * e->lin_Mw, true);
    return rc;
}

// An eager step under the engine's guidance switches: vd_p_sample and its siblings (the sample is wanted) and vd_p_mean_variance
static int run_step(vd_engine* e, StepReq r, bool want_sample, void* stream) {
    int rc = check_sampler(e, r.B, r.T, r.obs_mode, 2, kObsModes);
    if (rc) return rc;
    VD_REQUIRE(r.x && r.obs_src && r.obs && r.lat && r.km && r.fidx && r.t && (want_sample ? r.sample != nullptr : r.mean || r.xstart || r.eps_out),
               "null tensor");
    VD_REQUIRE(r.sampler != SAMPLER_DDIM || r.eta >= 0.f, "eta");
    if ((rc = require_history_rows(e, r.sampler, sampler_name(r.sampler)))) return rc;
    if (want_sample && e->part_K > 1 && (rc = refuse_with_particles(e, r.sampler, r.B, r.eta))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = step_workspace(e, r.B, r.T, st))) return rc;
    r.cfg_w = e->cfg_w; r.guid_phi = e->guid_phi; r.dyn_p = e->dyn_p;
    for (int i = 0; i < 2; ++i) { r.fu_b[i] = e->fu_b[i]; r.fu_s[i] = e->fu_s[i]; }
    r.fu_adaptive = e->fu_adaptive;
    if (want_sample && e->known_src) {
        VD_REQUIRE(!sampler_walks_up(r.sampler), std::string(sampler_name(r.sampler)) + " together with a known region (vd_set_known_region) is not served: the merge noises to t - 1");
        r.known_src = e->known_src; r.known_mask = e->known_mask; r.known_noise = e->known_noise;
        r.known_seed = e->known_seed; r.known_offset = e->known_offset;
    }
    if (e->meas_y) {
        if ((rc = refuse_with_measurement(e, r.sampler))) return rc;
        r.meas_y = e->meas_y; r.meas_scale = e->meas_scale; r.meas_gray = e->meas_gray;
    }
    if (e->lin_y) {
        if ((rc = refuse_with_linear_measurement(e, r.sampler))) return rc;
        r.lin_y = e->lin_y; r.lin_Mh = e->lin_Mh; r.lin_Mw = e->lin_Mw;
    }
    if (want_sample && e->part_K > 1 && e->part_y) {
        VD_REQUIRE(e->part_B == r.B && e->part_state_K == e->part_K, "particle steering: the state holds " + std::to_string(e->part_B) + " items in groups of " + std::to_string(e->part_state_K) + " (vd_particle_reset), the step " + std::to_string(r.B) + " in groups of " + std::to_string(e->part_K));
        VD_REQUIRE(e->part_draws_set, "particle steering: no uniforms for this step (vd_particle_draws)");
        if ((rc = ensure_particle_ws(e, r.B, r.T, false))) return rc;
        r.part_K = e->part_K; r.part_y = e->part_y; r.part_scale = e->part_scale; r.part_gray = e->part_gray;
        r.part_lambda = e->part_lambda; r.part_tau = e->part_tau; r.part_sigma = e->part_sigma;
        r.part_uni = e->part_uni; r.part_seed = e->part_seed; r.part_offset = e->part_offset;
        if (e->part_blur) { r.part_taps = e->d_blur_taps; r.part_blur_k = e->blur_k; }
        if (e->part_lin) { r.part_lin_Mh = e->lin_Mh; r.part_lin_Mw = e->lin_Mw; }
    }
    return step_launches(e, r, st);
}

int vd_p_mean_variance(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat,
                       const float* km, const long long* fidx, const long long* t, int obs_mode, int clip, float* mean,
                       float* xstart, float* eps, void* stream) {
    StepReq r{SAMPLER_P, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip};
    r.xstart = xstart; r.mean = mean; r.eps_out = eps;
    return run_step(e, r, false, stream);
}

int vd_vb_terms(vd_engine* e, int B, int T, const float* x_start, const float* x_t, const float* eps, const float* noise,
                const long long* t, int clip, const float* latent_mask, float* vb, float* xstart_mse, float* mse,
                float* pred_xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(!e->freeu_on(), "vb_terms (the NLL path) together with FreeU (vd_set_freeu) is not served: a likelihood is the trained model's");
    VD_REQUIRE(B > 0 && T > 0 && x_start && x_t && eps && t && vb, "arguments");
    VD_REQUIRE(mse == nullptr || noise != nullptr, "mse needs the noise x_t was drawn with");
    const long per = (long)T * 3 * e->cfg.image_size * e->cfg.image_size;
    const int nblk = vb_terms_blocks(per);
    int rc = e->grow(e->d_part, e->part_cap, (size_t)B * nblk * 3, false);
    if (rc) return rc;
    VbArgs a{x_start, x_t, eps, noise, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, latent_mask, B, T, per,
             clip, pred_xstart, e->d_part, nblk, vb, xstart_mse, mse};
    a.err = e->d_err;
    a.start_x = e->mean_type == 1;
    return launch_vb_terms(a, static_cast<hipStream_t>(stream));
}

int vd_prior_bpd(vd_engine* e, int B, int T, const float* x_start, const float* latent_mask, float* out, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && x_start && out, "arguments");
    const long per = (long)T * 3 * e->cfg.image_size * e->cfg.image_size;
    const int nblk = vb_terms_blocks(per);
    int rc = e->grow(e->d_part, e->part_cap, (size_t)B * nblk * 3, false);
    if (rc) return rc;
    return launch_prior_bpd(x_start, latent_mask, e->d_tab, e->num_timesteps, B, T, per, e->d_part, nblk, out,
                            static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------ observed-frame search
// One candidate evaluation of scripts/video_optimal_schedule.py:142-206 is run_bpd_evaluation at ONE timestep per item, of which the
// search reads `mse` only.  vd_score_windows is that: x_t from the item's own Philox stream, one forward in 'x_0' mode, and the
// latent frames' mean((eps' - noise)^2) in fp64 -- no KL / decoder-NLL terms, no noise or pred_xstart tensors, and (suffix_skip) no
// network suffix for the frames the score never reads.
static int score_args(vd_engine* e, int B, int T, const float* x_start, const float* eps, const long long* t, int clip, const float* lat,
                      unsigned long long seed, const unsigned long long* item_offset, const float* noise, ScoreArgs* a) {
    const long per = (long)T * 3 * e->cfg.image_size * e->cfg.image_size;
    const int nblk = vb_terms_blocks(per);
    int rc = e->grow(e->d_part, e->part_cap, (size_t)B * nblk, false);
    if (rc) return rc;
    *a = ScoreArgs{x_start, eps, noise, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, lat, B, T, per, clip,
                   e->mean_type == 1 ? 1 : 0, seed, item_offset, e->d_part, nblk, e->d_err};
    return 0;
}

int vd_op_eps_mse(vd_engine* e, int B, int T, const float* x_start, const float* eps, const long long* t, int clip, const float* lat,
                  unsigned long long seed, const unsigned long long* item_offset, const float* noise, double* mse_out, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && x_start && eps && t && lat && mse_out && (noise || item_offset), "arguments");
    ScoreArgs a;
    int rc = score_args(e, B, T, x_start, eps, t, clip, lat, seed, item_offset, noise, &a);
    if (rc) return rc;
    return launch_eps_mse(a, mse_out, static_cast<hipStream_t>(stream));
}

int vd_score_windows(vd_engine* e, int B, int T, const float* x_start, const float* obs, const float* lat, const float* km,
                     const long long* fidx, const long long* t, int clip, unsigned long long seed,
                     const unsigned long long* item_offset, const float* noise, int suffix_skip, double* mse_out, void* stream) {
    int rc = check_sampler(e, B, T, 0, 0, kObsModes);
    if (rc) return rc;
    VD_REQUIRE(x_start && obs && lat && km && fidx && t && mse_out && (noise || item_offset), "null tensor");
    VD_REQUIRE(!e->freeu_on(), "score_windows together with FreeU (vd_set_freeu) is not served: the search scores the model as trained");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = B * T;
    const size_t per = (size_t)T * 3 * e->cfg.image_size * e->cfg.image_size;
    // the suffix plan: the frames the score reads (latent_mask = 1), under vd_window_begin's conditions for the skip.  The list's
    // length shapes the launches, so the mask is read back first -- B*T floats, the only host wait of this entry (none without suffix_skip)
    SuffixPlan sp;
    if (suffix_skip && e->cfg.cond_emb_type == 0 && e->suf_blk >= -1 && !e->attn.empty()) {
        e->score_mask_h.resize(N);
        VD_HIP(hipMemcpyAsync(e->score_mask_h.data(), lat, N * sizeof(float), hipMemcpyDeviceToHost, st));
        VD_HIP(hipStreamSynchronize(st));          // (also: the previous call's list upload has left score_list_h)
        e->score_list_h.clear();
        for (int n = 0; n < N; ++n) if (e->score_mask_h[n] == 1.f) e->score_list_h.push_back(n);
        const int n_lat = (int)e->score_list_h.size();
        if (n_lat > 0 && n_lat < N) {
            if ((rc = e->grow(e->d_score_list, e->score_list_cap, (size_t)N, false))) return rc;
            VD_HIP(hipMemcpyAsync(e->d_score_list, e->score_list_h.data(), n_lat * sizeof(int), hipMemcpyHostToDevice, st));
            sp.n = n_lat; sp.list = e->d_score_list;
        }
    }
    if ((rc = e->ensure_ws(B, T, sp.n > 0))) return rc;
    if ((rc = e->grow(e->d_score_xt, e->score_xt_cap, (size_t)B * per, false))) return rc;
    float* eps = e->step_eps(B);
    ScoreArgs a;
    if ((rc = score_args(e, B, T, x_start, eps, t, clip, lat, seed, item_offset, noise, &a))) return rc;
    if ((rc = launch_score_q_sample(a, e->d_score_xt, st))) return rc;
    float* tm = e->step_tm();
    map_t(e, t, B, tm, st);
    Arena ar = e->step_arena();
    FwdIn fi{B, T, e->d_score_xt, x_start, obs, lat, km, tm, reinterpret_cast<const int64_t*>(fidx), 0, eps};
    if ((rc = e->forward(fi, st, ar, nullptr, sp.n > 0 ? &sp : nullptr))) return rc;
    return launch_eps_mse(a, mse_out, st);
}

// ------------------------------------------------------------------------------------------ window executor
// scripts/video_sample.py:149-168 runs `for timestep in reversed(range(num_timesteps)): local = p_sample(...)` from the
// host, ~330 launches per step.  Here the window's step index and Philox counter live in device memory, a step is ONE
// captured hipGraph (map_t -> UNet forward -> in-place posterior update -> advance the counters), cached per window
// signature, and a window is num_timesteps replays of it (BASELINE configs[4]).
__global__ void win_set_kernel(long long* t, unsigned long long* rng, int B, long long t_start, unsigned long long seed,
                               unsigned long long offset) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) t[b] = t_start;
    if (b == 0) { rng[0] = seed; rng[1] = offset; rng[2] = 0; }
}

__global__ void win_advance_kernel(long long* t, unsigned long long* rng, int B, long long dt, unsigned long long draws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) t[b] += dt;
    if (b == 0) { rng[1] += draws; rng[2] += 1; }
}

// ---- the steps of vd_window_begin
// the executor's device state for a window of B entries: the step counters, the Philox pair with the count of finished steps behind
// it, for a sampler with history B * per floats of it and, in 'x_t_minus_1' mode, the observed frames re-noised to t - 1 (per: floats of one entry)
static int window_buffers(vd_engine* e, int B, int obs_mode, int sampler, size_t per) {
    int rc = e->grow(e->d_win_t, e->win_t_cap, (size_t)B, true);
    if (rc) return rc;
    if (!e->d_win_rng) VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_win_rng), 3 * sizeof(unsigned long long)));
    if (sampler_has_history(sampler) && (rc = e->grow(e->d_win_hist, e->win_hist_cap, (size_t)B * per, true))) return rc;
    if (sampler_is_unipc(sampler) && ((rc = e->grow(e->d_win_ubase, e->win_ubase_cap, (size_t)B * per, true)) ||
                                      (rc = e->grow(e->d_win_ud2, e->win_ud2_cap, (size_t)B * per, true)))) return rc;
    return obs_mode == 2 ? e->grow(e->d_win_xtm1, e->win_xtm1_cap, (size_t)B * per, true) : 0;
}

// the frames whose network input cannot change during the window: pure observations (obs = 1, lat = 0); inv stays empty if none is
static int invariant_frames(const float* obs, const float* lat, int N, hipStream_t st, std::vector<unsigned char>* inv, int* n_inv) {
    std::vector<float> hm(2 * (size_t)N);
    VD_HIP(hipMemcpyAsync(hm.data(), obs, N * sizeof(float), hipMemcpyDeviceToHost, st));
    VD_HIP(hipMemcpyAsync(hm.data() + N, lat, N * sizeof(float), hipMemcpyDeviceToHost, st));
    VD_HIP(hipStreamSynchronize(st));
    inv->resize(N);
    for (int n = 0; n < N; ++n) { (*inv)[n] = hm[n] == 1.f && hm[N + n] == 0.f; *n_inv += (*inv)[n]; }
    if (*n_inv == 0) inv->clear();
    return 0;
}

static int find_window_graph(const vd_engine* e, const vd_engine::WinKey& key, const std::vector<unsigned char>& inv) {
    for (size_t i = 0; i < e->win_graphs.size(); ++i)
        if (e->win_graphs[i].key == key && e->win_graphs[i].inv == inv) return (int)i;
    return -1;
}

// 'x_t_minus_1' (gaussian_diffusion.py:565-568): obs_src holds the CLEAN observed frames x0; every step first draws
// x_t_minus_1 = q_sample(x0, t - 1) into the engine's buffer (the second half of the step's Philox range), the network reads that
static int renoise_observed(const vd_engine* e, const vd_engine::WinKey& k, hipStream_t st) {
    if (k.obs_mode != 2) return 0;
    const size_t per = (size_t)k.T * 3 * e->cfg.image_size * e->cfg.image_size;
    return launch_q_sample_prev(k.obs_src, reinterpret_cast<const int64_t*>(e->d_win_t), e->d_tab, e->num_timesteps, k.B, (long)per,
                                e->d_win_rng, (unsigned long long)k.B * per / 2, e->d_win_xtm1, st);
}

// the invariant frames' prefix, eagerly, into the graph's store (the window prefix cache is per window: its first pass, and again on
// every window that reuses the graph -- same buffers, possibly new contents)
static int prefix_build_pass(vd_engine* e, const vd_engine::WinKey& k, const vd_engine::WinGraph& g, hipStream_t st) {
    float* tm = e->step_tm();
    map_t(e, e->d_win_t, k.B, tm, st);
    Arena ar = e->step_arena();
    FwdIn fi{k.B, k.T, k.x, k.obs_src, k.obs, k.lat, k.km, tm, reinterpret_cast<const int64_t*>(k.fidx), k.obs_mode, e->step_eps(k.B)};
    PrefixPlan bp; bp.n = g.n_inv; bp.list = g.d_lists + (k.B * k.T - g.n_inv); bp.build_only = true; bp.store = g.store;
    ProfPause pause;
    return e->forward(fi, st, ar, &bp);
}

// A new signature.  Everything a launch needs lazily (kernel attributes, CU count, the workspace) is set up by one eager forward
// into the eps scratch before the capture; x is not touched by it.
static int warmup_forward(vd_engine* e, const vd_engine::WinKey& k, const float* net_obs_src, int net_mode, hipStream_t st) {
    float* tm = e->step_tm();
    map_t(e, e->d_win_t, k.B, tm, st);
    Arena ar = e->step_arena();
    int rc = renoise_observed(e, k, st);
    if (rc) return rc;
    FwdIn fi{k.B, k.T, k.x, net_obs_src, k.obs, k.lat, k.km, tm, reinterpret_cast<const int64_t*>(k.fidx), net_mode, e->step_eps(k.B)};
    FreeUReq fq;
    if (k.fu_on) {                                   // the graph's own passes, once outside the capture
        if ((rc = e->freeu_request(k.B, k.T, k.fu_b, k.fu_s, k.fu_adaptive, &fq))) return rc;
        fi.fu = &fq;
    }
    if ((rc = e->forward(fi, st, ar))) return rc;
    VD_HIP(hipStreamSynchronize(st));
    return 0;
}

// One step of the window as a new graph (prefix cache: after the first pass over the invariant frames), cached as the current window.
// The graph under construction owns its device lists and prefix store: every error return releases them.
static int capture_window(vd_engine* e, const vd_engine::WinKey& k, const std::vector<unsigned char>& inv, int n_inv,
                          const float* net_obs_src, int net_mode, hipStream_t st) {
    const int B = k.B, N = B * k.T;
    const bool pre_on = k.flags & 1, suf_on = k.flags & 2;
    const size_t per = (size_t)k.T * 3 * e->cfg.image_size * e->cfg.image_size;
    ProfPause pause;                                            // no event records inside a capture
    vd_engine::WinGraph wg{};
    struct Owner { vd_engine::WinGraph* g; ~Owner() { if (g) g->release(); } } owner{&wg};
    wg.key = k; wg.inv = inv; wg.n_inv = n_inv;
    PrefixPlan plan;
    SuffixPlan splan;
    if (pre_on || suf_on) {
        std::vector<int> lists;
        for (int n = 0; n < N; ++n) if (!inv[n]) lists.push_back(n);
        for (int n = 0; n < N; ++n) if (inv[n]) lists.push_back(n);
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&wg.d_lists), N * sizeof(int)));
        VD_HIP(hipMemcpy(wg.d_lists, lists.data(), N * sizeof(int), hipMemcpyHostToDevice));
        wg.n_suf = suf_on ? N - n_inv : 0;
        splan.n = N - n_inv; splan.list = wg.d_lists;
    }
    int rc;
    if (pre_on) {
        wg.store = new PrefixStore();
        rc = prefix_build_pass(e, k, wg, st);
        if (!rc && hipStreamSynchronize(st) != hipSuccess) { set_error("prefix cache: first pass"); rc = -2; }
        if (rc) return rc;
        plan.n = N - n_inv; plan.list = wg.d_lists; plan.store = wg.store;
    }
    VD_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    rc = renoise_observed(e, k, st);
    StepReq r{k.sampler, B, k.T, k.x, net_obs_src, k.obs, k.lat, k.km, k.fidx, e->d_win_t, net_mode, k.clip, k.eta};
    r.rng = e->d_win_rng;
    r.sample = k.x;
    if (sampler_is_unipc(k.sampler)) {
        // the three state tensors in place; the count of finished steps picks the order of both moves (0: no corrector, first-order predictor)
        r.ubase = r.ubase_out = e->d_win_ubase;
        r.ud1 = r.ud1_out = e->d_win_hist;
        r.ud2 = r.ud2_out = e->d_win_ud2;
        r.hist_on = e->d_win_rng + 2;
    } else if (sampler_has_history(k.sampler)) {
        // the pass reads the history and writes the step's x_0 prediction over it; the count of finished steps (0 on a window's first
        // step, whatever t_start is) tells it whether the buffer holds one
        r.hist = r.xstart = e->d_win_hist;
        r.hist_on = e->d_win_rng + 2;
    }
    if (pre_on) r.pp = &plan;
    if (suf_on) r.sp = &splan;
    r.cfg_w = k.cfg_w; r.guid_phi = k.guid_phi; r.dyn_p = k.dyn_p;
    if (k.fu_on) { for (int i = 0; i < 2; ++i) { r.fu_b[i] = k.fu_b[i]; r.fu_s[i] = k.fu_s[i]; } r.fu_adaptive = k.fu_adaptive; }
    r.known_src = k.known_src; r.known_mask = k.known_mask;      // the merge draws from the window's own Philox pair (r.rng)
    r.meas_y = k.meas_y; r.meas_scale = k.meas_scale; r.meas_gray = k.meas_gray;
    r.lin_y = k.lin_y; r.lin_Mh = k.lin_Mh; r.lin_Mw = k.lin_Mw;
    if (k.part_K > 1) {                                          // the uniforms come from the window's own Philox pair (r.rng)
        r.part_K = k.part_K; r.part_y = k.part_y; r.part_scale = k.part_scale; r.part_gray = k.part_gray;
        r.part_lambda = k.part_lambda; r.part_tau = k.part_tau; r.part_sigma = k.part_sigma;
        r.part_taps = e->d_blur_taps; r.part_blur_k = k.part_blur_k;
        r.part_lin_Mh = k.part_lin_Mh; r.part_lin_Mw = k.part_lin_Mw;
        if (!r.xstart) r.xstart = e->d_part_x0;
    }
    if (!rc) rc = step_launches(e, r, st);
    if (!rc) {
        // a step with a merge pass consumes its range whatever the sampler: the merge's quarter of it is drawn from
        hipLaunchKernelGGL(win_advance_kernel, dim3((B + 63) / 64), dim3(64), 0, st, e->d_win_t, e->d_win_rng, B,
                           sampler_walks_up(k.sampler) ? 1LL : -1LL, sampler_draws_noise(k.sampler) || k.known_src ? (unsigned long long)B * per : 0ULL);
        if (hipGetLastError() != hipSuccess) { set_error("win_advance_kernel launch"); rc = -2; }
    }
    const hipError_t ce = hipStreamEndCapture(st, &wg.graph);
    if (rc) return rc;
    if (ce != hipSuccess) { set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce)); return -2; }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, wg.graph, nullptr, nullptr, 0) != hipSuccess) { set_error("hipGraphInstantiate"); return -2; }
    wg.exec = exec;
    if (wg.store) {
        // a prefix store holds full-size copies of every tensor before the first attention layer (over 1 GB per block at 128x128,
        // N = 160): sampling modes whose observed-frame pattern changes from window to window (hierarchy, adaptive, mixed) would
        // grow device memory without bound.  At most four graphs keep a store; the oldest one goes first.
        int cnt = 0, oldest = -1;
        for (size_t i = 0; i < e->win_graphs.size(); ++i) if (e->win_graphs[i].store) { ++cnt; if (oldest < 0) oldest = (int)i; }
        if (cnt >= 4) {
            (void)hipDeviceSynchronize();                       // its graph may still be queued on the executor's stream
            e->win_graphs[oldest].release();
            e->win_graphs.erase(e->win_graphs.begin() + oldest);
        }
    }
    e->win_graphs.push_back(wg);
    owner.g = nullptr;
    e->win_cur = (int)e->win_graphs.size() - 1;
    return 0;
}

int vd_window_begin(vd_engine* e, int B, int T, float* x, const float* obs_src, const float* obs, const float* lat,
                    const float* km, const long long* fidx, int obs_mode, int sampler, int clip, float eta,
                    unsigned long long seed, unsigned long long offset, long long t_start, void* stream) {
    // 3 = 'x_t_minus_1' with the caller's tensor read as it is at every step -- what scripts/video_sample.py:149-166 does (it hands x0 as a
    // clean placeholder); 2 = p_sample_loop's form, which re-noises the clean frames to t - 1 before each step (gaussian_diffusion.py:565-568)
    int rc = check_sampler(e, B, T, obs_mode, 3, "observed_frames must be x_0 / x_t / x_t_minus_1 (2: re-noised per step, 3: the caller's tensor as it is)");
    if (rc) return rc;
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx, "null tensor");
    VD_REQUIRE(sampler_valid(sampler), "sampler: 0 p_sample, 1 ddim_sample, 2 ddim_reverse_sample, 3 dpmpp_2m_sample, 4 dpmpp_2m_sde_sample, 5 unipc_sample");
    VD_REQUIRE(sampler_draws_noise(sampler) || obs_mode != 2, "sampler " + std::to_string(sampler) + " (" + sampler_name(sampler) + ") draws no noise: observed_frames = 2 "
               "re-noises the observed frames to t - 1 inside the graph and is not served; hand x_t_minus_1 as it is (observed_frames = 3)");
    if ((rc = require_history_rows(e, sampler, "sampler " + std::to_string(sampler) + " (" + sampler_name(sampler) + ")"))) return rc;
    VD_REQUIRE(t_start >= 0 && t_start < e->num_timesteps, "t_start outside the schedule");
    if ((rc = refuse_cut_step(e->cfg_w, e->dyn_p != 0.f && clip, e->prefix_cache_on, e->suffix_skip_on))) return rc;
    // forward() launches the weight passes wherever the capture's pointers are set: a graph captured now would bake them in, and a graph
    // found would not write them.  return_attn_weights is served by the bare forward alone (armed for one call)
    VD_REQUIRE(e->attn_cap_t.empty() && e->attn_cap_s.empty(), "a window graph together with return_attn_weights (vd_set_attn_capture) is not served: clear the capture (n = 0) first");
    if (e->freeu_on()) {
        VD_REQUIRE(!e->prefix_cache_on, "FreeU (vd_set_freeu) together with the window prefix cache (vd_set_window_prefix_cache) is not served");
        VD_REQUIRE(!e->suffix_skip_on, "FreeU (vd_set_freeu) together with the window suffix skip (vd_set_window_suffix_skip) is not served");
    }
    if (e->part_K > 1) {
        VD_REQUIRE(e->part_y, "particle steering (vd_set_particles) with the caller's rewards inside a window graph is not served: a callback between two steps cannot be captured (the built-in reward can)");
        if ((rc = refuse_with_particles(e, sampler, B, eta))) return rc;
        VD_REQUIRE(!e->prefix_cache_on, "particle steering (vd_set_particles) together with the window prefix cache (vd_set_window_prefix_cache) is not served");
        VD_REQUIRE(!e->suffix_skip_on, "particle steering (vd_set_particles) together with the window suffix skip (vd_set_window_suffix_skip) is not served");
    }
    if (e->known_src) {
        VD_REQUIRE(!sampler_walks_up(sampler), "sampler 2 (ddim_reverse_sample) together with a known region (vd_set_known_region) is not served: the merge noises to t - 1");
        VD_REQUIRE(!e->known_noise, "a window draws the known region's noise from its own Philox stream: known_noise must be NULL (vd_set_known_region)");
        VD_REQUIRE(!e->prefix_cache_on, "a known region (vd_set_known_region) together with the window prefix cache (vd_set_window_prefix_cache) is not served");
        VD_REQUIRE(!e->suffix_skip_on, "a known region (vd_set_known_region) together with the window suffix skip (vd_set_window_suffix_skip) is not served");
    }
    if (e->meas_y) {
        if ((rc = refuse_with_measurement(e, sampler))) return rc;
        VD_REQUIRE(!e->prefix_cache_on, "a measurement (vd_set_measurement) together with the window prefix cache (vd_set_window_prefix_cache) is not served");
        VD_REQUIRE(!e->suffix_skip_on, "a measurement (vd_set_measurement) together with the window suffix skip (vd_set_window_suffix_skip) is not served");
    }
    if (e->lin_y) {
        if ((rc = refuse_with_linear_measurement(e, sampler))) return rc;
        VD_REQUIRE(!e->prefix_cache_on, "a linear measurement (vd_set_linear_measurement) together with the window prefix cache (vd_set_window_prefix_cache) is not served");
        VD_REQUIRE(!e->suffix_skip_on, "a linear measurement (vd_set_linear_measurement) together with the window suffix skip (vd_set_window_suffix_skip) is not served");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    VD_REQUIRE(st != nullptr, "the window executor captures a hipGraph: it needs a non-default stream");
    if ((rc = step_workspace(e, B, T, st))) return rc;
    if ((rc = window_buffers(e, B, obs_mode, sampler, (size_t)T * 3 * e->cfg.image_size * e->cfg.image_size))) return rc;
    if (e->part_K > 1 && ((rc = particle_state_reset(e, B)) || (rc = ensure_particle_ws(e, B, T, !sampler_has_history(sampler))))) return rc;
    hipLaunchKernelGGL(win_set_kernel, dim3((B + 63) / 64), dim3(64), 0, st, e->d_win_t, e->d_win_rng, B, t_start, seed, offset);
    VD_HIP(hipGetLastError());
    vd_engine::WinKey key;
    std::memset(&key, 0, sizeof(key));
    key.B = B; key.T = T; key.obs_mode = obs_mode; key.sampler = sampler; key.clip = clip; key.cfg_w = e->cfg_w;
    key.eta = sampler == SAMPLER_DPMPP_2M_SDE ? 0.f : eta;        // (sampler 4 reads no eta: one graph whatever the caller hands)
    key.guid_phi = e->guid_phi; key.dyn_p = e->dyn_p;
    key.x = x; key.obs_src = obs_src; key.obs = obs; key.lat = lat; key.km = km; key.fidx = fidx;
    key.known_src = e->known_src; key.known_mask = e->known_mask;
    if (e->part_K > 1) {
        key.part_y = e->part_y; key.part_K = e->part_K; key.part_scale = e->part_scale; key.part_gray = e->part_gray;
        key.part_lambda = e->part_lambda; key.part_tau = e->part_tau; key.part_sigma = e->part_sigma;
        key.part_blur_k = e->part_blur ? e->blur_k : 0;
        if (e->part_lin) { key.part_lin_Mh = e->lin_Mh; key.part_lin_Mw = e->lin_Mw; }
    }
    if (e->lin_y) { key.lin_y = e->lin_y; key.lin_Mh = e->lin_Mh; key.lin_Mw = e->lin_Mw; }
    if (e->meas_y) { key.meas_y = e->meas_y; key.meas_scale = e->meas_scale; key.meas_gray = e->meas_gray; }
    if (e->freeu_on()) {
        key.fu_on = 1; key.fu_adaptive = e->fu_adaptive;
        for (int i = 0; i < 2; ++i) { key.fu_b[i] = e->fu_b[i]; key.fu_s[i] = e->fu_s[i]; }
    }
    e->win_cur = -1;
    e->win_lost = false;
    ++e->win_gen;
    e->win_left = sampler_walks_up(sampler) ? e->num_timesteps - t_start : t_start + 1;
    // window prefix cache (opt-in): the frames whose network input cannot change during the window -- observed (obs = 1,
    // lat = 0) in 'x_0' mode with the default 'channel' conditioning (assemble_kernel: v = obs_src, indicator channels,
    // timestep 0) -- run the blocks before the first attention layer ONCE, now; the captured step runs them on the others.
    // Window suffix skip (opt-in): the same frames -- pure observations -- are not read back by the caller and re-enter the
    // network as the observation ('x_0', 'x_t_minus_1'; NOT 'x_t', where an observed frame's input is its own running sample):
    // everything behind the last attention layer runs without them
    const int N = B * T;
    const bool use_pre = e->prefix_cache_on && obs_mode == 0 && e->cfg.cond_emb_type == 0 && e->n_before_attn > 0;
    const bool want_suf = e->suffix_skip_on && obs_mode != 1 && e->cfg.cond_emb_type == 0 && e->suf_blk >= -1 && !e->attn.empty();
    std::vector<unsigned char> inv;
    int n_inv = 0;
    if ((use_pre || want_suf) && (rc = invariant_frames(obs, lat, N, st, &inv, &n_inv))) return rc;
    const bool pre_on = use_pre && n_inv > 0, suf_on = want_suf && n_inv > 0 && n_inv < N;
    key.flags = (pre_on ? 1 : 0) | (suf_on ? 2 : 0);
    const int hit = find_window_graph(e, key, inv);
    if (hit >= 0) {
        e->win_cur = hit;
        return pre_on ? prefix_build_pass(e, key, e->win_graphs[hit], st) : 0;
    }
    const float* net_obs_src = obs_mode == 2 ? e->d_win_xtm1 : obs_src;
    const int net_mode = obs_mode == 3 ? 2 : obs_mode;
    if ((rc = warmup_forward(e, key, net_obs_src, net_mode, st))) return rc;
    return capture_window(e, key, inv, n_inv, net_obs_src, net_mode, st);
}

int vd_set_window_prefix_cache(vd_engine* e, int on) {
    VD_REQUIRE(e, "null engine");
    e->prefix_cache_on = on != 0;
    return 0;
}

// cfg_scale, engine state like the two window switches: 1 = off.  A captured window graph carries the weight in its key (WinKey::cfg_w), so
// nothing is dropped here: the next vd_window_begin finds or captures the graph of the value then set.
int vd_set_cfg_scale(vd_engine* e, float w) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(w == w && std::fabs(w) <= 3.4028234e38f, "cfg_scale must be finite");
    e->cfg_w = w;
    return 0;
}

float vd_cfg_scale(vd_engine* e) { return e ? e->cfg_w : 1.f; }

// FreeU, engine state like cfg_scale: all four constants 1 = off.  A captured window graph carries the constants in its key.  The first
// call that switches it on uploads the cos / sin tables of the two stages' sides (double, host-computed): never inside a capture.
int vd_set_freeu(vd_engine* e, double b1, double b2, double s1, double s2, int adaptive) {
    VD_REQUIRE(e, "null engine");
    const double v[4] = {b1, b2, s1, s2};
    for (double x : v) VD_REQUIRE(x > 0.0 && x <= 1.7976931348623157e308, "freeu: b1, b2, s1 and s2 must be finite and > 0");
    VD_REQUIRE(!e->fu_blk.empty(), "freeu: engine not built");
    const bool on = b1 != 1.0 || b2 != 1.0 || s1 != 1.0 || s2 != 1.0;
    if (on && !e->d_fu_trig) {
        const int S0 = e->fu_blk.front().S, S1 = e->fu_blk.back().S;
        std::vector<double> tab(2 * (size_t)(S0 + S1));
        freeu_trig_table(S0, tab.data());
        freeu_trig_table(S1, tab.data() + 2 * S0);
        VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_fu_trig), tab.size() * sizeof(double)));
        VD_HIP(hipMemcpy(e->d_fu_trig, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    e->fu_b[0] = b1; e->fu_b[1] = b2; e->fu_s[0] = s1; e->fu_s[1] = s2;
    e->fu_adaptive = on && adaptive != 0;
    return 0;
}

int vd_freeu(vd_engine* e, double* consts, int* adaptive) {
    VD_REQUIRE(e, "null engine");
    if (consts) { consts[0] = e->fu_b[0]; consts[1] = e->fu_b[1]; consts[2] = e->fu_s[0]; consts[3] = e->fu_s[1]; }
    if (adaptive) *adaptive = e->fu_adaptive;
    return e->freeu_on() ? 1 : 0;
}

int vd_freeu_stages(vd_engine* e) { return e && e->fu_per_stage ? (int)e->fu_blk.size() / e->fu_per_stage : 0; }

int vd_op_freeu_filter(const float* x, int N, int S, int C, double s, float* y, void* stream) {
    VD_REQUIRE(S >= 2 && S <= 4096, "vd_op_freeu_filter: S >= 2 (at one pixel the four bins coincide and the published box is empty), at most 4096");
    OpScratch ws(stream);
    double* trig = nullptr;
    int rc = ws.get(&trig, 2 * (size_t)S);
    if (rc) return rc;
    std::vector<double> tab(2 * (size_t)S);
    freeu_trig_table(S, tab.data());
    VD_HIP(hipMemcpy(trig, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    return launch_freeu_filter(x, N, S, C, s, trig, y, ws.st);
}

int vd_op_freeu_backbone(const float* h, int N, int S, int C, double b, int adaptive, float* y, void* stream) {
    VD_REQUIRE(N > 0 && S > 0 && S <= 4096, "vd_op_freeu_backbone: shape");
    OpScratch ws(stream);
    double* map = nullptr;
    if (adaptive) { int rc = ws.get(&map, (size_t)N * S * S); if (rc) return rc; }
    return launch_freeu_backbone(h, N, S, C, b, adaptive, map, y, ws.st);
}

int vd_op_cfg_combine(const float* out_c, const float* out_u, float w, long long n, float* out, void* stream) {
    return launch_cfg_combine(out_c, out_u, w, n, out, static_cast<hipStream_t>(stream));
}

// guidance rescale and dynamic thresholding, engine state like cfg_scale: 0 = off; the window graph's key carries both
int vd_set_guidance_rescale(vd_engine* e, float phi) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(phi >= 0.f && phi <= 1.f, "guidance_rescale must lie in [0, 1]");
    e->guid_phi = phi;
    return 0;
}

float vd_guidance_rescale(vd_engine* e) { return e ? e->guid_phi : 0.f; }

int vd_set_dynamic_threshold(vd_engine* e, float p) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(p >= 0.f && p <= 1.f, "dynamic_threshold must lie in (0, 1], or be 0 (off)");
    e->dyn_p = p;
    return 0;
}

float vd_dynamic_threshold(vd_engine* e) { return e ? e->dyn_p : 0.f; }

// The op entries own their scratch for the length of the call (OpScratch; tests -- a step uses the workspace).
int vd_op_cfg_rescale(const float* out_c, const float* out_u, float w, const float* lat, int B, int T, long long frame_elems, float phi,
                      float* out, float* factor_out, void* stream) {
    VD_REQUIRE(B > 0 && frame_elems > 0, "vd_op_cfg_rescale: shape");
    OpScratch ws(stream);
    char* buf = nullptr;
    int rc = ws.get(&buf, guidance_scratch_bytes(B));
    return rc ? rc : launch_cfg_rescale(out_c, out_u, w, lat, B, T, (long)frame_elems, phi, out, factor_out, buf, ws.st);
}

int vd_op_dynamic_threshold(const float* x0, const float* lat, int B, int T, long long frame_elems, float p, float* out, float* s_out,
                            void* stream) {
    VD_REQUIRE(B > 0 && frame_elems > 0, "vd_op_dynamic_threshold: shape");
    OpScratch ws(stream);
    char* buf = nullptr;
    int rc = ws.get(&buf, guidance_scratch_bytes(B));
    if (rc) return rc;
    DynThreshArgs da{x0, nullptr, nullptr, nullptr, 0, lat, B, T, (long)frame_elems, p, out, s_out, nullptr, buf};
    return launch_dynamic_threshold(da, ws.st);
}

int vd_window_prefix_frames(vd_engine* e) {
    VD_REQUIRE(e, "null engine");
    return e->win_cur >= 0 && e->win_graphs[e->win_cur].store ? e->win_graphs[e->win_cur].n_inv : 0;
}

int vd_set_window_suffix_skip(vd_engine* e, int on) {
    VD_REQUIRE(e, "null engine");
    e->suffix_skip_on = on != 0;
    return 0;
}

int vd_window_suffix_frames(vd_engine* e) {
    VD_REQUIRE(e, "null engine");
    return e->win_cur >= 0 ? e->win_graphs[e->win_cur].n_suf : 0;
}

unsigned long long vd_window_generation(vd_engine* e) { return e ? e->win_gen : 0; }

int vd_window_run(vd_engine* e, int n_steps, void* stream) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(!e->win_lost, "window graphs invalidated (workspace growth or a new schedule since vd_window_begin): begin the window again");
    VD_REQUIRE(e->win_cur >= 0, "vd_window_begin first");
    const char* past = sampler_walks_up(e->win_graphs[e->win_cur].key.sampler) ? "more steps than the window has left (ddim_reverse_sample: t would pass num_timesteps - 1)"
                                                                  : "more steps than the window has left (t would pass 0)";
    VD_REQUIRE(n_steps >= 0 && n_steps <= e->win_left, past);
    hipStream_t st = static_cast<hipStream_t>(stream);
    e->drop_held();                                   // a captured step writes the workspace without passing forward()
    for (int i = 0; i < n_steps; ++i) VD_HIP(hipGraphLaunch(e->win_graphs[e->win_cur].exec, st));
    e->win_left -= n_steps;
    return 0;
}

int vd_window_graphs(vd_engine* e) { return e ? (int)e->win_graphs.size() : -1; }

// what the armed window carries from step to step, copied out on `stream` (device to device; each pointer optional): the history of
// samplers 3 and 4 / UniPC's D_{t+1} (`hist`), and UniPC's x^c_{t+1} and D_{t+2}.  Meaningful behind the window's first step.
int vd_window_history(vd_engine* e, int B, int T, float* hist, float* ubase, float* ud2, void* stream) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(!e->win_lost && e->win_cur >= 0, "vd_window_history: no window is armed (vd_window_begin first)");
    const vd_engine::WinKey& k = e->win_graphs[e->win_cur].key;
    VD_REQUIRE(B == k.B && T == k.T, "vd_window_history: B and T are the armed window's");
    VD_REQUIRE(sampler_has_history(k.sampler), std::string("vd_window_history: ") + sampler_name(k.sampler) + " carries no history");
    VD_REQUIRE((!ubase && !ud2) || sampler_is_unipc(k.sampler), std::string("vd_window_history: ") + sampler_name(k.sampler) + " carries one tensor, not UniPC's three");
    const size_t bytes = (size_t)B * T * 3 * e->cfg.image_size * e->cfg.image_size * sizeof(float);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hist) VD_HIP(hipMemcpyAsync(hist, e->d_win_hist, bytes, hipMemcpyDeviceToDevice, st));
    if (ubase) VD_HIP(hipMemcpyAsync(ubase, e->d_win_ubase, bytes, hipMemcpyDeviceToDevice, st));
    if (ud2) VD_HIP(hipMemcpyAsync(ud2, e->d_win_ud2, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- known region (pixel-mask inpainting): engine state like cfg_scale; a window graph's key carries the two addresses
int vd_set_known_region(vd_engine* e, const float* known_src, const float* known_mask, const float* known_noise, unsigned long long seed,
                        unsigned long long offset) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE((known_src == nullptr) == (known_mask == nullptr), "known region: known_src and known_mask are set together, or both NULL (clear)");
    VD_REQUIRE(known_src || !known_noise, "known region: known_noise without a region");
    e->known_src = known_src; e->known_mask = known_mask; e->known_noise = known_noise;
    e->known_seed = seed; e->known_offset = offset;
    return 0;
}

int vd_known_region(vd_engine* e) { return e && e->known_src ? 1 : 0; }

int vd_known_merge(vd_engine* e, int B, int T, long long frame_pixels, float* sample, const float* known_src, const float* known_mask,
                   const float* lat, const long long* t, const float* known_noise, unsigned long long seed, unsigned long long offset,
                   void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    KnownMergeArgs a{sample, known_src, known_mask, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, (long)frame_pixels};
    a.noise = known_noise; a.seed = seed; a.offset = offset;
    return launch_known_merge(a, static_cast<hipStream_t>(stream));
}

// ---- measurement (zero-shot restoration, DDNM): engine state like the known region; a window graph's key carries y, scale and gray
int vd_set_measurement(vd_engine* e, const float* y, int scale, int gray) {
    VD_REQUIRE(e, "null engine");
    if (!y) { e->meas_y = nullptr; e->meas_scale = 1; e->meas_gray = 0; return 0; }
    VD_REQUIRE(measurement_served(scale, gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
    e->meas_y = y; e->meas_scale = scale; e->meas_gray = gray ? 1 : 0;
    return 0;
}

int vd_measurement(vd_engine* e, int* scale, int* gray) {
    if (scale) *scale = e ? e->meas_scale : 1;
    if (gray) *gray = e ? e->meas_gray : 0;
    return e && e->meas_y ? 1 : 0;
}

// the projection alone on an x_0 handed in, in place, on frames of H x W (any size; the engine's image size is not read), no network
int vd_measurement_project(vd_engine* e, int B, int T, int H, int W, float* x0_inout, const float* y, const float* lat, int scale, int gray,
                           void* stream) {
    VD_REQUIRE(e, "null engine");
    MeasureArgs a{nullptr, x0_inout, x0_inout, y, lat, nullptr, nullptr, 0, B, T, H, W, scale, gray ? 1 : 0, 0};
    return launch_measurement_project(a, static_cast<hipStream_t>(stream));
}

// ---- particle steering (particles.hip): engine state like the measurement; the weights and counters live in the engine
int vd_set_particles(vd_engine* e, int K, double lambda, double ess_threshold, const float* y, int scale, int gray, double sigma_y) {
    VD_REQUIRE(e, "null engine");
    if (K <= 1 || lambda == 0.0) {
        e->part_K = 0; e->part_lambda = 0.0; e->part_tau = 0.0;
        e->part_y = nullptr; e->part_scale = 1; e->part_gray = 0; e->part_sigma = 0.0;
        e->part_uni = nullptr; e->part_draws_set = false;
        return 0;
    }
    VD_REQUIRE(K <= kMaxParticles, "particle steering: at most " + std::to_string(kMaxParticles) + " particles per group, got " + std::to_string(K));
    VD_REQUIRE(lambda > 0.0 && lambda <= 1.7976931348623157e308, "particle steering: the reward scale must be finite and not negative");
    VD_REQUIRE(ess_threshold >= 0.0 && ess_threshold <= 1.0, "particle steering: ess_threshold must lie in [0, 1]");
    if (y) {
        VD_REQUIRE(sigma_y > 0.0 && sigma_y <= 1.7976931348623157e308, "particle steering: sigma_y must be positive and finite");
        VD_REQUIRE(measurement_served(scale, gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
        VD_REQUIRE(e->cfg.image_size % scale == 0, "measurement: H and W must be divisible by scale");
    }
    e->part_K = K; e->part_lambda = lambda; e->part_tau = ess_threshold;
    e->part_y = y; e->part_scale = y ? scale : 1; e->part_gray = y && gray ? 1 : 0; e->part_sigma = y ? sigma_y : 0.0;
    return 0;
}

int vd_particles(vd_engine* e) { return e && e->part_K > 1 ? e->part_K : 0; }

// ---- the blur kernel (blur.hip): engine state; the taps live in the engine, at an address that never changes
int vd_set_blur_kernel(vd_engine* e, const float* taps_host, int k) {
    VD_REQUIRE(e, "null engine");
    if (k == 0) {
        VD_REQUIRE(!e->part_blur, "vd_set_blur_kernel: the built-in reward of particle steering reads the kernel (vd_set_particle_blur): switch that off first");
        e->blur_k = 0;
        return 0;
    }
    VD_REQUIRE(blur_served(k), "blur: the kernel is k x k with k odd and 1 <= k <= 15");
    VD_REQUIRE(taps_host, "vd_set_blur_kernel: null taps");
    bool nonzero = false;
    for (int i = 0; i < k * k; ++i) {
        VD_REQUIRE(std::isfinite(taps_host[i]), "blur: the taps must be finite");
        nonzero |= taps_host[i] != 0.f;
    }
    VD_REQUIRE(nonzero, "blur: the taps must not all be zero");
    if (!e->d_blur_taps) VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_blur_taps), kMaxBlurTaps * kMaxBlurTaps * sizeof(float)));
    VD_HIP(hipDeviceSynchronize());                  // a step that reads the taps may still run, on any stream
    VD_HIP(hipMemcpy(e->d_blur_taps, taps_host, (size_t)k * k * sizeof(float), hipMemcpyHostToDevice));
    e->blur_k = k;
    return 0;
}

int vd_blur_kernel(vd_engine* e, int* k) {
    if (k) *k = e ? e->blur_k : 0;
    return e && e->blur_k ? 1 : 0;
}

// The built-in reward of particle steering on the installed blur kernel in place of the cell mean: y (vd_set_particles) then has the
// video's shape, and the scale and gray handed to vd_set_particles are not read.  Runs inside the step's launches and is captured into a
// window graph, whose key carries k.
int vd_set_particle_blur(vd_engine* e, int on) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(!on || e->blur_k, "vd_set_particle_blur: no kernel is installed (vd_set_blur_kernel)");
    VD_REQUIRE(!on || !e->part_lin, "vd_set_particle_blur together with vd_set_particle_linear is not served: the built-in reward has one operator");
    e->part_blur = on ? 1 : 0;
    return 0;
}

int vd_particle_blur(vd_engine* e) { return e && e->part_blur ? 1 : 0; }

// ---- the separable linear operator (linop.hip): engine state; the four matrices live in the engine, at addresses that never change
int vd_set_linear_operator(vd_engine* e, const float* A_h_host, int Mh, const float* A_w_host, int Mw, const float* P_h_host, const float* P_w_host) {
    VD_REQUIRE(e, "null engine");
    if (!A_h_host || !A_w_host) {
        VD_REQUIRE(!e->part_lin, "vd_set_linear_operator: the built-in reward of particle steering reads the operator (vd_set_particle_linear): switch that off first");
        VD_REQUIRE(!e->lin_y, "vd_set_linear_operator: a linear measurement reads the operator (vd_set_linear_measurement): clear that first");
        e->lin_Mh = e->lin_Mw = e->lin_back = 0;
        return 0;
    }
    const int S = e->cfg.image_size;
    VD_REQUIRE(linop_served(S, Mh) && linop_served(S, Mw), "linear operator: A_h is Mh x H and A_w is Mw x W with 1 <= Mh <= H <= 128 and 1 <= Mw <= W <= 128");
    VD_REQUIRE((P_h_host == nullptr) == (P_w_host == nullptr), "linear operator: P_h and P_w come together, or neither");
    VD_REQUIRE((!e->lin_y && !e->part_lin) || (Mh == e->lin_Mh && Mw == e->lin_Mw && (!e->lin_y || P_h_host)),
               "vd_set_linear_operator: a linear measurement or the built-in reward reads the operator: new matrices keep its shape and its back-projection");
    const float* mats[4] = {A_h_host, A_w_host, P_h_host, P_w_host};
    const size_t counts[4] = {(size_t)Mh * S, (size_t)Mw * S, (size_t)S * Mh, (size_t)S * Mw};
    for (int m = 0; m < 4; ++m) {
        if (!mats[m]) continue;
        bool nonzero = false;
        for (size_t i = 0; i < counts[m]; ++i) {
            VD_REQUIRE(std::isfinite(mats[m][i]), "linear operator: the matrices must be finite");
            nonzero |= mats[m][i] != 0.f;
        }
        VD_REQUIRE(nonzero || m >= 2, "linear operator: A_h and A_w must not be all zero");
    }
    const size_t slot = (size_t)kMaxLinopSide * kMaxLinopSide;
    if (!e->d_lin_mats) VD_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_lin_mats), 4 * slot * sizeof(float)));
    VD_HIP(hipDeviceSynchronize());                  // a step that reads the matrices may still run, on any stream
    for (int m = 0; m < 4; ++m)
        if (mats[m]) VD_HIP(hipMemcpy(e->d_lin_mats + m * slot, mats[m], counts[m] * sizeof(float), hipMemcpyHostToDevice));
    e->lin_Mh = Mh; e->lin_Mw = Mw; e->lin_back = P_h_host ? 1 : 0;
    return 0;
}

int vd_linear_operator(vd_engine* e, int* Mh, int* Mw) {
    if (Mh) *Mh = e ? e->lin_Mh : 0;
    if (Mw) *Mw = e ? e->lin_Mw : 0;
    return e && e->lin_Mh ? (e->lin_back ? 2 : 1) : 0;
}

// the projection onto y [B][T][3][Mh][Mw] (device; the caller's) under the installed operator, in every step; a window graph's key
// carries y and the two sides.  NULL: off.
int vd_set_linear_measurement(vd_engine* e, const float* y) {
    VD_REQUIRE(e, "null engine");
    if (!y) { e->lin_y = nullptr; return 0; }
    VD_REQUIRE(e->lin_Mh, "linear measurement: no operator is installed (vd_set_linear_operator)");
    VD_REQUIRE(e->lin_back, "linear measurement: the installed operator has no back-projection (vd_set_linear_operator with P_h and P_w)");
    VD_REQUIRE(!e->meas_y, "a linear measurement (vd_set_linear_measurement) together with a measurement (vd_set_measurement) is not served");
    e->lin_y = y;
    return 0;
}

int vd_linear_measurement(vd_engine* e) { return e && e->lin_y ? 1 : 0; }

// The built-in reward of particle steering on the installed linear operator in place of the cell mean: y (vd_set_particles) is then
// [B][T][3][Mh][Mw], and the scale and gray handed to vd_set_particles are not read.  Runs inside the step's launches and is captured into
// a window graph, whose key carries (Mh, Mw).
int vd_set_particle_linear(vd_engine* e, int on) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(!on || e->lin_Mh, "vd_set_particle_linear: no operator is installed (vd_set_linear_operator)");
    VD_REQUIRE(!on || !e->part_blur, "vd_set_particle_linear together with vd_set_particle_blur is not served: the built-in reward has one operator");
    e->part_lin = on ? 1 : 0;
    return 0;
}

int vd_particle_linear(vd_engine* e) { return e && e->part_lin ? 1 : 0; }

// the projection alone on an x_0 handed in, in place, on frames of H x W under matrices on the device (the engine's are not read), no
// network: the analogue of vd_measurement_project
int vd_op_linear_project(vd_engine* e, int B, int T, int H, int W, float* x0_inout, const float* y, const float* lat, const float* A_h, int Mh,
                         const float* A_w, int Mw, const float* P_h, const float* P_w, int clip, void* stream) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(B > 0 && T > 0 && x0_inout && y && lat && A_h && A_w && P_h && P_w, "arguments");
    VD_REQUIRE(linop_served(H, Mh) && linop_served(W, Mw), "linear operator: A_h is Mh x H and A_w is Mw x W with 1 <= Mh <= H <= 128 and 1 <= Mw <= W <= 128");
    OpScratch sc(stream);
    float* rbuf;
    if (int rc = sc.get(&rbuf, (size_t)B * T * 3 * Mh * Mw)) return rc;
    LinopArgs la{nullptr, x0_inout, y, lat, nullptr, nullptr, 0, B, T, H, W, Mh, Mw, A_h, A_w, clip, rbuf, nullptr, nullptr, nullptr, x0_inout, nullptr, nullptr};
    if (int rc = launch_linop_residual(la, nullptr, static_cast<hipStream_t>(stream))) return rc;
    return launch_linop_project(x0_inout, rbuf, lat, P_h, P_w, B, T, H, W, Mh, Mw, static_cast<hipStream_t>(stream));
}

int vd_particle_reset(vd_engine* e, int B) {
    VD_REQUIRE(e && e->part_K > 1, "vd_particle_reset: no particles are set (vd_set_particles)");
    VD_REQUIRE(B > 0 && B % e->part_K == 0, "particle steering (vd_set_particles): the batch of " + std::to_string(B) + " items is no multiple of the " + std::to_string(e->part_K) + " particles of a group");
    return particle_state_reset(e, B);
}

int vd_particle_draws(vd_engine* e, const double* uniforms, unsigned long long seed, unsigned long long offset) {
    VD_REQUIRE(e, "null engine");
    e->part_uni = uniforms; e->part_seed = seed; e->part_offset = offset; e->part_draws_set = true;
    return 0;
}

int vd_particle_apply(vd_engine* e, int B, long long per, const double* rewards, const long long* t, const double* u, float* const* tensors,
                      int n, void* stream) {
    VD_REQUIRE(e && e->part_K > 1, "vd_particle_apply: no particles are set (vd_set_particles)");
    VD_REQUIRE(B > 0 && B == e->part_B && e->part_state_K == e->part_K, "vd_particle_apply: the state holds " + std::to_string(e->part_B) + " items in groups of " + std::to_string(e->part_state_K) + " (vd_particle_reset), got " + std::to_string(B) + " in groups of " + std::to_string(e->part_K));
    VD_REQUIRE(!e->part_y, "vd_particle_apply: the built-in reward is set (vd_set_particles with y): the step applies it itself");
    VD_REQUIRE(rewards && t && u && per > 0 && n >= 0 && n <= 4 && (n == 0 || tensors), "vd_particle_apply: arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = e->part_K;
    ParticleArgs pa{B / K, K, e->part_lambda, e->part_tau, rewards, nullptr, 0, 0.0, reinterpret_cast<const int64_t*>(t), u,
                    e->d_part_logw, e->d_part_rprev, e->d_part_anc, e->d_part_chosen, e->d_part_ess, e->d_part_counters};
    if (n > 0)
        if (int rc = e->grow(e->d_part_scratch, e->part_scratch_cap, (size_t)n * B * per, true)) return rc;
    if (int rc = launch_particle_weights(pa, st)) return rc;
    if (n == 0) return 0;
    GatherArgs ga{{nullptr, nullptr, nullptr, nullptr}, n, B, per, e->d_part_anc, e->d_part_scratch};
    for (int k = 0; k < n; ++k) ga.x[k] = tensors[k];
    ProfScope ps(PC_ELEMENTWISE, 0.0, 0.0, st, "particle_gather");
    return launch_particle_gather(ga, st);
}

int vd_particle_state(vd_engine* e, int B, double* logw, double* rprev, int* ancestors, int* chosen, double* ess, long long* counters) {
    VD_REQUIRE(e && e->part_state_K > 1 && B > 0 && B == e->part_B, "vd_particle_state: no state of this batch size is held (vd_particle_reset, vd_window_begin)");
    const size_t G = (size_t)B / e->part_state_K;
    VD_HIP(hipDeviceSynchronize());
    if (logw) VD_HIP(hipMemcpy(logw, e->d_part_logw, B * sizeof(double), hipMemcpyDefault));
    if (rprev) VD_HIP(hipMemcpy(rprev, e->d_part_rprev, B * sizeof(double), hipMemcpyDefault));
    if (ancestors) VD_HIP(hipMemcpy(ancestors, e->d_part_anc, B * sizeof(int), hipMemcpyDefault));
    if (chosen) VD_HIP(hipMemcpy(chosen, e->d_part_chosen, G * sizeof(int), hipMemcpyDefault));
    if (ess) VD_HIP(hipMemcpy(ess, e->d_part_ess, G * sizeof(double), hipMemcpyDefault));
    if (counters) VD_HIP(hipMemcpy(counters, e->d_part_counters, 2 * G * sizeof(long long), hipMemcpyDefault));
    return 0;
}

// the two passes alone on a caller's state (tests): no engine state is read or written
int vd_op_particle_weights(int G, int K, double lambda, double ess_threshold, const double* rewards, const double* partials, int nblk,
                           double sigma_y, const long long* t, const double* u, unsigned long long seed, unsigned long long offset, double* logw,
                           double* rprev, int* ancestors, int* chosen, double* ess, long long* counters, void* stream) {
    VD_REQUIRE(rewards || sigma_y > 0.0, "particle steering: sigma_y must be positive");
    ParticleArgs pa{G, K, lambda, ess_threshold, rewards, partials, nblk, rewards ? 0.0 : 1.0 / (2.0 * sigma_y * sigma_y),
                    reinterpret_cast<const int64_t*>(t), u, logw, rprev, ancestors, chosen, ess, counters};
    pa.seed = seed; pa.offset = offset;
    return launch_particle_weights(pa, static_cast<hipStream_t>(stream));
}

int vd_op_particle_gather(int B, long long per, const int* ancestors, float* const* tensors, int n, void* stream) {
    VD_REQUIRE(B > 0 && per > 0 && ancestors && tensors && n >= 1 && n <= 4, "vd_op_particle_gather: arguments");
    OpScratch sc(stream);
    float* scratch;
    if (int rc = sc.get(&scratch, (size_t)n * B * per)) return rc;
    GatherArgs ga{{nullptr, nullptr, nullptr, nullptr}, n, B, per, ancestors, scratch};
    for (int k = 0; k < n; ++k) ga.x[k] = tensors[k];
    return launch_particle_gather(ga, static_cast<hipStream_t>(stream));
}

static const char* const kNoJumpRows = "q_jump: no jump rows for the bound schedule (vd_set_jump_rows, after vd_set_schedule)";

int vd_q_jump(vd_engine* e, int B, int T, long long frame_pixels, const float* x, const float* lat, const long long* t, const float* noise,
              unsigned long long seed, unsigned long long offset, float* out, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(e->d_jump, kNoJumpRows);
    QJumpArgs a{x, out, lat, reinterpret_cast<const int64_t*>(t), e->d_jump, e->num_timesteps, B, T, (long)frame_pixels};
    a.noise = noise; a.seed = seed; a.offset = offset;
    return launch_q_jump(a, static_cast<hipStream_t>(stream));
}

// t += dt; the Philox counter moves on by `draws`; the count of finished steps returns to 0 (a dpmpp_2m or dpmpp_2m_sde window has no history behind a jump)
__global__ void win_jump_kernel(long long* t, unsigned long long* rng, int B, long long dt, unsigned long long draws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) t[b] += dt;
    if (b == 0) { rng[1] += draws; rng[2] = 0; }
}

// n forward jumps of the armed window as plain launches (the resampling walk of RePaint revisits a level a few times per window: not worth a
// graph): t += 1, the jump at the new t from the device's Philox pair, offset += B*per
int vd_window_jump(vd_engine* e, int n, void* stream) {
    VD_REQUIRE(e, "null engine");
    VD_REQUIRE(!e->win_lost, "window graphs invalidated (workspace growth or a new schedule since vd_window_begin): begin the window again");
    VD_REQUIRE(e->win_cur >= 0, "vd_window_begin first");
    const vd_engine::WinKey& k = e->win_graphs[e->win_cur].key;
    VD_REQUIRE(!sampler_walks_up(k.sampler), "vd_window_jump: sampler 2 (ddim_reverse_sample) walks upwards by itself");
    VD_REQUIRE(!sampler_is_unipc(k.sampler), "vd_window_jump: sampler 5 (unipc_sample) is not served: its corrector rebuilds the state from the one before the jump");
    VD_REQUIRE(k.known_src, "vd_window_jump: the armed window has no known region (vd_set_known_region before vd_window_begin)");
    VD_REQUIRE(e->d_jump, kNoJumpRows);
    VD_REQUIRE(n >= 0 && e->win_left + n <= e->num_timesteps, "vd_window_jump: t would pass num_timesteps - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t per = (size_t)k.T * 3 * e->cfg.image_size * e->cfg.image_size;
    for (int i = 0; i < n; ++i) {
        hipLaunchKernelGGL(win_jump_kernel, dim3((k.B + 63) / 64), dim3(64), 0, st, e->d_win_t, e->d_win_rng, k.B, 1LL, 0ULL);
        VD_HIP(hipGetLastError());
        QJumpArgs a{k.x, k.x, k.lat, reinterpret_cast<const int64_t*>(e->d_win_t), e->d_jump, e->num_timesteps, k.B, k.T,
                    (long)e->cfg.image_size * e->cfg.image_size};
        a.dstate = e->d_win_rng;
        int rc = launch_q_jump(a, st);
        if (rc) return rc;
        hipLaunchKernelGGL(win_jump_kernel, dim3((k.B + 63) / 64), dim3(64), 0, st, e->d_win_t, e->d_win_rng, k.B, 0LL, (unsigned long long)k.B * per);
        VD_HIP(hipGetLastError());
        ++e->win_left;
    }
    return 0;
}

int vd_p_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat,
                const float* km, const long long* fidx, const long long* t, int obs_mode, int clip, const float* noise,
                unsigned long long seed, unsigned long long offset, float* sample, float* xstart, float* eps, void* stream) {
    StepReq r{SAMPLER_P, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip};
    r.noise = noise; r.seed = seed; r.offset = offset;
    r.sample = sample; r.xstart = xstart; r.eps_out = eps;
    return run_step(e, r, true, stream);
}

int vd_ddim_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat,
                   const float* km, const long long* fidx, const long long* t, int obs_mode, int clip, float eta,
                   const float* noise, unsigned long long seed, unsigned long long offset, float* sample, float* xstart,
                   float* eps, void* stream) {
    StepReq r{SAMPLER_DDIM, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip, eta};
    r.noise = noise; r.seed = seed; r.offset = offset;
    r.sample = sample; r.xstart = xstart; r.eps_out = eps;
    return run_step(e, r, true, stream);
}

int vd_ddim_reverse_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat,
                           const float* km, const long long* fidx, const long long* t, int obs_mode, int clip, float* sample,
                           float* xstart, float* eps, void* stream) {
    StepReq r{SAMPLER_DDIM_REVERSE, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip};
    r.sample = sample; r.xstart = xstart; r.eps_out = eps;
    return run_step(e, r, true, stream);
}

int vd_dpmpp_2m_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat,
                       const float* km, const long long* fidx, const long long* t, const float* prev_xstart, int obs_mode, int clip,
                       float* sample, float* xstart, float* eps, void* stream) {
    StepReq r{SAMPLER_DPMPP_2M, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip};
    r.hist = prev_xstart;
    r.sample = sample; r.xstart = xstart; r.eps_out = eps;
    return run_step(e, r, true, stream);
}

// ---- the sampler passes alone, on an x_0 prediction (the step through denoised_fn) or on eps: no network
int vd_dpmpp_2m_from_xstart(vd_engine* e, int B, long long per, const float* x, const float* xstart_in, const float* prev_xstart,
                            const long long* t, int clip, float* sample, float* xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && x && xstart_in && t && sample, "arguments");
    SamplerPassArgs a = pass_args(e, SAMPLER_DPMPP_2M, B, per, x, t, clip, sample, xstart);
    a.x0_given = xstart_in; a.hist = prev_xstart;
    return launch_sampler_pass(a, static_cast<hipStream_t>(stream));
}

int vd_dpmpp_2m_sde_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat,
                           const float* km, const long long* fidx, const long long* t, const float* prev_xstart, int obs_mode, int clip,
                           const float* noise, unsigned long long seed, unsigned long long offset, float* sample, float* xstart,
                           float* eps, void* stream) {
    StepReq r{SAMPLER_DPMPP_2M_SDE, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip};
    r.hist = prev_xstart;
    r.noise = noise; r.seed = seed; r.offset = offset;
    r.sample = sample; r.xstart = xstart; r.eps_out = eps;
    return run_step(e, r, true, stream);
}

int vd_dpmpp_2m_sde_from_xstart(vd_engine* e, int B, long long per, const float* x, const float* xstart_in, const float* prev_xstart,
                                const long long* t, int clip, const float* noise, unsigned long long seed, unsigned long long offset,
                                float* sample, float* xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && x && xstart_in && t && sample, "arguments");
    SamplerPassArgs a = pass_args(e, SAMPLER_DPMPP_2M_SDE, B, per, x, t, clip, sample, xstart);
    a.x0_given = xstart_in; a.hist = prev_xstart;
    a.noise = noise; a.seed = seed; a.offset = offset;
    return launch_sampler_pass(a, static_cast<hipStream_t>(stream));
}

int vd_unipc_sample(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
                    const long long* fidx, const long long* t, const float* base, const float* d1, const float* d2, int count, int obs_mode,
                    int clip, float* sample, float* xstart, float* base_out, float* d1_out, float* d2_out, float* eps, void* stream) {
    StepReq r{SAMPLER_UNIPC, B, T, x, obs_src, obs, lat, km, fidx, t, obs_mode, clip};
    r.ubase = base; r.ud1 = d1; r.ud2 = d2; r.count = count;
    r.ubase_out = base_out; r.ud1_out = d1_out; r.ud2_out = d2_out;
    r.sample = sample; r.xstart = xstart; r.eps_out = eps;
    return run_step(e, r, true, stream);
}

int vd_unipc_from_xstart(vd_engine* e, int B, long long per, const float* x, const float* xstart_in, const float* base, const float* d1,
                         const float* d2, int count, const long long* t, int clip, float* sample, float* xstart, float* base_out,
                         float* d1_out, float* d2_out, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && x && xstart_in && t && sample, "arguments");
    SamplerPassArgs a = pass_args(e, SAMPLER_UNIPC, B, per, x, t, clip, sample, xstart);
    a.x0_given = xstart_in;
    a.ubase = base; a.ud1 = d1; a.ud2 = d2; a.count = count;
    a.ubase_out = base_out; a.ud1_out = d1_out; a.ud2_out = d2_out;
    return launch_sampler_pass(a, static_cast<hipStream_t>(stream));
}

int vd_ddim_reverse_from_xstart(vd_engine* e, int B, long long per, const float* x, const float* xstart_in, const long long* t,
                                int clip, float* sample, float* xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && x && xstart_in && t && sample, "arguments");
    SamplerPassArgs a = pass_args(e, SAMPLER_DDIM_REVERSE, B, per, x, t, clip, sample, xstart);
    a.x0_given = xstart_in;
    return launch_sampler_pass(a, static_cast<hipStream_t>(stream));
}

int vd_posterior_update(vd_engine* e, int mode, int B, long long per, const float* x, const float* eps,
                        const long long* t, int clip, float eta, const float* noise, unsigned long long seed,
                        unsigned long long offset, float* sample, float* xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(x && eps && t && sample && sampler_is_posterior(mode), "arguments");
    SamplerPassArgs a = pass_args(e, mode, B, per, x, t, clip, sample, xstart);
    a.eps = eps; a.eta = eta; a.noise = noise; a.seed = seed; a.offset = offset;
    return launch_sampler_pass(a, static_cast<hipStream_t>(stream));
}

int vd_posterior_from_xstart(vd_engine* e, int mode, int B, long long per, const float* x, const float* xstart_in,
                             const long long* t, int clip, float eta, const float* noise, unsigned long long seed,
                             unsigned long long offset, float* sample, float* xstart, float* mean, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(x && xstart_in && t && (sample || xstart || mean) && sampler_is_posterior(mode), "arguments");
    SamplerPassArgs a = pass_args(e, mode, B, per, x, t, clip, sample, xstart);
    a.x0_given = xstart_in; a.mean = mean; a.eta = eta; a.noise = noise; a.seed = seed; a.offset = offset;
    return launch_sampler_pass(a, static_cast<hipStream_t>(stream));
}


// ---- return_attn_weights (unet.py:457-466, 799-836) ---------------------------------------------------------------------
int vd_attn_blocks(vd_engine* e) { return e ? (int)e->attn.size() : -1; }

// resolution (pixels per side) and channels of attention block i, in execution order (input blocks, middle, output blocks)
int vd_attn_block_info(vd_engine* e, int i, int* res, int* channels) {
    VD_REQUIRE(e && i >= 0 && i < (int)e->attn.size() && res && channels, "attention block index");
    int k = 0;
    auto scan = [&](const std::vector<Layer>& blk, int r) { for (const Layer& L : blk) if (L.type == 2 && k++ == i) { *res = r; *channels = e->attn[L.idx].C; return true; } return false; };
    int r = e->cfg.image_size;
    for (auto& blk : e->input_blocks) { if (scan(blk, r)) return 0; for (const Layer& L : blk) if (L.type == 3) r /= 2; }
    if (scan(e->middle, r)) return 0;
    for (auto& blk : e->output_blocks) { if (scan(blk, r)) return 0; for (const Layer& L : blk) if (L.type == 4) r *= 2; }
    set_error("attention block not found"); return -1;
}

// Arm (n > 0) or clear (n = 0) the capture: the next forwards write block i's head-averaged softmax weights to
// temporal[i] ([B*HW][T][T]) and spatial[i] ([B*T][HW][HW]); a NULL entry skips that block.
int vd_set_attn_capture(vd_engine* e, float* const* temporal, float* const* spatial, int n) {
    VD_REQUIRE(e && n >= 0 && n <= (int)e->attn.size() && (n == 0 || (temporal && spatial)), "attention capture");
    e->attn_cap_t.assign(temporal, temporal + n);
    e->attn_cap_s.assign(spatial, spatial + n);
    return 0;
}

// ---- use_gradient_method (gaussian_diffusion.py:264-271,350-364) ------------------------------------------------------
long long vd_bwd_weights_bytes(vd_engine* e) { return e ? (long long)(e->packed_bwd_total * sizeof(float)) : -1; }

int vd_set_bwd_weight_storage(vd_engine* e, void* buf, long long bytes, int on_host) {
    VD_REQUIRE(e && buf, "null argument");
    VD_REQUIRE(split_math(), "use_gradient_method runs on the split arithmetic only (VD_MATH=f16x3 | bf16x6)");
    VD_REQUIRE(bytes >= (long long)(e->packed_bwd_total * sizeof(float)), "backward weight buffer too small");
    e->drop_held();
    e->wbuf_bwd = static_cast<float*>(buf);
    e->wbuf_bwd_on_host = on_host != 0;
    return 0;
}

// the backward-data image of one parameter (no-op for parameters the backward pass does not read)
int vd_load_weight_bwd(vd_engine* e, const char* name, const float* host, long long numel) {
    VD_REQUIRE(e && name && host, "null argument");
    VD_REQUIRE(e->wbuf_bwd, "vd_set_bwd_weight_storage first");
    auto it = e->pidx.find(name);
    if (it == e->pidx.end()) { set_error(std::string("unexpected key in state_dict: ") + name); return -1; }
    const Param& p = e->params[it->second];
    if (p.kind_bwd < 0) return 0;
    VD_REQUIRE((long long)p.numel == numel, "size mismatch");
    std::vector<float> tmp((size_t)p.packed_bwd, 0.f);
    pack_weight_bwd(host, bwd_kind_of(p), (int)p.shape[0], (int)p.shape[1], tmp.data());
    float* dst = e->wbuf_bwd + p.off_bwd;
    if (!e->wbuf_bwd_on_host && e->ws) VD_HIP(hipDeviceSynchronize());      // (as vd_load_weight: a differentiated pass may still read the image)
    if (e->wbuf_bwd_on_host) std::memcpy(dst, tmp.data(), p.packed_bwd * sizeof(float));
    else VD_HIP(hipMemcpy(dst, tmp.data(), p.packed_bwd * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// ---- the differentiated passes: taped forward -> seed -> backward-data pass (vd_guided_step, vd_dps_step, vd_eps_vjp, vd_ode_nll_eval)
// Their shared refusals under the entry's name.  plain_state: also the engine state that would act on a plain step, and the item limit
// (the guided step leaves those switches to its Python caller and has its own limit); eps_note: what the vjp entries add on a START_X model.
static int check_diff(vd_engine* e, int B, int T, const std::string& what, bool plain_state = true, const char* eps_note = "") {
    VD_REQUIRE(!e->freeu_on(), what + " together with FreeU (vd_set_freeu) is not served: the taped forward does not run its passes");
    VD_REQUIRE(T <= kMaxGuidedWindowFrames, what + ": windows of at most " + std::to_string(kMaxGuidedWindowFrames) +
                                            " frames (the temporal attention and GroupNorm backward kernels), got " + std::to_string(T));
    VD_REQUIRE(e->mean_type == 0, what + ": epsilon-prediction models only" + eps_note);
    VD_REQUIRE(e->wbuf_bwd && !e->wbuf_bwd_on_host, what + ": the backward-data weight image is not on the device (vd_set_bwd_weight_storage / vd_load_weight_bwd)");
    VD_REQUIRE(!e->meas_y, what + " together with a measurement (vd_set_measurement) is not served");
    VD_REQUIRE(!e->lin_y, what + " together with a linear measurement (vd_set_linear_measurement) is not served");
    VD_REQUIRE(e->part_K <= 1, what + " together with particle steering (vd_set_particles) is not served");
    if (!plain_state) return 0;
    VD_REQUIRE(e->cfg_w == 1.f, what + " together with cfg_scale != 1 (vd_set_cfg_scale) is not served");
    VD_REQUIRE(e->guid_phi == 0.f, what + " together with guidance_rescale (vd_set_guidance_rescale) is not served");
    VD_REQUIRE(e->dyn_p == 0.f, what + " together with dynamic_threshold (vd_set_dynamic_threshold) is not served");
    VD_REQUIRE(!e->known_src, what + " together with a known region (vd_set_known_region) is not served");
    VD_REQUIRE(e->attn_cap_t.empty() && e->attn_cap_s.empty(), what + " together with return_attn_weights is not served");
    VD_REQUIRE(B <= DiffWs::kRow, what + ": at most 256 items");
    return 0;
}

extern "C++" {
// The opening of every differentiated pass: the workspace, t_model, `pre` (the entry's own launches ahead of the network; it may point the
// forward at DiffWs's masks), the taped forward, then `body` under the tape, with the arena the backward goes on in.  The forward reads
// t_model from DiffWs and, where in.eps is null, writes its eps slot.  `kept`: record into this tape in place of the scope's own.
template <class Pre, class Body>
static int taped_pass(vd_engine* e, const DiffWs& w, FwdIn fi, const long long* t, hipStream_t st, Pre pre, Body body, Tape* kept = nullptr) {
    if (int rc = e->ensure_ws_guided(fi.B, fi.T)) return rc;
    fi.t_model = w.t_model();
    if (!fi.eps) fi.eps = w.eps();
    map_t(e, t, fi.B, w.t_model(), st);
    if (int rc = pre(fi)) return rc;
    Arena ar = w.arena();
    TapeScope ts(e, kept);
    const int rc = e->forward(fi, st, ar);
    return rc ? rc : body(fi, ar);
}
}
static int no_pre(FwdIn&) { return 0; }

__global__ void guided_masks_kernel(const float* obs, const float* lat, int n, float* obs_net, float* lat_net) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { obs_net[i] = 0.f; lat_net[i] = obs[i] + lat[i]; }      // gaussian_diffusion.py:268-271
}

// One guided step.  The network sees every frame as latent (obs_mask := 0, latent_mask := obs + latent); a sample of
// x_{t-1} is drawn with `noise` from the unguided posterior, its squared distance to x_t_minus_1 on the observed frames is
// back-propagated to x, and mean' = mean - 10 * alpha_t * grad / 2.  Outputs (any may be NULL): mean' , pred_xstart, grad,
// and sample = mean' + [t != 0] * sigma_t * noise2 (p_sample's own draw, gaussian_diffusion.py:438-443).
int vd_guided_step(vd_engine* e, int B, int T, const float* x, const float* obs, const float* lat, const float* km,
                   const long long* fidx, const long long* t, int clip, const float* x_t_minus_1, const float* noise,
                   const float* noise2, float* mean, float* xstart, float* grad, float* sample, void* stream) {
    if (int rc = check_ready(e, B, T)) return rc;
    VD_REQUIRE(e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(!e->cfg.learn_sigma, "learn_sigma: the reference's sampler asserts on video tensors (gaussian_diffusion.py:283)");
    if (int rc = check_diff(e, B, T, "use_gradient_method", false)) return rc;
    VD_REQUIRE(x && obs && lat && km && fidx && t && x_t_minus_1 && noise && (sample == nullptr || noise2 != nullptr), "null tensor");
    const int N = B * T;
    VD_REQUIRE(N <= DiffWs::kRow && B <= DiffWs::kRow, "window of at most 256 frames");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t per = (size_t)T * 3 * e->cfg.image_size * e->cfg.image_size;
    const DiffWs w(e, B, T);
    FwdIn in{B, T, x, x, nullptr, nullptr, km, nullptr, reinterpret_cast<const int64_t*>(fidx), 0, nullptr};
    return taped_pass(e, w, in, t, st, [&](FwdIn& fi) {
        fi.obs = w.obs_net(); fi.lat = w.lat_net();
        hipLaunchKernelGGL(guided_masks_kernel, dim3((N + 63) / 64), dim3(64), 0, st, obs, lat, N, w.obs_net(), w.lat_net());
        return 0;
    }, [&](const FwdIn& fi, Arena& ar) {
        GuidedArgs ga{x, fi.eps, noise, x_t_minus_1, obs, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, (long)per, clip,
                      w.deps(), w.dxd(), w.mean0(), xstart ? xstart : w.xstart0()};
        ga.err = e->d_err; ga.gscale = w.gscale();
        int rc = launch_guided_grad(ga, st);
        if (!rc) rc = launch_grad_rescale(w.deps(), w.tot, w.gscale(), st);
        if (!rc) rc = e->backward(fi, w.deps(), w.dx_net(), st, ar);
        if (!rc) rc = launch_guided_final(ga, w.dx_net(), noise2, grad, mean, sample, st);
        return rc;
    });
}

// One step of diffusion posterior sampling (dps.hip) on a measurement y of the "cell mean" operators.  The network sees the window as the
// plain step hands it over -- the caller's masks and obs_mode -- under the tape; the sampler pass writes the plain step's sample' and
// pred_xstart; the residual and seed passes give rho_b and its cotangents, the backward-data pass carries d eps to x_t (on a power-of-two
// multiple, launch_grad_rescale), and the final pass moves the latent frames: sample = fmaf(-zeta, g, sample').  Plain launches on
// `stream`, no host wait.  Workspace: DiffWs.
int vd_dps_step(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
                const long long* fidx, const long long* t, int obs_mode, int clip, int sampler, float eta, const float* noise,
                const float* y, int scale, int gray, float zeta, float* sample, float* xstart, float* grad, float* residual_norm,
                void* stream) {
    if (int rc = check_sampler(e, B, T, obs_mode, 2, kObsModes)) return rc;
    if (int rc = check_diff(e, B, T, "dps")) return rc;
    VD_REQUIRE(sampler == SAMPLER_P || sampler == SAMPLER_DDIM, "dps: p_sample (0) or ddim_sample (1), got sampler " + std::to_string(sampler));
    VD_REQUIRE(sampler == SAMPLER_P || eta >= 0.f, "eta");
    VD_REQUIRE(zeta >= 0.f && zeta <= 3.4028234e38f, "dps: zeta must be finite and not negative");
    VD_REQUIRE(measurement_served(scale, gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
    VD_REQUIRE(e->cfg.image_size % scale == 0, "measurement: H and W must be divisible by scale");
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t && noise && y && sample && xstart, "null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = e->cfg.image_size;
    const size_t per = (size_t)T * 3 * S * S;
    const DiffWs w(e, B, T);
    VD_REQUIRE(w.partials_fit((size_t)B * dps_partials_per_item()), "dps: window too small for its partial sums");
    FwdIn in{B, T, x, obs_src, obs, lat, km, nullptr, reinterpret_cast<const int64_t*>(fidx), obs_mode, nullptr};
    return taped_pass(e, w, in, t, st, no_pre, [&](const FwdIn& fi, Arena& ar) {
        SamplerPassArgs pa = pass_args(e, sampler, B, (long long)per, x, t, clip, sample, xstart);
        pa.eps = fi.eps; pa.eta = eta; pa.noise = noise;
        int rc;
        { ProfScope ps(PC_POSTERIOR, 0.0, 4.0 * B * per * 5.0, st); rc = launch_sampler_pass(pa, st); }
        if (!rc) {
            DpsArgs da{x, fi.eps, y, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, S, S, scale, gray ? 1 : 0, clip,
                       w.r(), w.partials(), w.deps(), w.dxd(), nullptr, residual_norm, e->d_err};
            ProfScope ps(PC_ELEMENTWISE, 4.0 * B * per, 4.0 * B * per * 6.0, st, "dps_seed");
            rc = launch_dps_seed(da, st);
        }
        if (!rc) rc = launch_grad_rescale(w.deps(), w.tot, w.gscale(), st);
        if (!rc) rc = e->backward(fi, w.deps(), w.dx_net(), st, ar);
        if (!rc) {
            ProfScope ps(PC_ELEMENTWISE, 3.0 * B * per, 4.0 * B * per * 5.0, st, "dps_final");
            rc = launch_dps_final(w.dxd(), w.dx_net(), w.gscale(), lat, B, T, (long)(per / T), zeta, sample, grad, st);
        }
        return rc;
    });
}

// The residual and seed passes of vd_dps_step alone, on a caller's (x_t, eps): no network, no workspace of the engine (tests).
int vd_op_dps_seed(vd_engine* e, int B, int T, int H, int W, const float* x, const float* eps, const long long* t, int clip,
                   const float* y, const float* lat, int scale, int gray, float* deps, float* dxd, float* rho, float* xstart,
                   void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && x && eps && t && y && lat && deps && dxd, "arguments");
    VD_REQUIRE(measurement_served(scale, gray), "measurement: scale is 2, 4 or 8, or 1 together with gray (scale 1 without gray is the identity)");
    VD_REQUIRE(H % scale == 0 && W % scale == 0, "measurement: H and W must be divisible by scale");
    OpScratch sc(stream);
    float* rbuf; double* part;
    int rc = sc.get(&rbuf, (size_t)B * T * (gray ? 1 : 3) * (H / scale) * (W / scale));
    if (!rc) rc = sc.get(&part, (size_t)B * dps_partials_per_item());
    if (rc) return rc;
    DpsArgs da{x, eps, y, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, H, W, scale, gray ? 1 : 0, clip,
               rbuf, part, deps, dxd, xstart, rho, e->d_err};
    return launch_dps_seed(da, static_cast<hipStream_t>(stream));
}

// vd_dps_step on the installed blur kernel (vd_set_blur_kernel): y has the video's shape, the residual and seed passes are blur.hip's, and
// everything else -- the taped forward, the sampler pass, the backward-data pass, the final pass and the outputs -- is that entry's.
int vd_deblur_step(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
                   const long long* fidx, const long long* t, int obs_mode, int clip, int sampler, float eta, const float* noise,
                   const float* y, float zeta, float* sample, float* xstart, float* grad, float* residual_norm, void* stream) {
    if (int rc = check_sampler(e, B, T, obs_mode, 2, kObsModes)) return rc;
    if (int rc = check_diff(e, B, T, "deblur")) return rc;
    VD_REQUIRE(sampler == SAMPLER_P || sampler == SAMPLER_DDIM, "deblur: p_sample (0) or ddim_sample (1), got sampler " + std::to_string(sampler));
    VD_REQUIRE(sampler == SAMPLER_P || eta >= 0.f, "eta");
    VD_REQUIRE(zeta >= 0.f && zeta <= 3.4028234e38f, "deblur: zeta must be finite and not negative");
    VD_REQUIRE(e->blur_k, "deblur: no kernel is installed (vd_set_blur_kernel)");
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t && noise && y && sample && xstart, "null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = e->cfg.image_size, k = e->blur_k;
    const size_t per = (size_t)T * 3 * S * S;
    const DiffWs w(e, B, T);
    VD_REQUIRE(w.partials_fit((size_t)B * dps_partials_per_item()), "deblur: window too small for its partial sums");
    FwdIn in{B, T, x, obs_src, obs, lat, km, nullptr, reinterpret_cast<const int64_t*>(fidx), obs_mode, nullptr};
    return taped_pass(e, w, in, t, st, no_pre, [&](const FwdIn& fi, Arena& ar) {
        SamplerPassArgs pa = pass_args(e, sampler, B, (long long)per, x, t, clip, sample, xstart);
        pa.eps = fi.eps; pa.eta = eta; pa.noise = noise;
        int rc;
        { ProfScope ps(PC_POSTERIOR, 0.0, 4.0 * B * per * 5.0, st); rc = launch_sampler_pass(pa, st); }
        if (!rc) {
            BlurArgs ba{x, fi.eps, y, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, S, S, e->d_blur_taps, k, clip,
                        w.r(), w.partials(), w.deps(), w.dxd(), nullptr, residual_norm, e->d_err};
            ProfScope ps(PC_ELEMENTWISE, 4.0 * k * k * B * per, 4.0 * B * per * 9.0, st, "deblur_seed");
            rc = launch_blur_seed(ba, st);
        }
        if (!rc) rc = launch_grad_rescale(w.deps(), w.tot, w.gscale(), st);
        if (!rc) rc = e->backward(fi, w.deps(), w.dx_net(), st, ar);
        if (!rc) {
            ProfScope ps(PC_ELEMENTWISE, 3.0 * B * per, 4.0 * B * per * 5.0, st, "dps_final");
            rc = launch_dps_final(w.dxd(), w.dx_net(), w.gscale(), lat, B, T, (long)(per / T), zeta, sample, grad, st);
        }
        return rc;
    });
}

// The residual and seed passes of vd_deblur_step alone, on a caller's (x_t, eps) and taps on the device: no network, no workspace of the
// engine (tests).
int vd_op_deblur_seed(vd_engine* e, int B, int T, int H, int W, const float* x, const float* eps, const long long* t, int clip,
                      const float* y, const float* lat, const float* taps_dev, int k, float* deps, float* dxd, float* rho, float* xstart,
                      void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && x && eps && t && y && lat && taps_dev && deps && dxd, "arguments");
    VD_REQUIRE(blur_served(k), "blur: the kernel is k x k with k odd and 1 <= k <= 15");
    OpScratch sc(stream);
    float* rbuf; double* part;
    int rc = sc.get(&rbuf, (size_t)B * T * 3 * H * W);
    if (!rc) rc = sc.get(&part, (size_t)B * dps_partials_per_item());
    if (rc) return rc;
    BlurArgs ba{x, eps, y, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, H, W, taps_dev, k, clip,
                rbuf, part, deps, dxd, xstart, rho, e->d_err};
    return launch_blur_seed(ba, static_cast<hipStream_t>(stream));
}

// out = A x (adjoint == 0) or A^T x of a [B][T][3][H][W] tensor for taps on the device; out != x.  No engine.
int vd_op_blur(int B, int T, int H, int W, const float* x, const float* taps_dev, int k, int adjoint, float* out, void* stream) {
    VD_REQUIRE(B > 0 && T > 0, "blur: shape");
    return launch_blur_apply(x, taps_dev, k, adjoint, (size_t)B * T * 3, H, W, out, static_cast<hipStream_t>(stream));
}

// vd_deblur_step on the installed linear operator (vd_set_linear_operator): y is [B][T][3][Mh][Mw], the residual and seed passes are
// linop.hip's, and everything else is that entry's.
int vd_linear_dps_step(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
                       const long long* fidx, const long long* t, int obs_mode, int clip, int sampler, float eta, const float* noise,
                       const float* y, float zeta, float* sample, float* xstart, float* grad, float* residual_norm, void* stream) {
    if (int rc = check_sampler(e, B, T, obs_mode, 2, kObsModes)) return rc;
    if (int rc = check_diff(e, B, T, "linear_dps")) return rc;
    VD_REQUIRE(sampler == SAMPLER_P || sampler == SAMPLER_DDIM, "linear_dps: p_sample (0) or ddim_sample (1), got sampler " + std::to_string(sampler));
    VD_REQUIRE(sampler == SAMPLER_P || eta >= 0.f, "eta");
    VD_REQUIRE(zeta >= 0.f && zeta <= 3.4028234e38f, "linear_dps: zeta must be finite and not negative");
    VD_REQUIRE(e->lin_Mh, "linear_dps: no operator is installed (vd_set_linear_operator)");
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t && noise && y && sample && xstart, "null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = e->cfg.image_size, Mh = e->lin_Mh, Mw = e->lin_Mw;
    const size_t per = (size_t)T * 3 * S * S;
    const DiffWs w(e, B, T);
    VD_REQUIRE(w.partials_fit((size_t)B * dps_partials_per_item()), "linear_dps: window too small for its partial sums");
    FwdIn in{B, T, x, obs_src, obs, lat, km, nullptr, reinterpret_cast<const int64_t*>(fidx), obs_mode, nullptr};
    return taped_pass(e, w, in, t, st, no_pre, [&](const FwdIn& fi, Arena& ar) {
        SamplerPassArgs pa = pass_args(e, sampler, B, (long long)per, x, t, clip, sample, xstart);
        pa.eps = fi.eps; pa.eta = eta; pa.noise = noise;
        int rc;
        { ProfScope ps(PC_POSTERIOR, 0.0, 4.0 * B * per * 5.0, st); rc = launch_sampler_pass(pa, st); }
        if (!rc) {
            LinopArgs la{x, fi.eps, y, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, S, S, Mh, Mw, e->lin_mat(0), e->lin_mat(1),
                         clip, w.r(), w.partials(), w.deps(), w.dxd(), nullptr, residual_norm, e->d_err};
            ProfScope ps(PC_ELEMENTWISE, 4.0 * (Mh + Mw) * B * per, 4.0 * B * per * 9.0, st, "linear_dps_seed");
            rc = launch_linop_seed(la, st);
        }
        if (!rc) rc = launch_grad_rescale(w.deps(), w.tot, w.gscale(), st);
        if (!rc) rc = e->backward(fi, w.deps(), w.dx_net(), st, ar);
        if (!rc) {
            ProfScope ps(PC_ELEMENTWISE, 3.0 * B * per, 4.0 * B * per * 5.0, st, "dps_final");
            rc = launch_dps_final(w.dxd(), w.dx_net(), w.gscale(), lat, B, T, (long)(per / T), zeta, sample, grad, st);
        }
        return rc;
    });
}

// The residual and seed passes of vd_linear_dps_step alone, on a caller's (x_t, eps) and matrices on the device: no network, no workspace
// of the engine (tests).
int vd_op_linear_dps_seed(vd_engine* e, int B, int T, int H, int W, const float* x, const float* eps, const long long* t, int clip,
                          const float* y, const float* lat, const float* A_h, int Mh, const float* A_w, int Mw, float* deps, float* dxd,
                          float* rho, float* xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && x && eps && t && y && lat && A_h && A_w && deps && dxd, "arguments");
    VD_REQUIRE(linop_served(H, Mh) && linop_served(W, Mw), "linear operator: A_h is Mh x H and A_w is Mw x W with 1 <= Mh <= H <= 128 and 1 <= Mw <= W <= 128");
    OpScratch sc(stream);
    float* rbuf; double* part;
    int rc = sc.get(&rbuf, (size_t)B * T * 3 * Mh * Mw);
    if (!rc) rc = sc.get(&part, (size_t)B * dps_partials_per_item());
    if (rc) return rc;
    LinopArgs la{x, eps, y, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, H, W, Mh, Mw, A_h, A_w, clip,
                 rbuf, part, deps, dxd, xstart, rho, e->d_err};
    return launch_linop_seed(la, static_cast<hipStream_t>(stream));
}

// out = L x R^T of `planes` planes of Q x U for matrices on the device (L: P x Q, R: S x U; out planes of P x S); out != x.  No engine.
int vd_op_linop(long long planes, int Q, int U, const float* x, const float* L, int P, const float* R, int S, float* out, void* stream) {
    VD_REQUIRE(planes > 0, "linop: shape");
    return launch_linop_apply(x, L, P, Q, R, S, U, (size_t)planes, out, static_cast<hipStream_t>(stream));
}

// ---- loss guidance: vd_dps_step split where the cotangent is formed, the caller's own code running between the two halves
// The first half: vd_dps_step's checks under the name "loss_guidance", the opening of taped_pass and the sampler pass -- the plain step's
// sample and pred_xstart.  The tape is then kept: it is recorded into the engine's held pass, beside what the second half reads, and
// *ticket names it.  A pass held before is dropped (ensure_ws_guided -> grow_ws).
int vd_guide_begin(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
                   const long long* fidx, const long long* t, int obs_mode, int clip, int sampler, float eta, const float* noise,
                   float* sample, float* xstart, unsigned long long* ticket, void* stream) {
    if (int rc = check_sampler(e, B, T, obs_mode, 2, kObsModes)) return rc;
    if (int rc = check_diff(e, B, T, "loss_guidance")) return rc;
    VD_REQUIRE(sampler == SAMPLER_P || sampler == SAMPLER_DDIM, "loss_guidance: p_sample (0) or ddim_sample (1), got sampler " + std::to_string(sampler));
    VD_REQUIRE(sampler == SAMPLER_P || eta >= 0.f, "eta");
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t && noise && sample && xstart && ticket, "null tensor");
    *ticket = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t per = (size_t)T * 3 * e->cfg.image_size * e->cfg.image_size;
    const DiffWs w(e, B, T);
    VD_REQUIRE(w.partials_fit((size_t)B * guide_norm_blocks((long)per)), "loss_guidance: window too small for its partial sums");
    auto hp = std::make_unique<vd_engine::HeldPass>();
    hp->B = B; hp->T = T; hp->clip = clip; hp->t = t;
    FwdIn in{B, T, x, obs_src, obs, lat, km, nullptr, reinterpret_cast<const int64_t*>(fidx), obs_mode, nullptr};
    const int rc = taped_pass(e, w, in, t, st, no_pre, [&](const FwdIn& fi, Arena& ar) {
        SamplerPassArgs pa = pass_args(e, sampler, B, (long long)per, x, t, clip, sample, xstart);
        pa.eps = fi.eps; pa.eta = eta; pa.noise = noise;
        hp->fi = fi; hp->ar = ar;
        ProfScope ps(PC_POSTERIOR, 0.0, 4.0 * B * per * 5.0, st);
        return launch_sampler_pass(pa, st);
    }, &hp->tape);
    if (rc) return rc;
    hp->ticket = *ticket = ++e->guide_seq;
    e->held = std::move(hp);
    return 0;
}

// The second half on the held pass `ticket` names: the seed pass on the caller's cotangent of x_0, launch_grad_rescale, the backward-data
// pass under the kept tape, the norm pass (normalize) and the final pass on `sample` in place.  A ticket that is not the live one fails
// before anything is launched; the held pass is released whatever happens behind that.
int vd_guide_finish(vd_engine* e, unsigned long long ticket, const float* cot, const float* scale, int normalize, float* sample, float* grad,
                    float* grad_norm, void* stream) {
    VD_REQUIRE(e, "null engine");
    if (!e->held || e->held->ticket != ticket) {
        const std::string why = ticket == 0 || ticket > e->guide_seq ? "it was never begun"
                                : ticket == e->guide_end_ticket      ? std::string(e->guide_end_why)
                                                                     : "already finished, or dropped by an engine call in between";
        set_error("loss_guidance: no taped pass is held for this ticket (" + why + ")");
        return -1;
    }
    std::unique_ptr<vd_engine::HeldPass> hp = std::move(e->held);
    e->guide_end_ticket = ticket; e->guide_end_why = "already finished";
    VD_REQUIRE(cot && scale && sample, "loss_guidance: null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = hp->B, T = hp->T, S = e->cfg.image_size;
    const long fe = 3L * S * S;
    const size_t per = (size_t)T * fe;
    const DiffWs w(e, B, T);
    int rc;
    {
        GuideSeedArgs ga{hp->fi.x, hp->fi.eps, cot, hp->fi.lat, reinterpret_cast<const int64_t*>(hp->t), e->d_tab, e->num_timesteps, B, T, S, S,
                         hp->clip, w.deps(), w.dxd(), e->d_err};
        ProfScope ps(PC_ELEMENTWISE, 2.0 * B * per, 4.0 * B * per * 5.0, st, "guide_seed");
        rc = launch_guide_seed(ga, st);
    }
    if (!rc) rc = launch_grad_rescale(w.deps(), w.tot, w.gscale(), st);
    if (!rc) {
        TapeScope ts(e, &hp->tape);
        rc = e->backward(hp->fi, w.deps(), w.dx_net(), st, hp->ar);
    }
    if (!rc && normalize) {
        ProfScope ps(PC_ELEMENTWISE, 3.0 * B * per, 4.0 * B * per * 2.0, st, "guide_norm");
        rc = launch_guide_norm(w.dxd(), w.dx_net(), w.gscale(), hp->fi.lat, B, T, fe, w.partials(), st);
    }
    if (!rc) {
        ProfScope ps(PC_ELEMENTWISE, 3.0 * B * per, 4.0 * B * per * 5.0, st, "guide_final");
        rc = launch_guide_final(w.dxd(), w.dx_net(), w.gscale(), hp->fi.lat, B, T, fe, scale, normalize ? w.partials() : nullptr, sample, grad,
                                normalize ? grad_norm : nullptr, st);
    }
    return rc;
}

int vd_guide_abort(vd_engine* e) {
    VD_REQUIRE(e, "null engine");
    e->end_held("aborted (vd_guide_abort)");
    return 0;
}

// The seed pass of vd_guide_finish alone, on a caller's (x_t, eps, cot): no network, no workspace of the engine (tests).
int vd_op_guide_seed(vd_engine* e, int B, int T, int H, int W, const float* x, const float* eps, const long long* t, int clip,
                     const float* cot, const float* lat, float* deps, float* dxd, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && x && eps && t && cot && lat && deps && dxd, "arguments");
    GuideSeedArgs ga{x, eps, cot, lat, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, H, W, clip, deps, dxd, e->d_err};
    return launch_guide_seed(ga, static_cast<hipStream_t>(stream));
}

// The opening checks of the two entries that hand out the vector-Jacobian product of the network (vd_eps_vjp, vd_ode_nll_eval): what
// vd_dps_step checks (check_diff) under the entry's name (`what`: "eps_vjp" | "ode_nll"), and two of their own.
static int check_vjp(vd_engine* e, int B, int T, int obs_mode, const std::string& what) {
    if (int rc = check_ready(e, B, T)) return rc;
    VD_REQUIRE(e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(!e->cfg.learn_sigma, what + ": learn_sigma is not served (the backward pass carries the 3-channel head only)");
    VD_REQUIRE(obs_mode == 0, what + ": observed_frames must be x_0 (the observed frames are conditioning: a constant of the derivative)");
    return check_diff(e, B, T, what, true, " (predict_xstart is not served)");
}

// The vector-Jacobian product of the network as a primitive: one taped forward, one backward-data pass with d eps = cot (a copy of it
// times a power of two, launch_grad_rescale, and 1 / s on the way out).  Workspace: DiffWs; plain launches on `stream`, no host wait.
// The observed frames come from obs_src (x_0 mode) and are constants: vjp is exactly 0 there.
int vd_eps_vjp(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
               const long long* fidx, const long long* t, int obs_mode, const float* cot, float* eps_out, float* vjp_out, void* stream) {
    if (int rc = check_vjp(e, B, T, obs_mode, "eps_vjp")) return rc;
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t && cot && vjp_out, "null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DiffWs w(e, B, T);
    FwdIn in{B, T, x, obs_src, obs, lat, km, nullptr, reinterpret_cast<const int64_t*>(fidx), obs_mode, eps_out};
    return taped_pass(e, w, in, t, st, [&](FwdIn&) -> int {
        VD_HIP(hipMemcpyAsync(w.deps(), cot, w.tot * sizeof(float), hipMemcpyDeviceToDevice, st));     // the forward does not touch the tail
        return 0;
    }, [&](const FwdIn& fi, Arena& ar) {
        int rc = launch_grad_rescale(w.deps(), w.tot, w.gscale(), st);
        if (!rc) rc = e->backward(fi, w.deps(), w.dx_net(), st, ar);
        if (!rc) {
            ProfScope ps(PC_ELEMENTWISE, 1.0 * w.tot, 4.0 * w.tot * 2.0, st, "eps_vjp_scale");
            rc = launch_scale_by(w.dx_net(), w.gscale(), w.tot, vjp_out, st);
        }
        return rc;
    });
}

// One point of the probability-flow ODE likelihood (ode_nll.hip): eps = eps_theta(x, t) under the tape, then per probe k the seed --
// rademacher_kernel at (seed, item_offset[b], probe0 + k), or the caller's probe[k] read in place -- the backward-data pass and
// masked_dot: trace[b] = (1 / K) sum_k v_k^T (d eps / d x)^T v_k over the item's latent frames, in fp64.  The tape is kept across the K
// probes: a backward pass reads the taped tensors and writes only what it takes from the arena above the mark, which is released behind
// it.  x_next (or null): the Euler move to t + 1, deterministic_kernel<SAMPLER_DDIM_REVERSE> on (x, eps) with its clamp off; the frames
// that are not latent then get the bits of x back (keep_frames_kernel).  Workspace: DiffWs; plain launches, no host wait.
int vd_ode_nll_eval(vd_engine* e, int B, int T, const float* x, const float* obs_src, const float* obs, const float* lat, const float* km,
                    const long long* fidx, const long long* t, int obs_mode, int n_probes, unsigned long long seed,
                    const unsigned long long* item_offset, unsigned long long probe0, const float* probe, float* eps_out, double* trace_out,
                    float* x_next, void* stream) {
    if (int rc = check_vjp(e, B, T, obs_mode, "ode_nll")) return rc;
    VD_REQUIRE(n_probes >= 1 && n_probes <= 64, "ode_nll: n_probes must be 1..64, got " + std::to_string(n_probes));
    VD_REQUIRE(x && obs_src && obs && lat && km && fidx && t && trace_out && (probe || item_offset), "null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long fe = 3L * e->cfg.image_size * e->cfg.image_size;
    const size_t per = (size_t)T * fe;
    const DiffWs w(e, B, T);
    VD_REQUIRE(w.partials_fit((size_t)B * masked_dot_blocks((long)per)), "ode_nll: window too small for its partial sums");
    FwdIn in{B, T, x, obs_src, obs, lat, km, nullptr, reinterpret_cast<const int64_t*>(fidx), obs_mode, eps_out};
    return taped_pass(e, w, in, t, st, no_pre, [&](const FwdIn& fi, Arena& ar) {
        int rc = 0;
        if (x_next) {
            SamplerPassArgs pa = pass_args(e, SAMPLER_DDIM_REVERSE, B, (long long)per, x, t, 0, x_next, nullptr);
            pa.eps = fi.eps;
            ProfScope ps(PC_POSTERIOR, 0.0, 4.0 * B * per * 3.0, st);
            rc = launch_sampler_pass(pa, st);
            if (!rc) rc = launch_keep_frames(x, lat, B, T, fe, x_next, st);
        }
        for (int k = 0; k < n_probes && !rc; ++k) {
            const float* v = probe ? probe + (size_t)k * w.tot : w.probe();
            if (!probe) {
                ProfScope ps(PC_ELEMENTWISE, 0.0, 4.0 * B * per, st, "rademacher");
                rc = launch_rademacher(w.probe(), lat, B, T, fe, seed, item_offset, probe0 + (unsigned long long)k, st);
            }
            const size_t mk = ar.mark();
            if (!rc) rc = e->backward(fi, v, w.dx_net(), st, ar);
            ar.release(mk);
            if (!rc) {
                ProfScope ps(PC_ELEMENTWISE, 2.0 * B * per, 4.0 * B * per * 2.0, st, "masked_dot");
                rc = launch_masked_dot(v, w.dx_net(), lat, B, T, fe, w.partials(), k > 0, k == n_probes - 1 ? (double)n_probes : 1.0, trace_out, st);
            }
        }
        return rc;
    });
}

// The passes of ode_nll.hip alone on caller's tensors of any frame size: no network, scratch from OpScratch (tests, and the loop's
// corrector and prior term).
int vd_rademacher(float* out, const float* lat, int B, int T, long long frame_elems, unsigned long long seed,
                  const unsigned long long* item_offset, unsigned long long probe, void* stream) {
    return launch_rademacher(out, lat, B, T, (long)frame_elems, seed, item_offset, probe, static_cast<hipStream_t>(stream));
}

int vd_dequantize(const float* x, const float* lat, int B, int T, long long frame_elems, unsigned long long seed,
                  const unsigned long long* item_offset, float* out, void* stream) {
    return launch_dequantize(x, lat, B, T, (long)frame_elems, seed, item_offset, out, static_cast<hipStream_t>(stream));
}

int vd_op_masked_dot(const float* a, const float* b, const float* lat, int B, int T, long long frame_elems, double* out, void* stream) {
    VD_REQUIRE(a && b && lat && out && B > 0 && T > 0 && frame_elems > 0, "masked_dot: arguments");
    VD_REQUIRE((double)T * (double)frame_elems < 2147483648.0, "masked_dot: an item of fewer than 2^31 elements");
    OpScratch sc(stream);
    double* part;
    int rc = sc.get(&part, (size_t)B * masked_dot_blocks((long)T * (long)frame_elems));
    if (rc) return rc;
    return launch_masked_dot(a, b, lat, B, T, (long)frame_elems, part, 0, 1.0, out, static_cast<hipStream_t>(stream));
}

int vd_op_ode_heun(vd_engine* e, int B, int T, long long frame_elems, const float* x, const float* eps, const float* eps2, const long long* t,
                   const float* lat, float* out, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    return launch_ode_heun(x, eps, eps2, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, lat, B, T, (long)frame_elems, out,
                           e->d_err, static_cast<hipStream_t>(stream));
}

int vd_q_sample(vd_engine* e, int B, long long per, const float* x0, const long long* t, const float* noise, float* out,
                void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(x0 && t && noise && out, "null tensor");
    return launch_q_sample(x0, noise, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, (long)per, out,
                           static_cast<hipStream_t>(stream));
}

int vd_randn(float* out, long long n, unsigned long long seed, unsigned long long offset, void* stream) {
    VD_REQUIRE(out && n >= 0, "arguments");
    return launch_randn(out, (long)n, seed, offset, static_cast<hipStream_t>(stream));
}

long long vd_split_image_u16(long long n_out, long long k_total) { return (long long)split_image_u16((size_t)n_out, (size_t)k_total); }
int vd_math_mode(void) { return math_mode(); }

int vd_pack_conv3_wino_split(const float* host_oihw, unsigned short* host_out, int O, int I) {
    VD_REQUIRE(host_oihw && host_out && O % 64 == 0 && I % 32 == 0, "vd_pack_conv3_wino_split: O multiple of 64, I of 32");
    pack_conv3_wino_split(host_oihw, host_out, O, I);
    return 0;
}

int vd_op_conv_wino_split(const float* src0, int Cin, int nfr, int Hs, int Ws, int ups, const void* w_split, const float* bias,
                          const float* res, const float* fbias, int fbias_ld, float* out, int Cout, double* gn_part,
                          void* stream) {
    IgemmArgs g = conv_args(src0, nullptr, Cin, Cin, nfr, Hs, Ws, ups, 1, 1, 3);
    g.wwino = static_cast<const float*>(w_split); g.wsplit = 2; g.bias = bias; g.res = res; g.res_ld = Cout;
    g.fbias = fbias; g.fbias_ld = fbias_ld; g.out = out; g.ldo = Cout; g.Cout = Cout;
    g.stats = gn_part; g.stats_split = conv_wino_stats_split(g.Ho);
    VD_REQUIRE(conv_wino_r64_supported(g), "vd_op_conv_wino_split: shape not covered by conv_wino_r64.hip");
    return launch_igemm(g, static_cast<hipStream_t>(stream));            // cuts big windows along frames like the engine
}

int vd_op_conv_wino_act(const float* src0, const float* src1, int C0, int Cin, int nfr, int Hs, int Ws, const void* w_split, const float* bias,
                        const float* affA, const float* affB, const float* res, float* out, int Cout, double* gn_part, void* stream) {
    VD_REQUIRE(src0 && (src1 ? C0 > 0 && C0 < Cin : C0 == Cin), "vd_op_conv_wino_act: one source of Cin channels, or two of C0 and Cin - C0");
    IgemmArgs g = conv_args(src0, src1, C0, Cin, nfr, Hs, Ws, 0, 1, 1, 3);
    g.wwino = static_cast<const float*>(w_split); g.wsplit = 2; g.bias = bias; g.res = res; g.res_ld = Cout;
    g.affA = affA; g.affB = affB; g.act = 1;
    g.out = out; g.ldo = Cout; g.Cout = Cout;
    g.stats = gn_part; g.stats_split = conv_wino_stats_split(g.Ho);
    VD_REQUIRE(conv_wino_z128_act_supported(g), "vd_op_conv_wino_act: shape not covered by conv_wino_z128.hip's activating form (vd_conv_wino_act_ok)");
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_conv_wino_act_ok(int nfr, int H, int Cin, int Cout) { return f16_math() && conv_wino_z128_act_shape(nfr, H, Cin, Cout) ? 1 : 0; }

int vd_pack_conv3_wino_ups(const float* host_oihw, unsigned short* host_out, int O, int I) {
    VD_REQUIRE(host_oihw && host_out && O % 64 == 0 && I % 32 == 0, "vd_pack_conv3_wino_ups: O multiple of 64, I of 32");
    pack_conv3_wino_ups(host_oihw, host_out, O, I);
    return 0;
}

int vd_conv_ups_stats_split(int Hs) { return conv_wino_ups_stats_split(Hs); }

int vd_op_conv_wino_ups(const float* src0, int Cin, int nfr, int Hs, const void* w_ups, const float* bias, float* out, int Cout,
                        double* gn_part, void* stream) {
    IgemmArgs g = conv_args(src0, nullptr, Cin, Cin, nfr, Hs, Hs, 1, 1, 1, 3);
    g.ups_phase = 1;
    g.wwino = static_cast<const float*>(w_ups); g.wsplit = 2; g.bias = bias; g.out = out; g.ldo = Cout; g.Cout = Cout;
    g.stats = gn_part; g.stats_split = conv_wino_ups_stats_split(Hs);
    VD_REQUIRE(conv_wino_r64_supported(g), "vd_op_conv_wino_ups: shape not covered (square power-of-two source map >= 8, Cout % 64, Cin % 32)");
    return launch_igemm(g, static_cast<hipStream_t>(stream));            // cuts big windows along frames like the engine
}

int vd_pack_conv3_split(const float* host_oihw, unsigned short* host_out, int O, int I) {
    VD_REQUIRE(host_oihw && host_out && O % 32 == 0 && I % 32 == 0, "vd_pack_conv3_split: O, I multiples of 32");
    pack_conv3_split(host_oihw, host_out, O, I);
    return 0;
}

int vd_op_conv_split(const float* src0, int Cin, int nfr, int Hs, int Ws, int stride, const void* w_split, const float* bias,
                     const float* res, float* out, int Cout, void* stream) {
    IgemmArgs g = conv_args(src0, nullptr, Cin, Cin, nfr, Hs, Ws, 0, stride, 1, 3);
    g.wfrag = static_cast<const float*>(w_split); g.wsplit = 1; g.bias = bias; g.res = res; g.res_ld = Cout;
    g.out = out; g.ldo = Cout; g.Cout = Cout;
    VD_REQUIRE(conv_split_supported(g), "vd_op_conv_split: shape not covered by the kernel");
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_pack_linear_split(const float* host_w, unsigned short* host_out, int N, int K) {
    VD_REQUIRE(host_w && host_out && N % 32 == 0 && K % 32 == 0, "vd_pack_linear_split: N, K multiples of 32");
    pack_linear_split(host_w, host_out, N, K, N, 0);
    return 0;
}

int vd_op_linear_split(const float* a, int M, int K, const void* w_split, const float* bias, const float* res, int act,
                       float* out, int N, void* stream) {
    IgemmArgs g = linear_args(M, K, N);
    g.src0 = a; g.wfrag = static_cast<const float*>(w_split); g.wsplit = 1; g.bias = bias; g.act = act; g.res = res; g.out = out;
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_op_linear_split_stats(const float* a, int M, int K, const void* w_split, const float* bias, const float* res, int act,
                             float* out, int N, int HW, double* gn_part, void* stream) {
    IgemmArgs g = linear_args(M, K, N);
    g.src0 = a; g.wfrag = static_cast<const float*>(w_split); g.wsplit = 1; g.bias = bias; g.act = act; g.res = res; g.out = out;
    VD_REQUIRE(gn_part && HW > 0 && gemm_split_supported(g), "vd_op_linear_split_stats: shape not covered by gemm_split.hip");
    g.stats = gn_part; g.stats_hw = HW; g.stats_split = HW / gemm_split_stats_rows(M, N);
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_linear_stats_split(int M, int N, int HW) { return HW / gemm_split_stats_rows(M, N); }

int vd_pack_conv3_wino(const float* host_oihw, float* host_out, int O, int I) {
    VD_REQUIRE(host_oihw && host_out && O % 64 == 0 && I % 16 == 0, "O multiple of 64, I multiple of 16");
    pack_conv3_wino(host_oihw, host_out, O, I);
    return 0;
}

int vd_pack_linear_frag(const float* host_w, float* host_out, int N, int K) {
    VD_REQUIRE(host_w && host_out && N % 32 == 0 && K % 32 == 0, "N and K multiples of 32");
    pack_linear_frag(host_w, host_out, N, K, N, 0);
    return 0;
}

int vd_profile_begin(void) {
    for (auto& r : g_prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.recs.clear();
    g_prof.on = true;
    return 0;
}

int vd_profile_end(double* out, int cap) {
    g_prof.on = false;
    VD_REQUIRE(out && cap >= 4 * PC_COUNT, "output needs 4*vd_profile_classes() doubles");
    for (int i = 0; i < 4 * PC_COUNT; ++i) out[i] = 0.0;
    for (auto& r : g_prof.recs) {
        VD_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        VD_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        out[r.cls * 4 + 0] += 1.0; out[r.cls * 4 + 1] += ms; out[r.cls * 4 + 2] += r.flops; out[r.cls * 4 + 3] += r.bytes;
        if (getenv("VD_PROF_DUMP"))                    // per-launch listing for kernel work (tools/)
            fprintf(stderr, "[vd_prof] %-28s %-40s %8.1f us %7.1f TFLOP/s\n", prof_name(r.cls), r.tag, ms * 1e3,
                    ms > 0 ? r.flops / ms / 1e9 : 0.0);
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    g_prof.recs.clear();
    return 0;
}

int vd_profile_classes(void) { return PC_COUNT; }
const char* vd_profile_class_name(int i) { return prof_name(i); }

// ---- single-operator entry points ---------------------------------------------------------------
int vd_op_conv(const float* src0, const float* src1, int C0, int Cin, int nfr, int Hs, int Ws, int ups, int stride,
               int pad, int ksz, const float* w, const float* w_frag, const float* w_wino, const float* bias, const float* affA,
               const float* affB, int act,
               const float* res, const float* fbias, int fbias_ld, float* out, int Cout, void* stream) {
    IgemmArgs g = conv_args(src0, src1, C0, Cin, nfr, Hs, Ws, ups, stride, pad, ksz);
    g.w = w; g.wfrag = w_frag; g.wwino = w_wino; g.bias = bias; g.affA = affA; g.affB = affB; g.act = act; g.res = res; g.res_ld = Cout;
    g.fbias = fbias; g.fbias_ld = fbias_ld; g.out = out; g.ldo = Cout; g.Cout = Cout;
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_conv_stats_split(int Hout) { return conv_wino_stats_split(Hout); }
int vd_conv_wino_block_couts(int nfr, int H, int Cin, int Cout) { return conv_wino_z128_shape(nfr, H, Cin, Cout) ? 128 : 64; }

// ---- which instantiation a conv / linear call runs on (the tables of igemm.hip, gemm_split.hip, gemm_frag.hip, conv_wino*.hip): no launch
static int copy_name(const std::string& n, char* name, int cap, const char* who) {
    VD_REQUIRE((int)n.size() < cap, std::string(who) + ": name buffer too small");
    memcpy(name, n.c_str(), n.size() + 1);
    return 0;
}

int vd_igemm_variant(int ksz, int stride, int ups, int Cin, int C0, int Cout, int nfr, int nfr_sel, int H, int weights, int act, int affine,
                     int fbias, int res, int side, int zcount, int ksplit_scratch, char* name, int cap) {
    VD_REQUIRE(name && cap > 0, "vd_igemm_variant: a name buffer");
    VD_REQUIRE(weights >= 0 && weights <= 5 && H > 0 && nfr > 0 && stride > 0, "vd_igemm_variant: weights 0..5, positive H, nfr and stride");
    const float* any = reinterpret_cast<const float*>(0x1000);      // presence only: nothing is read
    IgemmArgs g = conv_args(any, C0 < Cin ? any : nullptr, C0, Cin, nfr, H, H, ups, stride, ksz == 3 ? 1 : 0, ksz);
    g.nfr_sel = nfr_sel;
    g.w = weights == 0 ? any : nullptr;
    g.wfrag = weights == 1 || weights == 3 ? any : nullptr;
    g.wwino = weights == 2 || weights >= 4 ? any : nullptr;
    g.wsplit = weights == 3 ? 1 : weights >= 4 ? 2 : 0;
    g.ups_phase = weights == 5;
    g.act = act;
    if (affine) { g.affA = any; g.affB = any; }
    if (fbias) { g.fbias = any; g.fbias_ld = Cout; }
    if (res) g.res = any;
    g.res_ld = Cout; g.out = const_cast<float*>(any); g.ldo = Cout; g.Cout = Cout;
    if (side) { g.side = const_cast<float*>(any); g.sideA = any; g.sideB = any; g.side_hw = g.Ho * g.Wo; }
    g.zcount = zcount; g.zs_a = g.M * Cin; g.zs_out = g.M * Cout;
    if (ksplit_scratch) { g.ksplit_ws = const_cast<float*>(any); g.ksplit_ws_floats = conv_wino_r64_ksplit_floats(nfr, g.Ho, Cin, Cout, nfr_sel); }
    const IgemmVariant v = igemm_variant(g);
    if (int rc = copy_name(igemm_variant_name(v), name, cap, "vd_igemm_variant")) return rc;
    return v.name ? 1 : 0;
}

int vd_igemm_variant_list(char* names, int cap) {
    VD_REQUIRE(names && cap > 0, "vd_igemm_variant_list: a name buffer");
    std::vector<std::string> rows;
    igemm_variant_names(rows);
    std::string all;
    for (const std::string& r : rows) all += r + "\n";
    if (int rc = copy_name(all, names, cap, "vd_igemm_variant_list")) return rc;
    return (int)rows.size();
}

int vd_conv_wino_ksplit(int nfr, int H, int Cin, int Cout) { return conv_wino_r64_ksplit(nfr, H, Cin, Cout); }

// vd_op_conv_wino_split as the engine's res_block launches it: split-K scratch of conv_wino_r64_ksplit_floats() offered, slices and kernel
// chosen for nfr_sel frames (0: nfr)
int vd_op_conv_wino_split_k(const float* src0, int Cin, int nfr, int Hs, int Ws, int ups, const void* w_split, const float* bias,
                            const float* res, const float* fbias, int fbias_ld, float* out, int Cout, double* gn_part, int nfr_sel,
                            void* stream) {
    IgemmArgs g = conv_args(src0, nullptr, Cin, Cin, nfr, Hs, Ws, ups, 1, 1, 3);
    g.nfr_sel = nfr_sel;
    g.wwino = static_cast<const float*>(w_split); g.wsplit = 2; g.bias = bias; g.res = res; g.res_ld = Cout;
    g.fbias = fbias; g.fbias_ld = fbias_ld; g.out = out; g.ldo = Cout; g.Cout = Cout;
    g.stats = gn_part; g.stats_split = conv_wino_stats_split(g.Ho);
    VD_REQUIRE(conv_wino_r64_supported(g) && nfr_sel >= 0, "vd_op_conv_wino_split_k: shape not covered by conv_wino_r64.hip");
    OpScratch ws(stream);
    g.ksplit_ws_floats = conv_wino_r64_ksplit_floats(nfr, g.Ho, Cin, Cout, nfr_sel);
    if (g.ksplit_ws_floats)
        if (int rc = ws.get(&g.ksplit_ws, g.ksplit_ws_floats)) return rc;
    return launch_igemm(g, ws.st);
}

// The fused skip conv of res_block: a 1x1 over the virtual concat (a0: C0 channels, a1: K - C0 or null) on the 128x128 tile whose column
// blocks 0 also write side = SiLU(a * sideA[frame] + sideB[frame])
int vd_op_linear_split_side(const float* a0, const float* a1, int C0, int K, int M, int HW, const void* w_split, const float* bias,
                            const float* sideA, const float* sideB, float* out, float* side, int N, void* stream) {
    int H = 1;
    while (H * H < HW) ++H;
    VD_REQUIRE(a0 && (a1 ? C0 > 0 && C0 < K : C0 == K) && HW > 0 && H * H == HW && M > 0 && M % HW == 0 && out && side && sideA && sideB,
               "vd_op_linear_split_side: one source of K channels or two of C0 and K - C0, M whole frames of HW = H x H rows");
    IgemmArgs g = conv_args(a0, a1, C0, K, M / HW, H, H, 0, 1, 0, 1);
    g.wfrag = static_cast<const float*>(w_split); g.wsplit = 1; g.bias = bias; g.out = out; g.ldo = N; g.Cout = N; g.res_ld = N;
    g.side = side; g.sideA = sideA; g.sideB = sideB; g.side_hw = HW;
    VD_REQUIRE(gemm_split_side_supported(g), "vd_op_linear_split_side: not a plain 1x1 on the 128x128 tile of gemm_split.hip over whole frames of a multiple of 128 rows");
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

// The zcount launch of rpe_all in the process' arithmetic: problem z reads a + z M K, writes out + z M N, its weight image (the mode's:
// vd_pack_linear_split, or vd_pack_linear_frag under VD_MATH=fp32) at zbase + ztab[2z] and its bias at zbase + ztab[2z + 1]
int vd_op_linear_batched(const float* a, int zcount, int M, int K, int N, const float* zbase, const long long* ztab_dev, float* out,
                         void* stream) {
    VD_REQUIRE(a && zcount > 1 && M > 0 && zbase && ztab_dev && out, "vd_op_linear_batched: zcount >= 2 problems and a device table of 2 zcount offsets");
    long long z0[2];
    VD_HIP(hipMemcpy(z0, ztab_dev, sizeof(z0), hipMemcpyDeviceToHost));
    IgemmArgs q = linear_args(M, K, N);
    q.src0 = a; q.out = out;
    q.wfrag = zbase + z0[0]; q.bias = zbase + z0[1];                    // (problem 0's: the shape checks read them)
    q.zcount = zcount; q.zs_a = M * K; q.zs_out = M * N; q.ztab = ztab_dev; q.zbase = zbase;
    VD_REQUIRE(igemm_kernel(q) == (split_math() ? IK_SPLIT : IK_FRAG), "vd_op_linear_batched: shape not covered by gemm_split.hip / gemm_frag.hip");
    return launch_igemm(q, static_cast<hipStream_t>(stream));
}

int vd_op_conv_stats(const float* src0, int Cin, int nfr, int Hs, int Ws, int ups, const float* w_wino, const float* bias,
                     const float* res, const float* fbias, int fbias_ld, float* out, int Cout, double* gn_part,
                     void* stream) {
    IgemmArgs g = conv_args(src0, nullptr, Cin, Cin, nfr, Hs, Ws, ups, 1, 1, 3);
    g.wwino = w_wino; g.bias = bias; g.res = res; g.res_ld = Cout; g.fbias = fbias; g.fbias_ld = fbias_ld;
    g.out = out; g.ldo = Cout; g.Cout = Cout;
    g.stats = gn_part; g.stats_split = conv_wino_stats_split(g.Ho);
    VD_REQUIRE(conv_wino_supported(g), "vd_op_conv_stats: shape not covered by the Winograd kernel");
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_op_gn_affine(const double* part0, int split0, int C0, const double* part1, int split1, int C, int nfr, int HW,
                    const float* gamma, const float* beta, const float* film, int film_ld, float* affA, float* affB,
                    void* stream) {
    return launch_gn_affine(part0, split0, C0, part1, split1, (double)HW * (C / 32), gamma, beta, film, film_ld, nfr, C, affA,
                            affB, static_cast<hipStream_t>(stream));
}

int vd_op_gn_affine_mr(const double* part0, int split0, int C0, const double* part1, int split1, int C, int nfr, int HW,
                       const float* gamma, const float* beta, const float* film, int film_ld, float* affA, float* affB,
                       float* mr_out, void* stream) {
    return launch_gn_affine(part0, split0, C0, part1, split1, (double)HW * (C / 32), gamma, beta, film, film_ld, nfr, C, affA,
                            affB, static_cast<hipStream_t>(stream), mr_out);
}

int vd_gn_stats_split(int nfr, int HW, int C) {
    if (nfr <= 0 || HW <= 0 || C < 32 || C % 32 != 0 || C > 1024) return -1;
    return gn_stats_split(nfr, HW, C);
}

int vd_op_gn_stats(const float* src0, const float* src1, int C0, int C, int nfr, int HW, int split, double* part, void* stream) {
    VD_REQUIRE(nfr > 0 && HW > 0 && part, "vd_op_gn_stats: frames, pixels and the table");
    VD_REQUIRE(C >= 32 && C % 32 == 0 && C <= 1024, "GroupNorm32 channel constraints");
    return launch_gn_stats(src0, src1, C0, C, nfr, HW, part, split > 0 ? split : gn_stats_split(nfr, HW, C),
                           static_cast<hipStream_t>(stream));
}

int vd_op_gn_act_fold(const float* src0, const float* src1, int C0, int C, const double* part0, int split0, const double* part1,
                      int split1, int nfr, int HW, const float* gamma, const float* beta, const float* film, int film_ld, int act,
                      float* y, void* stream) {
    VD_REQUIRE(nfr > 0 && HW > 0 && y && gamma && beta, "vd_op_gn_act_fold: frames, pixels and buffers");
    GnFold f{part0, split0, part1, split1, (double)HW * (C / 32), gamma, beta, film, film_ld};
    return launch_affine_act_fold(src0, src1, C0, C, f, nfr, HW, act, y, static_cast<hipStream_t>(stream));
}

int vd_gn_act_form(int layer_frames, int HW, int C) { return gn_act_form(layer_frames, HW, C); }

int vd_op_gn_fold(const float* src0, const float* src1, int C0, int C, int nfr, int HW, const float* gamma,
                  const float* beta, const float* film, int film_ld, float* affA, float* affB, void* stream) {
    OpScratch ws(stream);
    const int split = gn_stats_split(nfr, HW, C);
    double* part;
    int rc = ws.get(&part, (size_t)nfr * split * C * 2);
    if (!rc) rc = launch_gn_stats(src0, src1, C0, C, nfr, HW, part, split, ws.st);
    if (!rc) rc = launch_gn_affine(part, split, C, nullptr, 0, (double)HW * (C / 32), gamma, beta, film, film_ld, nfr, C, affA, affB, ws.st);
    return rc;
}

int vd_op_affine_act(const float* src0, const float* src1, int C0, int C, const float* affA, const float* affB, int nfr,
                     int HW, int act, float* y, void* stream) {
    return launch_affine_act(src0, src1, C0, C, affA, affB, nfr, HW, act, y, static_cast<hipStream_t>(stream));
}

int vd_op_affine_apply(const float* x, const float* affA, const float* affB, int nfr, int HW, int C, float* y, void* stream) {
    return launch_affine_apply(x, affA, affB, nfr, HW, C, y, static_cast<hipStream_t>(stream));
}

int vd_op_gn_temporal(const float* x, const float* gamma, const float* beta, int B, int T, int HW, int C, float* y,
                      void* stream) {
    return launch_gn_temporal(x, gamma, beta, B, T, HW, C, y, static_cast<hipStream_t>(stream));
}

int vd_op_attn_spatial(const float* qkv, int nfr, int L, int C, int heads, float* out, void* stream) {
    AttnSpatialArgs a{qkv, out, nfr, L, C, heads, heads > 0 && C >= heads ? 1.0f / sqrtf((float)(C / heads)) : 0.f};     // (a refused shape: never read)
    return launch_attn_spatial(a, static_cast<hipStream_t>(stream));
}

int vd_op_attn_temporal(const float* qkv, const float* Rk, const float* Rq, const float* Rv, const float* mask, int B,
                        int T, int HW, int C, int heads, int allow_pad, float* out, void* stream) {
    AttnTemporalArgs a{qkv, Rk, Rq, Rv, mask, out, B, T, HW, C, heads, allow_pad, 1.0f / sqrtf((float)(C / heads))};
    return launch_attn_temporal(a, static_cast<hipStream_t>(stream));
}

// ---- the return_attn_weights maps (backward.hip) on caller's tensors: the launchers the forward calls under vd_set_attn_capture,
// args filled as by the two entries above
int vd_op_attn_temporal_weights(const float* qkv, const float* Rk, const float* Rq, const float* mask, int B, int T, int HW, int C,
                                int heads, int allow_pad, float* out, void* stream) {
    VD_REQUIRE(qkv && out && B > 0 && HW > 0 && C > 0 && heads > 0 && (Rk != nullptr) == (Rq != nullptr),
               "vd_op_attn_temporal_weights: tensors, a positive shape, Rk and Rq both or neither");
    AttnTemporalArgs a{qkv, Rk, Rq, nullptr, mask, nullptr, B, T, HW, C, heads, allow_pad, 1.0f / sqrtf((float)(C / heads))};
    return launch_attn_temporal_weights(a, out, static_cast<hipStream_t>(stream));
}

int vd_op_attn_spatial_weights(const float* qkv, int nfr, int L, int C, int heads, float* out, void* stream) {
    VD_REQUIRE(qkv && out && nfr > 0 && L > 0 && C > 0 && heads > 0, "vd_op_attn_spatial_weights: tensors and a positive shape");
    AttnSpatialArgs a{qkv, nullptr, nfr, L, C, heads, 1.0f / sqrtf((float)(C / heads))};
    return launch_attn_spatial_weights(a, out, static_cast<hipStream_t>(stream));
}

int vd_attn_temporal_variant(int T, int HW, int C, int heads, int rpe, char* name, int cap) {
    VD_REQUIRE(name && cap > 0, "vd_attn_temporal_variant: a name buffer");
    const AttnTemporalVariant v = attn_temporal_variant(T, HW, C, heads, rpe != 0);
    const std::string n = attn_temporal_variant_name(v);
    VD_REQUIRE((int)n.size() < cap, "vd_attn_temporal_variant: name buffer too small");
    memcpy(name, n.c_str(), n.size() + 1);
    return v.family != AttnTemporalVariant::kRefused ? 1 : 0;
}

int vd_attn_spatial_variant(int L, int C, int heads, char* name, int cap) {
    VD_REQUIRE(name && cap > 0, "vd_attn_spatial_variant: a name buffer");
    const AttnSpatialVariant v = attn_spatial_variant(L, C, heads);
    const std::string n = attn_spatial_variant_name(v);
    VD_REQUIRE((int)n.size() < cap, "vd_attn_spatial_variant: name buffer too small");
    memcpy(name, n.c_str(), n.size() + 1);
    return v.row >= 0 ? 1 : 0;
}

int vd_op_out_conv(const float* x, const float* affA, const float* affB, const float* w, const float* bias, int nfr,
                   int H, int W, int C, int Cout, float* out, void* stream) {
    return launch_out_conv(x, affA, affB, w, bias, nfr, H, W, C, Cout, out, static_cast<hipStream_t>(stream));
}

// ---- the output head as the forward runs it (out_head(): GEMM over (cout, tap) columns + 9-tap gather), on caller's tensors
static const char* out_head_refusal(int nfr, int H, int W, int C, int Cout) {
    if (!(nfr > 0 && H > 0 && W > 0 && C > 0)) return "output head: positive nfr, H, W and C";
    if (!(Cout == 3 || Cout == 6)) return "output head: 3 or 6 output channels";
    if ((size_t)nfr * H * W >= ((size_t)1 << 31)) return "output head: 2^31 pixels or more";
    return nullptr;
}

int vd_out_head_variant(int nfr, int H, int W, int C, int Cout, char* name, int cap) {
    VD_REQUIRE(name && cap > 0, "vd_out_head_variant: a name buffer");
    std::string path;
    if (const char* why = out_head_refusal(nfr, H, W, C, Cout)) path = std::string("refused: ") + why;
    else {
        float* any = reinterpret_cast<float*>(0x1000);              // presence only: nothing is read
        if (int rc = out_head(any, any, any, any, any, nfr, H, W, C, Cout, any, any, nullptr, &path)) return rc;
    }
    if (int rc = copy_name(path, name, cap, "vd_out_head_variant")) return rc;
    return path.compare(0, 8, "refused:") != 0 ? 1 : 0;
}

int vd_op_out_head(const float* h, const float* affA, const float* affB, const float* w_oihw, const float* bias, int nfr, int H, int W,
                   int C, int Cout, float* out_nchw, void* stream) {
    VD_REQUIRE(h && affA && affB && w_oihw && bias && out_nchw, "vd_op_out_head: null argument");
    if (const char* why = out_head_refusal(nfr, H, W, C, Cout)) { set_error(std::string("requirement failed: ") + why); return -1; }
    std::vector<float> oihw((size_t)Cout * C * 9), wt((size_t)out_t_cols(Cout) * C);
    VD_HIP(hipMemcpy(oihw.data(), w_oihw, oihw.size() * sizeof(float), hipMemcpyDefault));      // (host or device memory)
    pack_out_head(oihw.data(), Cout, C, wt.data());
    OpScratch ws(stream);
    float *Wt = nullptr, *T = nullptr;
    int rc = ws.get(&Wt, wt.size());
    if (!rc) rc = ws.get(&T, (size_t)nfr * H * W * out_t_cols(Cout));
    if (rc) return rc;
    VD_HIP(hipMemcpy(Wt, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
    return out_head(h, affA, affB, Wt, bias, nfr, H, W, C, Cout, T, out_nchw, ws.st);
}

// ---- backward-data operators of use_gradient_method (backward.hip)
int vd_op_gn_bwd(const float* x0, const float* x1, int C0, int C, const float* affA, const float* affB, const float* mr,
                 const float* dy, int act, int nfr, int HW, const float* extra, float* dx0, int acc0, float* dx1, int acc1,
                 void* stream) {
    VD_REQUIRE(nfr > 0 && HW > 0 && C > 0 && C % 32 == 0 && C <= 1024, "vd_op_gn_bwd: shape");
    OpScratch ws(stream);
    double* part = nullptr;
    float* K = nullptr;
    int rc = ws.get(&part, (size_t)nfr * gn_bwd_split(nfr, HW, C) * C * 2);
    if (!rc) rc = ws.get(&K, (size_t)nfr * 32 * 2);
    if (rc) return rc;
    GnBwdArgs a{x0, x1, C0, C, affA, affB, mr, dy, act, nfr, HW, dx0, dx1, acc0, acc1, extra, part, K};
    return launch_gn_bwd(a, ws.st);
}

int vd_op_gn_temporal_bwd(const float* x, const float* gamma, const float* dy, int B, int T, int HW, int C, int accumulate,
                          float* dx, void* stream) {
    return launch_gn_temporal_bwd(x, gamma, dy, B, T, HW, C, accumulate, dx, static_cast<hipStream_t>(stream));
}

int vd_op_attn_temporal_bwd(const float* qkv, const float* Rk, const float* Rq, const float* Rv, const float* mask, int B,
                            int T, int HW, int C, int heads, int allow_pad, const float* dout, float* dqkv, void* stream) {
    AttnTemporalArgs a{qkv, Rk, Rq, Rv, mask, nullptr, B, T, HW, C, heads, allow_pad, 1.0f / sqrtf((float)(C / heads))};
    return launch_attn_temporal_bwd(a, dout, dqkv, static_cast<hipStream_t>(stream));
}

int vd_op_attn_spatial_bwd(const float* qkv, int nfr, int L, int C, int heads, const float* dout, float* dqkv, void* stream) {
    VD_REQUIRE(nfr > 0 && L > 0 && heads > 0 && C % heads == 0, "vd_op_attn_spatial_bwd: shape");
    AttnSpatialArgs a{qkv, nullptr, nfr, L, C, heads, 1.0f / sqrtf((float)(C / heads))};
    OpScratch ws(stream);
    float* buf = nullptr;
    int rc = ws.get(&buf, attn_spatial_bwd_ws_floats(a));
    return rc ? rc : launch_attn_spatial_bwd(a, dout, dqkv, buf, ws.st);
}

int vd_op_out_conv_bwd(const float* deps, const float* w, int nfr, int H, int W, int C, int Cout, float* da, void* stream) {
    return launch_out_conv_bwd(deps, w, nfr, H, W, C, Cout, da, static_cast<hipStream_t>(stream));
}

int vd_op_stem_col2im(const float* dcols, const float* obs, const float* lat, const float* km, int nfr, int H, int W,
                      int cond_mode, float* dx, void* stream) {
    return launch_stem_col2im(dcols, obs, lat, km, nfr, H, W, STEM_KPAD, cond_mode, dx, static_cast<hipStream_t>(stream));
}

// ---- what lies between those kernels in backward(): the weight images, the two matrix-product calls, resampling, rescale, guidance
static const char* kBwdSplitOnly = "use_gradient_method runs on the split arithmetic only (VD_MATH=f16x3 | bf16x6)";

long long vd_bwd_image_floats(int kind, int O, int I) {
    if (kind < BWD_LINEAR || kind > BWD_CONV3_GENERIC || O <= 0 || I <= 0) return -1;
    return (long long)bwd_image_floats(kind, (size_t)O, (size_t)I);
}

int vd_pack_weight_bwd(const float* host_w, int kind, int O, int I, float* host_out) {
    VD_REQUIRE(host_w && host_out && kind >= BWD_LINEAR && kind <= BWD_CONV3_GENERIC && O > 0 && I > 0, "vd_pack_weight_bwd: weight, image, kind 0..3 and a positive shape");
    VD_REQUIRE(kind != BWD_STEM || 9 * I <= STEM_KPAD, "vd_pack_weight_bwd: a stem of at most 7 input channels");
    VD_REQUIRE(kind == BWD_CONV3_GENERIC || (O % 32 == 0 && (kind == BWD_STEM || I % 32 == 0)), "vd_pack_weight_bwd: split images need multiples of 32");
    VD_REQUIRE(kind != BWD_CONV3_WINO || I % 64 == 0, "vd_pack_weight_bwd: the Winograd-split image needs a multiple of 64 forward inputs");
    std::fill(host_out, host_out + bwd_image_floats(kind, (size_t)O, (size_t)I), 0.f);
    pack_weight_bwd(host_w, kind, O, I, host_out);
    return 0;
}

int vd_op_conv3_bwd_data(const float* dy, int nfr, int H, int cin_bwd, const void* w_bwd, int kind, int cout_bwd, const float* res, float* out,
                         void* stream) {
    VD_REQUIRE(split_math(), kBwdSplitOnly);
    VD_REQUIRE(dy && w_bwd && out && nfr > 0 && H > 0 && cin_bwd > 0 && cout_bwd > 0, "vd_op_conv3_bwd_data: tensors and a positive shape");
    VD_REQUIRE(kind == BWD_CONV3_WINO || kind == BWD_CONV3_GENERIC, "vd_op_conv3_bwd_data: kind 2 (Winograd-split image) or 3 ([tap][Cout'][Cin'])");
    const int pk = kind == BWD_CONV3_WINO ? (int)PK_CONV3W : (int)PK_CONV3;
    const Tens t{const_cast<float*>(dy), cin_bwd, H};
    OpScratch ws(stream);
    float* ksw = nullptr;
    const size_t ksf = bwd_conv3_scratch(Arena{}, pk, t, nfr, cout_bwd);
    if (ksf)
        if (int rc = ws.get(&ksw, ksf)) return rc;
    return launch_igemm(bwd_conv3_args(t, nfr, pk, static_cast<const float*>(w_bwd), cout_bwd, res, out, ksw, ksf), ws.st);
}

int vd_op_linear_bwd_data(const float* dy, int M, int K, const void* w_bwd, const float* res, float* out, int N, void* stream) {
    VD_REQUIRE(split_math(), kBwdSplitOnly);
    VD_REQUIRE(dy && w_bwd && out && M > 0 && K > 0 && N > 0, "vd_op_linear_bwd_data: tensors and a positive shape");
    const IgemmArgs g = bwd_linear_args(dy, M, K, N, static_cast<const float*>(w_bwd), res, out);
    VD_REQUIRE(gemm_split_supported(g), "backward linear layer: shape not covered by gemm_split.hip");
    return launch_igemm(g, static_cast<hipStream_t>(stream));
}

int vd_op_zero_stuff2(const float* x, int nfr, int Ho, int Wo, int C, float* y, void* stream) {
    VD_REQUIRE(x && y && nfr > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0, "vd_op_zero_stuff2: channels in 16-byte units");
    return launch_zero_stuff2(x, nfr, Ho, Wo, C, y, static_cast<hipStream_t>(stream));
}

int vd_op_sumpool2(const float* x, int nfr, int Ho, int Wo, int C, int accumulate, float* y, void* stream) {
    VD_REQUIRE(x && y && nfr > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0, "vd_op_sumpool2: channels in 16-byte units");
    return launch_sumpool2(x, nfr, Ho, Wo, C, accumulate, y, static_cast<hipStream_t>(stream));
}

int vd_op_add(const float* x, long long n, int accumulate, float* y, void* stream) {
    VD_REQUIRE(x && y && n > 0, "vd_op_add: tensors and a positive count");
    return launch_add(x, (size_t)n, accumulate, y, static_cast<hipStream_t>(stream));
}

int vd_op_grad_rescale(float* g, long long n, float* gs, void* stream) {
    VD_REQUIRE(g && gs && n > 0, "vd_op_grad_rescale: the gradient, four words and a positive count");
    return launch_grad_rescale(g, (size_t)n, gs, static_cast<hipStream_t>(stream));
}

int vd_op_guided_grad(vd_engine* e, int B, int T, long long per, const float* x, const float* eps, const float* noise, const float* x_t_minus_1,
                      const float* obs, const long long* t, int clip, float* deps, float* dxd, float* mean, float* xstart, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && per > 0 && per % T == 0 && x && eps && noise && x_t_minus_1 && obs && t && deps && dxd, "vd_op_guided_grad: arguments");
    GuidedArgs ga{x, eps, noise, x_t_minus_1, obs, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, (long)per, clip, deps, dxd, mean, xstart};
    ga.err = e->d_err;
    return launch_guided_grad(ga, static_cast<hipStream_t>(stream));
}

int vd_op_guided_final(vd_engine* e, int B, int T, long long per, const long long* t, const float* dxd, const float* mean, const float* dx_net,
                       const float* gs, const float* noise2, float* grad, float* mean_out, float* sample, void* stream) {
    VD_REQUIRE(e && e->d_tab, "vd_set_schedule not called");
    VD_REQUIRE(B > 0 && T > 0 && per > 0 && per % T == 0 && t && dxd && mean && dx_net && gs && (!sample || noise2), "vd_op_guided_final: arguments");
    GuidedArgs ga{nullptr, nullptr, nullptr, nullptr, nullptr, reinterpret_cast<const int64_t*>(t), e->d_tab, e->num_timesteps, B, T, (long)per, 0,
                  nullptr, const_cast<float*>(dxd), const_cast<float*>(mean), nullptr};
    ga.gscale = gs;
    return launch_guided_final(ga, dx_net, noise2, grad, mean_out, sample, static_cast<hipStream_t>(stream));
}

// ---- the kernels that build what the network is conditioned on (misc.hip), through the launchers forward() calls
int vd_op_sinus_embed(const float* t, int n, int dim, const float* freqs, float* out, void* stream) {
    VD_REQUIRE(t && freqs && out && n > 0 && dim >= 2, "vd_op_sinus_embed: n rows of dim >= 2 columns, dim / 2 frequencies");
    return launch_sinus_embed(t, n, dim, freqs, out, static_cast<hipStream_t>(stream));
}

int vd_op_frame_t(const long long* fidx, int B, int T, int center, float* tv, void* stream) {
    VD_REQUIRE(fidx && tv && B > 0 && T > 0, "vd_op_frame_t: shape");
    return launch_frame_t(reinterpret_cast<const int64_t*>(fidx), B, T, center, tv, static_cast<hipStream_t>(stream));
}

int vd_op_rpe_hidden(const float* te, int te_ld, const float* wbase, const long long* tab, const long long* fidx, int B, int T, int C,
                     float* E, int nz, long long zs_e, void* stream) {
    VD_REQUIRE(te && wbase && tab && fidx && E && B > 0 && T > 0 && C > 0 && nz > 0, "vd_op_rpe_hidden: shape");
    VD_REQUIRE(te_ld >= C && zs_e >= (long long)B * T * T * C, "vd_op_rpe_hidden: te rows of at least C floats, a net's output inside its stride");
    return launch_rpe_hidden_tab(te, te_ld, wbase, tab, reinterpret_cast<const int64_t*>(fidx), B, T, C, E, nz, (size_t)zs_e,
                                 static_cast<hipStream_t>(stream));
}

int vd_op_rpe_table(const float* table, const long long* fidx, int B, int T, int C, float alpha, float beta, float gamma, float* R,
                    void* stream) {
    VD_REQUIRE(table && fidx && R && B > 0 && T > 0 && C > 0, "vd_op_rpe_table: shape");
    VD_REQUIRE(alpha >= 1.f && beta >= alpha && gamma >= alpha, "vd_op_rpe_table: bucket parameters 1 <= alpha <= beta, alpha <= gamma");
    return launch_rpe_table(table, reinterpret_cast<const int64_t*>(fidx), B, T, C, alpha, beta, gamma, R, static_cast<hipStream_t>(stream));
}

int vd_op_posenc_add(const float* x, const float* P, const float* femb, int nfr, int HW, int C, float* y, void* stream) {
    VD_REQUIRE(x && y && nfr > 0 && HW > 0 && C > 0 && C % 4 == 0, "vd_op_posenc_add: channels in 16-byte units");
    return launch_posenc_add(x, P, femb, nfr, HW, C, y, static_cast<hipStream_t>(stream));
}

int vd_op_assemble(const float* x, const float* obs_src, const float* obs_mask, const float* latent_mask, const float* kinda_marg_mask,
                   const float* t_model, int obs_t_mode, int B, int T, int H, int W, int Kpad, int cond_mode, const int* frame_list,
                   int n_list, int scalars_only, float* x_cols, float* t_frames, float* amask, void* stream) {
    VD_REQUIRE(x && obs_src && obs_mask && latent_mask && kinda_marg_mask && B > 0 && T > 0 && H > 0 && W > 0, "vd_op_assemble: shape");
    VD_REQUIRE(cond_mode >= 0 && cond_mode <= 2 && obs_t_mode >= 0 && obs_t_mode <= 2, "vd_op_assemble: cond_mode / obs_t_mode 0, 1 or 2");
    VD_REQUIRE(frame_list ? n_list >= 0 && n_list <= B * T : (t_model && t_frames && amask), "vd_op_assemble: a list of at most B*T frames, or the per-frame scalars");
    VD_REQUIRE(scalars_only || x_cols, "vd_op_assemble: x_cols");
    AssembleArgs a{x, obs_src, obs_mask, latent_mask, kinda_marg_mask, t_model, obs_t_mode, B, T, H, W, Kpad, cond_mode, x_cols, t_frames, amask};
    a.frame_list = frame_list; a.n_list = n_list; a.scalars_only = scalars_only;
    return launch_assemble(a, static_cast<hipStream_t>(stream));
}

int vd_op_move_rows(int scatter, const float* src, const int* list, int n, long long row_floats, float* dst, void* stream) {
    VD_REQUIRE(n >= 0 && row_floats > 0 && (n == 0 || (src && list && dst)), "vd_op_move_rows: shape");
    return scatter ? launch_scatter_rows(src, list, n, (size_t)row_floats, dst, static_cast<hipStream_t>(stream))
                   : launch_gather_rows(src, list, n, (size_t)row_floats, dst, static_cast<hipStream_t>(stream));
}

int vd_op_scatter_stats(const double* src, int split, int C, const int* list, int n, double* dst, void* stream) {
    VD_REQUIRE(n >= 0 && split > 0 && C > 0 && (n == 0 || (src && list && dst)), "vd_op_scatter_stats: shape");
    return launch_scatter_stats(src, split, C, list, n, dst, static_cast<hipStream_t>(stream));
}

}  // extern "C"
