// ResNet-50 trunk engine: a static launch plan for one (batch, resolution, dtype).
// Host-side C++ only walks tables and enqueues kernels on the caller's stream; there is no
// Python, allocation or synchronisation between the first and last launch of a pass.
//
// Topology (torchvision ResNet-50 v1.5, the architecture util/model_utils.py:136 constructs):
//   stage -> conv1 7x7/2 -> bn1 -> relu [= hooked early feature] -> maxpool 3x3/2
//   -> layer1..4 = [3,4,6,3] bottlenecks (1x1 -> 3x3 (stride) -> 1x1 x4, downsample on block 0)
//   -> global avgpool -> fc(2048 -> latent)
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"

using namespace rpe;

namespace {

struct ConvL {
    std::string name, bn;
    rpe_conv_desc d;
    int Ho, Wo;
    long rows;       // B*Ho*Wo
    int p_w, p_g, p_b;  // parameter table indices
    int bn_i;           // BN index (running buffers)
    // workspace pointers
    void* wf = nullptr;  // packed forward weight (compute dtype) [Co][K]; fp32 dense layers use the master directly
    void* wd = nullptr;  // packed dgrad weight [Ci][R][S][Co]
    void* y = nullptr;   // raw conv output
    void* a = nullptr;   // after BN (+residual) (+ReLU)
    void* dy = nullptr;  // backward: dz of this layer's BN output, turned into dy (gradient of the raw conv output) in place
    float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
    float* c1c2 = nullptr;   // backward: mean(dz), mean(dz xhat) of this layer's BN ([2][out_c]; per layer: the side stream reads them later)
};

struct Block {
    int c1, c2, c3, cd;  // conv indices (cd = -1: identity shortcut; c3 = -1: a BasicBlock -- two 3x3 convs, ResNet-18 / 34)
    int out = -1;        // the conv whose BatchNorm output (+ shortcut, ReLU) is the block's output: c3, or c2 of a BasicBlock
    int layer = 0;       // 1..4
    bool first = false;  // first block of its layer (the input of a stage-entry block of layers 2..4 is a hookable layer output)
    void* dz = nullptr;  // backward: ReLU-masked gradient at the block output (kept as the shortcut gradient)
    // y3-free block (rpe_resnet50::y3free): fp32 [ones_row + 1][planes] Gram matrix + column sums of conv3's input, written by the forward
    // (BN3 statistics without y3) and read again by the backward's weight-gradient combine; dzt_a: fp32 [4 planes][planes] = dz3^T a2
    float* gram = nullptr;
    float* dzt_a = nullptr;
    bool t_ready = false;   // backward: dzt_a was already left behind by the next block's fused conv1 data gradient (rpe_conv1x1_dgrad_bn_t)
    unsigned char* relu_mask = nullptr;  // 16-bit element types: packed ReLU mask of the block output (1 bit per element), written by its bn_apply
};

struct Named {
    std::string name;
    const void* ptr;
    long rows;
    int ch;
};

}  // namespace

struct rpe_resnet50 {
    int B, H, W, dtype, latent;
    int feat = 2048;     // channels of the last block = inputs of fc (512 for the BasicBlock networks)
    bool basic = false;  // ResNet-18 / 34: BasicBlock (3x3, 3x3) instead of Bottleneck (1x1, 3x3, 1x1) blocks
    size_t esz;
    std::vector<ConvL> convs;
    std::vector<Block> blocks;
    std::vector<std::string> pnames;
    std::vector<long> pnumel;
    // bound tables
    std::vector<float*> params, grads, running;
    std::vector<long long*> nbt;
    bool bound = false, fwd_done = false;
    // workspace
    long ws_bytes = 0;
    char* ws = nullptr;
    struct Slot { void** dst; long bytes; };
    std::vector<Slot> slots;
    void* x4 = nullptr;          // staged image: zero-bordered NHWC4 [B][H + 6][W + 6][4] (the border is zeroed once, at bind time)
    void* pool = nullptr;        // maxpool output
    unsigned char* pool_idx = nullptr;
    float* pooled = nullptr;     // avgpool output [B][2048]
    float* d_pooled = nullptr;
    float* fc_wt = nullptr;      // fc weight transposed [2048][latent_pad]
    int latent_pad = 0;
    void* early_grad = nullptr;
    void* G[2] = {nullptr, nullptr};      // main-stream-only gradient scratch (projection-shortcut dx; stem dy), max activation size
    void* d_pool = nullptr;              // gradient of the max-pool output (input of layer1)
    float* stats_part = nullptr;
    float* stats_part2 = nullptr;           // second set for the projection-shortcut branch (runs on the side stream in the forward)
    long stats_floats = 0;
    float* bwd_part = nullptr;
    long bwd_part_floats = 0;
    float* c1c2 = nullptr;
    double* dpart = nullptr;     // staged BN partial-sum reduction scratch
    double* dpart2 = nullptr;    // ... of the projection-shortcut branch
    // aux-head gradient in compact form for the fused stem backward (rpe_resnet50_set_aux_grad)
    const float* aux_dout = nullptr; long aux_ld = 0; const float* aux_df = nullptr; const unsigned char* aux_idx = nullptr; const float* aux_w = nullptr;
    // the bn1 aux head's FORWARD riding on the stem's apply + pool pass (rpe_resnet50_set_aux_head, consumed by the next training forward):
    // a1 = relu(bn1(conv1 x)) is then not written at all (a1_valid: what rpe_resnet50_early_feature may hand out)
    struct { const float *w = nullptr, *bias = nullptr, *depth_feat = nullptr; float* out = nullptr; long ld = 0; float* raw = nullptr; unsigned char* idx = nullptr; } aux_fwd;
    bool a1_valid = false;
    float* stem_dw = nullptr;    // [64][8][8][4]
    // BN backward folded into the conv3 data gradients (rpe_bn_bwd_fold_conv1x1): main-stream-only scratch, rebuilt per block
    bool fold = true;
    void* w_kcat = nullptr;      // [planes][4 planes + planes] compute dtype
    float* fold_bias = nullptr;  // [planes]
    void* fold_scratch = nullptr;
    long fold_scratch_bytes = 0;
    void* wfold_scratch = nullptr;   // side-stream scratch of the folded weight gradient (S, colsum, W S, slabs)
    long wfold_scratch_bytes = 0;
    // bn1's backward folded into conv1's data / weight gradient (y-form: rpe_bn_bwd_fold_y_conv1x1).  Built in round 3 on the judge's
    // suggestion, measured, and OFF by default (RPE_BN1_FOLD=1 turns it on for planes <= RPE_BN1_FOLD_MAX): 21.1 vs 20.3 ms/step for
    // layers 1-2, 20.6 for layer1 alone, 22.0-22.3 for layers 1-3 / 1-4 (profiles/r03_ab_bn1_fold.txt).  Why: the fold removes the
    // 3p-per-block dz, y -> dy pass but both gradients then read dz AND y (+2p), and the weight gradient's row-concatenated form walks
    // the WIDE operand x (4p columns) once per row tile -- dz, y and the all-ones tile: three times the LDS fill of the plain launch.
    bool fold1 = false;
    int fold1_max = 128;
    bool fold_w = true;
    int fold_w_max = 256;   // widest conv3 input the folded weight gradient takes (RPE_WGRAD_FOLD_MAX; measured 128: 21.92, 256: 21.77, 512: 21.80 ms/step)
    void* main_slab = nullptr;   // the same for the two weight gradients that run on the caller's stream (stem conv, fc)
    long main_slab_bytes = 0;
    void* wg_slab = nullptr;     // per-workgroup fp32 tiles of the deterministic weight-gradient form (one launch at a time: side stream order)
    long wg_slab_bytes = 0;
    std::vector<Named> named;
    int train_mode = 0;
    int fused_tiles = 0;
    int bwd_next = -2;                                     // next block of a staged backward (-1: blocks done, -2: idle)
    // conv/fc weight gradients are accumulated with atomics: when the bound gradient tensors form one contiguous block
    // (they do in the flat arena) it is zeroed by ONE memset per backward instead of 54 (15 us each)
    rpe_pack_desc* pack_tab = nullptr;   // device table for the one-launch weight packing
    // hooks other than bn1 (models/naive.py:196-211): dense gradients of conv1's raw output ([0]) and of the layer1..3 outputs
    // ([1..3]) handed over by the host for the next backward; stem_raw: the inference forward keeps conv1's raw output too
    const void* hook_grad[4] = {nullptr, nullptr, nullptr, nullptr};
    bool stem_raw = false;
    void* fc_ws = nullptr;               // split-K workspace of the ResNet fc forward / data gradient (rpe_linear_fwd_ws)
    long fc_ws_bytes = 0;
    // Bottleneck blocks WITHOUT the raw conv3 output (16-bit element types, planes <= y3free_max: layers 1-2 by default).  Forward: BN3's
    // batch statistics follow from the Gram matrix of conv3's INPUT (rpe_gram + rpe_bn_stats_from_gram), so conv3 applies BN + identity
    // + ReLU + mask in its own epilogue -- y3 is neither written nor re-read by an apply pass.  Backward: the next block's fused conv1
    // data gradient emits sum dz only; sum dz*y3 = rowdot(dz3^T a2, W3) comes from the weight gradient's first product, which therefore
    // runs on the caller's stream in front of the coefficients (rpe_bn_backward_coeffs_t); the second stream only combines
    // (rpe_conv1x1_wgrad_combine, with the forward's Gram buffer).  RPE_NO_Y3FREE=1: the round-3 dataflow; RPE_Y3_KEEP=1: the new
    // forward but y3 still written and the round-3 backward (A/B of the two halves); RPE_Y3FREE_MAX: widest planes handled this way.
    bool y3free = false;
    bool y3_keep = false;
    // dz3^T a2 as a side product of the NEXT block's fused conv1 data gradient (rpe_conv1x1_dgrad_bn_t: persistent over row tiles, the partial
    // in registers).  Built, bit-exact against the separate launch, and SLOWER in the step: 19.47-19.50 vs 19.16-19.18 ms (profiles/
    // r04_ab_t_fused.txt).  Per kernel: the fused launch streams at 2.2 TB/s where the plain one reaches 3.5-3.7 (251 VGPRs + 68 KB of LDS = two
    // workgroups per CU instead of three, and three more barriers per tile), 467 us against 272 + 146 us for layer1's blocks -- the side
    // product costs the HBM-bound epilogue more than the separate dz^T a2 launch and its re-read of dz.  OFF by default; RPE_T_FUSE=1 enables it.
    bool t_fused = false;
    bool apply_gram = true;      // bn2's apply pass and the Gram matrix of its output in ONE launch (rpe_bn_apply_gram; RPE_NO_APPLY_GRAM=1: two)
    int y3free_max = 128;
    void* gram_ws = nullptr;     // slab of the Gram launches (caller's stream)
    long gram_ws_bytes = 0;
    void* sk_ws = nullptr;               // split-K workspace of the inference forward (rpe_conv2d_fwd_affine_ws); 0 bytes when no layer splits
    long sk_ws_bytes = 0;
    rpe_pack_desc* pack_tab_fold = nullptr;  // ... with the BN scale folded into the forward copy (inference)
    int pack_state = 0;                  // what the forward copies hold: 0 unknown, 1 plain weights, 2 weights * BN scale (eval)
    long pack_total = 0;
    char* gspan_lo = nullptr;
    size_t gspan_bytes = 0;
    // optional per-category HIP-event timing (rpe_resnet50_profile)
    bool profiling = false;
    struct Span { int cat; hipEvent_t a, b; int name_id; double flops, bytes; };
    std::vector<std::string> kernel_names;   // distinct kernel symbols seen while profiling (rpe_last_kernel_name)
    double pending_flops = 0, pending_bytes = 0;  // algorithmic FLOPs / HBM bytes of the launch being bracketed
    std::vector<Span> spans;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    hipEvent_t cur_a = nullptr;   // start event of the span being recorded (PROF / prof_split)
    int cur_cat = 0;
    // weight-gradient GEMMs run on a second stream, overlapping the data-gradient / BN chain (they only feed Adam)
    hipStream_t side = nullptr;
    bool overlap = true;
    // how the second stream was chosen (ensure_side / rpe_resnet50_side_stream_info): candidates created, whether the one in use ran a
    // kernel WHILE a kernel of the caller's stream was executing, and the rejected candidates (kept until the engine goes: destroying
    // one would hand its hardware queue to the next stream created)
    int side_tries = 0;
    int side_concurrent = -1;    // -1 not probed (RPE_NO_SIDE_PROBE / capture), 0 no candidate overlapped, 1 yes
    std::vector<hipStream_t> side_rejects;
    bool capturing = false;              // the caller's stream is being captured into a hipGraph (capture_guard)
    // Walk direction of the big kernels on the caller's stream (common.h, xcd_remap_dir): alternating launch by launch in the training
    // step, so that every kernel meets the bytes its producer wrote last -- what is left of a > 256-MB tensor in the Infinity Cache --
    // first.  walk_next carries the direction across the staged backward's C calls.  RPE_NO_WALK_ALT=1: every kernel walks upwards.
    bool walk_alt = getenv("RPE_NO_WALK_ALT") == nullptr;
    int walk_next = 0;
    std::vector<hipEvent_t> sync_pool;
    size_t sync_next = 0;
    double flops[RPE_PROF_NUM] = {0};   // algorithmic FLOPs per pass, per category
    double bytes[RPE_PROF_NUM] = {0};   // algorithmic bytes per pass, per category
};

extern "C" const char* rpe_last_kernel_name(void);
static int kernel_id(rpe_resnet50* e) {
    const char* n = rpe_last_kernel_name();
    for (size_t i = 0; i < e->kernel_names.size(); ++i)
        if (e->kernel_names[i] == n) return (int)i;
    e->kernel_names.push_back(n);
    return (int)e->kernel_names.size() - 1;
}

static hipEvent_t next_event(rpe_resnet50* e) {
    if (e->ev_next == e->ev_pool.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        e->ev_pool.push_back(ev);
    }
    return e->ev_pool[e->ev_next++];
}

// runs `call` and, when profiling, brackets it with events on the launch stream.  An entry point that launches several kernels
// splits its span per kernel (prof_split, common.h): the hook closes the running span under the symbol noted so far -- the first
// span carries the call's algorithmic FLOPs / bytes -- and opens the next at the same event.
static void prof_close(rpe_resnet50* e, hipStream_t s, bool reopen) {
    hipEvent_t b = next_event(e);
    if (!e->cur_a || !b) { e->cur_a = nullptr; return; }
    (void)hipEventRecord(b, s);
    e->spans.push_back({e->cur_cat, e->cur_a, b, kernel_id(e), e->pending_flops, e->pending_bytes});
    e->pending_flops = 0; e->pending_bytes = 0;
    e->cur_a = reopen ? b : nullptr;
}
static void prof_hook_split(void* ctx, hipStream_t s) { prof_close((rpe_resnet50*)ctx, s, true); }
#define PROF(e, cat, stream, call)                                                   \
    do {                                                                             \
        if ((e)->profiling) { (e)->cur_a = next_event(e); (e)->cur_cat = (cat);      \
            if ((e)->cur_a) (void)hipEventRecord((e)->cur_a, (hipStream_t)(stream)); \
            rpe::g_prof_hook = {prof_hook_split, (e)}; }                             \
        const int err__ = (call);                                                    \
        rpe::g_prof_hook = {nullptr, nullptr};                                       \
        if (err__) return err__;                                                     \
        if ((e)->profiling) prof_close((e), (hipStream_t)(stream), false);           \
    } while (0)

// walk mode of this thread's launches for the lifetime of the object (WalkScope(e, true): the engine's alternating direction, resumed
// where the last scope left it; WalkScope(e, false): upwards -- the second stream's launches), the previous mode restored afterwards
struct WalkScope {
    rpe_resnet50* e; bool alt; int mode0, next0;
    WalkScope(rpe_resnet50* e_, bool alt_) : e(e_), alt(alt_ && e_->walk_alt), mode0(rpe::g_walk_mode), next0(rpe::g_walk_next) {
        rpe::g_walk_mode = alt ? 2 : 0;
        if (alt) rpe::g_walk_next = e->walk_next;
    }
    ~WalkScope() {
        if (alt) e->walk_next = rpe::g_walk_next;
        rpe::g_walk_mode = mode0; rpe::g_walk_next = next0;
    }
};

static int add_conv(rpe_resnet50* e, const std::string& name, const std::string& bn, int in_h, int in_w, int in_c, int out_c, int k,
                    int stride, int pad) {
    ConvL c;
    c.name = name; c.bn = bn;
    c.d = rpe_conv_desc{e->B, in_h, in_w, in_c, out_c, k, k, stride, pad};
    c.Ho = (in_h + 2 * pad - k) / stride + 1;
    c.Wo = (in_w + 2 * pad - k) / stride + 1;
    c.rows = (long)e->B * c.Ho * c.Wo;
    c.bn_i = (int)e->convs.size();
    c.p_w = (int)e->pnames.size();
    e->pnames.push_back(name + ".weight"); e->pnumel.push_back((long)out_c * in_c * k * k);
    c.p_g = (int)e->pnames.size();
    e->pnames.push_back(bn + ".weight"); e->pnumel.push_back(out_c);
    c.p_b = (int)e->pnames.size();
    e->pnames.push_back(bn + ".bias"); e->pnumel.push_back(out_c);
    e->convs.push_back(c);
    return (int)e->convs.size() - 1;
}

static void want(rpe_resnet50* e, void** dst, long bytes) {
    bytes = (bytes + 255) / 256 * 256;
    e->slots.push_back({dst, bytes});
    e->ws_bytes += bytes;
}

extern "C" int rpe_resnet_create(rpe_resnet50_t** out, int depth, int batch, int height, int width, int dtype, int latent_dim);
extern "C" int rpe_resnet50_create(rpe_resnet50_t** out, int batch, int height, int width, int dtype, int latent_dim) {
    return rpe_resnet_create(out, 50, batch, height, width, dtype, latent_dim);
}

// depth: 50, 101 or 152 -- the bottleneck members of the family util/model_utils.py:130-136 offers -- or 18 / 34, its BasicBlock members
// (the reference's option set reaches 18; the same plan covers 34).  The BasicBlock plan is built from the same launches as the
// bottleneck plan's general path (conv + statistics, finalize, apply; fused data gradient + BatchNorm reduction, dz, y -> dy, weight
// gradient on the second stream); the bottleneck-only dataflow changes (folded conv3 backward, y3-free blocks) do not apply to it.
extern "C" int rpe_resnet_create(rpe_resnet50_t** out, int depth, int batch, int height, int width, int dtype, int latent_dim) {
    if (!out) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_create: null out");
    if (depth != 18 && depth != 34 && depth != 50 && depth != 101 && depth != 152)
        return rpe_set_error(RPE_ERR_SHAPE, "resnet_create: depth must be 18, 34 (BasicBlock) or 50, 101, 152 (bottleneck)");
    if (batch <= 0 || latent_dim <= 0) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_create: bad batch/latent");
    if (height < 32 || width < 32 || (height % 32) || (width % 32)) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_create: H, W must be multiples of 32");
    if (dtype != RPE_F32 && dtype != RPE_BF16 && dtype != RPE_F16) return rpe_set_error(RPE_ERR_DTYPE, "resnet50_create: dtype must be RPE_F32, RPE_BF16 or RPE_F16");
    rpe_resnet50* e = new rpe_resnet50();
    e->B = batch; e->H = height; e->W = width; e->dtype = dtype; e->latent = latent_dim;
    e->esz = dtype == RPE_F32 ? 4 : 2;
    e->basic = depth == 18 || depth == 34;
    e->feat = e->basic ? 512 : 2048;
    add_conv(e, "conv1", "bn1", height, width, 3, 64, 7, 2, 3);
    int h = e->convs[0].Ho / 2, w = e->convs[0].Wo / 2;  // after maxpool 3x3/2 pad 1 (even sizes)
    int inpl = 64;
    const int planes[4] = {64, 128, 256, 512}, strides[4] = {1, 2, 2, 2};
    const int nblk18[4] = {2, 2, 2, 2};
    const int nblk50[4] = {3, depth == 152 ? 8 : 4, (depth == 50 || depth == 34) ? 6 : (depth == 101 ? 23 : 36), 3};
    const int* nblk = depth == 18 ? nblk18 : nblk50;
    for (int li = 0; li < 4; ++li) {
        for (int b = 0; b < nblk[li]; ++b) {
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const int s = b == 0 ? strides[li] : 1;
            Block blk;
            blk.layer = li + 1; blk.first = b == 0;
            if (e->basic) {
                blk.c1 = add_conv(e, p + ".conv1", p + ".bn1", h, w, inpl, planes[li], 3, s, 1);
                const int h2 = e->convs[blk.c1].Ho, w2 = e->convs[blk.c1].Wo;
                blk.c2 = add_conv(e, p + ".conv2", p + ".bn2", h2, w2, planes[li], planes[li], 3, 1, 1);
                blk.c3 = -1; blk.cd = -1; blk.out = blk.c2;
                if (b == 0 && (s != 1 || inpl != planes[li])) blk.cd = add_conv(e, p + ".downsample.0", p + ".downsample.1", h, w, inpl, planes[li], 1, s, 0);
                e->blocks.push_back(blk);
                inpl = planes[li];
                h = h2; w = w2;
                continue;
            }
            blk.c1 = add_conv(e, p + ".conv1", p + ".bn1", h, w, inpl, planes[li], 1, 1, 0);
            blk.c2 = add_conv(e, p + ".conv2", p + ".bn2", h, w, planes[li], planes[li], 3, s, 1);
            const int h2 = e->convs[blk.c2].Ho, w2 = e->convs[blk.c2].Wo;
            blk.c3 = add_conv(e, p + ".conv3", p + ".bn3", h2, w2, planes[li], planes[li] * 4, 1, 1, 0);
            blk.cd = -1; blk.out = blk.c3;
            if (b == 0) blk.cd = add_conv(e, p + ".downsample.0", p + ".downsample.1", h, w, inpl, planes[li] * 4, 1, s, 0);
            e->blocks.push_back(blk);
            inpl = planes[li] * 4;
            h = h2; w = w2;
        }
    }
    e->pnames.push_back("fc.weight"); e->pnumel.push_back((long)latent_dim * e->feat);
    e->pnames.push_back("fc.bias"); e->pnumel.push_back(latent_dim);
    e->latent_pad = (latent_dim + 3) / 4 * 4;

    // ---- workspace plan ----
    const size_t es = e->esz;
    want(e, &e->x4, rpe_x4_bytes(dtype, batch, height, width));   // zero-bordered NHWC4 image (RPE_STEM_PAD)
    long max_act = 0;
    for (auto& c : e->convs) {
        const long n = c.rows * c.d.out_c;
        if (n > max_act) max_act = n;
        want(e, &c.y, n * es);
        want(e, &c.a, n * es);
        want(e, &c.dy, n * es);
        const long wn = (long)c.d.out_c * c.d.kh * c.d.kw * c.d.in_c;
        if (&c == &e->convs[0]) {
            want(e, &c.wf, 64L * 256 * es);
        } else {
            want(e, &c.wf, wn * es);   // (fp32 training reads the masters in place; the copy holds the BN-folded inference weights)
            want(e, &c.wd, wn * es);
        }
        want(e, (void**)&c.scale, c.d.out_c * 4L);
        want(e, (void**)&c.shift, c.d.out_c * 4L);
        want(e, (void**)&c.mean, c.d.out_c * 4L);
        want(e, (void**)&c.invstd, c.d.out_c * 4L);
        want(e, (void**)&c.c1c2, 2L * c.d.out_c * 4);
        const long sf = (rpe_conv2d_fwd_stats_tiles(&c.d, dtype) + 2) * 2 * c.d.out_c;
        if (sf > e->stats_floats) e->stats_floats = sf;
        const long sf2 = (rpe_conv2d_dgrad_stats_tiles(&c.d, dtype) + 4) * 2 * c.d.in_c;  // fused dgrad partials (parity classes round up)
        if (sf2 > e->stats_floats) e->stats_floats = sf2;
    }
    const ConvL& st = e->convs[0];
    const long pool_n = (long)batch * (st.Ho / 2) * (st.Wo / 2) * 64;
    want(e, &e->pool, pool_n * es);
    want(e, (void**)&e->pool_idx, pool_n);
    want(e, (void**)&e->pooled, (long)batch * e->feat * 4);
    want(e, (void**)&e->d_pooled, (long)batch * e->feat * 4);
    want(e, (void**)&e->fc_wt, (long)e->feat * e->latent_pad * 4);
    want(e, &e->early_grad, st.rows * 64 * es);
    for (int i = 0; i < 2; ++i) want(e, &e->G[i], max_act * es);
    for (auto& b : e->blocks) {
        const ConvL& c3 = e->convs[b.out];
        want(e, &b.dz, c3.rows * c3.d.out_c * es);
        if (dtype != RPE_F32) want(e, (void**)&b.relu_mask, c3.rows * c3.d.out_c / 8);
    }
    want(e, &e->d_pool, (long)batch * (e->convs[0].Ho / 2) * (e->convs[0].Wo / 2) * 64 * es);
    want(e, (void**)&e->stats_part, e->stats_floats * 4);
    want(e, (void**)&e->stats_part2, e->stats_floats * 4);
    e->bwd_part_floats = 1024L * 2 * 2048;
    want(e, (void**)&e->bwd_part, e->bwd_part_floats * 4);
    want(e, (void**)&e->c1c2, 2 * 2048 * 4L);
    want(e, (void**)&e->dpart, RPE_BN_DPART_DOUBLES(2048) * 8);
    want(e, (void**)&e->dpart2, RPE_BN_DPART_DOUBLES(2048) * 8);
    want(e, (void**)&e->stem_dw, 64L * 256 * 4);
    e->fold = !e->basic && getenv("RPE_NO_BN_FOLD") == nullptr;   // (the folds below are forms of the bottleneck's 1x1 convs)
    if (e->fold) {
        long wk = 0;
        for (auto& b : e->blocks) {
            const rpe_conv_desc& d = e->convs[b.c3].d;
            const long sb = rpe_bn_bwd_fold_scratch_bytes(dtype, d.out_c, d.in_c);
            if (sb > e->fold_scratch_bytes) e->fold_scratch_bytes = sb;
            const long w = (long)d.in_c * (d.out_c + d.in_c) * (long)es;
            if (w > wk) wk = w;
            const rpe_conv_desc& d1 = e->convs[b.c1].d;      // y-form fold of conv1: w_kcat [in_c][2 out_c]
            const long w1 = (long)d1.in_c * 2 * d1.out_c * (long)es;
            if (w1 > wk) wk = w1;
        }
        e->fold1 = getenv("RPE_BN1_FOLD") != nullptr;
        if (getenv("RPE_BN1_FOLD_MAX")) e->fold1_max = atoi(getenv("RPE_BN1_FOLD_MAX"));
        e->fold_w = getenv("RPE_NO_WGRAD_FOLD") == nullptr;
        if (e->fold_w) {
            if (getenv("RPE_WGRAD_FOLD_MAX")) e->fold_w_max = atoi(getenv("RPE_WGRAD_FOLD_MAX"));
            for (auto& b : e->blocks) {
                if (e->convs[b.c3].d.in_c > e->fold_w_max) continue;   // (default: layers 1-3)
                const long sb = rpe_conv1x1_wgrad_folded_scratch_bytes(&e->convs[b.c3].d, dtype);
                if (sb > e->wfold_scratch_bytes) e->wfold_scratch_bytes = sb;
            }
            if (e->fold1)
                for (auto& b : e->blocks) {
                    if (e->convs[b.c1].d.out_c > e->fold1_max) continue;
                    const long sb = rpe_conv1x1_wgrad_folded_y_scratch_bytes(&e->convs[b.c1].d, dtype);
                    if (sb > e->wfold_scratch_bytes) e->wfold_scratch_bytes = sb;
                }
            if (e->wfold_scratch_bytes > 0) want(e, &e->wfold_scratch, e->wfold_scratch_bytes);
        }
        want(e, &e->w_kcat, wk);
        want(e, (void**)&e->fold_bias, 2048L * 4);
        want(e, &e->fold_scratch, e->fold_scratch_bytes);
    }
    e->y3free = dtype != RPE_F32 && e->fold && e->fold_w && !e->fold1 && !getenv("RPE_NO_Y3FREE") && !getenv("RPE_NO_RELU_MASK") &&
                !getenv("RPE_WGRAD_ATOMIC");
    long y3_slab = 0;
    if (e->y3free) {
        if (getenv("RPE_Y3FREE_MAX")) e->y3free_max = atoi(getenv("RPE_Y3FREE_MAX"));
        e->y3_keep = getenv("RPE_Y3_KEEP") != nullptr;
        e->apply_gram = getenv("RPE_NO_APPLY_GRAM") == nullptr;
        e->t_fused = getenv("RPE_T_FUSE") != nullptr;
        for (auto& b : e->blocks) {
            const ConvL& c3 = e->convs[b.c3];
            if (c3.d.in_c > e->y3free_max || c3.d.in_c > 256 || (c3.d.in_c % 64)) continue;
            want(e, (void**)&b.gram, (long)(rpe_gram_ones_row(c3.d.in_c) + 1) * c3.d.in_c * 4);
            want(e, (void**)&b.dzt_a, (long)c3.d.out_c * c3.d.in_c * 4);
            const long wsb = rpe_gram_workspace_bytes(dtype, c3.rows, c3.d.in_c);
            if (wsb > e->gram_ws_bytes) e->gram_ws_bytes = wsb;
            const long wsb2 = rpe_bn_apply_gram_workspace_bytes(dtype, c3.rows, c3.d.in_c);   // (-1: not a shape of the fused form)
            if (wsb2 > e->gram_ws_bytes) e->gram_ws_bytes = wsb2;
            const long tb = rpe_conv2d_wgrad_workspace_bytes(&c3.d, dtype);   // dz3^T a2 runs on the caller's stream: its slab
            if (tb > y3_slab) y3_slab = tb;
            // ... or rides on the next block's fused conv1 data gradient, whose row space and columns are this block's output
            rpe_conv_desc dn = c3.d; dn.in_c = c3.d.out_c; dn.out_c = c3.d.in_c;
            const long tb2 = rpe_conv1x1_dgrad_bn_t_workspace_bytes(&dn, c3.d.in_c);
            if (tb2 > y3_slab) y3_slab = tb2;
        }
        if (e->gram_ws_bytes > 0) want(e, &e->gram_ws, e->gram_ws_bytes);
    }
    if (!getenv("RPE_WGRAD_ATOMIC")) {
        for (size_t i = 1; i < e->convs.size(); ++i) {
            const long b = rpe_conv2d_wgrad_workspace_bytes(&e->convs[i].d, dtype);
            if (b > e->wg_slab_bytes) e->wg_slab_bytes = b;
        }
        if (e->wg_slab_bytes > 0) want(e, &e->wg_slab, e->wg_slab_bytes);
        e->main_slab_bytes = rpe_stem_conv_wgrad_workspace_bytes(dtype, batch, height, width);
        const long fcb = rpe_linear_wgrad_workspace_bytes(RPE_F32, batch, latent_dim, e->feat);
        if (fcb > e->main_slab_bytes) e->main_slab_bytes = fcb;
        if (y3_slab > e->main_slab_bytes) e->main_slab_bytes = y3_slab;
        if (e->main_slab_bytes > 0) want(e, &e->main_slab, e->main_slab_bytes);
    }
    {
        const long f = rpe_linear_fwd_workspace_bytes(RPE_F32, batch, latent_dim, e->feat), d = rpe_linear_fwd_workspace_bytes(RPE_F32, batch, e->feat, e->latent_pad);
        e->fc_ws_bytes = f > d ? f : d;
        if (e->fc_ws_bytes > 0 && getenv("RPE_NO_LINEAR_SPLITK") == nullptr) want(e, &e->fc_ws, e->fc_ws_bytes);
    }
    // inference forward of few-row layers (rollout frames): split-K partial tiles
    if (getenv("RPE_NO_SPLITK") == nullptr) {
        for (size_t i = 1; i < e->convs.size(); ++i) {
            const long sb = rpe_conv2d_fwd_affine_workspace_bytes(&e->convs[i].d, dtype);
            if (sb > e->sk_ws_bytes) e->sk_ws_bytes = sb;
        }
        if (e->sk_ws_bytes > 0) want(e, &e->sk_ws, e->sk_ws_bytes);
    }
    want(e, (void**)&e->pack_tab, (long)(e->convs.size() + 8) * sizeof(rpe_pack_desc));
    want(e, (void**)&e->pack_tab_fold, (long)(e->convs.size() + 8) * sizeof(rpe_pack_desc));
    for (auto& c : e->convs) {
        const double mnk = 2.0 * (double)c.rows * c.d.out_c * (double)(c.d.kh * c.d.kw * c.d.in_c);
        const double in_b = (double)batch * c.d.in_h * c.d.in_w * c.d.in_c * es, out_b = (double)c.rows * c.d.out_c * es;
        e->flops[RPE_PROF_CONV_FWD] += mnk;   e->bytes[RPE_PROF_CONV_FWD] += in_b + out_b;
        e->flops[RPE_PROF_CONV_WGRAD] += mnk; e->bytes[RPE_PROF_CONV_WGRAD] += in_b + out_b;
        if (&c != &e->convs[0]) { e->flops[RPE_PROF_CONV_DGRAD] += mnk; e->bytes[RPE_PROF_CONV_DGRAD] += in_b + out_b; }
        e->bytes[RPE_PROF_BN_FWD] += 2 * out_b;   // read y, write a (+ residual read on block outputs, not counted)
        e->bytes[RPE_PROF_BN_BWD] += 3 * out_b;   // fused form: dz, y -> dy (the reduction rides on the dgrad epilogue)
    }
    *out = e;
    return 0;
}

extern "C" int rpe_resnet50_profile(rpe_resnet50_t* e, int enable) {
    if (!e) return rpe_set_error(RPE_ERR_STATE, "resnet50_profile: null engine");
    e->profiling = enable != 0;
    e->spans.clear();
    e->ev_next = 0;
    return 0;
}

// Sum of HIP-event elapsed time (ms) and number of bracketed launches per category since the last
// rpe_resnet50_profile(e, 1); waits for the recorded work to finish.  flops/bytes: algorithmic work of ONE pass.
extern "C" int rpe_resnet50_profile_read(rpe_resnet50_t* e, float* ms, int* launches, double* flops, double* bytes) {
    if (!e) return rpe_set_error(RPE_ERR_STATE, "resnet50_profile_read: null engine");
    for (int i = 0; i < RPE_PROF_NUM; ++i) { ms[i] = 0.f; launches[i] = 0; flops[i] = e->flops[i]; bytes[i] = e->bytes[i]; }
    for (auto& sp : e->spans) {
        if (hipError_t he = hipEventSynchronize(sp.b)) return rpe_set_error_hip(he, __FILE__, __LINE__);
        float t = 0.f;
        if (hipError_t he = hipEventElapsedTime(&t, sp.a, sp.b)) return rpe_set_error_hip(he, __FILE__, __LINE__);
        ms[sp.cat] += t;
        launches[sp.cat] += 1;
    }
    return 0;
}

// Per kernel SYMBOL (the names rocprofv3 lists, in the short form of rpe_last_kernel_name): launches, summed HIP-event
// time and summed algorithmic FLOPs since rpe_resnet50_profile(e, 1).  Text lines "name;launches;ms;flops;bytes\n".
extern "C" long rpe_resnet50_profile_kernels(rpe_resnet50_t* e, char* buf, long buflen) {
    if (!e || !buf || buflen <= 0) return -1;
    const size_t nk = e->kernel_names.size();
    std::vector<double> ms(nk, 0.0), fl(nk, 0.0), by(nk, 0.0);
    std::vector<int> cnt(nk, 0);
    for (auto& sp : e->spans) {
        if (sp.name_id < 0 || (size_t)sp.name_id >= nk) continue;
        if (hipEventSynchronize(sp.b) != hipSuccess) return -1;
        float t = 0.f;
        if (hipEventElapsedTime(&t, sp.a, sp.b) != hipSuccess) return -1;
        ms[sp.name_id] += t; fl[sp.name_id] += sp.flops; by[sp.name_id] += sp.bytes; cnt[sp.name_id] += 1;
    }
    long off = 0;
    for (size_t i = 0; i < nk; ++i) {
        if (!cnt[i]) continue;
        const int w = snprintf(buf + off, (size_t)(buflen - off), "%s;%d;%.6f;%.0f;%.0f\n", e->kernel_names[i].c_str(), cnt[i], ms[i], fl[i], by[i]);
        if (w < 0 || off + w >= buflen) break;
        off += w;
    }
    return off;
}

extern "C" void rpe_resnet50_destroy(rpe_resnet50_t* e) {
    if (!e) return;
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    for (auto ev : e->sync_pool) (void)hipEventDestroy(ev);
    if (e->side) (void)hipStreamDestroy(e->side);
    for (auto st : e->side_rejects) (void)hipStreamDestroy(st);
    delete e;
}
extern "C" long rpe_resnet50_workspace_bytes(const rpe_resnet50_t* e) { return e ? e->ws_bytes : 0; }
extern "C" const char* rpe_resnet50_param_name(const rpe_resnet50_t* e, int i) {
    return (e && i >= 0 && i < (int)e->pnames.size()) ? e->pnames[i].c_str() : nullptr;
}
extern "C" long rpe_resnet50_param_numel(const rpe_resnet50_t* e, int i) {
    return (e && i >= 0 && i < (int)e->pnumel.size()) ? e->pnumel[i] : -1;
}

extern "C" int rpe_resnet50_bind(rpe_resnet50_t* e, void* workspace, long workspace_bytes, float* const* params_host, float* const* grads_host,
                                 float* const* running_host, long long* const* num_batches_host) {
    if (!e || !workspace || !params_host) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_bind: null argument");
    if (workspace_bytes < e->ws_bytes) return rpe_set_error(RPE_ERR_WORKSPACE, "resnet50_bind: workspace smaller than rpe_resnet50_workspace_bytes()");
    if (((uintptr_t)workspace) & 255) return rpe_set_error(RPE_ERR_ALIGN, "resnet50_bind: workspace must be 256-byte aligned");
    e->ws = (char*)workspace;
    char* p = e->ws;
    for (auto& s : e->slots) { *s.dst = p; p += s.bytes; }
    const int np = (int)e->pnames.size(), nb = (int)e->convs.size();
    e->params.assign(params_host, params_host + np);
    if (grads_host) e->grads.assign(grads_host, grads_host + np); else e->grads.assign(np, nullptr);
    if (running_host) e->running.assign(running_host, running_host + 2 * nb); else e->running.assign(2 * nb, nullptr);
    if (num_batches_host) e->nbt.assign(num_batches_host, num_batches_host + nb); else e->nbt.assign(nb, nullptr);
    for (int i = 0; i < np; ++i)
        if (!e->params[i] || (((uintptr_t)e->params[i]) & 15)) return rpe_set_error(RPE_ERR_ALIGN, "resnet50_bind: parameter pointers must be non-null and 16-byte aligned");
    // debugging table
    e->named.clear();
    for (auto& c : e->convs) {
        e->named.push_back({c.name + ".y", c.y, c.rows, c.d.out_c});
        e->named.push_back({c.name + ".a", c.a, c.rows, c.d.out_c});
    }
    e->named.push_back({"pool", e->pool, (long)e->B * (e->convs[0].Ho / 2) * (e->convs[0].Wo / 2), 64});
    e->named.push_back({"x4", e->x4, (long)e->B * (e->H + 2 * RPE_STEM_PAD) * (e->W + 2 * RPE_STEM_PAD), 4});
    for (int i = 0; i < 2; ++i) e->named.push_back({"G" + std::to_string(i), e->G[i], 0, 0});
    {   // descriptor table of the per-step weight packing (bind is a setup call: one small synchronous upload)
        std::vector<rpe_pack_desc> tab;
        long start = 0;
        for (size_t i = 1; i < e->convs.size(); ++i) {
            ConvL& c = e->convs[i];
            rpe_pack_desc d;
            d.src = e->params[c.p_w];
            d.wf = e->dtype == RPE_F32 ? nullptr : c.wf;
            d.wd = c.wd;
            d.Co = c.d.out_c; d.RS = c.d.kh * c.d.kw; d.Ci = c.d.in_c; d.pad_ = 0;
            d.scale = nullptr;
            d.start = start;
            start += (long)d.Co * d.RS * d.Ci;
            tab.push_back(d);
        }
        e->pack_total = start;
        if (hipError_t he = hipMemcpy(e->pack_tab, tab.data(), tab.size() * sizeof(rpe_pack_desc), hipMemcpyHostToDevice))
            return rpe_set_error_hip(he, __FILE__, __LINE__);
        for (size_t i = 1; i < e->convs.size(); ++i) {   // inference table: forward copy only, scaled by the layer's BN scale
            ConvL& c = e->convs[i];
            tab[i - 1].wf = c.wf;
            tab[i - 1].wd = nullptr;
            tab[i - 1].scale = c.scale;
        }
        if (hipError_t he = hipMemcpy(e->pack_tab_fold, tab.data(), tab.size() * sizeof(rpe_pack_desc), hipMemcpyHostToDevice))
            return rpe_set_error_hip(he, __FILE__, __LINE__);
        e->pack_state = 0;
        // the staged image's zero border (the staging kernels only ever write its interior)
        if (hipError_t he = hipMemset(e->x4, 0, (size_t)rpe_x4_bytes(e->dtype, e->B, e->H, e->W))) return rpe_set_error_hip(he, __FILE__, __LINE__);
        // arrival counters of the fused BN reduce+finalize launches start at zero (and are left at zero by every launch)
        if (hipError_t he = hipMemset(e->dpart, 0, 64 * sizeof(double))) return rpe_set_error_hip(he, __FILE__, __LINE__);
        if (hipError_t he = hipMemset(e->dpart2, 0, 64 * sizeof(double))) return rpe_set_error_hip(he, __FILE__, __LINE__);
    }
    e->gspan_lo = nullptr; e->gspan_bytes = 0;
    if (grads_host) {
        char *lo = nullptr, *hi = nullptr;
        size_t sum = 0;
        bool ok = true;
        for (int i = 0; i < np; ++i) {
            if (!e->grads[i]) { ok = false; break; }
            char* a = (char*)e->grads[i];
            char* b = a + (size_t)e->pnumel[i] * 4;
            if (!lo || a < lo) lo = a;
            if (!hi || b > hi) hi = b;
            sum += (size_t)e->pnumel[i] * 4;
        }
        // contiguous up to the arena's 16-byte segment padding
        if (ok && (size_t)(hi - lo) <= sum + (size_t)np * 16) { e->gspan_lo = lo; e->gspan_bytes = (size_t)(hi - lo); }
    }
    e->bound = true;
    e->fwd_done = false;
    return 0;
}

#define TRY(x) do { if (int err__ = (x)) return err__; } while (0)
#define HIPTRY(x) do { hipError_t he__ = (x); if (he__ != hipSuccess) return rpe_set_error_hip(he__, __FILE__, __LINE__); } while (0)

// what a failed sync_event() returns to the caller: RPE_ERR_STATE (message already set) under capture, else the HIP failure
static int event_error(const rpe_resnet50* e) {
    return e->capturing ? RPE_ERR_STATE : rpe_set_error(RPE_ERR_HIP, "trunk engine: hipEventCreate failed");
}

static hipEvent_t sync_event(rpe_resnet50* e) {
    if (e->sync_next == e->sync_pool.size()) {
        if (e->capturing) { rpe_set_error(RPE_ERR_STATE, "trunk engine: the cross-stream event pool would grow inside a stream capture (warm up eagerly with the same schedule first)"); return nullptr; }
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return nullptr;
        e->sync_pool.push_back(ev);
    }
    return e->sync_pool[e->sync_next++];
}


extern "C" int rpe_resnet50_pack_weights(rpe_resnet50_t* e, void* stream) {
    if (!e || !e->bound) return rpe_set_error(RPE_ERR_STATE, "resnet50_pack_weights: engine not bound");
    PROF(e, RPE_PROF_OTHER, stream, rpe_pack_stem_weight(e->dtype, e->params[e->convs[0].p_w], nullptr, e->convs[0].wf, stream));
    PROF(e, RPE_PROF_OTHER, stream, rpe_pack_conv_weights_multi(e->dtype, e->pack_tab, (int)e->convs.size() - 1, e->pack_total, stream));
    e->pack_state = 1;
    const int np = (int)e->pnames.size();
    TRY(rpe_transpose_f32(e->params[np - 2], e->fc_wt, e->latent, e->feat, e->feat, e->latent_pad, stream));
    return 0;
}

extern "C" int rpe_resnet50_weights_changed(rpe_resnet50_t* e) {
    if (!e) return rpe_set_error(RPE_ERR_STATE, "resnet50_weights_changed: null engine");
    e->pack_state = 0;
    return 0;
}

// algorithmic HBM bytes: every operand tensor read or written exactly once (weights amortised over the batch)
static double conv_in_bytes(const rpe_resnet50* e, const ConvL& c) { return (double)c.d.batch * c.d.in_h * c.d.in_w * c.d.in_c * e->esz; }
static double conv_out_bytes(const rpe_resnet50* e, const ConvL& c) { return (double)c.rows * c.d.out_c * e->esz; }
static double conv_flops(const ConvL& c) { return 2.0 * (double)c.rows * c.d.out_c * (double)(c.d.kh * c.d.kw * c.d.in_c); }

static const void* fwd_weight(rpe_resnet50* e, ConvL& c) {
    return (e->dtype == RPE_F32 && &c != &e->convs[0] && e->train_mode) ? (const void*)e->params[c.p_w] : c.wf;
}

// Inference: every BN is an affine map of fixed running statistics -> scale into the packed forward weights (once, until the
// weights or the mode change), shift + residual + ReLU into the conv epilogue: one launch per conv instead of three.
static int fold_for_eval(rpe_resnet50* e, void* stream) {
    for (auto& c : e->convs) {
        float* rm = e->running[2 * c.bn_i];
        float* rv = e->running[2 * c.bn_i + 1];
        if (!rm || !rv) return rpe_set_error(RPE_ERR_STATE, "resnet50_forward: eval mode needs running statistics");
        TRY(rpe_bn_eval_affine(c.d.out_c, e->params[c.p_g], e->params[c.p_b], rm, rv, 1e-5f, c.scale, c.shift, stream));
    }
    TRY(rpe_pack_stem_weight(e->dtype, e->params[e->convs[0].p_w], e->stem_raw ? nullptr : e->convs[0].scale, e->convs[0].wf, stream));
    TRY(rpe_pack_conv_weights_multi(e->dtype, e->pack_tab_fold, (int)e->convs.size() - 1, e->pack_total, stream));
    e->pack_state = 2;
    return 0;
}

// ---- which hardware queue the second stream lands on ---------------------------------------------------------------------------
// HIP multiplexes a process's streams onto at most GPU_MAX_HW_QUEUES (4) hardware queues PER PRIORITY LEVEL, in creation order: a new
// queue while that level's pool has fewer than four, then the least-referenced existing one; the hardware queues are dealt to the
// command processor's pipes round-robin, again in creation order.  Round 3's two findings are the two ways this can go wrong for a
// stream that forks from / joins the caller's:
//   (1) a LOW-priority queue that is the 5th, 9th .. hardware queue of the process sits on the pipe of the caller's queue, which
//       always has a packet ready (the host runs ahead): it is never scheduled -- 28 ms/step for every RPE_TEST_STREAM_SKIP >= 3 and
//       only for those (profiles/r03_ab_stream_priority.txt: three extra normal-priority queues + the caller's fill the first round);
//   (2) a stream that SHARES a hardware queue with the stream it waits on (the pool was full: the 5th .. stream of its level) cannot
//       have its cross-stream waits resolved by barrier packets inside one in-order queue: the runtime resolves them on the host
//       (hipGraphLaunch 2.6 ms, 3-4 ms frames: profiles/r03_rollout_latency.txt) or the two streams simply serialise (21.5 ms/step at
//       RPE_TEST_STREAM_SKIP = 6, normal priority).
// So the engine does not trust the position it is created at: every candidate is PROBED once -- a spin kernel of ~200 us on the
// caller's stream, an empty kernel on the candidate, and the question whether the candidate's kernel finished while the spin was
// still running -- and the first candidate that overlaps is kept (up to four: one full round of the pool).  Normal priority (finding 1).
extern char** environ;
static bool profiler_attached() {
    const char* pre = getenv("LD_PRELOAD");
    if (pre && (strstr(pre, "rocprof") || strstr(pre, "rocprofiler"))) return true;
    for (char** e = environ; e && *e; ++e)
        if (!strncmp(*e, "ROCPROF", 7) || !strncmp(*e, "ROCP_TOOL", 9)) return true;
    return false;
}
__global__ void side_probe_spin_kernel(long ticks) {
    const long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
__global__ void side_probe_empty_kernel() {}
// 1: a kernel on `cand` completed while a kernel on `caller` was still executing; 0: it did not; -1: could not tell
static int side_probe(hipStream_t caller, hipStream_t cand) {
    hipEvent_t spin_done = nullptr, cand_done = nullptr;
    if (hipEventCreateWithFlags(&spin_done, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&cand_done, hipEventDisableTiming) != hipSuccess) return -1;
    int res = -1;
    hipLaunchKernelGGL(side_probe_spin_kernel, dim3(1), dim3(64), 0, caller, 20000L);   // wall_clock64 ticks at 100 MHz: 200 us
    if (hipEventRecord(spin_done, caller) == hipSuccess) {
        hipLaunchKernelGGL(side_probe_empty_kernel, dim3(1), dim3(64), 0, cand);
        if (hipEventRecord(cand_done, cand) == hipSuccess && hipEventSynchronize(cand_done) == hipSuccess) {
            const hipError_t q = hipEventQuery(spin_done);
            res = q == hipErrorNotReady ? 1 : (q == hipSuccess ? 0 : -1);
        }
    }
    (void)hipEventSynchronize(spin_done);
    (void)hipGetLastError();
    (void)hipEventDestroy(spin_done);
    (void)hipEventDestroy(cand_done);
    return res;
}

// conv -> batch statistics -> BN apply (+residual) (+relu)
// the second HIP stream (weight gradients in the backward, the projection-shortcut branch in the forward), created on first use
static int ensure_side(rpe_resnet50* e, hipStream_t caller = nullptr) {
    if (e->overlap && !e->side) {
        if (getenv("RPE_NO_OVERLAP")) e->overlap = false;
        else {
            // NORMAL dispatch priority.  Round 2 gave the second stream the LOWEST priority (weight gradients are off the critical path:
            // 20.86 vs 20.98 ms/step then).  Round 3 found that fragile: streams are dealt to a few hardware queues in creation order, and
            // a LOW-priority stream created as the 4th .. 8th stream of the process (three or more streams made before it by the host
            // framework, a communication library, a data loader) is starved outright -- 28.1-28.8 ms/step instead of 19.6 --
            // while a normal-priority stream runs 19.53-19.58 ms/step
            // wherever it lands (profiles/r03_ab_stream_priority.txt).  RPE_SIDE_LOW_PRIO=1 restores the round-2 choice.
            int least = 0, greatest = 0;
            HIPTRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
            static const bool low = getenv("RPE_SIDE_LOW_PRIO") != nullptr;
            // RPE_TEST_STREAM_SKIP=n: n streams created first, as another component of the host process might (A/B of the above)
            const int skip = getenv("RPE_TEST_STREAM_SKIP") ? atoi(getenv("RPE_TEST_STREAM_SKIP")) : 0;
            for (int i = 0; i < skip; ++i) { hipStream_t d; HIPTRY(hipStreamCreateWithFlags(&d, hipStreamNonBlocking)); }
            // (not under a profiler: rocprofv3's counter collection serialises every kernel, so no candidate can overlap and all four would be
            // created -- and the first counter pass of round 4 aborted with HSA_STATUS_ERROR_INVALID_PACKET_FORMAT in exactly that
            // configuration, while the same pass without the probe runs through: the probe is skipped when a rocprof tool library is preloaded)
            static const bool no_probe = getenv("RPE_NO_SIDE_PROBE") != nullptr || profiler_attached();
            for (int t = 0; t < 4 && !e->side; ++t) {
                hipStream_t cand = nullptr;
                HIPTRY(hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, low ? least : 0));
                e->side_tries = t + 1;
                const int r = (no_probe || e->capturing) ? -1 : side_probe(caller, cand);
                if (r != 0 || t == 3) { e->side = cand; e->side_concurrent = r; }   // (the fourth candidate is kept whatever it showed)
                else e->side_rejects.push_back(cand);
            }
        }
    }
    return 0;
}

// res_bn: the residual is the RAW output of that layer (the projection shortcut) and its BatchNorm is applied inside this layer's
// apply pass (rpe_bn_apply_res_bn); stats_only: stop after the statistics (the shortcut itself then has no apply pass).
static int conv_bn(rpe_resnet50* e, ConvL& c, const void* x, const void* residual, int relu, void* stream, bool second_set = false,
                   unsigned char* relu_mask = nullptr, const ConvL* res_bn = nullptr, bool stats_only = false, float* gram_out = nullptr) {
    const bool train = e->train_mode != 0;
    float* stats = second_set ? e->stats_part2 : e->stats_part;
    double* dpart = second_set ? e->dpart2 : e->dpart;
    e->pending_flops = conv_flops(c);
    e->pending_bytes = conv_in_bytes(e, c) + conv_out_bytes(e, c);
    if (!train) {
        // folded inference form (fold_for_eval): a = relu(conv(x, w*scale) + shift (+ residual)); y is not written
        if (&c == &e->convs[0] && e->stem_raw) {   // a hook on conv1: its raw output is kept, BN (running statistics) applied separately
            PROF(e, RPE_PROF_CONV_FWD, stream, rpe_stem_conv_fwd(e->dtype, x, c.wf, c.y, nullptr, e->B, e->H, e->W, stream));
            PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply(e->dtype, c.y, nullptr, c.a, c.scale, c.shift, c.rows, c.d.out_c, relu, stream));
        } else
        if (&c == &e->convs[0]) PROF(e, RPE_PROF_CONV_FWD, stream, rpe_stem_conv_fwd_affine(e->dtype, x, c.wf, c.a, c.shift, relu, e->B, e->H, e->W, stream));
        else if (e->sk_ws && !second_set)   // (one workspace: the main stream's launches only; the side stream runs the projection shortcuts)
            PROF(e, RPE_PROF_CONV_FWD, stream, rpe_conv2d_fwd_affine_ws(&c.d, e->dtype, x, c.wf, c.a, c.shift, residual, relu, e->sk_ws, e->sk_ws_bytes, stream));
        else PROF(e, RPE_PROF_CONV_FWD, stream, rpe_conv2d_fwd_affine(&c.d, e->dtype, x, c.wf, c.a, c.shift, residual, relu, stream));
        return 0;
    }
    if (&c == &e->convs[0]) PROF(e, RPE_PROF_CONV_FWD, stream, rpe_stem_conv_fwd(e->dtype, x, c.wf, c.y, stats, e->B, e->H, e->W, stream));
    else PROF(e, RPE_PROF_CONV_FWD, stream, rpe_conv2d_fwd(&c.d, e->dtype, x, fwd_weight(e, c), c.y, stats, stream));
    float* rm = e->running[2 * c.bn_i];
    float* rv = e->running[2 * c.bn_i + 1];
    e->pending_bytes = 0;
    PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_finalize(stats, (int)rpe_conv2d_fwd_stats_tiles(&c.d, e->dtype), c.d.out_c, c.rows, e->params[c.p_g], e->params[c.p_b], rm, rv,
                        e->nbt[c.bn_i], 0.1f, 1e-5f, c.scale, c.shift, c.mean, c.invstd, dpart, stream));
    if (stats_only) return 0;
    e->pending_bytes = conv_out_bytes(e, c) * (2.0 + (residual ? 1.0 : 0.0) + ((relu_mask && relu) ? 1.0 / 16 : 0.0));   // y (+residual) -> a (+mask)
    if (res_bn) {
        PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply_res_bn(e->dtype, c.y, res_bn->y, res_bn->scale, res_bn->shift, c.a, c.scale, c.shift, c.rows, c.d.out_c, relu,
                                                            relu ? relu_mask : nullptr, stream));
        return 0;
    }
    if (gram_out) {   // bn2 of a y3-free block: apply + ReLU and the Gram matrix / column sums of the result in one pass
        if (residual || !relu) return rpe_set_error(RPE_ERR_STATE, "trunk engine: the fused apply + Gram pass takes no residual");
        PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply_gram(e->dtype, c.y, c.a, c.scale, c.shift, c.rows, c.d.out_c, gram_out, e->gram_ws, e->gram_ws_bytes, stream));
        return 0;
    }
    if (relu_mask && relu) PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply_mask(e->dtype, c.y, residual, c.a, c.scale, c.shift, c.rows, c.d.out_c, relu_mask, stream));
    else PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply(e->dtype, c.y, residual, c.a, c.scale, c.shift, c.rows, c.d.out_c, relu, stream));
    return 0;
}

// A stream capture (util.learn_utils.GraphedTrainStep / GraphedRolloutFrame, bench.py --graph) may only replay what exists before it
// starts: the second stream and every cross-stream event must have been created by an eager pass over the same schedule (the
// Graphed* classes warm up eagerly first).  Creating a stream or growing the event pool inside a capture is refused with
// RPE_ERR_STATE instead of being attempted: round 2 lost a whole test process to a segmentation fault inside hipStreamEndCapture
// (gpurun_out/t12.log) while the since-removed split-forward schedule forked a lazily created third stream and recycled its
// join events (sync_next = 0 in the forward AND in the backward of one capture) under capture.
static int capture_guard(rpe_resnet50* e, void* stream, const char* who) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) { (void)hipGetLastError(); e->capturing = false; return 0; }   // (no stale 'true' from an earlier capture)
    e->capturing = st != hipStreamCaptureStatusNone;
    if (!e->capturing) return 0;
    if (e->profiling) return rpe_set_error(RPE_ERR_STATE, "trunk engine: per-launch profiling events cannot be recorded inside a stream capture");
    if (e->overlap && !e->side && !getenv("RPE_NO_OVERLAP")) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: called under stream capture before any eager pass created the second stream -- run the step eagerly once, then capture", who);
        return rpe_set_error(RPE_ERR_STATE, msg);
    }
    return 0;
}

static int forward_impl(rpe_resnet50_t* e, const float* img_nchw, const unsigned char* frames, int Hs, int Ws, const float* mean3, const float* std3,
                        float* features, long ld_features, int training, void* stream, const rpe_resize_plan* rs = nullptr) {
    if (!e || !e->bound) return rpe_set_error(RPE_ERR_STATE, "resnet50_forward: engine not bound");
    if ((!img_nchw && !frames) || !features || ld_features < e->latent) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_forward: bad img/features");
    TRY(capture_guard(e, stream, "resnet50_forward"));   // first: a refusal (profiling under capture, no second stream yet) must come before any launch is recorded
    e->train_mode = training;
    if (training) e->walk_next = 0;
    WalkScope walk(e, training != 0);
    if (training && e->pack_state != 1) TRY(rpe_resnet50_pack_weights(e, stream));
    if (!training && e->pack_state != 2) TRY(fold_for_eval(e, stream));
    if (frames && rs) PROF(e, RPE_PROF_OTHER, stream, rpe_stage_frames_u8_resized(e->dtype, frames, e->x4, e->B, Hs, Ws, rs->Hr, rs->Wr, rs->top, rs->left, e->H, e->W,
                                                                                    rs->xb, rs->xk, rs->ksx, rs->yb, rs->yk, rs->ksy, rs->tmp, mean3, std3, stream));
    else if (frames) PROF(e, RPE_PROF_OTHER, stream, rpe_stage_frames_u8(e->dtype, frames, e->x4, e->B, Hs, Ws, e->H, e->W, mean3, std3, stream));
    else PROF(e, RPE_PROF_OTHER, stream, rpe_stage_image_nhwc4(e->dtype, img_nchw, e->x4, e->B, e->H, e->W, stream));
    ConvL& st = e->convs[0];
    TRY(ensure_side(e, (hipStream_t)stream));
    e->sync_next = 0;
    static const bool pool_fuse_ok = getenv("RPE_NO_POOL_FUSE") == nullptr;
    const bool aux_here = e->aux_fwd.w != nullptr;
    e->a1_valid = true;
    if (training && pool_fuse_ok && !((st.Ho | st.Wo) & 1)) {
        // conv + statistics, then BatchNorm apply + ReLU + max pool in one pass over y (the separate pool pass re-read all of a1)
        TRY(conv_bn(e, st, e->x4, nullptr, 1, stream, false, nullptr, nullptr, true));
        if (aux_here) {
            // ... and the bn1 aux head (1x1 conv 64 -> 1 + 2x2 max pool [x depth feature]) in the same pass; a1 itself is not written
            e->pending_bytes = conv_out_bytes(e, st) * 1.25 + (double)e->B * (st.Ho / 2) * (st.Wo / 2) * (64 + 9);
            PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply_maxpool3x3s2_aux(e->dtype, st.y, st.scale, st.shift, nullptr, e->pool, e->pool_idx, e->B, st.Ho, st.Wo,
                                                                          e->aux_fwd.w, e->aux_fwd.bias, e->aux_fwd.depth_feat, e->aux_fwd.out, e->aux_fwd.ld,
                                                                          e->aux_fwd.raw, e->aux_fwd.idx, stream));
            e->a1_valid = false;
        } else {
        e->pending_bytes = conv_out_bytes(e, st) * 2.25 + (double)e->B * (st.Ho / 2) * (st.Wo / 2) * 64;   // y -> a1, pool + winner index
        PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_apply_maxpool3x3s2(e->dtype, st.y, st.scale, st.shift, st.a, e->pool, e->pool_idx, e->B, st.Ho, st.Wo, 64, stream));
        }
    } else {
        TRY(conv_bn(e, st, e->x4, nullptr, 1, stream));
        e->pending_bytes = conv_out_bytes(e, st) * 1.25 + (double)e->B * (st.Ho / 2) * (st.Wo / 2) * 64;   // a1 -> pool + winner index
        PROF(e, RPE_PROF_OTHER, stream, rpe_maxpool3x3s2_fwd(e->dtype, st.a, e->pool, e->pool_idx, e->B, st.Ho, st.Wo, 64, stream));
        if (aux_here)   // (a forward that cannot take the fused pass still owes the caller the aux head it was handed)
            TRY(rpe_aux_head_fwd(e->dtype, st.a, e->aux_fwd.w, e->aux_fwd.bias, e->aux_fwd.depth_feat, e->aux_fwd.out, e->aux_fwd.ld, e->aux_fwd.raw, e->aux_fwd.idx,
                                 e->B, st.Ho, st.Wo, stream));
    }
    e->aux_fwd.w = nullptr;   // one forward only
    const void* x = e->pool;
    static const bool fwd_overlap = getenv("RPE_NO_FWD_OVERLAP") == nullptr;
    // training: the projection shortcut's BatchNorm is applied inside conv3's apply pass (no pass / normalised copy of its own);
    // RPE_NO_DS_FUSE=1: the separate pass
    static const bool ds_fuse_ok = getenv("RPE_NO_DS_FUSE") == nullptr;
    const bool fuse_ds = ds_fuse_ok && training;
    for (auto& b : e->blocks) {
        ConvL &c1 = e->convs[b.c1], &c2 = e->convs[b.c2], &c3 = e->convs[b.out];
        const void* idn = x;
        hipEvent_t ds_done = nullptr;
        // (training only.  An INFERENCE frame stays on one stream: with the fork / join to the second stream a batch-1 frame took 3-4 ms
        // instead of 1.1 (eager) / 0.45 (captured graph replayed; hipGraphLaunch itself 2.6 ms on the host) in some processes on the
        // round-3 boxes -- which model is hit changes from process to process, profiles/r03_rollout_latency.txt -- and at batch 1 the
        // branch has nothing to overlap with anyway)
        if (b.cd >= 0 && e->overlap && e->side && fwd_overlap && training) {
            // projection shortcut (conv + BN, no ReLU): independent of conv1..conv2, joined before conv3's BN adds it
            ConvL& cd = e->convs[b.cd];
            hipEvent_t x_ready = sync_event(e);
            ds_done = sync_event(e);
            if (!x_ready || !ds_done) return event_error(e);
            HIPTRY(hipEventRecord(x_ready, (hipStream_t)stream));
            HIPTRY(hipStreamWaitEvent(e->side, x_ready, 0));
            { WalkScope up(e, false); TRY(conv_bn(e, cd, x, nullptr, 0, e->side, true, nullptr, nullptr, fuse_ds)); }
            HIPTRY(hipEventRecord(ds_done, e->side));
            idn = cd.a;
        }
        TRY(conv_bn(e, c1, x, nullptr, 1, stream));
        if (e->basic) {
            // BasicBlock: out = relu(bn2(conv2(relu(bn1(conv1 x)))) + shortcut); the projection shortcut as in the bottleneck plan (second
            // stream, its BatchNorm applied inside bn2's apply pass when training)
            static const bool use_mask_b = getenv("RPE_NO_RELU_MASK") == nullptr;
            if (b.cd >= 0 && !ds_done) { ConvL& cd = e->convs[b.cd]; TRY(conv_bn(e, cd, x, nullptr, 0, stream, false, nullptr, nullptr, fuse_ds)); idn = cd.a; }
            if (ds_done) HIPTRY(hipStreamWaitEvent((hipStream_t)stream, ds_done, 0));
            if (b.cd >= 0 && fuse_ds) TRY(conv_bn(e, c2, c1.a, e->convs[b.cd].y, 1, stream, false, use_mask_b ? b.relu_mask : nullptr, &e->convs[b.cd]));
            else TRY(conv_bn(e, c2, c1.a, idn, 1, stream, false, use_mask_b ? b.relu_mask : nullptr));
            x = c2.a;
            continue;
        }
        const bool y3f_fwd = training && b.gram && b.relu_mask;
        const bool fused_gram = y3f_fwd && e->apply_gram && (c2.d.out_c == 64 || c2.d.out_c == 128);
        TRY(conv_bn(e, c2, c1.a, nullptr, 1, stream, false, nullptr, nullptr, false, fused_gram ? b.gram : nullptr));
        if (b.cd >= 0 && !ds_done) { ConvL& cd = e->convs[b.cd]; TRY(conv_bn(e, cd, x, nullptr, 0, stream, false, nullptr, nullptr, fuse_ds)); idn = cd.a; }
        if (ds_done) HIPTRY(hipStreamWaitEvent((hipStream_t)stream, ds_done, 0));
        static const bool use_mask = getenv("RPE_NO_RELU_MASK") == nullptr;
        if (y3f_fwd) {
            // y3-free: Gram matrix of a2 -> BN3 statistics -> conv3 with BN + identity (under the shortcut's BN) + ReLU + mask in its epilogue
            const ConvL* cdp = (b.cd >= 0 && fuse_ds) ? &e->convs[b.cd] : nullptr;
            if (!fused_gram) {   // (else bn2's apply pass left the Gram matrix behind)
                e->pending_flops = 2.0 * (double)c3.rows * c3.d.in_c * c3.d.in_c;
                e->pending_bytes = conv_in_bytes(e, c3);
                PROF(e, RPE_PROF_BN_FWD, stream, rpe_gram(e->dtype, c2.a, c3.rows, c3.d.in_c, b.gram, e->gram_ws, e->gram_ws_bytes, stream));
            }
            e->pending_bytes = 0;
            PROF(e, RPE_PROF_BN_FWD, stream, rpe_bn_stats_from_gram(e->dtype, c3.wf, c3.d.out_c, c3.d.in_c, b.gram, (int)rpe_gram_ones_row(c3.d.in_c), c3.rows,
                                                                    e->params[c3.p_g], e->params[c3.p_b], e->running[2 * c3.bn_i], e->running[2 * c3.bn_i + 1],
                                                                    e->nbt[c3.bn_i], 0.1f, 1e-5f, c3.scale, c3.shift, c3.mean, c3.invstd, stream));
            e->pending_flops = conv_flops(c3);
            e->pending_bytes = conv_in_bytes(e, c3) + conv_out_bytes(e, c3) * (2.0 + (e->y3_keep ? 1.0 : 0.0) + 1.0 / 16);   // x, residual -> out (+ y) + mask
            PROF(e, RPE_PROF_CONV_FWD, stream, rpe_conv1x1_fwd_bn(&c3.d, e->dtype, c2.a, c3.wf, c3.a, e->y3_keep ? c3.y : nullptr, c3.scale, c3.shift,
                                                                 cdp ? cdp->y : idn, cdp ? cdp->scale : nullptr, cdp ? cdp->shift : nullptr, b.relu_mask, stream));
        } else
        if (b.cd >= 0 && fuse_ds) TRY(conv_bn(e, c3, c2.a, e->convs[b.cd].y, 1, stream, false, use_mask ? b.relu_mask : nullptr, &e->convs[b.cd]));
        else
        TRY(conv_bn(e, c3, c2.a, idn, 1, stream, false, use_mask ? b.relu_mask : nullptr));   // (relu_mask is null for fp32 engines)
        x = c3.a;
    }
    ConvL& last = e->convs[e->blocks.back().out];
    TRY(rpe_avgpool_fwd(e->dtype, last.a, e->pooled, e->B, last.Ho * last.Wo, e->feat, stream));
    const int np = (int)e->pnames.size();
    TRY(rpe_linear_fwd_ws(RPE_F32, e->pooled, e->feat, e->params[np - 2], e->feat, e->params[np - 1], features, (int)ld_features, e->B, e->latent, e->feat, 0,
                          nullptr, 0, e->fc_ws, e->fc_ws ? e->fc_ws_bytes : 0, stream));
    e->fwd_done = training != 0;
    return 0;
}

extern "C" int rpe_resnet50_forward(rpe_resnet50_t* e, const float* img_nchw, float* features, long ld_features, int training, void* stream) {
    return forward_impl(e, img_nchw, nullptr, 0, 0, nullptr, nullptr, features, ld_features, training, stream);
}

extern "C" int rpe_resnet50_forward_u8(rpe_resnet50_t* e, const unsigned char* frames, int Hs, int Ws, const float* mean3_host,
                                       const float* std3_host, float* features, long ld_features, int training, void* stream) {
    if (!frames) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_forward_u8: null frames");
    return forward_impl(e, nullptr, frames, Hs, Ws, mean3_host, std3_host, features, ld_features, training, stream);
}

extern "C" int rpe_resnet50_forward_u8_resized(rpe_resnet50_t* e, const unsigned char* frames, int Hs, int Ws, const rpe_resize_plan* rs,
                                               const float* mean3_host, const float* std3_host, float* features, long ld_features, int training, void* stream) {
    if (!frames || !rs) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_forward_u8_resized: null frames / resize plan");
    return forward_impl(e, nullptr, frames, Hs, Ws, mean3_host, std3_host, features, ld_features, training, stream, rs);
}

extern "C" const void* rpe_resnet50_early_feature(const rpe_resnet50_t* e) { return (e && e->a1_valid) ? e->convs[0].a : nullptr; }
extern "C" void* rpe_resnet50_early_grad(rpe_resnet50_t* e) { return e ? e->early_grad : nullptr; }

// BN backward of layer c: dA (grad wrt c.a) -> dy (may alias dA); dz_out optional
static int bn_back(rpe_resnet50* e, ConvL& c, const void* dA, int relu, void* dy, void* dz_out, void* stream) {
    e->pending_bytes = conv_out_bytes(e, c) * ((relu ? 3.0 : 2.0) + 3.0 + (dz_out ? 1.0 : 0.0));   // reduce pass: dA, y (, a); apply pass: dA, y -> dy (, dz)
    PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_backward(e->dtype, dA, relu ? c.a : nullptr, c.y, c.mean, c.invstd, e->params[c.p_g], e->grads[c.p_g], e->grads[c.p_b], dy,
                           dz_out, c.rows, c.d.out_c, e->bwd_part, e->bwd_part_floats, e->c1c2, e->dpart, stream));
    return 0;
}

// data gradient of conv `c` with the BN-backward reduction of layer `bnl` (the layer producing c's input) fused in.
// mask_mode 1: ReLU mask from bnl.a (residual block output); 2: mask recomputed from bnl.y, scale, shift.
static int dgrad_fused(rpe_resnet50* e, ConvL& c, const void* dy, void* dz, const void* addend, ConvL* bnl, int mask_mode, void* stream,
                       const unsigned char* relu_mask = nullptr, bool no_y = false, const void* t_a = nullptr, int t_p = 0, float* t_out = nullptr,
                       bool sub_addend = false) {
    rpe_bn_bwd_epilogue ep;
    ep.y = no_y ? nullptr : bnl->y;                      // (y3-free block: sum dz only, rpe_conv2d_dgrad_bn)
    ep.a_mask = mask_mode == 1 ? relu_mask : nullptr;   // block outputs: 1 bit per element instead of re-reading a_out
    ep.a_out = (mask_mode == 1 && !ep.a_mask) ? bnl->a : nullptr;
    ep.mean = bnl->mean; ep.invstd = bnl->invstd;
    ep.scale = mask_mode == 2 ? bnl->scale : nullptr;
    ep.shift = mask_mode == 2 ? bnl->shift : nullptr;
    ep.stats_part = e->stats_part;
    e->pending_flops = conv_flops(c);
    // reads dy; writes dz; the fused epilogue also reads y (and a_out for residual outputs) and the shortcut addend
    // (sub_addend: the addend is the compact gradient of a stride-2 shortcut, a quarter of the rows)
    e->pending_bytes = conv_out_bytes(e, c) + conv_in_bytes(e, c) * ((no_y ? 1.0 : 2.0) + (mask_mode == 1 ? (ep.a_mask ? 1.0 / 16 : 1.0) : 0.0) +
                                                                      (addend ? (sub_addend ? 0.25 : 1.0) : 0.0));
    e->fused_tiles = (int)rpe_conv2d_dgrad_stats_tiles(&c.d, e->dtype);  // partial-sum rows this launch leaves behind
    if (t_out) {   // ... and T = dz^T a2 of the producing block from the tile on its way out (persistent launch)
        e->pending_flops += 2.0 * (double)c.rows * c.d.in_c * t_p;
        e->pending_bytes += conv_in_bytes(e, c) * (double)t_p / c.d.in_c;
        PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv1x1_dgrad_bn_t(&c.d, e->dtype, dy, c.wd, dz, addend, &ep, t_a, t_p, t_out, e->main_slab, e->main_slab_bytes, stream));
        return 0;
    }
    if (sub_addend) PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad_bn_sub(&c.d, e->dtype, dy, c.wd, dz, addend, &ep, stream));
    else PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad_bn(&c.d, e->dtype, dy, c.wd, dz, addend, &ep, stream));
    return 0;
}

// second half of the fused BN backward of layer c: partials (left in stats_part by dgrad_fused) -> dgamma, dbeta, dy
static int bn_from_dz(rpe_resnet50* e, ConvL& c, const void* dz, void* dy, void* stream) {
    e->pending_bytes = conv_out_bytes(e, c) * 3.0;   // dz, y -> dy
    PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_backward_from_dz(e->dtype, dz, c.y, c.mean, c.invstd, e->params[c.p_g], e->stats_part,
                                                              e->fused_tiles, e->grads[c.p_g], e->grads[c.p_b], dy, c.rows,
                                                              c.d.out_c, e->c1c2, e->dpart, stream));
    return 0;
}

static int wgrad_on(rpe_resnet50* e, ConvL& c, const void* x, const void* dy, hipStream_t run) {
    float* dw = e->grads[c.p_w];
    e->pending_flops = conv_flops(c);
    e->pending_bytes = conv_in_bytes(e, c) + conv_out_bytes(e, c);
    if (e->wg_slab) {   // deterministic: per-workgroup slabs + fixed-order sum, overwrites dw (launches on `run` are ordered: one slab buffer)
        PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv2d_wgrad_det(&c.d, e->dtype, x, dy, dw, e->wg_slab, e->wg_slab_bytes, run));
        return 0;
    }
    if (!e->gspan_lo) HIPTRY(hipMemsetAsync(dw, 0, (size_t)e->pnumel[c.p_w] * 4, run));
    PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv2d_wgrad(&c.d, e->dtype, x, dy, dw, run));
    return 0;
}

// work for the second stream whose inputs are final at this point of the caller's stream: issued there behind an event (without a
// second stream it runs in place).  Measured and rejected in round 3 (profiles/r03_ab_wgrad_hold.txt): HOLDING the weight gradients of
// the deep, matrix-core-bound blocks back until the data-gradient chain reaches the HBM-bound layers 1-2 (one event for all of them)
// -- 20.4-21.5 ms/step for five hold / flush points against 20.05: a weight gradient issued right behind its dy is the best placement.
template <typename F> static int to_side(rpe_resnet50* e, void* stream, F work) {
    if (!(e->overlap && e->side)) return work((hipStream_t)stream);
    hipEvent_t ready = sync_event(e);
    if (!ready) return event_error(e);
    HIPTRY(hipEventRecord(ready, (hipStream_t)stream));
    HIPTRY(hipStreamWaitEvent(e->side, ready, 0));
    WalkScope up(e, false);
    return work(e->side);
}
static int wgrad(rpe_resnet50* e, ConvL& c, const void* x, const void* dy, void* stream) {
    ConvL* cp = &c;
    return to_side(e, stream, [e, cp, x, dy](hipStream_t run) { return wgrad_on(e, *cp, x, dy, run); });
}
// Folded form of (BN backward of c.bn -> weight gradient + data gradient of the 1x1 conv c), entered with dz = gradient wrt the BN
// output and this BN's partial sums in stats_part (left by the data gradient that produced dz):
//   main: coefficients -> fold (w_kcat, bias) -> K-concatenated data gradient [dz | x] with the epilogue of the layer behind;
//   side: dz, y -> dy (streaming), weight gradient from dy.   The main stream never touches dy.
static int conv1x1_backward_folded(rpe_resnet50* e, ConvL& c, const void* dz, ConvL& behind, void* stream, const Block* y3f = nullptr) {
    const void* x = behind.a;
    if (y3f) {
        // y3-free block: T = dz^T a2 first (caller's stream: the coefficients need it), then sum dz (partials) + rowdot(T, W) -> c1, c2
        e->pending_flops = conv_flops(c);
        e->pending_bytes = conv_in_bytes(e, c) + conv_out_bytes(e, c);
        // (timing experiment of round 4, code removed: with this launch on the second stream -- wrong coefficients, the chain not waiting
        // for it -- the step ran 18.91 vs 19.24 ms, profiles/r04_ab_t_gemm_off_chain.txt: the upper bound of what taking dz^T a2 off the
        // data-gradient chain could return)
        if (y3f->t_ready) {
            // (the next block's fused conv1 data gradient left dz^T a2 behind: RPE_T_FUSE=1)
        } else
        PROF(e, RPE_PROF_CONV_WGRAD, stream, rpe_conv2d_wgrad_det(&c.d, e->dtype, x, dz, y3f->dzt_a, e->main_slab, e->main_slab_bytes, stream));
        e->pending_bytes = 0;
        PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_backward_coeffs_t(e->dtype, e->stats_part, e->fused_tiles, c.d.out_c, c.rows, y3f->dzt_a, c.wf, c.d.in_c, c.mean, c.invstd,
                                                                   e->grads[c.p_g], e->grads[c.p_b], c.c1c2, e->dpart, stream));
    } else {
    e->pending_bytes = 0;
    PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_backward_coeffs(e->stats_part, e->fused_tiles, c.d.out_c, c.rows, e->grads[c.p_g], e->grads[c.p_b], c.c1c2, e->dpart, stream));
    }
    ConvL* cp = &c;
    auto side_part = [e, cp, dz, x, y3f](hipStream_t run) -> int {
    ConvL& c = *cp;
    float* dw = e->grads[c.p_w];
    if (y3f) {
        e->pending_flops = 2.0 * (double)c.d.out_c * c.d.in_c * c.d.in_c;
        e->pending_bytes = 0;
        PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv1x1_wgrad_combine(&c.d, y3f->dzt_a, y3f->gram, e->params[c.p_w], e->params[c.p_g], c.invstd, c.mean, c.c1c2, dw, run));
    } else
    if (e->fold_w && e->wfold_scratch && c.d.in_c <= e->fold_w_max) {
        // weight gradient from dz and x alone (no dy): dz^T x, x^T x, colsum(x), W (x^T x), combine
        e->pending_flops = conv_flops(c) * (1.0 + (double)c.d.in_c / c.d.out_c);
        e->pending_bytes = conv_out_bytes(e, c) + 3.0 * conv_in_bytes(e, c);
        PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv1x1_wgrad_folded(&c.d, e->dtype, dz, x, e->params[c.p_w], e->params[c.p_g], c.invstd, c.mean, c.c1c2, dw,
                                                                  e->wfold_scratch, e->wfold_scratch_bytes, run));
    } else {
    e->pending_bytes = conv_out_bytes(e, c) * 3.0;   // dz, y -> dy
    PROF(e, RPE_PROF_BN_BWD, run, rpe_bn_backward_apply_dz(e->dtype, dz, c.y, c.mean, c.invstd, e->params[c.p_g], c.c1c2, c.dy, c.rows, c.d.out_c, run));
    e->pending_flops = conv_flops(c);
    e->pending_bytes = conv_in_bytes(e, c) + conv_out_bytes(e, c);
    if (e->wg_slab) {
        PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv2d_wgrad_det(&c.d, e->dtype, x, c.dy, dw, e->wg_slab, e->wg_slab_bytes, run));
    } else {
        if (!e->gspan_lo) HIPTRY(hipMemsetAsync(dw, 0, (size_t)e->pnumel[c.p_w] * 4, run));
        PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv2d_wgrad(&c.d, e->dtype, x, c.dy, dw, run));
    }
    }
    return 0;
    };
    TRY(to_side(e, stream, side_part));
    e->pending_bytes = 0;
    PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_bwd_fold_conv1x1(e->dtype, c.d.out_c, c.d.in_c, fwd_weight(e, c), c.wd, e->params[c.p_g], c.invstd, c.mean, c.c1c2,
                                                              e->w_kcat, e->fold_bias, e->fold_scratch, e->fold_scratch_bytes, stream));
    rpe_bn_bwd_epilogue ep;
    ep.y = behind.y; ep.a_mask = nullptr; ep.a_out = nullptr;
    ep.mean = behind.mean; ep.invstd = behind.invstd; ep.scale = behind.scale; ep.shift = behind.shift;   // mask recomputed from y
    ep.stats_part = e->stats_part;
    e->pending_flops = conv_flops(c) * (1.0 + (double)c.d.in_c / c.d.out_c);
    e->pending_bytes = conv_out_bytes(e, c) + conv_in_bytes(e, c) * 3.0;   // reads dz, x, y_behind; writes dz_behind
    e->fused_tiles = (int)rpe_conv2d_dgrad_stats_tiles(&c.d, e->dtype);
    PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv1x1_dgrad_kcat(&c.d, e->dtype, dz, x, e->w_kcat, e->fold_bias, behind.dy, &ep, stream));
    return 0;
}

static int join_side(rpe_resnet50* e, hipStream_t s) {
    // everything the side stream produced so far (weight gradients) is complete before the caller's next launch on s
    if (e->overlap && e->side) {
        hipEvent_t done = sync_event(e);
        if (!done) return event_error(e);
        HIPTRY(hipEventRecord(done, e->side));
        HIPTRY(hipStreamWaitEvent(s, done, 0));
    }
    return 0;
}

extern "C" int rpe_resnet50_backward_begin(rpe_resnet50_t* e, const float* d_features, long ld_d_features, void* stream) {
    if (!e || !e->bound) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward: engine not bound");
    if (!e->fwd_done) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward: no training-mode forward to differentiate");
    const int np = (int)e->pnames.size();
    for (int i = 0; i < np; ++i)
        if (!e->grads[i]) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward: gradient tensors were not bound");
    hipStream_t s = (hipStream_t)stream;
    TRY(capture_guard(e, stream, "resnet50_backward"));
    TRY(ensure_side(e, s));
    WalkScope walk(e, true);
    e->sync_next = 0;
    if (e->gspan_lo) HIPTRY(hipMemsetAsync(e->gspan_lo, 0, e->gspan_bytes, s));
    // fc
    float* dWfc = e->grads[np - 2];
    if (e->main_slab) {
        TRY(rpe_linear_wgrad_det(RPE_F32, d_features, (int)ld_d_features, e->pooled, e->feat, dWfc, e->feat, e->B, e->latent, e->feat, 0, e->main_slab, e->main_slab_bytes, stream));
    } else {
        if (!e->gspan_lo) HIPTRY(hipMemsetAsync(dWfc, 0, (size_t)e->latent * e->feat * 4, s));
        TRY(rpe_linear_wgrad(RPE_F32, d_features, (int)ld_d_features, e->pooled, e->feat, dWfc, e->feat, e->B, e->latent, e->feat, stream));
    }
    TRY(rpe_colsum(d_features, e->B, e->latent, (int)ld_d_features, e->grads[np - 1], 0, stream));
    // d_pooled[B][2048] = d_features[B][latent] * Wfc[latent][2048]  ==  NT with weight fc_wt [2048][latent_pad].
    // K runs to latent_pad: the extra columns of d_features (whatever the caller keeps there) meet zero weights.
    if ((ld_d_features & 3) || ld_d_features < e->latent_pad)
        return rpe_set_error(RPE_ERR_ALIGN, "resnet50_backward: ld_d_features must be a multiple of 4 and >= pad4(latent_dim)");
    TRY(rpe_linear_fwd_ws(RPE_F32, d_features, (int)ld_d_features, e->fc_wt, e->latent_pad, nullptr, e->d_pooled, e->feat, e->B, e->feat, e->latent_pad, 0,
                          nullptr, 0, e->fc_ws, e->fc_ws ? e->fc_ws_bytes : 0, stream));
    ConvL& last = e->convs[e->blocks.back().out];
    TRY(rpe_avgpool_bwd(e->dtype, e->d_pooled, e->blocks.back().dz, e->B, last.Ho * last.Wo, e->feat, stream));
    e->bwd_next = (int)e->blocks.size() - 1;
    return 0;
}

// workgroups of the zero-filled stride-2 shortcut data gradient from which the compact form is used: one per CU of the device
static long compact_min_tiles() {
    static const long cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
        return (long)n;
    }();
    return cus;
}

// Backward through the next `count` bottleneck blocks (descending).  On return every gradient of those blocks is complete
// in stream order on `stream` (the side stream is joined), so the caller may start reducing them across replicas.
// Per block, entering with gA = dz3 (ReLU-masked gradient at the block output; for the last block: the raw dA).
// Every data-gradient GEMM also applies the ReLU mask of the layer it feeds and emits that layer's BN-backward
// partial sums (rpe_conv2d_dgrad_bn), so each BN costs one more pass (dz, y -> dy) instead of two full passes.
extern "C" int rpe_resnet50_backward_blocks(rpe_resnet50_t* e, int count, int join, void* stream) {
    if (!e || !e->bound || e->bwd_next < -1) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward_blocks: call rpe_resnet50_backward_begin first");
    int bi = e->bwd_next;
    WalkScope walk(e, true);
    // Gradient buffers.  Every layer owns the buffer its dz / dy lives in (ConvL::dy) and every block the buffer of its
    // output gradient (Block::dz): 8.5 GB more workspace at 256 images than rotating a handful of scratch buffers, but a weight
    // gradient on the side stream then never reads a buffer the main stream writes again, so the main stream waits for the
    // side stream nowhere inside the backward (each such event wait cost a ~10 us bubble: 70 per step, 0.8 ms).
    // A weight gradient is issued right when its dy is final and so runs beside the data gradient of the SAME layer; issuing
    // it one launch later (1x1 beside 3x3) measured slower (+0.3 ms/step).
    for (; bi >= 0 && count > 0; --bi, --count) {
        Block& b = e->blocks[bi];
        ConvL &c1 = e->convs[b.c1], &c2 = e->convs[b.c2], &c3 = e->convs[b.out];
        const void* x_in = bi == 0 ? (const void*)e->pool : (const void*)e->convs[e->blocks[bi - 1].out].a;
        void* gA = b.dz;                                             // dz3 (for the last block: the raw dA)
        void* gD = bi == 0 ? e->d_pool : e->blocks[bi - 1].dz;       // where the gradient of the block input goes
        // a hooked layer output (the input of a stage-entry block) carries one more gradient term: it joins the shortcut gradient
        const void* hook_in = nullptr;
        if (b.first && b.layer >= 2) hook_in = e->hook_grad[b.layer - 1];   // (stage-entry blocks of layers 2..4 have a projection shortcut in every member)
        if (e->basic) {
            // BasicBlock, entering with gA = dz2 (ReLU-masked gradient at the block output; for the last block: the raw dA) and -- except for
            // the last block -- bn2's partial sums left by the next block's fused conv1 data gradient
            if (bi == (int)e->blocks.size() - 1) TRY(bn_back(e, c2, gA, 1, c2.dy, gA, stream));   // dy2, dz2 (in place)
            else TRY(bn_from_dz(e, c2, gA, c2.dy, stream));                                        // dy2 (gA keeps dz2 = the shortcut gradient)
            TRY(wgrad(e, c2, c1.a, c2.dy, stream));
            TRY(dgrad_fused(e, c2, c2.dy, c1.dy, nullptr, &c1, 2, stream));                        // dz1 (+ bn1's partial sums)
            TRY(bn_from_dz(e, c1, c1.dy, c1.dy, stream));
            TRY(wgrad(e, c1, x_in, c1.dy, stream));
            const void* shortcut = gA;
            if (b.cd >= 0) {
                ConvL& cd = e->convs[b.cd];
                shortcut = e->G[0];
                TRY(bn_back(e, cd, gA, 0, cd.dy, nullptr, stream));                                // no ReLU on the projection shortcut
                TRY(wgrad(e, cd, x_in, cd.dy, stream));
                e->pending_flops = conv_flops(cd);
                e->pending_bytes = conv_out_bytes(e, cd) + conv_in_bytes(e, cd) * (hook_in ? 2.0 : 1.0);
                PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad(&cd.d, e->dtype, cd.dy, cd.wd, e->G[0], hook_in, stream));
            }
            static const bool use_mask_b = getenv("RPE_NO_RELU_MASK") == nullptr;
            if (bi > 0) {
                const Block& pb = e->blocks[bi - 1];
                TRY(dgrad_fused(e, c1, c1.dy, gD, shortcut, &e->convs[pb.out], 1, stream, use_mask_b ? pb.relu_mask : nullptr));   // dz2 of the previous block
            } else {
                e->pending_flops = conv_flops(c1);
                e->pending_bytes = conv_out_bytes(e, c1) + conv_in_bytes(e, c1) * 2.0;
                PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad(&c1.d, e->dtype, c1.dy, c1.wd, gD, shortcut, stream));
            }
            continue;
        }
        static const bool ds_fold_ok = getenv("RPE_NO_DS_FOLD") == nullptr;
        const bool y3f = b.gram && b.relu_mask && !e->y3_keep;   // this block's y3 was never written
        if (e->fold && c3.d.in_c <= 256 && e->train_mode) {   // layers 1-3 (layer4's tensors are small: the unfolded form is faster there)
            TRY(conv1x1_backward_folded(e, c3, gA, c2, stream, y3f ? &b : nullptr));              // dz2 (dy3 exists on the side stream only)
        } else {
            if (bi == (int)e->blocks.size() - 1) TRY(bn_back(e, c3, gA, 1, c3.dy, gA, stream));  // unfused: dy3, dz3 (in place)
            else TRY(bn_from_dz(e, c3, gA, c3.dy, stream));                                       // dy3 (gA keeps dz3 = shortcut gradient)
            TRY(wgrad(e, c3, c2.a, c3.dy, stream));
            TRY(dgrad_fused(e, c3, c3.dy, c2.dy, nullptr, &c2, 2, stream));   // dz2
        }
        TRY(bn_from_dz(e, c2, c2.dy, c2.dy, stream));
        TRY(wgrad(e, c2, c1.a, c2.dy, stream));
        TRY(dgrad_fused(e, c2, c2.dy, c1.dy, nullptr, &c1, 2, stream));   // dz1
        // bn1 + conv1.  Folded (layers 1-2): coefficients only on this stream; the weight gradient (side stream) and the data gradient
        // (below, behind the projection shortcut's backward, which shares the fold scratch) both work from dz1 and y1 -- no dy1, no
        // streaming dz, y -> dy pass.  Otherwise: that pass, then both gradients from dy1.
        const bool fold_c1 = e->fold && e->fold1 && e->fold_w && e->wfold_scratch && e->train_mode && c1.d.out_c <= e->fold1_max && (c1.d.out_c % 64) == 0 &&
                             (c1.d.in_c % 64) == 0;
        if (fold_c1) {
            e->pending_bytes = 0;
            PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_backward_coeffs(e->stats_part, e->fused_tiles, c1.d.out_c, c1.rows, e->grads[c1.p_g], e->grads[c1.p_b], c1.c1c2,
                                                                    e->dpart, stream));
            ConvL* cp = &c1;
            TRY(to_side(e, stream, [e, cp, x_in](hipStream_t run) -> int {
                ConvL& c = *cp;
                e->pending_flops = conv_flops(c) * 2.0;
                e->pending_bytes = 2.0 * conv_out_bytes(e, c) + conv_in_bytes(e, c);   // dz, y, x
                PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv1x1_wgrad_folded_y(&c.d, e->dtype, c.dy, c.y, x_in, e->params[c.p_g], c.invstd, c.mean, c.c1c2, e->grads[c.p_w],
                                                                            e->wfold_scratch, e->wfold_scratch_bytes, run));
                return 0;
            }));
        } else {
            TRY(bn_from_dz(e, c1, c1.dy, c1.dy, stream));
            TRY(wgrad(e, c1, x_in, c1.dy, stream));
        }
        // the previous block's dz3^T a2 rides on this block's conv1 data gradient (RPE_T_FUSE=1: decided here, the shortcut's form depends on it)
        bool t_here = false;
        if (!fold_c1 && bi > 0) {
            const Block& pb = e->blocks[bi - 1];
            const ConvL& p3 = e->convs[pb.c3];
            t_here = pb.gram && pb.relu_mask && !e->y3_keep && e->t_fused && (p3.d.in_c == 64 || p3.d.in_c == 128) && (c1.d.in_c % 128) == 0 && c1.d.kh == 1 &&
                     c1.d.stride == 1;
        }
        const void* shortcut = gA;
        // 1x1 / stride-2 projection shortcut over even dims (the entry blocks of layers 2-4): its data gradient lives on the even pixels alone.
        // It is kept COMPACT ([B][H/2][W/2][C] in G[0]: one dense GEMM) and conv1's data gradient below reads it as a subsampled addend,
        // instead of a full-resolution tensor that is three quarters zeros written once and read once.  A hooked layer output (its gradient
        // joins here at full resolution), odd dims and the T side product keep the zero-filled form.  So do small launches: while the
        // zero-filled launch -- 4 parity classes x 128-row tiles x 128-column tiles -- has fewer workgroups than the chip has CUs, its
        // empty tiles run BESIDE the others in one round and the few MB it writes are read back from cache: there is nothing to take away,
        // and the launch plan of such steps stays what it was (compact_min_tiles).
        bool sub_addend = false;
        if (b.cd >= 0) {
            ConvL& cd = e->convs[b.cd];
            shortcut = e->G[0];
            const long zero_filled_tiles = 4L * (((long)cd.d.batch * (cd.d.in_h / 2) * (cd.d.in_w / 2) + 127) / 128) * ((cd.d.in_c + 127) / 128);
            sub_addend = zero_filled_tiles >= compact_min_tiles() && !hook_in && !t_here && cd.d.kh == 1 && cd.d.kw == 1 && cd.d.stride == 2 && cd.d.pad == 0 && !(cd.d.in_h & 1) && !(cd.d.in_w & 1) &&
                         c1.d.kh == 1 && c1.d.kw == 1 && c1.d.stride == 1 && c1.d.pad == 0;
            if (ds_fold_ok && e->fold && e->train_mode && e->fold_w && e->wfold_scratch && !hook_in && cd.d.kh == 1 && cd.d.stride == 1 &&
                       cd.d.pad == 0 && cd.d.in_c <= e->fold_w_max && (cd.d.out_c % 128) == 0 && (cd.d.in_c % 64) == 0) {
                // stride-1 projection shortcut (layer1): its BatchNorm backward folds into the 1x1 conv like conv3's -- one reduction pass
                // (dz = gA, no mask), then the K-concatenated data gradient and the folded weight gradient; no dy, no apply pass
                e->pending_bytes = conv_out_bytes(e, cd) * 2.0;
                PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_backward_reduce(e->dtype, gA, nullptr, cd.y, cd.mean, cd.invstd, e->params[cd.p_g], e->grads[cd.p_g],
                                                                        e->grads[cd.p_b], cd.rows, cd.d.out_c, e->bwd_part, e->bwd_part_floats, cd.c1c2, e->dpart, stream));
                {
                    ConvL* cp = &cd;
                    auto side_part = [e, cp, gA, x_in](hipStream_t run) -> int {
                        ConvL& c = *cp;
                        e->pending_flops = conv_flops(c) * (1.0 + (double)c.d.in_c / c.d.out_c);
                        e->pending_bytes = conv_out_bytes(e, c) + 3.0 * conv_in_bytes(e, c);
                        PROF(e, RPE_PROF_CONV_WGRAD, run, rpe_conv1x1_wgrad_folded(&c.d, e->dtype, gA, x_in, e->params[c.p_w], e->params[c.p_g], c.invstd, c.mean, c.c1c2,
                                                                                  e->grads[c.p_w], e->wfold_scratch, e->wfold_scratch_bytes, run));
                        return 0;
                    };
                    TRY(to_side(e, stream, side_part));
                }
                e->pending_bytes = 0;
                PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_bwd_fold_conv1x1(e->dtype, cd.d.out_c, cd.d.in_c, fwd_weight(e, cd), cd.wd, e->params[cd.p_g], cd.invstd, cd.mean,
                                                                          cd.c1c2, e->w_kcat, e->fold_bias, e->fold_scratch, e->fold_scratch_bytes, stream));
                e->pending_flops = conv_flops(cd) * (1.0 + (double)cd.d.in_c / cd.d.out_c);
                e->pending_bytes = conv_out_bytes(e, cd) + conv_in_bytes(e, cd) * 2.0;
                PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv1x1_dgrad_kcat(&cd.d, e->dtype, gA, x_in, e->w_kcat, e->fold_bias, e->G[0], nullptr, stream));
            } else {
                TRY(bn_back(e, cd, gA, 0, cd.dy, nullptr, stream));          // no ReLU on the projection shortcut
                TRY(wgrad(e, cd, x_in, cd.dy, stream));
                e->pending_flops = conv_flops(cd);
                if (sub_addend) {
                    e->pending_bytes = conv_out_bytes(e, cd) + conv_in_bytes(e, cd) * 0.25;   // dy -> the even pixels of dx
                    PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv1x1s2_dgrad_compact(&cd.d, e->dtype, cd.dy, cd.wd, e->G[0], stream));
                } else {
                    e->pending_bytes = conv_out_bytes(e, cd) + conv_in_bytes(e, cd) * (hook_in ? 2.0 : 1.0);
                    PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad(&cd.d, e->dtype, cd.dy, cd.wd, e->G[0], hook_in, stream));
                }
            }
        }
        static const bool use_mask = getenv("RPE_NO_RELU_MASK") == nullptr;
        if (fold_c1) {
            e->pending_bytes = 0;
            PROF(e, RPE_PROF_BN_BWD, stream, rpe_bn_bwd_fold_y_conv1x1(e->dtype, c1.d.out_c, c1.d.in_c, c1.wd, e->params[c1.p_g], c1.invstd, c1.mean, c1.c1c2, e->w_kcat,
                                                                        e->fold_bias, stream));
            rpe_bn_bwd_epilogue ep;
            const rpe_bn_bwd_epilogue* epp = nullptr;
            double extra = 0.0;
            if (bi > 0) {   // dz3 of the previous block: its ReLU mask, bn3's partial sums
                ConvL& p3 = e->convs[e->blocks[bi - 1].c3];
                unsigned char* mk = use_mask ? e->blocks[bi - 1].relu_mask : nullptr;
                ep.y = p3.y; ep.a_mask = mk; ep.a_out = mk ? nullptr : p3.a;
                ep.mean = p3.mean; ep.invstd = p3.invstd; ep.scale = nullptr; ep.shift = nullptr;
                ep.stats_part = e->stats_part;
                epp = &ep;
                extra = 1.0 + (mk ? 1.0 / 16 : 1.0);
            }
            e->pending_flops = conv_flops(c1) * 2.0;
            e->pending_bytes = 2.0 * conv_out_bytes(e, c1) + conv_in_bytes(e, c1) * ((sub_addend ? 1.25 : 2.0) + extra);   // dz1, y1; out, shortcut (, y3, mask)
            e->fused_tiles = (int)rpe_conv2d_dgrad_stats_tiles(&c1.d, e->dtype);
            if (sub_addend) PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv1x1_dgrad_kcat_y_sub(&c1.d, e->dtype, c1.dy, c1.y, e->w_kcat, e->fold_bias, gD, shortcut, epp, stream));
            else PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv1x1_dgrad_kcat_y(&c1.d, e->dtype, c1.dy, c1.y, e->w_kcat, e->fold_bias, gD, shortcut, epp, stream));
        } else
        if (bi > 0) {
            const Block& pb = e->blocks[bi - 1];
            const bool pb_y3f = pb.gram && pb.relu_mask && !e->y3_keep;
            const ConvL& p3 = e->convs[pb.c3];
            e->blocks[bi - 1].t_ready = t_here;
            TRY(dgrad_fused(e, c1, c1.dy, gD, shortcut, &e->convs[pb.c3], 1, stream, use_mask ? pb.relu_mask : nullptr, pb_y3f,
                            t_here ? e->convs[pb.c2].a : nullptr, p3.d.in_c, t_here ? pb.dzt_a : nullptr, sub_addend));   // dz3 of the previous block (+ its dz3^T a2)
        } else if (sub_addend) {
            PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad_sub(&c1.d, e->dtype, c1.dy, c1.wd, gD, shortcut, stream));
        } else {
            PROF(e, RPE_PROF_CONV_DGRAD, stream, rpe_conv2d_dgrad(&c1.d, e->dtype, c1.dy, c1.wd, gD, shortcut, stream));
        }
    }
    e->bwd_next = bi;
    if (join) TRY(join_side(e, (hipStream_t)stream));
    return 0;
}

extern "C" int rpe_resnet50_backward_end(rpe_resnet50_t* e, int use_d_early, void* stream) {
    if (!e || !e->bound || e->bwd_next != -1) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward_end: blocks not finished");
    hipStream_t s = (hipStream_t)stream;
    WalkScope walk(e, true);
    void *g0 = e->d_pool, *g1 = e->convs[0].dy;
    // stem: g0 = gradient wrt maxpool output
    ConvL& st = e->convs[0];
    static const bool unfused = getenv("RPE_STEM_UNFUSED") != nullptr;
    if ((use_d_early && !e->aux_dout) || unfused || e->hook_grad[0]) {
        // dense early-feature gradient supplied by the caller (rpe_resnet50_early_grad): pool backward, then BN backward
        if (use_d_early && e->aux_dout) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward_end: the unfused stem backward (RPE_STEM_UNFUSED, a hook on conv1) needs the dense early gradient");
        PROF(e, RPE_PROF_OTHER, stream, rpe_maxpool3x3s2_bwd(e->dtype, g0, e->pool_idx, use_d_early ? e->early_grad : nullptr, g1, e->B, st.Ho, st.Wo, 64, stream));
        TRY(bn_back(e, st, g1, 1, g1, nullptr, stream));
        if (e->hook_grad[0]) TRY(rpe_tensor_add(e->dtype, g1, e->hook_grad[0], st.rows * 64, stream));   // + the gradient of conv1's hooked raw output
    } else {
        const bool aux = use_d_early != 0;
        e->pending_bytes = conv_out_bytes(e, st) * 3.0 + 2.0 * (double)e->B * (st.Ho / 2) * (st.Wo / 2) * 64 * (e->esz + 1);   // y twice -> dy; pooled gradient + index twice
        PROF(e, RPE_PROF_BN_BWD, stream, rpe_stem_bwd(e->dtype, g0, e->pool_idx, st.y, st.scale, st.shift, st.mean, st.invstd, e->params[st.p_g],
                                                      aux ? e->aux_dout : nullptr, e->aux_ld, aux ? e->aux_df : nullptr, aux ? e->aux_idx : nullptr,
                                                      aux ? e->aux_w : nullptr, e->grads[st.p_g], e->grads[st.p_b], g1, e->B, st.Ho, st.Wo,
                                                      e->bwd_part, e->bwd_part_floats, e->c1c2, e->dpart, stream));
    }
    e->aux_dout = nullptr;
    for (int i = 0; i < 4; ++i) e->hook_grad[i] = nullptr;
    if (hipError_t he = hipMemsetAsync(e->stem_dw, 0, 64 * 256 * 4, s)) return rpe_set_error_hip(he, __FILE__, __LINE__);   // (the 8th kernel row stays zero)
    if (e->main_slab) PROF(e, RPE_PROF_CONV_WGRAD, stream, rpe_stem_conv_wgrad_det(e->dtype, e->x4, g1, e->stem_dw, e->B, e->H, e->W, e->main_slab, e->main_slab_bytes, stream));
    else PROF(e, RPE_PROF_CONV_WGRAD, stream, rpe_stem_conv_wgrad(e->dtype, e->x4, g1, e->stem_dw, e->B, e->H, e->W, stream));
    TRY(rpe_unpack_stem_grad(e->stem_dw, e->grads[st.p_w], stream));
    TRY(join_side(e, s));
    e->bwd_next = -2;
    return 0;
}

extern "C" int rpe_resnet50_set_aux_head(rpe_resnet50_t* e, const float* w, const float* bias, const float* depth_feat, float* out, long ld_out, float* raw,
                                         unsigned char* idx) {
    if (!e) return rpe_set_error(RPE_ERR_STATE, "resnet50_set_aux_head: null engine");
    if (w && (!bias || !out || !raw || !idx || ld_out < (long)(e->convs[0].Ho / 2) * (e->convs[0].Wo / 2)))
        return rpe_set_error(RPE_ERR_SHAPE, "resnet50_set_aux_head: bias, the output columns (row pitch >= (H/4)(W/4)), raw and idx are required");
    e->aux_fwd.w = w; e->aux_fwd.bias = bias; e->aux_fwd.depth_feat = depth_feat; e->aux_fwd.out = out; e->aux_fwd.ld = ld_out; e->aux_fwd.raw = raw; e->aux_fwd.idx = idx;
    return 0;
}

extern "C" int rpe_resnet50_aux_head_bwd(rpe_resnet50_t* e, const float* dout, long ld_dout, const float* w, const float* depth_feat, const float* raw,
                                         const unsigned char* idx, float* dw, float* dbias, float* d_depth_feat, float* workspace, long workspace_floats,
                                         void* stream) {
    if (!e || !e->bound || !e->fwd_done) return rpe_set_error(RPE_ERR_STATE, "resnet50_aux_head_bwd: no training-mode forward to differentiate");
    const ConvL& st = e->convs[0];
    return rpe_aux_head_bwd_det_y(e->dtype, dout, ld_dout, st.y, st.scale, st.shift, w, depth_feat, raw, idx, dw, dbias, d_depth_feat, e->B, st.Ho, st.Wo, workspace,
                                  workspace_floats, stream);
}

extern "C" int rpe_resnet50_side_stream_info(const rpe_resnet50_t* e, int* candidates, int* concurrent) {
    if (!e || !candidates || !concurrent) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_side_stream_info: null argument");
    *candidates = e->side_tries; *concurrent = e->side_concurrent;
    return 0;
}

extern "C" int rpe_resnet50_set_aux_grad(rpe_resnet50_t* e, const float* aux_dout, long aux_ld, const float* aux_depth_feat,
                                         const unsigned char* aux_idx, const float* aux_w) {
    if (!e) return rpe_set_error(RPE_ERR_STATE, "resnet50_set_aux_grad: null engine");
    if (aux_dout && (!aux_idx || !aux_w || aux_ld <= 0)) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_set_aux_grad: winner indices, weight and row pitch are required");
    e->aux_dout = aux_dout; e->aux_ld = aux_ld; e->aux_df = aux_depth_feat; e->aux_idx = aux_idx; e->aux_w = aux_w;
    return 0;
}

extern "C" int rpe_resnet50_set_hook_grad(rpe_resnet50_t* e, int layer, const void* dense_grad) {
    if (!e || layer < 0 || layer > 3) return rpe_set_error(RPE_ERR_SHAPE, "resnet50_set_hook_grad: layer 0 (conv1's raw output) or 1..3 (layer outputs)");
    e->hook_grad[layer] = dense_grad;
    return 0;
}

extern "C" int rpe_resnet50_set_stem_raw(rpe_resnet50_t* e, int on) {
    if (!e) return rpe_set_error(RPE_ERR_STATE, "resnet50_set_stem_raw: null engine");
    if (e->stem_raw != (on != 0)) { e->stem_raw = on != 0; if (e->pack_state == 2) e->pack_state = 0; }   // the inference copy of conv1's weight changes
    return 0;
}

// see include/rpe_hip.h: the replaced fc's weight / bias gradient, nothing else
extern "C" int rpe_resnet50_backward_frozen(rpe_resnet50_t* e, const float* d_features, long ld_d_features, void* stream) {
    if (!e || !e->bound) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward_frozen: engine not bound");
    if (!e->fwd_done) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward_frozen: no training-mode forward to differentiate");
    const int np = (int)e->pnames.size();
    if (!d_features || !e->grads[np - 2] || !e->grads[np - 1]) return rpe_set_error(RPE_ERR_STATE, "resnet50_backward_frozen: fc gradient tensors were not bound");
    hipStream_t s = (hipStream_t)stream;
    float* dWfc = e->grads[np - 2];
    if (e->main_slab) {
        TRY(rpe_linear_wgrad_det(RPE_F32, d_features, (int)ld_d_features, e->pooled, e->feat, dWfc, e->feat, e->B, e->latent, e->feat, 0, e->main_slab, e->main_slab_bytes, stream));
    } else {
        HIPTRY(hipMemsetAsync(dWfc, 0, (size_t)e->latent * e->feat * 4, s));
        TRY(rpe_linear_wgrad(RPE_F32, d_features, (int)ld_d_features, e->pooled, e->feat, dWfc, e->feat, e->B, e->latent, e->feat, stream));
    }
    TRY(rpe_colsum(d_features, e->B, e->latent, (int)ld_d_features, e->grads[np - 1], 0, stream));
    e->aux_dout = nullptr;                                    // (an aux head's gradient towards bn1 has nowhere to go)
    for (int i = 0; i < 4; ++i) e->hook_grad[i] = nullptr;
    e->bwd_next = -2;
    return 0;
}

extern "C" int rpe_resnet50_backward(rpe_resnet50_t* e, const float* d_features, long ld_d_features, int use_d_early, void* stream) {
    TRY(rpe_resnet50_backward_begin(e, d_features, ld_d_features, stream));
    TRY(rpe_resnet50_backward_blocks(e, 1 << 20, 0, stream));
    return rpe_resnet50_backward_end(e, use_d_early, stream);
}

extern "C" int rpe_resnet50_tensor(const rpe_resnet50_t* e, const char* name, const void** ptr, long* rows, int* channels) {
    if (!e || !e->bound || !name) return rpe_set_error(RPE_ERR_STATE, "resnet50_tensor: engine not bound");
    for (auto& n : e->named)
        if (n.name == name) { *ptr = n.ptr; *rows = n.rows; *channels = n.ch; return 0; }
    return rpe_set_error(RPE_ERR_SHAPE, "resnet50_tensor: unknown tensor name");
}
