// Host side of the C-ABI declared in include/gsttaco.h: context, weight manifest, BN folding and
// MFMA-fragment repacking, HBM workspace, per-phase kernel enqueue and the hipGraph cache.
//
// Call-stack mirrored (reference Model.py:249-255 -> Model.py:145-156):
//   encoder (Taco2.py:12-51) -> style tokens (GST.py:72-109) -> [gst|enc] memory (GST.py:111-124, never
//   materialised) -> decoder loop (Taco2.py:153-228) -> postnet (Taco2.py:131-149,230).
// There is no CPU fallback: every compute entry point needs a gfx950 device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/gsttaco.h"
#include "kernels.h"
#include "manifest.h"
#include "vocoder_common.h"

namespace {

constexpr float kBnEps = 1e-3f;   // tf.keras.layers.BatchNormalization default epsilon

struct PackedLinear {       // skinny-GEMM operand set
    float* wp = nullptr;
    float* bias = nullptr;
    int nkb = 0, ntiles = 0, N = 0;
    int bf16 = 0;           // the pack holds bf16 weights (mixed precision)
};

// One conv / Dense weight that goes through gt_launch_conv_gemm, with the device forms (GSTTACO_CONV_FORM_* bits) prepare_conv_forms
// built for it: a form that was not built is a NULL pointer here.  conv_args turns it into the weight half of a ConvGemmArgs.
struct ConvLayer {
    float* w = nullptr;         // FP32 (always): [taps*Cin, Cout], row stride ldw
    float* scale = nullptr;     // [Cout] or NULL (a Dense: no BatchNorm)
    float* shift = nullptr;     // [Cout] or NULL (a Dense: its bias)
    int taps = 0, cin = 0, cout = 0;
    int ldw = 0;                // row stride of w (0 = cout)
    void* wt_bf16 = nullptr;    // BF16: the transposed bf16 copy (upload_bf16_t), row stride ldk
    int ldk = 0;
    float* wino_u = nullptr;    // WINO2: the F(2,5) transform of w, [6][wino_cin][Cout], for 5-tap layers (gemm_conv.hip)
    float* wino_u4 = nullptr;   // WINO4: F(4,5), [8][wino_cin][Cout]
    int wino_cin = 0;
    void *wino_s = nullptr, *wino_s4 = nullptr;     // WINO_SPLIT: the same U as three bf16 planes [xi][plane][wino_npad][wino_cin] (conv_wino_split.hip)
    void* gemm_s = nullptr;     // GEMM_SPLIT: w as three bf16 planes [plane][wino_npad][taps*Cin] (taps == 1)
    int wino_npad = 0;          // column padding of the planes (wino_s / wino_s4 / gemm_s / wino_h / wino_h4)
    void *wino_h = nullptr, *wino_h4 = nullptr;     // WINO_SPLIT_H: U[:, n] 2^SU[n] as two fp16 planes [xi][plane][wino_npad][wino_cin] (wino_split_h_planes)
    float *wino_hsc = nullptr, *wino_hsc4 = nullptr;    // ... and their epilogue scale [Cout]: scale[n] 2^-(SV + SU[n])
};

// The three launch forms that need their workgroups co-resident and can give up (note_give_up).  The context holds what it still allows
// (gsttaco_ctx::allow); run_cached narrows that to what ONE call may take, keys the graph by it and hands it to the segment's body.
struct LaunchForms {
    bool fuse12 = false;            // both decode LSTM cells in one launch with an in-kernel hand-off (else two launches)
    bool bilstm_persist = false;    // one persistent launch per BiLSTM (else one launch per time step)
    bool persist_decode = false;    // the whole decode loop as ONE persistent launch where it applies (else launches per step)
};

// What a cached graph segment enqueues.  (The values are only names: nothing outside this file sees them.)
enum SegKind : int {
    kSegEncoder = 1, kSegEncoderFork = 9,       // text encoder (gsttaco_encode and Inference_Step share it); with the GST branch forked inside
    kSegGst = 2, kSegPostnet = 4, kSegVocoder = 5,      // the other phases (gsttaco_vocoder and Inference_Step share the vocoder's)
    kSegDecode = 3, kSegDecodeForced = 12,      // value projection + decode loop: gsttaco_decode, gsttaco_decode_forced
    // Inference_Step's middle segment, [GST,] value projection, decode loop, postnet: from mels, with the style given, teacher-forced
    kSegStep = 0, kSegStepStyled = 10, kSegStepForced = 11,
};
// What run_cached needs to know about a kind.  `bilstm`: the segment holds persistent BiLSTM launches and is chained process-wide
// (g_persist_event); `decode`: it holds the decode loop, whose fused / persistent launches are recorded as in flight (g_fused_event).
// No default: the compiler names a new kind that does not answer here.
struct SegTraits { bool bilstm, decode; };
constexpr SegTraits seg_traits(SegKind k) {
    switch (k) {
        case kSegEncoder: case kSegEncoderFork: case kSegVocoder: return {true, false};
        case kSegStep: case kSegDecode: case kSegStepStyled: case kSegStepForced: case kSegDecodeForced: return {false, true};
        case kSegGst: case kSegPostnet: break;
    }
    return {false, false};
}

struct GraphKey {
    SegKind kind;
    int B = 0, Tv = 0, Tref1 = 0, steps = 0, has_mask = 0, has_noise = 0, prof = 0, masked = 0;
    LaunchForms forms;      // what the call that captured it could take (filled in by run_cached; the call sites name the rest)
    auto tie() const { return std::tie(kind, B, Tv, Tref1, steps, has_mask, has_noise, prof, masked, forms.fuse12, forms.bilstm_persist, forms.persist_decode); }
    bool operator<(const GraphKey& o) const { return tie() < o.tie(); }
};

std::string g_create_error;

// The persistent BiLSTM launch needs the 32 members of each of its groups resident on their XCD AT THE SAME TIME, one per CU.
// Two such launches of two contexts on two streams can split an XCD's CUs between them and wait for each other until the bounded
// spins give up (measured: four contexts on four streams did).  Ordinary kernels of other streams only delay a member (they
// drain), so the one thing to exclude is two persistent launches in flight together: every graph segment that contains one is
// launched between a wait on and a record of ONE process-wide event per device, under a mutex -- the segments of all contexts
// form a chain on the GPU, everything else (the decode loops above all) still overlaps freely.
// (Another PROCESS sharing the GPU is not seen here; a give-up is then detected, the call redone is the caller's business
// (gsttaco_synchronize reports it), and the context falls back to one launch per time step: see run_cached.)
std::atomic<int> g_live_contexts{0};
std::mutex g_persist_mu;
std::map<int, hipEvent_t> g_persist_event;      // device -> completion of the last persistent segment enqueued by this process
// The fused decode-LSTM launches need ALL their workgroups co-resident, which one decode loop alone on the GPU has.  The host takes
// them only while the process has one live context -- but a graph full of them may still be RUNNING when a second context is
// created and starts enqueueing.  So the completion of the last segment that contained fused launches is recorded per device, and
// the first thing any OTHER context's segment does is wait for it on the GPU: work in flight is what is guarded, not contexts
// constructed (guarded by g_persist_mu).
struct FusedInFlight { hipEvent_t ev = nullptr; const gsttaco_ctx* owner = nullptr; };
std::map<int, FusedInFlight> g_fused_event;

}  // namespace

struct gsttaco_ctx {
    gsttaco_config cfg{};
    Manifest weights;
    // Decoder sizes below the ones the persistent decode kernels are written for (prenet 256 / 256, attention 128, LSTM 1024 / 1024) are
    // ZERO-PADDED up to them at finalize (pad_decoder): the padded copies of the decoder's tensors, consulted by T() in front of `tensors`
    // (whose shapes stay the caller's: gsttaco_weight_info).  cfg keeps the caller's sizes; P0 .. att below are the padded ones once dec_padded.
    std::map<std::string, HostTensor> padded;
    bool dec_padded = false;
    mutable std::string err;
    bool finalized = false;
    bool use_graph = true;
    bool capturing = false;     // inside hipStreamBeginCapture..EndCapture (event records become external event nodes)

    // derived dims
    int r = 0, steps_max = 0, enc_out = 0, mem_dim = 0, proj_out = 0, conv_c = 0;
    int P0 = 0, P1 = 0, H1 = 0, H2 = 0, att = 0;

    // device memory
    std::vector<void*> allocs;
    hipStream_t cap_stream = nullptr;
    // GSTTACO_GST_FORK=1: the GST branch (six small convolutions + the tail, ~0.25 ms of mostly idle GPU) runs on a side stream beside
    // the text encoder's CONVOLUTIONS and joins in front of its persistent BiLSTM launch (beside THAT launch it cost a millisecond:
    // EXPERIMENTS round 3, item 2b)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool gst_fork = true;        // GSTTACO_GST_FORK (default 1 since round 6): the GST branch forked inside the captured encoder graph
    bool masks_lazy = false;     // the last decode did not write the keep-mask tensor (hashed decisions): gsttaco_debug_randomness regenerates it

    // weights on device
    float* d_emb = nullptr;
    std::vector<ConvLayer> enc_conv, post_conv;
    PackedLinear bilstm[2];
    // lean BiLSTMs (fp32; encoder and vocoder): input halves of both directions hoisted into one GEMM (columns in tile
    // order), recurrent-only packs, hoisted-GEMM output and ping-pong blocked state in the workspace
    struct LeanBiLstm {
        PackedLinear h[2];
        ConvLayer x;                                // the hoisted GEMM: [C, 2*4H] + bias [2*4H] (w == NULL: no lean form)
        float *z = nullptr, *hb[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
        float* ph = nullptr;                        // persistent kernel: [8 groups][3 slots] blocked state of 16 rows, tagged in bit 30
        uint32_t* pflags = nullptr;                 // persistent kernel: [8] member counters (right behind ph)
        int H = 0, C = 0;
    } enc_lean, voc_lean;
    struct RefConv { ConvLayer L; int k = 0, stride = 0; } ref_conv[GSTTACO_MAX_LAYERS];     // GST 2-D layers (taps = k*k): the FP32 form only
    float *gru_w = nullptr, *gru_u = nullptr, *gru_b = nullptr, *dense_w = nullptr, *dense_b = nullptr;
    float *mq_w = nullptr, *mq_b = nullptr, *v_tok = nullptr, *ln_g = nullptr, *ln_b = nullptr;
    PackedLinear prenet0, prenet1, query, val_gst, lstm0, lstm1, proj;
    PackedLinear lstm_x[2], lstm_h[2];   // split packs: input half (critical path) / recurrent half + bias (front-kernel workers)
    float* w_part[2] = {nullptr, nullptr};
    uint32_t* w_err = nullptr;   // device alias of h_err: give-up words of [0] the fused decode-LSTM launch, [1] the persistent BiLSTM, [2] the persistent decode launch
    uint32_t* h_err = nullptr;
    uint32_t gave_up = 0;        // sticky: give-ups seen by a later enqueue and not yet reported by gsttaco_synchronize (bit i = word i of h_err)
    bool announce_warn = false;  // the next compute call leaves `warn` in gsttaco_last_error
    // the launch forms still allowed: GSTTACO_FUSED_LSTM / GSTTACO_BILSTM_PERSIST / GSTTACO_PERSIST_DECODE = 0 or a give-up clear one for good
    LaunchForms allow{true, true, true};
    int persist_rows = 128;      // persistent decode: for batches up to this many rows (GSTTACO_PERSIST_ROWS; 32: the one-group kernel only)
    int persist_slots = 0;       // workgroups of gt_persist_decode_kernel the device holds at once
    uint64_t n_persist_decodes = 0;      // persistent decode launches enqueued (eagerly or into a captured graph)
    float* w_xa2 = nullptr; uint2* w_z0g = nullptr; float* w_hpart = nullptr; uint32_t* w_pctl = nullptr;    // its workspace
    float* w_stash = nullptr;
    int fuse12_slots[3] = {0, 0, 0};    // workgroups of gt_lstm12_kernel / gt_lstm12_mc_kernel fp32 / bf16 the device holds at once (occupancy x CUs)
    bool counted = false;        // this context is included in g_live_contexts
    uint64_t n_persist_enqueued = 0;     // persistent BiLSTM launches enqueued (eagerly or into a captured graph)
    int wino = 4;                // Winograd for the 5-tap Conv1D layers that fill the chip: 4 = F(4,5) where its grid fills the chip and F(2,5)
                                 // otherwise, 2 = F(2,5) only, 0 = implicit GEMM only (GSTTACO_WINO)
    bool wino_x3 = false;        // GSTTACO_WINO_SPLIT=3: the postnet's split kernel with two planes and three products (~2^-16; NOT fp32-accurate)
    bool wino_split_h = true;    // ... and as two fp16 planes x3 where the input is bounded by construction (the postnet layers behind a
                                 // tanh); GSTTACO_WINO_SPLIT=6: x6 everywhere
    bool wino_split = true;      // the Winograd layers' transform-domain GEMMs as split-bf16 x6 on the bf16 matrix pipe, fp32 accuracy
                                 // (conv_wino_split.hip; GSTTACO_WINO_SPLIT=0: the fp32-MFMA Winograd kernel)
    int enc_wino = 2;            // the text encoder's five-tap layers behind the token gather on the split-bf16 Winograd kernel (GSTTACO_ENC_WINO)
    bool pad_dec = true;         // a decoder smaller than the reference's is zero-padded up to it (pad_decoder; GSTTACO_PAD_DECODER=0: its own sizes)
    uint32_t* w_arrive = nullptr;    // [steps_max][8 x 32] arrival counters of the fused launch, zeroed at the start of every decode
    int debug_drop_member = -1;  // fault injection (gsttaco_debug_raise_handoff_error): a member of the next persistent launches never shows up
    mutable std::string warn;    // last warning (a recovered condition): readable through gsttaco_last_error until the next error
    bool lean = true;            // lean_body.h kernels for the decode shapes they cover (GSTTACO_LEAN=0: general kernels only)

    float *pw0 = nullptr, *pb0 = nullptr, *pw1 = nullptr, *pb1 = nullptr, *pwq = nullptr, *pbq = nullptr;  // plain layouts (fused front)
    bool fused_front = true;
    int front_mode = 2;         // GSTTACO_FUSED_FRONT: 0 = four-kernel front end, 1 = the general fused kernel, 2 = + the lean utterance path
    PackedLinear proj_z;        // projection columns | padding to a tile | (Wp_last . W0) columns: prenet 0 rides in the projection launch
    int z_col0 = 0;
    float* w_z0 = nullptr;
    // Teacher forcing (gsttaco_decode_forced / gsttaco_inference_step_forced): the consumed frames [S][B][mel] and every step's prenet-0
    // pre-activations [S][B][P0], allocated by the first forced call (ensure_forced); z0_dense = the plain pw0 / pb0 as a conv/GEMM layer
    float *w_teach = nullptr, *w_zf = nullptr;
    // MCD-DTW (gsttaco_mel_dtw): both sides' features, allocated by the first call; the back-pointers by the first call that asks for
    // the path; one DCT-II basis per n_ceps seen (ensure_dtw)
    double *w_dtw_fx = nullptr, *w_dtw_fy = nullptr;
    uint8_t* w_dtw_bp = nullptr;
    std::map<int, double*> dtw_basis;
    // The style map (gsttaco_style_map): the per-row partial sums [5 * GT_TSNE_MAX_N + 1], allocated by the first call
    double* w_tsne = nullptr;
    // The neural vocoder (gsttaco_melgan_*): its own manifest, the plan whose stages hold the device operands once finalized, and the
    // ping-pong activations for the capacity
    struct Melgan {
        bool configured = false, finalized = false;
        gsttaco_melgan_config cfg{};
        MgPlan plan{};
        Manifest man;
        float* ws[2] = {nullptr, nullptr};
    } mg;
    // The flow vocoder (gsttaco_waveglow_*): its own manifest, the plan that holds the device operands once finalized, and the
    // workspace for the capacity (spect, the two hid, out, audio)
    struct Waveglow {
        bool configured = false, finalized = false;
        gsttaco_waveglow_config cfg{};
        WgPlan plan{};
        Manifest man;
        float *spect = nullptr, *hid[2] = {nullptr, nullptr}, *out = nullptr, *audio = nullptr;
    } wg;
    // The HiFi-GAN vocoder (gsttaco_hifigan_*): its own manifest, the plan whose launches hold the device operands once finalized, and
    // the four activation buffers for the capacity
    struct Hifigan {
        bool configured = false, finalized = false;
        gsttaco_hifigan_config cfg{};
        HgPlan plan{};
        Manifest man;
        float* ws[GT_HG_BUFS] = {nullptr, nullptr, nullptr, nullptr};
        int operands = GSTTACO_HIFIGAN_F32;     // gsttaco_hifigan_set_operands: the form finalize packs for (the plan's copy is what runs)
    } hg;
    // Resampling (gsttaco_resample): the tables of up to GT_RS_MAX_PAIRS rate pairs, least recently used evicted (ensure_resample_pair).
    // A slot's device memory and pinned host image are allocated at its first use and reused by the pairs that follow in it; `uploaded`
    // is recorded behind a slot's upload, and waited for before its host image is rewritten.
    struct ResampleSlot {
        int sr_in = 0, sr_out = 0;          // 0: the slot has never held a pair
        uint64_t last_use = 0;
        double* d_time = nullptr;           // [max_wav_samples]
        double2* d_table = nullptr;         // [GT_RS_NWIN] {win, delta}
        double* h_image = nullptr;          // pinned: the register, then the table
        hipEvent_t uploaded = nullptr;
        double scale = 0.0;
        int step = 0;
    };
    ResampleSlot rs_slot[GT_RS_MAX_PAIRS];
    std::vector<double> rs_window;          // the un-gained kaiser_best table, built by the first call
    uint64_t rs_clock = 0;
    ConvLayer z0_dense;
    ConvLayer val_enc;          // the [enc] rows of the Value kernel (+ its bias when no GST row bias carries it)
    float *att_v = nullptr, *att_sb = nullptr;
    float *loc_cw = nullptr, *loc_cb = nullptr, *loc_dw = nullptr, *loc_db = nullptr, *att_bias = nullptr;   // LSA extension
    float* loc_pack = nullptr;          // the same as the fused front end's LDS image (kernels.h LsaPack)
    float* w_lsa_state = nullptr;

    // CBHG vocoder
    std::vector<ConvLayer> voc_bank, voc_proj;
    ConvLayer voc_pd, voc_hin, voc_dense;       // Dense layers (taps 1); voc_pd / voc_hin: w == NULL where the model has none
    std::vector<ConvLayer> voc_hw;              // per highway layer: [S, 2S] = [relu | sigmoid], bias [2S]
    PackedLinear voc_bilstm[2];
    float *w_vbank = nullptr, *w_vbuf[3] = {nullptr, nullptr, nullptr}, *w_vz = nullptr, *w_vrnn = nullptr, *w_vc = nullptr,
          *w_spec = nullptr;

    struct DbgConv { ConvLayer L; int forms; };
    std::vector<DbgConv> dbg_conv;      // gsttaco_debug_conv_prepare's weights (device memory in allocs, freed at destroy)

    // audio front / back end, initialised on first use
    bool audio_ready = false;
    int n_fft = 0;
    std::vector<float> h_mel_basis;
    float *a_window = nullptr, *a_mel_basis = nullptr;
    float2* a_twiddle = nullptr;
    int32_t *a_band_lo = nullptr, *a_band_hi = nullptr, *a_bounds = nullptr;
    double* a_mse = nullptr;
    int a_ld_mse = 0;
    double* a_win_sq = nullptr;
    float *gl_mag = nullptr, *gl_frm[2] = {nullptr, nullptr};
    size_t gl_frames_cap = 0;      // B*T frames the Griffin-Lim workspace holds

    // workspace
    int32_t *w_tokens = nullptr, *w_mel_len = nullptr, *w_tok_len = nullptr;
    float *w_mels_in = nullptr, *w_masks = nullptr, *w_noise = nullptr;
    uint64_t* w_seed = nullptr;
    unsigned long long* w_dbg = nullptr;   // [3][16] diagnostic stamps: front, lstm1, lstm2 (GSTTACO_STAMPS=1)
    bool stamps = false;
    float *w_act[2] = {nullptr, nullptr}, *w_enc = nullptr, *w_cenc = nullptr, *w_zero = nullptr;
    float *w_gconv[2] = {nullptr, nullptr}, *w_gst = nullptr, *w_rowbias = nullptr, *w_pm = nullptr;
    float *w_gst_attn = nullptr, *w_gst_q = nullptr;    // what the tail exports beside w_gst: token weights [B, heads, n_tokens], query [B, gst_att]
    float *w_p1 = nullptr, *w_xa = nullptr, *w_q = nullptr, *w_h1[2] = {nullptr, nullptr},
          *w_h2[2] = {nullptr, nullptr}, *w_c1 = nullptr, *w_c2 = nullptr;
    // bf16 mirrors of the blocked decoder activations (kernels.h gt_blk_off_h): mixed precision, batches above 32 rows
    uint16_t *w_xa_h = nullptr, *w_xa2_h = nullptr, *w_h1_h[2] = {nullptr, nullptr}, *w_h2_h[2] = {nullptr, nullptr};
    float *w_pre = nullptr, *w_stop = nullptr, *w_align = nullptr, *w_post[2] = {nullptr, nullptr},
          *w_mel = nullptr;
    size_t zero_floats = 0;

    // graphs: LRU-bounded cache of instantiated executables, one per (kind, shape, flags) key.  A full Inference_Step
    // graph holds ~2 200 kernel nodes; a caller whose shapes vary (the reference's Feeder pads to the batch maximum) would
    // otherwise grow host and device memory without bound.  `graph_capture_after` = n: a key is captured at its n-th use and
    // runs eagerly before (1 = capture at first use; 2 suits variable-shape serving, where most shapes never repeat).
    struct GraphEntry { hipGraphExec_t exec; uint64_t last_use; hipStream_t last_stream; };
    std::map<GraphKey, GraphEntry> graphs;
    std::map<GraphKey, std::pair<int, uint64_t>> graph_seen;     // uses so far (not yet captured), last use
    uint64_t graph_clock = 0;
    int graph_cache_max = 16;
    int graph_capture_after = 1;
    int n_cu = 256;             // compute units of the device (hipDeviceProp_t::multiProcessorCount), queried in ensure_device

    // profiling
    int prof_every = 0;
    // bracketed decode kernels: 0 = LSTM layer 1, 1 = LSTM layer 2, 2 = front (+ workers), 3 = projection (+ workers)
    // 4 = empty bracket (two event nodes back to back): the cost the bracketing itself adds, for calibration
    int prof_count[5] = {0, 0, 0, 0, 0};
    std::vector<hipEvent_t> prof_ev[5];     // pairs (start, stop) per bracketed launch
};

int gt_fail(const gsttaco_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

namespace {

int fail(const gsttaco_ctx* c, int code, const std::string& msg) { return gt_fail(c, code, msg); }

#define HIPCHECK(ctx, expr)                                                                   \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess)                                                                \
            return fail(ctx, GSTTACO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

void add_tensor(gsttaco_ctx* c, const std::string& name, std::vector<int64_t> shape) { c->weights.add(name, std::move(shape)); }

void add_bn(gsttaco_ctx* c, const std::string& prefix, int64_t n) {
    for (const char* f : {"gamma", "beta", "moving_mean", "moving_variance"}) add_tensor(c, prefix + ".bn." + f, {n});
}

// Width of the reference encoder's GRU input: the frequency bins left by the strided convolutions x the last filter count (GST.py:59-62)
int64_t ref_gru_in(const gsttaco_config& g) {
    int freq = g.mel_dim;
    for (int i = 0; i < g.n_ref_conv; ++i) freq = (freq + g.ref_strides[i] - 1) / g.ref_strides[i];
    return (int64_t)freq * g.ref_filters[g.n_ref_conv - 1];
}

// Same names/shapes/order as gst_tacotron_amd/weights.py::manifest.
void build_manifest(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    add_tensor(c, "encoder.embedding", {g.vocab, g.emb});
    int64_t cin = g.emb;
    for (int i = 0; i < g.n_enc_conv; ++i) {
        std::string p = "encoder.conv" + std::to_string(i);
        add_tensor(c, p + ".kernel", {g.enc_kernels[i], cin, g.enc_filters[i]});
        add_bn(c, p, g.enc_filters[i]);
        cin = g.enc_filters[i];
    }
    for (const char* d : {"fwd", "bwd"}) {
        std::string p = std::string("encoder.bilstm.") + d;
        add_tensor(c, p + ".kernel", {cin, 4 * (int64_t)g.enc_rnn});
        add_tensor(c, p + ".recurrent_kernel", {g.enc_rnn, 4 * (int64_t)g.enc_rnn});
        add_tensor(c, p + ".bias", {4 * (int64_t)g.enc_rnn});
    }
    if (g.gst_use) {
        cin = 1;
        for (int i = 0; i < g.n_ref_conv; ++i) {
            std::string p = "gst.ref.conv" + std::to_string(i);
            add_tensor(c, p + ".kernel", {g.ref_kernels[i], g.ref_kernels[i], cin, g.ref_filters[i]});
            add_bn(c, p, g.ref_filters[i]);
            cin = g.ref_filters[i];
        }
        const int64_t gru_in = ref_gru_in(g);
        add_tensor(c, "gst.ref.gru.kernel", {gru_in, 3 * (int64_t)g.ref_rnn});
        add_tensor(c, "gst.ref.gru.recurrent_kernel", {g.ref_rnn, 3 * (int64_t)g.ref_rnn});
        add_tensor(c, "gst.ref.gru.bias", {2, 3 * (int64_t)g.ref_rnn});
        add_tensor(c, "gst.ref.dense.kernel", {g.ref_rnn, g.ref_dense});
        add_tensor(c, "gst.ref.dense.bias", {g.ref_dense});
        add_tensor(c, "gst.tokens", {g.n_tokens, g.token_emb});
        add_tensor(c, "gst.mha.query.kernel", {g.ref_dense, g.gst_att});
        add_tensor(c, "gst.mha.query.bias", {g.gst_att});
        add_tensor(c, "gst.mha.value.kernel", {g.token_emb, g.gst_att});
        add_tensor(c, "gst.mha.value.bias", {g.gst_att});
        add_tensor(c, "gst.mha.ln.gamma", {g.gst_att});
        add_tensor(c, "gst.mha.ln.beta", {g.gst_att});
    }
    cin = g.mel_dim;
    for (int i = 0; i < g.n_prenet; ++i) {
        std::string p = "decoder.prenet" + std::to_string(i);
        add_tensor(c, p + ".kernel", {cin, g.prenet[i]});
        add_tensor(c, p + ".bias", {g.prenet[i]});
        cin = g.prenet[i];
    }
    add_tensor(c, "decoder.attention.query.kernel", {cin, g.att_size});
    add_tensor(c, "decoder.attention.query.bias", {g.att_size});
    add_tensor(c, "decoder.attention.value.kernel", {c->mem_dim, g.att_size});
    add_tensor(c, "decoder.attention.value.bias", {g.att_size});
    if (g.att_type == GSTTACO_ATT_LSA) {      // extension A13 (reference Layers.py:310-321, 335-341)
        add_tensor(c, "decoder.attention.location_conv.kernel", {g.loc_kernel, 1, g.loc_filters});
        add_tensor(c, "decoder.attention.location_conv.bias", {g.loc_filters});
        add_tensor(c, "decoder.attention.location_dense.kernel", {g.loc_filters, g.att_size});
        add_tensor(c, "decoder.attention.location_dense.bias", {g.att_size});
        add_tensor(c, "decoder.attention.bias", {g.att_size});
    } else {
        add_tensor(c, "decoder.attention.v", {g.att_size});
        add_tensor(c, "decoder.attention.score_bias", {});
    }
    cin = cin + g.att_size;
    for (int i = 0; i < g.n_dec_rnn; ++i) {
        std::string p = "decoder.lstm" + std::to_string(i);
        add_tensor(c, p + ".kernel", {cin, 4 * (int64_t)g.dec_rnn[i]});
        add_tensor(c, p + ".recurrent_kernel", {g.dec_rnn[i], 4 * (int64_t)g.dec_rnn[i]});
        add_tensor(c, p + ".bias", {4 * (int64_t)g.dec_rnn[i]});
        cin = g.dec_rnn[i];
    }
    add_tensor(c, "decoder.projection.kernel", {cin + g.att_size, c->proj_out});
    add_tensor(c, "decoder.projection.bias", {c->proj_out});
    cin = g.mel_dim;
    for (int i = 0; i < g.n_post; ++i) {
        std::string p = "postnet.conv" + std::to_string(i);
        add_tensor(c, p + ".kernel", {g.post_kernels[i], cin, g.post_filters[i]});
        add_bn(c, p, g.post_filters[i]);
        cin = g.post_filters[i];
    }
    if (g.voc_use) {        // CBHG vocoder (reference Taco2.py:234-260, 285-424), same order as weights.py::manifest
        for (int i = 0; i < g.bank_count; ++i) {
            std::string p = "vocoder.convbank" + std::to_string(i);
            add_tensor(c, p + ".kernel", {i + 1, g.mel_dim, g.bank_filters});
            add_bn(c, p, g.bank_filters);
        }
        cin = (int64_t)g.bank_count * g.bank_filters;
        for (int i = 0; i < g.n_voc_proj; ++i) {
            std::string p = "vocoder.proj" + std::to_string(i);
            add_tensor(c, p + ".kernel", {g.voc_proj_kernels[i], cin, g.voc_proj_filters[i]});
            add_bn(c, p, g.voc_proj_filters[i]);
            cin = g.voc_proj_filters[i];
        }
        if (cin != g.mel_dim) {
            add_tensor(c, "vocoder.proj_dense.kernel", {cin, g.mel_dim});
            add_tensor(c, "vocoder.proj_dense.bias", {g.mel_dim});
        }
        if (g.mel_dim != g.highway_size) {
            add_tensor(c, "vocoder.highway_in.kernel", {g.mel_dim, g.highway_size});
            add_tensor(c, "vocoder.highway_in.bias", {g.highway_size});
        }
        for (int i = 0; i < g.highway_count; ++i)
            for (const char* gt : {"relu", "sigmoid"}) {
                std::string p = "vocoder.highway" + std::to_string(i) + "." + gt;
                add_tensor(c, p + ".kernel", {g.highway_size, g.highway_size});
                add_tensor(c, p + ".bias", {g.highway_size});
            }
        for (const char* d : {"fwd", "bwd"}) {
            std::string p = std::string("vocoder.bilstm.") + d;
            add_tensor(c, p + ".kernel", {g.highway_size, 4 * (int64_t)g.voc_rnn});
            add_tensor(c, p + ".recurrent_kernel", {g.voc_rnn, 4 * (int64_t)g.voc_rnn});
            add_tensor(c, p + ".bias", {4 * (int64_t)g.voc_rnn});
        }
        add_tensor(c, "vocoder.dense.kernel", {2 * (int64_t)g.voc_rnn, g.spec_dim});
        add_tensor(c, "vocoder.dense.bias", {g.spec_dim});
    }
}

const HostTensor& T(const gsttaco_ctx* c, const std::string& name) {
    auto it = c->padded.find(name);
    return it != c->padded.end() ? it->second : c->weights.tensors[c->weights.index.at(name)];
}

// A decoder smaller than the reference's (Taco2.py:61-89 builds every layer from hp_Dict: any prenet / attention / LSTM size) used to leave
// every fast path at once -- the persistent decode kernels, the lean bodies and the fused front end are written for prenet 256 / 256,
// attention 128, LSTM 1024 / 1024 -- and ran 40-65 % SLOWER than the larger reference model (profiles/r05c_other_sizes.txt).  Such a
// model is now embedded in the reference-sized one with zeros, which is exact:
//   * a padded prenet unit has zero weights and bias: relu(0) = 0, times any keep decision = 0; its outgoing rows are zero;
//   * a padded attention channel has query = key = 0 and v = 0 (LSA: no v, tanh(0 + 0 + 0 + 0) = 0): it adds an exact 0 to every score,
//     and its context column is 0 (zero Value column) with zero outgoing rows;
//   * a padded LSTM unit has zero pre-activations: i = f = o = 1/2, c~ = 0, so c stays 0 and h = o tanh(0) = 0 for ever; zero outgoing rows.
// Adding exact zeros changes no sum, so the result is the unpadded model's up to fp32 summation ORDER (the k-blocks regroup): the same
// 5e-5 bar against the float64 oracle (tests/test_gpu_configs.py), not bitwise the unpadded launch path.  Cost: the small model runs at
// the reference model's speed, not faster.  Row / column maps: TF layouts -- Dense kernels [in, out]; LSTM kernels [in, 4 units]
// gate-major (i | f | c~ | o); LSTM 1's input is [prenet | context], the projection's [h2 | context].
// the rule: every size at most the reference's and not all equal to it (gsttaco_create asks too: the Attention.Size the model RUNS at)
bool decoder_pads(const gsttaco_config& g) {
    const int P0 = 256, P1 = 256, A = 128, H1 = 1024, H2 = 1024;
    const int p0 = g.prenet[0], p1 = g.prenet[1], a = g.att_size, h1 = g.dec_rnn[0], h2 = g.dec_rnn[1];     // the caller's
    return !(p0 > P0 || p1 > P1 || a > A || h1 > H1 || h2 > H2 || (p0 == P0 && p1 == P1 && a == A && h1 == H1 && h2 == H2));
}

void pad_decoder(gsttaco_ctx* c) {
    const int P0 = 256, P1 = 256, A = 128, H1 = 1024, H2 = 1024;
    if (c->dec_padded) return;      // (a second finalize after a failed one: the padded tensors and sizes are in place)
    const int p1 = c->cfg.prenet[1], h1 = c->cfg.dec_rnn[0], h2 = c->cfg.dec_rnn[1];     // the caller's
    if (!c->pad_dec || !decoder_pads(c->cfg)) return;
    // dst[rmap(r)][cmap(cc)] = src[r][cc]
    auto embed = [&](const std::string& name, int rows_out, int cols_out, auto rmap, auto cmap) {
        const HostTensor& src = c->weights.tensors[c->weights.index.at(name)];
        const int rows = src.shape.size() == 2 ? (int)src.shape[0] : 1, cols = (int)src.shape.back();
        HostTensor t;
        t.name = name; t.loaded = true;
        t.shape = src.shape.size() == 2 ? std::vector<int64_t>{rows_out, cols_out} : std::vector<int64_t>{cols_out};
        t.data.assign((size_t)rows_out * cols_out, 0.f);
        for (int r = 0; r < rows; ++r)
            for (int cc = 0; cc < cols; ++cc) t.data[(size_t)rmap(r) * cols_out + cmap(cc)] = src.data[(size_t)r * cols + cc];
        c->padded[name] = std::move(t);
    };
    auto id = [](int i) { return i; };
    auto gate = [](int h, int H) { return [h, H](int cc) { return (cc / h) * H + cc % h; }; };        // gate-major columns
    auto cat = [](int n, int N) { return [n, N](int r) { return r < n ? r : N + (r - n); }; };        // [first | second] rows
    const int mel = c->cfg.mel_dim;
    embed("decoder.prenet0.kernel", mel, P0, id, id);
    embed("decoder.prenet0.bias", 1, P0, id, id);
    embed("decoder.prenet1.kernel", P0, P1, id, id);
    embed("decoder.prenet1.bias", 1, P1, id, id);
    embed("decoder.attention.query.kernel", P1, A, id, id);
    embed("decoder.attention.query.bias", 1, A, id, id);
    embed("decoder.attention.value.kernel", c->mem_dim, A, id, id);
    embed("decoder.attention.value.bias", 1, A, id, id);
    if (c->cfg.att_type == GSTTACO_ATT_LSA) {
        embed("decoder.attention.location_dense.kernel", c->cfg.loc_filters, A, id, id);
        embed("decoder.attention.location_dense.bias", 1, A, id, id);
        embed("decoder.attention.bias", 1, A, id, id);
    } else {
        embed("decoder.attention.v", 1, A, id, id);
    }
    embed("decoder.lstm0.kernel", P1 + A, 4 * H1, cat(p1, P1), gate(h1, H1));
    embed("decoder.lstm0.recurrent_kernel", H1, 4 * H1, id, gate(h1, H1));
    embed("decoder.lstm0.bias", 1, 4 * H1, id, gate(h1, H1));
    embed("decoder.lstm1.kernel", H1, 4 * H2, id, gate(h2, H2));
    embed("decoder.lstm1.recurrent_kernel", H2, 4 * H2, id, gate(h2, H2));
    embed("decoder.lstm1.bias", 1, 4 * H2, id, gate(h2, H2));
    embed("decoder.projection.kernel", H2 + A, c->proj_out, cat(h2, H2), id);
    c->P0 = P0; c->P1 = P1; c->att = A; c->H1 = H1; c->H2 = H2;
    c->dec_padded = true;
}

int dev_alloc(gsttaco_ctx* c, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    HIPCHECK(c, hipMalloc(p, bytes));
    c->allocs.push_back(*p);
    return 0;
}

int upload(gsttaco_ctx* c, float** dst, const float* src, size_t n) {
    int rc = dev_alloc(c, (void**)dst, n * sizeof(float));
    if (rc) return rc;
    HIPCHECK(c, hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// float -> bf16 bits, round to nearest even (what v_cvt_pk_bf16_f32 does for finite values)
inline uint16_t bf16_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// The bf16 TRANSPOSED copy [ceil(N/256)*256][ldk] (k contiguous, zero padded, ldk = ceil(K/64)*64) of a conv-GEMM weight
// [K, N] (row stride ldw)
int upload_bf16_t(gsttaco_ctx* c, const float* host_w, int K, int N, int ldw, void** dst, int* ldk_out) {
    const int ldk = (K + 63) / 64 * 64, npad = (N + 255) / 256 * 256;     // (column blocks of up to 256: gt_conv5_bf16_kernel)
    std::vector<uint16_t> t((size_t)npad * ldk, 0);
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) t[(size_t)n * ldk + k] = bf16_bits(host_w[(size_t)k * ldw + n]);
    int rc = dev_alloc(c, dst, t.size() * sizeof(uint16_t));
    if (rc) return rc;
    HIPCHECK(c, hipMemcpy(*dst, t.data(), t.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    *ldk_out = ldk;
    return 0;
}
// Fold inference BatchNorm into y = x*scale + shift (Appendix A.4).
void fold_bn(const gsttaco_ctx* c, const std::string& prefix, std::vector<float>& scale, std::vector<float>& shift) {
    const auto& g = T(c, prefix + ".bn.gamma").data;
    const auto& b = T(c, prefix + ".bn.beta").data;
    const auto& m = T(c, prefix + ".bn.moving_mean").data;
    const auto& v = T(c, prefix + ".bn.moving_variance").data;
    scale.resize(g.size());
    shift.resize(g.size());
    for (size_t i = 0; i < g.size(); ++i) {
        const double s = (double)g[i] / std::sqrt((double)v[i] + (double)kBnEps);
        scale[i] = (float)s;
        shift[i] = (float)((double)b[i] - (double)m[i] * s);
    }
}

// Pack rows of (possibly several row-concatenated) [K_i, ncols] matrices into MFMA 16x16x4 B-fragment
// order: out[((tile*nkb + kb)*64 + lane)*4 + s] = W[kb*16 + 4*(lane>>4) + s][colmap(tile, lane&15)].
// lstm_units > 0: tile-local column g*4+u maps to source column g*H + tile*4 + u (gate-major Keras
// layout i,f,c,o -> unit-major tiles so a workgroup owns whole hidden units).
int pack_linear(gsttaco_ctx* c, PackedLinear* out, const std::vector<std::pair<const float*, int>>& mats,
                int ncols, const float* bias, int lstm_units, bool allow_bf16 = true) {
    int K = 0;
    for (auto& m : mats) {
        if (m.second % 16) return fail(c, GSTTACO_E_INVALID, "skinny GEMM segment length must be a multiple of 16");
        K += m.second;
    }
    const int nkb = K / 16;
    const int ntiles = lstm_units > 0 ? (lstm_units + 3) / 4 : (ncols + 15) / 16;
    std::vector<float> wp((size_t)ntiles * nkb * 256, 0.f), bp((size_t)ntiles * 16, 0.f);
    auto colmap = [&](int tile, int cl) -> int {
        if (lstm_units > 0) {
            const int g = cl >> 2, u = tile * 4 + (cl & 3);
            return u < lstm_units ? g * lstm_units + u : -1;
        }
        const int col = tile * 16 + cl;
        return col < ncols ? col : -1;
    };
    std::vector<const float*> rowptr(K);
    {
        int k = 0;
        for (auto& m : mats)
            for (int i = 0; i < m.second; ++i) rowptr[k++] = m.first + (size_t)i * ncols;
    }
    for (int tile = 0; tile < ntiles; ++tile) {
        for (int cl = 0; cl < 16; ++cl) {
            const int sc = colmap(tile, cl);
            if (sc >= 0 && bias) bp[(size_t)tile * 16 + cl] = bias[sc];
        }
        for (int kb = 0; kb < nkb; ++kb)
            for (int lane = 0; lane < 64; ++lane) {
                const int sc = colmap(tile, lane & 15);
                if (sc < 0) continue;
                for (int s = 0; s < 4; ++s) {
                    const int k = kb * 16 + 4 * (lane >> 4) + s;
                    wp[(((size_t)tile * nkb + kb) * 64 + lane) * 4 + s] = rowptr[k][sc];
                }
            }
    }
    out->nkb = nkb;
    out->ntiles = ntiles;
    out->N = lstm_units > 0 ? lstm_units : ncols;
    int rc = 0;
    out->bf16 = (c->cfg.mixed_precision && allow_bf16) ? 1 : 0;
    if (out->bf16) {
        // bf16 pack [tile][32-k block][lane][8]: slot i of lane (col = lane&15, q = lane>>4) holds
        // k = 32 j + 16 (i>>2) + 4 q + (i&3) -- the order in which the step kernels meet the activations (skinny_body.h)
        const int nkb32 = (nkb + 1) / 2;
        std::vector<uint16_t> wq((size_t)ntiles * nkb32 * 64 * 8, 0);
        for (int tile = 0; tile < ntiles; ++tile)
            for (int j = 0; j < nkb32; ++j)
                for (int lane = 0; lane < 64; ++lane) {
                    const int sc = colmap(tile, lane & 15);
                    if (sc < 0) continue;
                    for (int i = 0; i < 8; ++i) {
                        const int k = 32 * j + 16 * (i >> 2) + 4 * (lane >> 4) + (i & 3);
                        if (k < K) wq[(((size_t)tile * nkb32 + j) * 64 + lane) * 8 + i] = bf16_bits(rowptr[k][sc]);
                    }
                }
        void* d = nullptr;
        if ((rc = dev_alloc(c, &d, wq.size() * sizeof(uint16_t)))) return rc;
        HIPCHECK(c, hipMemcpy(d, wq.data(), wq.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        out->wp = reinterpret_cast<float*>(d);
    } else {
        rc = upload(c, &out->wp, wp.data(), wp.size());
    }
    if (rc) return rc;
    return upload(c, &out->bias, bp.data(), bp.size());
}

// Split-bf16 planes of the Winograd-domain weights (conv_wino_split.hip): u = hi + mid + lo, each a bf16 rounded to nearest even from
// what the planes before it left of the FLOAT64 transform (24 significand bits in all); layout [xi][plane][npad columns][wino_cin]
// with k contiguous -- a B fragment of the bf16 MFMA is 8 consecutive k of one column.  Padding columns / channels are zero.
int upload_wino_split(gsttaco_ctx* c, void** dst, const std::vector<double>& u, int al, int cin, int wino_cin, int cout, int npad) {
    std::vector<uint16_t> planes((size_t)al * 3 * npad * wino_cin, 0);
    auto bf = [](double v, uint16_t* bits) {       // rne(v) as bf16; returns the value it represents
        const uint16_t b = bf16_bits((float)v);
        *bits = b;
        const uint32_t w = (uint32_t)b << 16;
        float f;
        memcpy(&f, &w, 4);
        return (double)f;
    };
    for (int xi = 0; xi < al; ++xi)
        for (int k = 0; k < cin; ++k)
            for (int n = 0; n < cout; ++n) {
                double v = u[((size_t)xi * cin + k) * cout + n];
                for (int p = 0; p < 3; ++p) {
                    uint16_t bits;
                    v -= bf(v, &bits);
                    planes[(((size_t)xi * 3 + p) * npad + n) * wino_cin + k] = bits;
                }
            }
    int rc = dev_alloc(c, dst, planes.size() * 2);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpy(*dst, planes.data(), planes.size() * 2, hipMemcpyHostToDevice));
    return 0;
}

// rne(v) as fp16 bits, subnormals kept (|v| < 65 520), and back
uint16_t f16_bits(double v) {
    const uint16_t sign = std::signbit(v) ? 0x8000u : 0u;
    const double a = std::fabs(v);
    if (a == 0.0) return sign;
    int e;
    (void)std::frexp(a, &e);                            // a in [2^(e-1), 2^e)
    const int E = std::max(e - 1, -14);                 // (below 2^-14: the subnormal quantum 2^-24)
    const int r = (int)std::nearbyint(std::ldexp(a, 10 - E));      // exact scaling, one rounding to nearest even; 1024 <= r <= 2048 when normal
    return (uint16_t)(sign | (uint16_t)(a >= std::ldexp(1.0, -14) ? ((E + 15) << 10) + (r - 1024) : r));
}
double f16_value(uint16_t b) {
    const int ex = (b >> 10) & 31, man = b & 1023;
    const double a = ex ? std::ldexp(1024.0 + man, ex - 25) : std::ldexp((double)man, -24);
    return (b & 0x8000u) ? -a : a;
}

// Two-plane fp16 form of the Winograd-domain weights for the bounded-input kernel (conv_wino_split.hip, mode H3).  Plain host code: no
// device call (gsttaco_debug_wino_h_planes hands it to the CPU tests).  u: the FLOAT64 transform [al][cin][cout].  Per output column n,
// over every xi and k: SU[n] = floor(log2(2^14 / max|u|)) (0 for an all-zero column) brings the column's largest entry into (2^13, 2^14]
// -- fp16's 5-bit exponent then holds hi AND the remainder of every entry that matters as normal numbers; hi = fp16(u 2^SU),
// lo = fp16(u 2^SU - hi) (22 significand bits).  planes: [al][2][npad][wino_cin] fp16 bits, k contiguous, padding zero; su: [cout].
void wino_split_h_planes(const double* u, int al, int cin, int wino_cin, int cout, int npad, uint16_t* planes, int32_t* su) {
    std::fill(planes, planes + (size_t)al * 2 * npad * wino_cin, (uint16_t)0);
    for (int n = 0; n < cout; ++n) {
        double mx = 0.0;
        for (int xi = 0; xi < al; ++xi)
            for (int k = 0; k < cin; ++k) mx = std::max(mx, std::fabs(u[((size_t)xi * cin + k) * cout + n]));
        int sh = 0;
        if (mx > 0.0) {
            int e;
            const double m = std::frexp(mx, &e);                // mx = m 2^e, m in [0.5, 1)
            sh = std::min(14 - e + (m == 0.5 ? 1 : 0), 96);       // (a column below 2^-83 keeps a finite epilogue scale)
        }
        su[n] = sh;
        for (int xi = 0; xi < al; ++xi)
            for (int k = 0; k < cin; ++k) {
                const double v = std::ldexp(u[((size_t)xi * cin + k) * cout + n], sh);
                const uint16_t hi = f16_bits(v);
                planes[(((size_t)xi * 2 + 0) * npad + n) * wino_cin + k] = hi;
                planes[(((size_t)xi * 2 + 1) * npad + n) * wino_cin + k] = f16_bits(v - f16_value(hi));
            }
    }
}

// ... uploaded, with the epilogue scale that undoes both power-of-two factors: sc[n] 2^-(SV + SU[n]) (sc NULL: the power alone)
int upload_wino_split_h(gsttaco_ctx* c, void** dst, float** dst_sc, const std::vector<double>& u, int al, int cin, int wino_cin, int cout, int npad,
                        const float* sc) {
    std::vector<uint16_t> planes((size_t)al * 2 * npad * wino_cin);
    std::vector<int32_t> su(cout);
    wino_split_h_planes(u.data(), al, cin, wino_cin, cout, npad, planes.data(), su.data());
    std::vector<float> hs(cout);
    for (int n = 0; n < cout; ++n) hs[n] = std::ldexp(sc ? sc[n] : 1.f, -(gt_wino5h_sv() + su[n]));
    int rc = dev_alloc(c, dst, planes.size() * 2);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpy(*dst, planes.data(), planes.size() * 2, hipMemcpyHostToDevice));
    return upload(c, dst_sc, hs.data(), hs.size());
}

// the same for a plain GEMM's weights w [K, N] (row stride ldw): [plane][npad][K], k contiguous (conv_wino_split.hip gt_gemm_split_kernel)
int upload_gemm_split(gsttaco_ctx* c, void** dst, const float* w, int K, int N, int ldw, int* npad_out) {
    const int npad = (N + 127) / 128 * 128;
    std::vector<uint16_t> planes((size_t)3 * npad * K, 0);
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) {
            float v = w[(size_t)k * ldw + n];
            for (int p = 0; p < 3; ++p) {
                const uint16_t b = bf16_bits(v);
                const uint32_t u = (uint32_t)b << 16;
                float f;
                memcpy(&f, &u, 4);
                v -= f;                                          // (exact: the remainder of a round-to-nearest to 8 bits)
                planes[((size_t)p * npad + n) * K + k] = b;
            }
        }
    int rc = dev_alloc(c, dst, planes.size() * 2);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpy(*dst, planes.data(), planes.size() * 2, hipMemcpyHostToDevice));
    *npad_out = npad;
    return 0;
}

// The device forms (GSTTACO_CONV_FORM_* bits) of one conv / GEMM weight, host w [taps * cin, ldw] with scale / shift [cout] or NULL:
// finalize and gsttaco_debug_conv_prepare both build them here, and nothing else does.  FP32 is always built.
int prepare_conv_forms(gsttaco_ctx* c, ConvLayer* L, const float* w, int taps, int cin, int cout, int ldw, const float* sc,
                       const float* sh, int forms) {
    L->taps = taps; L->cin = cin; L->cout = cout; L->ldw = ldw == cout ? 0 : ldw;
    const int K = taps * cin;
    int rc = upload(c, &L->w, w, (size_t)K * ldw);
    if (!rc && (forms & GSTTACO_CONV_FORM_BF16)) rc = upload_bf16_t(c, w, K, cout, ldw, &L->wt_bf16, &L->ldk);
    if (!rc && sc) rc = upload(c, &L->scale, sc, cout);
    if (!rc && sh) rc = upload(c, &L->shift, sh, cout);
    const bool split = (forms & GSTTACO_CONV_FORM_WINO_SPLIT) != 0, split_h = (forms & GSTTACO_CONV_FORM_WINO_SPLIT_H) != 0;
    if (!rc && (forms & (GSTTACO_CONV_FORM_WINO2 | GSTTACO_CONV_FORM_WINO4))) {
        if (taps != 5 || cin % 4 || cout % 4) return fail(c, GSTTACO_E_INVALID, "Winograd forms need taps 5, cin and cout multiples of 4");
        const size_t cn = (size_t)cin * cout;
        L->wino_cin = std::max(128, (cin + 63) / 64 * 64);   // zero rows for the padding channels (an even number >= 4 of 32-channel slices)
        L->wino_npad = (cout + 127) / 128 * 128;
        const size_t cnp = (size_t)L->wino_cin * cout;
        std::vector<double> ud(split || split_h ? 8 * cn : 0);
        // U_xi = sum_k G[xi][k] w[k], formed in float64, [xi][wino_cin][cout]
        auto transform = [&](const double (*G)[5], int al, float** dst, void** dst_s, void** dst_h, float** dst_hsc) {
            std::vector<float> u(al * cnp, 0.f);
            for (int xi = 0; xi < al; ++xi)
                for (int ci = 0; ci < cin; ++ci)
                    for (int n = 0; n < cout; ++n) {
                        double acc = 0.0;
                        for (int tap = 0; tap < 5; ++tap) acc += G[xi][tap] * (double)w[((size_t)tap * cin + ci) * ldw + n];
                        u[xi * cnp + (size_t)ci * cout + n] = (float)acc;
                        if (split || split_h) ud[xi * cn + (size_t)ci * cout + n] = acc;
                    }
            int r = upload(c, dst, u.data(), u.size());
            if (!r && split) r = upload_wino_split(c, dst_s, ud, al, cin, L->wino_cin, cout, L->wino_npad);
            if (!r && split_h) r = upload_wino_split_h(c, dst_h, dst_hsc, ud, al, cin, L->wino_cin, cout, L->wino_npad, sc);
            return r;
        };
        if (forms & GSTTACO_CONV_FORM_WINO2) {
            // Cook-Toom F(2,5), points 0, +-1, +-1/2, infinity
            static const double G[6][5] = {{4, 0, 0, 0, 0},
                                           {2.0 / 3, 2.0 / 3, 2.0 / 3, 2.0 / 3, 2.0 / 3},
                                           {2.0 / 3, -2.0 / 3, 2.0 / 3, -2.0 / 3, 2.0 / 3},
                                           {-8.0 / 3, -4.0 / 3, -2.0 / 3, -1.0 / 3, -1.0 / 6},
                                           {-8.0 / 3, 4.0 / 3, -2.0 / 3, 1.0 / 3, -1.0 / 6},
                                           {0, 0, 0, 0, 1}};
            rc = transform(G, 6, &L->wino_u, &L->wino_s, &L->wino_h, &L->wino_hsc);
        }
        if (!rc && (forms & GSTTACO_CONV_FORM_WINO4)) {
            // F(4,5), points 0, +-1, +-1/2, +-2, infinity
            static const double G4[8][5] = {{-1, 0, 0, 0, 0},
                                            {-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9},
                                            {-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9},
                                            {32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45},
                                            {32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45},
                                            {1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45},
                                            {1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45},
                                            {0, 0, 0, 0, 1}};
            rc = transform(G4, 8, &L->wino_u4, &L->wino_s4, &L->wino_h4, &L->wino_hsc4);
        }
    }
    if (!rc && (forms & GSTTACO_CONV_FORM_GEMM_SPLIT)) {
        if (taps != 1) return fail(c, GSTTACO_E_INVALID, "the plain split-bf16 GEMM form needs taps 1");
        rc = upload_gemm_split(c, &L->gemm_s, w, K, cout, ldw, &L->wino_npad);
    }
    return rc;
}

// The weight half of a launch's arguments: `forms` is the call site's statement of which of L's forms this call may use (the
// GSTTACO_CONV_FORM_* bits gsttaco_conv_call::forms carries); a form L does not have stays NULL.  The site then sets what is its own:
// activations, output, geometry, epilogue.
ConvGemmArgs conv_args(const ConvLayer& L, int forms) {
    ConvGemmArgs a{};
    a.w = L.w; a.scale = L.scale; a.shift = L.shift; a.ldw = L.ldw;
    a.Cin = L.cin; a.N = L.cout; a.taps = L.taps;
    if (forms & GSTTACO_CONV_FORM_BF16) { a.wt_bf16 = L.wt_bf16; a.ldk = L.ldk; }
    const bool split = (forms & GSTTACO_CONV_FORM_WINO_SPLIT) != 0;
    const bool split_h = (forms & GSTTACO_CONV_FORM_WINO_SPLIT_H) != 0;     // (taken only by a call that also states a.x_absmax)
    if (forms & GSTTACO_CONV_FORM_WINO2) { a.wino_u = L.wino_u; if (split) a.wino_s = L.wino_s; if (split_h) { a.wino_h = L.wino_h; a.wino_hsc = L.wino_hsc; } }
    if (forms & GSTTACO_CONV_FORM_WINO4) { a.wino_u4 = L.wino_u4; if (split) a.wino_s4 = L.wino_s4; if (split_h) { a.wino_h4 = L.wino_h4; a.wino_hsc4 = L.wino_hsc4; } }
    if (forms & GSTTACO_CONV_FORM_GEMM_SPLIT) a.gemm_s = L.gemm_s;
    if (a.wino_u || a.wino_u4) a.wino_cin = L.wino_cin;
    if (a.wino_s || a.wino_s4 || a.gemm_s || a.wino_h || a.wino_h4) a.wino_npad = L.wino_npad;
    return a;
}

// Postnet layer i reads the output of a tanh (layer i - 1 is one of the first post_tanh layers): |x| <= 1 by construction
inline bool postnet_input_is_tanh(const gsttaco_config& g, int i) { return i >= 1 && i - 1 < g.post_tanh; }

// What every call may use: FP32, and the bf16 copy mixed precision builds (a call with wt_bf16 takes a bf16 kernel: gt_conv_gemm_variant)
constexpr int kFormsPlain = GSTTACO_CONV_FORM_FP32 | GSTTACO_CONV_FORM_BF16;
constexpr int kFormsWino = GSTTACO_CONV_FORM_WINO2 | GSTTACO_CONV_FORM_WINO4 | GSTTACO_CONV_FORM_WINO_SPLIT | GSTTACO_CONV_FORM_WINO_SPLIT_H;

// A Dense (or any taps-1 GEMM) w [K, N], row stride ldw, bias [N] or NULL.  split: the call site may take the plain split-bf16 GEMM
// (GSTTACO_WINO_SPLIT; mixed precision runs the bf16 kernel instead; its k loop needs K % 32 == 0).
int upload_dense(gsttaco_ctx* c, ConvLayer* L, const float* w, int K, int N, int ldw, const float* bias, bool split) {
    int forms = GSTTACO_CONV_FORM_FP32 | (c->cfg.mixed_precision ? GSTTACO_CONV_FORM_BF16 : 0);
    if (split && c->wino_split && !c->cfg.mixed_precision && K % 32 == 0) forms |= GSTTACO_CONV_FORM_GEMM_SPLIT;
    return prepare_conv_forms(c, L, w, 1, K, N, ldw, nullptr, bias, forms);
}

// A Conv1D + BatchNorm layer by manifest name.  wino: the module's call site can pass the Winograd forms of a five-tap layer (mixed
// precision runs the bf16 five-tap kernel instead and builds none); bounded_in: every call of the layer reads the output of a tanh, so
// the two-plane fp16 form is built too (its call site states the bound: enqueue_postnet)
int upload_conv(gsttaco_ctx* c, ConvLayer* L, const std::string& prefix, bool wino, bool bounded_in = false) {
    const HostTensor& k = T(c, prefix + ".kernel");
    const int taps = (int)k.shape[0], cin = (int)k.shape[1], cout = (int)k.shape[2];
    std::vector<float> sc, sh;
    fold_bn(c, prefix, sc, sh);
    int forms = GSTTACO_CONV_FORM_FP32 | (c->cfg.mixed_precision ? GSTTACO_CONV_FORM_BF16 : 0);
    if (wino && !c->cfg.mixed_precision && c->wino != 0 && taps == 5 && cin % 4 == 0 && cout % 4 == 0)
        forms |= GSTTACO_CONV_FORM_WINO2 | (c->wino >= 4 ? GSTTACO_CONV_FORM_WINO4 : 0) | (c->wino_split ? GSTTACO_CONV_FORM_WINO_SPLIT : 0) |
                 (c->wino_split && c->wino_split_h && bounded_in ? GSTTACO_CONV_FORM_WINO_SPLIT_H : 0);
    return prepare_conv_forms(c, L, k.data.data(), taps, cin, cout, cout, sc.data(), sh.data(), forms);
}

// upload tensor `name` as it is
int upload_tensor(gsttaco_ctx* c, float** dst, const std::string& name) {
    const HostTensor& t = T(c, name);
    return upload(c, dst, t.data.data(), t.data.size());
}

int same_pad_before(int n_in, int k, int s, int* out_n) {
    const int out = (n_in + s - 1) / s;
    int total = (out - 1) * s + k - n_in;
    if (total < 0) total = 0;
    if (out_n) *out_n = out;
    return total / 2;      // TF: before = total // 2, after = rest
}


// Records `ev` on `s`.  While `s` is being captured the record is inserted as an explicit event-record
// NODE that depends on everything captured so far (a plain hipEventRecord in capture only expresses a
// cross-stream dependency and records nothing at replay).
int record_event(gsttaco_ctx* c, hipEvent_t ev, hipStream_t s) {
    if (!c->capturing) {
        HIPCHECK(c, hipEventRecord(ev, s));
        return 0;
    }
    hipStreamCaptureStatus st;
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t ndeps = 0;
    HIPCHECK(c, hipStreamGetCaptureInfo_v2(s, &st, &id, &graph, &deps, &ndeps));
    hipGraphNode_t node;
    HIPCHECK(c, hipGraphAddEventRecordNode(&node, graph, deps, ndeps, ev));
    HIPCHECK(c, hipStreamUpdateCaptureDependencies(s, &node, 1, hipStreamSetCaptureDependencies));
    return 0;
}

// ------------------------------------------------------------------------------------------------ lean BiLSTM
// x_t . W_x + b of both directions for all time steps in one GEMM, output columns already in the recurrent kernel's tile
// order (direction d, tile, gate*4 + unit%4), and recurrent-only packs for gt_bilstm_lean_kernel.
// Under Use_Mixed_Precision the hoisted GEMM runs on the bf16 conv-GEMM path and the recurrent packs are bf16: only the persistent
// kernel has that variant, so the lean form is then used exactly when the persistent launch is (lean_bilstm_usable).
int build_lean_bilstm(gsttaco_ctx* c, gsttaco_ctx::LeanBiLstm* L, const std::string& prefix, int H) {
    if (!c->lean || H % 16 || !gt_bilstm_lean_supported(H / 16)) return 0;
    const int C = (int)T(c, prefix + ".fwd.kernel").shape[0];
    std::vector<float> xw((size_t)C * 8 * H), xb((size_t)8 * H);
    int d = 0, rc = 0;
    for (const char* dir : {"fwd", "bwd"}) {
        const std::string p = prefix + "." + dir;
        const HostTensor &k = T(c, p + ".kernel"), &u = T(c, p + ".recurrent_kernel"), &b = T(c, p + ".bias");
        for (int tile = 0; tile < H / 4; ++tile)
            for (int cl = 0; cl < 16; ++cl) {
                const int src = (cl >> 2) * H + tile * 4 + (cl & 3), dst = d * 4 * H + tile * 16 + cl;
                xb[dst] = b.data[src];
                for (int kk = 0; kk < C; ++kk) xw[(size_t)kk * 8 * H + dst] = k.data[(size_t)kk * 4 * H + src];
            }
        if ((rc = pack_linear(c, &L->h[d], {{u.data.data(), (int)u.shape[0]}}, 4 * H, nullptr, H, c->cfg.mixed_precision != 0))) return rc;
        ++d;
    }
    L->H = H; L->C = C;
    return upload_dense(c, &L->x, xw.data(), C, 8 * H, 8 * H, xb.data(), true);
}

int alloc_lean_bilstm(gsttaco_ctx* c, gsttaco_ctx::LeanBiLstm* L, size_t B, size_t Tmax) {
    if (!L->x.w) return 0;
    int rc = 0;
    if ((rc = dev_alloc(c, (void**)&L->z, B * Tmax * 8 * L->H * sizeof(float)))) return rc;
    for (int d = 0; d < 2; ++d)
        for (int q = 0; q < 2; ++q)
            if ((rc = dev_alloc(c, (void**)&L->hb[d][q], ((B + 15) / 16) * 16 * L->H * sizeof(float)))) return rc;
    if (gt_bilstm_persist_supported(L->H, 1, c->n_cu)) {        // used for calls of up to 64 utterances (8 groups)
        // [8 groups][3 slots] of tagged state + the 8 member counters right behind it (one zero-fill per launch covers both)
        if ((rc = dev_alloc(c, (void**)&L->ph, ((size_t)8 * 3 * 16 * L->H + 8) * sizeof(float)))) return rc;
        L->pflags = reinterpret_cast<uint32_t*>(L->ph + (size_t)8 * 3 * 16 * L->H);
    }
    return 0;
}

bool lean_bilstm_usable(const gsttaco_ctx* c, const LaunchForms& forms, const gsttaco_ctx::LeanBiLstm& L, int B) {
    if (!L.x.w) return false;
    if (!c->cfg.mixed_precision) return true;
    return L.ph && forms.bilstm_persist && gt_bilstm_persist_supported(L.H, std::min(B, 64), c->n_cu);
}

// x: [B*T, C] rows; cstate: [2, B, H] (zeroed by the caller); out: [B, T, 2H]
// join: an event the stream waits for BEHIND the hoisted GEMM, in front of the recurrence (the forked GST branch: the GEMM fills the chip
// for ~80 us and the branch's last small launches finish beside it instead of in front of it)
int enqueue_lean_bilstm(gsttaco_ctx* c, hipStream_t s, const LaunchForms& forms, const gsttaco_ctx::LeanBiLstm& L, const float* x, int B, int Tn, float* cstate,
                        float* out, const int32_t* row_len, hipEvent_t join = nullptr) {
    const int H = L.H, EO = 2 * H, MT = (B + 15) / 16;
    // (round 6: on the bf16 matrix pipe as split-bf16 x6 where the grid allows)
    ConvGemmArgs a = conv_args(L.x, kFormsPlain | GSTTACO_CONV_FORM_GEMM_SPLIT);
    a.x = x; a.out = L.z; a.ldo = 8 * H;
    a.B = B; a.T = Tn; a.act = ACT_NONE;
    HIPCHECK(c, gt_launch_conv_gemm(a, s));
    if (join) HIPCHECK(c, hipStreamWaitEvent(s, join, 0));
    // One persistent launch for the whole sequence, one (direction, 16 utterances) group per XCD (skinny_gemm.hip
    // gt_bilstm_persist_kernel; same arithmetic, bitwise the same outputs); GSTTACO_BILSTM_PERSIST=0 keeps the launch per step.
    if (L.ph && forms.bilstm_persist && gt_bilstm_persist_supported(H, std::min(B, 64), c->n_cu)) {
        // one launch per slab of 64 utterances (8 groups = 2 directions x 4 M-tiles fill the 8 XCDs); the recurrences of
        // different utterances are independent, so the slabs simply follow each other on the stream
        for (int r0 = 0; r0 < B; r0 += 64) {
            const int Bs = std::min(64, B - r0);
            HIPCHECK(c, gt_launch_zero(L.ph, (size_t)8 * 3 * 16 * H + 8, s));        // (tagged state: tag 0 = never written; + the member counters)
            BiLstmPersistArgs k{};
            k.wp[0] = L.h[0].wp; k.wp[1] = L.h[1].wp;
            k.ldz = (int64_t)Tn * 8 * H; k.ldo = (int64_t)Tn * EO;
            k.zx = L.z + (size_t)r0 * k.ldz; k.out = out + (size_t)r0 * k.ldo; k.h = L.ph; k.flags = L.pflags;
            k.row_len = row_len ? row_len + r0 : nullptr; k.err = c->w_err + 1;
            k.M = Bs; k.MT = (Bs + 15) / 16; k.H = H; k.T = Tn;
            k.debug_drop_member = c->debug_drop_member;
            HIPCHECK(c, gt_launch_bilstm_persist(k, L.h[0].bf16 != 0, s));
            ++c->n_persist_enqueued;
        }
        return 0;
    }
    for (int d = 0; d < 2; ++d) HIPCHECK(c, gt_launch_zero(L.hb[d][1], (size_t)MT * 16 * H, s));
    for (int t = 0; t < Tn; ++t) {
        BiLstmArgs k{};
        for (int d = 0; d < 2; ++d) {
            const int tt = d == 0 ? t : Tn - 1 - t;
            k.d[d] = BiLstmDir{L.h[d].wp, L.hb[d][(t & 1) ^ 1], L.hb[d][t & 1], cstate + (size_t)d * B * H,
                               L.z + (size_t)tt * 8 * H + (size_t)d * 4 * H, out + (size_t)tt * EO + d * H, tt};
        }
        k.row_len = row_len; k.ldz = (int64_t)Tn * 8 * H; k.ldo = (int64_t)Tn * EO;
        k.M = B; k.MT = MT; k.H = H;
        HIPCHECK(c, gt_launch_bilstm_lean(k, s));
    }
    return 0;
}

// The BiLSTM without the lean form: one launch per time step over the whole [x_t | h_prev] GEMM, both directions in grid.z; h is written
// straight into out.  x: [B, Tn, C]; cstate: [2, B, H] (zeroed by the caller); out: [B, Tn, 2H]; row_len: masked mode, or NULL
int enqueue_bilstm_steps(gsttaco_ctx* c, hipStream_t s, const PackedLinear* pk, const float* x, int B, int Tn, int C, int H, float* cstate,
                         float* out, const int32_t* row_len) {
    const int EO = 2 * H;
    for (int t = 0; t < Tn; ++t) {
        SkinnyArgs a[2];
        for (int d = 0; d < 2; ++d) {
            const int tt = d == 0 ? t : Tn - 1 - t;
            const int tp = d == 0 ? tt - 1 : tt + 1;
            SkinnyArgs& k = a[d];
            memset(&k, 0, sizeof(k));
            k.wp = pk[d].wp; k.bf16 = pk[d].bf16; k.bias = pk[d].bias;
            k.seg[0] = SkinnySeg{x + (size_t)tt * C, (int64_t)Tn * C, C / 16, 0};
            if (t == 0) k.seg[1] = SkinnySeg{c->w_zero, 0, H / 16, 0};
            else k.seg[1] = SkinnySeg{out + (size_t)tp * EO + d * H, (int64_t)Tn * EO, H / 16, 0};
            k.nkb = pk[d].nkb; k.M = B; k.N = H; k.MT = (B + 15) / 16;
            k.c = cstate + (size_t)d * B * H;
            k.h = out + (size_t)tt * EO + d * H; k.ldh = (int64_t)Tn * EO;
            k.row_len = row_len; k.t_index = tt;        // (t_index is read only beside row_len)
        }
        HIPCHECK(c, gt_launch_skinny(EPI_LSTM, a[0], &a[1], pk[0].ntiles, s, TAG_ENC_BILSTM));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ enqueue
int enqueue_gst(gsttaco_ctx* c, hipStream_t s, int B, int Tref1);
bool encoder_rows_path(const gsttaco_ctx* c, int B, int Tv);
ConvGemmArgs encoder_call(const gsttaco_ctx* c, int i, int B, int Tv, bool rows_path);

// gst_Tref1 > 0: the GST branch is forked onto the side stream here and joined in front of the BiLSTM (gsttaco_ctx::gst_fork)
int enqueue_encoder(gsttaco_ctx* c, hipStream_t s, const LaunchForms& forms, int B, int Tv, bool masked, int gst_Tref1 = 0) {
    const int32_t* tlen = masked ? c->w_tok_len : nullptr;      // masked-mode extension
    const gsttaco_config& g = c->cfg;
    const float* x = c->d_emb;
    int cur = 0;
    if (gst_Tref1 > 0) {
        HIPCHECK(c, hipEventRecord(c->ev_fork, s));
        HIPCHECK(c, hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
        const int rg = enqueue_gst(c, c->side_stream, B, gst_Tref1);
        // (joined on the error path too: a side stream left forked would leave an unjoined capture behind -- the capturing stream's
        // EndCapture fails -- or, eagerly, work of this call running on behind the error return)
        const hipError_t ej = hipEventRecord(c->ev_join, c->side_stream);
        if (rg || ej != hipSuccess) {
            if (ej == hipSuccess) (void)hipStreamWaitEvent(s, c->ev_join, 0);
            return rg ? rg : fail(c, GSTTACO_E_HIP, std::string("hipEventRecord(ev_join): ") + hipGetErrorString(ej));
        }
    }
    struct JoinGuard {      // an error return between the fork and the join below still joins the side stream
        gsttaco_ctx* c; hipStream_t s; bool armed;
        ~JoinGuard() { if (armed) (void)hipStreamWaitEvent(s, c->ev_join, 0); }
    } join_guard{c, s, gst_Tref1 > 0};
    const bool rows_path = encoder_rows_path(c, B, Tv);
    if (rows_path) {
        HIPCHECK(c, gt_launch_embed_rows(c->d_emb, c->w_tokens, c->w_act[1], B * Tv, g.emb, s));
        x = c->w_act[1];
    }
    for (int i = 0; i < g.n_enc_conv; ++i) {
        ConvGemmArgs a = encoder_call(c, i, B, Tv, rows_path);
        a.x = x;
        a.out = c->w_act[cur];
        a.row_len = tlen;
        HIPCHECK(c, gt_launch_conv_gemm(a, s));
        x = c->w_act[cur]; cur ^= 1;
    }
    const int H = g.enc_rnn;
    // (joining BEHIND the BiLSTM instead measured 10.83-10.86 against 10.85-10.89 ms per Inference_Step: not worth GST kernels lingering
    // beside a launch that needs its members co-resident)
    const bool lean_enc = lean_bilstm_usable(c, forms, c->enc_lean, B);
    const bool join_here = gst_Tref1 > 0;
    // (the lean BiLSTM joins behind its hoisted GEMM, see enqueue_lean_bilstm; the guard covers its error returns in front of that)
    if (join_here && !lean_enc) { join_guard.armed = false; HIPCHECK(c, hipStreamWaitEvent(s, c->ev_join, 0)); }
    HIPCHECK(c, gt_launch_zero(c->w_cenc, (size_t)2 * B * H, s));
    if (lean_enc) {
        const int rl = enqueue_lean_bilstm(c, s, forms, c->enc_lean, x, B, Tv, c->w_cenc, c->w_enc, tlen, join_here ? c->ev_join : nullptr);
        if (!rl) join_guard.armed = false;          // (joined inside)
        return rl;
    }
    return enqueue_bilstm_steps(c, s, c->bilstm, x, B, Tv, c->conv_c, H, c->w_cenc, c->w_enc, tlen);
}

int enqueue_gst(gsttaco_ctx* c, hipStream_t s, int B, int Tref1) {
    const gsttaco_config& g = c->cfg;
    int H = Tref1 - 1, W = g.mel_dim;
    const float* x = c->w_mels_in + g.mel_dim;          // drop frame 0 (GST.py:98)
    int64_t xb = (int64_t)Tref1 * g.mel_dim;
    int cur = 0;
    for (int i = 0; i < g.n_ref_conv; ++i) {
        const ConvLayer& L = c->ref_conv[i].L;
        Conv2dArgs a{};
        a.x = x; a.xb = xb;
        a.w = L.w; a.scale = L.scale; a.shift = L.shift;
        a.out = c->w_gconv[cur];
        a.B = B; a.H = H; a.W = W; a.Cin = L.cin; a.Cout = L.cout;
        a.k = c->ref_conv[i].k; a.stride = c->ref_conv[i].stride;
        a.pad_h = same_pad_before(H, a.k, a.stride, &a.Ho);
        a.pad_w = same_pad_before(W, a.k, a.stride, &a.Wo);
        if (a.Cin % 4 == 0 && a.Cin >= 16) {
            // implicit GEMM on the fp32 MFMA path (M = B*Ho*Wo rows, K = 9*Cin): the direct kernel's late layers have a
            // few thousand threads with K = 576..1152 serial loads each (124 us for the last one).  Under Use_Mixed_Precision
            // too: the GST branch stays fp32 there (the FP32 form is the only one its layers have)
            ConvGemmArgs ga = conv_args(L, GSTTACO_CONV_FORM_FP32);
            ga.x = a.x; ga.xb = a.xb;
            ga.out = a.out; ga.ldo = a.Cout;
            ga.B = B; ga.T = a.Ho * a.Wo; ga.act = ACT_RELU;
            ga.conv2d = 1; ga.H = H; ga.W = W; ga.Wo = a.Wo; ga.kw = a.k; ga.stride = a.stride; ga.pad_h = a.pad_h; ga.pad_w = a.pad_w;
            HIPCHECK(c, gt_launch_conv_gemm(ga, s));
        } else
        HIPCHECK(c, gt_launch_conv2d_bn_relu(a, s));
        x = a.out; H = a.Ho; W = a.Wo; xb = (int64_t)H * W * a.Cout; cur ^= 1;
    }
    GstTailArgs t{};
    t.x = x; t.mel_len = c->w_mel_len;
    t.gru_w = c->gru_w; t.gru_u = c->gru_u; t.gru_b = c->gru_b;
    t.dense_w = c->dense_w; t.dense_b = c->dense_b;
    t.q_w = c->mq_w; t.q_b = c->mq_b; t.v_tok = c->v_tok; t.ln_g = c->ln_g; t.ln_b = c->ln_b;
    t.gst = c->w_gst;
    t.attn = c->w_gst_attn; t.query = c->w_gst_q;       // (always stored: gsttaco_gst_ex copies them out, and no graph key depends on who asks)
    t.B = B; t.T2 = H; t.gru_in = W * c->ref_conv[g.n_ref_conv - 1].L.cout; t.u = g.ref_rnn;
    t.D = g.ref_dense; t.A = g.gst_att; t.ntok = g.n_tokens; t.heads = g.heads;
    t.stride_prod = 1;
    for (int i = 0; i < g.n_ref_conv; ++i) t.stride_prod *= g.ref_strides[i];
    HIPCHECK(c, gt_launch_gst_tail(t, s));
    return 0;
}

// processed memory pm = [gst|enc].Wv + bv, with the gst half folded into a per-utterance bias row
int enqueue_value_proj(gsttaco_ctx* c, hipStream_t s, int B, int Tv) {
    const gsttaco_config& g = c->cfg;
    const float* rowbias = nullptr;
    if (g.gst_use) {
        SkinnyArgs k;
        memset(&k, 0, sizeof(k));
        k.wp = c->val_gst.wp; k.bf16 = c->val_gst.bf16; k.bias = c->val_gst.bias;
        k.seg[0] = SkinnySeg{c->w_gst, g.gst_att, g.gst_att / 16, 0};
        k.nkb = c->val_gst.nkb; k.M = B; k.N = c->att; k.n_split = c->att; k.MT = (B + 15) / 16;
        k.out = c->w_rowbias; k.ldo = c->att;
        HIPCHECK(c, gt_launch_skinny(EPI_LINEAR, k, nullptr, c->val_gst.ntiles, s));
        rowbias = c->w_rowbias;
    }
    ConvGemmArgs a = conv_args(c->val_enc, kFormsPlain | GSTTACO_CONV_FORM_GEMM_SPLIT);      // (its bias: in the row bias with GST, else its shift)
    a.x = c->w_enc;
    a.rowbias = rowbias;
    a.out = c->w_pm; a.ldo = c->att;
    a.B = B; a.T = Tv; a.act = ACT_NONE;
    HIPCHECK(c, gt_launch_conv_gemm(a, s));
    return 0;
}

// Front launch, batches above 32 rows: who computes which recurrent-half job (kernels.h DecFrontArgs::sched_*).  A job is a pair
// of tiles over every 32-row chunk of the batch with the weights held in registers; at large fp32 batches it is MFMA-bound
// and outlasts the per-utterance chain, so the CUs of finished utterance workgroups are worth more than a second round on the
// pure workers.  Picks (e, y) -- the piece sizes in chunks for the pure workers' extra share and for the utterance
// workgroups -- by the makespan of a two-parameter cost model: `unit` = one pair of tiles x one chunk, `chain` = the utterance
// workgroup's prenet / attention chain (measured on MI355X with in-kernel stamps: 5.8 / 3.4 us per unit in fp32 / bf16 -- fp32
// MFMA-bound at the ~2.0 GHz the chip sustains, bf16 bound by the CU's load pipe -- and 9.5 us per chain).
struct FrontSched { int pf, ne, e, y, utt; };
FrontSched plan_front_jobs(int jobs, int chunks, int n_workers, int B, bool bf16) {
    const double unit = bf16 ? 3.4 : 5.8, chain = 9.5;
    FrontSched best{jobs, 0, 0, 0, 0};
    double best_t = 1e30;
    for (int y = 0; y <= chunks; ++y) {
        if (y && chunks % y) continue;
        for (int e = 0; e <= chunks; ++e) {
            if (e && chunks % e) continue;
            const int utt = y ? B : 0;
            const int ny = y ? std::min(jobs, (utt * y + chunks - 1) / chunks) : 0;
            const int ne = e ? std::min(jobs - ny, (n_workers * e + chunks - 1) / chunks) : 0;
            const int pf = jobs - ny - ne;
            const int full_rounds = (pf + n_workers - 1) / n_workers;
            const int e_rounds = e ? (ne * (chunks / e) + n_workers - 1) / n_workers : 0;
            const int y_rounds = utt ? (ny * (chunks / y) + utt - 1) / utt : 0;
            const double t = std::max((full_rounds * chunks + e_rounds * e) * unit, chain + y_rounds * y * unit);
            if (t < best_t - 1e-9) { best_t = t; best = FrontSched{pf, ne, e, y, utt}; }
        }
    }
    return best;
}

// Every launch-form question of one decode, answered in one place: enqueue_decode launches what the plan says, and
// gsttaco_decode_plan, gsttaco_lstm_launch_bytes and masks_lazy report it.  `forms` is the call's (run_cached); only `persist`,
// `persist_bf16` and `fuse12` depend on it, and the three reporters read none of those: they pass what the context allows.
struct DecodePlan {
    bool persist = false;         // the whole loop as ONE persistent launch (persist_decode.hip) ...
    bool persist_bf16 = false;    // ... its bf16 kernel (mixed precision)
    bool fused = false;           // fused front launch (dec_front.hip; dec_front_lsa.hip for LSA), whose worker workgroups compute the
                                  // recurrent halves of both decode LSTMs; else the four-kernel front end and whole LSTM GEMMs
    bool lean_front = false;      // ... its lean utterance path (front_lean.h)
    int n_workers = 0;            // ... its worker workgroups: one per CU the utterance workgroups leave free (a quarter of the chip at least)
    int lean_rec = 0;             // ... their body: 0 general, 1 lean fp32, 2 lean bf16
    bool z0 = false;              // prenet-0 pre-activations computed by the previous step's projection launch (proj_z)
    int fuse12 = 0;               // both LSTM cells in one launch: 0 no, 1 gt_lstm12_kernel (fp32, <= 32 rows), 2 the multi-chunk form
    bool lean_x[2] = {false, false};  // otherwise LSTM layer l's input half on the lean kernel (gt_launch_lstm_x)
    int co_tiles = 0;             // layer-2 recurrent tiles computed beside the projection (the rest beside the front end)
    bool lean_proj = false;       // ... that projection launch on the lean kernel (gt_launch_proj_lean), else gt_launch_skinny_co
    bool mirror = false;          // bf16 mirrors of the blocked activations (mixed precision above 32 rows)
    bool hashed = false;          // keep decisions hashed from the seed (throughput mode at the reference's rate 0.5) ...
    bool masks_unused = false;    // ... and no launch reads the keep-mask tensor
};

// `forced`: a teacher-forced decode (DecodeCall::forced): always launches per step -- the persistent kernels feed their own frame back.
DecodePlan plan_decode(const gsttaco_ctx* c, const LaunchForms& forms, int B, int Tv, bool injected_mask, bool forced = false) {
    const gsttaco_config& g = c->cfg;
    const bool lsa = g.att_type == GSTTACO_ATT_LSA;
    const PackedLinear *X = c->lstm_x, *R = c->lstm_h;
    DecodePlan p;
    p.fused = c->fused_front && gt_dec_front_supported(g.mel_dim, c->P0, c->P1, c->att, Tv, lsa ? g.loc_filters : 0, lsa ? g.loc_kernel : 0);
    p.hashed = !injected_mask && g.prenet_rate == 0.5f;
    // (at rate 0.5 every fused front end derives the keep decisions from the seed itself (gt_keep_word): the tensor is not generated
    // -- 32 MB and most of a 30 us launch per call at the headline shape --, gsttaco_debug_randomness regenerates it when asked)
    p.masks_unused = p.hashed && p.fused;
    if (!p.fused) return p;
    p.lean_front = c->front_mode >= 2;
    p.n_workers = B < c->n_cu * 3 / 4 ? c->n_cu - B : c->n_cu / 4;
    p.lean_rec = (c->lean && R[0].bf16 == R[1].bf16 && R[0].nkb == 64 && R[1].nkb == 64) ? (R[0].bf16 ? 2 : 1) : 0;
    p.z0 = c->proj_z.wp != nullptr;
    for (int l = 0; l < 2; ++l) p.lean_x[l] = c->lean && gt_lstm_x_supported(X[l].nkb);
    // (batches above 32 rows: every launch is throughput-bound, the front launch most of all, and the projection launch has ~150 CUs
    // to spare: it takes half of layer 2's recurrent tiles instead of a quarter.  The persistent kernels sum these tiles in the same
    // order -- persist_decode.hip pd_rec2, persist_groups.h pd_g_rec_all, persist_bf16.h -- which keeps the two paths bitwise equal)
    if (c->proj.nkb >= 32) p.co_tiles = std::min(R[1].ntiles, B > 32 ? 128 : 64);
    p.lean_proj = c->lean && c->proj_z.bf16 == R[1].bf16 && gt_proj_lean_supported(c->proj_z.nkb, R[1].nkb) &&
                  c->H2 / 16 + c->att / 16 == c->proj_z.nkb && (c->H2 / 16) % 2 == 0;
    // Mixed precision above 32 rows: the producers of the blocked activations (front launch: prenet output + context; LSTM launches:
    // h1, h2) also write bf16 MIRRORS, which the bf16 multi-chunk GEMM bodies read instead -- half the activation bytes through
    // each CU's load pipe, which is what bounds those launches (EXPERIMENTS round 4), and no conversion per consumer.  Only when
    // every producer and consumer of the step is one that knows about mirrors.
    p.mirror = B > 32 && c->w_xa_h != nullptr && p.lean_x[0] && p.lean_x[1] && R[0].nkb == 64 && R[1].nkb == 64;
    // both LSTM cells in one launch (skinny_gemm.hip gt_lstm12_kernel: fp32, batch <= 32; above: the multi-chunk form, fp32 or bf16),
    // while this is the process's one live context
    if (forms.fuse12 && c->lean && X[0].bf16 == X[1].bf16) {
        if (gt_lstm12_mc_supported(X[0].nkb, X[1].nkb, c->H1, c->H2, B, c->fuse12_slots[X[0].bf16 ? 2 : 1])) p.fuse12 = 2;
        else if (!X[0].bf16 && gt_lstm12_supported(X[0].nkb, X[1].nkb, c->H1, c->H2, B, c->fuse12_slots[0])) p.fuse12 = 1;
    }
    // The whole loop as ONE persistent launch: fp32, batch <= 128 (above 32 rows: groups of 32 through one set of resident weights),
    // T_v <= 256, the reference's decoder sizes, SMA / BMA / LSA -- while this is the process's only live context (its hand-offs need
    // every workgroup resident).  Mixed precision: the bf16 kernel -- every GEMM pack bf16, the activation mirrors allocated, one
    // group of up to 64 rows.
    const int n_bf16 = X[0].bf16 + X[1].bf16 + R[0].bf16 + R[1].bf16 + c->proj_z.bf16;
    const bool bf16 = n_bf16 == 5 && c->w_xa_h && c->w_xa2_h && c->w_h1_h[0] && c->w_h2_h[0];
    p.persist = forms.persist_decode && c->lean && p.lean_front && p.z0 && (n_bf16 == 0 || bf16) && c->proj.nkb >= 32 &&
                // (the LSA extension: the one-group fp32 kernel's LSA chain, up to 128 tokens -- else the launch path)
                (!lsa || (n_bf16 == 0 && c->loc_pack && gt_persist_decode_lsa_fits(B, Tv, g.loc_filters, g.loc_kernel))) &&
                X[0].nkb == 24 && X[1].nkb == 64 && R[0].nkb == 64 && R[1].nkb == 64 && B <= c->persist_rows && (B <= 32 || c->w_stash) &&
                gt_persist_decode_supported(g.mel_dim, c->r, c->P0, c->P1, c->att, c->H1, c->H2, B, Tv, c->proj_z.ntiles, c->proj_z.nkb,
                                            c->persist_slots, bf16 ? 1 : 0);
    if (forced) p.persist = false;
    p.persist_bf16 = p.persist && bf16;
    return p;
}

// Event brackets around the decode launches that gsttaco_set_profiling times (gsttaco_ctx::prof_ev): enqueue() runs between the two
// events of the next bracket `which` when `on`, and alone otherwise.
struct ProfBrackets {
    gsttaco_ctx* c;
    hipStream_t s;
    int n[5] = {0, 0, 0, 0, 0};
    template <class F> int run(bool on, int which, F&& enqueue) {
        if (!on) return enqueue();
        while (c->prof_ev[which].size() < (size_t)2 * (n[which] + 1)) {
            hipEvent_t e;
            HIPCHECK(c, hipEventCreate(&e));
            c->prof_ev[which].push_back(e);
        }
        int rc = record_event(c, c->prof_ev[which][2 * n[which]], s);
        if (!rc) rc = enqueue();
        if (rc) return rc;
        rc = record_event(c, c->prof_ev[which][2 * n[which] + 1], s);
        ++n[which];
        return rc;
    }
};

// One decode being enqueued: what the parts below share
struct DecodeCall {
    gsttaco_ctx* c;
    hipStream_t s;
    DecodePlan P;
    int B, Tv, steps, MT;
    bool has_mask, has_noise;       // the buffers hold keep masks / noise (injected, or generated up front)
    const int32_t* tlen;            // masked mode: token lengths, or NULL
    float drop_scale;
    int64_t ld_pre;                 // row stride of the pre-postnet frames
    ProfBrackets prof;
    bool forced = false;            // teacher forcing (Taco2.py:185): step t consumes the staged ground-truth frame w_teach[t]
    const float* frame(int t) const {       // the last frame step t - 1 emitted (Taco2.py:186: decodings[:, -1]; zeros at t = 0)
        if (forced) return c->w_teach + (size_t)t * B * c->cfg.mel_dim;
        return t == 0 ? c->w_zero : c->w_pre + ((size_t)(t - 1) * c->r + (c->r - 1)) * c->cfg.mel_dim;
    }
    int64_t ldframe(int t) const { return forced ? (int64_t)c->cfg.mel_dim : (t == 0 ? 0 : ld_pre); }
    const float* mask(int t, int layer) const {
        return has_mask ? c->w_masks + (size_t)t * B * (c->P0 + c->P1) + (layer ? (size_t)B * c->P0 : 0) : nullptr;
    }
    unsigned long long* stamps(int t, int slot) const { return (c->stamps && t == steps / 2) ? c->w_dbg + slot : nullptr; }
};

// The whole loop as ONE persistent launch.  Bitwise the launches below (GPU test), which stay the path for every other shape, for
// several contexts, and after a give-up.  It keeps its state in registers and initialises it itself: none of the launch path's
// zero-fill launches (and their boundaries) is enqueued for it.
int enqueue_decode_persist(DecodeCall& d) {
    gsttaco_ctx* c = d.c;
    const gsttaco_config& g = c->cfg;
    const bool lsa = g.att_type == GSTTACO_ATT_LSA;        // (LSA: softmax, no sigmoid noise)
    // (randomness: hashed keep decisions, or the masks / noise in the buffers -- injected, or generated up front -- always one of them)
    if (!((g.prenet_rate == 0.f || d.P.hashed || d.has_mask) && (g.sigmoid_noise == 0.f || d.has_noise || lsa)))
        return fail(c, GSTTACO_E_INVALID, "internal: the persistent decode launch was chosen without its randomness");
    PersistDecodeArgs a{};
    a.w1x = c->lstm_x[0].wp; a.w1h = c->lstm_h[0].wp; a.b1h = c->lstm_h[0].bias;
    a.w2x = c->lstm_x[1].wp; a.w2h = c->lstm_h[1].wp; a.b2h = c->lstm_h[1].bias;
    a.wp = c->proj_z.wp; a.bp = c->proj_z.bias; a.pj_tiles = c->proj_z.ntiles;
    a.n_out = c->proj_out; a.n_split = g.mel_dim * c->r; a.z_col0 = c->z_col0;
    a.W1 = c->pw1; a.b1 = c->pb1; a.Wq = c->pwq; a.bq = c->pbq; a.av = c->att_v; a.score_bias = c->att_sb;
    a.pm = c->w_pm;
    a.noise = (g.sigmoid_noise > 0.f && !lsa) ? c->w_noise : nullptr;
    a.masks = (g.prenet_rate > 0.f && !d.P.hashed) ? c->w_masks : nullptr;
    a.seed_ptr = c->w_seed; a.tok_len = d.tlen;
    a.drop_rate = g.prenet_rate; a.drop_scale = d.drop_scale; a.sigmoid_noise = lsa ? 0.f : g.sigmoid_noise;
    a.keep_hash = d.P.hashed ? 1 : 0; a.att_type = g.att_type;
    a.loc_pack = c->loc_pack; a.loc_f = g.loc_filters; a.loc_k = g.loc_kernel; a.lsa_cumulate = g.lsa_cumulate; a.lsa_smoothing = g.lsa_smoothing;
    a.xa[0] = c->w_xa; a.xa[1] = c->w_xa2;
    a.h1[0] = c->w_h1[0]; a.h1[1] = c->w_h1[1]; a.h2[0] = c->w_h2[0]; a.h2[1] = c->w_h2[1];
    a.stash = c->w_stash;
    a.bf16 = d.P.persist_bf16 ? 1 : 0;
    a.xah[0] = c->w_xa_h; a.xah[1] = c->w_xa2_h;
    a.h1h[0] = c->w_h1_h[0]; a.h1h[1] = c->w_h1_h[1]; a.h2h[0] = c->w_h2_h[0]; a.h2h[1] = c->w_h2_h[1];
    a.z0g = c->w_z0g; a.hpart = c->w_hpart; a.ctl = c->w_pctl; a.err = c->w_err + 2;        // (its own give-up word)
    a.pre = c->w_pre; a.ld_pre = d.ld_pre; a.stop = c->w_stop; a.align = c->w_align; a.ld_align = (int64_t)d.steps * d.Tv;
    a.B = d.B; a.MT = d.MT; a.Tv = d.Tv; a.steps = d.steps; a.co_tiles = d.P.co_tiles;
    a.expect_extra = c->debug_drop_member >= 0 ? 1 : 0;
    a.dbg = c->stamps ? c->w_dbg : nullptr;
    const int rc = d.prof.run(c->prof_every > 0, 2, [&] { HIPCHECK(c, gt_launch_persist_decode(a, c->pb0, d.s)); return 0; });
    if (!rc) ++c->n_persist_decodes;
    return rc;
}

// 1-4 of step t fused: prenet x2, query projection, score / alignment / context (dec_front.hip); its worker workgroups compute the
// recurrent halves h_{t-1} . W_h + b of both LSTM layers (those of layer 2's tiles [0, co_tiles) from step 1 on: the previous
// step's projection launch did them)
int enqueue_front_fused(DecodeCall& d, int t, bool on) {
    gsttaco_ctx* c = d.c;
    const gsttaco_config& g = c->cfg;
    const DecodePlan& P = d.P;
    const int B = d.B, Tv = d.Tv, MT = d.MT, p = t & 1;
    const bool lsa = g.att_type == GSTTACO_ATT_LSA;
    DecFrontArgs f{};
    f.frame = d.frame(t); f.ldframe = d.ldframe(t);
    f.z0 = (P.z0 && t > 0) ? c->w_z0 : nullptr;
    // (forced: every step's pre-activations were computed up front from the staged frames, step 0 included -- enqueue_forced_z0)
    if (d.forced) f.z0 = c->w_zf + (size_t)t * B * c->P0;
    f.w0 = c->pw0; f.b0 = c->pb0; f.w1 = c->pw1; f.b1 = c->pb1; f.wq = c->pwq; f.bq = c->pbq;
    f.mask0 = d.mask(t, 0); f.mask1 = d.mask(t, 1);
    if (P.hashed) {
        // throughput mode: the kernel derives the same decisions gt_rng_fill_kernel would write to w_masks from the seed
        // itself (gt_keep_word) and, at the reference's sizes, skips the weight rows they zero
        f.mask0 = f.mask1 = nullptr;
        f.keep_hash = (c->P0 == 256 && c->P1 == 256 && c->att == 128) ? 1 : 0;
    }
    f.drop_rate = g.prenet_rate; f.drop_scale = d.drop_scale; f.seed_ptr = c->w_seed; f.rng_step = (uint32_t)t;
    f.pm = c->w_pm; f.v = c->att_v; f.score_bias = c->att_sb;
    f.prev = t == 0 ? nullptr : c->w_align + (size_t)(t - 1) * Tv; f.ldprev = (int64_t)d.steps * Tv;
    if (lsa) {      // the state buffer (zeroed up front) in place of the previous alignment; softmax, no noise
        f.prev = c->w_lsa_state; f.ldprev = Tv;
        f.loc_pack = c->loc_pack;
        f.lsa_state = c->w_lsa_state; f.loc_k = g.loc_kernel; f.loc_f = g.loc_filters;
        f.lsa_cumulate = g.lsa_cumulate; f.lsa_smoothing = g.lsa_smoothing;
    }
    f.noise = (d.has_noise && !lsa) ? c->w_noise + (size_t)t * B * Tv : nullptr; f.ldnoise = Tv;
    f.align = c->w_align + (size_t)t * Tv; f.ldalign = (int64_t)d.steps * Tv;
    f.xa = c->w_xa; f.MT = MT;
    f.xah = P.mirror ? c->w_xa_h : nullptr;
    f.B = B; f.Tv = Tv; f.mel = g.mel_dim; f.P0 = c->P0; f.P1 = c->P1; f.A = c->att; f.type = g.att_type;
    f.sigmoid_noise = lsa ? 0.f : g.sigmoid_noise;
    f.tok_len = d.tlen;
    f.dbg = d.stamps(t, 0);
    f.lean_front = P.lean_front ? 1 : 0;
    for (int layer = 0; layer < 2; ++layer) {
        SkinnyArgs& rk = f.rec[layer];
        const PackedLinear& L = c->lstm_h[layer];
        const int H = layer == 0 ? c->H1 : c->H2;
        rk.wp = L.wp; rk.bf16 = L.bf16; rk.bias = L.bias; rk.nkb = L.nkb;
        rk.seg[0] = SkinnySeg{layer == 0 ? c->w_h1[p ^ 1] : c->w_h2[p ^ 1], 0, H / 16, 1};
        rk.M = B; rk.N = H; rk.MT = MT;
        rk.keep_weights = 1;                    // default cache policy (see lean_body.h gt_lean_partial)
        rk.partial_out = c->w_part[layer];
        f.rec_begin[layer] = 0; f.rec_end[layer] = L.ntiles;
        f.lrec[layer] = LeanPartialArgs{rk.wp, rk.bias, rk.seg[0].ptr, rk.partial_out, MT};
        if (P.mirror && P.lean_rec == 2) f.lrec[layer].xh = layer == 0 ? c->w_h1_h[p ^ 1] : c->w_h2_h[p ^ 1];
    }
    f.n_workers = P.n_workers;
    f.lean_rec = P.lean_rec;
    if (t > 0) f.rec_begin[1] = P.co_tiles;
    constexpr int wt = 2;           // tiles per worker job (front_body.h WT: pairs sharing one pass over the activations)
    const int jobs = (f.rec_end[0] - f.rec_begin[0] + wt - 1) / wt + (f.rec_end[1] - f.rec_begin[1] + wt - 1) / wt;
    f.sched_pf = jobs;
    if (P.lean_rec != 0 && B > 32) {
        const FrontSched fs = plan_front_jobs(jobs, (B + 31) / 32, f.n_workers, B, P.lean_rec == 2);
        f.sched_pf = fs.pf; f.sched_ne = fs.ne; f.sched_e = fs.e; f.sched_y = fs.y; f.utt_jobs = fs.utt;
    }
    return d.prof.run(on, 2, [&] { HIPCHECK(c, gt_launch_dec_front(f, d.s)); return 0; });
}

// 1-4 of step t as four kernels (GSTTACO_FUSED_FRONT=0, or a shape the fused kernel's LDS does not hold)
int enqueue_front_kernels(DecodeCall& d, int t) {
    gsttaco_ctx* c = d.c;
    const gsttaco_config& g = c->cfg;
    const int B = d.B, Tv = d.Tv, MT = d.MT, P0 = c->P0, P1 = c->P1, att = c->att, mel = g.mel_dim;
    hipStream_t s = d.s;
    float* xa_t = c->w_xa;
    SkinnyArgs k;
    // 1. prenet layer 0 on the last emitted frame
    memset(&k, 0, sizeof(k));
    k.wp = c->prenet0.wp; k.bf16 = c->prenet0.bf16; k.bias = c->prenet0.bias;
    k.seg[0] = SkinnySeg{d.frame(t), d.ldframe(t), mel / 16, 0};
    k.nkb = c->prenet0.nkb; k.M = B; k.N = P0; k.n_split = P0; k.MT = MT;
    k.out = c->w_p1; k.ldo = P0;
    k.mask = d.mask(t, 0); k.ldm = P0;
    k.drop_rate = g.prenet_rate; k.drop_scale = d.drop_scale;
    k.seed_ptr = c->w_seed; k.rng_step = (uint32_t)t; k.rng_stream = 0x1000u;
    HIPCHECK(c, gt_launch_skinny(EPI_RELU_DROP, k, nullptr, c->prenet0.ntiles, s));
    // 2. prenet layer 1 -> xa[:, 0:P1]
    memset(&k, 0, sizeof(k));
    k.wp = c->prenet1.wp; k.bf16 = c->prenet1.bf16; k.bias = c->prenet1.bias;
    k.seg[0] = SkinnySeg{c->w_p1, P0, P0 / 16, 0};
    k.nkb = c->prenet1.nkb; k.M = B; k.N = P1; k.n_split = P1; k.MT = MT;
    k.out = xa_t; k.out_blocked = 1;
    k.mask = d.mask(t, 1); k.ldm = P1;
    k.drop_rate = g.prenet_rate; k.drop_scale = d.drop_scale;
    k.seed_ptr = c->w_seed; k.rng_step = (uint32_t)t; k.rng_stream = 0x1001u;
    HIPCHECK(c, gt_launch_skinny(EPI_RELU_DROP, k, nullptr, c->prenet1.ntiles, s));
    // 3. attention query projection (Steps.py:122)
    memset(&k, 0, sizeof(k));
    k.wp = c->query.wp; k.bf16 = c->query.bf16; k.bias = c->query.bias;
    k.seg[0] = SkinnySeg{xa_t, 0, P1 / 16, 1};
    k.nkb = c->query.nkb; k.M = B; k.N = att; k.n_split = att; k.MT = MT;
    k.out = c->w_q; k.ldo = att;
    HIPCHECK(c, gt_launch_skinny(EPI_LINEAR, k, nullptr, c->query.ntiles, s));
    // 4. score / monotonic alignment / context -> xa[:, P1:P1+att]
    AttnStepArgs a{};
    a.q = c->w_q; a.ldq = att; a.pm = c->w_pm; a.v = c->att_v; a.score_bias = c->att_sb;
    a.prev = t == 0 ? nullptr : c->w_align + (size_t)(t - 1) * Tv; a.ldprev = (int64_t)d.steps * Tv;
    a.noise = d.has_noise ? c->w_noise + (size_t)t * B * Tv : nullptr; a.ldnoise = Tv;
    a.align = c->w_align + (size_t)t * Tv; a.ldalign = (int64_t)d.steps * Tv;
    a.ctx = xa_t + (size_t)(P1 / 16) * MT * 256; a.ldctx = 0; a.ctx_mt = MT;
    a.B = B; a.Tv = Tv; a.A = att; a.type = g.att_type; a.sigmoid_noise = g.sigmoid_noise;
    a.seed_ptr = c->w_seed; a.rng_step = (uint32_t)t; a.tok_len = d.tlen;
    a.loc_cw = c->loc_cw; a.loc_cb = c->loc_cb; a.loc_dw = c->loc_dw; a.loc_db = c->loc_db; a.att_bias = c->att_bias;
    a.lsa_state = c->w_lsa_state; a.loc_k = g.loc_kernel; a.loc_f = g.loc_filters;
    a.lsa_cumulate = g.lsa_cumulate; a.lsa_smoothing = g.lsa_smoothing;
    HIPCHECK(c, gt_launch_attn_step(a, s));
    return 0;
}

// 5/6. the two LSTM cells of step t (StackedRNNCells, Taco2.py:111): one fused launch, or one launch per cell -- the input half on
// top of the recurrent half the front launch's workers computed (fused front), or the whole GEMM
int enqueue_lstm_cells(DecodeCall& d, int t, bool on) {
    gsttaco_ctx* c = d.c;
    const DecodePlan& P = d.P;
    const int B = d.B, MT = d.MT, H1 = c->H1, H2 = c->H2, p = t & 1;
    float* xa_t = c->w_xa;
    if (P.fuse12) {
        Lstm12Args fa{};
        for (int layer = 0; layer < 2; ++layer) {
            const PackedLinear& L = c->lstm_x[layer];
            float** hb = layer == 0 ? c->w_h1 : c->w_h2;
            LstmXArgs& la = layer == 0 ? fa.l1 : fa.l2;
            la = LstmXArgs{L.wp, layer == 0 ? xa_t : c->w_h1[p], c->w_part[layer], layer == 0 ? c->w_c1 : c->w_c2, hb[p],
                           d.stamps(t, 16 * (1 + layer)), B, MT, layer == 0 ? H1 : H2, L.nkb};
            if (P.mirror) {
                la.xh = layer == 0 ? c->w_xa_h : c->w_h1_h[p];
                la.hh = layer == 0 ? c->w_h1_h[p] : c->w_h2_h[p];
            }
        }
        fa.arrive = c->w_arrive + (size_t)t * GT_L12_NSH * 32;
        fa.err = c->w_err;
        fa.expect = (uint32_t)(P.fuse12 == 2 ? gt_lstm12_mc_grid(H1) : (H1 + 3) / 4) + (c->debug_drop_member >= 0 ? 1u : 0u);
        return d.prof.run(on, 0, [&] {
            if (P.fuse12 == 2) HIPCHECK(c, gt_launch_lstm12_mc(fa, c->lstm_x[0].bf16 != 0, d.s));
            else HIPCHECK(c, gt_launch_lstm12(fa, d.s));
            return 0;
        });
    }
    const int XA = c->P1 + c->att;
    for (int layer = 0; layer < 2; ++layer) {
        SkinnyArgs k;
        memset(&k, 0, sizeof(k));
        const int H = layer == 0 ? H1 : H2;
        float** hb = layer == 0 ? c->w_h1 : c->w_h2;
        if (P.fused) {
            // only the half that depends on this step's inputs; + partial_in (recurrent half + bias)
            const PackedLinear& L = c->lstm_x[layer];
            k.wp = L.wp; k.bf16 = L.bf16; k.bias = L.bias; k.nkb = L.nkb;
            if (layer == 0) k.seg[0] = SkinnySeg{xa_t, 0, XA / 16, 1};
            else k.seg[0] = SkinnySeg{c->w_h1[p], 0, H1 / 16, 1};
            k.partial_in = c->w_part[layer];
            k.keep_weights = 1;
        } else {
            const PackedLinear& L = layer == 0 ? c->lstm0 : c->lstm1;
            k.wp = L.wp; k.bf16 = L.bf16; k.bias = L.bias; k.nkb = L.nkb;
            if (layer == 0) {
                k.seg[0] = SkinnySeg{xa_t, 0, XA / 16, 1};
                k.seg[1] = SkinnySeg{c->w_h1[p ^ 1], 0, H1 / 16, 1};
            } else {
                k.seg[0] = SkinnySeg{c->w_h1[p], 0, H1 / 16, 1};
                k.seg[1] = SkinnySeg{c->w_h2[p ^ 1], 0, H2 / 16, 1};
            }
        }
        k.N = H; k.c = layer == 0 ? c->w_c1 : c->w_c2; k.h = hb[p]; k.out_blocked = 1;
        k.M = B; k.MT = MT;
        k.dbg = d.stamps(t, 16 * (1 + layer));
        const int tag = layer == 0 ? TAG_DEC_LSTM1 : TAG_DEC_LSTM2;
        const int rc = d.prof.run(on, layer, [&] {
            if (P.lean_x[layer]) {
                LstmXArgs la{k.wp, k.seg[0].ptr, k.partial_in, k.c, k.h, k.dbg, B, MT, H, k.nkb};
                if (P.mirror) {
                    la.xh = layer == 0 ? c->w_xa_h : c->w_h1_h[p];
                    la.hh = layer == 0 ? c->w_h1_h[p] : c->w_h2_h[p];
                }
                HIPCHECK(c, gt_launch_lstm_x(la, k.nkb, tag, k.bf16 != 0, d.s));
            } else
                HIPCHECK(c, gt_launch_skinny(EPI_LSTM, k, nullptr, (H + 3) / 4, d.s, tag));
            return 0;
        });
        if (rc) return rc;
    }
    return 0;
}

// 7. projection [h2, ctx] -> r mel frames + stop logit, written in place (Taco2.py:112-118,194-205); + the next step's prenet-0
// pre-activations (proj_z) and, beside it, layer 2's recurrent tiles [0, co_tiles) for the next step
int enqueue_projection(DecodeCall& d, int t, bool on) {
    gsttaco_ctx* c = d.c;
    const DecodePlan& P = d.P;
    const int B = d.B, MT = d.MT, H2 = c->H2, P1 = c->P1, att = c->att, mel = c->cfg.mel_dim, r = c->r, p = t & 1;
    float* xa_t = c->w_xa;
    int rc = d.prof.run(on, 4, [] { return 0; });          // empty bracket
    if (rc) return rc;
    SkinnyArgs k;
    memset(&k, 0, sizeof(k));
    const PackedLinear& PJ = (P.z0 && t + 1 < d.steps) ? c->proj_z : c->proj;
    k.wp = PJ.wp; k.bf16 = PJ.bf16; k.bias = PJ.bias;
    k.seg[0] = SkinnySeg{c->w_h2[p], 0, H2 / 16, 1};
    k.seg[1] = SkinnySeg{xa_t + (size_t)(P1 / 16) * MT * 256, 0, att / 16, 1};
    k.nkb = PJ.nkb; k.M = B; k.N = c->proj_out; k.n_split = mel * r; k.MT = MT;
    if (&PJ == &c->proj_z) {
        k.N = c->z_col0 + c->P0; k.n_valid2 = c->proj_out; k.col3 = c->z_col0;
        k.out3 = c->w_z0; k.ldo3 = c->P0;
    }
    k.out = c->w_pre + (size_t)t * r * mel; k.ldo = d.ld_pre;
    k.out2 = c->w_stop + t; k.ldo2 = d.steps;
    return d.prof.run(on, 3, [&] {
        if (P.co_tiles > 0 && t + 1 < d.steps) {
            // co-scheduled workers: recurrent half of layer 2 for the NEXT step, h2_t . W_h + b (tiles [0, co_tiles))
            SkinnyArgs rk;
            memset(&rk, 0, sizeof(rk));
            const PackedLinear& L = c->lstm_h[1];
            rk.wp = L.wp; rk.bf16 = L.bf16; rk.bias = L.bias; rk.nkb = L.nkb;
            rk.seg[0] = SkinnySeg{c->w_h2[p], 0, H2 / 16, 1};
            rk.M = B; rk.N = H2; rk.MT = MT;
            rk.keep_weights = 1;
            rk.partial_out = c->w_part[1];
            if (P.lean_proj) {
                ProjArgs pa{k.wp, k.bias, k.seg[0].ptr, k.seg[1].ptr, k.seg[0].nkb, B, MT, k.N, k.n_split, k.n_valid2, k.col3,
                            k.out, k.ldo, k.out2, k.ldo2, k.out3, k.ldo3, d.stamps(t, 40)};
                if (P.mirror) { pa.xah = c->w_h2_h[p]; pa.xbh = c->w_xa_h + (size_t)(P1 / 32) * MT * 512; }
                HIPCHECK(c, gt_launch_proj_lean(pa, PJ.ntiles, rk.wp, rk.bias, rk.seg[0].ptr, rk.partial_out, 0, P.co_tiles, k.bf16 != 0, d.s));
            } else
                HIPCHECK(c, gt_launch_skinny_co(k, PJ.ntiles, rk, 0, P.co_tiles, d.s));
        } else
            HIPCHECK(c, gt_launch_skinny(EPI_LINEAR, k, nullptr, PJ.ntiles, d.s));
        return 0;
    });
}

// Z0 [S][B][P0] = w_teach [S*B, mel] . W0 + b0: the prenet-0 pre-activations of EVERY forced step in one fp32 GEMM (the implicit-GEMM
// kernel's v_mfma_f32_32x32x2_f32 chain; fp32 operands under Use_Mixed_Precision too, like the front kernel's own prenet 0)
int enqueue_forced_z0(gsttaco_ctx* c, hipStream_t s, int B, int steps) {
    ConvGemmArgs a = conv_args(c->z0_dense, GSTTACO_CONV_FORM_FP32);
    a.x = c->w_teach;
    a.out = c->w_zf; a.ldo = c->P0;
    a.B = 1; a.T = steps * B; a.act = ACT_NONE;
    HIPCHECK(c, gt_launch_conv_gemm(a, s));
    return 0;
}

int enqueue_decode(gsttaco_ctx* c, hipStream_t s, const LaunchForms& forms, int B, int Tv, int steps, bool has_mask, bool has_noise, bool masked, bool forced) {
    const gsttaco_config& g = c->cfg;
    const int MT = (B + 15) / 16;
    DecodeCall d{c, s, plan_decode(c, forms, B, Tv, has_mask, forced), B, Tv, steps, MT, has_mask, has_noise, masked ? c->w_tok_len : nullptr,
                 g.prenet_rate > 0.f ? 1.0f / (1.0f - g.prenet_rate) : 1.f, (int64_t)steps * c->r * g.mel_dim, ProfBrackets{c, s}};
    d.forced = forced;
    const DecodePlan& P = d.P;
    if (forced && P.fused) {
        const int rc0 = enqueue_forced_z0(c, s, B, steps);
        if (rc0) return rc0;
    }
    if (!P.persist) {
        HIPCHECK(c, gt_launch_zero(c->w_h1[1], (size_t)MT * 16 * c->H1, s));
        HIPCHECK(c, gt_launch_zero(c->w_h2[1], (size_t)MT * 16 * c->H2, s));
        HIPCHECK(c, gt_launch_zero(c->w_c1, (size_t)B * c->H1, s));
        HIPCHECK(c, gt_launch_zero(c->w_c2, (size_t)B * c->H2, s));
        if (P.mirror) {
            HIPCHECK(c, gt_launch_zero(reinterpret_cast<float*>(c->w_h1_h[1]), (size_t)MT * 16 * c->H1 / 2, s));
            HIPCHECK(c, gt_launch_zero(reinterpret_cast<float*>(c->w_h2_h[1]), (size_t)MT * 16 * c->H2 / 2, s));
        }
    }
    if (g.att_type == GSTTACO_ATT_LSA) HIPCHECK(c, gt_launch_zero(c->w_lsa_state, (size_t)B * Tv, s));   // Layers.py:356
    if (P.fuse12 && !P.persist) HIPCHECK(c, gt_launch_zero(reinterpret_cast<float*>(c->w_arrive), (size_t)steps * GT_L12_NSH * 32, s));
    // throughput mode: the whole decode's dropout masks and sigmoid noise are generated up front (same Philox streams the
    // step kernels would draw) into the buffers injected tensors use, so no step spends time on random numbers
    float* fm = (!has_mask && g.prenet_rate > 0.f && !P.masks_unused) ? c->w_masks : nullptr;
    float* fn = (!has_noise && g.sigmoid_noise > 0.f && g.att_type != GSTTACO_ATT_LSA) ? c->w_noise : nullptr;
    if (fm || fn) HIPCHECK(c, gt_launch_rng_fill(c->w_seed, fm, fn, steps, B, c->P0, c->P1, Tv, g.prenet_rate, s));
    if (fm) d.has_mask = true;
    if (fn) d.has_noise = true;
    int rc = 0;
    if (P.persist)
        rc = enqueue_decode_persist(d);
    else
        for (int t = 0; t < steps && !rc; ++t) {
            const bool on = c->prof_every > 0 && (t % c->prof_every) == 0;      // (bracketed steps)
            rc = P.fused ? enqueue_front_fused(d, t, on) : enqueue_front_kernels(d, t);
            if (!rc) rc = enqueue_lstm_cells(d, t, on);
            if (!rc) rc = enqueue_projection(d, t, on);
        }
    if (rc) return rc;
    if (c->prof_every > 0)      // an un-bracketed capture must not forget the brackets of an earlier, bracketed graph
        for (int i = 0; i < 5; ++i) c->prof_count[i] = d.prof.n[i];
    return 0;
}

// Postnet layer i's call without its buffers: everything the kernel choice depends on (enqueue_postnet adds x / out / res;
// gsttaco_postnet_variants asks gt_conv_gemm_variant about it)
ConvGemmArgs postnet_call(const gsttaco_ctx* c, int i, int B, int Tf) {
    const gsttaco_config& g = c->cfg;
    const ConvLayer& L = c->post_conv[i];
    ConvGemmArgs a = conv_args(L, kFormsPlain | kFormsWino);       // (everything the layer has)
    a.wino_x3 = c->wino_x3 ? 1 : 0;
    a.ldo = L.cout;
    a.B = B; a.T = Tf;
    a.pad_before = same_pad_before(Tf, L.taps, 1, nullptr);
    a.act = i < g.post_tanh ? ACT_TANH : ACT_NONE;     // tanh on the first post_tanh layers only (F9)
    // THE PROMISE the two-plane fp16 Winograd form needs: this layer reads what layer i - 1's tanh wrote, so |x| <= 1.  Made here and
    // nowhere else (layer 0 reads the decoder's mels: no bound)
    a.x_absmax = postnet_input_is_tanh(g, i) ? 1.f : 0.f;
    // mixed precision: the activations BETWEEN the layers are stored as bf16 -- the next layer rounds them to bf16 on its way into
    // LDS anyway, so no result changes and half the bytes move; the residual input and the last layer's output stay fp32
    if (a.wt_bf16) {
        a.x_bf16 = i > 0 && c->post_conv[i - 1].wt_bf16 ? 1 : 0;
        // (a bf16 output row is stored as PAIRS of columns: an even channel count only)
        a.out_bf16 = i != g.n_post - 1 && L.cout % 2 == 0 && c->post_conv[i + 1].wt_bf16 ? 1 : 0;
    }
    return a;
}

// (round 6) Whether the embedding lookup is written out as rows in front of encoder layer 0, so that layer 0 too can take the Winograd
// kernel on the bf16 pipe (it resolves the lookup inside its gather only as an implicit GEMM: 140 us against ~90 for lookup + Winograd
// at 4 096 rows).  The rows go to w_act[1]; layer 0 writes w_act[0].
bool encoder_rows_path(const gsttaco_ctx* c, int B, int Tv) {
    const gsttaco_config& g = c->cfg;
    return g.n_enc_conv > 0 && c->enc_wino && c->enc_conv[0].wino_s && c->w_tokens && c->enc_conv[0].cin == g.emb &&
           (B * ((Tv + 1) / 2) + 63) / 64 * ((c->enc_conv[0].cout + 127) / 128) >= 100;
}

// Encoder layer i's call without its buffers, as postnet_call (enqueue_encoder adds x / out / row_len; gsttaco_encoder_variants asks
// gt_conv_gemm_variant about it).  rows_path: encoder_rows_path() of the call; without it layer 0 gathers the embedding rows by token.
ConvGemmArgs encoder_call(const gsttaco_ctx* c, int i, int B, int Tv, bool rows_path) {
    const ConvLayer& L = c->enc_conv[i];
    const bool gather = i == 0 && !rows_path;
    // (round 6) the five-tap layers behind the token gather as Winograd on the bf16 pipe (conv_wino_split.hip): B x Tv = 4 096 rows are
    // 128 workgroups of F(2,5) -- half the chip, where the fp32 Winograd kernel lost to the implicit GEMM (275 against 136 us) --
    // enc_wino: 0 = implicit GEMM, 2 = F(2,5), 4 = F(4,5) where its grid reaches 60 workgroups
    const bool wino = c->enc_wino && !gather && L.wino_s;
    // (F(4,5) where ITS grid fills the chip -- batches of 128 utterances --, else F(2,5) down to 100 workgroups)
    const bool f4 = c->enc_wino == 4 || ((B * ((Tv + 3) / 4) + 63) / 64) * ((L.cout + 127) / 128) >= 240;
    // (nothing but FP32 / BF16 while the token gather is still in front)
    ConvGemmArgs a = conv_args(L, kFormsPlain | (wino ? GSTTACO_CONV_FORM_WINO2 | GSTTACO_CONV_FORM_WINO_SPLIT | (f4 ? GSTTACO_CONV_FORM_WINO4 : 0) : 0));
    if (wino) a.wino_min_wgs = c->enc_wino == 4 ? 60 : 100;
    a.tokens = gather ? c->w_tokens : nullptr;
    a.ldo = L.cout;
    a.B = B; a.T = Tv;
    a.pad_before = same_pad_before(Tv, L.taps, 1, nullptr);
    a.act = ACT_RELU;
    return a;
}

// One GEMM of the vocoder without its buffers, as postnet_call (enqueue_vocoder adds x / out / res; gsttaco_vocoder_variants asks
// gt_conv_gemm_variant about it).  which: GSTTACO_VOC_*; i: the layer among its kind (0 for the three single Dense layers).
// Every GEMM of the vocoder: FP32, BF16 under mixed precision, never Winograd.
ConvGemmArgs vocoder_call(const gsttaco_ctx* c, int which, int i, int B, int Tf) {
    const gsttaco_config& g = c->cfg;
    const ConvLayer& L = which == GSTTACO_VOC_BANK ? c->voc_bank[i] : which == GSTTACO_VOC_PROJ ? c->voc_proj[i] :
                         which == GSTTACO_VOC_PROJ_DENSE ? c->voc_pd : which == GSTTACO_VOC_HIGHWAY_IN ? c->voc_hin :
                         which == GSTTACO_VOC_HIGHWAY ? c->voc_hw[i] : c->voc_dense;
    ConvGemmArgs a = conv_args(L, kFormsPlain);
    a.ldo = which == GSTTACO_VOC_BANK ? g.bank_count * g.bank_filters : L.cout;     // (the bank layers write side by side)
    a.B = B; a.T = Tf;
    a.act = ACT_NONE;
    if (which == GSTTACO_VOC_BANK || which == GSTTACO_VOC_PROJ) {
        a.pad_before = same_pad_before(Tf, L.taps, 1, nullptr);       // even kernels pad asymmetrically (F10)
        // conv bank: + BN + ReLU each; projections: Conv1D + BN (+ReLU except the last) (Taco2.py:319-340, 383-407)
        a.act = which == GSTTACO_VOC_BANK || i < g.n_voc_proj - 1 ? ACT_RELU : ACT_NONE;
        a.pool2 = which == GSTTACO_VOC_PROJ && i == 0;                // MaxPool1D(2,1,'same') fused into the first projection's gather
    }
    return a;
}

int enqueue_postnet(gsttaco_ctx* c, hipStream_t s, int B, int Tf, const float* pre, float* out) {
    const gsttaco_config& g = c->cfg;
    const float* x = pre;
    int cur = 0;
    for (int i = 0; i < g.n_post; ++i) {
        const bool last = i == g.n_post - 1;
        ConvGemmArgs a = postnet_call(c, i, B, Tf);
        a.x = x;
        a.out = last ? out : c->w_post[cur];
        a.res = last ? pre : nullptr;                       // post = postnet(x) + x (Taco2.py:230)
        HIPCHECK(c, gt_launch_conv_gemm(a, s));
        x = a.out; cur ^= 1;
    }
    return 0;
}

// librosa.filters.mel(sr, n_fft, n_mels) with the 0.7.2 defaults the reference relies on (Audio.py:81-83): fmin 0,
// fmax sr/2, Slaney scale (htk=False), area normalisation (norm=1), float32.  [n_mels, n_fft/2+1] row-major.
std::vector<float> slaney_mel_basis(int sr, int n_fft, int n_mels) {
    const int nb = n_fft / 2 + 1;
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; };
    auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; };
    auto linspace = [](double a, double b, int n) {
        std::vector<double> v(n);
        const double step = (b - a) / (n - 1);
        for (int i = 0; i < n; ++i) v[i] = i * step + a;
        v[n - 1] = b;
        return v;
    };
    const std::vector<double> fftfreqs = linspace(0.0, sr / 2.0, nb);
    std::vector<double> mel_f = linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2);
    for (double& m : mel_f) m = mel_to_hz(m);
    std::vector<float> w((size_t)n_mels * nb, 0.f);
    for (int i = 0; i < n_mels; ++i) {
        const double fd0 = mel_f[i + 1] - mel_f[i], fd1 = mel_f[i + 2] - mel_f[i + 1];
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < nb; ++k) {
            const double lower = -(mel_f[i] - fftfreqs[k]) / fd0;
            const double upper = (mel_f[i + 2] - fftfreqs[k]) / fd1;
            const float tri = (float)std::max(0.0, std::min(lower, upper));     // stored in a float32 array first
            w[(size_t)i * nb + k] = (float)((double)tri * enorm);               // then scaled in place
        }
    }
    return w;
}

int ensure_device(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= g.device)
        return fail(c, GSTTACO_E_NO_DEVICE, "no HIP device: the gfx950 kernels are the only compute path (no CPU fallback)");
    HIPCHECK(c, hipSetDevice(g.device));
    hipDeviceProp_t prop;
    HIPCHECK(c, hipGetDeviceProperties(&prop, g.device));
    if (!strstr(prop.gcnArchName, "gfx950"))
        return fail(c, GSTTACO_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    if (prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    return 0;
}

void host_audio_tables(gsttaco_ctx* c) {
    if (!c->h_mel_basis.empty()) return;
    c->n_fft = 2 * (c->cfg.spec_dim - 1);
    c->h_mel_basis = slaney_mel_basis(c->cfg.sample_rate, c->n_fft, c->cfg.mel_dim);
}

int ensure_audio(gsttaco_ctx* c) {
    if (c->audio_ready) return 0;
    const gsttaco_config& g = c->cfg;
    if (g.max_wav_samples <= 0) return fail(c, GSTTACO_E_INVALID, "the context was created without audio capacity (max_wav_samples = 0)");
    int rc = ensure_device(c);
    if (rc) return rc;
    host_audio_tables(c);
    const int N = c->n_fft, H = N / 2, nb = H + 1;
    // scipy.signal.get_window('hann', win, fftbins=True), zero-padded centred to n_fft (librosa.util.pad_center)
    std::vector<float> win(N, 0.f);
    const int wl = g.frame_length, lpad = (N - wl) / 2;
    for (int i = 0; i < wl; ++i) win[lpad + i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / wl));
    std::vector<float> tw(2 * (size_t)H);
    for (int k = 0; k < H; ++k) {
        tw[2 * k] = (float)std::cos(-2.0 * M_PI * k / N);
        tw[2 * k + 1] = (float)std::sin(-2.0 * M_PI * k / N);
    }
    std::vector<int32_t> lo(g.mel_dim), hi(g.mel_dim);
    for (int m = 0; m < g.mel_dim; ++m) {
        int a = nb, b = 0;
        for (int k = 0; k < nb; ++k)
            if (c->h_mel_basis[(size_t)m * nb + k] != 0.f) { a = std::min(a, k); b = std::max(b, k + 1); }
        lo[m] = a < b ? a : 0; hi[m] = a < b ? b : 0;
    }
    if ((rc = upload(c, &c->a_window, win.data(), win.size()))) return rc;
    if ((rc = upload(c, reinterpret_cast<float**>(&c->a_twiddle), tw.data(), tw.size()))) return rc;
    if ((rc = upload(c, &c->a_mel_basis, c->h_mel_basis.data(), c->h_mel_basis.size()))) return rc;
    if ((rc = upload(c, reinterpret_cast<float**>(&c->a_band_lo), reinterpret_cast<const float*>(lo.data()), lo.size()))) return rc;
    if ((rc = upload(c, reinterpret_cast<float**>(&c->a_band_hi), reinterpret_cast<const float*>(hi.data()), hi.size()))) return rc;
    {   // window^2 in float64 (librosa.filters.window_sumsquare squares the float64 window), zero-padded like the window
        std::vector<double> wsq(N, 0.0);
        for (int i = 0; i < wl; ++i) {
            const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / wl);
            wsq[lpad + i] = w * w;
        }
        if ((rc = dev_alloc(c, (void**)&c->a_win_sq, (size_t)N * sizeof(double)))) return rc;
        HIPCHECK(c, hipMemcpy(c->a_win_sq, wsq.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCHECK(c, gt_gl_init());
    c->a_ld_mse = g.max_wav_samples / 16 + 1;
    if ((rc = dev_alloc(c, (void**)&c->a_mse, (size_t)g.max_batch * c->a_ld_mse * sizeof(double)))) return rc;
    if ((rc = dev_alloc(c, (void**)&c->a_bounds, (size_t)g.max_batch * 2 * sizeof(int32_t)))) return rc;
    c->audio_ready = true;
    return 0;
}

// mel [B,Tf,mel] -> spectrogram [B,Tf,spec]  (reference Taco2.py:258-260, 366-380)
int enqueue_vocoder(gsttaco_ctx* c, hipStream_t s, const LaunchForms& forms, int B, int Tf, const float* mel_in, float* spec) {
    const gsttaco_config& g = c->cfg;
    // conv bank: kernel sizes 1..N on the INPUT, each + BN + ReLU, concatenated on the channel axis (Taco2.py:383-407)
    // (every GEMM of the vocoder: FP32, BF16 under mixed precision, never Winograd)
    for (int i = 0; i < g.bank_count; ++i) {
        ConvGemmArgs a = vocoder_call(c, GSTTACO_VOC_BANK, i, B, Tf);
        a.x = mel_in;
        a.out = c->w_vbank + (size_t)i * g.bank_filters;
        HIPCHECK(c, gt_launch_conv_gemm(a, s));
    }
    // MaxPool1D(2,1,'same') fused into the first projection conv's gather; Conv1D + BN (+ReLU except the last) (Taco2.py:319-340)
    const float* x = c->w_vbank;
    int cur = 0;
    for (int i = 0; i < g.n_voc_proj; ++i) {
        ConvGemmArgs a = vocoder_call(c, GSTTACO_VOC_PROJ, i, B, Tf);
        a.x = x;
        a.out = c->w_vbuf[cur];
        const bool last = i == g.n_voc_proj - 1;
        if (last && !c->voc_pd.w) a.res = mel_in;                     // residual directly when no Dense follows (:373)
        HIPCHECK(c, gt_launch_conv_gemm(a, s));
        x = a.out; cur ^= 1;
    }
    // a Dense over the frames: x -> out [B*Tf, L.cout]
    auto dense = [&](int which, int i, const float* in, float* out, const float* res) {
        ConvGemmArgs a = vocoder_call(c, which, i, B, Tf);
        a.x = in; a.res = res;
        a.out = out;
        HIPCHECK(c, gt_launch_conv_gemm(a, s));
        return 0;
    };
    int rc = 0;
    if (c->voc_pd.w) {                                                // Dense back to mel width + residual (:342-345, 373)
        if ((rc = dense(GSTTACO_VOC_PROJ_DENSE, 0, x, c->w_vbuf[cur], mel_in))) return rc;
        x = c->w_vbuf[cur]; cur ^= 1;
    }
    const int S = g.highway_size;
    if (c->voc_hin.w) {                                               // Dense to the highway width (:348-351)
        if ((rc = dense(GSTTACO_VOC_HIGHWAY_IN, 0, x, c->w_vbuf[cur], nullptr))) return rc;
        x = c->w_vbuf[cur]; cur ^= 1;
    }
    float* hbuf[2] = {c->w_vbuf[cur], c->w_vbuf[2]};
    int hcur = 0;
    for (int i = 0; i < g.highway_count; ++i) {                       // Highwaynet (:409-424)
        if ((rc = dense(GSTTACO_VOC_HIGHWAY, i, x, c->w_vz, nullptr))) return rc;
        HIPCHECK(c, gt_launch_highway(c->w_vz, x, hbuf[hcur], (int64_t)B * Tf, S, s));
        x = hbuf[hcur]; hcur ^= 1;
    }
    // Bidirectional LSTM over the Tf frames (:353-361)
    const int H = g.voc_rnn;
    HIPCHECK(c, gt_launch_zero(c->w_vc, (size_t)2 * B * H, s));
    if (lean_bilstm_usable(c, forms, c->voc_lean, B)) rc = enqueue_lean_bilstm(c, s, forms, c->voc_lean, x, B, Tf, c->w_vc, c->w_vrnn, nullptr);
    else rc = enqueue_bilstm_steps(c, s, c->voc_bilstm, x, B, Tf, S, H, c->w_vc, c->w_vrnn, nullptr);
    if (rc) return rc;
    return dense(GSTTACO_VOC_DENSE, 0, c->w_vrnn, spec, nullptr);           // Dense to the linear-spectrogram width (Taco2.py:252-260)
}

int check_ready(gsttaco_ctx* c) {
    if (!c) return GSTTACO_E_INVALID;
    if (!c->finalized) return fail(c, GSTTACO_E_WEIGHTS, "weights not finalized (call gsttaco_finalize_weights)");
    return 0;
}

int check_shape(gsttaco_ctx* c, int B, int Tv, int Tref1, int steps) {
    const gsttaco_config& g = c->cfg;
    if (B < 1 || Tv < 1 || steps < 0 || steps > c->steps_max)
        return fail(c, GSTTACO_E_INVALID, "bad B / Tv / steps");
    if (B > g.max_batch || Tv > g.max_tokens || Tref1 > g.max_ref_frames)
        return fail(c, GSTTACO_E_CAPACITY, "batch / tokens / reference frames exceed the capacity given at create");
    return 0;
}

// Teacher forcing: the workspace of the staged frames and of every step's prenet-0 pre-activations, sized like the rest of the workspace
// by the capacity given at create and allocated by the FIRST forced call (outside any capture: check_forced), so a context that never
// forces pays nothing; freed with everything else at destroy.
int ensure_forced(gsttaco_ctx* c) {
    if (c->w_teach && c->w_zf) return 0;
    const size_t rows = (size_t)c->cfg.max_batch * c->steps_max;
    int rc = 0;
    if (!c->w_teach && (rc = dev_alloc(c, (void**)&c->w_teach, (rows + 16) * c->cfg.mel_dim * sizeof(float)))) return rc;
    if (!c->w_zf && (rc = dev_alloc(c, (void**)&c->w_zf, rows * c->P0 * sizeof(float)))) return rc;
    return 0;
}

// The arguments every forced entry point shares: teacher [B, Tq, mel] -> *S = ceil((Tq - 1) / r) decoder steps; and their workspace
int check_forced(gsttaco_ctx* c, const float* teacher, int Tq, int B, int Tv, int Tref1, int* S) {
    if (!teacher) return fail(c, GSTTACO_E_INVALID, "null teacher");
    if (Tq < 2) return fail(c, GSTTACO_E_INVALID, "teacher needs the go frame and at least one more (Tq >= 2)");
    const int64_t steps = ((int64_t)Tq - 1 + c->r - 1) / c->r;
    if (steps > c->steps_max) return fail(c, GSTTACO_E_CAPACITY, "teacher frames exceed Max_Step");
    *S = (int)steps;
    const int rc = check_shape(c, B, Tv, Tref1, *S);
    return rc ? rc : ensure_forced(c);
}

// One row per launch form that can give up: its flag, its word of h_err (bit `word` of gave_up) and the warning its fallback leaves.
// In the order note_give_up visits them, which decides whose warning is left when several gave up at once.
struct GiveUpForm { bool LaunchForms::*flag; int word; const char* warning; };
const GiveUpForm kGiveUpForms[3] = {
    {&LaunchForms::persist_decode, 2,
     "warning: a hand-off wait of the persistent decode launch gave up in an earlier call (its workgroups were not co-resident: "
     "is another process or a CU mask sharing this GPU?); that call's outputs were invalid.  This context now runs the decode "
     "loop as launches per step (bitwise the same results, ~25 % slower)"},
    {&LaunchForms::fuse12, 0,
     "warning: the in-kernel hand-off of the fused decode-LSTM launch gave up in an earlier call (its workgroups were not "
     "co-resident: is another process or a CU mask sharing this GPU?); that call's outputs were invalid.  This context now "
     "runs the two LSTM cells as two launches (same results, ~4 % slower)"},
    {&LaunchForms::bilstm_persist, 1,
     "warning: a hand-off wait of the persistent BiLSTM launch gave up in an earlier call (its members were not co-resident: is "
     "another process or a CU mask sharing this GPU?); that call's outputs were invalid.  This context now runs its BiLSTMs with "
     "one launch per time step (bitwise the same results in fp32, within the mixed-precision tolerance under "
     "Use_Mixed_Precision -- the per-step bf16 kernel sums in a different order; ~0.5 ms slower per call)"},
};

// A bounded in-kernel wait of an EARLIER enqueue gave up (its workgroups never became co-resident: another process on the GPU,
// a CU mask, a profiler's kernel): the outputs of the call it belongs to are garbage.  Seen here, at a later enqueue:
//   * the give-up is remembered in a STICKY per-context word that only gsttaco_synchronize reports and clears ("since the last
//     check"): a later call -- or a later graph segment of the same call -- must not erase it;
//   * the context stops using that launch form (two launches per decode step / one launch per BiLSTM time step: no co-residency
//     needed) and says so through gsttaco_last_error as a warning;
//   * the device-visible word is NOT cleared here: launches of this context may still be in flight, they poll the word and
//     leave at once while it is set; cleared, each of up to ~500 remaining fused launches would spin to its full bound.
//     gsttaco_synchronize clears it behind the stream synchronisation.
void note_give_up(gsttaco_ctx* c) {
    if (!c->h_err) return;
    // (one word per launch form: a kernel polls its own word to leave early once a sibling has given up, so a give-up of the persistent
    // decode launch must not make the fused LSTM launches enqueued behind it abort)
    for (const GiveUpForm& f : kGiveUpForms) {
        if (!c->h_err[f.word]) continue;
        c->gave_up |= 1u << f.word;
        if (!(c->allow.*f.flag)) continue;
        c->allow.*f.flag = false;
        c->debug_drop_member = -1;
        c->warn = f.warning;
        c->announce_warn = true;
    }
}

std::map<GraphKey, gsttaco_ctx::GraphEntry>::iterator lru_graph(gsttaco_ctx* c) {
    return std::min_element(c->graphs.begin(), c->graphs.end(), [](const auto& a, const auto& b) { return a.second.last_use < b.second.last_use; });
}

// run_cached with the key complete: the graph cache
template <typename F>
int run_cached_inner(gsttaco_ctx* c, hipStream_t stream, const GraphKey& key, F body) {
    if (!c->use_graph || c->graph_cache_max < 1) return body(stream, key.forms);
    const uint64_t now = ++c->graph_clock;
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
        if (c->graph_capture_after > 1) {
            auto& seen = c->graph_seen[key];
            seen.second = now;
            if (++seen.first < c->graph_capture_after) {
                if (c->graph_seen.size() > 256) {           // bound the bookkeeping too: forget the stalest key
                    auto old = c->graph_seen.begin();
                    for (auto j = c->graph_seen.begin(); j != c->graph_seen.end(); ++j)
                        if (j->second.second < old->second.second) old = j;
                    c->graph_seen.erase(old);
                }
                return body(stream, key.forms);
            }
            c->graph_seen.erase(key);
        }
        hipGraph_t graph = nullptr;
        HIPCHECK(c, hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeRelaxed));
        c->capturing = true;
        int rc = body(c->cap_stream, key.forms);
        c->capturing = false;
        hipError_t e = hipStreamEndCapture(c->cap_stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (e != hipSuccess) return fail(c, GSTTACO_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) return fail(c, GSTTACO_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        while ((int)c->graphs.size() >= c->graph_cache_max) {       // evict the least recently used executable
            auto old = lru_graph(c);
            // an evicted executable may still be running on the stream it was last launched on (the stream is a per-call argument)
            HIPCHECK(c, hipStreamSynchronize(old->second.last_stream));
            (void)hipGraphExecDestroy(old->second.exec);
            c->graphs.erase(old);
        }
        it = c->graphs.emplace(key, gsttaco_ctx::GraphEntry{exec, now, stream}).first;
    }
    it->second.last_use = now;
    it->second.last_stream = stream;
    HIPCHECK(c, hipGraphLaunch(it->second.exec, stream));
    return 0;
}

// Runs `body(stream, forms)` either eagerly on `stream` or through a cached hipGraph captured on the internal stream (LRU-bounded,
// see gsttaco_ctx::graphs).  `forms`: what this call may take, decided once -- what the context allows, the fused decode-LSTM and the
// persistent decode launch only while this is the process's one live context (several decode loops in flight could each hold part of
// the chip and wait for the rest of their launch).  It is part of the key, and what is recorded as in flight is what the body was given.
template <typename F>
int run_cached(gsttaco_ctx* c, hipStream_t stream, GraphKey key, F body) {
    note_give_up(c);
    if (c->announce_warn) { c->err = c->warn; c->announce_warn = false; }
    const bool alone = g_live_contexts.load() <= 1;
    const LaunchForms forms{c->allow.fuse12 && alone, c->allow.bilstm_persist, c->allow.persist_decode && alone};
    key.forms = forms;
    const SegTraits seg = seg_traits(key.kind);
    // The process-wide mutex guards the two event tables and -- for segments with a persistent BiLSTM launch only -- the order in which
    // such segments are chained on the GPU.  Every other segment is captured / instantiated / launched OUTSIDE it: several contexts on
    // several threads do not serialise their host-side enqueue on one lock.
    {   // another context's fused launches may still be in flight: this segment starts behind them (see g_fused_event)
        std::lock_guard<std::mutex> lock(g_persist_mu);
        auto it = g_fused_event.find(c->cfg.device);
        if (it != g_fused_event.end() && it->second.ev && it->second.owner != c) HIPCHECK(c, hipStreamWaitEvent(stream, it->second.ev, 0));
    }
    int rc = 0;
    if (!(seg.bilstm && forms.bilstm_persist)) {
        rc = run_cached_inner(c, stream, key, body);
    } else {
        std::lock_guard<std::mutex> lock(g_persist_mu);        // (wait -> enqueue -> record must not interleave with another context's)
        hipEvent_t& ev = g_persist_event[c->cfg.device];
        if (!ev) HIPCHECK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else HIPCHECK(c, hipStreamWaitEvent(stream, ev, 0));
        rc = run_cached_inner(c, stream, key, body);
        HIPCHECK(c, hipEventRecord(ev, stream));
    }
    if (!rc && seg.decode && (forms.fuse12 || forms.persist_decode)) {      // the segment held fused / persistent decode launches
        std::lock_guard<std::mutex> lock(g_persist_mu);
        FusedInFlight& f = g_fused_event[c->cfg.device];
        if (!f.ev) HIPCHECK(c, hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
        HIPCHECK(c, hipEventRecord(f.ev, stream));
        f.owner = c;
    }
    return rc;
}

void add_seg(GtCopySegs& cs, const void* src, void* dst, size_t words) {
    cs.src[cs.n] = src; cs.dst[cs.n] = dst; cs.words[cs.n] = words; ++cs.n;
}

// What every decode stages in front of its graph segment: injected keep masks (in the caller's prenet sizes: re-laid out for a padded
// decoder) and noise -- parity runs --, the seed unless the caller's own input launch carries it (`seed` NULL), the teacher frames a
// forced decode consumes (`teacher` NULL: a free run), and masks_lazy for gsttaco_debug_randomness.
int stage_decode_inputs(gsttaco_ctx* c, hipStream_t s, const float* mask, const float* noise, const uint64_t* seed, const float* teacher,
                        int Tq, int B, int Tv, int steps) {
    if (mask && c->dec_padded) HIPCHECK(c, gt_launch_relayout_masks(mask, c->w_masks, steps, B, c->cfg.prenet[0], c->cfg.prenet[1], c->P0, c->P1, 1, s));
    else if (mask) HIPCHECK(c, hipMemcpyAsync(c->w_masks, mask, (size_t)steps * B * (c->P0 + c->P1) * 4, hipMemcpyDeviceToDevice, s));
    if (noise) HIPCHECK(c, hipMemcpyAsync(c->w_noise, noise, (size_t)steps * B * Tv * 4, hipMemcpyDeviceToDevice, s));
    if (seed) HIPCHECK(c, gt_launch_set_seed(c->w_seed, *seed, s));
    if (teacher) HIPCHECK(c, gt_launch_stage_teacher(teacher, c->w_teach, B, Tq, steps, c->r, c->cfg.mel_dim, s));
    // (per CALL: a replayed graph does not pass through enqueue_decode; masks_unused does not depend on the launch forms)
    c->masks_lazy = plan_decode(c, c->allow, B, Tv, mask != nullptr, teacher != nullptr).masks_unused;
    return 0;
}

// gsttaco_decode (`teacher` NULL) and gsttaco_decode_forced (the reference's OTHER loop branch, Taco2.py:183-187, training=True: step t
// consumes teacher[:, t * r]; launches per step, plan_decode `forced`).  The callers have checked their own arguments.
int decode_call(gsttaco_ctx* c, const float* enc, const float* gst, const int32_t* token_lengths, const float* mask, const float* noise,
                uint64_t seed, int B, int Tv, int steps, const float* teacher, int Tq, float* pre_mel, float* stop, float* align, void* stream) {
    int rc = 0;
    const bool forced = teacher != nullptr;
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(c, hipMemcpyAsync(c->w_enc, enc, (size_t)B * Tv * c->enc_out * 4, hipMemcpyDeviceToDevice, s));
    if (c->cfg.gst_use) HIPCHECK(c, hipMemcpyAsync(c->w_gst, gst, (size_t)B * c->cfg.gst_att * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = stage_decode_inputs(c, s, mask, noise, &seed, teacher, Tq, B, Tv, steps))) return rc;
    const bool masked = token_lengths != nullptr;
    if (masked) HIPCHECK(c, hipMemcpyAsync(c->w_tok_len, token_lengths, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    const GraphKey key{.kind = forced ? kSegDecodeForced : kSegDecode, .B = B, .Tv = Tv, .steps = steps, .has_mask = mask != nullptr,
                       .has_noise = noise != nullptr, .prof = c->prof_every, .masked = masked};
    rc = run_cached(c, s, key, [&](hipStream_t st, const LaunchForms& forms) {
        int r2 = enqueue_value_proj(c, st, B, Tv);
        return r2 ? r2 : enqueue_decode(c, st, forms, B, Tv, steps, mask != nullptr, noise != nullptr, masked, forced);
    });
    if (rc) return rc;
    const size_t mel = c->cfg.mel_dim;
    HIPCHECK(c, hipMemcpyAsync(pre_mel, c->w_pre, (size_t)B * steps * c->r * mel * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(c, hipMemcpyAsync(stop, c->w_stop, (size_t)B * steps * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(c, hipMemcpyAsync(align, c->w_align, (size_t)B * steps * Tv * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace

// ================================================================================================ ABI
extern "C" {

int gsttaco_abi_version(void) { return GSTTACO_ABI_VERSION; }

const char* gsttaco_last_error(const gsttaco_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int gsttaco_create(const gsttaco_config* cfg, gsttaco_ctx** out) {
    if (!cfg || !out) return fail(nullptr, GSTTACO_E_INVALID, "null argument");
    *out = nullptr;
    const gsttaco_config& g = *cfg;
    if (g.abi_version != GSTTACO_ABI_VERSION) return fail(nullptr, GSTTACO_E_INVALID, "ABI version mismatch");
    auto bad = [&](const char* m) { return fail(nullptr, GSTTACO_E_INVALID, m); };
    if (g.mel_dim < 16 || g.mel_dim % 16) return bad("Sound.Mel_Dim must be a positive multiple of 16");
    if (g.step_reduction < 1 || g.max_step < g.step_reduction) return bad("bad Step_Reduction / Max_Step");
    if (g.vocab < 2 || g.emb < 4 || g.emb % 4) return bad("bad vocabulary / Embedding.Size (multiple of 4)");
    if (g.n_enc_conv < 1 || g.n_enc_conv > GSTTACO_MAX_LAYERS) return bad("bad encoder conv count");
    for (int i = 0; i < g.n_enc_conv; ++i)
        if (g.enc_filters[i] % 16 || g.enc_filters[i] < 16 || g.enc_kernels[i] < 1)
            return bad("encoder Conv.Filters must be multiples of 16");
    if (g.enc_rnn < 16 || g.enc_rnn % 16) return bad("Encoder.RNN.Size must be a multiple of 16");
    if (g.n_prenet != 2) return bad("Decoder.Prenet.Size must have exactly 2 layers");
    if (g.prenet[0] % 16 || g.prenet[1] % 16 || g.prenet[0] < 16 || g.prenet[1] < 16)
        return bad("Prenet sizes must be multiples of 16");
    if (!(g.prenet_rate >= 0.f && g.prenet_rate < 1.f)) return bad("Prenet.Dropout_Rate must be in [0,1)");
    if (g.n_dec_rnn != 2) return bad("Decoder.RNN.Size must have exactly 2 layers");
    if (g.dec_rnn[0] % 16 || g.dec_rnn[1] % 16 || g.dec_rnn[0] < 16 || g.dec_rnn[1] < 16)
        return bad("Decoder.RNN sizes must be multiples of 16");
    if (g.att_type != GSTTACO_ATT_BMA && g.att_type != GSTTACO_ATT_SMA && g.att_type != GSTTACO_ATT_LSA)
        return bad("Unsupported attention type");            // reference Taco2.py:74-75
    if (g.att_type == GSTTACO_ATT_LSA && (g.loc_filters < 1 || g.loc_filters > 128 || g.loc_kernel < 1 || g.loc_kernel > 255))
        return bad("LSA: Attention.Conv.Filters must be 1..128 and Kernel_Size 1..255");
    if (g.att_size < 16 || g.att_size % 16 || g.att_size > 256) return bad("Attention.Size must be a multiple of 16, <= 256");
    if (g.n_post < 1 || g.n_post > GSTTACO_MAX_LAYERS) return bad("bad postnet layer count");
    for (int i = 0; i < g.n_post; ++i)
        if (g.post_filters[i] % 4 || g.post_filters[i] < 4 || g.post_kernels[i] < 1) return bad("postnet Decoder.Conv.Filters must be multiples of 4");
    if (g.post_filters[g.n_post - 1] != g.mel_dim) return bad("last postnet filter count must equal Mel_Dim");
    if (g.gst_use) {
        if (g.n_ref_conv < 1 || g.n_ref_conv > GSTTACO_MAX_LAYERS) return bad("bad reference-encoder conv count");
        for (int i = 0; i < g.n_ref_conv; ++i)
            if (g.ref_filters[i] < 4 || g.ref_filters[i] % 4 || g.ref_kernels[i] < 1 || g.ref_strides[i] < 1)
                return bad("reference-encoder Conv.Filters must be multiples of 4");
        if (g.ref_rnn < 1 || g.ref_dense < 1 || g.n_tokens < 1 || g.token_emb < 1) return bad("bad GST sizes");
        if (g.heads < 1 || g.gst_att % g.heads)
            return bad("size must be divisible by num_heads.");   // reference Layers.py:155-156
        if (g.gst_att % 16) return bad("Style_Token.Attention.Size must be a multiple of 16");
        // (what gt_gst_tail_kernel cannot run is refused here, not at the first gsttaco_gst of a context that has its weights)
        std::string why;
        const int64_t gru_in = ref_gru_in(g);
        if (gru_in > INT32_MAX || !gt_gst_tail_supported((int)gru_in, g.ref_rnn, g.ref_dense, g.gst_att, g.heads, g.n_tokens, &why))
            return bad(why.empty() ? "the reference encoder's GRU input is too wide" : why.c_str());
    }
    if (g.voc_use) {
        if (g.spec_dim < 1 || g.bank_count < 1 || g.bank_count > 32 || g.bank_filters < 4 || g.bank_filters % 4)
            return bad("Vocoder_Taco1: Conv_Bank.Filters must be a multiple of 4, Stack_Count 1..32");
        if (g.n_voc_proj < 1 || g.n_voc_proj > GSTTACO_MAX_LAYERS) return bad("Vocoder_Taco1: bad Conv1D projection count");
        for (int i = 0; i < g.n_voc_proj; ++i)
            if (g.voc_proj_filters[i] < 4 || g.voc_proj_filters[i] % 4 || g.voc_proj_kernels[i] < 1)
                return bad("Vocoder_Taco1: Conv1D.Filters must be multiples of 4");
        if (g.highway_count < 0 || g.highway_size < 16 || g.highway_size % 16) return bad("Vocoder_Taco1: Highwaynet.Size must be a multiple of 16");
        if (g.voc_rnn < 16 || g.voc_rnn % 16) return bad("Vocoder_Taco1: RNN.Size must be a multiple of 16");
    }
    if (g.max_batch < 1 || g.max_tokens < 1 || (g.gst_use && g.max_ref_frames < 2)) return bad("bad capacity");
    auto env_int = [](const char* name, int dflt) { const char* e = getenv(name); return e && *e ? atoi(e) : dflt; };
    {   // The four-kernel attention step (attention.hip) is what every shape runs that the fused front end and the persistent chain
        // decline: its LDS at the context's capacity -- the memory tile, 3 x max_tokens floats of scores and alignments and, LSA, the
        // location filters -- must fit what gt_attn_init opts into.  Arithmetic on the host: nothing is launched to find out.
        const bool lsa = g.att_type == GSTTACO_ATT_LSA;
        const int att_run = (env_int("GSTTACO_PAD_DECODER", 1) != 0 && decoder_pads(g)) ? 128 : g.att_size;
        const size_t need = gt_attn_lds_bytes(g.max_tokens, att_run, lsa ? g.loc_filters : 0, lsa ? g.loc_kernel : 0, nullptr);
        if (need > GT_ATTN_LDS_MAX) {
            char m[256];
            if (lsa)
                snprintf(m, sizeof m, "LSA: Attention.Conv.Filters %d x Kernel_Size %d at Attention.Size %d and max_tokens %d needs %zu bytes of "
                         "LDS in the attention step, more than the %zu a workgroup has", g.loc_filters, g.loc_kernel, att_run, g.max_tokens,
                         need, GT_ATTN_LDS_MAX);
            else
                snprintf(m, sizeof m, "max_tokens %d at Attention.Size %d needs %zu bytes of LDS in the attention step, more than the %zu a "
                         "workgroup has", g.max_tokens, att_run, need, GT_ATTN_LDS_MAX);
            return bad(m);
        }
    }
    if (g.max_wav_samples > 0) {
        const int n_fft = 2 * (g.spec_dim - 1);
        if (g.spec_dim < 33 || n_fft > 8192 || (n_fft & (n_fft - 1))) return bad("Sound.Spectrogram_Dim must be 2^k + 1 with 64 <= n_fft <= 8192");
        if (g.frame_length < 1 || g.frame_length > n_fft) return bad("Sound.Frame_Length must be in [1, n_fft]");
        if (g.frame_shift < 1 || g.sample_rate < 1 || g.max_abs_mel < 0.f) return bad("bad Sound.Frame_Shift / Sample_Rate / Max_Abs_Mel");
        if (g.max_wav_samples <= n_fft) return bad("max_wav_samples must exceed n_fft");
    }

    gsttaco_ctx* c = new gsttaco_ctx();
    c->cfg = g;
    c->r = g.step_reduction;
    c->steps_max = g.max_step / g.step_reduction;
    c->enc_out = 2 * g.enc_rnn;
    c->mem_dim = c->enc_out + (g.gst_use ? g.gst_att : 0);
    c->proj_out = g.mel_dim * g.step_reduction + 1;
    c->conv_c = g.enc_filters[g.n_enc_conv - 1];
    c->P0 = g.prenet[0]; c->P1 = g.prenet[1]; c->H1 = g.dec_rnn[0]; c->H2 = g.dec_rnn[1]; c->att = g.att_size;
    // The environment is read ONCE, here (INTEGRATION.md section 6 documents these; GSTTACO_LIB is the Python binding's).
    c->use_graph = env_int("GSTTACO_GRAPH", 1) != 0;
    c->graph_cache_max = std::max(0, env_int("GSTTACO_GRAPH_CACHE", c->graph_cache_max));
    c->graph_capture_after = std::max(1, env_int("GSTTACO_GRAPH_CAPTURE_AFTER", c->graph_capture_after));
    c->front_mode = std::min(2, std::max(0, env_int("GSTTACO_FUSED_FRONT", 2)));
    c->fused_front = c->front_mode != 0;
    c->lean = env_int("GSTTACO_LEAN", 1) != 0;
    c->allow.bilstm_persist = env_int("GSTTACO_BILSTM_PERSIST", 1) != 0;
    c->allow.fuse12 = env_int("GSTTACO_FUSED_LSTM", 1) != 0;
    c->allow.persist_decode = env_int("GSTTACO_PERSIST_DECODE", 1) != 0;
    c->persist_rows = env_int("GSTTACO_PERSIST_ROWS", 128);
    // (round 6: the encoder's convolutions run on the Winograd split kernel's 128 workgroups = half the chip, and the GST branch -- 0.24 ms of
    // small launches -- now does hide beside them: 10.75 -> 10.5 ms per Inference_Step at the headline shape; when they filled the chip
    // the fork measured neutral, EXPERIMENTS round 5 item 6)
    c->gst_fork = env_int("GSTTACO_GST_FORK", 1) > 0;      // (0 or 1; the retired 2, a graph of its own for the GST branch, means 1)
    c->wino = env_int("GSTTACO_WINO", 4);
    if (c->wino != 0 && c->wino != 2) c->wino = 4;      // {0, 2, 4}; any other non-zero value (the old boolean's 1 included) means the default
    c->wino_split = env_int("GSTTACO_WINO_SPLIT", 1) != 0;
    c->wino_x3 = env_int("GSTTACO_WINO_SPLIT", 1) == 3;
    c->wino_split_h = env_int("GSTTACO_WINO_SPLIT", 1) == 1;       // (6: split-bf16 x6 everywhere, for A/B against the two-plane fp16 form)
    c->enc_wino = env_int("GSTTACO_ENC_WINO", 2);
    if (c->enc_wino != 0 && c->enc_wino != 4) c->enc_wino = 2;
    c->pad_dec = env_int("GSTTACO_PAD_DECODER", 1) != 0;
    c->stamps = env_int("GSTTACO_STAMPS", 0) == 1;
    build_manifest(c);
    c->counted = true;
    g_live_contexts.fetch_add(1);
    *out = c;
    return 0;
}

void gsttaco_destroy(gsttaco_ctx* c) {
    if (!c) return;
    for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second.exec);
    for (int l = 0; l < 5; ++l)
        for (auto e : c->prof_ev[l]) (void)hipEventDestroy(e);
    if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (void* p : c->allocs) (void)hipFree(p);
    for (auto& rs : c->rs_slot) {
        if (rs.h_image) (void)hipHostFree(rs.h_image);
        if (rs.uploaded) (void)hipEventDestroy(rs.uploaded);
    }
    if (c->h_err) (void)hipHostFree(c->h_err);
    if (c->counted) g_live_contexts.fetch_sub(1);
    {
        std::lock_guard<std::mutex> lock(g_persist_mu);
        for (auto& kv : g_fused_event)
            if (kv.second.owner == c) kv.second.owner = nullptr;    // (its work has finished: the caller synchronises before destroying)
    }
    delete c;
}

int gsttaco_num_weights(const gsttaco_ctx* c) { return c ? (int)c->weights.tensors.size() : GSTTACO_E_INVALID; }

int gsttaco_weight_info(const gsttaco_ctx* c, int i, const char** name, int64_t shape[4], int* ndim) {
    return c ? c->weights.info(i, name, shape, ndim) : GSTTACO_E_INVALID;
}

int gsttaco_load_weight(gsttaco_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!c || !name || !host) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (c->finalized) return fail(c, GSTTACO_E_WEIGHTS, "weights already finalized");
    return c->weights.load(c, "", name, host, shape, ndim);
}

}  // extern "C"

// ---------------------------------------------------------------------------- gsttaco_finalize_weights, module by module
namespace {

// the whole [x_t | h_prev] GEMM of both directions (the launch per time step) and, where it applies, the lean form
int finalize_bilstm(gsttaco_ctx* c, PackedLinear* pk, gsttaco_ctx::LeanBiLstm* lean, const std::string& prefix, int H) {
    int d = 0, rc = 0;
    for (const char* dir : {"fwd", "bwd"}) {
        const std::string p = prefix + "." + dir;
        const HostTensor &k = T(c, p + ".kernel"), &u = T(c, p + ".recurrent_kernel"), &b = T(c, p + ".bias");
        if ((rc = pack_linear(c, &pk[d], {{k.data.data(), (int)k.shape[0]}, {u.data.data(), (int)u.shape[0]}}, 4 * H, b.data.data(), H))) return rc;
        ++d;
    }
    return build_lean_bilstm(c, lean, prefix, H);
}

int finalize_encoder(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    int rc = upload_tensor(c, &c->d_emb, "encoder.embedding");
    c->enc_conv.resize(g.n_enc_conv);
    for (int i = 0; i < g.n_enc_conv && !rc; ++i) rc = upload_conv(c, &c->enc_conv[i], "encoder.conv" + std::to_string(i), true);
    return rc ? rc : finalize_bilstm(c, c->bilstm, &c->enc_lean, "encoder.bilstm", g.enc_rnn);
}

int finalize_gst(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    int rc = 0;
    for (int i = 0; i < g.n_ref_conv; ++i) {
        const std::string p = "gst.ref.conv" + std::to_string(i);
        const HostTensor& k = T(c, p + ".kernel");      // [k, k, cin, cout] == [taps * cin, cout]
        std::vector<float> sc, sh;
        fold_bn(c, p, sc, sh);
        auto& R = c->ref_conv[i];
        R.k = (int)k.shape[0]; R.stride = g.ref_strides[i];
        // (the FP32 form only: the GST branch never runs on bf16 operands, mixed precision or not)
        if ((rc = prepare_conv_forms(c, &R.L, k.data.data(), R.k * R.k, (int)k.shape[2], (int)k.shape[3], (int)k.shape[3], sc.data(), sh.data(),
                                     GSTTACO_CONV_FORM_FP32))) return rc;
    }
    const std::pair<float**, const char*> plain[] = {
        {&c->gru_w, "gst.ref.gru.kernel"}, {&c->gru_u, "gst.ref.gru.recurrent_kernel"}, {&c->gru_b, "gst.ref.gru.bias"},
        {&c->dense_w, "gst.ref.dense.kernel"}, {&c->dense_b, "gst.ref.dense.bias"}, {&c->mq_w, "gst.mha.query.kernel"},
        {&c->mq_b, "gst.mha.query.bias"}, {&c->ln_g, "gst.mha.ln.gamma"}, {&c->ln_b, "gst.mha.ln.beta"}};
    for (const auto& t : plain)
        if ((rc = upload_tensor(c, t.first, t.second))) return rc;
    // v_tok = tanh(tokens).Wv + bv  (GST.py:100-101, Layers.py:175; batch-invariant)
    const HostTensor &tok = T(c, "gst.tokens"), &wv = T(c, "gst.mha.value.kernel"), &bv = T(c, "gst.mha.value.bias");
    std::vector<float> vt((size_t)g.n_tokens * g.gst_att);
    for (int n = 0; n < g.n_tokens; ++n)
        for (int a = 0; a < g.gst_att; ++a) {
            double s = bv.data[a];
            for (int e = 0; e < g.token_emb; ++e)
                s += std::tanh((double)tok.data[(size_t)n * g.token_emb + e]) * (double)wv.data[(size_t)e * g.gst_att + a];
            vt[(size_t)n * g.gst_att + a] = (float)s;
        }
    return upload(c, &c->v_tok, vt.data(), vt.size());
}

int finalize_decoder_step(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    int rc = 0;
    pad_decoder(c);
    {
        const HostTensor &k0 = T(c, "decoder.prenet0.kernel"), &b0 = T(c, "decoder.prenet0.bias");
        const HostTensor &k1 = T(c, "decoder.prenet1.kernel"), &b1 = T(c, "decoder.prenet1.bias");
        if ((rc = pack_linear(c, &c->prenet0, {{k0.data.data(), (int)k0.shape[0]}}, c->P0, b0.data.data(), 0, false))) return rc;
        if ((rc = pack_linear(c, &c->prenet1, {{k1.data.data(), (int)k1.shape[0]}}, c->P1, b1.data.data(), 0, false))) return rc;
        if ((rc = upload(c, &c->pw0, k0.data.data(), k0.data.size()))) return rc;
        if ((rc = upload(c, &c->pb0, b0.data.data(), b0.data.size()))) return rc;
        if ((rc = upload(c, &c->pw1, k1.data.data(), k1.data.size()))) return rc;
        if ((rc = upload(c, &c->pb1, b1.data.data(), b1.data.size()))) return rc;
        // (teacher forcing: prenet 0 over all steps' frames at once is a plain Dense on the plain layouts -- FP32 form, nothing uploaded twice)
        c->z0_dense.w = c->pw0; c->z0_dense.shift = c->pb0;
        c->z0_dense.taps = 1; c->z0_dense.cin = g.mel_dim; c->z0_dense.cout = c->P0;
        const HostTensor &qk = T(c, "decoder.attention.query.kernel"), &qb = T(c, "decoder.attention.query.bias");
        if ((rc = upload(c, &c->pwq, qk.data.data(), qk.data.size()))) return rc;
        if ((rc = upload(c, &c->pbq, qb.data.data(), qb.data.size()))) return rc;
        if ((rc = pack_linear(c, &c->query, {{qk.data.data(), (int)qk.shape[0]}}, c->att, qb.data.data(), 0, false))) return rc;
        const HostTensor &vk = T(c, "decoder.attention.value.kernel"), &vb = T(c, "decoder.attention.value.bias");
        const int goff = g.gst_use ? g.gst_att : 0;     // memory channel order [gst | enc] (GST.py:121-124)
        if (g.gst_use)
            if ((rc = pack_linear(c, &c->val_gst, {{vk.data.data(), g.gst_att}}, c->att, vb.data.data(), 0))) return rc;
        // (with GST the bias rides in val_gst's row bias: enqueue_value_proj)
        if ((rc = upload_dense(c, &c->val_enc, vk.data.data() + (size_t)goff * c->att, c->enc_out, c->att, c->att,
                               g.gst_use ? nullptr : vb.data.data(), true))) return rc;
        if (g.att_type == GSTTACO_ATT_LSA) {
            if ((rc = upload_tensor(c, &c->loc_cw, "decoder.attention.location_conv.kernel"))) return rc;
            if ((rc = upload_tensor(c, &c->loc_cb, "decoder.attention.location_conv.bias"))) return rc;
            if ((rc = upload_tensor(c, &c->loc_dw, "decoder.attention.location_dense.kernel"))) return rc;
            if ((rc = upload_tensor(c, &c->loc_db, "decoder.attention.location_dense.bias"))) return rc;
            if ((rc = upload_tensor(c, &c->att_bias, "decoder.attention.bias"))) return rc;
            {   // the same five tensors as the fused front end's LDS image (kernels.h LsaPack)
                const HostTensor &cw = T(c, "decoder.attention.location_conv.kernel"), &cb = T(c, "decoder.attention.location_conv.bias");
                const HostTensor &dw = T(c, "decoder.attention.location_dense.kernel"), &db = T(c, "decoder.attention.location_dense.bias");
                const HostTensor& ab = T(c, "decoder.attention.bias");
                const int LF = g.loc_filters, LK = g.loc_kernel, A = c->att;
                const LsaPack lp = gt_lsa_pack(A, LF, LK);
                std::vector<float> img((size_t)lp.total, 0.f);
                for (int f = 0; f < LF; ++f)
                    for (int a = 0; a < A; ++a) img[(size_t)f * lp.LDWS + a] = dw.data[(size_t)f * A + a];
                for (int j = 0; j < LK; ++j)
                    for (int f = 0; f < LF; ++f) img[lp.off_cw + (size_t)j * lp.LCS + f] = cw.data[(size_t)j * LF + f];
                for (int f = 0; f < LF; ++f) img[lp.off_cb + f] = cb.data[f];
                for (int a = 0; a < A; ++a) img[lp.off_ab + a] = db.data[a] + ab.data[a];
                if ((rc = upload(c, &c->loc_pack, img.data(), img.size()))) return rc;
            }
        } else {
            const HostTensor& av = T(c, "decoder.attention.v");
            if ((rc = upload(c, &c->att_v, av.data.data(), av.data.size()))) return rc;
            const HostTensor& sb = T(c, "decoder.attention.score_bias");
            if ((rc = upload(c, &c->att_sb, sb.data.data(), 1))) return rc;
        }
        for (int l = 0; l < 2; ++l) {
            std::string p = "decoder.lstm" + std::to_string(l);
            const HostTensor &k = T(c, p + ".kernel"), &u = T(c, p + ".recurrent_kernel"), &b = T(c, p + ".bias");
            const int Hl = l == 0 ? c->H1 : c->H2;          // (the padded size where the decoder was padded)
            if ((rc = pack_linear(c, l == 0 ? &c->lstm0 : &c->lstm1,
                                  {{k.data.data(), (int)k.shape[0]}, {u.data.data(), (int)u.shape[0]}},
                                  4 * Hl, b.data.data(), Hl))) return rc;
            // split form: z = x.W_x + (h_prev.W_h + b); the second term is computed by the front kernel's workers
            if ((rc = pack_linear(c, &c->lstm_x[l], {{k.data.data(), (int)k.shape[0]}}, 4 * Hl, nullptr, Hl))) return rc;
            if ((rc = pack_linear(c, &c->lstm_h[l], {{u.data.data(), (int)u.shape[0]}}, 4 * Hl, b.data.data(), Hl))) return rc;
        }
        const HostTensor &pk = T(c, "decoder.projection.kernel"), &pb = T(c, "decoder.projection.bias");
        if ((rc = pack_linear(c, &c->proj, {{pk.data.data(), (int)pk.shape[0]}}, c->proj_out, pb.data.data(), 0))) return rc;
        // The projection and the first prenet Dense are both linear and nothing sits between them at inference
        // (Taco2.py:186 feeds decodings[:, -1] straight into the prenet): frame.W0 + b0 = [h2|ctx].(Wp_last.W0) +
        // (bp_last.W0 + b0), Wp_last = the projection columns of the last of the r frames.  The fused columns ride in the
        // projection launch, so the next step's front kernel starts at prenet 1 with 80 KB less to pull.
        const int K = (int)pk.shape[0], N0 = c->proj_out, mel = g.mel_dim, P0 = c->P0, last = (c->r - 1) * mel;
        c->z_col0 = (N0 + 15) / 16 * 16;
        const int NE = c->z_col0 + P0;
        std::vector<float> we((size_t)K * NE, 0.f), be(NE, 0.f);
        for (int k = 0; k < K; ++k) {
            for (int n = 0; n < N0; ++n) we[(size_t)k * NE + n] = pk.data[(size_t)k * N0 + n];
            for (int cc = 0; cc < P0; ++cc) {
                double a = 0.0;
                for (int j = 0; j < mel; ++j) a += (double)pk.data[(size_t)k * N0 + last + j] * (double)k0.data[(size_t)j * P0 + cc];
                we[(size_t)k * NE + c->z_col0 + cc] = (float)a;
            }
        }
        for (int n = 0; n < N0; ++n) be[n] = pb.data[n];
        for (int cc = 0; cc < P0; ++cc) {
            double a = b0.data[cc];
            for (int j = 0; j < mel; ++j) a += (double)pb.data[last + j] * (double)k0.data[(size_t)j * P0 + cc];
            be[c->z_col0 + cc] = (float)a;
        }
        if ((rc = pack_linear(c, &c->proj_z, {{we.data(), K}}, NE, be.data(), 0))) return rc;
    }
    return 0;
}

int finalize_postnet(gsttaco_ctx* c) {
    int rc = 0;
    c->post_conv.resize(c->cfg.n_post);
    for (int i = 0; i < c->cfg.n_post && !rc; ++i) rc = upload_conv(c, &c->post_conv[i], "postnet.conv" + std::to_string(i), true, postnet_input_is_tanh(c->cfg, i));
    return rc;
}

// CBHG vocoder.  No call of enqueue_vocoder passes a Winograd or split form, so none is built (not for its five-tap layers either).
int finalize_vocoder(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    int rc = 0;
    c->voc_bank.resize(g.bank_count);
    for (int i = 0; i < g.bank_count; ++i)
        if ((rc = upload_conv(c, &c->voc_bank[i], "vocoder.convbank" + std::to_string(i), false))) return rc;
    c->voc_proj.resize(g.n_voc_proj);
    for (int i = 0; i < g.n_voc_proj; ++i)
        if ((rc = upload_conv(c, &c->voc_proj[i], "vocoder.proj" + std::to_string(i), false))) return rc;
    // a Dense as the checkpoint holds it: name.kernel [K, N], name.bias [N]
    auto dense = [&](ConvLayer* L, const std::string& name) {
        const HostTensor &k = T(c, name + ".kernel"), &b = T(c, name + ".bias");
        return upload_dense(c, L, k.data.data(), (int)k.shape[0], (int)k.shape[1], (int)k.shape[1], b.data.data(), false);
    };
    if (c->weights.index.count("vocoder.proj_dense.kernel") && (rc = dense(&c->voc_pd, "vocoder.proj_dense"))) return rc;
    if (c->weights.index.count("vocoder.highway_in.kernel") && (rc = dense(&c->voc_hin, "vocoder.highway_in"))) return rc;
    const int S = g.highway_size;
    c->voc_hw.resize(g.highway_count);
    for (int i = 0; i < g.highway_count; ++i) {
        // one GEMM per layer: columns [0,S) = Dense_Relu, [S,2S) = Dense_Sigmoid (Taco2.py:412-420)
        const std::string p = "vocoder.highway" + std::to_string(i);
        const HostTensor &wr = T(c, p + ".relu.kernel"), &br = T(c, p + ".relu.bias");
        const HostTensor &ws = T(c, p + ".sigmoid.kernel"), &bs = T(c, p + ".sigmoid.bias");
        std::vector<float> wcat((size_t)S * 2 * S), bcat(2 * S);
        for (int k = 0; k < S; ++k)
            for (int n = 0; n < S; ++n) {
                wcat[(size_t)k * 2 * S + n] = wr.data[(size_t)k * S + n];
                wcat[(size_t)k * 2 * S + S + n] = ws.data[(size_t)k * S + n];
            }
        for (int n = 0; n < S; ++n) { bcat[n] = br.data[n]; bcat[S + n] = bs.data[n]; }
        if ((rc = upload_dense(c, &c->voc_hw[i], wcat.data(), S, 2 * S, 2 * S, bcat.data(), false))) return rc;
    }
    if ((rc = finalize_bilstm(c, c->voc_bilstm, &c->voc_lean, "vocoder.bilstm", g.voc_rnn))) return rc;
    // final Dense: rows padded to a multiple of 4 columns so the GEMM can load 16 bytes per lane
    const HostTensor &k = T(c, "vocoder.dense.kernel"), &b = T(c, "vocoder.dense.bias");
    const int K = (int)k.shape[0], N = g.spec_dim, ldw = (N + 3) / 4 * 4;
    std::vector<float> wpad((size_t)K * ldw, 0.f);
    for (int r = 0; r < K; ++r) memcpy(&wpad[(size_t)r * ldw], &k.data[(size_t)r * N], (size_t)N * sizeof(float));
    return upload_dense(c, &c->voc_dense, wpad.data(), K, N, ldw, b.data.data(), false);
}

// the workspace, sized once for the capacity given at create
int alloc_workspace(gsttaco_ctx* c) {
    const gsttaco_config& g = c->cfg;
    int rc = 0;
    const size_t B = g.max_batch, Tv = g.max_tokens, S = c->steps_max, Tf = S * c->r, mel = g.mel_dim;
    auto fa = [&](float** p, size_t n) { return dev_alloc(c, (void**)p, n * sizeof(float)); };
    if ((rc = dev_alloc(c, (void**)&c->w_tokens, B * Tv * 4))) return rc;
    if ((rc = dev_alloc(c, (void**)&c->w_mel_len, B * 4))) return rc;
    if ((rc = dev_alloc(c, (void**)&c->w_tok_len, B * 4))) return rc;
    if ((rc = dev_alloc(c, (void**)&c->w_seed, 16))) return rc;
    if ((rc = dev_alloc(c, (void**)&c->w_dbg, 3 * 32 * 8))) return rc;       // ([3][16] for the launch path's kernels, [3][32] for the persistent decode launch)
    HIPCHECK(c, hipMemset(c->w_dbg, 0, 3 * 32 * 8));
    if ((rc = fa(&c->w_masks, S * B * (c->P0 + c->P1)))) return rc;
    if ((rc = fa(&c->w_noise, S * B * Tv))) return rc;
    size_t actc = g.emb;
    for (int i = 0; i < g.n_enc_conv; ++i) actc = std::max<size_t>(actc, g.enc_filters[i]);
    for (int i = 0; i < 2; ++i)
        if ((rc = fa(&c->w_act[i], B * Tv * actc))) return rc;
    if ((rc = fa(&c->w_enc, B * Tv * c->enc_out))) return rc;
    if ((rc = fa(&c->w_cenc, 2 * B * g.enc_rnn))) return rc;
    if ((rc = alloc_lean_bilstm(c, &c->enc_lean, B, Tv))) return rc;
    if ((rc = fa(&c->w_z0, B * (size_t)c->P0))) return rc;
    c->zero_floats = ((B + 15) / 16 * 16) * std::max<size_t>({(size_t)mel, (size_t)g.enc_rnn, (size_t)c->H1, (size_t)c->H2,
                                                               (size_t)(g.voc_use ? g.voc_rnn : 0)});
    if ((rc = fa(&c->w_zero, c->zero_floats))) return rc;
    HIPCHECK(c, hipMemset(c->w_zero, 0, c->zero_floats * sizeof(float)));
    if (g.gst_use) {
        const size_t Tr = g.max_ref_frames;
        if ((rc = fa(&c->w_mels_in, B * Tr * mel))) return rc;
        size_t big = 0;
        int H = (int)Tr - 1, W = (int)mel;
        for (int i = 0; i < g.n_ref_conv; ++i) {
            H = (H + g.ref_strides[i] - 1) / g.ref_strides[i];
            W = (W + g.ref_strides[i] - 1) / g.ref_strides[i];
            big = std::max(big, (size_t)H * W * g.ref_filters[i]);
        }
        for (int i = 0; i < 2; ++i)
            if ((rc = fa(&c->w_gconv[i], B * big))) return rc;
        if ((rc = fa(&c->w_gst, B * g.gst_att))) return rc;
        if ((rc = fa(&c->w_gst_attn, B * (size_t)g.heads * g.n_tokens))) return rc;
        if ((rc = fa(&c->w_gst_q, B * g.gst_att))) return rc;
        if ((rc = fa(&c->w_rowbias, B * c->att))) return rc;
    }
    if ((rc = fa(&c->w_pm, B * Tv * c->att))) return rc;
    if ((rc = fa(&c->w_lsa_state, B * Tv))) return rc;
    if ((rc = fa(&c->w_p1, B * c->P0))) return rc;
    const size_t Bp = (B + 15) / 16 * 16;       // blocked activation buffers hold whole 16-row tiles
    if ((rc = fa(&c->w_xa, Bp * (c->P1 + c->att)))) return rc;
    HIPCHECK(c, hipMemset(c->w_xa, 0, Bp * (c->P1 + c->att) * sizeof(float)));
    if (c->lstm_x[0].bf16 && c->lstm_x[1].bf16 && c->lstm_h[0].bf16 && c->lstm_h[1].bf16 && c->proj.bf16 &&
        (c->P1 + c->att) % 32 == 0 && c->P1 % 32 == 0 && c->H1 % 32 == 0 && c->H2 % 32 == 0) {
        float* t = nullptr;
        if ((rc = fa(&t, Bp * (c->P1 + c->att) / 2))) return rc;
        c->w_xa_h = reinterpret_cast<uint16_t*>(t);
        HIPCHECK(c, hipMemset(t, 0, Bp * (c->P1 + c->att) * 2));
        if ((rc = fa(&t, Bp * (c->P1 + c->att) / 2))) return rc;        // (the persistent bf16 kernel ping-pongs it by step parity)
        c->w_xa2_h = reinterpret_cast<uint16_t*>(t);
        HIPCHECK(c, hipMemset(t, 0, Bp * (c->P1 + c->att) * 2));
        for (int i = 0; i < 2; ++i) {
            if ((rc = fa(&t, Bp * c->H1 / 2))) return rc;
            c->w_h1_h[i] = reinterpret_cast<uint16_t*>(t);
            if ((rc = fa(&t, Bp * c->H2 / 2))) return rc;
            c->w_h2_h[i] = reinterpret_cast<uint16_t*>(t);
        }
    }
    if ((rc = fa(&c->w_q, B * c->att))) return rc;
    for (int i = 0; i < 2; ++i) {
        if ((rc = fa(&c->w_h1[i], Bp * c->H1))) return rc;
        if ((rc = fa(&c->w_h2[i], Bp * c->H2))) return rc;
    }
    if ((rc = fa(&c->w_part[0], Bp * 4 * c->H1))) return rc;
    if ((rc = fa(&c->w_part[1], Bp * 4 * c->H2))) return rc;
    if ((rc = dev_alloc(c, (void**)&c->w_arrive, (size_t)S * GT_L12_NSH * 32 * sizeof(uint32_t)))) return rc;
    // persistent decode launch (persist_decode.hip): second prenet | context buffer (ping-pong by step parity), prenet-0 granules,
    // the chain workgroups' recurrent halves, control words
    if ((rc = fa(&c->w_xa2, Bp * (c->P1 + c->att)))) return rc;
    HIPCHECK(c, hipMemset(c->w_xa2, 0, Bp * (c->P1 + c->att) * sizeof(float)));
    if ((rc = dev_alloc(c, (void**)&c->w_z0g, std::max<size_t>(32, B) * 256 * sizeof(uint2)))) return rc;
    if ((rc = fa(&c->w_hpart, (size_t)2 * 64 * 1024))) return rc;         // (fp32 kernel: [2][32 tiles][512]; bf16 kernel: [2][64 tiles][1024])
    if (B > 32 && (rc = fa(&c->w_stash, (size_t)256 * 16 * 512))) return rc;      // (the group kernels: batches above 32 rows)
    if ((rc = dev_alloc(c, (void**)&c->w_pctl, gt_persist_decode_ctl_words() * sizeof(uint32_t)))) return rc;
    // the give-up words of the in-kernel hand-offs live in host-mapped memory: the device raises them with a system-scope
    // atomic (failure path only), the host reads them without a synchronisation at the start of the next call
    HIPCHECK(c, hipHostMalloc((void**)&c->h_err, 16, hipHostMallocMapped));
    memset(c->h_err, 0, 16);
    HIPCHECK(c, hipHostGetDevicePointer((void**)&c->w_err, c->h_err, 0));
    if ((rc = fa(&c->w_c1, B * c->H1))) return rc;
    if ((rc = fa(&c->w_c2, B * c->H2))) return rc;
    if ((rc = fa(&c->w_pre, B * Tf * mel))) return rc;
    if ((rc = fa(&c->w_stop, B * S))) return rc;
    if ((rc = fa(&c->w_align, B * S * Tv))) return rc;
    size_t postc = mel;
    for (int i = 0; i < g.n_post; ++i) postc = std::max<size_t>(postc, g.post_filters[i]);
    for (int i = 0; i < 2; ++i)
        if ((rc = fa(&c->w_post[i], B * Tf * postc))) return rc;
    if ((rc = fa(&c->w_mel, B * Tf * mel))) return rc;
    if (g.voc_use) {
        const size_t banks = (size_t)g.bank_count * g.bank_filters;
        size_t wide = std::max<size_t>({(size_t)mel, (size_t)g.highway_size});
        for (int i = 0; i < g.n_voc_proj; ++i) wide = std::max<size_t>(wide, g.voc_proj_filters[i]);
        if ((rc = fa(&c->w_vbank, B * Tf * banks))) return rc;
        for (int i = 0; i < 3; ++i)
            if ((rc = fa(&c->w_vbuf[i], B * Tf * wide))) return rc;
        if ((rc = fa(&c->w_vz, B * Tf * 2 * g.highway_size))) return rc;
        if ((rc = fa(&c->w_vrnn, B * Tf * 2 * g.voc_rnn))) return rc;
        if ((rc = fa(&c->w_vc, 2 * B * g.voc_rnn))) return rc;
        if ((rc = alloc_lean_bilstm(c, &c->voc_lean, B, Tf))) return rc;
        if ((rc = fa(&c->w_spec, B * Tf * g.spec_dim))) return rc;
    }
    return 0;
}

// ---- what the three vocoders (gsttaco_melgan_* / _waveglow_* / _hifigan_*) share.  V is the context's member for one of them
// (configured, finalized, cfg, plan, man); `model` its name, which starts every message ("melgan: ...").
template <typename V>
int voc_not_open(const gsttaco_ctx* c, const V& g, const char* model) {        // what load_weight and finalize refuse first
    if (!g.configured) return fail(c, GSTTACO_E_WEIGHTS, std::string(model) + ": not configured (gsttaco_" + model + "_configure)");
    if (g.finalized) return fail(c, GSTTACO_E_WEIGHTS, std::string(model) + ": weights already finalized");
    return 0;
}

template <typename V>
int voc_load_weight(gsttaco_ctx* c, V gsttaco_ctx::*which, const char* model, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!c || !name || !host || !shape) return fail(c, GSTTACO_E_INVALID, "null argument");
    V& g = c->*which;
    if (int rc = voc_not_open(c, g, model)) return rc;
    return g.man.load(c, (std::string(model) + ": ").c_str(), name, host, shape, ndim);
}

// finalize's prologue: configured, not yet finalized, every tensor loaded
template <typename V>
int voc_begin_finalize(gsttaco_ctx* c, const V& g, const char* model) {
    if (int rc = voc_not_open(c, g, model)) return rc;
    if (const HostTensor* t = g.man.first_unloaded()) return fail(c, GSTTACO_E_WEIGHTS, std::string(model) + ": weight '" + t->name + "' was not loaded");
    return 0;
}

int upload_vec(gsttaco_ctx* c, const float** dst, const std::vector<float>& v) {
    float* d = nullptr;
    int e = upload(c, &d, v.data(), v.size());
    *dst = d;
    return e;
}

// the bias `name` (plus the bias `plus`, unless empty) zero-padded to n_p floats, on the device
int upload_padded_bias(gsttaco_ctx* c, const Manifest& man, const float** dst, const std::string& name, const std::string& plus, int n_p) {
    std::vector<float> buf(n_p, 0.f);
    const std::vector<float>& b = man.host(name);
    for (size_t i = 0; i < b.size(); ++i) buf[i] = b[i];
    if (!plus.empty()) {
        const std::vector<float>& b2 = man.host(plus);
        for (size_t i = 0; i < b2.size(); ++i) buf[i] += b2[i];
    }
    return upload_vec(c, dst, buf);
}

// [taps * cin, cout] as the fp32 fragment pack (voc_pack_f32), on the device
int upload_packed(gsttaco_ctx* c, const float** dst, const std::vector<float>& w, int taps, int cin, int cout) {
    std::vector<float> buf((size_t)taps * voc_pad16(cin) * voc_pad16(cout));
    voc_pack_f32(w.data(), taps, cin, cout, buf.data());
    return upload_vec(c, dst, buf);
}

// HiFi-GAN: the manifest's name of a launch's weights, without the /kernel or /bias leaf
std::string hifigan_name(const HgStage& s) {
    if (s.kind == GT_HG_IN) return "hifigan/in";
    if (s.kind == GT_HG_OUT) return "hifigan/out";
    std::string p = "hifigan/up" + std::to_string(s.up);
    if (s.kind == GT_HG_UP) return p;
    return p + "/res" + std::to_string(s.block) + "/unit" + std::to_string(s.unit) + (s.conv ? "/conv2" : "/conv1");
}

// What every vocoder call refuses, in the order it always has.  after_null / after_bt: a further refusal of the caller's own
// (GSTTACO_E_INVALID with that text) at the place where it fires, NULL where there is none.
template <typename V>
int voc_check_call(const gsttaco_ctx* c, const V& g, const char* model, const float* mel, const float* wav, int B, int T, int ld_wav,
                   const char* after_null = nullptr, const char* after_bt = nullptr) {
    if (!g.finalized) return fail(c, GSTTACO_E_WEIGHTS, std::string(model) + ": weights not finalized (gsttaco_" + model + "_finalize)");
    if (!mel || !wav) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (after_null) return fail(c, GSTTACO_E_INVALID, after_null);
    if (B < 1 || T < 1) return fail(c, GSTTACO_E_INVALID, "bad B / T");
    if (after_bt) return fail(c, GSTTACO_E_INVALID, after_bt);
    if (B > g.cfg.max_batch || T > g.cfg.max_frames) return fail(c, GSTTACO_E_CAPACITY, std::string(model) + ": B or T exceeds the capacity given at configure");
    if ((int64_t)ld_wav < (int64_t)T * g.plan.hop) return fail(c, GSTTACO_E_INVALID, "ld_wav must be >= T * hop");
    return 0;
}

// The call of a chain with `ws` buffers (MgCall / HgCall) behind voc_check_call
template <typename Call, typename V>
int voc_chain_call(const gsttaco_ctx* c, const V& g, const char* model, Call* a, const float* mel, const int32_t* frames, int B, int T, float* wav,
                   int32_t* wav_lengths, int ld_wav, int only) {
    if (int rc = voc_check_call(c, g, model, mel, wav, B, T, ld_wav)) return rc;
    a->mel = mel; a->frames = frames; a->wav = wav; a->wav_lengths = wav_lengths;
    for (size_t k = 0; k < sizeof(g.ws) / sizeof(g.ws[0]); ++k) a->ws[k] = g.ws[k];
    a->B = B; a->T = T; a->ld_wav = ld_wav; a->only = only;
    return 0;
}

}  // namespace

extern "C" {

int gsttaco_finalize_weights(gsttaco_ctx* c) {
    if (!c) return GSTTACO_E_INVALID;
    if (c->finalized) return 0;
    for (auto& t : c->weights.tensors)
        if (!t.loaded) return fail(c, GSTTACO_E_WEIGHTS, "missing weight '" + t.name + "'");
    const gsttaco_config& g = c->cfg;
    int rc = ensure_device(c);
    if (rc) return rc;
    HIPCHECK(c, hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    HIPCHECK(c, hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    HIPCHECK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHECK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    if ((rc = finalize_encoder(c))) return rc;
    if (g.gst_use && (rc = finalize_gst(c))) return rc;
    if ((rc = finalize_decoder_step(c))) return rc;
    if ((rc = finalize_postnet(c))) return rc;
    if (g.voc_use && (rc = finalize_vocoder(c))) return rc;
    if ((rc = alloc_workspace(c))) return rc;
    HIPCHECK(c, gt_attn_init());
    HIPCHECK(c, gt_dec_front_init());
    HIPCHECK(c, gt_gst_init());
    HIPCHECK(c, gt_bilstm_persist_init());
    HIPCHECK(c, gt_conv5_bf16_init());
    HIPCHECK(c, gt_conv_wino5s_init());
    HIPCHECK(c, gt_persist_decode_init());
    // the persistent BiLSTM's groups need their 32 members each on a CU of their own: exactly one workgroup per CU must fit
    if (c->allow.bilstm_persist && gt_bilstm_persist_blocks_per_cu() != 1) {
        c->allow.bilstm_persist = false;
        c->warn = c->err = "warning: the persistent BiLSTM kernel does not get one workgroup per compute unit on this device; using one launch per time step";
    }
    // the fused decode-LSTM launches hand h1 over in-kernel: their whole grid must be resident (occupancy x CUs of THIS device;
    // a partition with fewer CUs than the grid simply keeps the two-launch form)
    for (int i = 0; i < 3; ++i) c->fuse12_slots[i] = gt_lstm12_blocks_per_cu(i) * c->n_cu;
    c->persist_slots = gt_persist_decode_blocks_per_cu() * c->n_cu;
    if (c->allow.fuse12 && c->H1 == c->H2 && (c->H1 + 3) / 4 > c->fuse12_slots[0])
        c->warn = c->err = "warning: this device cannot hold the fused decode-LSTM launch's whole grid at once (" + std::to_string((c->H1 + 3) / 4) +
                           " workgroups, " + std::to_string(c->fuse12_slots[0]) + " resident): the two LSTM cells run as two launches";
    HIPCHECK(c, hipDeviceSynchronize());
    // host copies are no longer needed
    for (auto& t : c->weights.tensors) std::vector<float>().swap(t.data);
    c->padded.clear();
    c->finalized = true;
    return 0;
}

int gsttaco_encode(gsttaco_ctx* c, const int32_t* tokens, const int32_t* token_lengths, int B, int Tv, float* enc, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!tokens || !enc) return fail(c, GSTTACO_E_INVALID, "null argument");
    if ((rc = check_shape(c, B, Tv, 0, 0))) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(c, hipMemcpyAsync(c->w_tokens, tokens, (size_t)B * Tv * 4, hipMemcpyDeviceToDevice, s));
    const bool masked = token_lengths != nullptr;
    if (masked) HIPCHECK(c, hipMemcpyAsync(c->w_tok_len, token_lengths, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = run_cached(c, s, GraphKey{.kind = kSegEncoder, .B = B, .Tv = Tv, .masked = masked},
                         [&](hipStream_t st, const LaunchForms& forms) { return enqueue_encoder(c, st, forms, B, Tv, masked); }))) return rc;
    HIPCHECK(c, hipMemcpyAsync(enc, c->w_enc, (size_t)B * Tv * c->enc_out * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int gsttaco_gst_ex(gsttaco_ctx* c, const float* mels, const int32_t* lens, int B, int Tref1, float* gst, float* token_weights, float* query,
                   void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->cfg.gst_use) return fail(c, GSTTACO_E_INVALID, "GST is not used");     // reference Model.py:258-259
    if (!mels || !lens || !gst) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (Tref1 < 2) return fail(c, GSTTACO_E_INVALID, "mels_for_gst needs at least one frame after the prepended zero frame");
    if ((rc = check_shape(c, B, 1, Tref1, 0))) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(c, hipMemcpyAsync(c->w_mels_in, mels, (size_t)B * Tref1 * c->cfg.mel_dim * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(c, hipMemcpyAsync(c->w_mel_len, lens, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = run_cached(c, s, GraphKey{.kind = kSegGst, .B = B, .Tref1 = Tref1},
                         [&](hipStream_t st, const LaunchForms&) { return enqueue_gst(c, st, B, Tref1); }))) return rc;
    HIPCHECK(c, hipMemcpyAsync(gst, c->w_gst, (size_t)B * c->cfg.gst_att * 4, hipMemcpyDeviceToDevice, s));
    if (token_weights)
        HIPCHECK(c, hipMemcpyAsync(token_weights, c->w_gst_attn, (size_t)B * c->cfg.heads * c->cfg.n_tokens * 4, hipMemcpyDeviceToDevice, s));
    if (query) HIPCHECK(c, hipMemcpyAsync(query, c->w_gst_q, (size_t)B * c->cfg.gst_att * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int gsttaco_gst(gsttaco_ctx* c, const float* mels, const int32_t* lens, int B, int Tref1, float* gst, void* stream) {
    return gsttaco_gst_ex(c, mels, lens, B, Tref1, gst, nullptr, nullptr, stream);
}

// EXTENSION (style control): gst = LayerNorm(concat_h(weights[b, h, :] . V[:, h-slice]) + query), the style-token layer's last stage
// (Layers.py:207-211) with the attention weights given.  One launch, straight from / to the caller's pointers.
int gsttaco_style_compose(gsttaco_ctx* c, const float* token_weights, const float* query, int B, float* gst, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    const gsttaco_config& g = c->cfg;
    if (!g.gst_use) return fail(c, GSTTACO_E_INVALID, "GST is not used");
    if (!token_weights || !gst) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1) return fail(c, GSTTACO_E_INVALID, "bad B");
    if (B > g.max_batch) return fail(c, GSTTACO_E_CAPACITY, "batch exceeds the capacity given at create");
    GstComposeArgs a{};
    a.weights = token_weights; a.query = query; a.v_tok = c->v_tok; a.ln_g = c->ln_g; a.ln_b = c->ln_b; a.gst = gst;
    a.B = B; a.A = g.gst_att; a.ntok = g.n_tokens; a.heads = g.heads;
    a.gru_in = (int)ref_gru_in(g); a.u = g.ref_rnn; a.D = g.ref_dense;
    HIPCHECK(c, gt_launch_gst_compose(a, (hipStream_t)stream));
    return 0;
}

int gsttaco_decode(gsttaco_ctx* c, const float* enc, const float* gst, const int32_t* token_lengths, const float* mask,
                   const float* noise, uint64_t seed, int B, int Tv, int steps, float* pre_mel, float* stop, float* align,
                   void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!enc || !pre_mel || !stop || !align || (c->cfg.gst_use && !gst)) return fail(c, GSTTACO_E_INVALID, "null argument");
    if ((rc = check_shape(c, B, Tv, 0, steps))) return rc;
    if (steps == 0) steps = c->steps_max;
    return decode_call(c, enc, gst, token_lengths, mask, noise, seed, B, Tv, steps, nullptr, 0, pre_mel, stop, align, stream);
}

// gsttaco_decode teacher-forced: S = ceil((Tq - 1) / r) steps, graph segment kSegDecodeForced
int gsttaco_decode_forced(gsttaco_ctx* c, const float* enc, const float* gst, const int32_t* token_lengths, const float* mask,
                          const float* noise, uint64_t seed, int B, int Tv, const float* teacher, int Tq, float* pre_mel, float* stop,
                          float* align, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!enc || !pre_mel || !stop || !align || (c->cfg.gst_use && !gst)) return fail(c, GSTTACO_E_INVALID, "null argument");
    int steps = 0;
    if ((rc = check_forced(c, teacher, Tq, B, Tv, 0, &steps))) return rc;
    return decode_call(c, enc, gst, token_lengths, mask, noise, seed, B, Tv, steps, teacher, Tq, pre_mel, stop, align, stream);
}

// Per-token frame counts of a (forced) alignment: one launch on the caller's stream straight from / to the caller's pointers.  Needs
// no weights (only Step_Reduction), so it works before finalize.
int gsttaco_forced_durations(gsttaco_ctx* c, const float* align, const int32_t* token_lengths, const int32_t* mel_lengths, int B, int S,
                             int Tv, int32_t* durations, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!align || !durations) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || S < 1 || Tv < 1) return fail(c, GSTTACO_E_INVALID, "bad B / S / Tv");
    if (S > c->steps_max || B > c->cfg.max_batch || Tv > c->cfg.max_tokens)
        return fail(c, GSTTACO_E_CAPACITY, "batch / tokens / steps exceed the capacity given at create");
    int rc = ensure_device(c);
    if (rc) return rc;
    HIPCHECK(c, gt_launch_forced_durations(align, token_lengths, mel_lengths, durations, B, S, Tv, c->r, (hipStream_t)stream));
    return 0;
}

// Per-utterance seeds: the randomness of a whole decode in the layouts every prenet_mask / attn_noise argument takes, row b drawn from
// seeds[b] as a batch of one draws its row 0.  One launch on the caller's stream straight into the caller's buffers; needs no weights.
int gsttaco_fill_randomness(gsttaco_ctx* c, const uint64_t* seeds, int B, int Tv, int steps, float* prenet_mask, float* attn_noise,
                            void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!seeds || (!prenet_mask && !attn_noise)) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || steps < 1 || Tv < 1) return fail(c, GSTTACO_E_INVALID, "bad B / steps / Tv");
    if (steps > c->steps_max || B > c->cfg.max_batch || Tv > c->cfg.max_tokens)
        return fail(c, GSTTACO_E_CAPACITY, "batch / tokens / steps exceed the capacity given at create");
    // (the caller's, unpadded, sizes: what an injected mask tensor has -- stage_decode_inputs re-lays it out for a padded decoder)
    const int p0 = c->cfg.prenet[0], p1 = c->cfg.prenet[1];
    if (prenet_mask && p0 != p1) return fail(c, GSTTACO_E_INVALID, "the injected mask layout [steps][2][B][prenet] needs equal prenet layer sizes");
    int rc = ensure_device(c);
    if (rc) return rc;
    HIPCHECK(c, gt_launch_fill_randomness(seeds, prenet_mask, attn_noise, steps, B, p0, p1, Tv, c->cfg.prenet_rate, (hipStream_t)stream));
    return 0;
}

// The synthesis report of a decode's stop logits and alignments (and, when given, its mels): one launch, one workgroup per utterance,
// straight from / to the caller's pointers.  Needs no weights (only Step_Reduction and Mel_Dim).
int gsttaco_utterance_report(gsttaco_ctx* c, const float* stop, const float* align, const int32_t* token_lengths, const float* mel, int B,
                             int S, int Tv, int32_t* report, float* focus, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!stop || !align || !report) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || S < 1 || Tv < 1) return fail(c, GSTTACO_E_INVALID, "bad B / S / Tv");
    if (S > c->steps_max || B > c->cfg.max_batch || Tv > c->cfg.max_tokens)
        return fail(c, GSTTACO_E_CAPACITY, "batch / tokens / steps exceed the capacity given at create");
    int rc = ensure_device(c);
    if (rc) return rc;
    HIPCHECK(c, gt_launch_utterance_report(stop, align, token_lengths, mel, report, focus, B, S, Tv, c->r, c->cfg.mel_dim, (hipStream_t)stream));
    return 0;
}

// The loss sums of a teacher-forced pass (the four terms of Train_Step, Model.py:210-241, per utterance): one launch, one workgroup per
// utterance, straight from / to the caller's pointers.  Needs no weights (only Step_Reduction, Mel_Dim and Spectrogram_Dim).
int gsttaco_losses(gsttaco_ctx* c, const float* pre_mel, const float* mel, const float* stop, const float* spectrogram,
                   const float* teacher, const float* spec_target, const int32_t* mel_lengths, const int32_t* spec_lengths, int B, int S,
                   int Tq, double* losses, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!pre_mel || !mel || !stop || !teacher || !losses) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || S < 1 || Tq < 2 || (int64_t)S * c->r < Tq - 1) return fail(c, GSTTACO_E_INVALID, "bad B / S / Tq (Tq >= 2, S * r >= Tq - 1)");
    if (S > c->steps_max || B > c->cfg.max_batch)
        return fail(c, GSTTACO_E_CAPACITY, "batch / steps exceed the capacity given at create");
    if (spectrogram && spec_target && c->cfg.spec_dim < 1) return fail(c, GSTTACO_E_INVALID, "Sound.Spectrogram_Dim not set");
    int rc = ensure_device(c);
    if (rc) return rc;
    LossArgs a{};
    a.pre_mel = pre_mel; a.mel = mel; a.stop = stop; a.spec = spectrogram; a.teacher = teacher; a.spec_target = spec_target;
    a.mel_len = mel_lengths; a.spec_len = spec_lengths; a.losses = losses;
    a.B = B; a.S = S; a.Tq = Tq; a.r = c->r; a.mel_dim = c->cfg.mel_dim; a.spec_dim = c->cfg.spec_dim > 0 ? c->cfg.spec_dim : 1;
    HIPCHECK(c, gt_launch_losses(a, (hipStream_t)stream));
    return 0;
}

// The workspace of gsttaco_mel_dtw, sized by the capacity given at create and allocated on first use like the forced decode's
// (ensure_forced); *basis = the device copy of rows 1..n_ceps of the orthonormal DCT-II over the channels (NULL for n_ceps 0).
static int ensure_dtw(gsttaco_ctx* c, int n_ceps, bool with_path, const double** basis) {
    const gsttaco_config& g = c->cfg;
    const size_t T = (size_t)g.max_step, M = (size_t)g.mel_dim;
    int rc = 0;
    if (!c->w_dtw_fx) {
        HIPCHECK(c, gt_dtw_init());
        if ((rc = dev_alloc(c, (void**)&c->w_dtw_fx, (size_t)g.max_batch * T * M * sizeof(double)))) return rc;
    }
    if (!c->w_dtw_fy && (rc = dev_alloc(c, (void**)&c->w_dtw_fy, (size_t)g.max_batch * T * M * sizeof(double)))) return rc;
    if (with_path && !c->w_dtw_bp && (rc = dev_alloc(c, (void**)&c->w_dtw_bp, (size_t)g.max_batch * T * T))) return rc;
    *basis = nullptr;
    if (n_ceps == 0) return 0;
    auto it = c->dtw_basis.find(n_ceps);
    if (it == c->dtw_basis.end()) {
        std::vector<double> h((size_t)n_ceps * M);
        const double norm = std::sqrt(2.0 / (double)M);
        for (int k = 1; k <= n_ceps; ++k)
            for (size_t m = 0; m < M; ++m) h[(size_t)(k - 1) * M + m] = norm * std::cos(M_PI * k * (2.0 * m + 1.0) / (2.0 * M));
        double* d = nullptr;
        if ((rc = dev_alloc(c, (void**)&d, h.size() * sizeof(double)))) return rc;
        HIPCHECK(c, hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        it = c->dtw_basis.emplace(n_ceps, d).first;
    }
    *basis = it->second;
    return 0;
}

// Mel-cepstral distortion along a DTW path: two launches on the caller's stream straight from / to the caller's pointers.  Needs no
// weights (only Mel_Dim, Max_Step and Max_Abs_Mel).
int gsttaco_mel_dtw(gsttaco_ctx* c, const float* x, const int32_t* x_len, int64_t x_stride, const float* y, const int32_t* y_len,
                    int64_t y_stride, int B, int Tx, int Ty, int n_ceps, double* cost, int32_t* path_len, int32_t* path, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    const gsttaco_config& g = c->cfg;
    if (!x || !y || !cost || !path_len) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || Tx < 1 || Ty < 1) return fail(c, GSTTACO_E_INVALID, "bad B / Tx / Ty");
    if (n_ceps < 0 || n_ceps >= g.mel_dim) return fail(c, GSTTACO_E_INVALID, "n_ceps must be in [0, Mel_Dim)");
    if (x_stride < 0 || y_stride < 0) return fail(c, GSTTACO_E_INVALID, "negative batch stride");
    if (B > g.max_batch || Tx > g.max_step || Ty > g.max_step)
        return fail(c, GSTTACO_E_CAPACITY, "batch / frames exceed the capacity given at create (max_batch, Max_Step)");
    if (gt_dtw_lds_bytes(Ty) > GT_DTW_MAX_LDS)
        return fail(c, GSTTACO_E_CAPACITY, "Ty exceeds the 4551 columns whose rolling diagonals fit a workgroup's LDS");
    int rc = ensure_device(c);
    if (rc) return rc;
    DtwArgs a{};
    if ((rc = ensure_dtw(c, n_ceps, path != nullptr, &a.basis))) return rc;
    a.x = x; a.y = y; a.x_len = x_len; a.y_len = y_len;
    a.x_stride = x_stride ? x_stride : (int64_t)Tx * g.mel_dim;
    a.y_stride = y_stride ? y_stride : (int64_t)Ty * g.mel_dim;
    const double db_per_unit = g.max_abs_mel > 0.f ? 100.0 / (2.0 * (double)g.max_abs_mel) : 100.0;
    a.scale = db_per_unit / std::sqrt(2.0);
    a.clip_lo = g.max_abs_mel > 0.f ? -g.max_abs_mel : 0.f;
    a.clip_hi = g.max_abs_mel > 0.f ? g.max_abs_mel : 1.f;
    a.fx = c->w_dtw_fx; a.fy = c->w_dtw_fy; a.backptr = c->w_dtw_bp;
    a.cost = cost; a.path_len = path_len; a.path = path;
    a.B = B; a.Tx = Tx; a.Ty = Ty; a.mel_dim = g.mel_dim; a.n_ceps = n_ceps;
    HIPCHECK(c, gt_launch_mel_dtw(a, (hipStream_t)stream));
    return 0;
}

// resampy's published 'kaiser_best' design (resampy/filters.py sinc_window): the right half of a Kaiser-windowed sinc, 64 zero crossings,
// 512 entries per crossing.  scipy.signal.windows.kaiser(2n + 1, beta)[n + j] = I0(beta sqrt(1 - (j / n)^2)) / I0(beta), I0 by its
// power series (all terms positive: no cancellation); numpy.sinc(x) = sin(pi x) / (pi x); linspace(0, 64, n + 1)[j] = j / 512 exactly.
static double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

static void kaiser_best_window(std::vector<double>& win) {
    const double beta = 14.769656459379492, rolloff = 0.9475937167399596;
    const int n = GT_RS_NWIN - 1;
    win.resize(GT_RS_NWIN);
    const double i0_beta = bessel_i0(beta);
    for (int j = 0; j <= n; ++j) {
        const double r = (double)j / (double)n;
        const double taper = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0_beta;
        const double px = M_PI * (rolloff * ((double)j / 512.0));
        const double sinc = j == 0 ? 1.0 : std::sin(px) / px;
        win[j] = taper * (rolloff * sinc);
    }
}

// The slot holding the tables of (sr_in, sr_out), built and uploaded on `s` when the cache does not hold the pair.  `clock` is this
// call's stamp: a slot stamped with it serves another row of the same call and is not evicted.
static int ensure_resample_pair(gsttaco_ctx* c, int sr_in, int sr_out, uint64_t clock, hipStream_t s, int* slot_out) {
    const int T = c->cfg.max_wav_samples;
    int victim = -1;
    for (int i = 0; i < GT_RS_MAX_PAIRS; ++i) {
        gsttaco_ctx::ResampleSlot& rs = c->rs_slot[i];
        if (rs.sr_in == sr_in && rs.sr_out == sr_out) {
            rs.last_use = clock;
            *slot_out = i;
            return 0;
        }
        if (rs.last_use != clock && (victim < 0 || rs.last_use < c->rs_slot[victim].last_use)) victim = i;
    }
    if (victim < 0) return fail(c, GSTTACO_E_INVALID, "internal: no resampling table slot left for this call");
    gsttaco_ctx::ResampleSlot& rs = c->rs_slot[victim];
    int rc = 0;
    if (!rs.d_time) {
        if ((rc = dev_alloc(c, (void**)&rs.d_time, (size_t)T * sizeof(double)))) return rc;
        if ((rc = dev_alloc(c, (void**)&rs.d_table, (size_t)GT_RS_NWIN * sizeof(double2)))) return rc;
        HIPCHECK(c, hipHostMalloc((void**)&rs.h_image, ((size_t)T + 2 * (size_t)GT_RS_NWIN) * sizeof(double), hipHostMallocDefault));
        HIPCHECK(c, hipEventCreateWithFlags(&rs.uploaded, hipEventDisableTiming));
    } else {
        HIPCHECK(c, hipEventSynchronize(rs.uploaded));          // the evicted pair's upload has read the host image
    }
    rs.sr_in = rs.sr_out = 0;                                   // (nothing valid in the slot until the uploads below are enqueued)
    if (c->rs_window.empty()) kaiser_best_window(c->rs_window);
    const double ratio = (double)sr_out / (double)sr_in, inc = 1.0 / ratio, gain = ratio < 1.0 ? ratio : 1.0;
    double* h_time = rs.h_image;
    double* h_table = rs.h_image + T;
    double reg = 0.0;
    for (int t = 0; t < T; ++t) {                               // accumulated, as resampy does: not t * inc
        h_time[t] = reg;
        reg += inc;
    }
    for (int j = 0; j < GT_RS_NWIN; ++j) h_table[2 * j] = ratio < 1.0 ? c->rs_window[j] * ratio : c->rs_window[j];
    for (int j = 0; j < GT_RS_NWIN; ++j) h_table[2 * j + 1] = j + 1 < GT_RS_NWIN ? h_table[2 * (j + 1)] - h_table[2 * j] : 0.0;
    HIPCHECK(c, hipMemcpyAsync(rs.d_time, h_time, (size_t)T * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(c, hipMemcpyAsync(rs.d_table, h_table, (size_t)GT_RS_NWIN * sizeof(double2), hipMemcpyHostToDevice, s));
    HIPCHECK(c, hipEventRecord(rs.uploaded, s));
    rs.scale = gain;
    rs.step = (int)(gain * 512.0);
    rs.sr_in = sr_in; rs.sr_out = sr_out; rs.last_use = clock;
    *slot_out = victim;
    return 0;
}

// wav at any rate -> wav at sr_out: one launch per GT_RS_MAX_ROWS rows on the caller's stream, straight from / to the caller's pointers.
// Everything is validated, and out_lengths filled, before the first table is built or anything is enqueued.
int gsttaco_resample(gsttaco_ctx* c, const float* x, const int32_t* in_lengths, const int32_t* sr_in, int B, int ld_in, int sr_out,
                     float* y, int ld_out, int32_t* out_lengths, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    int rc = ensure_audio(c);
    if (rc) return rc;
    const gsttaco_config& g = c->cfg;
    if (!x || !in_lengths || !sr_in || !y || !out_lengths) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || ld_in < 1 || ld_out < 1 || sr_out < 1) return fail(c, GSTTACO_E_INVALID, "bad B / ld_in / ld_out / sr_out");
    if (B > g.max_batch || ld_out > g.max_wav_samples) return fail(c, GSTTACO_E_CAPACITY, "batch / output samples exceed capacity");
    std::vector<int32_t> n_out(B), n_fix(B);
    std::vector<std::pair<int, int>> pairs;                     // the call's distinct rate pairs that need a table
    std::vector<int> pair_of(B, -1);
    for (int b = 0; b < B; ++b) {
        const int n = in_lengths[b], sr = sr_in[b];
        if (n < 0 || n > ld_in) return fail(c, GSTTACO_E_INVALID, "an input length is outside [0, ld_in]");
        if (sr < 1) return fail(c, GSTTACO_E_INVALID, "a sample rate is not positive");
        if ((int64_t)sr > (int64_t)GT_RS_MAX_FACTOR * sr_out || (int64_t)sr_out > (int64_t)GT_RS_MAX_FACTOR * sr)
            return fail(c, GSTTACO_E_INVALID, "a resampling factor is beyond 16 (sr_in <= 16 sr_out and sr_out <= 16 sr_in)");
        const double ratio = (double)sr_out / (double)sr;       // the expressions of audio.py resample_lengths
        const double fix = std::ceil((double)n * ratio);
        if (fix > (double)ld_out) return fail(c, GSTTACO_E_INVALID, "a row's resampled length ceil(in_length * sr_out / sr_in) exceeds ld_out");
        n_fix[b] = (int32_t)fix;
        n_out[b] = sr == sr_out ? n : (int32_t)((double)n * ratio);
        if (sr == sr_out) continue;
        const std::pair<int, int> key(sr, sr_out);
        size_t k = 0;
        while (k < pairs.size() && pairs[k] != key) ++k;
        if (k == pairs.size()) {
            if (pairs.size() == GT_RS_MAX_PAIRS)
                return fail(c, GSTTACO_E_INVALID, "more than eight distinct rate pairs in one call (the table cache holds eight)");
            pairs.push_back(key);
        }
        pair_of[b] = (int)k;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint64_t clock = ++c->rs_clock;
    int slot_of[GT_RS_MAX_PAIRS];
    ResampleArgs a{};
    for (size_t k = 0; k < pairs.size(); ++k) {
        if ((rc = ensure_resample_pair(c, pairs[k].first, pairs[k].second, clock, s, &slot_of[k]))) return rc;
        const gsttaco_ctx::ResampleSlot& rs = c->rs_slot[slot_of[k]];
        a.pair[slot_of[k]] = ResamplePair{rs.d_time, rs.d_table, rs.scale, rs.step, g.max_wav_samples};
    }
    a.x = x; a.y = y; a.ld_in = ld_in; a.ld_out = ld_out;
    for (int b0 = 0; b0 < B; b0 += GT_RS_MAX_ROWS) {
        a.row0 = b0; a.rows = std::min(B - b0, GT_RS_MAX_ROWS);
        for (int b = 0; b < a.rows; ++b) {
            a.n_in[b] = in_lengths[b0 + b];
            a.n_out[b] = n_out[b0 + b];
            a.slot[b] = pair_of[b0 + b] < 0 ? (uint8_t)GT_RS_PASS : (uint8_t)slot_of[pair_of[b0 + b]];
        }
        HIPCHECK(c, gt_launch_resample(a, s));
    }
    for (int b = 0; b < B; ++b) out_lengths[b] = n_fix[b];
    return 0;
}

int gsttaco_postnet(gsttaco_ctx* c, const float* pre_mel, int B, int Tf, float* mel, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!pre_mel || !mel) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || Tf < 1) return fail(c, GSTTACO_E_INVALID, "bad B / T");
    if (B > c->cfg.max_batch || Tf > c->steps_max * c->r) return fail(c, GSTTACO_E_CAPACITY, "batch / frames exceed capacity");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * Tf * c->cfg.mel_dim;
    HIPCHECK(c, hipMemcpyAsync(c->w_pre, pre_mel, n * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = run_cached(c, s, GraphKey{.kind = kSegPostnet, .B = B, .steps = Tf},
                         [&](hipStream_t st, const LaunchForms&) { return enqueue_postnet(c, st, B, Tf, c->w_pre, c->w_mel); }))) return rc;
    HIPCHECK(c, hipMemcpyAsync(mel, c->w_mel, n * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int gsttaco_vocoder(gsttaco_ctx* c, const float* mel, int B, int Tf, float* spectrogram, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->cfg.voc_use) return fail(c, GSTTACO_E_INVALID, "the context was created without Vocoder_Taco1");
    if (!mel || !spectrogram) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || Tf < 1) return fail(c, GSTTACO_E_INVALID, "bad B / T");
    if (B > c->cfg.max_batch || Tf > c->steps_max * c->r) return fail(c, GSTTACO_E_CAPACITY, "batch / frames exceed capacity");
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(c, hipMemcpyAsync(c->w_mel, mel, (size_t)B * Tf * c->cfg.mel_dim * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = run_cached(c, s, GraphKey{.kind = kSegVocoder, .B = B, .steps = Tf},
                         [&](hipStream_t st, const LaunchForms& f) { return enqueue_vocoder(c, st, f, B, Tf, c->w_mel, c->w_spec); }))) return rc;
    HIPCHECK(c, hipMemcpyAsync(spectrogram, c->w_spec, (size_t)B * Tf * c->cfg.spec_dim * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// wav -> mels and / or linear spectrograms of the same trimmed signal, from one STFT (either output may be NULL, not both).
int gsttaco_feature_frontend(gsttaco_ctx* c, const float* wav, const int32_t* wav_lengths, int B, int ld_wav, float top_db, float* mels,
                             float* spectrograms, int32_t* lengths, int cap_frames, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    int rc = ensure_audio(c);
    if (rc) return rc;
    const gsttaco_config& g = c->cfg;
    if (!wav || !wav_lengths || (!mels && !spectrograms) || !lengths) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || ld_wav < 17 || !(top_db > 0.f)) return fail(c, GSTTACO_E_INVALID, "bad B / ld_wav / top_db");
    if (B > g.max_batch || ld_wav > g.max_wav_samples) return fail(c, GSTTACO_E_CAPACITY, "batch / samples exceed capacity");
    if (cap_frames < 2 + ld_wav / g.frame_shift) return fail(c, GSTTACO_E_INVALID, "cap_frames must be >= 2 + ld_wav / Frame_Shift");
    AudioFrontArgs a{};
    a.wav = wav; a.wav_len = wav_lengths; a.mse = c->a_mse; a.bounds = c->a_bounds;
    a.mels = mels; a.specs = spectrograms; a.mel_len = lengths;
    a.window = c->a_window; a.twiddle = c->a_twiddle; a.mel_basis = c->a_mel_basis; a.band_lo = c->a_band_lo; a.band_hi = c->a_band_hi;
    a.B = B; a.ld_wav = ld_wav; a.ld_mse = c->a_ld_mse; a.cap_frames = cap_frames;
    a.n_fft = c->n_fft; a.log2_h = 0;
    while ((1 << a.log2_h) < c->n_fft / 2) ++a.log2_h;
    a.hop = g.frame_shift; a.n_mels = g.mel_dim;
    a.trim_frame = 32; a.trim_hop = 16;                 // Pattern_Generator.py:45
    a.preemph = 0.97f; a.trim_gain = 0.99f;             // Audio.py:11, Pattern_Generator.py:45
    a.top_db = top_db; a.max_abs = g.max_abs_mel;
    HIPCHECK(c, gt_launch_audio_front(a, (hipStream_t)stream));
    return 0;
}

int gsttaco_mel_frontend(gsttaco_ctx* c, const float* wav, const int32_t* wav_lengths, int B, int ld_wav, float top_db,
                         float* mels_for_gst, int32_t* mel_lengths, int cap_frames, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    int rc = ensure_audio(c);
    if (rc) return rc;
    if (!mels_for_gst) return fail(c, GSTTACO_E_INVALID, "null argument");
    return gsttaco_feature_frontend(c, wav, wav_lengths, B, ld_wav, top_db, mels_for_gst, nullptr, mel_lengths, cap_frames, stream);
}

// wav -> F0 and aperiodicity per frame of the front end's grid (YIN).  With top_db >= 0 the front end's two trim launches run first and
// the tracker reads the bounds they leave; everything is validated before anything is enqueued.
int gsttaco_pitch(gsttaco_ctx* c, const float* wav, const int32_t* wav_lengths, int B, int ld_wav, float top_db, float fmin, float fmax,
                  float threshold, int window, float* f0, float* aperiodicity, int32_t* frames, int cap_frames, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    int rc = ensure_audio(c);
    if (rc) return rc;
    const gsttaco_config& g = c->cfg;
    if (!wav || !wav_lengths || !f0 || !frames) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || ld_wav < 1 || cap_frames < 1 || top_db != top_db) return fail(c, GSTTACO_E_INVALID, "bad B / ld_wav / cap_frames / top_db");
    if (!(fmin > 0.f) || !(fmax > fmin)) return fail(c, GSTTACO_E_INVALID, "the F0 range needs 0 < fmin < fmax");
    if (!(threshold > 0.f) || !(threshold <= 1.f)) return fail(c, GSTTACO_E_INVALID, "threshold must be in (0, 1]");
    if (window < 0) return fail(c, GSTTACO_E_INVALID, "window must be >= 0 (0 = 25 ms)");
    const double sr = (double)g.sample_rate;
    const double lag_lo = std::floor(sr / (double)fmax), lag_hi = std::ceil(sr / (double)fmin);
    if (lag_lo < 2.0) return fail(c, GSTTACO_E_INVALID, "fmax is above Sample_Rate / 2 (tau_min = floor(Sample_Rate / fmax) must be >= 2)");
    if (lag_lo >= lag_hi) return fail(c, GSTTACO_E_INVALID, "the lag range is empty (tau_min >= tau_max)");
    const int64_t W = window ? (int64_t)window : (int64_t)std::llround(0.025 * sr);
    if (W < 1 || (double)W + lag_hi > (double)GT_PITCH_MAX_SPAN)
        return fail(c, GSTTACO_E_INVALID, "window + tau_max exceeds the 3072 samples one workgroup's LDS holds");
    if (B > g.max_batch || ld_wav > g.max_wav_samples) return fail(c, GSTTACO_E_CAPACITY, "batch / samples exceed capacity");
    hipStream_t s = (hipStream_t)stream;
    PitchArgs p{};
    if (top_db >= 0.f) {                                // the trim decision of gsttaco_feature_frontend: its kernels, its arguments
        AudioFrontArgs a{};
        a.wav = wav; a.wav_len = wav_lengths; a.mse = c->a_mse; a.bounds = c->a_bounds;
        a.mel_len = frames;                             // (unclipped here; the tracker writes the count again, clipped to cap_frames)
        a.B = B; a.ld_wav = ld_wav; a.ld_mse = c->a_ld_mse; a.cap_frames = INT_MAX;
        a.n_fft = c->n_fft; a.hop = g.frame_shift;
        a.trim_frame = 32; a.trim_hop = 16; a.preemph = 0.97f; a.top_db = top_db;
        HIPCHECK(c, gt_launch_trim_bounds(a, s));
        p.bounds = c->a_bounds;
    }
    p.wav = wav; p.wav_len = wav_lengths; p.f0 = f0; p.aperiodicity = aperiodicity; p.frames = frames;
    p.sr = sr; p.threshold = (double)threshold;
    p.B = B; p.ld_wav = ld_wav; p.cap_frames = cap_frames; p.n_fft = c->n_fft; p.hop = g.frame_shift;
    p.W = (int)W; p.tau_min = (int)lag_lo; p.tau_max = (int)lag_hi;
    HIPCHECK(c, gt_launch_pitch(p, s));
    return 0;
}

// The pitch errors of two F0 tracks along a path: one launch on the caller's stream.  Needs a created context only.
int gsttaco_pitch_errors(gsttaco_ctx* c, const float* f0_x, const int32_t* x_len, int Tx, const float* f0_y, const int32_t* y_len, int Ty,
                         const int32_t* path, const int32_t* path_len, int path_cap, int B, float gross, int32_t* counts, double* sums,
                         void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!f0_x || !f0_y || !counts || !sums) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (path && !path_len) return fail(c, GSTTACO_E_INVALID, "a path needs its path_len");
    if (B < 1 || Tx < 1 || Ty < 1 || (path && path_cap < 1)) return fail(c, GSTTACO_E_INVALID, "bad B / Tx / Ty / path_cap");
    if (!(gross >= 0.f)) return fail(c, GSTTACO_E_INVALID, "gross must be >= 0");
    if (B > c->cfg.max_batch) return fail(c, GSTTACO_E_CAPACITY, "batch exceeds the capacity given at create");
    int rc = ensure_device(c);
    if (rc) return rc;
    PitchErrorArgs a{};
    a.f0_x = f0_x; a.f0_y = f0_y; a.x_len = x_len; a.y_len = y_len; a.path = path; a.path_len = path_len;
    a.counts = counts; a.sums = sums; a.gross = (double)gross;
    a.B = B; a.Tx = Tx; a.Ty = Ty; a.path_cap = path_cap;
    HIPCHECK(c, gt_launch_pitch_errors(a, (hipStream_t)stream));
    return 0;
}

// Style embeddings -> the symmetric affinities of exact t-SNE: three launches on the caller's stream, everything in the caller's p.
// Needs a created context only.
int gsttaco_style_affinities(gsttaco_ctx* c, const float* x, int N, int D, int64_t ldx, float perplexity, double* p, double* beta,
                             int32_t* search_iters, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!x || !p || !beta) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (N < 3 || D < 1 || ldx < (int64_t)D) return fail(c, GSTTACO_E_INVALID, "bad N / D / ldx (N >= 3, D >= 1, ldx >= D)");
    if (!std::isfinite(perplexity) || !((double)perplexity > 1.0) || !((double)perplexity < (double)N - 1.0))
        return fail(c, GSTTACO_E_INVALID, "perplexity must lie in (1, N - 1): log(N - 1) is the entropy no beta exceeds");
    if (N > GT_TSNE_MAX_N) return fail(c, GSTTACO_E_CAPACITY, "N exceeds the 8192 points whose distances one workgroup's registers hold");
    int rc = ensure_device(c);
    if (rc) return rc;
    TsneAffinityArgs a{};
    a.x = x; a.p = p; a.beta = beta; a.search_iters = search_iters; a.ldx = ldx; a.perplexity = perplexity; a.N = N; a.D = D;
    HIPCHECK(c, gt_launch_style_affinities(a, (hipStream_t)stream));
    return 0;
}

// The descent of exact t-SNE from a given state: two launches per step on the caller's stream, four more for the KL divergence.
// Needs a created context only.
int gsttaco_style_map(gsttaco_ctx* c, const double* p, int N, double* y, double* velocity, double* gains, int first_iter, int iters,
                      float exaggeration, int stop_lying_iter, int mom_switch_iter, float momentum, float final_momentum, float eta,
                      double* kl, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!p || !y || !velocity || !gains) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (N < 3 || iters < 0 || first_iter < 0) return fail(c, GSTTACO_E_INVALID, "bad N / iters / first_iter (N >= 3, iters >= 0, first_iter >= 0)");
    if (!std::isfinite(eta) || !(eta > 0.f) || !std::isfinite(exaggeration) || !(exaggeration > 0.f))
        return fail(c, GSTTACO_E_INVALID, "eta and exaggeration must be finite and positive");
    if (!(momentum >= 0.f) || !(momentum < 1.f) || !(final_momentum >= 0.f) || !(final_momentum < 1.f))
        return fail(c, GSTTACO_E_INVALID, "momentum and final_momentum must lie in [0, 1)");
    if (N > GT_TSNE_MAX_N) return fail(c, GSTTACO_E_CAPACITY, "N exceeds the 8192 points of the style map");
    int rc = ensure_device(c);
    if (rc) return rc;
    if (iters == 0 && !kl) return 0;
    if (!c->w_tsne && (rc = dev_alloc(c, (void**)&c->w_tsne, ((size_t)5 * GT_TSNE_MAX_N + 1) * sizeof(double)))) return rc;
    TsneMapArgs a{};
    a.p = p; a.y = y; a.velocity = velocity; a.gains = gains; a.partials = c->w_tsne; a.kl = kl;
    a.exaggeration = (double)exaggeration; a.momentum = (double)momentum; a.final_momentum = (double)final_momentum; a.eta = (double)eta;
    a.N = N; a.first_iter = first_iter; a.iters = iters; a.stop_lying_iter = stop_lying_iter; a.mom_switch_iter = mom_switch_iter;
    HIPCHECK(c, gt_launch_style_map(a, (hipStream_t)stream));
    return 0;
}

// ---- the neural vocoder (melgan.hip).  Configure and the manifest need no device; finalize uploads and allocates once.
int gsttaco_melgan_configure(gsttaco_ctx* c, const gsttaco_melgan_config* m) {
    if (!c) return GSTTACO_E_INVALID;
    if (!m) return fail(c, GSTTACO_E_INVALID, "null argument");
    gsttaco_ctx::Melgan& g = c->mg;
    if (g.configured) return fail(c, GSTTACO_E_INVALID, "melgan: the context's vocoder is configured already");
    if (m->n_ratios < 1 || m->n_ratios > GSTTACO_MAX_LAYERS) return fail(c, GSTTACO_E_INVALID, "melgan: between 1 and 8 upsampling ratios");
    if (m->max_batch < 1 || m->max_frames < 1) return fail(c, GSTTACO_E_INVALID, "melgan: max_batch and max_frames must be at least 1");
    MgPlan plan;
    const char* why = gt_melgan_make_plan(m->mel_dim, m->base, m->n_ratios, m->ratios, m->n_res, m->slope, &plan);
    if (why) return fail(c, GSTTACO_E_INVALID, std::string("melgan: ") + why);
    if ((double)m->max_batch * m->max_frames * plan.hop > 2147483647.0)
        return fail(c, GSTTACO_E_INVALID, "melgan: max_batch * max_frames * hop exceeds 2^31 - 1 samples");
    g.cfg = *m;
    g.plan = plan;
    auto add = [&](const std::string& name, std::vector<int64_t> shape) { g.man.add(name, std::move(shape)); };
    int up = -1, res = 0;
    for (int i = 0; i < plan.n_stages; ++i) {
        const MgStage& s = plan.st[i];
        if (s.kind == GT_MG_IN) { add("melgan/in/kernel", {(int64_t)7 * s.cin, s.cout}); add("melgan/in/bias", {s.cout}); }
        else if (s.kind == GT_MG_UP) {
            ++up; res = 0;
            const std::string p = "melgan/up" + std::to_string(up);
            add(p + "/kernel", {(int64_t)2 * s.r, s.cin, s.cout});
            add(p + "/bias", {s.cout});
        } else if (s.kind == GT_MG_RES) {
            const std::string p = "melgan/up" + std::to_string(up) + "/res" + std::to_string(res++);
            add(p + "/conv3/kernel", {(int64_t)3 * s.cin, s.cout}); add(p + "/conv3/bias", {s.cout});
            add(p + "/conv1/kernel", {s.cin, s.cout}); add(p + "/conv1/bias", {s.cout});
            add(p + "/shortcut/kernel", {s.cin, s.cout}); add(p + "/shortcut/bias", {s.cout});
        } else { add("melgan/out/kernel", {(int64_t)7 * s.cin, 1}); add("melgan/out/bias", {1}); }
    }
    g.configured = true;
    return 0;
}

int gsttaco_melgan_num_weights(const gsttaco_ctx* c) { return c ? (int)c->mg.man.tensors.size() : GSTTACO_E_INVALID; }

int gsttaco_melgan_weight_info(const gsttaco_ctx* c, int i, const char** name, int64_t shape[4], int* ndim) {
    return c ? c->mg.man.info(i, name, shape, ndim) : GSTTACO_E_INVALID;
}

int gsttaco_melgan_load_weight(gsttaco_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    return voc_load_weight(c, &gsttaco_ctx::mg, "melgan", name, host, shape, ndim);
}

int gsttaco_melgan_finalize(gsttaco_ctx* c) {
    if (!c) return GSTTACO_E_INVALID;
    gsttaco_ctx::Melgan& g = c->mg;
    int rc = voc_begin_finalize(c, g, "melgan");
    if (rc || (rc = ensure_device(c))) return rc;
    HIPCHECK(c, gt_melgan_prepare());
    auto packed = [&](const float** dst, const std::string& name, int taps, int cin, int cout) {
        return upload_packed(c, dst, g.man.host(name), taps, cin, cout);
    };
    auto bias = [&](const float** dst, const std::string& name, const std::string& plus, int n_p) {
        return upload_padded_bias(c, g.man, dst, name, plus, n_p);
    };
    int up = -1, res = 0;
    for (int i = 0; i < g.plan.n_stages; ++i) {
        MgStage& s = g.plan.st[i];
        if (s.kind == GT_MG_IN) {
            if ((rc = packed(&s.w0, "melgan/in/kernel", 7, s.cin, s.cout)) || (rc = bias(&s.b0, "melgan/in/bias", "", s.n_p))) return rc;
        } else if (s.kind == GT_MG_UP) {
            ++up; res = 0;
            const std::string p = "melgan/up" + std::to_string(up);
            if ((rc = packed(&s.w0, p + "/kernel", 2 * s.r, s.cin, s.cout)) || (rc = bias(&s.b0, p + "/bias", "", s.n_p))) return rc;
        } else if (s.kind == GT_MG_RES) {
            const std::string p = "melgan/up" + std::to_string(up) + "/res" + std::to_string(res++);
            if ((rc = packed(&s.w0, p + "/conv3/kernel", 3, s.cin, s.cout)) || (rc = bias(&s.b0, p + "/conv3/bias", "", s.n_p))) return rc;
            if ((rc = packed(&s.w1, p + "/shortcut/kernel", 1, s.cin, s.cout)) || (rc = packed(&s.w2, p + "/conv1/kernel", 1, s.cin, s.cout))) return rc;
            if ((rc = bias(&s.b1, p + "/shortcut/bias", p + "/conv1/bias", s.n_p))) return rc;
        } else {
            if ((rc = upload_vec(c, &s.w0, g.man.host("melgan/out/kernel"))) || (rc = bias(&s.b0, "melgan/out/bias", "", 1))) return rc;
        }
    }
    const size_t ws = (size_t)g.cfg.max_batch * g.cfg.max_frames * g.plan.ws_floats_per_frame * sizeof(float);
    for (int k = 0; k < 2; ++k)
        if ((rc = dev_alloc(c, (void**)&g.ws[k], ws))) return rc;
    g.finalized = true;
    return 0;
}

namespace { int melgan_call(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths, int ld_wav,
                            int only, void* stream); }

int gsttaco_melgan(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths, int ld_wav,
                   void* stream) {
    return melgan_call(c, mel, frames, B, T, wav, wav_lengths, ld_wav, -1, stream);
}

int gsttaco_melgan_debug_stage(gsttaco_ctx* c, int stage, const float* mel, const int32_t* frames, int B, int T, float* wav, int ld_wav,
                               void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (stage < 0 || stage >= c->mg.plan.n_stages) return fail(c, GSTTACO_E_INVALID, "melgan: no such launch");
    return melgan_call(c, mel, frames, B, T, wav, nullptr, ld_wav, stage, stream);
}

namespace {
int melgan_call(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths, int ld_wav,
                int only, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Melgan& g = c->mg;
    MgCall a{};
    if (int rc = voc_chain_call(c, g, "melgan", &a, mel, frames, B, T, wav, wav_lengths, ld_wav, only)) return rc;
    HIPCHECK(c, gt_launch_melgan(g.plan, a, (hipStream_t)stream));
    return 0;
}
}  // namespace

int gsttaco_melgan_plan(const gsttaco_ctx* c, int32_t fields[]) {
    if (!c || !fields) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Melgan& g = c->mg;
    if (!g.configured) return fail(c, GSTTACO_E_WEIGHTS, "melgan: not configured (gsttaco_melgan_configure)");
    fields[0] = g.plan.n_stages; fields[1] = g.plan.min_frames; fields[2] = g.plan.hop;
    for (int i = 0; i < g.plan.n_stages; ++i) {
        const MgStage& s = g.plan.st[i];
        int32_t* f = fields + 3 + GSTTACO_MELGAN_PLAN_STRIDE * i;
        f[0] = s.kind; f[1] = s.cout; f[2] = s.tile; f[3] = s.form; f[4] = s.kind == GT_MG_UP ? s.rate_in : s.rate_out; f[5] = (int32_t)s.lds;
    }
    return 0;
}

// ---- the flow vocoder (waveglow.hip).  Configure and the manifest need no device; finalize inverts, repacks, uploads and allocates once.
int gsttaco_waveglow_configure(gsttaco_ctx* c, const gsttaco_waveglow_config* m) {
    if (!c) return GSTTACO_E_INVALID;
    if (!m) return fail(c, GSTTACO_E_INVALID, "null argument");
    gsttaco_ctx::Waveglow& g = c->wg;
    if (g.configured) return fail(c, GSTTACO_E_INVALID, "waveglow: the context's flow vocoder is configured already");
    if (m->kernel != 3) return fail(c, GSTTACO_E_INVALID, "waveglow: kernel must be 3 (the WN layers' taps are fixed)");
    if (m->max_batch < 1) return fail(c, GSTTACO_E_INVALID, "waveglow: max_batch must be at least 1");
    if (m->max_frames < 1) return fail(c, GSTTACO_E_INVALID, "waveglow: max_frames must be at least 1");
    WgPlan plan;
    const char* why = gt_waveglow_make_plan(m->mel_dim, m->hop, m->win, m->n_group, m->n_flows, m->n_early_every, m->n_early_size,
                                            m->n_layers, m->n_channels, &plan);
    if (why) return fail(c, GSTTACO_E_INVALID, std::string("waveglow: ") + why);
    if ((double)m->max_batch * m->max_frames * plan.hop > 2147483647.0)
        return fail(c, GSTTACO_E_INVALID, "waveglow: max_batch * max_frames * hop exceeds 2^31 - 1 samples");
    g.cfg = *m;
    g.plan = plan;
    auto add = [&](const std::string& name, std::vector<int64_t> shape) { g.man.add(name, std::move(shape)); };
    const int64_t C = plan.C;
    add("waveglow/up/kernel", {plan.win, plan.mel_dim, plan.mel_dim});
    add("waveglow/up/bias", {plan.mel_dim});
    for (int k = 0; k < plan.F; ++k) {
        const std::string p = "waveglow/flow" + std::to_string(k);
        const int64_t ck = plan.ck[k];
        add(p + "/W", {ck, ck});
        add(p + "/start/kernel", {ck / 2, C}); add(p + "/start/bias", {C});
        add(p + "/end/kernel", {C, ck}); add(p + "/end/bias", {ck});
        for (int i = 0; i < plan.NL; ++i) {
            const std::string q = p + "/layer" + std::to_string(i);
            const int64_t nrs = i == plan.NL - 1 ? C : 2 * C;
            add(q + "/in/kernel", {3 * C, 2 * C}); add(q + "/in/bias", {2 * C});
            add(q + "/cond/kernel", {plan.S, 2 * C}); add(q + "/cond/bias", {2 * C});
            add(q + "/res_skip/kernel", {C, nrs}); add(q + "/res_skip/bias", {nrs});
        }
    }
    g.configured = true;
    return 0;
}

int gsttaco_waveglow_num_weights(const gsttaco_ctx* c) { return c ? (int)c->wg.man.tensors.size() : GSTTACO_E_INVALID; }

int gsttaco_waveglow_weight_info(const gsttaco_ctx* c, int i, const char** name, int64_t shape[4], int* ndim) {
    return c ? c->wg.man.info(i, name, shape, ndim) : GSTTACO_E_INVALID;
}

int gsttaco_waveglow_load_weight(gsttaco_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    return voc_load_weight(c, &gsttaco_ctx::wg, "waveglow", name, host, shape, ndim);
}

namespace {
// inverse of the n x n matrix w (row-major) in float64 by Gauss-Jordan elimination with partial pivoting; false: singular
bool invert_f64(const float* w, int n, std::vector<double>& inv) {
    std::vector<double> a((size_t)n * n);
    for (int i = 0; i < n * n; ++i) a[i] = w[i];
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    for (int col = 0; col < n; ++col) {
        int piv = col;
        for (int r = col + 1; r < n; ++r)
            if (std::fabs(a[(size_t)r * n + col]) > std::fabs(a[(size_t)piv * n + col])) piv = r;
        const double p = a[(size_t)piv * n + col];
        if (!(std::fabs(p) > 0.0) || !std::isfinite(p)) return false;
        if (piv != col)
            for (int j = 0; j < n; ++j) { std::swap(a[(size_t)piv * n + j], a[(size_t)col * n + j]); std::swap(inv[(size_t)piv * n + j], inv[(size_t)col * n + j]); }
        for (int j = 0; j < n; ++j) { a[(size_t)col * n + j] /= p; inv[(size_t)col * n + j] /= p; }
        for (int r = 0; r < n; ++r) {
            const double f = a[(size_t)r * n + col];
            if (r == col || f == 0.0) continue;
            for (int j = 0; j < n; ++j) { a[(size_t)r * n + j] -= f * a[(size_t)col * n + j]; inv[(size_t)r * n + j] -= f * inv[(size_t)col * n + j]; }
        }
    }
    return true;
}
}  // namespace

int gsttaco_waveglow_finalize(gsttaco_ctx* c) {
    if (!c) return GSTTACO_E_INVALID;
    gsttaco_ctx::Waveglow& g = c->wg;
    int rc = voc_begin_finalize(c, g, "waveglow");
    if (rc || (rc = ensure_device(c))) return rc;
    HIPCHECK(c, gt_waveglow_prepare());
    WgPlan& P = g.plan;
    auto host = [&](const std::string& name) -> const std::vector<float>& { return g.man.host(name); };
    std::vector<float> buf, bbuf;
    auto up = [&](const float** dst, const std::vector<float>& v) { return upload_vec(c, dst, v); };
    const int C = P.C, C_p = P.C_p, n2 = 2 * C_p;
    if ((rc = upload_packed(c, &P.w_up, host("waveglow/up/kernel"), P.win, P.mel_dim, P.mel_dim))) return rc;
    if ((rc = upload_padded_bias(c, g.man, &P.b_up, "waveglow/up/bias", "", P.mel_p))) return rc;
    std::vector<double> inv;
    for (int k = 0; k < P.F; ++k) {
        const std::string p = "waveglow/flow" + std::to_string(k);
        const int ck = P.ck[k], h = ck / 2;
        WgFlowOps& f = P.flow[k];
        if (!invert_f64(host(p + "/W").data(), ck, inv)) return fail(c, GSTTACO_E_WEIGHTS, "waveglow: weight '" + p + "/W' is singular");
        buf.assign(16 * 16, 0.f);
        for (int i = 0; i < ck; ++i)
            for (int j = 0; j < ck; ++j) buf[i * 16 + j] = (float)inv[(size_t)i * ck + j];
        if ((rc = up(&f.winv, buf))) return rc;
        buf.assign((size_t)h * C_p, 0.f);
        for (int q = 0; q < h; ++q)
            for (int n = 0; n < C; ++n) buf[(size_t)q * C_p + n] = host(p + "/start/kernel")[(size_t)q * C + n];
        if ((rc = up(&f.w_start, buf))) return rc;
        if ((rc = upload_padded_bias(c, g.man, &f.b_start, p + "/start/bias", "", C_p))) return rc;
        buf.assign((size_t)C * 16, 0.f);
        for (int n = 0; n < C; ++n)
            for (int j = 0; j < ck; ++j) buf[(size_t)n * 16 + j] = host(p + "/end/kernel")[(size_t)n * ck + j];
        if ((rc = up(&f.w_end, buf))) return rc;
        if ((rc = upload_padded_bias(c, g.man, &f.b_end, p + "/end/bias", "", 16))) return rc;
        for (int i = 0; i < P.NL; ++i) {
            const std::string q = p + "/layer" + std::to_string(i);
            WgLayerOps& o = P.layer[k][i];
            const bool last = i == P.NL - 1;
            buf.resize((size_t)3 * C_p * n2);
            gt_waveglow_pack_gate(host(q + "/in/kernel").data(), 3, C, C, buf.data());
            if ((rc = up(&o.w_in, buf))) return rc;
            buf.resize((size_t)P.S_p * n2);
            gt_waveglow_pack_gate(host(q + "/cond/kernel").data(), 1, P.S, C, buf.data());
            if ((rc = up(&o.w_cond, buf))) return rc;
            buf.resize(n2);
            gt_waveglow_gate_bias(host(q + "/in/bias").data(), host(q + "/cond/bias").data(), C, buf.data());
            if ((rc = up(&o.b_ac, buf))) return rc;
            const int nB = last ? C_p : n2;
            buf.resize((size_t)C_p * nB);
            bbuf.resize(nB);
            gt_waveglow_pack_rs(host(q + "/res_skip/kernel").data(), host(q + "/res_skip/bias").data(), C, last, buf.data(), bbuf.data());
            if ((rc = up(&o.w_rs, buf)) || (rc = up(&o.b_rs, bbuf))) return rc;
        }
    }
    // the workspace for the capacity: max_batch * max_frames * hop / n_group columns of spect S_p, two hid C_p, out C_p and audio 16
    const size_t cols = (size_t)g.cfg.max_batch * g.cfg.max_frames * (P.hop / P.G);
    if ((rc = dev_alloc(c, (void**)&g.spect, cols * P.S_p * sizeof(float))) || (rc = dev_alloc(c, (void**)&g.hid[0], cols * C_p * sizeof(float))) ||
        (rc = dev_alloc(c, (void**)&g.hid[1], cols * C_p * sizeof(float))) || (rc = dev_alloc(c, (void**)&g.out, cols * C_p * sizeof(float))) ||
        (rc = dev_alloc(c, (void**)&g.audio, cols * 16 * sizeof(float)))) return rc;
    g.finalized = true;
    return 0;
}

int gsttaco_waveglow_noise(gsttaco_ctx* c, const uint64_t* seeds, int B, int T, float* z, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Waveglow& g = c->wg;
    if (!g.configured) return fail(c, GSTTACO_E_WEIGHTS, "waveglow: not configured (gsttaco_waveglow_configure)");
    if (!seeds || !z) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || T < 1) return fail(c, GSTTACO_E_INVALID, "bad B / T");
    if ((double)B * T * g.plan.hop > 2147483647.0) return fail(c, GSTTACO_E_CAPACITY, "waveglow: B * T * hop exceeds 2^31 - 1 samples");
    int rc = ensure_device(c);
    if (rc) return rc;
    HIPCHECK(c, gt_launch_waveglow_noise(seeds, z, B, T * g.plan.hop, g.plan.G, (hipStream_t)stream));
    return 0;
}

namespace {
int waveglow_call(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float sigma, const uint64_t* seeds, const float* z,
                  float* wav, int32_t* wav_lengths, int ld_wav, int only, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Waveglow& g = c->wg;
    if (int rc = voc_check_call(c, g, "waveglow", mel, wav, B, T, ld_wav,
                                (seeds != nullptr) == (z != nullptr) ? "waveglow: exactly one of seeds and z must be given" : nullptr,
                                !(sigma >= 0.f) || !std::isfinite(sigma) ? "sigma must be finite and at least 0" : nullptr)) return rc;
    WgCall a{};
    a.mel = mel; a.frames = frames; a.seeds = seeds; a.z = z; a.wav = wav; a.wav_lengths = wav_lengths;
    a.spect = g.spect; a.hid[0] = g.hid[0]; a.hid[1] = g.hid[1]; a.out = g.out; a.audio = g.audio;
    a.B = B; a.T = T; a.ld_wav = ld_wav; a.sigma = sigma; a.only = only;
    HIPCHECK(c, gt_launch_waveglow(g.plan, a, (hipStream_t)stream));
    return 0;
}
}  // namespace

int gsttaco_waveglow(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float sigma, const uint64_t* seeds, const float* z,
                     float* wav, int32_t* wav_lengths, int ld_wav, void* stream) {
    return waveglow_call(c, mel, frames, B, T, sigma, seeds, z, wav, wav_lengths, ld_wav, -1, stream);
}

int gsttaco_waveglow_debug_stage(gsttaco_ctx* c, int stage, const float* mel, const int32_t* frames, int B, int T, float sigma,
                                 const uint64_t* seeds, const float* z, float* wav, int ld_wav, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (!c->wg.configured || stage < 0 || stage >= 2 + c->wg.plan.F * (c->wg.plan.NL + 1)) return fail(c, GSTTACO_E_INVALID, "waveglow: no such launch");
    return waveglow_call(c, mel, frames, B, T, sigma, seeds, z, wav, nullptr, ld_wav, stage, stream);
}

int gsttaco_waveglow_plan(const gsttaco_ctx* c, int32_t fields[]) {
    if (!c || !fields) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Waveglow& g = c->wg;
    if (!g.configured) return fail(c, GSTTACO_E_WEIGHTS, "waveglow: not configured (gsttaco_waveglow_configure)");
    const WgPlan& P = g.plan;
    int n = 0;
    auto put = [&](int kind, int channels, int tile, int form, int unit, size_t lds) {
        int32_t* f = fields + 3 + GSTTACO_WAVEGLOW_PLAN_STRIDE * n++;
        f[0] = kind; f[1] = channels; f[2] = tile; f[3] = form; f[4] = unit; f[5] = (int32_t)lds;
    };
    put(GT_WG_UP, P.mel_dim, P.up_tile, P.up_form, P.hop, P.up_lds);
    put(GT_WG_FLOW, P.n_rem, GT_WG_FLOW_TILE, 0, P.G, P.flow_lds);
    for (int k = P.F - 1; k >= 0; --k) {
        for (int i = 0; i < P.NL; ++i) put(GT_WG_LAYER, P.C, P.tile, P.form, P.G, P.lds);
        put(GT_WG_FLOW, P.ck[k], GT_WG_FLOW_TILE, 0, P.G, P.flow_lds);
    }
    fields[0] = n; fields[1] = P.hop; fields[2] = P.G;
    return 0;
}

// ---- the HiFi-GAN vocoder (hifigan.hip).  Configure and the manifest need no device; finalize uploads and allocates once.
int gsttaco_hifigan_configure(gsttaco_ctx* c, const gsttaco_hifigan_config* m) {
    if (!c) return GSTTACO_E_INVALID;
    if (!m) return fail(c, GSTTACO_E_INVALID, "null argument");
    gsttaco_ctx::Hifigan& g = c->hg;
    if (g.configured) return fail(c, GSTTACO_E_INVALID, "hifigan: the context's HiFi-GAN is configured already");
    if (m->n_rates < 1 || m->n_rates > GSTTACO_MAX_LAYERS) return fail(c, GSTTACO_E_INVALID, "hifigan: n_rates: between 1 and 8 upsampling rates");
    if (m->n_kernels < 1 || m->n_kernels > GSTTACO_MAX_LAYERS) return fail(c, GSTTACO_E_INVALID, "hifigan: n_kernels: between 1 and 8 residual kernels");
    if (m->max_batch < 1 || m->max_frames < 1) return fail(c, GSTTACO_E_INVALID, "hifigan: max_batch and max_frames must be at least 1");
    HgConfig hc{};
    hc.mel_dim = m->mel_dim; hc.initial = m->initial; hc.n_rates = m->n_rates; hc.resblock = m->resblock; hc.n_kernels = m->n_kernels;
    hc.slope = m->slope; hc.out_slope = m->out_slope;
    for (int i = 0; i < m->n_rates; ++i) hc.rates[i] = m->rates[i];
    for (int j = 0; j < m->n_kernels; ++j) {
        hc.kernels[j] = m->kernels[j];
        hc.n_dilations[j] = m->n_dilations[j];
        for (int k = 0; k < GSTTACO_HIFIGAN_MAX_DILATIONS; ++k) hc.dilations[j][k] = m->dilations[j][k];
    }
    const char* why = gt_hifigan_make_plan(hc, &g.plan);
    if (why) {
        g.plan = HgPlan{};
        return fail(c, GSTTACO_E_INVALID, std::string("hifigan: ") + why);
    }
    if ((double)m->max_batch * m->max_frames * g.plan.hop > 2147483647.0) {
        g.plan = HgPlan{};
        return fail(c, GSTTACO_E_INVALID, "hifigan: max_batch * max_frames * hop exceeds 2^31 - 1 samples");
    }
    g.cfg = *m;
    auto add = [&](const std::string& name, std::vector<int64_t> shape) { g.man.add(name, std::move(shape)); };
    for (int i = 0; i < g.plan.n_stages; ++i) {
        const HgStage& s = g.plan.st[i];
        const std::string p = hifigan_name(s);
        if (s.kind == GT_HG_UP) add(p + "/kernel", {(int64_t)s.taps, s.cin, s.cout});
        else add(p + "/kernel", {(int64_t)s.taps * s.cin, s.cout});
        add(p + "/bias", {s.cout});
    }
    g.operands = GSTTACO_HIFIGAN_F32;           // a configure starts at the fp32 form, whatever was selected before it
    g.configured = true;
    return 0;
}

int gsttaco_hifigan_set_operands(gsttaco_ctx* c, int operands) {
    if (!c) return GSTTACO_E_INVALID;
    gsttaco_ctx::Hifigan& g = c->hg;
    if (operands != GSTTACO_HIFIGAN_F32 && operands != GSTTACO_HIFIGAN_BF16 && operands != GSTTACO_HIFIGAN_F16)
        return fail(c, GSTTACO_E_INVALID, "hifigan: operands must be GSTTACO_HIFIGAN_F32, _BF16 or _F16");
    if (!g.configured) return fail(c, GSTTACO_E_WEIGHTS, "hifigan: not configured (gsttaco_hifigan_configure)");
    if (g.finalized) return fail(c, GSTTACO_E_WEIGHTS, "hifigan: weights already finalized (the operand form is chosen before gsttaco_hifigan_finalize)");
    g.operands = operands;
    gt_hifigan_set_operands(&g.plan, operands);
    return 0;
}

int gsttaco_hifigan_num_weights(const gsttaco_ctx* c) { return c ? (int)c->hg.man.tensors.size() : GSTTACO_E_INVALID; }

int gsttaco_hifigan_weight_info(const gsttaco_ctx* c, int i, const char** name, int64_t shape[4], int* ndim) {
    return c ? c->hg.man.info(i, name, shape, ndim) : GSTTACO_E_INVALID;
}

int gsttaco_hifigan_load_weight(gsttaco_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    return voc_load_weight(c, &gsttaco_ctx::hg, "hifigan", name, host, shape, ndim);
}

int gsttaco_hifigan_finalize(gsttaco_ctx* c) {
    if (!c) return GSTTACO_E_INVALID;
    gsttaco_ctx::Hifigan& g = c->hg;
    int rc = voc_begin_finalize(c, g, "hifigan");
    if (rc) return rc;
    auto host = [&](const std::string& name) -> const std::vector<float>& { return g.man.host(name); };
    // The 16-bit packs first, on the host alone: a weight that fp16 cannot hold refuses the finalize before anything is uploaded, and
    // the context stays as it was (another form can be selected, or the tensor loaded again).
    static_assert(GSTTACO_HIFIGAN_F32 == GT_HG_OP_F32 && GSTTACO_HIFIGAN_BF16 == GT_HG_OP_BF16 && GSTTACO_HIFIGAN_F16 == GT_HG_OP_F16, "operand forms");
    std::vector<std::vector<float>> packs16(g.plan.n_stages);       // 16-bit words, two to a float
    if (g.operands != GSTTACO_HIFIGAN_F32)
        for (int i = 0; i < g.plan.n_stages; ++i) {
            const HgStage& s = g.plan.st[i];
            if (s.kind == GT_HG_OUT) continue;
            const std::string p = hifigan_name(s);
            packs16[i].resize(gt_hifigan_pack16_words(s.taps, s.cin, s.cout) / 2);
            const int64_t bad = gt_hifigan_pack16(host(p + "/kernel").data(), s.taps, s.cin, s.cout, g.operands, reinterpret_cast<uint16_t*>(packs16[i].data()));
            if (bad >= 0)
                return fail(c, GSTTACO_E_WEIGHTS, "hifigan: weight '" + p + "/kernel' is not finite in float16 (element " + std::to_string(bad) +
                                                  "): use the bfloat16 or float32 operands");
        }
    if ((rc = ensure_device(c))) return rc;
    HIPCHECK(c, gt_hifigan_prepare());
    for (int i = 0; i < g.plan.n_stages; ++i) {
        HgStage& s = g.plan.st[i];
        const std::string p = hifigan_name(s);
        if (s.kind == GT_HG_OUT) rc = upload_vec(c, &s.w0, host(p + "/kernel"));
        else if (g.operands != GSTTACO_HIFIGAN_F32) rc = upload_vec(c, &s.w0, packs16[i]);
        else rc = upload_packed(c, &s.w0, host(p + "/kernel"), s.taps, s.cin, s.cout);
        if (rc || (rc = upload_padded_bias(c, g.man, &s.b0, p + "/bias", "", s.kind == GT_HG_OUT ? 1 : s.n_p))) return rc;
    }
    const size_t ws = (size_t)g.cfg.max_batch * g.cfg.max_frames * g.plan.ws_floats_per_frame * sizeof(float);
    for (int k = 0; k < GT_HG_BUFS; ++k)
        if ((rc = dev_alloc(c, (void**)&g.ws[k], ws))) return rc;
    g.finalized = true;
    return 0;
}

namespace { int hifigan_call(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths, int ld_wav,
                             int only, void* stream); }

int gsttaco_hifigan(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths, int ld_wav,
                    void* stream) {
    return hifigan_call(c, mel, frames, B, T, wav, wav_lengths, ld_wav, -1, stream);
}

int gsttaco_hifigan_debug_stage(gsttaco_ctx* c, int stage, const float* mel, const int32_t* frames, int B, int T, float* wav, int ld_wav,
                                void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    if (stage < 0 || stage >= c->hg.plan.n_stages) return fail(c, GSTTACO_E_INVALID, "hifigan: no such launch");
    return hifigan_call(c, mel, frames, B, T, wav, nullptr, ld_wav, stage, stream);
}

int gsttaco_hifigan_debug_buffer(gsttaco_ctx* c, int buffer, float* device, int64_t floats, int write, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Hifigan& g = c->hg;
    if (!g.finalized) return fail(c, GSTTACO_E_WEIGHTS, "hifigan: weights not finalized (gsttaco_hifigan_finalize)");
    if (buffer < 0 || buffer >= GT_HG_BUFS) return fail(c, GSTTACO_E_INVALID, "hifigan: no such workspace buffer (0 sum, 1 up, 2 A, 3 B)");
    const int64_t size = (int64_t)g.cfg.max_batch * g.cfg.max_frames * (int64_t)g.plan.ws_floats_per_frame;
    if (!device || floats < 0 || floats > size) return fail(c, GSTTACO_E_INVALID, "hifigan: a NULL array, or more floats than the workspace buffer holds");
    if (floats == 0) return 0;
    HIPCHECK(c, hipMemcpyAsync(write ? (void*)g.ws[buffer] : (void*)device, write ? (const void*)device : (const void*)g.ws[buffer],
                               (size_t)floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

namespace {
int hifigan_call(gsttaco_ctx* c, const float* mel, const int32_t* frames, int B, int T, float* wav, int32_t* wav_lengths, int ld_wav,
                 int only, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Hifigan& g = c->hg;
    HgCall a{};
    if (int rc = voc_chain_call(c, g, "hifigan", &a, mel, frames, B, T, wav, wav_lengths, ld_wav, only)) return rc;
    HIPCHECK(c, gt_launch_hifigan(g.plan, a, (hipStream_t)stream));
    return 0;
}
}  // namespace

int gsttaco_hifigan_plan(const gsttaco_ctx* c, int32_t fields[]) {
    if (!c || !fields) return GSTTACO_E_INVALID;
    const gsttaco_ctx::Hifigan& g = c->hg;
    if (!g.configured) return fail(c, GSTTACO_E_WEIGHTS, "hifigan: not configured (gsttaco_hifigan_configure)");
    fields[0] = g.plan.n_stages; fields[1] = g.plan.min_frames; fields[2] = g.plan.hop;
    for (int i = 0; i < g.plan.n_stages; ++i) {
        const HgStage& s = g.plan.st[i];
        int32_t* f = fields + 3 + GSTTACO_HIFIGAN_PLAN_STRIDE * i;
        f[0] = s.kind; f[1] = s.cout; f[2] = s.taps; f[3] = s.dil; f[4] = s.tile; f[5] = s.form;
        f[6] = s.kind == GT_HG_UP ? s.rate_in : s.rate_out; f[7] = (int32_t)s.lds;
    }
    return 0;
}

int gsttaco_griffin_lim(gsttaco_ctx* c, const float* spectrogram, const int32_t* frames, int B, int T, int iters,
                        float power, float ref_level_db, const float* init_phase, uint64_t seed,
                        float* wav, int32_t* wav_lengths, int ld_wav, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    int rc = ensure_audio(c);
    if (rc) return rc;
    const gsttaco_config& g = c->cfg;
    if (!spectrogram || !wav) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (B < 1 || T < 1 || iters < 0 || !(power > 0.f)) return fail(c, GSTTACO_E_INVALID, "bad B / T / iters / power");
    if (B > g.max_batch) return fail(c, GSTTACO_E_CAPACITY, "batch exceeds capacity");
    if ((int64_t)g.frame_shift * (T - 1) > (int64_t)ld_wav || ld_wav < 1)
        return fail(c, GSTTACO_E_INVALID, "ld_wav must be >= Frame_Shift * (T - 1)");
    const size_t need = (size_t)B * T;
    if (need > c->gl_frames_cap) {                       // grown on demand, kept for the context's lifetime
        const size_t nb = (size_t)c->n_fft / 2 + 1;
        float* m = nullptr; float* f0 = nullptr; float* f1 = nullptr;
        if ((rc = dev_alloc(c, (void**)&m, need * nb * sizeof(float)))) return rc;
        if ((rc = dev_alloc(c, (void**)&f0, need * c->n_fft * sizeof(float)))) return rc;
        if ((rc = dev_alloc(c, (void**)&f1, need * c->n_fft * sizeof(float)))) return rc;
        c->gl_mag = m; c->gl_frm[0] = f0; c->gl_frm[1] = f1; c->gl_frames_cap = need;
    }
    GriffinLimArgs a{};
    a.spec = spectrogram; a.frames = frames; a.init_phase = init_phase; a.mag = c->gl_mag;
    a.wav = wav; a.wav_len = wav_lengths;
    a.window = c->a_window; a.win_sq = c->a_win_sq; a.twiddle = c->a_twiddle;
    a.seed = seed;
    a.B = B; a.T = T; a.n_fft = c->n_fft; a.log2_h = 0;
    while ((1 << a.log2_h) < c->n_fft / 2) ++a.log2_h;
    a.hop = g.frame_shift; a.ld_wav = ld_wav; a.iters = iters;
    a.power = power; a.ref_level_db = ref_level_db; a.max_abs = g.max_abs_mel; a.preemph = 0.97f;
    HIPCHECK(c, gt_launch_griffin_lim(a, c->gl_frm[0], c->gl_frm[1], (hipStream_t)stream));
    return 0;
}

int gsttaco_mel_basis(gsttaco_ctx* c, float* host_out) {
    if (!c || !host_out) return GSTTACO_E_INVALID;
    if (c->cfg.spec_dim < 2 || c->cfg.sample_rate < 1) return fail(c, GSTTACO_E_INVALID, "Sound.Spectrogram_Dim / Sample_Rate not set");
    host_audio_tables(c);
    memcpy(host_out, c->h_mel_basis.data(), c->h_mel_basis.size() * sizeof(float));
    return 0;
}

}  // extern "C"

namespace {

// gsttaco_inference_step (`style` NULL) and gsttaco_inference_step_styled (`style` [B, gst_att] given: it IS w_gst, the reference encoder
// and the tail are not run; mels_for_gst / mel_lengths NULL, Tref1 0).  The callers have checked their own arguments.
int inference_step(gsttaco_ctx* c, const int32_t* tokens, const int32_t* token_lengths, const float* mels_for_gst, const int32_t* mel_lengths,
                   const float* style, const float* mask, const float* noise, uint64_t seed, int B, int Tv, int Tref1, int steps,
                   float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream,
                   const float* teacher = nullptr, int Tq = 0, bool forced = false) {
    int rc = 0;
    const bool gst = c->cfg.gst_use != 0;
    const bool styled = style != nullptr;
    if (spectrogram && !c->cfg.voc_use) return fail(c, GSTTACO_E_INVALID, "the context was created without Vocoder_Taco1");
    // (gsttaco_inference_step_forced: the step count follows from the teacher; its workspace exists before any capture)
    if ((rc = forced ? check_forced(c, teacher, Tq, B, Tv, Tref1, &steps) : check_shape(c, B, Tv, Tref1, steps))) return rc;
    if (steps == 0) steps = c->steps_max;
    hipStream_t s = (hipStream_t)stream;
    const bool voc = spectrogram != nullptr;
    const size_t meld = c->cfg.mel_dim;
    // inputs -> the workspace the cached graphs read, and the seed: ONE launch (injected masks / noise -- parity runs -- keep their copies)
    const bool masked = token_lengths != nullptr;
    {
        GtCopySegs cs{};
        add_seg(cs, tokens, c->w_tokens, (size_t)B * Tv);
        if (styled) add_seg(cs, style, c->w_gst, (size_t)B * c->cfg.gst_att);
        else if (gst) { add_seg(cs, mels_for_gst, c->w_mels_in, (size_t)B * Tref1 * meld); add_seg(cs, mel_lengths, c->w_mel_len, (size_t)B); }
        if (masked) add_seg(cs, token_lengths, c->w_tok_len, (size_t)B);
        cs.seed = seed; cs.seed_dst = c->w_seed;
        HIPCHECK(c, gt_launch_copy_segments(cs, s));
    }
    // (the seed went with the input launch; the teacher frames are the forced graph's input copy)
    if ((rc = stage_decode_inputs(c, s, mask, noise, nullptr, forced ? teacher : nullptr, Tq, B, Tv, steps))) return rc;
    // Three graph segments: the encoder and the vocoder each contain a persistent BiLSTM launch and are chained process-wide
    // (run_cached, g_persist_event); the segment between them -- GST, value projection, the decode loop, the postnet: 95 % of the
    // call -- overlaps freely with other contexts' work.  The encoder / vocoder segments share their cached graphs with
    // gsttaco_encode / gsttaco_vocoder.
    // With the style given the encoder segment is gsttaco_encode's (no fork, no side stream) and the middle one starts at the value
    // projection (kSegStepStyled).  w_gst was written by this call's input copy on `s`; a forked call in front of it on `s` wrote w_gst on
    // the side stream and joined it into `s` inside its encoder segment, so the copy is ordered behind that write.
    const bool fork = gst && !styled && c->gst_fork;
    const int Tfork = fork ? Tref1 : 0;
    if ((rc = run_cached(c, s, GraphKey{.kind = fork ? kSegEncoderFork : kSegEncoder, .B = B, .Tv = Tv, .Tref1 = Tfork, .masked = masked},
                         [&](hipStream_t st, const LaunchForms& forms) { return enqueue_encoder(c, st, forms, B, Tv, masked, Tfork); }))) return rc;
    // (a forced call's middle segment has a kind of its own, kSegStepForced: with the style given Tref1 is 0, with mels it is >= 2, so the two
    // bodies never share a key; keys carry the step count, one graph per distinct S)
    const GraphKey key{.kind = forced ? kSegStepForced : styled ? kSegStepStyled : kSegStep, .B = B, .Tv = Tv, .Tref1 = Tref1, .steps = steps,
                       .has_mask = mask != nullptr, .has_noise = noise != nullptr, .prof = c->prof_every, .masked = masked};
    rc = run_cached(c, s, key, [&](hipStream_t st, const LaunchForms& forms) {
        int r2 = 0;
        if (gst && !styled && !fork) r2 = enqueue_gst(c, st, B, Tref1);
        if (!r2) r2 = enqueue_value_proj(c, st, B, Tv);
        if (!r2) r2 = enqueue_decode(c, st, forms, B, Tv, steps, mask != nullptr, noise != nullptr, masked, forced);
        if (!r2) r2 = enqueue_postnet(c, st, B, steps * c->r, c->w_pre, c->w_mel);
        return r2;
    });
    if (rc) return rc;
    if (voc) {                                                                                 // Model.py:126-129
        if ((rc = run_cached(c, s, GraphKey{.kind = kSegVocoder, .B = B, .steps = steps * c->r},
                             [&](hipStream_t st, const LaunchForms& f) { return enqueue_vocoder(c, st, f, B, steps * c->r, c->w_mel, c->w_spec); }))) return rc;
    }
    // outputs out of the workspace the graphs write: ONE launch
    const size_t nf = (size_t)B * steps * c->r * meld;
    {
        GtCopySegs cs{};
        add_seg(cs, c->w_mel, mel, nf);
        if (pre_mel) add_seg(cs, c->w_pre, pre_mel, nf);
        if (voc) add_seg(cs, c->w_spec, spectrogram, (size_t)B * steps * c->r * c->cfg.spec_dim);
        add_seg(cs, c->w_stop, stop, (size_t)B * steps);
        add_seg(cs, c->w_align, align, (size_t)B * steps * Tv);
        HIPCHECK(c, gt_launch_copy_segments(cs, s));
    }
    return 0;
}

}  // namespace

extern "C" {

int gsttaco_inference_step(gsttaco_ctx* c, const int32_t* tokens, const int32_t* token_lengths, const float* mels_for_gst, const int32_t* mel_lengths,
                           const float* mask, const float* noise, uint64_t seed, int B, int Tv, int Tref1, int steps,
                           float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    const bool gst = c->cfg.gst_use != 0;
    if (!tokens || !mel || !stop || !align) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (gst && (!mels_for_gst || !mel_lengths)) return fail(c, GSTTACO_E_INVALID, "GST is enabled, but no mel information.");
    if (!gst) Tref1 = 0;
    if (gst && Tref1 < 2) return fail(c, GSTTACO_E_INVALID, "mels_for_gst needs at least one frame after the prepended zero frame");
    return inference_step(c, tokens, token_lengths, mels_for_gst, mel_lengths, nullptr, mask, noise, seed, B, Tv, Tref1, steps,
                          mel, stop, align, pre_mel, spectrogram, stream);
}

int gsttaco_inference_step_styled(gsttaco_ctx* c, const int32_t* tokens, const int32_t* token_lengths, const float* style,
                                  const float* mask, const float* noise, uint64_t seed, int B, int Tv, int steps,
                                  float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->cfg.gst_use) return fail(c, GSTTACO_E_INVALID, "GST is not used");
    if (!tokens || !style || !mel || !stop || !align) return fail(c, GSTTACO_E_INVALID, "null argument");
    return inference_step(c, tokens, token_lengths, nullptr, nullptr, style, mask, noise, seed, B, Tv, 0, steps,
                          mel, stop, align, pre_mel, spectrogram, stream);
}

// gsttaco_inference_step / gsttaco_inference_step_styled with the decoder teacher-forced (Taco2.py:161,185): exactly one style source
// when GST is on (both ignored when it is off), no `steps` -- S = ceil((Tq - 1) / r).
int gsttaco_inference_step_forced(gsttaco_ctx* c, const int32_t* tokens, const int32_t* token_lengths, const float* mels_for_gst,
                                  const int32_t* mel_lengths, const float* style, const float* mask, const float* noise, uint64_t seed,
                                  int B, int Tv, int Tref1, const float* teacher, int Tq,
                                  float* mel, float* stop, float* align, float* pre_mel, float* spectrogram, void* stream) {
    int rc = check_ready(c);
    if (rc) return rc;
    const bool gst = c->cfg.gst_use != 0;
    if (!tokens || !mel || !stop || !align) return fail(c, GSTTACO_E_INVALID, "null argument");
    if (gst && ((mels_for_gst != nullptr) == (style != nullptr)))
        return fail(c, GSTTACO_E_INVALID, "exactly one of mels_for_gst and style must be given");
    if (gst && mels_for_gst && !mel_lengths) return fail(c, GSTTACO_E_INVALID, "GST is enabled, but no mel information.");
    if (!gst) { mels_for_gst = nullptr; mel_lengths = nullptr; style = nullptr; }
    if (!gst || style) Tref1 = 0;
    else if (Tref1 < 2) return fail(c, GSTTACO_E_INVALID, "mels_for_gst needs at least one frame after the prepended zero frame");
    return inference_step(c, tokens, token_lengths, mels_for_gst, mel_lengths, style, mask, noise, seed, B, Tv, Tref1, 0,
                          mel, stop, align, pre_mel, spectrogram, stream, teacher, Tq, true);
}

int gsttaco_synchronize(gsttaco_ctx* c, void* stream) {
    if (!c) return GSTTACO_E_INVALID;
    HIPCHECK(c, hipStreamSynchronize((hipStream_t)stream));
    // (the GST fork's side stream is joined into `stream` by every call that forks; after an error return in between it may not be)
    if (c->gst_fork && c->side_stream && !c->capturing) HIPCHECK(c, hipStreamSynchronize(c->side_stream));
    note_give_up(c);
    if (c->gave_up) {
        // the ONLY place the give-up words are cleared: behind the synchronisation, nothing of this context polls them any more
        c->gave_up = 0;
        c->h_err[0] = 0; c->h_err[1] = 0; c->h_err[2] = 0;
        return fail(c, GSTTACO_E_HIP, "a hand-off wait of the persistent decode launch / the persistent BiLSTM launch / the fused decode-LSTM launch gave up (its workgroups "
                                      "were not co-resident: is another process or a CU mask sharing this GPU?): the outputs of the calls since the last "
                                      "gsttaco_synchronize are invalid.  Repeat them: the context now uses the next launch form down (launches per decode step / "
                                      "one launch per BiLSTM time step / two launches for the two LSTM cells)");
    }
    return 0;
}

int gsttaco_set_graph_policy(gsttaco_ctx* c, int max_cached, int capture_after) {
    if (!c || max_cached < 0 || capture_after < 1) return GSTTACO_E_INVALID;
    c->graph_cache_max = max_cached;
    c->graph_capture_after = capture_after;
    while ((int)c->graphs.size() > max_cached) {
        auto old = lru_graph(c);
        HIPCHECK(c, hipDeviceSynchronize());
        (void)hipGraphExecDestroy(old->second.exec);
        c->graphs.erase(old);
    }
    return 0;
}

int gsttaco_graph_cache_size(const gsttaco_ctx* c) { return c ? (int)c->graphs.size() : GSTTACO_E_INVALID; }

int gsttaco_set_profiling(gsttaco_ctx* c, int every) {
    if (!c || every < 0) return GSTTACO_E_INVALID;
    c->prof_every = every;
    return 0;
}

int gsttaco_get_profile(gsttaco_ctx* c, int layer, float* avg_ms, int* count) {
    if (!c || layer < 0 || layer > 4 || !avg_ms || !count) return GSTTACO_E_INVALID;
    const int n = c->prof_count[layer];
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        HIPCHECK(c, hipEventElapsedTime(&ms, c->prof_ev[layer][2 * i], c->prof_ev[layer][2 * i + 1]));
        sum += ms;
    }
    *count = n;
    *avg_ms = n ? (float)(sum / n) : 0.f;
    return 0;
}

int gsttaco_debug_stamps(gsttaco_ctx* c, unsigned long long* host_out96) {
    if (!c || !host_out96 || !c->w_dbg) return GSTTACO_E_INVALID;
    HIPCHECK(c, hipMemcpy(host_out96, c->w_dbg, 3 * 32 * 8, hipMemcpyDeviceToHost));
    return 0;
}

// CRC-32C (Castagnoli, reflected 0x82F63B78), slicing-by-8: the checksum of TensorFlow checkpoint bundles
// (gst_tacotron_amd/tf_checkpoint.py reads / writes them).  Host only.
uint32_t gsttaco_crc32c(const void* data, size_t n, uint32_t crc) {
    static uint32_t tab[8][256];
    static bool ready = false;
    if (!ready) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            tab[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) tab[t][i] = (tab[t - 1][i] >> 8) ^ tab[0][tab[t - 1][i] & 0xff];
        ready = true;
    }
    const uint8_t* p = static_cast<const uint8_t*>(data);
    uint32_t c = crc ^ 0xffffffffu;
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = tab[7][lo & 0xff] ^ tab[6][(lo >> 8) & 0xff] ^ tab[5][(lo >> 16) & 0xff] ^ tab[4][lo >> 24] ^
            tab[3][hi & 0xff] ^ tab[2][(hi >> 8) & 0xff] ^ tab[1][(hi >> 16) & 0xff] ^ tab[0][hi >> 24];
        p += 8; n -= 8;
    }
    while (n--) c = tab[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

int gsttaco_debug_randomness(gsttaco_ctx* c, float* host_masks, float* host_noise, int steps, int B, int Tv) {
    if (!c || steps < 1 || B < 1 || Tv < 1 || steps > c->steps_max || B > c->cfg.max_batch || Tv > c->cfg.max_tokens)
        return GSTTACO_E_INVALID;
    HIPCHECK(c, hipDeviceSynchronize());
    if (host_masks && c->masks_lazy) {          // (the last decode derived its keep decisions from the seed: the tensor is written now)
        HIPCHECK(c, gt_launch_rng_fill(c->w_seed, c->w_masks, nullptr, steps, B, c->P0, c->P1, Tv, c->cfg.prenet_rate, nullptr));
        HIPCHECK(c, hipDeviceSynchronize());
    }
    if (host_masks && c->dec_padded) {          // (in the caller's layout: the columns of the caller's prenet sizes)
        float* tmp = nullptr;
        const int p0 = c->cfg.prenet[0], p1 = c->cfg.prenet[1];
        const size_t n = (size_t)steps * B * (p0 + p1);
        HIPCHECK(c, hipMalloc((void**)&tmp, n * 4));
        hipError_t e = gt_launch_relayout_masks(c->w_masks, tmp, steps, B, p0, p1, c->P0, c->P1, 0, nullptr);
        if (e == hipSuccess) e = hipMemcpy(host_masks, tmp, n * 4, hipMemcpyDeviceToHost);
        (void)hipFree(tmp);
        HIPCHECK(c, e);
    } else if (host_masks)
        HIPCHECK(c, hipMemcpy(host_masks, c->w_masks, (size_t)steps * B * (c->P0 + c->P1) * 4, hipMemcpyDeviceToHost));
    if (host_noise) HIPCHECK(c, hipMemcpy(host_noise, c->w_noise, (size_t)steps * B * Tv * 4, hipMemcpyDeviceToHost));
    return 0;
}

int gsttaco_debug_handoff_error(gsttaco_ctx* c, uint32_t* host_out) {
    if (!c || !host_out || !c->w_err) return GSTTACO_E_INVALID;
    HIPCHECK(c, hipDeviceSynchronize());
    // pending = raised by a kernel or noted by a later enqueue, and not yet reported by gsttaco_synchronize
    *host_out = 0;
    for (const GiveUpForm& f : kGiveUpForms) *host_out |= (c->h_err[f.word] | ((c->gave_up >> f.word) & 1u)) << (8 * f.word);
    return 0;
}

int gsttaco_debug_counters(const gsttaco_ctx* c, uint64_t out[4]) {
    if (!c || !out) return GSTTACO_E_INVALID;
    out[0] = c->n_persist_enqueued;
    out[1] = c->allow.bilstm_persist ? 1u : 0u;
    out[2] = c->n_persist_decodes;
    out[3] = c->allow.persist_decode ? 1u : 0u;
    return 0;
}

int gsttaco_debug_conv_prepare(gsttaco_ctx* c, const gsttaco_conv_desc* d, const float* w_host, const float* scale_host,
                               const float* shift_host, int* id) {
    if (!c || !d || !w_host || !id) return GSTTACO_E_INVALID;
    if (!c->finalized) return fail(c, GSTTACO_E_WEIGHTS, "weights not finalized (call gsttaco_finalize_weights)");
    const int ldw = d->ldw ? d->ldw : d->n;
    if (d->taps < 1 || d->cin < 4 || d->cin % 4 || d->n < 1 || ldw < d->n || ldw % 4 || !(d->forms & GSTTACO_CONV_FORM_FP32) || (d->forms & ~127))
        return fail(c, GSTTACO_E_INVALID, "gsttaco_debug_conv_prepare: bad descriptor");
    gsttaco_ctx::DbgConv e{};
    const int rc = prepare_conv_forms(c, &e.L, w_host, d->taps, d->cin, d->n, ldw, scale_host, shift_host, d->forms);
    if (rc) return rc;
    e.forms = d->forms;
    c->dbg_conv.push_back(e);
    *id = (int)c->dbg_conv.size() - 1;
    return 0;
}

int gsttaco_debug_conv_run(gsttaco_ctx* c, int id, const gsttaco_conv_call* k, const void* x, const int32_t* tokens,
                           const int32_t* row_len, const float* rowbias, const float* res, void* out, int* variant, void* stream) {
    if (!c || !k || !x || !out) return GSTTACO_E_INVALID;
    if (id < 0 || id >= (int)c->dbg_conv.size()) return fail(c, GSTTACO_E_INVALID, "gsttaco_debug_conv_run: unknown weight id");
    const ConvLayer& L = c->dbg_conv[id].L;
    const int f = k->forms;
    if ((f & c->dbg_conv[id].forms) != f || !(f & GSTTACO_CONV_FORM_FP32) || k->B < 1 || k->T < 1 || (k->ldo && k->ldo < L.cout) || !(k->x_absmax >= 0.f))
        return fail(c, GSTTACO_E_INVALID, "gsttaco_debug_conv_run: bad call (a form that was not prepared?)");
    // (the weight half through the builder the production call sites use; the call's own half from the caller's fields: no allocation,
    // no synchronisation)
    ConvGemmArgs a = conv_args(L, f);
    a.x = reinterpret_cast<const float*>(x); a.tokens = tokens;
    a.rowbias = rowbias; a.res = res; a.row_len = row_len; a.pool2 = k->pool2;
    a.x_bf16 = k->x_bf16; a.out_bf16 = k->out_bf16;
    a.wino_x3 = k->wino_x3; a.wino_min_wgs = k->wino_min_wgs; a.x_absmax = k->x_absmax;
    a.out = reinterpret_cast<float*>(out); a.ldo = k->ldo ? k->ldo : L.cout;
    a.B = k->B; a.T = k->T; a.pad_before = k->pad_before; a.act = k->act;
    a.conv2d = k->conv2d; a.H = k->H; a.W = k->W; a.Wo = k->Wo; a.kw = k->kw; a.stride = k->stride; a.pad_h = k->pad_h; a.pad_w = k->pad_w;
    a.xb = k->xb;
    const int v = gt_conv_gemm_variant(a);
    if (variant) *variant = v;
    if (v == GSTTACO_CONV_V_INVALID) return fail(c, GSTTACO_E_INVALID, "gsttaco_debug_conv_run: no kernel takes this call");
    HIPCHECK(c, gt_launch_conv_gemm(a, reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

int gsttaco_postnet_variants(const gsttaco_ctx* c, int B, int Tf, int32_t variants[8]) {
    if (!c || !variants || B < 1 || Tf < 1 || !c->finalized) return GSTTACO_E_INVALID;
    for (int i = 0; i < c->cfg.n_post && i < 8; ++i) variants[i] = gt_conv_gemm_variant(postnet_call(c, i, B, Tf));
    return 0;
}

int gsttaco_encoder_variants(const gsttaco_ctx* c, int B, int Tv, int32_t variants[8], int32_t* rows_path) {
    if (!c || !variants || !c->finalized || B < 1 || Tv < 1) return GSTTACO_E_INVALID;
    const bool rows = encoder_rows_path(c, B, Tv);
    if (rows_path) *rows_path = rows ? 1 : 0;
    for (int i = 0; i < c->cfg.n_enc_conv && i < 8; ++i) variants[i] = gt_conv_gemm_variant(encoder_call(c, i, B, Tv, rows));
    return 0;
}

int gsttaco_vocoder_variants(const gsttaco_ctx* c, int which, int B, int Tf, int32_t variants[32], int32_t* count) {
    if (!c || !variants || !count || !c->finalized || !c->cfg.voc_use || B < 1 || Tf < 1) return GSTTACO_E_INVALID;
    const gsttaco_config& g = c->cfg;
    int n = 0;
    switch (which) {
    case GSTTACO_VOC_BANK: n = g.bank_count; break;
    case GSTTACO_VOC_PROJ: n = g.n_voc_proj; break;
    case GSTTACO_VOC_PROJ_DENSE: n = c->voc_pd.w ? 1 : 0; break;
    case GSTTACO_VOC_HIGHWAY_IN: n = c->voc_hin.w ? 1 : 0; break;
    case GSTTACO_VOC_HIGHWAY: n = g.highway_count; break;
    case GSTTACO_VOC_DENSE: n = 1; break;
    default: return GSTTACO_E_INVALID;
    }
    *count = n;
    for (int i = 0; i < n && i < 32; ++i) variants[i] = gt_conv_gemm_variant(vocoder_call(c, which, i, B, Tf));
    return 0;
}

int gsttaco_debug_wino_h_planes(const double* u, int al, int cin, int wino_cin, int cout, int npad, uint16_t* planes, int32_t* su, int32_t* sv) {
    if (!u || !planes || !su || al < 1 || cin < 1 || wino_cin < cin || cout < 1 || npad < cout) return GSTTACO_E_INVALID;
    wino_split_h_planes(u, al, cin, wino_cin, cout, npad, planes, su);
    if (sv) *sv = gt_wino5h_sv();
    return 0;
}

int gsttaco_debug_raise_handoff_error(gsttaco_ctx* c, uint32_t bits) {
    if (!c || !c->h_err) return GSTTACO_E_INVALID;
    c->h_err[0] |= bits & 0x7Fu;
    c->h_err[2] |= (bits >> 7) & 1u;          // (bit 7: the persistent decode launch's word)
    c->h_err[1] |= (bits >> 8) & 0xFFu;
    if (bits >> 16) {               // fault injection for real: member (bits >> 16) - 1 of every group of the NEXT persistent launches exits
        c->debug_drop_member = (int)(bits >> 16) - 1;                // at once, so the launch's waits run into their bound
        HIPCHECK(c, hipDeviceSynchronize());                           // (an executable may still be running)
        for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second.exec);   // (captured launches carry the old argument)
        c->graphs.clear();
    }
    return 0;
}

int gsttaco_decode_plan(const gsttaco_ctx* c, int Tv, int32_t plan[3]) {
    if (!c || !plan || Tv < 1) return GSTTACO_E_INVALID;
    const DecodePlan p = plan_decode(c, c->allow, c->cfg.max_batch, Tv, false);      // (these three answers do not depend on the batch)
    plan[0] = p.fused ? 1 : 0;
    plan[1] = p.z0 ? 1 : 0;
    plan[2] = (p.lean_x[0] && p.lean_x[1]) ? 1 : 0;
    return 0;
}

int gsttaco_decode_plan_fields(const gsttaco_ctx* c, int B, int Tv, int forced, int32_t fields[GSTTACO_PLAN_COUNT]) {
    if (!c || !fields || !c->finalized || B < 1 || Tv < 1) return GSTTACO_E_INVALID;
    const DecodePlan p = plan_decode(c, c->allow, B, Tv, false, forced != 0);
    fields[GSTTACO_PLAN_PERSIST] = p.persist ? 1 : 0;
    fields[GSTTACO_PLAN_PERSIST_BF16] = p.persist_bf16 ? 1 : 0;
    fields[GSTTACO_PLAN_FUSED] = p.fused ? 1 : 0;
    fields[GSTTACO_PLAN_LEAN_FRONT] = p.lean_front ? 1 : 0;
    fields[GSTTACO_PLAN_LEAN_REC] = p.lean_rec;
    fields[GSTTACO_PLAN_Z0] = p.z0 ? 1 : 0;
    fields[GSTTACO_PLAN_FUSE12] = p.fuse12;
    fields[GSTTACO_PLAN_LEAN_X0] = p.lean_x[0] ? 1 : 0;
    fields[GSTTACO_PLAN_LEAN_X1] = p.lean_x[1] ? 1 : 0;
    fields[GSTTACO_PLAN_CO_TILES] = p.co_tiles;
    fields[GSTTACO_PLAN_LEAN_PROJ] = p.lean_proj ? 1 : 0;
    fields[GSTTACO_PLAN_MIRROR] = p.mirror ? 1 : 0;
    fields[GSTTACO_PLAN_DEC_PADDED] = c->dec_padded ? 1 : 0;
    fields[GSTTACO_PLAN_PJ_TILES] = c->proj_z.ntiles;
    return 0;
}

int64_t gsttaco_lstm_launch_bytes(const gsttaco_ctx* c, int which, int B) {
    if (!c || which < 0 || which > 3) return GSTTACO_E_INVALID;
    // Algorithmic bytes of one launch at batch B and T_v = max_tokens: every weight once, every activation row once
    // in and once out (the re-reads of the shared activations by every workgroup are NOT algorithmic).
    const int64_t P0 = c->P0, P1 = c->P1, A = c->att, H1 = c->H1, H2 = c->H2, mel = c->cfg.mel_dim, Tv = c->cfg.max_tokens;
    const DecodePlan p = plan_decode(c, c->allow, B, (int)Tv, false);
    const bool fused = p.fused;         // (the recurrent halves ride beside the front launch)
    // weight bytes by the dtype the packs hold: bf16 under Use_Mixed_Precision for the LSTM / projection GEMMs (biases, activations,
    // partial sums and the prenet / query weights stay fp32)
    const int64_t wb = c->lstm_x[0].bf16 ? 2 : 4;
    auto gemm = [&](int64_t K, int64_t N, int64_t extra_row_floats) { return wb * K * N + 4 * N + 4 * (int64_t)B * (K + extra_row_floats); };
    const int64_t ntile2 = (H2 + 3) / 4;
    const int64_t co_tiles = p.co_tiles;
    const int64_t rec_tile = wb * H2 * 16 + 4 * 16 + 4 * (int64_t)B * 16;      // one layer-2 recurrent tile: weights + bias + its partial sums
    switch (which) {
        case 0:     // LSTM layer 1: x-half only when the recurrent half runs in the front launch
            return fused ? gemm(P1 + A, 4 * H1, 4 * H1 + 3 * H1) : gemm(P1 + A + H1, 4 * H1, 3 * H1);
        case 1:
            return fused ? gemm(H1, 4 * H2, 4 * H2 + 3 * H2) : gemm(H1 + H2, 4 * H2, 3 * H2);
        case 2: {   // front: prenet x2 + query weights (fp32 in every mode), processed memory, alignments; + workers' recurrent halves
            int64_t b = 4 * (mel * P0 + P0 + P0 * P1 + P1 + P1 * A + A) + 4 * (int64_t)B * (Tv * A + mel + 2 * Tv + P1 + A);
            if (fused) b += gemm(H1, 4 * H1, 4 * H1) + (ntile2 - co_tiles) * rec_tile + 4 * (int64_t)B * H2;
            return b;
        }
        default: {  // projection (+ co-scheduled layer-2 recurrent tiles)
            int64_t b = gemm(H2 + A, c->proj_out, c->proj_out);
            if (fused) b += co_tiles * rec_tile;
            return b;
        }
    }
}

}  // extern "C"
