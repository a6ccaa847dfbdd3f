// Host-visible launch interface of the gfx950 kernels (internal; the public ABI is include/gsttaco.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

// ---------------------------------------------------------------- skinny_gemm.hip
enum { EPI_LINEAR = 0, EPI_RELU_DROP = 1, EPI_LSTM = 2, EPI_PARTIAL = 3 };

// Activation ("A operand") layouts of a [M, K] matrix:
//   row-major : element (row, k) at ptr[row*ld + k]
//   blocked   : MFMA-fragment order [k/16][row/16][lane = ((k%16)/4)*16 + row%16][k%4], i.e. one 1-KiB block per
//               (16 k, 16 rows): a wave reads its A fragment of a k-block with ONE coalesced 16-byte-per-lane load
//               instead of 16 rows x 64 B at a power-of-two row stride.  All decode-loop activations use it.
struct SkinnySeg {
    const float* ptr;   // row-major: [M, len] rows, 16-byte aligned; blocked: first k-block of the segment
    int64_t ld;         // row-major: row stride in floats (multiple of 4); blocked: unused
    int nkb;            // len / 16
    int blocked;        // 1 = blocked layout
};
__host__ __device__ inline size_t gt_blk_off(int row, int k, int MT) {
    return (((size_t)(k >> 4) * MT + (row >> 4)) << 8) + (size_t)(((((k & 15) >> 2) << 4) + (row & 15)) * 4 + (k & 3));
}

// bf16 MIRROR of a blocked activation buffer (mixed precision, batches above 32 rows): [K/32][MT][64 lanes][8 bf16], lane l of 32-k
// block j and M-tile mt holds row 16 mt + (l & 15), slot i <-> k = 32 j + 16 (i >> 2) + 4 (l >> 4) + (i & 3): exactly the A operand of
// v_mfma_f32_16x16x32_bf16 the consumers used to assemble from two fp32 fragments (lean_body.h), rounded (RNE) once by the producer
// instead of by every consumer.  Offset in bf16 elements.
__host__ __device__ inline size_t gt_blk_off_h(int row, int k, int MT) {
    return ((((size_t)(k >> 5) * MT + (row >> 4)) << 6) + (size_t)((((k & 15) >> 2) << 4) + (row & 15))) * 8 + (size_t)((((k >> 4) & 1) << 2) + (k & 3));
}

struct SkinnyArgs {
    const float* wp;    // packed weights [ntiles][nkb][64 lanes][4]; when `bf16`: bf16 [ntiles][ceil(nkb/2)][64 lanes][8]
    const float* bias;  // [ntiles*16] in packed column order
    SkinnySeg seg[3];
    int nkb;            // sum of seg nkb
    int M;              // batch rows
    int N;              // LINEAR: valid output columns; LSTM: hidden units H
    int n_split;        // LINEAR: columns >= n_split go to out2 (projection: mel | stop)
    int MT;             // M-tiles (ceil(M/16)) of blocked operands / outputs
    int out_blocked;    // LINEAR: `out` is a blocked activation buffer; LSTM: `h` is
    float* out; int64_t ldo;
    float* out2; int64_t ldo2;
    // LINEAR, optional third region: columns [col3, N) go to out3, [n_split, n_valid2) to out2, [n_valid2, col3) are padding
    float* out3; int64_t ldo3; int col3, n_valid2;
    // EPI_RELU_DROP
    const float* mask; int64_t ldm;     // keep-mask [M, N] or NULL -> Philox
    float drop_rate, drop_scale;
    const uint64_t* seed_ptr; uint32_t rng_step, rng_stream;   // Philox seed lives in HBM so a cached graph can be re-seeded
    // EPI_LSTM
    float* c;           // [M, H] cell state, updated in place
    float* h; int64_t ldh;
    // EPI_PARTIAL writes / EPI_LSTM adds pre-activation partial sums, tile order [tile][MT*16 rows][16 cols]
    float* partial_out;
    const float* partial_in;
    // masked-mode extension: EPI_LSTM rows whose time index t_index >= row_len[row] do not exist --
    // h is written as 0 and the cell state is left untouched (NULL = the reference's unmasked behaviour)
    const int32_t* row_len; int t_index;
    int bf16;           // mixed precision (Use_Mixed_Precision): weights are bf16, activations are rounded to bf16 on load,
                        // products accumulate in fp32 on v_mfma_f32_16x16x32_bf16; everything else stays fp32
    int keep_weights;   // 1: load the weights with the default cache policy (they are re-read every step and small enough
                        // to stay L2-resident) instead of non-temporally
    unsigned long long* dbg;   // diagnostic phase stamps (s_memrealtime, 100 MHz) of block 0, or NULL
};

// Recurrent-half worker job (lean_body.h gt_lean_partial): tiles of  h . W_h + b  as pre-activation partial sums.
struct LeanPartialArgs {
    const float* wp;            // packed weights [tiles][NKB][64][4]
    const float* bias;          // [tiles*16]
    const float* x;             // blocked state [NKB][MT][64][4]
    float* partial_out;         // [tile][MT*16 rows][16 cols]
    int MT;
    const uint16_t* xh = nullptr;   // bf16 mirror of x (gt_blk_off_h) or NULL: read instead of x by the bf16 multi-chunk bodies
};

enum { TAG_GENERIC = 0, TAG_DEC_LSTM1 = 1, TAG_DEC_LSTM2 = 2, TAG_ENC_BILSTM = 3 };
hipError_t gt_launch_skinny(int epi, const SkinnyArgs& a0, const SkinnyArgs* a1, int ntiles, hipStream_t stream,
                            int tag = TAG_GENERIC);
// EPI_LINEAR main GEMM (tiles [0, ntiles)) plus co-scheduled worker workgroups in the same launch that compute tiles
// [co_begin, co_end) of an independent EPI_PARTIAL GEMM `co` on CUs the small main grid leaves idle, one tile per worker.
hipError_t gt_launch_skinny_co(const SkinnyArgs& main_args, int ntiles, const SkinnyArgs& co, int co_begin, int co_end, hipStream_t stream);

// ---- lean decode-step kernels (lean_body.h): fp32, blocked operands, compile-time K; the host falls back to the
// general kernels above for any other shape or precision.
// Input half of a decode LSTM cell: z = x . W_x + partial_in (recurrent half + bias, from the workers), gates, cell update.
struct LstmXArgs {
    const float* wp;            // packed W_x [H/4 tiles][nkb][64][4]
    const float* x;             // blocked input [nkb][MT][64][4]
    const float* partial_in;    // [tiles][MT*16][16]
    float* c;                   // [M, H] cell state, in place
    float* h;                   // blocked output state
    unsigned long long* dbg;
    int M, MT, H;
    int nkb;                    // K / 16 (the bf16 variant's 32-k blocks need not fill NW x KPW)
    const uint16_t* xh = nullptr;   // bf16 mirror of x or NULL (read by the bf16 multi-chunk body instead of x)
    uint16_t* hh = nullptr;         // bf16 mirror of h or NULL (written beside h)
};
bool gt_lstm_x_supported(int nkb);
// Both cells in one launch with an in-kernel hand-off of h1 (skinny_gemm.hip gt_lstm12_kernel): fp32, batch <= 32.
#ifndef GT_L12_NSH
#define GT_L12_NSH 8        // shards (a 128-byte line each) of the fused LSTM launches' arrival counter; GT_L12_NSH * 32 words per decode step
#endif
struct Lstm12Args {
    LstmXArgs l1, l2;           // exactly the two launches' arguments (l2.x == l1.h)
    uint32_t* arrive;           // GT_L12_NSH x 32 words, zero before the launch: per-shard arrival counters of THIS decode step
    uint32_t* err;              // host-mapped give-up word
    uint32_t expect;            // arrivals to wait for = the grid size (fault injection: one more, so the wait runs into its bound)
};
bool gt_lstm12_supported(int nkb1, int nkb2, int H1, int H2, int M, int slots);      // slots: resident workgroups = occupancy x CUs
int gt_lstm12_blocks_per_cu(int which);     // occupancy of the fused kernels: 0 = gt_lstm12_kernel, 1 / 2 = gt_lstm12_mc_kernel fp32 / bf16
hipError_t gt_launch_lstm12(const Lstm12Args& a, hipStream_t stream);
bool gt_lstm12_mc_supported(int nkb1, int nkb2, int H1, int H2, int M, int slots);     // the same at batches above 32 rows (fp32 / bf16)
int gt_lstm12_mc_grid(int H);
hipError_t gt_launch_lstm12_mc(const Lstm12Args& a, bool bf16, hipStream_t stream);
hipError_t gt_launch_lstm_x(const LstmXArgs& a, int nkb, int tag, bool bf16, hipStream_t stream);

// One time step of a Bidirectional LSTM (reference Taco2.py:39-43, 394-398) whose input halves x_t . W_x + b were hoisted
// into ONE GEMM over all time steps (columns in tile order: tile*16 + gate*4 + unit%4): z = zx + h_{t-1} . W_h, gates, cell
// update.  grid = (H/4 tiles, ceil(M/32), 2 directions).
struct BiLstmDir {
    const float* wp;        // packed W_h [H/4 tiles][H/16][64][4]
    const float* hprev;     // blocked state [H/16][MT][64][4]
    float* hnext;
    float* c;               // [M, H]
    const float* zx;        // hoisted input half of THIS time step: element (row, tile, col) at zx[row*ldz + tile*16 + col]
    float* out;             // row-major output of this time step: (row, unit) at out[row*ldo + unit]
    int t_index;            // masked-mode extension (A12): rows with t_index >= row_len[row] write h = 0 and keep c
};
struct BiLstmArgs {
    BiLstmDir d[2];
    const int32_t* row_len;
    int64_t ldz, ldo;
    int M, MT, H;
};
bool gt_bilstm_lean_supported(int nkb_h);

// Persistent BiLSTM: every time step of both directions in one launch (skinny_gemm.hip gt_bilstm_persist_kernel).
// Group g = direction + 2 * M-tile lives on XCD g.
struct BiLstmPersistArgs {
    const float* wp[2];         // packed W_h per direction [H/4 tiles][H/16][64][4] (bf16 pack [tiles][H/32][64][8] in mixed precision)
    const float* zx;            // hoisted input halves: (row, time tt, direction d, tile, col) at zx[row*ldz + tt*8H + d*4H + tile*16 + col]
    float* out;                 // (row, tt, d, unit) at out[row*ldo + tt*2H + d*H + unit]
    float* h;                   // workspace [8 groups][3 slots][H/16][64][4]: blocked state of the group's 16 rows, each word tagged in bit 30;
                                // ZEROED before the launch (tag 0 = never written)
    uint32_t* flags;            // [8] member counters, zeroed before the launch (the words right behind `h`: one zero-fill for both)
    const int32_t* row_len;     // masked-mode extension (A12) or NULL
    uint32_t* err;              // host-mapped; bit 0: a wait gave up (every member then leaves the launch)
    int64_t ldz, ldo;
    int M, MT, H, T;
    int debug_drop_member;      // -1; >= 0: fault injection, that member rank of every group exits at once (tests)
};
bool gt_bilstm_persist_supported(int H, int B, int n_cu);
hipError_t gt_launch_bilstm_persist(const BiLstmPersistArgs& a, bool bf16, hipStream_t stream);
hipError_t gt_bilstm_persist_init();       // opt in to >64 KiB dynamic LDS; call once outside stream capture
int gt_bilstm_persist_blocks_per_cu();     // occupancy of the persistent kernel (must be 1)
hipError_t gt_launch_bilstm_lean(const BiLstmArgs& a, hipStream_t stream);

// Projection [h2 | ctx] -> mel frames | stop logit | (optional) next step's prenet-0 pre-activations, with co-scheduled
// recurrent-half worker tiles of LSTM layer 2 for the next step in the same launch.
struct ProjArgs {
    const float* wp; const float* bias;
    const float* xa; const float* xb; int nkb_a;    // blocked segments: k-blocks [0, nkb_a) from xa, the rest from xb
    int M, MT, N;                                   // N: valid columns
    int n_split, n_valid2, col3;                    // [0,n_split) -> out, [n_split,n_valid2) -> out2, [col3,N) -> out3 (NULL: none)
    float* out; int64_t ldo;
    float* out2; int64_t ldo2;
    float* out3; int64_t ldo3;
    unsigned long long* dbg;                        // diagnostic stamps (8 slots) or NULL
    const uint16_t* xah = nullptr; const uint16_t* xbh = nullptr;   // bf16 mirrors of xa / xb or NULL (gt_proj_mc_kernel<true>)
};
bool gt_proj_lean_supported(int nkb_main, int nkb_co);
hipError_t gt_launch_proj_lean(const ProjArgs& m, int ntiles, const float* co_wp, const float* co_bias, const float* co_x,
                               float* co_out, int co_begin, int co_end, bool bf16, hipStream_t stream);

// ---------------------------------------------------------------- gemm_conv.hip
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };

struct ConvGemmArgs {
    const float* x;         // [B, T, Cin] channels-last (or embedding table when tokens != NULL)
    const int32_t* tokens;  // optional [B, T]: row (b,t) of x is x[tokens[b,t], :]
    const float* w;         // [taps, Cin, N] (TF Conv1D kernel layout) == [taps*Cin, N]
    const float* scale;     // [N] or NULL (=1)   epilogue: y = acc*scale + shift (+rowbias[b]) ; act ; (+res)
    const float* shift;     // [N] or NULL (=0)
    const float* rowbias;   // [B, N] or NULL
    const float* res;       // [B*T, ldo] residual or NULL
    const int32_t* row_len; // masked-mode extension (A12): input rows t >= row_len[b] read as zero, or NULL
    int ldw;                // row stride of w in floats (0 = N); lets N be odd (513) over a zero-padded multiple of 4
    int pool2;              // 1: the input row is max(x[t], x[t+1]) -- MaxPool1D(2, stride 1, 'same') fused into the gather
    // mixed precision (Use_Mixed_Precision): the weights TRANSPOSED in bf16, [ceil(N/256)*256][ldk] with k contiguous and
    // zero padding (ldk = ceil(taps*Cin/64)*64), or NULL = fp32 path.  Activations are rounded to bf16 on their way into
    // LDS, products accumulate in fp32 (v_mfma_f32_32x32x16_bf16), the epilogue and the output stay fp32.
    const void* wt_bf16;
    int ldk;
    // mixed precision, activations BETWEEN bf16 layers: `x` / `out` hold bf16 instead of fp32 (same [rows, channels] layout, half the
    // bytes).  The consumer rounds its input to bf16 on the way into LDS anyway, so storing the rounded value changes no result.
    // Only the bf16 kernels honour them (the host sets them for layers it knows run there); residual input and `res` stay fp32.
    int x_bf16, out_bf16;
    // Winograd F(2,5) (gemm_conv.hip): the transformed weights U[6][Cin][N] = G . w (float64 at finalize), or NULL
    const float* wino_u;    // F(2,5): [6][wino_cin][N]
    const float* wino_u4;   // F(4,5): [8][wino_cin][N], or NULL
    int wino_cin;           // rows of each U_xi: Cin rounded up to a multiple of 32 (zero rows for the padding)
    // the same U as three bf16 planes (hi + mid + lo = the float64 transform to 2^-25), [xi][plane][wino_npad columns][wino_cin], k
    // contiguous: the transform-domain GEMMs then run as split-bf16 x6 on the bf16 matrix pipe at fp32 accuracy (conv_wino_split.hip)
    const void* wino_s;     // F(2,5), or NULL
    const void* wino_s4;    // F(4,5), or NULL
    int wino_npad;          // N rounded up to the kernel's 128-column block
    const void* gemm_s;     // taps == 1: W itself as three bf16 planes [plane][wino_npad][Cin], k contiguous -> the plain split-bf16 GEMM
                            // (conv_wino_split.hip gt_gemm_split_kernel), or NULL
    int wino_x3;            // 1 = the split Winograd kernel's reduced form (two planes, products hh hm mh: ~2^-16, GSTTACO_WINO_SPLIT=3)
    int wino_min_wgs;       // 0 = the default grid-fill rule (Winograd only where >= 240 workgroups); else the caller's threshold -- the
                            // split-bf16 kernel also pays on the encoder's 4 096-row layers, whose F(2,5) grid is 128 workgroups
    float* out;             // [B*T, ldo]
    int64_t ldo;
    int B, T, Cin, N, taps, pad_before, act;
    // 2-D mode (GST reference encoder, GST.py:23-31): rows are (b, ho, wo) with T = Ho*Wo, k = (i*kw + j)*Cin + c reads
    // x[b][ho*stride + i - pad_h][wo*stride + j - pad_w][c] of an NHWC input with batch stride xb floats; taps = kh*kw.
    int conv2d, H, W, Wo, kw, stride, pad_h, pad_w;
    int64_t xb;
    // Bounded-input Winograd (conv_wino_split.hip, plane mode fp16 x3): the call site's PROMISE that |x| <= x_absmax everywhere (0 = no
    // promise: the form is never taken), the same U as TWO fp16 planes of U[:, n] 2^SU[n], [xi][plane][wino_npad][wino_cin], and the
    // per-column epilogue scale that undoes both scalings: scale[n] 2^-(SV + SU[n]) (the power alone where the layer has no scale).
    float x_absmax;
    const void* wino_h;     // F(2,5), or NULL
    const void* wino_h4;    // F(4,5), or NULL
    const float* wino_hsc;  // [N] for wino_h
    const float* wino_hsc4; // [N] for wino_h4
};
// The largest bound the fp16 x3 form is built for: its transform-domain scaling 2^SV is derived from it (gt_wino5h_sv).
constexpr float GT_WINO_H_XMAX = 1.0f;
// true when `a` may run the fp16 x3 form of transform mo (4 / 2): the planes are there and the site has promised |x| <= GT_WINO_H_XMAX
inline bool gt_wino5h_takes(const ConvGemmArgs& a, int mo) {
    return a.x_absmax > 0.f && a.x_absmax <= GT_WINO_H_XMAX && !a.wino_x3 && (mo == 4 ? a.wino_h4 && a.wino_hsc4 : a.wino_h && a.wino_hsc);
}
int gt_wino5h_sv();      // SV: the fp16 x3 form's input transform carries the factor 2^SV (conv_wino_split.hip)

hipError_t gt_launch_conv_gemm(const ConvGemmArgs& a, hipStream_t stream);
int gt_conv_gemm_variant(const ConvGemmArgs& a);     // the GSTTACO_CONV_V_* the launch runs (include/gsttaco.h)
hipError_t gt_conv5_bf16_init();           // opt in to >64 KiB dynamic LDS; call once outside stream capture
// conv_wino_split.hip: the Winograd five-tap kernel on the bf16 pipe (split-bf16 x6); mo = 4 / 2 outputs per tile
hipError_t gt_conv_wino5s_init();
hipError_t gt_launch_conv_wino5s(const ConvGemmArgs& a, int mo, hipStream_t stream);
bool gt_gemm_split_applies(const ConvGemmArgs& a);
hipError_t gt_launch_gemm_split(const ConvGemmArgs& a, hipStream_t stream);
// Highwaynet combine (reference Taco2.py:409-424): z [M, 2S] = [relu-branch | sigmoid-branch] pre-activations,
// out = relu(z_h) * sigmoid(z_t) + x * (1 - sigmoid(z_t));  S % 4 == 0
hipError_t gt_launch_highway(const float* z, const float* x, float* out, int64_t M, int S, hipStream_t stream);

// ---------------------------------------------------------------- attention.hip
struct AttnStepArgs {
    const float* q; int64_t ldq;        // [B, A] projected query
    const float* pm;                    // [B, Tv, A] processed memory (Dense_Value(memory), hoisted)
    const float* v;                     // [A] attention_v
    const float* score_bias;            // [1]
    const float* prev;  int64_t ldprev; // previous alignment rows [B, Tv] (NULL -> one-hot(0), Steps.py:201-206)
    const float* noise; int64_t ldnoise;// N(0,1) [B, Tv] or NULL -> Philox
    float* align; int64_t ldalign;      // out [B, Tv]
    float* ctx; int64_t ldctx;          // out [B, A] (row-major) or blocked buffer when ctx_mt > 0
    int ctx_mt;
    int B, Tv, A, type;                 // type: GSTTACO_ATT_*
    float sigmoid_noise;
    const uint64_t* seed_ptr; uint32_t rng_step;
    const int32_t* tok_len;             // masked-mode extension (A12): positions >= tok_len[b] do not exist, or NULL
    // LSA extension (type == GSTTACO_ATT_LSA): location conv [k,1,F] + bias [F], location dense [F,A] + bias [A],
    // additive bias [A]; state [B,Tv] = cumulative (or last) alignment, read and updated in place
    const float *loc_cw, *loc_cb, *loc_dw, *loc_db, *att_bias;
    float* lsa_state;
    int loc_k, loc_f, lsa_cumulate, lsa_smoothing;
    int rows_lds;                       // rows of pm staged in LDS per chunk
};

hipError_t gt_launch_attn_step(const AttnStepArgs& a, hipStream_t stream);
hipError_t gt_attn_init();     // opt in to >64 KiB dynamic LDS; call once outside stream capture
hipError_t gt_launch_set_seed(uint64_t* dst, uint64_t seed, hipStream_t stream);
hipError_t gt_launch_rng_fill(const uint64_t* seed_ptr, float* masks, float* noise, int steps, int B, int P0, int P1, int Tv,
                              float drop_rate, hipStream_t stream);
hipError_t gt_launch_relayout_masks(const float* src, float* dst, int steps, int B, int p0, int p1, int P0, int P1, int to_padded, hipStream_t stream);
// up to 8 device-to-device copies of 4-byte words + the call's seed in one launch (attention.hip gt_copy_segments_kernel)
struct GtCopySegs { const void* src[8]; void* dst[8]; size_t words[8]; int n; uint64_t seed; uint64_t* seed_dst; };
hipError_t gt_launch_copy_segments(const GtCopySegs& S, hipStream_t stream);
hipError_t gt_launch_embed_rows(const float* table, const int32_t* tokens, float* out, int rows, int C, hipStream_t stream);
hipError_t gt_launch_zero(float* p, size_t n_floats, hipStream_t stream);   // n rounded up to a multiple of 4 floats
size_t gt_attn_lds_bytes(int Tv, int A, int loc_f, int loc_k, int* rows_lds);
// the dynamic LDS gt_attn_init opts the attention step into: a workgroup's whole 160 KiB (gsttaco_create refuses what needs more)
constexpr size_t GT_ATTN_LDS_MAX = 160 * 1024;

// ---------------------------------------------------------------- dec_front.hip
struct DecFrontArgs {
    const float* frame; int64_t ldframe;    // [B, mel] last emitted frame (zero rows, ld 0, at step 0)
    const float* z0;                        // [B, P0] prenet-0 PRE-activations incl. bias, produced with the previous step's
                                            // projection (NULL: compute them here from `frame`)
    const float* w0; const float* b0;       // prenet0 [mel, P0] (TF layout), [P0]
    const float* w1; const float* b1;       // prenet1 [P0, P1], [P1]
    const float* wq; const float* bq;       // attention Query [P1, A], [A]
    const float* mask0; const float* mask1; // keep-masks [B,P0] / [B,P1] or NULL -> Philox
    float drop_rate, drop_scale;
    const uint64_t* seed_ptr; uint32_t rng_step;
    const float* pm;                        // [B, Tv, A] processed memory
    const float* v; const float* score_bias;
    const float* prev; int64_t ldprev;      // NULL -> one-hot(0)
    const float* noise; int64_t ldnoise;    // NULL -> Philox
    float* align; int64_t ldalign;
    float* xa;                              // out, BLOCKED [ (P1+A)/16 ][MT][64][4]: prenet output k in [0,P1), context k in [P1,P1+A)
    int MT;
    int B, Tv, mel, P0, P1, A, type;
    float sigmoid_noise;
    const int32_t* tok_len;    // masked-mode extension (A12): memory positions >= tok_len[b] do not exist, or NULL
    unsigned long long* dbg;   // diagnostic phase stamps of block 0, or NULL
    // Worker workgroups (blockIdx.x >= B) of the same launch: recurrent halves h_{t-1}.W_h + b of the two decode LSTM
    // layers, written as pre-activation partial sums.  They only need the PREVIOUS step's state, so they run on the
    // ~224 CUs the per-utterance front end leaves idle.  n_workers == 0 disables them.
    SkinnyArgs rec[2];
    int rec_begin[2], rec_end[2];   // tile ranges [begin, end) of each layer handled by this launch's workers
    int n_workers;
    // Batches above 32 rows on the lean bodies (dec_front.hip front_worker): whole jobs [0, sched_pf) go round-robin to the pure
    // workers, jobs [sched_pf, sched_pf + sched_ne) are cut into pieces of sched_e chunks for them as well, and the remaining
    // jobs into pieces of sched_y chunks for the first `utt_jobs` utterance workgroups, which take them once their utterance is
    // done (a job = a pair of tiles over every 32-row chunk of the batch; at 128 rows in fp32 it outlasts the chain).
    // Otherwise sched_pf = all jobs, the rest 0.
    int utt_jobs, sched_pf, sched_ne, sched_e, sched_y;
    LeanPartialArgs lrec[2];        // the same two GEMMs for the lean body (fp32, K = 1024); used when lean_rec != 0
    int lean_rec;                   // 0: general body, 1: lean fp32, 2: lean bf16
    int keep_hash;                  // throughput mode at dropout rate 0.5 and the reference's prenet / attention sizes: rows of
                                    // the prenet-1 / query weights that the (hashed) keep decisions zero are not requested
    int lean_front;                 // 1: the lean utterance path (front_lean.h) where its preconditions hold; 0: the general kernel
    uint16_t* xah;                  // bf16 mirror of xa (gt_blk_off_h), written beside it, or NULL
    // type == GSTTACO_ATT_LSA (dec_front_lsa.hip; the four-kernel path's AttnStepArgs fields of the same names): `prev` is then the
    // state buffer itself (ldprev = Tv), read at the start of the step and rewritten at its end
    const float* loc_pack;                  // the LSA weights as the kernel's LDS image (LsaPack below), 16-byte aligned
    float* lsa_state;                       // [B, Tv] cumulative (or previous) alignment
    int loc_k, loc_f, lsa_cumulate, lsa_smoothing;
};
// LDS image of the LSA weights on the fused front end, built once on the host (gsttaco.cpp) and copied per step with 16-byte loads:
//   dw  [LFp][LDWS]  location Dense kernel [F, A], rows zero-padded to the MFMA k granule (4)
//   cw  [LKp][LCS]   location Conv1D kernel [K, 1, F] as [K][F], taps padded to 4, filters to the MFMA n granule (16)
//   cb  [LFc]        Conv1D bias (zero beyond F)
//   ab  [A]          Dense bias + the additive attention bias
// Row strides LDWS = A + 8 and LCS = LFc + 8 floats put the four k rows of a B fragment on different banks; LFS = LFc + 4 is the row
// stride of the location-feature tile the kernel writes behind the memory tile.
struct LsaPack { int LFc, LFp, LKp, LFS, LDWS, LCS, off_cw, off_cb, off_ab, total; };
inline __host__ __device__ LsaPack gt_lsa_pack(int A, int LF, int LK) {
    LsaPack p;
    p.LFc = (LF + 15) & ~15; p.LFp = (LF + 3) & ~3; p.LKp = (LK + 3) & ~3;
    p.LFS = p.LFc + 4; p.LDWS = A + 8; p.LCS = p.LFc + 8;
    p.off_cw = p.LFp * p.LDWS; p.off_cb = p.off_cw + p.LKp * p.LCS; p.off_ab = p.off_cb + p.LFc;
    p.total = (p.off_ab + A + 3) & ~3;
    return p;
}
// (loc_f > 0: the LSA form, whose operands share the LDS with the processed-memory tile)
bool gt_dec_front_supported(int mel, int P0, int P1, int A, int Tv, int loc_f = 0, int loc_k = 0);
// dec_front_lsa.hip: the LSA instantiations of the general kernel (shape = 0..4 for A = 16, 32, 64, 128, 256)
hipError_t gt_front_lsa_init();
void gt_front_lsa_launch(int shape, bool z0, int lean, bool exact, dim3 grid, size_t lds, hipStream_t s, const DecFrontArgs& a);
hipError_t gt_dec_front_init();
hipError_t gt_launch_dec_front(const DecFrontArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- persist_decode.hip
// The whole decoder loop as ONE persistent launch (batch <= 128, T_v <= 256, fp32, the reference's decoder sizes): see the file.
struct PersistDecodeArgs {
    // weights: the launch path's packs (MFMA-fragment order [tile][k-block][lane][4])
    const float *w1x, *w1h, *b1h, *w2x, *w2h, *b2h;   // lstm_x[l].wp / lstm_h[l].wp / lstm_h[l].bias
    const float *wp, *bp;                              // proj_z: projection columns | padding | fused prenet-0 columns
    int pj_tiles, n_out, n_split, z_col0;              // tiles of proj_z; mel*r + 1; mel*r; first prenet-0 column
    const float *W1, *b1, *Wq, *bq, *av, *score_bias;  // prenet-1 [P0][P1] + bias, query [P1][A] + bias (plain layouts), attention v, score bias
    const float* pm;                                   // processed memory [B][Tv][A]
    const float* noise;                                // N(0,1) [steps][B][Tv] (injected or pre-generated), or NULL when sigmoid_noise == 0
    const float* masks;                                // keep masks [steps][mask0 B*P0 | mask1 B*P1], or NULL (hashed / no dropout)
    const uint64_t* seed_ptr;
    const int32_t* tok_len;                            // masked-mode extension (A12) or NULL
    float drop_rate, drop_scale, sigmoid_noise;
    int keep_hash, att_type;
    // att_type == GSTTACO_ATT_LSA (the one-group kernel, up to 128 tokens): the location weights as the LDS image the fused front end
    // uses (LsaPack above; resident in the chain workgroups' LDS for the whole launch) -- the state lives in their LDS
    const float* loc_pack;
    int loc_f, loc_k, lsa_cumulate, lsa_smoothing;
    // state / workspace
    float* xa[2];                                      // blocked [24][MT][256], ping-pong by step parity
    float* h1[2]; float* h2[2];                        // blocked [64][MT][256]
    uint16_t* xah[2]; uint16_t* h1h[2]; uint16_t* h2h[2];  // mixed precision: the bf16 mirrors (gt_blk_off_h) of xa / h1 / h2, ping-pong by step parity
    int bf16;                                          // 1: the bf16 kernel (weights are the bf16 packs, activations travel as mirrors only)
    uint2* z0g;                                        // [B][256] {value bits, step tag}
    float* hpart;                                      // [2][32][512] (bf16 kernel: [2][64][1024]) recurrent halves of the chain workgroups' tiles
    float* stash;                                      // [256][16][512] the group kernels' chain workgroups park their tile state here during the chain
    uint32_t* ctl;                                     // gt_persist_decode_ctl_words() words, zeroed by the launcher
    uint32_t* err;                                     // host-mapped give-up word of this launch
    // outputs
    float* pre; int64_t ld_pre;                        // [B][steps*r*mel]
    float* stop;                                       // [B][steps]
    float* align; int64_t ld_align;                    // [B][steps][Tv]
    int B, MT, Tv, steps, co_tiles;                    // co_tiles: layer-2 tiles whose recurrent half the launch path sums in 8-wave order
    int G, n_chain, tvp, twopass;                      // filled in by the launcher: groups of rows, chain workgroups, T_v rounded up to 64, and
                                                       // whether the group kernels' chain workgroups sum their recurrent halves through 8 slabs
    int expect_extra;                                  // fault injection (tests): the all-to-all waits expect this many arrivals too many
    unsigned long long* dbg;                           // diagnostic stamps [3 roles][32] or NULL (GSTTACO_STAMPS=1)
};
size_t gt_persist_decode_ctl_words();
bool gt_persist_decode_supported(int mel, int r, int P0, int P1, int A, int H1, int H2, int B, int Tv, int pj_tiles, int pj_nkb, int slots, int bf16);
int gt_persist_decode_max_batch();
bool gt_persist_decode_lsa_fits(int B, int Tv, int loc_f, int loc_k);       // the LSA chain: one group, <= 128 tokens, operands beside the memory tile
hipError_t gt_persist_decode_init();                   // opt in to > 64 KiB dynamic LDS; once, outside stream capture
int gt_persist_decode_blocks_per_cu();
hipError_t gt_launch_persist_decode(const PersistDecodeArgs& a, const float* b0, hipStream_t stream);

// ---------------------------------------------------------------- gst.hip
struct Conv2dArgs {
    const float* x;         // [B, H, W, Cin] (batch stride xb floats; lets frame 0 be skipped)
    int64_t xb;
    const float* w;         // [kh, kw, Cin, Cout]
    const float* scale;     // [Cout] folded BN
    const float* shift;
    float* out;             // [B, Ho, Wo, Cout]
    int B, H, W, Cin, Cout, Ho, Wo, k, stride, pad_h, pad_w;
};
hipError_t gt_launch_conv2d_bn_relu(const Conv2dArgs& a, hipStream_t stream);

struct GstTailArgs {
    const float* x;         // [B, T2, gru_in] conv stack output
    const int32_t* mel_len; // [B]
    const float* gru_w;     // [gru_in, 3u]
    const float* gru_u;     // [u, 3u]
    const float* gru_b;     // [2, 3u]
    const float* dense_w;   // [u, D]
    const float* dense_b;   // [D]
    const float* q_w;       // [D, A]
    const float* q_b;       // [A]
    const float* v_tok;     // [ntok, A]  = tanh(tokens).Wv + bv  (batch-invariant, precomputed at finalize)
    const float* ln_g;      // [A]
    const float* ln_b;      // [A]
    float* gst;             // [B, A]
    float* attn;            // [B, heads, ntok] the normalised attention weights e / den of every head, or NULL = not stored
    float* query;           // [B, A] the projected query (the residual term), or NULL = not stored
    int B, T2, gru_in, u, D, A, ntok, heads, stride_prod;
};
hipError_t gt_launch_gst_tail(const GstTailArgs& a, hipStream_t stream);
// whether gt_gst_tail_kernel can run these sizes (divisibility, lane counts, its dynamic LDS against 160 KiB); `why` names the limit that fails.
// gt_launch_gst_tail refuses exactly what this refuses, and gsttaco_create asks it, so a context that exists never fails there.
bool gt_gst_tail_supported(int gru_in, int u, int D, int A, int heads, int ntok, std::string* why);
hipError_t gt_gst_init();      // opt in to >64 KiB dynamic LDS; call once outside stream capture

// gst[b] = LayerNorm(concat_h(weights[b, h, :] . v_tok[:, h-slice]) + query[b]): the tail's last stage with the attention weights GIVEN
// (any real numbers: not normalised, not clipped) instead of computed from a reference.  EXTENSION (style control, DESIGN A14).
struct GstComposeArgs {
    const float* weights;   // [B, heads, ntok]
    const float* query;     // [B, A], or NULL = 0 (tokens alone: outside the training distribution, the residual always carried a query)
    const float* v_tok;     // [ntok, A]
    const float* ln_g;      // [A]
    const float* ln_b;      // [A]
    float* gst;             // [B, A]
    int B, A, ntok, heads;
    int gru_in, u, D;       // the model's other GST sizes: the launch accepts what gt_gst_tail_supported accepts
};
hipError_t gt_launch_gst_compose(const GstComposeArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- audio.hip
struct AudioFrontArgs {
    const float* wav;           // [B, ld_wav] float samples in [-1, 1)
    const int32_t* wav_len;     // [B]
    double* mse;                // [B, ld_mse] workspace: trim frame mean-squares
    int32_t* bounds;            // [B, 2] workspace: trimmed (start, length) in samples
    float* mels;                // [B, cap_frames, n_mels] mels_for_gst layout (frame 0 = zeros), or NULL
    float* specs;               // [B, cap_frames, n_fft/2+1] linear spectrograms (Audio.spectrogram) in the same layout, or NULL
    int32_t* mel_len;           // [B] frames excluding the prepended one
    const float* window;        // [n_fft] hann (periodic), zero-padded centred to n_fft
    const float2* twiddle;      // [n_fft/2] exp(-2 pi i k / n_fft)
    const float* mel_basis;     // [n_mels, n_fft/2+1]
    const int32_t* band_lo;     // [n_mels] first non-zero bin of each band
    const int32_t* band_hi;     // [n_mels] one past the last non-zero bin
    int B, ld_wav, ld_mse, cap_frames, n_fft, log2_h, hop, n_mels, trim_frame, trim_hop;
    float preemph, trim_gain, top_db, max_abs;
};
hipError_t gt_launch_audio_front(const AudioFrontArgs& a, hipStream_t stream);

struct GriffinLimArgs {
    const float* spec;          // [B, T, n_fft/2+1] normalised spectrogram (the vocoder's output layout)
    const int32_t* frames;      // [B] frames to use per utterance, or NULL (= T)
    const float* init_phase;    // [B, T, n_fft/2+1] uniform [0,1) (x 2 pi), or NULL -> Philox(seed)
    float* mag;                 // [B, T, n_fft/2+1] workspace: S ^ power
    const float* frm_old;       // [B, T, n_fft] windowed inverse-FFT frames of the previous iteration
    float* frm_new;
    float* ybuf;                // [B, ld_y] final overlap-added signal (before de-emphasis)
    float* wav;                 // [B, ld_wav] output
    int32_t* wav_len;           // [B] output: hop * (frames - 1), or NULL
    const float* window;        // [n_fft]
    const double* win_sq;       // [n_fft] window^2 in float64
    const float2* twiddle;      // [n_fft/2]
    int64_t ld_y;
    uint64_t seed;
    int B, T, n_fft, log2_h, hop, ld_wav, iters;
    float power, ref_level_db, max_abs, preemph;
};
hipError_t gt_gl_init();
hipError_t gt_launch_griffin_lim(GriffinLimArgs a, float* frm_a, float* frm_b, hipStream_t stream);

// ---------------------------------------------------------------- forced.hip
// Teacher forcing (Taco2.py:161,185): out [S][B][mel] <- teacher[b, t*r, :] of teacher [B, Tq, mel], S = ceil((Tq - 1) / r)
hipError_t gt_launch_stage_teacher(const float* teacher, float* out, int B, int Tq, int S, int r, int mel, hipStream_t stream);
// dur [B, Tv] int32 <- frames per token of align [B, S, Tv]: frame f < L_b counts for argmax_{j < n_b} align[b, f / r, j] (lowest
// index on a tie); n_b = tok_len ? tok_len[b] : Tv, L_b = mel_len ? min(mel_len[b], S*r) : S*r.  One workgroup per utterance.
hipError_t gt_launch_forced_durations(const float* align, const int32_t* tok_len, const int32_t* mel_len, int32_t* dur, int B, int S,
                                      int Tv, int r, hipStream_t stream);

// ---------------------------------------------------------------- report.hip
// gt_launch_rng_fill's tensors (masks [steps][B*P0 | B*P1], noise [steps][B][Tv]) with row b drawn from seeds[b] (device [B]) as a
// batch of one draws its row 0: gt_drop_keep(seeds[b], step, layer, 0, col, ..), gt_philox(seeds[b], position, step, 0, GT_RNG_NOISE)
hipError_t gt_launch_fill_randomness(const uint64_t* seeds, float* masks, float* noise, int steps, int B, int P0, int P1, int Tv,
                                     float drop_rate, hipStream_t stream);
// report [B][8] int32 (stop_step, frames, end_gap, max_jump, back_steps, max_stall, visited, nonfinite: include/gsttaco.h) and focus [B]
// (or NULL) of stop [B,S], align [B,S,Tv], tok_len [B] or NULL, mel [B,S*r,mel_dim] or NULL.  One workgroup per utterance.
hipError_t gt_launch_utterance_report(const float* stop, const float* align, const int32_t* tok_len, const float* mel, int32_t* report,
                                      float* focus, int B, int S, int Tv, int r, int mel_dim, hipStream_t stream);


// ---------------------------------------------------------------- loss.hip
// The per-utterance loss sums of a teacher-forced pass (the table in include/gsttaco.h).  The target of prediction frame t is
// teacher[b, 1 + t]; only t < min(length, Tq - 1) is read.  One workgroup per utterance, double throughout after the fp32 subtraction.
struct LossArgs {
    const float* pre_mel;       // [B, S*r, mel_dim]
    const float* mel;           // [B, S*r, mel_dim]
    const float* stop;          // [B, S]
    const float* spec;          // [B, S*r, spec_dim], or NULL
    const float* teacher;       // [B, Tq, mel_dim] (frame 0 = the go frame)
    const float* spec_target;   // [B, Tq, spec_dim], or NULL
    const int32_t* mel_len;     // [B], or NULL (= Tq - 1)
    const int32_t* spec_len;    // [B], or NULL (= Tq - 1)
    double* losses;             // [B][6]
    int B, S, Tq, r, mel_dim, spec_dim;
};
hipError_t gt_launch_losses(const LossArgs& a, hipStream_t stream);


// ---------------------------------------------------------------- dtw.hip
// Mel-cepstral distortion along a DTW path (the contract: gsttaco_mel_dtw in include/gsttaco.h).  Two launches on the stream: the features
// of every used frame of both sides into fx / fy, then one workgroup per utterance for the sweep and the walk back.
struct DtwArgs {
    const float* x;             // [B, Tx, mel_dim] at batch stride x_stride floats (synthesised)
    const float* y;             // [B, Ty, mel_dim] at batch stride y_stride floats (reference)
    const int32_t* x_len;       // [B], or NULL (= Tx); clipped to [0, Tx]
    const int32_t* y_len;       // [B], or NULL (= Ty); clipped to [0, Ty]
    int64_t x_stride, y_stride;
    const double* basis;        // [n_ceps][mel_dim] rows 1..n_ceps of the orthonormal DCT-II, or NULL with n_ceps == 0
    double scale;               // dB per unit of the normalised mel, over sqrt(2)
    float clip_lo, clip_hi;     // the normalisation's range
    double *fx, *fy;            // workspace: [B, F, Tx] and [B, F, Ty] features, F = n_ceps ? n_ceps : mel_dim
    uint8_t* backptr;           // workspace: [B, Tx, Ty] predecessor of each cell (0 diagonal, 1 up, 2 left); needed only with path
    double* cost;               // [B]
    int32_t* path_len;          // [B]
    int32_t* path;              // [B, Tx + Ty - 1, 2], or NULL
    int B, Tx, Ty, mel_dim, n_ceps;
};
#define GT_DTW_MAX_LDS (160 * 1024)         // the sweep's rolling diagonals: gt_dtw_lds_bytes(Ty) of LDS, Ty <= 4551
size_t gt_dtw_lds_bytes(int Ty);
hipError_t gt_dtw_init();                   // once per process and device, before a launch that needs more than 64 KiB of LDS
hipError_t gt_launch_mel_dtw(const DtwArgs& a, hipStream_t stream);


// ---------------------------------------------------------------- resample.hip
// resampy 'kaiser_best' resampling of a batch of rows (the contract: gsttaco_resample in include/gsttaco.h).  One launch per
// GT_RS_MAX_ROWS rows; the per-row parameters and the rate pairs' tables travel by value in the kernel arguments.
#define GT_RS_THREADS 256
#define GT_RS_NWIN 32769                    // 64 zero crossings x 512 table entries + 1
#define GT_RS_MAX_FACTOR 16                 // sr_in <= 16 sr_out and sr_out <= 16 sr_in
#define GT_RS_MAX_PAIRS 8
#define GT_RS_MAX_ROWS 256
#define GT_RS_PASS 255                      // ResampleArgs::slot of a row already at the target rate
struct ResamplePair {
    const double* time;         // [time_len] the accumulated time register: time[0] = 0, time[t] = time[t-1] + 1 / ratio
    const double2* table;       // [GT_RS_NWIN] {win, delta}: the table times min(1, ratio) and its forward differences (the last 0)
    double scale;               // min(1, ratio)
    int step;                   // int(scale * 512)
    int time_len;
};
struct ResampleArgs {
    const float* x;             // [.., ld_in]
    float* y;                   // [.., ld_out]
    int row0, rows;             // rows row0 .. row0 + rows - 1 of x and y; entry b of the arrays below is row row0 + b
    int ld_in, ld_out;
    ResamplePair pair[GT_RS_MAX_PAIRS];
    int32_t n_in[GT_RS_MAX_ROWS];       // valid input samples (<= ld_in)
    int32_t n_out[GT_RS_MAX_ROWS];      // int(n_in * ratio) computed samples (<= ld_out); [n_out, ld_out) is zero-filled
    uint8_t slot[GT_RS_MAX_ROWS];       // index into pair, or GT_RS_PASS
};
hipError_t gt_launch_resample(const ResampleArgs& a, hipStream_t stream);


// ---------------------------------------------------------------- pitch.hip
// F0 by YIN on the mel front end's frame grid, and the pitch errors of two F0 tracks along a path (the contracts: gsttaco_pitch and
// gsttaco_pitch_errors in include/gsttaco.h).  The trim of gsttaco_pitch is the front end's: gt_launch_trim_bounds (audio.hip) runs
// ahead of gt_launch_pitch and leaves the bounds it reads.
#define GT_PITCH_MAX_SPAN 3072              // W + tau_max: 4 bytes per sample and 16 per lag (tau_max + 1 <= span) stay within 64 KiB of LDS
struct PitchArgs {
    const float* wav;           // [B, ld_wav]
    const int32_t* wav_len;     // [B]
    const int32_t* bounds;      // [B, 2] (start, length) as gt_trim_bounds_kernel left them, or NULL = (0, wav_len[b]): no trim
    float* f0;                  // [B, cap_frames] Hz, 0 = unvoiced
    float* aperiodicity;        // [B, cap_frames], or NULL
    int32_t* frames;            // [B]
    double sr, threshold;
    int B, ld_wav, cap_frames, n_fft, hop, W, tau_min, tau_max;
};
hipError_t gt_launch_trim_bounds(const AudioFrontArgs& a, hipStream_t stream);      // audio.hip: the front end's first two launches
hipError_t gt_launch_pitch(const PitchArgs& a, hipStream_t stream);

struct PitchErrorArgs {
    const float* f0_x;          // [B, Tx] synthesised
    const float* f0_y;          // [B, Ty] reference
    const int32_t* x_len;       // [B], or NULL (= Tx); clipped to [0, Tx]
    const int32_t* y_len;       // [B], or NULL (= Ty); clipped to [0, Ty]
    const int32_t* path;        // [B, path_cap, 2] cells (i, j), or NULL = (i, i) for i < min(Lx, Ly)
    const int32_t* path_len;    // [B] (with path); clipped to [0, path_cap]
    int32_t* counts;            // [B][6]
    double* sums;               // [B][2]
    double gross;
    int B, Tx, Ty, path_cap;
};
hipError_t gt_launch_pitch_errors(const PitchErrorArgs& a, hipStream_t stream);


// ---------------------------------------------------------------- tsne.hip
// The style map: exact t-SNE of style embeddings (the contracts: gsttaco_style_affinities and gsttaco_style_map in include/gsttaco.h).
#define GT_TSNE_MAX_N 8192                  // the search keeps a row of distances in the registers of one workgroup: 1024 lanes x 8
struct TsneAffinityArgs {
    const float* x;             // [N, ldx], D channels used
    double* p;                  // [N, N]: distances, then p_{j|i}, then p_ij, each in place
    double* beta;               // [N]
    int32_t* search_iters;      // [N], or NULL
    int64_t ldx;
    float perplexity;
    int N, D;
};
hipError_t gt_launch_style_affinities(const TsneAffinityArgs& a, hipStream_t stream);

struct TsneMapArgs {
    const double* p;            // [N, N]
    double* y;                  // [N, 2], as velocity and gains
    double* velocity;
    double* gains;
    double* partials;           // [5 N + 1] workspace: S, A_x, A_y, B_x, B_y per row, and Z for the KL
    double* kl;                 // [1], or NULL
    double exaggeration, momentum, final_momentum, eta;
    int N, first_iter, iters, stop_lying_iter, mom_switch_iter;
};
hipError_t gt_launch_style_map(const TsneMapArgs& a, hipStream_t stream);


// ---------------------------------------------------------------- melgan.hip
// The neural vocoder: the MelGAN generator, mel -> waveform (the contract: gsttaco_melgan in include/gsttaco.h).
#define GT_MG_MAX_RATIOS 8
#define GT_MG_MAX_RES 8
#define GT_MG_MAX_STAGES (2 + GT_MG_MAX_RATIOS * (1 + GT_MG_MAX_RES))
enum { GT_MG_IN = 0, GT_MG_UP = 1, GT_MG_RES = 2, GT_MG_OUT = 3 };
// One launch of the chain.  Channel counts with _p are the padded ones (multiples of 16) the fragment packs and the workspace use.
struct MgStage {
    int kind;
    int cin, cout;              // the network's channel counts
    int cin_p, n_p;
    int rate_in, rate_out;      // samples per mel frame of the stage's input and output
    int r, dil;                 // GT_MG_UP: the ratio;  GT_MG_RES: the dilation
    int tile, form;             // time tile (GT_MG_UP: in input positions, else in output samples); form: N-tiles a wave item owns (GT_MG_OUT: 0)
    size_t lds;                 // dynamic LDS of a workgroup, bytes
    // device operands (gsttaco_melgan_finalize).  GT_MG_RES: w0 / b0 = conv3, w1 = shortcut, w2 = conv1, b1 = the two biases summed
    const float *w0, *b0, *w1, *w2, *b1;
};
struct MgPlan {
    int n_stages;
    MgStage st[GT_MG_MAX_STAGES];
    int mel_dim, hop, min_frames;
    float slope;
    size_t ws_floats_per_frame;     // the largest activation of the chain, floats per mel frame of one row
};
// Fills the plan's shapes, tiles and LDS sizes (no device use).  Returns NULL, or the reason the configuration cannot run.
const char* gt_melgan_make_plan(int mel_dim, int base, int n_ratios, const int* ratios, int n_res, float slope, MgPlan* plan);
hipError_t gt_melgan_prepare();
struct MgCall {
    const float* mel;           // [B, T, mel_dim]
    const int32_t* frames;      // [B] or NULL
    float* wav;                 // [B, ld_wav]
    int32_t* wav_lengths;       // [B] or NULL
    float* ws[2];               // ping-pong activations, B * T * ws_floats_per_frame floats each
    int B, T, ld_wav;
    int only;                   // -1: the whole chain; else that launch alone, on what the workspace holds (timing: gsttaco_melgan_debug_stage)
};
hipError_t gt_launch_melgan(const MgPlan& plan, const MgCall& call, hipStream_t stream);


// ---------------------------------------------------------------- waveglow.hip
// The flow vocoder: WaveGlow inference, mel -> waveform (the contract: gsttaco_waveglow in include/gsttaco.h).
#define GT_WG_MAX_FLOWS 32
#define GT_WG_MAX_LAYERS 10
#define GT_WG_MAX_GROUP 16
#define GT_WG_FLOW_TILE 64      // columns of a workgroup of gt_wg_flow_kernel
enum { GT_WG_UP = 0, GT_WG_LAYER = 1, GT_WG_FLOW = 2 };
// device operands (gsttaco_waveglow_finalize).  w_in / w_cond / b_ac: the gate GEMM's, columns in pair order (gt_waveglow_pack_gate),
// b_ac the two biases summed;  w_rs / b_rs: res_skip, [res | skip] each padded to C_p (the last layer: skip only)
struct WgLayerOps { const float *w_in, *w_cond, *b_ac, *w_rs, *b_rs; };
// w_start [c_k / 2][C_p], b_start [C_p];  w_end [C][16], b_end [16];  winv [16][16] = inverse(W_k), zero padded
struct WgFlowOps { const float *w_start, *b_start, *w_end, *b_end, *winv; };
struct WgPlan {
    int mel_dim, hop, win, G, F, EE, ES, NL, C;
    int mel_p, C_p, S, S_p, n_rem;      // S = mel_dim * G; _p: rounded up to 16
    int ck[GT_WG_MAX_FLOWS];            // channels of flow k
    int up_tile, up_form;               // the upsampler: frames of a workgroup, N-tiles a wave item owns
    int tile, form, kc;                 // the WN layer: columns of a workgroup, N-tiles of the gate GEMM a wave item owns, K chunk
    size_t up_lds, lds, flow_lds;       // dynamic LDS of a workgroup, bytes
    size_t ws_floats_per_column;        // spect S_p + hid 2 C_p + out C_p + audio 16
    const float *w_up, *b_up;
    WgFlowOps flow[GT_WG_MAX_FLOWS];
    WgLayerOps layer[GT_WG_MAX_FLOWS][GT_WG_MAX_LAYERS];
};
// c_k = G - ES * #{j : 0 < j <= k, j % EE == 0}
int gt_waveglow_flow_channels(int G, int EE, int ES, int k);
// Fills the plan's shapes, tiles and LDS sizes (no device use).  Returns NULL, or the reason, which starts with the field's name.
const char* gt_waveglow_make_plan(int mel_dim, int hop, int win, int G, int F, int EE, int ES, int NL, int C, WgPlan* plan);
// in / cond [taps * cin, 2 C] -> the fragment pack of [taps][cin_p][2 C_p] with the columns in pair order: N-tile 2 j holds the tanh
// half's channels 16 j .. 16 j + 15, N-tile 2 j + 1 the sigmoid half's; gate_bias: b_in + b_cond in that order [2 C_p]
void gt_waveglow_pack_gate(const float* w, int taps, int cin, int C, float* out);
void gt_waveglow_gate_bias(const float* b_in, const float* b_cond, int C, float* out);
// res_skip [C, 2 C] (last: [C, C]) and its bias -> the fragment pack of [C_p][2 C_p] (last: [C_p][C_p]) and the padded bias
void gt_waveglow_pack_rs(const float* w, const float* bias, int C, bool last, float* out, float* bias_out);
hipError_t gt_waveglow_prepare();
hipError_t gt_launch_waveglow_noise(const uint64_t* seeds, float* z, int B, int n, int G, hipStream_t stream);
struct WgCall {
    const float* mel;           // [B, T, mel_dim]
    const int32_t* frames;      // [B] or NULL
    const uint64_t* seeds;      // [B], or
    const float* z;             // [B, T * hop]
    float* wav;                 // [B, ld_wav]
    int32_t* wav_lengths;       // [B] or NULL
    float *spect, *hid[2], *out, *audio;        // the workspace, B * T * hop / G columns each
    int B, T, ld_wav;
    float sigma;
    int only;                   // -1: the whole chain; else that launch alone (timing: gsttaco_waveglow_debug_stage)
};
hipError_t gt_launch_waveglow(const WgPlan& plan, const WgCall& call, hipStream_t stream);


// ---------------------------------------------------------------- hifigan.hip
// The HiFi-GAN generator, mel -> waveform (the contract: gsttaco_hifigan in include/gsttaco.h).
#define GT_HG_MAX_RATES 8
#define GT_HG_MAX_KERNELS 8
#define GT_HG_MAX_DILATIONS 4
#define GT_HG_MAX_TAPS 11
#define GT_HG_MAX_STAGES (2 + GT_HG_MAX_RATES * (1 + GT_HG_MAX_KERNELS * GT_HG_MAX_DILATIONS * 2))
enum { GT_HG_IN = 0, GT_HG_UP = 1, GT_HG_CONV = 2, GT_HG_OUT = 3 };
// The four activation buffers of the workspace: the fused sum (a stage's output, the next stage's input), the transposed conv's output
// (every residual block's input), and the two a block's chain alternates between.
enum { GT_HG_BUF_SUM = 0, GT_HG_BUF_UP = 1, GT_HG_BUF_A = 2, GT_HG_BUF_B = 3, GT_HG_BUFS = 4 };
// What a GT_HG_CONV launch does with its result v (bias + taps, then + residual): GT_HG_SUM_NONE writes v to dst; the last unit of block j
// writes the fused sum instead: sum = v (j = 0) or sum += v, times `scale` = 1 / n_k on the last block.
enum { GT_HG_SUM_NONE = 0, GT_HG_SUM_SET = 1, GT_HG_SUM_ADD = 2 };
// The MFMA's operand form (gsttaco_hifigan_set_operands): fp32 on v_mfma_f32_16x16x4_f32, or the staged tile and the weight pack rounded
// to bf16 / fp16 on v_mfma_f32_16x16x32_{bf16,f16}.  Activations, biases, accumulators and epilogues are fp32 in every form.
enum { GT_HG_OP_F32 = 0, GT_HG_OP_BF16 = 1, GT_HG_OP_F16 = 2 };
// One launch of the chain.  Channel counts with _p are the padded ones (multiples of 16) the fragment packs and the workspace use.
struct HgStage {
    int kind;
    int cin, cout, cin_p, n_p;
    int rate_in, rate_out;      // samples per mel frame of the stage's input and output
    int r;                      // GT_HG_UP: the rate
    int taps, dil;              // GT_HG_CONV: kernel size and dilation (GT_HG_IN / GT_HG_OUT: 7, 1)
    int src, res, dst;          // GT_HG_CONV: buffers read through the LeakyReLU, added raw in the epilogue (-1: none), written (-1: the sum alone)
    int sum;                    // GT_HG_SUM_*
    float scale;                // on the fused sum's last write, 1 / n_k; else 1
    int up, block, unit, conv;  // where the launch sits: stage i, residual block j, unit m, conv 0 / 1 (the manifest's names)
    int tile, form;             // time tile (GT_HG_UP: in input positions, else in output samples); form: N-tiles a wave item owns (GT_HG_OUT: 0)
    size_t lds;                 // dynamic LDS of a workgroup, bytes
    const float *w0, *b0;       // device operands (gsttaco_hifigan_finalize); w0 holds 16-bit words under GT_HG_OP_BF16 / _F16 (not GT_HG_OUT)
};
struct HgConfig {
    int mel_dim, initial, n_rates, rates[GT_HG_MAX_RATES], resblock, n_kernels, kernels[GT_HG_MAX_KERNELS];
    int n_dilations[GT_HG_MAX_KERNELS], dilations[GT_HG_MAX_KERNELS][GT_HG_MAX_DILATIONS];
    float slope, out_slope;
};
struct HgPlan {
    int n_stages;
    HgStage st[GT_HG_MAX_STAGES];
    int mel_dim, hop, min_frames;
    float slope, out_slope;
    size_t ws_floats_per_frame;     // the largest activation of the chain, floats per mel frame of one row
    int operands;                   // GT_HG_OP_*: gt_hifigan_make_plan leaves fp32, gt_hifigan_set_operands changes it
};
// Fills the plan's shapes, tiles and LDS sizes (no device use).  Returns NULL, or the reason the configuration cannot run.
const char* gt_hifigan_make_plan(const HgConfig& cfg, HgPlan* plan);
// The plan's operand form: the launches, tiles and forms stay the fp32 plan's, only every launch's LDS bytes are recomputed for the
// operand size (they shrink: a 16-bit row of round32(cin_p) + 8 elements is never longer than an fp32 row of cin_p + 4).
void gt_hifigan_set_operands(HgPlan* plan, int operands);
// Words of the 16-bit pack of a [taps * cin, cout] kernel: taps * round32(cin) * round16(cout)
size_t gt_hifigan_pack16_words(int taps, int cin, int cout);
// The 16-bit fragment pack [taps][cin_p32 / 32][n_p][4][8], zero padded, each weight rounded to nearest even once (operands: GT_HG_OP_BF16
// or GT_HG_OP_F16): one 16-byte load per lane and 32 k.  Returns -1, or under GT_HG_OP_F16 the index in w of the first weight that is
// not finite after rounding (the pack is then unusable).
int64_t gt_hifigan_pack16(const float* w, int taps, int cin, int cout, int operands, uint16_t* out);
hipError_t gt_hifigan_prepare();
struct HgCall {
    const float* mel;           // [B, T, mel_dim]
    const int32_t* frames;      // [B] or NULL
    float* wav;                 // [B, ld_wav]
    int32_t* wav_lengths;       // [B] or NULL
    float* ws[GT_HG_BUFS];      // B * T * ws_floats_per_frame floats each
    int B, T, ld_wav;
    int only;                   // -1: the whole chain; else that launch alone, on what the workspace holds (timing: gsttaco_hifigan_debug_stage)
};
hipError_t gt_launch_hifigan(const HgPlan& plan, const HgCall& call, hipStream_t stream);
