// The HiFi-GAN vocoder: the generator of Kong, Kim & Bae 2020 and its public implementation (V1 / V2 / V3 and anything of their shape),
// mel -> waveform (gsttaco_hifigan: include/gsttaco.h holds the contract).  fp32 storage, v_mfma_f32_16x16x4_f32 with fp32 accumulation.
//
// The network, x [T, mel_dim], L(.) = LeakyReLU of slope `slope`:
//   input    Conv1D mel_dim -> C0, 7 taps, zero padding 3, bias
//   per rate u (C the channels so far): L; ConvTranspose1D C -> C/2, kernel 2u, stride u, padding u/2, bias (output length exactly u len,
//            two taps per output sample, nothing beyond the input's ends); then the fusion y = (1 / n_k) sum_j ResBlock_j(x) over n_k
//            residual blocks of kernel size k_j and dilations D_j:
//              resblock 1, for d in D_j:  x = x + conv_{k_j,1}(L(conv_{k_j,d}(L(x))))
//              resblock 2, for d in D_j:  x = x + conv_{k_j,d}(L(x))
//            every conv C/2 -> C/2 with bias and zero padding (k - 1) / 2 * d
//   output   LeakyReLU of slope `out_slope`, Conv1D C_last -> 1, 7 taps, zero padding 3, bias, tanh
// Row b has frames[b] frames; every zero pad and every edge of a transposed conv is taken at the row's own length at that stage.
//
// The activation layout, the fragment packs, the wave items, the tap-GEMMs and the three kernels shared with MelGAN are
// vocoder_common.h's (the padding channels stay exact zeros here too: LeakyReLU(0) = 0, 0 + 0 = 0):
//   gt_voc_in_kernel<NT, OP, false>      the 7-tap input conv, zeros outside the row
//   gt_voc_up_kernel<NT, OP>             the transposed conv as a polyphase GEMM
//   gt_voc_out_kernel<false>             C_last -> 1 on the VALU with the tanh fused, LeakyReLU of `out_slope`
// HiFi-GAN's own:
//   gt_hg_conv_kernel  ONE launch per residual conv, at every width: the tile plus a halo of (k - 1) / 2 * d each side staged through the
//                      LeakyReLU (zeros outside the row), k dilated tap-GEMMs into one accumulator, and an epilogue that adds the raw
//                      residual and either writes the activation or, on the last unit of block j, the fused sum (sum = y for j = 0,
//                      sum += y else, times 1 / n_k on the last block).  The sum's read-modify-write is done by the element's owner and
//                      ordered by the stream: one order, no atomics.  (A fused pair would keep the intermediate in LDS, but at 256
//                      channels, k = 11, d = 5 the two tiles need 206 KB; one form for every width was chosen -- DESIGN 3.5.)
// Every output sample has one summation order -- bias, then taps ascending, k ascending in groups of 16, then the residual, then the fused sum in block
// order -- that depends on neither the batch nor the call's T nor the capacity: a row's samples are bitwise those of the row run alone.
// Every global access is bounded by the row's length at that stage (<= T * rate), every LDS access by the tile the plan sized; nothing
// waits on another workgroup.
//
// The 16-bit operand forms (gsttaco_hifigan_set_operands; GT_HG_OP_BF16 / GT_HG_OP_F16) run the same three GEMM kernels on
// v_mfma_f32_16x16x32_{bf16,f16}: one template over the operand type (the lane maps: vocoder_common.h).  HBM is untouched: activations
// stay fp32 at C_p = round16(C).  The staging (voc_stage; hg_stage below for the conv kernel) applies its bounds and the LeakyReLU in fp32,
// then rounds to nearest even once (fp16 saturating to +-65504) into a 16-bit LDS tile whose rows are padded with exact zeros to a
// multiple of 32 k, plus 8 elements: the row stride is then an odd number of 16-byte slots, and the 16 rows of a ds_read_b128 lane group
// (8 at one k quarter, 8 at the next) fall on 16-byte slots at worst 2-way.  The weights are rounded once on the host (gt_hifigan_pack16)
// into [tap][k / 32][n][q = (k % 32) / 8][j = k % 8]: one 16-byte load per lane and 32 k.  k advances in blocks of 32; a sample's order
// is bias, taps ascending, k ascending in blocks of 32 (inside a block the MFMA's own), the residual, the fused sum -- still independent
// of batch, T and capacity.  The output conv stays fp32 on the VALU in every form.
#include <algorithm>
#include <string.h>
#include <math.h>

#include "vocoder_common.h"

namespace {

// gt_hg_conv_kernel's own staging: voc_stage<OP, true, false> at vec = true, with the arguments as a struct.  Positions [p0, p0 + rows)
// of one row's input into xs[rows][cs] through the LeakyReLU, zeros outside [0, len) and in channels >= cin_p, rounded once to OP.  It is
// kept apart because with the shared voc_stage the compiler biased the K loop's weight pointer by 0x800 and the 128-channel float32
// launches ran 3.2 % slower ("shared core"); with this form the kernel's text is the one it had before the fold.
template <typename OP>
__device__ __forceinline__ void hg_stage(const VocArgs& a, const float* xb, OP* xs, int cs, int p0, int rows, int len) {
    const int ck = voc_kpad<OP>(a.cin_p), c4n = ck >> 2;
    for (int e = threadIdx.x; e < rows * c4n; e += VOC_THREADS) {
        const int i = e / c4n, c = (e - i * c4n) << 2;
        const int p = p0 + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p >= 0 && p < len && c < a.cin_p) v = *reinterpret_cast<const float4*>(xb + (size_t)p * a.ldx + c);
        v.x = voc_leaky(v.x, a.slope); v.y = voc_leaky(v.y, a.slope); v.z = voc_leaky(v.z, a.slope); v.w = voc_leaky(v.w, a.slope);
        voc_store4(xs + i * cs + c, v);
    }
}

// ------------------------------------------------------------------------------------------------ one residual conv
template <int NT, typename OP>
__global__ __launch_bounds__(VOC_THREADS) void gt_hg_conv_kernel(VocArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds_raw[];
    OP* hg_lds = reinterpret_cast<OP*>(hg_lds_raw);
    constexpr int KB = VocOp<OP>::K, Q = VocOp<OP>::Q;
    const OP* w0 = reinterpret_cast<const OP*>(a.w0);
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, 1) * a.rate_in, t0 = blockIdx.x * a.tile;      // (min_frames is 1: zero padding)
    if (t0 >= len) return;
    const int ck = voc_kpad<OP>(a.cin_p), cs = ck + VocOp<OP>::PAD, d = a.dil, halo = (a.taps >> 1) * d;
    const size_t row0 = (size_t)b * a.T * a.rate_in * a.n_p;            // cin_p == n_p: every buffer of the stage has this shape
    hg_stage<OP>(a, a.x + row0, hg_lds, cs, t0 - halo, a.tile + 2 * halo, len);
    __syncthreads();
    const float* rb = a.res ? a.res + row0 : nullptr;
    float* yb = a.y ? a.y + row0 : nullptr;
    float* sb = a.sum + row0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = ck / KB, ngroups = (a.n_p >> 4) / NT, items = (a.tile / VOC_ROWS) * ngroups;
    const size_t tap_stride = (size_t)ck * a.n_p;
    for (int item = wave; item < items; item += VOC_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        voc_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * KB + Q * g;
        for (int tap = 0; tap < a.taps; ++tap)
            voc_gemm<NT>(acc, hg_lds + (mg * VOC_ROWS + tap * d + col) * cs + Q * g, cs, w0 + tap * tap_stride + wl, nkb, a.n_p);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + mg * VOC_ROWS + mt * 16 + g * 4 + i;
                if (t < len) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const size_t idx = (size_t)t * a.n_p + n0 + nt * 16 + col;
                        float v = acc[mt][nt][i];
                        if (rb) v += rb[idx];
                        if (a.sum_mode == GT_HG_SUM_NONE) yb[idx] = v;
                        else {
                            if (a.sum_mode == GT_HG_SUM_ADD) v = sb[idx] + v;
                            sb[idx] = v * a.scale;
                        }
                    }
                }
            }
    }
}

// op_bytes: the size of an MFMA operand, 4 (fp32: rows of cin_p + 4) or 2 (16-bit: rows of round32(cin_p) + 8); the output conv is fp32 always
size_t hg_lds_bytes(const HgStage& s, size_t op_bytes) {
    const size_t cs = op_bytes == 4 ? (size_t)s.cin_p + VocOp<float>::PAD : (size_t)voc_kpad<__bf16>(s.cin_p) + VocOp<__bf16>::PAD;
    switch (s.kind) {
    case GT_HG_IN: return (size_t)(s.tile + VOC_TAPS_IO - 1) * cs * op_bytes;
    case GT_HG_UP: return (size_t)(s.tile + 1) * cs * op_bytes;
    case GT_HG_CONV: return ((size_t)s.tile + (size_t)(s.taps - 1) * s.dil) * cs * op_bytes;
    default: return voc_out_lds(s.cin);
    }
}

template <int NT, typename OP>
hipError_t hg_launch_form(const HgStage& s, const VocArgs& a, dim3 grid, hipStream_t stream) {
    switch (s.kind) {
    case GT_HG_IN: gt_voc_in_kernel<NT, OP, false><<<grid, VOC_THREADS, s.lds, stream>>>(a); break;
    case GT_HG_UP: gt_voc_up_kernel<NT, OP><<<grid, VOC_THREADS, s.lds, stream>>>(a); break;
    default: gt_hg_conv_kernel<NT, OP><<<grid, VOC_THREADS, s.lds, stream>>>(a); break;
    }
    return hipGetLastError();
}

template <typename OP>
hipError_t hg_launch_op(const HgStage& s, const VocArgs& a, dim3 grid, hipStream_t stream) {
    return s.form == 4 ? hg_launch_form<4, OP>(s, a, grid, stream) : s.form == 2 ? hg_launch_form<2, OP>(s, a, grid, stream)
                                                                                 : hg_launch_form<1, OP>(s, a, grid, stream);
}

template <int NT, typename OP>
hipError_t hg_prepare_form(hipError_t e) {
    e = voc_allow_lds(e, gt_voc_in_kernel<NT, OP, false>);
    e = voc_allow_lds(e, gt_voc_up_kernel<NT, OP>);
    return voc_allow_lds(e, gt_hg_conv_kernel<NT, OP>);
}

template <typename OP>
hipError_t hg_prepare_op(hipError_t e) { return hg_prepare_form<4, OP>(hg_prepare_form<2, OP>(hg_prepare_form<1, OP>(e))); }

// fp32 -> bf16 / fp16 bits, to nearest even, as the device's conversion does it
uint16_t hg_bf16_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);       // NaN stays a (quiet) NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
uint16_t hg_f16_bits(float v) {
    const _Float16 h = (_Float16)v;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

}  // namespace

const char* gt_hifigan_make_plan(const HgConfig& cfg, HgPlan* plan) {
    if (cfg.mel_dim < 1) return "mel_dim must be at least 1";
    if (cfg.initial < 1) return "initial must be at least 1";
    if (cfg.n_rates < 1 || cfg.n_rates > GT_HG_MAX_RATES) return "n_rates: between 1 and 8 upsampling rates";
    if (cfg.resblock != 1 && cfg.resblock != 2) return "resblock must be 1 or 2";
    if (cfg.n_kernels < 1 || cfg.n_kernels > GT_HG_MAX_KERNELS) return "n_kernels: between 1 and 8 residual kernels";
    if (!(cfg.slope >= 0.f) || !(cfg.slope <= 1.f)) return "slope must lie in [0, 1]";
    if (!(cfg.out_slope >= 0.f) || !(cfg.out_slope <= 1.f)) return "out_slope must lie in [0, 1]";
    int64_t hop = 1;
    for (int i = 0; i < cfg.n_rates; ++i) {
        if (cfg.rates[i] < 2 || (cfg.rates[i] & 1))
            return "rates: an upsampling rate must be even and at least 2 (an odd one needs output_padding, which is not supported)";
        hop *= cfg.rates[i];
        if (hop > 65536) return "rates: the product of the upsampling rates exceeds 65536";
    }
    if (cfg.initial > 16384) return "initial exceeds 16384 channels";
    if (cfg.initial % (1 << cfg.n_rates)) return "initial must be a multiple of 2^n_rates (every stage halves the channels)";
    for (int j = 0; j < cfg.n_kernels; ++j) {
        if (cfg.kernels[j] < 1 || cfg.kernels[j] > GT_HG_MAX_TAPS || !(cfg.kernels[j] & 1)) return "kernels: a residual kernel size must be odd and at most 11";
        if (cfg.n_dilations[j] < 1 || cfg.n_dilations[j] > GT_HG_MAX_DILATIONS) return "n_dilations: between 1 and 4 dilations per residual kernel";
        for (int m = 0; m < cfg.n_dilations[j]; ++m)
            if (cfg.dilations[j][m] < 1 || cfg.dilations[j][m] > 4096) return "dilations: a dilation must lie in [1, 4096]";
    }
    HgPlan& P = *plan;
    P = HgPlan{};
    // (min_frames must stay 1: the shared in / up / out kernels read it from the plan, gt_hg_conv_kernel has it as a literal)
    P.mel_dim = cfg.mel_dim; P.hop = (int)hop; P.slope = cfg.slope; P.out_slope = cfg.out_slope; P.min_frames = 1;
    int C = cfg.initial, rate = 1, n = 0;
    auto add = [&](int kind, int cin, int cout, int rate_in, int rate_out, int r, int taps, int dil) -> HgStage* {
        HgStage& s = P.st[n++];
        s.kind = kind; s.cin = cin; s.cout = cout; s.cin_p = voc_pad16(cin); s.n_p = voc_pad16(cout);
        s.rate_in = rate_in; s.rate_out = rate_out; s.r = r; s.taps = taps; s.dil = dil;
        s.src = s.res = s.dst = -1; s.sum = GT_HG_SUM_NONE; s.scale = 1.f; s.up = s.block = s.unit = s.conv = -1;
        if (kind == GT_HG_OUT) { s.tile = VOC_OUT_TILE; s.form = 0; }
        else voc_tile_form(s.n_p, &s.tile, &s.form);
        while ((s.lds = hg_lds_bytes(s, sizeof(float))) > GT_VOC_LDS_MAX && kind != GT_HG_OUT && s.tile > VOC_ROWS) s.tile >>= 1;
        if (kind != GT_HG_OUT) P.ws_floats_per_frame = std::max(P.ws_floats_per_frame, (size_t)rate_out * s.n_p);
        return s.lds <= GT_VOC_LDS_MAX ? &s : nullptr;
    };
    static const char* lds_msg = "a launch's smallest tile does not fit the 160 KB of LDS (initial: fewer channels, or dilations: a narrower halo)";
    if (!add(GT_HG_IN, cfg.mel_dim, C, 1, 1, 0, VOC_TAPS_IO, 1)) return lds_msg;
    for (int i = 0; i < cfg.n_rates; ++i) {
        HgStage* u = add(GT_HG_UP, C, C / 2, rate, rate * cfg.rates[i], cfg.rates[i], 2 * cfg.rates[i], 1);
        if (!u) return lds_msg;
        u->up = i;
        C /= 2; rate *= cfg.rates[i];
        for (int j = 0; j < cfg.n_kernels; ++j) {
            const int k = cfg.kernels[j], nd = cfg.n_dilations[j], last_sum = j == 0 ? GT_HG_SUM_SET : GT_HG_SUM_ADD;
            const float scale = j == cfg.n_kernels - 1 ? 1.f / (float)cfg.n_kernels : 1.f;
            int x = GT_HG_BUF_UP;                           // the buffer that holds the block's running x
            for (int m = 0; m < nd; ++m) {
                const bool last = m == nd - 1;
                const int dil = cfg.dilations[j][m];
                if (cfg.resblock == 1) {
                    // h = conv_{k,d}(L(x)) into A; x = x + conv_{k,1}(L(h)) into B -- in place from the second unit on: the conv reads A,
                    // and an element of B is read and written by its owner alone
                    HgStage* s = add(GT_HG_CONV, C, C, rate, rate, 0, k, dil);
                    if (!s) return lds_msg;
                    s->src = x; s->dst = GT_HG_BUF_A; s->up = i; s->block = j; s->unit = m; s->conv = 0;
                    s = add(GT_HG_CONV, C, C, rate, rate, 0, k, 1);
                    if (!s) return lds_msg;
                    s->src = GT_HG_BUF_A; s->res = x; s->up = i; s->block = j; s->unit = m; s->conv = 1;
                    if (last) { s->sum = last_sum; s->scale = scale; }
                    else { s->dst = GT_HG_BUF_B; x = GT_HG_BUF_B; }
                } else {
                    // x = x + conv_{k,d}(L(x)): other workgroups read x's halo, so the units alternate between A and B
                    HgStage* s = add(GT_HG_CONV, C, C, rate, rate, 0, k, dil);
                    if (!s) return lds_msg;
                    s->src = x; s->res = x; s->up = i; s->block = j; s->unit = m; s->conv = 0;
                    if (last) { s->sum = last_sum; s->scale = scale; }
                    else { s->dst = x == GT_HG_BUF_A ? GT_HG_BUF_B : GT_HG_BUF_A; x = s->dst; }
                }
            }
        }
    }
    if (!add(GT_HG_OUT, C, 1, rate, rate, 0, VOC_TAPS_IO, 1)) return lds_msg;
    P.n_stages = n;
    return nullptr;
}

void gt_hifigan_set_operands(HgPlan* plan, int operands) {
    plan->operands = operands;
    for (int i = 0; i < plan->n_stages; ++i) plan->st[i].lds = hg_lds_bytes(plan->st[i], operands == GT_HG_OP_F32 ? 4 : 2);
}

size_t gt_hifigan_pack16_words(int taps, int cin, int cout) { return (size_t)taps * voc_kpad<__bf16>(voc_pad16(cin)) * voc_pad16(cout); }

int64_t gt_hifigan_pack16(const float* w, int taps, int cin, int cout, int operands, uint16_t* out) {
    const int ck = voc_kpad<__bf16>(voc_pad16(cin)), n_p = voc_pad16(cout);
    std::fill(out, out + (size_t)taps * ck * n_p, (uint16_t)0);
    int64_t bad = -1;
    for (int tap = 0; tap < taps; ++tap)
        for (int k = 0; k < cin; ++k)
            for (int nn = 0; nn < cout; ++nn) {
                const size_t src = ((size_t)tap * cin + k) * cout + nn;
                uint16_t bits;
                if (operands == GT_HG_OP_F16) {
                    bits = hg_f16_bits(w[src]);
                    if ((bits & 0x7c00u) == 0x7c00u && bad < 0) bad = (int64_t)src;     // inf or NaN after rounding
                } else bits = hg_bf16_bits(w[src]);
                out[(size_t)tap * ck * n_p + ((size_t)(k >> 5) * n_p + nn) * 32 + (k & 31)] = bits;
            }
    return bad;
}

hipError_t gt_hifigan_prepare() {
    hipError_t e = voc_allow_lds(hipSuccess, gt_voc_out_kernel<false>);
    e = hg_prepare_op<float>(e); e = hg_prepare_op<__bf16>(e); e = hg_prepare_op<_Float16>(e);
    return e;
}

hipError_t gt_launch_hifigan(const HgPlan& P, const HgCall& c, hipStream_t stream) {
    for (int i = 0; i < P.n_stages; ++i) {
        if (c.only >= 0 && c.only != i) continue;
        const HgStage& s = P.st[i];
        VocArgs a{};
        a.frames = c.frames; a.wav_lengths = c.wav_lengths;
        a.w0 = s.w0; a.b0 = s.b0;
        a.T = c.T; a.cin = s.cin; a.cin_p = s.cin_p; a.n_p = s.n_p; a.rate_in = s.rate_in; a.rate_out = s.rate_out;
        a.r = s.r; a.taps = s.taps; a.dil = s.dil; a.tile = s.tile; a.min_frames = P.min_frames; a.ld_wav = c.ld_wav; a.sum_mode = s.sum;
        a.slope = s.kind == GT_HG_OUT ? P.out_slope : P.slope; a.scale = s.scale;
        a.sum = c.ws[GT_HG_BUF_SUM];
        dim3 grid(1, c.B);
        if (s.kind == GT_HG_IN) {
            a.x = c.mel; a.ldx = P.mel_dim; a.y = c.ws[GT_HG_BUF_SUM];
            grid.x = (c.T + s.tile - 1) / s.tile;
        } else if (s.kind == GT_HG_UP) {
            a.x = c.ws[GT_HG_BUF_SUM]; a.ldx = s.cin_p; a.y = c.ws[GT_HG_BUF_UP];
            grid.x = (unsigned)(((int64_t)c.T * s.rate_in + 1 + s.tile - 1) / s.tile);
        } else if (s.kind == GT_HG_CONV) {
            a.x = c.ws[s.src]; a.ldx = s.cin_p;
            a.res = s.res >= 0 ? c.ws[s.res] : nullptr;
            a.y = s.dst >= 0 ? c.ws[s.dst] : nullptr;
            grid.x = (unsigned)(((int64_t)c.T * s.rate_out + s.tile - 1) / s.tile);
        } else {
            a.x = c.ws[GT_HG_BUF_SUM]; a.ldx = s.cin_p; a.y = c.wav;
            grid.x = (c.ld_wav + VOC_OUT_TILE - 1) / VOC_OUT_TILE;
        }
        hipError_t e;
        if (s.kind == GT_HG_OUT) {
            gt_voc_out_kernel<false><<<grid, VOC_OUT_TILE, s.lds, stream>>>(a);
            e = hipGetLastError();
        } else {
            e = P.operands == GT_HG_OP_BF16 ? hg_launch_op<__bf16>(s, a, grid, stream)
              : P.operands == GT_HG_OP_F16 ? hg_launch_op<_Float16>(s, a, grid, stream) : hg_launch_op<float>(s, a, grid, stream);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
