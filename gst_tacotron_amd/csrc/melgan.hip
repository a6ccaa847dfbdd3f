// The neural vocoder: the MelGAN generator (Kumar et al. 2019, and its public implementation), mel -> waveform
// (gsttaco_melgan: include/gsttaco.h holds the contract).  fp32 storage, v_mfma_f32_16x16x4_f32 with fp32 accumulation.
//
// The network, with mult = 2^len(ratios), x [T, mel_dim], LeakyReLU of slope `slope`:
//   input    reflection-pad 3, Conv1D mel_dim -> mult * base, 7 taps, bias
//   per ratio r (C the channels so far): LeakyReLU; ConvTranspose1D C -> C/2, kernel 2r, stride r, padding r/2, bias (output length
//            exactly r L, two taps per output sample, nothing beyond the input's ends); then n_res residual blocks, block j at
//            dilation d = 3^j:  y = shortcut(x) + conv1(LeakyReLU(conv3_d(reflect_pad_d(LeakyReLU(x))))),  shortcut and conv1 one tap,
//            conv3_d three taps at dilation d, all C/2 -> C/2 with bias
//   output   LeakyReLU, reflection-pad 3, Conv1D base -> 1, 7 taps, bias, tanh
// Row b has frames[b] frames; every reflection and every edge of a transposed conv is taken at the row's own length at that stage.
//
// The activation layout, the fragment pack, the wave items, the tap-GEMM and the three kernels shared with HiFi-GAN are vocoder_common.h's:
//   gt_voc_in_kernel<NT, float, true>    the 7-tap input conv, 3 reflected frames each side
//   gt_voc_up_kernel<NT, float>          the transposed conv as a polyphase GEMM
//   gt_voc_out_kernel<true>              base -> 1 on the VALU with the tanh fused, reflection at the row's ends
// MelGAN's own:
//   gt_mg_res_kernel   ONE launch per residual block: the tile plus a halo of d each side (reflected at the row's ends) staged raw,
//                      LeakyReLU applied on the operand load of the dilated 3-tap GEMM, its LeakyReLU'd result kept in LDS, then the
//                      shortcut GEMM on the raw tile and the 1-tap GEMM on the kept one into one accumulator: five C x C GEMMs per
//                      sample for one read and one write of the activation
// Every output sample has one summation order -- bias, then taps ascending, k ascending in groups of 16 -- that depends on neither the
// batch nor the call's T nor the capacity: a row's samples are bitwise those of the row run alone.  No atomics.  Every global access is
// bounded by the row's length at that stage (<= T * rate), every LDS access by the tile the plan sized; nothing waits on another workgroup.
// A row shorter than the plan's min_frames (a reflection needs the frames it folds back onto) is empty.
#include <algorithm>
#include <math.h>

#include "vocoder_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ the residual block
template <int NT>
__global__ __launch_bounds__(VOC_THREADS) void gt_mg_res_kernel(VocArgs a) {
    extern __shared__ __attribute__((aligned(16))) float mg_lds[];
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, a.min_frames) * a.rate_in, t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int cs = a.cin_p + 4, d = a.dil;
    float* xs = mg_lds;                                     // [tile + 2 d][cs] raw
    float* hs = mg_lds + (size_t)(a.tile + 2 * d) * cs;     // [tile][cs]
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.rate_out * a.n_p;
    voc_stage<float, false, true>(xb, xs, cs, t0 - d, a.tile + 2 * d, len, true, a.ldx, a.cin, a.cin_p, a.slope);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = a.cin_p >> 4, ngroups = (a.n_p >> 4) / NT, items = (a.tile / VOC_ROWS) * ngroups;
    const size_t tap_stride = (size_t)a.cin_p * a.n_p;
    for (int item = wave; item < items; item += VOC_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        voc_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
        for (int tap = 0; tap < 3; ++tap)
            voc_gemm<NT, true>(acc, xs + (mg * VOC_ROWS + tap * d + col) * cs + 4 * g, cs, a.w0 + tap * tap_stride + wl, nkb, a.n_p, a.slope);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    hs[(mg * VOC_ROWS + mt * 16 + g * 4 + i) * cs + n0 + nt * 16 + col] = voc_leaky(acc[mt][nt][i], a.slope);
    }
    __syncthreads();
    for (int item = wave; item < items; item += VOC_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        voc_bias<NT>(acc, a.b1, n0, col);
        const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
        voc_gemm<NT>(acc, xs + (mg * VOC_ROWS + d + col) * cs + 4 * g, cs, a.w1 + wl, nkb, a.n_p);
        voc_gemm<NT>(acc, hs + (mg * VOC_ROWS + col) * cs + 4 * g, cs, a.w2 + wl, nkb, a.n_p);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + mg * VOC_ROWS + mt * 16 + g * 4 + i;
                if (t < len) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)t * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

size_t mg_lds_bytes(const MgStage& s) {
    const size_t cs = (size_t)s.cin_p + 4;
    switch (s.kind) {
    case GT_MG_IN: return (size_t)(s.tile + VOC_TAPS_IO - 1) * cs * sizeof(float);
    case GT_MG_UP: return (size_t)(s.tile + 1) * cs * sizeof(float);
    case GT_MG_RES: return ((size_t)(s.tile + 2 * s.dil) + s.tile) * cs * sizeof(float);
    default: return voc_out_lds(s.cin);
    }
}

template <int NT>
hipError_t mg_launch_form(const MgStage& s, const VocArgs& a, dim3 grid, hipStream_t stream) {
    switch (s.kind) {
    case GT_MG_IN: gt_voc_in_kernel<NT, float, true><<<grid, VOC_THREADS, s.lds, stream>>>(a); break;
    case GT_MG_UP: gt_voc_up_kernel<NT, float><<<grid, VOC_THREADS, s.lds, stream>>>(a); break;
    default: gt_mg_res_kernel<NT><<<grid, VOC_THREADS, s.lds, stream>>>(a); break;
    }
    return hipGetLastError();
}

template <int NT>
hipError_t mg_prepare_form(hipError_t e) {
    e = voc_allow_lds(e, gt_voc_in_kernel<NT, float, true>);
    e = voc_allow_lds(e, gt_voc_up_kernel<NT, float>);
    return voc_allow_lds(e, gt_mg_res_kernel<NT>);
}

}  // namespace

const char* gt_melgan_make_plan(int mel_dim, int base, int n_ratios, const int* ratios, int n_res, float slope, MgPlan* plan) {
    if (mel_dim < 1 || base < 1 || n_res < 1) return "mel_dim, base and n_res must be at least 1";
    if (n_ratios < 1 || n_ratios > GT_MG_MAX_RATIOS) return "between 1 and 8 upsampling ratios";
    if (n_res > GT_MG_MAX_RES) return "at most 8 residual blocks per ratio";
    if (!(slope >= 0.f) || !(slope <= 1.f)) return "the LeakyReLU slope must lie in [0, 1]";
    int64_t hop = 1;
    for (int i = 0; i < n_ratios; ++i) {
        if (ratios[i] < 2 || (ratios[i] & 1))
            return "an upsampling ratio must be even and at least 2 (an odd one needs output_padding, which is not supported)";
        hop *= ratios[i];
        if (hop > 65536) return "the product of the upsampling ratios exceeds 65536";
    }
    if ((int64_t)base << n_ratios > 16384) return "base * 2^len(ratios) exceeds 16384 channels";
    MgPlan& P = *plan;
    P = MgPlan{};
    P.mel_dim = mel_dim; P.hop = (int)hop; P.slope = slope;
    int dmax = 1;
    for (int j = 1; j < n_res; ++j) dmax *= 3;
    P.min_frames = std::max(4, dmax / ratios[0] + 1);
    int C = base << n_ratios, rate = 1, n = 0;
    auto add = [&](int kind, int cin, int cout, int rate_in, int rate_out, int r, int dil) {
        MgStage& s = P.st[n++];
        s.kind = kind; s.cin = cin; s.cout = cout; s.cin_p = voc_pad16(cin); s.n_p = voc_pad16(cout);
        s.rate_in = rate_in; s.rate_out = rate_out; s.r = r; s.dil = dil;
        if (kind == GT_MG_OUT) { s.tile = VOC_OUT_TILE; s.form = 0; }
        else voc_tile_form(s.n_p, &s.tile, &s.form);
        while ((s.lds = mg_lds_bytes(s)) > GT_VOC_LDS_MAX && kind != GT_MG_OUT && s.tile > VOC_ROWS) s.tile >>= 1;
        if (kind != GT_MG_OUT) P.ws_floats_per_frame = std::max(P.ws_floats_per_frame, (size_t)rate_out * s.n_p);
        return s.lds <= GT_VOC_LDS_MAX;
    };
    static const char* lds_msg = "a stage's tile does not fit the 160 KB of LDS (fewer channels, or fewer residual blocks: the halo is 3^(n_res-1))";
    if (!add(GT_MG_IN, mel_dim, C, 1, 1, 0, 0)) return lds_msg;
    for (int i = 0; i < n_ratios; ++i) {
        if (!add(GT_MG_UP, C, C / 2, rate, rate * ratios[i], ratios[i], 0)) return lds_msg;
        C /= 2; rate *= ratios[i];
        for (int j = 0, d = 1; j < n_res; ++j, d *= 3)
            if (!add(GT_MG_RES, C, C, rate, rate, 0, d)) return lds_msg;
    }
    if (!add(GT_MG_OUT, C, 1, rate, rate, 0, 0)) return lds_msg;
    P.n_stages = n;
    return nullptr;
}

hipError_t gt_melgan_prepare() {
    hipError_t e = voc_allow_lds(hipSuccess, gt_voc_out_kernel<true>);
    e = mg_prepare_form<1>(e); e = mg_prepare_form<2>(e); e = mg_prepare_form<4>(e);
    return e;
}

hipError_t gt_launch_melgan(const MgPlan& P, const MgCall& c, hipStream_t stream) {
    int cur = 0;
    for (int i = 0; i < P.n_stages; ++i) {
        const MgStage& s = P.st[i];
        VocArgs a{};
        a.frames = c.frames; a.wav_lengths = c.wav_lengths;
        a.w0 = s.w0; a.b0 = s.b0; a.w1 = s.w1; a.w2 = s.w2; a.b1 = s.b1;
        a.T = c.T; a.cin = s.cin; a.cin_p = s.cin_p; a.n_p = s.n_p; a.rate_in = s.rate_in; a.rate_out = s.rate_out;
        a.r = s.r; a.dil = s.dil; a.tile = s.tile; a.min_frames = P.min_frames; a.ld_wav = c.ld_wav; a.slope = P.slope;
        dim3 grid(1, c.B);
        if (s.kind == GT_MG_IN) {
            a.x = c.mel; a.ldx = P.mel_dim; a.y = c.ws[cur];
            grid.x = (c.T + s.tile - 1) / s.tile;
        } else {
            a.x = c.ws[cur]; a.ldx = s.cin_p;
            if (s.kind == GT_MG_OUT) {
                a.y = c.wav;
                grid.x = (c.ld_wav + VOC_OUT_TILE - 1) / VOC_OUT_TILE;
            } else {
                a.y = c.ws[cur ^ 1];
                cur ^= 1;
                const int64_t L = (int64_t)c.T * (s.kind == GT_MG_UP ? s.rate_in : s.rate_out) + (s.kind == GT_MG_UP ? 1 : 0);
                grid.x = (unsigned)((L + s.tile - 1) / s.tile);
            }
        }
        if (c.only >= 0 && c.only != i) continue;
        hipError_t e;
        if (s.kind == GT_MG_OUT) {
            gt_voc_out_kernel<true><<<grid, VOC_OUT_TILE, s.lds, stream>>>(a);
            e = hipGetLastError();
        } else {
            e = s.form == 4 ? mg_launch_form<4>(s, a, grid, stream) : s.form == 2 ? mg_launch_form<2>(s, a, grid, stream)
                                                                                  : mg_launch_form<1>(s, a, grid, stream);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
