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
// Activations are time-major [B, L, C_p], C_p = C rounded up to 16; the padding channels are exact zeros everywhere (zero weights, zero
// bias, LeakyReLU(0) = 0), so any channel count runs the same kernels.  Weights are repacked on the host (gt_melgan_pack) into the
// order the B operand is read in: [tap][k / 16][n][g = (k % 16) / 4][j = k % 4], one coalesced 16-byte load per lane and 16 k.
//
//   gt_mg_in_kernel    the 7-tap input conv: the mel tile plus 3 reflected frames each side staged in LDS, 7 GEMMs of K = mel_dim
//   gt_mg_up_kernel    the transposed conv as a polyphase GEMM: output phase p of input position q takes taps p and p + r of positions
//                      q and q - 1 (K = 2 C, no zero stuffing), LeakyReLU applied while staging; a workgroup owns a tile of q and
//                      walks the r phases
//   gt_mg_res_kernel   ONE launch per residual block: the tile plus a halo of d each side (reflected at the row's ends) staged raw,
//                      LeakyReLU applied on the operand load of the dilated 3-tap GEMM, its LeakyReLU'd result kept in LDS, then the
//                      shortcut GEMM on the raw tile and the 1-tap GEMM on the kept one into one accumulator: five C x C GEMMs per
//                      sample for one read and one write of the activation
//   gt_mg_out_kernel   base -> 1: a 7 * base term dot product per sample on the VALU with the tanh fused; zeros beyond the row's length
// A wave owns items of 64 time rows x NT N-tiles (the plan's `form`, by channel count); 256 threads a workgroup.  Every output sample
// has one summation order -- bias, then taps ascending, k ascending in groups of 16 -- that depends on neither the batch nor the
// call's T nor the capacity: a row's samples are bitwise those of the row run alone.  No atomics.  Every global access is bounded by
// the row's length at that stage (<= T * rate), every LDS access by the tile the plan sized; nothing waits on another workgroup.
#include <algorithm>
#include <math.h>

#include "kernels.h"
#include "device_utils.h"

#define MG_THREADS 256
#define MG_WAVES (MG_THREADS / GT_WAVE)
#define MG_ROWS 64              // time rows of a wave item: four M-tiles
#define MG_OUT_TILE 256
#define MG_TAPS_IO 7

namespace {

struct MgArgs {
    const float* x;
    float* y;
    const int32_t* frames;
    int32_t* wav_lengths;
    const float *w0, *b0, *w1, *w2, *b1;
    int T, ldx, cin, cin_p, n_p, rate_in, rate_out, r, dil, tile, min_frames, ld_wav;
    float slope;
};

__device__ __forceinline__ int mg_row_frames(const MgArgs& a, int b) {
    int f = a.frames ? a.frames[b] : a.T;
    f = f < a.T ? f : a.T;
    return f < a.min_frames ? 0 : f;
}

__device__ __forceinline__ float mg_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// Positions [p0, p0 + rows) of one row's input (len valid positions, row stride ldx) into xs[rows][cs], channels [0, cin_p).  A position
// outside [0, len) is folded back once when REFLECT; what is still outside, and every channel >= cin, is 0.
template <bool LEAKY, bool REFLECT>
__device__ __forceinline__ void mg_stage(const MgArgs& a, const float* xb, float* xs, int cs, int p0, int rows, int len, bool vec) {
    if (vec) {
        const int c4n = a.cin_p >> 2;
        for (int e = threadIdx.x; e < rows * c4n; e += MG_THREADS) {
            const int i = e / c4n, c = (e - i * c4n) << 2;
            int p = p0 + i;
            if (REFLECT) p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p >= 0 && p < len) v = *reinterpret_cast<const float4*>(xb + (size_t)p * a.ldx + c);
            if (LEAKY) { v.x = mg_leaky(v.x, a.slope); v.y = mg_leaky(v.y, a.slope); v.z = mg_leaky(v.z, a.slope); v.w = mg_leaky(v.w, a.slope); }
            *reinterpret_cast<float4*>(xs + i * cs + c) = v;
        }
    } else {
        for (int e = threadIdx.x; e < rows * a.cin_p; e += MG_THREADS) {
            const int i = e / a.cin_p, c = e - i * a.cin_p;
            int p = p0 + i;
            if (REFLECT) p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
            float v = 0.f;
            if (p >= 0 && p < len && c < a.cin) v = xb[(size_t)p * a.ldx + c];
            xs[i * cs + c] = LEAKY ? mg_leaky(v, a.slope) : v;
        }
    }
}

// acc[mt][nt] += A[64 rows, 16 nkb] * W[16 nkb, 16 NT]: A from LDS (a_lane: this lane's row l & 15 of M-tile 0, k offset 4 (l >> 4)),
// W from the fragment pack (w_lane: this lane's column and k group of N-tile 0).  k ascending in groups of 16; inside a group MFMA j
// takes k = 4 g + j of the four lane groups g.
template <int NT, bool LEAKY>
__device__ __forceinline__ void mg_gemm(f32x4 (&acc)[4][NT], const float* a_lane, int cs, const float* w_lane, int nkb, int n_p, float slope) {
    for (int kb = 0; kb < nkb; ++kb) {
        float av[4][4], bv[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float4 t = *reinterpret_cast<const float4*>(w_lane + ((size_t)kb * n_p + nt * 16) * 16);
            bv[nt][0] = t.x; bv[nt][1] = t.y; bv[nt][2] = t.z; bv[nt][3] = t.w;
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4 t = *reinterpret_cast<const float4*>(a_lane + mt * 16 * cs + kb * 16);
            av[mt][0] = t.x; av[mt][1] = t.y; av[mt][2] = t.z; av[mt][3] = t.w;
            if (LEAKY) {
#pragma unroll
                for (int j = 0; j < 4; ++j) av[mt][j] = mg_leaky(av[mt][j], slope);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][j], bv[nt][j], acc[mt][nt], 0, 0, 0);
    }
}

template <int NT>
__device__ __forceinline__ void mg_bias(f32x4 (&acc)[4][NT], const float* bias, int n0, int col) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float b = bias[n0 + nt * 16 + col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = f32x4{b, b, b, b};
    }
}

// ------------------------------------------------------------------------------------------------ the input conv
template <int NT>
__global__ __launch_bounds__(MG_THREADS) void gt_mg_in_kernel(MgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float mg_lds[];
    const int b = blockIdx.y, len = mg_row_frames(a, b), t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int cs = a.cin_p + 4, pad = MG_TAPS_IO / 2;
    const float* xb = a.x + (size_t)b * a.T * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.n_p;
    mg_stage<false, true>(a, xb, mg_lds, cs, t0 - pad, a.tile + 2 * pad, len, false);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = a.cin_p >> 4, ngroups = (a.n_p >> 4) / NT, items = (a.tile / MG_ROWS) * ngroups;
    for (int item = wave; item < items; item += MG_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        mg_bias<NT>(acc, a.b0, n0, col);
        for (int tap = 0; tap < MG_TAPS_IO; ++tap)
            mg_gemm<NT, false>(acc, mg_lds + (mg * MG_ROWS + tap + col) * cs + 4 * g, cs,
                               a.w0 + (size_t)tap * a.cin_p * a.n_p + (size_t)(n0 + col) * 16 + 4 * g, nkb, a.n_p, a.slope);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + mg * MG_ROWS + mt * 16 + g * 4 + i;
                if (t < len) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)t * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ the transposed conv
template <int NT>
__global__ __launch_bounds__(MG_THREADS) void gt_mg_up_kernel(MgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float mg_lds[];
    const int b = blockIdx.y, len = mg_row_frames(a, b) * a.rate_in, q0 = blockIdx.x * a.tile;
    if (len == 0 || q0 > len) return;                       // q runs over [0, len]: position len still feeds the last r / 2 samples
    const int cs = a.cin_p + 4;
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.rate_out * a.n_p;
    mg_stage<true, false>(a, xb, mg_lds, cs, q0 - 1, a.tile + 1, len, true);      // xs[i] = LeakyReLU(x[q0 - 1 + i]), 0 where absent
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = a.cin_p >> 4, ngroups = (a.n_p >> 4) / NT, per_phase = (a.tile / MG_ROWS) * ngroups, items = per_phase * a.r;
    const int len_out = len * a.r, half = a.r >> 1;
    const size_t tap_stride = (size_t)a.cin_p * a.n_p;
    for (int item = wave; item < items; item += MG_WAVES) {
        const int p = item / per_phase, rest = item - p * per_phase, mg = rest / ngroups, n0 = (rest - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        mg_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
        mg_gemm<NT, false>(acc, mg_lds + (mg * MG_ROWS + 1 + col) * cs + 4 * g, cs, a.w0 + p * tap_stride + wl, nkb, a.n_p, a.slope);
        mg_gemm<NT, false>(acc, mg_lds + (mg * MG_ROWS + col) * cs + 4 * g, cs, a.w0 + (p + a.r) * tap_stride + wl, nkb, a.n_p, a.slope);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = q0 + mg * MG_ROWS + mt * 16 + g * 4 + i;
                const int o = q * a.r + p - half;
                if (q <= len && o >= 0 && o < len_out) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)o * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ the residual block
template <int NT>
__global__ __launch_bounds__(MG_THREADS) void gt_mg_res_kernel(MgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float mg_lds[];
    const int b = blockIdx.y, len = mg_row_frames(a, b) * a.rate_in, t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int cs = a.cin_p + 4, d = a.dil;
    float* xs = mg_lds;                                     // [tile + 2 d][cs] raw
    float* hs = mg_lds + (size_t)(a.tile + 2 * d) * cs;     // [tile][cs]
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.rate_out * a.n_p;
    mg_stage<false, true>(a, xb, xs, cs, t0 - d, a.tile + 2 * d, len, true);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = a.cin_p >> 4, ngroups = (a.n_p >> 4) / NT, items = (a.tile / MG_ROWS) * ngroups;
    const size_t tap_stride = (size_t)a.cin_p * a.n_p;
    for (int item = wave; item < items; item += MG_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        mg_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
        for (int tap = 0; tap < 3; ++tap)
            mg_gemm<NT, true>(acc, xs + (mg * MG_ROWS + tap * d + col) * cs + 4 * g, cs, a.w0 + tap * tap_stride + wl, nkb, a.n_p, a.slope);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    hs[(mg * MG_ROWS + mt * 16 + g * 4 + i) * cs + n0 + nt * 16 + col] = mg_leaky(acc[mt][nt][i], a.slope);
    }
    __syncthreads();
    for (int item = wave; item < items; item += MG_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        mg_bias<NT>(acc, a.b1, n0, col);
        const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
        mg_gemm<NT, false>(acc, xs + (mg * MG_ROWS + d + col) * cs + 4 * g, cs, a.w1 + wl, nkb, a.n_p, a.slope);
        mg_gemm<NT, false>(acc, hs + (mg * MG_ROWS + col) * cs + 4 * g, cs, a.w2 + wl, nkb, a.n_p, a.slope);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + mg * MG_ROWS + mt * 16 + g * 4 + i;
                if (t < len) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)t * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ the output conv
__global__ __launch_bounds__(MG_OUT_TILE) void gt_mg_out_kernel(MgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float mg_lds[];
    const int b = blockIdx.y, len = mg_row_frames(a, b) * a.rate_in, t0 = blockIdx.x * MG_OUT_TILE, t = t0 + (int)threadIdx.x;
    float* wb = a.y + (size_t)b * a.ld_wav;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.wav_lengths) a.wav_lengths[b] = len;
    if (t0 >= len) {
        if (t < a.ld_wav) wb[t] = 0.f;
        return;
    }
    const int cs = a.cin | 1, pad = MG_TAPS_IO / 2, rows = MG_OUT_TILE + 2 * pad;
    float* xs = mg_lds;                                     // [rows][cs], LeakyReLU applied
    float* ws = mg_lds + rows * cs;                         // [7 * cin]
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    for (int e = threadIdx.x; e < rows * a.cin; e += MG_OUT_TILE) {
        const int i = e / a.cin, c = e - i * a.cin;
        int p = t0 - pad + i;
        p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
        xs[i * cs + c] = (p >= 0 && p < len) ? mg_leaky(xb[(size_t)p * a.ldx + c], a.slope) : 0.f;
    }
    for (int e = threadIdx.x; e < MG_TAPS_IO * a.cin; e += MG_OUT_TILE) ws[e] = a.w0[e];
    __syncthreads();
    float acc = a.b0[0];
    for (int tap = 0; tap < MG_TAPS_IO; ++tap) {
        const float* xr = xs + (threadIdx.x + tap) * cs;
        const float* wr = ws + tap * a.cin;
        for (int c = 0; c < a.cin; ++c) acc = __builtin_fmaf(xr[c], wr[c], acc);
    }
    if (t < a.ld_wav) wb[t] = t < len ? fminf(1.f, fmaxf(-1.f, tanhf(acc))) : 0.f;
}

int mg_pad16(int c) { return (c + 15) / 16 * 16; }

// N-tiles per wave item by channel count, and the time tile that gives the four waves an item each
void mg_tile_form(int n_p, int* tile, int* form) {
    const int ntiles = n_p / 16;
    const int nt = (ntiles % 4 == 0 && ntiles >= 16) ? 4 : (ntiles % 2 == 0 ? 2 : 1);
    const int ngroups = ntiles / nt;
    const int mgroups = ngroups >= 4 ? 1 : (ngroups >= 2 ? 2 : 4);
    *tile = MG_ROWS * mgroups;
    *form = nt;
}

size_t mg_lds_bytes(const MgStage& s) {
    const size_t cs = (size_t)s.cin_p + 4;
    switch (s.kind) {
    case GT_MG_IN: return (size_t)(s.tile + MG_TAPS_IO - 1) * cs * sizeof(float);
    case GT_MG_UP: return (size_t)(s.tile + 1) * cs * sizeof(float);
    case GT_MG_RES: return ((size_t)(s.tile + 2 * s.dil) + s.tile) * cs * sizeof(float);
    default: return ((size_t)(MG_OUT_TILE + MG_TAPS_IO - 1) * (s.cin | 1) + (size_t)MG_TAPS_IO * s.cin) * sizeof(float);
    }
}

template <int NT>
hipError_t mg_launch_form(const MgStage& s, const MgArgs& a, dim3 grid, hipStream_t stream) {
    switch (s.kind) {
    case GT_MG_IN: gt_mg_in_kernel<NT><<<grid, MG_THREADS, s.lds, stream>>>(a); break;
    case GT_MG_UP: gt_mg_up_kernel<NT><<<grid, MG_THREADS, s.lds, stream>>>(a); break;
    default: gt_mg_res_kernel<NT><<<grid, MG_THREADS, s.lds, stream>>>(a); break;
    }
    return hipGetLastError();
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
        s.kind = kind; s.cin = cin; s.cout = cout; s.cin_p = mg_pad16(cin); s.n_p = mg_pad16(cout);
        s.rate_in = rate_in; s.rate_out = rate_out; s.r = r; s.dil = dil;
        if (kind == GT_MG_OUT) { s.tile = MG_OUT_TILE; s.form = 0; }
        else mg_tile_form(s.n_p, &s.tile, &s.form);
        while ((s.lds = mg_lds_bytes(s)) > GT_MG_LDS_MAX && kind != GT_MG_OUT && s.tile > MG_ROWS) s.tile >>= 1;
        if (kind != GT_MG_OUT) P.ws_floats_per_frame = std::max(P.ws_floats_per_frame, (size_t)rate_out * s.n_p);
        return s.lds <= GT_MG_LDS_MAX;
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

void gt_melgan_pack(const float* w, int taps, int cin, int cout, float* out) {
    const int cin_p = mg_pad16(cin), n_p = mg_pad16(cout);
    std::fill(out, out + (size_t)taps * cin_p * n_p, 0.f);
    for (int tap = 0; tap < taps; ++tap)
        for (int k = 0; k < cin; ++k)
            for (int nn = 0; nn < cout; ++nn)
                out[(size_t)tap * cin_p * n_p + ((size_t)(k >> 4) * n_p + nn) * 16 + (k & 15)] = w[((size_t)tap * cin + k) * cout + nn];
}

hipError_t gt_melgan_prepare() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gt_mg_out_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GT_MG_LDS_MAX);
#define MG_ATTR(K) if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, GT_MG_LDS_MAX)
    MG_ATTR(gt_mg_in_kernel<1>); MG_ATTR(gt_mg_in_kernel<2>); MG_ATTR(gt_mg_in_kernel<4>);
    MG_ATTR(gt_mg_up_kernel<1>); MG_ATTR(gt_mg_up_kernel<2>); MG_ATTR(gt_mg_up_kernel<4>);
    MG_ATTR(gt_mg_res_kernel<1>); MG_ATTR(gt_mg_res_kernel<2>); MG_ATTR(gt_mg_res_kernel<4>);
#undef MG_ATTR
    return e;
}

hipError_t gt_launch_melgan(const MgPlan& P, const MgCall& c, hipStream_t stream) {
    int cur = 0;
    for (int i = 0; i < P.n_stages; ++i) {
        const MgStage& s = P.st[i];
        MgArgs a{};
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
                grid.x = (c.ld_wav + MG_OUT_TILE - 1) / MG_OUT_TILE;
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
            gt_mg_out_kernel<<<grid, MG_OUT_TILE, s.lds, stream>>>(a);
            e = hipGetLastError();
        } else {
            e = s.form == 4 ? mg_launch_form<4>(s, a, grid, stream) : s.form == 2 ? mg_launch_form<2>(s, a, grid, stream)
                                                                                  : mg_launch_form<1>(s, a, grid, stream);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
