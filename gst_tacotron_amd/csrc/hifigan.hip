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
// Activations are time-major [B, L, C_p], C_p = C rounded up to 16; the padding channels are exact zeros everywhere (zero weights, zero
// bias, LeakyReLU(0) = 0, 0 + 0 = 0), so any channel count runs the same kernels.  Weights are repacked on the host (gt_hifigan_pack)
// into the order the B operand is read in: [tap][k / 16][n][g = (k % 16) / 4][j = k % 4], one coalesced 16-byte load per lane and 16 k.
//
//   gt_hg_in_kernel    the 7-tap input conv: the mel tile plus 3 frames each side (zeros outside the row) staged in LDS, 7 GEMMs of K = mel_dim
//   gt_hg_up_kernel    the transposed conv as a polyphase GEMM: output phase p of input position q takes taps p and p + r of positions
//                      q and q - 1 (K = 2 C, no zero stuffing), LeakyReLU applied while staging; a workgroup owns a tile of q and
//                      walks the r phases
//   gt_hg_conv_kernel  ONE launch per residual conv, at every width: the tile plus a halo of (k - 1) / 2 * d each side staged through the
//                      LeakyReLU (zeros outside the row), k dilated tap-GEMMs into one accumulator, and an epilogue that adds the raw
//                      residual and either writes the activation or, on the last unit of block j, the fused sum (sum = y for j = 0,
//                      sum += y else, times 1 / n_k on the last block).  The sum's read-modify-write is done by the element's owner and
//                      ordered by the stream: one order, no atomics.  (A fused pair would keep the intermediate in LDS, but at 256
//                      channels, k = 11, d = 5 the two tiles need 206 KB; one form for every width was chosen -- DESIGN 3.5.)
//   gt_hg_out_kernel   C_last -> 1: a 7 * C_last term dot product per sample on the VALU with the tanh fused; zeros beyond the row's length
// A wave owns items of 64 time rows x NT N-tiles (the plan's `form`, by channel count); 256 threads a workgroup.  Every output sample
// has one summation order -- bias, then taps ascending, k ascending in groups of 16, then the residual, then the fused sum in block
// order -- that depends on neither the batch nor the call's T nor the capacity: a row's samples are bitwise those of the row run alone.
// Every global access is bounded by the row's length at that stage (<= T * rate), every LDS access by the tile the plan sized; nothing
// waits on another workgroup.
//
// The 16-bit operand forms (gsttaco_hifigan_set_operands; GT_HG_OP_BF16 / GT_HG_OP_F16) run the same three GEMM kernels on
// v_mfma_f32_16x16x32_{bf16,f16}: one template over the operand type, the two instructions share their lane maps (lane l holds
// A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0 .. 7; C as the fp32 16x16x4 form, so the epilogues are
// the same code).  HBM is untouched: activations stay fp32 at C_p = round16(C).  hg_stage applies its bounds and the LeakyReLU in fp32,
// then rounds to nearest even once (fp16 saturating to +-65504) into a 16-bit LDS tile whose rows are padded with exact zeros to a
// multiple of 32 k, plus 8 elements: the row stride is then an odd number of 16-byte slots, and the 16 rows of a ds_read_b128 lane group
// (8 at one k quarter, 8 at the next) fall on 16-byte slots at worst 2-way.  The weights are rounded once on the host (gt_hifigan_pack16)
// into [tap][k / 32][n][q = (k % 32) / 8][j = k % 8]: one 16-byte load per lane and 32 k.  k advances in blocks of 32; a sample's order
// is bias, taps ascending, k ascending in blocks of 32 (inside a block the MFMA's own), the residual, the fused sum -- still independent
// of batch, T and capacity.  The output conv stays fp32 on the VALU in every form.
#include <algorithm>
#include <string.h>
#include <math.h>

#include "kernels.h"
#include "device_utils.h"

#define HG_THREADS 256
#define HG_WAVES (HG_THREADS / GT_WAVE)
#define HG_ROWS 64              // time rows of a wave item: four M-tiles
#define HG_OUT_TILE 256
#define HG_TAPS_IO 7

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The operand type of the MFMA: K the k block an MFMA group consumes (the LDS row and the weight pack are padded to it), Q = K / 4 the
// elements a lane holds of it, PAD the row padding in elements (16 bytes in every form).
template <typename OP> struct HgOp;
template <> struct HgOp<float> { static constexpr int K = 16, Q = 4, PAD = 4; };
template <> struct HgOp<__bf16> { static constexpr int K = 32, Q = 8, PAD = 8; typedef bf16x8 frag; };
template <> struct HgOp<_Float16> { static constexpr int K = 32, Q = 8, PAD = 8; typedef f16x8 frag; };
template <typename OP> __host__ __device__ __forceinline__ int hg_kpad(int c) { return (c + HgOp<OP>::K - 1) / HgOp<OP>::K * HgOp<OP>::K; }

struct HgArgs {
    const float* x;             // the launch's input
    const float* res;           // GT_HG_CONV: the raw residual or NULL
    float* y;                   // the activation written, or NULL (the sum alone)
    float* sum;                 // GT_HG_CONV: the fused sum
    const int32_t* frames;
    int32_t* wav_lengths;
    const float *w0, *b0;
    int T, ldx, cin, cin_p, n_p, rate_in, rate_out, r, taps, dil, tile, ld_wav, sum_mode;
    float slope, scale;
};

__device__ __forceinline__ int hg_row_frames(const HgArgs& a, int b) {
    int f = a.frames ? a.frames[b] : a.T;
    f = f < a.T ? f : a.T;
    return f < 1 ? 0 : f;
}

__device__ __forceinline__ float hg_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// Positions [p0, p0 + rows) of one row's input (len valid positions, row stride ldx) into xs[rows][cs], channels [0, cin_p).  A position
// outside [0, len), and every channel >= cin, is 0.
// fp32 -> the operand type, to nearest even; fp16 saturates instead of overflowing to inf (a NaN stays a NaN)
template <typename OP> __device__ __forceinline__ OP hg_cvt(float v) { return (OP)v; }
template <> __device__ __forceinline__ _Float16 hg_cvt<_Float16>(float v) {
    v = v > 65504.f ? 65504.f : (v < -65504.f ? -65504.f : v);
    return (_Float16)v;
}
__device__ __forceinline__ void hg_store4(float* dst, const float4& v) { *reinterpret_cast<float4*>(dst) = v; }
template <typename OP>
__device__ __forceinline__ void hg_store4(OP* dst, const float4& v) {
    typedef OP op4 __attribute__((ext_vector_type(4)));
    const op4 o = {hg_cvt<OP>(v.x), hg_cvt<OP>(v.y), hg_cvt<OP>(v.z), hg_cvt<OP>(v.w)};
    *reinterpret_cast<op4*>(dst) = o;                       // 8 bytes: cs and c are multiples of 4 elements
}

// The same for the operand type OP: the fp32 value, bounds and LeakyReLU first, then rounded once; channels [cin_p, hg_kpad(cin_p)) are 0.
template <typename OP, bool LEAKY>
__device__ __forceinline__ void hg_stage(const HgArgs& a, const float* xb, OP* xs, int cs, int p0, int rows, int len, bool vec) {
    const int ck = hg_kpad<OP>(a.cin_p);
    if (vec) {
        const int c4n = ck >> 2;
        for (int e = threadIdx.x; e < rows * c4n; e += HG_THREADS) {
            const int i = e / c4n, c = (e - i * c4n) << 2;
            const int p = p0 + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p >= 0 && p < len && c < a.cin_p) v = *reinterpret_cast<const float4*>(xb + (size_t)p * a.ldx + c);
            if (LEAKY) { v.x = hg_leaky(v.x, a.slope); v.y = hg_leaky(v.y, a.slope); v.z = hg_leaky(v.z, a.slope); v.w = hg_leaky(v.w, a.slope); }
            hg_store4(xs + i * cs + c, v);
        }
    } else {
        for (int e = threadIdx.x; e < rows * ck; e += HG_THREADS) {
            const int i = e / ck, c = e - i * ck;
            const int p = p0 + i;
            float v = 0.f;
            if (p >= 0 && p < len && c < a.cin) v = xb[(size_t)p * a.ldx + c];
            xs[i * cs + c] = hg_cvt<OP>(LEAKY ? hg_leaky(v, a.slope) : v);
        }
    }
}

// acc[mt][nt] += A[64 rows, 16 nkb] * W[16 nkb, 16 NT]: A from LDS (a_lane: this lane's row l & 15 of M-tile 0, k offset 4 (l >> 4)),
// W from the fragment pack (w_lane: this lane's column and k group of N-tile 0).  k ascending in groups of 16; inside a group MFMA j
// takes k = 4 g + j of the four lane groups g.
template <int NT>
__device__ __forceinline__ void hg_gemm(f32x4 (&acc)[4][NT], const float* a_lane, int cs, const float* w_lane, int nkb, int n_p) {
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
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][j], bv[nt][j], acc[mt][nt], 0, 0, 0);
    }
}

// The 16-bit form: acc[mt][nt] += A[64 rows, 32 nkb] * W[32 nkb, 16 NT].  a_lane: this lane's row l & 15 of M-tile 0, k offset 8 (l >> 4);
// w_lane: this lane's column and k quarter of N-tile 0 in the 16-bit pack.  One MFMA per M-tile, N-tile and 32 k.
__device__ __forceinline__ f32x4 hg_mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 hg_mfma16(const f16x8& a, const f16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
template <int NT, typename OP>
__device__ __forceinline__ void hg_gemm(f32x4 (&acc)[4][NT], const OP* a_lane, int cs, const OP* w_lane, int nkb, int n_p) {
    typedef typename HgOp<OP>::frag frag;
    for (int kb = 0; kb < nkb; ++kb) {
        frag av[4], bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const frag*>(w_lane + ((size_t)kb * n_p + nt * 16) * 32);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) av[mt] = *reinterpret_cast<const frag*>(a_lane + mt * 16 * cs + kb * 32);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = hg_mfma16(av[mt], bv[nt], acc[mt][nt]);
    }
}

template <int NT>
__device__ __forceinline__ void hg_bias(f32x4 (&acc)[4][NT], const float* bias, int n0, int col) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float b = bias[n0 + nt * 16 + col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = f32x4{b, b, b, b};
    }
}

// ------------------------------------------------------------------------------------------------ the input conv
template <int NT, typename OP>
__global__ __launch_bounds__(HG_THREADS) void gt_hg_in_kernel(HgArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds_raw[];
    OP* hg_lds = reinterpret_cast<OP*>(hg_lds_raw);
    constexpr int KB = HgOp<OP>::K, Q = HgOp<OP>::Q;
    const OP* w0 = reinterpret_cast<const OP*>(a.w0);
    const int b = blockIdx.y, len = hg_row_frames(a, b), t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int ck = hg_kpad<OP>(a.cin_p), cs = ck + HgOp<OP>::PAD, pad = HG_TAPS_IO / 2;
    const float* xb = a.x + (size_t)b * a.T * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.n_p;
    hg_stage<OP, false>(a, xb, hg_lds, cs, t0 - pad, a.tile + 2 * pad, len, false);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = ck / KB, ngroups = (a.n_p >> 4) / NT, items = (a.tile / HG_ROWS) * ngroups;
    for (int item = wave; item < items; item += HG_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        hg_bias<NT>(acc, a.b0, n0, col);
        for (int tap = 0; tap < HG_TAPS_IO; ++tap)
            hg_gemm<NT>(acc, hg_lds + (mg * HG_ROWS + tap + col) * cs + Q * g, cs,
                        w0 + (size_t)tap * ck * a.n_p + (size_t)(n0 + col) * KB + Q * g, nkb, a.n_p);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + mg * HG_ROWS + mt * 16 + g * 4 + i;
                if (t < len) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)t * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ the transposed conv
template <int NT, typename OP>
__global__ __launch_bounds__(HG_THREADS) void gt_hg_up_kernel(HgArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds_raw[];
    OP* hg_lds = reinterpret_cast<OP*>(hg_lds_raw);
    constexpr int KB = HgOp<OP>::K, Q = HgOp<OP>::Q;
    const OP* w0 = reinterpret_cast<const OP*>(a.w0);
    const int b = blockIdx.y, len = hg_row_frames(a, b) * a.rate_in, q0 = blockIdx.x * a.tile;
    if (len == 0 || q0 > len) return;                       // q runs over [0, len]: position len still feeds the last r / 2 samples
    const int ck = hg_kpad<OP>(a.cin_p), cs = ck + HgOp<OP>::PAD;
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.rate_out * a.n_p;
    hg_stage<OP, true>(a, xb, hg_lds, cs, q0 - 1, a.tile + 1, len, true);       // xs[i] = LeakyReLU(x[q0 - 1 + i]), 0 where absent
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = ck / KB, ngroups = (a.n_p >> 4) / NT, per_phase = (a.tile / HG_ROWS) * ngroups, items = per_phase * a.r;
    const int len_out = len * a.r, half = a.r >> 1;
    const size_t tap_stride = (size_t)ck * a.n_p;
    for (int item = wave; item < items; item += HG_WAVES) {
        const int p = item / per_phase, rest = item - p * per_phase, mg = rest / ngroups, n0 = (rest - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        hg_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * KB + Q * g;
        hg_gemm<NT>(acc, hg_lds + (mg * HG_ROWS + 1 + col) * cs + Q * g, cs, w0 + p * tap_stride + wl, nkb, a.n_p);
        hg_gemm<NT>(acc, hg_lds + (mg * HG_ROWS + col) * cs + Q * g, cs, w0 + (p + a.r) * tap_stride + wl, nkb, a.n_p);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = q0 + mg * HG_ROWS + mt * 16 + g * 4 + i;
                const int o = q * a.r + p - half;
                if (q <= len && o >= 0 && o < len_out) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)o * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ one residual conv
template <int NT, typename OP>
__global__ __launch_bounds__(HG_THREADS) void gt_hg_conv_kernel(HgArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds_raw[];
    OP* hg_lds = reinterpret_cast<OP*>(hg_lds_raw);
    constexpr int KB = HgOp<OP>::K, Q = HgOp<OP>::Q;
    const OP* w0 = reinterpret_cast<const OP*>(a.w0);
    const int b = blockIdx.y, len = hg_row_frames(a, b) * a.rate_in, t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int ck = hg_kpad<OP>(a.cin_p), cs = ck + HgOp<OP>::PAD, d = a.dil, halo = (a.taps >> 1) * d;
    const size_t row0 = (size_t)b * a.T * a.rate_in * a.n_p;            // cin_p == n_p: every buffer of the stage has this shape
    hg_stage<OP, true>(a, a.x + row0, hg_lds, cs, t0 - halo, a.tile + 2 * halo, len, true);
    __syncthreads();
    const float* rb = a.res ? a.res + row0 : nullptr;
    float* yb = a.y ? a.y + row0 : nullptr;
    float* sb = a.sum + row0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = ck / KB, ngroups = (a.n_p >> 4) / NT, items = (a.tile / HG_ROWS) * ngroups;
    const size_t tap_stride = (size_t)ck * a.n_p;
    for (int item = wave; item < items; item += HG_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        hg_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * KB + Q * g;
        for (int tap = 0; tap < a.taps; ++tap)
            hg_gemm<NT>(acc, hg_lds + (mg * HG_ROWS + tap * d + col) * cs + Q * g, cs, w0 + tap * tap_stride + wl, nkb, a.n_p);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + mg * HG_ROWS + mt * 16 + g * 4 + i;
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

// ------------------------------------------------------------------------------------------------ the output conv
__global__ __launch_bounds__(HG_OUT_TILE) void gt_hg_out_kernel(HgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float hg_lds[];
    const int b = blockIdx.y, len = hg_row_frames(a, b) * a.rate_in, t0 = blockIdx.x * HG_OUT_TILE, t = t0 + (int)threadIdx.x;
    float* wb = a.y + (size_t)b * a.ld_wav;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.wav_lengths) a.wav_lengths[b] = len;
    if (t0 >= len) {
        if (t < a.ld_wav) wb[t] = 0.f;
        return;
    }
    const int cs = a.cin | 1, pad = HG_TAPS_IO / 2, rows = HG_OUT_TILE + 2 * pad;
    float* xs = hg_lds;                                     // [rows][cs], LeakyReLU (the output slope) applied
    float* ws = hg_lds + rows * cs;                         // [7 * cin]
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    for (int e = threadIdx.x; e < rows * a.cin; e += HG_OUT_TILE) {
        const int i = e / a.cin, c = e - i * a.cin;
        const int p = t0 - pad + i;
        xs[i * cs + c] = (p >= 0 && p < len) ? hg_leaky(xb[(size_t)p * a.ldx + c], a.slope) : 0.f;
    }
    for (int e = threadIdx.x; e < HG_TAPS_IO * a.cin; e += HG_OUT_TILE) ws[e] = a.w0[e];
    __syncthreads();
    float acc = a.b0[0];
    for (int tap = 0; tap < HG_TAPS_IO; ++tap) {
        const float* xr = xs + (threadIdx.x + tap) * cs;
        const float* wr = ws + tap * a.cin;
        for (int c = 0; c < a.cin; ++c) acc = __builtin_fmaf(xr[c], wr[c], acc);
    }
    if (t < a.ld_wav) wb[t] = t < len ? fminf(1.f, fmaxf(-1.f, tanhf(acc))) : 0.f;
}

int hg_pad16(int c) { return (c + 15) / 16 * 16; }

// N-tiles per wave item by channel count, and the time tile that gives the four waves an item each
void hg_tile_form(int n_p, int* tile, int* form) {
    const int ntiles = n_p / 16;
    const int nt = (ntiles % 4 == 0 && ntiles >= 16) ? 4 : (ntiles % 2 == 0 ? 2 : 1);
    const int ngroups = ntiles / nt;
    const int mgroups = ngroups >= 4 ? 1 : (ngroups >= 2 ? 2 : 4);
    *tile = HG_ROWS * mgroups;
    *form = nt;
}

// op_bytes: the size of an MFMA operand, 4 (fp32: rows of cin_p + 4) or 2 (16-bit: rows of round32(cin_p) + 8); the output conv is fp32 always
size_t hg_lds_bytes(const HgStage& s, size_t op_bytes) {
    const size_t cs = op_bytes == 4 ? (size_t)s.cin_p + HgOp<float>::PAD : (size_t)hg_kpad<__bf16>(s.cin_p) + HgOp<__bf16>::PAD;
    switch (s.kind) {
    case GT_HG_IN: return (size_t)(s.tile + HG_TAPS_IO - 1) * cs * op_bytes;
    case GT_HG_UP: return (size_t)(s.tile + 1) * cs * op_bytes;
    case GT_HG_CONV: return ((size_t)s.tile + (size_t)(s.taps - 1) * s.dil) * cs * op_bytes;
    default: return ((size_t)(HG_OUT_TILE + HG_TAPS_IO - 1) * (s.cin | 1) + (size_t)HG_TAPS_IO * s.cin) * sizeof(float);
    }
}

template <int NT, typename OP>
hipError_t hg_launch_form(const HgStage& s, const HgArgs& a, dim3 grid, hipStream_t stream) {
    switch (s.kind) {
    case GT_HG_IN: gt_hg_in_kernel<NT, OP><<<grid, HG_THREADS, s.lds, stream>>>(a); break;
    case GT_HG_UP: gt_hg_up_kernel<NT, OP><<<grid, HG_THREADS, s.lds, stream>>>(a); break;
    default: gt_hg_conv_kernel<NT, OP><<<grid, HG_THREADS, s.lds, stream>>>(a); break;
    }
    return hipGetLastError();
}

template <typename OP>
hipError_t hg_launch_op(const HgStage& s, const HgArgs& a, dim3 grid, hipStream_t stream) {
    return s.form == 4 ? hg_launch_form<4, OP>(s, a, grid, stream) : s.form == 2 ? hg_launch_form<2, OP>(s, a, grid, stream)
                                                                                 : hg_launch_form<1, OP>(s, a, grid, stream);
}

template <typename OP>
hipError_t hg_prepare_op() {
    hipError_t e = hipSuccess;
#define HG_ATTR(K) if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, GT_HG_LDS_MAX)
    HG_ATTR((gt_hg_in_kernel<1, OP>)); HG_ATTR((gt_hg_in_kernel<2, OP>)); HG_ATTR((gt_hg_in_kernel<4, OP>));
    HG_ATTR((gt_hg_up_kernel<1, OP>)); HG_ATTR((gt_hg_up_kernel<2, OP>)); HG_ATTR((gt_hg_up_kernel<4, OP>));
    HG_ATTR((gt_hg_conv_kernel<1, OP>)); HG_ATTR((gt_hg_conv_kernel<2, OP>)); HG_ATTR((gt_hg_conv_kernel<4, OP>));
#undef HG_ATTR
    return e;
}

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
    P.mel_dim = cfg.mel_dim; P.hop = (int)hop; P.slope = cfg.slope; P.out_slope = cfg.out_slope; P.min_frames = 1;
    int C = cfg.initial, rate = 1, n = 0;
    auto add = [&](int kind, int cin, int cout, int rate_in, int rate_out, int r, int taps, int dil) -> HgStage* {
        HgStage& s = P.st[n++];
        s.kind = kind; s.cin = cin; s.cout = cout; s.cin_p = hg_pad16(cin); s.n_p = hg_pad16(cout);
        s.rate_in = rate_in; s.rate_out = rate_out; s.r = r; s.taps = taps; s.dil = dil;
        s.src = s.res = s.dst = -1; s.sum = GT_HG_SUM_NONE; s.scale = 1.f; s.up = s.block = s.unit = s.conv = -1;
        if (kind == GT_HG_OUT) { s.tile = HG_OUT_TILE; s.form = 0; }
        else hg_tile_form(s.n_p, &s.tile, &s.form);
        while ((s.lds = hg_lds_bytes(s, sizeof(float))) > GT_HG_LDS_MAX && kind != GT_HG_OUT && s.tile > HG_ROWS) s.tile >>= 1;
        if (kind != GT_HG_OUT) P.ws_floats_per_frame = std::max(P.ws_floats_per_frame, (size_t)rate_out * s.n_p);
        return s.lds <= GT_HG_LDS_MAX ? &s : nullptr;
    };
    static const char* lds_msg = "a launch's smallest tile does not fit the 160 KB of LDS (initial: fewer channels, or dilations: a narrower halo)";
    if (!add(GT_HG_IN, cfg.mel_dim, C, 1, 1, 0, HG_TAPS_IO, 1)) return lds_msg;
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
    if (!add(GT_HG_OUT, C, 1, rate, rate, 0, HG_TAPS_IO, 1)) return lds_msg;
    P.n_stages = n;
    return nullptr;
}

void gt_hifigan_pack(const float* w, int taps, int cin, int cout, float* out) {
    const int cin_p = hg_pad16(cin), n_p = hg_pad16(cout);
    std::fill(out, out + (size_t)taps * cin_p * n_p, 0.f);
    for (int tap = 0; tap < taps; ++tap)
        for (int k = 0; k < cin; ++k)
            for (int nn = 0; nn < cout; ++nn)
                out[(size_t)tap * cin_p * n_p + ((size_t)(k >> 4) * n_p + nn) * 16 + (k & 15)] = w[((size_t)tap * cin + k) * cout + nn];
}

void gt_hifigan_set_operands(HgPlan* plan, int operands) {
    plan->operands = operands;
    for (int i = 0; i < plan->n_stages; ++i) plan->st[i].lds = hg_lds_bytes(plan->st[i], operands == GT_HG_OP_F32 ? 4 : 2);
}

size_t gt_hifigan_pack16_words(int taps, int cin, int cout) { return (size_t)taps * hg_kpad<__bf16>(hg_pad16(cin)) * hg_pad16(cout); }

int64_t gt_hifigan_pack16(const float* w, int taps, int cin, int cout, int operands, uint16_t* out) {
    const int ck = hg_kpad<__bf16>(hg_pad16(cin)), n_p = hg_pad16(cout);
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
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gt_hg_out_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GT_HG_LDS_MAX);
    if (e == hipSuccess) e = hg_prepare_op<float>();
    if (e == hipSuccess) e = hg_prepare_op<__bf16>();
    if (e == hipSuccess) e = hg_prepare_op<_Float16>();
    return e;
}

hipError_t gt_launch_hifigan(const HgPlan& P, const HgCall& c, hipStream_t stream) {
    for (int i = 0; i < P.n_stages; ++i) {
        if (c.only >= 0 && c.only != i) continue;
        const HgStage& s = P.st[i];
        HgArgs a{};
        a.frames = c.frames; a.wav_lengths = c.wav_lengths;
        a.w0 = s.w0; a.b0 = s.b0;
        a.T = c.T; a.cin = s.cin; a.cin_p = s.cin_p; a.n_p = s.n_p; a.rate_in = s.rate_in; a.rate_out = s.rate_out;
        a.r = s.r; a.taps = s.taps; a.dil = s.dil; a.tile = s.tile; a.ld_wav = c.ld_wav; a.sum_mode = s.sum;
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
            grid.x = (c.ld_wav + HG_OUT_TILE - 1) / HG_OUT_TILE;
        }
        hipError_t e;
        if (s.kind == GT_HG_OUT) {
            gt_hg_out_kernel<<<grid, HG_OUT_TILE, s.lds, stream>>>(a);
            e = hipGetLastError();
        } else {
            e = P.operands == GT_HG_OP_BF16 ? hg_launch_op<__bf16>(s, a, grid, stream)
              : P.operands == GT_HG_OP_F16 ? hg_launch_op<_Float16>(s, a, grid, stream) : hg_launch_op<float>(s, a, grid, stream);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
