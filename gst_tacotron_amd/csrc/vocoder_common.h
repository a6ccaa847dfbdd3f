// What the three vocoders (melgan.hip, hifigan.hip, waveglow.hip) share: the tap-GEMM of a time-major activation tile in LDS against a
// fragment-packed weight, its staging, and the three kernels MelGAN and HiFi-GAN have in common (input conv, polyphase transposed conv,
// output conv).  Each .hip file instantiates what it needs; everything here has internal linkage, so each file owns its copies.
//
// Activations are time-major [B, L, C_p], C_p = C rounded up to 16, the padding channels exact zeros.  A wave owns items of 64 time rows
// x NT N-tiles; 256 threads a workgroup.  The MFMA lane maps: fp32 v_mfma_f32_16x16x4_f32, lane l holds A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15]; four of them (j = 0 .. 3) take k = 4 g + j of a 16-k block, g = l >> 4.  The 16-bit
// v_mfma_f32_16x16x32_{bf16,f16}: lane l holds A[row l & 15][k = 8 g + j] and B[k = 8 g + j][col l & 15], j = 0 .. 7.  C in both:
// lane l holds rows 4 g + i, i = 0 .. 3, of column l & 15 -- so every epilogue is the same code.
// A sample's summation order is bias, then taps ascending, then k ascending in blocks of VocOp<OP>::K: nothing here may reorder it.
#pragma once
#include <algorithm>
#include <stddef.h>
#include <stdint.h>

#include "kernels.h"
#include "device_utils.h"

#define VOC_THREADS 256
#define VOC_WAVES (VOC_THREADS / GT_WAVE)
#define VOC_ROWS 64             // time rows of a wave item: four M-tiles
#define VOC_OUT_TILE 256
#define VOC_TAPS_IO 7
#define GT_VOC_LDS_MAX (160 * 1024)     // the dynamic LDS a workgroup of any vocoder kernel may ask for

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The operand type of the MFMA: K the k block an MFMA group consumes (the LDS row and the weight pack are padded to it), Q = K / 4 the
// elements a lane holds of it, PAD the row padding in elements (16 bytes in every form).
template <typename OP> struct VocOp;
template <> struct VocOp<float> { static constexpr int K = 16, Q = 4, PAD = 4; };
template <> struct VocOp<__bf16> { static constexpr int K = 32, Q = 8, PAD = 8; typedef bf16x8 frag; };
template <> struct VocOp<_Float16> { static constexpr int K = 32, Q = 8, PAD = 8; typedef f16x8 frag; };
template <typename OP> __host__ __device__ __forceinline__ int voc_kpad(int c) { return (c + VocOp<OP>::K - 1) / VocOp<OP>::K * VocOp<OP>::K; }

// One argument struct for every kernel of MelGAN and HiFi-GAN (160 bytes of kernarg); a kernel reads what applies to it.  What only
// MelGAN reads stands last, so the fields gt_hg_conv_kernel reads keep the offsets its own struct gave them.
struct VocArgs {
    const float* x;             // the launch's input
    const float* res;           // gt_hg_conv_kernel: the raw residual or NULL
    float* y;                   // the activation written (gt_hg_conv_kernel: or NULL, the sum alone)
    float* sum;                 // gt_hg_conv_kernel: the fused sum
    const int32_t* frames;
    int32_t* wav_lengths;
    const float *w0, *b0;       // w0 holds OP words
    int T, ldx, cin, cin_p, n_p, rate_in, rate_out, r, taps, dil, tile, ld_wav, sum_mode;
    float slope, scale;
    const float *w1, *w2, *b1;  // gt_mg_res_kernel: shortcut, conv1, the two biases summed
    int min_frames;             // a row shorter than this is empty (HiFi-GAN: 1)
};

// A row's frames: frames[b] (or T) capped at T; a row shorter than min_frames is empty
__device__ __forceinline__ int voc_row_frames(const int32_t* frames, int b, int T, int min_frames) {
    int f = frames ? frames[b] : T;
    f = f < T ? f : T;
    return f < min_frames ? 0 : f;
}

__device__ __forceinline__ float voc_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// fp32 -> the operand type, to nearest even; fp16 saturates instead of overflowing to inf (a NaN stays a NaN)
template <typename OP> __device__ __forceinline__ OP voc_cvt(float v) { return (OP)v; }
template <> __device__ __forceinline__ _Float16 voc_cvt<_Float16>(float v) {
    v = v > 65504.f ? 65504.f : (v < -65504.f ? -65504.f : v);
    return (_Float16)v;
}
__device__ __forceinline__ void voc_store4(float* dst, const float4& v) { *reinterpret_cast<float4*>(dst) = v; }
template <typename OP>
__device__ __forceinline__ void voc_store4(OP* dst, const float4& v) {
    typedef OP op4 __attribute__((ext_vector_type(4)));
    const op4 o = {voc_cvt<OP>(v.x), voc_cvt<OP>(v.y), voc_cvt<OP>(v.z), voc_cvt<OP>(v.w)};
    *reinterpret_cast<op4*>(dst) = o;                       // 8 bytes: cs and c are multiples of 4 elements
}

// Positions [p0, p0 + rows) of one row's input (len valid positions, row stride ldx) into xs[rows][cs], channels [0, voc_kpad(cin_p)).
// A position outside [0, len) is folded back once when REFLECT; what is still outside, and every channel >= cin, is 0.  The fp32 value,
// the bounds and the LeakyReLU first, then rounded once to OP.  vec: ldx and cin_p are multiples of 4 and the input's padding channels
// hold zeros (a workspace activation), so 16-byte loads.
template <typename OP, bool LEAKY, bool REFLECT>
__device__ __forceinline__ void voc_stage(const float* xb, OP* xs, int cs, int p0, int rows, int len, bool vec, int ldx, int cin, int cin_p,
                                          float slope) {
    const int ck = voc_kpad<OP>(cin_p);
    if (vec) {
        const int c4n = ck >> 2;
        for (int e = threadIdx.x; e < rows * c4n; e += VOC_THREADS) {
            const int i = e / c4n, c = (e - i * c4n) << 2;
            int p = p0 + i;
            if (REFLECT) p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p >= 0 && p < len && c < cin_p) v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx + c);
            if (LEAKY) { v.x = voc_leaky(v.x, slope); v.y = voc_leaky(v.y, slope); v.z = voc_leaky(v.z, slope); v.w = voc_leaky(v.w, slope); }
            voc_store4(xs + i * cs + c, v);
        }
    } else {
        for (int e = threadIdx.x; e < rows * ck; e += VOC_THREADS) {
            const int i = e / ck, c = e - i * ck;
            int p = p0 + i;
            if (REFLECT) p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
            float v = 0.f;
            if (p >= 0 && p < len && c < cin) v = xb[(size_t)p * ldx + c];
            xs[i * cs + c] = voc_cvt<OP>(LEAKY ? voc_leaky(v, slope) : v);
        }
    }
}

// acc[mt][nt] += A[64 rows, 16 nkb] * W[16 nkb, 16 NT]: A from LDS (a_lane: this lane's row l & 15 of M-tile 0, k offset 4 (l >> 4)),
// W from the fragment pack (w_lane: this lane's column and k group of N-tile 0).  k ascending in groups of 16; inside a group MFMA j
// takes k = 4 g + j of the four lane groups g.  LEAKY: the LeakyReLU on the A operand as it is loaded.
template <int NT, bool LEAKY = false>
__device__ __forceinline__ void voc_gemm(f32x4 (&acc)[4][NT], const float* a_lane, int cs, const float* w_lane, int nkb, int n_p, float slope = 0.f) {
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
                for (int j = 0; j < 4; ++j) av[mt][j] = voc_leaky(av[mt][j], slope);
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

// The 16-bit form: acc[mt][nt] += A[64 rows, 32 nkb] * W[32 nkb, 16 NT].  a_lane: this lane's row l & 15 of M-tile 0, k offset 8 (l >> 4);
// w_lane: this lane's column and k quarter of N-tile 0 in the 16-bit pack.  One MFMA per M-tile, N-tile and 32 k.
__device__ __forceinline__ f32x4 voc_mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 voc_mfma16(const f16x8& a, const f16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
template <int NT, typename OP>
__device__ __forceinline__ void voc_gemm(f32x4 (&acc)[4][NT], const OP* a_lane, int cs, const OP* w_lane, int nkb, int n_p) {
    typedef typename VocOp<OP>::frag frag;
    for (int kb = 0; kb < nkb; ++kb) {
        frag av[4], bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const frag*>(w_lane + ((size_t)kb * n_p + nt * 16) * 32);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) av[mt] = *reinterpret_cast<const frag*>(a_lane + mt * 16 * cs + kb * 32);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = voc_mfma16(av[mt], bv[nt], acc[mt][nt]);
    }
}

template <int NT>
__device__ __forceinline__ void voc_bias(f32x4 (&acc)[4][NT], const float* bias, int n0, int col) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float b = bias[n0 + nt * 16 + col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = f32x4{b, b, b, b};
    }
}

// (The accumulator-to-y[t][n_p] store loop is written out in every kernel body: as a helper, although forced inline, it changed the
// register allocation of some forms -- DESIGN 3.5, "shared core".)
// ------------------------------------------------------------------------------------------------ the input conv
// 7 taps, mel_dim -> n_p: the mel tile plus 3 frames each side (REFLECT: reflected at the row's ends, else zeros) staged in LDS, 7 GEMMs
template <int NT, typename OP, bool REFLECT>
__global__ __launch_bounds__(VOC_THREADS) void gt_voc_in_kernel(VocArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char voc_lds_raw[];
    OP* lds = reinterpret_cast<OP*>(voc_lds_raw);
    constexpr int KB = VocOp<OP>::K, Q = VocOp<OP>::Q;
    const OP* w0 = reinterpret_cast<const OP*>(a.w0);
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, a.min_frames), t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int ck = voc_kpad<OP>(a.cin_p), cs = ck + VocOp<OP>::PAD, pad = VOC_TAPS_IO / 2;
    const float* xb = a.x + (size_t)b * a.T * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.n_p;
    voc_stage<OP, false, REFLECT>(xb, lds, cs, t0 - pad, a.tile + 2 * pad, len, false, a.ldx, a.cin, a.cin_p, a.slope);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = ck / KB, ngroups = (a.n_p >> 4) / NT, items = (a.tile / VOC_ROWS) * ngroups;
    for (int item = wave; item < items; item += VOC_WAVES) {
        const int mg = item / ngroups, n0 = (item - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        voc_bias<NT>(acc, a.b0, n0, col);
        for (int tap = 0; tap < VOC_TAPS_IO; ++tap)
            voc_gemm<NT>(acc, lds + (mg * VOC_ROWS + tap + col) * cs + Q * g, cs,
                         w0 + (size_t)tap * ck * a.n_p + (size_t)(n0 + col) * KB + Q * g, nkb, a.n_p);
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

// ------------------------------------------------------------------------------------------------ the transposed conv
// Kernel 2 r, stride r, padding r / 2 as a polyphase GEMM: output phase p of input position q takes taps p and p + r of positions q and
// q - 1 (K = 2 C, no zero stuffing), LeakyReLU applied while staging; a workgroup owns a tile of q and walks the r phases.
template <int NT, typename OP>
__global__ __launch_bounds__(VOC_THREADS) void gt_voc_up_kernel(VocArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char voc_lds_raw[];
    OP* lds = reinterpret_cast<OP*>(voc_lds_raw);
    constexpr int KB = VocOp<OP>::K, Q = VocOp<OP>::Q;
    const OP* w0 = reinterpret_cast<const OP*>(a.w0);
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, a.min_frames) * a.rate_in, q0 = blockIdx.x * a.tile;
    if (len == 0 || q0 > len) return;                       // q runs over [0, len]: position len still feeds the last r / 2 samples
    const int ck = voc_kpad<OP>(a.cin_p), cs = ck + VocOp<OP>::PAD;
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    float* yb = a.y + (size_t)b * a.T * a.rate_out * a.n_p;
    voc_stage<OP, true, false>(xb, lds, cs, q0 - 1, a.tile + 1, len, true, a.ldx, a.cin, a.cin_p, a.slope);   // xs[i] = LeakyReLU(x[q0 - 1 + i]), 0 where absent
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = ck / KB, ngroups = (a.n_p >> 4) / NT, per_phase = (a.tile / VOC_ROWS) * ngroups, items = per_phase * a.r;
    const int len_out = len * a.r, half = a.r >> 1;
    const size_t tap_stride = (size_t)ck * a.n_p;
    for (int item = wave; item < items; item += VOC_WAVES) {
        const int p = item / per_phase, rest = item - p * per_phase, mg = rest / ngroups, n0 = (rest - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        voc_bias<NT>(acc, a.b0, n0, col);
        const size_t wl = (size_t)(n0 + col) * KB + Q * g;
        voc_gemm<NT>(acc, lds + (mg * VOC_ROWS + 1 + col) * cs + Q * g, cs, w0 + p * tap_stride + wl, nkb, a.n_p);
        voc_gemm<NT>(acc, lds + (mg * VOC_ROWS + col) * cs + Q * g, cs, w0 + (p + a.r) * tap_stride + wl, nkb, a.n_p);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = q0 + mg * VOC_ROWS + mt * 16 + g * 4 + i;
                const int o = q * a.r + p - half;
                if (q <= len && o >= 0 && o < len_out) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) yb[(size_t)o * a.n_p + n0 + nt * 16 + col] = acc[mt][nt][i];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ the output conv
// C -> 1, 7 taps: a 7 C term dot product per sample on the VALU with the LeakyReLU in front and the tanh behind it fused; REFLECT as in
// the input conv; zeros beyond the row's length; writes wav_lengths.  fp32 in every operand form.
template <bool REFLECT>
__global__ __launch_bounds__(VOC_OUT_TILE) void gt_voc_out_kernel(VocArgs a) {
    extern __shared__ __attribute__((aligned(16))) float voc_lds_f32[];
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, a.min_frames) * a.rate_in, t0 = blockIdx.x * VOC_OUT_TILE, t = t0 + (int)threadIdx.x;
    float* wb = a.y + (size_t)b * a.ld_wav;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.wav_lengths) a.wav_lengths[b] = len;
    if (t0 >= len) {
        if (t < a.ld_wav) wb[t] = 0.f;
        return;
    }
    const int cs = a.cin | 1, pad = VOC_TAPS_IO / 2, rows = VOC_OUT_TILE + 2 * pad;
    float* xs = voc_lds_f32;                                // [rows][cs], LeakyReLU applied
    float* ws = voc_lds_f32 + rows * cs;                    // [7 * cin]
    const float* xb = a.x + (size_t)b * a.T * a.rate_in * a.ldx;
    for (int e = threadIdx.x; e < rows * a.cin; e += VOC_OUT_TILE) {
        const int i = e / a.cin, c = e - i * a.cin;
        int p = t0 - pad + i;
        if (REFLECT) p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
        xs[i * cs + c] = (p >= 0 && p < len) ? voc_leaky(xb[(size_t)p * a.ldx + c], a.slope) : 0.f;
    }
    for (int e = threadIdx.x; e < VOC_TAPS_IO * a.cin; e += VOC_OUT_TILE) ws[e] = a.w0[e];
    __syncthreads();
    float acc = a.b0[0];
    for (int tap = 0; tap < VOC_TAPS_IO; ++tap) {
        const float* xr = xs + (threadIdx.x + tap) * cs;
        const float* wr = ws + tap * a.cin;
        for (int c = 0; c < a.cin; ++c) acc = __builtin_fmaf(xr[c], wr[c], acc);
    }
    if (t < a.ld_wav) wb[t] = t < len ? fminf(1.f, fmaxf(-1.f, tanhf(acc))) : 0.f;
}

// dynamic LDS of the output conv
inline size_t voc_out_lds(int cin) { return ((size_t)(VOC_OUT_TILE + VOC_TAPS_IO - 1) * (cin | 1) + (size_t)VOC_TAPS_IO * cin) * sizeof(float); }

// ------------------------------------------------------------------------------------------------ host
// e, or once e is an error nothing: lets `kernel` ask for up to GT_VOC_LDS_MAX of dynamic LDS
template <typename K>
hipError_t voc_allow_lds(hipError_t e, K* kernel) {
    return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GT_VOC_LDS_MAX);
}

inline int voc_pad16(int c) { return (c + 15) / 16 * 16; }

// N-tiles per wave item by channel count, and the time tile that gives the four waves an item each
inline void voc_tile_form(int n_p, int* tile, int* form) {
    const int ntiles = n_p / 16;
    const int nt = (ntiles % 4 == 0 && ntiles >= 16) ? 4 : (ntiles % 2 == 0 ? 2 : 1);
    const int ngroups = ntiles / nt;
    const int mgroups = ngroups >= 4 ? 1 : (ngroups >= 2 ? 2 : 4);
    *tile = VOC_ROWS * mgroups;
    *form = nt;
}

// [taps * cin, cout] (row stride cout) -> the fp32 fragment pack [taps][cin_p / 16][n_p][g = (k % 16) / 4][j = k % 4] the B operand is
// read in, zero padded: one coalesced 16-byte load per lane and 16 k
inline void voc_pack_f32(const float* w, int taps, int cin, int cout, float* out) {
    const int cin_p = voc_pad16(cin), n_p = voc_pad16(cout);
    std::fill(out, out + (size_t)taps * cin_p * n_p, 0.f);
    for (int tap = 0; tap < taps; ++tap)
        for (int k = 0; k < cin; ++k)
            for (int nn = 0; nn < cout; ++nn)
                out[(size_t)tap * cin_p * n_p + ((size_t)(k >> 4) * n_p + nn) * 16 + (k & 15)] = w[((size_t)tap * cin + k) * cout + nn];
}

}  // namespace
