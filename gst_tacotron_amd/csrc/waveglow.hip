// The flow vocoder: WaveGlow inference (Prenger, Valle & Catanzaro 2019), mel -> waveform, sampled from noise under a temperature
// (gsttaco_waveglow: include/gsttaco.h holds the contract).  fp32 storage, v_mfma_f32_16x16x4_f32 with fp32 accumulation.
//
// One row of `frames` frames, G = n_group, L = frames * hop / G columns, S = mel_dim * G, C = n_channels, c_k the channels of flow k:
//   up      ConvTranspose1D mel_dim -> mel_dim, kernel win, stride hop, bias, cropped to frames * hop samples: sample q hop + p sums taps
//           p + j hop of frames q - j, j = 0 .. win / hop - 1 (frames below 0 absent); stored grouped, spect[l, m G + g] = up[l G + g, m]
//   noise   audio [L, n_rem] = sigma z[:, 0:n_rem]
//   flow k = F-1 .. 0, h = c_k / 2:  hid = start_k(audio[:, :h]);  per layer i at dilation 2^i, zero padding at the row's ends:
//           acts = in_{k,i}(hid) (3 taps) + cond_{k,i}(spect) (1 tap), g = tanh(acts[:, :C]) sigmoid(acts[:, C:]), rs = res_skip_{k,i}(g),
//           hid += rs[:, :C], out += rs[:, C:] (the last layer: out += rs);  [b | s] = end_k(out);  audio[:, h:] = (audio[:, h:] - b) exp(-s);
//           audio = audio inverse(W_k)^T;  where k % n_early_every == 0 and k > 0: audio = [sigma z[:, next n_early_size] | audio]
//   wav[l G + g] = audio[l, g]
//
// Activations are time-major [B, L, C_p], C_p = C rounded up to 16, the padding channels exact zeros (zero weights and biases, and
// tanh(0) sigmoid(0) = 0).  The fp32 tap-GEMM (voc_gemm, voc_bias), the row-length rule and the fragment pack the weights use
// (voc_pack_f32: [tap][k / 16][n][4][4]) are vocoder_common.h's; wg_stage stages a column window of a row and is this file's own.
//
//   gt_wg_up_kernel     the transposed conv as a polyphase GEMM, K = (win / hop) mel_dim per sample: a workgroup owns a tile of frames
//                       (staged with the win / hop - 1 frames in front of it) and walks the hop phases; stores into the grouped layout
//   gt_wg_layer_kernel  ONE launch per WN layer.  The accumulator starts at the two biases summed; the three dilated taps of hid and the
//                       conditioning GEMM over spect are ONE K loop of 3 C_p + S_p, staged through LDS in chunks of `kc` (the spect
//                       tile would not fit beside hid); in / cond are packed so that a wave's N-tiles alternate a tanh tile and the
//                       sigmoid tile of the same 16 channels: the gate needs no shuffle.  The gated tile stays in LDS for the res_skip
//                       GEMM (K = C_p), whose epilogue writes hid_out = hid_in + res (ping-pong: a layer reads its neighbours'
//                       columns) and out (+)= skip.
//   gt_wg_flow_kernel   the flow's tail on the VALU, every width at most 16: end, the coupling, inverse(W), the early concatenation,
//                       and the NEXT flow's start into hid.  The first launch of this form draws or reads z and runs flow F-1's
//                       start; the last writes wav, the zeros beyond each row and wav_lengths.
//   gt_wg_noise_kernel  z[b, l G + g] = gt_normal of gt_philox(seeds[b], l, g, 0, GT_RNG_WAVEGLOW): what the flow kernels draw in place.
// Every output has one summation order (bias, taps ascending, k ascending in groups of 16, the conditioning behind the taps) that
// depends on neither the batch nor the call's T nor the capacity; no atomics; nothing waits on another workgroup; every global access
// is bounded by the row's own length, so stale workspace behind a row's end is never read.
#include <algorithm>
#include <math.h>
#include <vector>

#include "vocoder_common.h"

#define WG_AW 16                // the audio buffer's row width (n_group <= 16)
#define WG_OS (WG_AW + 1)       // row stride of the flow kernel's per-column LDS rows

namespace {

// Columns [k0, k0 + w) of positions [p0, p0 + rows) of one row's activation (len valid positions, row stride ld, w a multiple of 16)
// into xs[rows][cs]; a position outside [0, len) is zeros.
__device__ __forceinline__ void wg_stage(const float* xb, float* xs, int cs, int ld, int k0, int w, int p0, int rows, int len) {
    const int c4n = w >> 2;
    for (int e = threadIdx.x; e < rows * c4n; e += VOC_THREADS) {
        const int i = e / c4n, c = (e - i * c4n) << 2, p = p0 + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p >= 0 && p < len) v = *reinterpret_cast<const float4*>(xb + (size_t)p * ld + k0 + c);
        *reinterpret_cast<float4*>(xs + i * cs + c) = v;
    }
}

// ------------------------------------------------------------------------------------------------ the upsampler
struct WgUpArgs {
    const float* mel;           // [B, T, mel_dim]
    float* spect;               // [B, T * hop / G, S_p]
    const int32_t* frames;
    const float *w, *b;         // [win][mel_p / 16][mel_p][16], [mel_p]
    int T, mel_dim, mel_p, hop, taps, G, S, S_p, tile;      // taps = win / hop
};

template <int NT>
__global__ __launch_bounds__(VOC_THREADS) void gt_wg_up_kernel(WgUpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, 1), q0 = blockIdx.x * a.tile;
    if (q0 >= len) return;
    const int cs = a.mel_p + 4, back = a.taps - 1, rows = a.tile + back;
    const float* xb = a.mel + (size_t)b * a.T * a.mel_dim;
    for (int e = threadIdx.x; e < rows * a.mel_p; e += VOC_THREADS) {        // xs[i] = mel[q0 - back + i], 0 where absent
        const int i = e / a.mel_p, c = e - i * a.mel_p, p = q0 - back + i;
        wg_lds[i * cs + c] = (p >= 0 && p < len && c < a.mel_dim) ? xb[(size_t)p * a.mel_dim + c] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int nkb = a.mel_p >> 4, ngroups = (a.mel_p >> 4) / NT, per_phase = (a.tile / VOC_ROWS) * ngroups, items = per_phase * a.hop;
    const int cpf = a.hop / a.G;                            // columns per frame
    const size_t tap_stride = (size_t)a.mel_p * a.mel_p;
    float* sb = a.spect + (size_t)b * a.T * cpf * a.S_p;
    for (int item = wave; item < items; item += VOC_WAVES) {
        const int p = item / per_phase, rest = item - p * per_phase, mg = rest / ngroups, n0 = (rest - mg * ngroups) * NT * 16;
        f32x4 acc[4][NT];
        voc_bias<NT>(acc, a.b, n0, col);
        const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
        for (int j = 0; j < a.taps; ++j)                    // tap p + j hop of frame q - j
            voc_gemm<NT>(acc, wg_lds + (mg * VOC_ROWS + back - j + col) * cs + 4 * g, cs, a.w + (size_t)(p + j * a.hop) * tap_stride + wl, nkb, a.mel_p);
        const int lp = p / a.G, gp = p - lp * a.G;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = q0 + mg * VOC_ROWS + mt * 16 + g * 4 + i;
                if (q < len) {
                    float* row = sb + ((size_t)q * cpf + lp) * a.S_p + gp;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const int m = n0 + nt * 16 + col;
                        if (m < a.mel_dim) row[m * a.G] = acc[mt][nt][i];
                    }
                }
            }
    }
    const int npad = a.S_p - a.S;                           // the padding channels of the tile's columns: exact zeros
    if (npad) {
        const int l0 = q0 * cpf, l1 = min(q0 + a.tile, len) * cpf;
        for (int e = threadIdx.x; e < (l1 - l0) * npad; e += VOC_THREADS) {
            const int i = e / npad;
            sb[(size_t)(l0 + i) * a.S_p + a.S + (e - i * npad)] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the WN layer
struct WgLayerArgs {
    const float *hid_in, *spect;
    float *hid_out, *out;
    const int32_t* frames;
    const float *w_in, *w_cond, *b_ac, *w_rs, *b_rs;
    int T, cpf, C_p, S_p, dil, tile, kc, first, last;
};

// (two waves per SIMD: at NT = 8 the 128 accumulators and the fragments fit 256 registers without a spill, and a second workgroup on the
// CU multiplies while this one stages)
template <int NT>
__global__ __launch_bounds__(VOC_THREADS, 2) void gt_wg_layer_kernel(WgLayerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, 1) * a.cpf, t0 = blockIdx.x * a.tile;
    if (t0 >= len) return;
    const int xcs = a.kc + 4, gcs = a.C_p + 4, n2 = 2 * a.C_p;
    float* xs = wg_lds;                                     // [tile][xcs]: the K chunk in flight
    float* gs = wg_lds + (size_t)a.tile * xcs;              // [tile][gcs]: the gated tile
    const size_t rowbase = (size_t)b * a.T * a.cpf;
    const float* hb = a.hid_in + rowbase * a.C_p;
    const float* sb = a.spect + rowbase * a.S_p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    {
        const int ngroups = (n2 >> 4) / NT, items = (a.tile / VOC_ROWS) * ngroups, passes = (items + VOC_WAVES - 1) / VOC_WAVES;
        for (int pass = 0; pass < passes; ++pass) {
            const int item = pass * VOC_WAVES + wave;
            const bool active = item < items;
            const int mg = active ? item / ngroups : 0, n0 = active ? (item - mg * ngroups) * NT * 16 : 0;
            f32x4 acc[4][NT];
            voc_bias<NT>(acc, a.b_ac, n0, col);
            const size_t wl = (size_t)(n0 + col) * 16 + 4 * g;
            for (int src = 0; src < 4; ++src) {             // the taps at t - d, t, t + d of hid, then spect
                const float* xb = src < 3 ? hb : sb;
                const int ld = src < 3 ? a.C_p : a.S_p, K = ld, shift = src < 3 ? (src - 1) * a.dil : 0;
                const float* ws = src < 3 ? a.w_in + (size_t)src * a.C_p * n2 : a.w_cond;
                for (int k0 = 0; k0 < K; k0 += a.kc) {
                    const int w = min(a.kc, K - k0);
                    __syncthreads();                        // the chunk before this one has been consumed
                    wg_stage(xb, xs, xcs, ld, k0, w, t0 + shift, a.tile, len);
                    __syncthreads();
                    if (active) voc_gemm<NT>(acc, xs + (mg * VOC_ROWS + col) * xcs + 4 * g, xcs, ws + (size_t)(k0 >> 4) * n2 * 16 + wl, w >> 4, n2);
                }
            }
            if (active) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int u = 0; u < NT / 2; ++u) {  // N-tile 2 u: tanh half, 2 u + 1: sigmoid half of the same 16 channels
                            const float sg = 1.0f / (1.0f + expf(-acc[mt][2 * u + 1][i]));
                            gs[(mg * VOC_ROWS + mt * 16 + g * 4 + i) * gcs + (n0 >> 1) + u * 16 + col] = gt_tanh(acc[mt][2 * u][i]) * sg;
                        }
            }
        }
    }
    __syncthreads();
    {
        constexpr int NB = NT / 2;
        const int nB = a.last ? a.C_p : n2, ngroups = (nB >> 4) / NB, items = (a.tile / VOC_ROWS) * ngroups;
        float* ho = a.hid_out + rowbase * a.C_p;
        float* ob = a.out + rowbase * a.C_p;
        for (int item = wave; item < items; item += VOC_WAVES) {
            const int mg = item / ngroups, n0 = (item - mg * ngroups) * NB * 16;
            f32x4 acc[4][NB];
            voc_bias<NB>(acc, a.b_rs, n0, col);
            voc_gemm<NB>(acc, gs + (mg * VOC_ROWS + col) * gcs + 4 * g, gcs, a.w_rs + (size_t)(n0 + col) * 16 + 4 * g, a.C_p >> 4, nB);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = t0 + mg * VOC_ROWS + mt * 16 + g * 4 + i;
                    if (t < len) {
#pragma unroll
                        for (int nt = 0; nt < NB; ++nt) {
                            const int n = n0 + nt * 16 + col;
                            const float v = acc[mt][nt][i];
                            if (!a.last && n < a.C_p) {
                                ho[(size_t)t * a.C_p + n] = hb[(size_t)t * a.C_p + n] + v;
                            } else {
                                float* o = ob + (size_t)t * a.C_p + (a.last ? n : n - a.C_p);
                                *o = a.first ? v : *o + v;
                            }
                        }
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the flow's tail
struct WgFlowArgs {
    const float* out;           // [B, L, C_p]: the WN's skip sum (ck > 0)
    float* audio;               // [B, L, WG_AW]
    float* hid;                 // [B, L, C_p]: the next flow's start (wav == NULL)
    const float* z;             // [B, ldz] or NULL = draw from seeds
    const uint64_t* seeds;
    const int32_t* frames;
    float* wav;                 // the last launch: [B, ld_wav]
    int32_t* wav_lengths;
    const float *w_end, *b_end, *winv, *w_start, *b_start;      // [C][16], [16], [16][16], [hnext][C_p], [C_p]
    int T, cpf, C, C_p, G, ck, inject, zcol, hnext, ld_wav, ldz;        // ck = 0: the first launch (audio = sigma z[:, 0:inject])
    float sigma;
};

__device__ __forceinline__ float wg_z(const WgFlowArgs& a, int b, int l, int gcol) {
    if (a.z) return a.z[(size_t)b * a.ldz + (size_t)l * a.G + gcol];
    const Philox4 r = gt_philox(a.seeds[b], (uint32_t)l, (uint32_t)gcol, 0u, GT_RNG_WAVEGLOW);
    return gt_normal(r.x, r.y);
}

__global__ __launch_bounds__(VOC_THREADS) void gt_wg_flow_kernel(WgFlowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    const int b = blockIdx.y, len = voc_row_frames(a.frames, b, a.T, 1) * a.cpf, l0 = blockIdx.x * GT_WG_FLOW_TILE;
    if (a.wav) {
        float* wb = a.wav + (size_t)b * a.ld_wav;
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.wav_lengths) a.wav_lengths[b] = len * a.G;
        const int n0 = max(l0, len) * a.G, n1 = min((l0 + GT_WG_FLOW_TILE) * a.G, a.ld_wav);        // zeros beyond the row
        for (int n = n0 + (int)threadIdx.x; n < n1; n += VOC_THREADS) wb[n] = 0.f;
    }
    if (l0 >= len) return;
    const int xcs = a.C_p + 1, h = a.ck >> 1;
    float* os = wg_lds;                                     // [tile][WG_OS]: end's outputs b | s
    float* ar = os + GT_WG_FLOW_TILE * WG_OS;               // [tile][WG_OS]: the column's audio
    float* nr = ar + GT_WG_FLOW_TILE * WG_OS;               // [tile][WG_OS]: the column's audio behind the flow
    float* xs = nr + GT_WG_FLOW_TILE * WG_OS;               // [tile][xcs]: the out tile
    float* we = xs + GT_WG_FLOW_TILE * xcs;                 // [C][16]
    const size_t rowbase = (size_t)b * a.T * a.cpf;
    if (a.ck) {
        const float* ob = a.out + rowbase * a.C_p;
        for (int e = threadIdx.x; e < GT_WG_FLOW_TILE * a.C_p; e += VOC_THREADS) {
            const int i = e / a.C_p, c = e - i * a.C_p, l = l0 + i;
            xs[i * xcs + c] = l < len ? ob[(size_t)l * a.C_p + c] : 0.f;
        }
        for (int e = threadIdx.x; e < a.C * 16; e += VOC_THREADS) we[e] = a.w_end[e];
        __syncthreads();
        const int colr = threadIdx.x & (GT_WG_FLOW_TILE - 1);
        for (int j = threadIdx.x / GT_WG_FLOW_TILE; j < a.ck; j += VOC_THREADS / GT_WG_FLOW_TILE) {
            float acc = a.b_end[j];
            const float* xr = xs + colr * xcs;
            for (int c = 0; c < a.C; ++c) acc = __builtin_fmaf(xr[c], we[c * 16 + j], acc);
            os[colr * WG_OS + j] = acc;
        }
        __syncthreads();
    }
    const int cnext = a.ck + a.inject;
    if (threadIdx.x < GT_WG_FLOW_TILE && l0 + (int)threadIdx.x < len) {
        const int l = l0 + threadIdx.x;
        float* ap = a.audio + (rowbase + l) * WG_AW;
        float* mo = os + threadIdx.x * WG_OS;
        float* ma = ar + threadIdx.x * WG_OS;
        float* mn = nr + threadIdx.x * WG_OS;
        if (a.ck) {
            for (int i = 0; i < a.ck; ++i) ma[i] = ap[i];
            for (int j = 0; j < h; ++j) ma[h + j] = (ma[h + j] - mo[j]) * expf(-mo[h + j]);
            for (int i = 0; i < a.ck; ++i) {
                float v = 0.f;
                for (int j = 0; j < a.ck; ++j) v = __builtin_fmaf(ma[j], a.winv[i * 16 + j], v);
                mn[a.inject + i] = v;
            }
        }
        for (int i = 0; i < a.inject; ++i) mn[i] = a.sigma * wg_z(a, b, l, a.zcol + i);
        if (a.wav) {
            float* wb = a.wav + (size_t)b * a.ld_wav + (size_t)l * a.G;
            for (int i = 0; i < a.G; ++i) wb[i] = mn[i];
        } else {
            for (int i = 0; i < WG_AW; ++i) ap[i] = i < cnext ? mn[i] : 0.f;
        }
    }
    if (a.wav) return;
    __syncthreads();
    float* hb = a.hid + rowbase * a.C_p;
    for (int e = threadIdx.x; e < GT_WG_FLOW_TILE * a.C_p; e += VOC_THREADS) {        // the next flow's start
        const int i = e / a.C_p, n = e - i * a.C_p, l = l0 + i;
        if (l < len) {
            float v = a.b_start[n];
            for (int q = 0; q < a.hnext; ++q) v = __builtin_fmaf(nr[i * WG_OS + q], a.w_start[q * a.C_p + n], v);
            hb[(size_t)l * a.C_p + n] = v;
        }
    }
}

__global__ __launch_bounds__(VOC_THREADS) void gt_wg_noise_kernel(const uint64_t* seeds, float* z, int n, int G) {
    const int b = blockIdx.y, i = blockIdx.x * VOC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int l = i / G;
    const Philox4 r = gt_philox(seeds[b], (uint32_t)l, (uint32_t)(i - l * G), 0u, GT_RNG_WAVEGLOW);
    z[(size_t)b * n + i] = gt_normal(r.x, r.y);
}

size_t wg_flow_lds(int C, int C_p) {
    return ((size_t)GT_WG_FLOW_TILE * (3 * WG_OS + C_p + 1) + (size_t)C * 16) * sizeof(float);
}

template <int NT>
void wg_launch_layer(const WgLayerArgs& a, dim3 grid, size_t lds, hipStream_t stream) {
    gt_wg_layer_kernel<NT><<<grid, VOC_THREADS, lds, stream>>>(a);
}

}  // namespace

int gt_waveglow_flow_channels(int G, int EE, int ES, int k) {
    int n = 0;
    for (int j = 1; j <= k; ++j) n += (j % EE == 0);
    return G - ES * n;
}

const char* gt_waveglow_make_plan(int mel_dim, int hop, int win, int G, int F, int EE, int ES, int NL, int C, WgPlan* plan) {
    if (mel_dim < 1) return "mel_dim must be at least 1";
    if (hop < 1) return "hop must be at least 1";
    if (win < 1) return "win must be at least 1";
    if (G < 1) return "n_group must be at least 1";
    if (F < 1) return "n_flows must be at least 1";
    if (EE < 1) return "n_early_every must be at least 1";
    if (ES < 1) return "n_early_size must be at least 1";
    if (NL < 1) return "n_layers must be at least 1";
    if (C < 1) return "n_channels must be at least 1";
    if (NL > GT_WG_MAX_LAYERS) return "n_layers: at most 10 (the widest dilation is 2^(n_layers-1))";
    if (F > GT_WG_MAX_FLOWS) return "n_flows: at most 32";
    if (G > GT_WG_MAX_GROUP) return "n_group: at most 16";
    if (win % hop) return "win must be a multiple of hop";
    if (hop % G) return "hop must be a multiple of n_group";
    if (G % 2) return "n_group must be even";
    if (ES % 2) return "n_early_size must be even";
    if (hop > 65536 || win > 1048576 || mel_dim > 4096 || C > 16384) return "mel_dim, hop, win or n_channels is beyond what the kernels index";
    WgPlan& P = *plan;
    P = WgPlan{};
    P.mel_dim = mel_dim; P.hop = hop; P.win = win; P.G = G; P.F = F; P.EE = EE; P.ES = ES; P.NL = NL; P.C = C;
    P.mel_p = voc_pad16(mel_dim); P.C_p = voc_pad16(C); P.S = mel_dim * G; P.S_p = voc_pad16(P.S);
    for (int k = 0; k < F; ++k) {
        P.ck[k] = gt_waveglow_flow_channels(G, EE, ES, k);
        if (P.ck[k] < 2) return "n_early_size: fewer than 2 channels remain (n_rem < 2)";
        if (P.ck[k] % 2) return "n_early_size: a flow's channel count is odd";
    }
    P.n_rem = P.ck[F - 1];
    static const char* lds_msg = "n_channels: a tile does not fit the 160 KB of LDS";
    {   // the upsampler: the shared item form by channel count
        voc_tile_form(P.mel_p, &P.up_tile, &P.up_form);
        auto lds = [&]() { return (size_t)(P.up_tile + win / hop - 1) * (P.mel_p + 4) * sizeof(float); };
        while ((P.up_lds = lds()) > GT_VOC_LDS_MAX && P.up_tile > VOC_ROWS) P.up_tile >>= 1;
        if (P.up_lds > GT_VOC_LDS_MAX) return "win: the upsampler's tile does not fit the 160 KB of LDS";
    }
    {   // the WN layer: N-tiles a wave item owns in the gate GEMM (pairs of a tanh and a sigmoid tile), the time tile that gives four
        // waves an item each, and the widest K chunk with which two workgroups share a CU's LDS (else the widest that fits at all)
        const int pairs = P.C_p / 16;
        P.form = pairs % 4 == 0 ? 8 : (pairs % 2 == 0 ? 4 : 2);
        const int ngroups = 2 * pairs / P.form;
        P.tile = VOC_ROWS * (ngroups >= 4 ? 1 : (ngroups >= 2 ? 2 : 4));
        auto lds = [&](int kc) { return (size_t)P.tile * ((kc + 4) + (P.C_p + 4)) * sizeof(float); };
        P.kc = 0;
        for (int share = 2; share >= 1 && !P.kc; --share)
            for (int kc = 64; kc >= 16 && !P.kc; kc >>= 1)
                if (lds(kc) * share <= GT_VOC_LDS_MAX) P.kc = kc;
        if (!P.kc) return lds_msg;
        P.lds = lds(P.kc);
    }
    P.flow_lds = wg_flow_lds(C, P.C_p);
    if (P.flow_lds > GT_VOC_LDS_MAX) return lds_msg;
    P.ws_floats_per_column = (size_t)P.S_p + 3 * (size_t)P.C_p + WG_AW;
    return nullptr;
}

void gt_waveglow_pack_gate(const float* w, int taps, int cin, int C, float* out) {
    const int C_p = voc_pad16(C), n2 = 2 * C_p;
    std::vector<float> perm((size_t)taps * cin * n2, 0.f);
    for (int r = 0; r < taps * cin; ++r)
        for (int half = 0; half < 2; ++half)
            for (int ch = 0; ch < C; ++ch)
                perm[(size_t)r * n2 + ((ch >> 4) * 2 + half) * 16 + (ch & 15)] = w[(size_t)r * 2 * C + half * C + ch];
    voc_pack_f32(perm.data(), taps, cin, n2, out);
}

void gt_waveglow_gate_bias(const float* b_in, const float* b_cond, int C, float* out) {
    const int C_p = voc_pad16(C);
    std::fill(out, out + 2 * C_p, 0.f);
    for (int half = 0; half < 2; ++half)
        for (int ch = 0; ch < C; ++ch) out[((ch >> 4) * 2 + half) * 16 + (ch & 15)] = b_in[half * C + ch] + b_cond[half * C + ch];
}

void gt_waveglow_pack_rs(const float* w, const float* bias, int C, bool last, float* out, float* bias_out) {
    const int C_p = voc_pad16(C), halves = last ? 1 : 2, nB = halves * C_p;
    std::vector<float> perm((size_t)C * nB, 0.f);
    std::fill(bias_out, bias_out + nB, 0.f);
    for (int half = 0; half < halves; ++half)
        for (int ch = 0; ch < C; ++ch) {
            for (int r = 0; r < C; ++r) perm[(size_t)r * nB + half * C_p + ch] = w[(size_t)r * halves * C + half * C + ch];
            bias_out[half * C_p + ch] = bias[half * C + ch];
        }
    voc_pack_f32(perm.data(), 1, C, nB, out);
}

hipError_t gt_waveglow_prepare() {
    hipError_t e = voc_allow_lds(hipSuccess, gt_wg_flow_kernel);
    e = voc_allow_lds(e, gt_wg_up_kernel<1>); e = voc_allow_lds(e, gt_wg_up_kernel<2>); e = voc_allow_lds(e, gt_wg_up_kernel<4>);
    e = voc_allow_lds(e, gt_wg_layer_kernel<2>); e = voc_allow_lds(e, gt_wg_layer_kernel<4>); e = voc_allow_lds(e, gt_wg_layer_kernel<8>);
    return e;
}

hipError_t gt_launch_waveglow_noise(const uint64_t* seeds, float* z, int B, int n, int G, hipStream_t stream) {
    gt_wg_noise_kernel<<<dim3((n + VOC_THREADS - 1) / VOC_THREADS, B), VOC_THREADS, 0, stream>>>(seeds, z, n, G);
    return hipGetLastError();
}

hipError_t gt_launch_waveglow(const WgPlan& P, const WgCall& c, hipStream_t stream) {
    const int cpf = P.hop / P.G;
    const int64_t Lmax = (int64_t)c.T * cpf;
    int launch = 0;
    auto wanted = [&]() { const int i = launch++; return c.only < 0 || c.only == i; };
    if (wanted()) {
        WgUpArgs a{};
        a.mel = c.mel; a.spect = c.spect; a.frames = c.frames; a.w = P.w_up; a.b = P.b_up;
        a.T = c.T; a.mel_dim = P.mel_dim; a.mel_p = P.mel_p; a.hop = P.hop; a.taps = P.win / P.hop; a.G = P.G; a.S = P.S; a.S_p = P.S_p;
        a.tile = P.up_tile;
        const dim3 grid((c.T + P.up_tile - 1) / P.up_tile, c.B);
        if (P.up_form == 4) gt_wg_up_kernel<4><<<grid, VOC_THREADS, P.up_lds, stream>>>(a);
        else if (P.up_form == 2) gt_wg_up_kernel<2><<<grid, VOC_THREADS, P.up_lds, stream>>>(a);
        else gt_wg_up_kernel<1><<<grid, VOC_THREADS, P.up_lds, stream>>>(a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    int zcol = 0;
    auto flow = [&](int k) {                                // k = F: the first launch; else the tail of flow k
        WgFlowArgs a{};
        a.out = c.out; a.audio = c.audio; a.hid = c.hid[0]; a.z = c.z; a.seeds = c.seeds; a.frames = c.frames;
        a.T = c.T; a.cpf = cpf; a.C = P.C; a.C_p = P.C_p; a.G = P.G; a.ld_wav = c.ld_wav; a.ldz = c.T * P.hop; a.sigma = c.sigma;
        if (k == P.F) {
            a.ck = 0; a.inject = P.n_rem;
        } else {
            a.ck = P.ck[k]; a.inject = k > 0 ? P.ck[k - 1] - P.ck[k] : 0;
            a.w_end = P.flow[k].w_end; a.b_end = P.flow[k].b_end; a.winv = P.flow[k].winv;
        }
        a.zcol = zcol;
        zcol += a.inject;
        dim3 grid((unsigned)((Lmax + GT_WG_FLOW_TILE - 1) / GT_WG_FLOW_TILE), c.B);
        if (k > 0) {
            a.hnext = P.ck[k - 1] / 2; a.w_start = P.flow[k - 1].w_start; a.b_start = P.flow[k - 1].b_start;
        } else {
            a.wav = c.wav; a.wav_lengths = c.wav_lengths;
            grid.x = (unsigned)(((int64_t)(c.ld_wav + P.G - 1) / P.G + GT_WG_FLOW_TILE - 1) / GT_WG_FLOW_TILE);
        }
        if (!wanted()) return hipSuccess;
        gt_wg_flow_kernel<<<grid, VOC_THREADS, P.flow_lds, stream>>>(a);
        return hipGetLastError();
    };
    hipError_t e = flow(P.F);
    if (e != hipSuccess) return e;
    for (int k = P.F - 1; k >= 0; --k) {
        for (int i = 0; i < P.NL; ++i) {
            if (!wanted()) continue;
            const WgLayerOps& o = P.layer[k][i];
            WgLayerArgs a{};
            a.hid_in = c.hid[i & 1]; a.hid_out = c.hid[(i + 1) & 1]; a.spect = c.spect; a.out = c.out; a.frames = c.frames;
            a.w_in = o.w_in; a.w_cond = o.w_cond; a.b_ac = o.b_ac; a.w_rs = o.w_rs; a.b_rs = o.b_rs;
            a.T = c.T; a.cpf = cpf; a.C_p = P.C_p; a.S_p = P.S_p; a.dil = 1 << i; a.tile = P.tile; a.kc = P.kc;
            a.first = i == 0; a.last = i == P.NL - 1;
            const dim3 grid((unsigned)((Lmax + P.tile - 1) / P.tile), c.B);
            if (P.form == 8) wg_launch_layer<8>(a, grid, P.lds, stream);
            else if (P.form == 4) wg_launch_layer<4>(a, grid, P.lds, stream);
            else wg_launch_layer<2>(a, grid, P.lds, stream);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        if ((e = flow(k)) != hipSuccess) return e;
    }
    return hipSuccess;
}
